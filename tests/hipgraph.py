"""Stream capture and graph replay through the HIP runtime the product library has loaded (ctypes, no build step).

Only what tests/test_gpu_graph.py needs: capture a stream in thread-local mode, list the node types of the captured graph,
instantiate, launch, destroy.  Between begin() and end() the capturing thread must make no call that allocates, copies
synchronously or synchronises: the runtime refuses those in thread-local mode and invalidates the capture."""
import ctypes as C

from raytracedshadows_amd import api  # noqa: F401  (loads librts.so, and with it the runtime)

KERNEL, MEMCPY, MEMSET, HOST, GRAPH, EMPTY, WAIT_EVENT, EVENT_RECORD, SEM_SIGNAL, SEM_WAIT, MEM_ALLOC, MEM_FREE = range(12)
THREAD_LOCAL = 1                                     # hipStreamCaptureModeThreadLocal
CAPTURE_NONE, CAPTURE_ACTIVE, CAPTURE_INVALIDATED = 0, 1, 2


class HipError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        super().__init__(f"{where}: hipError {status} ({_hip.hipGetErrorString(status).decode()})")


def _loaded_runtime():
    """The libamdhip64 this process has mapped (the one librts.so is linked against), not whichever a search path finds."""
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.split(None, 5)[-1].strip()
                if "libamdhip64.so" in path and path.startswith("/"):
                    return path
    except OSError:
        pass
    return "libamdhip64.so"


_hip = C.CDLL(_loaded_runtime())
_hip.hipGetErrorString.restype = C.c_char_p
_hip.hipGetErrorString.argtypes = [C.c_int]
for _name, _args in (
        ("hipStreamBeginCapture", [C.c_void_p, C.c_int]),
        ("hipStreamEndCapture", [C.c_void_p, C.POINTER(C.c_void_p)]),
        ("hipStreamIsCapturing", [C.c_void_p, C.POINTER(C.c_int)]),
        ("hipGraphGetNodes", [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
        ("hipGraphNodeGetType", [C.c_void_p, C.POINTER(C.c_int)]),
        ("hipGraphInstantiate", [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]),
        ("hipGraphLaunch", [C.c_void_p, C.c_void_p]),
        ("hipGraphExecDestroy", [C.c_void_p]),
        ("hipGraphDestroy", [C.c_void_p])):
    getattr(_hip, _name).restype = C.c_int
    getattr(_hip, _name).argtypes = _args


def _check(status, where):
    if status != 0:
        raise HipError(status, where)


def capture_status(stream):
    st = C.c_int(-1)
    _check(_hip.hipStreamIsCapturing(C.c_void_p(stream), C.byref(st)), "hipStreamIsCapturing")
    return st.value


class Graph:
    """One captured graph and its executable."""

    def __init__(self, graph):
        self._graph, self._exec = C.c_void_p(graph), C.c_void_p()

    def node_types(self):
        n = C.c_size_t(0)
        _check(_hip.hipGraphGetNodes(self._graph, None, C.byref(n)), "hipGraphGetNodes")
        if n.value == 0:
            return []
        nodes = (C.c_void_p * n.value)()
        _check(_hip.hipGraphGetNodes(self._graph, nodes, C.byref(n)), "hipGraphGetNodes")
        types = []
        for node in nodes[:n.value]:
            t = C.c_int(-1)
            _check(_hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(t)), "hipGraphNodeGetType")
            types.append(t.value)
        return types

    def launch(self, stream):
        if not self._exec:
            _check(_hip.hipGraphInstantiate(C.byref(self._exec), self._graph, None, None, 0), "hipGraphInstantiate")
        _check(_hip.hipGraphLaunch(self._exec, C.c_void_p(stream)), "hipGraphLaunch")

    def close(self):
        if self._exec:
            _hip.hipGraphExecDestroy(self._exec)
            self._exec = C.c_void_p()
        if self._graph:
            _hip.hipGraphDestroy(self._graph)
            self._graph = C.c_void_p()


def capture(stream, record):
    """Runs record() between hipStreamBeginCapture(stream, thread-local) and hipStreamEndCapture; returns the Graph.  The capture
    is always ended, also when record() raises, so that no stream is left capturing; then the exception goes on."""
    assert stream, "the default stream cannot be captured"
    _check(_hip.hipStreamBeginCapture(C.c_void_p(stream), THREAD_LOCAL), "hipStreamBeginCapture")
    g = C.c_void_p()
    try:
        record()
        assert capture_status(stream) == CAPTURE_ACTIVE, "a call ended or invalidated the capture"
    except BaseException:
        _hip.hipStreamEndCapture(C.c_void_p(stream), C.byref(g))
        if g:
            _hip.hipGraphDestroy(g)
        raise
    _check(_hip.hipStreamEndCapture(C.c_void_p(stream), C.byref(g)), "hipStreamEndCapture")
    assert g.value, "hipStreamEndCapture returned no graph"
    return Graph(g.value)
