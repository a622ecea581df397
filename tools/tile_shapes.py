"""CPU count (oracle): distinct nodes an 8x8 / 16x4 / 4x16 / 32x2 / 64x1 tile of 64 shadow rays visits (the union a packet walks):
    python tools/tile_shapes.py city_4k courtyard_4k atrium_1080p"""
import ctypes as C, sys, os, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from raytracedshadows_amd import workloads
import oracle
_o = oracle._o
_o.orc_tile_union_stats_wh.restype = None
_o.orc_tile_union_stats_wh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
for cfg in sys.argv[1:]:
    wl = workloads.prepare_config(cfg, cache=True)
    lt = oracle.light_from_product(wl.light, wl.constants)
    k = np.ascontiguousarray(wl.constants.as_array(), np.float32)
    packed = np.ascontiguousarray(wl.packed, np.uint32); pos = np.ascontiguousarray(wl.positions, np.float32)
    for tw, th in ((8, 8), (16, 4), (4, 16), (32, 2), (64, 1)):
        u = np.zeros(8, np.uint64); t0 = time.time()
        _o.orc_tile_union_stats_wh(oracle._p(packed), oracle._p(k), C.byref(lt), oracle._p(pos), wl.W, wl.H, tw, th, oracle._p(u))
        tiles = int(u[0])
        print(f"{cfg} tile {tw}x{th}: {int(u[1]) / tiles:.1f} distinct nodes per tile ({int(u[4]) / tiles:.1f} leaves), longest ray {int(u[2]) / tiles:.1f}, visits per ray {int(u[3]) / tiles / 64:.1f}  ({time.time() - t0:.0f}s)", flush=True)
