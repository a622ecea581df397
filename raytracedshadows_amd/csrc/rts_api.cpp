// C ABI of librts.so (declared in include/rts.h): thin, exception-free glue between plain
// pointers and (a) the host BVH producer, (b) the HIP traversal kernels.
#include "../../include/rts.h"
#include "bvh_builder.h"
#include "bvh_refit.h"
#include "rts_device.h"
#include "rts_soft_distance.h"
#include "rts_ao.h"
#include "rts_ao_adaptive.h"
#include "rts_ao_bent.h"
#include "rts_ao_distance.h"
#include "rts_light_list.h"
#include "rts_adaptive.h"
#include "rts_soft_light_list.h"
#include "rts_soft_light_list_adaptive.h"
#include "rts_soft_light_list_distance.h"
#include "rts_light_list_sparse.h"
#include "rts_dispatch.h"
#include "rts_args.h"
#include "rts_refit.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

using rts::Dispatch;
using rts::TraceParams;

struct rts_ctx {
    int device = 0;
    void* d_bvh = nullptr;
    size_t bvhVec4 = 0;
    uint32_t P = 0;
    bool bvhFinite = false;
    bool bvhOrdered = false;
    int variant = rts::V_AUTO;
    int swizzle = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> marks;   // rts_timer_mark slots, created on first use
    // staging for the host-pointer entries
    void* d_in = nullptr; size_t inBytes = 0;
    void* d_out = nullptr; size_t outBytes = 0;
    void* d_act = nullptr; size_t actBytes = 0;      // ... and for the active map of rts_trace_shadow_mask_active
    uint64_t activeTraces = 0;                        // launches with an active map (get-only option "active_traces")
    void* d_dist = nullptr; size_t distBytes = 0;     // staging for the distances of the host-pointer distance traces
    uint64_t distanceTraces = 0;                      // launches of a distance kernel (get-only option "distance_traces")
    uint64_t softDistanceTraces = 0;                  // launches of a soft distance kernel (get-only option "soft_distance_traces")
    uint64_t lightListTraces = 0;                     // launches of a light list kernel (get-only option "light_list_traces")
    uint64_t adaptiveTraces = 0;                      // launches of an adaptive soft mask kernel (get-only option "adaptive_traces")
    uint64_t softListAdaptiveTraces = 0;              // launches of an adaptive soft light list kernel (get-only option "soft_list_adaptive_traces")
    uint64_t softListJitterTraces = 0;                // launches of a jittered adaptive soft light list kernel (get-only option "soft_list_jitter_traces")
    uint64_t softLightListTraces = 0;                 // launches of a soft light list kernel (get-only option "soft_light_list_traces")
    uint64_t softListDistanceTraces = 0;              // launches of a soft light list distance kernel (get-only option "soft_list_distance_traces")
    uint64_t aoTraces = 0;                            // launches of an ambient occlusion kernel (get-only option "ao_traces")
    uint64_t aoAdaptiveTraces = 0;                    // launches of an adaptive ambient occlusion kernel (get-only option "ao_adaptive_traces")
    uint64_t aoBentTraces = 0;                        // launches of a bent-normal ambient occlusion kernel (get-only option "ao_bent_traces")
    uint64_t aoDistanceTraces = 0;                    // launches of an AO distance kernel (get-only option "ao_distance_traces")
    uint64_t sparseListTraces = 0;                    // launches of a sparse light list kernel, hard or soft (get-only option "sparse_list_traces")
    const char* lastKernel = "";
    int packetBudget = 16;
    int packetShare = 4;
    int blockWaves = 1;
    int ldsPad = 0;              // experiment knob: dynamic LDS bytes per workgroup (throttles occupancy)
    uint32_t* d_tileOrder = nullptr; size_t tileOrderCount = 0;
    int useTileOrder = 1;                    // option "tile_order": 0 ignores an installed order
    uint32_t tileOrderSquare = 0, tileOrderBlock = 0;   // what rts_ctx_plan_tile_order planned with (0, 0: the caller's own order or none)
    bool tileOrderPlanned = false;           // installed by rts_ctx_plan_tile_order (the tuner may replace it), not by the caller
    bool tileOrderSoftOnly = false;          // planned on a dispatch of several samples: one-sample dispatches of the same size keep their everyday launch
    uint64_t* d_waveStats = nullptr; size_t waveStatsBytes = 0; size_t waveStatsUsed = 0;
    uint64_t launches = 0;
    int rowOrder = 0;                  // dispatch order of tile rows on 2-D grids: 0 top-down, 1 bottom-up, 2 middle-out
    void* d_scratch = nullptr; size_t scratchBytes = 0;    // working memory of the GPU builders, kept between builds
    // GPU-private copy for the wide packet kernel (rts_wide.hip): derived from d_bvh on the device, never visible outside
    void* d_wide = nullptr; size_t wideCap = 0;      // wide nodes (P * 128 B), triangle records (P * 64 B), parents (N * 4 B): one allocation
    void* d_tris = nullptr;
    void* d_parents = nullptr;
    uint32_t* d_word = nullptr;              // 4 bytes for the validation kernel's verdict
    uint32_t wideCount = 0, wideLevels = 0;
    // the root box of the installed stream and the fast set-up's bounds from it (TraceParams::sceneBounds, rts_alltable.h): 64 bytes,
    // allocated once, rewritten on the device after every install and refit that leaves a private copy
    uint32_t* d_sceneBounds = nullptr;
    uint64_t allTableTraces = 0;             // traces that ran the ALLTABLE instantiation (option "alltable_traces", read-only)
    bool bvhEnclosed = false;                // pre-order binary tree whose boxes enclose their children's (validateKernel)
    int wideCopy = 1;                        // option "wide_copy": build the private copy at upload
    int wideLane = 0;                        // option "wide_lane": dissolved wide packets walk the wide nodes lane per ray (LDS stacks: 28 waves per CU)
    int softSplit = 1;                       // option "soft_split": soft shadows with 4 waves per tile (samples side by side)
    uint32_t pixelBase = 0;                  // set around a host-pointer stripe (see rts_trace_shadow_mask)
    uint64_t* d_clockProbe = nullptr; size_t clockProbeRows = 0;    // option "clock_probe"
    // split table (rts_ctx_plan_splits): valid for ONE dispatch geometry (the key), used by every trace that matches it
    struct Splits {
        bool valid = false;
        Dispatch geom{}; uint32_t blocksX = 0, blocksY = 0;     // the dispatch it was planned for and its tiles (madeFor)
        uint32_t* d_skipMap = nullptr;       // one bit per tile of the dispatch
        uint32_t* d_pieces = nullptr;        // 8 dwords per piece
        uint32_t* d_frontMap = nullptr;      // one dword per record, XCD-major (TraceParams::frontMap)
        uint32_t frontStride = 0;
        uint32_t nPieces = 0, pieceRows = 0, nTiles = 0, nFront = 0;      // records (pieces + front tiles), split tiles, front tiles
        bool allTiles = false;
        rts_split_plan plan{};               // what the table was planned with (rts_ctx_get_split_plan)
        // {occluded lanes, pieces done} per split tile: one buffer per stream that traces with the table, so that frames in
        // flight on different streams never meet in it (frames on one stream follow each other)
        std::vector<std::pair<void*, uint64_t*>> state;
    } splits;
    int useSplits = 1;                       // option "tile_splits": 0 ignores an installed table
    int tuneForMotion = 0;                   // option "tune_for_motion": the tuner's tables must survive a camera path
    uint64_t* d_pieceClock = nullptr; size_t pieceClockCount = 0;    // option "piece_stats"
    struct Planning {                        // set by rts_ctx_plan_splits around its pieces-only launch
        const uint32_t* d_pieces; uint32_t nPieces, pieceRows; uint64_t* d_state; uint32_t* d_log; uint32_t logCap;
    };
    const Planning* planning = nullptr;
    uint32_t lastBlocksX = 0, lastBlocksY = 0; int lastVariant = 0; bool lastGrid2d = false;   // of the last mask dispatch
    // refit (rts_ctx_refit_bvh_device): what depends on the installed stream's topology alone is derived at its first refit
    // and kept until the next install (rts_ctx_set_bvh, the GPU builders' install) -- a refit per frame then allocates
    // nothing and reads back one status block
    struct Refit {
        bool valid = false;                  // topology verdict and schedule below belong to the installed stream
        int topology = RTS_OK;               // RTS_ERR_BAD_BVH: not a pre-order tree with the reference's miss links
        uint32_t treelet = 0;                // treelet size the schedule was made for
        uint32_t nRoots = 0, nTop = 0, nLevels = 0;
        void* d_sched = nullptr; size_t schedCap = 0;      // treelet roots, top nodes by height, level offsets
        void* d_geom = nullptr; size_t geomCap = 0;        // staging of host-pointer vertices / indices
        rts::RefitStatus* d_status = nullptr;
        bool haveBaseline = false;           // cost proxy of the stream as installed (taken before the first refit's writes)
        double baseline = 0;
        hipEvent_t ev[2] = { nullptr, nullptr };
    } refit;
    int refitTreelet = 1024;                 // option "refit_treelet": nodes per treelet workgroup (speed only)
    // follow mode (option "follow", rts_follow.hip): per stream, the lives of the last traced dispatch and the order the next one
    // runs in -- one dispatch geometry per stream; at most 8 streams, the least recently used evicted
    struct Follow {
        void* stream = nullptr;
        Dispatch geom{}; uint32_t blocksX = 0, blocksY = 0;     // the dispatch the lives belong to and its tiles (madeFor)
        void* d_mem = nullptr;               // one allocation: lives (2 u32 per tile), front map, all-ones skip map, planner scratch
        uint32_t* d_lives = nullptr; uint32_t* d_frontMap = nullptr; uint32_t* d_skipMap = nullptr; void* d_scratch = nullptr;
        uint32_t frontStride = 0;
        bool planned = false;                // the front map holds an order (the planner ran after a trace of this geometry)
        uint64_t lastUse = 0;
    };
    std::vector<Follow> follow;
    int followOn = 0;                        // option "follow"
    int followBlock = 8;                     // option "follow_block": life_block B of the rolling order
    int followSquare = 32;                   // option "follow_square": xcd_square S of the rolling order
    uint64_t followClock = 0, followTraces = 0, followOrdered = 0;
};

namespace {

inline int hipStatus(hipError_t e) { return e == hipSuccess ? RTS_OK : RTS_ERR_HIP + (int)e; }
}
namespace rts {   // rts_wide.hip
int deviceOf(const void* p);            // rts_lbvh.hip
hipError_t validateStreamDevice(const void* d_packed, uint32_t P, uint32_t* d_word, uint32_t* flagsOut);
size_t wideScratchBytes(uint32_t P);
hipError_t buildWideDevice(const void* d_packed, uint32_t P, void* d_wide, void* d_tris, void* d_parents, void* d_scratch,
                           uint32_t maxDepth, uint32_t* wideCount, uint32_t* levels);
}
extern "C" void* rts_ctx_scratch(rts_ctx* c, size_t bytes);
namespace {
#define RTS_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hipStatus(e_); } while (0)

int ensure(void** p, size_t* have, size_t want) {
    if (*have >= want && *p) return RTS_OK;
    if (*p) { hipError_t e = hipFree(*p); *p = nullptr; *have = 0; if (e != hipSuccess) return hipStatus(e); }
    hipError_t e = hipMalloc(p, want ? want : 16);
    if (e != hipSuccess) { *p = nullptr; return hipStatus(e); }
    *have = want;
    return RTS_OK;
}

void clearSplits(rts_ctx* c) {
    rts_ctx::Splits& t = c->splits;
    if (t.d_skipMap) (void)hipFree(t.d_skipMap);
    if (t.d_pieces) (void)hipFree(t.d_pieces);
    if (t.d_frontMap) (void)hipFree(t.d_frontMap);
    for (auto& e : t.state) if (e.second) (void)hipFree(e.second);
    t = rts_ctx::Splits();
}

void freeFollow(rts_ctx::Follow& f) { if (f.d_mem) (void)hipFree(f.d_mem); f = rts_ctx::Follow(); }

// follow mode: every stream's state (rts_ctx_set_bvh, a GPU build's install, option "follow" 0, rts_ctx_destroy)
void dropFollow(rts_ctx* c) {
    for (auto& f : c->follow) freeFollow(f);
    c->follow.clear();
}

// the {occluded, done} words of the split tiles for traces on `stream` (zeroed once; every launch leaves them zero).  Created
// outside graph capture only, as follow mode's state is (followFor): nothing is allocated or cleared in a captured trace, so a
// stream whose first trace with the table is being captured traces without the table
uint64_t* splitState(rts_ctx* c, void* stream) {
    rts_ctx::Splits& t = c->splits;
    for (auto& e : t.state) if (e.first == stream) return e.second;
    if (t.state.size() >= 8) return nullptr;                       // more streams than that trace without the table
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &capture) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (capture != hipStreamCaptureStatusNone) return nullptr;
    uint64_t* d = nullptr;
    if (hipMalloc((void**)&d, (size_t)t.nTiles * 16 + 16) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    // (cleared ON the stream that is about to use it: a memset on the default stream is not ordered before a launch on a
    //  non-blocking stream)
    if (hipMemsetAsync(d, 0, (size_t)t.nTiles * 16 + 16, (hipStream_t)stream) != hipSuccess) { (void)hipFree(d); return nullptr; }
    try { t.state.emplace_back(stream, d); } catch (...) { (void)hipFree(d); return nullptr; }
    return d;
}

int fillParams(rts_ctx* ctx, TraceParams& p) {
    memset(&p, 0, sizeof(p));
    if (!ctx->d_bvh) return RTS_ERR_NO_BVH;
    p.bvh = ctx->d_bvh;
    p.bvhBytes = (uint32_t)(ctx->bvhVec4 * 16);
    p.bvhFinite = ctx->bvhFinite ? 1u : 0u;
    p.bvhOrdered = (ctx->bvhFinite && ctx->bvhOrdered) ? 1u : 0u;
    p.packetBudget = (uint32_t)ctx->packetBudget;
    p.packetShare = (uint32_t)ctx->packetShare;
    p.wide = ctx->wideCount ? ctx->d_wide : nullptr;
    p.tris = ctx->wideCount ? ctx->d_tris : nullptr;
    p.primCount = ctx->P;
    p.parents = ctx->wideCount ? (const uint32_t*)ctx->d_parents : nullptr;
    p.wideBytes = (uint32_t)((size_t)ctx->P * 192u);
    p.trisOffset = (uint32_t)((size_t)ctx->P * 128u);
    p.wideLane = (uint32_t)ctx->wideLane;
    p.softSplit = (uint32_t)ctx->softSplit;
    p.pixelBase = ctx->pixelBase;
    return RTS_OK;
}

int deriveWideCopy(rts_ctx* c);

// The stream in c->d_bvh has just been installed (uploaded or adopted): what the kernels may assume about it is decided
// on the device (one kernel over all nodes), then the private copy of the wide kernel is derived from it.  A stream that
// breaks the layout rules is refused (RTS_ERR_BAD_BVH) and the context is left without a BVH.
int finishInstall(rts_ctx* c, bool freeOnRefusal) {
    uint32_t flags = 0xF;
    hipError_t e = rts::validateStreamDevice(c->d_bvh, c->P, c->d_word, &flags);
    if (e != hipSuccess || (flags & 1u)) {
        if (freeOnRefusal) (void)hipFree(c->d_bvh);
        c->d_bvh = nullptr; c->bvhVec4 = 0; c->P = 0; c->wideCount = 0;
        return e != hipSuccess ? hipStatus(e) : RTS_ERR_BAD_BVH;
    }
    c->bvhFinite = !(flags & 2u);
    c->bvhOrdered = !(flags & 4u);
    c->bvhEnclosed = !(flags & 8u);
    return deriveWideCopy(c);
}

// what the stream's flags allow: a private copy of kernel 8 (byte offsets inside it are 32-bit: 192 bytes per triangle)
bool wideAllowed(const rts_ctx* c) {
    return c->bvhFinite && c->bvhOrdered && c->bvhEnclosed && c->P >= 2 && c->P <= (1u << 24);
}

// The per-scene constants of the ALLTABLE launch, in the default stream behind whatever just wrote the stream's boxes (the kernels
// of an install or of a refit).  Without them (no memory, a failed launch) that launch is simply not selected.
void refreshSceneBounds(rts_ctx* c) {
    if (!c->d_sceneBounds && hipMalloc((void**)&c->d_sceneBounds, 64) != hipSuccess) { c->d_sceneBounds = nullptr; (void)hipGetLastError(); return; }
    if (rts::launchSceneBounds(c->d_bvh, c->d_sceneBounds, nullptr) != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(c->d_sceneBounds); c->d_sceneBounds = nullptr;
    }
}

// the private copy of kernel 8, derived in full from the installed stream (when the option and the flags allow one)
int deriveWideCopy(rts_ctx* c) {
    c->wideCount = 0; c->wideLevels = 0;
    if (!c->wideCopy || !wideAllowed(c)) return RTS_OK;
    int s = ensure(&c->d_wide, &c->wideCap, (size_t)c->P * 200 + 256);
    c->d_tris = s == RTS_OK ? (char*)c->d_wide + (size_t)c->P * 128 : nullptr;
    c->d_parents = s == RTS_OK ? (char*)c->d_wide + (size_t)c->P * 192 : nullptr;
    void* scratch = s == RTS_OK ? rts_ctx_scratch(c, rts::wideScratchBytes(c->P)) : nullptr;
    if (!scratch) return RTS_OK;                      // no memory for the copy: the stackless kernels need none
    // (trees deeper than 512 levels -- chains of single-triangle splits -- keep the stackless kernels)
    hipError_t e = rts::buildWideDevice(c->d_bvh, c->P, c->d_wide, c->d_tris, c->d_parents, scratch, 512, &c->wideCount, &c->wideLevels);
    // a failure here only costs the private copy: the stream itself is installed and valid, the stackless kernels need
    // nothing else.  (Returning the error would leave the caller of the adopt path freeing a stream the context still holds.)
    if (e != hipSuccess) { c->wideCount = 0; c->wideLevels = 0; (void)hipGetLastError(); }
    if (c->wideCount) refreshSceneBounds(c);
    return RTS_OK;
}

// a new stream is being installed: what the refit derived from the old one goes (its buffers stay for reuse)
void dropRefit(rts_ctx* c) {
    c->refit.valid = false;
    c->refit.haveBaseline = false;
}

// "The same dispatch", for a split table and for a stream's follow state alike: the geometry it was made for, cut into the same tiles.
template <class Kept> bool madeFor(const Kept& kept, const Dispatch& g, const TraceParams& p) {
    return kept.geom == g && kept.blocksX == p.blocksX && kept.blocksY == p.blocksY;
}

// A new stream is about to be installed (rts_ctx_set_bvh, the GPU builders' install): the old one is freed, and what was derived from
// it goes -- a split table holds its node indices, a rolling order and a planned tile order the lives of the tiles on the old scene.
int forgetInstalled(rts_ctx* c) {
    if (c->d_bvh) { void* old = c->d_bvh; c->d_bvh = nullptr; c->bvhVec4 = 0; c->P = 0; RTS_HIP(hipFree(old)); }
    dropRefit(c);
    clearSplits(c);
    dropFollow(c);
    if (c->tileOrderPlanned) (void)rts_ctx_set_tile_order(c, nullptr, 0);
    return RTS_OK;
}

// The refit schedule of the installed stream, from its tag and link words (read back once): the topology check of the host
// form, then the treelet roots -- nodes whose subtree [i, end(i)) has at most T nodes and whose parent's has more -- and the
// inner nodes above them, grouped by height (a treelet root has height 0).
int refitSchedule(rts_ctx* c, uint32_t T) {
    rts_ctx::Refit& R = c->refit;
    const uint32_t P = c->P, N = 2 * P - 1;
    std::vector<uint32_t> sched;
    uint32_t nRoots = 0, nTop = 0, nLevels = 0;
    try {
        std::vector<rts_vec4u> nodes((size_t)2 * N);
        RTS_HIP(hipMemcpy(nodes.data(), c->d_bvh, nodes.size() * 16, hipMemcpyDeviceToHost));
        std::vector<uint32_t> end;
        R.topology = rts::refitTopology(nodes.data(), P, &end);
        R.valid = true; R.treelet = T; R.nRoots = R.nTop = R.nLevels = 0;
        if (R.topology != RTS_OK) return RTS_OK;
        std::vector<uint32_t> parent(N, rts::kRefitEnd), height(N, 0);
        for (uint32_t i = 0; i < N; ++i)
            if (nodes[2 * (size_t)i].d == rts::kRefitEnd) { parent[i + 1] = i; parent[nodes[2 * (size_t)i + 3].d] = i; }
        std::vector<uint32_t> roots, top;
        for (uint32_t i = 0; i < N; ++i) {
            const uint32_t size = end[i] - i;
            if (size > T) top.push_back(i);
            else if (i == 0 || end[parent[i]] - parent[i] > T) roots.push_back(i);
        }
        for (size_t t = top.size(); t-- > 0;) {          // children before parents: reverse index order
            const uint32_t i = top[t], right = nodes[2 * (size_t)i + 3].d;
            height[i] = 1 + std::max(height[i + 1], height[right]);
            nLevels = std::max(nLevels, height[i]);
        }
        std::vector<uint32_t> levelOff(nLevels + 1, 0);
        for (uint32_t i : top) ++levelOff[height[i]];     // counts per height 1..H at [h], then exclusive offsets at [h - 1]
        for (uint32_t h = 1, run = 0; h <= nLevels; ++h) { const uint32_t n = levelOff[h]; levelOff[h - 1] = run; run += n; }
        if (nLevels) levelOff[nLevels] = (uint32_t)top.size();
        std::vector<uint32_t> byHeight(top.size());
        std::vector<uint32_t> fill(levelOff.begin(), levelOff.end());
        for (uint32_t i : top) byHeight[fill[height[i] - 1]++] = i;
        nRoots = (uint32_t)roots.size(); nTop = (uint32_t)top.size();
        sched.reserve(roots.size() + top.size() + levelOff.size());
        sched.insert(sched.end(), roots.begin(), roots.end());
        sched.insert(sched.end(), byHeight.begin(), byHeight.end());
        sched.insert(sched.end(), levelOff.begin(), levelOff.end());
    } catch (...) {
        R.valid = false;
        return RTS_ERR_CAPACITY;                          // no exception crosses the C ABI
    }
    R.valid = false;                                      // (until the schedule is on the device)
    int s = ensure(&R.d_sched, &R.schedCap, sched.size() * 4);
    if (s != RTS_OK) return s;
    RTS_HIP(hipMemcpy(R.d_sched, sched.data(), sched.size() * 4, hipMemcpyHostToDevice));
    if (!R.d_status) RTS_HIP(hipMalloc((void**)&R.d_status, sizeof(rts::RefitStatus)));
    for (hipEvent_t& e : R.ev) if (!e) RTS_HIP(hipEventCreate(&e));
    if (rts::refitLdsBytes(T) > 65536) RTS_HIP(rts::refitSetLds(T));
    R.nRoots = nRoots; R.nTop = nTop; R.nLevels = nLevels;
    R.valid = true;
    return RTS_OK;
}

} // namespace

extern "C" {

const char* rts_status_string(int s) {
    switch (s) {
    case RTS_OK: return "ok";
    case RTS_ERR_INVALID_ARG: return "invalid argument";
    case RTS_ERR_CAPACITY: return "output capacity too small";
    case RTS_ERR_NONFINITE: return "non-finite vertex";
    case RTS_ERR_NO_BVH: return "no BVH set on context";
    case RTS_ERR_BAD_BVH: return "packed BVH failed validation";
    case RTS_ERR_DEGENERATE: return "degenerate input: no SAH split position (coordinate extents overflow the cost) or a chain of equal boxes deeper than 262144 levels";
    default: break;
    }
    if (s >= RTS_ERR_HIP) return hipGetErrorString((hipError_t)(s - RTS_ERR_HIP));
    return "unknown";
}

size_t rts_bvh_packed_count(uint32_t P) { return P ? (size_t)5 * P - 2 : 0; }
size_t rts_bvh_node_count(uint32_t P) { return P ? (size_t)2 * P - 1 : 0; }

int rts_bvh_build_ex(const float* vertices, uint32_t stride, const uint32_t* indices, uint32_t P,
                     uint32_t sah_prim_limit, int threads, rts_vec4u* out, size_t cap, rts_bvh_node* out_nodes) {
    if (!vertices || !indices || !out || P == 0) return RTS_ERR_INVALID_ARG;
    if (cap < rts_bvh_packed_count(P)) return RTS_ERR_CAPACITY;
    try {
        rts::BVHBuilder b;
        b.sahPrimLimit = sah_prim_limit;
        b.threads = threads;
        if (!b.build(vertices, stride, indices, P)) return b.lastError ? b.lastError : RTS_ERR_INVALID_ARG;
        memcpy(out, b.m_packedNodes.data(), b.m_packedNodes.size() * sizeof(rts_vec4u));
        if (out_nodes) memcpy(out_nodes, b.m_nodes.data(), b.m_nodes.size() * sizeof(rts_bvh_node));
    } catch (...) {
        return RTS_ERR_INVALID_ARG;
    }
    return RTS_OK;
}

int rts_bvh_build(const float* vertices, uint32_t stride, const uint32_t* indices, uint32_t P,
                  rts_vec4u* out, size_t cap, rts_bvh_node* out_nodes) {
    return rts_bvh_build_ex(vertices, stride, indices, P, 1000000u, 0, out, cap, out_nodes);
}

int rts_bvh_validate(const rts_vec4u* packed, size_t count, uint32_t* prim_count_out) {
    if (!packed || count < 3 || (count + 2) % 5 != 0) return packed ? RTS_ERR_BAD_BVH : RTS_ERR_INVALID_ARG;
    const uint64_t P = (count + 2) / 5, N = 2 * P - 1;
    if (P > 0x33333333ull) return RTS_ERR_BAD_BVH;
    for (uint64_t i = 0; i < N; ++i) {
        const rts_vec4u& a = packed[2 * i];
        const rts_vec4u& b = packed[2 * i + 1];
        if (b.d != 0xFFFFFFFFu && !(b.d > i && b.d < N)) return RTS_ERR_BAD_BVH;      // strictly forward
        if (a.d == 0xFFFFFFFFu) { if (i + 1 >= N) return RTS_ERR_BAD_BVH; }            // inner: i+1 exists
        else if (a.d < 2 * N || a.d >= 2 * N + P) return RTS_ERR_BAD_BVH;               // leaf: tail pointer
    }
    if (prim_count_out) *prim_count_out = (uint32_t)P;
    return RTS_OK;
}

int rts_device_count(int* count) {
    if (!count) return RTS_ERR_INVALID_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = (e == hipSuccess) ? n : 0;
    return hipStatus(e);
}

int rts_ctx_create(int device, rts_ctx** out) {
    if (!out) return RTS_ERR_INVALID_ARG;
    *out = nullptr;
    RTS_HIP(hipSetDevice(device));
    rts_ctx* c = new (std::nothrow) rts_ctx();
    if (!c) return RTS_ERR_INVALID_ARG;
    c->device = device;
    hipError_t e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_word, 256);
    if (e != hipSuccess) { delete c; return hipStatus(e); }
    *out = c;
    return RTS_OK;
}

int rts_ctx_destroy(rts_ctx* c) {
    if (!c) return RTS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (c->d_bvh) (void)hipFree(c->d_bvh);
    if (c->d_in) (void)hipFree(c->d_in);
    if (c->d_out) (void)hipFree(c->d_out);
    if (c->d_act) (void)hipFree(c->d_act);
    if (c->d_dist) (void)hipFree(c->d_dist);
    if (c->d_waveStats) (void)hipFree(c->d_waveStats);
    if (c->d_tileOrder) (void)hipFree(c->d_tileOrder);
    if (c->d_scratch) (void)hipFree(c->d_scratch);
    if (c->d_wide) (void)hipFree(c->d_wide);
    if (c->d_sceneBounds) (void)hipFree(c->d_sceneBounds);
    if (c->d_word) (void)hipFree(c->d_word);
    if (c->d_clockProbe) (void)hipFree(c->d_clockProbe);
    if (c->d_pieceClock) (void)hipFree(c->d_pieceClock);
    if (c->refit.d_sched) (void)hipFree(c->refit.d_sched);
    if (c->refit.d_geom) (void)hipFree(c->refit.d_geom);
    if (c->refit.d_status) (void)hipFree(c->refit.d_status);
    for (hipEvent_t e : c->refit.ev) if (e) (void)hipEventDestroy(e);
    clearSplits(c);
    dropFollow(c);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->marks) if (e) (void)hipEventDestroy(e);
    delete c;
    return RTS_OK;
}

int rts_ctx_set_bvh(rts_ctx* c, const rts_vec4u* packed, size_t count) {
    if (!c || !packed) return RTS_ERR_INVALID_ARG;
    uint32_t P = 0;
    int s = rts_bvh_validate(packed, count, &P);
    if (s != RTS_OK) return s;
    if (count * 16 >= 0xFFFFFF00ull) return RTS_ERR_BAD_BVH;           // 32-bit byte offsets on the device (top 256 B = "nothing")
    RTS_HIP(hipSetDevice(c->device));
    // the context only changes once the new copy is complete; a failure leaves it without a BVH, never with a torn one
    s = forgetInstalled(c);
    if (s != RTS_OK) return s;
    void* d = nullptr;
    RTS_HIP(hipMalloc(&d, count * 16 + 64));          // + slack: the prefetching packet loop reads one node ahead
    hipError_t e = hipMemcpy(d, packed, count * 16, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return hipStatus(e); }
    c->d_bvh = d; c->bvhVec4 = count; c->P = P;
    return finishInstall(c, true);       // finite / ordered / enclosed are decided on the device; private wide copy
}

int rts_ctx_set_option(rts_ctx* c, const char* key, int value) {
    if (!c || !key) return RTS_ERR_INVALID_ARG;
    if (!strcmp(key, "kernel")) { if (value < rts::V_AUTO || value >= rts::V_COUNT) return RTS_ERR_INVALID_ARG; c->variant = value; return RTS_OK; }
    if (!strcmp(key, "xcd_swizzle")) { c->swizzle = value ? 1 : 0; return RTS_OK; }
    // (1..4096: the dissolve rule multiplies budget * share * live rays in 32 bits)
    if (!strcmp(key, "packet_budget")) { if (value < 1 || value > 4096) return RTS_ERR_INVALID_ARG; c->packetBudget = value; return RTS_OK; }
    if (!strcmp(key, "block_waves")) { if (value != 1 && value != 4) return RTS_ERR_INVALID_ARG; c->blockWaves = value; return RTS_OK; }
    if (!strcmp(key, "row_order")) { if (value < 0 || value > 2) return RTS_ERR_INVALID_ARG; c->rowOrder = value; return RTS_OK; }
    if (!strcmp(key, "lds_pad")) { if (value < 0 || value > 65536) return RTS_ERR_INVALID_ARG; c->ldsPad = value; return RTS_OK; }
    if (!strcmp(key, "packet_share")) { if (value < 0 || value > 16) return RTS_ERR_INVALID_ARG; c->packetShare = value; return RTS_OK; }
    if (!strcmp(key, "wide_copy")) { c->wideCopy = value ? 1 : 0; return RTS_OK; }      // takes effect at the next upload / build
    if (!strcmp(key, "refit_treelet")) {            // nodes per treelet workgroup of the device refit (LDS: 52 bytes per node)
        if (value < 32 || value > 2048) return RTS_ERR_INVALID_ARG;
        c->refitTreelet = value; return RTS_OK;
    }
    if (!strcmp(key, "builder_scratch")) {          // 0: release the working memory the GPU builders keep between builds
        if (value != 0) return RTS_ERR_INVALID_ARG;
        RTS_HIP(hipSetDevice(c->device));
        if (c->d_scratch) { void* old = c->d_scratch; c->d_scratch = nullptr; c->scratchBytes = 0; RTS_HIP(hipFree(old)); }
        return RTS_OK;
    }
    if (!strcmp(key, "wide_lane")) { c->wideLane = value ? 1 : 0; return RTS_OK; }
    if (!strcmp(key, "soft_split")) { c->softSplit = value ? 1 : 0; return RTS_OK; }
    if (!strcmp(key, "tile_splits")) { c->useSplits = value ? 1 : 0; return RTS_OK; }     // 0: traces ignore an installed split table
    if (!strcmp(key, "tile_order")) { c->useTileOrder = value ? 1 : 0; return RTS_OK; }            // 0: traces ignore an installed tile order
    if (!strcmp(key, "tune_for_motion")) { c->tuneForMotion = value ? 1 : 0; return RTS_OK; }   // rts_ctx_autotune: only tables that keep over a camera path
    if (!strcmp(key, "follow")) {                // follow mode: traces record tile lives and run the order planned from the last ones
        if (value != 0 && value != 1) return RTS_ERR_INVALID_ARG;
        RTS_HIP(hipSetDevice(c->device));
        if (!value) dropFollow(c);
        c->followOn = value; return RTS_OK;
    }
    if (!strcmp(key, "follow_block")) { if (value < 1 || value > 64) return RTS_ERR_INVALID_ARG; c->followBlock = value; return RTS_OK; }
    if (!strcmp(key, "follow_square")) { if (value < 0 || value > 65535) return RTS_ERR_INVALID_ARG; c->followSquare = value; return RTS_OK; }
    if (!strcmp(key, "piece_stats")) {          // diagnostics: value = pieces to stamp (0 = off), see rts_ctx_read_piece_stats
        RTS_HIP(hipSetDevice(c->device));
        if (c->d_pieceClock) { RTS_HIP(hipFree(c->d_pieceClock)); c->d_pieceClock = nullptr; c->pieceClockCount = 0; }
        if (value > 0) {
            RTS_HIP(hipMalloc((void**)&c->d_pieceClock, (size_t)value * 64));
            RTS_HIP(hipMemset(c->d_pieceClock, 0, (size_t)value * 64));
            c->pieceClockCount = (size_t)value;
        }
        return RTS_OK;
    }
    if (!strcmp(key, "clock_probe")) {          // value = tile rows to stamp (0 = off); packet kernels on 2-D grids
        RTS_HIP(hipSetDevice(c->device));
        if (c->d_clockProbe) { RTS_HIP(hipFree(c->d_clockProbe)); c->d_clockProbe = nullptr; c->clockProbeRows = 0; }
        if (value > 0) {
            RTS_HIP(hipMalloc((void**)&c->d_clockProbe, (size_t)value * 32));
            RTS_HIP(hipMemset(c->d_clockProbe, 0, (size_t)value * 32));
            c->clockProbeRows = (size_t)value;
        }
        return RTS_OK;
    }
    if (!strcmp(key, "wave_stats")) {            // diagnostics: value = number of waves to record (0 = off)
        RTS_HIP(hipSetDevice(c->device));
        if (c->d_waveStats) { RTS_HIP(hipFree(c->d_waveStats)); c->d_waveStats = nullptr; c->waveStatsBytes = 0; }
        if (value > 0) {
            c->waveStatsBytes = (size_t)value * 32;           // 4 u64 per wave, then 4 more per wave (realtime stamps)
            RTS_HIP(hipMalloc((void**)&c->d_waveStats, c->waveStatsBytes * 2));
            RTS_HIP(hipMemset(c->d_waveStats, 0, c->waveStatsBytes * 2));
        }
        return RTS_OK;
    }
    return RTS_ERR_INVALID_ARG;
}

int rts_ctx_get_option(rts_ctx* c, const char* key, int* value) {
    if (!c || !key || !value) return RTS_ERR_INVALID_ARG;
    if (!strcmp(key, "kernel")) { *value = c->variant; return RTS_OK; }
    if (!strcmp(key, "xcd_swizzle")) { *value = c->swizzle; return RTS_OK; }
    if (!strcmp(key, "packet_budget")) { *value = c->packetBudget; return RTS_OK; }
    if (!strcmp(key, "block_waves")) { *value = c->blockWaves; return RTS_OK; }
    if (!strcmp(key, "packet_share")) { *value = c->packetShare; return RTS_OK; }
    if (!strcmp(key, "kernel_count")) { *value = rts::V_COUNT; return RTS_OK; }
    if (!strcmp(key, "row_order")) { *value = c->rowOrder; return RTS_OK; }
    if (!strcmp(key, "bvh_finite")) { *value = c->bvhFinite ? 1 : 0; return RTS_OK; }
    if (!strcmp(key, "bvh_ordered")) { *value = c->bvhOrdered ? 1 : 0; return RTS_OK; }
    if (!strcmp(key, "bvh_enclosed")) { *value = c->bvhEnclosed ? 1 : 0; return RTS_OK; }
    if (!strcmp(key, "wide_copy")) { *value = c->wideCopy; return RTS_OK; }
    if (!strcmp(key, "refit_treelet")) { *value = c->refitTreelet; return RTS_OK; }
    if (!strcmp(key, "builder_scratch")) { *value = (int)(c->scratchBytes >> 20); return RTS_OK; }     // MiB held
    if (!strcmp(key, "wide_lane")) { *value = c->wideLane; return RTS_OK; }
    if (!strcmp(key, "soft_split")) { *value = c->softSplit; return RTS_OK; }
    if (!strcmp(key, "wide_nodes")) { *value = (int)c->wideCount; return RTS_OK; }
    if (!strcmp(key, "tile_splits")) { *value = c->useSplits; return RTS_OK; }
    if (!strcmp(key, "tune_for_motion")) { *value = c->tuneForMotion; return RTS_OK; }
    if (!strcmp(key, "follow")) { *value = c->followOn; return RTS_OK; }
    if (!strcmp(key, "follow_block")) { *value = c->followBlock; return RTS_OK; }
    if (!strcmp(key, "follow_square")) { *value = c->followSquare; return RTS_OK; }
    if (!strcmp(key, "follow_streams")) { *value = (int)c->follow.size(); return RTS_OK; }
    if (!strcmp(key, "alltable_traces")) { *value = (int)(c->allTableTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "follow_traces")) { *value = (int)(c->followTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "follow_ordered")) { *value = (int)(c->followOrdered & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "active_traces")) { *value = (int)(c->activeTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "distance_traces")) { *value = (int)(c->distanceTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "soft_distance_traces")) { *value = (int)(c->softDistanceTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "light_list_traces")) { *value = (int)(c->lightListTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "adaptive_traces")) { *value = (int)(c->adaptiveTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "soft_list_adaptive_traces")) { *value = (int)(c->softListAdaptiveTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "soft_list_jitter_traces")) { *value = (int)(c->softListJitterTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "soft_light_list_traces")) { *value = (int)(c->softLightListTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "ao_traces")) { *value = (int)(c->aoTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "ao_adaptive_traces")) { *value = (int)(c->aoAdaptiveTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "ao_bent_traces")) { *value = (int)(c->aoBentTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "ao_distance_traces")) { *value = (int)(c->aoDistanceTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "sparse_list_traces")) { *value = (int)(c->sparseListTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "soft_list_distance_traces")) { *value = (int)(c->softListDistanceTraces & 0x7FFFFFFF); return RTS_OK; }
    if (!strcmp(key, "tile_order")) { *value = c->useTileOrder; return RTS_OK; }
    if (!strcmp(key, "tile_order_tiles")) { *value = (int)c->tileOrderCount; return RTS_OK; }
    if (!strcmp(key, "tile_order_planned")) { *value = c->tileOrderPlanned ? 1 : 0; return RTS_OK; }
    if (!strcmp(key, "tile_order_square")) { *value = (int)c->tileOrderSquare; return RTS_OK; }
    if (!strcmp(key, "tile_order_block")) { *value = (int)c->tileOrderBlock; return RTS_OK; }
    if (!strcmp(key, "split_tiles")) { *value = c->splits.valid ? (int)c->splits.nTiles : 0; return RTS_OK; }
    if (!strcmp(key, "front_tiles")) { *value = c->splits.valid ? (int)c->splits.nFront : 0; return RTS_OK; }
    if (!strcmp(key, "split_pieces")) { *value = c->splits.valid ? (int)c->splits.nPieces : 0; return RTS_OK; }
    if (!strcmp(key, "wide_levels")) { *value = (int)c->wideLevels; return RTS_OK; }
    return RTS_ERR_INVALID_ARG;
}

// Diagnostics (RTS_TUNE_LOG set): why the planner refused.
static int planRefused(const char* why) {
    if (getenv("RTS_TUNE_LOG")) fprintf(stderr, "[rts plan] refused: %s\n", why);
    return RTS_ERR_INVALID_ARG;
}

// Test hook (tests/test_host_logic.py): rts::stripeRows (rts_dispatch.h), host only.
extern "C" int rtsh_stripe_rows(uint32_t H, uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint32_t* rows) {
    if (!rows || band_rows == 0 || n_stripes == 0 || stripe >= n_stripes) return RTS_ERR_INVALID_ARG;
    *rows = rts::stripeRows(H, band_rows, n_stripes, stripe);
    return RTS_OK;
}

static int lifeBand(float us);

// follow mode: the per-band lower bounds of the tick count, from the host's own lifeBand (which the device then never evaluates:
// it compares integers).  Bands grow with the tick count, so each bound is a binary search over the 32-bit counts.
static const rts::FollowBands& followBands() {
    static const rts::FollowBands table = [] {
        rts::FollowBands t{};
        for (uint32_t i = 0; i < rts::FOLLOW_BANDS; ++i) {
            const int b = rts::FOLLOW_BAND_LOW + (int)i;
            uint64_t lo = 0, hi = 0xFFFFFFFFull;                 // the smallest count whose band is b or more
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (lifeBand((float)(uint32_t)mid * 0.01f) >= b) hi = mid; else lo = mid + 1;
            }
            t.minTicks[i] = (uint32_t)lo;
        }
        return t;
    }();
    return table;
}

// follow mode: one allocation per stream for a dispatch of n tiles -- lives (2 u32 per tile), front map (8 columns of `stride`
// records), all-ones skip map, planner scratch, each from a 256-byte boundary (followFor; rtsh_follow_plan_device carves the same)
struct FollowLayout {
    uint32_t stride;
    size_t livesB, mapB, skipB, scratchB;
    explicit FollowLayout(uint32_t n) : stride((n + 7u) / 8u) {
        const auto al = [](size_t v) { return (v + 255u) & ~(size_t)255u; };
        livesB = al((size_t)n * 8); mapB = al((size_t)stride * 32); skipB = al(((size_t)n + 31) / 32 * 4 + 4);
        scratchB = rts::followScratchBytes(n);
    }
    size_t mapAt() const { return livesB; }
    size_t skipAt() const { return livesB + mapB; }
    size_t scratchAt() const { return livesB + mapB + skipB; }
    size_t bytes() const { return livesB + mapB + skipB + scratchB; }
};

// follow mode: the state of `stream` for this dispatch geometry.  A stream seen with another geometry starts over; a ninth stream
// evicts the least recently used.  Created and reset outside graph capture only (nothing is allocated in a captured trace):
// NULL = run the everyday launch.
static rts_ctx::Follow* followFor(rts_ctx* c, void* stream, const Dispatch& g, const TraceParams& p) {
    rts_ctx::Follow* f = nullptr;
    for (auto& e : c->follow) if (e.stream == stream) { f = &e; break; }
    if (f && f->d_mem && madeFor(*f, g, p)) {
        f->lastUse = ++c->followClock;
        return f;
    }
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &capture) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (capture != hipStreamCaptureStatusNone) return nullptr;
    if (f) freeFollow(*f);
    else {
        if (c->follow.size() >= 8) {
            size_t lru = 0;
            for (size_t i = 1; i < c->follow.size(); ++i) if (c->follow[i].lastUse < c->follow[lru].lastUse) lru = i;
            freeFollow(c->follow[lru]);
            c->follow.erase(c->follow.begin() + (long)lru);
        }
        try { c->follow.emplace_back(); } catch (...) { return nullptr; }
        f = &c->follow.back();
    }
    const FollowLayout lay(p.blocksX * p.blocksY);
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, lay.bytes());
    if (e == hipSuccess) e = hipMemsetAsync((char*)d + lay.skipAt(), 0xFF, lay.skipB, (hipStream_t)stream);    // (on the stream that uses it)
    if (e == hipSuccess) e = hipMemsetAsync((char*)d + lay.scratchAt(), 0, lay.scratchB, (hipStream_t)stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (d) (void)hipFree(d);
        c->follow.erase(c->follow.begin() + (f - c->follow.data()));
        return nullptr;
    }
    f->stream = stream;
    f->geom = g; f->blocksX = p.blocksX; f->blocksY = p.blocksY;
    f->d_mem = d;
    f->d_lives = (uint32_t*)d;
    f->d_frontMap = (uint32_t*)((char*)d + lay.mapAt());
    f->d_skipMap = (uint32_t*)((char*)d + lay.skipAt());
    f->d_scratch = (char*)d + lay.scratchAt();
    f->frontStride = lay.stride;
    f->planned = false;
    f->lastUse = ++c->followClock;
    return f;
}

// The light of a mask dispatch (light == NULL: the reference's directional light from the constants).
static void setLight(TraceParams& p, const rts_constants* k, const rts_light* light) {
    for (int i = 0; i < 3; ++i) p.cam[i] = k->cameraPosition[i];
    if (light) {
        p.lightType = light->type;
        p.nsamples = light->nsamples > 1 ? light->nsamples : 1;
        for (int i = 0; i < 3; ++i) p.light[i] = light->xyz[i];
        p.lightTable = p.nsamples > 1 ? light->table : 0u;
        if (p.nsamples > 1) memcpy(p.offsets, light->offsets, sizeof(float) * 4 * (p.lightTable ? p.lightTable : p.nsamples));
    } else {
        p.lightType = RTS_LIGHT_DIRECTIONAL;
        p.nsamples = 1;
        for (int i = 0; i < 3; ++i) p.light[i] = k->lightDirection[i];
    }
}

// The launch shape of a dispatch in blocks of bw x bh pixels: its tile counts (Dispatch::grid), then what the options and the tile order
// decide -- a 2-D grid unless the blocks are swizzled, walked in a tile order, or more than 65535 rows of them; "row_order" on the 2-D
// grid of an unstriped dispatch.  orderApplies: an installed order of as many tiles is used (never by an active or a distance trace).
static void setGrid(const rts_ctx* c, TraceParams& p, const Dispatch& g, uint32_t bw, uint32_t bh, bool orderApplies) {
    const rts::Grid gr = g.grid(bw, bh, c->swizzle != 0);
    p.blocksX = gr.blocksX; p.blocksY = gr.blocksY; p.nBlocks = gr.nBlocks; p.gridBlocks = gr.gridBlocks;
    p.swizzle = c->swizzle ? 1u : 0u;
    if (orderApplies && c->d_tileOrder && c->useTileOrder && c->tileOrderCount == p.nBlocks && !p.swizzle) p.tileOrder = c->d_tileOrder;
    p.grid2d = (!p.swizzle && !p.tileOrder && p.blocksY <= 65535u) ? 1u : 0u;
    p.rowOrder = (p.grid2d && g.nStripes <= 1) ? (uint32_t)c->rowOrder : 0u;
}

// The active and the distance traces: one block per workgroup in natural order, 16 x 16 pixels in the lane-per-ray family and 8 x 8 in
// the packet families; a band is a whole number of block rows.
static int setBlockGrid(const rts_ctx* c, TraceParams& p, const Dispatch& g, int variant) {
    const uint32_t b = variant == rts::V_SHARE ? 16u : 8u;       // pixels per side of a workgroup's block
    if (g.nStripes > 1 && g.bandRows % b != 0) return RTS_ERR_INVALID_ARG;
    setGrid(c, p, g, b, b, false);
    return RTS_OK;
}

// The prologue of a frame trace, mask or distance: the argument checks both share -- the caller's own (ownArgsOk) in their place
// among them --, the context's parameters, the geometry.  Return: *status is the call's result.  Nothing: an empty row range or a
// stripe without a band, no launch; *status is RTS_OK.  Go: p holds the context, the buffers and the geometry; *rows > 0.
enum class Begin { Return, Nothing, Go };
static Begin beginFrame(rts_ctx* c, const rts_constants* k, const float* d_positions, uint8_t* d_mask, bool ownArgsOk, const Dispatch& g,
                        TraceParams& p, uint32_t* rows, int* status) {
    *status = RTS_ERR_INVALID_ARG;
    if (!c || !k || !d_positions || !ownArgsOk || !rts::frameRowsOk(g.W, g.H, g.rowBegin, g.rowEnd)) return Begin::Return;
    if ((uint64_t)g.W * g.H > (1ull << 31)) return Begin::Return;      // tile counts are 32-bit on the device
    *status = fillParams(c, p);
    if (*status != RTS_OK) return Begin::Return;
    if (g.rowBegin == g.rowEnd) return Begin::Nothing;
    *status = hipStatus(hipSetDevice(c->device));
    if (*status != RTS_OK) return Begin::Return;
    p.positions = (const float4*)d_positions;
    p.mask = d_mask;
    p.W = g.W; p.H = g.H; p.rowBegin = g.rowBegin; p.rowEnd = g.rowEnd;
    p.bandRows = g.bandRows; p.nStripes = g.nStripes; p.stripe = g.stripe;
    p.bandShift = g.bandShift();
    *rows = g.rows();                                                  // (stripes: virtual rows = whole owned bands)
    return *rows ? Begin::Go : Begin::Nothing;                         // (a stripe without a band: no launch)
}

// The tail of a block trace -- active, distance, soft distance, light list: one block per workgroup in natural order, in the kernel
// FAMILY the caller chose; an installed split table, a tile order and follow mode are neither used nor touched, and no statistics are
// recorded.  p holds everything but the grid.  A band that is not a whole number of block rows is refused before anything is counted.
using BlockLaunch = hipError_t (*)(int variant, const TraceParams& p, hipStream_t stream, const char** name);
static int launchBlocks(rts_ctx* c, TraceParams& p, const Dispatch& g, int family, uint64_t rts_ctx::*counter, BlockLaunch launch, void* stream) {
    const int s = setBlockGrid(c, p, g, family);
    if (s != RTS_OK) return s;
    ++c->launches;
    ++(c->*counter);
    const char* name = "";
    const hipError_t e = launch(family, p, (hipStream_t)stream, &name);
    c->lastKernel = name;
    return hipStatus(e);
}

// The family of a distance, a soft distance and a light list trace: as "kernel" asks, except that 8 and 9 run the stackless packet too
// (the wide walk has none of these forms yet).
static int blockFamily(const rts_ctx* c, uint64_t pixels) {
    if (c->variant == rts::V_AUTO) return pixels < (1u << 18) ? rts::V_SHARE : rts::V_PACKET;
    return (c->variant >= rts::V_PACKET && c->variant != rts::V_SHARE) ? rts::V_PACKET : rts::V_SHARE;
}

// A trace with an active map (include/rts.h): the kernel FAMILY the options ask for, which may be the wide packet.
static int traceActive(rts_ctx* c, TraceParams& p, const Dispatch& g, uint32_t rows, const rts_constants* k, const rts_light* light,
                       const uint8_t* d_active, void* stream) {
    const uint64_t pixels = (uint64_t)g.W * rows;
    int variant = c->variant;
    if (variant == rts::V_AUTO)                      // (the plain trace's rule, traceMaskImpl, without its "block_waves" clause)
        variant = pixels < (1u << 18) ? rts::V_SHARE
                : (c->wideCount && (!light || light->nsamples <= 1) && pixels >= (1u << 22)) ? rts::V_WIDE : rts::V_PACKET;
    if (variant == rts::V_WIDE || variant == rts::V_WIDE_C) variant = p.wide ? rts::V_WIDE : rts::V_PACKET;
    else if (variant >= rts::V_PACKET && variant <= rts::V_PACKET_PF) variant = rts::V_PACKET;
    else variant = rts::V_SHARE;
    p.activeMap = d_active;
    setLight(p, k, light);
    return launchBlocks(c, p, g, variant, &rts_ctx::activeTraces, rts::launchShadowMaskActive, stream);
}

static int traceMaskImpl(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, const Dispatch& g,
                         uint8_t* d_mask, void* stream, const uint8_t* d_active = nullptr) {
    TraceParams p; uint32_t rows = 0; int s;
    if (beginFrame(c, k, d_positions, d_mask, d_mask && rts::softLightOk(light), g, p, &rows, &s) != Begin::Go) return s;
    if (d_active) return traceActive(c, p, g, rows, k, light, d_active, stream);
    // V_AUTO: a packet's steps are a dependent chain, so it needs several waves per SIMD to overlap them;
    // a launch with fewer than ~4 waves per SIMD is faster lane-per-ray (with in-wave work sharing: measured
    // 5-20 % ahead of the plain loop on every small frame).  (Bigger packets, V_PACKET2/4, were
    // measured slower or equal on every BASELINE config and are kept as selectable variants only.)
    int variant = c->variant;
    const uint64_t pixels = (uint64_t)g.W * rows;
    // Big one-sample dispatches of a stream with a private copy take the WIDE packet (a static rule from what rts_ctx_autotune
    // picks on the 4K frames: city 0.153 against 0.164 ms, courtyard 0.562 against 0.630; at 1080p and for soft shadows the
    // stackless packet is ahead or level -- profiles/r04/tuning_robustness.log): a caller that never tunes gets the kernel the
    // tuner would have picked there, not its launch options.
    if (variant == rts::V_AUTO)
        variant = pixels < (1u << 18) ? rts::V_SHARE
                : (c->wideCount && (!light || light->nsamples <= 1) && pixels >= (1u << 22) && c->blockWaves == 1) ? rts::V_WIDE : rts::V_PACKET;
    if ((variant == rts::V_WIDE || variant == rts::V_WIDE_C) && !p.wide) variant = rts::V_PACKET;     // no private copy for this stream (see finishInstall)
    uint32_t bw, bh;
    rts::tileShape(variant, c->blockWaves, &bw, &bh);
    if (g.nStripes > 1 && g.bandRows % bh != 0) return RTS_ERR_INVALID_ARG;   // a band is a whole number of workgroup rows (8, 16 or 32 pixel rows)
    const bool soft = light && light->nsamples > 1;
    setGrid(c, p, g, bw, bh, !c->tileOrderSoftOnly || soft);
    // (soft shadows in the one-tile packet forms run 4 waves per workgroup: "soft_split")
    const bool split = soft && c->softSplit && c->blockWaves == 1 && (variant == rts::V_PACKET || variant == rts::V_WIDE);
    const size_t statWaves = split ? 4 : (size_t)c->blockWaves;
    if (c->d_waveStats && (size_t)p.gridBlocks * statWaves * 32 <= c->waveStatsBytes) {
        p.waveStats = c->d_waveStats;
        p.waveRealtime = c->d_waveStats + c->waveStatsBytes / 8;
    }
    if (c->d_clockProbe && p.grid2d && p.blocksY <= c->clockProbeRows) p.clockProbe = c->d_clockProbe;
    setLight(p, k, light);
    c->lastBlocksX = p.blocksX; c->lastBlocksY = p.blocksY; c->lastVariant = variant; c->lastGrid2d = p.grid2d != 0;
    if (c->planning) {                       // pieces only: the planning walk of the selected tiles, with visit logs
        if (!(variant == rts::V_PACKET || variant == rts::V_WIDE) || c->blockWaves != 1 || p.nsamples != 1 || !p.grid2d || !p.wide ||
            (g.nStripes > 1 && p.bandShift == 0xFFFFFFFFu))
            return planRefused("the planning walk needs a one-tile packet kernel, one sample, a 2-D grid, the private copy");
        p.waveStats = nullptr; p.waveRealtime = nullptr; p.clockProbe = nullptr; p.rowOrder = 0;
        p.skipMap = c->planning->d_pieces;   // (never read: no tile rows in this launch)
        p.pieces = c->planning->d_pieces; p.nPieces = c->planning->nPieces; p.pieceRows = c->planning->pieceRows;
        p.frontMap = nullptr; p.frontStride = 0; p.hasPieces = 1u;               // (every record is a piece)
        p.tileState = c->planning->d_state; p.pieceLog = c->planning->d_log; p.pieceLogCap = c->planning->logCap;
        p.blocksY = 0;
        return hipStatus(rts::launchShadowMask(variant, c->blockWaves, p, (hipStream_t)stream, 0));
    }
    // split table: only the everyday one-tile packet launches of the very dispatch it was planned for
    const rts_ctx::Splits& sp = c->splits;
    if (sp.valid && c->useSplits && sp.nPieces && (variant == rts::V_PACKET || variant == rts::V_WIDE) && c->blockWaves == 1 &&
        p.nsamples == 1 && p.grid2d && !p.waveStats && !c->wideLane && p.wide &&
        (g.nStripes <= 1 || (p.bandShift != 0xFFFFFFFFu && p.rowOrder == 0)) &&
        madeFor(sp, g, p) && p.blocksY + sp.pieceRows <= 65535u) {
        if (uint64_t* st = splitState(c, stream)) {
            p.skipMap = sp.d_skipMap; p.pieces = sp.d_pieces; p.nPieces = sp.nPieces; p.pieceRows = sp.pieceRows;
            p.frontMap = sp.d_frontMap; p.frontStride = sp.frontStride;
            p.tileState = st;
            p.allInTable = sp.allTiles ? 1u : 0u;
            p.hasPieces = sp.nTiles ? 1u : 0u;
            if (c->d_pieceClock && c->pieceClockCount >= sp.nPieces) p.pieceClock = c->d_pieceClock;
            // (a whole-dispatch table without pieces: kernel 8 may take its ALLTABLE instantiation -- rts::allTableLaunch)
            if (variant == rts::V_WIDE && sp.allTiles && !sp.nTiles) p.sceneBounds = c->d_sceneBounds;
        }
    }
    // follow mode: where a split table could apply but none does, the trace records its tile lives and runs the order the planner
    // made from the lives of the stream's last trace of this dispatch (the front-only table launch, every tile a record: launch
    // parameters that depend on the geometry alone); then the planner's kernels make the next one, in the stream.  (Stripes: the
    // option "row_order" itself must be 0, as include/rts.h says -- p.rowOrder is 0 for every stripe, whatever the option.)
    rts_ctx::Follow* fol = nullptr;
    if (c->followOn && !p.pieces && (variant == rts::V_PACKET || variant == rts::V_WIDE) && c->blockWaves == 1 && p.nsamples == 1 &&
        p.grid2d && !p.waveStats && !c->wideLane && p.wide && (g.nStripes <= 1 || (p.bandShift != 0xFFFFFFFFu && c->rowOrder == 0)))
        fol = followFor(c, stream, g, p);
    if (fol) {
        p.followLives = fol->d_lives;
        if (fol->planned) {
            p.skipMap = fol->d_skipMap; p.pieces = fol->d_skipMap;            // (no tile rows and no pieces: neither is read)
            p.nPieces = p.nBlocks; p.pieceRows = p.blocksY;
            p.frontMap = fol->d_frontMap; p.frontStride = fol->frontStride;
            p.allInTable = 1u; p.hasPieces = 0u; p.tileState = nullptr;
            ++c->followOrdered;
        }
        ++c->followTraces;
    }
    // (the ALLTABLE instantiation is an instantiation of kernel 8 like the other table forms and keeps its name -- the committed counter
    //  summaries are keyed by it; the option "alltable_traces" counts its launches)
    c->lastKernel = fol ? (variant == rts::V_WIDE ? "shadowMaskFollowKernel<1,wide>" : "shadowMaskFollowKernel<1>") : rts::kernelName(variant, true);
    if (!fol && variant == rts::V_WIDE && rts::allTableLaunch(p, c->blockWaves)) ++c->allTableTraces;
    ++c->launches;
    hipError_t e = rts::launchShadowMask(variant, c->blockWaves, p, (hipStream_t)stream, (uint32_t)c->ldsPad);
    if (e == hipSuccess && fol) {
        e = rts::launchFollowPlan(fol->d_lives, p.blocksX, p.blocksY, (uint32_t)c->followSquare, (uint32_t)c->followBlock, followBands(),
                                  fol->d_scratch, fol->d_frontMap, fol->frontStride, (hipStream_t)stream);
        if (e == hipSuccess) fol->planned = true;
    }
    return hipStatus(e);
}

int rts_trace_shadow_mask_device(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, uint32_t W, uint32_t H,
                                 uint32_t row_begin, uint32_t row_end, uint8_t* d_mask, void* stream) {
    return traceMaskImpl(c, k, light, d_positions, Dispatch::ofRows(W, H, row_begin, row_end), d_mask, stream);
}

int rts_trace_shadow_mask_stripes_device(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, uint32_t W,
                                         uint32_t H, uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_mask, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    const Dispatch g = Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe);
    if (n_stripes > 1 && g.rows() == 0) return RTS_OK;     // a stripe that owns no band launches nothing, whatever the other arguments are
    // dispatch its virtual rows; the kernel maps them onto the frame (ownedRow) and guards with row < H
    return traceMaskImpl(c, k, light, d_positions, g, d_mask, stream);
}

int rts_trace_shadow_mask_active_device(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions,
                                        const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                        uint8_t* d_mask, void* stream) {
    return traceMaskImpl(c, k, light, d_positions, Dispatch::ofRows(W, H, row_begin, row_end), d_mask, stream, d_active);
}

int rts_trace_shadow_mask_active_stripes_device(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions,
                                                const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_stripes,
                                                uint32_t stripe, uint8_t* d_mask, void* stream) {
    if (!d_active) return rts_trace_shadow_mask_stripes_device(c, k, light, d_positions, W, H, band_rows, n_stripes, stripe, d_mask, stream);
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    // (a stripe that owns no band launches nothing: beginFrame, after the argument checks)
    return traceMaskImpl(c, k, light, d_positions, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), d_mask, stream, d_active);
}

int rts_trace_rays_device(rts_ctx* c, const rts_ray* d_rays, size_t n, uint8_t* d_out, void* stream) {
    if (!c || (n && (!d_rays || !d_out)) || n > (1ull << 38)) return RTS_ERR_INVALID_ARG;   // grid.x is 31-bit
    TraceParams p;
    int s = fillParams(c, p);
    if (s != RTS_OK) return s;
    if (n == 0) return RTS_OK;
    RTS_HIP(hipSetDevice(c->device));
    p.rays = d_rays; p.out = d_out; p.nrays = n;
    // generic rays carry no coherence promise: lane-per-ray with in-wave work sharing unless the caller asks for a
    // variant (random segments: 2x the plain loop; coherent rays: equal; profiles/r01/generic_rays_variants.log)
    const int variant = c->variant == rts::V_AUTO ? rts::V_SHARE : c->variant;
    c->lastKernel = rts::kernelName(variant, false);
    ++c->launches;
    return hipStatus(rts::launchTraceRays(variant, p, (hipStream_t)stream));
}

// ---- occluder distance (include/rts.h): the nearest accepted triangle's t beside the shadow byte ---------------------------------
// One launch of a distance kernel (rts_distance.inc) through the block traces' tail (launchBlocks), in the family of blockFamily.
static int traceDistanceImpl(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, const uint8_t* d_active,
                             const Dispatch& g, float* d_distance, uint8_t* d_mask, void* stream) {
    TraceParams p; uint32_t rows = 0; int s;
    if (beginFrame(c, k, d_positions, d_mask, d_distance && rts::hardLightOk(light), g, p, &rows, &s) != Begin::Go) return s;   // one sample in this version
    p.distance = d_distance;
    p.activeMap = d_active;
    setLight(p, k, light);
    return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::distanceTraces, rts::launchShadowDistance, stream);
}

int rts_trace_shadow_distance_device(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions,
                                     const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                     float* d_distance, uint8_t* d_mask, void* stream) {
    return traceDistanceImpl(c, k, light, d_positions, d_active, Dispatch::ofRows(W, H, row_begin, row_end), d_distance, d_mask, stream);
}

int rts_trace_shadow_distance_stripes_device(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions,
                                             const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_stripes,
                                             uint32_t stripe, float* d_distance, uint8_t* d_mask, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return traceDistanceImpl(c, k, light, d_positions, d_active, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), d_distance, d_mask, stream);
}

// ---- soft-shadow occluder distance (include/rts.h): the nearest blocker over all light samples, beside the count of unoccluded ones --
// One launch of a soft distance kernel (rts_soft_distance.inc) with the geometry, the family rule and the tail of a distance trace; a
// light of one sample IS the distance trace.
static int traceSoftDistanceImpl(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, const uint8_t* d_active,
                                 const Dispatch& g, float* d_distance, uint8_t* d_mask, void* stream) {
    if (!rts::softLightOk(light)) return RTS_ERR_INVALID_ARG;                                              // (the mask trace's rule)
    if (!light || light->nsamples <= 1) return traceDistanceImpl(c, k, light, d_positions, d_active, g, d_distance, d_mask, stream);
    TraceParams p; uint32_t rows = 0; int s;
    if (beginFrame(c, k, d_positions, d_mask, d_distance != nullptr, g, p, &rows, &s) != Begin::Go) return s;
    p.distance = d_distance;
    p.activeMap = d_active;
    setLight(p, k, light);
    return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::softDistanceTraces, rts::launchShadowSoftDistance, stream);
}

int rts_trace_soft_distance_device(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions,
                                   const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                   float* d_distance, uint8_t* d_mask, void* stream) {
    return traceSoftDistanceImpl(c, k, light, d_positions, d_active, Dispatch::ofRows(W, H, row_begin, row_end), d_distance, d_mask, stream);
}

int rts_trace_soft_distance_stripes_device(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions,
                                           const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_stripes,
                                           uint32_t stripe, float* d_distance, uint8_t* d_mask, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return traceSoftDistanceImpl(c, k, light, d_positions, d_active, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), d_distance, d_mask, stream);
}

// ---- ambient occlusion (include/rts.h): hemisphere segments around the G-buffer's normal, the unoccluded ones counted ----------------
// One launch of an AO kernel (rts_ao.inc) with the geometry, the family rule and the tail of a distance trace.  The normals travel in
// the distances' slot of the argument block, the radius in the light's x, the directions in the sample offsets and their table size
// in the light's table (rts_ao.h), so sampleIndex and pixelBase are the mask traces' own.
// probe == 0: the AO trace itself.  probe != 0: its adaptive form (rts_ao_adaptive.inc), the probe count and the refined plane in the
// slots rts_ao_adaptive.h names, counted by "ao_adaptive_traces" alone.
// bent: the bent-normal form (rts_ao_bent.inc): the bent plane in the slot rts_ao_bent.h names, required, the counts optional; counted by
// "ao_bent_traces" alone.
// dist: the distance form (rts_ao_distance.inc): the distance plane, the obscurance plane and the falloff's weights in the slots
// rts_ao_distance.h names, one of the two planes required, the counts optional; counted by "ao_distance_traces" alone.
struct AoDistanceOut { float* d_distance; uint16_t* d_obscurance; const rts_ao_falloff* falloff; };
static bool aoDistanceOutOk(const AoDistanceOut& o) {
    return (o.d_distance || o.d_obscurance) && (!o.d_obscurance || o.falloff) && ((uintptr_t)o.d_obscurance & 1u) == 0 &&
           ((uintptr_t)o.d_distance & 3u) == 0;
}
static int traceAmbientOcclusionImpl(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const float* d_positions,
                                     const float* d_normals, const uint8_t* d_active, const Dispatch& g, uint8_t* d_counts, void* stream,
                                     bool adaptive = false, uint32_t probe = 0, uint8_t* d_refined = nullptr, bool bent = false,
                                     float* d_bent = nullptr, const AoDistanceOut* dist = nullptr) {
    TraceParams p; uint32_t rows = 0; int s;
    const bool ownOk = (dist ? aoDistanceOutOk(*dist) : bent ? d_bent != nullptr : d_counts != nullptr) && d_normals &&
                       (adaptive ? rts::aoAdaptiveOk(ao, probe) : rts::aoParamsOk(ao));
    if (beginFrame(c, k, d_positions, d_counts, ownOk, g, p, &rows, &s) != Begin::Go) return s;
    rts::setAoNormals(p, d_normals);
    p.activeMap = d_active;
    for (int i = 0; i < 3; ++i) p.cam[i] = k->cameraPosition[i];
    p.lightType = RTS_LIGHT_POINT;
    p.nsamples = ao->nsamples > 1 ? ao->nsamples : 1u;
    p.lightTable = ao->table;
    p.light[0] = ao->radius; p.light[1] = 0.0f; p.light[2] = 0.0f;
    memcpy(p.offsets, ao->dirs, sizeof(float) * 4 * (p.lightTable ? p.lightTable : p.nsamples));
    if (adaptive) {
        p.nrays = probe;
        rts::setAoRefined(p, d_refined);
        return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::aoAdaptiveTraces, rts::launchAmbientOcclusionAdaptive, stream);
    }
    if (bent) {
        rts::setAoBent(p, d_bent);
        return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::aoBentTraces, rts::launchAmbientOcclusionBent, stream);
    }
    if (dist) {
        rts::setAoDistance(p, dist->d_distance, dist->d_obscurance, dist->falloff ? dist->falloff->weight : nullptr);
        return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::aoDistanceTraces, rts::launchAmbientOcclusionDistance, stream);
    }
    return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::aoTraces, rts::launchAmbientOcclusion, stream);
}

int rts_trace_ambient_occlusion_device(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const float* d_positions,
                                       const float* d_normals, const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t row_begin,
                                       uint32_t row_end, uint8_t* d_counts, void* stream) {
    return traceAmbientOcclusionImpl(c, k, ao, d_positions, d_normals, d_active, Dispatch::ofRows(W, H, row_begin, row_end), d_counts, stream);
}

int rts_trace_ambient_occlusion_stripes_device(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const float* d_positions,
                                               const float* d_normals, const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t band_rows,
                                               uint32_t n_stripes, uint32_t stripe, uint8_t* d_counts, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return traceAmbientOcclusionImpl(c, k, ao, d_positions, d_normals, d_active, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe),
                                     d_counts, stream);
}

int rts_trace_ambient_occlusion_adaptive_device(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const float* d_positions,
                                                const float* d_normals, const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t row_begin,
                                                uint32_t row_end, uint32_t probe, uint8_t* d_counts, uint8_t* d_refined, void* stream) {
    return traceAmbientOcclusionImpl(c, k, ao, d_positions, d_normals, d_active, Dispatch::ofRows(W, H, row_begin, row_end), d_counts, stream,
                                     true, probe, d_refined);
}

int rts_trace_ambient_occlusion_adaptive_stripes_device(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const float* d_positions,
                                                        const float* d_normals, const uint8_t* d_active, uint32_t W, uint32_t H,
                                                        uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint32_t probe,
                                                        uint8_t* d_counts, uint8_t* d_refined, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return traceAmbientOcclusionImpl(c, k, ao, d_positions, d_normals, d_active, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe),
                                     d_counts, stream, true, probe, d_refined);
}

int rts_trace_ambient_occlusion_bent_device(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const float* d_positions,
                                            const float* d_normals, const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t row_begin,
                                            uint32_t row_end, uint8_t* d_counts, float* d_bent, void* stream) {
    return traceAmbientOcclusionImpl(c, k, ao, d_positions, d_normals, d_active, Dispatch::ofRows(W, H, row_begin, row_end), d_counts, stream,
                                     false, 0, nullptr, true, d_bent);
}

int rts_trace_ambient_occlusion_bent_stripes_device(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const float* d_positions,
                                                    const float* d_normals, const uint8_t* d_active, uint32_t W, uint32_t H,
                                                    uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_counts,
                                                    float* d_bent, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return traceAmbientOcclusionImpl(c, k, ao, d_positions, d_normals, d_active, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe),
                                     d_counts, stream, false, 0, nullptr, true, d_bent);
}

int rts_trace_ambient_occlusion_distance_device(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const rts_ao_falloff* falloff,
                                                const float* d_positions, const float* d_normals, const uint8_t* d_active, uint32_t W,
                                                uint32_t H, uint32_t row_begin, uint32_t row_end, uint8_t* d_counts, float* d_distance,
                                                uint16_t* d_obscurance, void* stream) {
    const AoDistanceOut out{ d_distance, d_obscurance, falloff };
    return traceAmbientOcclusionImpl(c, k, ao, d_positions, d_normals, d_active, Dispatch::ofRows(W, H, row_begin, row_end), d_counts, stream,
                                     false, 0, nullptr, false, nullptr, &out);
}

int rts_trace_ambient_occlusion_distance_stripes_device(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao,
                                                        const rts_ao_falloff* falloff, const float* d_positions, const float* d_normals,
                                                        const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t band_rows,
                                                        uint32_t n_stripes, uint32_t stripe, uint8_t* d_counts, float* d_distance,
                                                        uint16_t* d_obscurance, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    const AoDistanceOut out{ d_distance, d_obscurance, falloff };
    return traceAmbientOcclusionImpl(c, k, ao, d_positions, d_normals, d_active, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe),
                                     d_counts, stream, false, 0, nullptr, false, nullptr, &out);
}

// ---- adaptive soft shadows (include/rts.h): a probe of a few samples per pixel, the others only where the probe disagrees ------------
// One launch of an adaptive kernel (rts_adaptive.inc) with the geometry, the family rule and the tail of a distance trace.  The probe
// count and the refined plane travel in the generic rays' slots of the argument block (rts_adaptive.h).
static int traceAdaptiveImpl(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, const uint8_t* d_active,
                             const Dispatch& g, uint32_t probe, uint8_t* d_mask, uint8_t* d_refined, void* stream) {
    TraceParams p; uint32_t rows = 0; int s;
    if (beginFrame(c, k, d_positions, d_mask, d_mask && rts::adaptiveLightOk(light, probe), g, p, &rows, &s) != Begin::Go) return s;
    p.activeMap = d_active;
    p.out = d_refined;
    p.nrays = probe;
    setLight(p, k, light);
    return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::adaptiveTraces, rts::launchShadowMaskAdaptive, stream);
}

int rts_trace_shadow_mask_adaptive_device(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions,
                                          const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                          uint32_t probe, uint8_t* d_mask, uint8_t* d_refined, void* stream) {
    return traceAdaptiveImpl(c, k, light, d_positions, d_active, Dispatch::ofRows(W, H, row_begin, row_end), probe, d_mask, d_refined, stream);
}

int rts_trace_shadow_mask_adaptive_stripes_device(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions,
                                                  const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_stripes,
                                                  uint32_t stripe, uint32_t probe, uint8_t* d_mask, uint8_t* d_refined, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return traceAdaptiveImpl(c, k, light, d_positions, d_active, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), probe, d_mask, d_refined,
                             stream);
}

int rts_trace_rays_distance_device(rts_ctx* c, const rts_ray* d_rays, size_t n, float* d_out_t, void* stream) {
    if (!c || (n && (!d_rays || !d_out_t)) || n > (1ull << 38)) return RTS_ERR_INVALID_ARG;   // grid.x is 31-bit
    TraceParams p;
    int s = fillParams(c, p);
    if (s != RTS_OK) return s;
    if (n == 0) return RTS_OK;
    RTS_HIP(hipSetDevice(c->device));
    p.rays = d_rays; p.distance = d_out_t; p.nrays = n;
    c->lastKernel = "traceRaysDistanceKernel";
    ++c->launches;
    ++c->distanceTraces;
    return hipStatus(rts::launchTraceRaysDistance(p, (hipStream_t)stream));
}

// ---- the host-pointer entries: the same traces through the context's staging buffers ----------------------------------------------
// Frames (arguments checked by the caller): only rows [rowBegin, rowEnd) travel -- their positions, map, mask and distances, as a
// frame of their own, to the device entry of what is being traced.  StagedRows names what a host entry hands over: the first nine
// members every entry gives, in this order; the others it sets by name, and what it leaves alone is NULL.
enum class Staged { Mask, Distance, SoftDistance, LightList, Adaptive, SoftLightList, SoftListAdaptive, SoftListDistance, AmbientOcclusion,
                    AoAdaptive, AoBent, AoDistance };
struct StagedRows {
    Staged what;
    const rts_constants* k;
    const void* lights;                  // the rts_light; Staged::LightList: the rts_light_list; the soft lists: the rts_soft_light_list;
                                         // Staged::AmbientOcclusion: the rts_ao_params --
                                         // each case below names the type it reads, and nothing else does
    const float* positions;
    const uint8_t* active;               // the active map, or a list's light map
    uint32_t W, H, rowBegin, rowEnd;     // the caller's frame: its planes are W * H apart, of the staged rows alone on the device
    uint8_t* mask = nullptr;             // the mask; a soft list's count planes, `count` of them (optional beside distances)
    float* distance = nullptr;           // of the distance traces alone; Staged::SoftListDistance: a plane per light, like the counts
    uint32_t probe = 0;                  // Staged::Adaptive, Staged::AoAdaptive
    uint8_t* refined = nullptr;          // Staged::Adaptive, Staged::SoftListAdaptive (optional): staged in the distances' buffer;
                                         // Staged::AoAdaptive (optional): behind the normals there
    const uint32_t* probes = nullptr;    // Staged::SoftListAdaptive: one per light
    const uint32_t* tables = nullptr;    // ... its jittered form, whose hash pixelBase makes that of the caller's frame
    const float* normals = nullptr;      // Staged::AmbientOcclusion, Staged::AoAdaptive, Staged::AoBent: staged in the distances' buffer
    float* bent = nullptr;               // Staged::AoBent: W x H RGBA32F, behind the normals there (its counts, `mask`, are optional)
    float* aoDistance = nullptr;         // Staged::AoDistance (optional): W x H floats, behind the normals there
    uint16_t* obscurance = nullptr;      // Staged::AoDistance (optional): W x H uint16_t, behind that plane's place
    const rts_ao_falloff* falloff = nullptr;   // ... and its falloff
};
static int traceStagedRows(rts_ctx* c, const StagedRows& r) {
    if (!c->d_bvh) return RTS_ERR_NO_BVH;
    if (r.rowBegin == r.rowEnd) return RTS_OK;
    RTS_HIP(hipSetDevice(c->device));
    const uint32_t W = r.W, rows = r.rowEnd - r.rowBegin;
    const size_t first = (size_t)r.rowBegin * W, pixels = (size_t)rows * W, frame = (size_t)W * r.H;
    int s = ensure(&c->d_in, &c->inBytes, pixels * 16);
    const bool softList = r.what == Staged::SoftLightList || r.what == Staged::SoftListAdaptive || r.what == Staged::SoftListDistance;
    const size_t planes = softList ? ((const rts_soft_light_list*)r.lights)->count : 1u;
    const size_t distPlanes = r.what == Staged::SoftListDistance ? planes : 1u;
    if (s == RTS_OK && r.distance) s = ensure(&c->d_dist, &c->distBytes, pixels * 4 * distPlanes);
    if (s == RTS_OK && r.refined) s = ensure(&c->d_dist, &c->distBytes, pixels);
    if (s == RTS_OK && r.normals) s = ensure(&c->d_dist, &c->distBytes, pixels * 16 + (r.refined ? pixels : 0u) + (r.bent ? pixels * 16 : 0u) +
                                                (r.what == Staged::AoDistance ? pixels * 6 : 0u));
    if (s == RTS_OK && r.mask) s = ensure(&c->d_out, &c->outBytes, pixels * planes);
    if (s == RTS_OK && r.active) s = ensure(&c->d_act, &c->actBytes, pixels);
    if (s != RTS_OK) return s;
    RTS_HIP(hipMemcpy(c->d_in, r.positions + first * 4, pixels * 16, hipMemcpyHostToDevice));
    if (r.active) RTS_HIP(hipMemcpy(c->d_act, r.active + first, pixels, hipMemcpyHostToDevice));
    if (r.normals) RTS_HIP(hipMemcpy(c->d_dist, r.normals + first * 4, pixels * 16, hipMemcpyHostToDevice));
    const rts_constants* const k = r.k;
    const rts_light* const light = (const rts_light*)r.lights;
    const rts_soft_light_list* const softLights = (const rts_soft_light_list*)r.lights;
    const uint8_t* d_active = r.active ? (const uint8_t*)c->d_act : nullptr;
    uint8_t* d_mask = r.mask ? (uint8_t*)c->d_out : nullptr;
    uint8_t* d_refined = r.refined ? (uint8_t*)c->d_dist + (r.normals ? pixels * 16 : 0u) : nullptr;
    const float* d_in = (const float*)c->d_in;
    float* d_dist = (float*)c->d_dist;
    float* d_bent = r.bent ? d_dist + pixels * 4 : nullptr;
    float* d_aoDistance = r.aoDistance ? d_dist + pixels * 4 : nullptr;
    uint16_t* d_obscurance = r.obscurance ? (uint16_t*)(d_dist + pixels * 5) : nullptr;
    // per-pixel jitter hashes the pixel's index in the caller's frame (sampleIndex, rts_kernels.hip: the one reader, and only of a
    // light with a table -- several samples, so in a mask trace or a soft distance trace; of the lists the jittered one alone reads it)
    c->pixelBase = r.rowBegin * W;
    switch (r.what) {
    case Staged::Mask:
        s = rts_trace_shadow_mask_active_device(c, k, light, d_in, d_active, W, rows, 0, rows, d_mask, nullptr); break;
    case Staged::Distance:
        s = rts_trace_shadow_distance_device(c, k, light, d_in, d_active, W, rows, 0, rows, d_dist, d_mask, nullptr); break;
    case Staged::SoftDistance:
        s = rts_trace_soft_distance_device(c, k, light, d_in, d_active, W, rows, 0, rows, d_dist, d_mask, nullptr); break;
    case Staged::LightList:
        s = rts_trace_light_list_device(c, k, (const rts_light_list*)r.lights, d_in, d_active, W, rows, 0, rows, d_mask, nullptr); break;
    case Staged::Adaptive:
        s = rts_trace_shadow_mask_adaptive_device(c, k, light, d_in, d_active, W, rows, 0, rows, r.probe, d_mask, d_refined, nullptr); break;
    case Staged::SoftLightList:
        s = rts_trace_soft_light_list_device(c, k, softLights, d_in, d_active, W, rows, 0, rows, d_mask, nullptr); break;
    case Staged::SoftListAdaptive:
        s = rts_trace_soft_light_list_jittered_device(c, k, softLights, d_in, d_active, W, rows, 0, rows, d_mask, r.probes, r.tables, d_refined,
                                                      nullptr); break;
    case Staged::SoftListDistance:
        s = rts_trace_soft_light_list_distance_device(c, k, softLights, d_in, d_active, W, rows, 0, rows, d_dist, d_mask, nullptr); break;
    case Staged::AmbientOcclusion:
        s = rts_trace_ambient_occlusion_device(c, k, (const rts_ao_params*)r.lights, d_in, d_dist, d_active, W, rows, 0, rows, d_mask,
                                               nullptr); break;
    case Staged::AoAdaptive:
        s = rts_trace_ambient_occlusion_adaptive_device(c, k, (const rts_ao_params*)r.lights, d_in, d_dist, d_active, W, rows, 0, rows,
                                                        r.probe, d_mask, d_refined, nullptr); break;
    case Staged::AoBent:
        s = rts_trace_ambient_occlusion_bent_device(c, k, (const rts_ao_params*)r.lights, d_in, d_dist, d_active, W, rows, 0, rows, d_mask,
                                                    d_bent, nullptr); break;
    case Staged::AoDistance:
        s = rts_trace_ambient_occlusion_distance_device(c, k, (const rts_ao_params*)r.lights, r.falloff, d_in, d_dist, d_active, W, rows, 0,
                                                        rows, d_mask, d_aoDistance, d_obscurance, nullptr); break;
    }
    c->pixelBase = 0;
    if (s != RTS_OK) return s;
    for (size_t l = 0; r.distance && l < distPlanes; ++l)
        RTS_HIP(hipMemcpy(r.distance + l * frame + first, (const float*)c->d_dist + l * pixels, pixels * 4, hipMemcpyDeviceToHost));
    if (r.refined) RTS_HIP(hipMemcpy(r.refined + first, d_refined, pixels, hipMemcpyDeviceToHost));
    if (r.bent) RTS_HIP(hipMemcpy(r.bent + first * 4, d_bent, pixels * 16, hipMemcpyDeviceToHost));
    if (r.aoDistance) RTS_HIP(hipMemcpy(r.aoDistance + first, d_aoDistance, pixels * 4, hipMemcpyDeviceToHost));
    if (r.obscurance) RTS_HIP(hipMemcpy(r.obscurance + first, d_obscurance, pixels * 2, hipMemcpyDeviceToHost));
    for (size_t l = 0; r.mask && l < planes; ++l)
        RTS_HIP(hipMemcpy(r.mask + l * frame + first, (const uint8_t*)c->d_out + l * pixels, pixels, hipMemcpyDeviceToHost));
    return RTS_OK;
}

// The frame of a soft list's host entry: its rows, and the device forms' limit of 2^31 pixels, said before anything is staged.
static bool stagedListFrameOk(uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end) {
    return rts::frameRowsOk(W, H, row_begin, row_end) && (uint64_t)W * H <= (1ull << 31);
}

int rts_trace_shadow_mask_active(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* positions, const uint8_t* active,
                                 uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, uint8_t* mask) {
    if (!c || !k || !positions || !mask || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::Mask, k, light, positions, active, W, H, row_begin, row_end };
    r.mask = mask;
    return traceStagedRows(c, r);
}

int rts_trace_shadow_mask(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* positions,
                          uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, uint8_t* mask) {
    return rts_trace_shadow_mask_active(c, k, light, positions, nullptr, W, H, row_begin, row_end, mask);
}

int rts_trace_shadow_distance(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* positions, const uint8_t* active,
                              uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, float* distance, uint8_t* mask) {
    if (!c || !k || !positions || !distance || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::hardLightOk(light)) return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::Distance, k, light, positions, active, W, H, row_begin, row_end };
    r.distance = distance; r.mask = mask;
    return traceStagedRows(c, r);
}

int rts_trace_soft_distance(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* positions, const uint8_t* active,
                            uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, float* distance, uint8_t* mask) {
    if (!c || !k || !positions || !distance || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::softLightOk(light)) return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::SoftDistance, k, light, positions, active, W, H, row_begin, row_end };
    r.distance = distance; r.mask = mask;
    return traceStagedRows(c, r);
}

int rts_trace_ambient_occlusion(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const float* positions, const float* normals,
                                const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, uint8_t* counts) {
    if (!c || !k || !positions || !normals || !counts || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::aoParamsOk(ao) || (uint64_t)W * H > (1ull << 31)) return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::AmbientOcclusion, k, ao, positions, active, W, H, row_begin, row_end };
    r.mask = counts; r.normals = normals;
    return traceStagedRows(c, r);
}

int rts_trace_ambient_occlusion_adaptive(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const float* positions,
                                         const float* normals, const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin,
                                         uint32_t row_end, uint32_t probe, uint8_t* counts, uint8_t* refined) {
    if (!c || !k || !positions || !normals || !counts || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::aoAdaptiveOk(ao, probe) || (uint64_t)W * H > (1ull << 31)) return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::AoAdaptive, k, ao, positions, active, W, H, row_begin, row_end };
    r.mask = counts; r.normals = normals; r.probe = probe; r.refined = refined;
    return traceStagedRows(c, r);
}

int rts_trace_ambient_occlusion_bent(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const float* positions,
                                     const float* normals, const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin,
                                     uint32_t row_end, uint8_t* counts, float* bent) {
    if (!c || !k || !positions || !normals || !bent || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::aoParamsOk(ao) || (uint64_t)W * H > (1ull << 31)) return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::AoBent, k, ao, positions, active, W, H, row_begin, row_end };
    r.mask = counts; r.normals = normals; r.bent = bent;
    return traceStagedRows(c, r);
}

int rts_trace_ambient_occlusion_distance(rts_ctx* c, const rts_constants* k, const rts_ao_params* ao, const rts_ao_falloff* falloff,
                                         const float* positions, const float* normals, const uint8_t* active, uint32_t W, uint32_t H,
                                         uint32_t row_begin, uint32_t row_end, uint8_t* counts, float* distance, uint16_t* obscurance) {
    if (!c || !k || !positions || !normals || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::aoParamsOk(ao) || (uint64_t)W * H > (1ull << 31) || !aoDistanceOutOk(AoDistanceOut{ distance, obscurance, falloff }))
        return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::AoDistance, k, ao, positions, active, W, H, row_begin, row_end };
    r.mask = counts; r.normals = normals; r.aoDistance = distance; r.obscurance = obscurance; r.falloff = falloff;
    return traceStagedRows(c, r);
}

// ---- light lists (include/rts.h): up to 8 hard lights in one dispatch, one bit per light in the mask byte ----------------------------
// What the hard and the soft list both say in front of their lights: the count in nsamples, the map in the active map's slot.
static void setListHeader(TraceParams& p, const rts_constants* k, uint32_t count, const uint8_t* d_lights_map) {
    p.activeMap = d_lights_map;
    for (int i = 0; i < 3; ++i) p.cam[i] = k->cameraPosition[i];
    p.lightType = RTS_LIGHT_DIRECTIONAL;               // (not read: every light carries its own type)
    p.nsamples = count;
    p.lightTable = 0;
    for (int i = 0; i < 3; ++i) p.light[i] = 0.0f;
}

// One launch of a light list kernel (rts_light_list.inc) with the geometry, the family rule and the tail of a distance trace.  The
// list travels in the argument block's 64 sample offsets: light l in offsets[l] = {x, y, z, 0.0f directional / 1.0f point}.
static int traceLightListImpl(rts_ctx* c, const rts_constants* k, const rts_light_list* list, const float* d_positions,
                              const uint8_t* d_lights_map, const Dispatch& g, uint8_t* d_mask, void* stream) {
    TraceParams p; uint32_t rows = 0; int s;
    if (beginFrame(c, k, d_positions, d_mask, d_mask && rts::lightListOk(list), g, p, &rows, &s) != Begin::Go) return s;
    setListHeader(p, k, list->count, d_lights_map);
    for (uint32_t l = 0; l < list->count; ++l) {
        for (int i = 0; i < 3; ++i) p.offsets[l][i] = list->lights[l].xyz[i];
        p.offsets[l][3] = list->lights[l].type == RTS_LIGHT_POINT ? 1.0f : 0.0f;
    }
    return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::lightListTraces, rts::launchShadowLightList, stream);
}

int rts_trace_light_list_device(rts_ctx* c, const rts_constants* k, const rts_light_list* list, const float* d_positions,
                                const uint8_t* d_lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                uint8_t* d_mask, void* stream) {
    return traceLightListImpl(c, k, list, d_positions, d_lights_map, Dispatch::ofRows(W, H, row_begin, row_end), d_mask, stream);
}

int rts_trace_light_list_stripes_device(rts_ctx* c, const rts_constants* k, const rts_light_list* list, const float* d_positions,
                                        const uint8_t* d_lights_map, uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_stripes,
                                        uint32_t stripe, uint8_t* d_mask, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return traceLightListImpl(c, k, list, d_positions, d_lights_map, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), d_mask, stream);
}

// The host form goes through traceStagedRows like the other host entries, the list in the light's place and the map in the active
// map's.  traceStagedRows sets pixelBase around the call all the same; of the list traces only the jittered soft list reads it.
int rts_trace_light_list(rts_ctx* c, const rts_constants* k, const rts_light_list* list, const float* positions, const uint8_t* lights_map,
                         uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, uint8_t* mask) {
    if (!c || !k || !positions || !mask || !rts::frameRowsOk(W, H, row_begin, row_end) || !rts::lightListOk(list)) return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::LightList, k, list, positions, lights_map, W, H, row_begin, row_end };
    r.mask = mask;
    return traceStagedRows(c, r);
}

// ---- soft light lists (include/rts.h): up to 8 lights, hard or soft, in one dispatch, one count plane per light -----------------------
// The list in the argument block, what the soft list trace and its adaptive form both launch with: it travels in the 64 sample offsets
// (rts_soft_light_list.h) -- the shared table in the first 48, two slots per light behind them -- behind the lists' header.
static void setSoftList(TraceParams& p, const rts_constants* k, const rts_soft_light_list* list, const uint8_t* d_lights_map) {
    setListHeader(p, k, list->count, d_lights_map);
    rts::setSoftList(p.offsets, list);
}

// One launch of a soft light list kernel (rts_soft_light_list.inc) with the geometry, the family rule and the tail of a distance trace.
// The planes travel in the mask's slot.
static int traceSoftLightListImpl(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* d_positions,
                                  const uint8_t* d_lights_map, const Dispatch& g, uint8_t* d_counts, void* stream) {
    TraceParams p; uint32_t rows = 0; int s;
    if (beginFrame(c, k, d_positions, d_counts, d_counts && rts::softListOk(list), g, p, &rows, &s) != Begin::Go) return s;
    setSoftList(p, k, list, d_lights_map);
    return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::softLightListTraces, rts::launchShadowSoftLightList, stream);
}

int rts_trace_soft_light_list_device(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* d_positions,
                                     const uint8_t* d_lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                     uint8_t* d_counts, void* stream) {
    return traceSoftLightListImpl(c, k, list, d_positions, d_lights_map, Dispatch::ofRows(W, H, row_begin, row_end), d_counts, stream);
}

int rts_trace_soft_light_list_stripes_device(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* d_positions,
                                             const uint8_t* d_lights_map, uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_stripes,
                                             uint32_t stripe, uint8_t* d_counts, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return traceSoftLightListImpl(c, k, list, d_positions, d_lights_map, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), d_counts, stream);
}

// The host form goes through traceStagedRows like the other host entries: its rows travel as a frame of their own, whose `count`
// planes come back to the caller's planes of H rows.
int rts_trace_soft_light_list(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* positions,
                              const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, uint8_t* counts) {
    if (!c || !k || !positions || !counts || !stagedListFrameOk(W, H, row_begin, row_end) || !rts::softListOk(list)) return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::SoftLightList, k, list, positions, lights_map, W, H, row_begin, row_end };
    r.mask = counts;
    return traceStagedRows(c, r);
}

// ---- sparse light lists (include/rts.h): the two list traces over a LIST of pixels, the marked pairs alone written -----------------
// One launch of a sparse kernel (rts_light_list_sparse.inc): the list trace's own argument block for the whole frame -- beginFrame's
// checks with the list's among them, so what the list traces refuse is refused here in the same order, a missing BVH behind the
// arguments -- and the pixel list beside it.  No grid of tiles: "kernel", "soft_split" and the other options choose nothing.
static int launchSparse(rts_ctx* c, const TraceParams& p, bool soft, const uint32_t* d_pixels, const uint32_t* d_n, uint32_t capacity,
                        void* stream) {
    ++c->launches;
    ++c->sparseListTraces;
    const char* name = "";
    const hipError_t e = soft ? rts::launchShadowSoftLightListSparse(p, d_pixels, d_n, capacity, (hipStream_t)stream, &name)
                              : rts::launchShadowLightListSparse(p, d_pixels, d_n, capacity, (hipStream_t)stream, &name);
    c->lastKernel = name;
    return hipStatus(e);
}

int rts_trace_light_list_sparse_device(rts_ctx* c, const rts_constants* k, const rts_light_list* list, const float* d_positions,
                                       const uint8_t* d_lights_map, uint32_t W, uint32_t H, const uint32_t* d_pixels, const uint32_t* d_n,
                                       uint32_t capacity, uint8_t* d_mask, void* stream) {
    TraceParams p; uint32_t rows = 0; int s;
    const bool ok = d_mask && rts::lightListOk(list) && rts::sparseListOk(d_pixels, d_n, capacity);
    if (beginFrame(c, k, d_positions, d_mask, ok, Dispatch::ofRows(W, H, 0, H), p, &rows, &s) != Begin::Go) return s;
    setListHeader(p, k, list->count, d_lights_map);
    for (uint32_t l = 0; l < list->count; ++l) {
        for (int i = 0; i < 3; ++i) p.offsets[l][i] = list->lights[l].xyz[i];
        p.offsets[l][3] = list->lights[l].type == RTS_LIGHT_POINT ? 1.0f : 0.0f;
    }
    return launchSparse(c, p, false, d_pixels, d_n, capacity, stream);
}

int rts_trace_soft_light_list_sparse_device(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* d_positions,
                                            const uint8_t* d_lights_map, uint32_t W, uint32_t H, const uint32_t* d_pixels,
                                            const uint32_t* d_n, uint32_t capacity, uint8_t* d_counts, void* stream) {
    TraceParams p; uint32_t rows = 0; int s;
    const bool ok = d_counts && rts::softListOk(list) && rts::sparseListOk(d_pixels, d_n, capacity);
    if (beginFrame(c, k, d_positions, d_counts, ok, Dispatch::ofRows(W, H, 0, H), p, &rows, &s) != Begin::Go) return s;
    setSoftList(p, k, list, d_lights_map);
    return launchSparse(c, p, true, d_pixels, d_n, capacity, stream);
}

// The host forms: the whole frame travels -- positions, map and the caller's PLANES, which the trace merges into --, the list and its
// length behind them in the distances' staging buffer; the planes come back.  An empty list is RTS_OK with nothing copied.
static int traceSparseStaged(rts_ctx* c, const rts_constants* k, const void* list, bool soft, const float* positions, const uint8_t* lights_map,
                             uint32_t W, uint32_t H, const uint32_t* pixels, uint32_t n, uint8_t* planes) {
    if (!c->d_bvh) return RTS_ERR_NO_BVH;
    if (n == 0) return RTS_OK;
    RTS_HIP(hipSetDevice(c->device));
    const size_t frame = (size_t)W * H, count = soft ? ((const rts_soft_light_list*)list)->count : 1u;
    int s = ensure(&c->d_in, &c->inBytes, frame * 16);
    if (s == RTS_OK) s = ensure(&c->d_out, &c->outBytes, frame * count);
    if (s == RTS_OK && lights_map) s = ensure(&c->d_act, &c->actBytes, frame);
    if (s == RTS_OK) s = ensure(&c->d_dist, &c->distBytes, ((size_t)n + 1u) * 4u);
    if (s != RTS_OK) return s;
    uint32_t* const d_n = (uint32_t*)c->d_dist;
    RTS_HIP(hipMemcpy(c->d_in, positions, frame * 16, hipMemcpyHostToDevice));
    RTS_HIP(hipMemcpy(c->d_out, planes, frame * count, hipMemcpyHostToDevice));
    if (lights_map) RTS_HIP(hipMemcpy(c->d_act, lights_map, frame, hipMemcpyHostToDevice));
    RTS_HIP(hipMemcpy(d_n, &n, 4, hipMemcpyHostToDevice));
    RTS_HIP(hipMemcpy(d_n + 1, pixels, (size_t)n * 4u, hipMemcpyHostToDevice));
    const uint8_t* const d_map = lights_map ? (const uint8_t*)c->d_act : nullptr;
    s = soft ? rts_trace_soft_light_list_sparse_device(c, k, (const rts_soft_light_list*)list, (const float*)c->d_in, d_map, W, H, d_n + 1, d_n,
                                                       n, (uint8_t*)c->d_out, nullptr)
             : rts_trace_light_list_sparse_device(c, k, (const rts_light_list*)list, (const float*)c->d_in, d_map, W, H, d_n + 1, d_n, n,
                                                  (uint8_t*)c->d_out, nullptr);
    if (s != RTS_OK) return s;
    RTS_HIP(hipMemcpy(planes, c->d_out, frame * count, hipMemcpyDeviceToHost));
    return RTS_OK;
}

int rts_trace_light_list_sparse(rts_ctx* c, const rts_constants* k, const rts_light_list* list, const float* positions, const uint8_t* lights_map,
                                uint32_t W, uint32_t H, const uint32_t* pixels, uint32_t n, uint8_t* mask) {
    if (!c || !k || !positions || !mask || !pixels || !stagedListFrameOk(W, H, 0, H) || !rts::lightListOk(list)) return RTS_ERR_INVALID_ARG;
    return traceSparseStaged(c, k, list, false, positions, lights_map, W, H, pixels, n, mask);
}

int rts_trace_soft_light_list_sparse(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* positions,
                                     const uint8_t* lights_map, uint32_t W, uint32_t H, const uint32_t* pixels, uint32_t n, uint8_t* counts) {
    if (!c || !k || !positions || !counts || !pixels || !stagedListFrameOk(W, H, 0, H) || !rts::softListOk(list)) return RTS_ERR_INVALID_ARG;
    return traceSparseStaged(c, k, list, true, positions, lights_map, W, H, pixels, n, counts);
}

// ---- soft light list distance (include/rts.h): a soft light list with the nearest blocker per light beside its count --------------
// One launch of a soft light list distance kernel (rts_soft_light_list_distance.inc): the soft list's argument block, the distance
// planes in the distance's slot, the count planes (optional) in the mask's.
static int traceSoftListDistanceImpl(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* d_positions,
                                     const uint8_t* d_lights_map, const Dispatch& g, float* d_distances, uint8_t* d_counts, void* stream) {
    TraceParams p; uint32_t rows = 0; int s;
    if (beginFrame(c, k, d_positions, d_counts, d_distances && rts::softListOk(list), g, p, &rows, &s) != Begin::Go) return s;
    setSoftList(p, k, list, d_lights_map);
    p.distance = d_distances;
    return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::softListDistanceTraces, rts::launchShadowSoftLightListDistance,
                        stream);
}

int rts_trace_soft_light_list_distance_device(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* d_positions,
                                              const uint8_t* d_lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                              float* d_distances, uint8_t* d_counts, void* stream) {
    return traceSoftListDistanceImpl(c, k, list, d_positions, d_lights_map, Dispatch::ofRows(W, H, row_begin, row_end), d_distances, d_counts,
                                     stream);
}

int rts_trace_soft_light_list_distance_stripes_device(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list,
                                                      const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                                      uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, float* d_distances,
                                                      uint8_t* d_counts, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return traceSoftListDistanceImpl(c, k, list, d_positions, d_lights_map, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), d_distances,
                                     d_counts, stream);
}

// The host form: the soft list's staging, both outputs coming back plane by plane to the caller's planes of H rows.
int rts_trace_soft_light_list_distance(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* positions,
                                       const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                       float* distances, uint8_t* counts) {
    if (!c || !k || !positions || !distances || !stagedListFrameOk(W, H, row_begin, row_end) || !rts::softListOk(list)) return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::SoftListDistance, k, list, positions, lights_map, W, H, row_begin, row_end };
    r.distance = distances; r.mask = counts;
    return traceStagedRows(c, r);
}

// ---- adaptive soft light lists (include/rts.h): a soft light list with a probe count per light, its penumbra alone refined ---------
// One launch of an adaptive soft light list kernel (rts_soft_light_list_adaptive.inc): the soft list's argument block, the probe
// counts in the fourth word of each light's second slot and the refined plane in the generic rays' output slot
// (rts_soft_light_list_adaptive.h).  probes is read here, by value: the caller may change it as soon as the call returns.
// tables (rts_trace_soft_light_list_jittered*): NULL or all zeros is the call without them -- the same launch of the same kernel under
// the same counter; else the table sizes travel in the .w of the shared table's first entries and the JITTER instantiations run.
static int traceSoftListAdaptiveImpl(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* d_positions,
                                     const uint8_t* d_lights_map, const Dispatch& g, uint8_t* d_counts, const uint32_t* probes,
                                     uint8_t* d_refined, void* stream, const uint32_t* tables = nullptr) {
    TraceParams p; uint32_t rows = 0; int s;
    if (beginFrame(c, k, d_positions, d_counts, d_counts && rts::softListTablesOk(list, probes, tables), g, p, &rows, &s) != Begin::Go) return s;
    setSoftList(p, k, list, d_lights_map);
    for (uint32_t l = 0; l < list->count; ++l) rts::setSoftListProbe(p.offsets, l, probes[l]);
    p.out = d_refined;
    if (!rts::softListHasTable(list, tables))
        return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::softListAdaptiveTraces,
                            rts::launchShadowSoftLightListAdaptive, stream);
    for (uint32_t l = 0; l < list->count; ++l) rts::setSoftListTable(p.offsets, l, tables[l]);
    return launchBlocks(c, p, g, blockFamily(c, (uint64_t)g.W * rows), &rts_ctx::softListJitterTraces, rts::launchShadowSoftLightListJittered,
                        stream);
}

int rts_trace_soft_light_list_adaptive_device(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* d_positions,
                                              const uint8_t* d_lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                              uint8_t* d_counts, const uint32_t* probes, uint8_t* d_refined, void* stream) {
    return traceSoftListAdaptiveImpl(c, k, list, d_positions, d_lights_map, Dispatch::ofRows(W, H, row_begin, row_end), d_counts, probes,
                                     d_refined, stream);
}

int rts_trace_soft_light_list_adaptive_stripes_device(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list,
                                                      const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                                      uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_counts,
                                                      const uint32_t* probes, uint8_t* d_refined, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return traceSoftListAdaptiveImpl(c, k, list, d_positions, d_lights_map, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), d_counts,
                                     probes, d_refined, stream);
}

// The host form: the jittered list's without tables.
int rts_trace_soft_light_list_adaptive(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* positions,
                                       const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                       uint8_t* counts, const uint32_t* probes, uint8_t* refined) {
    return rts_trace_soft_light_list_jittered(c, k, list, positions, lights_map, W, H, row_begin, row_end, counts, probes, nullptr, refined);
}

// ---- jittered soft light lists (include/rts.h): the adaptive list with a per-pixel jitter table per light ----------------------------
int rts_trace_soft_light_list_jittered_device(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* d_positions,
                                              const uint8_t* d_lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                              uint8_t* d_counts, const uint32_t* probes, const uint32_t* tables, uint8_t* d_refined,
                                              void* stream) {
    return traceSoftListAdaptiveImpl(c, k, list, d_positions, d_lights_map, Dispatch::ofRows(W, H, row_begin, row_end), d_counts, probes,
                                     d_refined, stream, tables);
}

int rts_trace_soft_light_list_jittered_stripes_device(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list,
                                                      const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                                      uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_counts,
                                                      const uint32_t* probes, const uint32_t* tables, uint8_t* d_refined, void* stream) {
    if (!rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return traceSoftListAdaptiveImpl(c, k, list, d_positions, d_lights_map, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), d_counts,
                                     probes, d_refined, stream, tables);
}

// The host form: the soft list's staging, with the refined rows staged as Staged::Adaptive stages its own; pixelBase, which
// traceStagedRows sets around the device call, makes the hash that of the caller's frame although the rows travel as a frame of their own.
int rts_trace_soft_light_list_jittered(rts_ctx* c, const rts_constants* k, const rts_soft_light_list* list, const float* positions,
                                       const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                       uint8_t* counts, const uint32_t* probes, const uint32_t* tables, uint8_t* refined) {
    if (!c || !k || !positions || !counts || !stagedListFrameOk(W, H, row_begin, row_end) || !rts::softListTablesOk(list, probes, tables))
        return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::SoftListAdaptive, k, list, positions, lights_map, W, H, row_begin, row_end };
    r.mask = counts; r.refined = refined; r.probes = probes; r.tables = tables;
    return traceStagedRows(c, r);
}

int rts_trace_shadow_mask_adaptive(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* positions, const uint8_t* active,
                                   uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, uint32_t probe, uint8_t* mask, uint8_t* refined) {
    if (!c || !k || !positions || !mask || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::adaptiveLightOk(light, probe)) return RTS_ERR_INVALID_ARG;
    StagedRows r{ Staged::Adaptive, k, light, positions, active, W, H, row_begin, row_end };
    r.mask = mask; r.probe = probe; r.refined = refined;
    return traceStagedRows(c, r);
}

// Rays (the caller's arguments are checked): occlusion bytes to `out`, or distances to `out_t` where out is NULL.
static int traceStagedRays(rts_ctx* c, const rts_ray* rays, size_t n, uint8_t* out, float* out_t) {
    if (!c->d_bvh) return RTS_ERR_NO_BVH;
    if (n == 0) return RTS_OK;
    RTS_HIP(hipSetDevice(c->device));
    const size_t outB = out ? n : n * 4;
    int s = ensure(&c->d_in, &c->inBytes, n * sizeof(rts_ray));
    if (s == RTS_OK) s = out ? ensure(&c->d_out, &c->outBytes, outB) : ensure(&c->d_dist, &c->distBytes, outB);
    if (s != RTS_OK) return s;
    RTS_HIP(hipMemcpy(c->d_in, rays, n * sizeof(rts_ray), hipMemcpyHostToDevice));
    s = out ? rts_trace_rays_device(c, (const rts_ray*)c->d_in, n, (uint8_t*)c->d_out, nullptr)
            : rts_trace_rays_distance_device(c, (const rts_ray*)c->d_in, n, (float*)c->d_dist, nullptr);
    if (s != RTS_OK) return s;
    RTS_HIP(hipMemcpy(out ? (void*)out : (void*)out_t, out ? c->d_out : c->d_dist, outB, hipMemcpyDeviceToHost));
    return RTS_OK;
}

int rts_trace_rays(rts_ctx* c, const rts_ray* rays, size_t n, uint8_t* out) {
    if (!c || (n && (!rays || !out))) return RTS_ERR_INVALID_ARG;
    return traceStagedRays(c, rays, n, out, nullptr);
}

int rts_trace_rays_distance(rts_ctx* c, const rts_ray* rays, size_t n, float* out_t) {
    if (!c || (n && (!rays || !out_t))) return RTS_ERR_INVALID_ARG;
    return traceStagedRays(c, rays, n, nullptr, out_t);
}

int rts_device_malloc(rts_ctx* c, void** p, size_t bytes) {
    if (!c || !p) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipMalloc(p, bytes ? bytes : 16));
    return RTS_OK;
}
int rts_device_free(rts_ctx* c, void* p) {
    if (!c) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipFree(p));
    return RTS_OK;
}
int rts_memcpy_h2d(rts_ctx* c, void* d, const void* s, size_t bytes) {
    if (!c || !d || !s) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipMemcpy(d, s, bytes, hipMemcpyHostToDevice));
    return RTS_OK;
}
int rts_memcpy_d2h(rts_ctx* c, void* d, const void* s, size_t bytes) {
    if (!c || !d || !s) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipMemcpy(d, s, bytes, hipMemcpyDeviceToHost));
    return RTS_OK;
}
int rts_device_mem_info(rts_ctx* c, size_t* free_bytes, size_t* total_bytes) {
    if (!c) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    size_t f = 0, t = 0;
    RTS_HIP(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return RTS_OK;
}
int rts_stream_create(rts_ctx* c, void** stream) {
    if (!c || !stream) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    hipStream_t s = nullptr;
    RTS_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void*)s;
    return RTS_OK;
}
int rts_stream_destroy(rts_ctx* c, void* stream) {
    if (!c || !stream) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    for (size_t i = 0; i < c->follow.size(); ++i)
        if (c->follow[i].stream == stream) { freeFollow(c->follow[i]); c->follow.erase(c->follow.begin() + (long)i); break; }
    RTS_HIP(hipStreamDestroy((hipStream_t)stream));
    return RTS_OK;
}
int rts_stream_synchronize(rts_ctx* c, void* stream) {
    if (!c) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipStreamSynchronize((hipStream_t)stream));
    return RTS_OK;
}
int rts_timer_begin(rts_ctx* c, void* stream) {
    if (!c) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipEventRecord(c->ev0, (hipStream_t)stream));
    return RTS_OK;
}
int rts_timer_end(rts_ctx* c, void* stream) {
    if (!c) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipEventRecord(c->ev1, (hipStream_t)stream));
    return RTS_OK;
}
int rts_timer_elapsed_ms(rts_ctx* c, float* ms) {
    if (!c || !ms) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipEventSynchronize(c->ev1));
    RTS_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return RTS_OK;
}
int rts_timer_mark(rts_ctx* c, void* stream, uint32_t slot) {
    if (!c || slot >= 65536u) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    try {
        if (c->marks.size() <= slot) c->marks.resize((size_t)slot + 1, nullptr);
    } catch (...) {
        return RTS_ERR_CAPACITY;
    }
    if (!c->marks[slot]) RTS_HIP(hipEventCreate(&c->marks[slot]));
    RTS_HIP(hipEventRecord(c->marks[slot], (hipStream_t)stream));
    return RTS_OK;
}
int rts_timer_between_ms(rts_ctx* c, uint32_t a, uint32_t b, float* ms) {
    if (!c || !ms || a >= c->marks.size() || b >= c->marks.size() || !c->marks[a] || !c->marks[b]) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipEventSynchronize(c->marks[b]));
    RTS_HIP(hipEventElapsedTime(ms, c->marks[a], c->marks[b]));
    return RTS_OK;
}
const char* rts_ctx_last_kernel_name(rts_ctx* c) { return c ? c->lastKernel : ""; }

int rts_ctx_device_ordinal(rts_ctx* c) { return c ? c->device : 0; }

// used by the GPU builders (rts_lbvh.hip): one buffer the context keeps between builds (a rebuild per frame pays no
// hipMalloc / hipFree: fifty of them cost more than the build).  NULL if it cannot be had; the builders then allocate
// every buffer on their own (DeviceArena::getOwn).
void* rts_ctx_scratch(rts_ctx* c, size_t bytes) {
    if (!c || hipSetDevice(c->device) != hipSuccess) return nullptr;
    if (bytes > c->scratchBytes) {
        // grows by at least half (a scene that grows a little every frame must not pay a hipFree -- a device-wide
        // synchronisation -- per frame); option "builder_scratch" = 0 gives the memory back
        size_t want = bytes > c->scratchBytes + c->scratchBytes / 2 ? bytes : c->scratchBytes + c->scratchBytes / 2;
        if (c->d_scratch) { (void)hipFree(c->d_scratch); c->d_scratch = nullptr; c->scratchBytes = 0; }
        void* p = nullptr;
        if (hipMalloc(&p, want) != hipSuccess) {
            (void)hipGetLastError();
            want = bytes;
            if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        }
        c->d_scratch = p; c->scratchBytes = want;
    }
    return c->d_scratch;
}

// used by the GPU builder (rts_lbvh.hip): the context takes ownership of a packed stream that is already on the device
// (RTS_OK), or refuses it and leaves it with the caller (any other status)
int rts_ctx_adopt_device_bvh(rts_ctx* c, void* d_packed, size_t count, uint32_t P) {
    if (!c || !d_packed || count != (size_t)5 * P - 2 || count * 16 >= 0xFFFFFF00ull) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    const int s = forgetInstalled(c);
    if (s != RTS_OK) return s;
    c->d_bvh = d_packed;
    c->bvhVec4 = count; c->P = P;
    // the same checks as for an uploaded stream, on the device: layout, finiteness (edges of finite vertices can
    // overflow), box order, enclosure.  A refused stream stays the caller's to free.
    return finishInstall(c, false);
}

int rts_ctx_refit_bvh_device(rts_ctx* c, const float* vertices, size_t vertex_floats, uint32_t stride, const uint32_t* indices,
                             uint32_t P, rts_vec4u* out_packed, size_t out_cap, float* refit_ms, float* cost_ratio) {
    if (!c || !vertices || !indices || P == 0 || stride < 3) return RTS_ERR_INVALID_ARG;
    if (!c->d_bvh) return RTS_ERR_NO_BVH;
    if (P != c->P) return RTS_ERR_INVALID_ARG;
    if (out_packed && out_cap < c->bvhVec4) return RTS_ERR_CAPACITY;
    RTS_HIP(hipSetDevice(c->device));
    // geometry on the context's device is used where it lies (its indices are checked by the check kernel); host geometry
    // is staged in a buffer the context keeps
    const int vertsOn = rts::deviceOf(vertices), idxOn = rts::deviceOf(indices);
    if ((vertsOn >= 0 && vertsOn != c->device) || (idxOn >= 0 && idxOn != c->device)) return RTS_ERR_INVALID_ARG;
    if (idxOn < 0)
        for (size_t i = 0; i < (size_t)3 * P; ++i)
            if ((size_t)indices[i] * stride + 3 > vertex_floats) return RTS_ERR_INVALID_ARG;
    rts_ctx::Refit& R = c->refit;
    const uint32_t T = (uint32_t)c->refitTreelet;
    if (!R.valid || (R.topology == RTS_OK && R.treelet != T)) { int s = refitSchedule(c, T); if (s != RTS_OK) return s; }
    if (R.topology != RTS_OK) return R.topology;
    const size_t vBytes = vertsOn >= 0 ? 0 : ((vertex_floats * 4 + 255) & ~(size_t)255), iBytes = idxOn >= 0 ? 0 : (size_t)P * 12;
    if (vBytes + iBytes) { int s = ensure(&R.d_geom, &R.geomCap, vBytes + iBytes); if (s != RTS_OK) return s; }
    const float* d_verts = vertices;
    const uint32_t* d_idx = indices;
    if (vertsOn < 0) { RTS_HIP(hipMemcpy(R.d_geom, vertices, vertex_floats * 4, hipMemcpyHostToDevice)); d_verts = (const float*)R.d_geom; }
    if (idxOn < 0) { d_idx = (const uint32_t*)((char*)R.d_geom + vBytes); RTS_HIP(hipMemcpy((void*)d_idx, indices, iBytes, hipMemcpyHostToDevice)); }

    const uint32_t* sched = (const uint32_t*)R.d_sched;
    rts::RefitLaunch L{};
    L.d_packed = c->d_bvh; L.P = P;
    L.verts = d_verts; L.vertexFloats = vertex_floats; L.stride = stride; L.indices = d_idx;
    L.roots = sched; L.nRoots = R.nRoots; L.treelet = T;
    L.top = sched + R.nRoots; L.levelOff = sched + R.nRoots + R.nTop; L.nLevels = R.nLevels;
    L.d_wide = c->d_wide; L.wideCount = c->wideCount; L.d_tris = c->d_tris; L.d_parents = (const uint32_t*)c->d_parents;
    L.status = R.d_status;
    L.baseline = !R.haveBaseline;
    RTS_HIP(hipEventRecord(R.ev[0], nullptr));
    RTS_HIP(rts::refitLaunch(L));
    if (c->wideCount) refreshSceneBounds(c);              // (the root box may have moved: in stream order, before the read-back below)
    RTS_HIP(hipEventRecord(R.ev[1], nullptr));
    rts::RefitStatus st{};
    RTS_HIP(hipMemcpy(&st, R.d_status, sizeof(st), hipMemcpyDeviceToHost));      // (the one read-back of a steady refit)
    if (L.baseline) { R.baseline = st.baseRootArea > 0 ? st.baseCost / st.baseRootArea : 0.0; R.haveBaseline = true; }
    if (st.err) return (st.err & rts::REFIT_ERR_INDEX) ? RTS_ERR_INVALID_ARG : RTS_ERR_NONFINITE;   // nothing was written

    // the context as rts_ctx_set_bvh of the refitted bytes would leave it -- but the split table, the tile order, the options,
    // the allocation and the cost baseline are kept (they hold node indices and tile coordinates only)
    const bool allowedBefore = wideAllowed(c);
    c->bvhFinite = !(st.valid & 2u);
    c->bvhOrdered = !(st.valid & 4u);
    c->bvhEnclosed = !(st.valid & 8u);
    if (c->wideCount && !wideAllowed(c)) {          // edges overflowed: the copy (refreshed above) goes, and the table that needs it
        c->wideCount = 0; c->wideLevels = 0;
        clearSplits(c);
    } else if (!c->wideCount && !allowedBefore && wideAllowed(c)) {
        int s = deriveWideCopy(c);
        if (s != RTS_OK) return s;
    }
    if (out_packed) RTS_HIP(hipMemcpy(out_packed, c->d_bvh, c->bvhVec4 * 16, hipMemcpyDeviceToHost));
    if (refit_ms) RTS_HIP(hipEventElapsedTime(refit_ms, R.ev[0], R.ev[1]));
    if (cost_ratio) {
        const double now = st.rootArea > 0 ? st.cost / st.rootArea : 0.0;
        *cost_ratio = R.baseline > 0 ? (float)(now / R.baseline) : 1.0f;
    }
    return RTS_OK;
}

// Diagnostics (tests): the private copy of kernel 8 -- wide_nodes x 128 bytes of wide nodes, P x 64 bytes of triangle records,
// (2P - 1) x 4 bytes of parents, in that order; *bytes = its size (0: no copy).  `out` NULL: the size only.
int rtsh_ctx_read_private_copy(rts_ctx* c, void* out, size_t capacity, size_t* bytes) {
    if (!c || !bytes) return RTS_ERR_INVALID_ARG;
    const size_t wideB = (size_t)c->wideCount * 128, trisB = c->wideCount ? (size_t)c->P * 64 : 0,
                 parB = c->wideCount ? ((size_t)2 * c->P - 1) * 4 : 0;
    *bytes = wideB + trisB + parB;
    if (!out || !*bytes) return RTS_OK;
    if (capacity < *bytes) return RTS_ERR_CAPACITY;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipMemcpy(out, c->d_wide, wideB, hipMemcpyDeviceToHost));
    RTS_HIP(hipMemcpy((char*)out + wideB, c->d_tris, trisB, hipMemcpyDeviceToHost));
    RTS_HIP(hipMemcpy((char*)out + wideB + trisB, c->d_parents, parB, hipMemcpyDeviceToHost));
    return RTS_OK;
}

// used by the harness (rts_primary.hip): the device copy of the packed stream, NULL before rts_ctx_set_bvh
const void* rts_ctx_device_bvh(rts_ctx* c) {
    if (!c) return nullptr;
    (void)hipSetDevice(c->device);
    return c->d_bvh;
}

// the installed stream's size in vec4, 0 before rts_ctx_set_bvh (include/rts_scene.h)
size_t rtsh_ctx_bvh_count(rts_ctx* c) { return (c && c->d_bvh) ? c->bvhVec4 : 0; }

// The installed stream into a caller's device buffer (include/rts_scene.h): one asynchronous device-to-device copy.
int rtsh_ctx_snapshot_bvh_device(rts_ctx* c, rts_vec4u* d_out, size_t capacity_vec4, void* stream) {
    if (!c || !d_out) return RTS_ERR_INVALID_ARG;
    if (!c->d_bvh) return RTS_ERR_NO_BVH;
    if (capacity_vec4 < c->bvhVec4) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipMemcpyAsync(d_out, c->d_bvh, c->bvhVec4 * 16, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RTS_OK;
}

// Dispatch order for the next traces whose block count equals `count` (NULL/0 = natural order).  Every tile index
// must appear exactly once (checked).  Speed only: results never depend on it.
int rts_ctx_set_tile_order(rts_ctx* c, const uint32_t* order, size_t count) {
    if (!c) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    if (c->d_tileOrder) { RTS_HIP(hipFree(c->d_tileOrder)); c->d_tileOrder = nullptr; c->tileOrderCount = 0; }
    c->tileOrderSquare = 0; c->tileOrderBlock = 0; c->tileOrderSoftOnly = false; c->tileOrderPlanned = false;
    if (!order || count == 0) return RTS_OK;
    try {
        std::vector<uint8_t> seen(count, 0);
        for (size_t i = 0; i < count; ++i) { if (order[i] >= count || seen[order[i]]) return RTS_ERR_INVALID_ARG; seen[order[i]] = 1; }
    } catch (...) {
        return RTS_ERR_CAPACITY;                   // no exception crosses the C ABI
    }
    RTS_HIP(hipMalloc((void**)&c->d_tileOrder, count * 4));
    RTS_HIP(hipMemcpy(c->d_tileOrder, order, count * 4, hipMemcpyHostToDevice));
    c->tileOrderCount = count;
    return RTS_OK;
}

int rts_ctx_read_wave_stats(rts_ctx* c, uint64_t* out, size_t waves) {
    if (!c || !out || !c->d_waveStats || waves * 32 > c->waveStatsBytes) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipMemcpy(out, c->d_waveStats, waves * 32, hipMemcpyDeviceToHost));
    return RTS_OK;
}

int rts_ctx_read_clock_probe(rts_ctx* c, uint64_t* out, size_t rows) {
    if (!c || !out || !c->d_clockProbe || rows > c->clockProbeRows) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipMemcpy(out, c->d_clockProbe, rows * 32, hipMemcpyDeviceToHost));
    return RTS_OK;
}

// Wave statistics of ONE dispatch (what rts_ctx_read_wave_stats / _realtime return): two launches of the diagnostic
// instantiation without a table, the second one read back.  Used by the planner and, once per tuning call, by the tuner.
static int measureDispatch(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, const Dispatch& g,
                           uint8_t* d_mask, std::vector<uint64_t>& stats, std::vector<uint64_t>& rt, uint32_t perTile = 1) {
    int status = RTS_OK;
    uint64_t* keep = c->d_waveStats; const size_t keepBytes = c->waveStatsBytes;
    c->d_waveStats = nullptr; c->waveStatsBytes = 0;
    const rts::Grid gr = g.grid(8, 8, false);
    const size_t tiles = (size_t)gr.blocksX * gr.blocksY;
    const size_t waves = tiles * perTile;                             // (soft shadows, "soft_split": 4 waves per tile)
    hipError_t e = hipMalloc((void**)&c->d_waveStats, waves * 64);
    if (e == hipSuccess) e = hipMemset(c->d_waveStats, 0, waves * 64);
    if (e == hipSuccess) {
        c->waveStatsBytes = waves * 32;
        const int use = c->useSplits; c->useSplits = 0;
        for (int i = 0; i < 2 && status == RTS_OK; ++i)                   // (the second launch is the one that counts: warm caches)
            status = traceMaskImpl(c, k, light, d_positions, g, d_mask, nullptr);
        c->useSplits = use;
        if (status == RTS_OK) e = hipDeviceSynchronize();
        if (status == RTS_OK && e == hipSuccess && (size_t)c->lastBlocksX * c->lastBlocksY != tiles) status = planRefused("not a dispatch of 8x8 tiles");
        if (status == RTS_OK && e == hipSuccess) {
            try { stats.resize(waves * 4); rt.resize(waves * 4); } catch (...) { status = RTS_ERR_CAPACITY; }   // (no exception crosses the C ABI)
            if (status == RTS_OK) e = hipMemcpy(stats.data(), c->d_waveStats, waves * 32, hipMemcpyDeviceToHost);
            if (status == RTS_OK && e == hipSuccess) e = hipMemcpy(rt.data(), c->d_waveStats + waves * 4, waves * 32, hipMemcpyDeviceToHost);
        }
    }
    if (c->d_waveStats) (void)hipFree(c->d_waveStats);
    c->d_waveStats = keep; c->waveStatsBytes = keepBytes;
    if (status != RTS_OK) return status;
    return hipStatus(e);
}

// ---- the order of a split table's front records: host logic, also reachable without a device (rtsh_split_front_order) --------
struct SplitSel { float us; uint32_t tile; };     // a tile (bx | by << 16) and the life it is sorted by

// half-octaves of life (0.5 / 1 / 2 / 4 bands per octave and the exact order measured: profiles/r04/table_order_bands.log -- 2 and 4 are level)
static int lifeBand(float us) { return (int)std::floor(std::log2(us < 0.25f ? 0.25f : us) * 2.f); }

// life_block B: the front order knows the image only in blocks of B x B tiles -- a tile is as long as the longest tile of its
// block.  Coarser, so a little less gain on the frame it was measured on, but a camera that moves shifts what is long by whole
// tiles and leaves the blocks' order nearly as it was (profiles/r04/table_granularity.log).
static std::unordered_map<uint32_t, float> blockLives(const std::vector<SplitSel>& tiles, uint32_t B) {
    std::unordered_map<uint32_t, float> longest;
    for (const SplitSel& t : tiles) {
        float& m = longest[((t.tile & 0xFFFFu) / B) | (((t.tile >> 16) / B) << 16)];
        if (t.us > m) m = t.us;
    }
    return longest;
}

// front tiles: longest first in half-octaves of life, image order inside one (neighbouring tiles walk the same part of the
// tree: started together they share the scalar cache and the L2 as in the plain launch)
static void sortFront(std::vector<SplitSel>& front) {
    std::sort(front.begin(), front.end(), [](const SplitSel& a, const SplitSel& b) {
        const int ba = lifeBand(a.us), bb = lifeBand(b.us);
        if (ba != bb) return ba > bb;
        const uint32_t ka = ((a.tile >> 16) << 16) | (a.tile & 0xFFFFu), kb = ((b.tile >> 16) << 16) | (b.tile & 0xFFFFu);
        return ka < kb;
    });
}

// xcd_square: the workgroups of a dispatch go round-robin over the 8 XCDs (record i runs on XCD i mod 8, each with an L2 of its
// own), so inside a band record i is taken from the tiles of "its" S x S-tile squares of the image: an XCD's L2 then holds the
// part of the tree its squares see instead of every XCD holding all of it.  (As a static placement of the plain launch this
// lost -- regions differ in cost and unbalance the XCDs, EXPERIMENTS.md --; inside a band of equal measured life every XCD gets
// the same number of equally long tiles.  profiles/r04/xcd_regions_in_table_order.log)  Bands stay where they are, and the
// order inside a bucket stays the image order.
static void dealOverXcds(std::vector<SplitSel>& front, uint32_t firstRecord, uint32_t S) {
    const size_t F = front.size();
    std::vector<SplitSel> out; out.reserve(F);
    for (size_t i = 0; i < F;) {
        size_t j = i; const int b = lifeBand(front[i].us);
        while (j < F && lifeBand(front[j].us) == b) ++j;
        std::vector<SplitSel> bucket[8]; size_t head[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        for (size_t q = i; q < j; ++q) {
            const uint32_t rx = (front[q].tile & 0xFFFFu) / S, ry = (front[q].tile >> 16) / S;
            bucket[(rx + ry * 3u) & 7u].push_back(front[q]);
        }
        for (size_t q = i; q < j; ++q) {
            uint32_t x = (uint32_t)(firstRecord + q) & 7u;              // the XCD this record will run on
            if (head[x] == bucket[x].size()) {                           // none of its own left: from the fullest bucket
                size_t most = 0;
                for (uint32_t y = 0; y < 8; ++y) if (bucket[y].size() - head[y] > most) { most = bucket[y].size() - head[y]; x = y; }
            }
            out.push_back(bucket[x][head[x]++]);
        }
        i = j;
    }
    front.swap(out);
}

// Test hook (tests/test_host_logic.py): the front order of n tiles {life_us[i], tiles[i] = bx | by << 16} as rts_ctx_plan_splits
// would build it with front_share 1 and no splits; order_out[r] = index of the tile that becomes record first_record + r.
extern "C" int rtsh_split_front_order(const float* life_us, const uint32_t* tiles, size_t n, uint32_t first_record, uint32_t xcd_square,
                                      uint32_t life_block, uint32_t* order_out) {
    if ((n && (!life_us || !tiles || !order_out)) || xcd_square > 65535u || life_block > 65535u) return RTS_ERR_INVALID_ARG;
    try {
        std::vector<SplitSel> all(n);
        std::unordered_map<uint32_t, uint32_t> index;
        for (size_t i = 0; i < n; ++i) { all[i] = { life_us[i], tiles[i] }; index[tiles[i]] = (uint32_t)i; }
        if (index.size() != n) return RTS_ERR_INVALID_ARG;                 // a tile twice
        const uint32_t B = life_block > 1 ? life_block : 1u;
        std::vector<SplitSel> front = all;
        if (B > 1) {
            const auto longest = blockLives(all, B);
            for (SplitSel& t : front) t.us = longest.at(((t.tile & 0xFFFFu) / B) | (((t.tile >> 16) / B) << 16));
        }
        sortFront(front);
        if (xcd_square) dealOverXcds(front, first_record, xcd_square);
        for (size_t r = 0; r < n; ++r) order_out[r] = index[front[r].tile];
    } catch (...) { return RTS_ERR_CAPACITY; }
    return RTS_OK;
}

// Follow mode's order on the host (include/rts_scene.h): the checker of the device planner (rts_follow.hip), written plainly --
// a stable sort by band, then the deal of include/rts.h by filling positions.
extern "C" int rtsh_follow_order(const uint32_t* life_ticks, uint32_t blocks_x, uint32_t blocks_y, uint32_t first_record, uint32_t xcd_square,
                                 uint32_t life_block, uint32_t* order_out) {
    const uint64_t n64 = (uint64_t)blocks_x * blocks_y;
    if ((n64 && (!life_ticks || !order_out)) || n64 > (1ull << 31) || xcd_square > 65535u || life_block > 64u) return RTS_ERR_INVALID_ARG;
    try {
        const uint32_t n = (uint32_t)n64, B = life_block > 1 ? life_block : 1u, S = xcd_square;
        std::vector<uint32_t> life(life_ticks, life_ticks + n);
        if (B > 1) {
            const uint32_t gx = (blocks_x + B - 1) / B;
            std::vector<uint32_t> m((size_t)gx * ((blocks_y + B - 1) / B), 0u);
            for (uint32_t t = 0; t < n; ++t) { uint32_t& v = m[(size_t)(t / blocks_x / B) * gx + (t % blocks_x) / B]; if (life[t] > v) v = life[t]; }
            for (uint32_t t = 0; t < n; ++t) life[t] = m[(size_t)(t / blocks_x / B) * gx + (t % blocks_x) / B];
        }
        std::vector<int> band(n);
        for (uint32_t t = 0; t < n; ++t) band[t] = lifeBand((float)life[t] * 0.01f);
        std::vector<uint32_t> sorted(n);
        for (uint32_t t = 0; t < n; ++t) sorted[t] = t;
        std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return band[a] > band[b]; });
        if (!S) { std::copy(sorted.begin(), sorted.end(), order_out); return RTS_OK; }
        for (uint32_t i = 0; i < n;) {
            uint32_t j = i;
            while (j < n && band[sorted[j]] == band[sorted[i]]) ++j;
            const uint32_t R = first_record + i, L = j - i;
            std::vector<uint32_t> bucket[8];
            for (uint32_t q = i; q < j; ++q) {
                const uint32_t t = sorted[q], bx = t % blocks_x, by = t / blocks_x;
                bucket[((bx / S) + (by / S) * 3u) & 7u].push_back(t);
            }
            std::vector<uint32_t> out(L, 0xFFFFFFFFu), left;
            for (uint32_t y = 0; y < 8; ++y) {
                const uint32_t off = (y - R) & 7u, slots = L > off ? (L - 1 - off) / 8 + 1 : 0;
                for (uint32_t k = 0; k < (uint32_t)bucket[y].size(); ++k)
                    if (k < slots) out[off + 8 * k] = bucket[y][k]; else left.push_back(bucket[y][k]);
            }
            size_t next = 0;
            for (uint32_t q = 0; q < L; ++q) if (out[q] == 0xFFFFFFFFu) out[q] = left[next++];
            std::copy(out.begin(), out.end(), order_out + i);
            i = j;
        }
    } catch (...) { return RTS_ERR_CAPACITY; }
    return RTS_OK;
}

// the records of a front map of `tiles` tiles (record i in column i mod 8, row i / 8), read back: order[i] = bx | by << 16
static int readFollowOrder(const uint32_t* d_frontMap, uint32_t frontStride, size_t tiles, uint32_t* order) {
    std::vector<uint32_t> buf((size_t)frontStride * 8);
    RTS_HIP(hipMemcpy(buf.data(), d_frontMap, buf.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tiles; ++i) order[i] = buf[(i & 7u) * frontStride + (i >> 3)];
    return RTS_OK;
}

extern "C" int rts_ctx_read_follow(rts_ctx* c, void* stream, uint32_t* lives, uint32_t* order, size_t tiles) {
    if (!c) return RTS_ERR_INVALID_ARG;
    const rts_ctx::Follow* f = nullptr;
    for (const auto& e : c->follow) if (e.stream == stream) { f = &e; break; }
    if (!f || !f->planned || tiles != (size_t)f->blocksX * f->blocksY) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipStreamSynchronize((hipStream_t)stream));
    try {
        if (lives) {
            std::vector<uint32_t> buf(tiles * 2);
            RTS_HIP(hipMemcpy(buf.data(), f->d_lives, tiles * 8, hipMemcpyDeviceToHost));
            for (size_t t = 0; t < tiles; ++t) lives[t] = buf[2 * t + 1] - buf[2 * t];
        }
        if (order) { const int s = readFollowOrder(f->d_frontMap, f->frontStride, tiles, order); if (s != RTS_OK) return s; }
    } catch (...) { return RTS_ERR_CAPACITY; }
    return RTS_OK;
}

// Harness (include/rts_scene.h): the device planner on the caller's lives, in buffers laid out as a stream's follow state is.
// No stream's state, no counter and no option is touched.
extern "C" int rtsh_follow_plan_device(rts_ctx* c, const uint32_t* life_ticks, const uint32_t* start_ticks, uint32_t blocks_x,
                                       uint32_t blocks_y, uint32_t xcd_square, uint32_t life_block, uint32_t* order_out) {
    const uint64_t n64 = (uint64_t)blocks_x * blocks_y;
    if (!c || (n64 && (!life_ticks || !order_out)) || n64 > (1ull << 31) || xcd_square > 65535u || life_block > 64u) return RTS_ERR_INVALID_ARG;
    if (!n64) return RTS_OK;
    if (blocks_x > 65536u || blocks_y > 65536u) return RTS_ERR_INVALID_ARG;          // (a record holds bx and by in 16 bits each)
    RTS_HIP(hipSetDevice(c->device));
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)nullptr, &capture) != hipSuccess) { (void)hipGetLastError(); return RTS_ERR_INVALID_ARG; }
    if (capture != hipStreamCaptureStatusNone) return RTS_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)n64;
    const FollowLayout lay(n);
    void* d = nullptr;
    int status = RTS_OK;
    try {
        std::vector<uint32_t> stamps((size_t)n * 2);
        for (uint32_t t = 0; t < n; ++t) {
            const uint32_t s = start_ticks ? start_ticks[t] : 0u;
            stamps[2 * (size_t)t] = s; stamps[2 * (size_t)t + 1] = s + life_ticks[t];      // (mod 2^32, as the clock's low word wraps)
        }
        hipError_t e = hipMalloc(&d, lay.bytes());
        if (e == hipSuccess) e = hipMemcpy(d, stamps.data(), (size_t)n * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset((char*)d + lay.mapAt(), 0xFF, lay.mapB);
        if (e == hipSuccess) e = hipMemset((char*)d + lay.scratchAt(), 0, lay.scratchB);
        if (e == hipSuccess) e = rts::launchFollowPlan((const uint32_t*)d, blocks_x, blocks_y, xcd_square, life_block, followBands(),
                                                       (char*)d + lay.scratchAt(), (uint32_t*)((char*)d + lay.mapAt()), lay.stride, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        status = hipStatus(e);
        if (status == RTS_OK) status = readFollowOrder((const uint32_t*)((char*)d + lay.mapAt()), lay.stride, n, order_out);
    } catch (...) { status = RTS_ERR_CAPACITY; }
    if (status != RTS_OK) (void)hipGetLastError();
    if (d) (void)hipFree(d);
    return status;
}

// Plans the split table for ONE dispatch geometry (see include/rts.h).  Synchronous, default stream.
static int planSplitsImpl(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, const Dispatch& g,
                          uint8_t* d_mask, const rts_split_plan* plan, uint32_t* tiles_out, uint32_t* pieces_out) {
    if (tiles_out) *tiles_out = 0;
    if (pieces_out) *pieces_out = 0;
    if (!c || !k || !d_positions || !d_mask || !plan || !(plan->min_life_us > 0.f) || !(plan->piece_us > 0.f) || !(plan->end_after_us >= 0.f) ||
        !(plan->front_life_us >= 0.f) || plan->front_life_us > plan->min_life_us || !(plan->front_share >= 0.f) || plan->front_share > 1.f ||
        plan->xcd_square > 65535u || plan->life_block > 65535u)
        return planRefused("arguments");
    if (light && light->nsamples > 1) return planRefused("more than one light sample");   // (soft shadows are dealt over waves by "soft_split")
    RTS_HIP(hipSetDevice(c->device));
    clearSplits(c);
    if (!c->wideCount) return RTS_OK;                                            // pieces walk the private copy: none, no table
    if (g.nStripes > 1 && !g.rows()) return RTS_OK;                              // a stripe without a band: nothing to launch, no table
    const uint32_t maxPieces = plan->max_pieces < 2 ? 2 : (plan->max_pieces > 64 ? 64 : plan->max_pieces);
    const uint32_t maxTiles = plan->max_tiles ? (plan->max_tiles > 65536u ? 65536u : plan->max_tiles) : 4096u;
    const uint32_t logCap = 16384;
    int status = RTS_OK;
    std::vector<uint64_t> stats, rt;
    size_t waves = 0;
    try {
        if (plan->prev_stats && plan->prev_realtime && plan->prev_waves) {      // the caller's statistics of an earlier frame
            waves = plan->prev_waves;
            stats.assign(plan->prev_stats, plan->prev_stats + waves * 4);
            rt.assign(plan->prev_realtime, plan->prev_realtime + waves * 4);
        } else {                                                                 // one launch of this dispatch with wave statistics
            status = measureDispatch(c, k, light, d_positions, g, d_mask, stats, rt);
            if (status != RTS_OK) return status;
            waves = stats.size() / 4;
        }
        // the tiles whose wave lived longer than min_life_us, longest first
        using Sel = SplitSel;
        std::vector<Sel> sel, front;                                            // to be split / to be started first, unsplit
        const rts::Grid key = g.grid(8, 8, false);                              // the dispatch this table belongs to, in 8 x 8 tiles
        const uint32_t blocksX = key.blocksX, keyBlocksY = key.blocksY;
        uint32_t blocksY = 0;
        uint64_t began = ~0ull;                                                 // the dispatch's first wave
        for (size_t i = 0; i < waves; ++i) if (rt[i * 4 + 1] > rt[i * 4] && rt[i * 4] < began) began = rt[i * 4];
        float frontLife = plan->front_life_us;
        if (plan->front_share >= 1.f) frontLife = 1e-6f;                          // (every tile: the whole dispatch in table order)
        else if (plan->front_share > 0.f) {                                      // the life the longest front_share of the tiles exceed
            std::vector<float> lives;
            lives.reserve(waves);
            for (size_t i = 0; i < waves; ++i) if (rt[i * 4 + 1] > rt[i * 4]) lives.push_back((float)(rt[i * 4 + 1] - rt[i * 4]) * 0.01f);
            if (!lives.empty()) {
                size_t nth = (size_t)((1.0 - (double)plan->front_share) * (double)lives.size());
                if (nth >= lives.size()) nth = lives.size() - 1;
                std::nth_element(lives.begin(), lives.begin() + nth, lives.end());
                if (lives[nth] > frontLife) frontLife = lives[nth];
            }
        }
        const uint32_t B = plan->life_block > 1 ? plan->life_block : 1u;       // (blockLives)
        std::unordered_map<uint32_t, float> blockLife;
        if (B > 1) {
            std::vector<SplitSel> all;
            all.reserve(waves);
            for (size_t i = 0; i < waves; ++i) {
                const uint64_t r0 = rt[i * 4], r1 = rt[i * 4 + 1];
                if (r1 <= r0) continue;
                all.push_back({ (float)(r1 - r0) * 0.01f, (uint32_t)(stats[i * 4 + 3] >> 48) | (((uint32_t)(stats[i * 4 + 3] >> 32) & 0xFFFFu) << 16) });
            }
            blockLife = blockLives(all, B);
        }
        for (size_t i = 0; i < waves; ++i) {
            const uint64_t r0 = rt[i * 4], r1 = rt[i * 4 + 1];
            if (r1 <= r0) continue;
            const float us = (float)(r1 - r0) * 0.01f;
            const uint32_t bx = (uint32_t)(stats[i * 4 + 3] >> 48), by = (uint32_t)(stats[i * 4 + 3] >> 32) & 0xFFFFu;
            if (by >= blocksY) blocksY = by + 1;
            if (bx >= blocksX) continue;
            if (us > plan->min_life_us && (float)(r1 - began) * 0.01f > plan->end_after_us) sel.push_back({ us, bx | (by << 16) });
            else if (frontLife > 0.f && us > frontLife) front.push_back({ B > 1 ? blockLife[(bx / B) | ((by / B) << 16)] : us, bx | (by << 16) });
        }
        if (blocksY > keyBlocksY) return planRefused("statistics of another dispatch");
        {                                                                       // (the caller's statistics may name a tile twice)
            std::vector<uint32_t> named(((size_t)blocksX * keyBlocksY + 31) / 32, 0u);
            for (size_t i = 0; i < waves; ++i) {
                const uint32_t bx = (uint32_t)(stats[i * 4 + 3] >> 48), by = (uint32_t)(stats[i * 4 + 3] >> 32) & 0xFFFFu;
                if (rt[i * 4 + 1] <= rt[i * 4] || bx >= blocksX) continue;
                const size_t id = (size_t)by * blocksX + bx;
                if (named[id >> 5] & (1u << (id & 31u))) return planRefused("statistics that name a tile twice");
                named[id >> 5] |= 1u << (id & 31u);
            }
        }
        if (sel.empty() && front.empty()) return RTS_OK;
        const auto longer = [](const Sel& a, const Sel& b) { return a.us > b.us || (a.us == b.us && a.tile < b.tile); };
        std::sort(sel.begin(), sel.end(), longer);
        sortFront(front);
        if (sel.size() > maxTiles) { front.insert(front.begin(), sel.begin() + maxTiles, sel.end()); sel.resize(maxTiles); }   // (what is not split starts first at least)
        if (front.size() > 262144) front.resize(262144);
        const uint32_t T = (uint32_t)sel.size(), F = (uint32_t)front.size();
        std::vector<rts::SplitCut> cuts(T);
        std::vector<uint32_t> first(T), provisional((size_t)T * 8, 0u);
        uint32_t nPieces = 0;
        for (uint32_t t = 0; t < T; ++t) {
            uint32_t S = (uint32_t)std::ceil(sel[t].us / plan->piece_us);
            S = S < 2 ? 2 : (S > maxPieces ? maxPieces : S);
            cuts[t] = { sel[t].tile, S };
            first[t] = nPieces;
            nPieces += S;
            provisional[(size_t)t * 8 + 0] = sel[t].tile; provisional[(size_t)t * 8 + 1] = 0; provisional[(size_t)t * 8 + 2] = 0xFFFFFFFFu;
            provisional[(size_t)t * 8 + 3] = t | (1u << 24);                       // (dword 4: the walk starts at the root, offset 0)
        }
        if (plan->xcd_square) dealOverXcds(front, nPieces, plan->xcd_square);
        std::vector<uint32_t> bitmap(((size_t)blocksX * keyBlocksY + 31) / 32 + 1, 0u);
        std::vector<uint32_t> frontRecords((size_t)F * 8, 0u);                   // {tile, 0, END, 0 = "front tile", 0...}
        for (uint32_t t = 0; t < T + F; ++t) {
            const uint32_t tile = t < T ? sel[t].tile : front[t - T].tile;
            const uint32_t id = (tile >> 16) * blocksX + (tile & 0xFFFFu);
            bitmap[id >> 5] |= 1u << (id & 31u);
            if (t >= T) { frontRecords[(size_t)(t - T) * 8] = tile; frontRecords[(size_t)(t - T) * 8 + 2] = 0xFFFFFFFFu; }
        }
        // device side: planning walk of the selected tiles (one piece each, everything logged), then the quantiles
        const uint32_t frontStride = (nPieces + F + 7u) / 8u;
        std::vector<uint32_t> frontMap((size_t)frontStride * 8u, 0xFFFFFFFFu);   // (TraceParams::frontMap: record i at (i mod 8) * stride + i / 8)
        for (uint32_t j = 0; j < F; ++j) { const uint32_t id = nPieces + j; frontMap[(size_t)(id & 7u) * frontStride + (id >> 3)] = front[j].tile; }
        void *d_cuts = nullptr, *d_first = nullptr, *d_prov = nullptr, *d_log = nullptr, *d_state = nullptr, *d_pieces = nullptr, *d_map = nullptr;
        void* d_front = nullptr;
        const size_t logBytes = (size_t)T * (logCap + 1) * 4 + 16;
        hipError_t e = hipMalloc(&d_cuts, (size_t)T * 8 + 16);
        if (e == hipSuccess) e = hipMalloc(&d_first, (size_t)T * 4 + 16);
        if (e == hipSuccess) e = hipMalloc(&d_prov, (size_t)T * 32 + 16);
        if (e == hipSuccess) e = hipMalloc(&d_log, logBytes);
        if (e == hipSuccess) e = hipMalloc(&d_state, (size_t)T * 16 + 16);
        if (e == hipSuccess) e = hipMalloc(&d_pieces, (size_t)(nPieces + F) * 32 + 16);
        if (e == hipSuccess && F) e = hipMemcpy((char*)d_pieces + (size_t)nPieces * 32, frontRecords.data(), (size_t)F * 32, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc(&d_map, bitmap.size() * 4);
        if (e == hipSuccess) e = hipMalloc(&d_front, frontMap.size() * 4 + 16);
        if (e == hipSuccess) e = hipMemcpy(d_front, frontMap.data(), frontMap.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_cuts, cuts.data(), (size_t)T * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_first, first.data(), (size_t)T * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_prov, provisional.data(), (size_t)T * 32, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_map, bitmap.data(), bitmap.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(d_log, 0, logBytes);
        if (e == hipSuccess) e = hipMemset(d_state, 0, (size_t)T * 16 + 16);
        if (e == hipSuccess && T) {
            const rts_ctx::Planning pl{ (const uint32_t*)d_prov, T, (T + blocksX - 1) / blocksX, (uint64_t*)d_state, (uint32_t*)d_log, logCap };
            c->planning = &pl;
            status = traceMaskImpl(c, k, light, d_positions, g, d_mask, nullptr);
            c->planning = nullptr;
            if (status == RTS_OK) e = rts::launchSplitQuantiles((const uint32_t*)d_log, logCap, (const rts::SplitCut*)d_cuts, (const uint32_t*)d_first,
                                                                T, (uint32_t*)d_pieces, c->d_wide, nullptr);
            if (status == RTS_OK && e == hipSuccess) e = hipDeviceSynchronize();
        }
        if (d_cuts) (void)hipFree(d_cuts);
        if (d_first) (void)hipFree(d_first);
        if (d_prov) (void)hipFree(d_prov);
        if (d_log) (void)hipFree(d_log);
        if (d_state) (void)hipFree(d_state);
        if (status != RTS_OK || e != hipSuccess) {
            if (d_pieces) (void)hipFree(d_pieces);
            if (d_map) (void)hipFree(d_map);
            if (d_front) (void)hipFree(d_front);
            (void)hipGetLastError();
            return status != RTS_OK ? status : hipStatus(e);
        }
        rts_ctx::Splits& t = c->splits;
        t.valid = true;
        t.geom = g; t.blocksX = blocksX; t.blocksY = keyBlocksY;
        t.d_skipMap = (uint32_t*)d_map; t.d_pieces = (uint32_t*)d_pieces;
        t.d_frontMap = (uint32_t*)d_front; t.frontStride = frontStride;
        t.nPieces = nPieces + F; t.pieceRows = (nPieces + F + blocksX - 1) / blocksX; t.nTiles = T; t.nFront = F;
        size_t covered = 0;                                                    // tiles with a record (the skip bitmap's bits)
        for (uint32_t w : bitmap) covered += (size_t)__builtin_popcount(w);
        t.allTiles = covered == (size_t)blocksX * keyBlocksY;                  // every tile has a record: no tile rows are launched
        t.plan = *plan; t.plan.prev_stats = nullptr; t.plan.prev_realtime = nullptr; t.plan.prev_waves = 0;
        if (tiles_out) *tiles_out = T + F;
        if (pieces_out) *pieces_out = nPieces + F;
    } catch (...) {
        c->planning = nullptr;
        return RTS_ERR_CAPACITY;                       // no exception crosses the C ABI
    }
    return RTS_OK;
}

// rts_ctx_plan_tile_order: the dispatch order of a split table's whole-dispatch form for the launches that cannot carry a table --
// soft shadows (several samples per pixel, 4 waves per tile).  Wave statistics of this dispatch, a tile as long as its longest wave,
// the order of sortFront / dealOverXcds (bands of life, longest first, each band dealt over the XCDs by image squares), installed as
// the context's tile order (rts_ctx_set_tile_order: workgroup i walks tile order[i]).
static int planTileOrderImpl(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, const Dispatch& g,
                             uint8_t* d_mask, uint32_t xcd_square, uint32_t life_block, uint32_t* tiles_out) {
    if (tiles_out) *tiles_out = 0;
    if (!c || !k || !d_positions || !d_mask || xcd_square > 65535u || life_block > 65535u) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    int status = rts_ctx_set_tile_order(c, nullptr, 0);
    if (status != RTS_OK) return status;
    if (c->blockWaves != 1 || c->swizzle) return RTS_OK;                           // (one tile per workgroup only)
    if (g.nStripes > 1 && !g.rows()) return RTS_OK;                              // a stripe without a band: nothing to order
    const uint32_t perTile = (light && light->nsamples > 1 && c->softSplit) ? 4u : 1u;
    std::vector<uint64_t> stats, rt;
    status = measureDispatch(c, k, light, d_positions, g, d_mask, stats, rt, perTile);
    if (status == RTS_ERR_INVALID_ARG) return RTS_OK;                               // not a dispatch of 8x8 tiles: no order
    if (status != RTS_OK) return status;
    if (c->lastVariant != rts::V_PACKET && c->lastVariant != rts::V_WIDE) return RTS_OK;
    try {
        const uint32_t blocksX = c->lastBlocksX, nTiles = c->lastBlocksX * c->lastBlocksY;
        std::vector<float> life(nTiles, 0.f);
        for (size_t i = 0; i < stats.size() / 4; ++i) {
            const uint64_t r0 = rt[i * 4], r1 = rt[i * 4 + 1];
            if (r1 <= r0) continue;
            const uint32_t bx = (uint32_t)(stats[i * 4 + 3] >> 48), by = (uint32_t)(stats[i * 4 + 3] >> 32) & 0xFFFFu;
            if (bx >= blocksX || by >= c->lastBlocksY) continue;
            const float us = (float)(r1 - r0) * 0.01f;
            float& m = life[(size_t)by * blocksX + bx];
            if (us > m) m = us;                                                     // a tile is as long as its longest wave
        }
        std::vector<SplitSel> front(nTiles);
        for (uint32_t t = 0; t < nTiles; ++t) front[t] = { life[t] > 0.f ? life[t] : 0.25f, (t % blocksX) | ((t / blocksX) << 16) };
        if (life_block > 1) {
            const auto longest = blockLives(front, life_block);
            for (SplitSel& f : front) f.us = longest.at(((f.tile & 0xFFFFu) / life_block) | (((f.tile >> 16) / life_block) << 16));
        }
        sortFront(front);
        if (xcd_square) dealOverXcds(front, 0u, xcd_square);
        std::vector<uint32_t> order(nTiles);
        for (uint32_t i = 0; i < nTiles; ++i) order[i] = (front[i].tile >> 16) * blocksX + (front[i].tile & 0xFFFFu);
        status = rts_ctx_set_tile_order(c, order.data(), order.size());
        if (status != RTS_OK) return status;
        c->tileOrderSquare = xcd_square; c->tileOrderBlock = life_block;
        c->tileOrderSoftOnly = light && light->nsamples > 1;
        c->tileOrderPlanned = true;
        if (tiles_out) *tiles_out = nTiles;
    } catch (...) { return RTS_ERR_CAPACITY; }
    return RTS_OK;
}

// Picks the kernel for THIS dispatch by timing the candidates on it (what a renderer does once per scene and resolution):
// the lane-per-ray walk with work sharing, the packet kernel, the wide packet kernel (when the stream has a private copy).
// Then, for a packet kernel, two launch parameters that are worth 2-6 % on some frames and cost as much on others
// (profiles/r03/autotune_stage2_sweep.log): the dissolve threshold ("packet_share" 4 or 6) and the order in which the tile
// rows are started ("row_order" top-down or bottom-up: the rows started last are the kernel's tail).  Third stage (round 4):
// a split table for the tiles measured to be long (rts_ctx_plan_splits), kept when it gains 1.5 % -- frames whose time is a
// few long waves (atrium 1080p: -30 %), and the stripes of a multi-GPU frame; a frame that is throughput-bound to its end
// (city, courtyard at 4K) keeps the plain launch.  Leaves the options and the table of the winners installed.  Results
// never depend on any of them.
static int autotuneImpl(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, const Dispatch& g,
                        uint8_t* d_mask, int* chosen, float* ms_out) {
    if (!c || !k || !d_positions || !d_mask) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    clearSplits(c);
    int status = RTS_OK;
    if (g.nStripes > 1 && !g.rows()) {                                          // a stripe without a band: nothing to time, nothing tuned
        if (c->tileOrderPlanned) status = rts_ctx_set_tile_order(c, nullptr, 0);
        if (chosen) *chosen = c->variant;
        if (ms_out) *ms_out = 0.f;
        return status;
    }
    int reps = 5;                              // (nine for the tables of a dispatch below 0.1 ms: its launches are cheap, its noise is not)
    auto median5 = [&](float* out) {          // two untimed launches, then the median of five (or nine)
        float times[9];
        for (int i = -2; i < reps; ++i) {
            hipError_t e = hipEventRecord(c->ev0, nullptr);
            if (e != hipSuccess) { status = hipStatus(e); return false; }
            status = traceMaskImpl(c, k, light, d_positions, g, d_mask, nullptr);
            if (status != RTS_OK) return false;
            float ms = 0;
            e = hipEventRecord(c->ev1, nullptr);
            if (e == hipSuccess) e = hipEventSynchronize(c->ev1);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0, c->ev1);
            if (e != hipSuccess) { status = hipStatus(e); return false; }
            if (i >= 0) times[i] = ms;
        }
        for (int i = 1; i < reps; ++i) for (int j = i; j > 0 && times[j] < times[j - 1]; --j) { float t = times[j]; times[j] = times[j - 1]; times[j - 1] = t; }
        *out = times[reps / 2];
        return true;
    };
    // (the wide kernel first, and a later candidate must beat the best by 2 %: at equal frame time the wide kernel's waves
    //  are shorter, which is what a striped multi-GPU frame needs -- tools/stripe_scaling.py)
    const int candidates[3] = { rts::V_WIDE, rts::V_PACKET, rts::V_SHARE };
    const int before = c->variant, shareBefore = c->packetShare, orderBefore = c->rowOrder;
    auto giveUp = [&]() {
        c->variant = before; c->packetShare = shareBefore; c->rowOrder = orderBefore; clearSplits(c);
        if (c->tileOrderPlanned) (void)rts_ctx_set_tile_order(c, nullptr, 0);
        return status;
    };
    if (c->tileOrderPlanned) {                                // (an order an earlier tuning planned: the candidates meet the plain dispatch)
        status = rts_ctx_set_tile_order(c, nullptr, 0);
        if (status != RTS_OK) return status;
    }
    uint64_t pixels = (uint64_t)g.W * (g.rowEnd - g.rowBegin);
    if (g.nStripes > 1) pixels /= g.nStripes;
    int best = before;
    float bestMs = 1e30f;
    for (int v : candidates) {
        if (v == rts::V_WIDE && !c->wideCount) continue;
        if (v == rts::V_SHARE && pixels > (1u << 20)) continue;                  // (never close on a big frame: skip its long launches)
        c->variant = v;
        float ms;
        if (!median5(&ms)) return giveUp();
        if (ms < bestMs * 0.98f) { bestMs = ms; best = v; }
    }
    c->variant = best;
    if (best == rts::V_WIDE || best == rts::V_PACKET) {
        // second stage, one parameter at a time; a change must gain 1.5 % to be kept (launch-to-launch noise is below 1 %)
        float ms;
        if (c->packetShare == 4) {
            c->packetShare = 6;
            if (!median5(&ms)) return giveUp();
            if (ms < bestMs * 0.985f) bestMs = ms; else c->packetShare = shareBefore;
        }
        if (c->rowOrder == 0 && !c->d_tileOrder && !c->swizzle && g.nStripes <= 1) {
            c->rowOrder = 1;
            if (!median5(&ms)) return giveUp();
            if (ms < bestMs * 0.985f) bestMs = ms; else c->rowOrder = orderBefore;
        }
        // third stage: split tables.  Tiles that lived longer than a share of the dispatch and ended in its later part.
        if (c->wideCount && c->blockWaves == 1 && !c->wideLane && (!light || light->nsamples <= 1) && c->useSplits) {
            // Seven tables from ONE set of wave statistics (profiles/r04/front_tiles_sweep.log, whole_dispatch_order.log): the tiles
            // that lived longer than max(T/4, 20 us) and ended in the second half split into pieces of max(T/10, 8 us) -- or none
            // split --, with the longest 3 % / third / ALL of the tiles started first (all: the whole dispatch in table order, no
            // tile rows at all); and the splits alone with a lower threshold.  A frame whose time is a few long waves wants the
            // first kind (atrium), a throughput-bound one a short front list (city) or the table order (courtyard), the stripe of
            // a multi-GPU frame both.
            const float T = bestMs * 1000.f;                                      // us
            if (bestMs < 0.1f) { reps = 9; if (!median5(&bestMs)) return giveUp(); }   // (the plain launch once more, by the same measure)
            const int trials = 7;
            int kept = -1, installed = -1;
            rts_split_plan plan{};
            std::vector<uint64_t> tuneStats, tuneRt;
            status = measureDispatch(c, k, light, d_positions, g, d_mask, tuneStats, tuneRt);
            if (status == RTS_ERR_INVALID_ARG) { status = RTS_OK; goto tuned; }    // (not a dispatch of 8x8 tiles: no table)
            if (status != RTS_OK) return giveUp();
            {
            auto fill = [&](int i) {
                plan = rts_split_plan{};
                plan.max_pieces = 8;
                plan.max_tiles = 8192;
                plan.prev_stats = tuneStats.data(); plan.prev_realtime = tuneRt.data(); plan.prev_waves = tuneStats.size() / 4;
                static const float share[3] = { 0.03f, 1.f / 3.f, 1.f };
                if (i < 6) {
                    plan.front_share = share[i % 3];
                    if (i % 3 == 2) plan.xcd_square = 32;                       // (the whole dispatch in table order: XCD-local too)
                    if (c->tuneForMotion) plan.life_block = 16;                  // (sorted by 128 x 128-pixel blocks: see rts_split_plan)
                    if (i < 3) {
                        plan.min_life_us = 0.25f * T < 20.f ? 20.f : 0.25f * T; plan.end_after_us = 0.5f * T;
                        plan.piece_us = 0.1f * T < 8.f ? 8.f : 0.1f * T;
                    } else { plan.min_life_us = 1e9f; plan.piece_us = 1e9f; }
                } else {
                    plan.min_life_us = 0.15f * T < 8.f ? 8.f : 0.15f * T; plan.end_after_us = 0.5f * T; plan.piece_us = plan.min_life_us * 0.5f;
                }
            };
            // Every table is timed against the PLAIN launch measured right beside it (planning leaves the device idle for
            // milliseconds and its clocks drop: a figure from before the planning is not comparable; 20 ms of the launch itself
            // first).  The table with the best ratio is the candidate; it must gain 1 %.
            float bestRatio = 1e30f, tableMs = bestMs;
            for (int i = 0; i < trials; ++i) {
                // (a camera path: pieces belong to the very tiles of one camera, and a front list that is a share of the tiles is a set
                //  of tiles too -- only the whole dispatch in block order was measured to keep: profiles/r04/table_granularity.log)
                if (c->tuneForMotion && i != 5) continue;
                fill(i);
                uint32_t tiles = 0;
                status = planSplitsImpl(c, k, light, d_positions, g, d_mask, &plan, &tiles, nullptr);
                if (status != RTS_OK) return giveUp();
                installed = i;
                if (!tiles) continue;
                for (const auto t0 = std::chrono::steady_clock::now(); status == RTS_OK && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(20);) {
                    for (int w = 0; w < 8 && status == RTS_OK; ++w)
                        status = traceMaskImpl(c, k, light, d_positions, g, d_mask, nullptr);
                    if (hipStreamSynchronize(nullptr) != hipSuccess) status = RTS_ERR_HIP;
                }
                if (status != RTS_OK) return giveUp();
                float plainMs;
                if (!median5(&ms)) return giveUp();
                c->useSplits = 0;
                const bool ok = median5(&plainMs);
                c->useSplits = 1;
                if (!ok) return giveUp();
                if (getenv("RTS_TUNE_LOG"))           // diagnostics: what the tuner saw
                    fprintf(stderr, "rts tune: table %d (life > %.1f us, front share %.2f): %u split + %u front tiles, %.4f ms against %.4f plain beside it\n", i,
                            plan.min_life_us, plan.front_share, c->splits.nTiles, c->splits.nFront, ms, plainMs);
                if (ms / plainMs < bestRatio) { bestRatio = ms / plainMs; tableMs = ms; kept = i; }
            }
            if (kept >= 0 && bestRatio < 0.99f) bestMs = tableMs; else kept = -1;    // (paired figures: 1 % is outside their noise)
            if (kept < 0) clearSplits(c);
            else if (kept != installed) {
                fill(kept);
                status = planSplitsImpl(c, k, light, d_positions, g, d_mask, &plan, nullptr, nullptr);
                if (status != RTS_OK) return giveUp();
            }
            }
        } else if (light && light->nsamples > 1 && c->blockWaves == 1 && !c->swizzle && c->useTileOrder) {
            // ... for soft shadows (no table: 4 waves per tile) the whole-dispatch order as a tile order: bands of measured life,
            // longest first, dealt over the XCDs by image squares (city x 16 samples - 5.6 %, courtyard - 6.3 %:
            // profiles/r04/soft_tile_order.log); sorted by blocks when the camera will move.  Timed beside the plain launch.
            // Both packet families are tried in their own order (the first stage chose between them in the plain order, where they
            // are within 2 % on these frames; in order the stackless packet gains more: city x 16 samples 2.25 against 2.39 ms).
            auto ordered = [&](int variant, float* ms, uint32_t* tiles) {
                c->variant = variant;
                status = planTileOrderImpl(c, k, light, d_positions, g, d_mask, 32u,
                                           c->tuneForMotion ? 16u : 0u, tiles);
                if (status != RTS_OK) return false;
                if (!*tiles) return true;
                for (const auto t0 = std::chrono::steady_clock::now(); status == RTS_OK && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(20);) {
                    status = traceMaskImpl(c, k, light, d_positions, g, d_mask, nullptr);
                    if (hipStreamSynchronize(nullptr) != hipSuccess) status = RTS_ERR_HIP;
                }
                return status == RTS_OK && median5(ms);
            };
            const int other = best == rts::V_WIDE ? rts::V_PACKET : (c->wideCount ? rts::V_WIDE : -1);
            uint32_t tiles = 0, tilesOther = 0;
            float ms = 0.f, msOther = 1e30f;
            if (other >= 0) { if (!ordered(other, &msOther, &tilesOther)) return giveUp(); if (!tilesOther) msOther = 1e30f; }
            if (!ordered(best, &ms, &tiles)) return giveUp();                     // (last: its order is the one left installed)
            if (tiles && msOther < ms * 0.98f) {                                   // the other family, in its order, is ahead: take it
                best = other;
                if (!ordered(best, &ms, &tiles)) return giveUp();
            }
            c->variant = best;
            if (tiles) {
                float plainMs;
                c->useTileOrder = 0;
                const bool ok = median5(&plainMs);
                c->useTileOrder = 1;
                if (!ok) return giveUp();
                if (getenv("RTS_TUNE_LOG"))
                    fprintf(stderr, "rts tune: tile order (%u tiles, kernel %d): %.4f ms against %.4f plain beside it (the other family in its order: %.4f)\n",
                            tiles, best, ms, plainMs, msOther);
                if (ms / plainMs < 0.99f) bestMs = ms;
                else { status = rts_ctx_set_tile_order(c, nullptr, 0); if (status != RTS_OK) return giveUp(); }
            }
        }
    }
tuned:
    if (chosen) *chosen = best;
    if (ms_out) *ms_out = bestMs;
    return RTS_OK;
}

int rts_ctx_plan_tile_order(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, uint32_t W, uint32_t H,
                            uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_mask, uint32_t xcd_square, uint32_t life_block,
                            uint32_t* tiles) {
    if (W == 0 || H == 0 || n_stripes == 0 || stripe >= n_stripes || (n_stripes > 1 && (band_rows == 0 || band_rows % 8 != 0))) return RTS_ERR_INVALID_ARG;
    return planTileOrderImpl(c, k, light, d_positions, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), d_mask, xcd_square, life_block, tiles);
}

int rts_ctx_autotune(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, uint32_t W,
                     uint32_t H, uint8_t* d_mask, int* chosen, float* ms_out) {
    if (W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    return autotuneImpl(c, k, light, d_positions, Dispatch::ofRows(W, H, 0, H), d_mask, chosen, ms_out);
}

int rts_ctx_autotune_stripes(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, uint32_t W, uint32_t H,
                             uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_mask, int* chosen, float* ms_out) {
    if (W == 0 || H == 0 || !rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return autotuneImpl(c, k, light, d_positions, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), d_mask, chosen, ms_out);
}

int rts_ctx_get_split_plan(rts_ctx* c, rts_split_plan* out) {
    if (!c || !out || !c->splits.valid) return RTS_ERR_INVALID_ARG;
    *out = c->splits.plan;
    return RTS_OK;
}

int rts_ctx_plan_splits(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, uint32_t W, uint32_t H,
                        uint32_t row_begin, uint32_t row_end, uint8_t* d_mask, const rts_split_plan* plan, uint32_t* tiles, uint32_t* pieces) {
    if (W == 0 || H == 0 || row_begin >= row_end || row_end > H) return RTS_ERR_INVALID_ARG;
    return planSplitsImpl(c, k, light, d_positions, Dispatch::ofRows(W, H, row_begin, row_end), d_mask, plan, tiles, pieces);
}

int rts_ctx_plan_splits_stripes(rts_ctx* c, const rts_constants* k, const rts_light* light, const float* d_positions, uint32_t W, uint32_t H,
                                uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_mask, const rts_split_plan* plan,
                                uint32_t* tiles, uint32_t* pieces) {
    if (W == 0 || H == 0 || !rts::stripeArgsOk(band_rows, n_stripes, stripe)) return RTS_ERR_INVALID_ARG;
    return planSplitsImpl(c, k, light, d_positions, Dispatch::ofStripe(W, H, band_rows, n_stripes, stripe), d_mask, plan, tiles, pieces);
}

// diagnostics: per piece of the installed table {tile x | y << 16, first node, end node, pieces of its tile} and the 100 MHz
// stamps of its start and end in the last launch that used the table (option "piece_stats")
int rts_ctx_read_piece_stats(rts_ctx* c, uint32_t* records, uint64_t* clocks, size_t pieces) {
    if (!c || !c->splits.valid || pieces > c->splits.nPieces || (clocks && (!c->d_pieceClock || pieces > c->pieceClockCount))) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    if (records) RTS_HIP(hipMemcpy(records, c->splits.d_pieces, pieces * 32, hipMemcpyDeviceToHost));
    if (clocks) RTS_HIP(hipMemcpy(clocks, c->d_pieceClock, pieces * 64, hipMemcpyDeviceToHost));
    return RTS_OK;
}

// The kernels replace 1.0f / x by v_rcp_f32 + one Newton step where 2^-100 <= |x| <= 2^100 (rts_kernels.hip: rcpFast); that this
// is the IEEE quotient for EVERY such bit pattern is checked here, on the device it runs on: out[0] = patterns in the range,
// out[1] = patterns whose result differs from the division (must be 0), out[2] = one of them.
int rts_selftest_reciprocal(rts_ctx* c, uint64_t out[3]) {
    if (!c || !out) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    unsigned long long* d = nullptr;
    RTS_HIP(hipMalloc((void**)&d, 32));
    hipError_t e = hipMemset(d, 0, 32);
    if (e == hipSuccess) e = rts::launchReciprocalSelfTest(d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d, 24, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return hipStatus(e);
}

int rts_ctx_clear_splits(rts_ctx* c) {
    if (!c) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    clearSplits(c);
    return RTS_OK;
}

int rts_ctx_read_wave_realtime(rts_ctx* c, uint64_t* out, size_t waves) {
    if (!c || !out || !c->d_waveStats || waves * 32 > c->waveStatsBytes) return RTS_ERR_INVALID_ARG;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(hipMemcpy(out, c->d_waveStats + c->waveStatsBytes / 8, waves * 32, hipMemcpyDeviceToHost));
    return RTS_OK;
}

} // extern "C"
