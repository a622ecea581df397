// Internal interface between the C-ABI layer (rts_api.cpp) and the HIP kernels (rts_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rts_alltable.h"

namespace rts {

enum Variant {
    V_STRAIGHT = 0,    // loop as the shader spells it
    V_WHILEWHILE = 1,  // inner-node descent loop + batched leaf test
    V_POSTPONE = 2,    // leaves parked in registers, tested wave-wide
    V_PACKET = 3,      // wave (8x8 px) walks the union of its rays' paths; nodes via scalar loads
    V_PACKET2 = 4,     // same, 2 rays per lane (16x8 px per wave)
    V_PACKET4 = 5,     // same, 4 rays per lane (16x16 px per wave)
    V_PACKET_PF = 6,   // V_PACKET with the sequential successor node prefetched into a second SGPR set
    V_SHARE = 7,       // lane-per-ray with work sharing inside the wave (idle lanes take half of a busy ray's range)
    V_WIDE = 8,        // packet over the private WIDE nodes (rts_wide.hip): four grandchild boxes per dependent fetch,
                       // cheap conservative slab test, triangle hits confirmed by the exact test of the leaf's parent box
    V_WIDE_C = 9,      // V_WIDE with the loop compiled from C++ instead of hand-written (reference form of the same algorithm)
    V_COUNT,
    V_AUTO = -1        // packet for big launches, V_SHARE for small ones and for generic rays
};

// Kernel argument block (passed by value; lives in the kernarg segment, read with scalar loads).
struct TraceParams {
    // ---- what a tile wave needs before it can ask for its G-buffer texel: 64 bytes, one batch of scalar loads -------------
    const float4* positions;  // W x H RGBA32F, camera-relative (device)
    uint8_t* mask;            // W x H bytes (device)
    uint32_t W, H, rowBegin, rowEnd;
    uint32_t pieceRows;       // rows of the 2-D grid that hold the pieces of split tiles (they come first); 0 without a table
    uint32_t blocksX, blocksY;
    uint32_t rowOrder;        // dispatch order of the tile rows (speed only): 0 first to last, 1 last to first, 2 middle row outwards
    const uint32_t* skipMap;  // split tiles: bit (by * blocksX + bx) set: the tile's own wave has nothing to do (NULL: no split table)
    uint32_t bandShift;       // interleaved stripes: log2(bandRows / 8) when that is a power of two, else 0xFFFFFFFF
    uint32_t stripe;
    // ------------------------------------------------------------------------------------------------------------------
    uint32_t bandRows, nStripes;           // interleaved stripes (nStripes <= 1: plain rowBegin..rowEnd)
    const void* bvh;          // packed vec4 stream, SURVEY.md Appendix A (device)
    uint32_t bvhBytes;
    uint32_t bvhFinite;       // every float of the stream is finite -> FAST slab test is legal
    uint32_t bvhOrdered;      // ... and every inner node has bboxMin <= bboxMax -> ordered slab test is legal
    uint32_t nBlocks, gridBlocks, swizzle;
    uint32_t grid2d;            // 1: launched as a blocksX x blocksY grid in natural order (no swizzle, no order table)
    float cam[3];
    uint32_t lightType, nsamples;
    uint32_t softSplit;         // soft shadows: 4 waves per tile, samples dealt over them (option "soft_split")
    uint32_t pixelBase;         // index in the caller's frame of this dispatch's pixel 0 (host-pointer stripes travel as frames of their own)
    uint32_t lightTable;        // per-pixel jitter: entries of offsets[] a pixel starts in (0 = off); rts_light.table
    float light[3];
    // generic rays
    union {
        const void* rays;     // rts_ray[n] (device)
        // active traces (rts_trace_shadow_mask_active*), mask launches only: W x H bytes, non-zero = this pixel sends its ray; non-NULL
        // only in the launches of the shadowMaskActive* kernels.  (It shares the slot of the generic rays' input, which no mask
        // kernel reads: the argument block keeps its size, and every other kernel its code.)
        const uint8_t* activeMap;
    };
    union {
        uint8_t* out;
        // follow mode (rts_follow.hip), mask launches only: {s_memrealtime low 32 bits at the wave's start, at its end} per tile of
        // the dispatch, row-major; non-NULL only in the launches of shadowMaskFollowKernel.  (It shares the slot of the generic rays'
        // output, which no mask kernel reads: the argument block keeps its size, and every other kernel its code.)
        uint32_t* followLives;
        // distance traces (rts_trace_shadow_distance*, rts_trace_rays_distance*): W x H floats beside the (then optional) mask, or one
        // float per generic ray; non-NULL only in the launches of the distance kernels (rts_distance.inc).  The same slot again.
        float* distance;
    };
    uint64_t nrays;
    const uint32_t* tileOrder; // optional: block i works on tile tileOrder[i] (device array of nBlocks entries)
    uint64_t* waveStats;      // diagnostics (tools/wave_stats.py): 4 u64 per wave, or NULL
    uint64_t* waveRealtime;   // diagnostics: 4 u64 per wave {s_memrealtime at start, at end (100 MHz), clocks to first ray, XCC id}
    uint64_t* clockProbe;     // diagnostics that the EVERYDAY instantiation carries too: the first wave of every tile row
                              // stamps {shader clock, 100 MHz clock} at its start and end (4 u64 per row), or NULL
    uint32_t packetBudget;    // side-steps between two coherence checks of a packet (dissolve rule)
    uint32_t packetShare;     // dissolve when rays served per step < packetShare/16 of the rays alive
    const void* wide;         // private wide nodes (128 B each, root first) or NULL: V_WIDE falls back to V_PACKET
    const void* tris;         // private triangle records (48 B each, leaves in stream order)
    const uint32_t* parents;  // private: parent node of every node of the stream
    uint32_t primCount;
    uint32_t wideBytes;       // size of the private copy (wide nodes + triangle records, one allocation)
    uint32_t trisOffset;      // byte offset of the triangle records in it (tris == wide + trisOffset)
    uint32_t wideLane;        // dissolved wide packets continue lane per ray over the WIDE nodes (0: over the stream, stackless)
    // split tiles (rts_ctx_plan_splits): tiles measured to be long are walked by several one-wave workgroups ("pieces"), each
    // over one index range of the node stream; the pieces occupy the first pieceRows rows of the 2-D grid (dispatched first)
    const uint32_t* pieces;   // 8 dwords per piece: {bx | by << 16, first node, end node, state slot | pieces of the tile << 24,
                              //  byte offset of the wide node the piece starts at, 0, 0, 0}
    uint64_t* tileState;      // 2 u64 per split tile {lanes found occluded by any piece, pieces done}; zero between launches
    union {
        uint32_t* pieceLog;   // split planning only: per piece 1 + pieceLogCap dwords {count, node indices visited ...}
        // the ALLTABLE launch only (allTableLaunch below): the context's block of per-scene constants, 9 dwords of device memory
        // {rootLo.xyz, bound.x, rootHi.xyz, bound.y, bound.z} -- the root box of the installed stream and wideSetupBound of it,
        // written by sceneBoundsKernel in stream order whenever the stream's boxes change (install, adopt, refit).  In memory and
        // not by value: a captured trace replayed after an in-place refit must see the refitted root, as it does through p.bvh.
        // (It shares the slot of the planning log, which only the piece path of a planning launch reads: the argument block
        // keeps its size, and every other kernel its code.)
        const uint32_t* sceneBounds;
    };
    uint64_t* pieceClock;     // diagnostics ("piece_stats"): per piece {100 MHz clock at its start, at its end}, or NULL
    uint32_t nPieces, pieceLogCap;
    uint32_t allInTable;      // every tile of the dispatch has a record: the grid is the records alone (no tile rows at all)
    uint32_t hasPieces;       // the table has split tiles (0: front tiles only -- the instantiation without the piece path)
    uint32_t frontStride;     // ... records per XCD in frontMap
    // One dword per record, what a record's wave reads first: bx | by << 16 of a FRONT tile, 0xFFFFFFFF for a piece (which then
    // reads its 8 dwords).  Record i lives at (i mod 8) * frontStride + i / 8: the dispatcher deals workgroups round-robin over
    // the 8 XCDs, so every XCD reads ONE contiguous run of dwords -- 32 records per 128-byte line of its own L2 -- instead of
    // every eighth 32-byte record of an array all eight L2s have to pull in (a dependent miss in front of the texel request:
    // a table in plain image order was 2-5 % slower than no table).  NULL (planning launches): every record is a piece.
    const uint32_t* frontMap;
    float offsets[64][4];
};

struct SplitCut {             // planning: one selected tile
    uint32_t tile;            // bx | by << 16 (tile coordinates of the dispatch)
    uint32_t pieces;          // S
};

// Kernel 8's launch of `p` runs the ALLTABLE instantiation (rts_alltable.h: the rule itself, checked on the CPU).
inline bool allTableLaunch(const TraceParams& p, int wavesPerBlock) {
    AllTableFacts f{};
    f.wavesPerBlock = (uint32_t)wavesPerBlock; f.nsamples = p.nsamples; f.wideLane = p.wideLane != 0; f.follow = p.followLives != nullptr;
    f.table = p.pieces != nullptr; f.hasPieces = p.hasPieces != 0; f.allInTable = p.allInTable != 0; f.frontMap = p.frontMap != nullptr;
    f.stripes = p.nStripes > 1; f.waveStats = p.waveStats != nullptr; f.sceneBounds = p.sceneBounds != nullptr;
    f.nPieces = p.nPieces; f.blocksX = p.blocksX; f.pieceRows = p.pieceRows;
    return allTableRule(f);
}
// the context's per-scene constants (TraceParams::sceneBounds, SCENE_BOUNDS_DWORDS dwords) from node 0 of the stream: one thread
hipError_t launchSceneBounds(const void* d_packed, uint32_t* d_sceneBounds, hipStream_t stream);

const char* kernelName(int variant, bool mask);
void tileShape(int variant, int wavesPerBlock, uint32_t* blockW, uint32_t* blockH);   // pixels covered by one block
hipError_t launchShadowMask(int variant, int wavesPerBlock, const TraceParams& p, hipStream_t stream, uint32_t ldsPad = 0);
// active traces: the kernel family of `variant` with p.activeMap as the mark (V_SHARE: lane per ray with work sharing, V_PACKET: the
// stackless packet, V_WIDE: the wide packet); one tile per workgroup.  *name: the kernel's stable name.
hipError_t launchShadowMaskActive(int variant, const TraceParams& p, hipStream_t stream, const char** name);
hipError_t launchTraceRays(int variant, const TraceParams& p, hipStream_t stream);
// distance traces (rts_distance.inc): V_SHARE = lane per ray over 16 x 16 blocks, V_PACKET = the stackless packet over 8 x 8 tiles;
// p.distance is written, p.mask and p.activeMap may be NULL.  *name: the kernel's stable name.
hipError_t launchShadowDistance(int variant, const TraceParams& p, hipStream_t stream, const char** name);
hipError_t launchTraceRaysDistance(const TraceParams& p, hipStream_t stream);   // p.rays -> p.distance, lane per ray
// follow mode (rts_follow.hip): the per-band lower bounds of the tick counts (band b = lifeBand of the host, bands longest first)
constexpr uint32_t FOLLOW_BANDS = 55;          // lifeBand -4 (0.25 us and less) .. 50 (2^32 - 1 ticks, 42.9 s, is in band 50)
constexpr int FOLLOW_BAND_LOW = -4;
struct FollowBands { uint32_t minTicks[FOLLOW_BANDS]; };   // minTicks[i]: smallest tick count of band FOLLOW_BAND_LOW + i (ascending)
size_t followScratchBytes(uint32_t tiles);
// the order the next launch of the dispatch runs: lives (2 u32 per tile) -> frontMap (record i at (i mod 8) * frontStride + i / 8)
hipError_t launchFollowPlan(const uint32_t* d_lives, uint32_t blocksX, uint32_t blocksY, uint32_t xcdSquare, uint32_t lifeBlock,
                            const FollowBands& bands, void* d_scratch, uint32_t* d_frontMap, uint32_t frontStride, hipStream_t stream);
hipError_t launchReciprocalSelfTest(unsigned long long* d_counts, hipStream_t stream);      // 3 counters, zeroed by the caller
// planning: from the visit logs of `tiles` one-piece walks (p.pieceLog layout) to the piece table: tile t gets cuts[t].pieces
// records starting at record firstPiece[t], its index ranges cut at the quantiles of its log
hipError_t launchSplitQuantiles(const uint32_t* d_log, uint32_t logCap, const SplitCut* d_cuts, const uint32_t* d_firstPiece,
                                uint32_t tiles, uint32_t* d_pieces, const void* d_wide, hipStream_t stream);

} // namespace rts
