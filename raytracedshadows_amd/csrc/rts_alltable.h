// The ALLTABLE instantiation of the wide packet kernel (rts_packet_tile.inc): when the host selects it, and the
// per-scene constants its waves read.  Plain C++ without HIP headers, so that tests/cpp/alltable_host.cpp checks both on the CPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RTS_ALLTABLE_HD __host__ __device__
#else
#define RTS_ALLTABLE_HD
#endif

namespace rts {

// What launchWide knows about a one-wave-per-tile launch of kernel 8 (fields of TraceParams, as booleans where only that counts).
struct AllTableFacts {
    uint32_t wavesPerBlock;   // "block_waves"
    uint32_t nsamples;        // light samples per pixel
    bool wideLane;            // option "wide_lane": the instantiation with LDS stacks
    bool follow;              // follow mode records tile lives: its own kernel template
    bool table;               // a split table or a follow order is installed for this launch (p.pieces)
    bool hasPieces;           // ... and it holds split tiles
    bool allInTable;          // ... and every tile of the dispatch has a record (no tile rows)
    bool frontMap;            // ... and the XCD-major dword map exists (NULL in planning launches)
    bool stripes;             // nStripes > 1: one stripe of an interleaved frame (the BANDS instantiations)
    bool waveStats;           // wave statistics are being recorded
    bool sceneBounds;         // the context has its block of per-scene constants
    uint32_t nPieces, blocksX, pieceRows;   // records, and the grid that holds them
};

// ALLTABLE: every tile a record, no pieces, no tile rows, one sample, whole frames -- and a grid of exactly the records, so that
// a wave needs no `id >= nPieces` test (a whole-dispatch table has blocksX * blocksY records in blocksY rows).
inline bool allTableRule(const AllTableFacts& f) {
    return f.wavesPerBlock == 1 && f.nsamples == 1 && !f.wideLane && !f.follow && f.table && !f.hasPieces && f.allInTable && f.frontMap &&
           !f.stripes && !f.waveStats && f.sceneBounds && f.pieceRows != 0 && (uint64_t)f.blocksX * f.pieceRows == f.nPieces;
}

// wideAxisBound of rts_kernels.hip, restated for the one-thread kernel that fills the constants (sceneBoundsKernel) and for the
// CPU test: 2^k >= max(|lo|, |hi|) * 2^-122 and >= 2^-100 as float bits; +Inf when a coordinate is Inf or NaN.
RTS_ALLTABLE_HD inline uint32_t sceneAxisBound(uint32_t loBits, uint32_t hiBits) {
    const uint32_t a = loBits & 0x7FFFFFFFu, b = hiBits & 0x7FFFFFFFu;
    const uint32_t e = (a > b ? a : b) >> 23;
    return e == 255u ? 0x7F800000u : ((e > 148u ? e : 148u) - 121u) << 23;
}

// The block: {rootLo.xyz, bound.x, rootHi.xyz, bound.y, bound.z} from the root node's eight dwords {lo.xyz, link, hi.xyz, link}.
constexpr uint32_t SCENE_BOUNDS_DWORDS = 9;
RTS_ALLTABLE_HD inline void sceneBoundsOf(const uint32_t* root8, uint32_t* out9) {
    out9[0] = root8[0]; out9[1] = root8[1]; out9[2] = root8[2];
    out9[4] = root8[4]; out9[5] = root8[5]; out9[6] = root8[6];
    out9[3] = sceneAxisBound(root8[0], root8[4]);
    out9[7] = sceneAxisBound(root8[1], root8[5]);
    out9[8] = sceneAxisBound(root8[2], root8[6]);
}

} // namespace rts
