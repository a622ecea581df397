// The geometry of one frame dispatch and what follows from it alone: the rows it launches, the band shift of its stripes, its tile
// counts.  No HIP and no context: rts_api.cpp and a stand-alone host program (tests/cpp/dispatch_host.cpp) include it alike.
#pragma once
#include <stdint.h>

namespace rts {

// tiles of a dispatch: blocksX x blocksY blocks, gridBlocks workgroups launched (nBlocks, or the next multiple of 8 for the swizzle)
struct Grid { uint32_t blocksX, blocksY, nBlocks, gridBlocks; };

// include/rts.h: band_rows a nonzero multiple of 8 pixel rows, stripe one of n_stripes
inline bool stripeArgsOk(uint32_t band_rows, uint32_t n_stripes, uint32_t stripe) {
    return band_rows != 0 && band_rows % 8 == 0 && n_stripes != 0 && stripe < n_stripes;
}

// Virtual rows of one interleaved stripe's dispatch: band_rows times the number of bands stripe, stripe + n_stripes, ... it
// owns (the last one may be cut by H: guarded in-kernel).  0 when the stripe owns no band (stripe >= bands): nothing to launch.
inline uint32_t stripeRows(uint32_t H, uint32_t band_rows, uint32_t n_stripes, uint32_t stripe) {
    const uint32_t bands = (uint32_t)(((uint64_t)H + band_rows - 1) / band_rows);
    return stripe < bands ? ((bands - stripe - 1) / n_stripes + 1) * band_rows : 0u;
}

// Rows [rowBegin, rowEnd) of a W x H frame (nStripes 1, bandRows and stripe 0), or stripe `stripe` of nStripes > 1 interleaved
// stripes in bands of bandRows rows (rowBegin 0, rowEnd H).  Two dispatches are the same dispatch when all seven are equal.
struct Dispatch {
    uint32_t W, H, rowBegin, rowEnd, bandRows, nStripes, stripe;

    static Dispatch ofRows(uint32_t W, uint32_t H, uint32_t rowBegin, uint32_t rowEnd) { return { W, H, rowBegin, rowEnd, 0, 1, 0 }; }
    static Dispatch ofStripe(uint32_t W, uint32_t H, uint32_t bandRows, uint32_t nStripes, uint32_t stripe) {
        return nStripes == 1 ? ofRows(W, H, 0, H) : Dispatch{ W, H, 0, H, bandRows, nStripes, stripe };     // (one stripe: the whole frame)
    }
    bool operator==(const Dispatch& o) const {
        return W == o.W && H == o.H && rowBegin == o.rowBegin && rowEnd == o.rowEnd && bandRows == o.bandRows &&
               nStripes == o.nStripes && stripe == o.stripe;
    }
    // the rows it launches (stripes: whole owned bands)
    uint32_t rows() const { return nStripes <= 1 ? rowEnd - rowBegin : stripeRows(H, bandRows, nStripes, stripe); }
    // stripes in bands of a power of two of 8-row tiles: its log2; 0xFFFFFFFF otherwise
    uint32_t bandShift() const {
        uint32_t bandShift = 0xFFFFFFFFu;
        if (nStripes > 1 && bandRows != 0 && bandRows % 8 == 0) {
            const uint32_t tiles = bandRows / 8;
            if ((tiles & (tiles - 1)) == 0) { uint32_t sh = 0; while ((1u << sh) < tiles) ++sh; bandShift = sh; }
        }
        return bandShift;
    }
    // blocks of blockW x blockH pixels over W x rows()
    Grid grid(uint32_t blockW, uint32_t blockH, bool swizzle) const {
        Grid g;
        g.blocksX = (W + blockW - 1) / blockW;
        g.blocksY = (rows() + blockH - 1) / blockH;
        g.nBlocks = g.blocksX * g.blocksY;
        g.gridBlocks = swizzle ? ((g.nBlocks + 7) / 8) * 8 : g.nBlocks;
        return g;
    }
};

} // namespace rts
