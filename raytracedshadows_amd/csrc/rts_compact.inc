// Compacted light maps on the GPU (include/rts_scene.h: rtsh_compact_light_map_device): a light map -> the dense list of its marked
// pixels in tile order, the length left on the device.  The tile order and the mark are the host twin's own source
// (rts_closest_hit.h: makeCompactFrame, compactSlotPixel, compactMarked).  Included at the end of rts_primary.hip (the scene passes'
// translation unit), whose own kernels keep their instruction text.
//
// FOUR kernels (kCompactNodes, rts_closest_hit.h), integers only, and NO workgroup ever waits for another: each kernel reads what the one in front of
// it on the stream has finished writing.
//   1 compactCountKernel   one wave per tile: the ballot of its marked slots, popcount -> offsets[tile]
//   2 compactScanKernel    one workgroup per kCompactScanTiles tiles: offsets[] becomes the exclusive sum INSIDE the group, the group's
//                          total -> sums[group]
//   3 compactSumsKernel    ONE workgroup: sums[] becomes its exclusive sum (strips of kCompactScanTiles with a carry), the frame's total -> *n
//   4 compactWriteKernel   one wave per tile: the ballot again; marked slot k writes its pixel at sums[group] + offsets[tile] + the marked
//                          slots below k, where that lies below capacity
// d_scratch: offsets[tiles], then sums[ceil(tiles / kCompactScanTiles)], 32-bit words (rtsh_compact_scratch_bytes).  A frame has at
// most 2^31 pixels, so every sum fits 32 bits.

namespace rts_harness {
__device__ __forceinline__ uint64_t compactTileBallot(const CompactFrame& f, const uint8_t* map, uint32_t tile, uint32_t lane, uint32_t* p) {
    bool marked = false;
    if (tile < f.tiles && compactSlotPixel(f, tile, lane, p)) marked = compactMarked(f, map[*p]);
    return __builtin_amdgcn_ballot_w64(marked);
}

__global__ __launch_bounds__(256) void compactCountKernel(CompactFrame f, const uint8_t* map, uint32_t* offsets) {
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    uint32_t p;
    const uint64_t marked = compactTileBallot(f, map, tile, lane, &p);
    if (tile < f.tiles && lane == 0u) offsets[tile] = (uint32_t)__builtin_popcountll(marked);
}

// The exclusive sum of one value per lane over the workgroup's 256 lanes; *total: their sum.  (Barriers INSIDE a workgroup only.)
__device__ __forceinline__ uint32_t compactBlockScan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t o = 1; o < kCompactScanLanes; o <<= 1) {
        const uint32_t below = t >= o ? lds[t - o] : 0u;
        __syncthreads();
        lds[t] += below;
        __syncthreads();
    }
    const uint32_t inclusive = lds[t];
    *total = lds[kCompactScanLanes - 1u];
    __syncthreads();                                                     // (the next strip writes lds again)
    return inclusive - v;
}

// words[base .. base + kCompactScanTiles) below `end` become their exclusive sum plus carry; -> the strip's total
__device__ __forceinline__ uint32_t compactScanStrip(uint32_t* words, uint32_t base, uint32_t end, uint32_t carry, uint32_t* lds) {
    const uint32_t first = base + threadIdx.x * kCompactScanPerLane;  // (tiles <= 2^28: no index here wraps)
    uint32_t v[kCompactScanPerLane], mine = 0;
#pragma unroll
    for (uint32_t i = 0; i < kCompactScanPerLane; ++i) {
        v[i] = first + i < end ? words[first + i] : 0u;
        mine += v[i];
    }
    uint32_t total;
    uint32_t below = carry + compactBlockScan(mine, lds, &total);
#pragma unroll
    for (uint32_t i = 0; i < kCompactScanPerLane; ++i) {
        if (first + i < end) words[first + i] = below;
        below += v[i];
    }
    return total;
}

__global__ __launch_bounds__(256) void compactScanKernel(uint32_t tiles, uint32_t* offsets, uint32_t* sums) {
    __shared__ uint32_t lds[kCompactScanLanes];
    const uint32_t total = compactScanStrip(offsets, blockIdx.x * kCompactScanTiles, tiles, 0u, lds);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void compactSumsKernel(uint32_t groups, uint32_t* sums, uint32_t* n) {
    __shared__ uint32_t lds[kCompactScanLanes];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < groups; base += kCompactScanTiles)    // (groups <= 2^18 + 1: at most 257 strips, one for a 4K frame)
        carry += compactScanStrip(sums, base, groups, carry, lds);
    if (threadIdx.x == 0u) *n = carry;
}

__global__ __launch_bounds__(256) void compactWriteKernel(CompactFrame f, const uint8_t* map, const uint32_t* offsets, const uint32_t* sums,
                                                          uint32_t* pixels, uint32_t capacity) {
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    uint32_t p;
    const uint64_t marked = compactTileBallot(f, map, tile, lane, &p);
    if (marked == 0) return;                                             // (wave-uniform; a tile beyond the frame has none)
    const uint32_t at = sums[tile / kCompactScanTiles] + offsets[tile] + (uint32_t)__builtin_popcountll(marked & ((1ull << lane) - 1ull));
    if (((marked >> lane) & 1ull) && at < capacity) pixels[at] = p;
}
} // namespace rts_harness

extern "C" int rtsh_compact_light_map_device(rts_ctx* ctx, uint32_t count, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                             uint32_t* d_pixels, uint32_t capacity, uint32_t* d_n, void* d_scratch, void* stream) {
    using namespace rts_harness;
    CompactFrame f;
    if (!ctx || !d_lights_map || !d_pixels || !d_n || !d_scratch || capacity == 0 || !makeCompactFrame(count, W, H, &f)) return RTS_ERR_INVALID_ARG;
    const uint32_t groups = (uint32_t)(((uint64_t)f.tiles + kCompactScanTiles - 1u) / kCompactScanTiles);
    uint32_t* const offsets = (uint32_t*)d_scratch;
    uint32_t* const sums = offsets + f.tiles;
    const dim3 perTile((uint32_t)(((uint64_t)f.tiles + 3u) / 4u)), block(256);
    int s = launchPass(ctx, stream, perTile, block, 0, compactCountKernel, f, d_lights_map, offsets);
    if (s == RTS_OK) s = launchPass(ctx, stream, dim3(groups), block, 0, compactScanKernel, f.tiles, offsets, sums);
    if (s == RTS_OK) s = launchPass(ctx, stream, dim3(1), block, 0, compactSumsKernel, groups, sums, d_n);
    if (s == RTS_OK) s = launchPass(ctx, stream, perTile, block, 0, compactWriteKernel, f, d_lights_map, (const uint32_t*)offsets,
                                    (const uint32_t*)sums, d_pixels, capacity);
    return s;
}
