// SOFT-SHADOW OCCLUDER DISTANCE (rts_trace_soft_distance*, include/rts.h): included by rts_distance.inc after its own kernels.
// From the common part (rts_block_common.inc): DIST_NONE, SoftPixel, softPrologue<true>, tileBlock, tilePixel, blockPixel,
// tileWave, freshLaneId, launchLoopFamily.  From rts_distance.inc: shareDistance, traversePacketDistance.
//
// distance[p] = min over the light's samples j of sample j's one-ray distance (rts_distance.inc), mask[p] = the number of samples
// whose distance is +Inf (the byte the soft mask trace writes).  Every one-ray distance is a bit pattern >= +0 whose integer order
// is the float order, so the minimum over samples is again an integer minimum: it does not depend on the order the samples are
// walked in, nor on which wave walked which -- the per-wave minima of the 4-wave form are joined in LDS by one more integer minimum
// and the counts by an integer sum, like the soft mask kernels' counts.  (A MEAN blocker distance would be a float sum, which has no
// order-free definition: DESIGN.md 4.13.)

// (the zeros of a pixel that sends no ray are stored by softPrologue<true>; from then on a lane is live or has nothing to store)
__device__ __forceinline__ void softDistanceStore(const TraceParams& p, const SoftPixel& d, uint32_t best, uint32_t lit) {
    if (!d.live) return;
    __builtin_nontemporal_store(__uint_as_float(best), &p.distance[d.pix]);
    if (p.mask) __builtin_nontemporal_store((uint8_t)lit, &p.mask[d.pix]);                              // comp:148-150, per sample
}

// Lane per ray: shadowDistanceShareKernel's block, the samples one after the other around traverseShareDistance.
__global__ __launch_bounds__(256) void shadowSoftDistanceShareKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][2][64];    // per wave: lane numbers exchanged by the walk, and the owners' minima
    uint32_t* lds = shareSlots[threadIdx.x >> 6][0];
    uint32_t* ldsMin = shareSlots[threadIdx.x >> 6][1];
    uint32_t x, y;
    if (!blockPixel(p, &x, &y)) return;
    SoftPixel d;
    if (!softPrologue<true>(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, true, &d)) return;
    const NodeStream bvh = openStream(p);
    uint32_t best = DIST_NONE, lit = 0;
    for (uint32_t s = 0; s < p.nsamples; ++s) {
        const Ray r = makeShadowRay(p, d.rel, s, d.pix);
        const uint32_t one = shareDistance(p, bvh, r, d.live, d.live && !raySafe(r), lds, ldsMin);   // (every sample's minimum starts at +Inf)
        lit += one == DIST_NONE ? 1u : 0u;
        best = one < best ? one : best;
    }
    softDistanceStore(p, d, best, lit);
}

// Stackless packet over 8 x 8 tiles, traversePacketDistance once per sample.  GEOM as in shadowDistancePacketKernel (1: a row range
// on a 2-D grid, 2: one stripe of power-of-two bands, 0: every other geometry).  SPLIT 1: one wave walks every sample.  SPLIT 4: four
// waves per tile, wave w takes the samples w, w + 4, ... (rts_packet_tile.inc); wave 0 folds and stores after ONE workgroup barrier.
// Every wave reaches that barrier or none does: the only exits in front of it (a block outside the dispatch, a tile without an
// active pixel) depend on the tile alone, which the four waves share; a wave that owns no sample (nsamples < 4) runs no walk and
// contributes +Inf / 0.
// A wave keeps its running minimum and count in LDS (each lane its own two words, so no ordering question arises), not in registers
// across the walk; in the 4-wave form these are the very words wave 0 folds.
// (makeShadowRay<false>: the general set-up alone, as in the soft mask kernels.)
template <int SPLIT, int GEOM>
__global__ __launch_bounds__(64 * SPLIT) __attribute__((amdgpu_waves_per_eu(8)))
void shadowSoftDistancePacketKernel(TraceParams p) {
    static_assert(SPLIT == 1 || SPLIT == 4, "one wave per tile, or four that deal its samples");
    __shared__ uint32_t shareSlots[SPLIT][2][64];
    __shared__ uint32_t partial[SPLIT][2][64];                           // per wave: {minimum, unoccluded samples} per lane
    uint32_t bx, by, x, y;
    if (!tileBlock<GEOM>(p, &bx, &by)) return;
    const uint32_t wave = tileWave<SPLIT>();
    tilePixel<GEOM>(p, bx, by, &x, &y);
    SoftPixel d;
    if (!softPrologue<true>(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, wave == 0, &d)) return;
    const NodeStream bvh = openStream(p);
    // (LDS is addressed by laneId(), the number the walks themselves keep: threadIdx.x & 63 would be one more register held to the end)
    uint32_t* const mine = &partial[wave][0][laneId()];
    mine[0] = DIST_NONE; mine[64] = 0;
    for (uint32_t s = wave; s < p.nsamples; s += SPLIT) {
        // (the texel and the pixel index are made opaque per sample: otherwise the compiler hoists every part of the set-up that
        //  does not depend on the sample -- origin, bias, the table's hashed start -- out of the loop and keeps it in registers
        //  across the walk, which costs scratch at 64 VGPRs; recomputing it is a dozen VALU operations per sample)
        asm volatile("" : "+v"(d.rel.x), "+v"(d.rel.y), "+v"(d.rel.z), "+v"(d.pix));
        const Ray r = makeShadowRay<false>(p, d.rel, s, d.pix);
        const uint32_t one = traversePacketDistance(p, bvh, r, d.live, shareSlots[wave][0], shareSlots[wave][1]);
        const uint32_t m = mine[0];
        mine[0] = one < m ? one : m;
        mine[64] += one == DIST_NONE ? 1u : 0u;
    }
    if constexpr (SPLIT > 1) {
        __syncthreads();
        if (wave != 0) return;
    }
    const uint32_t l = freshLaneId();                                    // (not laneId(): no address is carried from in front of the loop)
    uint32_t best = DIST_NONE, lit = 0;
#pragma unroll
    for (int w = 0; w < SPLIT; ++w) {
        const uint32_t m = partial[w][0][l];
        best = m < best ? m : best;
        lit += partial[w][1][l];
    }
    softDistanceStore(p, d, best, lit);
}

hipError_t launchShadowSoftDistance(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.distance || p.nsamples < 2 || p.nsamples > 64) return hipErrorInvalidValue;
    static const char* const names[2][3] = RTS_PACKET_NAMES("shadowSoftDistancePacketKernel", "");
    return launchLoopFamily(variant, p, stream, name, shadowSoftDistanceShareKernel, "shadowSoftDistanceShareKernel", names,
                            [&](dim3 grid, auto split, auto geom) {
        constexpr int SPLIT = decltype(split)::value, GEOM = decltype(geom)::value;
        hipLaunchKernelGGL((shadowSoftDistancePacketKernel<SPLIT, GEOM>), grid, dim3(64 * SPLIT), 0, stream, p); });
}
