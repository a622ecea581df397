// AO DISTANCE AND FALLOFF (rts_trace_ambient_occlusion_distance*, include/rts.h): included last by rts_distance.inc, behind
// rts_ao_bent.inc; rts_ao.inc's prologue and ray set-up (aoPrologue, makeAoRay, makePointRayAt as they stand) around
// rts_soft_distance.inc's walks (shareDistance, traversePacketDistance).
// From the common part (rts_block_common.inc): DIST_NONE, tileBlock, tilePixel, blockPixel, tileWave, freshLaneId, launchLoopFamily.
// From rts_closest_hit.h: aoFalloffBin, aoOpenness, aoObscurance -- the host twin's own source.
//
// With d_j the one-ray distance of AO sample j (a bit pattern >= +0, +Inf where the segment is free):
//   best = min_j d_j (an integer minimum),  c = #{ j : d_j == +Inf } (the AO trace's byte),
//   A = sum_j a_j,  a_j = 255 where d_j == +Inf, else weight[min(63, (uint32_t)(min(d_j, 1) * 64))]  (an integer sum),
//   obscurance = (2 * A * S + 255) / 510,  S = 65535 / n.
// Minimum, count and A are an integer minimum and two integer sums of functions of (pixel, sample) alone, so none of them depends on
// the order the samples are walked in, nor on which wave walked which (DESIGN.md 4.37).
// In the argument block (rts_ao_distance.h): the distance plane in p.pieceClock, the obscurance plane in p.nrays -- either may be NULL,
// not both --, the 64 weights in the .w of the 64 direction entries.

// (the header has a namespace of its own, so rts_kernels.hip's is closed around it, as in rts_ao.inc)
} // namespace rts
#include <stddef.h>
#include "rts_ao_distance.h"
namespace rts {

__device__ __forceinline__ float* aoDistancePlane(const TraceParams& p) { return (float*)p.pieceClock; }
__device__ __forceinline__ uint16_t* aoObscurancePlane(const TraceParams& p) { return (uint16_t*)(uintptr_t)p.nrays; }

// The 64 weights, once per wave, into the wave's own 64 bytes of LDS: lane b takes weight[b].  The table lives in the argument block,
// and indexing a by-value argument with a lane's number makes the compiler copy the block to scratch; the kernel argument segment
// IS memory, though, so the lane reads its word there with one vector load (the block is the kernel's one argument: offset 0).
// The fence and the wave barrier order the bytes in front of the other lanes' reads, as in traverseShareDistance.
__device__ __forceinline__ void aoStageFalloff(uint8_t* table) {
    typedef const __attribute__((address_space(4))) uint32_t* ArgWords;
    const ArgWords args = (ArgWords)__builtin_amdgcn_kernarg_segment_ptr();
    const uint32_t b = freshLaneId();
    table[b] = (uint8_t)args[(offsetof(TraceParams, offsets) + 12u) / 4u + b * 4u];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// aoPrologue, and the zeros of an owned pixel that sends no ray: its count gets its zero in there -- where there IS a count plane --,
// its distance (+0.0f) and its obscurance (0) HERE, each where its plane is given (aoPrologue leaves d->live in place whatever it answers).
__device__ __forceinline__ bool aoDistancePrologue(const TraceParams& p, bool owns, uint32_t pix, bool stores, AoPixel* d) {
    const bool walks = aoPrologue(p, owns, pix, stores && p.mask != nullptr, d);
    if (owns && !d->live && stores) {
        if (aoDistancePlane(p)) __builtin_nontemporal_store(0.0f, aoDistancePlane(p) + pix);
        if (aoObscurancePlane(p)) __builtin_nontemporal_store((uint16_t)0, aoObscurancePlane(p) + pix);
    }
    return walks;
}

// The end of a live pixel: up to three stores, each where its plane is given (wave-uniform branches).
__device__ __forceinline__ void aoDistanceStore(const TraceParams& p, const AoPixel& d, uint32_t best, uint32_t lit, uint32_t open) {
    if (!d.live) return;
    if (aoDistancePlane(p)) __builtin_nontemporal_store(__uint_as_float(best), aoDistancePlane(p) + d.pix);
    if (aoObscurancePlane(p))
        __builtin_nontemporal_store((uint16_t)rts_harness::aoObscurance(open, p.nsamples), aoObscurancePlane(p) + d.pix);
    if (p.mask) __builtin_nontemporal_store((uint8_t)lit, &p.mask[d.pix]);                       // comp:150
}

// Lane per ray: shadowSoftDistanceShareKernel's 16 x 16 block and LDS shape, the AO samples one after the other around
// traverseShareDistance.  The four waves share nothing but the LDS each owns a quarter of, so each decides for its own 8 x 8 quarter.
__global__ __launch_bounds__(256) void ambientOcclusionDistanceShareKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][2][64];    // per wave: lane numbers exchanged by the walk, and the owners' minima
    __shared__ uint8_t falloff[4][64];           // per wave: the 64 weights (staged only where there is an obscurance plane)
    uint32_t* lds = shareSlots[threadIdx.x >> 6][0];
    uint32_t* ldsMin = shareSlots[threadIdx.x >> 6][1];
    uint8_t* table = falloff[threadIdx.x >> 6];
    uint32_t x, y;
    if (!blockPixel(p, &x, &y)) return;
    AoPixel d;
    if (!aoDistancePrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, true, &d)) return;
    const bool weighs = aoObscurancePlane(p) != nullptr;
    if (weighs) aoStageFalloff(table);
    const NodeStream bvh = openStream(p);
    uint32_t best = DIST_NONE, lit = 0, open = 0;
    for (uint32_t j = 0; j < p.nsamples; ++j) {
        const Ray r = makeAoRay(p, d.pix, j);
        const uint32_t one = shareDistance(p, bvh, r, d.live, d.live && !raySafe(r), lds, ldsMin);   // (every sample's minimum starts at +Inf)
        lit += one == DIST_NONE ? 1u : 0u;                               // comp:148, per sample
        best = one < best ? one : best;
        if (weighs) open += rts_harness::aoOpenness(one, [&](uint32_t b) { return table[b]; });
    }
    aoDistanceStore(p, d, best, lit, open);
}

// Stackless packet over 8 x 8 tiles: aoPrologue, then makeAoRay and traversePacketDistance once per sample.  GEOM and SPLIT as in
// ambientOcclusionPacketKernel: SPLIT 4 deals the samples over four waves, wave w taking w, w + 4, ...; wave 0 joins the four waves'
// words -- one integer minimum, two integer sums -- and stores after ONE workgroup barrier.  Every wave reaches that barrier or none
// does: the only exits in front of it (a block outside the dispatch, a tile without an active non-background pixel) depend on the tile
// alone, which the four waves share -- aoPrologue's answer is a ballot over the tile's 64 pixels, the same in each --; the branches on
// the two plane pointers are uniform over the whole dispatch and end no wave; a wave that owns no sample (nsamples < 4) runs no walk
// and contributes +Inf, 0 and 0.
// A wave keeps its three running words (minimum, count, A) in LDS, each lane its own, not in registers across the walk -- 3 KiB at
// SPLIT 4 --; in the 4-wave form these are the very words wave 0 joins.  Each wave stages the weights for itself (its own 64 bytes):
// no wave reads another's table, so the staging needs no barrier.  Without an obscurance plane no weight is staged or looked up.
template <int SPLIT, int GEOM>
__global__ __launch_bounds__(64 * SPLIT) __attribute__((amdgpu_waves_per_eu(8)))
void ambientOcclusionDistancePacketKernel(TraceParams p) {
    static_assert(SPLIT == 1 || SPLIT == 4, "one wave per tile, or four that deal its samples");
    __shared__ uint32_t shareSlots[SPLIT][2][64];
    __shared__ uint32_t partial[SPLIT][3][64];                           // per wave: minimum, unoccluded samples and A, per lane
    __shared__ uint8_t falloff[SPLIT][64];
    uint32_t bx, by, x, y;
    if (!tileBlock<GEOM>(p, &bx, &by)) return;
    const uint32_t wave = tileWave<SPLIT>();
    tilePixel<GEOM>(p, bx, by, &x, &y);
    AoPixel d;
    if (!aoDistancePrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, wave == 0, &d)) return;
    const bool weighs = aoObscurancePlane(p) != nullptr;
    if (weighs) aoStageFalloff(falloff[wave]);
    const NodeStream bvh = openStream(p);
    {
        const uint32_t l = freshLaneId();
        partial[wave][0][l] = DIST_NONE; partial[wave][1][l] = 0; partial[wave][2][l] = 0;
    }
    for (uint32_t j = wave; j < p.nsamples; j += SPLIT) {
        // (the pixel index is made opaque per sample, so that nothing of the set-up is kept in registers across the walk: rts_ao.inc)
        asm volatile("" : "+v"(d.pix));
        const Ray r = makeAoRay(p, d.pix, j);
        const uint32_t one = traversePacketDistance(p, bvh, r, d.live, shareSlots[wave][0], shareSlots[wave][1]);
        const uint32_t l = freshLaneId();
        const uint32_t m = partial[wave][0][l];
        partial[wave][0][l] = one < m ? one : m;
        partial[wave][1][l] += one == DIST_NONE ? 1u : 0u;               // comp:148, per sample
        if (weighs) partial[wave][2][l] += rts_harness::aoOpenness(one, [&](uint32_t b) { return falloff[wave][b]; });
    }
    if constexpr (SPLIT > 1) {
        __syncthreads();
        if (wave != 0) return;
    }
    const uint32_t l = freshLaneId();
    uint32_t best = DIST_NONE, lit = 0, open = 0;
#pragma unroll
    for (int w = 0; w < SPLIT; ++w) {
        const uint32_t m = partial[w][0][l];
        best = m < best ? m : best;
        lit += partial[w][1][l];
        open += partial[w][2][l];
    }
    aoDistanceStore(p, d, best, lit, open);
}

hipError_t launchAmbientOcclusionDistance(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.distance || (!p.pieceClock && !p.nrays) || p.nsamples < 1 || p.nsamples > 48 || p.lightTable > 64 ||
        (p.lightTable && p.lightTable < p.nsamples))
        return hipErrorInvalidValue;
    static const char* const names[2][3] = RTS_PACKET_NAMES("ambientOcclusionDistancePacketKernel", "");
    return launchLoopFamily(variant, p, stream, name, ambientOcclusionDistanceShareKernel, "ambientOcclusionDistanceShareKernel", names,
                            [&](dim3 grid, auto split, auto geom) {
        constexpr int SPLIT = decltype(split)::value, GEOM = decltype(geom)::value;
        hipLaunchKernelGGL((ambientOcclusionDistancePacketKernel<SPLIT, GEOM>), grid, dim3(64 * SPLIT), 0, stream, p); });
}
