// ADAPTIVE AMBIENT OCCLUSION (rts_trace_ambient_occlusion_adaptive*, include/rts.h): included by rts_distance.inc behind rts_ao.inc,
// modelled on rts_adaptive.inc with rts_ao.inc's prologue and ray set-up (aoPrologue, makeAoRay, makePointRayAt as they stand).
// From the common part (rts_block_common.inc): tileBlock, tilePixel, blockPixel, tileWave, freshLaneId, shareAnyHit, launchLoopFamily.
//
// For n = p.nsamples samples and a probe count k = p.nrays (rts_ao_adaptive.h: the slots), with u_j the any-hit byte of AO sample j
// (1 = unoccluded), c_k = u_0 + ... + u_(k-1) and c_n = u_0 + ... + u_(n-1):
//   counts[p] = 0 where the pixel is background or inactive or c_k == 0, n where c_k == k, c_n otherwise; refined[p] = 1 exactly in the
//   last case.
// Everything is integer counting of bytes that are functions of (pixel, sample) alone, so the result does not depend on the order
// the samples are walked in, nor on which wave walked which (DESIGN.md 4.35).

// (the header has a namespace of its own, so rts_kernels.hip's is closed around it, as in rts_ao.inc)
} // namespace rts
#include "rts_ao_adaptive.h"
namespace rts {

__device__ __forceinline__ uint8_t* aoRefined(const TraceParams& p) { return (uint8_t*)p.pieceClock; }

// aoPrologue, and the refined byte of an owned pixel that sends no ray: its count got its zero in there, its refined byte gets it HERE
// (aoPrologue leaves d->live in place whatever it answers).
__device__ __forceinline__ bool aoAdaptivePrologue(const TraceParams& p, bool owns, uint32_t pix, bool stores, AoPixel* d) {
    const bool walks = aoPrologue(p, owns, pix, stores, d);
    if (owns && !d->live && stores && aoRefined(p)) __builtin_nontemporal_store((uint8_t)0, &aoRefined(p)[pix]);
    return walks;
}

// Between the phases, as adaptiveRefineSetup (rts_adaptive.inc): a live pixel whose probe was unanimous gets its verdict NOW (0 or n,
// refined 0), stored in front of the second walk so that nothing of such a pixel stays in registers across it.  Then the lanes that do
// not refine take the pixel index of the first lane that does (d->live becomes `pen`) -- position and normal are fetched by that index
// per sample, so the stand-in sets up that lane's very rays: the wave is in the state aoPrologue leaves, with the refining pixels as
// its live set.  pens != 0.  `stores`: as in the prologue.
__device__ __forceinline__ void aoAdaptiveRefineSetup(const TraceParams& p, AoPixel* d, uint32_t ck, bool pen, uint64_t pens, bool stores) {
    if (d->live && !pen && stores) {
        __builtin_nontemporal_store((uint8_t)(ck != 0u ? p.nsamples : 0u), &p.mask[d->pix]);    // (unanimous: c_k is 0 or k)
        if (aoRefined(p)) __builtin_nontemporal_store((uint8_t)0, &aoRefined(p)[d->pix]);
    }
    const uint32_t sp = (uint32_t)__builtin_amdgcn_readlane((int)d->pix, __builtin_ctzll(pens));
    d->pix = pen ? d->pix : sp;
    d->live = pen;
}
// A wave without a refining pixel: every live pixel's verdict, and the wave is done.
__device__ __forceinline__ void aoAdaptiveStoreUnanimous(const TraceParams& p, const AoPixel& d, uint32_t ck) {
    if (!d.live) return;
    __builtin_nontemporal_store((uint8_t)(ck != 0u ? p.nsamples : 0u), &p.mask[d.pix]);
    if (aoRefined(p)) __builtin_nontemporal_store((uint8_t)0, &aoRefined(p)[d.pix]);
}
__device__ __forceinline__ void aoAdaptiveStoreRefined(const TraceParams& p, const AoPixel& d, uint32_t cn) {
    if (!d.live) return;                                                 // (live: the refining pixels, since aoAdaptiveRefineSetup)
    __builtin_nontemporal_store((uint8_t)cn, &p.mask[d.pix]);
    if (aoRefined(p)) __builtin_nontemporal_store((uint8_t)1, &aoRefined(p)[d.pix]);
}

// Lane per ray: ambientOcclusionShareKernel's 16 x 16 block, the probe samples and then the others one after the other around the
// any-hit walk.  The four waves share nothing but the LDS each owns a quarter of, so each decides for its own 8 x 8 quarter.
__global__ __launch_bounds__(256) void ambientOcclusionAdaptiveShareKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][64];       // lane numbers exchanged by traverseShare (256 B per wave)
    uint32_t* lds = shareSlots[threadIdx.x >> 6];
    uint32_t x, y;
    if (!blockPixel(p, &x, &y)) return;
    AoPixel d;
    if (!aoAdaptivePrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, true, &d)) return;
    const NodeStream bvh = openStream(p);
    const uint32_t probe = (uint32_t)p.nrays;
    uint32_t count = 0;
    for (uint32_t j = 0; j < probe; ++j) {
        const Ray r = makeAoRay(p, d.pix, j);
        const bool occluded = shareAnyHit(p, bvh, r, d.live, d.live && !raySafe(r), lds);
        count += (d.live && !occluded) ? 1u : 0u;
    }
    const bool pen = d.live && count != 0u && count != probe;
    const uint64_t pens = __builtin_amdgcn_ballot_w64(pen);
    if (pens == 0) { aoAdaptiveStoreUnanimous(p, d, count); return; }
    aoAdaptiveRefineSetup(p, &d, count, pen, pens, true);
    for (uint32_t j = probe; j < p.nsamples; ++j) {
        const Ray r = makeAoRay(p, d.pix, j);
        const bool occluded = shareAnyHit(p, bvh, r, d.live, d.live && !raySafe(r), lds);
        count += (d.live && !occluded) ? 1u : 0u;
    }
    aoAdaptiveStoreRefined(p, d, count);
}

// One sample of a packet wave: the ray of (pixel, j) and traversePacket<1, false> (any-hit, the early-out kept) -> the lane's byte.
// (The pixel index is made opaque per sample: otherwise the compiler hoists the sample-independent part of the set-up -- texel, frame,
//  origin, bias -- out of the loop and keeps it in registers across the walk: rts_ao.inc.)
__device__ __forceinline__ uint32_t aoAdaptiveSample(const TraceParams& p, const NodeStream& bvh, AoPixel& d, uint32_t j, uint32_t* lds) {
    asm volatile("" : "+v"(d.pix));
    const Ray r[1] = { makeAoRay(p, d.pix, j) };
    const bool walks[1] = { d.live };
    bool occluded[1];
    traversePacket<1, false>(p, bvh, r, walks, occluded, lds);
    return (walks[0] && !occluded[0]) ? 1u : 0u;
}

// Stackless packet over 8 x 8 tiles.  GEOM as in ambientOcclusionPacketKernel.  SPLIT 1: one wave walks the probe, decides, walks the
// rest.  SPLIT 4: shadowMaskAdaptivePacketKernel's two-phase scheme -- four waves per tile, which map lane -> pixel identically:
//   phase 1  wave w walks the probe samples w, w + 4, ... < k over the live pixels and counts per lane in partial[0][w];
//   BARRIER 1; every wave reads all four words of its lane: c_k, pen = live && 0 < c_k < k, ballot(pen) -- the same words in the
//            same lanes, so the same ballot in the four waves.  No refining pixel: wave 0 stores the verdicts, every wave returns;
//   phase 2  wave w walks the samples k + w, k + w + 4, ... < n over the refining pixels and counts in partial[1][w] -- a SECOND set
//            of words, so no wave writes a word that another may still be reading for its c_k (wave 0 starts its word at c_k);
//   BARRIER 2; wave 0 sums the four words of the second set and stores them where pen, with refined = 1.
// Every wave reaches each barrier or none does: the exits in front of barrier 1 (a block outside the dispatch, a tile without an
// active non-background pixel) and the one between the barriers (no refining pixel) depend on the tile alone -- on the geometry, on
// the tile's normals and active bytes and on LDS words all four waves read alike after barrier 1 --, never on the wave.  A wave that
// owns no sample of a phase (k < 4, n - k < 4) runs no walk in it and contributes 0.
// A wave keeps its counts in LDS (each lane its own word), not in registers across the walks: the kernel compiles for 64 VGPRs.
template <int SPLIT, int GEOM>
__global__ __launch_bounds__(64 * SPLIT) __attribute__((amdgpu_waves_per_eu(8)))
void ambientOcclusionAdaptivePacketKernel(TraceParams p) {
    static_assert(SPLIT == 1 || SPLIT == 4, "one wave per tile, or four that deal its samples");
    __shared__ uint32_t shareSlots[SPLIT][64];
    __shared__ uint32_t partial[2][SPLIT][64];                           // per phase and wave: unoccluded samples per lane
    uint32_t bx, by, x, y;
    if (!tileBlock<GEOM>(p, &bx, &by)) return;
    const uint32_t wave = tileWave<SPLIT>();
    tilePixel<GEOM>(p, bx, by, &x, &y);
    AoPixel d;
    if (!aoAdaptivePrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, wave == 0, &d)) return;
    const NodeStream bvh = openStream(p);
    const uint32_t probe = (uint32_t)p.nrays;
    partial[0][wave][freshLaneId()] = 0;
    for (uint32_t j = wave; j < probe; j += SPLIT) {
        const uint32_t one = aoAdaptiveSample(p, bvh, d, j, shareSlots[wave]);
        partial[0][wave][freshLaneId()] += one;
    }
    if constexpr (SPLIT > 1) __syncthreads();                            // BARRIER 1
    uint32_t ck = 0;
    {
        const uint32_t l = freshLaneId();
#pragma unroll
        for (int w = 0; w < SPLIT; ++w) ck += partial[0][w][l];
    }
    const bool pen = d.live && ck != 0u && ck != probe;
    const uint64_t pens = __builtin_amdgcn_ballot_w64(pen);
    if (pens == 0) {
        if (wave == 0) aoAdaptiveStoreUnanimous(p, d, ck);
        return;
    }
    aoAdaptiveRefineSetup(p, &d, ck, pen, pens, wave == 0);
    partial[1][wave][freshLaneId()] = wave == 0 ? ck : 0u;
    for (uint32_t j = probe + wave; j < p.nsamples; j += SPLIT) {
        const uint32_t one = aoAdaptiveSample(p, bvh, d, j, shareSlots[wave]);
        partial[1][wave][freshLaneId()] += one;
    }
    if constexpr (SPLIT > 1) {
        __syncthreads();                                                 // BARRIER 2
        if (wave != 0) return;
    }
    uint32_t cn = 0;
    const uint32_t l = freshLaneId();
#pragma unroll
    for (int w = 0; w < SPLIT; ++w) cn += partial[1][w][l];
    aoAdaptiveStoreRefined(p, d, cn);
}

hipError_t launchAmbientOcclusionAdaptive(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.distance || !p.mask || p.nsamples < 2 || p.nsamples > 48 || p.lightTable > 64 || (p.lightTable && p.lightTable < p.nsamples) ||
        p.nrays == 0 || p.nrays >= p.nsamples)
        return hipErrorInvalidValue;
    static const char* const names[2][3] = RTS_PACKET_NAMES("ambientOcclusionAdaptivePacketKernel", "");
    return launchLoopFamily(variant, p, stream, name, ambientOcclusionAdaptiveShareKernel, "ambientOcclusionAdaptiveShareKernel", names,
                            [&](dim3 grid, auto split, auto geom) {
        constexpr int SPLIT = decltype(split)::value, GEOM = decltype(geom)::value;
        hipLaunchKernelGGL((ambientOcclusionAdaptivePacketKernel<SPLIT, GEOM>), grid, dim3(64 * SPLIT), 0, stream, p); });
}
