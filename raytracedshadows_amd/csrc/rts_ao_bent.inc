// BENT NORMALS (rts_trace_ambient_occlusion_bent*, include/rts.h): included last by rts_distance.inc, behind rts_ao_adaptive.inc; a
// sibling of rts_ao.inc with its prologue and ray set-up (aoPrologue, makeAoRay, makePointRayAt as they stand).
// From the common part (rts_block_common.inc): tileBlock, tilePixel, blockPixel, tileWave, freshLaneId, shareAnyHit, launchLoopFamily.
// From rts_closest_hit.h: aoQuantise, aoBent -- the host twin's own source.
//
// With u_j the any-hit byte of AO sample j (1 = unoccluded) and q_j = Q(dirs[idx(p, j)]) its tangent-space direction in 1/16384ths:
//   S = sum u_j * q_j (three integers), c = sum u_j (the AO trace's byte);  bent[p] = (frame(N) * (S * 2^-14), (float)c).
// Everything in front of the frame is integer addition of values that are functions of (pixel, sample) alone, so the result does not
// depend on the order the samples are walked in, nor on which wave walked which; the frame is applied ONCE, to the finished sum, by
// the one lane that stores the texel (DESIGN.md 4.36).

// (the header has a namespace of its own, so rts_kernels.hip's is closed around it, as in rts_ao.inc)
} // namespace rts
#include "rts_ao_bent.h"
namespace rts {

__device__ __forceinline__ f32x4* aoBentPlane(const TraceParams& p) { return (f32x4*)p.pieceClock; }

// aoPrologue, and the texel of an owned pixel that sends no ray: its count gets its zero in there -- where there IS a count plane: it is
// optional here --, its texel gets (+0, +0, +0, +0) HERE (aoPrologue leaves d->live in place whatever it answers).
__device__ __forceinline__ bool aoBentPrologue(const TraceParams& p, bool owns, uint32_t pix, bool stores, AoPixel* d) {
    const bool walks = aoPrologue(p, owns, pix, stores && p.mask != nullptr, d);
    if (owns && !d->live && stores) __builtin_nontemporal_store(f32x4{ 0.0f, 0.0f, 0.0f, 0.0f }, aoBentPlane(p) + pix);
    return walks;
}

// What sample j adds for the lane's pixel where it is unoccluded: Q of its table entry (without a table the index is wave-uniform).
struct AoBentStep { uint32_t x, y, z; };
__device__ __forceinline__ AoBentStep aoBentStep(const TraceParams& p, uint32_t pix, uint32_t j) {
    const float* s = p.offsets[sampleIndex(p, j, pix)];
    return AoBentStep{ (uint32_t)rts_harness::aoQuantise(s[0]), (uint32_t)rts_harness::aoQuantise(s[1]),
                       (uint32_t)rts_harness::aoQuantise(s[2]) };
}

// The end of a live pixel: N once more by the pixel index, the frame applied to the finished sum, one 16-byte texel, and the count.
__device__ __forceinline__ void aoBentStore(const TraceParams& p, const AoPixel& d, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t lit) {
    if (!d.live) return;
    const f32x4 n = *(aoNormals(p) + d.pix);
    float b[4];
    rts_harness::aoBent(rts_harness::V3{ n.x, n.y, n.z }, (int32_t)sx, (int32_t)sy, (int32_t)sz, lit, b);
    __builtin_nontemporal_store(f32x4{ b[0], b[1], b[2], b[3] }, aoBentPlane(p) + d.pix);
    if (p.mask) __builtin_nontemporal_store((uint8_t)lit, &p.mask[d.pix]);                       // comp:150
}

// Lane per ray: ambientOcclusionShareKernel's 16 x 16 block, four integer accumulators per lane around the any-hit walk.  The four
// waves share nothing but the LDS each owns a quarter of, so each decides for its own 8 x 8 quarter.
__global__ __launch_bounds__(256) void ambientOcclusionBentShareKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][64];       // lane numbers exchanged by traverseShare (256 B per wave)
    uint32_t* lds = shareSlots[threadIdx.x >> 6];
    uint32_t x, y;
    if (!blockPixel(p, &x, &y)) return;
    AoPixel d;
    if (!aoBentPrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, true, &d)) return;
    const NodeStream bvh = openStream(p);
    uint32_t sx = 0, sy = 0, sz = 0, lit = 0;
    for (uint32_t j = 0; j < p.nsamples; ++j) {
        const Ray r = makeAoRay(p, d.pix, j);
        const bool occluded = shareAnyHit(p, bvh, r, d.live, d.live && !raySafe(r), lds);
        const uint32_t keep = (d.live && !occluded) ? 0xFFFFFFFFu : 0u;
        const AoBentStep q = aoBentStep(p, d.pix, j);
        sx += q.x & keep; sy += q.y & keep; sz += q.z & keep; lit += keep & 1u;                   // comp:148, per sample
    }
    aoBentStore(p, d, sx, sy, sz, lit);
}

// Stackless packet over 8 x 8 tiles, traversePacket<1, false> once per sample.  GEOM and SPLIT as in ambientOcclusionPacketKernel:
// SPLIT 4 deals the samples over four waves, wave w taking w, w + 4, ...; wave 0 adds the four waves' words and stores after ONE
// workgroup barrier.  Every wave reaches that barrier or none does: the only exits in front of it (a block outside the dispatch, a
// tile without an active non-background pixel) depend on the tile alone, which the four waves share; a wave that owns no sample
// (nsamples < 4) runs no walk and contributes zeros.
// A wave keeps its four running words (S.x, S.y, S.z, c) in LDS, each lane its own, not in registers across the walk -- 4 KiB at
// SPLIT 4 --; in the 4-wave form these are the very words wave 0 adds.  The sample's Q is worked out BEHIND its walk.
template <int SPLIT, int GEOM>
__global__ __launch_bounds__(64 * SPLIT) __attribute__((amdgpu_waves_per_eu(8)))
void ambientOcclusionBentPacketKernel(TraceParams p) {
    static_assert(SPLIT == 1 || SPLIT == 4, "one wave per tile, or four that deal its samples");
    __shared__ uint32_t shareSlots[SPLIT][64];
    __shared__ uint32_t partial[SPLIT][4][64];                           // per wave: S.x, S.y, S.z and the count, per lane
    uint32_t bx, by, x, y;
    if (!tileBlock<GEOM>(p, &bx, &by)) return;
    const uint32_t wave = tileWave<SPLIT>();
    tilePixel<GEOM>(p, bx, by, &x, &y);
    AoPixel d;
    if (!aoBentPrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, wave == 0, &d)) return;
    const NodeStream bvh = openStream(p);
    {
        const uint32_t l = freshLaneId();
#pragma unroll
        for (int c = 0; c < 4; ++c) partial[wave][c][l] = 0;
    }
    for (uint32_t j = wave; j < p.nsamples; j += SPLIT) {
        // (the pixel index is made opaque per sample, so that nothing of the set-up is kept in registers across the walk: rts_ao.inc)
        asm volatile("" : "+v"(d.pix));
        const Ray r[1] = { makeAoRay(p, d.pix, j) };
        const bool walks[1] = { d.live };
        bool occluded[1];
        traversePacket<1, false>(p, bvh, r, walks, occluded, shareSlots[wave]);
        const uint32_t keep = (walks[0] && !occluded[0]) ? 0xFFFFFFFFu : 0u;
        const AoBentStep q = aoBentStep(p, d.pix, j);
        const uint32_t l = freshLaneId();
        partial[wave][0][l] += q.x & keep; partial[wave][1][l] += q.y & keep; partial[wave][2][l] += q.z & keep;
        partial[wave][3][l] += keep & 1u;                                // comp:148, per sample
    }
    if constexpr (SPLIT > 1) {
        __syncthreads();
        if (wave != 0) return;
    }
    const uint32_t l = freshLaneId();
    uint32_t sum[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int w = 0; w < SPLIT; ++w) {
#pragma unroll
        for (int c = 0; c < 4; ++c) sum[c] += partial[w][c][l];
    }
    aoBentStore(p, d, sum[0], sum[1], sum[2], sum[3]);
}

hipError_t launchAmbientOcclusionBent(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.distance || !p.pieceClock || p.nsamples < 1 || p.nsamples > 48 || p.lightTable > 64 || (p.lightTable && p.lightTable < p.nsamples))
        return hipErrorInvalidValue;
    static const char* const names[2][3] = RTS_PACKET_NAMES("ambientOcclusionBentPacketKernel", "");
    return launchLoopFamily(variant, p, stream, name, ambientOcclusionBentShareKernel, "ambientOcclusionBentShareKernel", names,
                            [&](dim3 grid, auto split, auto geom) {
        constexpr int SPLIT = decltype(split)::value, GEOM = decltype(geom)::value;
        hipLaunchKernelGGL((ambientOcclusionBentPacketKernel<SPLIT, GEOM>), grid, dim3(64 * SPLIT), 0, stream, p); });
}
