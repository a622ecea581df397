// AMBIENT OCCLUSION (rts_trace_ambient_occlusion*, include/rts.h): included last by rts_distance.inc, modelled on rts_soft_distance.inc.
// From the common part (rts_block_common.inc): tileBlock, tilePixel, blockPixel, tileWave, freshLaneId, shareAnyHit,
// launchLoopFamily.  From rts_kernels.hip: sampleIndex, traversePacket, and the pieces of makeShadowRay's general set-up.
// From rts_closest_hit.h: aoFrame, aoAim -- the host twin's own source.
//
// counts[p] = the number of sample j < nsamples whose segment from the surface to L_j(p) meets no triangle: sample j IS the shadow
// ray of the hard point light at L_j(p) = o0 + radius * (frame(N) * dirs[idx(p, j)]).  A count is a sum of bytes that are functions of
// (pixel, sample) alone, and integer addition is associative and commutative: it does not depend on the order the samples are
// walked in, nor on which wave walked which -- the 4-wave form adds the waves' counts in LDS (DESIGN.md 4.34).
// In the argument block (rts_ao.h): the normals in the distances' slot, the counts in p.mask, the radius in p.light[0], the
// directions in p.offsets, their table size in p.lightTable (so sampleIndex is the mask kernels' own), the active map in p.activeMap.

// (rts_closest_hit.h has a namespace of its own, so rts_kernels.hip's is closed around it, as around rts_soft_list_slots.h)
} // namespace rts
#include "rts_closest_hit.h"
#include "rts_ao.h"
namespace rts {

__device__ __forceinline__ const f32x4* aoNormals(const TraceParams& p) { return (const f32x4*)p.distance; }

// The ray of the hard point light at L -- a position PER LANE -- at the texel rel: makeShadowRay's general set-up for a point light,
// restated operation for operation as makeSoftListRay restates it (rts_soft_light_list.inc), because makeShadowRay reads its light
// from the argument block and lives in rts_kernels.hip, whose text the committed counter profiles are keyed to (handing it a
// per-lane light under `if constexpr` kept every kernel's instruction text, but not that key).  A fix to either goes to both; the
// host twin pins the bits.  The choices between rcpFast and the division are made per wave, as there.
__device__ __forceinline__ Ray makePointRayAt(const TraceParams& p, F3 rel, F3 L) {
    F3 origin{ p.cam[0] + rel.x, p.cam[1] + rel.y, p.cam[2] + rel.z };
    float mo = gmax(gmax(__builtin_fabsf(origin.x), __builtin_fabsf(origin.y)), __builtin_fabsf(origin.z));
    float mr = gmax(gmax(__builtin_fabsf(rel.x), __builtin_fabsf(rel.y)), __builtin_fabsf(rel.z));
    float bias = gmax(epsilonFor(mo, 13), epsilonFor(mr, 13));
    Ray r;
    F3 d0 = sub3(L, origin);
    const float len = __builtin_sqrtf(dot3(d0, d0));
    float inv;
    if (__builtin_amdgcn_ballot_w64(!rcpInRange(len)) == 0) inv = rcpFast(len); else inv = 1.0f / len;
    origin.x = origin.x + (d0.x * inv) * bias; origin.y = origin.y + (d0.y * inv) * bias;
    origin.z = origin.z + (d0.z * inv) * bias;
    r.o = origin; r.tmax = 1.0f; r.d = sub3(L, origin);
    if (__builtin_amdgcn_ballot_w64(!(rcpInRange(r.d.x) && rcpInRange(r.d.y) && rcpInRange(r.d.z))) == 0)
        r.inv = F3{ rcpFast(r.d.x), rcpFast(r.d.y), rcpFast(r.d.z) };
    else
        r.inv = F3{ 1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z };   // comp:77
    return r;
}

// What an AO kernel does in front of its sample loop, softPrologue's arrangement with the NORMAL as the texel that decides:
// - the normal and the active byte are requested in one batch; a pixel sends rays where it is owned, marked and not background;
// - an owned pixel that sends none gets its zero HERE (`stores`: in the 4-wave form only wave 0 writes the tile);
// - a lane that is not live stands in for the first one that is, by its 32-bit pixel index: the kernels fetch position and normal by
//   that index, so the stand-in sets up that lane's very rays (the same frame, the same hashed start) and discards the result;
// - the POSITION of a pixel that sends no ray is never requested.
// -> false: no lane of the wave sends a ray (the same answer in the four waves of a tile); no ray is set up.
struct AoPixel { bool live; uint32_t pix; };
__device__ __forceinline__ bool aoPrologue(const TraceParams& p, bool owns, uint32_t pix, bool stores, AoPixel* d) {
    // (no branch around the requests: a lane without a pixel asks for texel 0 and byte 0 and never looks at them)
    const f32x4 n = __builtin_nontemporal_load(aoNormals(p) + (owns ? pix : 0u));
    uint8_t act = 1;
    if (p.activeMap) act = __builtin_nontemporal_load(p.activeMap + (owns ? pix : 0u));
    d->live = owns && act != 0 && !(n.x == 0.0f && n.y == 0.0f && n.z == 0.0f);
    if (owns && !d->live && stores) __builtin_nontemporal_store((uint8_t)0, &p.mask[pix]);
    const uint64_t walkers = __builtin_amdgcn_ballot_w64(d->live);
    if (walkers == 0) return false;
    const uint32_t sp = (uint32_t)__builtin_amdgcn_readlane((int)pix, __builtin_ctzll(walkers));
    d->pix = d->live ? pix : sp;
    return true;
}

// The ray of (pixel, sample j): the frame and L from the shared source, then the point light's set-up at L.
// Position and normal are fetched HERE, per sample, by the pixel index (of a live pixel, always): 32 bytes a lane that hit in the
// cache a sample ago, against seven registers held across every walk -- the packet forms compile for 64 VGPRs.
__device__ __forceinline__ Ray makeAoRay(const TraceParams& p, uint32_t pix, uint32_t j) {
    const f32x4 t = *((const f32x4*)p.positions + pix);
    const f32x4 n = *(aoNormals(p) + pix);
    const rts_harness::V3 N{ n.x, n.y, n.z }, rel{ t.x, t.y, t.z };
    const rts_harness::AoFrame f = rts_harness::aoFrame(N);
    const rts_harness::V3 L = rts_harness::aoAim(rts_harness::V3{ p.cam[0], p.cam[1], p.cam[2] }, rel, N, f,
                                                p.offsets[sampleIndex(p, j, pix)], p.light[0]);
    return makePointRayAt(p, F3{ t.x, t.y, t.z }, F3{ L.x, L.y, L.z });
}

// Lane per ray: shadowSoftDistanceShareKernel's 16 x 16 block, the samples one after the other around the any-hit walk.  The four
// waves share nothing but the LDS each owns a quarter of, so each decides for its own 8 x 8 quarter.
__global__ __launch_bounds__(256) void ambientOcclusionShareKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][64];       // lane numbers exchanged by traverseShare (256 B per wave)
    uint32_t* lds = shareSlots[threadIdx.x >> 6];
    uint32_t x, y;
    if (!blockPixel(p, &x, &y)) return;
    AoPixel d;
    if (!aoPrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, true, &d)) return;
    const NodeStream bvh = openStream(p);
    uint32_t lit = 0;
    for (uint32_t j = 0; j < p.nsamples; ++j) {
        const Ray r = makeAoRay(p, d.pix, j);
        const bool occluded = shareAnyHit(p, bvh, r, d.live, d.live && !raySafe(r), lds);
        lit += (d.live && !occluded) ? 1u : 0u;                          // comp:148, per sample
    }
    if (d.live) __builtin_nontemporal_store((uint8_t)lit, &p.mask[d.pix]);   // comp:150
}

// Stackless packet over 8 x 8 tiles, traversePacket<1, false> once per sample (any-hit, the early-out kept).  GEOM as in
// shadowSoftDistancePacketKernel (1: a row range on a 2-D grid, 2: one stripe of power-of-two bands, 0: every other geometry).
// SPLIT 1: one wave walks every sample.  SPLIT 4: four waves per tile, wave w takes the samples w, w + 4, ...; wave 0 adds the four
// counts and stores after ONE workgroup barrier.  Every wave reaches that barrier or none does: the only exits in front of it (a
// block outside the dispatch, a tile without an active non-background pixel) depend on the tile alone, which the four waves share; a
// wave that owns no sample (nsamples < 4) runs no walk and contributes 0.
// A wave keeps its count in LDS (each lane its own word, so no ordering question arises), not in a register across the walk; in the
// 4-wave form these are the very words wave 0 adds.
template <int SPLIT, int GEOM>
__global__ __launch_bounds__(64 * SPLIT) __attribute__((amdgpu_waves_per_eu(8)))
void ambientOcclusionPacketKernel(TraceParams p) {
    static_assert(SPLIT == 1 || SPLIT == 4, "one wave per tile, or four that deal its samples");
    __shared__ uint32_t shareSlots[SPLIT][64];
    __shared__ uint32_t partial[SPLIT][64];                              // per wave: unoccluded samples per lane
    uint32_t bx, by, x, y;
    if (!tileBlock<GEOM>(p, &bx, &by)) return;
    const uint32_t wave = tileWave<SPLIT>();
    tilePixel<GEOM>(p, bx, by, &x, &y);
    AoPixel d;
    if (!aoPrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, wave == 0, &d)) return;
    const NodeStream bvh = openStream(p);
    partial[wave][freshLaneId()] = 0;
    for (uint32_t j = wave; j < p.nsamples; j += SPLIT) {
        // (the pixel index is made opaque per sample: otherwise the compiler hoists the sample-independent part of the set-up --
        //  texel, frame, origin, bias -- out of the loop and keeps it in registers across the walk: rts_soft_distance.inc)
        asm volatile("" : "+v"(d.pix));
        const Ray r[1] = { makeAoRay(p, d.pix, j) };
        const bool walks[1] = { d.live };
        bool occluded[1];
        traversePacket<1, false>(p, bvh, r, walks, occluded, shareSlots[wave]);
        partial[wave][freshLaneId()] += (walks[0] && !occluded[0]) ? 1u : 0u;   // comp:148, per sample
    }
    if constexpr (SPLIT > 1) {
        __syncthreads();
        if (wave != 0) return;
    }
    const uint32_t l = freshLaneId();
    uint32_t lit = 0;
#pragma unroll
    for (int w = 0; w < SPLIT; ++w) lit += partial[w][l];
    if (d.live) __builtin_nontemporal_store((uint8_t)lit, &p.mask[d.pix]);       // comp:150
}

hipError_t launchAmbientOcclusion(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.distance || !p.mask || p.nsamples < 1 || p.nsamples > 48 || p.lightTable > 64 || (p.lightTable && p.lightTable < p.nsamples))
        return hipErrorInvalidValue;
    static const char* const names[2][3] = RTS_PACKET_NAMES("ambientOcclusionPacketKernel", "");
    return launchLoopFamily(variant, p, stream, name, ambientOcclusionShareKernel, "ambientOcclusionShareKernel", names,
                            [&](dim3 grid, auto split, auto geom) {
        constexpr int SPLIT = decltype(split)::value, GEOM = decltype(geom)::value;
        hipLaunchKernelGGL((ambientOcclusionPacketKernel<SPLIT, GEOM>), grid, dim3(64 * SPLIT), 0, stream, p); });
}
