// SOFT LIGHT LISTS (rts_trace_soft_light_list*, include/rts.h): included by rts_distance.inc after the adaptive kernels.  From the
// common part (rts_block_common.inc): tileBlock, tilePixel, blockPixel, tileWave, freshLaneId, standInTexel, shareAnyHit,
// launchLoopFamily; from the light lists (rts_light_list.inc): ListPixel, lightListPrologue.
//
// Up to 8 lights, each hard or soft, in one dispatch, a COUNT PLANE per light: plane l at pixel p = the byte the soft mask trace
// writes at p for light l alone -- the number of unoccluded samples --, where bit l of the pixel's byte of the light map is set (no
// map: everywhere), else 0.  p.nsamples is the number of lights; the shared sample table and the lights travel in p.offsets
// (rts_soft_light_list.h: the slots), the map in p.activeMap, the planes in p.mask.  A count is a sum of bytes that are functions of
// (pixel, light, sample) alone, and integer addition is associative and commutative, so a plane does not depend on the order the
// pairs are walked in, nor on which wave walked which: the 4-wave form adds the waves' counts in LDS (DESIGN.md 4.17).

// SOFT_LIST_SLOT, the slots' writers and the guard of every launcher below, softListSlotsOk: a header of its own with its own
// namespace, so rts_kernels.hip's is closed around it.
} // namespace rts
#include "rts_soft_list_slots.h"
namespace rts {

// samples of light l: 1 (a hard entry) .. 48.  Wave-uniform like l: a scalar load from the argument block.
__device__ __forceinline__ uint32_t softListSamples(const TraceParams& p, uint32_t l) {
    return __float_as_uint(p.offsets[SOFT_LIST_SLOT + 2u * l + 1u][1]);
}

// The ray of (pixel, light l, sample j), bit for bit the ray the soft mask kernels set up for the derived light of include/rts.h
// alone: makeShadowRay's general set-up restated (as makeListRay restates it for a hard light) with
//   L = xyz + radius * offsets[first + j]   for a soft entry -- the product ONE rounded multiply per component (the kernels are built
//                                           without FMA contraction), then makeShadowRay's own add;
//   L = xyz AS GIVEN                        for a hard entry (makeShadowRay adds no offset to a light of one sample: 0 + (-0) is +0).
// The choices between rcpFast and the division are made per wave, as there.
// AT (the jittered lists, rts_soft_light_list_adaptive.inc): j is the entry of the shared table itself, first + sampleIndexOf(...),
// and may differ from lane to lane; the launcher has checked that the light's whole table lies below SOFT_LIST_SLOT.
template <bool AT = false>
__device__ __forceinline__ Ray makeSoftListRay(const TraceParams& p, F3 rel, uint32_t l, uint32_t j) {
    const float* const e = p.offsets[SOFT_LIST_SLOT + 2u * l];         // { x, y, z, radius }
    const float* const u = p.offsets[SOFT_LIST_SLOT + 2u * l + 1u];    // bit patterns of { type, samples, first, 0 }
    F3 L{ e[0], e[1], e[2] };
    if (__float_as_uint(u[1]) > 1u) {                                    // (wave-uniform: l is)
        const float radius = e[3];
        const float* const o = p.offsets[AT ? j : __float_as_uint(u[2]) + j];
        L.x = L.x + radius * o[0]; L.y = L.y + radius * o[1]; L.z = L.z + radius * o[2];
    }
    F3 origin{ p.cam[0] + rel.x, p.cam[1] + rel.y, p.cam[2] + rel.z };
    float mo = gmax(gmax(__builtin_fabsf(origin.x), __builtin_fabsf(origin.y)), __builtin_fabsf(origin.z));
    float mr = gmax(gmax(__builtin_fabsf(rel.x), __builtin_fabsf(rel.y)), __builtin_fabsf(rel.z));
    float bias = gmax(epsilonFor(mo, 13), epsilonFor(mr, 13));
    Ray r;
    if (__float_as_uint(u[0]) == 0u) {                                   // RTS_LIGHT_DIRECTIONAL
        origin.x = origin.x + L.x * bias; origin.y = origin.y + L.y * bias; origin.z = origin.z + L.z * bias;
        r.o = origin; r.tmax = 1e9f; r.d = L;
    } else {
        F3 d0 = sub3(L, origin);
        const float len = __builtin_sqrtf(dot3(d0, d0));
        float inv;
        if (__builtin_amdgcn_ballot_w64(!rcpInRange(len)) == 0) inv = rcpFast(len); else inv = 1.0f / len;
        origin.x = origin.x + (d0.x * inv) * bias; origin.y = origin.y + (d0.y * inv) * bias;
        origin.z = origin.z + (d0.z * inv) * bias;
        r.o = origin; r.tmax = 1.0f; r.d = sub3(L, origin);
    }
    if (__builtin_amdgcn_ballot_w64(!(rcpInRange(r.d.x) && rcpInRange(r.d.y) && rcpInRange(r.d.z))) == 0)
        r.inv = F3{ rcpFast(r.d.x), rcpFast(r.d.y), rcpFast(r.d.z) };
    else
        r.inv = F3{ 1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z };   // comp:77
    return r;
}

// Plane l of the counts: W * H bytes each, 64-bit (8 planes of 2^31 pixels).
__device__ __forceinline__ uint8_t* softListPlane(const TraceParams& p, uint32_t l) {
    return p.mask + (uint64_t)l * ((uint64_t)p.W * p.H);
}

// lightListPrologue with the zeros of a tile that has no bit below the count stored to all `count` planes by the storing wave.
// -> false: the wave leaves before the stream is opened.  The same answer in the four waves of a tile.
__device__ __forceinline__ bool softListPrologue(const TraceParams& p, bool owns, uint32_t pix, bool stores, ListPixel* d) {
    if (lightListPrologue(p, owns, pix, false, d)) return true;
    if (owns && stores)
        for (uint32_t l = 0; l < p.nsamples; ++l) __builtin_nontemporal_store((uint8_t)0, softListPlane(p, l) + pix);
    return false;
}

// Lane per ray: shadowLightListShareKernel's 16 x 16 block, lights in order and samples in order around traverseShare.  The four
// waves share nothing but the LDS each owns a quarter of, so each decides for its own 8 x 8 quarter; a light's plane is stored as
// soon as its samples are done, so only one count lives across a walk.
__global__ __launch_bounds__(256) void shadowSoftLightListShareKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][64];       // lane numbers exchanged by traverseShare (256 B per wave)
    uint32_t* lds = shareSlots[threadIdx.x >> 6];
    uint32_t x, y;
    if (!blockPixel(p, &x, &y)) return;
    ListPixel d;
    if (!softListPrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, true, &d)) return;
    const NodeStream bvh = openStream(p);
    for (uint32_t l = 0; l < p.nsamples; ++l) {
        const bool walks = ((d.bits >> l) & 1u) != 0u;
        const uint64_t walkers = __builtin_amdgcn_ballot_w64(walks);
        uint32_t count = 0;
        if (walkers != 0) {                                              // the cull's gain: else no ray of this light is set up
            const F3 rel = standInTexel(d.rel, walks, walkers);          // (lanes that do not walk light l stand in)
            const uint32_t n = softListSamples(p, l);
            for (uint32_t j = 0; j < n; ++j) {
                const Ray r = makeSoftListRay(p, rel, l, j);
                const bool occluded = shareAnyHit(p, bvh, r, walks, walks && !raySafe(r), lds);
                count += (walks && !occluded) ? 1u : 0u;                 // comp:148, per sample
            }
        }
        if (d.owns) __builtin_nontemporal_store((uint8_t)count, softListPlane(p, l) + d.pix);   // comp:150
    }
}

// Stackless packet over 8 x 8 tiles, traversePacket<1, false> once per (light, sample) pair (any-hit, the early-out kept).  GEOM as in
// shadowSoftDistancePacketKernel (1: a row range on a 2-D grid, 2: one stripe of power-of-two bands, 0: every other geometry).
// The pairs of the list are numbered in list order -- light 0's samples, then light 1's, ... -- and wave w of SPLIT takes the pairs
// r = w, w + SPLIT, ...: with SPLIT 1 one wave walks the lights in order and the samples in order, with SPLIT 4 a list of many small
// lights and a list of one large light both keep four waves busy.  (l, j) of the wave's next pair are kept on the scalar unit.
// A wave keeps its counts in LDS, not in registers across a walk: two words per lane, light l in byte l & 3 of word l >> 2.  A byte
// holds at most 48, also summed over the waves, so a packed add never carries into the next byte.
// SPLIT 4: after ONE workgroup barrier wave 0 adds the four waves' words and stores the `count` planes.  Every wave reaches that
// barrier or none does: the only exits in front of it (a block outside the dispatch, a tile with no bit below the count in any
// pixel) depend on the tile alone, which the four waves share; a wave that owns no pair, or whose pairs' lights have no pixel in the
// tile, runs no walk and contributes 0.
template <int SPLIT, int GEOM>
__global__ __launch_bounds__(64 * SPLIT) __attribute__((amdgpu_waves_per_eu(8)))
void shadowSoftLightListPacketKernel(TraceParams p) {
    static_assert(SPLIT == 1 || SPLIT == 4, "one wave per tile, or four that deal its pairs");
    __shared__ uint32_t shareSlots[SPLIT][64];
    __shared__ uint32_t partial[SPLIT][2][64];                           // per wave: its pairs' counts per lane, packed
    uint32_t bx, by, x, y;
    if (!tileBlock<GEOM>(p, &bx, &by)) return;
    const uint32_t wave = tileWave<SPLIT>();
    tilePixel<GEOM>(p, bx, by, &x, &y);
    ListPixel d;
    if (!softListPrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, wave == 0, &d)) return;
    const NodeStream bvh = openStream(p);
    const uint32_t pix = d.owns ? d.pix : 0xFFFFFFFFu;                   // (one register across the walks for both; a dispatch has at most 2^31 pixels)
    {
        const uint32_t ln = freshLaneId();
        partial[wave][0][ln] = 0; partial[wave][1][ln] = 0;
    }
    uint32_t l = 0, j = wave;
    for (;;) {
        uint32_t n = 0;
        while (l < p.nsamples && j >= (n = softListSamples(p, l))) { j -= n; ++l; }      // (n >= 1: it ends)
        if (l >= p.nsamples) break;
        const bool walks[1] = { ((d.bits >> l) & 1u) != 0u };
        const uint64_t walkers = __builtin_amdgcn_ballot_w64(walks[0]);
        if (walkers == 0) {                                              // the cull's gain, wave-uniform: on to the wave's first pair
            j += ((n - j + (uint32_t)SPLIT - 1u) / (uint32_t)SPLIT) * (uint32_t)SPLIT;   // past this light, and no ray of it is set up
            continue;
        }
        F3 rel = standInTexel(d.rel, walks[0], walkers);
        // (made opaque per pair: otherwise the compiler hoists the pair-independent half of the set-up out of the loop and keeps it
        //  in registers across the walk -- rts_soft_distance.inc)
        asm volatile("" : "+v"(rel.x), "+v"(rel.y), "+v"(rel.z));
        const Ray r[1] = { makeSoftListRay(p, rel, l, j) };
        bool occluded[1];
        traversePacket<1, false>(p, bvh, r, walks, occluded, shareSlots[wave]);
        partial[wave][l >> 2][freshLaneId()] += (walks[0] && !occluded[0]) ? (1u << ((l & 3u) * 8u)) : 0u;   // comp:148, per sample
        j += (uint32_t)SPLIT;
    }
    if constexpr (SPLIT > 1) {
        __syncthreads();
        if (wave != 0) return;
    }
    const uint32_t ln = freshLaneId();
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int w = 0; w < SPLIT; ++w) { lo += partial[w][0][ln]; hi += partial[w][1][ln]; }
    if (pix != 0xFFFFFFFFu)
        for (uint32_t k = 0; k < p.nsamples; ++k) {
            const uint32_t word = k < 4u ? lo : hi;
            __builtin_nontemporal_store((uint8_t)(word >> ((k & 3u) * 8u)), softListPlane(p, k) + pix);   // comp:150
        }
}

hipError_t launchShadowSoftLightList(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.mask || !softListSlotsOk(p.offsets, p.nsamples, false, false)) return hipErrorInvalidValue;
    static const char* const names[2][3] = RTS_PACKET_NAMES("shadowSoftLightListPacketKernel", "");
    return launchLoopFamily(variant, p, stream, name, shadowSoftLightListShareKernel, "shadowSoftLightListShareKernel", names,
                            [&](dim3 grid, auto split, auto geom) {
        constexpr int SPLIT = decltype(split)::value, GEOM = decltype(geom)::value;
        hipLaunchKernelGGL((shadowSoftLightListPacketKernel<SPLIT, GEOM>), grid, dim3(64 * SPLIT), 0, stream, p); });
}
