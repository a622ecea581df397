// SOFT-SHADOW OCCLUDER DISTANCE (rts_trace_soft_distance*, include/rts.h): included at the end of rts_distance.inc -- so by
// rts_kernels.hip, inside namespace rts, after every distance kernel -- it adds kernels and changes none.
//
// distance[p] = min over the light's samples j of sample j's one-ray distance (rts_distance.inc), mask[p] = the number of samples
// whose distance is +Inf (the byte the soft mask trace writes).  Every one-ray distance is a bit pattern >= +0 whose integer order
// is the float order, so the minimum over samples is again an integer minimum: it does not depend on the order the samples are
// walked in, nor on which wave walked which -- the per-wave minima of the 4-wave form are joined in LDS by one more integer minimum
// and the counts by an integer sum, like the soft mask kernels' counts.  (A MEAN blocker distance would be a float sum, which has no
// order-free definition: DESIGN.md 4.13.)

// What every soft distance kernel does around its sample loop: distancePrologue's requests and stand-in, arranged so that little
// stays in registers across the walks -- the packet forms compile for 64 VGPRs.
// - A pixel that owns no ray gets its zeros HERE, in front of the walks; from then on a lane is `live` or has nothing to store.
// - One 32-bit pixel index per lane (a dispatch has at most 2^31 pixels): its own where it is live, else the index of the first
//   live lane -- per-pixel jitter hashes it, so a lane without a ray picks the very offsets of the lane it stands in for and sets up
//   the very same ray (shadowMaskActiveShareKernel); exact, since its result is discarded.
// - `stores`: in the 4-wave form every wave looks at the same tile and only wave 0 writes it.
struct SoftPixel { bool live; uint32_t pix; F3 rel; };

// -> false: no lane of the wave sends a ray (the zeros are stored); the same answer in the four waves of a tile.
__device__ __forceinline__ bool softDistancePrologue(const TraceParams& p, bool owns, uint32_t pix, bool stores, SoftPixel* d) {
    // (no branch around the requests: a lane without a pixel asks for texel 0 and byte 0 and never looks at them)
    const f32x4 t = __builtin_nontemporal_load((const f32x4*)p.positions + (owns ? pix : 0u));          // comp:135
    uint8_t act = 1;
    if (p.activeMap) act = __builtin_nontemporal_load(p.activeMap + (owns ? pix : 0u));
    d->live = owns && act != 0;
    if (owns && !d->live && stores) {
        __builtin_nontemporal_store(0.0f, &p.distance[pix]);
        if (p.mask) __builtin_nontemporal_store((uint8_t)0, &p.mask[pix]);
    }
    const uint64_t walkers = __builtin_amdgcn_ballot_w64(d->live);
    if (walkers == 0) return false;
    const int firstWalker = __builtin_ctzll(walkers);
    const float sx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t.x), firstWalker));
    const float sy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t.y), firstWalker));
    const float sz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t.z), firstWalker));
    const uint32_t sp = (uint32_t)__builtin_amdgcn_readlane((int)pix, firstWalker);
    d->rel = d->live ? F3{ t.x, t.y, t.z } : F3{ sx, sy, sz };
    d->pix = d->live ? pix : sp;
    return true;
}
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
    uint32_t bx, by;
    if (!blockToXY(p, blockIdx.x, &bx, &by)) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t x = bx * 16u + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t y = ownedRow(p, by * 16u + (wave >> 1) * 8u + (lane >> 3));
    SoftPixel d;
    if (!softDistancePrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, true, &d)) return;
    const NodeStream bvh = openStream(p);
    uint32_t best = DIST_NONE, lit = 0;
    for (uint32_t s = 0; s < p.nsamples; ++s) {
        const Ray r = makeShadowRay(p, d.rel, s, d.pix);
        const bool unsafe = d.live && !raySafe(r);
        uint32_t one;                                                    // (the walk starts every sample's minimum at +Inf itself)
        if (p.bvhFinite && __builtin_amdgcn_ballot_w64(unsafe) == 0)
            one = traverseShareDistance<true>(bvh, r, d.live, 0u, lds, ldsMin, DIST_NONE);
        else
            one = traverseShareDistance<false>(bvh, r, d.live, 0u, lds, ldsMin, DIST_NONE);
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
    uint32_t bx = blockIdx.x, by = 0;
    if constexpr (GEOM == 0) { if (!blockToXY(p, blockIdx.x, &bx, &by)) return; }
    else by = dispatchRow(p, blockIdx.y);
    // (the wave's number is wave-uniform: said so, the sample counter and the wave's LDS addresses stay on the scalar unit)
    const uint32_t lane = threadIdx.x & 63u, wave = SPLIT > 1 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0u;
    const uint32_t x = bx * 8u + (lane & 7u);
    uint32_t y;
    if constexpr (GEOM == 2) {
        const uint32_t band = by >> p.bandShift, within = by - (band << p.bandShift);
        y = (band * p.nStripes + p.stripe) * p.bandRows + within * 8u + (lane >> 3);
    } else if constexpr (GEOM == 1) y = p.rowBegin + by * 8u + (lane >> 3);
    else y = ownedRow(p, by * 8u + (lane >> 3));
    SoftPixel d;
    if (!softDistancePrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, wave == 0, &d)) return;
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
    // (the lane number is computed AGAIN, from an operand the compiler cannot see through: it would otherwise carry the address from
    //  in front of the loop to here -- in the 4-wave form the one register too many, 8 bytes of scratch)
    uint32_t zero = 0;
    asm volatile("" : "+v"(zero));
    const uint32_t l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));
    uint32_t best = DIST_NONE, lit = 0;
#pragma unroll
    for (int w = 0; w < SPLIT; ++w) {
        const uint32_t m = partial[w][0][l];
        best = m < best ? m : best;
        lit += partial[w][1][l];
    }
    softDistanceStore(p, d, best, lit);
}

template <int SPLIT>
static hipError_t launchSoftDistancePacket(const TraceParams& p, dim3 grid, hipStream_t stream, const char** name) {
    static const char* const names[2][3] = {
        { "shadowSoftDistancePacketKernel<1,general>", "shadowSoftDistancePacketKernel<1,rows>", "shadowSoftDistancePacketKernel<1,bands>" },
        { "shadowSoftDistancePacketKernel<4,general>", "shadowSoftDistancePacketKernel<4,rows>", "shadowSoftDistancePacketKernel<4,bands>" } };
    const int geom = packetGeom(p);                                      // (rts_distance.inc)
    *name = names[SPLIT == 4][geom];
    if (geom == 2) hipLaunchKernelGGL((shadowSoftDistancePacketKernel<SPLIT, 2>), grid, dim3(64 * SPLIT), 0, stream, p);
    else if (geom == 1) hipLaunchKernelGGL((shadowSoftDistancePacketKernel<SPLIT, 1>), grid, dim3(64 * SPLIT), 0, stream, p);
    else hipLaunchKernelGGL((shadowSoftDistancePacketKernel<SPLIT, 0>), grid, dim3(64 * SPLIT), 0, stream, p);
    return hipGetLastError();
}

hipError_t launchShadowSoftDistance(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.distance || p.nsamples < 2 || p.nsamples > 64) return hipErrorInvalidValue;
    const dim3 grid = blockGrid(p);
    if (variant == V_SHARE) {
        *name = "shadowSoftDistanceShareKernel";
        hipLaunchKernelGGL(shadowSoftDistanceShareKernel, grid, dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    if (variant != V_PACKET) return hipErrorInvalidValue;
    return p.softSplit ? launchSoftDistancePacket<4>(p, grid, stream, name) : launchSoftDistancePacket<1>(p, grid, stream, name);
}

// light lists: up to 8 hard lights in one dispatch, one bit per light (its launch is declared in rts_light_list.h)
#include "rts_light_list.inc"
