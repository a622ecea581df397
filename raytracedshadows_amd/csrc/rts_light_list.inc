// LIGHT LISTS (rts_trace_light_list*, include/rts.h): included by rts_distance.inc after the soft-distance kernels.  From the common
// part (rts_block_common.inc): tileBlock, tilePixel, blockPixel, tileWave, standInTexel, shareAnyHit, launchLoopFamily.
//
// Up to 8 hard lights in one dispatch: bit l of mask[p] = the byte the mask trace writes at p for light l alone, where bit l of the
// pixel's byte of the light map is set (no map: everywhere), else 0.  p.nsamples is the number of lights, light l travels in
// p.offsets[l] = {x, y, z, 0.0f directional / 1.0f point}, the map in p.activeMap.  A bit is a function of (pixel, light) alone, and
// bits are joined by an integer OR -- associative, commutative, idempotent --, so the byte does not depend on the order the lights
// are walked in, nor on which wave walked which: the 4-wave form ORs the waves' bytes in LDS (DESIGN.md 4.14).

// The ray of (pixel, light l), bit for bit the ray makeShadowRay sets up for the hard light {type, 1 sample, xyz} alone: its general
// set-up restated with the light taken from p.offsets[l] AS GIVEN (a light is not carried as p.light + offsets[j]: 0 + (-0) is +0, and
// a directional light's d is the light itself).  The general set-up and makeShadowRay's fast path give the same bits wherever both
// apply (tests/test_ray_setup.py), and so do rcpFast and the division in rcpFast's range; the choices between them are made per wave.
__device__ __forceinline__ Ray makeListRay(const TraceParams& p, F3 rel, uint32_t l) {
    const F3 L{ p.offsets[l][0], p.offsets[l][1], p.offsets[l][2] };
    F3 origin{ p.cam[0] + rel.x, p.cam[1] + rel.y, p.cam[2] + rel.z };
    float mo = gmax(gmax(__builtin_fabsf(origin.x), __builtin_fabsf(origin.y)), __builtin_fabsf(origin.z));
    float mr = gmax(gmax(__builtin_fabsf(rel.x), __builtin_fabsf(rel.y)), __builtin_fabsf(rel.z));
    float bias = gmax(epsilonFor(mo, 13), epsilonFor(mr, 13));
    Ray r;
    if (p.offsets[l][3] == 0.0f) {                                       // (wave-uniform: l is)
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

// What a lane knows of its pixel.  bits: the lights that send a ray from it -- the map's byte (0xFF without a map) below bit
// p.nsamples, 0 where the lane owns no pixel; pix is only looked at where the lane owns one.
struct ListPixel { bool owns; uint32_t pix; uint32_t bits; F3 rel; };

// The texel and the map's byte are requested in one batch (softPrologue).  -> false: no pixel of the wave's tile has a bit
// below p.nsamples; the zeros are stored (`stores`: in the 4-wave form every wave looks at the same tile and only wave 0 writes it)
// and the wave leaves before the stream is opened.  The same answer in the four waves of a tile.
__device__ __forceinline__ bool lightListPrologue(const TraceParams& p, bool owns, uint32_t pix, bool stores, ListPixel* d) {
    // (no branch around the requests: a lane without a pixel asks for texel 0 and byte 0 and never looks at them)
    const f32x4 t = __builtin_nontemporal_load((const f32x4*)p.positions + (owns ? pix : 0u));          // comp:135
    uint32_t byte = 0xFFu;
    if (p.activeMap) byte = __builtin_nontemporal_load(p.activeMap + (owns ? pix : 0u));
    d->owns = owns;
    d->pix = pix;
    d->bits = owns ? (byte & ((1u << p.nsamples) - 1u)) : 0u;            // (p.nsamples <= 8; bits >= count are 0 whatever the map holds)
    d->rel = F3{ t.x, t.y, t.z };
    if (__builtin_amdgcn_ballot_w64(d->bits != 0u) != 0) return true;
    if (owns && stores) __builtin_nontemporal_store((uint8_t)0, &p.mask[pix]);
    return false;
}

// Lane per ray: shadowMaskActiveShareKernel's 16 x 16 block, the lights one after the other around traverseShare.  The four waves
// share nothing but the LDS each owns a quarter of, so each decides for itself.
__global__ __launch_bounds__(256) void shadowLightListShareKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][64];       // lane numbers exchanged by traverseShare (256 B per wave)
    uint32_t* lds = shareSlots[threadIdx.x >> 6];
    uint32_t x, y;
    if (!blockPixel(p, &x, &y)) return;
    ListPixel d;
    if (!lightListPrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, true, &d)) return;
    const NodeStream bvh = openStream(p);
    uint32_t byte = 0;
    for (uint32_t l = 0; l < p.nsamples; ++l) {
        const bool walks = ((d.bits >> l) & 1u) != 0u;
        const uint64_t walkers = __builtin_amdgcn_ballot_w64(walks);
        if (walkers == 0) continue;                                      // the cull's gain: no ray of this light is set up
        const Ray r = makeListRay(p, standInTexel(d.rel, walks, walkers), l);   // (lanes that do not walk light l stand in)
        const bool occluded = shareAnyHit(p, bvh, r, walks, walks && !raySafe(r), lds);
        byte |= (walks && !occluded) ? (1u << l) : 0u;                   // comp:148, as light l's bit
    }
    if (d.owns) __builtin_nontemporal_store((uint8_t)byte, &p.mask[d.pix]);   // comp:150
}

// Stackless packet over 8 x 8 tiles, traversePacket<1, false> once per light (any-hit, the early-out kept).  GEOM as in
// shadowSoftDistancePacketKernel (1: a row range on a 2-D grid, 2: one stripe of power-of-two bands, 0: every other geometry).
// SPLIT 1: one wave walks every light.  SPLIT 4: four waves per tile, wave w takes the lights w and w + 4; each wave keeps its byte
// in an LDS word of its own per lane, and after ONE workgroup barrier wave 0 ORs the four words and stores.  Every wave reaches
// that barrier or none does: the only exits in front of it (a block outside the dispatch, a tile with no bit below the count in any
// pixel) depend on the tile alone, which the four waves share; a wave that owns no light, or whose lights have no pixel in the
// tile, runs no walk and contributes 0.
template <int SPLIT, int GEOM>
__global__ __launch_bounds__(64 * SPLIT) __attribute__((amdgpu_waves_per_eu(8)))
void shadowLightListPacketKernel(TraceParams p) {
    static_assert(SPLIT == 1 || SPLIT == 4, "one wave per tile, or four that deal its lights");
    __shared__ uint32_t shareSlots[SPLIT][64];
    __shared__ uint32_t partial[SPLIT][64];                              // per wave: its lights' bits per lane
    uint32_t bx, by, x, y;
    if (!tileBlock<GEOM>(p, &bx, &by)) return;
    const uint32_t wave = tileWave<SPLIT>();
    tilePixel<GEOM>(p, bx, by, &x, &y);
    ListPixel d;
    if (!lightListPrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, wave == 0, &d)) return;
    const NodeStream bvh = openStream(p);
    // (LDS is addressed by laneId(), the number the walks themselves keep; the byte lives there, not in a register across the walk)
    uint32_t* const mine = &partial[wave][laneId()];
    *mine = 0;
    for (uint32_t l = wave; l < p.nsamples; l += SPLIT) {
        const bool walks[1] = { ((d.bits >> l) & 1u) != 0u };
        const uint64_t walkers = __builtin_amdgcn_ballot_w64(walks[0]);
        if (walkers == 0) continue;                                      // the cull's gain, wave-uniform: no ray of this light is set up
        F3 rel = standInTexel(d.rel, walks[0], walkers);
        // (made opaque per light: otherwise the compiler hoists the light-independent half of the set-up out of the loop and keeps
        //  it in registers across the walk -- rts_soft_distance.inc)
        asm volatile("" : "+v"(rel.x), "+v"(rel.y), "+v"(rel.z));
        const Ray r[1] = { makeListRay(p, rel, l) };
        bool occluded[1];
        traversePacket<1, false>(p, bvh, r, walks, occluded, shareSlots[wave]);
        *mine |= (walks[0] && !occluded[0]) ? (1u << l) : 0u;            // comp:148, as light l's bit
    }
    uint32_t byte;
    if constexpr (SPLIT > 1) {
        __syncthreads();
        if (wave != 0) return;
        const uint32_t ln = laneId();
        byte = 0;
#pragma unroll
        for (int w = 0; w < SPLIT; ++w) byte |= partial[w][ln];
    } else byte = *mine;
    if (d.owns) __builtin_nontemporal_store((uint8_t)byte, &p.mask[d.pix]);   // comp:150
}

hipError_t launchShadowLightList(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.mask || p.nsamples < 1 || p.nsamples > 8) return hipErrorInvalidValue;
    static const char* const names[2][3] = RTS_PACKET_NAMES("shadowLightListPacketKernel", "");
    return launchLoopFamily(variant, p, stream, name, shadowLightListShareKernel, "shadowLightListShareKernel", names,
                            [&](dim3 grid, auto split, auto geom) {
        constexpr int SPLIT = decltype(split)::value, GEOM = decltype(geom)::value;
        hipLaunchKernelGGL((shadowLightListPacketKernel<SPLIT, GEOM>), grid, dim3(64 * SPLIT), 0, stream, p); });
}
