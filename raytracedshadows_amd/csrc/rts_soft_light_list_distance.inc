// SOFT LIGHT LIST DISTANCE (rts_trace_soft_light_list_distance*, include/rts.h): included by rts_distance.inc after the adaptive soft
// light list kernels.  From the common part (rts_block_common.inc): DIST_NONE, tileBlock, tilePixel, blockPixel, tileWave, freshLaneId,
// standInTexel, launchLoopFamily; from rts_distance.inc: shareDistance, traversePacketDistance; from the light lists
// (rts_light_list.inc): ListPixel, lightListPrologue; from the soft light lists (rts_soft_light_list.inc): makeSoftListRay,
// softListSamples, softListPlane, SOFT_LIST_SLOT.
//
// A soft light list (DESIGN.md 4.17) with a DISTANCE PLANE per light beside its count plane: distance plane l at pixel p = the float
// the soft distance trace writes at p for light l alone -- the minimum over that light's samples of the one-ray distance --, where bit
// l of the pixel's byte of the light map is set (no map: everywhere), else +0; count plane l = the soft light list's byte, the number
// of samples whose distance is +Inf.  The list travels as in rts_soft_light_list.h, the distance planes in p.distance, the count planes
// in p.mask (nullable, wave-uniform).  Every one-ray distance is a bit pattern >= +0 whose unsigned order is the float order, so a
// light's minimum is an integer minimum per (pixel, light) and its count an integer sum: neither depends on the order the pairs are
// walked in, nor on which wave walked which (DESIGN.md 4.20).

// Plane l of the distances: W * H floats each, 64-bit (8 planes of 2^31 pixels).
__device__ __forceinline__ float* softListDistancePlane(const TraceParams& p, uint32_t l) {
    return p.distance + (uint64_t)l * ((uint64_t)p.W * p.H);
}

// lightListPrologue with the zeros of a tile that has no bit below the count stored to all `count` planes of BOTH outputs by the
// storing wave.  -> false: the wave leaves before the stream is opened.  The same answer in the four waves of a tile.
__device__ __forceinline__ bool softListDistancePrologue(const TraceParams& p, bool owns, uint32_t pix, bool stores, ListPixel* d) {
    if (lightListPrologue(p, owns, pix, false, d)) return true;
    if (owns && stores)
        for (uint32_t l = 0; l < p.nsamples; ++l) {
            __builtin_nontemporal_store(0.0f, softListDistancePlane(p, l) + pix);
            if (p.mask) __builtin_nontemporal_store((uint8_t)0, softListPlane(p, l) + pix);
        }
    return false;
}

// Lane per ray: shadowSoftLightListShareKernel's 16 x 16 block, lights in order and samples in order around shareDistance, every
// sample's minimum starting at +Inf.  A light's minimum and count are stored as soon as its samples are done, so only one pair of
// accumulators lives across a walk.  (A lane that does not walk light l comes back from the walk with +Inf: it is counted nowhere
// and stores +0 / 0.)
__global__ __launch_bounds__(256) void shadowSoftLightListDistanceShareKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][2][64];    // per wave: lane numbers exchanged by the walk, and the owners' minima
    uint32_t* lds = shareSlots[threadIdx.x >> 6][0];
    uint32_t* ldsMin = shareSlots[threadIdx.x >> 6][1];
    uint32_t x, y;
    if (!blockPixel(p, &x, &y)) return;
    ListPixel d;
    if (!softListDistancePrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, true, &d)) return;
    const NodeStream bvh = openStream(p);
    for (uint32_t l = 0; l < p.nsamples; ++l) {
        const bool walks = ((d.bits >> l) & 1u) != 0u;
        const uint64_t walkers = __builtin_amdgcn_ballot_w64(walks);
        uint32_t best = DIST_NONE, lit = 0;
        if (walkers != 0) {                                              // the cull's gain: else no ray of this light is set up
            const uint32_t n = softListSamples(p, l);
            for (uint32_t j = 0; j < n; ++j) {
                // (the stand-in is taken per sample and made opaque: else the sample-independent half of the set-up is hoisted out
                //  of the loop and kept in registers across the walk beside the texel itself -- rts_soft_distance.inc)
                F3 rel = standInTexel(d.rel, walks, walkers);            // (lanes that do not walk light l stand in)
                asm volatile("" : "+v"(rel.x), "+v"(rel.y), "+v"(rel.z));
                const Ray r = makeSoftListRay(p, rel, l, j);
                const uint32_t one = shareDistance(p, bvh, r, walks, walks && !raySafe(r), lds, ldsMin);
                lit += (walks && one == DIST_NONE) ? 1u : 0u;            // comp:148, per sample
                best = one < best ? one : best;
            }
        }
        if (d.owns) {
            __builtin_nontemporal_store(walks ? __uint_as_float(best) : 0.0f, softListDistancePlane(p, l) + d.pix);
            if (p.mask) __builtin_nontemporal_store((uint8_t)lit, softListPlane(p, l) + d.pix);   // comp:150
        }
    }
}

// Stackless packet over 8 x 8 tiles, traversePacketDistance once per (light, sample) pair.  GEOM as in shadowSoftDistancePacketKernel
// (1: a row range on a 2-D grid, 2: one stripe of power-of-two bands, 0: every other geometry).  The pairs are numbered in list order
// and wave w of SPLIT takes the pairs r = w, w + SPLIT, ..., exactly as shadowSoftLightListPacketKernel deals them, the one-move step
// over a culled light included.
// A wave keeps per lane, in LDS and not in registers across a walk, ten words: the minimum of light l in word l (+Inf to begin with;
// only the first `count` are initialised and read), and in words 8 and 9 the packed counts of the soft light lists (light l in byte
// l & 3 of word 8 + (l >> 2)).  A count byte holds at most 48, also summed over the waves, so a packed add never carries.
// SPLIT 4: after ONE workgroup barrier wave 0 folds the four waves' words -- an integer minimum per light, packed adds for the counts --
// and stores the planes.  Every wave reaches that barrier or none does: the only exits in front of it (a block outside the dispatch,
// a tile with no bit below the count in any pixel) depend on the tile alone, which the four waves share; a wave that owns no pair, or
// whose pairs' lights have no pixel in the tile, runs no walk, contributes +Inf / 0 and still reaches the barrier.
template <int SPLIT, int GEOM>
__global__ __launch_bounds__(64 * SPLIT) __attribute__((amdgpu_waves_per_eu(8)))
void shadowSoftLightListDistancePacketKernel(TraceParams p) {
    static_assert(SPLIT == 1 || SPLIT == 4, "one wave per tile, or four that deal its pairs");
    __shared__ uint32_t shareSlots[SPLIT][2][64];
    __shared__ uint32_t partial[SPLIT][10][64];                          // per wave: 8 minima and 2 words of packed counts per lane
    uint32_t bx, by, x, y;
    if (!tileBlock<GEOM>(p, &bx, &by)) return;
    const uint32_t wave = tileWave<SPLIT>();
    tilePixel<GEOM>(p, bx, by, &x, &y);
    ListPixel d;
    if (!softListDistancePrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, wave == 0, &d)) return;
    const NodeStream bvh = openStream(p);
    const uint32_t pix = d.owns ? d.pix : 0xFFFFFFFFu;                   // (one register across the walks for both; a dispatch has at most 2^31 pixels)
    {
        const uint32_t ln = freshLaneId();
        for (uint32_t k = 0; k < p.nsamples; ++k) partial[wave][k][ln] = DIST_NONE;
        partial[wave][8][ln] = 0; partial[wave][9][ln] = 0;
    }
    uint32_t l = 0, j = wave;
    for (;;) {
        uint32_t n = 0;
        while (l < p.nsamples && j >= (n = softListSamples(p, l))) { j -= n; ++l; }      // (n >= 1: it ends)
        if (l >= p.nsamples) break;
        const bool walks = ((d.bits >> l) & 1u) != 0u;
        const uint64_t walkers = __builtin_amdgcn_ballot_w64(walks);
        if (walkers == 0) {                                              // the cull's gain, wave-uniform: on to the wave's first pair
            j += ((n - j + (uint32_t)SPLIT - 1u) / (uint32_t)SPLIT) * (uint32_t)SPLIT;   // past this light, and no ray of it is set up
            continue;
        }
        F3 rel = standInTexel(d.rel, walks, walkers);
        // (made opaque per pair: otherwise the compiler hoists the pair-independent half of the set-up out of the loop and keeps it
        //  in registers across the walk -- rts_soft_distance.inc)
        asm volatile("" : "+v"(rel.x), "+v"(rel.y), "+v"(rel.z));
        const Ray r = makeSoftListRay(p, rel, l, j);
        // (a lane that does not walk light l is no member of the packet and comes back with +Inf)
        const uint32_t one = traversePacketDistance(p, bvh, r, walks, shareSlots[wave][0], shareSlots[wave][1]);
        const uint32_t ln = freshLaneId();
        const uint32_t m = partial[wave][l][ln];
        partial[wave][l][ln] = one < m ? one : m;
        partial[wave][8u + (l >> 2)][ln] += (walks && one == DIST_NONE) ? (1u << ((l & 3u) * 8u)) : 0u;   // comp:148, per sample
        j += (uint32_t)SPLIT;
    }
    if constexpr (SPLIT > 1) {
        __syncthreads();
        if (wave != 0) return;
    }
    if (pix == 0xFFFFFFFFu) return;
    const uint32_t ln = freshLaneId();
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int w = 0; w < SPLIT; ++w) { lo += partial[w][8][ln]; hi += partial[w][9][ln]; }
    for (uint32_t k = 0; k < p.nsamples; ++k) {
        uint32_t best = DIST_NONE;
#pragma unroll
        for (int w = 0; w < SPLIT; ++w) {
            const uint32_t m = partial[w][k][ln];
            best = m < best ? m : best;
        }
        __builtin_nontemporal_store(((d.bits >> k) & 1u) != 0u ? __uint_as_float(best) : 0.0f, softListDistancePlane(p, k) + pix);
        if (p.mask) {
            const uint32_t word = k < 4u ? lo : hi;
            __builtin_nontemporal_store((uint8_t)(word >> ((k & 3u) * 8u)), softListPlane(p, k) + pix);   // comp:150
        }
    }
}

hipError_t launchShadowSoftLightListDistance(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.distance || !softListSlotsOk(p.offsets, p.nsamples, false, false)) return hipErrorInvalidValue;
    static const char* const names[2][3] = RTS_PACKET_NAMES("shadowSoftLightListDistancePacketKernel", "");
    return launchLoopFamily(variant, p, stream, name, shadowSoftLightListDistanceShareKernel, "shadowSoftLightListDistanceShareKernel", names,
                            [&](dim3 grid, auto split, auto geom) {
        constexpr int SPLIT = decltype(split)::value, GEOM = decltype(geom)::value;
        hipLaunchKernelGGL((shadowSoftLightListDistancePacketKernel<SPLIT, GEOM>), grid, dim3(64 * SPLIT), 0, stream, p); });
}
