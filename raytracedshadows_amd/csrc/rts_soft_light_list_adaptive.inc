// ADAPTIVE SOFT LIGHT LISTS (rts_trace_soft_light_list_adaptive*, include/rts.h): included by rts_distance.inc after the soft light
// list kernels.  From the common part (rts_block_common.inc): tileBlock, tilePixel, blockPixel, tileWave, freshLaneId, standInTexel,
// shareAnyHit, launchLoopFamily; from the soft light lists (rts_soft_light_list.inc): softListPrologue, makeSoftListRay,
// softListSamples, softListPlane, SOFT_LIST_SLOT.
//
// A soft light list (DESIGN.md 4.17) with a probe count k_l per light (rts_soft_light_list_adaptive.h: the slots).  With u_j the
// any-hit byte of sample j of light l at the pixel (1 = unoccluded, 0 where the map's bit l is clear), n = the light's samples,
// c_k = u_0 + ... + u_(k-1), c_n = u_0 + ... + u_(n-1):
//   k_l == 0:  plane l = c_n (the soft list trace's byte), bit l of refined = 0;
//   k_l >= 1:  plane l = 0 where c_k == 0, n where c_k == k, c_n otherwise; bit l of refined = 1 exactly in the last case.
// Everything is integer counting of bytes that are functions of (pixel, light, sample) alone, so no byte depends on the order the
// pairs are walked in, nor on which wave walked which (DESIGN.md 4.18).

// k_l: 0 (every sample in the first phase) .. samples - 1.  Wave-uniform like l: a scalar load from the argument block.
__device__ __forceinline__ uint32_t softListProbe(const TraceParams& p, uint32_t l) {
    return __float_as_uint(p.offsets[SOFT_LIST_SLOT + 2u * l + 1u][3]);
}

// JITTERED LISTS (rts_trace_soft_light_list_jittered*): a table size T_l per light (rts_soft_light_list_adaptive.h: the slot).
// T_l == 0: sample j of light l is entry first + j of the shared table for every pixel, as above.  T_l != 0: pixel p takes entry
// first + (start(p) + j) mod T_l, start(p) = (hash32(p) * T_l) >> 32, p the pixel's index in the caller's full frame -- sampleIndex
// (rts_kernels.hip) with T_l in p.lightTable's place, so the ray is the one the mask kernels set up for the derived light with that
// table.  Which pairs are walked over which lanes is decided by k_l, the map and the tile, never by an offset: the counting above
// and the barriers' argument below hold as they stand (DESIGN.md 4.19).
// T_l.  Wave-uniform like l: a scalar load from the argument block.
__device__ __forceinline__ uint32_t softListTable(const TraceParams& p, uint32_t l) {
    return __float_as_uint(p.offsets[l][3]);
}

// The shared table's entry of (light l, sample j) at the pixel `pixel` of this dispatch.  j < n_l <= T_l, so one subtraction wraps.
__device__ __forceinline__ uint32_t softListSampleAt(const TraceParams& p, uint32_t l, uint32_t j, uint32_t pixel) {
    const uint32_t first = __float_as_uint(p.offsets[SOFT_LIST_SLOT + 2u * l + 1u][2]), table = softListTable(p, l);
    if (table == 0u) return first + j;                                   // (wave-uniform: l is)
    const uint32_t at = __umulhi(hash32(pixel + p.pixelBase), table) + j;
    return first + (at >= table ? at - table : at);
}

// standInTexel for the pixel index: a lane that stands in sets up the walker's very ray only if it hashes the walker's pixel.
__device__ __forceinline__ uint32_t standInPixel(uint32_t pix, bool keeps, uint64_t walkers) {
    const uint32_t sp = (uint32_t)__builtin_amdgcn_readlane((int)pix, __builtin_ctzll(walkers));
    return keeps ? pix : sp;
}

// softListPrologue with the refined plane: a tile that has no bit below the count gets its zeros there too.
__device__ __forceinline__ bool softListAdaptivePrologue(const TraceParams& p, bool owns, uint32_t pix, bool stores, ListPixel* d) {
    if (softListPrologue(p, owns, pix, stores, d)) return true;
    if (owns && stores && p.out) __builtin_nontemporal_store((uint8_t)0, &p.out[pix]);
    return false;
}

// Lane per ray: shadowSoftLightListShareKernel's 16 x 16 block, the lights in order: the probe's samples, the decision of the wave's
// own 8 x 8 quarter (the four waves share nothing but the LDS each owns a quarter of), then the remaining samples over the penumbra
// lanes.  A light's plane is stored as soon as the light is done, the refined byte at the end.
// JITTER: the tables are honoured; a stand-in takes the pixel index with the texel, per light and again per penumbra.
template <bool JITTER>
__global__ __launch_bounds__(256) void shadowSoftLightListAdaptiveShareKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][64];       // lane numbers exchanged by traverseShare (256 B per wave)
    uint32_t* lds = shareSlots[threadIdx.x >> 6];
    uint32_t x, y;
    if (!blockPixel(p, &x, &y)) return;
    ListPixel d;
    if (!softListAdaptivePrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, true, &d)) return;
    const NodeStream bvh = openStream(p);
    uint32_t refined = 0;
    for (uint32_t l = 0; l < p.nsamples; ++l) {
        const bool walks = ((d.bits >> l) & 1u) != 0u;
        const uint64_t walkers = __builtin_amdgcn_ballot_w64(walks);
        uint32_t count = 0;
        if (walkers != 0) {                                              // the cull's gain: else no ray of this light is set up
            const uint32_t n = softListSamples(p, l), k = softListProbe(p, l);
            const uint32_t first = k != 0u ? k : n;                      // samples of the first phase
            {
                const F3 rel = standInTexel(d.rel, walks, walkers);      // (lanes that do not walk light l stand in)
                uint32_t px = 0;
                if constexpr (JITTER) px = standInPixel(d.pix, walks, walkers);
                for (uint32_t j = 0; j < first; ++j) {
                    Ray r;
                    if constexpr (JITTER) r = makeSoftListRay<true>(p, rel, l, softListSampleAt(p, l, j, px));
                    else r = makeSoftListRay(p, rel, l, j);
                    const bool occluded = shareAnyHit(p, bvh, r, walks, walks && !raySafe(r), lds);
                    count += (walks && !occluded) ? 1u : 0u;             // comp:148, per sample
                }
            }
            if (k != 0u) {
                const bool pen = count != 0u && count != k;              // (count != 0 only where the lane walks)
                const uint64_t pens = __builtin_amdgcn_ballot_w64(pen);
                if (pens != 0) {                                         // else the quarter's probe was unanimous: no further ray
                    const F3 rel = standInTexel(d.rel, pen, pens);       // (lanes that do not refine light l stand in)
                    uint32_t px = 0;
                    if constexpr (JITTER) px = standInPixel(d.pix, pen, pens);
                    for (uint32_t j = k; j < n; ++j) {
                        Ray r;
                        if constexpr (JITTER) r = makeSoftListRay<true>(p, rel, l, softListSampleAt(p, l, j, px));
                        else r = makeSoftListRay(p, rel, l, j);
                        const bool occluded = shareAnyHit(p, bvh, r, pen, pen && !raySafe(r), lds);
                        count += (pen && !occluded) ? 1u : 0u;
                    }
                }
                if (!pen) count = count != 0u ? n : 0u;                  // unanimous: c_k is 0 or k
                refined |= pen ? (1u << l) : 0u;
            }
        }
        if (d.owns) __builtin_nontemporal_store((uint8_t)count, softListPlane(p, l) + d.pix);   // comp:150
    }
    if (d.owns && p.out) __builtin_nontemporal_store((uint8_t)refined, &p.out[d.pix]);
}

// One phase of a packet wave: the pairs of the phase, numbered in list order, r = wave, wave + SPLIT, ... of them.
//   REFINE false (phase 1): light l has its first k_l samples, or all n_l where k_l == 0;
//   REFINE true  (phase 2): light l has the samples k_l .. n_l - 1, none where k_l == 0.
// bits: per lane, the lights it walks in this phase (the map's byte; the penumbra mask).  A light no lane of the tile walks is
// stepped over before any ray is set up, as the cull does.  The counts go to mine[l >> 2][lane], byte l & 3 (rts_soft_light_list.inc).
// JITTER: pix is the lane's pixel index where it has a bit in `bits` (the kernel keeps it across the walks anyway); a stand-in takes
// the walker's, and the index is made opaque per pair with the texel.
template <int SPLIT, bool REFINE, bool JITTER>
__device__ __forceinline__ void softListAdaptivePhase(const TraceParams& p, const NodeStream& bvh, const F3& texel, uint32_t bits,
                                                      uint32_t wave, uint32_t* share, uint32_t (*mine)[64], uint32_t pix) {
    uint32_t l = 0, j = wave;
    for (;;) {
        uint32_t n = 0, from = 0;
        for (; l < p.nsamples; ++l) {                                    // (every light is passed once: it ends)
            const uint32_t k = softListProbe(p, l), ns = softListSamples(p, l);      // (k < ns: the launcher's check)
            n = REFINE ? (k != 0u ? ns - k : 0u) : (k != 0u ? k : ns);
            from = REFINE ? k : 0u;
            if (j < n) break;
            j -= n;
        }
        if (l >= p.nsamples) break;
        const bool walks[1] = { ((bits >> l) & 1u) != 0u };
        const uint64_t walkers = __builtin_amdgcn_ballot_w64(walks[0]);
        if (walkers == 0) {                                              // wave-uniform: on to the wave's first pair past this light
            j += ((n - j + (uint32_t)SPLIT - 1u) / (uint32_t)SPLIT) * (uint32_t)SPLIT;
            continue;
        }
        F3 rel = standInTexel(texel, walks[0], walkers);
        // (made opaque per pair: otherwise the compiler hoists the pair-independent half of the set-up out of the loop and keeps it
        //  in registers across the walk -- rts_soft_distance.inc)
        asm volatile("" : "+v"(rel.x), "+v"(rel.y), "+v"(rel.z));
        Ray r[1];
        if constexpr (JITTER) {
            uint32_t px = standInPixel(pix, walks[0], walkers);
            asm volatile("" : "+v"(px));
            r[0] = makeSoftListRay<true>(p, rel, l, softListSampleAt(p, l, from + j, px));
        } else r[0] = makeSoftListRay(p, rel, l, from + j);
        bool occluded[1];
        traversePacket<1, false>(p, bvh, r, walks, occluded, share);
        mine[l >> 2][freshLaneId()] += (walks[0] && !occluded[0]) ? (1u << ((l & 3u) * 8u)) : 0u;   // comp:148, per sample
        j += (uint32_t)SPLIT;
    }
}

// The penumbra mask of a lane from its probe counts (lo: lights 0..3, hi: 4..7, a byte each): bit l where k_l != 0 and 0 < c_k < k_l.
// (c_k != 0 only where the lane walked light l, so the map's bit need not be looked at again.)
__device__ __forceinline__ uint32_t softListPenumbra(const TraceParams& p, uint32_t lo, uint32_t hi) {
    uint32_t pen = 0;
    for (uint32_t l = 0; l < p.nsamples; ++l) {
        const uint32_t ck = ((l < 4u ? lo : hi) >> ((l & 3u) * 8u)) & 0xFFu, k = softListProbe(p, l);
        pen |= (k != 0u && ck != 0u && ck != k) ? (1u << l) : 0u;
    }
    return pen;
}

// The storing wave's end: per light the byte of the definition from the probe counts (lo0, hi0) and the refinement's (lo1, hi1).
__device__ __forceinline__ void softListAdaptiveStore(const TraceParams& p, uint32_t pix, uint32_t lo0, uint32_t hi0, uint32_t lo1, uint32_t hi1) {
    if (pix == 0xFFFFFFFFu) return;
    uint32_t pen = 0;
    for (uint32_t l = 0; l < p.nsamples; ++l) {
        const uint32_t shift = (l & 3u) * 8u;
        const uint32_t ck = ((l < 4u ? lo0 : hi0) >> shift) & 0xFFu, rest = ((l < 4u ? lo1 : hi1) >> shift) & 0xFFu;
        const uint32_t k = softListProbe(p, l);
        uint32_t byte = ck;                                              // k == 0: the full count
        if (k != 0u) {
            const bool refines = ck != 0u && ck != k;
            byte = refines ? ck + rest : (ck != 0u ? softListSamples(p, l) : 0u);
            pen |= refines ? (1u << l) : 0u;
        }
        __builtin_nontemporal_store((uint8_t)byte, softListPlane(p, l) + pix);   // comp:150
    }
    if (p.out) __builtin_nontemporal_store((uint8_t)pen, &p.out[pix]);
}

// Stackless packet over 8 x 8 tiles, traversePacket<1, false> once per (light, sample) pair that is walked.  GEOM as in
// shadowSoftDistancePacketKernel (1: a row range on a 2-D grid, 2: one stripe of power-of-two bands, 0: every other geometry).
// SPLIT 4: four waves per tile, which map lane -> pixel identically:
//   phase 1  the pairs (l, j < k_l) -- all of a light's samples where k_l == 0 -- dealt r = w, w + 4, ... over the waves, walked over
//            the lanes the map marks; the counts go to set 0, two words per lane and wave, a byte per light;
//   BARRIER 1; every wave adds the four waves' words of set 0 for its lane and derives `pen`, a bit per light: the same words in the
//            same lanes, so the same mask and the same ballot in the four waves.  No penumbra pixel of any light in the tile: wave 0
//            stores, every wave returns;
//   phase 2  the pairs (l, k_l <= j < n_l) of the lights with k_l != 0, dealt over the waves, walked over the lanes whose `pen` has
//            bit l; a light without such a lane is stepped over.  The counts go to set 1 -- a SECOND set of words, so no wave writes
//            a word that another may still be reading for its c_k;
//   BARRIER 2; wave 0 reads set 0 again (nobody wrote it since barrier 1), adds set 1 and stores planes and refined.
// Every wave reaches each barrier or none does: the exits in front of barrier 1 (a block outside the dispatch, a tile with no bit
// below the count in any pixel) and the one between the barriers (no penumbra bit) depend on the tile alone -- on the geometry, on the
// tile's map bytes and on LDS words all four waves read alike after barrier 1 --, never on the wave.  A wave that owns no pair of a
// phase, or whose pairs' lights have no lane in the tile, runs no walk in it, contributes 0 and still reaches both barriers.
// A byte holds at most 48 summed over BOTH sets and all four waves -- c_k + rest <= n_l <= 48 --, so a packed add never carries into
// the next byte.  SPLIT 1: one wave, the same two loops, no barrier.
// JITTER: the tables are honoured.  They change the offsets alone, so nothing above changes: no barrier is added or moved.
template <int SPLIT, int GEOM, bool JITTER>
__global__ __launch_bounds__(64 * SPLIT) __attribute__((amdgpu_waves_per_eu(8)))
void shadowSoftLightListAdaptivePacketKernel(TraceParams p) {
    static_assert(SPLIT == 1 || SPLIT == 4, "one wave per tile, or four that deal its pairs");
    __shared__ uint32_t shareSlots[SPLIT][64];
    __shared__ uint32_t partial[2][SPLIT][2][64];                        // per phase and wave: its pairs' counts per lane, packed
    uint32_t bx, by, x, y;
    if (!tileBlock<GEOM>(p, &bx, &by)) return;
    const uint32_t wave = tileWave<SPLIT>();
    tilePixel<GEOM>(p, bx, by, &x, &y);
    ListPixel d;
    if (!softListAdaptivePrologue(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, wave == 0, &d)) return;
    const NodeStream bvh = openStream(p);
    const uint32_t pix = d.owns ? d.pix : 0xFFFFFFFFu;                   // (one register across the walks for both; a dispatch has at most 2^31 pixels)
    {
        const uint32_t ln = freshLaneId();
        partial[0][wave][0][ln] = 0; partial[0][wave][1][ln] = 0;
        partial[1][wave][0][ln] = 0; partial[1][wave][1][ln] = 0;
    }
    softListAdaptivePhase<SPLIT, false, JITTER>(p, bvh, d.rel, d.bits, wave, shareSlots[wave], partial[0][wave], pix);
    if constexpr (SPLIT > 1) __syncthreads();                            // BARRIER 1
    uint32_t pen;
    {
        const uint32_t ln = freshLaneId();
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int w = 0; w < SPLIT; ++w) { lo += partial[0][w][0][ln]; hi += partial[0][w][1][ln]; }
        pen = softListPenumbra(p, lo, hi);
        if (__builtin_amdgcn_ballot_w64(pen != 0u) == 0) {               // the same answer in the four waves
            if (wave == 0) softListAdaptiveStore(p, pix, lo, hi, 0u, 0u);
            return;
        }
    }
    softListAdaptivePhase<SPLIT, true, JITTER>(p, bvh, d.rel, pen, wave, shareSlots[wave], partial[1][wave], pix);
    if constexpr (SPLIT > 1) {
        __syncthreads();                                                 // BARRIER 2
        if (wave != 0) return;
    }
    const uint32_t ln = freshLaneId();
    uint32_t lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
#pragma unroll
    for (int w = 0; w < SPLIT; ++w) {
        lo0 += partial[0][w][0][ln]; hi0 += partial[0][w][1][ln];
        lo1 += partial[1][w][0][ln]; hi1 += partial[1][w][1][ln];
    }
    softListAdaptiveStore(p, pix, lo0, hi0, lo1, hi1);
}

hipError_t launchShadowSoftLightListAdaptive(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.mask || !softListSlotsOk(p.offsets, p.nsamples, true, false)) return hipErrorInvalidValue;
    static const char* const names[2][3] = RTS_PACKET_NAMES("shadowSoftLightListAdaptivePacketKernel", "");
    return launchLoopFamily(variant, p, stream, name, shadowSoftLightListAdaptiveShareKernel<false>, "shadowSoftLightListAdaptiveShareKernel",
                            names, [&](dim3 grid, auto split, auto geom) {
        constexpr int SPLIT = decltype(split)::value, GEOM = decltype(geom)::value;
        hipLaunchKernelGGL((shadowSoftLightListAdaptivePacketKernel<SPLIT, GEOM, false>), grid, dim3(64 * SPLIT), 0, stream, p); });
}

hipError_t launchShadowSoftLightListJittered(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.mask || !softListSlotsOk(p.offsets, p.nsamples, true, true)) return hipErrorInvalidValue;
    static const char* const names[2][3] = RTS_PACKET_NAMES("shadowSoftLightListAdaptivePacketKernel", ",jitter");
    return launchLoopFamily(variant, p, stream, name, shadowSoftLightListAdaptiveShareKernel<true>,
                            "shadowSoftLightListAdaptiveShareKernel<jitter>", names, [&](dim3 grid, auto split, auto geom) {
        constexpr int SPLIT = decltype(split)::value, GEOM = decltype(geom)::value;
        hipLaunchKernelGGL((shadowSoftLightListAdaptivePacketKernel<SPLIT, GEOM, true>), grid, dim3(64 * SPLIT), 0, stream, p); });
}
