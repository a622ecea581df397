// ADAPTIVE SOFT SHADOWS (rts_trace_shadow_mask_adaptive*, include/rts.h): included by rts_distance.inc after the light-list kernels.
// From the common part (rts_block_common.inc): SoftPixel, softPrologue<false>, tileBlock, tilePixel, blockPixel, tileWave, freshLaneId,
// launchLoopFamily.
//
// For a light of n = p.nsamples samples and a probe count k = p.nrays (rts_adaptive.h: the slots), with u_j the any-hit byte of
// sample j (1 = unoccluded), c_k = u_0 + ... + u_(k-1) and c_n = u_0 + ... + u_(n-1):
//   mask[p] = 0 where the pixel is inactive or c_k == 0, n where c_k == k, c_n otherwise; refined[p] = 1 exactly in the last case.
// Everything is integer counting of bytes that are functions of (pixel, sample) alone, so the result does not depend on the order
// the samples are walked in, nor on which wave walked which (DESIGN.md 4.16).

// Between the phases: a live pixel whose probe was unanimous gets its verdict NOW (0 or n, refined 0) -- the bytes the definition
// gives it, stored in front of the second walk like the prologue's zeros, so that nothing of such a pixel stays in registers across
// it.  Then the lanes that do not refine take the texel and pixel index of the first lane that does (d->live becomes `pen`): from
// here on the wave is in the state softPrologue leaves, with the penumbra as its live set.
// pens != 0.  `stores`: as in the prologue.
__device__ __forceinline__ void adaptiveRefineSetup(const TraceParams& p, SoftPixel* d, uint32_t ck, bool pen, uint64_t pens, bool stores) {
    if (d->live && !pen && stores) {
        __builtin_nontemporal_store((uint8_t)(ck != 0u ? p.nsamples : 0u), &p.mask[d->pix]);    // (unanimous: c_k is 0 or k)
        if (p.out) __builtin_nontemporal_store((uint8_t)0, &p.out[d->pix]);
    }
    // (standInTexel with the pixel index, written out: through the helper the lane-per-ray kernel's text changes)
    const int first = __builtin_ctzll(pens);
    const float sx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d->rel.x), first));
    const float sy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d->rel.y), first));
    const float sz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d->rel.z), first));
    const uint32_t sp = (uint32_t)__builtin_amdgcn_readlane((int)d->pix, first);
    d->rel = pen ? d->rel : F3{ sx, sy, sz };
    d->pix = pen ? d->pix : sp;
    d->live = pen;
}
// A wave without a penumbra pixel: every live pixel's verdict, and the wave is done.
__device__ __forceinline__ void adaptiveStoreUnanimous(const TraceParams& p, const SoftPixel& d, uint32_t ck) {
    if (!d.live) return;
    __builtin_nontemporal_store((uint8_t)(ck != 0u ? p.nsamples : 0u), &p.mask[d.pix]);
    if (p.out) __builtin_nontemporal_store((uint8_t)0, &p.out[d.pix]);
}
__device__ __forceinline__ void adaptiveStoreRefined(const TraceParams& p, const SoftPixel& d, uint32_t cn) {
    if (!d.live) return;                                                 // (live: the penumbra, since adaptiveRefineSetup)
    __builtin_nontemporal_store((uint8_t)cn, &p.mask[d.pix]);           // comp:148-150, per sample
    if (p.out) __builtin_nontemporal_store((uint8_t)1, &p.out[d.pix]);
}

// Lane per ray: shadowLightListShareKernel's 16 x 16 block, the probe samples and then the others one after the other around
// traverseShare.  The four waves share nothing but the LDS each owns a quarter of, so each decides for its own 8 x 8 quarter.
__global__ __launch_bounds__(256) void shadowMaskAdaptiveShareKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][64];       // lane numbers exchanged by traverseShare (256 B per wave)
    uint32_t* lds = shareSlots[threadIdx.x >> 6];
    uint32_t x, y;
    if (!blockPixel(p, &x, &y)) return;
    SoftPixel d;
    if (!softPrologue<false>(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, true, &d)) return;
    const NodeStream bvh = openStream(p);
    const uint32_t probe = (uint32_t)p.nrays;
    uint32_t count = 0;
    for (uint32_t s = 0; s < probe; ++s) {
        const Ray r = makeShadowRay(p, d.rel, s, d.pix);
        const bool unsafe = d.live && !raySafe(r);
        bool occluded;
        if (p.bvhFinite && __builtin_amdgcn_ballot_w64(unsafe) == 0)
            occluded = traverseShare<true>(bvh, r, d.live, 0u, lds);
        else
            occluded = traverseShare<false>(bvh, r, d.live, 0u, lds);
        count += (d.live && !occluded) ? 1u : 0u;                        // comp:148
    }
    const bool pen = d.live && count != 0u && count != probe;
    const uint64_t pens = __builtin_amdgcn_ballot_w64(pen);
    if (pens == 0) { adaptiveStoreUnanimous(p, d, count); return; }
    adaptiveRefineSetup(p, &d, count, pen, pens, true);
    // (the probe's loop again, shareAnyHit's gate written out in both: as one helper over [from, to) the loop is optimised on its
    //  own before it is inlined, hoists differently, and this kernel's text moves)
    for (uint32_t s = probe; s < p.nsamples; ++s) {
        const Ray r = makeShadowRay(p, d.rel, s, d.pix);
        const bool unsafe = d.live && !raySafe(r);
        bool occluded;
        if (p.bvhFinite && __builtin_amdgcn_ballot_w64(unsafe) == 0)
            occluded = traverseShare<true>(bvh, r, d.live, 0u, lds);
        else
            occluded = traverseShare<false>(bvh, r, d.live, 0u, lds);
        count += (d.live && !occluded) ? 1u : 0u;
    }
    adaptiveStoreRefined(p, d, count);
}

// One sample of a packet wave: the ray of (pixel, s) and traversePacket<1, false> (any-hit, the early-out kept) -> the lane's byte.
// (The texel and the pixel index are made opaque per sample: otherwise the compiler hoists every part of the set-up that does not
//  depend on the sample out of the loop and keeps it in registers across the walk -- rts_soft_distance.inc.  makeShadowRay<false>:
//  the general set-up alone, as in the soft mask kernels.)
__device__ __forceinline__ uint32_t adaptiveSample(const TraceParams& p, const NodeStream& bvh, SoftPixel& d, uint32_t s, uint32_t* lds) {
    asm volatile("" : "+v"(d.rel.x), "+v"(d.rel.y), "+v"(d.rel.z), "+v"(d.pix));
    const Ray r[1] = { makeShadowRay<false>(p, d.rel, s, d.pix) };
    const bool walks[1] = { d.live };
    bool occluded[1];
    traversePacket<1, false>(p, bvh, r, walks, occluded, lds);
    return (walks[0] && !occluded[0]) ? 1u : 0u;                         // comp:148
}

// Stackless packet over 8 x 8 tiles.  GEOM as in shadowSoftDistancePacketKernel (1: a row range on a 2-D grid, 2: one stripe of
// power-of-two bands, 0: every other geometry).  SPLIT 1: one wave walks the probe, decides, walks the rest.  SPLIT 4: four waves
// per tile, which map lane -> pixel identically:
//   phase 1  wave w walks the probe samples w, w + 4, ... < k over the live pixels and counts per lane in partial[0][w];
//   BARRIER 1; every wave reads all four words of its lane: c_k, pen = live && 0 < c_k < k, ballot(pen) -- the same words in the
//            same lanes, so the same ballot in the four waves.  No penumbra pixel: wave 0 stores the verdicts, every wave returns;
//   phase 2  wave w walks the samples k + w, k + w + 4, ... < n over the penumbra pixels and counts in partial[1][w] -- a SECOND set
//            of words, so no wave writes a word that another may still be reading for its c_k (wave 0 starts its word at c_k);
//   BARRIER 2; wave 0 sums the four words of the second set and stores them where pen, with refined = 1.
// Every wave reaches each barrier or none does: the exits in front of barrier 1 (a block outside the dispatch, a tile without an
// active pixel) and the one between the barriers (no penumbra pixel) depend on the tile alone -- on the geometry, on the tile's
// active bytes and on LDS words all four waves read alike after barrier 1 --, never on the wave.  A wave that owns no sample of a
// phase (k < 4, n - k < 4) runs no walk in it and contributes 0.
// A wave keeps its counts in LDS (each lane its own word), not in registers across the walks: the kernel compiles for 64 VGPRs.
template <int SPLIT, int GEOM>
__global__ __launch_bounds__(64 * SPLIT) __attribute__((amdgpu_waves_per_eu(8)))
void shadowMaskAdaptivePacketKernel(TraceParams p) {
    static_assert(SPLIT == 1 || SPLIT == 4, "one wave per tile, or four that deal its samples");
    __shared__ uint32_t shareSlots[SPLIT][64];
    __shared__ uint32_t partial[2][SPLIT][64];                           // per phase and wave: unoccluded samples per lane
    uint32_t bx, by, x, y;
    if (!tileBlock<GEOM>(p, &bx, &by)) return;
    const uint32_t wave = tileWave<SPLIT>();
    tilePixel<GEOM>(p, bx, by, &x, &y);
    SoftPixel d;
    if (!softPrologue<false>(p, (x < p.W) && (y < p.rowEnd), y * p.W + x, wave == 0, &d)) return;
    const NodeStream bvh = openStream(p);
    const uint32_t probe = (uint32_t)p.nrays;
    partial[0][wave][freshLaneId()] = 0;
    for (uint32_t s = wave; s < probe; s += SPLIT) {
        const uint32_t one = adaptiveSample(p, bvh, d, s, shareSlots[wave]);
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
        if (wave == 0) adaptiveStoreUnanimous(p, d, ck);
        return;
    }
    adaptiveRefineSetup(p, &d, ck, pen, pens, wave == 0);
    partial[1][wave][freshLaneId()] = wave == 0 ? ck : 0u;
    for (uint32_t s = probe + wave; s < p.nsamples; s += SPLIT) {
        const uint32_t one = adaptiveSample(p, bvh, d, s, shareSlots[wave]);
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
    adaptiveStoreRefined(p, d, cn);
}

hipError_t launchShadowMaskAdaptive(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    if (!p.mask || p.nsamples < 2 || p.nsamples > 64 || p.nrays == 0 || p.nrays >= p.nsamples) return hipErrorInvalidValue;
    static const char* const names[2][3] = RTS_PACKET_NAMES("shadowMaskAdaptivePacketKernel", "");
    return launchLoopFamily(variant, p, stream, name, shadowMaskAdaptiveShareKernel, "shadowMaskAdaptiveShareKernel", names,
                            [&](dim3 grid, auto split, auto geom) {
        constexpr int SPLIT = decltype(split)::value, GEOM = decltype(geom)::value;
        hipLaunchKernelGGL((shadowMaskAdaptivePacketKernel<SPLIT, GEOM>), grid, dim3(64 * SPLIT), 0, stream, p); });
}
