// SPARSE LIGHT LISTS (rts_trace_light_list_sparse*, rts_trace_soft_light_list_sparse*, include/rts.h): included last by
// rts_distance.inc.  From the common part (rts_block_common.inc): standInTexel, shareAnyHit; from the light lists
// (rts_light_list.inc): ListPixel, lightListPrologue, makeListRay; from the soft light lists (rts_soft_light_list.inc):
// softListSamples, makeSoftListRay, softListPlane.
//
// The two lane-per-ray list kernels with the lane's pixel taken from a LIST of pixel indices (rtsh_compact_light_map*,
// include/rts_scene.h) where they take it from the block's place in the frame: lane i of the launch owns pixels[i] for
// i < min(*n, capacity), lights in order and samples in order around shareAnyHit, so every ray has the bits the block traces give it
// and a byte stays a function of (pixel, light, sample) alone (DESIGN.md 4.17, 4.33).  A tile that holds one marked pixel costs the
// block traces a whole wave; here 64 marked pixels fill one.
// - ceil(capacity / 256) workgroups are launched -- the list's length lives on the device and is not read back --; a wave whose
//   first entry lies at or beyond min(*n, capacity) leaves at once, in front of every other load.  Every exit is wave-uniform and
//   there is no workgroup barrier: the four waves of a block share nothing but the LDS each owns a quarter of (traverseShare's slots).
// - An entry of W * H or above owns nothing: nothing is read or written for it (it asks for texel 0 like a lane without an entry and
//   never looks at it).
// - ONLY the marked pairs are written: plane l at p where bit l < count of the map's byte is set (no map: every l < count); a hard
//   list's byte is read, its marked bits replaced and the byte stored by the one lane that owns the entry.  A pixel named twice is
//   owned by two lanes that compute and store the same bytes.
// pixels, n and capacity travel beside the argument block as arguments of their own: TraceParams keeps its size and layout.

// The lane's entry.  -> false: the whole wave lies beyond the list (wave-uniform: the first lane's index is).
__device__ __forceinline__ bool sparsePixel(const TraceParams& p, const uint32_t* pixels, const uint32_t* n, uint32_t capacity,
                                            bool* owns, uint32_t* pix) {
    const uint32_t listed = *n < capacity ? *n : capacity;               // (a scalar load: the same for every lane)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;                  // (below 2^32: the grid is ceil(capacity / 256))
    if ((i & ~63u) >= listed) return false;
    uint32_t q = 0xFFFFFFFFu;
    if (i < listed) q = __builtin_nontemporal_load(pixels + i);
    *owns = (i < listed) && (uint64_t)q < (uint64_t)p.W * p.H;
    *pix = q;
    return true;
}

__global__ __launch_bounds__(256) void shadowLightListSparseKernel(TraceParams p, const uint32_t* pixels, const uint32_t* n, uint32_t capacity) {
    __shared__ uint32_t shareSlots[4][64];       // lane numbers exchanged by traverseShare (256 B per wave)
    uint32_t* lds = shareSlots[threadIdx.x >> 6];
    bool owns; uint32_t pix;
    if (!sparsePixel(p, pixels, n, capacity, &owns, &pix)) return;
    ListPixel d;
    if (!lightListPrologue(p, owns, pix, false, &d)) return;             // (no marked pair in the wave: nothing is stored)
    const NodeStream bvh = openStream(p);
    uint32_t byte = 0;
    for (uint32_t l = 0; l < p.nsamples; ++l) {
        const bool walks = ((d.bits >> l) & 1u) != 0u;
        const uint64_t walkers = __builtin_amdgcn_ballot_w64(walks);
        if (walkers == 0) continue;
        const Ray r = makeListRay(p, standInTexel(d.rel, walks, walkers), l);
        const bool occluded = shareAnyHit(p, bvh, r, walks, walks && !raySafe(r), lds);
        byte |= (walks && !occluded) ? (1u << l) : 0u;                   // comp:148, as light l's bit
    }
    if (d.bits != 0u) {                                                  // (d.bits != 0 only where the lane owns a pixel)
        const uint32_t held = p.mask[d.pix];
        p.mask[d.pix] = (uint8_t)((held & ~d.bits) | byte);              // comp:150, the marked bits alone
    }
}

__global__ __launch_bounds__(256) void shadowSoftLightListSparseKernel(TraceParams p, const uint32_t* pixels, const uint32_t* n, uint32_t capacity) {
    __shared__ uint32_t shareSlots[4][64];       // lane numbers exchanged by traverseShare (256 B per wave)
    uint32_t* lds = shareSlots[threadIdx.x >> 6];
    bool owns; uint32_t pix;
    if (!sparsePixel(p, pixels, n, capacity, &owns, &pix)) return;
    ListPixel d;
    if (!lightListPrologue(p, owns, pix, false, &d)) return;             // (no marked pair in the wave: nothing is stored)
    const NodeStream bvh = openStream(p);
    for (uint32_t l = 0; l < p.nsamples; ++l) {
        const bool walks = ((d.bits >> l) & 1u) != 0u;
        const uint64_t walkers = __builtin_amdgcn_ballot_w64(walks);
        if (walkers == 0) continue;                                      // (no lane of the wave stores to plane l)
        const F3 rel = standInTexel(d.rel, walks, walkers);              // (lanes that do not walk light l stand in)
        const uint32_t samples = softListSamples(p, l);
        uint32_t count = 0;
        for (uint32_t j = 0; j < samples; ++j) {
            const Ray r = makeSoftListRay(p, rel, l, j);
            const bool occluded = shareAnyHit(p, bvh, r, walks, walks && !raySafe(r), lds);
            count += (walks && !occluded) ? 1u : 0u;                     // comp:148, per sample
        }
        if (walks) __builtin_nontemporal_store((uint8_t)count, softListPlane(p, l) + d.pix);   // comp:150, the marked pairs alone
    }
}

// p: the argument block of the list's block trace (its lights, map, planes and frame; the grid's members are not read).
hipError_t launchShadowLightListSparse(const TraceParams& p, const uint32_t* d_pixels, const uint32_t* d_n, uint32_t capacity,
                                       hipStream_t stream, const char** name) {
    if (!p.mask || p.nsamples < 1 || p.nsamples > 8 || !d_pixels || !d_n || capacity == 0) return hipErrorInvalidValue;
    *name = "shadowLightListSparseKernel";
    const dim3 grid((uint32_t)(((uint64_t)capacity + 255u) / 256u));
    hipLaunchKernelGGL(shadowLightListSparseKernel, grid, dim3(256), 0, stream, p, d_pixels, d_n, capacity);
    return hipGetLastError();
}

hipError_t launchShadowSoftLightListSparse(const TraceParams& p, const uint32_t* d_pixels, const uint32_t* d_n, uint32_t capacity,
                                           hipStream_t stream, const char** name) {
    if (!p.mask || !softListSlotsOk(p.offsets, p.nsamples, false, false) || !d_pixels || !d_n || capacity == 0) return hipErrorInvalidValue;
    *name = "shadowSoftLightListSparseKernel";
    const dim3 grid((uint32_t)(((uint64_t)capacity + 255u) / 256u));
    hipLaunchKernelGGL(shadowSoftLightListSparseKernel, grid, dim3(256), 0, stream, p, d_pixels, d_n, capacity);
    return hipGetLastError();
}
