// WHAT THE BLOCK TRACES SHARE: included first by rts_distance.inc (inside namespace rts, after every kernel of the mask traces), in
// front of the four families -- distance, soft distance, light list, adaptive.  It holds what more than one of them uses: the
// lane's pixel in both block forms, the stand-in, the soft prologue, the exact-path gate, the launch helpers (DESIGN.md 4.15).
// A fold is kept only where every kernel's instruction text stays what it was (profiles/r18/kernel_resources.txt): the compiler
// optimises a helper on its own before it inlines it.  So the stand-in is still written out in softPrologue, in distancePrologue
// (rts_distance.inc) and in adaptiveRefineSetup (rts_adaptive.inc) beside standInTexel, and the gate in the adaptive lane-per-ray
// kernel beside shareAnyHit / shareDistance: a fix to either goes to each of these, and to rts_kernels.hip's own copies.
static constexpr uint32_t DIST_NONE = 0x7F800000u;                       // +Inf: no triangle accepted

// The wave's number in a tile of SPLIT waves.  (It is wave-uniform: said so, the sample or light counter and the wave's LDS
// addresses stay on the scalar unit.)
template <int SPLIT>
__device__ __forceinline__ uint32_t tileWave() {
    return SPLIT > 1 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0u;
}
// The lane's pixel in the stackless-packet forms, one wave per 8 x 8 tile.  GEOM 1: a contiguous row range on a 2-D grid; 2: one
// stripe of power-of-two bands on a 2-D grid (the frame row of a tile row is two shifts and a multiply); 0: every other geometry
// (blockToXY, ownedRow).  Also gives the wave's number in the tile.  -> false: the block lies outside the dispatch.
template <int GEOM>
__device__ __forceinline__ bool tileBlock(const TraceParams& p, uint32_t* bx, uint32_t* by) {
    *bx = blockIdx.x; *by = 0;
    if constexpr (GEOM == 0) return blockToXY(p, blockIdx.x, bx, by);
    else *by = dispatchRow(p, blockIdx.y);
    return true;
}
template <int GEOM>
__device__ __forceinline__ void tilePixel(const TraceParams& p, uint32_t bx, uint32_t by, uint32_t* x, uint32_t* y) {
    const uint32_t lane = threadIdx.x & 63u;
    *x = bx * 8u + (lane & 7u);
    if constexpr (GEOM == 2) {
        const uint32_t band = by >> p.bandShift, within = by - (band << p.bandShift);
        *y = (band * p.nStripes + p.stripe) * p.bandRows + within * 8u + (lane >> 3);
    } else if constexpr (GEOM == 1) *y = p.rowBegin + by * 8u + (lane >> 3);
    else *y = ownedRow(p, by * 8u + (lane >> 3));
}
// The same in the lane-per-ray forms: shadowMaskActiveShareKernel's 16 x 16 block of four waves, an 8 x 8 quarter each.
__device__ __forceinline__ bool blockPixel(const TraceParams& p, uint32_t* x, uint32_t* y) {
    uint32_t bx, by;
    if (!blockToXY(p, blockIdx.x, &bx, &by)) return false;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    *x = bx * 16u + (wave & 1u) * 8u + (lane & 7u);
    *y = ownedRow(p, by * 16u + (wave >> 1) * 8u + (lane >> 3));
    return true;
}
// The lane's number from an operand the compiler cannot see through: asked for wherever a per-lane LDS word is touched after a walk,
// so that no LDS address is carried in a register across it (in the 4-wave forms that is the one register too many, 8 bytes of scratch).
__device__ __forceinline__ uint32_t freshLaneId() {
    uint32_t zero = 0;
    asm volatile("" : "+v"(zero));
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));
}

// The stand-in of rts_packet_tile.inc: a lane without a ray takes the texel of the first lane that has one and sets up that lane's
// ray.  Exact, because its result is discarded, and it keeps the wave-wide gates of the ray set-up on real rays -- a background
// texel or the garbage an unmarked pixel may hold would send the whole wave down the slow forms.  walkers != 0.
// (shadowMaskActiveShareKernel keeps its own copy: it lives in rts_kernels.hip, whose text is part of the kernel-build hash that
// the committed counter profiles carry.)
__device__ __forceinline__ F3 standInTexel(F3 rel, bool keeps, uint64_t walkers) {
    const int firstWalker = __builtin_ctzll(walkers);
    const float sx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rel.x), firstWalker));
    const float sy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rel.y), firstWalker));
    const float sz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rel.z), firstWalker));
    return keeps ? rel : F3{ sx, sy, sz };
}

// What the soft-distance and the adaptive kernels do in front of their sample loops, arranged so that little stays in registers
// across the walks -- the packet forms compile for 64 VGPRs.
// - The texel and the active byte are requested in one batch.
// - An owned pixel that sends no ray gets its zeros HERE, in front of the walks; from then on a lane is `live` or has nothing to
//   store.  DISTANCE: distance = +0, mask = 0 (soft distance); else mask = 0, refined = 0 (adaptive).
// - `stores`: in the 4-wave form every wave looks at the same tile and only wave 0 writes it.
// - A lane that is not live stands in for the first one that is, with its texel and with its 32-bit pixel index (a dispatch has
//   at most 2^31 pixels): per-pixel jitter hashes the index, so the lane picks the very offsets of the lane it stands in for.
// -> false: no lane of the wave sends a ray; the same answer in the four waves of a tile.
struct SoftPixel { bool live; uint32_t pix; F3 rel; };
template <bool DISTANCE>
__device__ __forceinline__ bool softPrologue(const TraceParams& p, bool owns, uint32_t pix, bool stores, SoftPixel* d) {
    // (no branch around the requests: a lane without a pixel asks for texel 0 and byte 0 and never looks at them)
    const f32x4 t = __builtin_nontemporal_load((const f32x4*)p.positions + (owns ? pix : 0u));          // comp:135
    uint8_t act = 1;
    if (p.activeMap) act = __builtin_nontemporal_load(p.activeMap + (owns ? pix : 0u));
    d->live = owns && act != 0;
    if (owns && !d->live && stores) {
        if constexpr (DISTANCE) {
            __builtin_nontemporal_store(0.0f, &p.distance[pix]);
            if (p.mask) __builtin_nontemporal_store((uint8_t)0, &p.mask[pix]);
        } else {
            __builtin_nontemporal_store((uint8_t)0, &p.mask[pix]);
            if (p.out) __builtin_nontemporal_store((uint8_t)0, &p.out[pix]);
        }
    }
    const uint64_t walkers = __builtin_amdgcn_ballot_w64(d->live);
    if (walkers == 0) return false;
    // (standInTexel, written out on the texel as loaded and with the pixel index: through the helper the kernels' text changes)
    const int firstWalker = __builtin_ctzll(walkers);
    const float sx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t.x), firstWalker));
    const float sy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t.y), firstWalker));
    const float sz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t.z), firstWalker));
    const uint32_t sp = (uint32_t)__builtin_amdgcn_readlane((int)pix, firstWalker);
    d->rel = d->live ? F3{ t.x, t.y, t.z } : F3{ sx, sy, sz };
    d->pix = d->live ? pix : sp;
    return true;
}

// The exact-path gate around the lane-per-ray any-hit walk: where a NaN could occur somewhere in this wave (unsafe = live &&
// !raySafe(r), said by the caller), the EXACT slab test.  (rts_distance.inc has the same gate around its own walk.)
__device__ __forceinline__ bool shareAnyHit(const TraceParams& p, const NodeStream& bvh, const Ray& r, bool live, bool unsafe, uint32_t* lds) {
    if (p.bvhFinite && __builtin_amdgcn_ballot_w64(unsafe) == 0) return traverseShare<true>(bvh, r, live, 0u, lds);
    return traverseShare<false>(bvh, r, live, 0u, lds);
}

// The host side of a block launch: the grid, the GEOM of the packet kernels (2: bands on a 2-D grid, 1: rows on a 2-D grid, 0:
// general) and the launch of that instantiation under its name.  (launchShadowMaskActive and launchActivePacket keep their own copy
// of the geometry choice: they live in rts_kernels.hip, whose text is part of the kernel-build hash of the committed counter profiles.)
static int packetGeom(const TraceParams& p) {
    if (p.grid2d && p.nStripes > 1 && p.bandShift != 0xFFFFFFFFu && p.rowOrder == 0) return 2;
    return (p.grid2d && p.nStripes <= 1) ? 1 : 0;
}
static dim3 blockGrid(const TraceParams& p) { return p.grid2d ? dim3(p.blocksX, p.blocksY) : dim3(p.gridBlocks); }
// launch(std::integral_constant<int, GEOM>) launches the packet kernel of that geometry; names: general, rows, bands.
template <class Launch>
static hipError_t launchPacketGeom(const TraceParams& p, const char* const (&names)[3], const char** name, Launch launch) {
    const int geom = packetGeom(p);
    *name = names[geom];
    if (geom == 2) launch(std::integral_constant<int, 2>{});
    else if (geom == 1) launch(std::integral_constant<int, 1>{});
    else launch(std::integral_constant<int, 0>{});
    return hipGetLastError();
}
// The names of a family's packet kernels as launchLoopFamily takes them, [SPLIT == 4][GEOM], from the kernel's stem and what follows the
// geometry ("" or ",jitter"): "stem<1,general>" .. "stem<4,bands>".
#define RTS_PACKET_NAMES(stem, more) { { stem "<1,general" more ">", stem "<1,rows" more ">", stem "<1,bands" more ">" }, \
                                       { stem "<4,general" more ">", stem "<4,rows" more ">", stem "<4,bands" more ">" } }
// The families with a sample or light loop, after their argument guards: the lane-per-ray kernel, or the packet kernel with one
// wave or four per tile.  packet(grid, integral_constant SPLIT, integral_constant GEOM) launches that instantiation; names[SPLIT == 4][GEOM].
template <class Packet>
static hipError_t launchLoopFamily(int variant, const TraceParams& p, hipStream_t stream, const char** name, void (*share)(TraceParams),
                                   const char* shareName, const char* const (&names)[2][3], Packet packet) {
    const dim3 grid = blockGrid(p);
    if (variant == V_SHARE) {
        *name = shareName;
        hipLaunchKernelGGL(share, grid, dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    if (variant != V_PACKET) return hipErrorInvalidValue;
    if (p.softSplit) return launchPacketGeom(p, names[1], name, [&](auto geom) { packet(grid, std::integral_constant<int, 4>{}, geom); });
    return launchPacketGeom(p, names[0], name, [&](auto geom) { packet(grid, std::integral_constant<int, 1>{}, geom); });
}
