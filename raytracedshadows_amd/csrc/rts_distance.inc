// THE BLOCK TRACES: included by rts_kernels.hip, inside namespace rts, after every kernel of the mask traces -- they add kernels and
// change none.  The common part first, then this file's family and the three built beside it, each in a file of its own below.
#include "rts_block_common.inc"

// OCCLUDER DISTANCE (rts_trace_shadow_distance*, rts_trace_rays_distance*, include/rts.h).  From the common part: DIST_NONE,
// tileBlock, tilePixel, blockPixel, launchPacketGeom, blockGrid.
//
// distance = min over every triangle the reference's test accepts on the reference's walk WITHOUT its return at a hit
// (comp:75-111: a leaf that hits goes on through its miss link, like a leaf that misses) of  c = (t > 0) ? t : +0,  t as
// intersectRayTri computes it (comp:41-59); +Inf where there is none.  The box test never looks at tmax (comp:61-73), so the
// leaves visited do not depend on any hit, and nothing is culled against the best t so far: the boxes and the triangles round
// differently, and a cull could change a bit.  Every contribution is >= +0, so the float order is the order of the bits as
// unsigned integers and the minimum is an integer minimum that does not depend on the order of the tests.

// comp:41-59, handing the contribution back: triHit's arithmetic, operation for operation (rcpFast behind the same wave-wide gate).
__device__ __forceinline__ bool triHitT(const Ray& r, F3 v0, F3 e0, F3 e1, uint32_t* c) {
    F3 s1 = cross3(r.d, e1);
    const float det = dot3(s1, e0);
    float invd;                                                          // = 1.0f / det (comp:44), bit for bit
    if (__builtin_amdgcn_ballot_w64(!rcpInRange(det)) == 0) invd = rcpFast(det); else invd = 1.0f / det;
    F3 dd = sub3(r.o, v0);
    float b1 = dot3(dd, s1) * invd;
    F3 s2 = cross3(dd, e0);
    float b2 = dot3(r.d, s2) * invd;
    float t = dot3(e1, s2) * invd;
    if (b1 < 0.0f || b1 > 1.0f || b2 < 0.0f || b1 + b2 > 1.0f || t < 0.0f || t > r.tmax) return false;
    *c = t > 0.0f ? __float_as_uint(t) : 0u;                             // an accepted NaN or -0 counts as +0
    return true;
}

// traverseShare's walk (the rotated loop, the hand-over of [next(c), bound) to idle lanes) for the distance: no owner is ever dropped,
// every piece runs to its bound.  The minimum of owner o lives in ldsMin[o] (256 B per wave beside the 256 B of lane numbers): it
// starts as best0 of lane o -- what a dissolved packet already found --, and whichever lane meets an accepted triangle of o's ray
// folds its contribution in with an LDS integer minimum, as it is found.  Returns the lane's own minimum.
template <bool FAST>
__device__ __forceinline__ uint32_t traverseShareDistance(const NodeStream& bvh, Ray r, bool live, uint32_t start, uint32_t* ldsSlots,
                                                          uint32_t* ldsMin, uint32_t best0) {
    uint32_t node = live ? start : END, bound = END, owner = laneId();
    uint32_t iter = 0;
    ldsMin[owner] = best0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    bool active = node < bound;
    u32x4 a = bvh.vec4(active ? node * 2u : OOB_VEC4), b = bvh.vec4(active ? node * 2u + 1u : OOB_VEC4);
    for (;;) {
        const uint64_t act = __builtin_amdgcn_ballot_w64(active);
        if (act == 0) break;
        uint32_t next = node;                                        // lanes that do not move keep their (finished) range
        if ((iter++ & 3u) == 0) {
            const uint64_t idle = ~act;
            const bool canGive = active && b.w < bound;              // there is a second part to give away
            const uint64_t givers = __builtin_amdgcn_ballot_w64(canGive);
            const uint32_t nIdle = (uint32_t)__builtin_popcountll(idle), nGive = (uint32_t)__builtin_popcountll(givers);
            if (nIdle >= SHARE_MIN_IDLE && nGive != 0) {
                const uint32_t pairs = nIdle < nGive ? nIdle : nGive;
                const uint32_t lane = laneId();
                const uint32_t below = (1u << (lane & 31u)) - 1u;
                const uint32_t rankG = lane < 32 ? __builtin_popcount((uint32_t)givers & below)
                                                 : __builtin_popcount((uint32_t)givers) + __builtin_popcount((uint32_t)(givers >> 32) & below);
                const uint32_t rankI = lane < 32 ? __builtin_popcount((uint32_t)idle & below)
                                                 : __builtin_popcount((uint32_t)idle) + __builtin_popcount((uint32_t)(idle >> 32) & below);
                const bool gives = canGive && rankG < pairs;
                const bool takes = !active && rankI < pairs;
                if (gives) ldsSlots[rankG] = lane;                   // k-th giver announces itself ...
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const uint32_t src = takes ? ldsSlots[rankI] : lane;  // ... to the k-th idle lane
                const int sel = (int)(src << 2);
                const float ox = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(sel, __builtin_bit_cast(int, r.o.x)));
                const float oy = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(sel, __builtin_bit_cast(int, r.o.y)));
                const float oz = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(sel, __builtin_bit_cast(int, r.o.z)));
                const float dx = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(sel, __builtin_bit_cast(int, r.d.x)));
                const float dy = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(sel, __builtin_bit_cast(int, r.d.y)));
                const float dz = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(sel, __builtin_bit_cast(int, r.d.z)));
                const float ix = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(sel, __builtin_bit_cast(int, r.inv.x)));
                const float iy = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(sel, __builtin_bit_cast(int, r.inv.y)));
                const float iz = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(sel, __builtin_bit_cast(int, r.inv.z)));
                const float tm = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(sel, __builtin_bit_cast(int, r.tmax)));
                const uint32_t srcNext = (uint32_t)__builtin_amdgcn_ds_bpermute(sel, (int)b.w);
                const uint32_t srcBound = (uint32_t)__builtin_amdgcn_ds_bpermute(sel, (int)bound);
                const uint32_t srcOwner = (uint32_t)__builtin_amdgcn_ds_bpermute(sel, (int)owner);
                if (takes) {
                    r.o = F3{ ox, oy, oz }; r.d = F3{ dx, dy, dz }; r.inv = F3{ ix, iy, iz }; r.tmax = tm;
                    next = srcNext; bound = srcBound; owner = srcOwner;   // its first node is requested below
                }
                if (gives) bound = b.w;                              // keeps [node, next(node))
                __builtin_amdgcn_wave_barrier();
            }
        }
        const bool leaf = active && a.w != END;
        const u32x4 v0 = bvh.vec4(leaf ? a.w : OOB_VEC4);
        if (active) {
            if (leaf) {
                next = b.w;                                          // hit or miss: on through the miss link
            } else {
                const bool h = boxHit<FAST>(r, __uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z),
                                            __uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z));
                next = h ? node + 1 : b.w;
            }
        }
        // request the next node, then test the triangle while it travels
        const bool nextActive = next < bound;
        const uint32_t nv = nextActive ? next * 2u : OOB_VEC4;
        const u32x4 na = bvh.vec4(nv), nb = bvh.vec4(nv + 1u);
        uint32_t c = DIST_NONE;
        if (leaf && triHitT(r, xyz(v0), xyz(a), xyz(b), &c))
            (void)__hip_atomic_fetch_min(&ldsMin[owner], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        node = next; a = na; b = nb;
        active = nextActive;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return ldsMin[laneId()];
}
// shareAnyHit's gate around that walk, every minimum starting at +Inf.
__device__ __forceinline__ uint32_t shareDistance(const TraceParams& p, const NodeStream& bvh, const Ray& r, bool live, bool unsafe,
                                                  uint32_t* lds, uint32_t* ldsMin) {
    if (p.bvhFinite && __builtin_amdgcn_ballot_w64(unsafe) == 0) return traverseShareDistance<true>(bvh, r, live, 0u, lds, ldsMin, DIST_NONE);
    return traverseShareDistance<false>(bvh, r, live, 0u, lds, ldsMin, DIST_NONE);
}

// traversePacket's one-ray form for the distance, on packetDescend -- the assembly descent that comes back at leaves.  The leaf is
// tested here: the members that hit fold t into their minimum and STAY members through the miss link with those that miss, so a
// packet never stands on a node nobody is on.  Dissolve rule and hand-over as in traversePacket; each lane takes its minimum along.
__device__ __forceinline__ uint32_t traversePacketDistance(const TraceParams& p, const NodeStream& bvh, const Ray& ray, bool live,
                                                           uint32_t* lds, uint32_t* ldsMin) {
    const uint64_t bvhAddr = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)((uint64_t)(uintptr_t)p.bvh >> 32)) << 32) |
                             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)p.bvh);
    const void* const bvhBase = (const void*)(uintptr_t)bvhAddr;
    const ConstNodePtr nodes = (ConstNodePtr)(uintptr_t)bvhAddr;
    const ConstVec4Ptr vec4s = (ConstVec4Ptr)(uintptr_t)bvhAddr;
    const Ray r[1] = { ray };
    uint64_t members[1] = { __builtin_amdgcn_ballot_w64(live) };
    uint32_t wait[1] = { END };
    const uint64_t unsafe = __builtin_amdgcn_ballot_w64(live && !raySafe(r[0]));
    if (members[0] == 0) return DIST_NONE;
    if (!p.bvhFinite || unsafe != 0)             // a NaN could occur somewhere in this wave: EXACT form, lane per ray
        return traverseShareDistance<false>(bvh, r[0], live, 0u, lds, ldsMin, DIST_NONE);
    uint32_t form = 8;
    if (p.bvhOrdered) {                          // uniform sign pattern of 1/d over the live rays: the ordered slab test
        const uint32_t oct = (__float_as_uint(r[0].inv.x) >> 31) | ((__float_as_uint(r[0].inv.y) >> 31) << 1) |
                             ((__float_as_uint(r[0].inv.z) >> 31) << 2);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)oct, __builtin_ctzll(members[0]));
        if ((__builtin_amdgcn_ballot_w64(oct != first) & members[0]) == 0) form = first;
    }
    form = (uint32_t)__builtin_amdgcn_readfirstlane((int)form);
    uint32_t cur = 0;
    const uint32_t window = p.packetBudget - 1u;
    const uint32_t thr = p.packetBudget * p.packetShare;
    int32_t budget = (int32_t)window;
    uint32_t acc = 0, best = DIST_NONE;
    bool leaf;
    do {
        cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur);
        budget = __builtin_amdgcn_readfirstlane(budget);
        acc = (uint32_t)__builtin_amdgcn_readfirstlane((int)acc);
        members[0] = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(members[0] >> 32)) << 32) |
                     (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)members[0]);
        leaf = packetDescend(form, bvhBase, r, cur, members, wait, budget, acc, thr, window) != 0;
        if (leaf) {
            const u32x8 n = nodes[cur];
            const u32x4 t = vec4s[n.s3];
            const uint32_t next = n.s7;
            const F3 e0{ __uint_as_float(n.s0), __uint_as_float(n.s1), __uint_as_float(n.s2) };
            const F3 e1{ __uint_as_float(n.s4), __uint_as_float(n.s5), __uint_as_float(n.s6) };
            const bool member = __builtin_amdgcn_inverse_ballot_w64(members[0]);
            uint32_t c = DIST_NONE;
            const bool hit = triHitT(r[0], xyz(t), e0, e1, &c);
            best = (member && hit && c < best) ? c : best;
            wait[0] = member ? next : wait[0];                       // every member goes on; whoever waits on `next` joins
            members[0] = __builtin_amdgcn_ballot_w64(wait[0] == next);
            cur = next;
        }
    } while (leaf && cur != END);
    if (cur != END) {                            // dissolved: every unfinished ray continues alone, its minimum with it
        const uint32_t mine = __builtin_amdgcn_inverse_ballot_w64(members[0]) ? cur : wait[0];
        best = traverseShareDistance<true>(bvh, r[0], mine != END, mine, lds, ldsMin, best);
    }
    return best;
}

// What every distance kernel of a frame does around its walk.  p.activeMap may be NULL (every pixel sends its ray), p.mask may be
// NULL (no mask wanted); both are wave-uniform.  A lane stores when it owns a pixel: the ray's distance, or +0 where the map's
// byte is 0; the mask byte is the one the active mask trace writes, 1 exactly where the distance is +Inf.
struct DistancePixel { bool owns, live; size_t pix; F3 rel; };

// -> false: no lane of the wave sends a ray; the zeros are stored and the wave may end (before the stream is opened or a ray is set up)
__device__ __forceinline__ bool distancePrologue(const TraceParams& p, bool owns, size_t pix, DistancePixel* d) {
    // (no branch around the requests: a lane without a pixel asks for texel 0 and byte 0 and never looks at them)
    const f32x4 t = __builtin_nontemporal_load((const f32x4*)p.positions + (owns ? pix : (size_t)0));   // comp:135
    uint8_t act = 1;
    if (p.activeMap) act = __builtin_nontemporal_load(p.activeMap + (owns ? pix : (size_t)0));
    d->owns = owns; d->pix = pix;
    d->live = owns && act != 0;
    d->rel = F3{ t.x, t.y, t.z };
    const uint64_t walkers = __builtin_amdgcn_ballot_w64(d->live);
    if (walkers == 0) {
        if (owns) {
            __builtin_nontemporal_store(0.0f, &p.distance[pix]);
            if (p.mask) __builtin_nontemporal_store((uint8_t)0, &p.mask[pix]);
        }
        return false;
    }
    // (standInTexel, written out: through the helper the three packet kernels' text changes)
    const int firstWalker = __builtin_ctzll(walkers);
    const float sx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d->rel.x), firstWalker));
    const float sy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d->rel.y), firstWalker));
    const float sz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d->rel.z), firstWalker));
    d->rel = d->live ? d->rel : F3{ sx, sy, sz };                        // (no pixel stand-in: a hard light has no per-pixel jitter)
    return true;
}
__device__ __forceinline__ void distanceStore(const TraceParams& p, const DistancePixel& d, uint32_t best) {
    if (!d.owns) return;
    __builtin_nontemporal_store(d.live ? __uint_as_float(best) : 0.0f, &p.distance[d.pix]);
    if (p.mask) __builtin_nontemporal_store((uint8_t)((d.live && best == DIST_NONE) ? 1u : 0u), &p.mask[d.pix]);   // comp:148-150
}

// Lane per ray: shadowMaskActiveShareKernel's 16 x 16 block of four waves around traverseShareDistance (small frames, "kernel" 0, 1, 2, 7).
__global__ __launch_bounds__(256) void shadowDistanceShareKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][2][64];    // per wave: lane numbers exchanged by the walk, and the owners' minima
    uint32_t* lds = shareSlots[threadIdx.x >> 6][0];
    uint32_t* ldsMin = shareSlots[threadIdx.x >> 6][1];
    uint32_t x, y;
    if (!blockPixel(p, &x, &y)) return;
    DistancePixel d;
    if (!distancePrologue(p, (x < p.W) && (y < p.rowEnd), (size_t)y * p.W + x, &d)) return;
    const NodeStream bvh = openStream(p);
    const Ray r = makeShadowRay(p, d.rel, 0u, 0u);
    distanceStore(p, d, shareDistance(p, bvh, r, d.live, d.live && !raySafe(r), lds, ldsMin));
}

// Stackless packet, one wave per 8 x 8 tile.  GEOM: tilePixel.
template <int GEOM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8)))
void shadowDistancePacketKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[2][64];
    uint32_t bx, by, x, y;
    if (!tileBlock<GEOM>(p, &bx, &by)) return;
    tilePixel<GEOM>(p, bx, by, &x, &y);
    DistancePixel d;
    if (!distancePrologue(p, (x < p.W) && (y < p.rowEnd), (size_t)y * p.W + x, &d)) return;
    const NodeStream bvh = openStream(p);
    const Ray r = makeShadowRay(p, d.rel, 0u, 0u);
    distanceStore(p, d, traversePacketDistance(p, bvh, r, d.live, shareSlots[0], shareSlots[1]));
}

// Generic rays: traceRaysKernel's set-up around the lane-per-ray walk (they carry no coherence promise).
__global__ __launch_bounds__(256) void traceRaysDistanceKernel(TraceParams p) {
    __shared__ uint32_t shareSlots[4][2][64];
    uint32_t* lds = shareSlots[threadIdx.x >> 6][0];
    uint32_t* ldsMin = shareSlots[threadIdx.x >> 6][1];
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = i < p.nrays;
    Ray r;
    r.o = F3{ 0, 0, 0 }; r.d = F3{ 1, 1, 1 }; r.tmax = 0.f;
    if (live) {
        const float4* src = (const float4*)p.rays + i * 2;
        float4 o = src[0], dd = src[1];
        r.o = F3{ o.x, o.y, o.z }; r.tmax = o.w; r.d = F3{ dd.x, dd.y, dd.z };
    }
    r.inv = F3{ 1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z };
    const NodeStream bvh = openStream(p);
    const uint32_t best = shareDistance(p, bvh, r, live, live && !raySafe(r), lds, ldsMin);
    if (live) p.distance[i] = __uint_as_float(best);
}

hipError_t launchShadowDistance(int variant, const TraceParams& p, hipStream_t stream, const char** name) {
    static const char* const names[3] = { "shadowDistancePacketKernel<general>", "shadowDistancePacketKernel<rows>", "shadowDistancePacketKernel<bands>" };
    if (!p.distance) return hipErrorInvalidValue;
    const dim3 grid = blockGrid(p);
    if (variant == V_SHARE) {
        *name = "shadowDistanceShareKernel";
        hipLaunchKernelGGL(shadowDistanceShareKernel, grid, dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    if (variant != V_PACKET) return hipErrorInvalidValue;
    return launchPacketGeom(p, names, name, [&](auto geom) {
        hipLaunchKernelGGL(shadowDistancePacketKernel<decltype(geom)::value>, grid, dim3(64), 0, stream, p); });
}

hipError_t launchTraceRaysDistance(const TraceParams& p, hipStream_t stream) {
    const dim3 grid((uint32_t)((p.nrays + 255) / 256)), block(256);
    hipLaunchKernelGGL(traceRaysDistanceKernel, grid, block, 0, stream, p);
    return hipGetLastError();
}

// the soft-shadow forms: the minimum over a light's samples, built on the walks above (its launch is declared in rts_soft_distance.h)
#include "rts_soft_distance.inc"
// light lists: up to 8 hard lights in one dispatch, one bit per light (its launch is declared in rts_light_list.h)
#include "rts_light_list.inc"
// adaptive soft shadows: a probe of a few samples, the others only in the penumbra (its launch is declared in rts_adaptive.h)
#include "rts_adaptive.inc"
// soft light lists: up to 8 lights, hard or soft, in one dispatch, a count plane per light (its launch is declared in rts_soft_light_list.h)
#include "rts_soft_light_list.inc"
// adaptive soft light lists: a probe per light, its penumbra alone refined (its launch is declared in rts_soft_light_list_adaptive.h)
#include "rts_soft_light_list_adaptive.inc"
// soft light list distance: a distance plane per light beside its count plane (its launch is declared in rts_soft_light_list_distance.h)
#include "rts_soft_light_list_distance.inc"
// sparse light lists: the two lane-per-ray list kernels fed from a list of pixels (their launches are declared in rts_light_list_sparse.h)
#include "rts_light_list_sparse.inc"
// ambient occlusion: hemisphere segments around the G-buffer's normal, counted (its launch is declared in rts_ao.h)
#include "rts_ao.inc"
// adaptive ambient occlusion: a probe of a few AO samples, the others only where it disagrees (its launch is declared in rts_ao_adaptive.h)
#include "rts_ao_adaptive.inc"
// bent normals: the AO trace with the integer sum of its unoccluded directions beside the count (its launch is declared in rts_ao_bent.h)
#include "rts_ao_bent.inc"
// AO distance and falloff: the AO trace with the nearest blocker and the falloff-weighted obscurance beside the count (its launch is declared in rts_ao_distance.h)
#include "rts_ao_distance.inc"
