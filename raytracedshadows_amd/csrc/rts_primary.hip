// Harness: G-buffer generation on the GPU -- the same closest-hit tests as the host version
// (rts_closest_hit.h), one primary ray per lane, one wave per 8x8 pixel tile, walked as a packet.  Replaces the reference's raster pass
// (Source/RayTracedShadows.cpp:512-568, Model.vert/.frag) as the producer of the position target the shadow kernel
// reads; not part of the timed shadow path.
#include <hip/hip_runtime.h>
#include "../../include/rts_scene.h"
#include "rts_closest_hit.h"

extern "C" const void* rts_ctx_device_bvh(rts_ctx* ctx);   // rts_api.cpp
extern "C" int rts_ctx_device_ordinal(rts_ctx* ctx);

namespace rts_harness {
Camera makeCamera(const float eye[3], const float target[3], float fovy, uint32_t W, uint32_t H);

// The launch of every scene pass, after the entry's own argument checks: the context's device, the kernel, the RTS_* status.
template <class... Params, class... Args>
static int launchPass(rts_ctx* ctx, void* stream, dim3 grid, dim3 block, size_t ldsBytes, void (*kernel)(Params...), Args... args) {
    hipError_t e = hipSetDevice(rts_ctx_device_ordinal(ctx));
    if (e != hipSuccess) return RTS_ERR_HIP + (int)e;
    hipLaunchKernelGGL(kernel, grid, block, ldsBytes, (hipStream_t)stream, args...);
    e = hipGetLastError();
    return e == hipSuccess ? RTS_OK : RTS_ERR_HIP + (int)e;
}
// ... of a pass of one pixel per lane: 256 lanes per workgroup over n pixels (n travels among the kernel's own arguments too).
template <class... Params, class... Args>
static int launchPerPixel(rts_ctx* ctx, void* stream, uint64_t n, void (*kernel)(Params...), Args... args) {
    return launchPass(ctx, stream, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, kernel, args...);
}

// One wave = one 8x8 tile of primary rays, walked as a PACKET: the rays of a tile are coherent, every index only grows, and
// every way out of a subtree leads to its root's miss link -- so the smallest index any ray stands on is wave-uniform
// (the argument of the shadow kernel): the node comes through the scalar cache once per wave, and each ray
// takes part only where it stands.  Every ray performs exactly the tests, in the order, that closestHit() performs for it
// alone (same helpers, no contraction), so the texels are the same bits as the host pass and the oracle's.
__global__ __launch_bounds__(64) void gbufferKernel(const uint32_t* __restrict__ bvh, Camera cam, uint32_t W, uint32_t H,
                                                    float* __restrict__ positions, float* __restrict__ normals) {
    const uint32_t END = 0xFFFFFFFFu;
    const uint32_t lane = threadIdx.x;
    const uint32_t x = blockIdx.x * 8u + (lane & 7u), y = blockIdx.y * 8u + (lane >> 3);
    const bool live = x < W && y < H;
    const V3 d = primaryDirection(cam, live ? x : 0u, live ? y : 0u, W, H);
    const V3 o = cam.eye;
    const V3 inv{ 1.0f / d.x, 1.0f / d.y, 1.0f / d.z };
    Hit best{ asFloat(0x7F800000u), END };
    uint32_t pos = live ? 0u : END;                                     // the node this ray tests next
    uint32_t cur = 0;
    while (cur != END) {
        cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur);
        const uint32_t* a = bvh + (size_t)cur * 8;
        const uint32_t a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], b0 = a[4], b1 = a[5], b2 = a[6], b3 = a[7];
        const uint32_t na[4] = { a0, a1, a2, a3 }, nb[4] = { b0, b1, b2, b3 };
        const bool here = pos == cur;
        bool entered = false;
        if (a3 != END) {                                                // (wave-uniform branch)
            if (here) {
                leafTest(na, nb, bvh + (size_t)a3 * 4, cur, o, d, &best);
                pos = b3;
            }
        } else if (here) {
            entered = boxTest(na, nb, o, inv, best.t);
            pos = entered ? cur + 1u : b3;
        }
        cur = __builtin_amdgcn_ballot_w64(entered) != 0 ? cur + 1u : b3;   // nobody inside: everyone waits at or beyond the miss link
    }
    if (!live) return;
    const size_t i = ((size_t)y * W + x) * 4;
    writeTexel(bvh, d, best, positions + i, normals ? normals + i : nullptr);
}
int makeCombineParams(const rts_constants* k, const rts_light* light, bool havePositions, CombineParams* out);

// Combine pass (Combine.frag:18-37), one pixel per lane; rgb is 3 bytes per pixel like the host version.
__global__ __launch_bounds__(256) void combineKernel(CombineParams c, const float* positions, const float* normals,
                                                     const uint8_t* mask, uint64_t n, uint8_t* rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float zero[4] = { 0.f, 0.f, 0.f, 0.f };
    const uint8_t q = combinePixel(c, positions ? positions + i * 4 : zero, normals + i * 4, mask[i]);
    rgb[i * 3] = q; rgb[i * 3 + 1] = q; rgb[i * 3 + 2] = q;
}

// The facing mark (rts_closest_hit.h: facingPixel), one pixel per lane like combineKernel.
__global__ __launch_bounds__(256) void facingKernel(CombineParams c, const float* positions, const float* normals, uint64_t n,
                                                    uint8_t* active) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float zero[4] = { 0.f, 0.f, 0.f, 0.f };
    active[i] = facingPixel(c, positions ? positions + i * 4 : zero, normals + i * 4);
}

int makeFacingLights(const rts_constants* k, const rts_light_list* list, bool havePositions, FacingLights* out);

// The light map of a light list (rts_closest_hit.h: facingLightsPixel), one pixel per lane like facingKernel.
__global__ __launch_bounds__(256) void facingLightsKernel(FacingLights f, const float* positions, const float* normals, uint64_t n,
                                                          uint8_t* lightsMap) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float zero[4] = { 0.f, 0.f, 0.f, 0.f };
    lightsMap[i] = facingLightsPixel(f, positions ? positions + i * 4 : zero, normals + i * 4);
}

int makeCombineList(const rts_constants* k, const rts_light_list* list, const float* colors, bool havePositions, CombineList* out);
int makeCombineSoftList(const rts_constants* k, const rts_soft_light_list* list, const float* colors, bool havePositions, CombineList* out);

// The combine pass of a light list (rts_closest_hit.h: combineListPixel), one pixel per lane like combineKernel, for every frame size
// and every pointer.  (A form of four pixels per lane -- dword loads of the planes and the map, 16-byte loads of the normals, three
// dword stores -- was measured 1.3 to 1.7 times slower at 4K and removed: EXPERIMENTS.md)  HARD: `planes` is the one mask plane of rts_trace_light_list*, light l in bit l; else the count
// planes of rts_trace_soft_light_list*, plane l at planes + l * n.
template <bool HARD>
__global__ __launch_bounds__(256) void combineListKernel(CombineList f, const float* positions, const float* normals,
                                                         const uint8_t* lightsMap, const uint8_t* planes, uint64_t n, uint8_t* rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float zero[4] = { 0.f, 0.f, 0.f, 0.f };
    const float* n4 = normals + i * 4;
    const float nx = n4[0], ny = n4[1], nz = n4[2];
    const float nrm[4] = { nx, ny, nz, 0.f };
    const bool background = nx == 0.0f && ny == 0.0f && nz == 0.0f;        // (its map byte is not read)
    const uint32_t bits = (lightsMap && !background) ? lightsMap[i] : 0xFFu;
    uint8_t q[3];
    combineListPixel(f, positions ? positions + i * 4 : zero, nrm, bits,
                     [&](uint32_t l) { return HARD ? (uint8_t)((planes[i] >> l) & 1u) : planes[(uint64_t)l * n + i]; }, q);
    rgb[i * 3] = q[0]; rgb[i * 3 + 1] = q[1]; rgb[i * 3 + 2] = q[2];
}

template <bool HARD>
static int launchCombineList(rts_ctx* ctx, const CombineList& f, const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                             const uint8_t* d_planes, uint32_t W, uint32_t H, uint8_t* d_rgb, void* stream) {
    const uint64_t n = (uint64_t)W * H;
    return launchPerPixel(ctx, stream, n, combineListKernel<HARD>, f, d_positions, d_normals, d_lights_map, d_planes, n, d_rgb);
}
} // namespace rts_harness

extern "C" int rtsh_combine_device(rts_ctx* ctx, const rts_constants* k, const rts_light* light, const float* d_positions,
                                   const float* d_normals, const uint8_t* d_mask, uint32_t W, uint32_t H, uint8_t* d_rgb,
                                   void* stream) {
    if (!ctx || !k || !d_normals || !d_mask || !d_rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    rts_harness::CombineParams c;
    int s = rts_harness::makeCombineParams(k, light, d_positions != nullptr, &c);
    if (s != RTS_OK) return s;
    const uint64_t n = (uint64_t)W * H;
    return rts_harness::launchPerPixel(ctx, stream, n, rts_harness::combineKernel, c, d_positions, d_normals, d_mask, n, d_rgb);
}

extern "C" int rtsh_facing_active_device(rts_ctx* ctx, const rts_constants* k, const rts_light* light, const float* d_positions,
                                         const float* d_normals, uint32_t W, uint32_t H, uint8_t* d_active, void* stream) {
    if (!ctx || !k || !d_normals || !d_active || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    rts_harness::CombineParams c;
    int s = rts_harness::makeCombineParams(k, light, d_positions != nullptr, &c);
    if (s != RTS_OK) return s;
    const uint64_t n = (uint64_t)W * H;
    return rts_harness::launchPerPixel(ctx, stream, n, rts_harness::facingKernel, c, d_positions, d_normals, n, d_active);
}

extern "C" int rtsh_facing_lights_device(rts_ctx* ctx, const rts_constants* k, const rts_light_list* list, const float* d_positions,
                                         const float* d_normals, uint32_t W, uint32_t H, uint8_t* d_lights_map, void* stream) {
    if (!ctx || !d_normals || !d_lights_map || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    rts_harness::FacingLights f;
    int s = rts_harness::makeFacingLights(k, list, d_positions != nullptr, &f);
    if (s != RTS_OK) return s;
    const uint64_t n = (uint64_t)W * H;
    return rts_harness::launchPerPixel(ctx, stream, n, rts_harness::facingLightsKernel, f, d_positions, d_normals, n, d_lights_map);
}

extern "C" int rtsh_primary_gbuffer_device(rts_ctx* ctx, const float eye[3], const float target[3], float fovy,
                                           uint32_t W, uint32_t H, float* d_positions, float* d_normals, void* stream) {
    if (!ctx || !eye || !target || !d_positions || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    if (H > RTSH_GBUFFER_MAX_HEIGHT) return RTS_ERR_INVALID_ARG;        // the grid's y extent: refused here, not by the launch
    const void* bvh = rts_ctx_device_bvh(ctx);
    if (!bvh) return RTS_ERR_NO_BVH;
    const rts_harness::Camera cam = rts_harness::makeCamera(eye, target, fovy, W, H);
    return rts_harness::launchPass(ctx, stream, dim3((W + 7) / 8, (H + 7) / 8), dim3(64), 0, rts_harness::gbufferKernel, (const uint32_t*)bvh,
                                   cam, W, H, d_positions, d_normals);
}

// The combine pass of a light list on the GPU (include/rts_scene.h): one kernel, the list, the colours and the constants by value.
extern "C" int rtsh_combine_light_list_device(rts_ctx* ctx, const rts_constants* k, const rts_light_list* list, const float* colors,
                                              const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                              const uint8_t* d_mask, uint32_t W, uint32_t H, uint8_t* d_rgb, void* stream) {
    if (!ctx || !k || !d_normals || !d_mask || !d_rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    rts_harness::CombineList f;
    const int s = rts_harness::makeCombineList(k, list, colors, d_positions != nullptr, &f);
    if (s != RTS_OK) return s;
    return rts_harness::launchCombineList<true>(ctx, f, d_positions, d_normals, d_lights_map, d_mask, W, H, d_rgb, stream);
}

extern "C" int rtsh_combine_soft_light_list_device(rts_ctx* ctx, const rts_constants* k, const rts_soft_light_list* list, const float* colors,
                                                   const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                   const uint8_t* d_counts, uint32_t W, uint32_t H, uint8_t* d_rgb, void* stream) {
    if (!ctx || !k || !d_normals || !d_counts || !d_rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    rts_harness::CombineList f;
    const int s = rts_harness::makeCombineSoftList(k, list, colors, d_positions != nullptr, &f);
    if (s != RTS_OK) return s;
    return rts_harness::launchCombineList<false>(ctx, f, d_positions, d_normals, d_lights_map, d_counts, W, H, d_rgb, stream);
}

#include "rts_filter.inc"   // the filter of a light list's planes and the visibility combine
#include "rts_temporal.inc" // the temporal accumulation of a light list's visibility
#include "rts_wide_filter.inc" // the wide (a-trous) filter of a light list's planes
#include "rts_wide_guided.inc" // the variance-guided wide filter of a soft light list's planes
#include "rts_moments.inc" // the temporal accumulation of a soft light list's count moments and the filter they guide
#include "rts_wide_mean.inc" // the wide filters fed from the accumulated mean of the count moments
#include "rts_motion.inc" // the motion G-buffer pass: where the seen surface was in the previous frame's stream
#include "rts_wide_propagated.inc" // the guided mean filter with a variance plane carried through the passes
#include "rts_upsample.inc" // half-resolution light lists: subsample, retrace map, upsample
#include "rts_compact.inc" // a light map compacted into the list of its marked pixels, for the sparse list traces
#include "rts_wide_bent.inc" // the wide filter of the bent plane: a-trous over integer vectors
#include "rts_bent_temporal.inc" // the bent texel accumulated over frames, and the wide bent filter fed from it
