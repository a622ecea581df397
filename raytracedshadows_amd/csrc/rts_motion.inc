// The motion G-buffer pass on the GPU (include/rts_scene.h: rtsh_primary_gbuffer_motion_device; DESIGN.md 4.29).  The per-pixel rule is
// the host twin's own source (rts_closest_hit.h: writeTexel, writeMotionTexel), compiled with the same flags.  Included at the end of
// rts_primary.hip; every kernel in front of it keeps its instruction text: gbufferMotionKernel is a SIBLING of gbufferKernel, whose
// walk it repeats statement for statement.

namespace rts_harness {
int makeMotionEyes(const float eye[3], const float prev_eye[3], const float target[3], const void* positions, const void* prevPoints,
                   const void* prevPointNormals, uint32_t W, uint32_t H, V3* prevEye, V3* eyeDelta);                   // rts_scene.cpp

// gbufferKernel's shape, for its reasons: one wave per 8 x 8 tile, the tile's rays walked as a packet through the scalar cache.  After
// the walk each live lane reads nine words of its hit leaf from both streams -- neighbouring lanes mostly share the leaf, so the reads
// fall on a few cache lines -- and writes two more texels and, if asked, the leaf index.  The texels are formed in registers (constant
// indices only: no scratch) and stored once.
__global__ __launch_bounds__(64) void gbufferMotionKernel(const uint32_t* __restrict__ bvh, const uint32_t* __restrict__ prev, Camera cam,
                                                          V3 prevEye, V3 eyeDelta, uint32_t W, uint32_t H, float* __restrict__ positions,
                                                          float* __restrict__ normals, float* __restrict__ prevPoints,
                                                          float* __restrict__ prevPointNormals, uint32_t* __restrict__ leaves) {
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
    const size_t p = (size_t)y * W + x, i = p * 4;
    float p4[4], n4[4], q4[4], m4[4];
    writeTexel(bvh, d, best, p4, n4);
    writeMotionTexel(bvh, prev, o, prevEye, eyeDelta, d, best, p4, n4, q4, m4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        positions[i + k] = p4[k];
        if (normals) normals[i + k] = n4[k];
        prevPoints[i + k] = q4[k];
        prevPointNormals[i + k] = m4[k];
    }
    if (leaves) leaves[p] = best.leaf;
}
} // namespace rts_harness

extern "C" size_t rtsh_ctx_bvh_count(rts_ctx* ctx);   // rts_api.cpp

extern "C" int rtsh_primary_gbuffer_motion_device(rts_ctx* ctx, const rts_vec4u* d_prev_packed, size_t prev_count_vec4, const float eye[3],
                                                  const float prev_eye[3], const float target[3], float fovy, uint32_t W, uint32_t H,
                                                  float* d_positions, float* d_normals, float* d_prev_points, float* d_prev_point_normals,
                                                  uint32_t* d_leaves, void* stream) {
    if (!ctx || !d_prev_packed) return RTS_ERR_INVALID_ARG;
    rts_harness::V3 prevEye, eyeDelta;
    const int s = rts_harness::makeMotionEyes(eye, prev_eye, target, d_positions, d_prev_points, d_prev_point_normals, W, H, &prevEye, &eyeDelta);
    if (s != RTS_OK) return s;
    if (H > RTSH_GBUFFER_MAX_HEIGHT) return RTS_ERR_INVALID_ARG;        // the grid's y extent: refused here, not by the launch
    const void* bvh = rts_ctx_device_bvh(ctx);
    if (!bvh) return RTS_ERR_NO_BVH;
    if (prev_count_vec4 != rtsh_ctx_bvh_count(ctx)) return RTS_ERR_INVALID_ARG;
    const rts_harness::Camera cam = rts_harness::makeCamera(eye, target, fovy, W, H);
    return rts_harness::launchPass(ctx, stream, dim3((W + 7) / 8, (H + 7) / 8), dim3(64), 0, rts_harness::gbufferMotionKernel,
                                   (const uint32_t*)bvh, (const uint32_t*)d_prev_packed, cam, prevEye, eyeDelta, W, H, d_positions, d_normals,
                                   d_prev_points, d_prev_point_normals, d_leaves);
}
