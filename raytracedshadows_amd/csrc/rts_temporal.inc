// The temporal accumulation of a light list's visibility on the GPU (include/rts_scene.h: rtsh_accumulate_visibility_list_device).
// The per-pixel rule is the host twin's own source (rts_closest_hit.h: accumulatePixel), compiled with the same flags: no
// contraction, correctly rounded division.  Included at the end of rts_primary.hip (the scene passes' translation unit), whose own
// kernels keep their instruction text.

namespace rts_harness {
int makeTemporalList(const rts_light_list* list, const rtsh_temporal_params* p, const void* positions, const void* normals,
                     const void* visibility, const void* prevPositions, const void* prevNormals, const void* prevVisibility,
                     const void* prevLengths, uint32_t W, uint32_t H, const void* visibilityOut, const void* lengthsOut,
                     TemporalList* out);                                                                                 // rts_scene.cpp
int checkHistoryClamp(const rtsh_history_clamp* clamp, const void* visibility, const void* visibilityOut);              // rts_scene.cpp

// ACCUMULATE KERNEL.  One pixel per lane, one workgroup of 256 lanes per block of 16 x 16 pixels, each of its four waves 16 x 4 of
// them.  Most of the pass's bytes are streamed -- this frame's texel, its visibility, both outputs -- and a wave's row of 16 pixels is
// 256 contiguous bytes of texels and 64 of a float plane: whole cache lines.  The four gathers of a wave's lanes fall in a patch of
// about 17 x 5 texels of the previous frame.  A wave of 8 x 8 pixels has the more compact patch (9 x 9) but halves every contiguous
// run; measured, it was 1.1 to 1.55 times slower on every row and was deleted (EXPERIMENTS.md, DESIGN.md 4.23).  No LDS: where the
// patch lies depends on the data.  The geometry of the four taps is decided once per pixel (a 4-bit mask); the light loop sits
// behind the wave-uniform l < count.  A tap of weight 0 or a rejected tap is never loaded, so a still camera costs one texel and one
// gather per light.  What is streamed once goes non-temporal; the previous frame's texels and history, which neighbours share, plain.
// No buffer needs more than its element type's alignment, so a texel is three dword loads.
struct TemporalDeviceFrames {
    const float *positions, *normals, *visibility, *prevPositions, *prevNormals, *history;
    const uint8_t *map, *prevLengths;
    float* visibilityOut;
    uint8_t* lengthsOut;
    uint64_t W, n;
    __device__ uint64_t at(int x, int y) const { return (uint64_t)y * W + (uint64_t)x; }
    __device__ static V3 streamed(const float* base, uint64_t i) {
        const float* v = base + i * 4;
        return V3{ __builtin_nontemporal_load(v), __builtin_nontemporal_load(v + 1), __builtin_nontemporal_load(v + 2) };
    }
    __device__ static V3 shared(const float* base, uint64_t i) { const float* v = base + i * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ V3 normal(int x, int y) const { return streamed(normals, at(x, y)); }
    __device__ V3 position(int x, int y) const { return streamed(positions, at(x, y)); }
    __device__ uint32_t bits(int x, int y) const { return map ? __builtin_nontemporal_load(map + at(x, y)) : 0xFFu; }
    __device__ uint32_t current(uint32_t l, int x, int y) const {
        return __float_as_uint(__builtin_nontemporal_load(visibility + (uint64_t)l * n + at(x, y)));      // (a register move: the bits stay)
    }
    __device__ V3 prevNormal(int x, int y) const { return shared(prevNormals, at(x, y)); }
    __device__ V3 prevPosition(int x, int y) const { return shared(prevPositions, at(x, y)); }
    __device__ uint32_t prevLength(uint32_t l, int x, int y) const { return prevLengths[(uint64_t)l * n + at(x, y)]; }
    __device__ float prevVisibility(uint32_t l, int x, int y) const { return history[(uint64_t)l * n + at(x, y)]; }
    __device__ void store(uint32_t l, int x, int y, uint32_t bits, uint32_t length) const {
        __builtin_nontemporal_store(__uint_as_float(bits), visibilityOut + (uint64_t)l * n + at(x, y));
        __builtin_nontemporal_store((uint8_t)length, lengthsOut + (uint64_t)l * n + at(x, y));
    }
};

__global__ __launch_bounds__(256) void accumulateListKernel(TemporalList f, TemporalDeviceFrames t, int W, int H) {
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    accumulatePixel(f, t, x, y, W, H);
}

// CLAMPED ACCUMULATE KERNEL (rtsh_accumulate_visibility_list_clamped_device).  The parent's shape -- 256 lanes per block of 16 x 16
// pixels, four waves of 16 x 4, one pixel per lane, the pixel's own streams non-temporal -- in front of which the block builds every
// pixel's box in LDS.  S = 16 + 2r <= 24 is the side of the block's window.
//   ACTIVITY, once per block: one byte per window pixel, (not background) AND the map byte AND the list's bits; 0 outside the frame.
//   Per light that can blend (below), one at a time through the same LDS:
//     KEYS: the window's S x S keys, kClampNoKey where the pixel is inactive for the light or its value a NaN;          barrier A
//     ROWS: for each of the S window rows and 16 pixel columns the min and max over 2r + 1 keys (kClampNoKey never wins a minimum
//           and counts as 0 in a maximum: no key of a float is 0);                                                     barrier B
//     COLUMNS: each lane reduces 2r + 1 row results to its pixel's box, kept in two registers per light.
//   Then the lanes inside the frame run accumulatePixel<true>, whose box() reads those registers.
// Window values are read with plain loads (neighbouring blocks share them); the normals and map bytes the pixel rule streams again
// come from the cache the staging just filled.
// BARRIERS: every condition around a barrier is a function of kernel arguments alone (f.count, f.history, f.maxLength, f.resetLights,
// radius), so all four waves of a block reach each barrier or none does; lanes outside the frame stage, reduce and wait like the
// others and only skip the pixel rule, which has no barrier.  A light's KEYS may be written while a slow wave still reduces the
// previous light's COLUMNS: those read the row arrays only, and nobody writes the row arrays before barrier A of the next light, which
// that wave must reach first.  Boxes are needed only where a value is blended: the first frame and max_length 1 skip all of them, a
// reset light skips its own (DESIGN.md 4.24).
struct ClampedDeviceFrames : TemporalDeviceFrames {
    uint32_t lo[8], hi[8];
    __device__ bool box(uint32_t l, int, int, uint32_t* loKey, uint32_t* hiKey) const {
        *loKey = lo[l];
        *hiKey = hi[l];
        return lo[l] != kClampNoKey;
    }
};

__global__ __launch_bounds__(256) void accumulateListClampedKernel(TemporalList f, TemporalDeviceFrames t, int W, int H, int radius,
                                                                   float margin) {
    enum { S_MAX = 16 + 2 * RTSH_CLAMP_MAX_RADIUS };
    __shared__ uint8_t activity[S_MAX * S_MAX];
    __shared__ uint32_t keys[S_MAX * S_MAX], rowLo[S_MAX * 16], rowHi[S_MAX * 16];
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y, lane = ty * 16 + tx;
    const int x = (int)blockIdx.x * 16 + tx, y = (int)blockIdx.y * 16 + ty;
    const int S = 16 + 2 * radius, taps = 2 * radius + 1;
    const int x0 = (int)blockIdx.x * 16 - radius, y0 = (int)blockIdx.y * 16 - radius;
    ClampedDeviceFrames c{ t, {}, {} };
#pragma unroll
    for (int l = 0; l < 8; ++l) { c.lo[l] = kClampNoKey; c.hi[l] = 0u; }
    const uint32_t all = (1u << f.count) - 1u;
    const uint32_t boxed = (f.history != 0u && f.maxLength > 1u) ? (all & ~f.resetLights) : 0u;      // lights that can blend: block-uniform
    if (boxed != 0u) {
        int wx[3], wy[3];                                              // the lane's window pixels, lane + 256 k: divided once
#pragma unroll
        for (int k = 0; k < 3; ++k) { wx[k] = x0 + (lane + 256 * k) % S; wy[k] = y0 + (lane + 256 * k) / S; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = lane + 256 * k;
            if (i >= S * S) break;
            uint32_t a = 0u;
            if (wx[k] >= 0 && wx[k] < W && wy[k] >= 0 && wy[k] < H) {
                const uint64_t q = t.at(wx[k], wy[k]);
                if (!isBackground(TemporalDeviceFrames::shared(t.normals, q))) a = (t.map ? (uint32_t)t.map[q] : 0xFFu) & all;
            }
            activity[i] = (uint8_t)a;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l) {
            if (l >= f.count) break;
            if (!((boxed >> l) & 1u)) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int i = lane + 256 * k;
                if (i >= S * S) break;
                uint32_t key = kClampNoKey;
                if ((activity[i] >> l) & 1u) {                           // (set only inside the frame)
                    const uint32_t u = __float_as_uint(t.visibility[(uint64_t)l * t.n + t.at(wx[k], wy[k])]);
                    if (!bitsAreNaN(u)) key = clampKey(u);
                }
                keys[i] = key;
            }
            __syncthreads();                                                                                             // barrier A
            for (int i = lane; i < S * 16; i += 256) {
                const uint32_t* row = keys + (i >> 4) * S + (i & 15);
                uint32_t lo = kClampNoKey, hi = 0u;
                for (int d = 0; d < taps; ++d) {
                    const uint32_t k = row[d];
                    lo = k < lo ? k : lo;
                    hi = (k != kClampNoKey && k > hi) ? k : hi;
                }
                rowLo[i] = lo;
                rowHi[i] = hi;
            }
            __syncthreads();                                                                                             // barrier B
            uint32_t lo = kClampNoKey, hi = 0u;
            for (int d = 0; d < taps; ++d) {
                const uint32_t a = rowLo[(ty + d) * 16 + tx], b = rowHi[(ty + d) * 16 + tx];
                lo = a < lo ? a : lo;
                hi = b > hi ? b : hi;
            }
            c.lo[l] = lo;
            c.hi[l] = hi;
        }
    }
    if (x >= W || y >= H) return;                                                                     // (after the last barrier)
    accumulatePixel<true>(f, c, x, y, W, H, margin);
}

// MOTION FORMS (rtsh_accumulate_visibility_list_motion_device, ..._clamped_motion_device; DESIGN.md 4.29).  SIBLINGS of the two kernels
// above in their shape; accumulatePixel<Clamped, true> takes Q and M_p from this frame's two motion texels, each read once by its own
// pixel: non-temporal, like the pixel's other streams.  The current position is not read at all.  The clamped sibling repeats the
// parent's staging statement for statement (the barriers' conditions are the same functions of kernel arguments alone).
template <class Base>
struct MotionDeviceFrames : Base {
    const float *prevPoints, *prevPointNormals;
    __device__ V3 prevPoint(int x, int y) const { return TemporalDeviceFrames::streamed(prevPoints, this->at(x, y)); }
    __device__ V3 prevPointNormal(int x, int y) const { return TemporalDeviceFrames::streamed(prevPointNormals, this->at(x, y)); }
};

__global__ __launch_bounds__(256) void accumulateListMotionKernel(TemporalList f, TemporalDeviceFrames t, const float* prevPoints,
                                                                  const float* prevPointNormals, int W, int H) {
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const MotionDeviceFrames<TemporalDeviceFrames> m{ t, prevPoints, prevPointNormals };
    accumulatePixel<false, true>(f, m, x, y, W, H);
}

__global__ __launch_bounds__(256) void accumulateListClampedMotionKernel(TemporalList f, TemporalDeviceFrames t, const float* prevPoints,
                                                                         const float* prevPointNormals, int W, int H, int radius,
                                                                         float margin) {
    enum { S_MAX = 16 + 2 * RTSH_CLAMP_MAX_RADIUS };
    __shared__ uint8_t activity[S_MAX * S_MAX];
    __shared__ uint32_t keys[S_MAX * S_MAX], rowLo[S_MAX * 16], rowHi[S_MAX * 16];
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y, lane = ty * 16 + tx;
    const int x = (int)blockIdx.x * 16 + tx, y = (int)blockIdx.y * 16 + ty;
    const int S = 16 + 2 * radius, taps = 2 * radius + 1;
    const int x0 = (int)blockIdx.x * 16 - radius, y0 = (int)blockIdx.y * 16 - radius;
    MotionDeviceFrames<ClampedDeviceFrames> c{ { t, {}, {} }, prevPoints, prevPointNormals };
#pragma unroll
    for (int l = 0; l < 8; ++l) { c.lo[l] = kClampNoKey; c.hi[l] = 0u; }
    const uint32_t all = (1u << f.count) - 1u;
    const uint32_t boxed = (f.history != 0u && f.maxLength > 1u) ? (all & ~f.resetLights) : 0u;      // lights that can blend: block-uniform
    if (boxed != 0u) {
        int wx[3], wy[3];                                              // the lane's window pixels, lane + 256 k: divided once
#pragma unroll
        for (int k = 0; k < 3; ++k) { wx[k] = x0 + (lane + 256 * k) % S; wy[k] = y0 + (lane + 256 * k) / S; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = lane + 256 * k;
            if (i >= S * S) break;
            uint32_t a = 0u;
            if (wx[k] >= 0 && wx[k] < W && wy[k] >= 0 && wy[k] < H) {
                const uint64_t q = t.at(wx[k], wy[k]);
                if (!isBackground(TemporalDeviceFrames::shared(t.normals, q))) a = (t.map ? (uint32_t)t.map[q] : 0xFFu) & all;
            }
            activity[i] = (uint8_t)a;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l) {
            if (l >= f.count) break;
            if (!((boxed >> l) & 1u)) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int i = lane + 256 * k;
                if (i >= S * S) break;
                uint32_t key = kClampNoKey;
                if ((activity[i] >> l) & 1u) {                           // (set only inside the frame)
                    const uint32_t u = __float_as_uint(t.visibility[(uint64_t)l * t.n + t.at(wx[k], wy[k])]);
                    if (!bitsAreNaN(u)) key = clampKey(u);
                }
                keys[i] = key;
            }
            __syncthreads();                                                                                             // barrier A
            for (int i = lane; i < S * 16; i += 256) {
                const uint32_t* row = keys + (i >> 4) * S + (i & 15);
                uint32_t lo = kClampNoKey, hi = 0u;
                for (int d = 0; d < taps; ++d) {
                    const uint32_t k = row[d];
                    lo = k < lo ? k : lo;
                    hi = (k != kClampNoKey && k > hi) ? k : hi;
                }
                rowLo[i] = lo;
                rowHi[i] = hi;
            }
            __syncthreads();                                                                                             // barrier B
            uint32_t lo = kClampNoKey, hi = 0u;
            for (int d = 0; d < taps; ++d) {
                const uint32_t a = rowLo[(ty + d) * 16 + tx], b = rowHi[(ty + d) * 16 + tx];
                lo = a < lo ? a : lo;
                hi = b > hi ? b : hi;
            }
            c.lo[l] = lo;
            c.hi[l] = hi;
        }
    }
    if (x >= W || y >= H) return;                                                                     // (after the last barrier)
    accumulatePixel<true, true>(f, c, x, y, W, H, margin);
}
int checkMotionPlanes(uint32_t history, const void* prevPoints, const void* prevPointNormals);                          // rts_scene.cpp
} // namespace rts_harness

extern "C" int rtsh_accumulate_visibility_list_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_temporal_params* params,
                                                      const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                      const float* d_visibility, const float* d_prev_positions,
                                                      const float* d_prev_normals, const float* d_prev_visibility,
                                                      const uint8_t* d_prev_lengths, uint32_t W, uint32_t H, float* d_visibility_out,
                                                      uint8_t* d_lengths_out, void* stream) {
    if (!ctx) return RTS_ERR_INVALID_ARG;
    rts_harness::TemporalList f;
    const int s = rts_harness::makeTemporalList(list, params, d_positions, d_normals, d_visibility, d_prev_positions, d_prev_normals,
                                                d_prev_visibility, d_prev_lengths, W, H, d_visibility_out, d_lengths_out, &f);
    if (s != RTS_OK) return s;
    // W, H <= 65536 (makeTemporalList): at most 4096 x 4096 blocks, inside every grid limit
    const rts_harness::TemporalDeviceFrames t{ d_positions, d_normals, d_visibility, d_prev_positions, d_prev_normals, d_prev_visibility,
                                               d_lights_map, d_prev_lengths, d_visibility_out, d_lengths_out, W, (uint64_t)W * H };
    return rts_harness::launchPass(ctx, stream, dim3((W + 15) / 16, (H + 15) / 16), dim3(16, 16), 0, rts_harness::accumulateListKernel, f, t,
                                   (int)W, (int)H);
}

extern "C" int rtsh_accumulate_visibility_list_clamped_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_temporal_params* params,
                                                              const float* d_positions, const float* d_normals,
                                                              const uint8_t* d_lights_map, const float* d_visibility,
                                                              const float* d_prev_positions, const float* d_prev_normals,
                                                              const float* d_prev_visibility, const uint8_t* d_prev_lengths, uint32_t W,
                                                              uint32_t H, float* d_visibility_out, uint8_t* d_lengths_out,
                                                              const rtsh_history_clamp* clamp, void* stream) {
    if (!ctx) return RTS_ERR_INVALID_ARG;
    rts_harness::TemporalList f;
    int s = rts_harness::makeTemporalList(list, params, d_positions, d_normals, d_visibility, d_prev_positions, d_prev_normals,
                                          d_prev_visibility, d_prev_lengths, W, H, d_visibility_out, d_lengths_out, &f);
    if (s == RTS_OK) s = rts_harness::checkHistoryClamp(clamp, d_visibility, d_visibility_out);
    if (s != RTS_OK) return s;
    const rts_harness::TemporalDeviceFrames t{ d_positions, d_normals, d_visibility, d_prev_positions, d_prev_normals, d_prev_visibility,
                                               d_lights_map, d_prev_lengths, d_visibility_out, d_lengths_out, W, (uint64_t)W * H };
    return rts_harness::launchPass(ctx, stream, dim3((W + 15) / 16, (H + 15) / 16), dim3(16, 16), 0, rts_harness::accumulateListClampedKernel,
                                   f, t, (int)W, (int)H, (int)clamp->radius, clamp->margin);
}

extern "C" int rtsh_accumulate_visibility_list_motion_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_temporal_params* params,
                                                             const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                             const float* d_visibility, const float* d_prev_positions,
                                                             const float* d_prev_normals, const float* d_prev_visibility,
                                                             const uint8_t* d_prev_lengths, const float* d_prev_points,
                                                             const float* d_prev_point_normals, uint32_t W, uint32_t H,
                                                             float* d_visibility_out, uint8_t* d_lengths_out, void* stream) {
    if (!ctx) return RTS_ERR_INVALID_ARG;
    rts_harness::TemporalList f;
    int s = rts_harness::makeTemporalList(list, params, d_positions, d_normals, d_visibility, d_prev_positions, d_prev_normals,
                                          d_prev_visibility, d_prev_lengths, W, H, d_visibility_out, d_lengths_out, &f);
    if (s == RTS_OK) s = rts_harness::checkMotionPlanes(f.history, d_prev_points, d_prev_point_normals);
    if (s != RTS_OK) return s;
    const rts_harness::TemporalDeviceFrames t{ d_positions, d_normals, d_visibility, d_prev_positions, d_prev_normals, d_prev_visibility,
                                               d_lights_map, d_prev_lengths, d_visibility_out, d_lengths_out, W, (uint64_t)W * H };
    return rts_harness::launchPass(ctx, stream, dim3((W + 15) / 16, (H + 15) / 16), dim3(16, 16), 0, rts_harness::accumulateListMotionKernel,
                                   f, t, d_prev_points, d_prev_point_normals, (int)W, (int)H);
}

extern "C" int rtsh_accumulate_visibility_list_clamped_motion_device(rts_ctx* ctx, const rts_light_list* list,
                                                                     const rtsh_temporal_params* params, const float* d_positions,
                                                                     const float* d_normals, const uint8_t* d_lights_map,
                                                                     const float* d_visibility, const float* d_prev_positions,
                                                                     const float* d_prev_normals, const float* d_prev_visibility,
                                                                     const uint8_t* d_prev_lengths, const float* d_prev_points,
                                                                     const float* d_prev_point_normals, uint32_t W, uint32_t H,
                                                                     float* d_visibility_out, uint8_t* d_lengths_out,
                                                                     const rtsh_history_clamp* clamp, void* stream) {
    if (!ctx) return RTS_ERR_INVALID_ARG;
    rts_harness::TemporalList f;
    int s = rts_harness::makeTemporalList(list, params, d_positions, d_normals, d_visibility, d_prev_positions, d_prev_normals,
                                          d_prev_visibility, d_prev_lengths, W, H, d_visibility_out, d_lengths_out, &f);
    if (s == RTS_OK) s = rts_harness::checkHistoryClamp(clamp, d_visibility, d_visibility_out);
    if (s == RTS_OK) s = rts_harness::checkMotionPlanes(f.history, d_prev_points, d_prev_point_normals);
    if (s != RTS_OK) return s;
    const rts_harness::TemporalDeviceFrames t{ d_positions, d_normals, d_visibility, d_prev_positions, d_prev_normals, d_prev_visibility,
                                               d_lights_map, d_prev_lengths, d_visibility_out, d_lengths_out, W, (uint64_t)W * H };
    return rts_harness::launchPass(ctx, stream, dim3((W + 15) / 16, (H + 15) / 16), dim3(16, 16), 0,
                                   rts_harness::accumulateListClampedMotionKernel, f, t, d_prev_points, d_prev_point_normals, (int)W, (int)H,
                                   (int)clamp->radius, clamp->margin);
}
