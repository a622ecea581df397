// The temporal accumulation of a soft light list's count moments, and the guided wide filter whose threshold reads them, on the GPU
// (include/rts_scene.h: rtsh_accumulate_moments_soft_light_list_device, rtsh_wide_filter_guided_temporal_soft_light_list_device).  The
// per-pixel rules are the host twin's own source (rts_closest_hit.h: accumulateMomentsPixel, wideGuideTemporalThresholdPixel,
// wideGuidedPassPixel), compiled with the same flags.  Included at the end of rts_primary.hip after rts_wide_guided.inc; every kernel
// in front of it keeps its instruction text: both kernels here are SIBLINGS, nothing above is touched.

namespace rts_harness {
int makeMomentsList(const rts_soft_light_list* list, const rtsh_temporal_params* p, const void* positions, const void* normals,
                    const void* counts, const void* prevPositions, const void* prevNormals, const void* prevMean, const void* prevSquare,
                    const void* prevLengths, uint32_t W, uint32_t H, const void* meanOut, const void* squareOut, const void* lengthsOut,
                    MomentsList* out);                                                                                  // rts_scene.cpp
int makeWideGuidedTemporalList(const rts_soft_light_list* list, const rtsh_wide_guide_temporal_params* p, uint32_t W, uint32_t H,
                               WideFilterList* out);                                                                    // rts_scene.cpp

// MOMENTS KERNEL.  accumulateListKernel's shape, for its reasons (rts_temporal.inc): one pixel per lane, 256 lanes per block of 16 x 16
// pixels, four waves of 16 x 4, no LDS -- where the gathered patch lies depends on the data.  The geometry of the four taps is decided
// once per pixel; the light loop sits behind the wave-uniform l < count; a tap of weight 0 or a rejected tap is never loaded.  What is
// streamed once -- this frame's texel, map byte and count bytes, the three outputs -- goes non-temporal; the previous frame's texels
// and history (1 + 2 + 4 bytes per tap and light), which neighbours share, plain.  Every load is of its element type's size.
struct MomentsDeviceFrames {
    const float *positions, *normals, *prevPositions, *prevNormals;
    const uint8_t *map, *counts, *prevLengths;
    const uint16_t* prevMeans;
    const uint32_t* prevSquares;
    uint16_t* meanOut;
    uint32_t* squareOut;
    uint8_t* lengthsOut;
    uint64_t W, n;
    __device__ uint64_t at(int x, int y) const { return (uint64_t)y * W + (uint64_t)x; }
    __device__ V3 normal(int x, int y) const { return TemporalDeviceFrames::streamed(normals, at(x, y)); }
    __device__ V3 position(int x, int y) const { return TemporalDeviceFrames::streamed(positions, at(x, y)); }
    __device__ uint32_t bits(int x, int y) const { return map ? __builtin_nontemporal_load(map + at(x, y)) : 0xFFu; }
    __device__ uint32_t count(uint32_t l, int x, int y) const { return __builtin_nontemporal_load(counts + (uint64_t)l * n + at(x, y)); }
    __device__ V3 prevNormal(int x, int y) const { return TemporalDeviceFrames::shared(prevNormals, at(x, y)); }
    __device__ V3 prevPosition(int x, int y) const { return TemporalDeviceFrames::shared(prevPositions, at(x, y)); }
    __device__ uint32_t prevLength(uint32_t l, int x, int y) const { return prevLengths[(uint64_t)l * n + at(x, y)]; }
    __device__ uint32_t prevMean(uint32_t l, int x, int y) const { return prevMeans[(uint64_t)l * n + at(x, y)]; }
    __device__ uint32_t prevSquare(uint32_t l, int x, int y) const { return prevSquares[(uint64_t)l * n + at(x, y)]; }
    __device__ void store(uint32_t l, int x, int y, uint32_t mean, uint32_t square, uint32_t length) const {
        __builtin_nontemporal_store((uint16_t)mean, meanOut + (uint64_t)l * n + at(x, y));
        __builtin_nontemporal_store(square, squareOut + (uint64_t)l * n + at(x, y));
        __builtin_nontemporal_store((uint8_t)length, lengthsOut + (uint64_t)l * n + at(x, y));
    }
};

__global__ __launch_bounds__(256) void accumulateMomentsKernel(MomentsList f, MomentsDeviceFrames t, int W, int H) {
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    accumulateMomentsPixel(f, t, x, y, W, H);
}

// MOTION FORM (rtsh_accumulate_moments_soft_light_list_motion_device; DESIGN.md 4.29): a SIBLING of the kernel above in its shape;
// accumulateMomentsPixel<true> takes Q and M_p from this frame's two motion texels, each read once by its own pixel: non-temporal.
struct MotionMomentsDeviceFrames : MomentsDeviceFrames {
    const float *prevPoints, *prevPointNormals;
    __device__ V3 prevPoint(int x, int y) const { return TemporalDeviceFrames::streamed(prevPoints, at(x, y)); }
    __device__ V3 prevPointNormal(int x, int y) const { return TemporalDeviceFrames::streamed(prevPointNormals, at(x, y)); }
};

__global__ __launch_bounds__(256) void accumulateMomentsMotionKernel(MomentsList f, MomentsDeviceFrames t, const float* prevPoints,
                                                                     const float* prevPointNormals, int W, int H) {
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const MotionMomentsDeviceFrames m{ t, prevPoints, prevPointNormals };
    accumulateMomentsPixel<true>(f, m, x, y, W, H);
}

// CLAMPED MOMENTS KERNEL (rtsh_accumulate_moments_soft_light_list_clamped_device and its motion form; DESIGN.md 4.30).
// accumulateListClampedKernel's shape, for its reasons (rts_temporal.inc, DESIGN.md 4.24): 256 lanes per block of 16 x 16 pixels, four
// waves of 16 x 4, one pixel per lane, in front of which the block builds every pixel's box in LDS.  S = 16 + 2r <= 24 is the side of
// the block's window.
//   ACTIVITY, once per block: one byte per window pixel, (not background) AND the map byte AND the list's bits; 0 outside the frame.
//   Per light that can blend (below), ONE LIGHT AT A TIME through the same LDS (all lights at once was not built: eight times the
//   row arrays would take a block from 9 KiB to about 60 KiB and the CU from sixteen resident blocks to two):
//     VALUES: the window's S x S values V_0 as 32-bit words, kNoValue where the pixel does not contribute;              barrier A
//     ROWS: for each of the S window rows and 16 pixel columns, over 2r + 1 words: min and max (one packed word), count and sum
//           (count <= 9 in bits 20.., sum <= 9 * 65535 < 2^20: one packed word) and the sum of squares (<= 9 * 2^32: 64 bits); barrier B
//     COLUMNS: each lane reduces 2r + 1 row results to its pixel's (m, S1, S2, lo, hi), then momentsClampBounds -- the source that
//           rtsh_moments_clamp_bounds exports -- to (Lv', Hv'), kept packed in ONE register per light.  The bounds are evaluated
//           only where the lane's own pixel is active for the light (there m >= 1: the centre contributes); this branch holds no
//           barrier.
//   Then the lanes inside the frame run accumulateMomentsPixel<Motion, true>, whose box() unpacks that register.
// Window counts are read with plain loads (neighbouring blocks share them); the pixel's own streams stay non-temporal.
// BARRIERS: every condition around a barrier is a function of kernel arguments alone (f.t.count, f.t.history, f.t.maxLength,
// f.t.resetLights, radius), so all four waves of a block reach each barrier or none does; lanes outside the frame stage, reduce and
// wait like the others and only skip the bounds and the pixel rule, which hold no barrier.  A light's VALUES may be written while a
// slow wave still reduces the previous light's COLUMNS: those read the row arrays only, and nobody writes the row arrays before
// barrier A of the next light, which that wave must reach first.  Boxes are needed only where a pair is blended: the first frame and
// max_length 1 skip all of them, a reset light skips its own.
enum : uint32_t { kNoValue = 0xFFFFFFFFu };

template <class Base>
struct ClampedMomentsDeviceFrames : Base {
    uint32_t bounds[8];                                                // Hv' << 16 | Lv'
    __device__ void box(uint32_t l, int, int, uint32_t* Lv, uint32_t* Hv) const {
        *Lv = bounds[l] & 0xFFFFu;
        *Hv = bounds[l] >> 16;
    }
};

template <bool Motion>
__global__ __launch_bounds__(256) void accumulateMomentsClampedKernel(MomentsList f, MomentsDeviceFrames t, const float* prevPoints,
                                                                      const float* prevPointNormals, int W, int H, int radius,
                                                                      uint32_t k4, uint32_t margin) {
    enum { S_MAX = 16 + 2 * RTSH_MOMENTS_CLAMP_MAX_RADIUS };
    __shared__ uint8_t activity[S_MAX * S_MAX];
    __shared__ uint32_t values[S_MAX * S_MAX], rowLoHi[S_MAX * 16], rowCountSum[S_MAX * 16];
    __shared__ uint64_t rowSquares[S_MAX * 16];
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y, lane = ty * 16 + tx;
    const int x = (int)blockIdx.x * 16 + tx, y = (int)blockIdx.y * 16 + ty;
    const int S = 16 + 2 * radius, taps = 2 * radius + 1;
    const int x0 = (int)blockIdx.x * 16 - radius, y0 = (int)blockIdx.y * 16 - radius;
    using Frames = typename std::conditional<Motion, MotionMomentsDeviceFrames, MomentsDeviceFrames>::type;
    ClampedMomentsDeviceFrames<Frames> c;
    if constexpr (Motion) static_cast<Frames&>(c) = Frames{ t, prevPoints, prevPointNormals };
    else static_cast<Frames&>(c) = t;
#pragma unroll
    for (int l = 0; l < 8; ++l) c.bounds[l] = 0xFFFF0000u;             // (never read: box() is asked at blended pairs, all of them boxed)
    const uint32_t all = (1u << f.t.count) - 1u;
    const uint32_t boxed = (f.t.history != 0u && f.t.maxLength > 1u) ? (all & ~f.t.resetLights) : 0u;   // lights that can blend: block-uniform
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
        const uint32_t own = activity[(ty + radius) * S + tx + radius];  // the lane's own pixel: 0 outside the frame
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l) {
            if (l >= f.t.count) break;
            if (!((boxed >> l) & 1u)) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int i = lane + 256 * k;
                if (i >= S * S) break;
                uint32_t v = kNoValue;
                if ((activity[i] >> l) & 1u)                             // (set only inside the frame)
                    v = wideFilterInput(t.counts[(uint64_t)l * t.n + t.at(wx[k], wy[k])], f.samples[l], f.scale[l]);
                values[i] = v;
            }
            __syncthreads();                                                                                             // barrier A
            for (int i = lane; i < S * 16; i += 256) {
                const uint32_t* row = values + (i >> 4) * S + (i & 15);
                uint32_t lo = 0xFFFFu, hi = 0u, countSum = 0u;
                uint64_t squares = 0u;
                for (int d = 0; d < taps; ++d) {
                    const uint32_t v = row[d];
                    if (v == kNoValue) continue;
                    lo = v < lo ? v : lo;
                    hi = v > hi ? v : hi;
                    countSum += (1u << 20) + v;
                    squares += (uint64_t)(v * v);
                }
                rowLoHi[i] = hi << 16 | lo;
                rowCountSum[i] = countSum;
                rowSquares[i] = squares;
            }
            __syncthreads();                                                                                             // barrier B
            uint32_t lo = 0xFFFFu, hi = 0u, m = 0u;
            uint64_t S1 = 0u, S2 = 0u;
            for (int d = 0; d < taps; ++d) {
                const int i = (ty + d) * 16 + tx;
                const uint32_t a = rowLoHi[i], b = rowCountSum[i];
                lo = (a & 0xFFFFu) < lo ? (a & 0xFFFFu) : lo;
                hi = (a >> 16) > hi ? (a >> 16) : hi;
                m += b >> 20;
                S1 += b & 0xFFFFFu;
                S2 += rowSquares[i];
            }
            if ((own >> l) & 1u) {                                       // (no barrier inside; m >= 1 here)
                uint32_t lv, hv;
                momentsClampBounds(m, S1, S2, lo, hi, k4, margin, &lv, &hv);
                c.bounds[l] = hv << 16 | lv;
            }
        }
    }
    if (x >= W || y >= H) return;                                                                     // (after the last barrier)
    accumulateMomentsPixel<Motion, true>(f, c, x, y, W, H);
}

// THE FIRST PASS OF THE TEMPORAL GUIDE: wideGuidedKernel<true, LAST, DENSE> with wideGuideTemporalThresholdPixel in the place of
// wideGuideThresholdPixel -- a sibling, so that every instantiation of wideGuidedKernel keeps its text; later passes ARE
// wideGuidedKernel<false, ...>, which read T from the third set of the scratch.  The staging loop is wideFilterKernel's, statement for
// statement.  The nine (length, mean, square) triples per light are loaded from GLOBAL memory, not staged: 7 bytes per texel and light
// beside the window's 25 + 2 * count would take the step-1 window of eight lights (pitch 48 x 20 rows) from 39 KiB to 92 KiB, beyond
// the 64 KiB a workgroup gets without opting in, and a compact 18 x 18 side array (18 KiB more) would still cut the workgroups per CU
// from four to two (160 KiB of LDS) for a read that neighbouring lanes share through the vector cache anyway: a wave's row of 16
// pixels reads 18 consecutive elements of a plane's row.  `length` is read first; the moments only where it reaches minHistory.
template <bool LAST, bool DENSE>
__global__ __launch_bounds__(256) void wideGuidedTemporalKernel(WideFilterList f, uint32_t k4, uint32_t minHistory, GuideMoments h,
                                                                const float* positions, const float* normals, const uint8_t* lightsMap,
                                                                const void* in, int W, int H, int step, int pitch, void* out,
                                                                uint16_t* guide) {
    const uint32_t count = f.count;
    const uint64_t n = (uint64_t)W * (uint64_t)H;
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    const uint64_t p = (uint64_t)y * (uint64_t)W + (uint64_t)x;
    uint32_t v[8], T[8];
    auto storeGuide = [&]() {
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l) {
            if (l >= count) break;
            guide[(uint64_t)l * n + p] = (uint16_t)T[l];
        }
    };
#pragma unroll
    for (uint32_t l = 0; l < 8; ++l) T[l] = 0u;
    if constexpr (DENSE) {
        extern __shared__ __align__(16) unsigned char lds[];
        const int reach = 2 * step, TW = 16 + 2 * reach, cells = pitch * TW;
        float2* sa = (float2*)lds;
        float2* sb = sa + cells;
        float2* sc = sb + cells;
        uint16_t* svalues = (uint16_t*)(sc + cells);
        uint8_t* smap = (uint8_t*)(svalues + count * cells);
        const int x0 = (int)blockIdx.x * 16 - reach, y0 = (int)blockIdx.y * 16 - reach;
        const int tid = (int)(threadIdx.y * 16 + threadIdx.x);
        for (int i = tid; i < TW * TW; i += 256) {
            const int ty = i / TW, tx = i - ty * TW, gx = x0 + tx, gy = y0 + ty, s = ty * pitch + tx;
            float nx = 0.f, ny = 0.f, nz = 0.f, px = 0.f, py = 0.f, pz = 0.f;
            uint32_t bits = 0;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const uint64_t g = (uint64_t)gy * (uint64_t)W + (uint64_t)gx;
                nx = normals[g * 4]; ny = normals[g * 4 + 1]; nz = normals[g * 4 + 2];
                if (!(nx == 0.0f && ny == 0.0f && nz == 0.0f)) {       // (a background texel: only its normal is read)
                    px = positions[g * 4]; py = positions[g * 4 + 1]; pz = positions[g * 4 + 2];
                    bits = (lightsMap ? lightsMap[g] : 0xFFu) & ((1u << count) - 1u);
#pragma unroll
                    for (uint32_t l = 0; l < 8; ++l) {
                        if (l >= count) break;
                        if (!((bits >> l) & 1u)) continue;             // (a value whose map bit is clear is neither read nor staged)
                        svalues[l * cells + s] = (uint16_t)wideLoadValue<true, false>(f, in, n, g, l);
                    }
                }
            }
            sa[s] = make_float2(nx, ny); sb[s] = make_float2(nz, px); sc[s] = make_float2(py, pz);
            smap[s] = (uint8_t)bits;
        }
        __syncthreads();
        if (x >= W || y >= H) return;
        const WideTile t{ sa, sb, sc, svalues, smap, x0, y0, pitch, cells };
        wideGuideTemporalThresholdPixel(f, k4, minHistory, t, h, x, y, W, H, T);   // (a DENSE pass has step >= 1)
        if (!LAST) storeGuide();
        wideGuidedPassPixel(f, t, x, y, W, H, step, T, v);
    } else {
        if (x >= W || y >= H) return;
        const WideGlobal<true, false> t{ f, positions, normals, lightsMap, in, (uint64_t)W, n };
        if (step > 0) wideGuideTemporalThresholdPixel(f, k4, minHistory, t, h, x, y, W, H, T);   // (step 0: the conversion needs no T)
        if (!LAST) storeGuide();
        wideGuidedPassPixel(f, t, x, y, W, H, step, T, v);
    }
#pragma unroll
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= count) break;
        if (LAST) ((float*)out)[(uint64_t)l * n + p] = wideFilterOutput(v[l], f.samples[l], f.scale[l]);
        else ((uint16_t*)out)[(uint64_t)l * n + p] = (uint16_t)v[l];
    }
}
} // namespace rts_harness

extern "C" int rtsh_accumulate_moments_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_temporal_params* params,
                                                              const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                              const uint8_t* d_counts, const float* d_prev_positions,
                                                              const float* d_prev_normals, const uint16_t* d_prev_mean,
                                                              const uint32_t* d_prev_square, const uint8_t* d_prev_lengths, uint32_t W,
                                                              uint32_t H, uint16_t* d_mean_out, uint32_t* d_square_out,
                                                              uint8_t* d_lengths_out, void* stream) {
    if (!ctx) return RTS_ERR_INVALID_ARG;
    rts_harness::MomentsList f;
    const int s = rts_harness::makeMomentsList(list, params, d_positions, d_normals, d_counts, d_prev_positions, d_prev_normals, d_prev_mean,
                                               d_prev_square, d_prev_lengths, W, H, d_mean_out, d_square_out, d_lengths_out, &f);
    if (s != RTS_OK) return s;
    // W, H <= 65536 (makeTemporalList): at most 4096 x 4096 blocks, inside every grid limit
    const rts_harness::MomentsDeviceFrames t{ d_positions, d_normals, d_prev_positions, d_prev_normals, d_lights_map, d_counts, d_prev_lengths,
                                              d_prev_mean, d_prev_square, d_mean_out, d_square_out, d_lengths_out, W, (uint64_t)W * H };
    return rts_harness::launchPass(ctx, stream, dim3((W + 15) / 16, (H + 15) / 16), dim3(16, 16), 0, rts_harness::accumulateMomentsKernel, f,
                                   t, (int)W, (int)H);
}

extern "C" int rtsh_accumulate_moments_soft_light_list_motion_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                                     const rtsh_temporal_params* params, const float* d_positions,
                                                                     const float* d_normals, const uint8_t* d_lights_map,
                                                                     const uint8_t* d_counts, const float* d_prev_positions,
                                                                     const float* d_prev_normals, const uint16_t* d_prev_mean,
                                                                     const uint32_t* d_prev_square, const uint8_t* d_prev_lengths,
                                                                     const float* d_prev_points, const float* d_prev_point_normals,
                                                                     uint32_t W, uint32_t H, uint16_t* d_mean_out, uint32_t* d_square_out,
                                                                     uint8_t* d_lengths_out, void* stream) {
    if (!ctx) return RTS_ERR_INVALID_ARG;
    rts_harness::MomentsList f;
    int s = rts_harness::makeMomentsList(list, params, d_positions, d_normals, d_counts, d_prev_positions, d_prev_normals, d_prev_mean,
                                         d_prev_square, d_prev_lengths, W, H, d_mean_out, d_square_out, d_lengths_out, &f);
    if (s == RTS_OK) s = rts_harness::checkMotionPlanes(f.t.history, d_prev_points, d_prev_point_normals);
    if (s != RTS_OK) return s;
    const rts_harness::MomentsDeviceFrames t{ d_positions, d_normals, d_prev_positions, d_prev_normals, d_lights_map, d_counts, d_prev_lengths,
                                              d_prev_mean, d_prev_square, d_mean_out, d_square_out, d_lengths_out, W, (uint64_t)W * H };
    return rts_harness::launchPass(ctx, stream, dim3((W + 15) / 16, (H + 15) / 16), dim3(16, 16), 0,
                                   rts_harness::accumulateMomentsMotionKernel, f, t, d_prev_points, d_prev_point_normals, (int)W, (int)H);
}

namespace rts_harness {
int checkMomentsClamp(const rtsh_moments_clamp* clamp);                                                                // rts_scene.cpp
}

extern "C" int rtsh_accumulate_moments_soft_light_list_clamped_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                                      const rtsh_temporal_params* params, const float* d_positions,
                                                                      const float* d_normals, const uint8_t* d_lights_map,
                                                                      const uint8_t* d_counts, const float* d_prev_positions,
                                                                      const float* d_prev_normals, const uint16_t* d_prev_mean,
                                                                      const uint32_t* d_prev_square, const uint8_t* d_prev_lengths,
                                                                      uint32_t W, uint32_t H, uint16_t* d_mean_out, uint32_t* d_square_out,
                                                                      uint8_t* d_lengths_out, const rtsh_moments_clamp* clamp, void* stream) {
    if (!ctx) return RTS_ERR_INVALID_ARG;
    rts_harness::MomentsList f;
    int s = rts_harness::makeMomentsList(list, params, d_positions, d_normals, d_counts, d_prev_positions, d_prev_normals, d_prev_mean,
                                         d_prev_square, d_prev_lengths, W, H, d_mean_out, d_square_out, d_lengths_out, &f);
    if (s == RTS_OK) s = rts_harness::checkMomentsClamp(clamp);
    if (s != RTS_OK) return s;
    const rts_harness::MomentsDeviceFrames t{ d_positions, d_normals, d_prev_positions, d_prev_normals, d_lights_map, d_counts, d_prev_lengths,
                                              d_prev_mean, d_prev_square, d_mean_out, d_square_out, d_lengths_out, W, (uint64_t)W * H };
    return rts_harness::launchPass(ctx, stream, dim3((W + 15) / 16, (H + 15) / 16), dim3(16, 16), 0,
                                   rts_harness::accumulateMomentsClampedKernel<false>, f, t, (const float*)nullptr, (const float*)nullptr,
                                   (int)W, (int)H, (int)clamp->radius, clamp->sigma_k4, clamp->margin);
}

extern "C" int rtsh_accumulate_moments_soft_light_list_clamped_motion_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                                             const rtsh_temporal_params* params, const float* d_positions,
                                                                             const float* d_normals, const uint8_t* d_lights_map,
                                                                             const uint8_t* d_counts, const float* d_prev_positions,
                                                                             const float* d_prev_normals, const uint16_t* d_prev_mean,
                                                                             const uint32_t* d_prev_square, const uint8_t* d_prev_lengths,
                                                                             const float* d_prev_points, const float* d_prev_point_normals,
                                                                             uint32_t W, uint32_t H, uint16_t* d_mean_out,
                                                                             uint32_t* d_square_out, uint8_t* d_lengths_out,
                                                                             const rtsh_moments_clamp* clamp, void* stream) {
    if (!ctx) return RTS_ERR_INVALID_ARG;
    rts_harness::MomentsList f;
    int s = rts_harness::makeMomentsList(list, params, d_positions, d_normals, d_counts, d_prev_positions, d_prev_normals, d_prev_mean,
                                         d_prev_square, d_prev_lengths, W, H, d_mean_out, d_square_out, d_lengths_out, &f);
    if (s == RTS_OK) s = rts_harness::checkMomentsClamp(clamp);
    if (s == RTS_OK) s = rts_harness::checkMotionPlanes(f.t.history, d_prev_points, d_prev_point_normals);
    if (s != RTS_OK) return s;
    const rts_harness::MomentsDeviceFrames t{ d_positions, d_normals, d_prev_positions, d_prev_normals, d_lights_map, d_counts, d_prev_lengths,
                                              d_prev_mean, d_prev_square, d_mean_out, d_square_out, d_lengths_out, W, (uint64_t)W * H };
    return rts_harness::launchPass(ctx, stream, dim3((W + 15) / 16, (H + 15) / 16), dim3(16, 16), 0,
                                   rts_harness::accumulateMomentsClampedKernel<true>, f, t, d_prev_points, d_prev_point_normals, (int)W, (int)H,
                                   (int)clamp->radius, clamp->sigma_k4, clamp->margin);
}

// The chain of a call is launchWideChain (rts_wide_filter.inc), with three sets and the sibling kernel as its first pass.
extern "C" int rtsh_wide_filter_guided_temporal_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                                       const rtsh_wide_guide_temporal_params* params, const float* d_positions,
                                                                       const float* d_normals, const uint8_t* d_lights_map,
                                                                       const uint8_t* d_counts, const uint16_t* d_mean, const uint32_t* d_square,
                                                                       const uint8_t* d_lengths, uint32_t W, uint32_t H, float* d_visibility,
                                                                       uint16_t* d_scratch, void* stream) {
    using namespace rts_harness;
    if (!ctx || !d_positions || !d_normals || !d_counts || !d_mean || !d_square || !d_lengths || !d_visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int made = makeWideGuidedTemporalList(list, params, W, H, &f);
    if (made != RTS_OK) return made;
    const uint32_t k4 = params->guide_k4, minHistory = params->min_history;
    const GuideMoments h{ d_mean, d_square, d_lengths, W, (uint64_t)W * H };
    auto firstPass = [&](dim3 grid, auto last, int step, void* out, uint16_t* guide) {
        constexpr bool LAST = decltype(last)::value;
        return launchWideKernel(ctx, stream, grid, f, W, H, step, wideGuidedTemporalKernel<LAST, true>, wideGuidedTemporalKernel<LAST, false>,
                                std::make_tuple(k4, minHistory, h, d_positions, d_normals, d_lights_map, (const void*)d_counts), out, guide);
    };
    return launchWideChain(ctx, f, W, H, d_visibility, d_scratch, 3, firstPass,
                           wideGuidedLaterPass(ctx, stream, f, k4, d_positions, d_normals, d_lights_map, W, H));
}
