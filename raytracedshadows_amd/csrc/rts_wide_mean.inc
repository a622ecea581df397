// The wide filters fed from the accumulated mean of a soft light list's count moments, on the GPU (include/rts_scene.h:
// rtsh_wide_filter_mean_soft_light_list_device, rtsh_wide_filter_guided_temporal_mean_soft_light_list_device).  The per-pixel rules are
// the host twin's own source (rts_closest_hit.h: wideMeanInput, wideFilterPassPixel, wideGuideTemporalMeanThresholdPixel,
// wideGuidedPassPixel), compiled with the same flags.  Included at the end of rts_primary.hip after rts_moments.inc; every kernel in
// front of it keeps its instruction text: both kernels here are SIBLINGS, nothing above is touched.
//
// ONLY THE FIRST PASS IS NEW: it forms V_0' = min(mean, n_l * S_l) where the shipped first passes form V_0 from the count byte -- a
// 2-byte load per light in the place of a 1-byte load and a multiply; the window, its pitch, its 25 + 2 * count bytes per texel
// (wideGeometry) and the one barrier are wideFilterKernel's, the staging loop is its loop statement for statement.  Later passes ARE
// wideFilterKernel<false, ...> and wideGuidedKernel<false, ...>.

namespace rts_harness {
// V_0' of pixel g for light l from global memory.
__device__ inline uint32_t wideLoadMean(const WideFilterList& f, const uint16_t* mean, uint64_t n, uint64_t g, uint32_t l) {
    return wideMeanInput(mean[(uint64_t)l * n + g], f.samples[l], f.scale[l]);
}

struct WideMeanGlobal {
    const WideFilterList& f;
    const float *positions, *normals;
    const uint8_t* map;
    const uint16_t* mean;
    uint64_t W, n;
    __device__ uint64_t at(int x, int y) const { return (uint64_t)y * W + (uint64_t)x; }
    __device__ V3 normal(int x, int y) const { const float* v = normals + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ V3 position(int x, int y) const { const float* v = positions + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ uint32_t bits(int x, int y) const { return map ? map[at(x, y)] : 0xFFu; }
    __device__ uint32_t value(int x, int y, uint32_t l) const { return wideLoadMean(f, mean, n, at(x, y), l); }
};

// THE FIRST PASS OF THE UNGUIDED MEAN FILTER: wideFilterKernel<true, LAST, false, DENSE> with wideLoadMean in the place of wideLoadValue.
template <bool LAST, bool DENSE>
__global__ __launch_bounds__(256) void wideMeanKernel(WideFilterList f, const float* positions, const float* normals, const uint8_t* lightsMap,
                                                      const uint16_t* mean, int W, int H, int step, int pitch, void* out) {
    const uint32_t count = f.count;
    const uint64_t n = (uint64_t)W * (uint64_t)H;
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    uint32_t v[8];
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
                        svalues[l * cells + s] = (uint16_t)wideLoadMean(f, mean, n, g, l);
                    }
                }
            }
            sa[s] = make_float2(nx, ny); sb[s] = make_float2(nz, px); sc[s] = make_float2(py, pz);
            smap[s] = (uint8_t)bits;
        }
        __syncthreads();
        if (x >= W || y >= H) return;
        const WideTile t{ sa, sb, sc, svalues, smap, x0, y0, pitch, cells };
        wideFilterPassPixel(f, t, x, y, W, H, step, v);
    } else {
        if (x >= W || y >= H) return;
        const WideMeanGlobal t{ f, positions, normals, lightsMap, mean, (uint64_t)W, n };
        wideFilterPassPixel(f, t, x, y, W, H, step, v);
    }
    const uint64_t p = (uint64_t)y * (uint64_t)W + (uint64_t)x;
#pragma unroll
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= count) break;
        if (LAST) ((float*)out)[(uint64_t)l * n + p] = wideFilterOutput(v[l], f.samples[l], f.scale[l]);
        else ((uint16_t*)out)[(uint64_t)l * n + p] = (uint16_t)v[l];
    }
}

// THE FIRST PASS OF THE GUIDED MEAN FILTER: wideGuidedTemporalKernel<LAST, DENSE> (rts_moments.inc) with the same ONE change of input and
// wideGuideTemporalMeanThresholdPixel in the place of wideGuideTemporalThresholdPixel.  (length, mean, square) of the nine threshold
// pixels come from GLOBAL memory for that kernel's reasons; the count byte of one is read, from global memory too, only where its
// length is below minHistory.
template <bool LAST, bool DENSE>
__global__ __launch_bounds__(256) void wideGuidedTemporalMeanKernel(WideFilterList f, uint32_t k4, uint32_t minHistory, GuideMomentsCounts h,
                                                                    const float* positions, const float* normals, const uint8_t* lightsMap,
                                                                    int W, int H, int step, int pitch, void* out, uint16_t* guide) {
    const uint32_t count = f.count;
    const uint64_t n = (uint64_t)W * (uint64_t)H;
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    const uint64_t p = (uint64_t)y * (uint64_t)W + (uint64_t)x;
    const uint16_t* mean = h.m.mean;
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
                        svalues[l * cells + s] = (uint16_t)wideLoadMean(f, mean, n, g, l);
                    }
                }
            }
            sa[s] = make_float2(nx, ny); sb[s] = make_float2(nz, px); sc[s] = make_float2(py, pz);
            smap[s] = (uint8_t)bits;
        }
        __syncthreads();
        if (x >= W || y >= H) return;
        const WideTile t{ sa, sb, sc, svalues, smap, x0, y0, pitch, cells };
        wideGuideTemporalMeanThresholdPixel(f, k4, minHistory, t, h, x, y, W, H, T);   // (a DENSE pass has step >= 1)
        if (!LAST) storeGuide();
        wideGuidedPassPixel(f, t, x, y, W, H, step, T, v);
    } else {
        if (x >= W || y >= H) return;
        const WideMeanGlobal t{ f, positions, normals, lightsMap, mean, (uint64_t)W, n };
        if (step > 0) wideGuideTemporalMeanThresholdPixel(f, k4, minHistory, t, h, x, y, W, H, T);   // (step 0: the conversion needs no T)
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

template <bool LAST>
static int launchWideMeanFirst(rts_ctx* ctx, void* stream, dim3 grid, const WideFilterList& f, const float* d_positions, const float* d_normals,
                               const uint8_t* d_lights_map, const uint16_t* d_mean, uint32_t W, uint32_t H, int step, void* out) {
    if (step >= 1 && step <= kWideDenseMaxStep) {
        const WideGeometry g = wideGeometry(f.count, step);
        return launchPass(ctx, stream, grid, dim3(16, 16), g.bytes, wideMeanKernel<LAST, true>, f, d_positions, d_normals, d_lights_map, d_mean,
                          (int)W, (int)H, step, g.pitch, out);
    }
    return launchPass(ctx, stream, grid, dim3(16, 16), 0, wideMeanKernel<LAST, false>, f, d_positions, d_normals, d_lights_map, d_mean, (int)W,
                      (int)H, step, 0, out);
}

template <bool LAST>
static int launchWideGuidedTemporalMeanFirst(rts_ctx* ctx, void* stream, dim3 grid, const WideFilterList& f, uint32_t k4, uint32_t minHistory,
                                             const GuideMomentsCounts& h, const float* d_positions, const float* d_normals,
                                             const uint8_t* d_lights_map, uint32_t W, uint32_t H, int step, void* out, uint16_t* guide) {
    if (step >= 1 && step <= kWideDenseMaxStep) {
        const WideGeometry g = wideGeometry(f.count, step);
        return launchPass(ctx, stream, grid, dim3(16, 16), g.bytes, wideGuidedTemporalMeanKernel<LAST, true>, f, k4, minHistory, h, d_positions,
                          d_normals, d_lights_map, (int)W, (int)H, step, g.pitch, out, guide);
    }
    return launchPass(ctx, stream, grid, dim3(16, 16), 0, wideGuidedTemporalMeanKernel<LAST, false>, f, k4, minHistory, h, d_positions,
                      d_normals, d_lights_map, (int)W, (int)H, step, 0, out, guide);
}
} // namespace rts_harness

// The chain of a call: launchWideFilter's, with the sibling kernel as its first pass.
extern "C" int rtsh_wide_filter_mean_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_wide_filter_params* params,
                                                            const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                            const uint16_t* d_mean, uint32_t W, uint32_t H, float* d_visibility,
                                                            uint16_t* d_scratch, void* stream) {
    using namespace rts_harness;
    if (!ctx || !d_positions || !d_normals || !d_mean || !d_visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int made = makeWideFilterSoftList(list, params, W, H, &f);
    if (made != RTS_OK) return made;
    const dim3 grid((W + 15) / 16, (H + 15) / 16);
    if (grid.y > 65535u) return RTS_ERR_INVALID_ARG;
    const size_t half = (size_t)f.count * (size_t)W * (size_t)H;
    if (f.passes >= 2u && !d_scratch) return RTS_ERR_INVALID_ARG;
    if (d_scratch && ((const void*)d_visibility == (const void*)d_scratch || (const void*)d_visibility == (const void*)(d_scratch + half)))
        return RTS_ERR_INVALID_ARG;
    if (f.passes <= 1u)
        return launchWideMeanFirst<true>(ctx, stream, grid, f, d_positions, d_normals, d_lights_map, d_mean, W, H, (int)f.passes, d_visibility);
    for (uint32_t k = 0; k < f.passes; ++k) {
        const int step = 1 << k;
        const void* in = k == 0 ? nullptr : (const void*)(d_scratch + ((k - 1u) & 1u) * half);
        uint16_t* mid = d_scratch + (k & 1u) * half;
        int s;
        if (k == 0) s = launchWideMeanFirst<false>(ctx, stream, grid, f, d_positions, d_normals, d_lights_map, d_mean, W, H, step, mid);
        else if (k + 1u < f.passes)
            s = launchWidePass<false, false, false>(ctx, stream, grid, f, d_positions, d_normals, d_lights_map, in, W, H, step, mid);
        else s = launchWidePass<false, true, false>(ctx, stream, grid, f, d_positions, d_normals, d_lights_map, in, W, H, step, d_visibility);
        if (s != RTS_OK) return s;
    }
    return RTS_OK;
}

// The chain of a call: rtsh_wide_filter_guided_temporal_soft_light_list_device's, with the sibling kernel as its first pass.
extern "C" int rtsh_wide_filter_guided_temporal_mean_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                                            const rtsh_wide_guide_temporal_params* params,
                                                                            const float* d_positions, const float* d_normals,
                                                                            const uint8_t* d_lights_map, const uint8_t* d_counts,
                                                                            const uint16_t* d_mean, const uint32_t* d_square,
                                                                            const uint8_t* d_lengths, uint32_t W, uint32_t H,
                                                                            float* d_visibility, uint16_t* d_scratch, void* stream) {
    using namespace rts_harness;
    if (!ctx || !d_positions || !d_normals || !d_counts || !d_mean || !d_square || !d_lengths || !d_visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int made = makeWideGuidedTemporalList(list, params, W, H, &f);
    if (made != RTS_OK) return made;
    const uint32_t k4 = params->guide_k4, minHistory = params->min_history;
    const dim3 grid((W + 15) / 16, (H + 15) / 16);
    if (grid.y > 65535u) return RTS_ERR_INVALID_ARG;
    const size_t set = (size_t)f.count * (size_t)W * (size_t)H;
    if (f.passes >= 2u && !d_scratch) return RTS_ERR_INVALID_ARG;
    if (d_scratch)
        for (size_t i = 0; i < 3; ++i)
            if ((const void*)d_visibility == (const void*)(d_scratch + i * set)) return RTS_ERR_INVALID_ARG;
    const GuideMomentsCounts h{ GuideMoments{ d_mean, d_square, d_lengths, W, (uint64_t)W * H }, d_counts };
    if (f.passes <= 1u)
        return launchWideGuidedTemporalMeanFirst<true>(ctx, stream, grid, f, k4, minHistory, h, d_positions, d_normals, d_lights_map, W, H,
                                                       (int)f.passes, d_visibility, nullptr);
    uint16_t* guide = d_scratch + 2 * set;
    for (uint32_t k = 0; k < f.passes; ++k) {
        const int step = 1 << k;
        const void* in = k == 0 ? nullptr : (const void*)(d_scratch + ((k - 1u) & 1u) * set);
        uint16_t* mid = d_scratch + (k & 1u) * set;
        int s;
        if (k == 0)
            s = launchWideGuidedTemporalMeanFirst<false>(ctx, stream, grid, f, k4, minHistory, h, d_positions, d_normals, d_lights_map, W, H, step,
                                                         mid, guide);
        else if (k + 1u < f.passes)
            s = launchWideGuidedPass<false, false>(ctx, stream, grid, f, k4, d_positions, d_normals, d_lights_map, in, W, H, step, mid, guide);
        else s = launchWideGuidedPass<false, true>(ctx, stream, grid, f, k4, d_positions, d_normals, d_lights_map, in, W, H, step, d_visibility, guide);
        if (s != RTS_OK) return s;
    }
    return RTS_OK;
}
