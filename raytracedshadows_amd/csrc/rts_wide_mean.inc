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
} // namespace rts_harness

// The chain of both calls is launchWideChain (rts_wide_filter.inc), with two and three sets and the sibling kernel as its first pass.
extern "C" int rtsh_wide_filter_mean_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_wide_filter_params* params,
                                                            const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                            const uint16_t* d_mean, uint32_t W, uint32_t H, float* d_visibility,
                                                            uint16_t* d_scratch, void* stream) {
    using namespace rts_harness;
    if (!ctx || !d_positions || !d_normals || !d_mean || !d_visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int made = makeWideFilterSoftList(list, params, W, H, &f);
    if (made != RTS_OK) return made;
    auto firstPass = [&](dim3 grid, auto last, int step, void* out, uint16_t*) {
        constexpr bool LAST = decltype(last)::value;
        return launchWideKernel(ctx, stream, grid, f, W, H, step, wideMeanKernel<LAST, true>, wideMeanKernel<LAST, false>,
                                std::make_tuple(d_positions, d_normals, d_lights_map, d_mean), out);
    };
    return launchWideChain(ctx, f, W, H, d_visibility, d_scratch, 2, firstPass,
                           wideLaterPass<false>(ctx, stream, f, d_positions, d_normals, d_lights_map, W, H));
}

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
    const GuideMomentsCounts h{ GuideMoments{ d_mean, d_square, d_lengths, W, (uint64_t)W * H }, d_counts };
    auto firstPass = [&](dim3 grid, auto last, int step, void* out, uint16_t* guide) {
        constexpr bool LAST = decltype(last)::value;
        return launchWideKernel(ctx, stream, grid, f, W, H, step, wideGuidedTemporalMeanKernel<LAST, true>,
                                wideGuidedTemporalMeanKernel<LAST, false>,
                                std::make_tuple(k4, minHistory, h, d_positions, d_normals, d_lights_map), out, guide);
    };
    return launchWideChain(ctx, f, W, H, d_visibility, d_scratch, 3, firstPass,
                           wideGuidedLaterPass(ctx, stream, f, k4, d_positions, d_normals, d_lights_map, W, H));
}
