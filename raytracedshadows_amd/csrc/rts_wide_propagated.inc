// The guided mean filter with a propagated variance on the GPU (include/rts_scene.h:
// rtsh_wide_filter_propagated_mean_soft_light_list_device; DESIGN.md 4.31).  The per-pixel rules are the host twin's own source
// (rts_closest_hit.h: wideVarianceInput, widePropagatedFirstThresholdPixel, widePropagatedThresholdPixel, widePropagatedPassPixel),
// compiled with the same flags.  Included at the end of rts_primary.hip after rts_wide_mean.inc; every kernel in front of it keeps its
// instruction text: the kernel here is a SIBLING, nothing above is touched.
//
// ONE KERNEL PER PASS as in rts_wide_filter.inc: one pixel per lane, 16 x 16 pixels per workgroup, templated on FIRST (reads the mean and
// the moments as wideGuidedTemporalMeanKernel does, forms Q_0 and T_0), LAST (forms the float visibility and writes no Q) and the staging
// form of the VALUES (DENSE for steps 1, 2, 4 -- the window, its pitch, its 25 + 2 * count bytes per texel and the one barrier are
// wideFilterKernel's, the staging loop is its loop statement for statement --, DIRECT for steps 8, 16 and the passes == 0 conversion).
// THE VARIANCE IS NOT STAGED: at 4 bytes per texel and light beside the values it takes the step-4 window of eight lights to 109.5 KiB,
// past the 64 KiB a workgroup gets without opting in; the 25 Q taps and the nine Q of T_k are loaded from global memory where a tap is
// accepted (a tap row of a block is 16 consecutive pixels: 64 B per light), L2 carries the reuse.  No plane of T: a later pass forms
// T_k from the nine Q_k around its pixel before it walks its taps.

namespace rts_harness {
int makeWidePropagatedList(const rts_soft_light_list* list, const rtsh_wide_guide_propagated_params* p, uint32_t W, uint32_t H,
                           WideFilterList* out);                                 // rts_scene.cpp

template <bool FIRST, bool LAST, bool DENSE>
__global__ __launch_bounds__(256) void widePropagatedKernel(WideFilterList f, WidePropagatedRule r, GuideMomentsCounts h, const float* positions,
                                                            const float* normals, const uint8_t* lightsMap, const void* in,
                                                            const uint32_t* qin, int W, int H, int step, int pitch, void* out,
                                                            uint32_t* qout) {
    const uint32_t count = f.count;
    const uint64_t n = (uint64_t)W * (uint64_t)H;
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    const uint64_t p = (uint64_t)y * (uint64_t)W + (uint64_t)x;
    const uint16_t* mean = h.m.mean;
    const WideVarianceGlobal q{ f, r, h, FIRST ? nullptr : qin };
    uint32_t v[8], T[8], Q[8];
    // T_k, then the pass, over the texels `t` (the LDS tile or the buffers)
    auto pixel = [&](const auto& t) {
        if (FIRST) {
            if (step > 0) widePropagatedFirstThresholdPixel(f, r, t, h, x, y, W, H, T);   // (step 0: the conversion needs no T)
        } else {
            widePropagatedThresholdPixel(f, r.k4, t, q, x, y, W, H, T);
        }
        widePropagatedPassPixel<!LAST>(f, t, q, x, y, W, H, step, T, v, Q);
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
                        svalues[l * cells + s] = (uint16_t)(FIRST ? wideLoadMean(f, mean, n, g, l) : wideLoadValue<false, false>(f, in, n, g, l));
                    }
                }
            }
            sa[s] = make_float2(nx, ny); sb[s] = make_float2(nz, px); sc[s] = make_float2(py, pz);
            smap[s] = (uint8_t)bits;
        }
        __syncthreads();
        if (x >= W || y >= H) return;
        const WideTile t{ sa, sb, sc, svalues, smap, x0, y0, pitch, cells };
        pixel(t);
    } else {
        if (x >= W || y >= H) return;
        if constexpr (FIRST) {
            const WideMeanGlobal t{ f, positions, normals, lightsMap, mean, (uint64_t)W, n };
            pixel(t);
        } else {
            const WideGlobal<false, false> t{ f, positions, normals, lightsMap, in, (uint64_t)W, n };
            pixel(t);
        }
    }
#pragma unroll
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= count) break;
        if (LAST) ((float*)out)[(uint64_t)l * n + p] = wideFilterOutput(v[l], f.samples[l], f.scale[l]);
        else {
            ((uint16_t*)out)[(uint64_t)l * n + p] = (uint16_t)v[l];
            qout[(uint64_t)l * n + p] = Q[l];
        }
    }
}

// THE CHAIN OF A CALL: a SIBLING of launchWideChain, which keeps its text and with it the five shipped entries -- that chain knows equal
// sets of uint16_t with a plane of T behind them; this one has two sets of uint16_t values, then two sets of uint32_t variance, and hands
// each pass a variance plane to read and one to write.  The launch of a pass is launchWideKernel as it is.
template <class Pass>
static int launchWidePropagatedChain(const WideFilterList& f, uint32_t W, uint32_t H, float* d_visibility, void* d_scratch, Pass pass) {
    const dim3 grid((W + 15) / 16, (H + 15) / 16);
    if (grid.y > 65535u) return RTS_ERR_INVALID_ARG;
    const size_t set = (size_t)f.count * (size_t)W * (size_t)H;
    if (f.passes >= 2u && !d_scratch) return RTS_ERR_INVALID_ARG;
    if (((uintptr_t)d_scratch & 3u) != 0u) return RTS_ERR_INVALID_ARG;
    uint16_t* values = (uint16_t*)d_scratch;
    uint32_t* variance = (uint32_t*)(values + 2 * set);
    if (d_scratch)
        for (size_t i = 0; i < 2; ++i)
            if ((const void*)d_visibility == (const void*)(values + i * set) || (const void*)d_visibility == (const void*)(variance + i * set))
                return RTS_ERR_INVALID_ARG;
    if (f.passes <= 1u)
        return pass(grid, std::true_type{}, std::true_type{}, (const void*)nullptr, (const uint32_t*)nullptr, (int)f.passes, (void*)d_visibility,
                    (uint32_t*)nullptr);
    for (uint32_t k = 0; k < f.passes; ++k) {
        const int step = 1 << k;
        const void* in = k == 0 ? nullptr : (const void*)(values + ((k - 1u) & 1u) * set);
        const uint32_t* qin = k == 0 ? nullptr : variance + ((k - 1u) & 1u) * set;
        void* mid = values + (k & 1u) * set;
        uint32_t* qmid = variance + (k & 1u) * set;
        int s;
        if (k == 0) s = pass(grid, std::true_type{}, std::false_type{}, in, qin, step, mid, qmid);
        else if (k + 1u < f.passes) s = pass(grid, std::false_type{}, std::false_type{}, in, qin, step, mid, qmid);
        else s = pass(grid, std::false_type{}, std::true_type{}, in, qin, step, (void*)d_visibility, (uint32_t*)nullptr);
        if (s != RTS_OK) return s;
    }
    return RTS_OK;
}
} // namespace rts_harness

extern "C" int rtsh_wide_filter_propagated_mean_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                                       const rtsh_wide_guide_propagated_params* params,
                                                                       const float* d_positions, const float* d_normals,
                                                                       const uint8_t* d_lights_map, const uint8_t* d_counts,
                                                                       const uint16_t* d_mean, const uint32_t* d_square,
                                                                       const uint8_t* d_lengths, uint32_t W, uint32_t H, float* d_visibility,
                                                                       void* d_scratch, void* stream) {
    using namespace rts_harness;
    if (!ctx || !d_positions || !d_normals || !d_counts || !d_mean || !d_square || !d_lengths || !d_visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int made = makeWidePropagatedList(list, params, W, H, &f);
    if (made != RTS_OK) return made;
    const WidePropagatedRule r{ params->guide_k4, params->min_history, params->by_length };
    const GuideMomentsCounts h{ GuideMoments{ d_mean, d_square, d_lengths, W, (uint64_t)W * H }, d_counts };
    auto pass = [&](dim3 grid, auto first, auto last, const void* in, const uint32_t* qin, int step, void* out, uint32_t* qout) {
        constexpr bool FIRST = decltype(first)::value, LAST = decltype(last)::value;
        return launchWideKernel(ctx, stream, grid, f, W, H, step, widePropagatedKernel<FIRST, LAST, true>,
                                widePropagatedKernel<FIRST, LAST, false>,
                                std::make_tuple(r, h, d_positions, d_normals, d_lights_map, in, qin), out, qout);
    };
    return launchWidePropagatedChain(f, W, H, d_visibility, d_scratch, pass);
}
