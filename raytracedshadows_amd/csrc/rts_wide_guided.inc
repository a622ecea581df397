// The variance-guided wide filter of a soft light list's planes on the GPU (include/rts_scene.h:
// rtsh_wide_filter_guided_soft_light_list_device).  The per-pixel rule is the host twin's own source (rts_closest_hit.h:
// wideGuideThresholdPixel, wideGuidedPassPixel).  Included by rts_primary.hip after rts_wide_filter.inc, whose tile, global texels,
// window geometry, staging layout, launch of a pass (launchWideKernel) and chain of a call (launchWideChain) this file uses as they
// are; wideFilterKernel is not touched: a SIBLING kernel, so that every instantiation of the unguided kernel keeps its instruction text.
//
// ONE KERNEL PER PASS as there: one pixel per lane, 16 x 16 pixels per workgroup, templated on FIRST, LAST and the staging form (DENSE
// for steps 1, 2, 4; DIRECT for steps 8, 16 and the passes == 0 conversion).  The FIRST pass forms T(p, l) for its own pixel: its
// step-1 DENSE window reaches two pixels, so the 3 x 3 of V_0, the map bytes and the normals are already in LDS (the DIRECT form loads
// the nine values from global memory); unless it is also the LAST it writes T to the third set of planes of the scratch.  A later pass
// reads its centre's T: one uint16_t per pixel and light.  The staging loop is wideFilterKernel's, statement for statement.

namespace rts_harness {
int makeWideGuidedList(const rts_soft_light_list* list, const rtsh_wide_guide_params* p, uint32_t W, uint32_t H, WideFilterList* out);  // rts_scene.cpp

template <bool FIRST, bool LAST, bool DENSE>
__global__ __launch_bounds__(256) void wideGuidedKernel(WideFilterList f, uint32_t k4, const float* positions, const float* normals,
                                                        const uint8_t* lightsMap, const void* in, int W, int H, int step, int pitch,
                                                        void* out, uint16_t* guide) {
    const uint32_t count = f.count;
    const uint64_t n = (uint64_t)W * (uint64_t)H;
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    const uint64_t p = (uint64_t)y * (uint64_t)W + (uint64_t)x;
    uint32_t v[8], T[8];
    // T of a later pass: the first pass's plane (0 where the light is not on at p: the pass gives 0 there whatever T is)
    auto loadGuide = [&]() {
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l) {
            if (l >= count) break;
            T[l] = guide[(uint64_t)l * n + p];
        }
    };
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
                        svalues[l * cells + s] = (uint16_t)wideLoadValue<FIRST, false>(f, in, n, g, l);
                    }
                }
            }
            sa[s] = make_float2(nx, ny); sb[s] = make_float2(nz, px); sc[s] = make_float2(py, pz);
            smap[s] = (uint8_t)bits;
        }
        __syncthreads();
        if (x >= W || y >= H) return;
        const WideTile t{ sa, sb, sc, svalues, smap, x0, y0, pitch, cells };
        if (FIRST) {
            wideGuideThresholdPixel(f, k4, t, x, y, W, H, T);          // (a DENSE pass has step >= 1)
            if (!LAST) storeGuide();
        } else loadGuide();
        wideGuidedPassPixel(f, t, x, y, W, H, step, T, v);
    } else {
        if (x >= W || y >= H) return;
        const WideGlobal<FIRST, false> t{ f, positions, normals, lightsMap, in, (uint64_t)W, n };
        if (FIRST) {
            if (step > 0) wideGuideThresholdPixel(f, k4, t, x, y, W, H, T);   // (step 0: the conversion walks no tap and needs no T)
            if (!LAST) storeGuide();
        } else loadGuide();
        wideGuidedPassPixel(f, t, x, y, W, H, step, T, v);
    }
#pragma unroll
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= count) break;
        if (LAST) ((float*)out)[(uint64_t)l * n + p] = wideFilterOutput(v[l], f.samples[l], f.scale[l]);
        else ((uint16_t*)out)[(uint64_t)l * n + p] = (uint16_t)v[l];
    }
}

// The later passes of the guided chains (this file's, rts_moments.inc's and rts_wide_mean.inc's): wideGuidedKernel<false, LAST>.
static auto wideGuidedLaterPass(rts_ctx* ctx, void* stream, const WideFilterList& f, uint32_t k4, const float* d_positions,
                                const float* d_normals, const uint8_t* d_lights_map, uint32_t W, uint32_t H) {
    return [=, &f](dim3 grid, auto last, const void* in, int step, void* out, uint16_t* guide) {
        constexpr bool LAST = decltype(last)::value;
        return launchWideKernel(ctx, stream, grid, f, W, H, step, wideGuidedKernel<false, LAST, true>, wideGuidedKernel<false, LAST, false>,
                                std::make_tuple(k4, d_positions, d_normals, d_lights_map, in), out, guide);
    };
}
} // namespace rts_harness

// The chain of a call is launchWideChain (rts_wide_filter.inc), with three sets.
extern "C" int rtsh_wide_filter_guided_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                              const rtsh_wide_guide_params* params, const float* d_positions,
                                                              const float* d_normals, const uint8_t* d_lights_map, const uint8_t* d_counts,
                                                              uint32_t W, uint32_t H, float* d_visibility, uint16_t* d_scratch, void* stream) {
    using namespace rts_harness;
    if (!ctx || !d_positions || !d_normals || !d_counts || !d_visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int made = makeWideGuidedList(list, params, W, H, &f);
    if (made != RTS_OK) return made;
    const uint32_t k4 = params->guide_k4;
    auto firstPass = [&](dim3 grid, auto last, int step, void* out, uint16_t* guide) {
        constexpr bool LAST = decltype(last)::value;
        return launchWideKernel(ctx, stream, grid, f, W, H, step, wideGuidedKernel<true, LAST, true>, wideGuidedKernel<true, LAST, false>,
                                std::make_tuple(k4, d_positions, d_normals, d_lights_map, (const void*)d_counts), out, guide);
    };
    return launchWideChain(ctx, f, W, H, d_visibility, d_scratch, 3, firstPass,
                           wideGuidedLaterPass(ctx, stream, f, k4, d_positions, d_normals, d_lights_map, W, H));
}
