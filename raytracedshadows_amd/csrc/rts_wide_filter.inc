// The wide (a-trous) filter of a light list's planes on the GPU (include/rts_scene.h: rtsh_wide_filter_*_light_list_device).  The
// per-pixel rule of a pass is the host twin's own source (rts_closest_hit.h: wideFilterPassPixel), compiled with the same flags: no
// contraction, correctly rounded division.  Included at the end of rts_primary.hip, whose other kernels keep their instruction text.
//
// ONE KERNEL PER PASS, one pixel per lane, one workgroup per block of 16 x 16 pixels (256 lanes, four waves of 16 x 4 pixels), templated
// on FIRST (reads the count bytes / the mask and forms V_0 itself; later passes read the previous pass's uint16_t planes), LAST (forms
// the float visibility; earlier passes write uint16_t planes), HARD, and the STAGING FORM of the taps:
//   DENSE   the (16 + 4 * step)^2 window of the block staged ONCE in LDS, structure of arrays as in rts_filter.inc -- three float2
//           arrays (nx, ny), (nz, px), (py, pz) read with ds_read_b64, pitch % 32 == 16 texels so that the two rows of a half-wave
//           fall on disjoint halves of the 64 banks; one uint16_t array per light (V_k, for the first pass formed while staging) and
//           one byte array for the map.  A half-wave's uint16_t read is two rows of 16 consecutive values, 8 dwords each (9 where the
//           tap's column is odd), pitch / 2 = 24 dwords apart modulo 32: the rows share a bank only through that ninth dword.
//           1.6, 2.3 and 4 texels staged per pixel at step 1, 2 and 4; 25 + 2 * count bytes per texel: 61.5 KiB for eight lights at
//           step 4, inside the 64 KiB a workgroup gets without opting in.  Texels outside the frame are staged as background with no
//           map bit.  All lanes reach the one barrier; the out-of-frame return sits behind it.
//   DIRECT  every tap loaded from global memory: a tap row of a block is 16 consecutive pixels (256 B of normals), L2 carries the
//           reuse between the 25 taps.  No LDS, no barrier.  The form for step 8 and 16, whose dense windows (48^2 and 80^2 texels)
//           do not fit; and for the passes == 0 conversion (step 0: no tap is walked).
// kWideDenseMaxStep: the largest step that takes the DENSE form (tools/list_wide_filter_ab.py builds a second library with
// -DRTS_WIDE_FILTER_DENSE_MAX_STEP=0, every pass DIRECT, to measure the choice per step).
#include <tuple>
#include <type_traits>

namespace rts_harness {
int makeWideFilterHardList(const rts_light_list* list, const rtsh_wide_filter_params* p, uint32_t W, uint32_t H, WideFilterList* out); // rts_scene.cpp
int makeWideFilterSoftList(const rts_soft_light_list* list, const rtsh_wide_filter_params* p, uint32_t W, uint32_t H, WideFilterList* out);

#if defined(RTS_WIDE_FILTER_DENSE_MAX_STEP)
constexpr int kWideDenseMaxStep = RTS_WIDE_FILTER_DENSE_MAX_STEP;
#else
constexpr int kWideDenseMaxStep = 4;
#endif
static_assert(kWideDenseMaxStep <= 4, "the dense window of step 8 does not fit 64 KiB for more than one light");

struct WideTile {
    const float2 *a, *b, *c;             // (nx, ny), (nz, px), (py, pz)
    const uint16_t* values;              // [count][cells]
    const uint8_t* map;                  // [cells]
    int x0, y0, pitch, cells;            // frame coordinates of texel (0, 0); row pitch; pitch * rows
    __device__ int at(int x, int y) const { return (y - y0) * pitch + (x - x0); }
    __device__ V3 normal(int x, int y) const { const int i = at(x, y); const float2 u = a[i]; return V3{ u.x, u.y, b[i].x }; }
    __device__ V3 position(int x, int y) const { const int i = at(x, y); const float2 u = c[i]; return V3{ b[i].y, u.x, u.y }; }
    __device__ uint32_t bits(int x, int y) const { return map[at(x, y)]; }
    __device__ uint32_t value(int x, int y, uint32_t l) const { return values[l * cells + at(x, y)]; }
};

// V_k of pixel g for light l as a pass reads it from global memory.
template <bool FIRST, bool HARD>
__device__ inline uint32_t wideLoadValue(const WideFilterList& f, const void* in, uint64_t n, uint64_t g, uint32_t l) {
    if (!FIRST) return ((const uint16_t*)in)[(uint64_t)l * n + g];
    const uint8_t* bytes = (const uint8_t*)in;
    return wideFilterInput(HARD ? (bytes[g] >> l) & 1u : bytes[(uint64_t)l * n + g], f.samples[l], f.scale[l]);
}

template <bool FIRST, bool HARD>
struct WideGlobal {
    const WideFilterList& f;
    const float *positions, *normals;
    const uint8_t* map;
    const void* in;
    uint64_t W, n;
    __device__ uint64_t at(int x, int y) const { return (uint64_t)y * W + (uint64_t)x; }
    __device__ V3 normal(int x, int y) const { const float* v = normals + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ V3 position(int x, int y) const { const float* v = positions + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ uint32_t bits(int x, int y) const { return map ? map[at(x, y)] : 0xFFu; }
    __device__ uint32_t value(int x, int y, uint32_t l) const { return wideLoadValue<FIRST, HARD>(f, in, n, at(x, y), l); }
};

template <bool FIRST, bool LAST, bool HARD, bool DENSE>
__global__ __launch_bounds__(256) void wideFilterKernel(WideFilterList f, const float* positions, const float* normals, const uint8_t* lightsMap,
                                                        const void* in, int W, int H, int step, int pitch, void* out) {
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
                        svalues[l * cells + s] = (uint16_t)wideLoadValue<FIRST, HARD>(f, in, n, g, l);
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
        const WideGlobal<FIRST, HARD> t{ f, positions, normals, lightsMap, in, (uint64_t)W, n };
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

// Pitch and LDS bytes of a DENSE pass: the window's width rounded up to 16 modulo 32.
struct WideGeometry { int pitch; size_t bytes; };
static WideGeometry wideGeometry(uint32_t count, int step) {
    const int TW = 16 + 4 * step;
    const int pitch = ((TW + 15) / 32) * 32 + 16;
    return WideGeometry{ pitch, (size_t)pitch * (size_t)TW * (24 + 2 * (size_t)count + 1) };
}

// THE ONE LAUNCH OF A PASS, for the five kernels of the wide filters (wideFilterKernel here; wideGuidedKernel, wideGuidedTemporalKernel,
// wideMeanKernel, wideGuidedTemporalMeanKernel in the files included after this one): the DENSE instantiation with its window's pitch
// and LDS bytes for steps 1 .. kWideDenseMaxStep, else the DIRECT one with pitch 0.  Every one of the kernels takes
// (f, head..., int W, int H, int step, int pitch, tail...): `head` is what stands between the list and the frame size, in the kernel's order.
template <class... Params, class... Head, class... Tail>
static int launchWideKernel(rts_ctx* ctx, void* stream, dim3 grid, const WideFilterList& f, uint32_t W, uint32_t H, int step,
                            void (*denseKernel)(Params...), void (*directKernel)(Params...), const std::tuple<Head...>& head, Tail... tail) {
    const bool dense = step >= 1 && step <= kWideDenseMaxStep;
    const WideGeometry g = dense ? wideGeometry(f.count, step) : WideGeometry{ 0, 0 };
    auto launch = [&](Head... h) {
        return launchPass(ctx, stream, grid, dim3(16, 16), g.bytes, dense ? denseKernel : directKernel, f, h..., (int)W, (int)H, step, g.pitch,
                          tail...);
    };
    return std::apply(launch, head);
}

// THE ONE CHAIN OF A CALL, for the five device entries: max(1, passes) launches on `stream`, pass k from the entry's own input (k == 0) or
// from set (k - 1) & 1 of the scratch into set k & 1, the last one into visibility.  `sets`: 2, or 3 for the guided forms, whose planes
// of T lie behind the two ping-pong sets (`guide`; NULL for the one launch of passes <= 1, which is FIRST and LAST and stores no T).
// firstPass(grid, last, step, out, guide) and laterPass(grid, last, in, step, out, guide) launch the entry's instantiations; `last` is a
// std::bool_constant, so that LAST stays a template argument.
template <class First, class Later>
static int launchWideChain(rts_ctx* ctx, const WideFilterList& f, uint32_t W, uint32_t H, float* d_visibility, uint16_t* d_scratch, size_t sets,
                           First firstPass, Later laterPass) {
    const dim3 grid((W + 15) / 16, (H + 15) / 16);
    if (grid.y > 65535u) return RTS_ERR_INVALID_ARG;
    const size_t set = (size_t)f.count * (size_t)W * (size_t)H;
    if (f.passes >= 2u && !d_scratch) return RTS_ERR_INVALID_ARG;
    if (d_scratch)
        for (size_t i = 0; i < sets; ++i)
            if ((const void*)d_visibility == (const void*)(d_scratch + i * set)) return RTS_ERR_INVALID_ARG;
    if (f.passes <= 1u) return firstPass(grid, std::true_type{}, (int)f.passes, (void*)d_visibility, (uint16_t*)nullptr);
    uint16_t* guide = sets > 2 ? d_scratch + 2 * set : nullptr;
    for (uint32_t k = 0; k < f.passes; ++k) {
        const int step = 1 << k;
        const void* in = k == 0 ? nullptr : (const void*)(d_scratch + ((k - 1u) & 1u) * set);
        void* mid = d_scratch + (k & 1u) * set;
        int s;
        if (k == 0) s = firstPass(grid, std::false_type{}, step, mid, guide);
        else if (k + 1u < f.passes) s = laterPass(grid, std::false_type{}, in, step, mid, guide);
        else s = laterPass(grid, std::true_type{}, in, step, (void*)d_visibility, guide);
        if (s != RTS_OK) return s;
    }
    return RTS_OK;
}

// The later passes of the unguided chains (this file's and rts_wide_mean.inc's): wideFilterKernel<false, LAST, HARD>.
template <bool HARD>
static auto wideLaterPass(rts_ctx* ctx, void* stream, const WideFilterList& f, const float* d_positions, const float* d_normals,
                          const uint8_t* d_lights_map, uint32_t W, uint32_t H) {
    return [=, &f](dim3 grid, auto last, const void* in, int step, void* out, uint16_t*) {
        constexpr bool LAST = decltype(last)::value;
        return launchWideKernel(ctx, stream, grid, f, W, H, step, wideFilterKernel<false, LAST, HARD, true>,
                                wideFilterKernel<false, LAST, HARD, false>, std::make_tuple(d_positions, d_normals, d_lights_map, in), out);
    };
}

template <bool HARD>
static int launchWideFilter(rts_ctx* ctx, const WideFilterList& f, const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                            const uint8_t* d_planes, uint32_t W, uint32_t H, float* d_visibility, uint16_t* d_scratch, void* stream) {
    auto firstPass = [&](dim3 grid, auto last, int step, void* out, uint16_t*) {
        constexpr bool LAST = decltype(last)::value;
        return launchWideKernel(ctx, stream, grid, f, W, H, step, wideFilterKernel<true, LAST, HARD, true>,
                                wideFilterKernel<true, LAST, HARD, false>,
                                std::make_tuple(d_positions, d_normals, d_lights_map, (const void*)d_planes), out);
    };
    return launchWideChain(ctx, f, W, H, d_visibility, d_scratch, 2, firstPass,
                           wideLaterPass<HARD>(ctx, stream, f, d_positions, d_normals, d_lights_map, W, H));
}
} // namespace rts_harness

extern "C" int rtsh_wide_filter_light_list_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_wide_filter_params* params,
                                                  const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                  const uint8_t* d_mask, uint32_t W, uint32_t H, float* d_visibility, uint16_t* d_scratch,
                                                  void* stream) {
    if (!ctx || !d_positions || !d_normals || !d_mask || !d_visibility) return RTS_ERR_INVALID_ARG;
    rts_harness::WideFilterList f;
    const int s = rts_harness::makeWideFilterHardList(list, params, W, H, &f);
    if (s != RTS_OK) return s;
    return rts_harness::launchWideFilter<true>(ctx, f, d_positions, d_normals, d_lights_map, d_mask, W, H, d_visibility, d_scratch, stream);
}

extern "C" int rtsh_wide_filter_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_wide_filter_params* params,
                                                       const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                       const uint8_t* d_counts, uint32_t W, uint32_t H, float* d_visibility,
                                                       uint16_t* d_scratch, void* stream) {
    if (!ctx || !d_positions || !d_normals || !d_counts || !d_visibility) return RTS_ERR_INVALID_ARG;
    rts_harness::WideFilterList f;
    const int s = rts_harness::makeWideFilterSoftList(list, params, W, H, &f);
    if (s != RTS_OK) return s;
    return rts_harness::launchWideFilter<false>(ctx, f, d_positions, d_normals, d_lights_map, d_counts, W, H, d_visibility, d_scratch, stream);
}
