// The temporal accumulation of the bent texel, and the wide bent filter fed from it, on the GPU (include/rts_scene.h:
// rtsh_accumulate_bent_device, rtsh_accumulate_bent_motion_device, rtsh_wide_filter_bent_mean_device; DESIGN.md 4.39).  The per-pixel
// rules are the host twin's own source (rts_closest_hit.h: accumulateBentPixel, bentFilterMeanInput, bentFilterPassPixel), compiled with
// the same flags: no contraction, correctly rounded division.  Included at the end of rts_primary.hip, after rts_wide_bent.inc; every
// kernel in front of it keeps its instruction text: the kernels here are SIBLINGS, nothing above is touched.
namespace rts_harness {
int makeBentTemporalList(const rtsh_temporal_params* p, uint32_t nsamples, const void* positions, const void* normals, const void* bent,
                         const void* prevPositions, const void* prevNormals, const void* prevTexels, const void* prevLengths, uint32_t W,
                         uint32_t H, const void* texelsOut, const void* lengthsOut, BentTemporalList* out);              // rts_scene.cpp

// ACCUMULATE KERNEL.  accumulateMomentsKernel's shape, for its reasons (rts_temporal.inc): one pixel per lane, 256 lanes per block of
// 16 x 16 pixels, four waves of 16 x 4, no LDS -- where the gathered patch lies depends on the data.  The geometry of the four taps is
// decided once per pixel; a tap of weight 0 or a rejected tap is never loaded.  What is streamed once goes non-temporal: this frame's
// G-buffer texels and `active` byte, the float texel of the trace (ONE 16-byte load) and the two outputs (ONE 8-byte and one 1-byte
// store).  The previous frame's G-buffer texels and its history, which neighbours share, are plain loads: the length byte first, then
// ONE 8-byte load of the texel where the length is not 0.
typedef float BentFloat4 __attribute__((ext_vector_type(4)));     // (the builtin takes a native vector, not HIP's float4 struct)
struct BentTemporalDeviceFrames {
    const float *positions, *normals, *prevPositions, *prevNormals;
    const BentFloat4* bent;
    const uint8_t *map, *prevLengths;
    const uint64_t* prevTexels;
    uint64_t* texelsOut;
    uint8_t* lengthsOut;
    BentFilterList f;
    uint64_t W;
    __device__ uint64_t at(int x, int y) const { return (uint64_t)y * W + (uint64_t)x; }
    __device__ V3 normal(int x, int y) const { return TemporalDeviceFrames::streamed(normals, at(x, y)); }
    __device__ V3 position(int x, int y) const { return TemporalDeviceFrames::streamed(positions, at(x, y)); }
    __device__ bool active(int x, int y) const { return !map || __builtin_nontemporal_load(map + at(x, y)) != 0; }
    __device__ BentTexel current(int x, int y) const {
        const BentFloat4 b = __builtin_nontemporal_load(bent + at(x, y));
        return bentFilterInput(b.x, b.y, b.z, b.w, f);
    }
    __device__ V3 prevNormal(int x, int y) const { return TemporalDeviceFrames::shared(prevNormals, at(x, y)); }
    __device__ V3 prevPosition(int x, int y) const { return TemporalDeviceFrames::shared(prevPositions, at(x, y)); }
    __device__ uint32_t prevLength(int x, int y) const { return prevLengths[at(x, y)]; }
    __device__ BentTexel prevTexel(int x, int y) const { return bentFilterUnpack(prevTexels[at(x, y)]); }
    __device__ void store(int x, int y, uint64_t texel, uint32_t length) const {
        __builtin_nontemporal_store(texel, texelsOut + at(x, y));
        __builtin_nontemporal_store((uint8_t)length, lengthsOut + at(x, y));
    }
};

__global__ __launch_bounds__(256) void accumulateBentKernel(TemporalList f, BentTemporalDeviceFrames t, int W, int H) {
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    accumulateBentPixel(BentTemporalList{ f, t.f }, t, x, y, W, H);
}

// MOTION FORM (rtsh_accumulate_bent_motion_device): a sibling in the same shape; accumulateBentPixel<true> takes Q and M_p from this
// frame's two motion texels, each read once by its own pixel: non-temporal.
struct MotionBentTemporalDeviceFrames : BentTemporalDeviceFrames {
    const float *prevPoints, *prevPointNormals;
    __device__ V3 prevPoint(int x, int y) const { return TemporalDeviceFrames::streamed(prevPoints, at(x, y)); }
    __device__ V3 prevPointNormal(int x, int y) const { return TemporalDeviceFrames::streamed(prevPointNormals, at(x, y)); }
};

__global__ __launch_bounds__(256) void accumulateBentMotionKernel(TemporalList f, BentTemporalDeviceFrames t, const float* prevPoints,
                                                                  const float* prevPointNormals, int W, int H) {
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const MotionBentTemporalDeviceFrames m{ t, prevPoints, prevPointNormals };
    accumulateBentPixel<true>(BentTemporalList{ f, t.f }, m, x, y, W, H);
}

static int accumulateBentDevice(rts_ctx* ctx, bool motion, const rtsh_temporal_params* params, uint32_t nsamples, const float* d_positions,
                                const float* d_normals, const uint8_t* d_active, const float* d_bent, const float* d_prev_positions,
                                const float* d_prev_normals, const void* d_prev_texels, const uint8_t* d_prev_lengths,
                                const float* d_prev_points, const float* d_prev_point_normals, uint32_t W, uint32_t H, void* d_texels_out,
                                uint8_t* d_lengths_out, void* stream) {
    if (!ctx) return RTS_ERR_INVALID_ARG;
    BentTemporalList f;
    int s = makeBentTemporalList(params, nsamples, d_positions, d_normals, d_bent, d_prev_positions, d_prev_normals, d_prev_texels,
                                 d_prev_lengths, W, H, d_texels_out, d_lengths_out, &f);
    if (s == RTS_OK && motion) s = checkMotionPlanes(f.t.history, d_prev_points, d_prev_point_normals);
    if (s != RTS_OK) return s;
    const dim3 grid((W + 15) / 16, (H + 15) / 16);
    if (grid.y > 65535u) return RTS_ERR_INVALID_ARG;
    if (((uintptr_t)d_bent & 15u) || (((uintptr_t)d_texels_out | (uintptr_t)d_prev_texels) & 7u)) return RTS_ERR_INVALID_ARG;
    const BentTemporalDeviceFrames t{ d_positions, d_normals, d_prev_positions, d_prev_normals, (const BentFloat4*)d_bent, d_active,
                                      d_prev_lengths, (const uint64_t*)d_prev_texels, (uint64_t*)d_texels_out, d_lengths_out, f.q, W };
    if (motion)
        return launchPass(ctx, stream, grid, dim3(16, 16), 0, accumulateBentMotionKernel, f.t, t, d_prev_points, d_prev_point_normals, (int)W,
                          (int)H);
    return launchPass(ctx, stream, grid, dim3(16, 16), 0, accumulateBentKernel, f.t, t, (int)W, (int)H);
}

// THE FIRST PASS OF THE MEAN-FED FILTER: wideBentKernel<true, LAST, DENSE> with bentFilterMeanInput of the 8-byte texel in the place of
// bentFilterInput of the float texel -- a sibling, so that every instantiation of wideBentKernel keeps its text; later passes ARE
// wideBentKernel<false, ...>.  The staging loop and the LDS layout are wideBentKernel's, statement for statement.
struct WideBentMeanGlobal {
    const BentFilterList& f;
    const float *positions, *normals;
    const uint8_t* map;
    const uint64_t* in;
    uint64_t W;
    __device__ uint64_t at(int x, int y) const { return (uint64_t)y * W + (uint64_t)x; }
    __device__ V3 normal(int x, int y) const { const float* v = normals + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ V3 position(int x, int y) const { const float* v = positions + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ bool active(int x, int y) const { return !map || map[at(x, y)] != 0; }
    __device__ BentTexel texel(int x, int y) const { return bentFilterMeanInput(in[at(x, y)], f); }
};

template <bool LAST, bool DENSE>
__global__ __launch_bounds__(256) void wideBentMeanKernel(BentFilterList f, const float* positions, const float* normals,
                                                          const uint8_t* activeMap, const uint64_t* in, int W, int H, int step, int pitch,
                                                          void* out, float* ao) {
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    BentTexel v;
    if constexpr (DENSE) {
        extern __shared__ __align__(16) unsigned char lds[];
        const int reach = 2 * step, TW = 16 + 2 * reach, cells = pitch * TW;
        float2* sa = (float2*)lds;
        float2* sb = sa + cells;
        float2* sc = sb + cells;
        uint64_t* svalues = (uint64_t*)(sc + cells);
        uint8_t* smap = (uint8_t*)(svalues + cells);
        const int x0 = (int)blockIdx.x * 16 - reach, y0 = (int)blockIdx.y * 16 - reach;
        const int tid = (int)(threadIdx.y * 16 + threadIdx.x);
        for (int i = tid; i < TW * TW; i += 256) {
            const int ty = i / TW, tx = i - ty * TW, gx = x0 + tx, gy = y0 + ty, s = ty * pitch + tx;
            float nx = 0.f, ny = 0.f, nz = 0.f, px = 0.f, py = 0.f, pz = 0.f;
            uint32_t on = 0;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const uint64_t g = (uint64_t)gy * (uint64_t)W + (uint64_t)gx;
                const float mx = normals[g * 4], my = normals[g * 4 + 1], mz = normals[g * 4 + 2];
                if (!(mx == 0.0f && my == 0.0f && mz == 0.0f) && (!activeMap || activeMap[g] != 0)) {
                    nx = mx; ny = my; nz = mz;
                    px = positions[g * 4]; py = positions[g * 4 + 1]; pz = positions[g * 4 + 2];
                    on = 1u;
                    svalues[s] = bentFilterPack(bentFilterMeanInput(in[g], f));
                }
            }
            sa[s] = make_float2(nx, ny); sb[s] = make_float2(nz, px); sc[s] = make_float2(py, pz);
            smap[s] = (uint8_t)on;
        }
        __syncthreads();
        if (x >= W || y >= H) return;
        const WideBentTile t{ sa, sb, sc, svalues, smap, x0, y0, pitch };
        bentFilterPassPixel(f, t, x, y, W, H, step, &v);
    } else {
        if (x >= W || y >= H) return;
        const WideBentMeanGlobal t{ f, positions, normals, activeMap, in, (uint64_t)W };
        bentFilterPassPixel(f, t, x, y, W, H, step, &v);
    }
    const uint64_t p = (uint64_t)y * (uint64_t)W + (uint64_t)x;
    if (LAST) {
        const float w = wideFilterOutput(v.v, f.samples, f.scaleL);
        ((float4*)out)[p] = make_float4(bentFilterOutput(v.x, f.samples, f.scaleB), bentFilterOutput(v.y, f.samples, f.scaleB),
                                        bentFilterOutput(v.z, f.samples, f.scaleB), w);
        if (ao) ao[p] = w;
    } else {
        ((uint64_t*)out)[p] = bentFilterPack(v);
    }
}

template <bool LAST>
static int launchWideBentMeanPass(rts_ctx* ctx, void* stream, dim3 grid, const BentFilterList& f, const float* d_positions,
                                  const float* d_normals, const uint8_t* d_active, const uint64_t* in, uint32_t W, uint32_t H, int step,
                                  void* out, float* d_ao) {
    const bool dense = step >= 1 && step <= kWideDenseMaxStep;
    const WideGeometry g = dense ? wideBentGeometry(step) : WideGeometry{ 0, 0 };
    return launchPass(ctx, stream, grid, dim3(16, 16), g.bytes, dense ? wideBentMeanKernel<LAST, true> : wideBentMeanKernel<LAST, false>, f,
                      d_positions, d_normals, d_active, in, (int)W, (int)H, step, g.pitch, out, d_ao);
}
} // namespace rts_harness

extern "C" int rtsh_accumulate_bent_device(rts_ctx* ctx, const rtsh_temporal_params* params, uint32_t nsamples, const float* d_positions,
                                           const float* d_normals, const uint8_t* d_active, const float* d_bent,
                                           const float* d_prev_positions, const float* d_prev_normals, const void* d_prev_texels,
                                           const uint8_t* d_prev_lengths, uint32_t W, uint32_t H, void* d_texels_out,
                                           uint8_t* d_lengths_out, void* stream) {
    return rts_harness::accumulateBentDevice(ctx, false, params, nsamples, d_positions, d_normals, d_active, d_bent, d_prev_positions,
                                             d_prev_normals, d_prev_texels, d_prev_lengths, nullptr, nullptr, W, H, d_texels_out,
                                             d_lengths_out, stream);
}

extern "C" int rtsh_accumulate_bent_motion_device(rts_ctx* ctx, const rtsh_temporal_params* params, uint32_t nsamples,
                                                  const float* d_positions, const float* d_normals, const uint8_t* d_active,
                                                  const float* d_bent, const float* d_prev_positions, const float* d_prev_normals,
                                                  const void* d_prev_texels, const uint8_t* d_prev_lengths, const float* d_prev_points,
                                                  const float* d_prev_point_normals, uint32_t W, uint32_t H, void* d_texels_out,
                                                  uint8_t* d_lengths_out, void* stream) {
    return rts_harness::accumulateBentDevice(ctx, true, params, nsamples, d_positions, d_normals, d_active, d_bent, d_prev_positions,
                                             d_prev_normals, d_prev_texels, d_prev_lengths, d_prev_points, d_prev_point_normals, W, H,
                                             d_texels_out, d_lengths_out, stream);
}

extern "C" int rtsh_wide_filter_bent_mean_device(rts_ctx* ctx, const rtsh_wide_filter_params* params, uint32_t nsamples,
                                                 const float* d_positions, const float* d_normals, const uint8_t* d_active,
                                                 const void* d_texels, uint32_t W, uint32_t H, float* d_out, float* d_ao, void* d_scratch,
                                                 void* stream) {
    using namespace rts_harness;
    if (!ctx || !d_positions || !d_normals || !d_texels || !d_out) return RTS_ERR_INVALID_ARG;
    BentFilterList f;
    const int s = makeBentFilterList(params, nsamples, W, H, &f);
    if (s != RTS_OK) return s;
    const dim3 grid((W + 15) / 16, (H + 15) / 16);
    if (grid.y > 65535u) return RTS_ERR_INVALID_ARG;
    if (((uintptr_t)d_out & 15u) || (((uintptr_t)d_scratch | (uintptr_t)d_texels) & 7u)) return RTS_ERR_INVALID_ARG;
    if (f.passes >= 2u && !d_scratch) return RTS_ERR_INVALID_ARG;
    const size_t n = (size_t)W * (size_t)H;
    uint64_t* scratch = (uint64_t*)d_scratch;
    const uint64_t* texels = (const uint64_t*)d_texels;
    if (scratch && (texels == scratch || texels == scratch + n)) return RTS_ERR_INVALID_ARG;
    for (const void* o : { (const void*)d_out, (const void*)d_ao }) {
        if (!o) continue;
        if (o == d_texels) return RTS_ERR_INVALID_ARG;
        if (scratch && (o == (const void*)scratch || o == (const void*)(scratch + n))) return RTS_ERR_INVALID_ARG;
    }
    if (f.passes <= 1u)
        return launchWideBentMeanPass<true>(ctx, stream, grid, f, d_positions, d_normals, d_active, texels, W, H, (int)f.passes, d_out, d_ao);
    for (uint32_t k = 0; k < f.passes; ++k) {
        const int step = 1 << k;
        const void* in = scratch + ((k - 1u) & 1u) * n;
        void* mid = scratch + (k & 1u) * n;
        int st;
        if (k == 0) st = launchWideBentMeanPass<false>(ctx, stream, grid, f, d_positions, d_normals, d_active, texels, W, H, step, mid, nullptr);
        else if (k + 1u < f.passes)
            st = launchWideBentPass<false, false>(ctx, stream, grid, f, d_positions, d_normals, d_active, in, W, H, step, mid, nullptr);
        else st = launchWideBentPass<false, true>(ctx, stream, grid, f, d_positions, d_normals, d_active, in, W, H, step, d_out, d_ao);
        if (st != RTS_OK) return st;
    }
    return RTS_OK;
}
