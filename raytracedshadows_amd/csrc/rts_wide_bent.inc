// The wide (a-trous) filter of the bent plane on the GPU (include/rts_scene.h: rtsh_wide_filter_bent_device; DESIGN.md 4.38).  The
// per-pixel rule of a pass is the host twin's own source (rts_closest_hit.h: bentFilterPassPixel), compiled with the same flags: no
// contraction, correctly rounded division.  Included at the end of rts_primary.hip, after the other wide filters, whose kernels keep
// their instruction text.
//
// ONE KERNEL PER PASS, one pixel per lane, one workgroup per block of 16 x 16 pixels, templated as rts_wide_filter.inc's on FIRST (reads
// the 16-byte float texel of the trace and quantises it; later passes read the previous pass's 8-byte texels: int16 x, y, z and uint16
// V), LAST (divides and stores the 16-byte float texel, and `ao` when given; earlier passes store 8-byte texels) and the STAGING FORM:
//   DENSE   steps 1, 2, 4: the (16 + 4 * step)^2 window staged ONCE in LDS.  The geometry is rts_wide_filter.inc's structure of arrays
//           -- three float2 arrays (nx, ny), (nz, px), (py, pz) -- at its pitch, 48 texels at every dense step; beside it ONE array of
//           8-byte texels, read with a single ds_read_b64 per tap and unpacked with integer operations, and the byte array of `active`.
//           24 + 8 + 1 = 33 bytes per texel; at step 4 the window is 32 rows of pitch 48: 1536 texels, 50688 bytes (49.5 KiB), inside
//           the 64 KiB a workgroup gets without opting in (step 1: 20 rows, 31680 bytes; step 2: 24 rows, 38016 bytes).
//           THE PITCH: a ds_read_b64 is banked per 32-lane half over 64 dword banks.  A half-wave reads two rows of 16 consecutive
//           8-byte texels: 32 consecutive dwords each, 2 * 48 = 96 dwords apart, which is 32 modulo 64 -- the two rows fall on
//           disjoint halves of the banks for every tap offset.  The value array has the float2 arrays' element size, so their pitch
//           is right for it as it is (a 2-byte array at this pitch shares a ninth dword; an 8-byte one does not).
//           A texel outside the frame, a background texel or one whose byte is clear is staged as background with a clear byte: its
//           position and value are never read.  All lanes reach the one barrier; the out-of-frame return sits behind it.
//   DIRECT  steps 8 and 16 and the passes == 0 conversion: every tap from global memory, one 8-byte load per tap; no LDS, no barrier.
namespace rts_harness {
int makeBentFilterList(const rtsh_wide_filter_params* p, uint32_t nsamples, uint32_t W, uint32_t H, BentFilterList* out);   // rts_scene.cpp

struct WideBentTile {
    const float2 *a, *b, *c;             // (nx, ny), (nz, px), (py, pz)
    const uint64_t* values;              // [cells]
    const uint8_t* map;                  // [cells]
    int x0, y0, pitch;                   // frame coordinates of texel (0, 0); row pitch
    __device__ int at(int x, int y) const { return (y - y0) * pitch + (x - x0); }
    __device__ V3 normal(int x, int y) const { const int i = at(x, y); const float2 u = a[i]; return V3{ u.x, u.y, b[i].x }; }
    __device__ V3 position(int x, int y) const { const int i = at(x, y); const float2 u = c[i]; return V3{ b[i].y, u.x, u.y }; }
    __device__ bool active(int x, int y) const { return map[at(x, y)] != 0; }
    __device__ BentTexel texel(int x, int y) const { return bentFilterUnpack(values[at(x, y)]); }
};

// X_k, V_k of pixel g as a pass reads them from global memory.
template <bool FIRST>
__device__ inline BentTexel wideBentLoad(const BentFilterList& f, const void* in, uint64_t g) {
    if (!FIRST) return bentFilterUnpack(((const uint64_t*)in)[g]);
    const float4 b = ((const float4*)in)[g];
    return bentFilterInput(b.x, b.y, b.z, b.w, f);
}

template <bool FIRST>
struct WideBentGlobal {
    const BentFilterList& f;
    const float *positions, *normals;
    const uint8_t* map;
    const void* in;
    uint64_t W;
    __device__ uint64_t at(int x, int y) const { return (uint64_t)y * W + (uint64_t)x; }
    __device__ V3 normal(int x, int y) const { const float* v = normals + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ V3 position(int x, int y) const { const float* v = positions + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ bool active(int x, int y) const { return !map || map[at(x, y)] != 0; }
    __device__ BentTexel texel(int x, int y) const { return wideBentLoad<FIRST>(f, in, at(x, y)); }
};

template <bool FIRST, bool LAST, bool DENSE>
__global__ __launch_bounds__(256) void wideBentKernel(BentFilterList f, const float* positions, const float* normals, const uint8_t* activeMap,
                                                      const void* in, int W, int H, int step, int pitch, void* out, float* ao) {
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
                    svalues[s] = bentFilterPack(wideBentLoad<FIRST>(f, in, g));
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
        const WideBentGlobal<FIRST> t{ f, positions, normals, activeMap, in, (uint64_t)W };
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

// LDS bytes of a DENSE pass at rts_wide_filter.inc's pitch: 24 bytes of geometry, the 8-byte texel and the byte per staged texel.
static WideGeometry wideBentGeometry(int step) {
    const int TW = 16 + 4 * step, pitch = wideGeometry(1, step).pitch;
    return WideGeometry{ pitch, (size_t)pitch * (size_t)TW * (24 + 8 + 1) };
}

template <bool FIRST, bool LAST>
static int launchWideBentPass(rts_ctx* ctx, void* stream, dim3 grid, const BentFilterList& f, const float* d_positions, const float* d_normals,
                              const uint8_t* d_active, const void* in, uint32_t W, uint32_t H, int step, void* out, float* d_ao) {
    const bool dense = step >= 1 && step <= kWideDenseMaxStep;
    const WideGeometry g = dense ? wideBentGeometry(step) : WideGeometry{ 0, 0 };
    return launchPass(ctx, stream, grid, dim3(16, 16), g.bytes, dense ? wideBentKernel<FIRST, LAST, true> : wideBentKernel<FIRST, LAST, false>, f,
                      d_positions, d_normals, d_active, in, (int)W, (int)H, step, g.pitch, out, d_ao);
}
} // namespace rts_harness

extern "C" int rtsh_wide_filter_bent_device(rts_ctx* ctx, const rtsh_wide_filter_params* params, uint32_t nsamples, const float* d_positions,
                                            const float* d_normals, const uint8_t* d_active, const float* d_bent, uint32_t W, uint32_t H,
                                            float* d_out, float* d_ao, void* d_scratch, void* stream) {
    using namespace rts_harness;
    if (!ctx || !d_positions || !d_normals || !d_bent || !d_out) return RTS_ERR_INVALID_ARG;
    BentFilterList f;
    const int s = makeBentFilterList(params, nsamples, W, H, &f);
    if (s != RTS_OK) return s;
    const dim3 grid((W + 15) / 16, (H + 15) / 16);
    if (grid.y > 65535u) return RTS_ERR_INVALID_ARG;
    if (((uintptr_t)d_bent | (uintptr_t)d_out) & 15u || ((uintptr_t)d_scratch & 7u)) return RTS_ERR_INVALID_ARG;
    if (f.passes >= 2u && !d_scratch) return RTS_ERR_INVALID_ARG;
    const size_t n = (size_t)W * (size_t)H;
    uint64_t* scratch = (uint64_t*)d_scratch;
    for (const void* o : { (const void*)d_out, (const void*)d_ao }) {
        if (!o) continue;
        if (o == (const void*)d_bent) return RTS_ERR_INVALID_ARG;
        if (scratch && (o == (const void*)scratch || o == (const void*)(scratch + n))) return RTS_ERR_INVALID_ARG;
    }
    if (f.passes <= 1u)
        return launchWideBentPass<true, true>(ctx, stream, grid, f, d_positions, d_normals, d_active, d_bent, W, H, (int)f.passes, d_out, d_ao);
    for (uint32_t k = 0; k < f.passes; ++k) {
        const int step = 1 << k;
        const void* in = scratch + ((k - 1u) & 1u) * n;
        void* mid = scratch + (k & 1u) * n;
        int st;
        if (k == 0) st = launchWideBentPass<true, false>(ctx, stream, grid, f, d_positions, d_normals, d_active, d_bent, W, H, step, mid, nullptr);
        else if (k + 1u < f.passes)
            st = launchWideBentPass<false, false>(ctx, stream, grid, f, d_positions, d_normals, d_active, in, W, H, step, mid, nullptr);
        else st = launchWideBentPass<false, true>(ctx, stream, grid, f, d_positions, d_normals, d_active, in, W, H, step, d_out, d_ao);
        if (st != RTS_OK) return st;
    }
    return RTS_OK;
}
