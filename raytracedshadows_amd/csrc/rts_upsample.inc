// Half-resolution light lists on the GPU (include/rts_scene.h: rtsh_subsample_gbuffer_device, rtsh_upsample_retrace_map_device,
// rtsh_upsample_light_list_device, rtsh_upsample_soft_light_list_device).  The per-pixel rules are the host twins' own source
// (rts_closest_hit.h: upsampleTaps, upsampleRetracePixel, upsamplePixel), compiled with the same flags.  Included at the end of
// rts_primary.hip (the scene passes' translation unit), whose own kernels keep their instruction text.

namespace rts_harness {
int makeUpsampleList(uint32_t count, const rtsh_upsample_params* p, uint32_t W, uint32_t H, UpsampleList* out);          // rts_scene.cpp

// SUBSAMPLE KERNEL.  One low-resolution pixel per lane: two texels and a map byte gathered from the sampled full-resolution pixel.
__global__ __launch_bounds__(256) void subsampleKernel(UpsampleList f, const float* positions, const float* normals, const uint8_t* lightsMap,
                                                       uint64_t W, uint64_t nlo, float* loPositions, float* loNormals, uint8_t* loMap) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= nlo) return;
    const uint64_t Y = q / (uint64_t)f.w, X = q - Y * (uint64_t)f.w;
    const uint64_t p = (2u * Y + f.phaseY) * W + (2u * X + f.phaseX);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        loPositions[q * 4 + i] = positions[p * 4 + i];
        loNormals[q * 4 + i] = normals[p * 4 + i];
    }
    if (lightsMap) loMap[q] = lightsMap[p];
}

// RETRACE MAP AND UPSAMPLE KERNELS.  One full-resolution pixel per lane, one workgroup per block of 32 x 8 pixels (four waves of
// 32 x 2): a wave's row is 512 contiguous bytes of each G-buffer target and 32 of each byte plane.  The block's taps lie in a window
// of (32 / 2 + 2) x (8 / 2 + 2) = 18 x 6 low-resolution texels beginning at (16 * blockIdx.x - phase_x, 4 * blockIdx.y - phase_y) --
// X0 of the block's first column is (32 * bx - phase_x) >> 1 and X0 + 1 of its last is 16 * bx + 16 --, each read by up to nine pixels.
// STAGED: the window is loaded ONCE into LDS by the block's first 108 lanes, structure of arrays (six float arrays, the map bytes, one
// byte array per plane; 3.4 KiB, so LDS never limits occupancy): the 32 lanes of an LDS lane group share one row of pixels, so one
// tap of theirs reads 16 or 17 consecutive dwords of one window row, each by two lanes -- no bank is asked twice.  A texel outside w x h
// is never asked for (the rule tests the coordinates first) and is not staged.  Not STAGED: the rule reads the low-resolution buffers
// themselves (tools/list_upsample_ab.py builds a second library with -DRTS_UPSAMPLE_DIRECT; EXPERIMENTS.md has both forms' figures).
#if defined(RTS_UPSAMPLE_DIRECT)
constexpr bool kUpsampleStaged = false;
#else
constexpr bool kUpsampleStaged = true;
#endif
constexpr int kUpsampleBW = 32, kUpsampleBH = 8, kUpsampleWX = kUpsampleBW / 2 + 2, kUpsampleWY = kUpsampleBH / 2 + 2;
constexpr int kUpsampleCells = kUpsampleWX * kUpsampleWY;

struct UpsampleFull {                                        // the full-resolution frame: a lane reads its own pixel only
    const float *positions, *normals;
    const uint8_t* map;
    uint64_t W;
    __device__ uint64_t at(int x, int y) const { return (uint64_t)y * W + (uint64_t)x; }
    __device__ V3 normal(int x, int y) const { const float* v = normals + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ V3 position(int x, int y) const { const float* v = positions + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ uint32_t bits(int x, int y) const { return map ? map[at(x, y)] : 0xFFu; }
};

template <bool HARD>
struct UpsampleLowDirect {                                   // the low-resolution frame from its buffers
    const float *positions, *normals;
    const uint8_t *map, *planes;
    uint64_t w, n;
    __device__ uint64_t at(int X, int Y) const { return (uint64_t)Y * w + (uint64_t)X; }
    __device__ V3 normal(int X, int Y) const { const float* v = normals + at(X, Y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ V3 position(int X, int Y) const { const float* v = positions + at(X, Y) * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ uint32_t bits(int X, int Y) const { return map ? map[at(X, Y)] : 0xFFu; }
    __device__ uint32_t byte(int X, int Y, uint32_t l) const { return HARD ? (planes[at(X, Y)] >> l) & 1u : planes[(uint64_t)l * n + at(X, Y)]; }
};

struct UpsampleWindow {                                      // the block's window in LDS
    float n[3][kUpsampleCells], p[3][kUpsampleCells];
    uint8_t map[kUpsampleCells], bytes[8][kUpsampleCells];
};

template <bool HARD>
struct UpsampleLowTile {
    const UpsampleWindow* s;
    int X0, Y0;
    __device__ int at(int X, int Y) const { return (Y - Y0) * kUpsampleWX + (X - X0); }
    __device__ V3 normal(int X, int Y) const { const int i = at(X, Y); return V3{ s->n[0][i], s->n[1][i], s->n[2][i] }; }
    __device__ V3 position(int X, int Y) const { const int i = at(X, Y); return V3{ s->p[0][i], s->p[1][i], s->p[2][i] }; }
    __device__ uint32_t bits(int X, int Y) const { return s->map[at(X, Y)]; }
    __device__ uint32_t byte(int X, int Y, uint32_t l) const { return HARD ? (s->bytes[0][at(X, Y)] >> l) & 1u : s->bytes[l][at(X, Y)]; }
};

// Stages the block's window (the caller's __syncthreads follows).  PLANES: 0 = none (the retrace map), 1 = the mask of a hard list,
// 2 = the count planes of a soft one (every plane below count: the tap that is the pixel itself does not look at its map bit).
template <int PLANES>
__device__ void upsampleStage(const UpsampleList& f, UpsampleWindow* s, int X0, int Y0, const float* loPositions, const float* loNormals,
                              const uint8_t* loMap, const uint8_t* loPlanes) {
    const int tid = (int)(threadIdx.y * kUpsampleBW + threadIdx.x);
    if (tid >= kUpsampleCells) return;
    const int ty = tid / kUpsampleWX, tx = tid - ty * kUpsampleWX, X = X0 + tx, Y = Y0 + ty;
    if (X < 0 || X >= f.w || Y < 0 || Y >= f.h) return;
    const uint64_t q = (uint64_t)Y * (uint64_t)f.w + (uint64_t)X, nlo = (uint64_t)f.w * (uint64_t)f.h;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        s->n[i][tid] = loNormals[q * 4 + i];
        s->p[i][tid] = loPositions[q * 4 + i];
    }
    const uint32_t bits = (loMap ? loMap[q] : 0xFFu) & ((1u << f.count) - 1u);
    s->map[tid] = (uint8_t)bits;
    if (PLANES == 1) s->bytes[0][tid] = loPlanes[q];
    if (PLANES == 2) {
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l) {
            if (l >= f.count) break;
            s->bytes[l][tid] = loPlanes[(uint64_t)l * nlo + q];
        }
    }
}

template <bool STAGED>
__global__ __launch_bounds__(256) void upsampleRetraceKernel(UpsampleList f, const float* positions, const float* normals,
                                                             const uint8_t* lightsMap, const float* loPositions, const float* loNormals,
                                                             const uint8_t* loMap, int W, int H, uint8_t* retrace) {
    __shared__ UpsampleWindow s;
    const int X0 = (int)blockIdx.x * (kUpsampleBW / 2) - (int)f.phaseX, Y0 = (int)blockIdx.y * (kUpsampleBH / 2) - (int)f.phaseY;
    if (STAGED) {
        upsampleStage<0>(f, &s, X0, Y0, loPositions, loNormals, loMap, nullptr);
        __syncthreads();
    }
    const int x = (int)blockIdx.x * kUpsampleBW + (int)threadIdx.x, y = (int)blockIdx.y * kUpsampleBH + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const UpsampleFull full{ positions, normals, lightsMap, (uint64_t)W };
    uint8_t bits;
    if (STAGED) bits = upsampleRetracePixel(f, full, UpsampleLowTile<false>{ &s, X0, Y0 }, x, y);
    else bits = upsampleRetracePixel(f, full, UpsampleLowDirect<false>{ loPositions, loNormals, loMap, nullptr, (uint64_t)f.w, 0 }, x, y);
    retrace[full.at(x, y)] = bits;
}

template <bool HARD, bool STAGED>
__global__ __launch_bounds__(256) void upsampleListKernel(UpsampleList f, const float* positions, const float* normals,
                                                          const uint8_t* lightsMap, const float* loPositions, const float* loNormals,
                                                          const uint8_t* loMap, const uint8_t* loPlanes, const uint8_t* keep, int W, int H,
                                                          uint8_t* planes) {
    __shared__ UpsampleWindow s;
    const int X0 = (int)blockIdx.x * (kUpsampleBW / 2) - (int)f.phaseX, Y0 = (int)blockIdx.y * (kUpsampleBH / 2) - (int)f.phaseY;
    if (STAGED) {
        upsampleStage<HARD ? 1 : 2>(f, &s, X0, Y0, loPositions, loNormals, loMap, loPlanes);
        __syncthreads();
    }
    const int x = (int)blockIdx.x * kUpsampleBW + (int)threadIdx.x, y = (int)blockIdx.y * kUpsampleBH + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const UpsampleFull full{ positions, normals, lightsMap, (uint64_t)W };
    const uint64_t p = full.at(x, y), n = (uint64_t)W * (uint64_t)H;
    const uint32_t all = (1u << f.count) - 1u, kept = keep ? keep[p] & all : 0u, todo = all & ~kept;
    if (todo == 0u) return;
    uint32_t b[8];
    if (STAGED) upsamplePixel(f, full, UpsampleLowTile<HARD>{ &s, X0, Y0 }, x, y, todo, b);
    else upsamplePixel(f, full, UpsampleLowDirect<HARD>{ loPositions, loNormals, loMap, loPlanes, (uint64_t)f.w, (uint64_t)f.w * (uint64_t)f.h }, x, y, todo, b);
    if (HARD) {
        uint32_t bits = kept ? planes[p] & kept : 0u;
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l)
            if (l < f.count && ((todo >> l) & 1u)) bits |= (b[l] & 1u) << l;
        planes[p] = (uint8_t)bits;
    } else {
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l) {
            if (l >= f.count) break;
            if ((todo >> l) & 1u) planes[(uint64_t)l * n + p] = (uint8_t)b[l];
        }
    }
}

// The launch of the two full-resolution passes: the grid of 32 x 8 blocks, refused where its y extent would not fit.
static bool upsampleGrid(uint32_t W, uint32_t H, dim3* grid) {
    *grid = dim3((W + kUpsampleBW - 1) / kUpsampleBW, (H + kUpsampleBH - 1) / kUpsampleBH);
    return grid->y <= 65535u;
}

template <bool HARD>
static int launchUpsampleList(rts_ctx* ctx, uint32_t count, const rtsh_upsample_params* params, const float* d_positions, const float* d_normals,
                              const uint8_t* d_lights_map, const float* d_lo_positions, const float* d_lo_normals, const uint8_t* d_lo_lights_map,
                              const uint8_t* d_lo_planes, const uint8_t* d_keep, uint32_t W, uint32_t H, uint8_t* d_planes, void* stream) {
    if (!ctx || !d_positions || !d_normals || !d_lo_positions || !d_lo_normals || !d_lo_planes || !d_planes || d_planes == d_lo_planes)
        return RTS_ERR_INVALID_ARG;
    UpsampleList f;
    const int s = makeUpsampleList(count, params, W, H, &f);
    if (s != RTS_OK) return s;
    dim3 grid;
    if (!upsampleGrid(W, H, &grid)) return RTS_ERR_INVALID_ARG;
    return launchPass(ctx, stream, grid, dim3(kUpsampleBW, kUpsampleBH), 0, upsampleListKernel<HARD, kUpsampleStaged>, f, d_positions, d_normals,
                      d_lights_map, d_lo_positions, d_lo_normals, d_lo_lights_map, d_lo_planes, d_keep, (int)W, (int)H, d_planes);
}
} // namespace rts_harness

extern "C" int rtsh_subsample_gbuffer_device(rts_ctx* ctx, const rtsh_upsample_params* params, const float* d_positions,
                                             const float* d_normals, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                             float* d_lo_positions, float* d_lo_normals, uint8_t* d_lo_lights_map, void* stream) {
    if (!ctx || !d_positions || !d_normals || !d_lo_positions || !d_lo_normals || (d_lights_map && !d_lo_lights_map)) return RTS_ERR_INVALID_ARG;
    rts_harness::UpsampleList f;
    const int s = rts_harness::makeUpsampleList(1, params, W, H, &f);
    if (s != RTS_OK) return s;
    const uint64_t nlo = (uint64_t)f.w * (uint64_t)f.h;
    return rts_harness::launchPerPixel(ctx, stream, nlo, rts_harness::subsampleKernel, f, d_positions, d_normals, d_lights_map, (uint64_t)W, nlo,
                                       d_lo_positions, d_lo_normals, d_lo_lights_map);
}

extern "C" int rtsh_upsample_retrace_map_device(rts_ctx* ctx, uint32_t count, const rtsh_upsample_params* params, const float* d_positions,
                                                const float* d_normals, const uint8_t* d_lights_map, const float* d_lo_positions,
                                                const float* d_lo_normals, const uint8_t* d_lo_lights_map, uint32_t W, uint32_t H,
                                                uint8_t* d_retrace, void* stream) {
    if (!ctx || !d_positions || !d_normals || !d_lo_positions || !d_lo_normals || !d_retrace) return RTS_ERR_INVALID_ARG;
    rts_harness::UpsampleList f;
    const int s = rts_harness::makeUpsampleList(count, params, W, H, &f);
    if (s != RTS_OK) return s;
    dim3 grid;
    if (!rts_harness::upsampleGrid(W, H, &grid)) return RTS_ERR_INVALID_ARG;
    return rts_harness::launchPass(ctx, stream, grid, dim3(rts_harness::kUpsampleBW, rts_harness::kUpsampleBH), 0,
                                   rts_harness::upsampleRetraceKernel<rts_harness::kUpsampleStaged>, f, d_positions, d_normals, d_lights_map,
                                   d_lo_positions, d_lo_normals, d_lo_lights_map, (int)W, (int)H, d_retrace);
}

extern "C" int rtsh_upsample_light_list_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_upsample_params* params,
                                               const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                               const float* d_lo_positions, const float* d_lo_normals, const uint8_t* d_lo_lights_map,
                                               const uint8_t* d_lo_mask, const uint8_t* d_keep, uint32_t W, uint32_t H, uint8_t* d_mask,
                                               void* stream) {
    rts_harness::FilterList unused;
    const rtsh_filter_params any{};
    if (rts_harness::makeFilterHardList(list, &any, &unused) != RTS_OK) return RTS_ERR_INVALID_ARG;      // what the filter refuses of a list
    return rts_harness::launchUpsampleList<true>(ctx, list->count, params, d_positions, d_normals, d_lights_map, d_lo_positions, d_lo_normals,
                                                 d_lo_lights_map, d_lo_mask, d_keep, W, H, d_mask, stream);
}

extern "C" int rtsh_upsample_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_upsample_params* params,
                                                    const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                    const float* d_lo_positions, const float* d_lo_normals, const uint8_t* d_lo_lights_map,
                                                    const uint8_t* d_lo_counts, const uint8_t* d_keep, uint32_t W, uint32_t H,
                                                    uint8_t* d_counts, void* stream) {
    rts_harness::FilterList unused;
    const rtsh_filter_params any{};
    if (rts_harness::makeFilterSoftList(list, &any, false, &unused) != RTS_OK) return RTS_ERR_INVALID_ARG;
    return rts_harness::launchUpsampleList<false>(ctx, list->count, params, d_positions, d_normals, d_lights_map, d_lo_positions, d_lo_normals,
                                                  d_lo_lights_map, d_lo_counts, d_keep, W, H, d_counts, stream);
}
