// The filter of a light list's planes and the visibility combine on the GPU (include/rts_scene.h: rtsh_filter_*_light_list_device,
// rtsh_combine_visibility_list_device).  The per-pixel rules are the host twins' own source (rts_closest_hit.h: filterListPixel,
// combineVisibilityPixel), compiled with the same flags: no contraction, correctly rounded division.  Included at the end of
// rts_primary.hip (the scene passes' translation unit), whose own kernels keep their instruction text.

namespace rts_harness {
int makeFilterHardList(const rts_light_list* list, const rtsh_filter_params* p, FilterList* out);                       // rts_scene.cpp
int makeFilterSoftList(const rts_soft_light_list* list, const rtsh_filter_params* p, bool withDistances, FilterList* out);

// FILTER KERNEL.  One pixel per lane, one workgroup per block of 16 x BH pixels (BH = blockDim.y, 16: 256 lanes, four waves of 16 x 4
// pixels).  16 x 16 rather than 8 x 8 per wave: the staged window is (16 + 2R)^2 texels for 256 pixels -- 4 texels staged per pixel at
// R = 8 where four 8 x 8 tiles would stage (8 + 2R)^2 each, 9 per pixel -- and a block is uniform per light about as often.
// The window is staged ONCE in LDS, structure of arrays, texel (tx, ty) at ty * pitch + tx in every array:
//   three float2 arrays (nx, ny), (nz, px), (py, pz)      -- ds_read_b64: a half-wave is two rows of 16 consecutive float2; with
//                                                            pitch % 32 == 16 the two rows fall on disjoint halves of the 64 banks
//   (DIST) one dword array per light                         (the 24-byte record as an array of structures would put lanes 6 dwords
//   one byte array for the map, one per plane                apart: 3- and 6-way conflicts on every read)
// Texels outside the frame are staged as background with no map bit, so they stage nothing else and are never accepted.
// The launcher picks pitch and BH so that the tile fits the 64 KiB a workgroup may ask for without opting in (filterGeometry).
// SHORTCUT (anchor 2 of the header): while staging, every lane notes per light the bytes of the texels that could be accepted (in the
// frame, not background, map bit set); waves agree by ballot, the block through 32 dwords of LDS.  A light with ONE byte over the
// whole window takes the centre quotient and is left out of `walk`; when no light is left, the block walks no taps at all.
#if defined(RTS_FILTER_NO_SHORTCUT)
constexpr bool kFilterShortcut = false;                    // (tools/list_filter_ab.py builds a second library with this)
#else
constexpr bool kFilterShortcut = true;
#endif

struct FilterTile {
    const float2 *a, *b, *c;             // (nx, ny), (nz, px), (py, pz)
    const uint32_t* dist;                // [count][cells]
    const uint8_t *map, *bytes;          // [cells], [planes][cells]
    int x0, y0, pitch, cells;            // frame coordinates of texel (0, 0); row pitch; pitch * rows
    bool hard;
    __device__ int at(int x, int y) const { return (y - y0) * pitch + (x - x0); }
    __device__ V3 normal(int x, int y) const { const int i = at(x, y); const float2 u = a[i]; return V3{ u.x, u.y, b[i].x }; }
    __device__ V3 position(int x, int y) const { const int i = at(x, y); const float2 u = c[i]; return V3{ b[i].y, u.x, u.y }; }
    __device__ uint32_t bits(int x, int y) const { return map[at(x, y)]; }
    __device__ uint32_t byte(int x, int y, uint32_t l) const { return hard ? (bytes[at(x, y)] >> l) & 1u : bytes[l * cells + at(x, y)]; }
    __device__ uint32_t distance(int x, int y, uint32_t l) const { return dist[l * cells + at(x, y)]; }
};

template <bool HARD, bool DIST>
__global__ __launch_bounds__(256) void filterListKernel(FilterList f, const float* positions, const float* normals, const uint8_t* lightsMap,
                                                        const uint8_t* planes, const uint32_t* distances, int W, int H, int pitch,
                                                        float* visibility) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int R = (int)f.radius, TW = 16 + 2 * R, TH = (int)blockDim.y + 2 * R, cells = pitch * TH;
    const uint32_t count = f.count, nplanes = HARD ? 1u : count;
    uint32_t* info = (uint32_t*)lds;                                   // [4 waves][8 lights]
    float2* sa = (float2*)(lds + 128);
    float2* sb = sa + cells;
    float2* sc = sb + cells;
    uint32_t* sdist = (uint32_t*)(sc + cells);
    uint8_t* smap = (uint8_t*)(sdist + (DIST ? count * cells : 0));
    uint8_t* sbytes = smap + cells;
    const int x0 = (int)blockIdx.x * 16 - R, y0 = (int)blockIdx.y * (int)blockDim.y - R;
    const int tid = (int)(threadIdx.y * 16 + threadIdx.x), nthreads = 16 * (int)blockDim.y;
    const uint64_t n = (uint64_t)W * (uint64_t)H;

    uint32_t seen = 0, mixed = 0, first[8];                            // per light: a byte seen, two different bytes seen, the first one
#pragma unroll
    for (uint32_t l = 0; l < 8; ++l) first[l] = 0;
    for (int i = tid; i < TW * TH; i += nthreads) {
        const int ty = i / TW, tx = i - ty * TW, gx = x0 + tx, gy = y0 + ty, s = ty * pitch + tx;
        float nx = 0.f, ny = 0.f, nz = 0.f, px = 0.f, py = 0.f, pz = 0.f;
        uint32_t bits = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const uint64_t g = (uint64_t)gy * (uint64_t)W + (uint64_t)gx;
            nx = normals[g * 4]; ny = normals[g * 4 + 1]; nz = normals[g * 4 + 2];
            if (!(nx == 0.0f && ny == 0.0f && nz == 0.0f)) {           // (a background texel: only its normal is read)
                px = positions[g * 4]; py = positions[g * 4 + 1]; pz = positions[g * 4 + 2];
                bits = (lightsMap ? lightsMap[g] : 0xFFu) & ((1u << count) - 1u);
                const uint32_t hardByte = HARD ? planes[g] : 0u;
                if (HARD) sbytes[s] = (uint8_t)hardByte;
#pragma unroll
                for (uint32_t l = 0; l < 8; ++l) {
                    if (l >= count) break;
                    if (!((bits >> l) & 1u)) continue;                 // (a plane byte whose map bit is clear is not read)
                    uint32_t v;
                    if (HARD) v = (hardByte >> l) & 1u;
                    else { v = planes[(uint64_t)l * n + g]; sbytes[l * cells + s] = (uint8_t)v; }
                    if (DIST) sdist[l * cells + s] = distances[(uint64_t)l * n + g];
                    if (!((seen >> l) & 1u)) { first[l] = v; seen |= 1u << l; }
                    else if (v != first[l]) mixed |= 1u << l;
                }
            }
        }
        sa[s] = make_float2(nx, ny); sb[s] = make_float2(nz, px); sc[s] = make_float2(py, pz);
        smap[s] = (uint8_t)bits;
    }
    if (kFilterShortcut) {
        const int wave = tid >> 6;
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l) {
            if (l >= count) break;
            const bool has = (seen >> l) & 1u;
            const unsigned long long any = __ballot(has);
            uint32_t word = 0;
            if (any) {
                const uint32_t ref = (uint32_t)__shfl((int)first[l], __ffsll(any) - 1);
                const unsigned long long differs = __ballot(has && (((mixed >> l) & 1u) || first[l] != ref));
                word = 0x200u | (differs ? 0x100u : 0u) | ref;        // seen, mixed, the byte
            }
            if ((tid & 63) == 0) info[wave * 8 + l] = word;
        }
    }
    __syncthreads();
    uint32_t walk = (1u << count) - 1u;
    if (kFilterShortcut) {
        const int waves = (nthreads + 63) >> 6;
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l) {
            if (l >= count) break;
            bool one = true, have = false;
            uint32_t ref = 0;
            for (int w = 0; w < waves; ++w) {
                const uint32_t word = info[w * 8 + l];
                if (!(word & 0x200u)) continue;
                if ((word & 0x100u) || (have && (word & 0xFFu) != ref)) one = false;
                ref = word & 0xFFu; have = true;
            }
            if (one) walk &= ~(1u << l);
        }
    }
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * (int)blockDim.y + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const FilterTile t{ sa, sb, sc, sdist, smap, sbytes, x0, y0, pitch, cells, HARD };
    float v[8];
    filterListPixel<DIST>(f, t, x, y, W, H, walk, v);
    const uint64_t p = (uint64_t)y * (uint64_t)W + (uint64_t)x;
#pragma unroll
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= count) break;
        visibility[(uint64_t)l * n + p] = v[l];
    }
    (void)nplanes;
}

// Pitch, block height and LDS bytes of a launch.  The pitch is the window's width rounded up to 16 modulo 32 (conflict-free ds_read_b64
// of two rows per half-wave) where that fits 64 KiB; else the bare width (two-way conflicts on some banks); and where a block of 16 rows
// still does not fit -- eight lights with distances at R = 8, 65 bytes per texel -- the block is 16 x 8 pixels, two waves.
struct FilterGeometry { int pitch, rows; size_t bytes; };
static FilterGeometry filterGeometry(const FilterList& f, bool hard, bool dist) {
    const int TW = 16 + 2 * (int)f.radius;
    const size_t perTexel = 24 + 1 + (hard ? 1 : f.count) + (dist ? 4 * f.count : 0);
    const int padded = ((TW + 15) / 32) * 32 + 16;
    const size_t limit = 64 * 1024;
    FilterGeometry g{ padded, 16, 0 };
    auto bytes = [&](int pitch, int rows) { return 128 + (size_t)pitch * (size_t)(rows + 2 * (int)f.radius) * perTexel; };
    if (bytes(g.pitch, g.rows) > limit) g.pitch = TW;
    if (bytes(g.pitch, g.rows) > limit) g.rows = 8;
    g.bytes = bytes(g.pitch, g.rows);
    return g;
}

template <bool HARD, bool DIST>
static int launchFilter(rts_ctx* ctx, const FilterList& f, const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                        const uint8_t* d_planes, const float* d_distances, uint32_t W, uint32_t H, float* d_visibility, void* stream) {
    if (W > 0x7FFFFFF0u || H > 0x7FFFFFF0u) return RTS_ERR_INVALID_ARG;
    const FilterGeometry g = filterGeometry(f, HARD, DIST);
    const dim3 grid((W + 15) / 16, (H + (uint32_t)g.rows - 1) / (uint32_t)g.rows);
    if (grid.y > 65535u) return RTS_ERR_INVALID_ARG;
    return launchPass(ctx, stream, grid, dim3(16, (unsigned)g.rows), g.bytes, filterListKernel<HARD, DIST>, f, d_positions, d_normals,
                      d_lights_map, d_planes, (const uint32_t*)d_distances, (int)W, (int)H, g.pitch, d_visibility);
}

// The visibility combine: combineListKernel's frame (one pixel per lane) over float planes.
__global__ __launch_bounds__(256) void combineVisibilityKernel(CombineList f, const float* positions, const float* normals,
                                                               const uint8_t* lightsMap, const float* visibility, uint64_t n, uint8_t* rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float zero[4] = { 0.f, 0.f, 0.f, 0.f };
    const float* n4 = normals + i * 4;
    const float nx = n4[0], ny = n4[1], nz = n4[2];
    const float nrm[4] = { nx, ny, nz, 0.f };
    const bool background = nx == 0.0f && ny == 0.0f && nz == 0.0f;        // (its map byte is not read)
    const uint32_t bits = (lightsMap && !background) ? lightsMap[i] : 0xFFu;
    uint8_t q[3];
    combineVisibilityPixel(f, positions ? positions + i * 4 : zero, nrm, bits, [&](uint32_t l) { return visibility[(uint64_t)l * n + i]; }, q);
    rgb[i * 3] = q[0]; rgb[i * 3 + 1] = q[1]; rgb[i * 3 + 2] = q[2];
}

// The same with the ambient term times the pixel's ambient occlusion (rtsh_combine_visibility_list_ao_device): a kernel of its own, so
// that combineVisibilityKernel keeps its text.
__global__ __launch_bounds__(256) void combineVisibilityAoKernel(CombineList f, const float* positions, const float* normals,
                                                                 const uint8_t* lightsMap, const float* visibility, const float* ao, uint64_t n,
                                                                 uint8_t* rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float zero[4] = { 0.f, 0.f, 0.f, 0.f };
    const float* n4 = normals + i * 4;
    const float nx = n4[0], ny = n4[1], nz = n4[2];
    const float nrm[4] = { nx, ny, nz, 0.f };
    const bool background = nx == 0.0f && ny == 0.0f && nz == 0.0f;        // (neither its map byte nor its ao is read)
    const uint32_t bits = (lightsMap && !background) ? lightsMap[i] : 0xFFu;
    uint8_t q[3];
    combineVisibilityPixel(f, positions ? positions + i * 4 : zero, nrm, bits, [&](uint32_t l) { return visibility[(uint64_t)l * n + i]; },
                           [&](float ambient) { return ambient * ao[i]; }, q);
    rgb[i * 3] = q[0]; rgb[i * 3 + 1] = q[1]; rgb[i * 3 + 2] = q[2];
}

// The same again with the hemispheric sky tint on the ambient term, aimed by the pixel's bent vector (rtsh_combine_visibility_list_ao_
// bent_device): a third kernel, so that the two above keep their text.  The sky's nine floats travel by value.
struct SkyAmbient9 { float v[9]; };
__global__ __launch_bounds__(256) void combineVisibilityAoBentKernel(CombineList f, SkyAmbient9 sky, const float* positions,
                                                                     const float* normals, const uint8_t* lightsMap, const float* visibility,
                                                                     const float* ao, const float* bent, uint64_t n, uint8_t* rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float zero[4] = { 0.f, 0.f, 0.f, 0.f };
    const float* n4 = normals + i * 4;
    const float nx = n4[0], ny = n4[1], nz = n4[2];
    const float nrm[4] = { nx, ny, nz, 0.f };
    const bool background = nx == 0.0f && ny == 0.0f && nz == 0.0f;        // (neither its map byte, its ao nor its bent texel is read)
    const uint32_t bits = (lightsMap && !background) ? lightsMap[i] : 0xFFu;
    uint8_t q[3];
    combineVisibilityPixelRgb(f, positions ? positions + i * 4 : zero, nrm, bits, [&](uint32_t l) { return visibility[(uint64_t)l * n + i]; },
                              [&](float ambient, float* out3) {
                                  const float* b4 = bent + i * 4;
                                  const float b[4] = { b4[0], b4[1], b4[2], 0.f };
                                  skyAmbient3(ambient, ao[i], sky.v, b, out3);
                              }, q);
    rgb[i * 3] = q[0]; rgb[i * 3 + 1] = q[1]; rgb[i * 3 + 2] = q[2];
}
} // namespace rts_harness

extern "C" int rtsh_combine_visibility_list_ao_bent_device(rts_ctx* ctx, const rts_constants* k, const rts_light_list* list, const float* colors,
                                                           const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                           const float* d_visibility, const float* d_ao, const float* d_bent,
                                                           const rtsh_sky_ambient* sky, uint32_t W, uint32_t H, uint8_t* d_rgb, void* stream) {
    if (!ctx || !k || !d_normals || !d_visibility || !d_ao || !d_bent || !sky || !d_rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    rts_harness::CombineList f;
    const int s = rts_harness::makeCombineList(k, list, colors, d_positions != nullptr, &f);
    if (s != RTS_OK) return s;
    rts_harness::SkyAmbient9 sky9;
    memcpy(sky9.v, sky, sizeof(sky9.v));                                   // { up, sky, ground }
    const uint64_t n = (uint64_t)W * H;
    return rts_harness::launchPerPixel(ctx, stream, n, rts_harness::combineVisibilityAoBentKernel, f, sky9, d_positions, d_normals, d_lights_map,
                                       d_visibility, d_ao, d_bent, n, d_rgb);
}

extern "C" int rtsh_combine_visibility_list_ao_device(rts_ctx* ctx, const rts_constants* k, const rts_light_list* list, const float* colors,
                                                      const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                      const float* d_visibility, const float* d_ao, uint32_t W, uint32_t H, uint8_t* d_rgb,
                                                      void* stream) {
    if (!ctx || !k || !d_normals || !d_visibility || !d_ao || !d_rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    rts_harness::CombineList f;
    const int s = rts_harness::makeCombineList(k, list, colors, d_positions != nullptr, &f);
    if (s != RTS_OK) return s;
    const uint64_t n = (uint64_t)W * H;
    return rts_harness::launchPerPixel(ctx, stream, n, rts_harness::combineVisibilityAoKernel, f, d_positions, d_normals, d_lights_map,
                                       d_visibility, d_ao, n, d_rgb);
}

extern "C" int rtsh_filter_light_list_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_filter_params* params,
                                             const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                             const uint8_t* d_mask, uint32_t W, uint32_t H, float* d_visibility, void* stream) {
    if (!ctx || !d_positions || !d_normals || !d_mask || !d_visibility || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    rts_harness::FilterList f;
    const int s = rts_harness::makeFilterHardList(list, params, &f);
    if (s != RTS_OK) return s;
    return rts_harness::launchFilter<true, false>(ctx, f, d_positions, d_normals, d_lights_map, d_mask, nullptr, W, H, d_visibility, stream);
}

extern "C" int rtsh_filter_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_filter_params* params,
                                                  const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                  const uint8_t* d_counts, const float* d_distances, uint32_t W, uint32_t H,
                                                  float* d_visibility, void* stream) {
    if (!ctx || !d_positions || !d_normals || !d_counts || !d_visibility || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    rts_harness::FilterList f;
    const int s = rts_harness::makeFilterSoftList(list, params, d_distances != nullptr, &f);
    if (s != RTS_OK) return s;
    if (d_distances)
        return rts_harness::launchFilter<false, true>(ctx, f, d_positions, d_normals, d_lights_map, d_counts, d_distances, W, H, d_visibility,
                                                      stream);
    return rts_harness::launchFilter<false, false>(ctx, f, d_positions, d_normals, d_lights_map, d_counts, nullptr, W, H, d_visibility, stream);
}

extern "C" int rtsh_combine_visibility_list_device(rts_ctx* ctx, const rts_constants* k, const rts_light_list* list, const float* colors,
                                                   const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                   const float* d_visibility, uint32_t W, uint32_t H, uint8_t* d_rgb, void* stream) {
    if (!ctx || !k || !d_normals || !d_visibility || !d_rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    rts_harness::CombineList f;
    const int s = rts_harness::makeCombineList(k, list, colors, d_positions != nullptr, &f);
    if (s != RTS_OK) return s;
    const uint64_t n = (uint64_t)W * H;
    return rts_harness::launchPerPixel(ctx, stream, n, rts_harness::combineVisibilityKernel, f, d_positions, d_normals, d_lights_map,
                                       d_visibility, n, d_rgb);
}
