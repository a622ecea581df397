// The temporal accumulation of a light list's visibility on the GPU (include/rts_scene.h: rtsh_accumulate_visibility_list_device).
// The per-pixel rule is the host twin's own source (rts_closest_hit.h: accumulatePixel), compiled with the same flags: no
// contraction, correctly rounded division.  Included at the end of rts_primary.hip (the scene passes' translation unit), whose own
// kernels keep their instruction text.

namespace rts_harness {
int makeTemporalList(const rts_light_list* list, const rtsh_temporal_params* p, const void* positions, const void* normals,
                     const void* visibility, const void* prevPositions, const void* prevNormals, const void* prevVisibility,
                     const void* prevLengths, uint32_t W, uint32_t H, const void* visibilityOut, const void* lengthsOut,
                     TemporalList* out);                                                                                 // rts_scene.cpp

// ACCUMULATE KERNEL.  One pixel per lane, one workgroup of 256 lanes per block of 16 x 16 pixels, each of its four waves 16 x 4 of
// them.  Most of the pass's bytes are streamed -- this frame's texel, its visibility, both outputs -- and a wave's row of 16 pixels is
// 256 contiguous bytes of texels and 64 of a float plane: whole cache lines.  The four gathers of a wave's lanes fall in a patch of
// about 17 x 5 texels of the previous frame.  A wave of 8 x 8 pixels has the more compact patch (9 x 9) but halves every contiguous
// run; measured, it was 1.1 to 1.55 times slower on every row and was deleted (EXPERIMENTS.md, DESIGN.md 4.23).  No LDS: where the
// patch lies depends on the data.  The geometry of the four taps is decided once per pixel (a 4-bit mask); the light loop sits
// behind the wave-uniform l < count.  A tap of weight 0 or a rejected tap is never loaded, so a still camera costs one texel and one
// gather per light.  What is streamed once goes non-temporal; the previous frame's texels and history, which neighbours share, plain.
// No buffer needs more than its element type's alignment, so a texel is three dword loads.
struct TemporalDeviceFrames {
    const float *positions, *normals, *visibility, *prevPositions, *prevNormals, *history;
    const uint8_t *map, *prevLengths;
    float* visibilityOut;
    uint8_t* lengthsOut;
    uint64_t W, n;
    __device__ uint64_t at(int x, int y) const { return (uint64_t)y * W + (uint64_t)x; }
    __device__ static V3 streamed(const float* base, uint64_t i) {
        const float* v = base + i * 4;
        return V3{ __builtin_nontemporal_load(v), __builtin_nontemporal_load(v + 1), __builtin_nontemporal_load(v + 2) };
    }
    __device__ static V3 shared(const float* base, uint64_t i) { const float* v = base + i * 4; return V3{ v[0], v[1], v[2] }; }
    __device__ V3 normal(int x, int y) const { return streamed(normals, at(x, y)); }
    __device__ V3 position(int x, int y) const { return streamed(positions, at(x, y)); }
    __device__ uint32_t bits(int x, int y) const { return map ? __builtin_nontemporal_load(map + at(x, y)) : 0xFFu; }
    __device__ uint32_t current(uint32_t l, int x, int y) const {
        return __float_as_uint(__builtin_nontemporal_load(visibility + (uint64_t)l * n + at(x, y)));      // (a register move: the bits stay)
    }
    __device__ V3 prevNormal(int x, int y) const { return shared(prevNormals, at(x, y)); }
    __device__ V3 prevPosition(int x, int y) const { return shared(prevPositions, at(x, y)); }
    __device__ uint32_t prevLength(uint32_t l, int x, int y) const { return prevLengths[(uint64_t)l * n + at(x, y)]; }
    __device__ float prevVisibility(uint32_t l, int x, int y) const { return history[(uint64_t)l * n + at(x, y)]; }
    __device__ void store(uint32_t l, int x, int y, uint32_t bits, uint32_t length) const {
        __builtin_nontemporal_store(__uint_as_float(bits), visibilityOut + (uint64_t)l * n + at(x, y));
        __builtin_nontemporal_store((uint8_t)length, lengthsOut + (uint64_t)l * n + at(x, y));
    }
};

__global__ __launch_bounds__(256) void accumulateListKernel(TemporalList f, TemporalDeviceFrames t, int W, int H) {
    const int x = (int)blockIdx.x * 16 + (int)threadIdx.x, y = (int)blockIdx.y * 16 + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    accumulatePixel(f, t, x, y, W, H);
}
} // namespace rts_harness

extern "C" int rtsh_accumulate_visibility_list_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_temporal_params* params,
                                                      const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                      const float* d_visibility, const float* d_prev_positions,
                                                      const float* d_prev_normals, const float* d_prev_visibility,
                                                      const uint8_t* d_prev_lengths, uint32_t W, uint32_t H, float* d_visibility_out,
                                                      uint8_t* d_lengths_out, void* stream) {
    if (!ctx) return RTS_ERR_INVALID_ARG;
    rts_harness::TemporalList f;
    const int s = rts_harness::makeTemporalList(list, params, d_positions, d_normals, d_visibility, d_prev_positions, d_prev_normals,
                                                d_prev_visibility, d_prev_lengths, W, H, d_visibility_out, d_lengths_out, &f);
    if (s != RTS_OK) return s;
    // W, H <= 65536 (makeTemporalList): at most 4096 x 4096 blocks, inside every grid limit
    const rts_harness::TemporalDeviceFrames t{ d_positions, d_normals, d_visibility, d_prev_positions, d_prev_normals, d_prev_visibility,
                                               d_lights_map, d_prev_lengths, d_visibility_out, d_lengths_out, W, (uint64_t)W * H };
    return rts_harness::launchPass(ctx, stream, dim3((W + 15) / 16, (H + 15) / 16), dim3(16, 16), 0, rts_harness::accumulateListKernel, f, t,
                                   (int)W, (int)H);
}
