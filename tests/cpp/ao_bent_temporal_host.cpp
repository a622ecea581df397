// Host-only check of the temporal accumulation of the bent texel and of the wide bent filter fed from it
// (tests/test_ao_bent_temporal_host.py, built with -fsanitize=address,undefined,float-cast-overflow together with
// raytracedshadows_amd/csrc/rts_scene.cpp): rtsh_accumulate_bent, rtsh_accumulate_bent_motion and rtsh_wide_filter_bent_mean over every
// refusal of include/rts_scene.h and over small frames of awkward texels -- NaN, Inf, huge and denormal floats in both G-buffers, in the
// motion planes and in the bent plane; any 8 bytes in the history, 0x8000 components and V = 65535 included; lengths 0, 1, 2, 254, 255
// -- whose buffers are heap blocks of exactly the stated size, so that a gather outside the previous frame or a write behind an output
// is reported, and a float that does not fit its integer is reported by float-cast-overflow.  The sanitizers are the first check; the
// second: an inactive pixel is an all-zero texel of length 0, an active one has a length in 1 .. max_length, one thread and three
// threads give the same bytes, the first frame equals a reset, the filter's output lies in [-1, 1] (.w in [0, 1]), and the refusals
// leave the outputs as they were.  Prints the first case that differs and exits 1; "ok <cases>" otherwise.
#include "../../include/rts_scene.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

// rts_scene.cpp's traces validate their stream through the library proper; the passes under test never get there
extern "C" int rts_bvh_validate(const rts_vec4u*, size_t, uint32_t*) { return RTS_ERR_INVALID_ARG; }

static unsigned long cases = 0;

#define CHECK(got, want, ...) \
    do { ++cases; if ((got) != (want)) { std::printf(__VA_ARGS__); std::printf(": got %d, want %d\n", (int)(got), (int)(want)); std::exit(1); } } while (0)

static const float kInf = std::numeric_limits<float>::infinity();
static const float kNaN = std::numeric_limits<float>::quiet_NaN();
static const float kValues[] = { 0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 1e-41f, 1e7f, 1e30f, 3e38f, -3e38f, kInf, -kInf, kNaN };
static const int kCount = (int)(sizeof(kValues) / sizeof(kValues[0]));

static uint32_t state = 2463534242u;
static uint32_t next() { state = state * 1664525u + 1013904223u; return state >> 8; }
static float value() { return (next() & 3u) ? (float)((int)(next() % 2001u) - 1000) * 0.002f : kValues[next() % (uint32_t)kCount]; }

template <class T> static T* block(size_t n) { return (T*)std::malloc(n * sizeof(T)); }      // exactly n elements

struct Frame {
    uint32_t W, H;
    size_t n;
    float *normals, *positions, *prevNormals, *prevPositions, *points, *pointNormals, *bent, *out, *ao;
    uint64_t *history, *texels, *texels2;
    uint8_t *map, *prevLengths, *lengths, *lengths2;
    Frame(uint32_t w, uint32_t h, uint32_t samples) : W(w), H(h), n((size_t)w * h) {
        normals = block<float>(n * 4); positions = block<float>(n * 4); prevNormals = block<float>(n * 4); prevPositions = block<float>(n * 4);
        points = block<float>(n * 4); pointNormals = block<float>(n * 4); bent = block<float>(n * 4); out = block<float>(n * 4);
        ao = block<float>(n);
        history = block<uint64_t>(n); texels = block<uint64_t>(n); texels2 = block<uint64_t>(n);
        map = block<uint8_t>(n); prevLengths = block<uint8_t>(n); lengths = block<uint8_t>(n); lengths2 = block<uint8_t>(n);
        static const uint8_t kLengths[] = { 0, 1, 2, 254, 255 };
        static const uint16_t kWords[] = { 0x8000, 0x7FFF, 0, 1, 0xFFFF, 0x1234 };
        for (size_t i = 0; i < n; ++i) {
            const uint32_t x = (uint32_t)(i % W), y = (uint32_t)(i / W);
            // a plane z = -4 seen by the camera of params(): most pixels reproject near themselves; then awkward floats on top
            float* P = positions + i * 4; float* N = normals + i * 4;
            P[0] = (((float)x + 0.5f) / (float)W * 2.0f - 1.0f) * 4.0f; P[1] = (1.0f - ((float)y + 0.5f) / (float)H * 2.0f) * 4.0f; P[2] = -4.0f; P[3] = 1.0f;
            N[0] = 0.0f; N[1] = 0.0f; N[2] = 1.0f; N[3] = 0.0f;
            for (int c = 0; c < 4; ++c) {
                prevPositions[i * 4 + c] = P[c]; prevNormals[i * 4 + c] = N[c];
                points[i * 4 + c] = c < 2 ? P[c] + value() * 0.5f : P[c]; pointNormals[i * 4 + c] = N[c];
            }
            if (next() % 6u == 0) for (int c = 0; c < 3; ++c) { P[c] = value() * 8.0f; points[i * 4 + c] = value() * 8.0f; }
            if (next() % 6u == 0) for (int c = 0; c < 3; ++c) prevPositions[i * 4 + c] = value();
            if (next() % 7u == 0) for (int c = 0; c < 3; ++c) N[c] = value();
            if (next() % 7u == 0) for (int c = 0; c < 3; ++c) prevNormals[i * 4 + c] = value();
            if (next() % 7u == 0) for (int c = 0; c < 3; ++c) pointNormals[i * 4 + c] = (next() & 1u) ? 0.0f : value();
            if (next() % 6u == 0) N[0] = N[1] = N[2] = 0.0f;                                         // background
            if (next() % 6u == 0) prevNormals[i * 4] = prevNormals[i * 4 + 1] = prevNormals[i * 4 + 2] = 0.0f;
            map[i] = (next() % 4u) ? (uint8_t)(next() | 1u) : (uint8_t)0;
            prevLengths[i] = kLengths[next() % 5u];
            uint64_t t = 0;
            for (int c = 0; c < 4; ++c) t |= (uint64_t)((next() & 1u) ? kWords[next() % 6u] : (uint16_t)next()) << (16 * c);
            history[i] = t;
            for (int c = 0; c < 3; ++c) bent[i * 4 + c] = (next() & 3u) ? value() * (float)samples : kValues[next() % (uint32_t)kCount];
            bent[i * 4 + 3] = (next() & 3u) ? (float)(next() % (samples + 2u)) : value() * 60.0f;
        }
        reset();
    }
    void reset() {
        for (size_t i = 0; i < n; ++i) { texels[i] = texels2[i] = 0xABABABABABABABABull; lengths[i] = lengths2[i] = 0xAB; ao[i] = 7.5f; }
        for (size_t i = 0; i < n * 4; ++i) out[i] = 7.5f;
    }
    bool untouched() const {
        for (size_t i = 0; i < n; ++i) if (texels[i] != 0xABABABABABABABABull || lengths[i] != 0xAB || ao[i] != 7.5f) return false;
        for (size_t i = 0; i < n * 4; ++i) if (out[i] != 7.5f) return false;
        return true;
    }
    ~Frame() {
        for (float* p : { normals, positions, prevNormals, prevPositions, points, pointNormals, bent, out, ao }) std::free(p);
        for (uint64_t* p : { history, texels, texels2 }) std::free(p);
        for (uint8_t* p : { map, prevLengths, lengths, lengths2 }) std::free(p);
    }
};

static rtsh_temporal_params params(uint32_t maxLength, uint32_t reset) {
    rtsh_temporal_params p;
    std::memset(&p, 0, sizeof(p));
    p.eye_delta[0] = 0.013f; p.eye_delta[1] = -0.021f;
    p.prev_right[0] = 1.0f; p.prev_up[1] = 1.0f; p.prev_fwd[2] = -1.0f;
    p.prev_scale_x = 1.0f; p.prev_scale_y = 1.0f;
    p.normal_cos_min = 0.5f; p.plane_eps = 10.0f;
    p.max_length = maxLength; p.reset_lights = reset;
    return p;
}

static rtsh_wide_filter_params filterParams(uint32_t passes) {
    rtsh_wide_filter_params p;
    std::memset(&p, 0, sizeof(p));
    p.passes = passes; p.normal_cos_min = 0.5f; p.plane_eps = 10.0f;
    return p;
}

static bool background(const Frame& f, size_t i) { return f.normals[i * 4] == 0.0f && f.normals[i * 4 + 1] == 0.0f && f.normals[i * 4 + 2] == 0.0f; }

static int accumulate(const Frame& f, const rtsh_temporal_params& p, uint32_t samples, const uint8_t* map, bool history, int motion,
                      uint64_t* texels, uint8_t* lengths, int threads) {
    const float* pp = history ? f.prevPositions : nullptr; const float* pn = history ? f.prevNormals : nullptr;
    const uint64_t* pt = history ? f.history : nullptr; const uint8_t* pl = history ? f.prevLengths : nullptr;
    if (motion)
        return rtsh_accumulate_bent_motion(&p, samples, f.positions, f.normals, map, f.bent, pp, pn, pt, pl, f.points, f.pointNormals, f.W, f.H,
                                           texels, lengths, threads);
    return rtsh_accumulate_bent(&p, samples, f.positions, f.normals, map, f.bent, pp, pn, pt, pl, f.W, f.H, texels, lengths, threads);
}

static void frames() {
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 2 }, { 17, 1 }, { 1, 5 }, { 9, 9 }, { 40, 24 } };
    for (const auto& wh : sizes) for (uint32_t samples : { 0u, 1u, 4u, 48u }) {
        Frame f(wh[0], wh[1], samples ? samples : 1u);
        for (uint32_t maxLength : { 1u, 2u, 5u, 255u }) for (int withMap = 0; withMap < 2; ++withMap) for (int motion = 0; motion < 2; ++motion) {
            const uint8_t* map = withMap ? f.map : nullptr;
            const rtsh_temporal_params p = params(maxLength, 0);
            CHECK(accumulate(f, p, samples, map, true, motion, f.texels, f.lengths, 1), RTS_OK, "%ux%u samples %u max_length %u motion %d",
                  f.W, f.H, samples, maxLength, motion);
            CHECK(accumulate(f, p, samples, map, true, motion, f.texels2, f.lengths2, 3), RTS_OK, "3 threads");
            CHECK(std::memcmp(f.texels, f.texels2, f.n * 8), 0, "threads change texels, %ux%u", f.W, f.H);
            CHECK(std::memcmp(f.lengths, f.lengths2, f.n), 0, "threads change lengths, %ux%u", f.W, f.H);
            for (size_t i = 0; i < f.n; ++i) {
                const bool on = !background(f, i) && (!map || map[i] != 0);
                if (!on) CHECK(f.texels[i] == 0 && f.lengths[i] == 0, true, "inactive pixel %zu of %ux%u", i, f.W, f.H);
                else CHECK(f.lengths[i] >= 1 && f.lengths[i] <= maxLength, true, "length of pixel %zu of %ux%u", i, f.W, f.H);
            }
            // the first frame and a reset: the same bytes, every length 0 or 1
            const rtsh_temporal_params r = params(maxLength, 1);
            CHECK(accumulate(f, p, samples, map, false, motion, f.texels, f.lengths, 2), RTS_OK, "first frame");
            CHECK(accumulate(f, r, samples, map, true, motion, f.texels2, f.lengths2, 2), RTS_OK, "reset");
            CHECK(std::memcmp(f.texels, f.texels2, f.n * 8), 0, "first frame != reset, %ux%u", f.W, f.H);
            CHECK(std::memcmp(f.lengths, f.lengths2, f.n), 0, "first frame != reset (lengths), %ux%u", f.W, f.H);
            for (size_t i = 0; i < f.n; ++i) CHECK(f.lengths[i] <= 1, true, "first-frame length, pixel %zu", i);
        }
        // the filter over the awkward history as it is: any 8 bytes are legal, the output stays in range
        for (uint32_t passes = 0; passes <= (uint32_t)RTSH_WIDE_FILTER_MAX_PASSES; ++passes) for (int withMap = 0; withMap < 2; ++withMap) {
            const rtsh_wide_filter_params p = filterParams(passes);
            const uint8_t* map = withMap ? f.map : nullptr;
            CHECK(rtsh_wide_filter_bent_mean(&p, samples, f.positions, f.normals, map, f.history, f.W, f.H, f.out, withMap ? f.ao : nullptr, 2),
                  RTS_OK, "filter %ux%u samples %u passes %u", f.W, f.H, samples, passes);
            for (size_t i = 0; i < f.n; ++i) {
                const bool on = !background(f, i) && (!map || map[i] != 0);
                for (int c = 0; c < 4; ++c) {
                    const float v = f.out[i * 4 + c];
                    uint32_t u; std::memcpy(&u, &v, 4);
                    if (!on) CHECK(u, 0u, "inactive pixel %zu of %ux%u", i, f.W, f.H);
                    else CHECK(v >= (c < 3 ? -1.0f : 0.0f) && v <= 1.0f, true, "out of range, pixel %zu component %d", i, c);
                }
            }
        }
    }
}

static void refusals() {
    Frame f(5, 3, 4);
    const rtsh_temporal_params good = params(5, 0);
#define REFUSED(call, what) do { CHECK(call, RTS_ERR_INVALID_ARG, what); CHECK(f.untouched(), true, what ": output written"); } while (0)
    auto ACC = [&](const rtsh_temporal_params* p, uint32_t ns, const float* pos, const float* nrm, const float* b, const float* pp,
                   const float* pn, const void* pt, const uint8_t* pl, uint32_t w, uint32_t h, void* to, uint8_t* lo) {
        return rtsh_accumulate_bent(p, ns, pos, nrm, f.map, b, pp, pn, pt, pl, w, h, to, lo, 0);
    };
#define PREV f.prevPositions, f.prevNormals, f.history, f.prevLengths
    REFUSED(ACC(nullptr, 4, f.positions, f.normals, f.bent, PREV, f.W, f.H, f.texels, f.lengths), "NULL params");
    for (uint32_t ns : { 49u, 64u, 0xFFFFFFFFu }) REFUSED(ACC(&good, ns, f.positions, f.normals, f.bent, PREV, f.W, f.H, f.texels, f.lengths), "nsamples > 48");
    REFUSED(ACC(&good, 4, nullptr, f.normals, f.bent, PREV, f.W, f.H, f.texels, f.lengths), "NULL positions");
    REFUSED(ACC(&good, 4, f.positions, nullptr, f.bent, PREV, f.W, f.H, f.texels, f.lengths), "NULL normals");
    REFUSED(ACC(&good, 4, f.positions, f.normals, nullptr, PREV, f.W, f.H, f.texels, f.lengths), "NULL bent");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, PREV, f.W, f.H, nullptr, f.lengths), "NULL texels_out");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, PREV, f.W, f.H, f.texels, nullptr), "NULL lengths_out");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, nullptr, f.prevNormals, f.history, f.prevLengths, f.W, f.H, f.texels, f.lengths), "three prev (positions)");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, f.prevPositions, nullptr, f.history, f.prevLengths, f.W, f.H, f.texels, f.lengths), "three prev (normals)");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, f.prevPositions, f.prevNormals, nullptr, f.prevLengths, f.W, f.H, f.texels, f.lengths), "three prev (texels)");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, f.prevPositions, f.prevNormals, f.history, nullptr, f.W, f.H, f.texels, f.lengths), "three prev (lengths)");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, f.prevPositions, f.prevNormals, f.texels, f.prevLengths, f.W, f.H, f.texels, f.lengths), "texels_out == prev_texels");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, f.prevPositions, f.prevNormals, f.history, f.lengths, f.W, f.H, f.texels, f.lengths), "lengths_out == prev_lengths");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, PREV, 0, f.H, f.texels, f.lengths), "W 0");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, PREV, f.W, 0, f.texels, f.lengths), "H 0");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, PREV, 65537, 1, f.texels, f.lengths), "W too large");
    REFUSED(ACC(&good, 4, f.positions, f.normals, f.bent, PREV, 1, 65537, f.texels, f.lengths), "H too large");
    for (uint32_t m : { 0u, 256u, 0xFFFFFFFFu }) {
        rtsh_temporal_params p = good; p.max_length = m;
        REFUSED(ACC(&p, 4, f.positions, f.normals, f.bent, PREV, f.W, f.H, f.texels, f.lengths), "max_length");
    }
    for (float v : { kNaN, kInf, -kInf }) {
        rtsh_temporal_params p = good; p.eye_delta[2] = v;
        REFUSED(ACC(&p, 4, f.positions, f.normals, f.bent, PREV, f.W, f.H, f.texels, f.lengths), "eye_delta");
        p = good; p.prev_fwd[0] = v;
        REFUSED(ACC(&p, 4, f.positions, f.normals, f.bent, PREV, f.W, f.H, f.texels, f.lengths), "prev_fwd");
        p = good; p.normal_cos_min = v;
        REFUSED(ACC(&p, 4, f.positions, f.normals, f.bent, PREV, f.W, f.H, f.texels, f.lengths), "normal_cos_min");
        p = good; p.plane_eps = v;
        REFUSED(ACC(&p, 4, f.positions, f.normals, f.bent, PREV, f.W, f.H, f.texels, f.lengths), "plane_eps");
        p = good; p.prev_scale_x = v;
        REFUSED(ACC(&p, 4, f.positions, f.normals, f.bent, PREV, f.W, f.H, f.texels, f.lengths), "prev_scale_x");
    }
    for (float v : { 0.0f, -1.0f }) {
        rtsh_temporal_params p = good; p.prev_scale_y = v;
        REFUSED(ACC(&p, 4, f.positions, f.normals, f.bent, PREV, f.W, f.H, f.texels, f.lengths), "prev_scale_y");
    }
    REFUSED(rtsh_accumulate_bent_motion(&good, 4, f.positions, f.normals, f.map, f.bent, PREV, nullptr, f.pointNormals, f.W, f.H, f.texels,
                                        f.lengths, 0), "motion: NULL prev_points");
    REFUSED(rtsh_accumulate_bent_motion(&good, 4, f.positions, f.normals, f.map, f.bent, PREV, f.points, nullptr, f.W, f.H, f.texels, f.lengths, 0),
            "motion: NULL prev_point_normals");
    CHECK(rtsh_accumulate_bent_motion(&good, 4, f.positions, f.normals, f.map, f.bent, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, f.W,
                                      f.H, f.texels2, f.lengths2, 0), RTS_OK, "motion: the first frame needs no motion planes");
    CHECK(ACC(&good, 48, f.positions, f.normals, f.bent, PREV, f.W, f.H, f.texels2, f.lengths2), RTS_OK, "48 samples are allowed");

    const rtsh_wide_filter_params fine = filterParams(3);
#define MEAN(p, ns, pos, nrm, t, w, h, o) rtsh_wide_filter_bent_mean(p, ns, pos, nrm, f.map, t, w, h, o, f.ao, 0)
    for (uint32_t passes : { 6u, 0xFFFFFFFFu }) {
        rtsh_wide_filter_params p = fine; p.passes = passes;
        REFUSED(MEAN(&p, 4, f.positions, f.normals, f.history, f.W, f.H, f.out), "passes > 5");
    }
    for (float v : { kNaN, kInf, -kInf }) {
        rtsh_wide_filter_params p = fine; p.normal_cos_min = v;
        REFUSED(MEAN(&p, 4, f.positions, f.normals, f.history, f.W, f.H, f.out), "filter normal_cos_min");
        p = fine; p.plane_eps = v;
        REFUSED(MEAN(&p, 4, f.positions, f.normals, f.history, f.W, f.H, f.out), "filter plane_eps");
    }
    REFUSED(MEAN(&fine, 49, f.positions, f.normals, f.history, f.W, f.H, f.out), "filter nsamples > 48");
    REFUSED(MEAN(nullptr, 4, f.positions, f.normals, f.history, f.W, f.H, f.out), "filter NULL params");
    REFUSED(MEAN(&fine, 4, nullptr, f.normals, f.history, f.W, f.H, f.out), "filter NULL positions");
    REFUSED(MEAN(&fine, 4, f.positions, nullptr, f.history, f.W, f.H, f.out), "filter NULL normals");
    REFUSED(MEAN(&fine, 4, f.positions, f.normals, nullptr, f.W, f.H, f.out), "filter NULL texels");
    REFUSED(MEAN(&fine, 4, f.positions, f.normals, f.history, f.W, f.H, nullptr), "filter NULL out");
    REFUSED(MEAN(&fine, 4, f.positions, f.normals, f.history, 0, f.H, f.out), "filter W 0");
    REFUSED(MEAN(&fine, 4, f.positions, f.normals, f.history, f.W, 0, f.out), "filter H 0");
#undef REFUSED
#undef PREV
#undef MEAN
}

int main() {
    refusals();
    frames();
    std::printf("ok %lu\n", cases);
    return 0;
}
