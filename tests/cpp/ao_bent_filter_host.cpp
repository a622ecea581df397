// Host-only check of the wide filter of the bent plane (tests/test_ao_bent_filter_host.py, built with
// -fsanitize=address,undefined,float-cast-overflow together with raytracedshadows_amd/csrc/rts_scene.cpp): rtsh_wide_filter_bent over
// every refusal of include/rts_scene.h and over frames of awkward texels (NaN, Inf, huge and denormal floats in the G-buffer AND in the
// bent plane) -- the tiny ones (1 x 1, 3 x 2, 17 x 1: at large steps every tap but the centre is outside) and 72 x 72 (a step-16 pass with
// both far taps inside) -- whose buffers are heap blocks of exactly the stated size, so that a read of a texel outside the frame or a
// write behind `out` or `ao` is reported, and a float that does not fit its integer is reported by float-cast-overflow.  The sanitizers
// are the first check; the second: every value lies in [-1, 1] (.w in [0, 1]), an inactive pixel is four +0, ao holds out.w's bits, one
// thread and three threads give the same bits, the negated plane gives the negated vectors, and the refusals leave the outputs as they
// were.  Prints the first case that differs and exits 1; "ok <cases>" otherwise.
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
    float *normals, *positions, *bent, *negated, *out, *out2, *ao, *ao2;
    uint8_t* map;
    Frame(uint32_t w, uint32_t h, uint32_t samples) : W(w), H(h), n((size_t)w * h) {
        normals = block<float>(n * 4); positions = block<float>(n * 4); bent = block<float>(n * 4); negated = block<float>(n * 4);
        out = block<float>(n * 4); out2 = block<float>(n * 4); ao = block<float>(n); ao2 = block<float>(n);
        map = block<uint8_t>(n);
        for (size_t i = 0; i < n * 4; ++i) { normals[i] = (next() % 7u) ? value() : 0.0f; positions[i] = value(); }
        for (size_t i = 0; i < n; ++i) {
            if (next() % 5u == 0) normals[i * 4] = normals[i * 4 + 1] = normals[i * 4 + 2] = 0.0f;   // background
            if (next() % 2u == 0) { normals[i * 4] = 0.0f; normals[i * 4 + 1] = 1.0f; normals[i * 4 + 2] = 0.0f; positions[i * 4 + 1] = 0.25f; }
            map[i] = (next() % 3u) ? (uint8_t)(next() | 1u) : (uint8_t)0;
            for (int c = 0; c < 3; ++c) bent[i * 4 + c] = (next() & 3u) ? value() * (float)samples : kValues[next() % (uint32_t)kCount];
            bent[i * 4 + 3] = (next() & 3u) ? (float)(next() % (samples + 2u)) : value() * 60.0f;
            for (int c = 0; c < 4; ++c) negated[i * 4 + c] = c < 3 ? -bent[i * 4 + c] : bent[i * 4 + c];
        }
        reset();
    }
    void reset() { for (size_t i = 0; i < n * 4; ++i) out[i] = out2[i] = 7.5f; for (size_t i = 0; i < n; ++i) ao[i] = ao2[i] = 7.5f; }
    bool untouched() const {
        for (size_t i = 0; i < n * 4; ++i) if (out[i] != 7.5f) return false;
        for (size_t i = 0; i < n; ++i) if (ao[i] != 7.5f) return false;
        return true;
    }
    ~Frame() {
        std::free(normals); std::free(positions); std::free(bent); std::free(negated); std::free(out); std::free(out2); std::free(ao);
        std::free(ao2); std::free(map);
    }
};

static rtsh_wide_filter_params params(uint32_t passes) {
    rtsh_wide_filter_params p;
    std::memset(&p, 0, sizeof(p));
    p.passes = passes; p.normal_cos_min = 0.5f; p.plane_eps = 10.0f;
    return p;
}

static bool background(const Frame& f, size_t i) { return f.normals[i * 4] == 0.0f && f.normals[i * 4 + 1] == 0.0f && f.normals[i * 4 + 2] == 0.0f; }
static uint32_t bitsOf(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

static void frames() {
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 2 }, { 17, 1 }, { 1, 5 }, { 9, 9 }, { 72, 72 } };
    for (const auto& wh : sizes) for (uint32_t samples : { 0u, 1u, 4u, 16u, 48u }) {
        if (wh[0] == 72u && (samples == 0u || samples == 16u)) continue;
        Frame f(wh[0], wh[1], samples ? samples : 1u);
        for (uint32_t passes = 0; passes <= (uint32_t)RTSH_WIDE_FILTER_MAX_PASSES; ++passes) for (int withMap = 0; withMap < 2; ++withMap) {
            const rtsh_wide_filter_params p = params(passes);
            const uint8_t* map = withMap ? f.map : nullptr;
            CHECK(rtsh_wide_filter_bent(&p, samples, f.positions, f.normals, map, f.bent, f.W, f.H, f.out, f.ao, 1), RTS_OK,
                  "%ux%u samples %u passes %u", f.W, f.H, samples, passes);
            CHECK(rtsh_wide_filter_bent(&p, samples, f.positions, f.normals, map, f.bent, f.W, f.H, f.out2, f.ao2, 3), RTS_OK, "3 threads");
            CHECK(std::memcmp(f.out, f.out2, f.n * 16), 0, "threads change bits, %ux%u passes %u", f.W, f.H, passes);
            CHECK(std::memcmp(f.ao, f.ao2, f.n * 4), 0, "threads change ao, %ux%u passes %u", f.W, f.H, passes);
            for (size_t i = 0; i < f.n; ++i) {
                const bool on = !background(f, i) && (!map || map[i] != 0);
                CHECK(bitsOf(f.ao[i]), bitsOf(f.out[i * 4 + 3]), "ao is not out.w, pixel %zu", i);
                for (int c = 0; c < 4; ++c) {
                    const float v = f.out[i * 4 + c];
                    if (!on) CHECK(bitsOf(v), 0u, "inactive pixel %zu of %ux%u", i, f.W, f.H);
                    else CHECK(v >= (c < 3 ? -1.0f : 0.0f) && v <= 1.0f, true, "out of range, pixel %zu component %d", i, c);
                }
            }
            // the negated plane, without `ao`: the negated vectors, +0 staying +0
            CHECK(rtsh_wide_filter_bent(&p, samples, f.positions, f.normals, map, f.negated, f.W, f.H, f.out2, nullptr, 2), RTS_OK, "negated");
            for (size_t i = 0; i < f.n * 4; ++i) {
                const float v = f.out[i], m = f.out2[i];
                const uint32_t want = (i & 3u) == 3u || v == 0.0f ? bitsOf(v) : bitsOf(-v);
                CHECK(bitsOf(m), want, "negation, float %zu of %ux%u passes %u", i, f.W, f.H, passes);
            }
        }
    }
}

static void refusals() {
    Frame f(5, 3, 4);
    const rtsh_wide_filter_params good = params(3);
#define REFUSED(call, what) do { CHECK(call, RTS_ERR_INVALID_ARG, what); CHECK(f.untouched(), true, what ": output written"); } while (0)
#define BENT(p, ns, pos, nrm, b, w, h, o) rtsh_wide_filter_bent(p, ns, pos, nrm, f.map, b, w, h, o, f.ao, 0)
    for (uint32_t passes : { 6u, 0xFFFFFFFFu }) {
        rtsh_wide_filter_params p = good; p.passes = passes;
        REFUSED(BENT(&p, 4, f.positions, f.normals, f.bent, f.W, f.H, f.out), "passes > 5");
    }
    for (float v : { kNaN, kInf, -kInf }) {
        rtsh_wide_filter_params p = good; p.normal_cos_min = v;
        REFUSED(BENT(&p, 4, f.positions, f.normals, f.bent, f.W, f.H, f.out), "normal_cos_min");
        p = good; p.plane_eps = v;
        REFUSED(BENT(&p, 4, f.positions, f.normals, f.bent, f.W, f.H, f.out), "plane_eps");
    }
    for (uint32_t ns : { 49u, 64u, 0xFFFFFFFFu }) REFUSED(BENT(&good, ns, f.positions, f.normals, f.bent, f.W, f.H, f.out), "nsamples > 48");
    REFUSED(BENT(nullptr, 4, f.positions, f.normals, f.bent, f.W, f.H, f.out), "NULL params");
    REFUSED(BENT(&good, 4, nullptr, f.normals, f.bent, f.W, f.H, f.out), "NULL positions");
    REFUSED(BENT(&good, 4, f.positions, nullptr, f.bent, f.W, f.H, f.out), "NULL normals");
    REFUSED(BENT(&good, 4, f.positions, f.normals, nullptr, f.W, f.H, f.out), "NULL bent");
    REFUSED(BENT(&good, 4, f.positions, f.normals, f.bent, f.W, f.H, nullptr), "NULL out");
    REFUSED(BENT(&good, 4, f.positions, f.normals, f.bent, 0, f.H, f.out), "W 0");
    REFUSED(BENT(&good, 4, f.positions, f.normals, f.bent, f.W, 0, f.out), "H 0");
    REFUSED(BENT(&good, 4, f.positions, f.normals, f.bent, 0x7FFFFFF1u, 1, f.out), "W too large");
    REFUSED(BENT(&good, 4, f.positions, f.normals, f.bent, 1, 0x7FFFFFF1u, f.out), "H too large");
    CHECK(BENT(&good, 48, f.positions, f.normals, f.bent, f.W, f.H, f.out), RTS_OK, "48 samples are allowed");
    CHECK(rtsh_wide_filter_bent_scratch_bytes(5, 3), (size_t)(2 * 15 * 8), "scratch bytes");
    CHECK(rtsh_wide_filter_bent_scratch_bytes(0, 3), (size_t)0, "scratch bytes, W 0");
#undef REFUSED
#undef BENT
}

int main() {
    refusals();
    frames();
    std::printf("ok %lu\n", cases);
    return 0;
}
