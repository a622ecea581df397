// Host-only check of the guided mean filter with a propagated variance (tests/test_list_propagated_host.py, built with
// -fsanitize=address,undefined,float-cast-overflow together with raytracedshadows_amd/csrc/rts_scene.cpp):
// rtsh_wide_filter_propagated_mean_soft_light_list on small frames of awkward texels (NaN, Inf, huge normals and positions; arbitrary
// bytes, means and squares, 65535 and 2^32 - 1 included) whose buffers are heap blocks of exactly the stated size with guard bytes
// behind the output -- so that a read of a plane from the count up, of a tap outside the frame or a write behind the output is
// reported.  The sanitizers are the first check; the second: visibility stays in [0, 1], one and three threads give the same bits,
// passes <= 1 with by_length == 0 gives the guided mean filter's bits (anchor 1), guide_k4 == 0 the passes == 0 plane (anchor 2),
// lengths of 1 make by_length a no-op (anchor 7), rtsh_wide_variance_step at its extremes, and a refusal writes nothing.  Prints the
// first case that differs and exits 1; "ok <cases>" otherwise.
#include "../../include/rts_scene.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

// rts_scene.cpp's traces validate their stream through the library proper; the pass under test never gets there
extern "C" int rts_bvh_validate(const rts_vec4u*, size_t, uint32_t*) { return RTS_ERR_INVALID_ARG; }

static unsigned long cases = 0;

#define CHECK(got, want, ...) \
    do { ++cases; if ((got) != (want)) { std::printf(__VA_ARGS__); std::printf(": got %ld, want %ld\n", (long)(got), (long)(want)); std::exit(1); } } while (0)

static const float kInf = std::numeric_limits<float>::infinity();
static const float kNaN = std::numeric_limits<float>::quiet_NaN();
static const float kValues[] = { 0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 1e-41f, 1e7f, 1e30f, 3e38f, -3e38f, kInf, -kInf, kNaN };
static const int kCount = (int)(sizeof(kValues) / sizeof(kValues[0]));
enum { GUARD = 16 };

static uint32_t state = 2463534242u;
static uint32_t next() { state = state * 1664525u + 1013904223u; return state >> 8; }
static float value() { return (next() & 3u) ? (float)((int)(next() % 2001u) - 1000) * 0.002f : kValues[next() % (uint32_t)kCount]; }

template <class T> static T* block(size_t n) { return (T*)std::malloc(n * sizeof(T)); }      // exactly n elements
template <class T> static T* guarded(size_t n) { unsigned char* p = (unsigned char*)std::malloc(n * sizeof(T) + GUARD); std::memset(p, 0xAB, n * sizeof(T) + GUARD); return (T*)p; }
template <class T> static bool guardOk(const T* p, size_t n) {
    const unsigned char* g = (const unsigned char*)(p + n);
    for (int i = 0; i < GUARD; ++i) if (g[i] != 0xAB) return false;
    return true;
}
template <class T> static bool allAB(const T* p, size_t n) {
    const unsigned char* g = (const unsigned char*)p;
    for (size_t i = 0; i < n * sizeof(T); ++i) if (g[i] != 0xAB) return false;
    return true;
}

static const uint32_t kSamples[8] = { 4, 16, 48, 1, 0, 4, 16, 48 };

static void list(uint32_t count, rts_soft_light_list* soft) {
    std::memset(soft, 0, sizeof(*soft));
    soft->count = count;
    for (uint32_t l = 0; l < count; ++l) {
        soft->lights[l].type = (l & 1u) ? RTS_LIGHT_POINT : RTS_LIGHT_DIRECTIONAL;
        soft->lights[l].nsamples = kSamples[l];
        soft->lights[l].first = kSamples[l] < 2 ? 0 : 48 - kSamples[l];
        soft->lights[l].radius = 0.25f;
    }
}

struct Frame {
    uint32_t W, H, planes;
    size_t n;
    float *normals, *positions;
    uint8_t *map, *counts, *lengths, *ones;
    uint16_t* mean;
    uint32_t* square;
    Frame(uint32_t w, uint32_t h, uint32_t planes_) : W(w), H(h), planes(planes_), n((size_t)w * h) {
        normals = block<float>(n * 4); positions = block<float>(n * 4);
        map = block<uint8_t>(n); counts = block<uint8_t>(n * planes); lengths = block<uint8_t>(n * planes); ones = block<uint8_t>(n * planes);
        mean = block<uint16_t>(n * planes); square = block<uint32_t>(n * planes);
        for (size_t i = 0; i < n * 4; ++i) { normals[i] = (next() % 7u) ? value() : 0.0f; positions[i] = value(); }
        for (size_t i = 0; i < n; ++i) {
            if (next() % 5u == 0) normals[i * 4] = normals[i * 4 + 1] = normals[i * 4 + 2] = 0.0f;   // background
            if (next() % 2u == 0) {                                      // a floor: taps that pass geom
                normals[i * 4] = 0.0f; normals[i * 4 + 1] = 1.0f; normals[i * 4 + 2] = 0.0f;
                positions[i * 4] = (float)(i % w) * 0.1f; positions[i * 4 + 1] = 0.25f; positions[i * 4 + 2] = (float)(i / w) * 0.1f;
            }
            map[i] = (uint8_t)next();
        }
        static const uint8_t lens[5] = { 0, 1, 2, 254, 255 };
        for (size_t i = 0; i < n * planes; ++i) {
            counts[i] = (uint8_t)(next() % 52u);
            lengths[i] = lens[next() % 5u];
            ones[i] = 1;
            mean[i] = (uint16_t)((next() & 3u) ? next() : ((next() & 1u) ? 65535u : 0u));
            square[i] = (next() & 3u) ? next() * 251u : ((next() & 1u) ? 0xFFFFFFFFu : 0u);
        }
    }
    ~Frame() {
        std::free(normals); std::free(positions); std::free(map); std::free(counts); std::free(lengths); std::free(ones); std::free(mean);
        std::free(square);
    }
};

static rtsh_wide_guide_propagated_params rule(uint32_t passes, uint32_t k4, uint32_t minHistory, uint32_t byLength) {
    rtsh_wide_guide_propagated_params p;
    std::memset(&p, 0, sizeof(p));
    p.passes = passes; p.normal_cos_min = 0.5f; p.plane_eps = 10.0f; p.guide_k4 = k4; p.min_history = minHistory; p.by_length = byLength;
    return p;
}

static int run(const Frame& f, const rts_soft_light_list* soft, const rtsh_wide_guide_propagated_params* p, bool withMap, const uint8_t* lengths,
               float* out, int threads) {
    return rtsh_wide_filter_propagated_mean_soft_light_list(soft, p, f.positions, f.normals, withMap ? f.map : nullptr, f.counts, f.mean,
                                                            f.square, lengths, f.W, f.H, out, threads);
}

static void frames() {
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 2 }, { 17, 1 }, { 1, 5 }, { 9, 9 }, { 40, 24 } };
    static const uint32_t k4s[] = { 0, 1, 12, 255 }, histories[] = { 1, 4, 255 };
    for (const auto& wh : sizes) for (uint32_t count : { 1u, 4u, 8u }) {
        Frame f(wh[0], wh[1], count);                                   // exactly `count` planes of everything
        const size_t m = f.n * count;
        rts_soft_light_list soft;
        list(count, &soft);
        float *out = guarded<float>(m), *out2 = guarded<float>(m), *raw = guarded<float>(m);
        for (int withMap = 0; withMap < 2; ++withMap) {
            rtsh_wide_guide_propagated_params zero = rule(0, 12, 4, 0);
            CHECK(run(f, &soft, &zero, withMap, f.lengths, raw, 1), RTS_OK, "passes 0");
            for (uint32_t passes = 0; passes <= 5; ++passes) for (uint32_t k4 : k4s) for (uint32_t byLength = 0; byLength < 2; ++byLength) {
                const uint32_t minHistory = histories[(passes + k4 + byLength) % 3u];
                rtsh_wide_guide_propagated_params p = rule(passes, k4, minHistory, byLength);
                CHECK(run(f, &soft, &p, withMap, f.lengths, out, 1), RTS_OK, "%ux%u count %u passes %u k4 %u", f.W, f.H, count, passes, k4);
                CHECK(guardOk(out, m), true, "guard behind visibility");
                for (size_t i = 0; i < m; ++i) CHECK(out[i] >= 0.0f && out[i] <= 1.0f, true, "range at %zu", i);
                CHECK(run(f, &soft, &p, withMap, f.lengths, out2, 3), RTS_OK, "three threads");
                CHECK(std::memcmp(out, out2, m * sizeof(float)), 0, "threads change bits: passes %u k4 %u", passes, k4);
                if (k4 == 0)                                            // anchor 2
                    for (uint32_t l = 0; l < count; ++l)
                        if (kSamples[l] >= 2) CHECK(std::memcmp(out + l * f.n, raw + l * f.n, f.n * sizeof(float)), 0, "anchor 2, light %u", l);
                if (passes <= 1 && byLength == 0) {                     // anchor 1
                    rtsh_wide_guide_temporal_params g;
                    std::memset(&g, 0, sizeof(g));
                    g.passes = passes; g.normal_cos_min = 0.5f; g.plane_eps = 10.0f; g.guide_k4 = k4; g.min_history = minHistory;
                    CHECK(rtsh_wide_filter_guided_temporal_mean_soft_light_list(&soft, &g, f.positions, f.normals, withMap ? f.map : nullptr,
                                                                                f.counts, f.mean, f.square, f.lengths, f.W, f.H, out2, 1),
                          RTS_OK, "guided mean filter");
                    CHECK(std::memcmp(out, out2, m * sizeof(float)), 0, "anchor 1: passes %u k4 %u", passes, k4);
                }
                if (byLength == 1) {                                    // anchor 7
                    rtsh_wide_guide_propagated_params q = rule(passes, k4, 1, 0), q1 = rule(passes, k4, 1, 1);
                    CHECK(run(f, &soft, &q, withMap, f.ones, out, 1), RTS_OK, "lengths of 1");
                    CHECK(run(f, &soft, &q1, withMap, f.ones, out2, 1), RTS_OK, "lengths of 1, by_length");
                    CHECK(std::memcmp(out, out2, m * sizeof(float)), 0, "anchor 7: passes %u k4 %u", passes, k4);
                }
            }
        }
        // refusals write nothing
        std::memset(out, 0xAB, m * sizeof(float));
        rtsh_wide_guide_propagated_params bad = rule(3, 12, 4, 2);
        CHECK(run(f, &soft, &bad, true, f.lengths, out, 1), RTS_ERR_INVALID_ARG, "by_length 2");
        bad = rule(6, 12, 4, 0);
        CHECK(run(f, &soft, &bad, true, f.lengths, out, 1), RTS_ERR_INVALID_ARG, "passes 6");
        bad = rule(3, 12, 0, 0);
        CHECK(run(f, &soft, &bad, true, f.lengths, out, 1), RTS_ERR_INVALID_ARG, "min_history 0");
        bad = rule(3, 12, 4, 0);
        CHECK(run(f, &soft, &bad, true, nullptr, out, 1), RTS_ERR_INVALID_ARG, "NULL lengths");
        CHECK(run(f, &soft, nullptr, true, f.lengths, out, 1), RTS_ERR_INVALID_ARG, "NULL params");
        CHECK(allAB(out, m), true, "a refusal wrote");
        std::free(out); std::free(out2); std::free(raw);
    }
}

static void varianceStep() {
    const uint64_t top = 0xFFFFFFFFull;
    CHECK(rtsh_wide_variance_step(1296ull * top, 36), top, "the centre alone keeps Q");
    CHECK(rtsh_wide_variance_step(4900ull * top, 256), (2ull * 4900ull * top + 65536ull) / 131072ull, "all 25 taps at the largest Q");
    CHECK(rtsh_wide_variance_step(0, 36), 0, "zero");
    CHECK(rtsh_wide_variance_step(0, 256), 0, "zero, full");
    CHECK(rtsh_wide_variance_step(648, 36), 1, "a half rounds up");
    CHECK(rtsh_wide_variance_step(647, 36), 0, "below a half rounds down");
    CHECK(rtsh_wide_variance_step(1, 0), top, "den 0 is outside the domain");
    CHECK(rtsh_wide_variance_step(1, 257), top, "den 257 is outside the domain");
    for (uint32_t den = 36; den <= 256; ++den)
        for (int k = 0; k < 200; ++k) {
            const uint64_t numQ = (((uint64_t)next() << 24) ^ next()) % ((uint64_t)den * den * top + 1u);
            const uint64_t d2 = (uint64_t)den * den;
            CHECK(rtsh_wide_variance_step(numQ, den), (2u * numQ + d2) / (2u * d2), "den %u numQ %llu", den, (unsigned long long)numQ);
        }
}

int main() {
    CHECK(sizeof(rtsh_wide_guide_propagated_params), 32, "the struct's size");
    CHECK(rtsh_wide_filter_propagated_scratch_bytes(8, 40, 24), 12u * 8u * 40u * 24u, "scratch bytes");
    CHECK(rtsh_wide_filter_propagated_scratch_bytes(9, 40, 24), 0, "scratch bytes of 9 lights");
    varianceStep();
    frames();
    std::printf("ok %lu\n", cases);
    return 0;
}
