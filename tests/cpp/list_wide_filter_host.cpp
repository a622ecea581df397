// Host-only check of the wide (a-trous) filter of a light list's planes (tests/test_list_wide_filter_host.py, built with
// -fsanitize=address,undefined,float-cast-overflow together with raytracedshadows_amd/csrc/rts_scene.cpp): rtsh_wide_filter_light_list
// and rtsh_wide_filter_soft_light_list over every refusal of include/rts_scene.h and over frames of awkward texels (NaN, Inf, huge and
// denormal normals and positions; arbitrary bytes) -- the tiny ones (1 x 1, 3 x 2, 17 x 1: at large steps every tap but the centre is
// outside) and 72 x 72 (a step-16 pass with both far taps inside) -- whose buffers are heap blocks of exactly the stated size, so that a
// read of a plane from the count up, of a texel outside the frame or a write behind visibility is reported.  The sanitizers are the
// first check; the second: passes == 0 gives (float)min(c, n) / (float)n, every value lies in [0, 1], one thread and three threads give
// the same bits, and the refusals leave the output as it was.  Prints the first case that differs and exits 1; "ok <cases>" otherwise.
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
    uint32_t W, H, planes;
    size_t n;
    float *normals, *positions, *vis, *vis2;
    uint8_t *map, *mask, *counts;
    Frame(uint32_t w, uint32_t h, uint32_t planes_) : W(w), H(h), planes(planes_), n((size_t)w * h) {
        normals = block<float>(n * 4); positions = block<float>(n * 4);
        vis = block<float>(n * planes); vis2 = block<float>(n * planes);
        map = block<uint8_t>(n); mask = block<uint8_t>(n); counts = block<uint8_t>(n * planes);
        for (size_t i = 0; i < n * 4; ++i) { normals[i] = (next() % 7u) ? value() : 0.0f; positions[i] = value(); }
        for (size_t i = 0; i < n; ++i) {
            if (next() % 5u == 0) normals[i * 4] = normals[i * 4 + 1] = normals[i * 4 + 2] = 0.0f;   // background
            if (next() % 2u == 0) { normals[i * 4] = 0.0f; normals[i * 4 + 1] = 1.0f; normals[i * 4 + 2] = 0.0f; positions[i * 4 + 1] = 0.25f; }
            map[i] = (uint8_t)next(); mask[i] = (uint8_t)next();
        }
        for (size_t i = 0; i < n * planes; ++i) counts[i] = (uint8_t)next();
        reset();
    }
    void reset() { for (size_t i = 0; i < n * planes; ++i) vis[i] = vis2[i] = 7.5f; }
    bool untouched() const {
        for (size_t i = 0; i < n * planes; ++i) if (vis[i] != 7.5f) return false;
        return true;
    }
    ~Frame() { std::free(normals); std::free(positions); std::free(vis); std::free(vis2); std::free(map); std::free(mask); std::free(counts); }
};

static const uint32_t kSamples[8] = { 4, 16, 48, 1, 0, 4, 16, 48 };

static void lists(uint32_t count, rts_light_list* hard, rts_soft_light_list* soft) {
    std::memset(hard, 0, sizeof(*hard)); std::memset(soft, 0, sizeof(*soft));
    hard->count = soft->count = count;
    for (uint32_t l = 0; l < count; ++l) {
        const uint32_t type = (l & 1u) ? RTS_LIGHT_POINT : RTS_LIGHT_DIRECTIONAL;
        const float xyz[3] = { 0.6f - 0.3f * (float)l, 0.64f, 0.48f + (float)l };
        hard->lights[l].type = soft->lights[l].type = type;
        for (int i = 0; i < 3; ++i) hard->lights[l].xyz[i] = soft->lights[l].xyz[i] = xyz[i];
        soft->lights[l].nsamples = kSamples[l];
        soft->lights[l].first = kSamples[l] < 2 ? 0 : 48 - kSamples[l];
        soft->lights[l].radius = 0.25f;
    }
}

static rtsh_wide_filter_params params(uint32_t passes) {
    rtsh_wide_filter_params p;
    std::memset(&p, 0, sizeof(p));
    p.passes = passes; p.normal_cos_min = 0.5f; p.plane_eps = 10.0f;
    return p;
}

static bool background(const Frame& f, size_t i) { return f.normals[i * 4] == 0.0f && f.normals[i * 4 + 1] == 0.0f && f.normals[i * 4 + 2] == 0.0f; }

static void frames() {
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 2 }, { 17, 1 }, { 1, 5 }, { 9, 9 }, { 72, 72 } };
    for (const auto& wh : sizes) for (uint32_t count : { 1u, 4u, 8u }) {
        if (wh[0] == 72u && count == 4u) continue;
        Frame f(wh[0], wh[1], count);                                   // exactly `count` planes of everything
        rts_light_list hard; rts_soft_light_list soft;
        lists(count, &hard, &soft);
        for (uint32_t passes = 0; passes <= (uint32_t)RTSH_WIDE_FILTER_MAX_PASSES; ++passes) for (int withMap = 0; withMap < 2; ++withMap) {
            const rtsh_wide_filter_params p = params(passes);
            const uint8_t* map = withMap ? f.map : nullptr;
            CHECK(rtsh_wide_filter_soft_light_list(&soft, &p, f.positions, f.normals, map, f.counts, f.W, f.H, f.vis, 1), RTS_OK,
                  "soft %ux%u count %u passes %u", f.W, f.H, count, passes);
            CHECK(rtsh_wide_filter_soft_light_list(&soft, &p, f.positions, f.normals, map, f.counts, f.W, f.H, f.vis2, 3), RTS_OK, "soft, 3 threads");
            CHECK(std::memcmp(f.vis, f.vis2, f.n * count * 4), 0, "soft: threads change bits, %ux%u passes %u", f.W, f.H, passes);
            for (size_t i = 0; i < f.n; ++i) for (uint32_t l = 0; l < count; ++l) {
                const float v = f.vis[l * f.n + i];
                const bool on = !background(f, i) && (!map || ((map[i] >> l) & 1u));
                if (!on) { uint32_t u; std::memcpy(&u, &v, 4); CHECK(u, 0u, "inactive pixel %zu light %u of %ux%u", i, l, f.W, f.H); }
                else if (passes == 0) {
                    const uint32_t n = kSamples[l] > 1 ? kSamples[l] : 1u, c = f.counts[l * f.n + i] < n ? f.counts[l * f.n + i] : n;
                    const float want = (float)c / (float)n;
                    CHECK(std::memcmp(&v, &want, 4), 0, "passes 0 quotient, pixel %zu light %u", i, l);
                } else CHECK(v >= 0.0f && v <= 1.0f, true, "visibility out of range, pixel %zu light %u", i, l);
            }
            CHECK(rtsh_wide_filter_light_list(&hard, &p, f.positions, f.normals, map, f.mask, f.W, f.H, f.vis2, 2), RTS_OK, "hard %ux%u", f.W, f.H);
            for (size_t i = 0; i < f.n * count; ++i) CHECK(f.vis2[i] >= 0.0f && f.vis2[i] <= 1.0f, true, "hard visibility %zu", i);
        }
    }
}

static void refusals() {
    Frame f(5, 3, 8);
    rts_light_list hard; rts_soft_light_list soft;
    lists(3, &hard, &soft);
    const rtsh_wide_filter_params good = params(3);
#define REFUSED(call, what) do { CHECK(call, RTS_ERR_INVALID_ARG, what); CHECK(f.untouched(), true, what ": output written"); } while (0)
#define SOFT(list, p, pos, nrm, cnt, w, h, out) rtsh_wide_filter_soft_light_list(list, p, pos, nrm, f.map, cnt, w, h, out, 0)
#define HARD(list, p, pos, nrm, msk, w, h, out) rtsh_wide_filter_light_list(list, p, pos, nrm, f.map, msk, w, h, out, 0)
    REFUSED(SOFT(nullptr, &good, f.positions, f.normals, f.counts, f.W, f.H, f.vis), "soft: NULL list");
    REFUSED(HARD(nullptr, &good, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: NULL list");
    for (uint32_t count : { 0u, 9u, 0xFFFFFFFFu }) {
        rts_light_list h = hard; rts_soft_light_list s = soft;
        h.count = s.count = count;
        REFUSED(SOFT(&s, &good, f.positions, f.normals, f.counts, f.W, f.H, f.vis), "soft: count");
        REFUSED(HARD(&h, &good, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: count");
    }
    for (uint32_t l = 0; l < 3; ++l) {
        rts_light_list h = hard; rts_soft_light_list s = soft;
        h.lights[l].type = s.lights[l].type = 2;
        REFUSED(SOFT(&s, &good, f.positions, f.normals, f.counts, f.W, f.H, f.vis), "soft: type");
        REFUSED(HARD(&h, &good, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: type");
        s = soft; s.lights[l].nsamples = 49;
        REFUSED(SOFT(&s, &good, f.positions, f.normals, f.counts, f.W, f.H, f.vis), "soft: nsamples");
        s = soft; s.lights[l].radius = kNaN;
        REFUSED(SOFT(&s, &good, f.positions, f.normals, f.counts, f.W, f.H, f.vis), "soft: radius");
    }
    for (uint32_t passes : { 6u, 0xFFFFFFFFu }) {
        rtsh_wide_filter_params p = good; p.passes = passes;
        REFUSED(SOFT(&soft, &p, f.positions, f.normals, f.counts, f.W, f.H, f.vis), "soft: passes > 5");
        REFUSED(HARD(&hard, &p, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: passes > 5");
    }
    for (float v : { kNaN, kInf, -kInf }) {
        rtsh_wide_filter_params p = good; p.normal_cos_min = v;
        REFUSED(SOFT(&soft, &p, f.positions, f.normals, f.counts, f.W, f.H, f.vis), "soft: normal_cos_min");
        REFUSED(HARD(&hard, &p, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: normal_cos_min");
        p = good; p.plane_eps = v;
        REFUSED(SOFT(&soft, &p, f.positions, f.normals, f.counts, f.W, f.H, f.vis), "soft: plane_eps");
        REFUSED(HARD(&hard, &p, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: plane_eps");
    }
    REFUSED(SOFT(&soft, nullptr, f.positions, f.normals, f.counts, f.W, f.H, f.vis), "soft: NULL params");
    REFUSED(SOFT(&soft, &good, nullptr, f.normals, f.counts, f.W, f.H, f.vis), "soft: NULL positions");
    REFUSED(SOFT(&soft, &good, f.positions, nullptr, f.counts, f.W, f.H, f.vis), "soft: NULL normals");
    REFUSED(SOFT(&soft, &good, f.positions, f.normals, nullptr, f.W, f.H, f.vis), "soft: NULL counts");
    REFUSED(SOFT(&soft, &good, f.positions, f.normals, f.counts, 0, f.H, f.vis), "soft: W 0");
    REFUSED(SOFT(&soft, &good, f.positions, f.normals, f.counts, f.W, 0, f.vis), "soft: H 0");
    REFUSED(SOFT(&soft, &good, f.positions, f.normals, f.counts, 0x7FFFFFF1u, 1, f.vis), "soft: W too large");
    CHECK(SOFT(&soft, &good, f.positions, f.normals, f.counts, f.W, f.H, nullptr), RTS_ERR_INVALID_ARG, "soft: NULL visibility");
    REFUSED(HARD(&hard, nullptr, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: NULL params");
    REFUSED(HARD(&hard, &good, nullptr, f.normals, f.mask, f.W, f.H, f.vis), "hard: NULL positions");
    REFUSED(HARD(&hard, &good, f.positions, nullptr, f.mask, f.W, f.H, f.vis), "hard: NULL normals");
    REFUSED(HARD(&hard, &good, f.positions, f.normals, nullptr, f.W, f.H, f.vis), "hard: NULL mask");
    REFUSED(HARD(&hard, &good, f.positions, f.normals, f.mask, 0, f.H, f.vis), "hard: W 0");
    REFUSED(HARD(&hard, &good, f.positions, f.normals, f.mask, f.W, 0, f.vis), "hard: H 0");
    REFUSED(HARD(&hard, &good, f.positions, f.normals, f.mask, 1, 0x7FFFFFF1u, f.vis), "hard: H too large");
    CHECK(HARD(&hard, &good, f.positions, f.normals, f.mask, f.W, f.H, nullptr), RTS_ERR_INVALID_ARG, "hard: NULL visibility");
    CHECK(rtsh_wide_filter_scratch_bytes(3, 5, 3), (size_t)(2 * 3 * 15 * 2), "scratch bytes");
#undef REFUSED
#undef SOFT
#undef HARD
}

int main() {
    refusals();
    frames();
    std::printf("ok %lu\n", cases);
    return 0;
}
