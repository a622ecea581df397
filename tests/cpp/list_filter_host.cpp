// Host-only check of the filter of a light list's planes and of the visibility combine (tests/test_list_filter_host.py, built with
// -fsanitize=address,undefined,float-cast-overflow together with raytracedshadows_amd/csrc/rts_scene.cpp): rtsh_filter_light_list,
// rtsh_filter_soft_light_list and rtsh_combine_visibility_list over every refusal of include/rts_scene.h and over small frames of
// awkward texels (NaN, Inf, huge, denormal normals, positions and distances; arbitrary bytes) whose buffers are heap blocks of exactly
// the stated size -- normals and positions 16 bytes per pixel, the map and the hard mask 1, `count` planes of counts, distances and
// visibility -- so that a read of a plane from the count up, of a texel outside the frame or a write behind visibility is reported.
// The sanitizers are the first check; the second: R = 0 gives (float)c / (float)n, one thread and three threads give the same bits,
// the visibility combine over an R = 0 filter gives the list combine's bytes, and the refusals leave the outputs as they were.
// Prints the first case that differs and exits 1; "ok <cases>" otherwise.
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
    float *normals, *positions, *distances, *vis, *vis2;
    uint8_t *map, *mask, *counts, *rgb, *rgb2;
    Frame(uint32_t w, uint32_t h, uint32_t planes_) : W(w), H(h), planes(planes_), n((size_t)w * h) {
        normals = block<float>(n * 4); positions = block<float>(n * 4);
        distances = block<float>(n * planes); vis = block<float>(n * planes); vis2 = block<float>(n * planes);
        map = block<uint8_t>(n); mask = block<uint8_t>(n); counts = block<uint8_t>(n * planes);
        rgb = block<uint8_t>(n * 3); rgb2 = block<uint8_t>(n * 3);
        for (size_t i = 0; i < n * 4; ++i) { normals[i] = (next() % 7u) ? value() : 0.0f; positions[i] = value(); }
        for (size_t i = 0; i < n; ++i) {
            if (next() % 5u == 0) normals[i * 4] = normals[i * 4 + 1] = normals[i * 4 + 2] = 0.0f;   // background
            if (next() % 3u == 0) { normals[i * 4] = 0.0f; normals[i * 4 + 1] = 1.0f; normals[i * 4 + 2] = 0.0f; positions[i * 4 + 1] = 0.25f; }
            map[i] = (uint8_t)next(); mask[i] = (uint8_t)next();
        }
        for (size_t i = 0; i < n * planes; ++i) { counts[i] = (uint8_t)next(); distances[i] = (next() & 1u) ? value() : kInf; }
        reset();
    }
    void reset() {
        for (size_t i = 0; i < n * planes; ++i) vis[i] = vis2[i] = 7.5f;
        std::memset(rgb, 0xAB, n * 3); std::memset(rgb2, 0xAB, n * 3);
    }
    bool untouched() const {
        for (size_t i = 0; i < n * planes; ++i) if (vis[i] != 7.5f) return false;
        for (size_t i = 0; i < n * 3; ++i) if (rgb[i] != 0xAB) return false;
        return true;
    }
    ~Frame() {
        std::free(normals); std::free(positions); std::free(distances); std::free(vis); std::free(vis2); std::free(map); std::free(mask);
        std::free(counts); std::free(rgb); std::free(rgb2);
    }
};

static rts_constants constants() {
    rts_constants k;
    std::memset(&k, 0, sizeof(k));
    k.cameraPosition[0] = 1; k.cameraPosition[1] = 2; k.cameraPosition[2] = 3;
    k.cameraDirection[2] = -1;
    k.lightDirection[1] = 1;
    return k;
}

static const uint32_t kSamples[8] = { 16, 2, 1, 48, 0, 16, 2, 3 };

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

static rtsh_filter_params params(uint32_t radius) {
    rtsh_filter_params p;
    std::memset(&p, 0, sizeof(p));
    p.radius = radius; p.normal_cos_min = 0.5f; p.plane_eps = 10.0f;
    const float spread[8] = { 0.5f, 0.0f, 3.0f, 1e30f, 1e-3f, 2.0f, 1.0f, 0.25f };
    for (int l = 0; l < 8; ++l) p.spread[l] = spread[l];
    return p;
}

static bool background(const Frame& f, size_t i) { return f.normals[i * 4] == 0.0f && f.normals[i * 4 + 1] == 0.0f && f.normals[i * 4 + 2] == 0.0f; }

static void frames() {
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 1 }, { 1, 3 }, { 2, 2 }, { 5, 4 }, { 19, 3 }, { 1, 41 }, { 9, 9 } };
    const rts_constants k = constants();
    for (const auto& wh : sizes) for (uint32_t count : { 1u, 3u, 8u }) {
        Frame f(wh[0], wh[1], count);                                   // exactly `count` planes of everything
        rts_light_list hard; rts_soft_light_list soft;
        lists(count, &hard, &soft);
        for (uint32_t radius : { 0u, 1u, 2u, 8u }) for (int withMap = 0; withMap < 2; ++withMap) for (int withDist = 0; withDist < 2; ++withDist) {
            const rtsh_filter_params p = params(radius);
            const uint8_t* map = withMap ? f.map : nullptr;
            const float* dist = withDist ? f.distances : nullptr;
            CHECK(rtsh_filter_soft_light_list(&soft, &p, f.positions, f.normals, map, f.counts, dist, f.W, f.H, f.vis, 1), RTS_OK,
                  "soft %ux%u count %u R %u", f.W, f.H, count, radius);
            CHECK(rtsh_filter_soft_light_list(&soft, &p, f.positions, f.normals, map, f.counts, dist, f.W, f.H, f.vis2, 3), RTS_OK, "soft, 3 threads");
            CHECK(std::memcmp(f.vis, f.vis2, f.n * count * 4), 0, "soft: threads change bits, %ux%u R %u", f.W, f.H, radius);
            for (size_t i = 0; i < f.n; ++i) for (uint32_t l = 0; l < count; ++l) {
                const float v = f.vis[l * f.n + i];
                const bool on = !background(f, i) && (!map || ((map[i] >> l) & 1u));
                if (!on) { uint32_t u; std::memcpy(&u, &v, 4); CHECK(u, 0u, "inactive pixel %zu light %u of %ux%u", i, l, f.W, f.H); }
                else if (radius == 0) {
                    const float want = (float)f.counts[l * f.n + i] / (float)(kSamples[l] > 1 ? kSamples[l] : 1u);
                    CHECK(std::memcmp(&v, &want, 4), 0, "R = 0 quotient, pixel %zu light %u", i, l);
                } else CHECK(v >= 0.0f && v <= 255.0f, true, "quotient out of range, pixel %zu light %u", i, l);
            }
            if (withDist) continue;
            CHECK(rtsh_filter_light_list(&hard, &p, f.positions, f.normals, map, f.mask, f.W, f.H, f.vis2, 2), RTS_OK, "hard %ux%u", f.W, f.H);
            for (size_t i = 0; i < f.n * count; ++i) CHECK(f.vis2[i] >= 0.0f && f.vis2[i] <= 1.0f, true, "hard quotient %zu", i);
            if (radius == 0) {                                          // the visibility combine over an R = 0 filter
                CHECK(rtsh_combine_visibility_list(&k, &hard, nullptr, f.positions, f.normals, map, f.vis, f.W, f.H, f.rgb), RTS_OK, "vis combine");
                CHECK(rtsh_combine_soft_light_list(&k, &soft, nullptr, f.positions, f.normals, map, f.counts, f.W, f.H, f.rgb2), RTS_OK, "soft combine");
                CHECK(std::memcmp(f.rgb, f.rgb2, f.n * 3), 0, "soft combine anchor, %ux%u count %u", f.W, f.H, count);
                CHECK(rtsh_combine_visibility_list(&k, &hard, nullptr, f.positions, f.normals, map, f.vis2, f.W, f.H, f.rgb), RTS_OK, "vis combine");
                CHECK(rtsh_combine_light_list(&k, &hard, nullptr, f.positions, f.normals, map, f.mask, f.W, f.H, f.rgb2), RTS_OK, "hard combine");
                CHECK(std::memcmp(f.rgb, f.rgb2, f.n * 3), 0, "hard combine anchor, %ux%u count %u", f.W, f.H, count);
            }
        }
        // any float as visibility: the distance planes hold NaN, Inf, huge and negative values
        CHECK(rtsh_combine_visibility_list(&k, &hard, nullptr, f.positions, f.normals, f.map, f.distances, f.W, f.H, f.rgb), RTS_OK, "wild visibility");
    }
}

static void refusals() {
    const rts_constants k = constants();
    Frame f(5, 3, 8);
    rts_light_list hard; rts_soft_light_list soft;
    lists(3, &hard, &soft);
    const rtsh_filter_params good = params(2);
#define REFUSED(call, what) do { CHECK(call, RTS_ERR_INVALID_ARG, what); CHECK(f.untouched(), true, what ": output written"); } while (0)
#define SOFT(list, p, pos, nrm, cnt, dist, w, h, out) rtsh_filter_soft_light_list(list, p, pos, nrm, f.map, cnt, dist, w, h, out, 0)
#define HARD(list, p, pos, nrm, msk, w, h, out) rtsh_filter_light_list(list, p, pos, nrm, f.map, msk, w, h, out, 0)
    REFUSED(SOFT(nullptr, &good, f.positions, f.normals, f.counts, f.distances, f.W, f.H, f.vis), "soft: NULL list");
    REFUSED(HARD(nullptr, &good, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: NULL list");
    for (uint32_t count : { 0u, 9u, 0xFFFFFFFFu }) {
        rts_light_list h = hard; rts_soft_light_list s = soft;
        h.count = s.count = count;
        REFUSED(SOFT(&s, &good, f.positions, f.normals, f.counts, f.distances, f.W, f.H, f.vis), "soft: count");
        REFUSED(HARD(&h, &good, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: count");
        REFUSED(rtsh_combine_visibility_list(&k, &h, nullptr, f.positions, f.normals, f.map, f.distances, f.W, f.H, f.rgb), "combine: count");
    }
    for (uint32_t l = 0; l < 3; ++l) {
        rts_light_list h = hard; rts_soft_light_list s = soft;
        h.lights[l].type = s.lights[l].type = 2;
        REFUSED(SOFT(&s, &good, f.positions, f.normals, f.counts, f.distances, f.W, f.H, f.vis), "soft: type");
        REFUSED(HARD(&h, &good, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: type");
        s = soft; s.lights[l].nsamples = 49;
        REFUSED(SOFT(&s, &good, f.positions, f.normals, f.counts, f.distances, f.W, f.H, f.vis), "soft: nsamples");
        s = soft; s.lights[l].radius = kNaN;
        REFUSED(SOFT(&s, &good, f.positions, f.normals, f.counts, f.distances, f.W, f.H, f.vis), "soft: radius");
        for (float v : { -1.0f, kNaN, kInf, -kInf }) {
            rtsh_filter_params p = good; p.spread[l] = v;
            REFUSED(SOFT(&soft, &p, f.positions, f.normals, f.counts, f.distances, f.W, f.H, f.vis), "soft: spread");
        }
    }
    for (uint32_t radius : { 9u, 0xFFFFFFFFu }) {
        rtsh_filter_params p = good; p.radius = radius;
        REFUSED(SOFT(&soft, &p, f.positions, f.normals, f.counts, f.distances, f.W, f.H, f.vis), "soft: radius > 8");
        REFUSED(HARD(&hard, &p, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: radius > 8");
    }
    for (float v : { kNaN, kInf, -kInf }) {
        rtsh_filter_params p = good; p.normal_cos_min = v;
        REFUSED(SOFT(&soft, &p, f.positions, f.normals, f.counts, nullptr, f.W, f.H, f.vis), "soft: normal_cos_min");
        REFUSED(HARD(&hard, &p, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: normal_cos_min");
        p = good; p.plane_eps = v;
        REFUSED(SOFT(&soft, &p, f.positions, f.normals, f.counts, nullptr, f.W, f.H, f.vis), "soft: plane_eps");
        REFUSED(HARD(&hard, &p, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: plane_eps");
    }
    REFUSED(SOFT(&soft, nullptr, f.positions, f.normals, f.counts, f.distances, f.W, f.H, f.vis), "soft: NULL params");
    REFUSED(SOFT(&soft, &good, nullptr, f.normals, f.counts, f.distances, f.W, f.H, f.vis), "soft: NULL positions");
    REFUSED(SOFT(&soft, &good, f.positions, nullptr, f.counts, f.distances, f.W, f.H, f.vis), "soft: NULL normals");
    REFUSED(SOFT(&soft, &good, f.positions, f.normals, nullptr, f.distances, f.W, f.H, f.vis), "soft: NULL counts");
    REFUSED(SOFT(&soft, &good, f.positions, f.normals, f.counts, f.distances, 0, f.H, f.vis), "soft: W 0");
    REFUSED(SOFT(&soft, &good, f.positions, f.normals, f.counts, f.distances, f.W, 0, f.vis), "soft: H 0");
    CHECK(SOFT(&soft, &good, f.positions, f.normals, f.counts, f.distances, f.W, f.H, nullptr), RTS_ERR_INVALID_ARG, "soft: NULL visibility");
    REFUSED(HARD(&hard, nullptr, f.positions, f.normals, f.mask, f.W, f.H, f.vis), "hard: NULL params");
    REFUSED(HARD(&hard, &good, nullptr, f.normals, f.mask, f.W, f.H, f.vis), "hard: NULL positions");
    REFUSED(HARD(&hard, &good, f.positions, nullptr, f.mask, f.W, f.H, f.vis), "hard: NULL normals");
    REFUSED(HARD(&hard, &good, f.positions, f.normals, nullptr, f.W, f.H, f.vis), "hard: NULL mask");
    REFUSED(HARD(&hard, &good, f.positions, f.normals, f.mask, 0, f.H, f.vis), "hard: W 0");
    REFUSED(HARD(&hard, &good, f.positions, f.normals, f.mask, f.W, 0, f.vis), "hard: H 0");
    CHECK(HARD(&hard, &good, f.positions, f.normals, f.mask, f.W, f.H, nullptr), RTS_ERR_INVALID_ARG, "hard: NULL visibility");
    REFUSED(rtsh_combine_visibility_list(nullptr, &hard, nullptr, f.positions, f.normals, f.map, f.distances, f.W, f.H, f.rgb), "combine: NULL constants");
    REFUSED(rtsh_combine_visibility_list(&k, &hard, nullptr, f.positions, nullptr, f.map, f.distances, f.W, f.H, f.rgb), "combine: NULL normals");
    REFUSED(rtsh_combine_visibility_list(&k, &hard, nullptr, f.positions, f.normals, f.map, nullptr, f.W, f.H, f.rgb), "combine: NULL visibility");
    REFUSED(rtsh_combine_visibility_list(&k, &hard, nullptr, nullptr, f.normals, f.map, f.distances, f.W, f.H, f.rgb), "combine: a point light, no positions");
    REFUSED(rtsh_combine_visibility_list(&k, &hard, nullptr, f.positions, f.normals, f.map, f.distances, 0, f.H, f.rgb), "combine: W 0");
    REFUSED(rtsh_combine_visibility_list(&k, &hard, nullptr, f.positions, f.normals, f.map, f.distances, f.W, 0, f.rgb), "combine: H 0");
    CHECK(rtsh_combine_visibility_list(&k, &hard, nullptr, f.positions, f.normals, f.map, f.distances, f.W, f.H, nullptr), RTS_ERR_INVALID_ARG, "combine: NULL rgb");
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
