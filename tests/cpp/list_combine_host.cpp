// Host-only check of the combine pass of a light list (tests/test_list_combine_host.py, built with -fsanitize=address,undefined,
// float-cast-overflow together with raytracedshadows_amd/csrc/rts_scene.cpp): rtsh_combine_light_list and rtsh_combine_soft_light_list
// over every refusal of include/rts_scene.h and over frames of 1, 3, 4, 5 and 257 pixels whose buffers are heap blocks of exactly the
// stated size -- normals and positions 16 bytes per pixel, the map and the hard mask 1, `count` planes of W*H bytes, rgb 3 -- so that a
// read of a plane from the count up, of a byte behind a frame or a write behind rgb is reported.  The sanitizers are the first check;
// the second is the anchor (a list of one white light gives rtsh_combine's bytes) and the refusals leaving rgb as it was.
// Prints the first case that differs and exits 1; "ok <cases>" otherwise.
#include "../../include/rts_scene.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

// rts_scene.cpp's traces validate their stream through the library proper; the combine passes never get there
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
    float *normals, *positions;
    uint8_t *map, *mask, *counts, *rgb, *rgb2;
    Frame(uint32_t w, uint32_t h, uint32_t planes) : W(w), H(h), n((size_t)w * h) {
        normals = block<float>(n * 4); positions = block<float>(n * 4);
        map = block<uint8_t>(n); mask = block<uint8_t>(n); counts = block<uint8_t>(n * planes);
        rgb = block<uint8_t>(n * 3); rgb2 = block<uint8_t>(n * 3);
        for (size_t i = 0; i < n * 4; ++i) { normals[i] = (next() % 7u) ? value() : 0.0f; positions[i] = value(); }
        for (size_t i = 0; i < n; ++i) {
            if (next() % 5u == 0) normals[i * 4] = normals[i * 4 + 1] = normals[i * 4 + 2] = 0.0f;   // background
            map[i] = (uint8_t)next(); mask[i] = (uint8_t)next();
        }
        for (size_t i = 0; i < n * planes; ++i) counts[i] = (uint8_t)next();
        std::memset(rgb, 0xAB, n * 3); std::memset(rgb2, 0xAB, n * 3);
    }
    ~Frame() { std::free(normals); std::free(positions); std::free(map); std::free(mask); std::free(counts); std::free(rgb); std::free(rgb2); }
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

static void lists(uint32_t count, bool points, rts_light_list* hard, rts_soft_light_list* soft) {
    std::memset(hard, 0, sizeof(*hard)); std::memset(soft, 0, sizeof(*soft));
    hard->count = soft->count = count;
    for (uint32_t l = 0; l < count; ++l) {
        const uint32_t type = (points && (l & 1u)) ? RTS_LIGHT_POINT : RTS_LIGHT_DIRECTIONAL;
        const float xyz[3] = { 0.6f - 0.3f * (float)l, 0.64f, 0.48f + (float)l };
        hard->lights[l].type = soft->lights[l].type = type;
        for (int i = 0; i < 3; ++i) hard->lights[l].xyz[i] = soft->lights[l].xyz[i] = xyz[i];
        soft->lights[l].nsamples = kSamples[l];
        soft->lights[l].first = kSamples[l] < 2 ? 0 : 48 - kSamples[l];
        soft->lights[l].radius = 0.25f;
    }
}

static bool untouched(const uint8_t* rgb, size_t bytes) {
    for (size_t i = 0; i < bytes; ++i) if (rgb[i] != 0xAB) return false;
    return true;
}

static void frames() {
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 1 }, { 1, 3 }, { 2, 2 }, { 4, 1 }, { 5, 1 }, { 1, 257 }, { 257, 1 } };
    const rts_constants k = constants();
    for (const auto& wh : sizes) for (uint32_t count = 1; count <= 8; ++count) for (int points = 0; points < 2; ++points) {
        Frame f(wh[0], wh[1], count);                                   // exactly `count` planes
        rts_light_list hard; rts_soft_light_list soft;
        lists(count, points != 0, &hard, &soft);
        float* colors = block<float>((size_t)count * 4);                // exactly count * 4 floats
        for (uint32_t i = 0; i < count * 4; ++i) colors[i] = value();
        for (int withMap = 0; withMap < 2; ++withMap) for (int withColors = 0; withColors < 2; ++withColors) {
            const float* pos = (points || withMap) ? f.positions : nullptr;      // NULL positions where no light is a point light
            CHECK(rtsh_combine_light_list(&k, &hard, withColors ? colors : nullptr, pos, f.normals, withMap ? f.map : nullptr, f.mask, f.W, f.H,
                                          f.rgb), RTS_OK, "hard %ux%u count %u", f.W, f.H, count);
            CHECK(rtsh_combine_soft_light_list(&k, &soft, withColors ? colors : nullptr, pos, f.normals, withMap ? f.map : nullptr, f.counts, f.W,
                                               f.H, f.rgb2), RTS_OK, "soft %ux%u count %u", f.W, f.H, count);
            for (size_t i = 0; i < f.n; ++i) {
                const float* n4 = f.normals + i * 4;
                if (n4[0] == 0.0f && n4[1] == 0.0f && n4[2] == 0.0f) {
                    CHECK(f.rgb[i * 3] | f.rgb[i * 3 + 1] | f.rgb[i * 3 + 2] | f.rgb2[i * 3] | f.rgb2[i * 3 + 1] | f.rgb2[i * 3 + 2], 0,
                          "background pixel %zu of %ux%u", i, f.W, f.H);
                }
            }
        }
        // the anchor: light 0 alone, white, no map -- rtsh_combine over plane 0 (soft) and over bit 0 (hard)
        rts_light one;
        std::memset(&one, 0, sizeof(one));
        one.type = soft.lights[0].type; one.nsamples = soft.lights[0].nsamples;
        for (int i = 0; i < 3; ++i) one.xyz[i] = soft.lights[0].xyz[i];
        rts_light_list hard1 = hard; rts_soft_light_list soft1 = soft;
        hard1.count = soft1.count = 1;
        uint8_t* bit0 = block<uint8_t>(f.n);
        uint8_t* want = block<uint8_t>(f.n * 3);
        for (size_t i = 0; i < f.n; ++i) bit0[i] = f.mask[i] & 1u;
        CHECK(rtsh_combine(&k, &one, f.positions, f.normals, f.counts, f.W, f.H, want), RTS_OK, "rtsh_combine");
        CHECK(rtsh_combine_soft_light_list(&k, &soft1, nullptr, f.positions, f.normals, nullptr, f.counts, f.W, f.H, f.rgb2), RTS_OK, "soft anchor");
        CHECK(std::memcmp(want, f.rgb2, f.n * 3), 0, "soft anchor bytes, %ux%u", f.W, f.H);
        one.nsamples = 1;
        CHECK(rtsh_combine(&k, &one, f.positions, f.normals, bit0, f.W, f.H, want), RTS_OK, "rtsh_combine");
        CHECK(rtsh_combine_light_list(&k, &hard1, nullptr, f.positions, f.normals, nullptr, f.mask, f.W, f.H, f.rgb), RTS_OK, "hard anchor");
        CHECK(std::memcmp(want, f.rgb, f.n * 3), 0, "hard anchor bytes, %ux%u", f.W, f.H);
        std::free(bit0); std::free(want); std::free(colors);
    }
}

static void refusals() {
    const rts_constants k = constants();
    Frame f(5, 3, 8);
    rts_light_list hard; rts_soft_light_list soft;
    lists(3, true, &hard, &soft);
    const size_t bytes = f.n * 3;
#define REFUSED(call, what) do { CHECK(call, RTS_ERR_INVALID_ARG, what); CHECK(untouched(f.rgb, bytes), true, what ": rgb written"); } while (0)
    // the list's own rules
    REFUSED(rtsh_combine_light_list(&k, nullptr, nullptr, f.positions, f.normals, f.map, f.mask, f.W, f.H, f.rgb), "hard: NULL list");
    REFUSED(rtsh_combine_soft_light_list(&k, nullptr, nullptr, f.positions, f.normals, f.map, f.counts, f.W, f.H, f.rgb), "soft: NULL list");
    for (uint32_t count : { 0u, 9u, 0xFFFFFFFFu }) {
        rts_light_list h = hard; rts_soft_light_list s = soft;
        h.count = s.count = count;
        REFUSED(rtsh_combine_light_list(&k, &h, nullptr, f.positions, f.normals, f.map, f.mask, f.W, f.H, f.rgb), "hard: count");
        REFUSED(rtsh_combine_soft_light_list(&k, &s, nullptr, f.positions, f.normals, f.map, f.counts, f.W, f.H, f.rgb), "soft: count");
    }
    for (uint32_t l = 0; l < 3; ++l) {
        rts_light_list h = hard; rts_soft_light_list s = soft;
        h.lights[l].type = s.lights[l].type = 2;
        REFUSED(rtsh_combine_light_list(&k, &h, nullptr, f.positions, f.normals, f.map, f.mask, f.W, f.H, f.rgb), "hard: type");
        REFUSED(rtsh_combine_soft_light_list(&k, &s, nullptr, f.positions, f.normals, f.map, f.counts, f.W, f.H, f.rgb), "soft: type");
        s = soft; s.lights[l].nsamples = 49;
        REFUSED(rtsh_combine_soft_light_list(&k, &s, nullptr, f.positions, f.normals, f.map, f.counts, f.W, f.H, f.rgb), "soft: nsamples");
        s = soft; s.lights[l].nsamples = 16; s.lights[l].first = 33;
        REFUSED(rtsh_combine_soft_light_list(&k, &s, nullptr, f.positions, f.normals, f.map, f.counts, f.W, f.H, f.rgb), "soft: first");
        for (float r : { kInf, -kInf, kNaN }) {
            s = soft; s.lights[l].radius = r;
            REFUSED(rtsh_combine_soft_light_list(&k, &s, nullptr, f.positions, f.normals, f.map, f.counts, f.W, f.H, f.rgb), "soft: radius");
        }
    }
    // the pointers and the frame
    REFUSED(rtsh_combine_light_list(nullptr, &hard, nullptr, f.positions, f.normals, f.map, f.mask, f.W, f.H, f.rgb), "hard: NULL constants");
    REFUSED(rtsh_combine_light_list(&k, &hard, nullptr, f.positions, nullptr, f.map, f.mask, f.W, f.H, f.rgb), "hard: NULL normals");
    REFUSED(rtsh_combine_light_list(&k, &hard, nullptr, f.positions, f.normals, f.map, nullptr, f.W, f.H, f.rgb), "hard: NULL mask");
    REFUSED(rtsh_combine_light_list(&k, &hard, nullptr, nullptr, f.normals, f.map, f.mask, f.W, f.H, f.rgb), "hard: a point light, no positions");
    REFUSED(rtsh_combine_light_list(&k, &hard, nullptr, f.positions, f.normals, f.map, f.mask, 0, f.H, f.rgb), "hard: W 0");
    REFUSED(rtsh_combine_light_list(&k, &hard, nullptr, f.positions, f.normals, f.map, f.mask, f.W, 0, f.rgb), "hard: H 0");
    CHECK(rtsh_combine_light_list(&k, &hard, nullptr, f.positions, f.normals, f.map, f.mask, f.W, f.H, nullptr), RTS_ERR_INVALID_ARG, "hard: NULL rgb");
    REFUSED(rtsh_combine_soft_light_list(nullptr, &soft, nullptr, f.positions, f.normals, f.map, f.counts, f.W, f.H, f.rgb), "soft: NULL constants");
    REFUSED(rtsh_combine_soft_light_list(&k, &soft, nullptr, f.positions, nullptr, f.map, f.counts, f.W, f.H, f.rgb), "soft: NULL normals");
    REFUSED(rtsh_combine_soft_light_list(&k, &soft, nullptr, f.positions, f.normals, f.map, nullptr, f.W, f.H, f.rgb), "soft: NULL counts");
    REFUSED(rtsh_combine_soft_light_list(&k, &soft, nullptr, nullptr, f.normals, f.map, f.counts, f.W, f.H, f.rgb), "soft: a point light, no positions");
    REFUSED(rtsh_combine_soft_light_list(&k, &soft, nullptr, f.positions, f.normals, f.map, f.counts, 0, f.H, f.rgb), "soft: W 0");
    REFUSED(rtsh_combine_soft_light_list(&k, &soft, nullptr, f.positions, f.normals, f.map, f.counts, f.W, 0, f.rgb), "soft: H 0");
    CHECK(rtsh_combine_soft_light_list(&k, &soft, nullptr, f.positions, f.normals, f.map, f.counts, f.W, f.H, nullptr), RTS_ERR_INVALID_ARG, "soft: NULL rgb");
#undef REFUSED
}

int main() {
    refusals();
    frames();
    std::printf("ok %lu\n", cases);
    return 0;
}
