// Host-only check of adaptive ambient occlusion on the host (tests/test_ao_adaptive_host.py, built with -fsanitize=address,undefined
// together with raytracedshadows_amd/csrc/rts_scene.cpp): rtsh_ambient_occlusion_adaptive over frames of 1 x 1, 8 x 8, 17 x 5 and 33 x 9
// above tests/cpp/ao_host.cpp's hand-made stream (a ground quad of two triangles under a small roof triangle), with background pixels,
// an active map, NaN positions wherever no ray may start, (n, probe) of (2, 1), (3, 1), (4, 3), (5, 4), (16, 4), (48, 47) and (48, 1)
// and tables 0, n and 64.  Positions, normals, map, counts and refined are heap blocks of exactly the stated size, so an index outside
// the frame or a write to a row outside the range is a sanitizer report.  The sanitizers are the first check.  The second: the
// definition against rtsh_ambient_occlusion's planes of n and of probe samples (same table, so the same idx); refined = NULL gives the
// same counts; a row range against the whole frame, rows outside it untouched; every refusal with nothing written.  Prints the first
// case that differs and exits 1; "ok <cases>" otherwise.
#include "../../include/rts_scene.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

extern "C" int rts_bvh_validate(const rts_vec4u*, size_t, uint32_t*) { return RTS_OK; }   // (the stream below is made by hand)

static unsigned long cases = 0;
#define CHECK(cond, ...) \
    do { ++cases; if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

template <class T> static T* block(size_t n) { return (T*)std::malloc((n ? n : 1) * sizeof(T)); }
static uint32_t bitsOf(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// The stream: node i = vec4 2i, 2i + 1.  Inner: {bboxMin, 0xFFFFFFFF}, {bboxMax, miss link}; a hit goes on to
// node i + 1.  Leaf: {e0, vec4 index of v0}, {e1, miss link}; then the v0 records.  Root, three leaves.
static const uint32_t END = 0xFFFFFFFFu;
static rts_vec4u* makeStream(size_t* count) {
    const float tris[3][3][3] = { { { -50, 0, -50 }, { 50, 0, -50 }, { 50, 0, 50 } }, { { -50, 0, -50 }, { 50, 0, 50 }, { -50, 0, 50 } },
                                  { { -1, 0.5f, -1 }, { 3, 0.5f, -1 }, { -1, 0.5f, 3 } } };   // the roof: over the pixels around the origin
    *count = 8 + 3;
    rts_vec4u* s = block<rts_vec4u>(*count);
    uint32_t* w = (uint32_t*)s;
    const float lo[3] = { -50, 0, -50 }, hi[3] = { 50, 0.5f, 50 };
    for (int c = 0; c < 3; ++c) { w[c] = bitsOf(lo[c]); w[4 + c] = bitsOf(hi[c]); }
    w[3] = END; w[7] = END;
    for (uint32_t t = 0; t < 3; ++t) {
        uint32_t* a = w + (1 + t) * 8;
        for (int c = 0; c < 3; ++c) {
            a[c] = bitsOf(tris[t][1][c] - tris[t][0][c]);
            a[4 + c] = bitsOf(tris[t][2][c] - tris[t][0][c]);
            w[(8 + t) * 4 + c] = bitsOf(tris[t][0][c]);
        }
        a[3] = 8 + t;
        a[7] = t == 2 ? END : 2 + t;
        w[(8 + t) * 4 + 3] = 0;
    }
    return s;
}

static unsigned long sawFull = 0, sawRefined = 0, sawZero = 0;

static void frame(const rts_vec4u* stream, size_t count, uint32_t W, uint32_t H, uint32_t n, uint32_t probe, uint32_t table, bool masked) {
    const size_t px = (size_t)W * H;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    float* pos = block<float>(px * 4);
    float* nrm = block<float>(px * 4);
    uint8_t* act = masked ? block<uint8_t>(px) : nullptr;
    bool* live = block<bool>(px);
    rts_constants k;
    std::memset(&k, 0, sizeof(k));
    k.cameraPosition[1] = 4.0f;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const bool background = (x * 5u + y * 11u) % 13u == 7u;
            const bool on = !masked || ((x >> 3) + (y >> 3)) % 2u == 0u || (x + 3u * y) % 5u == 0u;
            if (act) act[i] = on ? (uint8_t)(1u + i % 200u) : 0;
            live[i] = !background && on;
            const float nz = (i % 4u == 0u) ? 0.0f : (i % 4u == 1u) ? -0.0f : 0.28f;      // N.z of +0, -0, and a tilted normal
            const float ny = nz == 0.28f ? 0.96f : 1.0f;
            nrm[i * 4] = 0; nrm[i * 4 + 1] = background ? 0 : ny; nrm[i * 4 + 2] = background ? 0 : nz; nrm[i * 4 + 3] = nan;
            pos[i * 4] = live[i] ? ((float)x - (float)W * 0.5f) * 0.25f : nan;
            pos[i * 4 + 1] = live[i] ? -4.0f : nan;                       // the plane y = 0
            pos[i * 4 + 2] = live[i] ? ((float)y - (float)H * 0.5f) * 0.25f : nan;
            pos[i * 4 + 3] = nan;
        }
    rts_ao_params ao;
    std::memset(&ao, 0, sizeof(ao));
    ao.nsamples = n; ao.table = table; ao.radius = 1.5f;
    uint32_t seed = W * 131u + H * 7u + n;
    for (uint32_t j = 0; j < 64; ++j)
        for (int c = 0; c < 3; ++c) {
            seed = seed * 1664525u + 1013904223u;
            ao.dirs[j][c] = (float)(seed >> 8) / 8388608.0f - (c == 2 ? 0.0f : 1.0f);   // x, y in [-1, 1), z in [0, 2)
        }
    uint8_t* whole = block<uint8_t>(px);
    uint8_t* refined = block<uint8_t>(px);
    std::memset(whole, 0xAB, px); std::memset(refined, 0xAB, px);
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &ao, pos, nrm, act, W, H, 0, H, probe, whole, refined, 2) == RTS_OK,
          "%ux%u n %u probe %u: the whole frame", W, H, n, probe);
    // the definition from the AO twin's planes: c_n with n samples, c_k with `probe` samples of the same table (where that is legal)
    uint8_t* cn = block<uint8_t>(px);
    uint8_t* ck = block<uint8_t>(px);
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &ao, pos, nrm, act, W, H, 0, H, cn, 1) == RTS_OK, "the full plane");
    rts_ao_params aok = ao;
    aok.nsamples = probe;
    const bool haveCk = !(table && probe < 2);
    if (haveCk) CHECK(rtsh_ambient_occlusion(stream, count, &k, &aok, pos, nrm, act, W, H, 0, H, ck, 1) == RTS_OK, "the probe's plane");
    for (size_t i = 0; i < px; ++i) {
        CHECK(refined[i] <= 1 && (live[i] || (whole[i] == 0 && refined[i] == 0)), "%ux%u n %u probe %u: dead pixel %zu", W, H, n, probe, i);
        if (refined[i]) CHECK(whole[i] == cn[i], "%ux%u n %u probe %u table %u: refined pixel %zu has %u, not %u", W, H, n, probe, table, i, whole[i], cn[i]);
        else CHECK(whole[i] == 0 || whole[i] == n, "%ux%u n %u probe %u: verdict %u at %zu", W, H, n, probe, whole[i], i);
        if (haveCk && live[i]) {
            const bool pen = ck[i] != 0 && ck[i] != probe;
            CHECK(refined[i] == (pen ? 1 : 0) && (pen || whole[i] == (ck[i] ? n : 0)), "%ux%u n %u probe %u table %u: pixel %zu c_k %u -> %u, %u",
                  W, H, n, probe, table, i, ck[i], whole[i], refined[i]);
        }
        if (live[i]) { sawRefined += refined[i]; sawFull += !refined[i] && whole[i] == n; sawZero += !refined[i] && whole[i] == 0; }
    }
    // refined = NULL: the same counts
    uint8_t* alone = block<uint8_t>(px);
    std::memset(alone, 0xAB, px);
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &ao, pos, nrm, act, W, H, 0, H, probe, alone, nullptr, 1) == RTS_OK, "refined NULL");
    CHECK(std::memcmp(alone, whole, px) == 0, "%ux%u n %u probe %u: refined = NULL changes the counts", W, H, n, probe);
    // a row range: the same bytes inside, the fill outside
    const uint32_t r0 = H / 3, r1 = H - H / 4;
    uint8_t* part = block<uint8_t>(px);
    uint8_t* partRefined = block<uint8_t>(px);
    std::memset(part, 0xAB, px); std::memset(partRefined, 0xAB, px);
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &ao, pos, nrm, act, W, H, r0, r1, probe, part, partRefined, 1) == RTS_OK, "%ux%u: rows", W, H);
    for (size_t i = 0; i < px; ++i) {
        const uint32_t y = (uint32_t)(i / W);
        const bool in = y >= r0 && y < r1;
        CHECK(part[i] == (in ? whole[i] : 0xAB) && partRefined[i] == (in ? refined[i] : 0xAB), "%ux%u n %u rows %u..%u: byte %zu", W, H, n, r0, r1, i);
    }
    std::free(partRefined); std::free(part); std::free(alone); std::free(ck); std::free(cn); std::free(refined); std::free(whole);
    std::free(live); std::free(act); std::free(nrm); std::free(pos);
}

static void refusals(const rts_vec4u* stream, size_t count) {
    const uint32_t W = 5, H = 3;
    float* pos = block<float>(W * H * 4);
    float* nrm = block<float>(W * H * 4);
    for (uint32_t i = 0; i < W * H * 4; ++i) { pos[i] = i % 4 == 1 ? -4.0f : 0.25f * (float)(i % 7); nrm[i] = i % 4 == 1 ? 1.0f : 0.0f; }
    uint8_t* counts = block<uint8_t>(W * H);
    uint8_t* refined = block<uint8_t>(W * H);
    std::memset(counts, 0xAB, W * H); std::memset(refined, 0xAB, W * H);
    rts_constants k;
    std::memset(&k, 0, sizeof(k));
    rts_ao_params good;
    std::memset(&good, 0, sizeof(good));
    good.nsamples = 4; good.radius = 1.0f;
    for (int j = 0; j < 64; ++j) good.dirs[j][2] = 1.0f;
    const float inf = std::numeric_limits<float>::infinity();
    rts_ao_params bad[9] = { good, good, good, good, good, good, good, good, good };
    bad[0].nsamples = 49; bad[1].table = 3; bad[2].table = 65; bad[3].nsamples = 1; bad[3].table = 2; bad[4].radius = inf;
    bad[5].radius = -inf; bad[6].radius = std::numeric_limits<float>::quiet_NaN(); bad[7].nsamples = 1; bad[8].nsamples = 0;
    const int E = RTS_ERR_INVALID_ARG;
    for (const rts_ao_params& b : bad)
        CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &b, pos, nrm, nullptr, W, H, 0, H, 1, counts, refined, 1) == E, "bad params accepted");
    for (uint32_t probe : { 0u, 4u, 5u, 0xFFFFFFFFu })
        CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &good, pos, nrm, nullptr, W, H, 0, H, probe, counts, refined, 1) == E, "probe %u accepted", probe);
    CHECK(rtsh_ambient_occlusion_adaptive(nullptr, count, &k, &good, pos, nrm, nullptr, W, H, 0, H, 2, counts, refined, 1) == E, "no stream");
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, nullptr, &good, pos, nrm, nullptr, W, H, 0, H, 2, counts, refined, 1) == E, "no constants");
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, nullptr, pos, nrm, nullptr, W, H, 0, H, 2, counts, refined, 1) == E, "no params");
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &good, nullptr, nrm, nullptr, W, H, 0, H, 2, counts, refined, 1) == E, "no positions");
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &good, pos, nullptr, nullptr, W, H, 0, H, 2, counts, refined, 1) == E, "no normals");
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &good, pos, nrm, nullptr, W, H, 0, H, 2, nullptr, refined, 1) == E, "no counts");
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &good, pos, nrm, nullptr, 0, H, 0, H, 2, counts, refined, 1) == E, "W 0");
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &good, pos, nrm, nullptr, W, H, 2, 1, 2, counts, refined, 1) == E, "rows reversed");
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &good, pos, nrm, nullptr, W, H, 0, H + 1, 2, counts, refined, 1) == E, "rows past H");
    for (uint32_t i = 0; i < W * H; ++i) CHECK(counts[i] == 0xAB && refined[i] == 0xAB, "a refusal wrote byte %u", i);
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &good, pos, nrm, nullptr, W, H, 1, 1, 2, counts, refined, 1) == RTS_OK && counts[0] == 0xAB,
          "an empty range");
    CHECK(rtsh_ambient_occlusion_adaptive(stream, count, &k, &good, pos, nrm, nullptr, W, H, 0, H, 2, counts, refined, 1) == RTS_OK &&
          counts[W * H - 1] <= 4 && refined[W * H - 1] <= 1, "the good call");
    std::free(refined); std::free(counts); std::free(nrm); std::free(pos);
}

int main() {
    size_t count = 0;
    rts_vec4u* stream = makeStream(&count);
    const uint32_t frames[4][2] = { { 1, 1 }, { 8, 8 }, { 17, 5 }, { 33, 9 } };
    const uint32_t pairs[7][2] = { { 2, 1 }, { 3, 1 }, { 4, 3 }, { 5, 4 }, { 16, 4 }, { 48, 47 }, { 48, 1 } };
    for (const auto& f : frames)
        for (const auto& nk : pairs)
            for (uint32_t table : { 0u, nk[0], 64u }) {
                frame(stream, count, f[0], f[1], nk[0], nk[1], table, false);
                frame(stream, count, f[0], f[1], nk[0], nk[1], table, true);
            }
    CHECK(sawFull > 0 && sawRefined > 0 && sawZero > 0, "a branch of the decision was never taken (%lu, %lu, %lu)", sawFull, sawRefined, sawZero);
    refusals(stream, count);
    std::free(stream);
    std::printf("ok %lu\n", cases);
    return 0;
}
