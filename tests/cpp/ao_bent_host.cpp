// Host-only check of bent normals on the host (tests/test_ao_bent_host.py, built with -fsanitize=address,undefined together with
// raytracedshadows_amd/csrc/rts_scene.cpp): rtsh_ambient_occlusion_bent over frames of 1 x 1, 8 x 8, 17 x 5 and 33 x 9 above
// tests/cpp/ao_host.cpp's hand-made stream (a ground quad of two triangles under a small roof triangle), with background pixels, an
// active map, NaN positions wherever no ray may start, n of 1, 3, 4, 5, 16 and 48 and tables 0, n and 64; and
// rtsh_combine_visibility_list_ao_bent over a small frame.  Positions, normals, map, counts and bent are heap blocks of exactly the
// stated size, so an index outside the frame or a write to a row outside the range is a sanitizer report.  The sanitizers are the first
// check (the conversion of Q to an integer included).  The second: Q itself on the header's awkward values; counts equal
// rtsh_ambient_occlusion's plane, bent.w the count, inactive texels four +0; counts = NULL gives the same bent; a row range against the
// whole frame, rows outside it untouched; every refusal with nothing written; the combine's two anchors.  Prints the first case that
// differs and exits 1; "ok <cases>" otherwise.
#include "../../include/rts_scene.h"
#include "../../raytracedshadows_amd/csrc/rts_closest_hit.h"
#include <cmath>
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

static void quantise() {
    using rts_harness::aoQuantise;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float v[] = { nan, -nan, inf, -inf, 0.0f, -0.0f, 1.0f, -1.0f, 1.5f, -1.5f, 0x1p-15f, -0x1p-15f, 3 * 0x1p-15f, -3 * 0x1p-15f,
                        1e-40f, -1e-40f, 0x1p-14f, 0.5f, 5 * 0x1p-15f, 0.99999994f, 3e38f };
    const int32_t q[] = { 0, 0, 16384, -16384, 0, 0, 16384, -16384, 16384, -16384, 0, 0, 2, -2, 0, 0, 1, 8192, 2, 16384, 16384 };
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i)
        CHECK(aoQuantise(v[i]) == q[i], "Q(%g) = %d, not %d", (double)v[i], aoQuantise(v[i]), q[i]);
}

static unsigned long sawPartly = 0, sawFull = 0, sawZero = 0;

static void frame(const rts_vec4u* stream, size_t count, uint32_t W, uint32_t H, uint32_t n, uint32_t table, bool masked) {
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
            nrm[i * 4] = 0; nrm[i * 4 + 1] = background ? 0 : ny; nrm[i * 4 + 2] = background ? (i % 2u ? -0.0f : 0.0f) : nz; nrm[i * 4 + 3] = nan;
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
            ao.dirs[j][c] = (float)(seed >> 8) / 8388608.0f - (c == 2 ? 0.0f : 1.0f);   // x, y in [-1, 1), z in [0, 2): z clamps
        }
    uint8_t* counts = block<uint8_t>(px);
    float* bent = block<float>(px * 4);
    std::memset(counts, 0xAB, px); std::memset(bent, 0xAB, px * 16);
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &ao, pos, nrm, act, W, H, 0, H, counts, bent, 2) == RTS_OK, "%ux%u n %u: the whole frame", W, H, n);
    uint8_t* plain = block<uint8_t>(px);
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &ao, pos, nrm, act, W, H, 0, H, plain, 1) == RTS_OK, "the AO plane");
    const uint32_t ns = n ? n : 1u;
    for (size_t i = 0; i < px; ++i) {
        CHECK(counts[i] == plain[i], "%ux%u n %u table %u: count %zu is %u, not %u", W, H, n, table, i, counts[i], plain[i]);
        CHECK(bitsOf(bent[i * 4 + 3]) == bitsOf((float)counts[i]), "%ux%u n %u: bent.w at %zu", W, H, n, i);
        if (!live[i])
            CHECK(counts[i] == 0 && bitsOf(bent[i * 4]) == 0 && bitsOf(bent[i * 4 + 1]) == 0 && bitsOf(bent[i * 4 + 2]) == 0 && bitsOf(bent[i * 4 + 3]) == 0,
                  "%ux%u n %u: dead pixel %zu", W, H, n, i);
        else {
            const double len = std::sqrt((double)bent[i * 4] * bent[i * 4] + (double)bent[i * 4 + 1] * bent[i * 4 + 1] + (double)bent[i * 4 + 2] * bent[i * 4 + 2]);
            // |q| <= sqrt(3) per sample; the frame is orthonormal up to rounding
            CHECK(len <= 1.7321 * counts[i] + 1e-3 && (counts[i] != 0 || len == 0.0), "%ux%u n %u: pixel %zu has length %g with %u free", W, H, n, i, len, counts[i]);
            sawZero += counts[i] == 0; sawFull += counts[i] == ns; sawPartly += counts[i] != 0 && counts[i] != ns;
        }
    }
    // counts = NULL: the same bent
    float* alone = block<float>(px * 4);
    std::memset(alone, 0xAB, px * 16);
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &ao, pos, nrm, act, W, H, 0, H, nullptr, alone, 1) == RTS_OK, "counts NULL");
    CHECK(std::memcmp(alone, bent, px * 16) == 0, "%ux%u n %u: counts = NULL changes bent", W, H, n);
    // a row range: the same bits inside, the fill outside
    const uint32_t r0 = H / 3, r1 = H - H / 4;
    uint8_t* part = block<uint8_t>(px);
    float* partBent = block<float>(px * 4);
    std::memset(part, 0xAB, px); std::memset(partBent, 0xAB, px * 16);
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &ao, pos, nrm, act, W, H, r0, r1, part, partBent, 1) == RTS_OK, "%ux%u: rows", W, H);
    for (size_t i = 0; i < px; ++i) {
        const uint32_t y = (uint32_t)(i / W);
        const bool in = y >= r0 && y < r1;
        CHECK(part[i] == (in ? counts[i] : 0xAB), "%ux%u n %u rows %u..%u: byte %zu", W, H, n, r0, r1, i);
        for (int c = 0; c < 4; ++c)
            CHECK(bitsOf(partBent[i * 4 + c]) == (in ? bitsOf(bent[i * 4 + c]) : 0xABABABABu), "%ux%u n %u rows %u..%u: texel %zu", W, H, n, r0, r1, i);
    }
    std::free(partBent); std::free(part); std::free(alone); std::free(plain); std::free(bent); std::free(counts);
    std::free(live); std::free(act); std::free(nrm); std::free(pos);
}

static void refusals(const rts_vec4u* stream, size_t count) {
    const uint32_t W = 5, H = 3;
    float* pos = block<float>(W * H * 4);
    float* nrm = block<float>(W * H * 4);
    for (uint32_t i = 0; i < W * H * 4; ++i) { pos[i] = i % 4 == 1 ? -4.0f : 0.25f * (float)(i % 7); nrm[i] = i % 4 == 1 ? 1.0f : 0.0f; }
    uint8_t* counts = block<uint8_t>(W * H);
    float* bent = block<float>(W * H * 4);
    std::memset(counts, 0xAB, W * H); std::memset(bent, 0xAB, W * H * 16);
    rts_constants k;
    std::memset(&k, 0, sizeof(k));
    rts_ao_params good;
    std::memset(&good, 0, sizeof(good));
    good.nsamples = 4; good.radius = 1.0f;
    for (int j = 0; j < 64; ++j) good.dirs[j][2] = 1.0f;
    const float inf = std::numeric_limits<float>::infinity();
    rts_ao_params bad[7] = { good, good, good, good, good, good, good };
    bad[0].nsamples = 49; bad[1].table = 3; bad[2].table = 65; bad[3].nsamples = 1; bad[3].table = 2; bad[4].radius = inf;
    bad[5].radius = -inf; bad[6].radius = std::numeric_limits<float>::quiet_NaN();
    const int E = RTS_ERR_INVALID_ARG;
    for (const rts_ao_params& b : bad)
        CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &b, pos, nrm, nullptr, W, H, 0, H, counts, bent, 1) == E, "bad params accepted");
    CHECK(rtsh_ambient_occlusion_bent(nullptr, count, &k, &good, pos, nrm, nullptr, W, H, 0, H, counts, bent, 1) == E, "no stream");
    CHECK(rtsh_ambient_occlusion_bent(stream, count, nullptr, &good, pos, nrm, nullptr, W, H, 0, H, counts, bent, 1) == E, "no constants");
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, nullptr, pos, nrm, nullptr, W, H, 0, H, counts, bent, 1) == E, "no params");
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &good, nullptr, nrm, nullptr, W, H, 0, H, counts, bent, 1) == E, "no positions");
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &good, pos, nullptr, nullptr, W, H, 0, H, counts, bent, 1) == E, "no normals");
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &good, pos, nrm, nullptr, W, H, 0, H, counts, nullptr, 1) == E, "no bent");
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &good, pos, nrm, nullptr, 0, H, 0, H, counts, bent, 1) == E, "W 0");
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &good, pos, nrm, nullptr, W, H, 2, 1, counts, bent, 1) == E, "rows reversed");
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &good, pos, nrm, nullptr, W, H, 0, H + 1, counts, bent, 1) == E, "rows past H");
    for (uint32_t i = 0; i < W * H; ++i) CHECK(counts[i] == 0xAB && bitsOf(bent[i * 4 + (i & 3)]) == 0xABABABABu, "a refusal wrote pixel %u", i);
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &good, pos, nrm, nullptr, W, H, 1, 1, counts, bent, 1) == RTS_OK && counts[0] == 0xAB,
          "an empty range");
    // dirs (0, 0, 1) above an open quad at a flat normal: S = c * (0, 0, 16384), bent = c * N exactly
    CHECK(rtsh_ambient_occlusion_bent(stream, count, &k, &good, pos, nrm, nullptr, W, H, 0, H, counts, bent, 1) == RTS_OK, "the good call");
    for (uint32_t i = 0; i < W * H; ++i)
        CHECK(counts[i] <= 4 && bent[i * 4] == 0.0f && bent[i * 4 + 1] == (float)counts[i] && bent[i * 4 + 2] == 0.0f, "the good call: pixel %u", i);
    std::free(bent); std::free(counts); std::free(nrm); std::free(pos);
}

static void combine() {
    const uint32_t W = 7, H = 3, px = W * H;
    float* nrm = block<float>(px * 4);
    float* pos = block<float>(px * 4);
    float* vis = block<float>(px);
    float* ao = block<float>(px);
    float* bent = block<float>(px * 4);
    uint8_t* a = block<uint8_t>(px * 3);
    uint8_t* b = block<uint8_t>(px * 3);
    uint8_t* z = block<uint8_t>(px * 3);
    for (uint32_t i = 0; i < px; ++i) {
        const bool background = i % 5u == 2u;
        nrm[i * 4] = background ? 0.0f : 0.6f; nrm[i * 4 + 1] = background ? 0.0f : 0.8f; nrm[i * 4 + 2] = 0.0f; nrm[i * 4 + 3] = 0.0f;
        for (int c = 0; c < 4; ++c) pos[i * 4 + c] = 0.1f * (float)(i + c);
        vis[i] = (float)(i % 4u) / 3.0f; ao[i] = (float)(i % 7u) / 6.0f;
        bent[i * 4] = (float)i - 9.0f; bent[i * 4 + 1] = 3.0f - (float)(i % 6u); bent[i * 4 + 2] = (i % 3u) ? 0.5f : -2.0f; bent[i * 4 + 3] = 4.0f;
    }
    rts_constants k;
    std::memset(&k, 0, sizeof(k));
    k.cameraDirection[2] = -1.0f; k.lightDirection[1] = 1.0f;
    rts_light_list lst;
    std::memset(&lst, 0, sizeof(lst));
    lst.count = 1; lst.lights[0].type = RTS_LIGHT_DIRECTIONAL; lst.lights[0].xyz[1] = 1.0f;
    rtsh_sky_ambient white = { { 0, 1, 0 }, { 1, 1, 1 }, { 1, 1, 1 }, { 0, 0, 0 } };
    rtsh_sky_ambient sky = { { 0, 1, 0 }, { 0.25f, 0.5f, 1.0f }, { 0.5f, 0.25f, 0.125f }, { 0, 0, 0 } };
    CHECK(rtsh_combine_visibility_list_ao(&k, &lst, nullptr, pos, nrm, nullptr, vis, ao, W, H, a) == RTS_OK, "the AO combine");
    CHECK(rtsh_combine_visibility_list_ao_bent(&k, &lst, nullptr, pos, nrm, nullptr, vis, ao, bent, &white, W, H, b) == RTS_OK, "the bent combine");
    CHECK(std::memcmp(a, b, px * 3) == 0, "a white sky is not the AO combine");
    CHECK(rtsh_combine_visibility_list_ao_bent(&k, &lst, nullptr, pos, nrm, nullptr, vis, ao, bent, &sky, W, H, b) == RTS_OK, "a sky");
    CHECK(std::memcmp(a, b, px * 3) != 0, "the sky changes nothing");
    // an all-zero bent plane: h = 0.5 everywhere, the tint the mean of sky and ground -- the same bytes as a sky of that one colour
    std::memset(bent, 0, px * 16);
    rtsh_sky_ambient mean = sky;
    for (int c = 0; c < 3; ++c) mean.sky[c] = mean.ground[c] = sky.ground[c] + (sky.sky[c] - sky.ground[c]) * 0.5f;
    CHECK(rtsh_combine_visibility_list_ao_bent(&k, &lst, nullptr, pos, nrm, nullptr, vis, ao, bent, &sky, W, H, b) == RTS_OK, "zero bent");
    CHECK(rtsh_combine_visibility_list_ao_bent(&k, &lst, nullptr, pos, nrm, nullptr, vis, ao, bent, &mean, W, H, z) == RTS_OK, "the mean sky");
    CHECK(std::memcmp(z, b, px * 3) == 0, "an all-zero bent texel is not h = 0.5");
    std::memset(z, 0xAB, px * 3);
    const int E = RTS_ERR_INVALID_ARG;
    CHECK(rtsh_combine_visibility_list_ao_bent(&k, &lst, nullptr, pos, nrm, nullptr, vis, ao, nullptr, &sky, W, H, z) == E, "no bent");
    CHECK(rtsh_combine_visibility_list_ao_bent(&k, &lst, nullptr, pos, nrm, nullptr, vis, ao, bent, nullptr, W, H, z) == E, "no sky");
    CHECK(rtsh_combine_visibility_list_ao_bent(&k, &lst, nullptr, pos, nrm, nullptr, vis, nullptr, bent, &sky, W, H, z) == E, "no ao");
    CHECK(rtsh_combine_visibility_list_ao_bent(&k, &lst, nullptr, pos, nullptr, nullptr, vis, ao, bent, &sky, W, H, z) == E, "no normals");
    CHECK(rtsh_combine_visibility_list_ao_bent(&k, &lst, nullptr, pos, nrm, nullptr, vis, ao, bent, &sky, 0, H, z) == E, "W 0");
    for (uint32_t i = 0; i < px * 3; ++i) CHECK(z[i] == 0xAB, "a refusal wrote byte %u", i);
    CHECK(sizeof(rtsh_sky_ambient) == 48, "rtsh_sky_ambient is %zu bytes", sizeof(rtsh_sky_ambient));
    std::free(z); std::free(b); std::free(a); std::free(bent); std::free(ao); std::free(vis); std::free(pos); std::free(nrm);
}

int main() {
    quantise();
    size_t count = 0;
    rts_vec4u* stream = makeStream(&count);
    const uint32_t frames[4][2] = { { 1, 1 }, { 8, 8 }, { 17, 5 }, { 33, 9 } };
    for (const auto& f : frames)
        for (uint32_t n : { 1u, 3u, 4u, 5u, 16u, 48u })
            for (uint32_t table : { 0u, n, 64u }) {
                if (table && n < 2) continue;
                frame(stream, count, f[0], f[1], n, table, false);
                frame(stream, count, f[0], f[1], n, table, true);
            }
    CHECK(sawPartly > 0 && sawFull > 0 && sawZero > 0, "a class of pixels was never seen (%lu, %lu, %lu)", sawPartly, sawFull, sawZero);
    refusals(stream, count);
    combine();
    std::free(stream);
    std::printf("ok %lu\n", cases);
    return 0;
}
