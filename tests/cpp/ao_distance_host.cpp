// Host-only check of AO distance and falloff on the host (tests/test_ao_distance_host.py, built with -fsanitize=address,undefined
// together with raytracedshadows_amd/csrc/rts_scene.cpp): rtsh_ambient_occlusion_distance over frames of 1 x 1, 8 x 8, 17 x 5 and
// 33 x 9 above tests/cpp/ao_bent_host.cpp's hand-made stream (a ground quad of two triangles under a small roof triangle), with
// background pixels, an active map, NaN positions wherever no ray may start, n of 1, 3, 4, 5, 16 and 48 and tables 0, n and 64.
// Positions, normals, map and the three planes are heap blocks of exactly the stated size, so an index outside the frame, outside the
// 64 weights or a write to a row outside the range is a sanitizer report.  The sanitizers are the first check (the conversion of the
// bin to an integer included).  The second: the bin on the edges k / 64 and their predecessors, +0, 1.0 and beyond; the quotient's two
// ends; counts equal rtsh_ambient_occlusion's plane; distance finite exactly where counts < n; anchors 2, 3 and 4; inactive texels 0,
// +0 and 0; each plane NULL in turn gives the others unchanged; a row range against the whole frame, rows outside it untouched; every
// refusal with nothing written.  Prints the first case that differs and exits 1; "ok <cases>" otherwise.
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
static float floatOf(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static const uint32_t INF = 0x7F800000u;

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

// The shared per-sample source on its edges: bin k starts exactly at k / 64, the float in front of it is bin k - 1; +0 is bin 0; 1.0,
// anything beyond it and the largest finite float are bin 63.
static void perSample() {
    using rts_harness::aoFalloffBin;
    using rts_harness::aoObscurance;
    using rts_harness::aoOpenness;
    CHECK(aoFalloffBin(0u) == 0u, "+0 is bin %u", aoFalloffBin(0u));
    CHECK(aoFalloffBin(1u) == 0u, "the smallest denormal is bin %u", aoFalloffBin(1u));
    for (uint32_t kk = 1; kk <= 64; ++kk) {
        const uint32_t edge = bitsOf((float)kk / 64.0f);
        const uint32_t at = kk < 64 ? kk : 63u;
        CHECK(aoFalloffBin(edge) == at, "%u / 64 is bin %u", kk, aoFalloffBin(edge));
        CHECK(aoFalloffBin(edge - 1u) == kk - 1u, "the float in front of %u / 64 is bin %u", kk, aoFalloffBin(edge - 1u));
    }
    CHECK(aoFalloffBin(bitsOf(1.0f) + 1u) == 63u && aoFalloffBin(bitsOf(7.5f)) == 63u && aoFalloffBin(INF - 1u) == 63u, "beyond the segment");
    uint8_t w[64];
    for (int b = 0; b < 64; ++b) w[b] = (uint8_t)(b * 3 + 1);
    const auto weightOf = [&](uint32_t b) { return w[b]; };
    CHECK(aoOpenness(INF, weightOf) == 255u, "a free sample");
    CHECK(aoOpenness(0u, weightOf) == 1u && aoOpenness(bitsOf(0.5f), weightOf) == 97u && aoOpenness(bitsOf(1.0f), weightOf) == 190u, "a blocked sample");
    for (uint32_t n : { 1u, 2u, 3u, 16u, 47u, 48u }) {
        const uint32_t S = 65535u / n;
        CHECK(aoObscurance(0u, n) == 0u, "A = 0");
        CHECK(aoObscurance(255u * n, n) == n * S, "n %u: A = 255 n gives %u, not %u", n, aoObscurance(255u * n, n), n * S);
        for (uint32_t c = 0; c <= n; ++c) CHECK(aoObscurance(255u * c, n) == c * S, "n %u: A = 255 * %u", n, c);
        for (uint32_t A = 1; A <= 255u * n; ++A)
            CHECK(aoObscurance(A, n) >= aoObscurance(A - 1u, n) && aoObscurance(A, n) <= n * S, "n %u: the quotient at A = %u", n, A);
    }
}

static unsigned long sawPartly = 0, sawFull = 0, sawZero = 0, sawBins = 0;

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
            ao.dirs[j][c] = (float)(seed >> 8) / 8388608.0f - (c == 2 ? 0.0f : 1.0f);   // x, y in [-1, 1), z in [0, 2)
        }
    rts_ao_falloff saw, zeros, full, raised;
    for (int b = 0; b < 64; ++b) { saw.weight[b] = (uint8_t)((b * 37 + 11) % 256); zeros.weight[b] = 0; full.weight[b] = 255; }
    raised = saw;
    for (int b = 0; b < 64; b += 3) raised.weight[b] = (uint8_t)(saw.weight[b] < 200 ? saw.weight[b] + 55 : 255);
    const uint32_t ns = n ? n : 1u, S = 65535u / ns;
    uint8_t* counts = block<uint8_t>(px);
    float* dist = block<float>(px);
    uint16_t* obs = block<uint16_t>(px);
    std::memset(counts, 0xAB, px); std::memset(dist, 0xAB, px * 4); std::memset(obs, 0xAB, px * 2);
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &ao, &saw, pos, nrm, act, W, H, 0, H, counts, dist, obs, 2) == RTS_OK,
          "%ux%u n %u: the whole frame", W, H, n);
    uint8_t* plain = block<uint8_t>(px);
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &ao, pos, nrm, act, W, H, 0, H, plain, 1) == RTS_OK, "the AO plane");
    uint16_t* o0 = block<uint16_t>(px);
    uint16_t* o255 = block<uint16_t>(px);
    uint16_t* oUp = block<uint16_t>(px);
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &ao, &zeros, pos, nrm, act, W, H, 0, H, nullptr, nullptr, o0, 1) == RTS_OK, "zeros");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &ao, &full, pos, nrm, act, W, H, 0, H, nullptr, nullptr, o255, 1) == RTS_OK, "all 255");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &ao, &raised, pos, nrm, act, W, H, 0, H, nullptr, nullptr, oUp, 1) == RTS_OK, "raised");
    for (size_t i = 0; i < px; ++i) {
        CHECK(counts[i] == plain[i], "%ux%u n %u table %u: count %zu is %u, not %u", W, H, n, table, i, counts[i], plain[i]);   // anchor 1
        if (!live[i]) {
            CHECK(counts[i] == 0 && bitsOf(dist[i]) == 0 && obs[i] == 0 && o0[i] == 0 && o255[i] == 0, "%ux%u n %u: dead pixel %zu", W, H, n, i);
            continue;
        }
        CHECK((bitsOf(dist[i]) < INF) == (counts[i] < ns) && bitsOf(dist[i]) <= INF, "%ux%u n %u: pixel %zu: distance %g with %u free", W, H, n, i,
              (double)dist[i], counts[i]);
        CHECK(o0[i] == counts[i] * S, "%ux%u n %u: anchor 2 at %zu: %u", W, H, n, i, o0[i]);
        CHECK(o255[i] == ns * S, "%ux%u n %u: anchor 3 at %zu: %u", W, H, n, i, o255[i]);
        CHECK(obs[i] >= counts[i] * S && obs[i] <= ns * S && oUp[i] >= obs[i], "%ux%u n %u: anchor 4 at %zu: %u, raised %u", W, H, n, i, obs[i], oUp[i]);
        if (ns == 1u && counts[i] == 0u) {                               // one blocked sample: the plane shows the weight of its bin
            const uint32_t b = rts_harness::aoFalloffBin(bitsOf(dist[i]));
            CHECK(obs[i] == (2u * saw.weight[b] * S + 255u) / 510u, "%ux%u: one sample at %zu: bin %u", W, H, i, b);
            sawBins |= 1ul << (b & 63u);
        }
        sawZero += counts[i] == 0; sawFull += counts[i] == ns; sawPartly += counts[i] != 0 && counts[i] != ns;
    }
    // each plane NULL in turn: the others keep their bytes
    uint8_t* c2 = block<uint8_t>(px);
    float* d2 = block<float>(px);
    uint16_t* s2 = block<uint16_t>(px);
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &ao, &saw, pos, nrm, act, W, H, 0, H, nullptr, d2, s2, 1) == RTS_OK, "counts NULL");
    CHECK(std::memcmp(d2, dist, px * 4) == 0 && std::memcmp(s2, obs, px * 2) == 0, "%ux%u n %u: counts = NULL changes a plane", W, H, n);
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &ao, nullptr, pos, nrm, act, W, H, 0, H, c2, d2, nullptr, 1) == RTS_OK, "obscurance NULL");
    CHECK(std::memcmp(d2, dist, px * 4) == 0 && std::memcmp(c2, counts, px) == 0, "%ux%u n %u: obscurance = NULL changes a plane", W, H, n);
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &ao, &saw, pos, nrm, act, W, H, 0, H, c2, nullptr, s2, 1) == RTS_OK, "distance NULL");
    CHECK(std::memcmp(s2, obs, px * 2) == 0 && std::memcmp(c2, counts, px) == 0, "%ux%u n %u: distance = NULL changes a plane", W, H, n);
    // a row range: the same bits inside, the fill outside
    const uint32_t r0 = H / 3, r1 = H - H / 4;
    std::memset(c2, 0xAB, px); std::memset(d2, 0xAB, px * 4); std::memset(s2, 0xAB, px * 2);
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &ao, &saw, pos, nrm, act, W, H, r0, r1, c2, d2, s2, 1) == RTS_OK, "%ux%u: rows", W, H);
    for (size_t i = 0; i < px; ++i) {
        const uint32_t y = (uint32_t)(i / W);
        const bool in = y >= r0 && y < r1;
        CHECK(c2[i] == (in ? counts[i] : 0xAB) && bitsOf(d2[i]) == (in ? bitsOf(dist[i]) : 0xABABABABu) && s2[i] == (in ? obs[i] : 0xABAB),
              "%ux%u n %u rows %u..%u: pixel %zu", W, H, n, r0, r1, i);
    }
    std::free(s2); std::free(d2); std::free(c2); std::free(oUp); std::free(o255); std::free(o0); std::free(plain); std::free(obs);
    std::free(dist); std::free(counts); std::free(live); std::free(act); std::free(nrm); std::free(pos);
}

static void refusals(const rts_vec4u* stream, size_t count) {
    const uint32_t W = 5, H = 3;
    float* pos = block<float>(W * H * 4);
    float* nrm = block<float>(W * H * 4);
    for (uint32_t i = 0; i < W * H * 4; ++i) { pos[i] = i % 4 == 1 ? -4.0f : 0.25f * (float)(i % 7); nrm[i] = i % 4 == 1 ? 1.0f : 0.0f; }
    uint8_t* counts = block<uint8_t>(W * H);
    float* dist = block<float>(W * H + 1);
    uint16_t* obs = block<uint16_t>(W * H + 1);
    std::memset(counts, 0xAB, W * H); std::memset(dist, 0xAB, (W * H + 1) * 4); std::memset(obs, 0xAB, (W * H + 1) * 2);
    rts_constants k;
    std::memset(&k, 0, sizeof(k));
    rts_ao_params good;
    std::memset(&good, 0, sizeof(good));
    good.nsamples = 4; good.radius = 1.0f;
    for (int j = 0; j < 64; ++j) good.dirs[j][2] = 1.0f;
    rts_ao_falloff f;
    std::memset(&f, 7, sizeof(f));
    const float inf = std::numeric_limits<float>::infinity();
    rts_ao_params bad[7] = { good, good, good, good, good, good, good };
    bad[0].nsamples = 49; bad[1].table = 3; bad[2].table = 65; bad[3].nsamples = 1; bad[3].table = 2; bad[4].radius = inf;
    bad[5].radius = -inf; bad[6].radius = std::numeric_limits<float>::quiet_NaN();
    const int E = RTS_ERR_INVALID_ARG;
    for (const rts_ao_params& b : bad)
        CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &b, &f, pos, nrm, nullptr, W, H, 0, H, counts, dist, obs, 1) == E, "bad params accepted");
    CHECK(rtsh_ambient_occlusion_distance(nullptr, count, &k, &good, &f, pos, nrm, nullptr, W, H, 0, H, counts, dist, obs, 1) == E, "no stream");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, nullptr, &good, &f, pos, nrm, nullptr, W, H, 0, H, counts, dist, obs, 1) == E, "no constants");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, nullptr, &f, pos, nrm, nullptr, W, H, 0, H, counts, dist, obs, 1) == E, "no params");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &good, &f, nullptr, nrm, nullptr, W, H, 0, H, counts, dist, obs, 1) == E, "no positions");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &good, &f, pos, nullptr, nullptr, W, H, 0, H, counts, dist, obs, 1) == E, "no normals");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &good, &f, pos, nrm, nullptr, W, H, 0, H, counts, nullptr, nullptr, 1) == E, "both outputs NULL");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &good, nullptr, pos, nrm, nullptr, W, H, 0, H, counts, dist, obs, 1) == E, "obscurance without falloff");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &good, &f, pos, nrm, nullptr, W, H, 0, H, counts, dist, (uint16_t*)((uint8_t*)obs + 1), 1) == E,
          "an odd obscurance pointer");
    for (int off = 1; off < 4; ++off)
        CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &good, &f, pos, nrm, nullptr, W, H, 0, H, counts, (float*)((uint8_t*)dist + off), obs, 1) == E,
              "a distance pointer at + %d", off);
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &good, &f, pos, nrm, nullptr, 0, H, 0, H, counts, dist, obs, 1) == E, "W 0");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &good, &f, pos, nrm, nullptr, W, H, 2, 1, counts, dist, obs, 1) == E, "rows reversed");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &good, &f, pos, nrm, nullptr, W, H, 0, H + 1, counts, dist, obs, 1) == E, "rows past H");
    for (uint32_t i = 0; i < W * H; ++i)
        CHECK(counts[i] == 0xAB && bitsOf(dist[i]) == 0xABABABABu && obs[i] == 0xABAB, "a refusal wrote pixel %u", i);
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &good, &f, pos, nrm, nullptr, W, H, 1, 1, counts, dist, obs, 1) == RTS_OK && counts[0] == 0xAB,
          "an empty range");
    CHECK(rtsh_ambient_occlusion_distance(stream, count, &k, &good, &f, pos, nrm, nullptr, W, H, 0, H, counts, dist, obs, 1) == RTS_OK, "the good call");
    for (uint32_t i = 0; i < W * H; ++i) CHECK(counts[i] <= 4 && (floatOf(bitsOf(dist[i])) >= 0.0f), "the good call: pixel %u", i);
    CHECK(sizeof(rts_ao_falloff) == 64, "rts_ao_falloff is %zu bytes", sizeof(rts_ao_falloff));
    std::free(obs); std::free(dist); std::free(counts); std::free(nrm); std::free(pos);
}

int main() {
    perSample();
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
    std::free(stream);
    std::printf("ok %lu\n", cases);
    return 0;
}
