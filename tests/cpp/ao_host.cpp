// Host-only check of ambient occlusion on the host (tests/test_ao_host.py, built with -fsanitize=address,undefined together with
// raytracedshadows_amd/csrc/rts_scene.cpp): rtsh_ambient_occlusion and rtsh_ao_rays over frames of 1 x 1, 8 x 8, 17 x 5 and 33 x 9 above
// a hand-made stream (a ground quad of two triangles under a small roof triangle), with background pixels, an active map, NaN positions
// wherever no ray may start, sample counts 1, 3, 4 and 48 and tables 0, n and 64.  Positions, normals, map, counts and rays are heap
// blocks of exactly the stated size, so an index outside the frame, a read of a row outside the range's counts or a ray record past
// W * H * n is a sanitizer report.  The sanitizers are the first check.  The second: counts of a row range against the counts of the
// whole frame, rows outside it untouched; zeros exactly at the pixels that send no ray; the zero records of rtsh_ao_rays; every ray
// of a live pixel a segment (tmax 1) that leaves the surface; every refusal with nothing written.  Prints the first case that differs
// and exits 1; "ok <cases>" otherwise.
#include "../../include/rts_scene.h"
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
    const uint32_t ns = n > 1 ? n : 1;
    uint8_t* whole = block<uint8_t>(px);
    std::memset(whole, 0xAB, px);
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &ao, pos, nrm, act, W, H, 0, H, whole, 2) == RTS_OK, "%ux%u n %u: the whole frame", W, H, n);
    unsigned long open = 0, shut = 0;
    for (size_t i = 0; i < px; ++i) {
        CHECK(whole[i] <= ns && (live[i] || whole[i] == 0), "%ux%u n %u table %u: count %u at %zu", W, H, n, table, whole[i], i);
        if (live[i]) { open += whole[i]; shut += ns - whole[i]; }
    }
    if (W >= 17 && !masked) CHECK(open > 0 && shut > 0, "%ux%u n %u: the roof shades nothing or everything (%lu, %lu)", W, H, n, open, shut);
    // a row range: the same counts inside, the fill outside
    const uint32_t r0 = H / 3, r1 = H - H / 4;
    uint8_t* part = block<uint8_t>(px);
    std::memset(part, 0xAB, px);
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &ao, pos, nrm, act, W, H, r0, r1, part, 1) == RTS_OK, "%ux%u: rows", W, H);
    for (size_t i = 0; i < px; ++i) {
        const uint32_t y = (uint32_t)(i / W);
        CHECK(part[i] == ((y >= r0 && y < r1) ? whole[i] : 0xAB), "%ux%u n %u rows %u..%u: byte %zu", W, H, n, r0, r1, i);
    }
    // the rays: exactly W * H * ns records
    rts_ray* rays = block<rts_ray>(px * ns);
    std::memset(rays, 0xCD, px * ns * sizeof(rts_ray));
    CHECK(rtsh_ao_rays(&k, &ao, pos, nrm, act, W, H, rays) == RTS_OK, "%ux%u n %u: rays", W, H, n);
    for (size_t i = 0; i < px; ++i)
        for (uint32_t j = 0; j < ns; ++j) {
            const rts_ray& r = rays[i * ns + j];
            if (!live[i]) {
                bool zero = true;
                for (int c = 0; c < 4; ++c) zero = zero && bitsOf(r.o[c]) == 0 && bitsOf(r.d[c]) == 0;
                CHECK(zero, "%ux%u n %u: ray %u of dead pixel %zu is not zero", W, H, n, j, i);
            } else {
                CHECK(r.o[3] == 1.0f && bitsOf(r.d[3]) == 0 && std::isfinite(r.o[0]) && std::isfinite(r.d[1]) && std::fabs(r.o[1]) < 1e-2f,
                      "%ux%u n %u: ray %u of pixel %zu", W, H, n, j, i);
            }
        }
    std::free(rays); std::free(part); std::free(whole); std::free(live); std::free(act); std::free(nrm); std::free(pos);
}

static void refusals(const rts_vec4u* stream, size_t count) {
    const uint32_t W = 5, H = 3;
    float* pos = block<float>(W * H * 4);
    float* nrm = block<float>(W * H * 4);
    for (uint32_t i = 0; i < W * H * 4; ++i) { pos[i] = i % 4 == 1 ? -4.0f : 0.25f * (float)(i % 7); nrm[i] = i % 4 == 1 ? 1.0f : 0.0f; }
    uint8_t* counts = block<uint8_t>(W * H);
    std::memset(counts, 0xAB, W * H);
    rts_ray* rays = block<rts_ray>(W * H * 4);
    std::memset(rays, 0xCD, W * H * 4 * sizeof(rts_ray));
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
    for (const rts_ao_params& b : bad) {
        CHECK(rtsh_ambient_occlusion(stream, count, &k, &b, pos, nrm, nullptr, W, H, 0, H, counts, 1) == E, "bad params accepted");
        CHECK(rtsh_ao_rays(&k, &b, pos, nrm, nullptr, W, H, rays) == E, "bad params accepted for rays");
    }
    CHECK(rtsh_ambient_occlusion(nullptr, count, &k, &good, pos, nrm, nullptr, W, H, 0, H, counts, 1) == E, "no stream");
    CHECK(rtsh_ambient_occlusion(stream, count, nullptr, &good, pos, nrm, nullptr, W, H, 0, H, counts, 1) == E, "no constants");
    CHECK(rtsh_ambient_occlusion(stream, count, &k, nullptr, pos, nrm, nullptr, W, H, 0, H, counts, 1) == E, "no params");
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &good, nullptr, nrm, nullptr, W, H, 0, H, counts, 1) == E, "no positions");
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &good, pos, nullptr, nullptr, W, H, 0, H, counts, 1) == E, "no normals");
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &good, pos, nrm, nullptr, W, H, 0, H, nullptr, 1) == E, "no counts");
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &good, pos, nrm, nullptr, 0, H, 0, H, counts, 1) == E, "W 0");
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &good, pos, nrm, nullptr, W, H, 2, 1, counts, 1) == E, "rows reversed");
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &good, pos, nrm, nullptr, W, H, 0, H + 1, counts, 1) == E, "rows past H");
    CHECK(rtsh_ao_rays(nullptr, &good, pos, nrm, nullptr, W, H, rays) == E && rtsh_ao_rays(&k, nullptr, pos, nrm, nullptr, W, H, rays) == E &&
          rtsh_ao_rays(&k, &good, nullptr, nrm, nullptr, W, H, rays) == E && rtsh_ao_rays(&k, &good, pos, nullptr, nullptr, W, H, rays) == E &&
          rtsh_ao_rays(&k, &good, pos, nrm, nullptr, W, H, nullptr) == E && rtsh_ao_rays(&k, &good, pos, nrm, nullptr, W, 0, rays) == E,
          "a NULL or an empty frame accepted for rays");
    for (uint32_t i = 0; i < W * H; ++i) CHECK(counts[i] == 0xAB, "a refusal wrote count %u", i);
    const unsigned char* raw = (const unsigned char*)rays;
    for (size_t i = 0; i < (size_t)W * H * 4 * sizeof(rts_ray); ++i) CHECK(raw[i] == 0xCD, "a refusal wrote a ray");
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &good, pos, nrm, nullptr, W, H, 1, 1, counts, 1) == RTS_OK && counts[0] == 0xAB, "an empty range");
    CHECK(rtsh_ambient_occlusion(stream, count, &k, &good, pos, nrm, nullptr, W, H, 0, H, counts, 1) == RTS_OK && counts[W * H - 1] <= 4, "the good call");
    std::free(rays); std::free(counts); std::free(nrm); std::free(pos);
}

int main() {
    size_t count = 0;
    rts_vec4u* stream = makeStream(&count);
    const uint32_t frames[4][2] = { { 1, 1 }, { 8, 8 }, { 17, 5 }, { 33, 9 } };
    for (const auto& f : frames)
        for (uint32_t n : { 0u, 1u, 3u, 4u, 48u })
            for (uint32_t table : { 0u, n, 64u }) {
                if (table && (n < 2 || table < n)) continue;
                frame(stream, count, f[0], f[1], n, table, false);
                frame(stream, count, f[0], f[1], n, table, true);
            }
    refusals(stream, count);
    std::free(stream);
    std::printf("ok %lu\n", cases);
    return 0;
}
