// Host-only check of the half-resolution light list passes on TINY frames (tests/test_list_upsample_host.py, built with
// -fsanitize=address,undefined,float-cast-overflow together with raytracedshadows_amd/csrc/rts_scene.cpp).  Frames of 1 x 1, 1 x 5, 5 x 1,
// 2 x 2 and 3 x 3 in all four phases; every buffer is a heap block of exactly the stated size, so a tap outside w x h, a sampled pixel
// outside W x H or a plane from `count` up that is touched is a sanitizer report.  The sanitizers are the first check.  The second: a
// phase that leaves no sampled pixel is refused with nothing written; a sampled active pixel gets its low-resolution byte (anchor 1);
// uniform planes give their byte or 0 (anchor 2); under the retrace map's keep only bytes whose bit is clear are written; the end-to-end
// merge with thresholds that accept no neighbour rebuilds a "trace" that is a function of the pixel alone (anchor 4); one thread and
// three agree.  Prints the first case that differs and exits 1; "ok <cases>" otherwise.
#include "../../include/rts_scene.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

extern "C" int rts_bvh_validate(const rts_vec4u*, size_t, uint32_t*) { return RTS_ERR_BAD_BVH; }   // (no pass here takes a stream)

static unsigned long cases = 0;
#define CHECK(cond, ...) \
    do { ++cases; if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

template <class T> static T* block(size_t n) { return (T*)std::malloc(n * sizeof(T)); }      // exactly n elements

// The "trace" of the end-to-end check: a byte that depends on the pixel's position (its G-buffer texel) and the light alone.
static uint8_t traced(const float* position4, uint32_t l) { return (uint8_t)((int)(position4[0] * 10.0f + 0.5f) * 7 + (int)(position4[2] * 10.0f + 0.5f) * 3 + (int)l); }

static void frame(uint32_t W, uint32_t H, uint32_t px, uint32_t py, uint32_t count) {
    const size_t n = (size_t)W * H;
    float* pos = block<float>(n * 4);
    float* nrm = block<float>(n * 4);
    uint8_t* map = block<uint8_t>(n);
    for (size_t i = 0; i < n; ++i) {
        const float x = (float)(i % W), y = (float)(i / W);
        const float p[4] = { x * 0.1f, 0.0f, y * 0.1f, 1.0f }, up[4] = { 0.0f, 1.0f, 0.0f, 0.0f };
        std::memcpy(pos + i * 4, p, 16);
        std::memcpy(nrm + i * 4, up, 16);
        map[i] = (uint8_t)(0xFFu - (i % 3 == 2 ? 0x11u : 0u));
    }
    if (n >= 4) { nrm[1 * 4 + 1] = 0.0f; pos[2 * 4 + 1] = std::numeric_limits<float>::quiet_NaN(); }       // a background texel, a NaN one
    if (n >= 9) { nrm[4 * 4 + 0] = std::numeric_limits<float>::infinity(); pos[8 * 4 + 1] = 1.0f; }        // an Inf normal, a texel off the plane

    rtsh_upsample_params prm;
    std::memset(&prm, 0, sizeof prm);
    prm.phase_x = px; prm.phase_y = py; prm.normal_cos_min = 0.9f; prm.plane_eps = 0.05f;
    uint32_t w = 77, h = 77;
    const int sized = rtsh_subsampled_size(W, H, px, py, &w, &h);
    const bool empty = (W + 1 - px) / 2 == 0 || (H + 1 - py) / 2 == 0;
    CHECK((sized == RTS_OK) == !empty, "size %ux%u phase %u%u: status %d", W, H, px, py, sized);
    rts_soft_light_list* soft = block<rts_soft_light_list>(1);
    rts_light_list* hard = block<rts_light_list>(1);
    std::memset(soft, 0, sizeof *soft);
    std::memset(hard, 0, sizeof *hard);
    soft->count = hard->count = count;
    for (uint32_t l = 0; l < count; ++l) {
        soft->lights[l].type = hard->lights[l].type = RTS_LIGHT_DIRECTIONAL;
        soft->lights[l].xyz[1] = hard->lights[l].xyz[1] = 1.0f;
        soft->lights[l].nsamples = l % 2 ? 4u : 1u;
        soft->lights[l].radius = 0.5f;
    }
    uint8_t* planes = block<uint8_t>(count * n);
    uint8_t* mask = block<uint8_t>(n);
    uint8_t* retrace = block<uint8_t>(n);
    if (empty) {
        CHECK(w == 77 && h == 77, "size %ux%u: a refused call wrote its outputs", W, H);
        float* one = block<float>(4);
        uint8_t* byte = block<uint8_t>(1);
        one[0] = 5.0f; byte[0] = 9; std::memset(planes, 0x5A, count * n); std::memset(retrace, 0x5A, n); std::memset(mask, 0x5A, n);
        CHECK(rtsh_subsample_gbuffer(&prm, pos, nrm, map, W, H, one, one, byte) == RTS_ERR_INVALID_ARG, "subsample of an empty lattice");
        CHECK(rtsh_upsample_retrace_map(count, &prm, pos, nrm, map, one, one, byte, W, H, retrace, 0) == RTS_ERR_INVALID_ARG, "retrace, empty");
        CHECK(rtsh_upsample_soft_light_list(soft, &prm, pos, nrm, map, one, one, byte, byte, nullptr, W, H, planes, 0) == RTS_ERR_INVALID_ARG, "soft, empty");
        CHECK(rtsh_upsample_light_list(hard, &prm, pos, nrm, map, one, one, byte, byte, nullptr, W, H, mask, 0) == RTS_ERR_INVALID_ARG, "hard, empty");
        bool clean = one[0] == 5.0f && byte[0] == 9;
        for (size_t i = 0; i < n; ++i) clean = clean && retrace[i] == 0x5A && mask[i] == 0x5A;
        for (size_t i = 0; i < count * n; ++i) clean = clean && planes[i] == 0x5A;
        CHECK(clean, "size %ux%u phase %u%u: a refused call wrote", W, H, px, py);
        std::free(one); std::free(byte);
    } else {
        const size_t m = (size_t)w * h;
        float* lpos = block<float>(m * 4);
        float* lnrm = block<float>(m * 4);
        uint8_t* lmap = block<uint8_t>(m);
        uint8_t* lo = block<uint8_t>(count * m);
        uint8_t* lmask = block<uint8_t>(m);
        CHECK(rtsh_subsample_gbuffer(&prm, pos, nrm, map, W, H, lpos, lnrm, lmap) == RTS_OK, "subsample %ux%u", W, H);
        for (size_t q = 0; q < m; ++q) {
            const size_t p = (2 * (q / w) + py) * W + 2 * (q % w) + px;
            CHECK(std::memcmp(lpos + q * 4, pos + p * 4, 16) == 0 && std::memcmp(lnrm + q * 4, nrm + p * 4, 16) == 0 && lmap[q] == map[p],
                  "subsample %ux%u phase %u%u: texel %zu", W, H, px, py, q);
        }
        CHECK(rtsh_subsample_gbuffer(&prm, pos, nrm, nullptr, W, H, lpos, lnrm, nullptr) == RTS_OK, "subsample without a map");
        for (int withMaps = 0; withMaps < 2; ++withMaps) {
            const uint8_t *fm = withMaps ? map : nullptr, *lm = withMaps ? lmap : nullptr;
            // anchors 1 and 2 at the ordinary thresholds, without keep
            for (size_t q = 0; q < m; ++q) {
                lmask[q] = (uint8_t)(q * 37 + 5);
                for (uint32_t l = 0; l < count; ++l) lo[l * m + q] = (uint8_t)(q * 51 + l * 17 + 200);
            }
            CHECK(rtsh_upsample_soft_light_list(soft, &prm, pos, nrm, fm, lpos, lnrm, lm, lo, nullptr, W, H, planes, 1) == RTS_OK, "soft");
            CHECK(rtsh_upsample_light_list(hard, &prm, pos, nrm, fm, lpos, lnrm, lm, lmask, nullptr, W, H, mask, 1) == RTS_OK, "hard");
            for (size_t q = 0; q < m; ++q) {
                const size_t p = (2 * (q / w) + py) * W + 2 * (q % w) + px;
                const bool bg = nrm[p * 4] == 0.0f && nrm[p * 4 + 1] == 0.0f && nrm[p * 4 + 2] == 0.0f;
                const uint32_t on = bg ? 0u : (fm ? fm[p] : 0xFFu) & ((1u << count) - 1u);
                for (uint32_t l = 0; l < count; ++l)
                    CHECK(planes[l * n + p] == (((on >> l) & 1u) ? lo[l * m + q] : 0), "anchor 1, %ux%u phase %u%u light %u texel %zu", W, H, px, py, l, q);
                CHECK(mask[p] == (lmask[q] & on), "anchor 1 (hard), %ux%u phase %u%u texel %zu", W, H, px, py, q);
            }
            uint8_t* again = block<uint8_t>(count * n);
            CHECK(rtsh_upsample_soft_light_list(soft, &prm, pos, nrm, fm, lpos, lnrm, lm, lo, nullptr, W, H, again, 3) == RTS_OK, "soft, 3 threads");
            CHECK(std::memcmp(again, planes, count * n) == 0, "one thread and three differ, %ux%u", W, H);
            std::memset(lo, 201, count * m);
            CHECK(rtsh_upsample_soft_light_list(soft, &prm, pos, nrm, fm, lpos, lnrm, lm, lo, nullptr, W, H, again, 0) == RTS_OK, "soft, uniform");
            for (size_t i = 0; i < count * n; ++i) CHECK(again[i] == 201 || again[i] == 0, "anchor 2, %ux%u: byte %u", W, H, again[i]);
            std::free(again);
            // anchor 4: no neighbour accepted; low-resolution "trace", retrace map, masked full-resolution "trace", upsample with keep
            rtsh_upsample_params none = prm;
            none.plane_eps = -1.0f;
            CHECK(rtsh_upsample_retrace_map(count, &none, pos, nrm, fm, lpos, lnrm, lm, W, H, retrace, 0) == RTS_OK, "retrace map");
            for (size_t q = 0; q < m; ++q)
                for (uint32_t l = 0; l < count; ++l) lo[l * m + q] = (lm == nullptr || ((lm[q] >> l) & 1u)) ? traced(lpos + q * 4, l) : 0;
            for (size_t p = 0; p < n; ++p)
                for (uint32_t l = 0; l < count; ++l) planes[l * n + p] = ((retrace[p] >> l) & 1u) ? traced(pos + p * 4, l) : 0;
            CHECK(rtsh_upsample_soft_light_list(soft, &none, pos, nrm, fm, lpos, lnrm, lm, lo, retrace, W, H, planes, 0) == RTS_OK, "merge");
            for (size_t p = 0; p < n; ++p) {
                const bool bg = nrm[p * 4] == 0.0f && nrm[p * 4 + 1] == 0.0f && nrm[p * 4 + 2] == 0.0f;
                const uint32_t on = bg ? 0u : (fm ? fm[p] : 0xFFu) & ((1u << count) - 1u);
                for (uint32_t l = 0; l < count; ++l)
                    CHECK(planes[l * n + p] == (((on >> l) & 1u) ? traced(pos + p * 4, l) : 0), "anchor 4, %ux%u phase %u%u light %u pixel %zu: %u",
                          W, H, px, py, l, p, planes[l * n + p]);
            }
            // keep: the bytes whose bit is set stay; the ordinary retrace map marks no sampled pixel and no inactive one
            CHECK(rtsh_upsample_retrace_map(count, &prm, pos, nrm, fm, lpos, lnrm, lm, W, H, retrace, 3) == RTS_OK, "retrace map, ordinary");
            std::memset(planes, 0x5A, count * n);
            std::memset(mask, 0x5A, n);
            CHECK(rtsh_upsample_soft_light_list(soft, &prm, pos, nrm, fm, lpos, lnrm, lm, lo, retrace, W, H, planes, 0) == RTS_OK, "soft, keep");
            CHECK(rtsh_upsample_light_list(hard, &prm, pos, nrm, fm, lpos, lnrm, lm, lmask, retrace, W, H, mask, 0) == RTS_OK, "hard, keep");
            for (size_t p = 0; p < n; ++p) {
                const bool sampled = (p % W) % 2 == px && (p / W) % 2 == py;
                CHECK(!(sampled && retrace[p]), "a sampled pixel in the retrace map, %ux%u pixel %zu", W, H, p);
                for (uint32_t l = 0; l < count; ++l)
                    if ((retrace[p] >> l) & 1u) {
                        CHECK(planes[l * n + p] == 0x5A, "a kept byte was written, %ux%u pixel %zu light %u", W, H, p, l);
                        CHECK(((mask[p] >> l) & 1u) == ((0x5Au >> l) & 1u), "a kept bit was written, %ux%u pixel %zu light %u", W, H, p, l);
                    }
            }
        }
        std::free(lpos); std::free(lnrm); std::free(lmap); std::free(lo); std::free(lmask);
    }
    std::free(pos); std::free(nrm); std::free(map); std::free(soft); std::free(hard); std::free(planes); std::free(mask); std::free(retrace);
}

int main() {
    const uint32_t sizes[5][2] = { { 1, 1 }, { 1, 5 }, { 5, 1 }, { 2, 2 }, { 3, 3 } };
    for (const auto& s : sizes)
        for (uint32_t phase = 0; phase < 4; ++phase)
            for (uint32_t count = 1; count <= 8; count += 7) frame(s[0], s[1], phase & 1u, phase >> 1, count);
    std::printf("ok %lu\n", cases);
    return 0;
}
