// Host-only check of the motion G-buffer pass and the motion forms of the three temporal passes (tests/test_list_motion_host.py, built
// with -fsanitize=address,undefined together with raytracedshadows_amd/csrc/rts_scene.cpp).  A hand-made stream of two triangles (one
// inner node, two leaves, two tails: 8 vec4) and its moved sibling; every buffer is a heap block of exactly the stated size, so that a
// read of prev_packed beyond its end, of a tap outside the frame or a write behind an output is reported.  The sanitizers are the first
// check; the second: the refusals leave the outputs as they were, a previous stream equal to the current one gives w == 1 and the parents'
// bytes from all three motion forms, a moved one gives w == 2 on the moved triangle, one thread and three threads agree, and the first
// frame takes NULL motion planes.  Prints the first case that differs and exits 1; "ok <cases>" otherwise.
#include "../../include/rts_scene.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

// the library proper validates streams; here the stream is the hand-made one below or a truncated copy of it
extern "C" int rts_bvh_validate(const rts_vec4u*, size_t count, uint32_t* prims) {
    if (count != 8) return RTS_ERR_BAD_BVH;
    if (prims) *prims = 2;
    return RTS_OK;
}

static unsigned long cases = 0;
#define CHECK(cond, ...) \
    do { ++cases; if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

template <class T> static T* block(size_t n) { return (T*)std::malloc(n * sizeof(T)); }      // exactly n elements

static uint32_t bitsOf(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static const uint32_t END = 0xFFFFFFFFu;

// two triangles in the plane z = -3 (+ lift), left and right of x = 0; node 0 their box, nodes 1 and 2 the leaves, tails at vec4 6 and 7
static uint32_t* makeStream(float liftRight) {
    uint32_t* w = block<uint32_t>(8 * 4);
    const float z1 = -3.0f + liftRight;
    const float lo[3] = { -2.0f, -2.0f, z1 < -3.0f ? z1 : -3.0f }, hi[3] = { 2.0f, 2.0f, z1 > -3.0f ? z1 : -3.0f };
    for (int k = 0; k < 3; ++k) { w[k] = bitsOf(lo[k]); w[4 + k] = bitsOf(hi[k]); }
    w[3] = END; w[7] = END;
    const float v0[2][3] = { { -2.0f, -2.0f, -3.0f }, { 0.0f, -2.0f, z1 } };
    for (int t = 0; t < 2; ++t) {
        uint32_t* a = w + (1 + t) * 8;
        const float e0[3] = { 2.0f, 0.0f, 0.0f }, e1[3] = { 0.0f, 4.0f, 0.0f };
        for (int k = 0; k < 3; ++k) { a[k] = bitsOf(e0[k]); a[4 + k] = bitsOf(e1[k]); w[(6 + t) * 4 + k] = bitsOf(v0[t][k]); }
        a[3] = 6u + (uint32_t)t;
        a[7] = t == 0 ? 2u : END;
        w[(6 + t) * 4 + 3] = 0u;
    }
    return w;
}

struct Frame {
    uint32_t W, H;
    size_t n;
    float *pos, *nrm, *pts, *pnr, *prevPos, *prevNrm, *vis, *hist, *out, *out2;
    uint32_t *leaves, *sqHist, *sq, *sq2;
    uint16_t *meanHist, *mean, *mean2;
    uint8_t *counts, *lens, *len, *len2;
    Frame(uint32_t w, uint32_t h) : W(w), H(h), n((size_t)w * h) {
        pos = block<float>(n * 4); nrm = block<float>(n * 4); pts = block<float>(n * 4); pnr = block<float>(n * 4);
        prevPos = block<float>(n * 4); prevNrm = block<float>(n * 4);
        vis = block<float>(n * 2); hist = block<float>(n * 2); out = block<float>(n * 2); out2 = block<float>(n * 2);
        leaves = block<uint32_t>(n); sqHist = block<uint32_t>(n * 2); sq = block<uint32_t>(n * 2); sq2 = block<uint32_t>(n * 2);
        meanHist = block<uint16_t>(n * 2); mean = block<uint16_t>(n * 2); mean2 = block<uint16_t>(n * 2);
        counts = block<uint8_t>(n * 2); lens = block<uint8_t>(n * 2); len = block<uint8_t>(n * 2); len2 = block<uint8_t>(n * 2);
        for (size_t i = 0; i < n * 2; ++i) {
            vis[i] = (float)(i % 5) * 0.25f; hist[i] = (float)(i % 7) / 8.0f; counts[i] = (uint8_t)(i % 5); lens[i] = (uint8_t)(i % 4);
            meanHist[i] = (uint16_t)(i * 977u); sqHist[i] = (uint32_t)(i * 2654435761u);
        }
        reset();
    }
    void reset() {
        for (size_t i = 0; i < n * 2; ++i) { out[i] = out2[i] = 7.5f; sq[i] = sq2[i] = 0xA5A5A5A5u; mean[i] = mean2[i] = 0xA5A5u; }
        std::memset(len, 0xAB, n * 2); std::memset(len2, 0xAB, n * 2);
    }
    bool untouched() const {
        for (size_t i = 0; i < n * 2; ++i) if (out[i] != 7.5f || len[i] != 0xAB || sq[i] != 0xA5A5A5A5u || mean[i] != 0xA5A5u) return false;
        return true;
    }
    ~Frame() {
        void* all[] = { pos, nrm, pts, pnr, prevPos, prevNrm, vis, hist, out, out2, leaves, sqHist, sq, sq2, meanHist, mean, mean2, counts, lens, len, len2 };
        for (void* p : all) std::free(p);
    }
};

int main() {
    uint32_t* cur = makeStream(0.5f);
    uint32_t* old = makeStream(0.0f);
    const rts_vec4u *packed = (const rts_vec4u*)cur, *prev = (const rts_vec4u*)old;
    const float eye[3] = { 0.0f, 0.0f, 0.0f }, prevEye[3] = { 0.05f, 0.0f, 0.0f }, target[3] = { 0.0f, 0.0f, -1.0f };
    const float nanEye[3] = { 0.0f, std::numeric_limits<float>::quiet_NaN(), 0.0f };
    rts_light_list hard; std::memset(&hard, 0, sizeof hard); hard.count = 2;
    rts_soft_light_list soft; std::memset(&soft, 0, sizeof soft); soft.count = 2;
    for (int l = 0; l < 2; ++l) soft.lights[l].nsamples = 4;
    float basis[14];
    const uint32_t sizes[][2] = { { 1, 1 }, { 9, 7 }, { 17, 33 } };
    for (const auto& wh : sizes) {
        const uint32_t W = wh[0], H = wh[1];
        Frame f(W, H);
        const size_t n = f.n;
        CHECK(rtsh_camera_basis(prevEye, target, 1.0f, W, H, basis) == RTS_OK, "basis");
        rtsh_temporal_params p; std::memset(&p, 0, sizeof p);
        for (int k = 0; k < 3; ++k) { p.eye_delta[k] = eye[k] - prevEye[k]; p.prev_fwd[k] = basis[3 + k]; p.prev_right[k] = basis[6 + k]; p.prev_up[k] = basis[9 + k]; }
        p.prev_scale_x = basis[12] * basis[13]; p.prev_scale_y = basis[12]; p.normal_cos_min = 0.9f; p.plane_eps = 0.02f; p.max_length = 5;
        const rtsh_history_clamp clamp = { 1, 0.0f, { 0, 0 } };
        uint64_t hits = 77;
        // ---- refusals of the G-buffer pass: nothing written
        std::memset(f.pos, 0x5A, n * 16); std::memset(f.pts, 0x5A, n * 16); std::memset(f.pnr, 0x5A, n * 16); std::memset(f.leaves, 0x5A, n * 4);
        auto clean = [&]() {
            const unsigned char* b[] = { (unsigned char*)f.pos, (unsigned char*)f.pts, (unsigned char*)f.pnr };
            for (auto* q : b) for (size_t i = 0; i < n * 16; ++i) if (q[i] != 0x5A) return false;
            for (size_t i = 0; i < n * 4; ++i) if (((unsigned char*)f.leaves)[i] != 0x5A) return false;
            return hits == 77;
        };
#define G(PK, C, PV, PC, E, PE, T, PTS, PNR) rtsh_primary_gbuffer_motion(PK, C, PV, PC, E, PE, T, 1.0f, W, H, f.pos, f.nrm, PTS, PNR, f.leaves, &hits, 1)
        CHECK(G(nullptr, 8, prev, 8, eye, prevEye, target, f.pts, f.pnr) == RTS_ERR_INVALID_ARG && clean(), "NULL packed");
        CHECK(G(packed, 8, nullptr, 8, eye, prevEye, target, f.pts, f.pnr) == RTS_ERR_INVALID_ARG && clean(), "NULL prev_packed");
        CHECK(G(packed, 8, prev, 8, eye, nullptr, target, f.pts, f.pnr) == RTS_ERR_INVALID_ARG && clean(), "NULL prev_eye");
        CHECK(G(packed, 8, prev, 8, eye, nanEye, target, f.pts, f.pnr) == RTS_ERR_INVALID_ARG && clean(), "NaN prev_eye");
        CHECK(G(packed, 8, prev, 8, eye, prevEye, target, nullptr, f.pnr) == RTS_ERR_INVALID_ARG && clean(), "NULL prev_points");
        CHECK(G(packed, 8, prev, 8, eye, prevEye, target, f.pts, nullptr) == RTS_ERR_INVALID_ARG && clean(), "NULL prev_point_normals");
        CHECK(G(packed, 8, prev, 7, eye, prevEye, target, f.pts, f.pnr) == RTS_ERR_INVALID_ARG && clean(), "prev count");
        old[1 * 8 + 7] = END;                                             // another link word: another topology
        CHECK(G(packed, 8, prev, 8, eye, prevEye, target, f.pts, f.pnr) == RTS_ERR_BAD_BVH && clean(), "topology");
        old[1 * 8 + 7] = 2u;
        // ---- frame 0 (the previous stream seen from the previous eye), then STATIC and MOVED frames
        CHECK(rtsh_primary_gbuffer_motion(prev, 8, prev, 8, prevEye, prevEye, target, 1.0f, W, H, f.prevPos, f.prevNrm, f.pts, f.pnr, nullptr, nullptr, 3) == RTS_OK, "frame 0");
        for (int moved = 0; moved < 2; ++moved) {
            const rts_vec4u* now = moved ? packed : prev;
            CHECK(rtsh_primary_gbuffer_motion(now, 8, prev, 8, eye, prevEye, target, 1.0f, W, H, f.pos, f.nrm, f.pts, f.pnr, f.leaves, &hits, 1) == RTS_OK, "frame 1");
            uint64_t count = 0;
            for (size_t i = 0; i < n; ++i) {
                count += f.pos[i * 4 + 3] != 0.0f;
                const float want = f.leaves[i] == END ? 0.0f : ((moved && f.leaves[i] == 2u) ? 2.0f : 1.0f);
                CHECK(f.pts[i * 4 + 3] == want, "w of pixel %zu at %u x %u, moved %d: %g", i, W, H, moved, f.pts[i * 4 + 3]);
            }
            CHECK(count == hits, "hit count");
            // ---- the refusals of the three motion forms, then their results
            f.reset();
#define A(PTS, PNR, OUT, LEN, TH) rtsh_accumulate_visibility_list_motion(&hard, &p, f.pos, f.nrm, nullptr, f.vis, f.prevPos, f.prevNrm, f.hist, f.lens, PTS, PNR, W, H, OUT, LEN, TH)
#define B(PTS, PNR, OUT, LEN, TH) rtsh_accumulate_visibility_list_clamped_motion(&hard, &p, f.pos, f.nrm, nullptr, f.vis, f.prevPos, f.prevNrm, f.hist, f.lens, PTS, PNR, W, H, OUT, LEN, &clamp, TH)
#define M(PTS, PNR, MEAN, SQ, LEN, TH) rtsh_accumulate_moments_soft_light_list_motion(&soft, &p, f.pos, f.nrm, nullptr, f.counts, f.prevPos, f.prevNrm, f.meanHist, f.sqHist, f.lens, PTS, PNR, W, H, MEAN, SQ, LEN, TH)
            CHECK(A(nullptr, f.pnr, f.out, f.len, 1) == RTS_ERR_INVALID_ARG && A(f.pts, nullptr, f.out, f.len, 1) == RTS_ERR_INVALID_ARG && f.untouched(), "plain: NULL plane");
            CHECK(B(nullptr, f.pnr, f.out, f.len, 1) == RTS_ERR_INVALID_ARG && B(f.pts, nullptr, f.out, f.len, 1) == RTS_ERR_INVALID_ARG && f.untouched(), "clamped: NULL plane");
            CHECK(M(nullptr, f.pnr, f.mean, f.sq, f.len, 1) == RTS_ERR_INVALID_ARG && M(f.pts, nullptr, f.mean, f.sq, f.len, 1) == RTS_ERR_INVALID_ARG && f.untouched(), "moments: NULL plane");
            CHECK(A(f.pts, f.pnr, f.out, f.len, 1) == RTS_OK && A(f.pts, f.pnr, f.out2, f.len2, 3) == RTS_OK, "plain");
            CHECK(!std::memcmp(f.out, f.out2, n * 8) && !std::memcmp(f.len, f.len2, n * 2), "plain: threads");
            if (!moved) {
                CHECK(rtsh_accumulate_visibility_list(&hard, &p, f.pos, f.nrm, nullptr, f.vis, f.prevPos, f.prevNrm, f.hist, f.lens, W, H, f.out2, f.len2, 1) == RTS_OK, "parent");
                CHECK(!std::memcmp(f.out, f.out2, n * 8) && !std::memcmp(f.len, f.len2, n * 2), "plain: anchor A at %u x %u", W, H);
            }
            CHECK(B(f.pts, f.pnr, f.out, f.len, 1) == RTS_OK && B(f.pts, f.pnr, f.out2, f.len2, 3) == RTS_OK, "clamped");
            CHECK(!std::memcmp(f.out, f.out2, n * 8) && !std::memcmp(f.len, f.len2, n * 2), "clamped: threads");
            if (!moved) {
                CHECK(rtsh_accumulate_visibility_list_clamped(&hard, &p, f.pos, f.nrm, nullptr, f.vis, f.prevPos, f.prevNrm, f.hist, f.lens, W, H, f.out2, f.len2, &clamp, 1) == RTS_OK, "parent");
                CHECK(!std::memcmp(f.out, f.out2, n * 8) && !std::memcmp(f.len, f.len2, n * 2), "clamped: anchor A at %u x %u", W, H);
            }
            CHECK(M(f.pts, f.pnr, f.mean, f.sq, f.len, 1) == RTS_OK && M(f.pts, f.pnr, f.mean2, f.sq2, f.len2, 3) == RTS_OK, "moments");
            CHECK(!std::memcmp(f.mean, f.mean2, n * 4) && !std::memcmp(f.sq, f.sq2, n * 8) && !std::memcmp(f.len, f.len2, n * 2), "moments: threads");
            if (!moved) {
                CHECK(rtsh_accumulate_moments_soft_light_list(&soft, &p, f.pos, f.nrm, nullptr, f.counts, f.prevPos, f.prevNrm, f.meanHist, f.sqHist, f.lens, W, H, f.mean2, f.sq2, f.len2, 1) == RTS_OK, "parent");
                CHECK(!std::memcmp(f.mean, f.mean2, n * 4) && !std::memcmp(f.sq, f.sq2, n * 8) && !std::memcmp(f.len, f.len2, n * 2), "moments: anchor A at %u x %u", W, H);
            }
        }
        // ---- the first frame: no history, and both motion planes may be NULL
        CHECK(rtsh_accumulate_visibility_list_motion(&hard, &p, f.pos, f.nrm, nullptr, f.vis, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, W, H, f.out, f.len, 1) == RTS_OK, "first frame");
        for (size_t i = 0; i < n * 2; ++i) CHECK(f.len[i] == (f.nrm[(i % n) * 4 + 2] != 0.0f ? 1 : 0), "first frame: length of %zu", i);
    }
    std::free(cur); std::free(old);
    std::printf("ok %lu\n", cases);
    return 0;
}
