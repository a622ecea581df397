// BVH refit on the host (rts_bvh_refit): keep a packed stream's topology, recompute its boxes and leaf data from new
// vertex positions.  Contract, byte for byte:
//   * tag and link words (.w of every node vec4) unchanged;
//   * leaf i with prim p = tag - 2N: e0 = v1 - v0, e1 = v2 - v0 in fp32 (BVHBuilder.cpp:324-341); tail p = {v0, 0};
//   * inner i: per-axis min / max over the vertices of the triangles in [i, link(i)) (END: N), taken in the total order of
//     the order-preserving integer encoding (-0.0 < +0.0), so that no reduction order can change a byte.
// This file is also the checker of the device form (rts_refit.hip) and holds the topology check both forms share.
#include "bvh_refit.h"
#include "../../include/rts.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace rts {

int refitTopology(const rts_vec4u* packed, uint32_t P, std::vector<uint32_t>* end) {
    const uint64_t N = 2 * (uint64_t)P - 1;
    if (end) end->assign((size_t)N, 0);
    if (packed[1].d != kRefitEnd) return RTS_ERR_BAD_BVH;                          // the root's link
    for (uint64_t i = 0; i < N; ++i) {
        const uint32_t tag = packed[2 * i].d, link = packed[2 * i + 1].d;
        if (link != kRefitEnd && !(link > i && link < N)) return RTS_ERR_BAD_BVH;  // strictly forward
        if (tag != kRefitEnd) {                                                     // leaf: a tail pointer, link = next node
            if (tag < 2 * N || tag >= 2 * N + P) return RTS_ERR_BAD_BVH;
            if (link != (i + 1 < N ? (uint32_t)(i + 1) : kRefitEnd)) return RTS_ERR_BAD_BVH;
        } else {                                                                    // inner: left = i + 1, right = link(left)
            if (i + 1 >= N) return RTS_ERR_BAD_BVH;
            const uint64_t left = i + 1;
            const uint32_t right = packed[2 * left + 1].d;
            if (right == kRefitEnd || right <= left || right >= N || packed[2 * (uint64_t)right + 1].d != link) return RTS_ERR_BAD_BVH;
        }
        if (end) (*end)[(size_t)i] = link == kRefitEnd ? (uint32_t)N : link;
    }
    return RTS_OK;
}

namespace {

inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline uint32_t encodeOrdered(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
inline uint32_t decodeOrdered(uint32_t e) { return (e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e; }

} // namespace

} // namespace rts

extern "C" int rts_bvh_refit(const float* vertices, size_t vertex_floats, uint32_t stride, const uint32_t* indices,
                             uint32_t P, rts_vec4u* packed, size_t count) {
    using namespace rts;
    if (!vertices || !indices || !packed || P == 0 || stride < 3 || P > 0x33333333u) return RTS_ERR_INVALID_ARG;
    if (count != (size_t)5 * P - 2) return RTS_ERR_INVALID_ARG;
    const uint32_t N = 2 * P - 1;
    // every check before the first write: a refused call leaves the blob as it was
    for (size_t k = 0; k < (size_t)3 * P; ++k)
        if ((size_t)indices[k] * stride + 3 > vertex_floats) return RTS_ERR_INVALID_ARG;
    for (size_t k = 0; k < (size_t)3 * P; ++k) {
        const float* v = vertices + (size_t)stride * indices[k];
        if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) return RTS_ERR_NONFINITE;
    }
    std::vector<uint32_t> box;
    try {
        int s = refitTopology(packed, P, nullptr);
        if (s != RTS_OK) return s;
        box.assign((size_t)N * 6, 0);                                          // encoded {min xyz, max xyz} per node
    } catch (...) {
        return RTS_ERR_CAPACITY;
    }
    // leaves and tails; inner boxes in reverse index order (in pre-order every child has a larger index than its parent)
    for (uint32_t p = 0; p < P; ++p) {
        const float* v0 = vertices + (size_t)stride * indices[(size_t)p * 3 + 0];
        packed[(size_t)2 * N + p] = rts_vec4u{ f2u(v0[0]), f2u(v0[1]), f2u(v0[2]), 0u };
    }
    for (uint32_t i = N; i-- > 0;) {
        rts_vec4u& a = packed[2 * (size_t)i];
        rts_vec4u& b = packed[2 * (size_t)i + 1];
        uint32_t* o = &box[(size_t)i * 6];
        if (a.d != kRefitEnd) {
            const uint32_t p = a.d - 2 * N;
            const float* v[3];
            for (int c = 0; c < 3; ++c) v[c] = vertices + (size_t)stride * indices[(size_t)p * 3 + c];
            a.a = f2u(v[1][0] - v[0][0]); a.b = f2u(v[1][1] - v[0][1]); a.c = f2u(v[1][2] - v[0][2]);
            b.a = f2u(v[2][0] - v[0][0]); b.b = f2u(v[2][1] - v[0][1]); b.c = f2u(v[2][2] - v[0][2]);
            for (int k = 0; k < 3; ++k) {
                uint32_t lo = 0xFFFFFFFFu, hi = 0;
                for (int c = 0; c < 3; ++c) {
                    const uint32_t e = encodeOrdered(f2u(v[c][k]));
                    lo = e < lo ? e : lo;
                    hi = e > hi ? e : hi;
                }
                o[k] = lo; o[3 + k] = hi;
            }
        } else {
            const uint32_t* l = &box[(size_t)(i + 1) * 6];
            const uint32_t* r = &box[(size_t)packed[2 * (size_t)i + 3].d * 6];   // right child = link(left)
            for (int k = 0; k < 3; ++k) {
                o[k] = l[k] < r[k] ? l[k] : r[k];
                o[3 + k] = l[3 + k] > r[3 + k] ? l[3 + k] : r[3 + k];
            }
            a.a = decodeOrdered(o[0]); a.b = decodeOrdered(o[1]); a.c = decodeOrdered(o[2]);
            b.a = decodeOrdered(o[3]); b.b = decodeOrdered(o[4]); b.c = decodeOrdered(o[5]);
        }
    }
    return RTS_OK;
}
