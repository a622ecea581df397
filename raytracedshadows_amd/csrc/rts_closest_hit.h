// Harness: closest hit of one primary ray through the packed BVH, shared verbatim by the
// host (rts_scene.cpp) and device (rts_primary.hip) G-buffer generators so that both produce the same bits.
// Stackless walk over the miss links; boxes are culled against the best t so far.  Input synthesis only -- this is
// not the path under test (the reference rasterises its G-buffer, Source/Shaders/Model.vert/.frag).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define RTS_HD __host__ __device__ inline
#else
#define RTS_HD inline
#endif

namespace rts_harness {

struct V3 { float x, y, z; };
RTS_HD V3 sub(V3 a, V3 b) { return V3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
RTS_HD V3 add(V3 a, V3 b) { return V3{ a.x + b.x, a.y + b.y, a.z + b.z }; }
RTS_HD V3 mul(V3 a, float s) { return V3{ a.x * s, a.y * s, a.z * s }; }
RTS_HD V3 cross(V3 a, V3 b) { return V3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
RTS_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
RTS_HD float asFloat(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

struct Camera { V3 eye, fwd, right, up; float tanHalf, aspect; };

struct Hit { float t; uint32_t leaf; };   // leaf = node index of the hit triangle, 0xFFFFFFFF = none

RTS_HD V3 primaryDirection(const Camera& c, uint32_t x, uint32_t y, uint32_t W, uint32_t H) {
    float sx = (((float)x + 0.5f) / (float)W * 2.0f - 1.0f) * c.tanHalf * c.aspect;
    float sy = (1.0f - ((float)y + 0.5f) / (float)H * 2.0f) * c.tanHalf;
    return add(add(c.fwd, mul(c.right, sx)), mul(c.up, sy));
}

// One triangle against the best hit so far (a = {e0, tail index}, b = {e1, next}, t = {v0}): strictly nearer hits replace it,
// so of two triangles at the same distance the one met first in depth-first order stays.
RTS_HD void leafTest(const uint32_t* a, const uint32_t* b, const uint32_t* t, uint32_t node, V3 o, V3 d, Hit* best) {
    V3 e0{ asFloat(a[0]), asFloat(a[1]), asFloat(a[2]) }, e1{ asFloat(b[0]), asFloat(b[1]), asFloat(b[2]) };
    V3 v0{ asFloat(t[0]), asFloat(t[1]), asFloat(t[2]) };
    V3 s1 = cross(d, e1);
    float det = dot(s1, e0);
    if (det != 0.0f) {
        float invd = 1.0f / det;
        V3 dd = sub(o, v0);
        float b1 = dot(dd, s1) * invd;
        V3 s2 = cross(dd, e0);
        float b2 = dot(d, s2) * invd;
        float tt = dot(e1, s2) * invd;
        if (b1 >= 0.0f && b2 >= 0.0f && b1 + b2 <= 1.0f && tt > 0.0f && tt < best->t) { best->t = tt; best->leaf = node; }
    }
}

// Slab test of an inner node (a = {bboxMin, -}, b = {bboxMax, next}) against [0, best t].
RTS_HD bool boxTest(const uint32_t* a, const uint32_t* b, V3 o, V3 inv, float bestT) {
    float lo[3] = { asFloat(a[0]), asFloat(a[1]), asFloat(a[2]) }, hi[3] = { asFloat(b[0]), asFloat(b[1]), asFloat(b[2]) };
    float oo[3] = { o.x, o.y, o.z }, ii[3] = { inv.x, inv.y, inv.z };
    float t0 = 0.0f, t1 = bestT;
    for (int k = 0; k < 3; ++k) {
        float f = (hi[k] - oo[k]) * ii[k], n = (lo[k] - oo[k]) * ii[k];
        float mx = f > n ? f : n, mn = f > n ? n : f;
        if (mx < t1) t1 = mx;      // NaN (0*inf) compares false: the slab is ignored
        if (mn > t0) t0 = mn;
    }
    return t1 >= t0;
}

RTS_HD Hit closestHit(const uint32_t* bvh, V3 o, V3 d) {
    const float inf = asFloat(0x7F800000u);
    const V3 inv{ 1.0f / d.x, 1.0f / d.y, 1.0f / d.z };
    Hit best{ inf, 0xFFFFFFFFu };
    uint32_t node = 0;
    while (node != 0xFFFFFFFFu) {
        const uint32_t* a = bvh + (size_t)node * 8;
        const uint32_t* b = a + 4;
        if (a[3] != 0xFFFFFFFFu) {
            leafTest(a, b, bvh + (size_t)a[3] * 4, node, o, d, &best);
        } else if (boxTest(a, b, o, inv, best.t)) {
            ++node;
            continue;
        }
        node = b[3];
    }
    return best;
}

// G-buffer texel: camera-relative position (Model.frag:39) and the face normal turned towards the viewer
// (Model.frag:38 `gl_FrontFacing ? n : -n`; the harness has no vertex normals, so the geometric one is used).
RTS_HD void writeTexel(const uint32_t* bvh, V3 d, Hit h, float* position4, float* normal4) {
    if (h.leaf == 0xFFFFFFFFu) {
        position4[0] = position4[1] = position4[2] = position4[3] = 0.0f;       // clear value (background)
        if (normal4) normal4[0] = normal4[1] = normal4[2] = normal4[3] = 0.0f;
        return;
    }
    V3 rel = mul(d, h.t);
    position4[0] = rel.x; position4[1] = rel.y; position4[2] = rel.z; position4[3] = 1.0f;
    if (normal4) {
        const uint32_t* a = bvh + (size_t)h.leaf * 8;
        V3 e0{ asFloat(a[0]), asFloat(a[1]), asFloat(a[2]) }, e1{ asFloat(a[4]), asFloat(a[5]), asFloat(a[6]) };
        V3 n = cross(e0, e1);
        float len2 = dot(n, n);
        float s = len2 > 0.0f ? 1.0f / __builtin_sqrtf(len2) : 0.0f;
        if (dot(n, d) > 0.0f) s = -s;
        normal4[0] = n.x * s; normal4[1] = n.y * s; normal4[2] = n.z * s; normal4[3] = 0.0f;
    }
}

RTS_HD void shadePixel(const uint32_t* bvh, const Camera& c, uint32_t x, uint32_t y, uint32_t W, uint32_t H,
                       float* position4, float* normal4) {
    V3 d = primaryDirection(c, x, y, W, H);
    writeTexel(bvh, d, closestHit(bvh, c.eye, d), position4, normal4);
}

// The MOTION G-buffer texels (include/rts_scene.h, rtsh_primary_gbuffer_motion): beside writeTexel's two, where the seen surface point
// was in the previous frame -- relative to the previous eye -- and that surface's normal then.  `prev` is the previous frame's stream, a
// refit sibling of `bvh`: the same node indices.  The nine words of the hit leaf (e0, e1 and the tail's v0) are read at the SAME word
// indices of both streams, the tail index from the CURRENT stream alone, so a `prev` of the right size is never read out of bounds.
//   STATIC (the nine words are bit-identical): position + eyeDelta, .w = 1, and the current normal's bits -- 4.23's Q.
//   MOVED: b1, b2 by leafTest's own expressions on the current leaf, then (v0' + (e0' * b1 + e1' * b2)) - prevEye per component, .w = 2;
//          the normal of (e0', e1') turned to the side writeTexel chose for the CURRENT normal.
// position4 / normal4: what writeTexel wrote for this pixel (the normal always, whether or not the caller keeps it).
RTS_HD void writeMotionTexel(const uint32_t* bvh, const uint32_t* prev, V3 o, V3 prevEye, V3 eyeDelta, V3 d, Hit h, const float* position4,
                             const float* normal4, float* prevPoint4, float* prevNormal4) {
    if (h.leaf == 0xFFFFFFFFu) {
        prevPoint4[0] = prevPoint4[1] = prevPoint4[2] = prevPoint4[3] = 0.0f;
        prevNormal4[0] = prevNormal4[1] = prevNormal4[2] = prevNormal4[3] = 0.0f;
        return;
    }
    const size_t leafWord = (size_t)h.leaf * 8;
    const size_t tailWord = (size_t)bvh[leafWord + 3] * 4;                   // (the CURRENT stream's index)
    uint32_t cw[9], pw[9];
    bool moved = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 9; ++k) {
        const size_t i = k < 3 ? leafWord + (size_t)k : (k < 6 ? leafWord + 4 + (size_t)(k - 3) : tailWord + (size_t)(k - 6));
        cw[k] = bvh[i];
        pw[k] = prev[i];
        moved |= cw[k] != pw[k];
    }
    if (!moved) {
        prevPoint4[0] = position4[0] + eyeDelta.x; prevPoint4[1] = position4[1] + eyeDelta.y; prevPoint4[2] = position4[2] + eyeDelta.z;
        prevPoint4[3] = 1.0f;
        prevNormal4[0] = normal4[0]; prevNormal4[1] = normal4[1]; prevNormal4[2] = normal4[2]; prevNormal4[3] = normal4[3];
        return;
    }
    const V3 e0{ asFloat(cw[0]), asFloat(cw[1]), asFloat(cw[2]) }, e1{ asFloat(cw[3]), asFloat(cw[4]), asFloat(cw[5]) };
    const V3 v0{ asFloat(cw[6]), asFloat(cw[7]), asFloat(cw[8]) };
    const V3 pe0{ asFloat(pw[0]), asFloat(pw[1]), asFloat(pw[2]) }, pe1{ asFloat(pw[3]), asFloat(pw[4]), asFloat(pw[5]) };
    const V3 pv0{ asFloat(pw[6]), asFloat(pw[7]), asFloat(pw[8]) };
    const V3 s1 = cross(d, e1);                                              // leafTest's expressions, in its order
    const float det = dot(s1, e0);
    const float invd = 1.0f / det;
    const V3 dd = sub(o, v0);
    const float b1 = dot(dd, s1) * invd;
    const V3 s2 = cross(dd, e0);
    const float b2 = dot(d, s2) * invd;
    prevPoint4[0] = (pv0.x + (pe0.x * b1 + pe1.x * b2)) - prevEye.x;
    prevPoint4[1] = (pv0.y + (pe0.y * b1 + pe1.y * b2)) - prevEye.y;
    prevPoint4[2] = (pv0.z + (pe0.z * b1 + pe1.z * b2)) - prevEye.z;
    prevPoint4[3] = 2.0f;
    const V3 n = cross(e0, e1), pn = cross(pe0, pe1);
    const float len2 = dot(pn, pn);
    float s = len2 > 0.0f ? 1.0f / __builtin_sqrtf(len2) : 0.0f;
    if (dot(n, d) > 0.0f) s = -s;                                            // writeTexel's side of the CURRENT triangle
    prevNormal4[0] = pn.x * s; prevNormal4[1] = pn.y * s; prevNormal4[2] = pn.z * s; prevNormal4[3] = 0.0f;
}

RTS_HD void shadeMotionPixel(const uint32_t* bvh, const uint32_t* prev, const Camera& c, V3 prevEye, V3 eyeDelta, uint32_t x, uint32_t y,
                             uint32_t W, uint32_t H, float* position4, float* normal4, float* prevPoint4, float* prevNormal4,
                             uint32_t* leaf) {
    const V3 d = primaryDirection(c, x, y, W, H);
    const Hit h = closestHit(bvh, c.eye, d);
    float n4[4];
    writeTexel(bvh, d, h, position4, n4);
    if (normal4) { normal4[0] = n4[0]; normal4[1] = n4[1]; normal4[2] = n4[2]; normal4[3] = n4[3]; }
    writeMotionTexel(bvh, prev, c.eye, prevEye, eyeDelta, d, h, position4, n4, prevPoint4, prevNormal4);
    if (leaf) *leaf = h.leaf;
}

// Combine.frag:18-37 with baseColor = 1 (the default white material, RayTracedShadows.cpp:1013-1018), one pixel:
//   direct  = 1.25 * max(0, N.L) * shadowMask            shadowMask = mask / samples
//   ambient = 0.15 + 0.05 * (1 - max(0, N.(-cameraDirection)))
//   pixel discarded (left 0) where the normal is 0 (background)
//   max(0, x) = x > 0 ? x : 0, as GLSL defines it: a NaN N.L or N.V contributes 0 (the ambient term stays)
//   byte = 255 where scaled >= 255, int(scaled) where 0 < scaled < 255, 0 otherwise (NaN included); scaled = value * 255 + 0.5
// L = the light direction for a directional light; for the point-light extension L = normalize(light - P).
struct CombineParams { V3 cam, viewDir /* normalised */, light; uint32_t pointLight; float samples; };

// N.L as the combine pass takes it, before the clamp (frag:24-29): the one value both combinePixel and the facing mark
// (facingPixel) decide on, so that the mark can never cull a pixel the combine pass would have lit.
RTS_HD float facingNdl(const CombineParams& c, const float* position4, V3 n) {
    V3 L = c.light;
    if (c.pointLight) {
        V3 p{ c.cam.x + position4[0], c.cam.y + position4[1], c.cam.z + position4[2] };
        L = sub(L, p);
        float ll = __builtin_sqrtf(dot(L, L));
        if (ll > 0) L = mul(L, 1.0f / ll);
    }
    return dot(n, L);
}

// combinePixel's pieces, shared with the light list rule below (combineListPixel).
RTS_HD float clamp0(float x) { return x > 0 ? x : 0.0f; }                                        // GLSL's max(0.0, x): 0 for a NaN
RTS_HD float viewNdv(const CombineParams& c, V3 n) { return dot(n, mul(c.viewDir, -1.0f)); }
RTS_HD float combineDirect(float ndl, uint8_t mask, float samples) { return 1.25f * ndl * ((float)mask / samples); }   // frag:29
RTS_HD float combineAmbient(float ndv) { return 0.15f + 0.05f * (1.0f - ndv); }                 // frag:30
// UNORM8, saturated in float BEFORE the conversion: converting a float outside int's range (a normal of 1e7, +Inf, a NaN from
// Inf * 0) is undefined on the host, and the host and the device then disagree.  A NaN is 0.
RTS_HD uint8_t combineByte(float v) {
    const float scaled = v * 255.0f + 0.5f;
    return scaled >= 255.0f ? (uint8_t)255 : (scaled > 0.0f ? (uint8_t)(int)scaled : (uint8_t)0);
}

RTS_HD uint8_t combinePixel(const CombineParams& c, const float* position4, const float* normal4, uint8_t mask) {
    V3 n{ normal4[0], normal4[1], normal4[2] };
    if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) return 0;
    const float ndl = clamp0(facingNdl(c, position4, n));
    const float ndv = clamp0(viewNdv(c, n));
    const float direct = combineDirect(ndl, mask, c.samples);
    const float ambient = combineAmbient(ndv);
    return combineByte(direct + ambient);                                   // frag:32 (baseColor = 1)
}

// The combine pass of a LIGHT LIST (include/rts_scene.h, rtsh_combine_light_list / rtsh_combine_soft_light_list), one pixel: the
// lights' direct terms, each times its colour, summed in list order from +0, plus ONE ambient term --
//   rgb[c] = byte(((0 + direct_0 * color_0[c]) + direct_1 * color_1[c] + ...) + ambient),   direct_l = combinePixel's for light l alone
// over its own byte (byteOf(l): the count plane's byte, or the mask's bit as 0 / 1).  A light whose bit of `bits` (the light map's byte)
// is clear adds nothing and byteOf is not asked for it; a background pixel is 0 and nothing but the normal is looked at.  Every product
// and every sum is rounded on its own (no contraction), in this order, on the host and on the device.
struct CombineList { uint32_t count; CombineParams light[8]; float color[8][3]; };

template <class ByteOf>
RTS_HD void combineListPixel(const CombineList& f, const float* position4, const float* normal4, uint32_t bits, ByteOf byteOf,
                             uint8_t* rgb3) {
    V3 n{ normal4[0], normal4[1], normal4[2] };
    if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) { rgb3[0] = rgb3[1] = rgb3[2] = 0; return; }
    const float ambient = combineAmbient(clamp0(viewNdv(f.light[0], n)));     // (camera and view direction: the same in every entry)
    float sum[3] = { 0.0f, 0.0f, 0.0f };
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        if (!((bits >> l) & 1u)) continue;
        const float direct = combineDirect(clamp0(facingNdl(f.light[l], position4, n)), byteOf(l), f.light[l].samples);
        for (int c = 0; c < 3; ++c) sum[c] = sum[c] + direct * f.color[l][c];
    }
    for (int c = 0; c < 3; ++c) rgb3[c] = combineByte(sum[c] + ambient);
}

// The VISIBILITY combine (include/rts_scene.h, rtsh_combine_visibility_list): combineListPixel with a float visibility per light --
// what the filter below writes -- in place of (float)byte / samples; everything else, the order of the sum included, is the same, so
// over the quotients of an R = 0 filter it gives combineListPixel's bytes.
// ambientOf(ambient): the ambient term as it enters the sum -- itself, or times the pixel's ambient occlusion (rtsh_combine_visibility_
// list_ao: ONE rounded multiply, asked for on non-background pixels only).
// ambient3Of(ambient, out3): the PER-CHANNEL form of the same -- the ambient term of each channel as it enters that channel's sum
// (rtsh_combine_visibility_list_ao_bent: the sky tint); the one-value forms hand every channel the same float.
template <class VisibilityOf, class Ambient3Of>
RTS_HD void combineVisibilityPixelRgb(const CombineList& f, const float* position4, const float* normal4, uint32_t bits,
                                      VisibilityOf visibilityOf, Ambient3Of ambient3Of, uint8_t* rgb3) {
    V3 n{ normal4[0], normal4[1], normal4[2] };
    if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) { rgb3[0] = rgb3[1] = rgb3[2] = 0; return; }
    float ambient[3];
    ambient3Of(combineAmbient(clamp0(viewNdv(f.light[0], n))), ambient);
    float sum[3] = { 0.0f, 0.0f, 0.0f };
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        if (!((bits >> l) & 1u)) continue;
        const float direct = 1.25f * clamp0(facingNdl(f.light[l], position4, n)) * visibilityOf(l);
        for (int c = 0; c < 3; ++c) sum[c] = sum[c] + direct * f.color[l][c];
    }
    for (int c = 0; c < 3; ++c) rgb3[c] = combineByte(sum[c] + ambient[c]);
}
template <class VisibilityOf, class AmbientOf>
RTS_HD void combineVisibilityPixel(const CombineList& f, const float* position4, const float* normal4, uint32_t bits,
                                   VisibilityOf visibilityOf, AmbientOf ambientOf, uint8_t* rgb3) {
    combineVisibilityPixelRgb(f, position4, normal4, bits, visibilityOf,
                              [&](float ambient, float* out3) { out3[0] = out3[1] = out3[2] = ambientOf(ambient); }, rgb3);
}
template <class VisibilityOf>
RTS_HD void combineVisibilityPixel(const CombineList& f, const float* position4, const float* normal4, uint32_t bits,
                                   VisibilityOf visibilityOf, uint8_t* rgb3) {
    combineVisibilityPixel(f, position4, normal4, bits, visibilityOf, [](float ambient) { return ambient; }, rgb3);
}

// The FILTER of a light list's planes (include/rts_scene.h, rtsh_filter_light_list / rtsh_filter_soft_light_list), one pixel: a
// (2R+1) x (2R+1) window of integer tent weights over the taps that pass the geometry test (normal and plane distance, once per
// tap) and, per light, the map bit and -- with distances -- the spread test.  num and den are integer sums (< 2^24), so no order of
// the taps can change them; the floats are per-tap comparisons, each written so that a NaN rejects, and one division per light.
// `Texels` gives the frame by pixel coordinates (the host twin reads the buffers, the kernel its LDS tile):
//   V3 normal(x, y), V3 position(x, y); uint32_t bits(x, y) (the map byte, 0xFF without a map); uint32_t byte(x, y, l) (the count
//   byte, or the mask's bit as 0 / 1); uint32_t distance(x, y, l) (the bit pattern; DIST only).
// `walk`: the lights whose taps are walked.  A light outside it takes the centre tap alone -- (float)c / (float)n, which is also what
// the walk gives wherever every accepted tap carries the centre's byte (the weights cancel, the quotient is rounded once): the kernel
// clears a light's bit for a block whose staged window holds one byte for that light.  The host twin walks every light.
struct FilterList { uint32_t count, radius; float normalCosMin, planeEps; uint32_t samples[8]; float spread[8]; };

RTS_HD bool isBackground(V3 n) { return n.x == 0.0f && n.y == 0.0f && n.z == 0.0f; }

template <bool DIST, class Texels>
RTS_HD void filterListPixel(const FilterList& f, const Texels& t, int x, int y, int W, int H, uint32_t walk, float* visibility8) {
    const V3 np = t.normal(x, y);
    const uint32_t onp = isBackground(np) ? 0u : (t.bits(x, y) & ((1u << f.count) - 1u));
    const int R = (int)f.radius;
    const uint32_t w0 = (uint32_t)((R + 1) * (R + 1));
    uint32_t num[8], den[8], dp[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        num[l] = den[l] = dp[l] = 0u;
        if (l >= f.count || !((onp >> l) & 1u)) continue;
        num[l] = w0 * t.byte(x, y, l);                                            // the centre tap: always accepted
        den[l] = w0 * f.samples[l];
        if (DIST) dp[l] = t.distance(x, y, l);
    }
    const uint32_t todo = onp & walk;
    if (todo != 0u && R > 0) {
        const V3 pp = t.position(x, y);
        for (int dy = -R; dy <= R; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= H) continue;
            const uint32_t wy = (uint32_t)(R + 1 - (dy < 0 ? -dy : dy));
            for (int dx = -R; dx <= R; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= W || (dx == 0 && dy == 0)) continue;
                const V3 nq = t.normal(qx, qy);
                if (isBackground(nq)) continue;
                if (!((np.x * nq.x + np.y * nq.y) + np.z * nq.z >= f.normalCosMin)) continue;
                const V3 d = sub(t.position(qx, qy), pp);
                const float h = (np.x * d.x + np.y * d.y) + np.z * d.z;
                if (!(__builtin_fabsf(h) <= f.planeEps)) continue;
                const uint32_t acc = t.bits(qx, qy) & todo;
                if (acc == 0u) continue;
                const float d2 = (d.x * d.x + d.y * d.y) + d.z * d.z;
                const uint32_t w = wy * (uint32_t)(R + 1 - (dx < 0 ? -dx : dx));
#if defined(__HIPCC__)
#pragma unroll
#endif
                for (uint32_t l = 0; l < 8; ++l) {
                    if (l >= f.count) break;
                    if (!((acc >> l) & 1u)) continue;
                    if (DIST) {
                        const uint32_t dq = t.distance(qx, qy, l);
                        const uint32_t m = dq < dp[l] ? dq : dp[l];
                        if (m != 0x7F800000u) {
                            const float sm = f.spread[l] * asFloat(m);
                            if (!(d2 <= sm * sm)) continue;
                        }
                    }
                    num[l] += w * t.byte(qx, qy, l);
                    den[l] += w * f.samples[l];
                }
            }
        }
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        visibility8[l] = ((onp >> l) & 1u) ? (float)num[l] / (float)den[l] : 0.0f;
    }
}

// The WIDE FILTER of a light list's planes (include/rts_scene.h, rtsh_wide_filter_light_list / rtsh_wide_filter_soft_light_list), ONE
// PASS at one pixel: the 5 x 5 taps `step` pixels apart, integer weights b[|dx|] * b[|dy|] with b = {6, 4, 1}, over the taps that pass
// wideFilterGeom (once per tap) and, per light, the map bit; num and den are integer sums (num <= 65535 * 256), the result is the rounded
// mean (2 * num + den) / (2 * den) as a 16-bit value, 0 at an inactive pixel.  step == 0 walks no tap: the centre's own value (the
// passes == 0 form).  `Texels` gives the frame by pixel coordinates (the host twin reads the buffers, the kernel its LDS tile or the
// buffers): V3 normal(x, y), V3 position(x, y); uint32_t bits(x, y) (the map byte, 0xFF without a map); uint32_t value(x, y, l): V_k --
// for the first pass wideFilterInput of the count byte (or of the mask's bit), later the previous pass's plane.
// geom(p, q) of the header for a tap q inside the frame: not background, the normal test, the plane test, each comparison written so that
// a NaN rejects; the position of a background tap or of one the normal test rejects is never looked at.  A COPY of filterListPixel's
// expression, operation for operation: calling this from filterListPixel changed the instruction text of filterListKernel<false, true>
// (the spread test reads D again), and that kernel keeps its text.
template <class Texels>
RTS_HD bool wideFilterGeom(const Texels& t, V3 np, V3 pp, int qx, int qy, float normalCosMin, float planeEps) {
    const V3 nq = t.normal(qx, qy);
    if (isBackground(nq)) return false;
    if (!((np.x * nq.x + np.y * nq.y) + np.z * nq.z >= normalCosMin)) return false;
    const V3 d = sub(t.position(qx, qy), pp);
    const float h = (np.x * d.x + np.y * d.y) + np.z * d.z;
    return __builtin_fabsf(h) <= planeEps;
}

struct WideFilterList { uint32_t count, passes; float normalCosMin, planeEps; uint32_t samples[8], scale[8]; };   // n_l, S_l

RTS_HD uint32_t wideFilterScale(uint32_t samples) { return 65535u / samples; }                            // S_l
RTS_HD uint32_t wideFilterInput(uint32_t byte, uint32_t samples, uint32_t scale) { return (byte < samples ? byte : samples) * scale; }   // V_0
// visibility = (float)V / (float)(n_l * S_l): one rounded division
RTS_HD float wideFilterOutput(uint32_t v, uint32_t samples, uint32_t scale) { return (float)v / (float)(samples * scale); }

template <class Texels>
RTS_HD void wideFilterPassPixel(const WideFilterList& f, const Texels& t, int x, int y, int W, int H, int step, uint32_t* value8) {
    const V3 np = t.normal(x, y);
    const uint32_t onp = isBackground(np) ? 0u : (t.bits(x, y) & ((1u << f.count) - 1u));
    uint32_t num[8], den[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        num[l] = 0u; den[l] = 1u;
        if (l >= f.count || !((onp >> l) & 1u)) continue;
        num[l] = 36u * t.value(x, y, l);                                          // the centre tap: always accepted
        den[l] = 36u;
    }
    if (onp != 0u && step > 0) {
        const V3 pp = t.position(x, y);
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + dy * step;
            if (qy < 0 || qy >= H) continue;
            const uint32_t wy = dy == 0 ? 6u : ((dy == 1 || dy == -1) ? 4u : 1u);
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + dx * step;
                if (qx < 0 || qx >= W || (dx == 0 && dy == 0)) continue;
                if (!wideFilterGeom(t, np, pp, qx, qy, f.normalCosMin, f.planeEps)) continue;
                const uint32_t acc = t.bits(qx, qy) & onp;
                if (acc == 0u) continue;
                const uint32_t w = wy * (dx == 0 ? 6u : ((dx == 1 || dx == -1) ? 4u : 1u));
#if defined(__HIPCC__)
#pragma unroll
#endif
                for (uint32_t l = 0; l < 8; ++l) {
                    if (l >= f.count) break;
                    if (!((acc >> l) & 1u)) continue;
                    num[l] += w * t.value(qx, qy, l);
                    den[l] += w;
                }
            }
        }
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        value8[l] = ((onp >> l) & 1u) ? (2u * num[l] + den[l]) / (2u * den[l]) : 0u;
    }
}

// The WIDE FILTER OF THE BENT PLANE (include/rts_scene.h, rtsh_wide_filter_bent): the pass above over one texel of FOUR
// 16-bit integers -- the bent vector's components, signed, in units of 1 / S_b, and V of the count, unsigned, in units of 1 / S_l --,
// one geometry test and one `active` byte per tap for all four.  The three small rules (quantise, rounded signed mean, quotient) and the
// texel's packing are the source of the host twin and of the kernels alike.
struct BentFilterList { uint32_t passes, samples, scaleB, scaleL; float normalCosMin, planeEps; };       // n, S_b, S_l
struct BentTexel { int32_t x, y, z; uint32_t v; };                                                      // each fits 16 bits

RTS_HD uint32_t bentFilterScale(uint32_t samples) { return 32767u / samples; }                            // S_b
// X_0.c: one rounded multiply, a NaN is 0, the clamp to +-(n * S_b), rint (ties to even)
RTS_HD int32_t bentFilterQuantise(float c, uint32_t samples, uint32_t scaleB) {
    const float t = c * (float)scaleB;
    if (t != t) return 0;
    const float lim = (float)(samples * scaleB);
    return (int32_t)__builtin_rintf(t < -lim ? -lim : (t > lim ? lim : t));
}
// V_0 from bent.w: a NaN is 0, the clamp to [0, n], rint, times S_l -- wideFilterInput of the count wherever .w is that count
RTS_HD uint32_t bentFilterCount(float w, uint32_t samples, uint32_t scaleL) {
    if (w != w) return 0u;
    const float lim = (float)samples;
    return (uint32_t)(int32_t)__builtin_rintf(w < 0.0f ? 0.0f : (w > lim ? lim : w)) * scaleL;
}
// the rounded mean of a signed sum, half away from zero: the mean of the negated values is the negated mean
RTS_HD int32_t bentFilterMean(int32_t num, uint32_t den) {
    const uint32_t a = num < 0 ? (uint32_t)(-num) : (uint32_t)num;
    const int32_t q = (int32_t)((2u * a + den) / (2u * den));
    return num < 0 ? -q : q;
}
// out.c = (float)X.c / (float)(n * S_b): one rounded division; a zero numerator gives +0
RTS_HD float bentFilterOutput(int32_t x, uint32_t samples, uint32_t scaleB) { return (float)x / (float)(samples * scaleB); }

// The 8-byte texel between passes: int16 x, y, z and uint16 V, lowest bits first; unpacked with integer operations alone.
RTS_HD uint64_t bentFilterPack(const BentTexel& t) {
    return (uint64_t)((uint32_t)t.x & 0xFFFFu) | ((uint64_t)((uint32_t)t.y & 0xFFFFu) << 16) | ((uint64_t)((uint32_t)t.z & 0xFFFFu) << 32) |
           ((uint64_t)(t.v & 0xFFFFu) << 48);
}
RTS_HD BentTexel bentFilterUnpack(uint64_t u) {
    const uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
    return BentTexel{ (int32_t)(int16_t)(uint16_t)(lo & 0xFFFFu), (int32_t)(int16_t)(uint16_t)(lo >> 16), (int32_t)(int16_t)(uint16_t)(hi & 0xFFFFu),
                      hi >> 16 };
}
RTS_HD BentTexel bentFilterInput(float bx, float by, float bz, float bw, const BentFilterList& f) {
    return BentTexel{ bentFilterQuantise(bx, f.samples, f.scaleB), bentFilterQuantise(by, f.samples, f.scaleB),
                      bentFilterQuantise(bz, f.samples, f.scaleB), bentFilterCount(bw, f.samples, f.scaleL) };
}

// One pass at one pixel.  `Texels`: V3 normal(x, y), V3 position(x, y); bool active(x, y) (the byte, true without a plane);
// BentTexel texel(x, y): X_k and V_k -- the first pass's from bentFilterInput of the float texel, later the unpacked 8 bytes.  Returns
// whether the pixel is active; an inactive pixel gets four zeros and reads nothing beyond its normal and its byte.  A tap's byte is
// looked at before its geometry (the verdict is the conjunction either way; the byte is the cheaper read).  step == 0 walks no tap.
template <class Texels>
RTS_HD bool bentFilterPassPixel(const BentFilterList& f, const Texels& t, int x, int y, int W, int H, int step, BentTexel* result) {
    const V3 np = t.normal(x, y);
    *result = BentTexel{ 0, 0, 0, 0u };
    if (isBackground(np) || !t.active(x, y)) return false;
    const BentTexel c = t.texel(x, y);
    int32_t sx = 36 * c.x, sy = 36 * c.y, sz = 36 * c.z;                            // the centre tap: always accepted
    uint32_t sv = 36u * c.v, den = 36u;
    if (step > 0) {
        const V3 pp = t.position(x, y);
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + dy * step;
            if (qy < 0 || qy >= H) continue;
            const int32_t wy = dy == 0 ? 6 : ((dy == 1 || dy == -1) ? 4 : 1);
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + dx * step;
                if (qx < 0 || qx >= W || (dx == 0 && dy == 0)) continue;
                if (!t.active(qx, qy)) continue;
                if (!wideFilterGeom(t, np, pp, qx, qy, f.normalCosMin, f.planeEps)) continue;
                const int32_t w = wy * (dx == 0 ? 6 : ((dx == 1 || dx == -1) ? 4 : 1));
                const BentTexel q = t.texel(qx, qy);
                sx += w * q.x; sy += w * q.y; sz += w * q.z;                        // |sum| <= 256 * 32767 < 2^23
                sv += (uint32_t)w * q.v; den += (uint32_t)w;
            }
        }
    }
    *result = BentTexel{ bentFilterMean(sx, den), bentFilterMean(sy, den), bentFilterMean(sz, den), (2u * sv + den) / (2u * den) };
    return true;
}

// The VARIANCE-GUIDED wide filter of a soft light list's planes (include/rts_scene.h, rtsh_wide_filter_guided_soft_light_list): the
// threshold T(p, l) of the header from the 3 x 3 neighbourhood of V_0, and one pass that accepts a tap for light l only where
// |V_k(q, l) - V_k(p, l)| <= T(p, l).  Integers throughout, so header, host twin, numpy rule and kernels agree bit for bit.
//
// T = min(65535, isqrt((k4^2 * G) / (16 * D * n))) WITHOUT the 64-bit division: for integers r, N and d > 0, r * r <= N / d (the
// integer quotient) exactly when r * r * d <= N, so T is the largest r <= 65535 with r * r * d <= N -- a float estimate, then an integer
// fix-up in 64 bits (r * r * d < 2^49) that makes it exact whatever the estimate's rounding: the same source on host and device.
RTS_HD uint32_t wideGuideThreshold(uint64_t G, uint32_t D, uint32_t samples, uint32_t k4) {
    const uint64_t N = (uint64_t)(k4 * k4) * G;                                  // < 2^16 * 2^35
    const uint64_t d = (uint64_t)(16u * D * samples);                            // 128 .. 16 * 16 * 48
    const float est = __builtin_sqrtf((float)N / (float)d);
    uint32_t r = est < 65535.0f ? (uint32_t)est : 65535u;
    while ((uint64_t)r * r * d > N) --r;
    while (r < 65535u && (uint64_t)(r + 1u) * (r + 1u) * d <= N) ++r;
    return r;
}

// T(p, l) for every light of the list at pixel (x, y); `t` gives V_0.  The 3 x 3 pixels inside the frame, not background, with the
// light's map bit -- NO geom test (the header says why) --, weights {1, 2, 1} x {1, 2, 1}; a light of one sample gets 65535 (every tap
// passes: the unguided filter), a light that is not on at p gets 0 (its value is 0 whatever the taps).
template <class Texels>
RTS_HD void wideGuideThresholdPixel(const WideFilterList& f, uint32_t k4, const Texels& t, int x, int y, int W, int H, uint32_t* T8) {
    const uint32_t onp = isBackground(t.normal(x, y)) ? 0u : (t.bits(x, y) & ((1u << f.count) - 1u));
    uint32_t nb[9];                                                              // the map bits of the nine pixels that count
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 9; ++j) {
        const int qx = x + j % 3 - 1, qy = y + j / 3 - 1;
        nb[j] = 0u;
        if (onp == 0u || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        nb[j] = j == 4 ? onp : (isBackground(t.normal(qx, qy)) ? 0u : t.bits(qx, qy));
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        T8[l] = 0u;
        if (!((onp >> l) & 1u)) continue;
        T8[l] = 65535u;
        if (f.samples[l] < 2u) continue;
        const uint32_t full = f.samples[l] * f.scale[l];                         // n_l * S_l
        uint64_t G = 0;
        uint32_t D = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 9; ++j) {
            if (!((nb[j] >> l) & 1u)) continue;
            const uint32_t w = (j % 3 == 1 ? 2u : 1u) * (j / 3 == 1 ? 2u : 1u);
            const uint32_t v = t.value(x + j % 3 - 1, y + j / 3 - 1, l);
            G += (uint64_t)w * (uint64_t)(v * (full - v));                       // E = V_0 * (n S - V_0) < 2^30
            D += w;
        }
        T8[l] = wideGuideThreshold(G, D, f.samples[l], k4);
    }
}

// One guided pass at one pixel: wideFilterPassPixel with the per-light test of the tap's value against the centre's (T8: T(p, l)).
template <class Texels>
RTS_HD void wideGuidedPassPixel(const WideFilterList& f, const Texels& t, int x, int y, int W, int H, int step, const uint32_t* T8,
                                uint32_t* value8) {
    const V3 np = t.normal(x, y);
    const uint32_t onp = isBackground(np) ? 0u : (t.bits(x, y) & ((1u << f.count) - 1u));
    uint32_t num[8], den[8], ctr[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        num[l] = 0u; den[l] = 1u; ctr[l] = 0u;
        if (l >= f.count || !((onp >> l) & 1u)) continue;
        ctr[l] = t.value(x, y, l);
        num[l] = 36u * ctr[l];                                                    // the centre tap: always accepted
        den[l] = 36u;
    }
    if (onp != 0u && step > 0) {
        const V3 pp = t.position(x, y);
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + dy * step;
            if (qy < 0 || qy >= H) continue;
            const uint32_t wy = dy == 0 ? 6u : ((dy == 1 || dy == -1) ? 4u : 1u);
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + dx * step;
                if (qx < 0 || qx >= W || (dx == 0 && dy == 0)) continue;
                if (!wideFilterGeom(t, np, pp, qx, qy, f.normalCosMin, f.planeEps)) continue;
                const uint32_t acc = t.bits(qx, qy) & onp;
                if (acc == 0u) continue;
                const uint32_t w = wy * (dx == 0 ? 6u : ((dx == 1 || dx == -1) ? 4u : 1u));
#if defined(__HIPCC__)
#pragma unroll
#endif
                for (uint32_t l = 0; l < 8; ++l) {
                    if (l >= f.count) break;
                    if (!((acc >> l) & 1u)) continue;
                    const uint32_t v = t.value(qx, qy, l);
                    if ((v > ctr[l] ? v - ctr[l] : ctr[l] - v) > T8[l]) continue;  // the guide
                    num[l] += w * v;
                    den[l] += w;
                }
            }
        }
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        value8[l] = ((onp >> l) & 1u) ? (2u * num[l] + den[l]) / (2u * den[l]) : 0u;
    }
}

// The TEMPORAL ACCUMULATION of a light list's visibility (include/rts_scene.h, rtsh_accumulate_visibility_list), one pixel: reproject
// through the previous camera onto a 1/32-pixel grid, four bilinear taps of INTEGER weights (they sum to 1024), each accepted by the
// geometry (inside the frame, not background, normal, plane distance: once per tap, a 4-bit mask) and per light by its history length;
// then one division, one reciprocal and one lerp per light.  Every float step is one rounded operation in the order the header states;
// every comparison is written so that a NaN rejects.  A tap of weight 0 or a rejected tap is never loaded: a still camera costs one
// gather per light.  `Frames` gives both frames by pixel coordinates (the host twin reads the buffers, the kernel reads them with its
// own cache policy):
//   V3 normal(x, y), position(x, y); uint32_t bits(x, y) (the map byte, 0xFF without a map); uint32_t current(l, x, y) (the BITS of
//   visibility[l][p]); V3 prevNormal(x, y), prevPosition(x, y); uint32_t prevLength(l, x, y); float prevVisibility(l, x, y);
//   void store(l, x, y, uint32_t visibilityBits, uint32_t length).
// A blended value that is a NaN is stored as 0x7FC00000: which NaN an operation returns is the one thing the machines disagree on.
// CLAMPED (rtsh_accumulate_visibility_list_clamped): one step between `prev` and the lerp, compiled in by the switch alone -- the
// unclamped instantiation is the text it was.  `Frames` then also gives
//   bool box(l, x, y, uint32_t* loKey, uint32_t* hiKey): the smallest and largest clampKey over the contributing taps of the pixel's
//   window for light l; false when no tap contributes.  The host twin loops over the window, the kernel reduces it in LDS: a minimum
//   and a maximum of integers, so no order of taps can change a bit.
// MOTION (rtsh_accumulate_visibility_list_motion and its clamped form; accumulateMomentsPixel alike): Q and the normal the taps are
// tested with come from this frame's motion G-buffer planes, compiled in by the switch alone -- the non-motion instantiations are the
// text they were.  `Frames` then also gives V3 prevPoint(x, y) (Q) and V3 prevPointNormal(x, y) (M_p; all zero: no tap is accepted).
struct TemporalList {
    uint32_t count, maxLength, resetLights, history;      // history: 0 on the first frame (no prev_* buffers)
    V3 eyeDelta, right, up, fwd;
    float scaleX, scaleY, normalCosMin, planeEps;
};

RTS_HD float dotGrouped(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RTS_HD uint32_t floatBits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// ORDER of the clamp's box: a total order on the non-NaN floats as unsigned integers, -0 < +0.  No non-NaN float has the key
// kClampNoKey (keys of the non-NaN floats lie in 0x007FFFFF .. 0xFF800000): it marks a tap that does not contribute.
enum : uint32_t { kClampNoKey = 0xFFFFFFFFu };
RTS_HD uint32_t clampKey(uint32_t u) { return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
RTS_HD uint32_t clampUnkey(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
RTS_HD bool bitsAreNaN(uint32_t u) { return (u & 0x7FFFFFFFu) > 0x7F800000u; }

template <bool Clamped = false, bool Motion = false, class Frames>
RTS_HD void accumulatePixel(const TemporalList& f, const Frames& t, int x, int y, int W, int H, float margin = 0.0f) {
    const V3 np = t.normal(x, y);
    const uint32_t all = (1u << f.count) - 1u;
    const uint32_t onp = isBackground(np) ? 0u : (t.bits(x, y) & all);
    int qx[4] = { 0, 0, 0, 0 }, qy[4] = { 0, 0, 0, 0 };
    uint32_t w[4] = { 0, 0, 0, 0 }, taps = 0;                                                      // taps: bit k = tap k passes the geometry
    if (onp != 0u && f.history != 0u && (all & ~f.resetLights) != 0u) {
        V3 q, mp;                                                                                  // Q, and the normal the taps are tested with
        if constexpr (Motion) { q = t.prevPoint(x, y); mp = t.prevPointNormal(x, y); }
        else { q = add(t.position(x, y), f.eyeDelta); mp = np; }
        const float z = dotGrouped(q, f.fwd);
        const float a = dotGrouped(q, f.right) / z, b = dotGrouped(q, f.up) / z;
        const float fx = (a / f.scaleX + 1.0f) * (0.5f * (float)W) - 0.5f;
        const float fy = (1.0f - b / f.scaleY) * (0.5f * (float)H) - 0.5f;
        const float gx = fx * 32.0f + 0.5f, gy = fy * 32.0f + 0.5f;
        if (z > 0.0f && gx >= -32.0f && gx < (float)W * 32.0f && gy >= -32.0f && gy < (float)H * 32.0f && !(Motion && isBackground(mp))) {
            const int32_t ix = (int32_t)__builtin_floorf(gx), iy = (int32_t)__builtin_floorf(gy);
            const int x0 = ix >> 5, y0 = iy >> 5;
            const uint32_t ax = (uint32_t)(ix & 31), ay = (uint32_t)(iy & 31);
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < 4; ++k) {
                qx[k] = x0 + (k & 1); qy[k] = y0 + (k >> 1);
                w[k] = ((k & 1) ? ax : 32u - ax) * ((k >> 1) ? ay : 32u - ay);
                if (w[k] == 0u || qx[k] < 0 || qx[k] >= W || qy[k] < 0 || qy[k] >= H) continue;
                const V3 nq = t.prevNormal(qx[k], qy[k]);
                if (isBackground(nq)) continue;
                if (!(dotGrouped(mp, nq) >= f.normalCosMin)) continue;
                const float h = dotGrouped(mp, sub(t.prevPosition(qx[k], qy[k]), q));
                if (!(__builtin_fabsf(h) <= f.planeEps)) continue;
                taps |= 1u << k;
            }
        }
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        if (!((onp >> l) & 1u)) { t.store(l, x, y, 0u, 0u); continue; }
        const uint32_t cur = t.current(l, x, y);
        uint32_t sw = 0, m = 255u;
        float sv = 0.0f;
        if (taps != 0u && !((f.resetLights >> l) & 1u)) {
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < 4; ++k) {
                if (!((taps >> k) & 1u)) continue;
                const uint32_t len = t.prevLength(l, qx[k], qy[k]);
                if (len == 0u) continue;
                sw += w[k];
                sv = sv + (float)w[k] * t.prevVisibility(l, qx[k], qy[k]);
                if (len < m) m = len;
            }
        }
        const uint32_t n = sw == 0u ? 1u : (m + 1u < f.maxLength ? m + 1u : f.maxLength);
        uint32_t out = cur;
        if (n != 1u) {
            float prev = sv / (float)sw;
            const float c = asFloat(cur);
            if constexpr (Clamped) {
                uint32_t loKey, hiKey;
                if (t.box(l, x, y, &loKey, &hiKey)) {
                    const float lo = asFloat(clampUnkey(loKey)) - margin, hi = asFloat(clampUnkey(hiKey)) + margin;
                    prev = prev < lo ? lo : (prev > hi ? hi : prev);                              // a NaN fails both and stays
                }
            }
            const float v = prev + (c - prev) * (1.0f / (float)n);
            out = v != v ? 0x7FC00000u : floatBits(v);
        }
        t.store(l, x, y, out, n);
    }
}

// The TEMPORAL ACCUMULATION OF A SOFT LIGHT LIST'S COUNT MOMENTS (include/rts_scene.h, rtsh_accumulate_moments_soft_light_list), one
// pixel: accumulatePixel's geometry -- INACTIVE, REPROJECT, the four taps, their integer weights and their acceptance, a COPY of its
// statements (accumulateListKernel keeps its instruction text) -- in front of an INTEGER blend of the first and second moment of
// V_0 = min(c, n_l) * S_l.  s = the sum of w * prev over the accepted taps (< 2^26 for the mean, < 2^42 for the square),
// num = (n - 1) * s + sw * cur, den = n * sw < 2^18, out = (2 * num + den) / (2 * den): 2 * num + den < 2^52, so everything is exact in
// unsigned 64 bits and no order of taps can change a bit.  `Frames`: V3 normal(x, y), position(x, y); uint32_t bits(x, y);
// uint32_t count(l, x, y) (the byte); V3 prevNormal(x, y), prevPosition(x, y); uint32_t prevLength(l, x, y), prevMean(l, x, y),
// prevSquare(l, x, y); void store(l, x, y, uint32_t mean, uint32_t square, uint32_t length).
struct MomentsList { TemporalList t; uint32_t samples[8], scale[8]; };                            // n_l, S_l as in WideFilterList

// a / b by integer division for a < 2^53 and 0 < b < 2^20 WITHOUT the 64-bit division (on the GPU a loop of some 90 instructions): both
// are exact as doubles, their correctly rounded quotient misses a / b by less than 2^-18, so its integer part is the quotient or one
// above it (where a / b lies just below an integer and rounds onto it; never below: rounding is monotonic and integers are
// representable).  Two integer comparisons make the result exact whatever the estimate: the same source on host and device.
RTS_HD uint64_t momentsQuotient(uint64_t a, uint32_t b) {
    uint64_t q = (uint64_t)((double)a / (double)b);
    if (q * b > a) --q;
    if ((q + 1u) * b <= a) ++q;
    return q;
}

// CLAMPED (rtsh_accumulate_moments_soft_light_list_clamped and its motion form): the box of the header from the window's
// five integers -- m contributing taps, S1 = the sum of their V_0, S2 = the sum of the squares, lo and hi --, everything in unsigned
// 64 bits: D = m S2 - S1^2 < 2^43, x = k4^2 D < 2^59, R = ceil(sqrt(x)) by a double estimate and an integer fix-up that makes it exact
// (R < 2^30, so (R + 1)^2 < 2^61); the quotients by m are of numbers below 2^23.  The same source
// on host and device; rtsh_moments_clamp_bounds exports it.
RTS_HD void momentsClampBounds(uint32_t m, uint64_t S1, uint64_t S2, uint32_t lo, uint32_t hi, uint32_t k4, uint32_t margin, uint32_t* Lv,
                               uint32_t* Hv) {
    const uint64_t D = (uint64_t)m * S2 - S1 * S1;
    const uint64_t xx = (uint64_t)(k4 * k4) * D;
    // (double)x misses x by at most 2^-53 of it and the root of that by less than 2^-22 for x < 2^62, so the estimate's integer part is
    // isqrt(x) or one beside it: one step down and one step up make it exact, as in momentsQuotient.  NO LOOP: a loop here would
    // not end for an x near 2^64, which only parts that no window gives (m * S2 < S1^2) can produce -- a kernel must end anyway.
    uint64_t R = (uint64_t)__builtin_sqrt((double)xx);
    if (R * R > xx) --R;
    if ((R + 1u) * (R + 1u) <= xx) ++R;                                                            // R = isqrt(x)
    if (R * R < xx) ++R;                                                                           // ... its ceiling
    const uint64_t Rc = (R + 3u) / 4u;
    const uint64_t A = S1 > Rc ? S1 - Rc : 0u, B = S1 + Rc;
    const uint64_t mlo = (uint64_t)m * lo, mhi = (uint64_t)m * hi;
    const uint32_t Lm = (uint32_t)(mlo > A ? mlo : A), Hm = (uint32_t)(mhi < B ? mhi : B);         // both at most m * hi < 2^23
    const uint32_t lv = Lm / m, hv = (Hm + m - 1u) / m;                                            // rounded OUTWARD
    const uint64_t top = (uint64_t)hv + margin;
    *Lv = lv > margin ? lv - margin : 0u;
    *Hv = top < 65535u ? (uint32_t)top : 65535u;
}

// `Frames` of the clamped instantiation also gives  void box(l, x, y, uint32_t* Lv, uint32_t* Hv): Lv' and Hv' of the pixel's window for
// light l (the host twin loops over the window and calls momentsClampBounds; the kernel reads what it staged).  It is asked only at a
// blended pair, whose centre contributes: m >= 1.  Compiled in by the switch alone -- the other instantiations are the text they were.
template <bool Motion = false, bool Clamped = false, class Frames>
RTS_HD void accumulateMomentsPixel(const MomentsList& g, const Frames& t, int x, int y, int W, int H) {
    const TemporalList& f = g.t;
    const V3 np = t.normal(x, y);
    const uint32_t all = (1u << f.count) - 1u;
    const uint32_t onp = isBackground(np) ? 0u : (t.bits(x, y) & all);
    int qx[4] = { 0, 0, 0, 0 }, qy[4] = { 0, 0, 0, 0 };
    uint32_t w[4] = { 0, 0, 0, 0 }, taps = 0;                                                      // taps: bit k = tap k passes the geometry
    if (onp != 0u && f.history != 0u && (all & ~f.resetLights) != 0u) {
        V3 q, mp;                                                                                  // Q, and the normal the taps are tested with
        if constexpr (Motion) { q = t.prevPoint(x, y); mp = t.prevPointNormal(x, y); }
        else { q = add(t.position(x, y), f.eyeDelta); mp = np; }
        const float z = dotGrouped(q, f.fwd);
        const float a = dotGrouped(q, f.right) / z, b = dotGrouped(q, f.up) / z;
        const float fx = (a / f.scaleX + 1.0f) * (0.5f * (float)W) - 0.5f;
        const float fy = (1.0f - b / f.scaleY) * (0.5f * (float)H) - 0.5f;
        const float gx = fx * 32.0f + 0.5f, gy = fy * 32.0f + 0.5f;
        if (z > 0.0f && gx >= -32.0f && gx < (float)W * 32.0f && gy >= -32.0f && gy < (float)H * 32.0f && !(Motion && isBackground(mp))) {
            const int32_t ix = (int32_t)__builtin_floorf(gx), iy = (int32_t)__builtin_floorf(gy);
            const int x0 = ix >> 5, y0 = iy >> 5;
            const uint32_t ax = (uint32_t)(ix & 31), ay = (uint32_t)(iy & 31);
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < 4; ++k) {
                qx[k] = x0 + (k & 1); qy[k] = y0 + (k >> 1);
                w[k] = ((k & 1) ? ax : 32u - ax) * ((k >> 1) ? ay : 32u - ay);
                if (w[k] == 0u || qx[k] < 0 || qx[k] >= W || qy[k] < 0 || qy[k] >= H) continue;
                const V3 nq = t.prevNormal(qx[k], qy[k]);
                if (isBackground(nq)) continue;
                if (!(dotGrouped(mp, nq) >= f.normalCosMin)) continue;
                const float h = dotGrouped(mp, sub(t.prevPosition(qx[k], qy[k]), q));
                if (!(__builtin_fabsf(h) <= f.planeEps)) continue;
                taps |= 1u << k;
            }
        }
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        if (!((onp >> l) & 1u)) { t.store(l, x, y, 0u, 0u, 0u); continue; }
        const uint32_t cur1 = wideFilterInput(t.count(l, x, y), g.samples[l], g.scale[l]);         // V_0 <= 65535
        const uint32_t cur2 = cur1 * cur1;                                                        // < 2^32
        uint32_t sw = 0, m = 255u;
        uint64_t s1 = 0, s2 = 0;
        if (taps != 0u && !((f.resetLights >> l) & 1u)) {
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < 4; ++k) {
                if (!((taps >> k) & 1u)) continue;
                const uint32_t len = t.prevLength(l, qx[k], qy[k]);
                if (len == 0u) continue;
                sw += w[k];
                s1 += (uint64_t)(w[k] * t.prevMean(l, qx[k], qy[k]));                              // 1024 * 65535 < 2^26
                s2 += (uint64_t)w[k] * (uint64_t)t.prevSquare(l, qx[k], qy[k]);
                if (len < m) m = len;
            }
        }
        const uint32_t n = sw == 0u ? 1u : (m + 1u < f.maxLength ? m + 1u : f.maxLength);
        uint32_t out1 = cur1, out2 = cur2;
        if (n != 1u) {
            const uint32_t den = n * sw;                                                           // <= 255 * 1024
            if constexpr (Clamped) {
                uint32_t lv, hv;
                t.box(l, x, y, &lv, &hv);
                const uint64_t lo1 = (uint64_t)sw * lv, hi1 = (uint64_t)sw * hv;                   // sw * Hv'^2 <= 2^10 * 2^32
                const uint64_t lo2 = (uint64_t)sw * (uint64_t)(lv * lv), hi2 = (uint64_t)sw * (uint64_t)(hv * hv);
                s1 = s1 < lo1 ? lo1 : (s1 > hi1 ? hi1 : s1);
                s2 = s2 < lo2 ? lo2 : (s2 > hi2 ? hi2 : s2);
            }
            out1 = (uint32_t)momentsQuotient(2u * ((uint64_t)(n - 1u) * s1 + (uint64_t)sw * cur1) + den, 2u * den);
            out2 = (uint32_t)momentsQuotient(2u * ((uint64_t)(n - 1u) * s2 + (uint64_t)sw * cur2) + den, 2u * den);
        }
        t.store(l, x, y, out1, out2, n);
    }
}

// The TEMPORAL ACCUMULATION OF THE BENT TEXEL (include/rts_scene.h, rtsh_accumulate_bent), one pixel: the geometry of
// accumulateMomentsPixel for ONE plane -- INACTIVE by the bent filter's rule (not background, byte non-zero), REPROJECT, the four taps,
// their integer weights and their acceptance, a COPY of its statements once more (accumulateMomentsKernel keeps its instruction text)
// -- in front of an integer blend of the wide bent filter's 8-byte texel: V by the moments pass's rounded mean, x, y, z by the same mean
// of the magnitude with the sign put back (half away from zero), so the pass commutes with negation.  |s| <= 1024 * 32768 = 2^25,
// |num| <= 254 * 2^25 + 2^10 * 2^15 < 2^34, den = n * sw < 2^18: exact in 64 bits, and no order of taps can change a bit.  `Frames`:
// V3 normal(x, y), position(x, y); bool active(x, y) (the byte, true without a plane); BentTexel current(x, y) (X_0, V_0: bentFilterInput
// of this frame's float texel); V3 prevNormal(x, y), prevPosition(x, y); uint32_t prevLength(x, y); BentTexel prevTexel(x, y) (the
// unpacked 8 bytes, whatever they hold); void store(x, y, uint64_t texel, uint32_t length); with Motion also prevPoint, prevPointNormal.
struct BentTemporalList { TemporalList t; BentFilterList q; };                                     // q: n, S_b, S_l (its thresholds unused)

RTS_HD int32_t bentTemporalMean(int64_t num, uint32_t den) {
    const uint64_t a = num < 0 ? (uint64_t)(-num) : (uint64_t)num;
    const int32_t q = (int32_t)momentsQuotient(2u * a + den, 2u * den);
    return num < 0 ? -q : q;
}

template <bool Motion = false, class Frames>
RTS_HD void accumulateBentPixel(const BentTemporalList& g, const Frames& t, int x, int y, int W, int H) {
    const TemporalList& f = g.t;
    const V3 np = t.normal(x, y);
    if (isBackground(np) || !t.active(x, y)) { t.store(x, y, 0u, 0u); return; }
    int qx[4] = { 0, 0, 0, 0 }, qy[4] = { 0, 0, 0, 0 };
    uint32_t w[4] = { 0, 0, 0, 0 }, taps = 0;                                                      // taps: bit k = tap k passes the geometry
    if (f.history != 0u && !(f.resetLights & 1u)) {
        V3 q, mp;                                                                                  // Q, and the normal the taps are tested with
        if constexpr (Motion) { q = t.prevPoint(x, y); mp = t.prevPointNormal(x, y); }
        else { q = add(t.position(x, y), f.eyeDelta); mp = np; }
        const float z = dotGrouped(q, f.fwd);
        const float a = dotGrouped(q, f.right) / z, b = dotGrouped(q, f.up) / z;
        const float fx = (a / f.scaleX + 1.0f) * (0.5f * (float)W) - 0.5f;
        const float fy = (1.0f - b / f.scaleY) * (0.5f * (float)H) - 0.5f;
        const float gx = fx * 32.0f + 0.5f, gy = fy * 32.0f + 0.5f;
        if (z > 0.0f && gx >= -32.0f && gx < (float)W * 32.0f && gy >= -32.0f && gy < (float)H * 32.0f && !(Motion && isBackground(mp))) {
            const int32_t ix = (int32_t)__builtin_floorf(gx), iy = (int32_t)__builtin_floorf(gy);
            const int x0 = ix >> 5, y0 = iy >> 5;
            const uint32_t ax = (uint32_t)(ix & 31), ay = (uint32_t)(iy & 31);
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < 4; ++k) {
                qx[k] = x0 + (k & 1); qy[k] = y0 + (k >> 1);
                w[k] = ((k & 1) ? ax : 32u - ax) * ((k >> 1) ? ay : 32u - ay);
                if (w[k] == 0u || qx[k] < 0 || qx[k] >= W || qy[k] < 0 || qy[k] >= H) continue;
                const V3 nq = t.prevNormal(qx[k], qy[k]);
                if (isBackground(nq)) continue;
                if (!(dotGrouped(mp, nq) >= f.normalCosMin)) continue;
                const float h = dotGrouped(mp, sub(t.prevPosition(qx[k], qy[k]), q));
                if (!(__builtin_fabsf(h) <= f.planeEps)) continue;
                taps |= 1u << k;
            }
        }
    }
    const BentTexel cur = t.current(x, y);
    uint32_t sw = 0, m = 255u, sv = 0;
    int32_t sx = 0, sy = 0, sz = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        if (!((taps >> k) & 1u)) continue;
        const uint32_t len = t.prevLength(qx[k], qy[k]);
        if (len == 0u) continue;
        const BentTexel h = t.prevTexel(qx[k], qy[k]);
        const int32_t wk = (int32_t)w[k];
        sw += w[k];
        sx += wk * h.x; sy += wk * h.y; sz += wk * h.z;                                            // |sum| <= 1024 * 32768 = 2^25
        sv += w[k] * h.v;                                                                          // 1024 * 65535 < 2^26
        if (len < m) m = len;
    }
    const uint32_t n = sw == 0u ? 1u : (m + 1u < f.maxLength ? m + 1u : f.maxLength);
    BentTexel out = cur;
    if (n != 1u) {
        const uint32_t den = n * sw;                                                               // <= 255 * 1024
        const int64_t k = (int64_t)(n - 1u), c = (int64_t)sw;
        out.x = bentTemporalMean(k * sx + c * cur.x, den);
        out.y = bentTemporalMean(k * sy + c * cur.y, den);
        out.z = bentTemporalMean(k * sz + c * cur.z, den);
        out.v = (uint32_t)momentsQuotient(2u * ((uint64_t)(n - 1u) * sv + (uint64_t)sw * cur.v) + den, 2u * den);
    }
    t.store(x, y, bentFilterPack(out), n);
}

// INPUT of the wide bent filter fed from the accumulated texel (rtsh_wide_filter_bent_mean): the 8 bytes clamped to what the trace can
// give -- the accumulate never writes more (its RANGE anchor), but any 8 bytes are allowed and out.xyz must stay in [-1, 1], out.w in
// [0, 1] (a component 0x8000 is -32768 < -(n * S_b); 65535 > n * S_l for n = 48).
RTS_HD BentTexel bentFilterMeanInput(uint64_t texel, const BentFilterList& f) {
    BentTexel v = bentFilterUnpack(texel);
    const int32_t lim = (int32_t)(f.samples * f.scaleB);
    const uint32_t full = f.samples * f.scaleL;
    v.x = v.x < -lim ? -lim : (v.x > lim ? lim : v.x);
    v.y = v.y < -lim ? -lim : (v.y > lim ? lim : v.y);
    v.z = v.z < -lim ? -lim : (v.z > lim ? lim : v.z);
    v.v = v.v < full ? v.v : full;
    return v;
}

// The TEMPORAL THRESHOLD of the guided wide filter (include/rts_scene.h, rtsh_wide_filter_guided_temporal_soft_light_list):
// wideGuideThresholdPixel with one change, in the energy of a counted pixel q: n_l * max(0, square - mean^2) where the moments'
// history at q is at least minHistory frames long, else the Bernoulli energy V_0 * (n S - V_0) as there.  The planes are read where
// they are (the host twin and the kernel alike): `length` first, then either the two moments or V_0.  E* < 48 * 2^32, G < 2^42,
// k4^2 * G < 2^58: wideGuideThreshold's fix-up multiplies r * r * d < 2^46 and is exact whatever G is.
struct GuideMoments {
    const uint16_t* mean;
    const uint32_t* square;
    const uint8_t* lengths;
    uint64_t W, n;
    RTS_HD uint64_t at(int x, int y, uint32_t l) const { return (uint64_t)l * n + (uint64_t)y * W + (uint64_t)x; }
};

template <class Texels>
RTS_HD void wideGuideTemporalThresholdPixel(const WideFilterList& f, uint32_t k4, uint32_t minHistory, const Texels& t, const GuideMoments& h,
                                            int x, int y, int W, int H, uint32_t* T8) {
    const uint32_t onp = isBackground(t.normal(x, y)) ? 0u : (t.bits(x, y) & ((1u << f.count) - 1u));
    uint32_t nb[9];                                                              // the map bits of the nine pixels that count
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 9; ++j) {
        const int qx = x + j % 3 - 1, qy = y + j / 3 - 1;
        nb[j] = 0u;
        if (onp == 0u || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        nb[j] = j == 4 ? onp : (isBackground(t.normal(qx, qy)) ? 0u : t.bits(qx, qy));
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        T8[l] = 0u;
        if (!((onp >> l) & 1u)) continue;
        T8[l] = 65535u;
        if (f.samples[l] < 2u) continue;
        const uint32_t full = f.samples[l] * f.scale[l];                         // n_l * S_l
        uint64_t G = 0;
        uint32_t D = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 9; ++j) {
            if (!((nb[j] >> l) & 1u)) continue;
            const int qx = x + j % 3 - 1, qy = y + j / 3 - 1;
            const uint32_t w = (j % 3 == 1 ? 2u : 1u) * (j / 3 == 1 ? 2u : 1u);
            const uint64_t i = h.at(qx, qy, l);
            uint64_t E;
            if ((uint32_t)h.lengths[i] >= minHistory) {
                const uint64_t mean = h.mean[i], square = h.square[i];
                E = square > mean * mean ? (uint64_t)f.samples[l] * (square - mean * mean) : 0u;   // n_l * max(0, square - mean^2)
            } else {
                const uint32_t v = t.value(qx, qy, l);
                E = (uint64_t)(v * (full - v));                                  // E = V_0 * (n S - V_0) < 2^30
            }
            G += (uint64_t)w * E;
            D += w;
        }
        T8[l] = wideGuideThreshold(G, D, f.samples[l], k4);
    }
}

// The WIDE FILTERS FED FROM THE ACCUMULATED MEAN (include/rts_scene.h, rtsh_wide_filter_mean_soft_light_list and
// rtsh_wide_filter_guided_temporal_mean_soft_light_list): the passes above over V_0' = min(mean, n_l * S_l) in the place of V_0.  The
// passes are wideFilterPassPixel and wideGuidedPassPixel as they are -- a `Texels` whose value(x, y, l) is wideMeanInput of the mean
// plane is the whole change.  The threshold of the guided form is a SIBLING of wideGuideTemporalThresholdPixel (which keeps its text, and
// with it every kernel that calls it): E* is that function's, from the UNCLAMPED moments where the history is long enough, but its
// Bernoulli fallback cannot come from t.value -- the window now holds the mean --, so the count byte is read where it is, and only
// where lengths < minHistory.
RTS_HD uint32_t wideMeanInput(uint32_t mean, uint32_t samples, uint32_t scale) {                          // V_0'
    const uint32_t full = samples * scale;
    return mean < full ? mean : full;
}

struct GuideMomentsCounts {
    GuideMoments m;
    const uint8_t* counts;
};

template <class Texels>
RTS_HD void wideGuideTemporalMeanThresholdPixel(const WideFilterList& f, uint32_t k4, uint32_t minHistory, const Texels& t,
                                                const GuideMomentsCounts& h, int x, int y, int W, int H, uint32_t* T8) {
    const uint32_t onp = isBackground(t.normal(x, y)) ? 0u : (t.bits(x, y) & ((1u << f.count) - 1u));
    uint32_t nb[9];                                                              // the map bits of the nine pixels that count
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 9; ++j) {
        const int qx = x + j % 3 - 1, qy = y + j / 3 - 1;
        nb[j] = 0u;
        if (onp == 0u || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        nb[j] = j == 4 ? onp : (isBackground(t.normal(qx, qy)) ? 0u : t.bits(qx, qy));
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        T8[l] = 0u;
        if (!((onp >> l) & 1u)) continue;
        T8[l] = 65535u;
        if (f.samples[l] < 2u) continue;
        const uint32_t full = f.samples[l] * f.scale[l];                         // n_l * S_l
        uint64_t G = 0;
        uint32_t D = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 9; ++j) {
            if (!((nb[j] >> l) & 1u)) continue;
            const int qx = x + j % 3 - 1, qy = y + j / 3 - 1;
            const uint32_t w = (j % 3 == 1 ? 2u : 1u) * (j / 3 == 1 ? 2u : 1u);
            const uint64_t i = h.m.at(qx, qy, l);
            uint64_t E;
            if ((uint32_t)h.m.lengths[i] >= minHistory) {
                const uint64_t mean = h.m.mean[i], square = h.m.square[i];
                E = square > mean * mean ? (uint64_t)f.samples[l] * (square - mean * mean) : 0u;   // n_l * max(0, square - mean^2)
            } else {
                const uint32_t v = wideFilterInput(h.counts[i], f.samples[l], f.scale[l]);         // V_0 of THIS frame's count
                E = (uint64_t)(v * (full - v));                                  // E = c (n - c) S^2 < 2^30
            }
            G += (uint64_t)w * E;
            D += w;
        }
        T8[l] = wideGuideThreshold(G, D, f.samples[l], k4);
    }
}

// The GUIDED MEAN FILTER WITH A PROPAGATED VARIANCE (include/rts_scene.h, rtsh_wide_filter_propagated_mean_soft_light_list; DESIGN.md
// 4.31): the guided mean filter above with a per-pixel variance plane Q_k (uint32_t, V^2 units) carried from pass to pass, and the
// threshold re-derived from it at every pass.  Everything here is NEW TEXT -- no function above is edited, so every kernel that calls
// one keeps its instruction text.  `Variance` gives Q_k by pixel coordinates: uint32_t variance(x, y, l), asked only at a pair that is
// inside the frame, not background and on, of a light with n_l >= 2.
struct WidePropagatedRule { uint32_t k4, minHistory, byLength; };

// Q_(k+1) = (2 * numQ + den^2) / (2 * den^2) for numQ < 2^45 and 1 <= den <= 256: 2 * numQ + den^2 < 2^46, 2 * den^2 <= 2^17.
RTS_HD uint32_t wideVarianceStep(uint64_t numQ, uint32_t den) {
    const uint32_t d2 = den * den;
    return (uint32_t)momentsQuotient(2u * numQ + d2, 2u * d2);
}

// Q_0 of an active pair (i: its index into the planes): R, R / lengths, or this frame's Bernoulli energy over n_l.
RTS_HD uint32_t wideVarianceInput(const WideFilterList& f, const WidePropagatedRule& r, const GuideMomentsCounts& h, uint64_t i, uint32_t l) {
    const uint32_t len = h.m.lengths[i];
    if (len >= r.minHistory) {                                                   // (minHistory >= 1: len != 0)
        const uint64_t mean = h.m.mean[i], square = h.m.square[i];
        const uint32_t R = square > mean * mean ? (uint32_t)(square - mean * mean) : 0u;
        return r.byLength ? R / len : R;
    }
    const uint32_t v = wideFilterInput(h.counts[i], f.samples[l], f.scale[l]);
    return (v * (f.samples[l] * f.scale[l] - v)) / f.samples[l];                 // c (n - c) S^2 / n
}

// Q_k where a pass reads it: Q_0 formed from the moments (planes == NULL: the first pass), else the previous pass's planes.
struct WideVarianceGlobal {
    const WideFilterList& f;
    WidePropagatedRule r;
    GuideMomentsCounts h;
    const uint32_t* planes;
    RTS_HD uint32_t variance(int x, int y, uint32_t l) const {
        const uint64_t i = h.m.at(x, y, l);
        return planes ? planes[i] : wideVarianceInput(f, r, h, i, l);
    }
};

// T_0: wideGuideTemporalMeanThresholdPixel's statements with E* = n_l * (R / lengths) in the temporal branch where byLength is set;
// with byLength == 0 it is that function's expression value for value.
template <class Texels>
RTS_HD void widePropagatedFirstThresholdPixel(const WideFilterList& f, const WidePropagatedRule& r, const Texels& t, const GuideMomentsCounts& h,
                                              int x, int y, int W, int H, uint32_t* T8) {
    const uint32_t onp = isBackground(t.normal(x, y)) ? 0u : (t.bits(x, y) & ((1u << f.count) - 1u));
    uint32_t nb[9];                                                              // the map bits of the nine pixels that count
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 9; ++j) {
        const int qx = x + j % 3 - 1, qy = y + j / 3 - 1;
        nb[j] = 0u;
        if (onp == 0u || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        nb[j] = j == 4 ? onp : (isBackground(t.normal(qx, qy)) ? 0u : t.bits(qx, qy));
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        T8[l] = 0u;
        if (!((onp >> l) & 1u)) continue;
        T8[l] = 65535u;
        if (f.samples[l] < 2u) continue;
        const uint32_t full = f.samples[l] * f.scale[l];                         // n_l * S_l
        uint64_t G = 0;
        uint32_t D = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 9; ++j) {
            if (!((nb[j] >> l) & 1u)) continue;
            const int qx = x + j % 3 - 1, qy = y + j / 3 - 1;
            const uint32_t w = (j % 3 == 1 ? 2u : 1u) * (j / 3 == 1 ? 2u : 1u);
            const uint64_t i = h.m.at(qx, qy, l);
            const uint32_t len = h.m.lengths[i];
            uint64_t E;
            if (len >= r.minHistory) {
                const uint64_t mean = h.m.mean[i], square = h.m.square[i];
                const uint32_t R = square > mean * mean ? (uint32_t)(square - mean * mean) : 0u;
                E = (uint64_t)f.samples[l] * (uint64_t)(r.byLength ? R / len : R);                 // n_l * Q_0
            } else {
                const uint32_t v = wideFilterInput(h.counts[i], f.samples[l], f.scale[l]);         // V_0 of THIS frame's count
                E = (uint64_t)(v * (full - v));                                  // E = c (n - c) S^2 < 2^30
            }
            G += (uint64_t)w * E;
            D += w;
        }
        T8[l] = wideGuideThreshold(G, D, f.samples[l], r.k4);
    }
}

// T_k for k >= 1, formed by pass k before its taps: G_k = sum of w * Q_k(q) < 2^36 over the 3 x 3 ADJACENT pixels that count (inside the
// frame, not background, on; no geom test; weights {1, 2, 1} x {1, 2, 1}), T_k = wideGuideThreshold(G_k, D_k, 1, k4): Q is a variance
// of V already, so n_l leaves the divisor.  The shipped function is exact there: its fix-up multiplies r * r * d < 2^40.
template <class Texels, class Variance>
RTS_HD void widePropagatedThresholdPixel(const WideFilterList& f, uint32_t k4, const Texels& t, const Variance& q, int x, int y, int W, int H,
                                         uint32_t* T8) {
    const uint32_t onp = isBackground(t.normal(x, y)) ? 0u : (t.bits(x, y) & ((1u << f.count) - 1u));
    uint32_t nb[9];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 9; ++j) {
        const int qx = x + j % 3 - 1, qy = y + j / 3 - 1;
        nb[j] = 0u;
        if (onp == 0u || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        nb[j] = j == 4 ? onp : (isBackground(t.normal(qx, qy)) ? 0u : t.bits(qx, qy));
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        T8[l] = 0u;
        if (!((onp >> l) & 1u)) continue;
        T8[l] = 65535u;
        if (f.samples[l] < 2u) continue;
        uint64_t G = 0;
        uint32_t D = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 9; ++j) {
            if (!((nb[j] >> l) & 1u)) continue;
            const uint32_t w = (j % 3 == 1 ? 2u : 1u) * (j / 3 == 1 ? 2u : 1u);
            G += (uint64_t)w * (uint64_t)q.variance(x + j % 3 - 1, y + j / 3 - 1, l);
            D += w;
        }
        T8[l] = wideGuideThreshold(G, D, 1u, k4);
    }
}

// One pass at one pixel: wideGuidedPassPixel's statements for the values, and with VARIANCE (every pass but the last) numQ = the sum of
// w^2 * Q_k(q) over exactly the taps accepted for the light, the centre included; variance8[l] = Q_(k+1), 0 at an inactive pair and for
// a light with n_l <= 1, whose Q is never read.
template <bool VARIANCE, class Texels, class Variance>
RTS_HD void widePropagatedPassPixel(const WideFilterList& f, const Texels& t, const Variance& q, int x, int y, int W, int H, int step,
                                    const uint32_t* T8, uint32_t* value8, uint32_t* variance8) {
    const V3 np = t.normal(x, y);
    const uint32_t onp = isBackground(np) ? 0u : (t.bits(x, y) & ((1u << f.count) - 1u));
    uint32_t num[8], den[8], ctr[8];
    uint64_t numQ[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        num[l] = 0u; den[l] = 1u; ctr[l] = 0u; numQ[l] = 0u;
        if (l >= f.count || !((onp >> l) & 1u)) continue;
        ctr[l] = t.value(x, y, l);
        num[l] = 36u * ctr[l];                                                    // the centre tap: always accepted
        den[l] = 36u;
        if (VARIANCE && f.samples[l] >= 2u) numQ[l] = 1296u * (uint64_t)q.variance(x, y, l);
    }
    if (onp != 0u && step > 0) {
        const V3 pp = t.position(x, y);
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + dy * step;
            if (qy < 0 || qy >= H) continue;
            const uint32_t wy = dy == 0 ? 6u : ((dy == 1 || dy == -1) ? 4u : 1u);
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + dx * step;
                if (qx < 0 || qx >= W || (dx == 0 && dy == 0)) continue;
                if (!wideFilterGeom(t, np, pp, qx, qy, f.normalCosMin, f.planeEps)) continue;
                const uint32_t acc = t.bits(qx, qy) & onp;
                if (acc == 0u) continue;
                const uint32_t w = wy * (dx == 0 ? 6u : ((dx == 1 || dx == -1) ? 4u : 1u));
#if defined(__HIPCC__)
#pragma unroll
#endif
                for (uint32_t l = 0; l < 8; ++l) {
                    if (l >= f.count) break;
                    if (!((acc >> l) & 1u)) continue;
                    const uint32_t v = t.value(qx, qy, l);
                    if ((v > ctr[l] ? v - ctr[l] : ctr[l] - v) > T8[l]) continue;  // the guide
                    num[l] += w * v;
                    den[l] += w;
                    if (VARIANCE && f.samples[l] >= 2u) numQ[l] += (uint64_t)(w * w) * (uint64_t)q.variance(qx, qy, l);
                }
            }
        }
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        const bool on = ((onp >> l) & 1u) != 0u;
        value8[l] = on ? (2u * num[l] + den[l]) / (2u * den[l]) : 0u;
        if (VARIANCE) variance8[l] = on && f.samples[l] >= 2u ? wideVarianceStep(numQ[l], den[l]) : 0u;
    }
}

// The facing mark (include/rts_scene.h, rtsh_facing_active): 0 where the shadow mask's byte cannot reach the image -- the
// background (combinePixel leaves the pixel 0) and N.L <= 0 (direct = 1.25 * 0 * mask: either zero) --, 1 everywhere else.
// `!(ndl > 0)` would cull a NaN; `ndl <= 0` is false for one, so a NaN is traced.
RTS_HD uint8_t facingPixel(const CombineParams& c, const float* position4, const float* normal4) {
    V3 n{ normal4[0], normal4[1], normal4[2] };
    if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) return 0;
    return facingNdl(c, position4, n) <= 0 ? 0 : 1;
}

// The light map of a light list (include/rts_scene.h, rtsh_facing_lights): bit l = facingPixel for light l, bits >= count are 0.
struct FacingLights { uint32_t count; CombineParams light[8]; };

RTS_HD uint8_t facingLightsPixel(const FacingLights& f, const float* position4, const float* normal4) {
    uint32_t bits = 0;
    for (uint32_t l = 0; l < f.count; ++l) bits |= (uint32_t)facingPixel(f.light[l], position4, normal4) << l;
    return (uint8_t)bits;
}

// HALF-RESOLUTION LIGHT LISTS (include/rts_scene.h, rtsh_upsample_*): the four taps of a full-resolution pixel in the low-resolution
// frame, and the two per-pixel rules read from them.  `Full` gives the full-resolution frame by pixel coordinates: V3 normal(x, y),
// V3 position(x, y), uint32_t bits(x, y) (the map byte, 0xFF without a map).  `Low` gives the low-resolution one the same way, plus
// uint32_t byte(X, Y, l) (the count byte, or the mask's bit as 0 / 1): the host twin reads the buffers, the kernel its LDS window.
struct UpsampleList { uint32_t count, phaseX, phaseY; float normalCosMin, planeEps; int w, h; };

// weight[t] == 0: the tap does not exist (weight 0 by the tent, or outside w x h).  bits[t]: on(q, .) of an existing tap, below count;
// all of them for the tap that IS the pixel (its map bit is not looked at).  geom: bit t set where tap t passed the geometry test (the
// pixel itself always does).
struct UpsampleTaps { int X[4], Y[4]; uint32_t weight[4], bits[4], geom; };

template <class Low>
RTS_HD UpsampleTaps upsampleTaps(const UpsampleList& f, const Low& lo, V3 np, V3 pp, int x, int y) {
    const int ux = x - (int)f.phaseX, uy = y - (int)f.phaseY;
    const int X0 = ux >> 1, Y0 = uy >> 1;
    const uint32_t ax = (uint32_t)(ux & 1), ay = (uint32_t)(uy & 1), all = (1u << f.count) - 1u;
    const bool self = ax == 0u && ay == 0u;
    UpsampleTaps t;
    t.geom = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const int X = X0 + (k & 1), Y = Y0 + (k >> 1);
        const uint32_t wx = (k & 1) ? ax : 2u - ax, wy = (k >> 1) ? ay : 2u - ay;
        const bool exists = wx * wy != 0u && X >= 0 && X < f.w && Y >= 0 && Y < f.h;
        t.X[k] = X; t.Y[k] = Y;
        t.weight[k] = exists ? wx * wy : 0u;
        t.bits[k] = 0u;
        if (!exists) continue;
        if (self) { t.bits[k] = all; t.geom |= 1u << k; continue; }
        t.bits[k] = lo.bits(X, Y) & all;
        if (wideFilterGeom(lo, np, pp, X, Y, f.normalCosMin, f.planeEps)) t.geom |= 1u << k;
    }
    return t;
}

// The retrace map's byte: the lights of an active, unsampled pixel for which no tap is accepted.
template <class Full, class Low>
RTS_HD uint8_t upsampleRetracePixel(const UpsampleList& f, const Full& full, const Low& lo, int x, int y) {
    const V3 np = full.normal(x, y);
    if (isBackground(np)) return 0;
    const uint32_t onp = full.bits(x, y) & ((1u << f.count) - 1u);
    if (onp == 0u) return 0;
    if ((((uint32_t)x ^ f.phaseX) & 1u) == 0u && (((uint32_t)y ^ f.phaseY) & 1u) == 0u) return 0;       // a sampled pixel
    const UpsampleTaps t = upsampleTaps(f, lo, np, full.position(x, y), x, y);
    uint32_t accepted = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k)
        if ((t.geom >> k) & 1u) accepted |= t.bits[k];
    return (uint8_t)(onp & ~accepted);
}

// The upsampled bytes of the lights in `todo` (the lights below count whose keep bit is clear; not 0) at one pixel: byte8[l] for every
// l in todo.  Returns the lights of todo that took the fallback (the tests' census; the kernels drop it).
template <class Full, class Low>
RTS_HD uint32_t upsamplePixel(const UpsampleList& f, const Full& full, const Low& lo, int x, int y, uint32_t todo, uint32_t* byte8) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) byte8[l] = 0u;
    const V3 np = full.normal(x, y);
    if (isBackground(np)) return 0u;
    const uint32_t active = full.bits(x, y) & todo;
    if (active == 0u) return 0u;
    const UpsampleTaps t = upsampleTaps(f, lo, np, full.position(x, y), x, y);
    uint32_t fell = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t l = 0; l < 8; ++l) {
        if (l >= f.count) break;
        if (!((active >> l) & 1u)) continue;
        uint32_t num = 0u, den = 0u, best = 0u, bestByte = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < 4; ++k) {
            if (!((t.bits[k] >> l) & 1u)) continue;                               // (0 for a tap that does not exist)
            const uint32_t c = lo.byte(t.X[k], t.Y[k], l);
            if ((t.geom >> k) & 1u) { num += t.weight[k] * c; den += t.weight[k]; }
            if (t.weight[k] > best) { best = t.weight[k]; bestByte = c; }         // the fallback: largest weight, the first of equals
        }
        if (den != 0u) byte8[l] = (2u * num + den) / (2u * den);
        else { byte8[l] = bestByte; fell |= 1u << l; }
    }
    return fell;
}

// COMPACTED LIGHT MAPS (include/rts_scene.h, rtsh_compact_light_map*): the tile order of the list and the mark.  Integers only.
// Tiles of 8 x 8 pixels, row-major over the frame; slot k = 0..63 of a tile is its pixel (k & 7, k >> 3), so the slots in order are the
// tile's pixels row-major.  The host twin walks the tiles and slots in order; the kernels give a tile to a wave and slot k to lane k.
constexpr int kCompactNodes = 4;                                                   // kernels of the device form (rts_compact.inc)
constexpr uint32_t kCompactScanLanes = 256, kCompactScanPerLane = 4;
constexpr uint32_t kCompactScanTiles = kCompactScanLanes * kCompactScanPerLane;    // tiles one scan workgroup handles
struct CompactFrame { uint32_t W, H, tilesX, tiles, allBelowCount; };

RTS_HD bool makeCompactFrame(uint32_t count, uint32_t W, uint32_t H, CompactFrame* out) {
    if (count == 0u || count > 8u || W == 0u || H == 0u || (uint64_t)W * H > (1ull << 31)) return false;
    const uint64_t tilesX = ((uint64_t)W + 7u) / 8u, tilesY = ((uint64_t)H + 7u) / 8u;          // (tilesX * tilesY <= 2^28 + ...: 32 bits hold it)
    *out = CompactFrame{ W, H, (uint32_t)tilesX, (uint32_t)(tilesX * tilesY), (1u << count) - 1u };
    return true;
}
// -> whether slot k of tile t lies in the frame; *p: its pixel index y * W + x
RTS_HD bool compactSlotPixel(const CompactFrame& f, uint32_t t, uint32_t k, uint32_t* p) {
    const uint32_t ty = t / f.tilesX, tx = t - ty * f.tilesX;
    const uint32_t x = tx * 8u + (k & 7u), y = ty * 8u + (k >> 3);
    *p = y * f.W + x;                                                                           // (read only where the slot is in the frame)
    return x < f.W && y < f.H;
}
RTS_HD bool compactMarked(const CompactFrame& f, uint8_t mapByte) { return (mapByte & f.allBelowCount) != 0u; }

// AMBIENT OCCLUSION (include/rts.h, rts_trace_ambient_occlusion*): the frame around the normal and the point a sample's segment ends at
// -- the light position of the hard point light whose shadow ray the sample IS.  Shared by the host twin (rts_scene.cpp), rtsh_ao_rays
// and the kernels (rts_ao.inc); every operation is one rounded float operation, parenthesised as in the header (no contraction, the
// division correctly rounded).  sg + N.z is never 0 (sg carries N.z's sign), so a is finite for a finite normal.
struct AoFrame { V3 T, B; };
RTS_HD AoFrame aoFrame(V3 N) {
    const float sg = (floatBits(N.z) >> 31) ? -1.0f : 1.0f;
    const float a = -1.0f / (sg + N.z);
    const float b = (N.x * N.y) * a;
    return AoFrame{ V3{ 1.0f + (sg * (N.x * N.x)) * a, sg * b, -(sg * N.x) }, V3{ b, sg + (N.y * N.y) * a, -N.y } };
}
// L of sample direction s = dirs[idx] (x, y, z read): o0 + radius * dir, dir = ((T * s.x) + (B * s.y)) + (N * s.z) per component
RTS_HD V3 aoAim(V3 cam, V3 rel, V3 N, const AoFrame& f, const float* s, float radius) {
    const V3 dir{ ((f.T.x * s[0]) + (f.B.x * s[1])) + (N.x * s[2]), ((f.T.y * s[0]) + (f.B.y * s[1])) + (N.y * s[2]),
                  ((f.T.z * s[0]) + (f.B.z * s[1])) + (N.z * s[2]) };
    const V3 o0{ cam.x + rel.x, cam.y + rel.y, cam.z + rel.z };
    return V3{ o0.x + (radius * dir.x), o0.y + (radius * dir.y), o0.z + (radius * dir.z) };
}

// BENT NORMALS (include/rts.h, rts_trace_ambient_occlusion_bent*): the sum of the unoccluded samples' directions, taken over INTEGERS.
// aoQuantise is Q of the header -- a tangent-space component in 1/16384ths, a function of the table entry alone --; the kernels and the
// host twin add these integers per pixel (associative: no deal over waves and no order changes the sum) and aoBent applies the pixel's
// frame to the finished sum ONCE, in float, parenthesised as in the header.  |S.c| <= 48 * 16384 < 2^24, so both (float)S.c and the
// scale by 2^-14 are exact.  Shared by the host twin (rts_scene.cpp) and the kernels (rts_ao_bent.inc).
RTS_HD int32_t aoQuantise(float v) {
    if (v != v) return 0;
    const float c = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
    return (int32_t)__builtin_rintf(c * 16384.0f);                       // (exact product; ties to even)
}
// bent4 = (frame * (S * 2^-14), (float)count) for the normal N of an active, non-background pixel
RTS_HD void aoBent(V3 N, int32_t sx, int32_t sy, int32_t sz, uint32_t count, float* bent4) {
    const AoFrame f = aoFrame(N);
    const float fx = (float)sx * 0x1p-14f, fy = (float)sy * 0x1p-14f, fz = (float)sz * 0x1p-14f;
    bent4[0] = ((f.T.x * fx) + (f.B.x * fy)) + (N.x * fz);
    bent4[1] = ((f.T.y * fx) + (f.B.y * fy)) + (N.y * fz);
    bent4[2] = ((f.T.z * fx) + (f.B.z * fy)) + (N.z * fz);
    bent4[3] = (float)count;
}

// THE HEMISPHERIC SKY TINT of the bent combine (include/rts_scene.h, rtsh_combine_visibility_list_ao_bent): where the bent vector
// points along `up` the ambient term takes the sky's colour, against it the ground's.  up3, sky3, ground3: rtsh_sky_ambient's members.
// Every operation is one rounded float operation in the written order; the clamp sends a NaN to 0.
RTS_HD void skyTint(const float* up3, const float* sky3, const float* ground3, const float* bent4, float* tint3) {
    const float bx = bent4[0], by = bent4[1], bz = bent4[2];
    const float l2 = ((bx * bx) + (by * by)) + (bz * bz);
    const float len = __builtin_sqrtf(l2);
    float u = 0.0f;
    if (len > 0.0f && len < __builtin_inff()) u = (((bx * up3[0]) + (by * up3[1])) + (bz * up3[2])) / len;
    float h = 0.5f + 0.5f * u;
    h = (h > 0.0f) ? ((h < 1.0f) ? h : 1.0f) : 0.0f;
    for (int c = 0; c < 3; ++c) tint3[c] = ground3[c] + (sky3[c] - ground3[c]) * h;
}
// The ambient terms of the bent combine, per channel: (ambient * ao) * tint_c -- what combineVisibilityPixelRgb's ambient3Of hands back,
// on the host and in the kernel.  sky9 = { up, sky, ground }, rtsh_sky_ambient's first nine floats.
RTS_HD void skyAmbient3(float ambient, float ao, const float* sky9, const float* bent4, float* out3) {
    float tint[3];
    skyTint(sky9, sky9 + 3, sky9 + 6, bent4, tint);
    const float scaled = ambient * ao;
    for (int c = 0; c < 3; ++c) out3[c] = scaled * tint[c];
}

// AO DISTANCE AND FALLOFF (include/rts.h, rts_trace_ambient_occlusion_distance*): how OPEN a sample counts, looked up from its one-ray
// distance quantised to 64ths of the segment -- an integer per (pixel, sample), so the per-pixel sum A is as order-free as the count is.
// aoFalloffBin is b_j of the header: bits is a blocked sample's distance, a bit pattern in [+0, +Inf); min(d, 1) * 64 is exact (a power
// of two) and the conversion truncates, so bin k starts exactly at k / 64 and d >= 63 / 64 (1.0 included) falls in bin 63.
// aoOpenness is a_j: 255 for a free sample, else the table's byte; weightOf(b) reads weight[b] wherever the caller keeps the table.
// aoObscurance is the quotient: A <= 48 * 255 and S = 65535 / n, so 2 * A * S + 255 < 2^26, and the result never exceeds n * S.
// Shared by the host twin (rts_scene.cpp) and the kernels (rts_ao_distance.inc).
RTS_HD uint32_t aoFalloffBin(uint32_t bits) {
    const float d = asFloat(bits);
    const float c = d < 1.0f ? d : 1.0f;
    const uint32_t b = (uint32_t)(c * 64.0f);
    return b < 63u ? b : 63u;
}
template <class WeightOf>
RTS_HD uint32_t aoOpenness(uint32_t bits, WeightOf weightOf) {
    return bits == 0x7F800000u ? 255u : (uint32_t)weightOf(aoFalloffBin(bits));
}
RTS_HD uint32_t aoObscurance(uint32_t A, uint32_t n) {
    const uint32_t S = 65535u / n;
    return (2u * A * S + 255u) / 510u;
}

} // namespace rts_harness
