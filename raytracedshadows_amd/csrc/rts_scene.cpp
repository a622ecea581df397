// Harness: synthesises the G-buffer targets the shadow kernel and the combine pass consume
// (Source/Shaders/Model.frag:35-39 writes normal and worldPosition - cameraPosition; targets created at
// Source/RayTracedShadows.cpp:378-387) and evaluates the combine pass (Source/Shaders/Combine.frag:18-37).
// Host versions, multi-threaded; the device version of the G-buffer pass is rts_primary.hip.
// This is input synthesis / presentation, not the path under test: both the GPU kernels and the CPU oracle are fed
// the buffers this file produces.
#include "../../include/rts_scene.h"
#include "rts_closest_hit.h"
#include "rts_args.h"

#include <atomic>
#include <cmath>
#include <cstring>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

using namespace rts_harness;

namespace rts_harness {
// Pinhole camera as the reference sets it up (RayTracedShadows.cpp:238-242): vertical fov, lookAt, +Y up.
Camera makeCamera(const float eye[3], const float target[3], float fovy, uint32_t W, uint32_t H) {
    Camera c;
    c.eye = V3{ eye[0], eye[1], eye[2] };
    V3 f = sub(V3{ target[0], target[1], target[2] }, c.eye);
    float fl = std::sqrt(dot(f, f));
    c.fwd = fl > 0 ? mul(f, 1.0f / fl) : V3{ 0, 0, -1 };
    V3 r = cross(V3{ 0, 1, 0 }, c.fwd);
    float rl = std::sqrt(dot(r, r));
    c.right = rl > 0 ? mul(r, 1.0f / rl) : V3{ 1, 0, 0 };
    c.up = cross(c.fwd, c.right);
    c.tanHalf = std::tan(fovy * 0.5f);
    c.aspect = (float)W / (float)H;
    return c;
}

namespace {
// body(i) for every i < n, in chunks of `chunk` dealt over `threads` threads (0: the machine's), 64 at the most
template <class F>
void parallelFor(size_t n, size_t chunk, int threads, F&& body) {
    int nt = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > 64) nt = 64;
    std::atomic<size_t> next{ 0 };
    auto work = [&]() {
        for (;;) {
            const size_t b = next.fetch_add(chunk);
            if (b >= n) break;
            const size_t e = b + chunk < n ? b + chunk : n;
            for (size_t i = b; i < e; ++i) body(i);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt && (size_t)t * chunk < n; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}
} // namespace
} // namespace rts_harness

extern "C" int rtsh_primary_gbuffer(const rts_vec4u* packed, size_t count, const float eye[3], const float target[3],
                                    float fovy, uint32_t W, uint32_t H, float* positions, float* normals,
                                    uint64_t* hit_count, int threads) {
    if (!packed || !eye || !target || !positions || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    uint32_t P = 0;
    int s = rts_bvh_validate(packed, count, &P);
    if (s != RTS_OK) return s;
    const Camera cam = makeCamera(eye, target, fovy, W, H);
    const uint32_t* bvh = (const uint32_t*)packed;
    std::atomic<uint64_t> hits{ 0 };                                    // (integer adds: exact, whichever thread took which row)
    parallelFor(H, 1, threads, [&](size_t y) {
        uint64_t local = 0;
        for (uint32_t x = 0; x < W; ++x) {
            const size_t i = (y * W + x) * 4;
            shadePixel(bvh, cam, x, (uint32_t)y, W, H, positions + i, normals ? normals + i : nullptr);
            local += positions[i + 3] != 0.0f;
        }
        hits.fetch_add(local);
    });
    if (hit_count) *hit_count = hits.load();
    return RTS_OK;
}

extern "C" int rtsh_primary_positions(const rts_vec4u* packed, size_t count, const float eye[3], const float target[3],
                                      float fovy, uint32_t W, uint32_t H, float* positions, uint64_t* hit_count,
                                      int threads) {
    return rtsh_primary_gbuffer(packed, count, eye, target, fovy, W, H, positions, nullptr, hit_count, threads);
}

// ---- the motion G-buffer pass (include/rts_scene.h; per-pixel rule in rts_closest_hit.h: shadeMotionPixel) ----
namespace rts_harness {
// Shared by the host and device forms: the refusals that need neither stream, and eye - prev_eye, formed once.
int makeMotionEyes(const float eye[3], const float prev_eye[3], const float target[3], const void* positions, const void* prevPoints,
                   const void* prevPointNormals, uint32_t W, uint32_t H, V3* prevEye, V3* eyeDelta) {
    if (!eye || !prev_eye || !target || !positions || !prevPoints || !prevPointNormals || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(prev_eye[i])) return RTS_ERR_INVALID_ARG;
    *prevEye = V3{ prev_eye[0], prev_eye[1], prev_eye[2] };
    *eyeDelta = V3{ eye[0] - prev_eye[0], eye[1] - prev_eye[1], eye[2] - prev_eye[2] };
    return RTS_OK;
}
} // namespace rts_harness

extern "C" int rtsh_primary_gbuffer_motion(const rts_vec4u* packed, size_t count, const rts_vec4u* prev_packed, size_t prev_count,
                                           const float eye[3], const float prev_eye[3], const float target[3], float fovy, uint32_t W,
                                           uint32_t H, float* positions, float* normals, float* prev_points, float* prev_point_normals,
                                           uint32_t* leaves, uint64_t* hit_count, int threads) {
    V3 prevEye, eyeDelta;
    if (!packed || !prev_packed) return RTS_ERR_INVALID_ARG;
    int s = makeMotionEyes(eye, prev_eye, target, positions, prev_points, prev_point_normals, W, H, &prevEye, &eyeDelta);
    if (s != RTS_OK) return s;
    uint32_t P = 0;
    s = rts_bvh_validate(packed, count, &P);
    if (s != RTS_OK) return s;
    if (prev_count != count) return RTS_ERR_INVALID_ARG;
    const uint32_t* bvh = (const uint32_t*)packed;
    const uint32_t* prev = (const uint32_t*)prev_packed;
    for (size_t node = 0; node + 1 < (size_t)2 * P; ++node)                // the 2P - 1 nodes: the tag and the link word of each
        if (bvh[node * 8 + 3] != prev[node * 8 + 3] || bvh[node * 8 + 7] != prev[node * 8 + 7]) return RTS_ERR_BAD_BVH;
    const Camera cam = makeCamera(eye, target, fovy, W, H);
    std::atomic<uint64_t> hits{ 0 };
    parallelFor(H, 1, threads, [&](size_t y) {
        uint64_t local = 0;
        for (uint32_t x = 0; x < W; ++x) {
            const size_t p = y * W + x, i = p * 4;
            shadeMotionPixel(bvh, prev, cam, prevEye, eyeDelta, x, (uint32_t)y, W, H, positions + i, normals ? normals + i : nullptr,
                             prev_points + i, prev_point_normals + i, leaves ? leaves + p : nullptr);
            local += positions[i + 3] != 0.0f;
        }
        hits.fetch_add(local);
    });
    if (hit_count) *hit_count = hits.load();
    return RTS_OK;
}

namespace rts_harness {
// Shared by the host and device combine passes: validates and condenses the arguments.
int makeCombineParams(const rts_constants* k, const rts_light* light, bool havePositions, CombineParams* out) {
    if (!k || !out) return RTS_ERR_INVALID_ARG;
    if (light && light->type == RTS_LIGHT_POINT && !havePositions) return RTS_ERR_INVALID_ARG;
    CombineParams c;
    c.samples = (light && light->nsamples > 1) ? (float)light->nsamples : 1.0f;
    c.cam = V3{ k->cameraPosition[0], k->cameraPosition[1], k->cameraPosition[2] };
    V3 cd{ k->cameraDirection[0], k->cameraDirection[1], k->cameraDirection[2] };
    float cl = std::sqrt(dot(cd, cd));
    if (cl > 0) cd = mul(cd, 1.0f / cl);
    c.viewDir = cd;
    c.light = light ? V3{ light->xyz[0], light->xyz[1], light->xyz[2] }
                    : V3{ k->lightDirection[0], k->lightDirection[1], k->lightDirection[2] };
    c.pointLight = (light && light->type == RTS_LIGHT_POINT) ? 1u : 0u;
    *out = c;
    return RTS_OK;
}
} // namespace rts_harness

// Combine pass on the host (Combine.frag:18-37; per-pixel arithmetic in rts_closest_hit.h: combinePixel).
extern "C" int rtsh_combine(const rts_constants* k, const rts_light* light, const float* positions, const float* normals,
                            const uint8_t* mask, uint32_t W, uint32_t H, uint8_t* rgb) {
    if (!k || !normals || !mask || !rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    CombineParams c;
    int s = makeCombineParams(k, light, positions != nullptr, &c);
    if (s != RTS_OK) return s;
    const float zero[4] = { 0, 0, 0, 0 };
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        const uint8_t q = combinePixel(c, positions ? positions + i * 4 : zero, normals + i * 4, mask[i]);
        rgb[i * 3] = rgb[i * 3 + 1] = rgb[i * 3 + 2] = q;
    }
    return RTS_OK;
}

// The facing mark on the host (per-pixel rule in rts_closest_hit.h: facingPixel): the checker of rtsh_facing_active_device.
extern "C" int rtsh_facing_active(const rts_constants* k, const rts_light* light, const float* positions, const float* normals,
                                  uint32_t W, uint32_t H, uint8_t* active) {
    if (!k || !normals || !active || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    CombineParams c;
    int s = makeCombineParams(k, light, positions != nullptr, &c);
    if (s != RTS_OK) return s;
    const float zero[4] = { 0, 0, 0, 0 };
    for (size_t i = 0; i < (size_t)W * H; ++i) active[i] = facingPixel(c, positions ? positions + i * 4 : zero, normals + i * 4);
    return RTS_OK;
}

// ---- one ray's occluder distance on the host (include/rts_scene.h): the checker of rts_trace_rays_distance*, and of the frames below ----
// The definition of include/rts.h spelled as one straight loop per ray: the reference's walk (comp:75-111) without its return at a
// hit, the reference's box test (comp:61-73, GLSL compare-select min / max) and triangle test (comp:41-59), and the library's ray
// set-up in its general form (comp:128-146 + the point-light extension; rts_kernels.hip: makeShadowRay below its fast path, whose
// bits are the same wherever it applies).  This file is compiled without contraction, like the kernels.
namespace rts_harness {
namespace {
inline float gmin(float x, float y) { return (y < x) ? y : x; }         // GLSL min
inline float gmax(float x, float y) { return (x < y) ? y : x; }         // GLSL max
inline uint32_t asBits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline V3 crossG(V3 a, V3 b) { return V3{ a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y }; }   // GLSL cross()

struct DRay { V3 o; float tmax; V3 d; };

inline float epsilonFor(float f, uint32_t diff) {                        // comp:113-120
    uint32_t u = asBits(f);
    uint32_t e = (u >> 23) & 0xFFu;
    e -= (diff < e) ? diff : e;
    u = (u & ~(0xFFu << 23)) | (e << 23);
    return asFloat(u);
}
inline float max3abs(V3 v) { return gmax(gmax(std::fabs(v.x), std::fabs(v.y)), std::fabs(v.z)); }

inline DRay shadowRay(const float* cam, V3 rel, uint32_t lightType, V3 L) {
    V3 origin{ cam[0] + rel.x, cam[1] + rel.y, cam[2] + rel.z };                          // comp:136
    const float bias = gmax(epsilonFor(max3abs(origin), 13), epsilonFor(max3abs(rel), 13));   // comp:138-140
    DRay r;
    if (lightType == RTS_LIGHT_DIRECTIONAL) {
        origin.x = origin.x + L.x * bias; origin.y = origin.y + L.y * bias; origin.z = origin.z + L.z * bias;   // comp:143
        r.o = origin; r.tmax = 1e9f; r.d = L;                                             // comp:145-146
    } else {
        const V3 d0 = sub(L, origin);
        const float inv = 1.0f / std::sqrt(dot(d0, d0));
        origin.x = origin.x + (d0.x * inv) * bias; origin.y = origin.y + (d0.y * inv) * bias; origin.z = origin.z + (d0.z * inv) * bias;
        r.o = origin; r.tmax = 1.0f; r.d = sub(L, origin);
    }
    return r;
}

inline uint32_t rayDistanceBits(const uint32_t* bvh, const DRay& r) {
    const V3 inv{ 1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z };                             // comp:77
    uint32_t best = 0x7F800000u, node = 0;
    while (node != 0xFFFFFFFFu) {
        const uint32_t* a = bvh + (size_t)node * 8;
        const uint32_t* b = a + 4;
        if (a[3] != 0xFFFFFFFFu) {
            const uint32_t* t = bvh + (size_t)a[3] * 4;
            const V3 e0{ asFloat(a[0]), asFloat(a[1]), asFloat(a[2]) }, e1{ asFloat(b[0]), asFloat(b[1]), asFloat(b[2]) };
            const V3 v0{ asFloat(t[0]), asFloat(t[1]), asFloat(t[2]) };
            const V3 s1 = crossG(r.d, e1);
            const float invd = 1.0f / dot(s1, e0);
            const V3 dd = sub(r.o, v0);
            const float b1 = dot(dd, s1) * invd;
            const V3 s2 = crossG(dd, e0);
            const float b2 = dot(r.d, s2) * invd;
            const float tt = dot(e1, s2) * invd;
            if (!(b1 < 0.0f || b1 > 1.0f || b2 < 0.0f || b1 + b2 > 1.0f || tt < 0.0f || tt > r.tmax)) {
                const uint32_t c = tt > 0.0f ? asBits(tt) : 0u;          // an accepted NaN or -0 counts as +0
                if (c < best) best = c;
            }
        } else {
            const float fx = (asFloat(b[0]) - r.o.x) * inv.x, fy = (asFloat(b[1]) - r.o.y) * inv.y, fz = (asFloat(b[2]) - r.o.z) * inv.z;
            const float nx = (asFloat(a[0]) - r.o.x) * inv.x, ny = (asFloat(a[1]) - r.o.y) * inv.y, nz = (asFloat(a[2]) - r.o.z) * inv.z;
            const float t1 = gmin(gmax(fx, nx), gmin(gmax(fy, ny), gmax(fz, nz)));
            const float t0 = gmax(gmax(gmin(fx, nx), gmax(gmin(fy, ny), gmin(fz, nz))), 0.0f);
            if (t1 >= t0) { ++node; continue; }
        }
        node = b[3];                                                     // hit or miss: on through the miss link
    }
    return best;
}
} // namespace
} // namespace rts_harness

extern "C" int rtsh_rays_distance(const rts_vec4u* packed, size_t count_vec4, const rts_ray* rays, size_t n, float* out_t, int threads) {
    if (!packed || (n && (!rays || !out_t))) return RTS_ERR_INVALID_ARG;
    const int s = rts_bvh_validate(packed, count_vec4, nullptr);
    if (s != RTS_OK) return s;
    const uint32_t* bvh = (const uint32_t*)packed;
    const float* f = (const float*)rays;                                 // rts_ray = {o.xyz, tmax, d.xyz, pad}: 8 floats
    parallelFor(n, 256, threads, [&](size_t i) {
        const float* q = f + i * 8;
        const DRay r{ V3{ q[0], q[1], q[2] }, q[3], V3{ q[4], q[5], q[6] } };
        out_t[i] = asFloat(rayDistanceBits(bvh, r));
    });
    return RTS_OK;
}

// ---- occluder distance of a frame on the host (include/rts_scene.h): the checker of rts_trace_shadow_distance* and rts_trace_soft_distance* ----
// The definition of include/rts.h as a straight loop over (pixel, sample): the light position of sample j (rts_light: offsets[j], or
// the table entry the pixel's hashed start picks), the ray and the one-ray distance above, an integer minimum.  One sample: the hard
// light itself, and the count of unoccluded samples is the 0/1 shadow byte.
namespace rts_harness {
namespace {
inline uint32_t hash32(uint32_t v) {                                     // rts_light.table (include/rts.h)
    v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
    return v;
}
inline uint32_t sampleIndex(uint32_t table, uint32_t sample, uint32_t pixel) {
    if (table == 0) return sample;
    const uint32_t j = (uint32_t)(((uint64_t)hash32(pixel) * table) >> 32) + sample;    // start < table, sample < nsamples <= table
    return j >= table ? j - table : j;
}
} // namespace
} // namespace rts_harness

// rows [row_begin, row_end) of a frame, ns samples per pixel (the light's rule checked by the caller; ns > 1 only with a light)
static int frameDistance(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_light* light, uint32_t ns, uint32_t table,
                         const float* positions, const uint8_t* active, uint32_t W, uint32_t row_begin, uint32_t row_end,
                         float* distance, uint8_t* mask, int threads) {
    const int s = rts_bvh_validate(packed, count_vec4, nullptr);
    if (s != RTS_OK) return s;
    const uint32_t* bvh = (const uint32_t*)packed;
    const uint32_t lightType = light ? light->type : (uint32_t)RTS_LIGHT_DIRECTIONAL;
    const V3 L0 = light ? V3{ light->xyz[0], light->xyz[1], light->xyz[2] } : V3{ k->lightDirection[0], k->lightDirection[1], k->lightDirection[2] };
    const size_t first = (size_t)row_begin * W;
    parallelFor((size_t)(row_end - row_begin) * W, 64, threads, [&](size_t n) {
        const size_t i = first + n;
        if (active && !active[i]) { distance[i] = 0.0f; if (mask) mask[i] = 0; return; }
        const float* q = positions + i * 4;
        uint32_t best = 0x7F800000u, lit = 0;
        for (uint32_t j = 0; j < ns; ++j) {
            V3 L = L0;
            if (ns > 1) {
                const float* o = light->offsets[sampleIndex(table, j, (uint32_t)i)];
                L.x = L.x + o[0]; L.y = L.y + o[1]; L.z = L.z + o[2];
            }
            const uint32_t one = rayDistanceBits(bvh, shadowRay(k->cameraPosition, V3{ q[0], q[1], q[2] }, lightType, L));
            lit += one == 0x7F800000u ? 1u : 0u;                         // comp:148, per sample
            if (one < best) best = one;
        }
        distance[i] = asFloat(best);
        if (mask) mask[i] = (uint8_t)lit;                                // comp:150
    });
    return RTS_OK;
}

extern "C" int rtsh_shadow_distance(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_light* light,
                                    const float* positions, const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin,
                                    uint32_t row_end, float* distance, uint8_t* mask, int threads) {
    if (!packed || !k || !positions || !distance || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::hardLightOk(light)) return RTS_ERR_INVALID_ARG;            // one sample in this version
    return frameDistance(packed, count_vec4, k, light, 1u, 0u, positions, active, W, row_begin, row_end, distance, mask, threads);
}

extern "C" int rtsh_soft_distance(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_light* light,
                                  const float* positions, const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin,
                                  uint32_t row_end, float* distance, uint8_t* mask, int threads) {
    if (!packed || !k || !positions || !distance || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::softLightOk(light)) return RTS_ERR_INVALID_ARG;
    const uint32_t ns = (light && light->nsamples > 1) ? light->nsamples : 1u;
    return frameDistance(packed, count_vec4, k, light, ns, ns > 1 ? light->table : 0u, positions, active, W, row_begin, row_end, distance, mask, threads);
}

// ---- ambient occlusion on the host (include/rts_scene.h): the checker of rts_trace_ambient_occlusion*, and its rays as records ----
// The definition of include/rts.h as a straight loop over (pixel, sample): the frame and L from rts_closest_hit.h (aoFrame, aoAim: the
// kernels' own source), the point-light ray set-up and the one-ray distance of frameDistance.  aoPixelRays calls ray(j, r) for the n
// rays of an active, non-background pixel in sample order; -> false, and no position read, for any other pixel.
namespace rts_harness {
namespace {
template <class EachRay>
inline bool aoPixelRays(const rts_constants* k, const rts_ao_params* ao, uint32_t n, const float* positions, const float* normals,
                        const uint8_t* active, size_t i, EachRay&& ray) {
    const float* n4 = normals + i * 4;
    const V3 N{ n4[0], n4[1], n4[2] };
    if (isBackground(N) || (active && !active[i])) return false;
    const float* q = positions + i * 4;
    const V3 cam{ k->cameraPosition[0], k->cameraPosition[1], k->cameraPosition[2] }, rel{ q[0], q[1], q[2] };
    const AoFrame f = aoFrame(N);
    for (uint32_t j = 0; j < n; ++j) {
        const V3 L = aoAim(cam, rel, N, f, ao->dirs[sampleIndex(ao->table, j, (uint32_t)i)], ao->radius);
        ray(j, shadowRay(k->cameraPosition, rel, RTS_LIGHT_POINT, L));
    }
    return true;
}
} // namespace
} // namespace rts_harness

extern "C" int rtsh_ambient_occlusion(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_ao_params* ao,
                                      const float* positions, const float* normals, const uint8_t* active, uint32_t W, uint32_t H,
                                      uint32_t row_begin, uint32_t row_end, uint8_t* counts, int threads) {
    if (!packed || !k || !positions || !normals || !counts || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::aoParamsOk(ao)) return RTS_ERR_INVALID_ARG;
    const int s = rts_bvh_validate(packed, count_vec4, nullptr);
    if (s != RTS_OK) return s;
    const uint32_t* bvh = (const uint32_t*)packed;
    const uint32_t n = ao->nsamples > 1 ? ao->nsamples : 1u;
    const size_t first = (size_t)row_begin * W;
    parallelFor((size_t)(row_end - row_begin) * W, 64, threads, [&](size_t at) {
        const size_t i = first + at;
        uint32_t lit = 0;
        aoPixelRays(k, ao, n, positions, normals, active, i, [&](uint32_t, const DRay& r) {
            lit += rayDistanceBits(bvh, r) == 0x7F800000u ? 1u : 0u;    // u_j: comp:148, per sample
        });
        counts[i] = (uint8_t)lit;
    });
    return RTS_OK;
}

extern "C" int rtsh_ao_rays(const rts_constants* k, const rts_ao_params* ao, const float* positions, const float* normals,
                            const uint8_t* active, uint32_t W, uint32_t H, rts_ray* rays) {
    if (!k || !positions || !normals || !rays || W == 0 || H == 0 || !rts::aoParamsOk(ao)) return RTS_ERR_INVALID_ARG;
    const uint32_t n = ao->nsamples > 1 ? ao->nsamples : 1u;
    parallelFor((size_t)W * H, 256, 0, [&](size_t i) {                    // (every pixel writes its own n records)
        rts_ray* out = rays + i * n;
        memset(out, 0, sizeof(rts_ray) * n);
        aoPixelRays(k, ao, n, positions, normals, active, i, [&](uint32_t j, const DRay& r) {
            out[j] = rts_ray{ { r.o.x, r.o.y, r.o.z, r.tmax }, { r.d.x, r.d.y, r.d.z, 0.0f } };
        });
    });
    return RTS_OK;
}

// ---- adaptive ambient occlusion on the host (include/rts_scene.h): the checker of rts_trace_ambient_occlusion_adaptive* ----
// The definition of include/rts.h applied literally on rtsh_ambient_occlusion's walk and set-up (aoFrame, aoAim, the point light's ray
// at L): the probe's samples, then the others only where the probe disagrees.
extern "C" int rtsh_ambient_occlusion_adaptive(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_ao_params* ao,
                                               const float* positions, const float* normals, const uint8_t* active, uint32_t W, uint32_t H,
                                               uint32_t row_begin, uint32_t row_end, uint32_t probe, uint8_t* counts, uint8_t* refined,
                                               int threads) {
    if (!packed || !k || !positions || !normals || !counts || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::aoAdaptiveOk(ao, probe)) return RTS_ERR_INVALID_ARG;
    const int s = rts_bvh_validate(packed, count_vec4, nullptr);
    if (s != RTS_OK) return s;
    const uint32_t* bvh = (const uint32_t*)packed;
    const uint32_t n = ao->nsamples;
    const size_t first = (size_t)row_begin * W;
    parallelFor((size_t)(row_end - row_begin) * W, 64, threads, [&](size_t at) {
        const size_t i = first + at;
        if (refined) refined[i] = 0;
        const float* n4 = normals + i * 4;
        const V3 N{ n4[0], n4[1], n4[2] };
        if (isBackground(N) || (active && !active[i])) { counts[i] = 0; return; }
        const float* q = positions + i * 4;
        const V3 cam{ k->cameraPosition[0], k->cameraPosition[1], k->cameraPosition[2] }, rel{ q[0], q[1], q[2] };
        const AoFrame f = aoFrame(N);
        uint32_t lit = 0;
        for (uint32_t j = 0; j < n; ++j) {
            if (j == probe && (lit == 0 || lit == probe)) {              // the probe agrees: its verdict, no further ray
                counts[i] = (uint8_t)(lit ? n : 0u);
                return;
            }
            const V3 L = aoAim(cam, rel, N, f, ao->dirs[sampleIndex(ao->table, j, (uint32_t)i)], ao->radius);
            lit += rayDistanceBits(bvh, shadowRay(k->cameraPosition, rel, RTS_LIGHT_POINT, L)) == 0x7F800000u ? 1u : 0u;   // u_j
        }
        counts[i] = (uint8_t)lit;
        if (refined) refined[i] = 1;
    });
    return RTS_OK;
}

// ---- bent normals on the host (include/rts_scene.h): the checker of rts_trace_ambient_occlusion_bent* ----
// rtsh_ambient_occlusion's loop with the integer sum beside the count: aoQuantise of the sample's table entry where its ray is free,
// aoBent on the finished sum (rts_closest_hit.h: the kernels' own source).
extern "C" int rtsh_ambient_occlusion_bent(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_ao_params* ao,
                                           const float* positions, const float* normals, const uint8_t* active, uint32_t W, uint32_t H,
                                           uint32_t row_begin, uint32_t row_end, uint8_t* counts, float* bent, int threads) {
    if (!packed || !k || !positions || !normals || !bent || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::aoParamsOk(ao)) return RTS_ERR_INVALID_ARG;
    const int s = rts_bvh_validate(packed, count_vec4, nullptr);
    if (s != RTS_OK) return s;
    const uint32_t* bvh = (const uint32_t*)packed;
    const uint32_t n = ao->nsamples > 1 ? ao->nsamples : 1u;
    const size_t first = (size_t)row_begin * W;
    parallelFor((size_t)(row_end - row_begin) * W, 64, threads, [&](size_t at) {
        const size_t i = first + at;
        int32_t S[3] = { 0, 0, 0 };
        uint32_t lit = 0;
        const bool live = aoPixelRays(k, ao, n, positions, normals, active, i, [&](uint32_t j, const DRay& r) {
            if (rayDistanceBits(bvh, r) != 0x7F800000u) return;         // u_j == 0
            const float* d = ao->dirs[sampleIndex(ao->table, j, (uint32_t)i)];
            for (int c = 0; c < 3; ++c) S[c] += aoQuantise(d[c]);
            ++lit;
        });
        float* b = bent + i * 4;
        if (live) aoBent(V3{ normals[i * 4], normals[i * 4 + 1], normals[i * 4 + 2] }, S[0], S[1], S[2], lit, b);
        else b[0] = b[1] = b[2] = b[3] = 0.0f;
        if (counts) counts[i] = (uint8_t)lit;
    });
    return RTS_OK;
}

// ---- AO distance and falloff on the host (include/rts_scene.h): the checker of rts_trace_ambient_occlusion_distance* ----
// rtsh_ambient_occlusion's loop with the minimum and the weighted sum beside the count: aoOpenness of the sample's one-ray distance,
// aoObscurance on the finished sum (rts_closest_hit.h: the kernels' own source).
extern "C" int rtsh_ambient_occlusion_distance(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_ao_params* ao,
                                               const rts_ao_falloff* falloff, const float* positions, const float* normals,
                                               const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                               uint8_t* counts, float* distance, uint16_t* obscurance, int threads) {
    if (!packed || !k || !positions || !normals || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::aoParamsOk(ao) || (!distance && !obscurance) || (obscurance && !falloff)) return RTS_ERR_INVALID_ARG;
    if (((uintptr_t)obscurance & 1u) != 0 || ((uintptr_t)distance & 3u) != 0) return RTS_ERR_INVALID_ARG;
    const int s = rts_bvh_validate(packed, count_vec4, nullptr);
    if (s != RTS_OK) return s;
    const uint32_t* bvh = (const uint32_t*)packed;
    const uint32_t n = ao->nsamples > 1 ? ao->nsamples : 1u;
    const size_t first = (size_t)row_begin * W;
    parallelFor((size_t)(row_end - row_begin) * W, 64, threads, [&](size_t at) {
        const size_t i = first + at;
        uint32_t best = 0x7F800000u, lit = 0, open = 0;
        const bool live = aoPixelRays(k, ao, n, positions, normals, active, i, [&](uint32_t, const DRay& r) {
            const uint32_t one = rayDistanceBits(bvh, r);                // d_j
            lit += one == 0x7F800000u ? 1u : 0u;                         // u_j: comp:148, per sample
            if (one < best) best = one;
            if (obscurance) open += aoOpenness(one, [&](uint32_t b) { return falloff->weight[b]; });
        });
        if (counts) counts[i] = (uint8_t)lit;
        if (distance) distance[i] = live ? asFloat(best) : 0.0f;
        if (obscurance) obscurance[i] = live ? (uint16_t)aoObscurance(open, n) : (uint16_t)0;
    });
    return RTS_OK;
}

// ---- adaptive soft shadows on the host (include/rts_scene.h): the checker of rts_trace_shadow_mask_adaptive* ----
// The definition of include/rts.h applied literally, one straight loop over (pixel, sample) on frameDistance's walk: the probe's
// samples, then the others only where the probe disagrees.
extern "C" int rtsh_shadow_mask_adaptive(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_light* light,
                                         const float* positions, const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin,
                                         uint32_t row_end, uint32_t probe, uint8_t* mask, uint8_t* refined, int threads) {
    if (!packed || !k || !positions || !mask || !rts::frameRowsOk(W, H, row_begin, row_end)) return RTS_ERR_INVALID_ARG;
    if (!rts::adaptiveLightOk(light, probe)) return RTS_ERR_INVALID_ARG;
    const int s = rts_bvh_validate(packed, count_vec4, nullptr);
    if (s != RTS_OK) return s;
    const uint32_t* bvh = (const uint32_t*)packed;
    const uint32_t n = light->nsamples, table = light->table;
    const V3 L0{ light->xyz[0], light->xyz[1], light->xyz[2] };
    const size_t first = (size_t)row_begin * W;
    parallelFor((size_t)(row_end - row_begin) * W, 64, threads, [&](size_t at) {
        const size_t i = first + at;
        if (refined) refined[i] = 0;
        if (active && !active[i]) { mask[i] = 0; return; }
        const float* q = positions + i * 4;
        uint32_t lit = 0;
        for (uint32_t j = 0; j < n; ++j) {
            if (j == probe && (lit == 0 || lit == probe)) {              // the probe agrees: its verdict, no further ray
                mask[i] = (uint8_t)(lit ? n : 0u);
                return;
            }
            const float* o = light->offsets[sampleIndex(table, j, (uint32_t)i)];
            const V3 L{ L0.x + o[0], L0.y + o[1], L0.z + o[2] };
            const uint32_t one = rayDistanceBits(bvh, shadowRay(k->cameraPosition, V3{ q[0], q[1], q[2] }, light->type, L));
            lit += one == 0x7F800000u ? 1u : 0u;                         // comp:148, per sample
        }
        mask[i] = (uint8_t)lit;                                          // comp:150
        if (refined) refined[i] = 1;
    });
    return RTS_OK;
}

// ---- light lists on the host (include/rts_scene.h): the checker of rts_trace_light_list*, and the light map of a deferred renderer ----
// The definition of include/rts.h as a straight loop over (pixel, light): light l's ray and one-ray distance as rtsh_shadow_distance
// takes them for that light alone, its bit set where the distance is +Inf.
namespace rts_harness {
namespace {
// One light of a list as makeCombineParams reads it: its type, its sample count and its position or direction.
rts_light lightOf(uint32_t type, uint32_t nsamples, const float* xyz) {
    rts_light one;
    memset(&one, 0, sizeof(one));
    one.type = type;
    one.nsamples = nsamples;
    for (int i = 0; i < 3; ++i) one.xyz[i] = xyz[i];
    return one;
}
} // namespace

// Shared by the host and device facing passes: one CombineParams per light, as makeCombineParams condenses that light alone.
int makeFacingLights(const rts_constants* k, const rts_light_list* list, bool havePositions, FacingLights* out) {
    if (!k || !out || !rts::lightListOk(list)) return RTS_ERR_INVALID_ARG;
    out->count = list->count;
    for (uint32_t l = 0; l < list->count; ++l) {
        const rts_light one = lightOf(list->lights[l].type, 1u, list->lights[l].xyz);
        const int s = makeCombineParams(k, &one, havePositions, &out->light[l]);
        if (s != RTS_OK) return s;
    }
    return RTS_OK;
}
} // namespace rts_harness

extern "C" int rtsh_light_list(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_light_list* list,
                               const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                               uint32_t row_end, uint8_t* mask, int threads) {
    if (!packed || !k || !positions || !mask || !rts::frameRowsOk(W, H, row_begin, row_end) || !rts::lightListOk(list)) return RTS_ERR_INVALID_ARG;
    const int s = rts_bvh_validate(packed, count_vec4, nullptr);
    if (s != RTS_OK) return s;
    const uint32_t* bvh = (const uint32_t*)packed;
    const uint32_t below = (1u << list->count) - 1u;
    const size_t first = (size_t)row_begin * W;
    parallelFor((size_t)(row_end - row_begin) * W, 64, threads, [&](size_t n) {
        const size_t i = first + n;
        const uint32_t bits = (lights_map ? lights_map[i] : 0xFFu) & below;
        uint32_t byte = 0;
        if (bits) {
            const float* q = positions + i * 4;
            for (uint32_t l = 0; l < list->count; ++l) {
                if (!((bits >> l) & 1u)) continue;
                const rts_light_entry& e = list->lights[l];
                const uint32_t one = rayDistanceBits(bvh, shadowRay(k->cameraPosition, V3{ q[0], q[1], q[2] }, e.type, V3{ e.xyz[0], e.xyz[1], e.xyz[2] }));
                byte |= one == 0x7F800000u ? 1u << l : 0u;                 // comp:148, as light l's bit
            }
        }
        mask[i] = (uint8_t)byte;                                          // comp:150
    });
    return RTS_OK;
}

// ---- soft light lists on the host (include/rts_scene.h): the checker of rts_trace_soft_light_list*, their distance, adaptive and
// jittered forms ----
// The definition of include/rts.h as ONE straight loop over (pixel, light, sample), every form a thin caller of it:
//   the aim      a sample of a soft entry aims at xyz + radius * offsets[at] -- the product rounded on its own (this file is built
//                without FMA contraction), then frameDistance's add --, a hard entry at xyz as given;
//   counts       the plane's byte counts the samples whose one-ray distance is +Inf;
//   distances    frameDistance's integer minimum per light, +0 where the map's bit is clear;
//   probes       per light rtsh_shadow_mask_adaptive's decision after the probe's samples, `refined` the lights that walked them all;
//   tables       sampleIndex(T_l, j, pixel) in front of the offset; without tables sampleIndex(0, j, .) is j.
// NULL for distances, counts, probes, tables or refined is the trace without them.
namespace rts_harness {
namespace {
inline V3 softListAim(const rts_soft_light_entry& e, const float (*offsets)[4], uint32_t at) {
    const float* o = offsets[at];
    const float ox = e.radius * o[0], oy = e.radius * o[1], oz = e.radius * o[2];
    return V3{ e.xyz[0] + ox, e.xyz[1] + oy, e.xyz[2] + oz };
}

// rows [row_begin, row_end) of a frame (the arguments checked by the caller, each form by its own rule)
int softListFrame(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_soft_light_list* list, const float* positions,
                  const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, float* distances, uint8_t* counts,
                  const uint32_t* probes, const uint32_t* tables, uint8_t* refined, int threads) {
    const int s = rts_bvh_validate(packed, count_vec4, nullptr);
    if (s != RTS_OK) return s;
    const uint32_t* bvh = (const uint32_t*)packed;
    const uint32_t below = (1u << list->count) - 1u;
    const size_t first = (size_t)row_begin * W, plane = (size_t)W * H;
    parallelFor((size_t)(row_end - row_begin) * W, 64, threads, [&](size_t n) {
        const size_t i = first + n;
        const uint32_t bits = (lights_map ? lights_map[i] : 0xFFu) & below;
        const float* q = positions + i * 4;                              // (not read where bits == 0)
        uint32_t took = 0;
        for (uint32_t l = 0; l < list->count; ++l) {
            uint32_t best = 0u, lit = 0;                                 // (+0.0f and 0 where the map's bit is clear)
            if ((bits >> l) & 1u) {
                const rts_soft_light_entry& e = list->lights[l];
                const uint32_t ns = e.nsamples > 1 ? e.nsamples : 1u, probe = probes ? probes[l] : 0u, table = tables ? tables[l] : 0u;
                best = 0x7F800000u;
                uint32_t j = 0;
                for (; j < ns; ++j) {
                    if (probe != 0 && j == probe && (lit == 0 || lit == probe)) break;      // the probe agrees: its verdict, no further ray
                    const V3 L = ns > 1 ? softListAim(e, list->offsets, e.first + sampleIndex(table, j, (uint32_t)i))
                                        : V3{ e.xyz[0], e.xyz[1], e.xyz[2] };
                    const uint32_t one = rayDistanceBits(bvh, shadowRay(k->cameraPosition, V3{ q[0], q[1], q[2] }, e.type, L));
                    lit += one == 0x7F800000u ? 1u : 0u;                 // comp:148, per sample
                    if (one < best) best = one;
                }
                if (j < ns) lit = lit ? ns : 0u;                         // (left at the probe)
                else if (probe != 0) took |= 1u << l;                    // every sample walked because the probe disagreed
            }
            if (distances) distances[l * plane + i] = asFloat(best);
            if (counts) counts[l * plane + i] = (uint8_t)lit;            // comp:150
        }
        if (refined) refined[i] = (uint8_t)took;
    });
    return RTS_OK;
}
} // namespace
} // namespace rts_harness

extern "C" int rtsh_soft_light_list(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_soft_light_list* list,
                                    const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                                    uint32_t row_end, uint8_t* counts, int threads) {
    if (!packed || !k || !positions || !counts || !rts::frameRowsOk(W, H, row_begin, row_end) || !rts::softListOk(list)) return RTS_ERR_INVALID_ARG;
    return softListFrame(packed, count_vec4, k, list, positions, lights_map, W, H, row_begin, row_end, nullptr, counts, nullptr, nullptr, nullptr,
                         threads);
}

extern "C" int rtsh_soft_light_list_distance(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_soft_light_list* list,
                                             const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                                             uint32_t row_end, float* distances, uint8_t* counts, int threads) {
    if (!packed || !k || !positions || !distances || !rts::frameRowsOk(W, H, row_begin, row_end) || !rts::softListOk(list)) return RTS_ERR_INVALID_ARG;
    return softListFrame(packed, count_vec4, k, list, positions, lights_map, W, H, row_begin, row_end, distances, counts, nullptr, nullptr, nullptr,
                         threads);
}

extern "C" int rtsh_soft_light_list_jittered(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_soft_light_list* list,
                                             const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                                             uint32_t row_end, uint8_t* counts, const uint32_t* probes, const uint32_t* tables, uint8_t* refined,
                                             int threads) {
    if (!packed || !k || !positions || !counts || !rts::frameRowsOk(W, H, row_begin, row_end) || !rts::softListTablesOk(list, probes, tables))
        return RTS_ERR_INVALID_ARG;
    return softListFrame(packed, count_vec4, k, list, positions, lights_map, W, H, row_begin, row_end, nullptr, counts, probes, tables, refined,
                         threads);
}

extern "C" int rtsh_soft_light_list_adaptive(const rts_vec4u* packed, size_t count_vec4, const rts_constants* k, const rts_soft_light_list* list,
                                             const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                                             uint32_t row_end, uint8_t* counts, const uint32_t* probes, uint8_t* refined, int threads) {
    return rtsh_soft_light_list_jittered(packed, count_vec4, k, list, positions, lights_map, W, H, row_begin, row_end, counts, probes, nullptr,
                                         refined, threads);
}

extern "C" int rtsh_facing_lights(const rts_constants* k, const rts_light_list* list, const float* positions, const float* normals,
                                  uint32_t W, uint32_t H, uint8_t* lights_map) {
    if (!normals || !lights_map || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    FacingLights f;
    const int s = makeFacingLights(k, list, positions != nullptr, &f);
    if (s != RTS_OK) return s;
    const float zero[4] = { 0, 0, 0, 0 };
    for (size_t i = 0; i < (size_t)W * H; ++i) lights_map[i] = facingLightsPixel(f, positions ? positions + i * 4 : zero, normals + i * 4);
    return RTS_OK;
}

// ---- the combine pass of a light list (include/rts_scene.h; per-pixel rule in rts_closest_hit.h: combineListPixel) ----
namespace rts_harness {
// Shared by the host and device list combine passes: one CombineParams per light, as makeCombineParams condenses that light alone
// (type, xyz and its sample count; an area light counts by its centre), and the colours -- count * 4 floats, .w ignored, NULL = white.
static int makeCombineListOf(const rts_constants* k, uint32_t count, const uint32_t* types, const uint32_t* nsamples, const float (*xyz)[3],
                             const float* colors, bool havePositions, CombineList* out) {
    out->count = count;
    for (uint32_t l = 0; l < count; ++l) {
        const rts_light one = lightOf(types[l], nsamples[l], xyz[l]);
        const int s = makeCombineParams(k, &one, havePositions, &out->light[l]);
        if (s != RTS_OK) return s;
        for (int c = 0; c < 3; ++c) out->color[l][c] = colors ? colors[l * 4 + c] : 1.0f;
    }
    for (uint32_t l = count; l < 8; ++l) {                               // (never looked at: defined bytes for the by-value copy)
        out->light[l] = out->light[0];
        for (int c = 0; c < 3; ++c) out->color[l][c] = 0.0f;
    }
    return RTS_OK;
}

int makeCombineList(const rts_constants* k, const rts_light_list* list, const float* colors, bool havePositions, CombineList* out) {
    if (!k || !out || !rts::lightListOk(list)) return RTS_ERR_INVALID_ARG;
    uint32_t types[8], ns[8];
    float xyz[8][3];
    for (uint32_t l = 0; l < list->count; ++l) {
        types[l] = list->lights[l].type;
        ns[l] = 1u;
        for (int i = 0; i < 3; ++i) xyz[l][i] = list->lights[l].xyz[i];
    }
    return makeCombineListOf(k, list->count, types, ns, xyz, colors, havePositions, out);
}

int makeCombineSoftList(const rts_constants* k, const rts_soft_light_list* list, const float* colors, bool havePositions, CombineList* out) {
    if (!k || !out || !rts::softListOk(list)) return RTS_ERR_INVALID_ARG;
    uint32_t types[8], ns[8];
    float xyz[8][3];
    for (uint32_t l = 0; l < list->count; ++l) {
        types[l] = list->lights[l].type;
        ns[l] = list->lights[l].nsamples;
        for (int i = 0; i < 3; ++i) xyz[l][i] = list->lights[l].xyz[i];
    }
    return makeCombineListOf(k, list->count, types, ns, xyz, colors, havePositions, out);
}

namespace {
// The frame walk of the three list combines: pixel(i, position, normal, bits) for every pixel, bits its byte of the light map -- every
// light where there is no map, and on the background, whose map byte is not read.
template <class Pixel>
void combineFrame(const float* positions, const float* normals, const uint8_t* lights_map, size_t n, Pixel&& pixel) {
    const float zero[4] = { 0, 0, 0, 0 };
    for (size_t i = 0; i < n; ++i) {
        const float* n4 = normals + i * 4;
        const bool background = n4[0] == 0.0f && n4[1] == 0.0f && n4[2] == 0.0f;
        pixel(i, positions ? positions + i * 4 : zero, n4, (lights_map && !background) ? lights_map[i] : 0xFFu);
    }
}
} // namespace
} // namespace rts_harness

extern "C" int rtsh_combine_light_list(const rts_constants* k, const rts_light_list* list, const float* colors, const float* positions,
                                       const float* normals, const uint8_t* lights_map, const uint8_t* mask, uint32_t W, uint32_t H,
                                       uint8_t* rgb) {
    if (!k || !normals || !mask || !rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    CombineList f;
    const int s = makeCombineList(k, list, colors, positions != nullptr, &f);
    if (s != RTS_OK) return s;
    combineFrame(positions, normals, lights_map, (size_t)W * H, [&](size_t i, const float* p4, const float* n4, uint32_t bits) {
        combineListPixel(f, p4, n4, bits, [&](uint32_t l) { return (uint8_t)((mask[i] >> l) & 1u); }, rgb + i * 3);
    });
    return RTS_OK;
}

extern "C" int rtsh_combine_soft_light_list(const rts_constants* k, const rts_soft_light_list* list, const float* colors, const float* positions,
                                            const float* normals, const uint8_t* lights_map, const uint8_t* counts, uint32_t W, uint32_t H,
                                            uint8_t* rgb) {
    if (!k || !normals || !counts || !rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    CombineList f;
    const int s = makeCombineSoftList(k, list, colors, positions != nullptr, &f);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    combineFrame(positions, normals, lights_map, n, [&](size_t i, const float* p4, const float* n4, uint32_t bits) {
        combineListPixel(f, p4, n4, bits, [&](uint32_t l) { return counts[(size_t)l * n + i]; }, rgb + i * 3);
    });
    return RTS_OK;
}

// ---- the filter of a light list's planes and the visibility combine (include/rts_scene.h; per-pixel rules in rts_closest_hit.h:
// filterListPixel, combineVisibilityPixel) ----
namespace rts_harness {
// Shared by the host and device filters: the refusals of the parameters and the condensed form the per-pixel rule reads.
int makeFilterList(uint32_t count, const uint32_t* nsamples, const rtsh_filter_params* p, bool withDistances, FilterList* out) {
    if (!p || !out || p->radius > (uint32_t)RTSH_FILTER_MAX_RADIUS || !std::isfinite(p->normal_cos_min) || !std::isfinite(p->plane_eps))
        return RTS_ERR_INVALID_ARG;
    out->count = count;
    out->radius = p->radius;
    out->normalCosMin = p->normal_cos_min;
    out->planeEps = p->plane_eps;
    for (uint32_t l = 0; l < 8; ++l) {
        const bool used = l < count;
        if (used && withDistances && !(std::isfinite(p->spread[l]) && p->spread[l] >= 0.0f)) return RTS_ERR_INVALID_ARG;
        out->samples[l] = used && nsamples && nsamples[l] > 1u ? nsamples[l] : 1u;
        out->spread[l] = used && withDistances ? p->spread[l] : 0.0f;              // (defined bytes for the by-value copy)
    }
    return RTS_OK;
}

int makeFilterHardList(const rts_light_list* list, const rtsh_filter_params* p, FilterList* out) {
    if (!rts::lightListOk(list)) return RTS_ERR_INVALID_ARG;
    return makeFilterList(list->count, nullptr, p, false, out);
}

int makeFilterSoftList(const rts_soft_light_list* list, const rtsh_filter_params* p, bool withDistances, FilterList* out) {
    if (!rts::softListOk(list)) return RTS_ERR_INVALID_ARG;
    uint32_t ns[8];
    for (uint32_t l = 0; l < list->count; ++l) ns[l] = list->lights[l].nsamples;
    return makeFilterList(list->count, ns, p, withDistances, out);
}

namespace {
// The frame as filterListPixel reads it on the host: straight from the buffers.
template <bool HARD>
struct FrameTexels {
    const float *positions, *normals, *distances;
    const uint8_t *map, *planes;
    size_t W, n;
    size_t at(int x, int y) const { return (size_t)y * W + (size_t)x; }
    V3 normal(int x, int y) const { const float* v = normals + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    V3 position(int x, int y) const { const float* v = positions + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    uint32_t bits(int x, int y) const { return map ? map[at(x, y)] : 0xFFu; }
    uint32_t byte(int x, int y, uint32_t l) const { return HARD ? (planes[at(x, y)] >> l) & 1u : planes[(size_t)l * n + at(x, y)]; }
    uint32_t distance(int x, int y, uint32_t l) const { uint32_t u; memcpy(&u, distances + (size_t)l * n + at(x, y), 4); return u; }
};

template <bool HARD>
void filterListFrame(const FilterList& f, const float* positions, const float* normals, const uint8_t* lights_map, const uint8_t* planes,
                     const float* distances, uint32_t W, uint32_t H, float* visibility, int threads) {
    const size_t n = (size_t)W * H;
    const FrameTexels<HARD> t{ positions, normals, distances, lights_map, planes, W, n };
    parallelFor(n, 256, threads, [&](size_t i) {
        float v[8];
        const int x = (int)(i % W), y = (int)(i / W);
        if (distances) filterListPixel<true>(f, t, x, y, (int)W, (int)H, 0xFFu, v);
        else filterListPixel<false>(f, t, x, y, (int)W, (int)H, 0xFFu, v);
        for (uint32_t l = 0; l < f.count; ++l) visibility[(size_t)l * n + i] = v[l];
    });
}
} // namespace
} // namespace rts_harness

extern "C" int rtsh_filter_light_list(const rts_light_list* list, const rtsh_filter_params* params, const float* positions,
                                      const float* normals, const uint8_t* lights_map, const uint8_t* mask, uint32_t W, uint32_t H,
                                      float* visibility, int threads) {
    if (!positions || !normals || !mask || !visibility || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    FilterList f;
    const int s = makeFilterHardList(list, params, &f);
    if (s != RTS_OK) return s;
    filterListFrame<true>(f, positions, normals, lights_map, mask, nullptr, W, H, visibility, threads);
    return RTS_OK;
}

extern "C" int rtsh_filter_soft_light_list(const rts_soft_light_list* list, const rtsh_filter_params* params, const float* positions,
                                           const float* normals, const uint8_t* lights_map, const uint8_t* counts, const float* distances,
                                           uint32_t W, uint32_t H, float* visibility, int threads) {
    if (!positions || !normals || !counts || !visibility || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    FilterList f;
    const int s = makeFilterSoftList(list, params, distances != nullptr, &f);
    if (s != RTS_OK) return s;
    filterListFrame<false>(f, positions, normals, lights_map, counts, distances, W, H, visibility, threads);
    return RTS_OK;
}

extern "C" int rtsh_combine_visibility_list(const rts_constants* k, const rts_light_list* list, const float* colors, const float* positions,
                                            const float* normals, const uint8_t* lights_map, const float* visibility, uint32_t W, uint32_t H,
                                            uint8_t* rgb) {
    if (!k || !normals || !visibility || !rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    CombineList f;
    const int s = makeCombineList(k, list, colors, positions != nullptr, &f);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    combineFrame(positions, normals, lights_map, n, [&](size_t i, const float* p4, const float* n4, uint32_t bits) {
        combineVisibilityPixel(f, p4, n4, bits, [&](uint32_t l) { return visibility[(size_t)l * n + i]; }, rgb + i * 3);
    });
    return RTS_OK;
}

extern "C" int rtsh_combine_visibility_list_ao(const rts_constants* k, const rts_light_list* list, const float* colors, const float* positions,
                                               const float* normals, const uint8_t* lights_map, const float* visibility, const float* ao,
                                               uint32_t W, uint32_t H, uint8_t* rgb) {
    if (!k || !normals || !visibility || !ao || !rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    CombineList f;
    const int s = makeCombineList(k, list, colors, positions != nullptr, &f);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    combineFrame(positions, normals, lights_map, n, [&](size_t i, const float* p4, const float* n4, uint32_t bits) {
        combineVisibilityPixel(f, p4, n4, bits, [&](uint32_t l) { return visibility[(size_t)l * n + i]; },
                               [&](float ambient) { return ambient * ao[i]; }, rgb + i * 3);
    });
    return RTS_OK;
}

extern "C" int rtsh_combine_visibility_list_ao_bent(const rts_constants* k, const rts_light_list* list, const float* colors,
                                                    const float* positions, const float* normals, const uint8_t* lights_map,
                                                    const float* visibility, const float* ao, const float* bent, const rtsh_sky_ambient* sky,
                                                    uint32_t W, uint32_t H, uint8_t* rgb) {
    if (!k || !normals || !visibility || !ao || !bent || !sky || !rgb || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    CombineList f;
    const int s = makeCombineList(k, list, colors, positions != nullptr, &f);
    if (s != RTS_OK) return s;
    float sky9[9];
    memcpy(sky9, sky, sizeof(sky9));                                       // { up, sky, ground }
    const size_t n = (size_t)W * H;
    combineFrame(positions, normals, lights_map, n, [&](size_t i, const float* p4, const float* n4, uint32_t bits) {
        combineVisibilityPixelRgb(f, p4, n4, bits, [&](uint32_t l) { return visibility[(size_t)l * n + i]; },
                                  [&](float ambient, float* out3) { skyAmbient3(ambient, ao[i], sky9, bent + i * 4, out3); }, rgb + i * 3);
    });
    return RTS_OK;
}

// ---- the wide filter of a light list's planes (include/rts_scene.h; per-pixel rule in rts_closest_hit.h: wideFilterPassPixel) ----
namespace rts_harness {
// Shared by the host and device forms: the refusals of the parameters and of the frame, and the condensed form the per-pixel rule reads.
int makeWideFilterList(uint32_t count, const uint32_t* nsamples, const rtsh_wide_filter_params* p, uint32_t W, uint32_t H,
                       WideFilterList* out) {
    if (!p || !out || p->passes > (uint32_t)RTSH_WIDE_FILTER_MAX_PASSES || !std::isfinite(p->normal_cos_min) || !std::isfinite(p->plane_eps))
        return RTS_ERR_INVALID_ARG;
    if (W == 0 || H == 0 || W > 0x7FFFFFF0u || H > 0x7FFFFFF0u) return RTS_ERR_INVALID_ARG;
    out->count = count;
    out->passes = p->passes;
    out->normalCosMin = p->normal_cos_min;
    out->planeEps = p->plane_eps;
    for (uint32_t l = 0; l < 8; ++l) {
        out->samples[l] = l < count && nsamples && nsamples[l] > 1u ? nsamples[l] : 1u;
        out->scale[l] = wideFilterScale(out->samples[l]);
    }
    return RTS_OK;
}

int makeWideFilterHardList(const rts_light_list* list, const rtsh_wide_filter_params* p, uint32_t W, uint32_t H, WideFilterList* out) {
    if (!rts::lightListOk(list)) return RTS_ERR_INVALID_ARG;
    return makeWideFilterList(list->count, nullptr, p, W, H, out);
}

int makeWideFilterSoftList(const rts_soft_light_list* list, const rtsh_wide_filter_params* p, uint32_t W, uint32_t H, WideFilterList* out) {
    if (!rts::softListOk(list)) return RTS_ERR_INVALID_ARG;
    uint32_t ns[8];
    for (uint32_t l = 0; l < list->count; ++l) ns[l] = list->lights[l].nsamples;
    return makeWideFilterList(list->count, ns, p, W, H, out);
}

namespace {
// The first pass's input rule: V_0 of light l at texel `at` from the mask byte of a hard list, from the count bytes of a soft list, or
// V_0' from the accumulated mean (plane l at + l * n).
struct WideHardInput {
    const uint8_t* mask;
    uint32_t operator()(size_t at, uint32_t l, size_t, uint32_t samples, uint32_t scale) const {
        return wideFilterInput((mask[at] >> l) & 1u, samples, scale);
    }
};
struct WideSoftInput {
    const uint8_t* counts;
    uint32_t operator()(size_t at, uint32_t l, size_t n, uint32_t samples, uint32_t scale) const {
        return wideFilterInput(counts[(size_t)l * n + at], samples, scale);
    }
};
struct WideMeanInput {
    const uint16_t* mean;
    uint32_t operator()(size_t at, uint32_t l, size_t n, uint32_t samples, uint32_t scale) const {
        return wideMeanInput(mean[(size_t)l * n + at], samples, scale);
    }
};

// The frame as a pass reads it on the host: the G-buffer and the map straight from the buffers, V_k from the input rule (the first pass)
// or from the previous pass's 16-bit planes.
template <class Input>
struct WideFrameTexels {
    const float *positions, *normals;
    const uint8_t* map;
    Input input;
    const uint16_t* values;                      // the previous pass's planes; NULL: the first pass
    const uint32_t *samples, *scale;
    size_t W, n;
    size_t at(int x, int y) const { return (size_t)y * W + (size_t)x; }
    V3 normal(int x, int y) const { const float* v = normals + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    V3 position(int x, int y) const { const float* v = positions + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    uint32_t bits(int x, int y) const { return map ? map[at(x, y)] : 0xFFu; }
    uint32_t value(int x, int y, uint32_t l) const {
        if (values) return values[(size_t)l * n + at(x, y)];
        return input(at(x, y), l, n, samples[l], scale[l]);
    }
};

// THE ONE CHAIN OF A CALL, for the five host twins: max(1, passes) passes, pass k from the input rule (k == 0) or from set (k - 1) & 1
// of the scratch into set k & 1, the last one into visibility.  threshold(texels, x, y, T) is the first pass's rule of a guided chain:
// T goes to a third set of planes behind the two ping-pong sets, as in the device form, and later passes read it there.  nullptr: the
// unguided chain, two sets.
template <class Input, class Threshold>
int widePassChain(const WideFilterList& f, const float* positions, const float* normals, const uint8_t* lights_map, const Input& input,
                  uint32_t W, uint32_t H, float* visibility, int threads, const Threshold& threshold) {
    constexpr bool GUIDED = !std::is_same<Threshold, std::nullptr_t>::value;
    const size_t n = (size_t)W * H, set = (size_t)f.count * n;
    std::vector<uint16_t> scratch;
    try {
        if (f.passes >= 2u) scratch.resize((GUIDED ? 3 : 2) * set);
    } catch (const std::bad_alloc&) {
        return RTS_ERR_CAPACITY;
    }
    const uint32_t launches = f.passes == 0u ? 1u : f.passes;
    for (uint32_t k = 0; k < launches; ++k) {
        const bool first = k == 0u, last = k + 1u == launches;
        const int step = f.passes == 0u ? 0 : 1 << k;
        const uint16_t* in = first ? nullptr : scratch.data() + ((k - 1u) & 1u) * set;
        uint16_t* out = last ? nullptr : scratch.data() + (k & 1u) * set;
        uint16_t* guide = GUIDED && f.passes >= 2u ? scratch.data() + 2 * set : nullptr;
        const WideFrameTexels<Input> t{ positions, normals, lights_map, input, in, f.samples, f.scale, W, n };
        parallelFor(n, 256, threads, [&](size_t i) {
            const int x = (int)(i % W), y = (int)(i / W);
            uint32_t v[8];
            if constexpr (GUIDED) {
                uint32_t T[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
                if (first) {
                    if (step > 0) threshold(t, x, y, T);
                    if (!last) for (uint32_t l = 0; l < f.count; ++l) guide[(size_t)l * n + i] = (uint16_t)T[l];
                } else {
                    for (uint32_t l = 0; l < f.count; ++l) T[l] = guide[(size_t)l * n + i];
                }
                wideGuidedPassPixel(f, t, x, y, (int)W, (int)H, step, T, v);
            } else {
                wideFilterPassPixel(f, t, x, y, (int)W, (int)H, step, v);
            }
            for (uint32_t l = 0; l < f.count; ++l) {
                if (last) visibility[(size_t)l * n + i] = wideFilterOutput(v[l], f.samples[l], f.scale[l]);
                else out[(size_t)l * n + i] = (uint16_t)v[l];
            }
        });
    }
    return RTS_OK;
}

size_t wideScratchBytes(size_t sets, uint32_t count, uint32_t W, uint32_t H) {
    if (count == 0 || count > 8u || W == 0 || H == 0) return 0;
    return sets * (size_t)count * (size_t)W * (size_t)H * sizeof(uint16_t);
}
} // namespace
} // namespace rts_harness

extern "C" size_t rtsh_wide_filter_scratch_bytes(uint32_t count, uint32_t W, uint32_t H) { return wideScratchBytes(2, count, W, H); }

extern "C" int rtsh_wide_filter_light_list(const rts_light_list* list, const rtsh_wide_filter_params* params, const float* positions,
                                           const float* normals, const uint8_t* lights_map, const uint8_t* mask, uint32_t W, uint32_t H,
                                           float* visibility, int threads) {
    if (!positions || !normals || !mask || !visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int s = makeWideFilterHardList(list, params, W, H, &f);
    if (s != RTS_OK) return s;
    return widePassChain(f, positions, normals, lights_map, WideHardInput{ mask }, W, H, visibility, threads, nullptr);
}

extern "C" int rtsh_wide_filter_soft_light_list(const rts_soft_light_list* list, const rtsh_wide_filter_params* params, const float* positions,
                                                const float* normals, const uint8_t* lights_map, const uint8_t* counts, uint32_t W,
                                                uint32_t H, float* visibility, int threads) {
    if (!positions || !normals || !counts || !visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int s = makeWideFilterSoftList(list, params, W, H, &f);
    if (s != RTS_OK) return s;
    return widePassChain(f, positions, normals, lights_map, WideSoftInput{ counts }, W, H, visibility, threads, nullptr);
}

// ---- the wide filter of the bent plane (include/rts_scene.h; per-pixel rule in rts_closest_hit.h: bentFilterPassPixel) ----
namespace rts_harness {
// Shared by the host and device forms: the refusals of the parameters, of the frame and of the sample count, and n, S_b, S_l.
int makeBentFilterList(const rtsh_wide_filter_params* p, uint32_t nsamples, uint32_t W, uint32_t H, BentFilterList* out) {
    WideFilterList w;
    const int s = makeWideFilterList(1, &nsamples, p, W, H, &w);
    if (s != RTS_OK) return s;
    if (!out || nsamples > (uint32_t)RTS_AO_MAX_SAMPLES) return RTS_ERR_INVALID_ARG;
    *out = BentFilterList{ w.passes, w.samples[0], bentFilterScale(w.samples[0]), w.scale[0], w.normalCosMin, w.planeEps };
    return RTS_OK;
}

namespace {
// The frame as a pass reads it on the host: the first pass quantises the float texel, later ones unpack the previous pass's 8 bytes.
struct BentFrameTexels {
    const float *positions, *normals, *bent;
    const uint8_t* map;
    const uint64_t* values;                      // the previous pass's plane; NULL: the first pass
    const BentFilterList& f;
    size_t W;
    size_t at(int x, int y) const { return (size_t)y * W + (size_t)x; }
    V3 normal(int x, int y) const { const float* v = normals + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    V3 position(int x, int y) const { const float* v = positions + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    bool active(int x, int y) const { return !map || map[at(x, y)] != 0; }
    BentTexel texel(int x, int y) const {
        if (values) return bentFilterUnpack(values[at(x, y)]);
        const float* b = bent + at(x, y) * 4;
        return bentFilterInput(b[0], b[1], b[2], b[3], f);
    }
};
} // namespace
} // namespace rts_harness

extern "C" size_t rtsh_wide_filter_bent_scratch_bytes(uint32_t W, uint32_t H) {
    return W == 0 || H == 0 ? 0 : 2 * (size_t)W * (size_t)H * sizeof(uint64_t);
}

extern "C" int rtsh_wide_filter_bent(const rtsh_wide_filter_params* params, uint32_t nsamples, const float* positions, const float* normals,
                                     const uint8_t* active, const float* bent, uint32_t W, uint32_t H, float* out, float* ao, int threads) {
    if (!positions || !normals || !bent || !out) return RTS_ERR_INVALID_ARG;
    BentFilterList f;
    const int s = makeBentFilterList(params, nsamples, W, H, &f);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    std::vector<uint64_t> scratch;
    try {
        if (f.passes >= 2u) scratch.resize(2 * n);
    } catch (const std::bad_alloc&) {
        return RTS_ERR_CAPACITY;
    }
    const uint32_t launches = f.passes == 0u ? 1u : f.passes;
    for (uint32_t k = 0; k < launches; ++k) {
        const bool first = k == 0u, last = k + 1u == launches;
        const int step = f.passes == 0u ? 0 : 1 << k;
        const uint64_t* in = first ? nullptr : scratch.data() + ((k - 1u) & 1u) * n;
        uint64_t* mid = last ? nullptr : scratch.data() + (k & 1u) * n;
        const BentFrameTexels t{ positions, normals, bent, active, in, f, W };
        parallelFor(n, 256, threads, [&](size_t i) {
            BentTexel v;
            bentFilterPassPixel(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H, step, &v);
            if (!last) { mid[i] = bentFilterPack(v); return; }
            float* o = out + i * 4;
            o[0] = bentFilterOutput(v.x, f.samples, f.scaleB);
            o[1] = bentFilterOutput(v.y, f.samples, f.scaleB);
            o[2] = bentFilterOutput(v.z, f.samples, f.scaleB);
            o[3] = wideFilterOutput(v.v, f.samples, f.scaleL);
            if (ao) ao[i] = o[3];
        });
    }
    return RTS_OK;
}

// ---- the variance-guided wide filter of a soft light list's planes (include/rts_scene.h; per-pixel rule in rts_closest_hit.h:
// wideGuideThresholdPixel, wideGuidedPassPixel) ----
namespace rts_harness {
// Shared by the host and device forms: the refusals, and the unguided filter's condensed list.
int makeWideGuidedList(const rts_soft_light_list* list, const rtsh_wide_guide_params* p, uint32_t W, uint32_t H, WideFilterList* out) {
    if (!p || p->guide_k4 > (uint32_t)RTSH_WIDE_GUIDE_MAX_K4) return RTS_ERR_INVALID_ARG;
    rtsh_wide_filter_params q;
    std::memset(&q, 0, sizeof(q));
    q.passes = p->passes; q.normal_cos_min = p->normal_cos_min; q.plane_eps = p->plane_eps;
    return makeWideFilterSoftList(list, &q, W, H, out);
}
} // namespace rts_harness

extern "C" size_t rtsh_wide_filter_guided_scratch_bytes(uint32_t count, uint32_t W, uint32_t H) { return wideScratchBytes(3, count, W, H); }

extern "C" uint32_t rtsh_wide_guide_threshold(uint64_t G, uint32_t D, uint32_t n, uint32_t guide_k4) {
    if (D == 0 || n == 0) return 65535u;
    return wideGuideThreshold(G, D, n, guide_k4);
}

extern "C" int rtsh_wide_filter_guided_soft_light_list(const rts_soft_light_list* list, const rtsh_wide_guide_params* params,
                                                       const float* positions, const float* normals, const uint8_t* lights_map,
                                                       const uint8_t* counts, uint32_t W, uint32_t H, float* visibility, int threads) {
    if (!positions || !normals || !counts || !visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int s = makeWideGuidedList(list, params, W, H, &f);
    if (s != RTS_OK) return s;
    const uint32_t k4 = params->guide_k4;
    return widePassChain(f, positions, normals, lights_map, WideSoftInput{ counts }, W, H, visibility, threads,
                         [&](const auto& t, int x, int y, uint32_t* T) { wideGuideThresholdPixel(f, k4, t, x, y, (int)W, (int)H, T); });
}

// ---- the temporal accumulation of a light list's visibility (include/rts_scene.h; per-pixel rule in rts_closest_hit.h: accumulatePixel) ----
extern "C" int rtsh_camera_basis(const float eye[3], const float target[3], float fovy, uint32_t W, uint32_t H, float out[14]) {
    if (!eye || !target || !out || W == 0 || H == 0) return RTS_ERR_INVALID_ARG;
    const Camera c = makeCamera(eye, target, fovy, W, H);
    const V3 v[4] = { c.eye, c.fwd, c.right, c.up };
    for (int i = 0; i < 4; ++i) { out[i * 3] = v[i].x; out[i * 3 + 1] = v[i].y; out[i * 3 + 2] = v[i].z; }
    out[12] = c.tanHalf;
    out[13] = c.aspect;
    return RTS_OK;
}

namespace rts_harness {
// Shared by the host and device forms: every refusal that needs no context, and the condensed form the per-pixel rule reads.
int makeTemporalList(const rts_light_list* list, const rtsh_temporal_params* p, const void* positions, const void* normals,
                     const void* visibility, const void* prevPositions, const void* prevNormals, const void* prevVisibility,
                     const void* prevLengths, uint32_t W, uint32_t H, const void* visibilityOut, const void* lengthsOut, TemporalList* out) {
    if (!rts::lightListOk(list) || !p || !positions || !normals || !visibility || !visibilityOut || !lengthsOut) return RTS_ERR_INVALID_ARG;
    const int prevs = (prevPositions != nullptr) + (prevNormals != nullptr) + (prevVisibility != nullptr) + (prevLengths != nullptr);
    if (prevs != 0 && prevs != 4) return RTS_ERR_INVALID_ARG;
    if (W == 0 || H == 0 || W > 65536u || H > 65536u || p->max_length == 0 || p->max_length > 255u) return RTS_ERR_INVALID_ARG;
    const float* numbers[] = { p->eye_delta, p->prev_right, p->prev_up, p->prev_fwd };
    for (const float* v : numbers)
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(v[i])) return RTS_ERR_INVALID_ARG;
    if (!std::isfinite(p->normal_cos_min) || !std::isfinite(p->plane_eps) || !std::isfinite(p->prev_scale_x) ||
        !std::isfinite(p->prev_scale_y) || !(p->prev_scale_x > 0.0f) || !(p->prev_scale_y > 0.0f))
        return RTS_ERR_INVALID_ARG;
    if (prevs == 4 && (visibilityOut == prevVisibility || lengthsOut == prevLengths)) return RTS_ERR_INVALID_ARG;   // history must ping-pong
    out->count = list->count;
    out->maxLength = p->max_length;
    out->resetLights = p->reset_lights & 0xFFu;
    out->history = prevs == 4 ? 1u : 0u;
    out->eyeDelta = V3{ p->eye_delta[0], p->eye_delta[1], p->eye_delta[2] };
    out->right = V3{ p->prev_right[0], p->prev_right[1], p->prev_right[2] };
    out->up = V3{ p->prev_up[0], p->prev_up[1], p->prev_up[2] };
    out->fwd = V3{ p->prev_fwd[0], p->prev_fwd[1], p->prev_fwd[2] };
    out->scaleX = p->prev_scale_x;
    out->scaleY = p->prev_scale_y;
    out->normalCosMin = p->normal_cos_min;
    out->planeEps = p->plane_eps;
    return RTS_OK;
}

// The clamp's own refusals, beside makeTemporalList's: also shared by the host and device forms.
int checkHistoryClamp(const rtsh_history_clamp* clamp, const void* visibility, const void* visibilityOut) {
    if (!clamp || clamp->radius > (uint32_t)RTSH_CLAMP_MAX_RADIUS || !std::isfinite(clamp->margin) || !(clamp->margin >= 0.0f))
        return RTS_ERR_INVALID_ARG;
    if (visibilityOut == visibility) return RTS_ERR_INVALID_ARG;                      // the pass reads its neighbours' current values
    return RTS_OK;
}

namespace {
// Both frames as accumulatePixel reads them on the host: straight from the buffers.
struct TemporalFrames {
    const float *positions, *normals, *visibility, *prevPositions, *prevNormals, *history;
    const uint8_t *map, *prevLengths;
    float* visibilityOut;
    uint8_t* lengthsOut;
    size_t W, n;
    size_t at(int x, int y) const { return (size_t)y * W + (size_t)x; }
    static V3 xyz(const float* base, size_t i) { const float* v = base + i * 4; return V3{ v[0], v[1], v[2] }; }
    V3 normal(int x, int y) const { return xyz(normals, at(x, y)); }
    V3 position(int x, int y) const { return xyz(positions, at(x, y)); }
    uint32_t bits(int x, int y) const { return map ? map[at(x, y)] : 0xFFu; }
    uint32_t current(uint32_t l, int x, int y) const { uint32_t u; memcpy(&u, visibility + (size_t)l * n + at(x, y), 4); return u; }
    V3 prevNormal(int x, int y) const { return xyz(prevNormals, at(x, y)); }
    V3 prevPosition(int x, int y) const { return xyz(prevPositions, at(x, y)); }
    uint32_t prevLength(uint32_t l, int x, int y) const { return prevLengths[(size_t)l * n + at(x, y)]; }
    float prevVisibility(uint32_t l, int x, int y) const { return history[(size_t)l * n + at(x, y)]; }
    void store(uint32_t l, int x, int y, uint32_t bits, uint32_t length) const {
        memcpy(visibilityOut + (size_t)l * n + at(x, y), &bits, 4);
        lengthsOut[(size_t)l * n + at(x, y)] = (uint8_t)length;
    }
};

// ... and with the clamp's box: a straight loop over the window.
struct ClampedTemporalFrames : TemporalFrames {
    int W_, H_, radius;
    bool box(uint32_t l, int x, int y, uint32_t* loKey, uint32_t* hiKey) const {
        uint32_t lo = kClampNoKey, hi = 0u;
        bool any = false;
        for (int qy = y - radius; qy <= y + radius; ++qy)
            for (int qx = x - radius; qx <= x + radius; ++qx) {
                if (qx < 0 || qx >= W_ || qy < 0 || qy >= H_) continue;
                if (isBackground(normal(qx, qy)) || !((bits(qx, qy) >> l) & 1u)) continue;
                const uint32_t u = current(l, qx, qy);
                if (bitsAreNaN(u)) continue;
                const uint32_t k = clampKey(u);
                lo = k < lo ? k : lo;
                hi = k > hi ? k : hi;
                any = true;
            }
        *loKey = lo;
        *hiKey = hi;
        return any;
    }
};

// ... and with this frame's motion planes (the motion forms): Q and M_p of the pixel itself.
template <class Base>
struct MotionOf : Base {
    const float *prevPoints, *prevPointNormals;
    V3 prevPoint(int x, int y) const { return Base::xyz(prevPoints, Base::at(x, y)); }
    V3 prevPointNormal(int x, int y) const { return Base::xyz(prevPointNormals, Base::at(x, y)); }
};
} // namespace

// The motion forms' own refusal, beside their parents': with a history, both of this frame's motion planes.
int checkMotionPlanes(uint32_t history, const void* prevPoints, const void* prevPointNormals) {
    return (history != 0u && (!prevPoints || !prevPointNormals)) ? RTS_ERR_INVALID_ARG : RTS_OK;
}
} // namespace rts_harness

extern "C" int rtsh_accumulate_visibility_list(const rts_light_list* list, const rtsh_temporal_params* params, const float* positions,
                                               const float* normals, const uint8_t* lights_map, const float* visibility,
                                               const float* prev_positions, const float* prev_normals, const float* prev_visibility,
                                               const uint8_t* prev_lengths, uint32_t W, uint32_t H, float* visibility_out,
                                               uint8_t* lengths_out, int threads) {
    TemporalList f;
    const int s = makeTemporalList(list, params, positions, normals, visibility, prev_positions, prev_normals, prev_visibility, prev_lengths,
                                   W, H, visibility_out, lengths_out, &f);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    const TemporalFrames t{ positions, normals, visibility, prev_positions, prev_normals, prev_visibility, lights_map, prev_lengths,
                            visibility_out, lengths_out, W, n };
    parallelFor(n, 256, threads, [&](size_t i) { accumulatePixel(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H); });
    return RTS_OK;
}

extern "C" int rtsh_accumulate_visibility_list_clamped(const rts_light_list* list, const rtsh_temporal_params* params, const float* positions,
                                                       const float* normals, const uint8_t* lights_map, const float* visibility,
                                                       const float* prev_positions, const float* prev_normals,
                                                       const float* prev_visibility, const uint8_t* prev_lengths, uint32_t W, uint32_t H,
                                                       float* visibility_out, uint8_t* lengths_out, const rtsh_history_clamp* clamp,
                                                       int threads) {
    TemporalList f;
    int s = makeTemporalList(list, params, positions, normals, visibility, prev_positions, prev_normals, prev_visibility, prev_lengths, W, H,
                             visibility_out, lengths_out, &f);
    if (s == RTS_OK) s = checkHistoryClamp(clamp, visibility, visibility_out);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    const float margin = clamp->margin;
    const ClampedTemporalFrames t{ { positions, normals, visibility, prev_positions, prev_normals, prev_visibility, lights_map, prev_lengths,
                                     visibility_out, lengths_out, W, n }, (int)W, (int)H, (int)clamp->radius };
    parallelFor(n, 256, threads, [&](size_t i) { accumulatePixel<true>(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H, margin); });
    return RTS_OK;
}

// ---- the motion forms of the two passes above (include/rts_scene.h): accumulatePixel<Clamped, true> ----
extern "C" int rtsh_accumulate_visibility_list_motion(const rts_light_list* list, const rtsh_temporal_params* params, const float* positions,
                                                      const float* normals, const uint8_t* lights_map, const float* visibility,
                                                      const float* prev_positions, const float* prev_normals, const float* prev_visibility,
                                                      const uint8_t* prev_lengths, const float* prev_points,
                                                      const float* prev_point_normals, uint32_t W, uint32_t H, float* visibility_out,
                                                      uint8_t* lengths_out, int threads) {
    TemporalList f;
    int s = makeTemporalList(list, params, positions, normals, visibility, prev_positions, prev_normals, prev_visibility, prev_lengths, W, H,
                             visibility_out, lengths_out, &f);
    if (s == RTS_OK) s = checkMotionPlanes(f.history, prev_points, prev_point_normals);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    const MotionOf<TemporalFrames> t{ { positions, normals, visibility, prev_positions, prev_normals, prev_visibility, lights_map, prev_lengths,
                                        visibility_out, lengths_out, W, n }, prev_points, prev_point_normals };
    parallelFor(n, 256, threads, [&](size_t i) { accumulatePixel<false, true>(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H); });
    return RTS_OK;
}

extern "C" int rtsh_accumulate_visibility_list_clamped_motion(const rts_light_list* list, const rtsh_temporal_params* params,
                                                              const float* positions, const float* normals, const uint8_t* lights_map,
                                                              const float* visibility, const float* prev_positions,
                                                              const float* prev_normals, const float* prev_visibility,
                                                              const uint8_t* prev_lengths, const float* prev_points,
                                                              const float* prev_point_normals, uint32_t W, uint32_t H,
                                                              float* visibility_out, uint8_t* lengths_out, const rtsh_history_clamp* clamp,
                                                              int threads) {
    TemporalList f;
    int s = makeTemporalList(list, params, positions, normals, visibility, prev_positions, prev_normals, prev_visibility, prev_lengths, W, H,
                             visibility_out, lengths_out, &f);
    if (s == RTS_OK) s = checkHistoryClamp(clamp, visibility, visibility_out);
    if (s == RTS_OK) s = checkMotionPlanes(f.history, prev_points, prev_point_normals);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    const float margin = clamp->margin;
    const MotionOf<ClampedTemporalFrames> t{ { { positions, normals, visibility, prev_positions, prev_normals, prev_visibility, lights_map,
                                                 prev_lengths, visibility_out, lengths_out, W, n }, (int)W, (int)H, (int)clamp->radius },
                                             prev_points, prev_point_normals };
    parallelFor(n, 256, threads, [&](size_t i) { accumulatePixel<true, true>(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H, margin); });
    return RTS_OK;
}

// ---- the temporal accumulation of a soft light list's count moments (include/rts_scene.h; per-pixel rule in rts_closest_hit.h:
// accumulateMomentsPixel) ----
namespace rts_harness {
// Shared by the host and device forms: every refusal that needs no context -- makeTemporalList's own over a stand-in list of the same
// count (counts in the place of visibility, the mean planes in the place of the float history), then the square planes' -- and the
// condensed form the per-pixel rule reads.
int makeMomentsList(const rts_soft_light_list* list, const rtsh_temporal_params* p, const void* positions, const void* normals,
                    const void* counts, const void* prevPositions, const void* prevNormals, const void* prevMean, const void* prevSquare,
                    const void* prevLengths, uint32_t W, uint32_t H, const void* meanOut, const void* squareOut, const void* lengthsOut,
                    MomentsList* out) {
    if (!rts::softListOk(list) || !squareOut) return RTS_ERR_INVALID_ARG;
    rts_light_list hard;
    std::memset(&hard, 0, sizeof(hard));
    hard.count = list->count;
    for (uint32_t l = 0; l < list->count; ++l) hard.lights[l].type = list->lights[l].type;
    if ((prevSquare != nullptr) != (prevMean != nullptr)) return RTS_ERR_INVALID_ARG;               // all five prev_* or none
    const int s = makeTemporalList(&hard, p, positions, normals, counts, prevPositions, prevNormals, prevMean, prevLengths, W, H, meanOut,
                                   lengthsOut, &out->t);
    if (s != RTS_OK) return s;
    if (prevSquare && squareOut == prevSquare) return RTS_ERR_INVALID_ARG;                          // history must ping-pong
    for (uint32_t l = 0; l < 8; ++l) {
        out->samples[l] = l < list->count && list->lights[l].nsamples > 1u ? list->lights[l].nsamples : 1u;
        out->scale[l] = wideFilterScale(out->samples[l]);
    }
    return RTS_OK;
}

namespace {
// Both frames as accumulateMomentsPixel reads them on the host: straight from the buffers.
struct MomentsFrames {
    const float *positions, *normals, *prevPositions, *prevNormals;
    const uint8_t *map, *counts, *prevLengths;
    const uint16_t* prevMeans;
    const uint32_t* prevSquares;
    uint16_t* meanOut;
    uint32_t* squareOut;
    uint8_t* lengthsOut;
    size_t W, n;
    size_t at(int x, int y) const { return (size_t)y * W + (size_t)x; }
    static V3 xyz(const float* base, size_t i) { const float* v = base + i * 4; return V3{ v[0], v[1], v[2] }; }
    V3 normal(int x, int y) const { return xyz(normals, at(x, y)); }
    V3 position(int x, int y) const { return xyz(positions, at(x, y)); }
    uint32_t bits(int x, int y) const { return map ? map[at(x, y)] : 0xFFu; }
    uint32_t count(uint32_t l, int x, int y) const { return counts[(size_t)l * n + at(x, y)]; }
    V3 prevNormal(int x, int y) const { return xyz(prevNormals, at(x, y)); }
    V3 prevPosition(int x, int y) const { return xyz(prevPositions, at(x, y)); }
    uint32_t prevLength(uint32_t l, int x, int y) const { return prevLengths[(size_t)l * n + at(x, y)]; }
    uint32_t prevMean(uint32_t l, int x, int y) const { return prevMeans[(size_t)l * n + at(x, y)]; }
    uint32_t prevSquare(uint32_t l, int x, int y) const { return prevSquares[(size_t)l * n + at(x, y)]; }
    void store(uint32_t l, int x, int y, uint32_t mean, uint32_t square, uint32_t length) const {
        meanOut[(size_t)l * n + at(x, y)] = (uint16_t)mean;
        squareOut[(size_t)l * n + at(x, y)] = square;
        lengthsOut[(size_t)l * n + at(x, y)] = (uint8_t)length;
    }
};
} // namespace
} // namespace rts_harness

extern "C" int rtsh_accumulate_moments_soft_light_list(const rts_soft_light_list* list, const rtsh_temporal_params* params,
                                                       const float* positions, const float* normals, const uint8_t* lights_map,
                                                       const uint8_t* counts, const float* prev_positions, const float* prev_normals,
                                                       const uint16_t* prev_mean, const uint32_t* prev_square, const uint8_t* prev_lengths,
                                                       uint32_t W, uint32_t H, uint16_t* mean_out, uint32_t* square_out,
                                                       uint8_t* lengths_out, int threads) {
    MomentsList f;
    const int s = makeMomentsList(list, params, positions, normals, counts, prev_positions, prev_normals, prev_mean, prev_square,
                                  prev_lengths, W, H, mean_out, square_out, lengths_out, &f);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    const MomentsFrames t{ positions, normals, prev_positions, prev_normals, lights_map, counts, prev_lengths, prev_mean, prev_square,
                           mean_out, square_out, lengths_out, W, n };
    parallelFor(n, 256, threads, [&](size_t i) { accumulateMomentsPixel(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H); });
    return RTS_OK;
}

namespace rts_harness {
namespace {
struct MotionMomentsFrames : MomentsFrames {
    const float *prevPoints, *prevPointNormals;
    V3 prevPoint(int x, int y) const { return xyz(prevPoints, at(x, y)); }
    V3 prevPointNormal(int x, int y) const { return xyz(prevPointNormals, at(x, y)); }
};
} // namespace
} // namespace rts_harness

// ---- the motion form of the moments pass (include/rts_scene.h): accumulateMomentsPixel<true> ----
extern "C" int rtsh_accumulate_moments_soft_light_list_motion(const rts_soft_light_list* list, const rtsh_temporal_params* params,
                                                              const float* positions, const float* normals, const uint8_t* lights_map,
                                                              const uint8_t* counts, const float* prev_positions, const float* prev_normals,
                                                              const uint16_t* prev_mean, const uint32_t* prev_square,
                                                              const uint8_t* prev_lengths, const float* prev_points,
                                                              const float* prev_point_normals, uint32_t W, uint32_t H, uint16_t* mean_out,
                                                              uint32_t* square_out, uint8_t* lengths_out, int threads) {
    MomentsList f;
    int s = makeMomentsList(list, params, positions, normals, counts, prev_positions, prev_normals, prev_mean, prev_square, prev_lengths, W, H,
                            mean_out, square_out, lengths_out, &f);
    if (s == RTS_OK) s = checkMotionPlanes(f.t.history, prev_points, prev_point_normals);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    const MotionMomentsFrames t{ { positions, normals, prev_positions, prev_normals, lights_map, counts, prev_lengths, prev_mean, prev_square,
                                   mean_out, square_out, lengths_out, W, n }, prev_points, prev_point_normals };
    parallelFor(n, 256, threads, [&](size_t i) { accumulateMomentsPixel<true>(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H); });
    return RTS_OK;
}

// ---- the temporal accumulation of the bent texel and the wide bent filter fed from it (include/rts_scene.h; per-pixel
// rules in rts_closest_hit.h: accumulateBentPixel, bentFilterMeanInput) ----
namespace rts_harness {
// Shared by the host and device forms: makeTemporalList's refusals over a one-entry stand-in list (bent in the place of visibility, the
// texel planes in the place of the float history), the sample count's, and n, S_b, S_l.
int makeBentTemporalList(const rtsh_temporal_params* p, uint32_t nsamples, const void* positions, const void* normals, const void* bent,
                         const void* prevPositions, const void* prevNormals, const void* prevTexels, const void* prevLengths, uint32_t W,
                         uint32_t H, const void* texelsOut, const void* lengthsOut, BentTemporalList* out) {
    if (!out || nsamples > (uint32_t)RTS_AO_MAX_SAMPLES) return RTS_ERR_INVALID_ARG;
    rts_light_list one;
    std::memset(&one, 0, sizeof(one));
    one.count = 1;
    const int s = makeTemporalList(&one, p, positions, normals, bent, prevPositions, prevNormals, prevTexels, prevLengths, W, H, texelsOut,
                                   lengthsOut, &out->t);
    if (s != RTS_OK) return s;
    const uint32_t n = nsamples > 1u ? nsamples : 1u;
    out->q = BentFilterList{ 0u, n, bentFilterScale(n), wideFilterScale(n), 0.0f, 0.0f };
    return RTS_OK;
}

namespace {
// Both frames as accumulateBentPixel reads them on the host: straight from the buffers.
struct BentTemporalFrames {
    const float *positions, *normals, *bent, *prevPositions, *prevNormals;
    const uint8_t *map, *prevLengths;
    const uint64_t* prevTexels;
    uint64_t* texelsOut;
    uint8_t* lengthsOut;
    const BentFilterList& f;
    size_t W;
    size_t at(int x, int y) const { return (size_t)y * W + (size_t)x; }
    static V3 xyz(const float* base, size_t i) { const float* v = base + i * 4; return V3{ v[0], v[1], v[2] }; }
    V3 normal(int x, int y) const { return xyz(normals, at(x, y)); }
    V3 position(int x, int y) const { return xyz(positions, at(x, y)); }
    bool active(int x, int y) const { return !map || map[at(x, y)] != 0; }
    BentTexel current(int x, int y) const { const float* b = bent + at(x, y) * 4; return bentFilterInput(b[0], b[1], b[2], b[3], f); }
    V3 prevNormal(int x, int y) const { return xyz(prevNormals, at(x, y)); }
    V3 prevPosition(int x, int y) const { return xyz(prevPositions, at(x, y)); }
    uint32_t prevLength(int x, int y) const { return prevLengths[at(x, y)]; }
    BentTexel prevTexel(int x, int y) const { return bentFilterUnpack(prevTexels[at(x, y)]); }
    void store(int x, int y, uint64_t texel, uint32_t length) const { texelsOut[at(x, y)] = texel; lengthsOut[at(x, y)] = (uint8_t)length; }
};

int accumulateBentHost(bool motion, const rtsh_temporal_params* params, uint32_t nsamples, const float* positions, const float* normals,
                       const uint8_t* active, const float* bent, const float* prev_positions, const float* prev_normals,
                       const void* prev_texels, const uint8_t* prev_lengths, const float* prev_points, const float* prev_point_normals,
                       uint32_t W, uint32_t H, void* texels_out, uint8_t* lengths_out, int threads) {
    BentTemporalList f;
    int s = makeBentTemporalList(params, nsamples, positions, normals, bent, prev_positions, prev_normals, prev_texels, prev_lengths, W, H,
                                 texels_out, lengths_out, &f);
    if (s == RTS_OK && motion) s = checkMotionPlanes(f.t.history, prev_points, prev_point_normals);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    const MotionOf<BentTemporalFrames> t{ { positions, normals, bent, prev_positions, prev_normals, active, prev_lengths,
                                            (const uint64_t*)prev_texels, (uint64_t*)texels_out, lengths_out, f.q, W },
                                          prev_points, prev_point_normals };
    if (motion) parallelFor(n, 256, threads, [&](size_t i) { accumulateBentPixel<true>(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H); });
    else parallelFor(n, 256, threads, [&](size_t i) { accumulateBentPixel(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H); });
    return RTS_OK;
}
} // namespace
} // namespace rts_harness

extern "C" int rtsh_accumulate_bent(const rtsh_temporal_params* params, uint32_t nsamples, const float* positions, const float* normals,
                                    const uint8_t* active, const float* bent, const float* prev_positions, const float* prev_normals,
                                    const void* prev_texels, const uint8_t* prev_lengths, uint32_t W, uint32_t H, void* texels_out,
                                    uint8_t* lengths_out, int threads) {
    return accumulateBentHost(false, params, nsamples, positions, normals, active, bent, prev_positions, prev_normals, prev_texels,
                              prev_lengths, nullptr, nullptr, W, H, texels_out, lengths_out, threads);
}

extern "C" int rtsh_accumulate_bent_motion(const rtsh_temporal_params* params, uint32_t nsamples, const float* positions,
                                           const float* normals, const uint8_t* active, const float* bent, const float* prev_positions,
                                           const float* prev_normals, const void* prev_texels, const uint8_t* prev_lengths,
                                           const float* prev_points, const float* prev_point_normals, uint32_t W, uint32_t H,
                                           void* texels_out, uint8_t* lengths_out, int threads) {
    return accumulateBentHost(true, params, nsamples, positions, normals, active, bent, prev_positions, prev_normals, prev_texels,
                              prev_lengths, prev_points, prev_point_normals, W, H, texels_out, lengths_out, threads);
}

// The passes of rtsh_wide_filter_bent over the accumulated texel: its loop, statement for statement, with a frame of its own whose
// first pass reads and clamps the 8-byte texels (the parent's host form keeps its text, as its kernels do).
namespace rts_harness {
namespace {
struct BentMeanFrameTexels {
    const float *positions, *normals;
    const uint64_t* mean;                        // the accumulated texels: the first pass's input
    const uint8_t* map;
    const uint64_t* values;                      // the previous pass's plane; NULL: the first pass
    const BentFilterList& f;
    size_t W;
    size_t at(int x, int y) const { return (size_t)y * W + (size_t)x; }
    V3 normal(int x, int y) const { const float* v = normals + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    V3 position(int x, int y) const { const float* v = positions + at(x, y) * 4; return V3{ v[0], v[1], v[2] }; }
    bool active(int x, int y) const { return !map || map[at(x, y)] != 0; }
    BentTexel texel(int x, int y) const { return values ? bentFilterUnpack(values[at(x, y)]) : bentFilterMeanInput(mean[at(x, y)], f); }
};
} // namespace
} // namespace rts_harness

extern "C" int rtsh_wide_filter_bent_mean(const rtsh_wide_filter_params* params, uint32_t nsamples, const float* positions,
                                          const float* normals, const uint8_t* active, const void* texels, uint32_t W, uint32_t H, float* out,
                                          float* ao, int threads) {
    if (!positions || !normals || !texels || !out) return RTS_ERR_INVALID_ARG;
    BentFilterList f;
    const int s = makeBentFilterList(params, nsamples, W, H, &f);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    std::vector<uint64_t> scratch;
    try {
        if (f.passes >= 2u) scratch.resize(2 * n);
    } catch (const std::bad_alloc&) {
        return RTS_ERR_CAPACITY;
    }
    const uint32_t launches = f.passes == 0u ? 1u : f.passes;
    for (uint32_t k = 0; k < launches; ++k) {
        const bool first = k == 0u, last = k + 1u == launches;
        const int step = f.passes == 0u ? 0 : 1 << k;
        const uint64_t* in = first ? nullptr : scratch.data() + ((k - 1u) & 1u) * n;
        uint64_t* mid = last ? nullptr : scratch.data() + (k & 1u) * n;
        const BentMeanFrameTexels t{ positions, normals, (const uint64_t*)texels, active, in, f, W };
        parallelFor(n, 256, threads, [&](size_t i) {
            BentTexel v;
            bentFilterPassPixel(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H, step, &v);
            if (!last) { mid[i] = bentFilterPack(v); return; }
            float* o = out + i * 4;
            o[0] = bentFilterOutput(v.x, f.samples, f.scaleB);
            o[1] = bentFilterOutput(v.y, f.samples, f.scaleB);
            o[2] = bentFilterOutput(v.z, f.samples, f.scaleB);
            o[3] = wideFilterOutput(v.v, f.samples, f.scaleL);
            if (ao) ao[i] = o[3];
        });
    }
    return RTS_OK;
}

// ---- the clamped forms of the moments pass (include/rts_scene.h): accumulateMomentsPixel<Motion, true> ----
namespace rts_harness {
// The clamp's own refusals, beside makeMomentsList's: shared by the host and device forms.
int checkMomentsClamp(const rtsh_moments_clamp* clamp) {
    return (!clamp || clamp->radius > (uint32_t)RTSH_MOMENTS_CLAMP_MAX_RADIUS || clamp->sigma_k4 > 255u || clamp->margin > 65535u)
               ? RTS_ERR_INVALID_ARG : RTS_OK;
}

namespace {
// The frames with the clamp's box: a straight loop over the window, then the bounds from its five integers.
template <class Base>
struct ClampedMomentsOf : Base {
    const uint32_t *samples, *scale;
    int W_, H_, radius;
    uint32_t k4, margin;
    void box(uint32_t l, int x, int y, uint32_t* Lv, uint32_t* Hv) const {
        uint32_t m = 0, lo = 65535u, hi = 0u;
        uint64_t S1 = 0, S2 = 0;
        for (int qy = y - radius; qy <= y + radius; ++qy)
            for (int qx = x - radius; qx <= x + radius; ++qx) {
                if (qx < 0 || qx >= W_ || qy < 0 || qy >= H_) continue;
                if (isBackground(Base::normal(qx, qy)) || !((Base::bits(qx, qy) >> l) & 1u)) continue;
                const uint32_t v = wideFilterInput(Base::count(l, qx, qy), samples[l], scale[l]);
                ++m;
                S1 += v;
                S2 += (uint64_t)(v * v);
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
        momentsClampBounds(m, S1, S2, lo, hi, k4, margin, Lv, Hv);                    // (m >= 1: asked at blended pairs only)
    }
};
} // namespace
} // namespace rts_harness

extern "C" void rtsh_moments_clamp_bounds(uint32_t m, uint64_t S1, uint64_t S2, uint32_t lo, uint32_t hi, uint32_t sigma_k4, uint32_t margin,
                                          uint32_t* Lv, uint32_t* Hv) {
    if (!Lv || !Hv) return;
    *Lv = 0u;
    *Hv = 65535u;
    // outside the widths of the rule (no window gives such parts): no box.  Inside them x < 2^62 and every step stays in 64 bits.
    if (m == 0u || m > 81u || sigma_k4 > 255u || hi > 65535u || lo > hi || S1 >= (1ull << 23) || S2 >= (1ull << 39)) return;
    if ((uint64_t)m * S2 < S1 * S1) return;
    momentsClampBounds(m, S1, S2, lo, hi, sigma_k4, margin, Lv, Hv);
}

extern "C" int rtsh_accumulate_moments_soft_light_list_clamped(const rts_soft_light_list* list, const rtsh_temporal_params* params,
                                                               const float* positions, const float* normals, const uint8_t* lights_map,
                                                               const uint8_t* counts, const float* prev_positions, const float* prev_normals,
                                                               const uint16_t* prev_mean, const uint32_t* prev_square,
                                                               const uint8_t* prev_lengths, uint32_t W, uint32_t H, uint16_t* mean_out,
                                                               uint32_t* square_out, uint8_t* lengths_out, const rtsh_moments_clamp* clamp,
                                                               int threads) {
    MomentsList f;
    int s = makeMomentsList(list, params, positions, normals, counts, prev_positions, prev_normals, prev_mean, prev_square, prev_lengths, W, H,
                            mean_out, square_out, lengths_out, &f);
    if (s == RTS_OK) s = checkMomentsClamp(clamp);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    const ClampedMomentsOf<MomentsFrames> t{ { positions, normals, prev_positions, prev_normals, lights_map, counts, prev_lengths, prev_mean,
                                               prev_square, mean_out, square_out, lengths_out, W, n },
                                             f.samples, f.scale, (int)W, (int)H, (int)clamp->radius, clamp->sigma_k4, clamp->margin };
    parallelFor(n, 256, threads, [&](size_t i) { accumulateMomentsPixel<false, true>(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H); });
    return RTS_OK;
}

extern "C" int rtsh_accumulate_moments_soft_light_list_clamped_motion(const rts_soft_light_list* list, const rtsh_temporal_params* params,
                                                                      const float* positions, const float* normals,
                                                                      const uint8_t* lights_map, const uint8_t* counts,
                                                                      const float* prev_positions, const float* prev_normals,
                                                                      const uint16_t* prev_mean, const uint32_t* prev_square,
                                                                      const uint8_t* prev_lengths, const float* prev_points,
                                                                      const float* prev_point_normals, uint32_t W, uint32_t H,
                                                                      uint16_t* mean_out, uint32_t* square_out, uint8_t* lengths_out,
                                                                      const rtsh_moments_clamp* clamp, int threads) {
    MomentsList f;
    int s = makeMomentsList(list, params, positions, normals, counts, prev_positions, prev_normals, prev_mean, prev_square, prev_lengths, W, H,
                            mean_out, square_out, lengths_out, &f);
    if (s == RTS_OK) s = checkMomentsClamp(clamp);
    if (s == RTS_OK) s = checkMotionPlanes(f.t.history, prev_points, prev_point_normals);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    const ClampedMomentsOf<MotionMomentsFrames> t{ { { positions, normals, prev_positions, prev_normals, lights_map, counts, prev_lengths,
                                                       prev_mean, prev_square, mean_out, square_out, lengths_out, W, n },
                                                     prev_points, prev_point_normals },
                                                   f.samples, f.scale, (int)W, (int)H, (int)clamp->radius, clamp->sigma_k4, clamp->margin };
    parallelFor(n, 256, threads, [&](size_t i) { accumulateMomentsPixel<true, true>(f, t, (int)(i % W), (int)(i / W), (int)W, (int)H); });
    return RTS_OK;
}

// ---- the guided wide filter with a temporal threshold (include/rts_scene.h; per-pixel rule in rts_closest_hit.h:
// wideGuideTemporalThresholdPixel, wideGuidedPassPixel) ----
namespace rts_harness {
// Shared by the host and device forms: the refusals, and the unguided filter's condensed list.
int makeWideGuidedTemporalList(const rts_soft_light_list* list, const rtsh_wide_guide_temporal_params* p, uint32_t W, uint32_t H,
                               WideFilterList* out) {
    if (!p || p->min_history == 0u || p->min_history > 255u) return RTS_ERR_INVALID_ARG;
    rtsh_wide_guide_params q;
    std::memset(&q, 0, sizeof(q));
    q.passes = p->passes; q.normal_cos_min = p->normal_cos_min; q.plane_eps = p->plane_eps; q.guide_k4 = p->guide_k4;
    return makeWideGuidedList(list, &q, W, H, out);
}
} // namespace rts_harness

extern "C" int rtsh_wide_filter_guided_temporal_soft_light_list(const rts_soft_light_list* list, const rtsh_wide_guide_temporal_params* params,
                                                                const float* positions, const float* normals, const uint8_t* lights_map,
                                                                const uint8_t* counts, const uint16_t* mean, const uint32_t* square,
                                                                const uint8_t* lengths, uint32_t W, uint32_t H, float* visibility,
                                                                int threads) {
    if (!positions || !normals || !counts || !mean || !square || !lengths || !visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int s = makeWideGuidedTemporalList(list, params, W, H, &f);
    if (s != RTS_OK) return s;
    const uint32_t k4 = params->guide_k4, minHistory = params->min_history;
    const GuideMoments h{ mean, square, lengths, W, (size_t)W * H };
    return widePassChain(f, positions, normals, lights_map, WideSoftInput{ counts }, W, H, visibility, threads,
                         [&](const auto& t, int x, int y, uint32_t* T) {
                             wideGuideTemporalThresholdPixel(f, k4, minHistory, t, h, x, y, (int)W, (int)H, T);
                         });
}

// ---- the wide filters fed from the accumulated mean (include/rts_scene.h; per-pixel rule in rts_closest_hit.h: wideMeanInput,
// wideFilterPassPixel, wideGuideTemporalMeanThresholdPixel, wideGuidedPassPixel) ----
extern "C" int rtsh_wide_filter_mean_soft_light_list(const rts_soft_light_list* list, const rtsh_wide_filter_params* params,
                                                     const float* positions, const float* normals, const uint8_t* lights_map,
                                                     const uint16_t* mean, uint32_t W, uint32_t H, float* visibility, int threads) {
    if (!positions || !normals || !mean || !visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int s = makeWideFilterSoftList(list, params, W, H, &f);
    if (s != RTS_OK) return s;
    return widePassChain(f, positions, normals, lights_map, WideMeanInput{ mean }, W, H, visibility, threads, nullptr);
}

extern "C" int rtsh_wide_filter_guided_temporal_mean_soft_light_list(const rts_soft_light_list* list,
                                                                     const rtsh_wide_guide_temporal_params* params, const float* positions,
                                                                     const float* normals, const uint8_t* lights_map, const uint8_t* counts,
                                                                     const uint16_t* mean, const uint32_t* square, const uint8_t* lengths,
                                                                     uint32_t W, uint32_t H, float* visibility, int threads) {
    if (!positions || !normals || !counts || !mean || !square || !lengths || !visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int s = makeWideGuidedTemporalList(list, params, W, H, &f);
    if (s != RTS_OK) return s;
    const uint32_t k4 = params->guide_k4, minHistory = params->min_history;
    const GuideMomentsCounts h{ GuideMoments{ mean, square, lengths, W, (size_t)W * H }, counts };
    return widePassChain(f, positions, normals, lights_map, WideMeanInput{ mean }, W, H, visibility, threads,
                         [&](const auto& t, int x, int y, uint32_t* T) {
                             wideGuideTemporalMeanThresholdPixel(f, k4, minHistory, t, h, x, y, (int)W, (int)H, T);
                         });
}

// ---- the guided mean filter with a propagated variance (include/rts_scene.h; per-pixel rule in rts_closest_hit.h:
// wideVarianceInput, widePropagatedFirstThresholdPixel, widePropagatedThresholdPixel, widePropagatedPassPixel) ----
namespace rts_harness {
// Shared by the host and device forms: the refusals, and the unguided filter's condensed list.
int makeWidePropagatedList(const rts_soft_light_list* list, const rtsh_wide_guide_propagated_params* p, uint32_t W, uint32_t H,
                           WideFilterList* out) {
    if (!p || p->by_length > 1u) return RTS_ERR_INVALID_ARG;
    rtsh_wide_guide_temporal_params q;
    std::memset(&q, 0, sizeof(q));
    q.passes = p->passes; q.normal_cos_min = p->normal_cos_min; q.plane_eps = p->plane_eps; q.guide_k4 = p->guide_k4;
    q.min_history = p->min_history;
    return makeWideGuidedTemporalList(list, &q, W, H, out);
}

namespace {
// A SIBLING of widePassChain, which keeps its text and with it the five shipped twins: this chain carries two kinds of planes (uint16_t
// values and uint32_t variance, each ping-pong), has no plane of T, and its later passes form T_k themselves from the variance plane they
// read -- three differences that would each be a branch in the shared chain.
int widePropagatedChain(const WideFilterList& f, const WidePropagatedRule& r, const GuideMomentsCounts& h, const float* positions,
                        const float* normals, const uint8_t* lights_map, uint32_t W, uint32_t H, float* visibility, int threads) {
    const size_t n = (size_t)W * H, set = (size_t)f.count * n;
    std::vector<uint16_t> values;
    std::vector<uint32_t> variance;
    try {
        if (f.passes >= 2u) { values.resize(2 * set); variance.resize(2 * set); }
    } catch (const std::bad_alloc&) {
        return RTS_ERR_CAPACITY;
    }
    const uint32_t launches = f.passes == 0u ? 1u : f.passes;
    for (uint32_t k = 0; k < launches; ++k) {
        const bool first = k == 0u, last = k + 1u == launches;
        const int step = f.passes == 0u ? 0 : 1 << k;
        const uint16_t* in = first ? nullptr : values.data() + ((k - 1u) & 1u) * set;
        const uint32_t* qin = first ? nullptr : variance.data() + ((k - 1u) & 1u) * set;
        uint16_t* out = last ? nullptr : values.data() + (k & 1u) * set;
        uint32_t* qout = last ? nullptr : variance.data() + (k & 1u) * set;
        const WideFrameTexels<WideMeanInput> t{ positions, normals, lights_map, WideMeanInput{ h.m.mean }, in, f.samples, f.scale, W, n };
        const WideVarianceGlobal q{ f, r, h, qin };
        parallelFor(n, 256, threads, [&](size_t i) {
            const int x = (int)(i % W), y = (int)(i / W);
            uint32_t v[8], Q[8], T[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
            if (first) {
                if (step > 0) widePropagatedFirstThresholdPixel(f, r, t, h, x, y, (int)W, (int)H, T);
            } else {
                widePropagatedThresholdPixel(f, r.k4, t, q, x, y, (int)W, (int)H, T);
            }
            if (last) widePropagatedPassPixel<false>(f, t, q, x, y, (int)W, (int)H, step, T, v, Q);
            else widePropagatedPassPixel<true>(f, t, q, x, y, (int)W, (int)H, step, T, v, Q);
            for (uint32_t l = 0; l < f.count; ++l) {
                if (last) visibility[(size_t)l * n + i] = wideFilterOutput(v[l], f.samples[l], f.scale[l]);
                else { out[(size_t)l * n + i] = (uint16_t)v[l]; qout[(size_t)l * n + i] = Q[l]; }
            }
        });
    }
    return RTS_OK;
}
} // namespace
} // namespace rts_harness

extern "C" size_t rtsh_wide_filter_propagated_scratch_bytes(uint32_t count, uint32_t W, uint32_t H) {
    return wideScratchBytes(2, count, W, H) * 3;                                 // 2 * 2 bytes of values, then 2 * 4 bytes of variance
}

extern "C" uint32_t rtsh_wide_variance_step(uint64_t numQ, uint32_t den) {
    if (den == 0 || den > 256u || numQ > (uint64_t)(den * den) * 0xFFFFFFFFull) return 0xFFFFFFFFu;
    return wideVarianceStep(numQ, den);
}

extern "C" int rtsh_wide_filter_propagated_mean_soft_light_list(const rts_soft_light_list* list,
                                                                const rtsh_wide_guide_propagated_params* params, const float* positions,
                                                                const float* normals, const uint8_t* lights_map, const uint8_t* counts,
                                                                const uint16_t* mean, const uint32_t* square, const uint8_t* lengths,
                                                                uint32_t W, uint32_t H, float* visibility, int threads) {
    if (!positions || !normals || !counts || !mean || !square || !lengths || !visibility) return RTS_ERR_INVALID_ARG;
    WideFilterList f;
    const int s = makeWidePropagatedList(list, params, W, H, &f);
    if (s != RTS_OK) return s;
    const WidePropagatedRule r{ params->guide_k4, params->min_history, params->by_length };
    const GuideMomentsCounts h{ GuideMoments{ mean, square, lengths, W, (size_t)W * H }, counts };
    return widePropagatedChain(f, r, h, positions, normals, lights_map, W, H, visibility, threads);
}

// ---- half-resolution light lists: subsample, retrace map, upsample (include/rts_scene.h; per-pixel rules in rts_closest_hit.h:
// upsampleTaps, upsampleRetracePixel, upsamplePixel) ----
namespace rts_harness {
// Shared by the host and device forms: the refusals of the parameters and the frame, and the condensed form the per-pixel rules read.
int makeUpsampleList(uint32_t count, const rtsh_upsample_params* p, uint32_t W, uint32_t H, UpsampleList* out) {
    if (!p || !out || count == 0 || count > (uint32_t)RTS_MAX_LIST_LIGHTS || p->phase_x > 1u || p->phase_y > 1u ||
        !std::isfinite(p->normal_cos_min) || !std::isfinite(p->plane_eps) || W == 0 || H == 0 || W > 0x7FFFFFF0u || H > 0x7FFFFFF0u)
        return RTS_ERR_INVALID_ARG;
    const uint32_t w = (W + 1u - p->phase_x) >> 1, h = (H + 1u - p->phase_y) >> 1;
    if (w == 0 || h == 0) return RTS_ERR_INVALID_ARG;
    *out = UpsampleList{ count, p->phase_x, p->phase_y, p->normal_cos_min, p->plane_eps, (int)w, (int)h };
    return RTS_OK;
}

namespace {
template <bool HARD>
int upsampleListFrame(uint32_t count, const rtsh_upsample_params* params, const float* positions, const float* normals,
                      const uint8_t* lights_map, const float* lo_positions, const float* lo_normals, const uint8_t* lo_lights_map,
                      const uint8_t* lo_planes, const uint8_t* keep, uint32_t W, uint32_t H, uint8_t* planes, int threads) {
    if (!positions || !normals || !lo_positions || !lo_normals || !lo_planes || !planes || planes == lo_planes) return RTS_ERR_INVALID_ARG;
    UpsampleList f;
    const int s = makeUpsampleList(count, params, W, H, &f);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    const FrameTexels<false> full{ positions, normals, nullptr, lights_map, nullptr, W, n };
    const FrameTexels<HARD> lo{ lo_positions, lo_normals, nullptr, lo_lights_map, lo_planes, (size_t)f.w, (size_t)f.w * (size_t)f.h };
    const uint32_t all = (1u << count) - 1u;
    parallelFor(n, 256, threads, [&](size_t i) {
        const uint32_t kept = keep ? keep[i] & all : 0u, todo = all & ~kept;
        if (todo == 0u) return;
        uint32_t b[8];
        upsamplePixel(f, full, lo, (int)(i % W), (int)(i / W), todo, b);
        if (HARD) {
            uint32_t bits = kept ? planes[i] & kept : 0u;
            for (uint32_t l = 0; l < count; ++l)
                if ((todo >> l) & 1u) bits |= (b[l] & 1u) << l;
            planes[i] = (uint8_t)bits;
        } else {
            for (uint32_t l = 0; l < count; ++l)
                if ((todo >> l) & 1u) planes[(size_t)l * n + i] = (uint8_t)b[l];
        }
    });
    return RTS_OK;
}
} // namespace
} // namespace rts_harness

extern "C" int rtsh_subsampled_size(uint32_t W, uint32_t H, uint32_t phase_x, uint32_t phase_y, uint32_t* w, uint32_t* h) {
    const rtsh_upsample_params p{ phase_x, phase_y, 0.0f, 0.0f, { 0, 0, 0, 0 } };
    UpsampleList f;
    if (!w || !h || makeUpsampleList(1, &p, W, H, &f) != RTS_OK) return RTS_ERR_INVALID_ARG;
    *w = (uint32_t)f.w;
    *h = (uint32_t)f.h;
    return RTS_OK;
}

extern "C" int rtsh_subsample_gbuffer(const rtsh_upsample_params* params, const float* positions, const float* normals,
                                      const uint8_t* lights_map, uint32_t W, uint32_t H, float* lo_positions, float* lo_normals,
                                      uint8_t* lo_lights_map) {
    if (!positions || !normals || !lo_positions || !lo_normals || (lights_map && !lo_lights_map)) return RTS_ERR_INVALID_ARG;
    UpsampleList f;
    const int s = makeUpsampleList(1, params, W, H, &f);
    if (s != RTS_OK) return s;
    for (size_t Y = 0; Y < (size_t)f.h; ++Y)
        for (size_t X = 0; X < (size_t)f.w; ++X) {
            const size_t q = Y * (size_t)f.w + X, p = (2 * Y + f.phaseY) * W + (2 * X + f.phaseX);
            memcpy(lo_positions + q * 4, positions + p * 4, 16);
            memcpy(lo_normals + q * 4, normals + p * 4, 16);
            if (lights_map) lo_lights_map[q] = lights_map[p];
        }
    return RTS_OK;
}

extern "C" int rtsh_upsample_retrace_map(uint32_t count, const rtsh_upsample_params* params, const float* positions, const float* normals,
                                         const uint8_t* lights_map, const float* lo_positions, const float* lo_normals,
                                         const uint8_t* lo_lights_map, uint32_t W, uint32_t H, uint8_t* retrace, int threads) {
    if (!positions || !normals || !lo_positions || !lo_normals || !retrace) return RTS_ERR_INVALID_ARG;
    UpsampleList f;
    const int s = makeUpsampleList(count, params, W, H, &f);
    if (s != RTS_OK) return s;
    const size_t n = (size_t)W * H;
    const FrameTexels<false> full{ positions, normals, nullptr, lights_map, nullptr, W, n };
    const FrameTexels<false> lo{ lo_positions, lo_normals, nullptr, lo_lights_map, nullptr, (size_t)f.w, (size_t)f.w * (size_t)f.h };
    parallelFor(n, 256, threads, [&](size_t i) { retrace[i] = upsampleRetracePixel(f, full, lo, (int)(i % W), (int)(i / W)); });
    return RTS_OK;
}

extern "C" int rtsh_upsample_light_list(const rts_light_list* list, const rtsh_upsample_params* params, const float* positions,
                                        const float* normals, const uint8_t* lights_map, const float* lo_positions, const float* lo_normals,
                                        const uint8_t* lo_lights_map, const uint8_t* lo_mask, const uint8_t* keep, uint32_t W, uint32_t H,
                                        uint8_t* mask, int threads) {
    if (!rts::lightListOk(list)) return RTS_ERR_INVALID_ARG;
    return upsampleListFrame<true>(list->count, params, positions, normals, lights_map, lo_positions, lo_normals, lo_lights_map, lo_mask, keep,
                                   W, H, mask, threads);
}

extern "C" int rtsh_upsample_soft_light_list(const rts_soft_light_list* list, const rtsh_upsample_params* params, const float* positions,
                                             const float* normals, const uint8_t* lights_map, const float* lo_positions,
                                             const float* lo_normals, const uint8_t* lo_lights_map, const uint8_t* lo_counts,
                                             const uint8_t* keep, uint32_t W, uint32_t H, uint8_t* counts, int threads) {
    if (!rts::softListOk(list)) return RTS_ERR_INVALID_ARG;
    return upsampleListFrame<false>(list->count, params, positions, normals, lights_map, lo_positions, lo_normals, lo_lights_map, lo_counts,
                                    keep, W, H, counts, threads);
}

// ---- compacted light maps (include/rts_scene.h; the tile order and the mark in rts_closest_hit.h: makeCompactFrame, compactSlotPixel,
// compactMarked) ----
extern "C" int rtsh_compact_light_map(uint32_t count, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t* pixels, uint32_t capacity,
                                      uint32_t* n_out) {
    CompactFrame f;
    if (!lights_map || !pixels || !n_out || capacity == 0 || !makeCompactFrame(count, W, H, &f)) return RTS_ERR_INVALID_ARG;
    uint32_t n = 0;
    for (uint32_t t = 0; t < f.tiles; ++t)
        for (uint32_t k = 0; k < 64u; ++k) {
            uint32_t p;
            if (!compactSlotPixel(f, t, k, &p) || !compactMarked(f, lights_map[p])) continue;
            if (n < capacity) pixels[n] = p;
            ++n;
        }
    *n_out = n;
    return RTS_OK;
}

extern "C" size_t rtsh_compact_scratch_bytes(uint32_t W, uint32_t H) {
    CompactFrame f;
    if (!makeCompactFrame(1, W, H, &f)) return 0;
    const size_t groups = ((size_t)f.tiles + kCompactScanTiles - 1u) / kCompactScanTiles;
    return ((size_t)f.tiles + groups) * sizeof(uint32_t);
}

extern "C" int rtsh_compact_nodes(void) { return kCompactNodes; }
