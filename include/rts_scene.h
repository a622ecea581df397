/* =============================================================================
 * rts_scene.h -- HARNESS entry points of librts.so (not part of the drop-in path).
 *
 * The reference feeds its shadow kernel from a Vulkan G-buffer pass and an OBJ file; neither
 * exists here, so the harness synthesises the same inputs:
 *   * rtsh_primary_positions : the RGBA32F "camera-relative world position" target that
 *     Source/Shaders/Model.frag:35,39 writes (closest hit per pixel centre through the same packed
 *     BVH; background pixels = (0,0,0,0), i.e. the clear value).
 *   * rtsh_obj_* : OBJ reader with the semantics of External/zeux_objparser/objparser.cpp and the
 *     flat-vertex expansion of RayTracedShadowsApp::loadModel (Source/RayTracedShadows.cpp:783-824).
 * ========================================================================== */
#ifndef RTS_SCENE_H
#define RTS_SCENE_H

#include <stddef.h>
#include <stdint.h>
#include "rts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pinhole camera as set up at Source/RayTracedShadows.cpp:238-242 (vertical fov in radians, lookAt
 * eye -> target, +Y up).  positions: W*H*4 floats.  hit_count (nullable) receives the number of
 * pixels that hit geometry.  threads: 0 = all host threads. */
int rtsh_primary_positions(const rts_vec4u* packed, size_t count_vec4, const float eye[3],
                           const float target[3], float fovy, uint32_t W, uint32_t H,
                           float* positions, uint64_t* hit_count, int threads);

/* Same plus the normal target (Model.frag:35,38: RGBA, face normal turned towards the viewer; 0 = background).
 * normals may be NULL. */
int rtsh_primary_gbuffer(const rts_vec4u* packed, size_t count_vec4, const float eye[3], const float target[3],
                         float fovy, uint32_t W, uint32_t H, float* positions, float* normals,
                         uint64_t* hit_count, int threads);

/* The same pass on the GPU: traces through the BVH already uploaded to `ctx`, writes DEVICE
 * buffers (W*H*4 floats each, d_normals may be NULL), asynchronous on `stream`, on the context's device.  Produces the
 * same bits as the host version (shared code, same FP rules).  One block per 8x8 tile in a two-dimensional grid, so the
 * frame may be at most RTSH_GBUFFER_MAX_HEIGHT rows tall: a taller one is RTS_ERR_INVALID_ARG, with nothing launched or
 * written (the host version has no such limit).  RTS_ERR_NO_BVH before rts_ctx_set_bvh. */
#define RTSH_GBUFFER_MAX_HEIGHT (8u * 65535u)
int rtsh_primary_gbuffer_device(rts_ctx* ctx, const float eye[3], const float target[3], float fovy,
                                uint32_t W, uint32_t H, float* d_positions, float* d_normals, void* stream);

/* Combine pass (Source/Shaders/Combine.frag:18-37 with the default white material):
 * rgb[W*H*3] = 255 * (1.25*max(0,N.L)*mask/samples + 0.15 + 0.05*(1 - max(0, N.-cameraDirection))), 0 where the
 * normal is 0.  max(0, x) is GLSL's (x > 0 ? x : 0: a NaN N.L or N.V contributes 0); the byte is 255 where
 * value*255 + 0.5 >= 255, its integer part where it lies in (0, 255), 0 otherwise, NaN included -- saturated before the
 * conversion, so huge, infinite and NaN normals give defined bytes, the same on the host and the device.
 * light == NULL: directional light from constants->lightDirection; positions needed for point lights. */
int rtsh_combine(const rts_constants* constants, const rts_light* light, const float* positions, const float* normals,
                 const uint8_t* mask, uint32_t W, uint32_t H, uint8_t* rgb);

/* The combine pass on the GPU (same per-pixel arithmetic, shared source): DEVICE buffers, d_rgb = W*H*3 bytes,
 * asynchronous on `stream`.  Together with rtsh_primary_gbuffer_device and rts_trace_shadow_mask_device the whole
 * frame -- G-buffer, shadow mask, lighting -- stays on the device (tools/render.py). */
int rtsh_combine_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light, const float* d_positions,
                        const float* d_normals, const uint8_t* d_mask, uint32_t W, uint32_t H, uint8_t* d_rgb,
                        void* stream);

/* The facing mark: an active map (include/rts.h, rts_trace_shadow_mask_active) for one light, made from the G-buffer.
 * active[p] = 0 where the normal's xyz are all zero (background: the combine pass leaves the pixel 0) or where N.L <= 0 -- N.L being
 * the very value the combine pass clamps (one shared function: L = the directional light, or normalize(light.xyz - P) for a point
 * light; a jittered light counts by its centre, as in the combine pass); 1 everywhere else, NaN included (a NaN is traced, never
 * culled).  For such a pixel direct = 1.25 * 0 * mask whatever the mask holds, so for finite inputs rtsh_combine over a mask traced
 * with this map equals rtsh_combine over the full mask, byte for byte: culling by this mark never changes the image.
 * light == NULL: directional light from constants->lightDirection; positions needed for point lights.  active: W*H bytes. */
int rtsh_facing_active(const rts_constants* constants, const rts_light* light, const float* positions, const float* normals,
                       uint32_t W, uint32_t H, uint8_t* active);

/* The same on the GPU (shared per-pixel source, the same bytes): DEVICE buffers, asynchronous on `stream`, one pixel per lane. */
int rtsh_facing_active_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light, const float* d_positions,
                              const float* d_normals, uint32_t W, uint32_t H, uint8_t* d_active, void* stream);

/* OCCLUDER DISTANCE on the host: the definition of rts_trace_rays_distance / rts_trace_shadow_distance (include/rts.h) as one
 * straight loop per ray -- the reference's walk without its return at a hit, its box and triangle tests, and the library's ray
 * set-up (same bias, same light model) --, multi-threaded (threads: 0 = all host threads).  Runs without a GPU: the checker of the
 * device forms, bit for bit.  packed / count_vec4: the Appendix-A stream (validated like rts_ctx_set_bvh's input).
 *   rtsh_rays_distance   : out_t[i] = distance of generic ray i.
 *   rtsh_shadow_distance : for rows [row_begin, row_end): distance[p] = the ray's distance where active[p] != 0 (active == NULL:
 *                          everywhere), +0.0f where it is 0; mask (nullable) = 1 exactly where the distance is +Inf, 0 elsewhere
 *                          and at inactive pixels.  Other rows are not touched.  Inactive positions are never read.
 *                          light->nsamples > 1 returns RTS_ERR_INVALID_ARG (several samples: rtsh_soft_distance). */
int rtsh_rays_distance(const rts_vec4u* packed, size_t count_vec4, const rts_ray* rays, size_t n, float* out_t, int threads);
int rtsh_shadow_distance(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_light* light,
                         const float* positions, const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin,
                         uint32_t row_end, float* distance, uint8_t* mask, int threads);

/* SOFT-SHADOW OCCLUDER DISTANCE on the host: the definition of rts_trace_soft_distance* (include/rts.h) as one straight loop over
 * (pixel, sample) -- sample j's light position xyz + offsets[j] (with light->table: the table index hashed from the pixel's index
 * y*W + x in the frame given here), rtsh_shadow_distance's ray set-up and one-ray distance, distance[p] = the integer minimum over the
 * samples, mask[p] (nullable) = the number of samples whose distance is +Inf.  Inactive pixels: +0.0f and 0, positions never read;
 * rows outside [row_begin, row_end) are not touched.  nsamples 0 or 1 gives rtsh_shadow_distance's bytes; nsamples > 64, a bad table or
 * type > RTS_LIGHT_POINT: RTS_ERR_INVALID_ARG.  Runs without a GPU: the checker of the device forms, bit for bit. */
int rtsh_soft_distance(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_light* light,
                       const float* positions, const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin,
                       uint32_t row_end, float* distance, uint8_t* mask, int threads);

/* AMBIENT OCCLUSION on the host: the definition of rts_trace_ambient_occlusion* (include/rts.h) as one straight loop over (pixel,
 * sample) on rtsh_soft_distance's walk -- the frame around the normal, L of sample j (with ao->table: the index hashed from the pixel's
 * index y*W + x in the frame given here), rtsh_shadow_distance's point-light ray set-up, u_j = 1 where the one-ray distance is +Inf;
 * counts[p] = their sum.  Background and inactive pixels: 0, positions never read; rows outside [row_begin, row_end) are not touched.
 * The refusals are rts_trace_ambient_occlusion's.  Runs without a GPU: the checker of the device forms, byte for byte.
 *
 * rtsh_ao_rays: the same rays as records for rts_trace_rays* / rtsh_rays_distance -- the n = max(1, nsamples) rays of pixel p at
 * rays[p * n + j] = { o.xyz, tmax = 1, d.xyz, 0 } as defined there; the 32 bytes of every ray of a background or inactive pixel are
 * zero (what the walk answers for such a record is no part of any count: sum the bytes of the other pixels only).  Whole frames only,
 * on all host threads.
 * rays: W * H * n records.  The refusals are rts_trace_ambient_occlusion's, without the row range.
 * BEWARE of tracing the zero records: a generic ray with d = 0 is never occluded but is no cheap ray -- its slab tests are NaN or
 * infinite, and from the world's origin it walks every box that contains the origin (all 2 M nodes of a 1 M-triangle city).  A frame
 * with sky should drop or compact them before rts_trace_rays* (DESIGN.md 4.34). */
int rtsh_ambient_occlusion(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_ao_params* ao,
                           const float* positions, const float* normals, const uint8_t* active, uint32_t W, uint32_t H,
                           uint32_t row_begin, uint32_t row_end, uint8_t* counts, int threads);
int rtsh_ao_rays(const rts_constants* constants, const rts_ao_params* ao, const float* positions, const float* normals,
                 const uint8_t* active, uint32_t W, uint32_t H, rts_ray* rays);

/* ADAPTIVE AMBIENT OCCLUSION on the host: the definition of rts_trace_ambient_occlusion_adaptive* (include/rts.h) applied literally,
 * one straight loop over (pixel, sample) on rtsh_ambient_occlusion's walk and set-up (the same frame, the same idx, the same point
 * light's ray at L) -- the first `probe` samples; where they agree, 0 or nsamples; where they disagree, the remaining samples and the
 * full count.  counts[p] as defined there, refined[p] (nullable) = 1 exactly where the full count was taken.  Background and inactive
 * pixels: 0 and 0, positions never read; rows outside [row_begin, row_end) are not touched.  The refusals are
 * rts_trace_ambient_occlusion_adaptive's.  Runs without a GPU: the checker of the device forms, byte for byte. */
int rtsh_ambient_occlusion_adaptive(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_ao_params* ao,
                                    const float* positions, const float* normals, const uint8_t* active, uint32_t W, uint32_t H,
                                    uint32_t row_begin, uint32_t row_end, uint32_t probe, uint8_t* counts, uint8_t* refined,
                                    int threads);

/* BENT NORMALS on the host: the definition of rts_trace_ambient_occlusion_bent* (include/rts.h) applied literally, one straight loop
 * over (pixel, sample) on rtsh_ambient_occlusion's walk and set-up -- the integer sum of Q(dirs[idx]) over the unoccluded samples, the
 * frame applied to it once; the quantisation and the final transform are the kernels' own source.  counts (nullable) and bent as
 * defined there.  Background and inactive pixels: 0 and (+0, +0, +0, +0), positions never read; rows outside [row_begin, row_end) are
 * not touched.  The refusals are rts_trace_ambient_occlusion_bent's.  Runs without a GPU: the checker of the device forms, bit for bit. */
int rtsh_ambient_occlusion_bent(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_ao_params* ao,
                                const float* positions, const float* normals, const uint8_t* active, uint32_t W, uint32_t H,
                                uint32_t row_begin, uint32_t row_end, uint8_t* counts, float* bent, int threads);

/* AO DISTANCE AND FALLOFF on the host: the definition of rts_trace_ambient_occlusion_distance* (include/rts.h) applied literally, one
 * straight loop over (pixel, sample) on rtsh_ambient_occlusion's walk and set-up -- the one-ray distance of every sample, their integer
 * minimum, the count of the free ones and the integer sum of the falloff's weights; bin, weight and quotient are the kernels' own
 * source.  counts, distance and obscurance (each nullable, distance or obscurance given) as defined there.  Background and inactive
 * pixels: 0, +0.0f and 0, positions never read; rows outside [row_begin, row_end) are not touched.  The refusals are
 * rts_trace_ambient_occlusion_distance's.  Runs without a GPU, multi-threaded: the checker of the device forms, bit for bit. */
int rtsh_ambient_occlusion_distance(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_ao_params* ao,
                                    const rts_ao_falloff* falloff, const float* positions, const float* normals, const uint8_t* active,
                                    uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, uint8_t* counts, float* distance,
                                    uint16_t* obscurance, int threads);

/* ADAPTIVE SOFT SHADOWS on the host: the definition of rts_trace_shadow_mask_adaptive* (include/rts.h) applied literally, one straight
 * loop over (pixel, sample) on rtsh_soft_distance's walk and ray set-up -- the first `probe` samples; where they agree, 0 or nsamples;
 * where they disagree, the remaining samples and the full count.  mask[p] as defined there, refined[p] (nullable) = 1 exactly where the
 * full count was taken.  Inactive pixels: 0 and 0, positions never read; rows outside [row_begin, row_end) are not touched.
 * light == NULL, nsamples < 2 or > 64, a bad table, type > RTS_LIGHT_POINT, probe == 0 or probe >= nsamples: RTS_ERR_INVALID_ARG.
 * Runs without a GPU: the checker of the device forms, byte for byte. */
int rtsh_shadow_mask_adaptive(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_light* light,
                              const float* positions, const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin,
                              uint32_t row_end, uint32_t probe, uint8_t* mask, uint8_t* refined, int threads);

/* LIGHT LISTS on the host: the definition of rts_trace_light_list* (include/rts.h) as one straight loop over (pixel, light) on
 * rtsh_shadow_distance's walk -- for rows [row_begin, row_end) and l < list->count, bit l of mask[p] = light l's one-ray distance is
 * +Inf, where lights_map == NULL or bit l of lights_map[p] is set; every other bit is 0.  A pixel whose map byte has no bit below
 * count gets 0 and its position is never read; other rows are not touched.  list == NULL, count 0 or > RTS_MAX_LIST_LIGHTS, or a
 * type > RTS_LIGHT_POINT: RTS_ERR_INVALID_ARG.  Runs without a GPU: the checker of the device forms, byte for byte.
 *
 * rtsh_facing_lights / rtsh_facing_lights_device: the light map a deferred renderer wants -- bit l of lights_map[p] = the facing mark
 * of light l (the one function the combine pass shares, so it equals rtsh_facing_active's byte for the light
 * { lights[l].type, 1 sample, lights[l].xyz }), bits >= count are 0.  positions may be NULL when no light of the list is a point
 * light.  The device form is asynchronous, one pixel per lane. */
int rtsh_light_list(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_light_list* list,
                    const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                    uint8_t* mask, int threads);
/* SOFT LIGHT LISTS on the host: the definition of rts_trace_soft_light_list* (include/rts.h) as one straight loop over (pixel, light,
 * sample) on rtsh_soft_distance's walk and ray set-up -- for rows [row_begin, row_end) and l < list->count, counts[l * W * H + p] = the
 * number of samples j of light l whose one-ray distance from p to xyz + radius * offsets[first + j] (a hard entry: to xyz as given) is
 * +Inf, where lights_map == NULL or bit l of lights_map[p] is set, else 0.  A pixel whose map byte has no bit below count gets 0 in
 * every plane and its position is never read; other rows and the planes l >= count are not touched.  The refusals of include/rts.h:
 * RTS_ERR_INVALID_ARG.  Runs without a GPU: the checker of the device forms, byte for byte. */
int rtsh_soft_light_list(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_soft_light_list* list,
                         const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                         uint8_t* counts, int threads);
/* SOFT LIGHT LIST DISTANCE on the host: the definition of rts_trace_soft_light_list_distance* (include/rts.h) as one straight loop over
 * (pixel, light, sample) on rtsh_soft_distance's walk and rtsh_soft_light_list's ray set-up -- distances[l * W * H + p] = the integer
 * minimum over light l's samples of the one-ray distance, counts[l * W * H + p] (counts nullable) = the number of them that are +Inf,
 * where lights_map == NULL or bit l of lights_map[p] is set, else +0.0f and 0.  A pixel whose map byte has no bit below count gets +0.0f
 * and 0 in every plane and its position is never read; other rows and the planes l >= count are not touched.  The refusals of
 * include/rts.h: RTS_ERR_INVALID_ARG.  Runs without a GPU: the checker of the device forms, bit for bit. */
int rtsh_soft_light_list_distance(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_soft_light_list* list,
                                  const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                                  uint32_t row_end, float* distances, uint8_t* counts, int threads);
/* ADAPTIVE SOFT LIGHT LISTS on the host: the definition of rts_trace_soft_light_list_adaptive* (include/rts.h) as one straight loop
 * over (pixel, light, sample) on rtsh_soft_light_list's walk and ray set-up -- light l's samples in order, and after its first
 * probes[l] != 0 of them the verdict 0 or max(1, nsamples_l) where they agree, no further ray; else the full count, and bit l of
 * refined[p] (optional; one plane for the list).  The refusals of include/rts.h: RTS_ERR_INVALID_ARG.  Runs without a GPU: the
 * checker of the device forms, byte for byte. */
int rtsh_soft_light_list_adaptive(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_soft_light_list* list,
                                  const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                                  uint32_t row_end, uint8_t* counts, const uint32_t* probes, uint8_t* refined, int threads);
/* JITTERED SOFT LIGHT LISTS on the host: the definition of rts_trace_soft_light_list_jittered* (include/rts.h) --
 * rtsh_soft_light_list_adaptive's loop, sample j of a light with a table tables[l] != 0 aimed at offsets[first + (start(p) + j) mod
 * tables[l]], p the pixel's index in the full frame.  tables == NULL: all zeros.  The refusals of include/rts.h: RTS_ERR_INVALID_ARG.
 * Runs without a GPU: the checker of the device forms, byte for byte. */
int rtsh_soft_light_list_jittered(const rts_vec4u* packed, size_t count_vec4, const rts_constants* constants, const rts_soft_light_list* list,
                                  const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                                  uint32_t row_end, uint8_t* counts, const uint32_t* probes, const uint32_t* tables, uint8_t* refined,
                                  int threads);
int rtsh_facing_lights(const rts_constants* constants, const rts_light_list* list, const float* positions, const float* normals,
                       uint32_t W, uint32_t H, uint8_t* lights_map);
int rtsh_facing_lights_device(rts_ctx* ctx, const rts_constants* constants, const rts_light_list* list, const float* d_positions,
                              const float* d_normals, uint32_t W, uint32_t H, uint8_t* d_lights_map, void* stream);

/* THE COMBINE PASS OF A LIGHT LIST: the image of a frame lit by all of a list's lights, from the list's own output, in ONE pass -- one
 * read of the normal (and, for point lights, the position) per pixel, one launch, one RGB frame.  For pixel p, n = normals[p].xyz:
 *   n all zero (background): rgb[p] = 0, 0, 0; nothing else of p is looked at (position, map byte and plane bytes may hold anything);
 *   ambient = 0.15f + 0.05f * (1 - max0(N.(-cameraDirection)))                                  -- rtsh_combine's, once per pixel;
 *   sum[c] = +0.0f;  for l = 0 .. count - 1, in this order, where lights_map == NULL or bit l of lights_map[p] is set:
 *       direct = 1.25f * max0(N.L_l) * ((float)byte_l / samples_l)    -- rtsh_combine's expression for light l alone (an area light
 *                                                                        counts by its centre), samples_l = (float)max(1, nsamples_l)
 *       sum[c] = sum[c] + direct * color_l[c]                         -- two rounded operations: the library is built without contraction
 *     (a light whose bit is clear adds nothing, and its plane byte at p is not looked at);
 *   rgb[p][c] = rtsh_combine's byte of sum[c] + ambient (saturated in float before the conversion, a NaN gives 0).
 * byte_l = counts[l * W * H + p] for a soft list (rts_trace_soft_light_list*'s planes); bit l of mask[p] as 0 or 1 with samples_l = 1
 * for a hard list (rts_trace_light_list*'s mask).  max0(x) = x > 0 ? x : 0.  The order of the sum is part of the definition: float
 * addition is not associative, and a fixed order is what lets the host form check the device form byte for byte.
 * ANCHOR: a list of one light, white or colors == NULL, no map, gives rtsh_combine's bytes for that light over that plane
 * (0 + direct * 1 + ambient is direct + ambient).  With the map of rtsh_facing_lights* and finite inputs the image equals the one
 * without a map (a culled light's direct term is 1.25 * 0 * byte).
 *   * colors: HOST memory in every form, count * 4 floats (light l at colors + 4 * l, .w ignored), passed to the kernel by value;
 *     NULL: every light (1, 1, 1).  Any float is allowed; the rule above defines the result.
 *   * positions may be NULL exactly when no light of the list is a point light; lights_map may be NULL; planes l >= count are never read.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: what rts_trace_light_list* / rts_trace_soft_light_list* refuse of a
 *     list; NULL constants, normals, mask / counts or rgb; a point light without positions; W == 0 or H == 0; a NULL ctx.
 *   * the device forms take DEVICE buffers (colors excepted), are asynchronous on `stream`, allocate nothing and read nothing back;
 *     under graph capture each adds ONE kernel node, list, colours and constants by value.  They need no BVH and no alignment of any
 *     buffer beyond its element type's.  One pixel per lane. */
int rtsh_combine_light_list(const rts_constants* constants, const rts_light_list* list, const float* colors, const float* positions,
                            const float* normals, const uint8_t* lights_map, const uint8_t* mask, uint32_t W, uint32_t H, uint8_t* rgb);
int rtsh_combine_soft_light_list(const rts_constants* constants, const rts_soft_light_list* list, const float* colors,
                                 const float* positions, const float* normals, const uint8_t* lights_map, const uint8_t* counts,
                                 uint32_t W, uint32_t H, uint8_t* rgb);
int rtsh_combine_light_list_device(rts_ctx* ctx, const rts_constants* constants, const rts_light_list* list, const float* colors,
                                   const float* d_positions, const float* d_normals, const uint8_t* d_lights_map, const uint8_t* d_mask,
                                   uint32_t W, uint32_t H, uint8_t* d_rgb, void* stream);
int rtsh_combine_soft_light_list_device(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list, const float* colors,
                                        const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                        const uint8_t* d_counts, uint32_t W, uint32_t H, uint8_t* d_rgb, void* stream);

/* THE FILTER OF A LIGHT LIST'S PLANES: from the count planes of a soft light list (or the mask of a hard one) to one FLOAT VISIBILITY
 * plane per light -- a spatial, edge-aware, optionally distance-guided filter: the stage between a trace of few samples (five grey
 * levels for four samples; the noise of a jitter table) and the image.  The result is a function of the inputs alone: every sum
 * across pixels is an INTEGER sum, floats appear in per-tap comparisons and in one division per light, and the library is built
 * without contraction -- so no order of the taps, no tiling and no option can change a bit, and the host form checks the device form
 * bit for bit.  All buffers are whole frames of W x H.
 *   typedef struct rtsh_filter_params: radius R (0 .. RTSH_FILTER_MAX_RADIUS: the window is (2R+1) x (2R+1) pixels), normal_cos_min,
 *   plane_eps (world units), spread[l] (per light, used with distances only), reserved_ (ignored).
 * For pixel p = (x, y) and light l < count:  n_l = max(1, nsamples_l) (1 for a hard list);  c_l(q) = the byte of plane l at q
 * (counts[l * W * H + q]; bit l of mask[q] as 0 or 1 for a hard list), unclamped, as the combine pass reads it;  on(q, l) = lights_map
 * == NULL or bit l of lights_map[q] is set;  bg(q) = normals[q].xyz all zero;  N_q = normals[q].xyz, P_q = positions[q].xyz.
 *   INACTIVE: where bg(p) or not on(p, l), visibility[l * W * H + p] = +0.0f and nothing else of p is looked at for that light.
 *   TAPS: otherwise, over the taps q = (x + dx, y + dy) INSIDE THE FRAME with |dx|, |dy| <= R, each of the integer tent weight
 *     w = (R + 1 - |dx|) * (R + 1 - |dy|):  the centre tap q == p is always accepted; another tap is accepted when geom(p, q) and
 *     lit(p, q, l) both hold; every comparison is written so that a NaN rejects the tap --
 *       geom(p, q): not bg(q), and (Np.x*Nq.x + Np.y*Nq.y) + Np.z*Nq.z >= normal_cos_min, and fabsf(h) <= plane_eps, where
 *                   D = P_q - P_p (three subtractions) and h = (Np.x*D.x + Np.y*D.y) + Np.z*D.z.  It does not depend on the light;
 *                   the position of a background tap is never looked at.
 *       lit(p, q, l), distances == NULL: on(q, l).
 *       lit(p, q, l), with distances:    on(q, l), and either m is +Inf (0x7F800000) or (D.x*D.x + D.y*D.y) + D.z*D.z <=
 *                   (spread_l * m) * (spread_l * m), m = the smaller of the BIT PATTERNS of distances[l][p] and distances[l][q] taken
 *                   as unsigned 32-bit integers (for the traces' planes, which hold +0 .. +Inf: the smaller distance), read as a float.
 *                   This is the contact-hardening guide: two pixels share their counts only across less than the penumbra width at
 *                   the nearer blocker, spread_l times the ray parameter -- world distance for a directional light, a fraction of
 *                   the segment for a point light.  The CALLER folds the light's size and range into spread_l.
 *   QUOTIENT: num = sum of w * c_l(q), den = sum of w * n_l over the accepted taps, both unsigned 32-bit integers below 2^24
 *     (255 * 81 * 289);  visibility[l * W * H + p] = (float)num / (float)den, one rounded division.
 * ANCHORS: (1) R = 0, or thresholds that accept no neighbour: (float)c / (float)n_l, the very quotient the list combine pass forms
 * (the fraction reduces: the weight cancels exactly).  (2) Where every accepted tap of a pixel carries the same byte c, the result is
 * (float)c / (float)n_l: the device form skips the walk for a light whose bytes are all equal over a block's window.
 *   * distances: NULL, or the planes of rts_trace_soft_light_list_distance* (soft form only).  lights_map may be NULL.  positions is
 *     always required.  visibility: count * W * H floats; planes of any buffer from `count` up are never touched.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: what rtsh_combine_*_light_list* refuse of a list; NULL params, positions,
 *     normals, mask / counts or visibility; radius > RTSH_FILTER_MAX_RADIUS; a normal_cos_min or plane_eps that is not finite; with
 *     distances, a spread_l (l < count) that is negative or not finite; W == 0 or H == 0; a NULL ctx.
 *   * host forms: multi-threaded (threads: 0 = all host threads).  Device forms: DEVICE buffers, asynchronous on `stream`, allocate
 *     nothing and read nothing back; under graph capture each adds ONE kernel node, list and parameters by value (params is read
 *     during the call).  They need no BVH and no alignment of any buffer beyond its element type's.
 *   * OUT OF SCOPE: row ranges and stripes (a stripe would need a halo of R rows from its neighbours), variance guidance.  (The
 *     temporal stage is rtsh_accumulate_visibility_list below; the form for a reach beyond 8 pixels is rtsh_wide_filter_*_light_list*
 *     further below: another filter, an a-trous one.) */
enum { RTSH_FILTER_MAX_RADIUS = 8 };
typedef struct rtsh_filter_params {
    uint32_t radius;          /* R, 0 .. RTSH_FILTER_MAX_RADIUS (8): the window is (2R+1) x (2R+1) pixels */
    float    normal_cos_min;  /* a tap needs N_p . N_q >= this */
    float    plane_eps;       /* ... and |N_p . (P_q - P_p)| <= this (world units) */
    float    spread[RTS_MAX_LIST_LIGHTS]; /* per light, used with distances only: finite, >= 0 */
    uint32_t reserved_[5];    /* ignored */
} rtsh_filter_params;                                                              /* 64 bytes */
int rtsh_filter_light_list(const rts_light_list* list, const rtsh_filter_params* params, const float* positions, const float* normals,
                           const uint8_t* lights_map, const uint8_t* mask, uint32_t W, uint32_t H, float* visibility, int threads);
int rtsh_filter_soft_light_list(const rts_soft_light_list* list, const rtsh_filter_params* params, const float* positions,
                                const float* normals, const uint8_t* lights_map, const uint8_t* counts, const float* distances,
                                uint32_t W, uint32_t H, float* visibility, int threads);
int rtsh_filter_light_list_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_filter_params* params, const float* d_positions,
                                  const float* d_normals, const uint8_t* d_lights_map, const uint8_t* d_mask, uint32_t W, uint32_t H,
                                  float* d_visibility, void* stream);
int rtsh_filter_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_filter_params* params,
                                       const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                       const uint8_t* d_counts, const float* d_distances, uint32_t W, uint32_t H, float* d_visibility,
                                       void* stream);

/* THE VISIBILITY COMBINE: the combine pass of a light list (above) with visibility[l * W * H + p] -- a filter's plane -- in place of
 * (float)byte_l / samples_l:  direct = 1.25f * max0(N.L_l) * visibility_l;  everything else, the order of the sum and every refusal
 * included, is rtsh_combine_light_list's (`visibility` in the place of `mask`).  Any float is allowed in a plane; a light whose map
 * bit is clear and a background pixel do not look at theirs.  ANCHOR: over the planes of an R = 0 filter it gives
 * rtsh_combine_soft_light_list's bytes (rtsh_combine_light_list's for a hard list), byte for byte.  `list` gives types and positions;
 * for a soft list pass the rts_light_list of the same types and positions. */
int rtsh_combine_visibility_list(const rts_constants* constants, const rts_light_list* list, const float* colors, const float* positions,
                                 const float* normals, const uint8_t* lights_map, const float* visibility, uint32_t W, uint32_t H,
                                 uint8_t* rgb);
int rtsh_combine_visibility_list_device(rts_ctx* ctx, const rts_constants* constants, const rts_light_list* list, const float* colors,
                                        const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                        const float* d_visibility, uint32_t W, uint32_t H, uint8_t* d_rgb, void* stream);

/* THE VISIBILITY COMBINE WITH AMBIENT OCCLUSION: rtsh_combine_visibility_list* with the ambient term scaled per pixel --
 * ambient' = ambient * ao[p], ONE rounded multiply; nothing else changes, every refusal included.  `ao`: W x H floats, any float
 * allowed (the filtered plane of an AO count plane: (float)c / (float)n after the R = 0 filter); not looked at on background pixels.
 * ao == NULL: RTS_ERR_INVALID_ARG (the call above is the form without AO).  ANCHOR: with a plane of 1.0f it gives
 * rtsh_combine_visibility_list's bytes.  The device form adds one kernel node; the per-pixel source is shared, byte for byte. */
int rtsh_combine_visibility_list_ao(const rts_constants* constants, const rts_light_list* list, const float* colors, const float* positions,
                                    const float* normals, const uint8_t* lights_map, const float* visibility, const float* ao, uint32_t W,
                                    uint32_t H, uint8_t* rgb);
int rtsh_combine_visibility_list_ao_device(rts_ctx* ctx, const rts_constants* constants, const rts_light_list* list, const float* colors,
                                           const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                           const float* d_visibility, const float* d_ao, uint32_t W, uint32_t H, uint8_t* d_rgb,
                                           void* stream);

/* THE VISIBILITY COMBINE WITH AMBIENT OCCLUSION AND A SKY: rtsh_combine_visibility_list_ao* with a hemispheric tint on the ambient
 * term, aimed by the pixel's bent vector (rts_trace_ambient_occlusion_bent*'s plane, W x H RGBA32F; .w is not read): where the open
 * part of the hemisphere looks along `up` the ambient light takes the sky's colour, against it the ground's.  Per non-background pixel
 * p, b = bent[p].xyz, every operation ONE rounded float operation, parenthesised as written, no contraction:
 *   l2 = ((b.x * b.x) + (b.y * b.y)) + (b.z * b.z);   len = sqrtf(l2);
 *   u  = (((b.x * up.x) + (b.y * up.y)) + (b.z * up.z)) / len  if len > 0 and len is finite, else 0;
 *   h  = 0.5f + 0.5f * u;   h = (h > 0) ? ((h < 1) ? h : 1) : 0   (a NaN becomes 0);
 *   tint_c = ground_c + (sky_c - ground_c) * h;   channel c's ambient term = (ambient * ao[p]) * tint_c.
 * Everything else is rtsh_combine_visibility_list_ao's: the direct terms, the order of the sum, the rounding to bytes and every refusal;
 * NULL bent or NULL sky: RTS_ERR_INVALID_ARG as well.  Any float is allowed in `bent` and in the sky.  ANCHORS: sky == ground ==
 * (1, 1, 1) gives rtsh_combine_visibility_list_ao's bytes (1 + 0 * h == 1); an all-zero bent texel gives h = 0.5.  The device form adds
 * one kernel node, the sky by value; the per-pixel source is shared, byte for byte. */
typedef struct rtsh_sky_ambient {
    float up[3];        /* the direction of the sky; normalise it (it is used as given) */
    float sky[3];       /* the ambient light's colour where the bent vector points along up */
    float ground[3];    /* ... and where it points against it */
    float reserved_[3]; /* ignored */
} rtsh_sky_ambient;     /* 48 bytes */
int rtsh_combine_visibility_list_ao_bent(const rts_constants* constants, const rts_light_list* list, const float* colors,
                                         const float* positions, const float* normals, const uint8_t* lights_map, const float* visibility,
                                         const float* ao, const float* bent, const rtsh_sky_ambient* sky, uint32_t W, uint32_t H,
                                         uint8_t* rgb);
int rtsh_combine_visibility_list_ao_bent_device(rts_ctx* ctx, const rts_constants* constants, const rts_light_list* list, const float* colors,
                                                const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                const float* d_visibility, const float* d_ao, const float* d_bent,
                                                const rtsh_sky_ambient* sky, uint32_t W, uint32_t H, uint8_t* d_rgb, void* stream);

/* THE TEMPORAL ACCUMULATION OF A LIGHT LIST'S VISIBILITY: this frame's float visibility planes (a filter's output; the R = 0 filter is
 * the conversion from counts) blended with LAST frame's result, which is fetched through the camera motion -- reprojected -- and
 * rejected where the surface seen last frame is another one (a disocclusion).  It is the stage that turns 4 samples per frame into 16
 * or 48 over frames: the jitter hash takes no frame term, the CALLER rotates its shared offsets table per frame.  The result is a
 * function of the inputs alone: bilinear weights are INTEGERS on a 1/32-pixel grid, every float step below is one rounded float32
 * operation (the library is built without contraction), and the order of the four taps is part of the definition -- so the host form
 * checks the device form bit for bit.  All buffers are whole frames of W x H.
 *   CURRENT frame: positions, normals, lights_map (may be NULL), visibility (count float planes).
 *   PREVIOUS frame: prev_positions, prev_normals, prev_visibility (the history, count float planes), prev_lengths (count byte planes:
 *     how many frames a pixel's history holds, 0 = none).  All four NULL: the FIRST FRAME (no history); all four or none.
 *   Outputs: visibility_out (count float planes), lengths_out (count byte planes).
 *   typedef struct rtsh_temporal_params: eye_delta (current eye minus previous eye; positions are camera-relative), prev_right, prev_up,
 *   prev_fwd (the previous camera's basis), prev_scale_x = tanHalf * aspect and prev_scale_y = tanHalf of the previous camera,
 *   normal_cos_min, plane_eps, max_length (1 .. 255), reset_lights (bit l set: light l takes no history this frame -- it moved),
 *   reserved_ (ignored).  rtsh_camera_basis gives the numbers the G-buffer pass itself used.
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  For pixel p = (x, y) and light l < count, N_p = normals[p].xyz, P_p = positions[p].xyz:
 *   INACTIVE: where N_p is all zero, or lights_map != NULL and bit l of lights_map[p] is clear: visibility_out[l][p] = +0.0f,
 *     lengths_out[l][p] = 0, and nothing else of p is looked at for that light.
 *   REPROJECT (once per pixel): Q = P_p + eye_delta (three additions); z = dot3(Q, prev_fwd); a = dot3(Q, prev_right) / z;
 *     b = dot3(Q, prev_up) / z;  fx = (a / prev_scale_x + 1.0f) * (0.5f * (float)W) - 0.5f;
 *     fy = (1.0f - b / prev_scale_y) * (0.5f * (float)H) - 0.5f  (the inverse of the primary pass's pixel-to-direction map);
 *     gx = fx * 32.0f + 0.5f, gy = fy * 32.0f + 0.5f.  p is ON SCREEN when z > 0, gx >= -32.0f, gx < (float)W * 32.0f, gy >= -32.0f and
 *     gy < (float)H * 32.0f all hold (a NaN fails).  Then ix = (int32_t)floorf(gx), x0 = ix >> 5 (floor), ax = ix & 31, and the same
 *     for y.  The four taps IN THIS ORDER: (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), of the INTEGER weights
 *     (32-ax)*(32-ay), ax*(32-ay), (32-ax)*ay, ax*ay, which sum to 1024.
 *   A tap q is ACCEPTED for light l when: its weight is not 0; q is inside the frame; prev_normals[q].xyz is not all zero;
 *     dot3(N_p, N'_q) >= normal_cos_min; fabsf(dot3(N_p, P'_q - Q)) <= plane_eps (three subtractions; P'_q and Q are both relative to
 *     the previous eye, so for static geometry this is the disocclusion test); prev_lengths[l][q] != 0; bit l of reset_lights is clear.
 *     The first five do not depend on the light.  Every comparison is written so that a NaN rejects.  The position and the history of a
 *     rejected tap are not looked at.
 *   BLEND: sw = the integer sum of the accepted weights; sv = +0.0f, then for the accepted taps in the order above
 *     sv = sv + (float)w * prev_visibility[l][q]; m = the smallest prev_lengths[l][q] over the accepted taps.  With no accepted tap, or p
 *     not on screen, or on the first frame: visibility_out[l][p] = visibility[l][p] (its bits), lengths_out[l][p] = 1.  Otherwise
 *     n = min(m + 1, max_length), lengths_out[l][p] = n, and visibility_out[l][p] = visibility[l][p] if n == 1, else
 *     v = prev + (cur - prev) * (1.0f / (float)n) with prev = sv / (float)sw and cur = visibility[l][p]; where v is a NaN (v != v),
 *     the word stored is the canonical quiet NaN 0x7FC00000, whatever NaN the machine's arithmetic produced -- which NaN an operation
 *     returns is the one thing hosts and the GPU disagree on.  Only a BLENDED value is treated so: a value passed through
 *     (visibility_out = visibility[l][p]: no accepted tap, off screen, first frame, n == 1) keeps its bits, a NaN's payload included.
 *   Any float is allowed in any plane; the rule, with the NaN step, defines every bit of the result.
 * ANCHORS: (1) max_length == 1, or all-ones reset_lights, or the first frame: visibility_out is visibility, bit for bit, at active
 * pixels, and lengths_out is 1 there.  (2) A still camera -- params from rtsh_camera_basis of the very camera both G-buffers were made
 * with, eye_delta 0: every non-background pixel lands on itself (ax == ay == 0: one tap of weight 1024; the float32 inverse misses a
 * pixel centre by up to 0.0023 pixel at 7680 wide for frames of ordinary aspect, well inside the 1/64 pixel that rounds to ax == 0;
 * the miss grows with W / H -- 0.0084 pixel for a strip of 1920 x 8 -- and from an aspect of a few hundred on some pixels of a still
 * camera take two taps: the rule still defines them, the anchor no longer covers them), 1024 * h / 1024 is exact for
 * a history value in the normal range, and frame k holds h_k = h_(k-1) + (c_k - h_(k-1)) * (1 / min(k, max_length)): a running mean,
 * then an exponential one.  (3) A light whose bit is set in reset_lights gets anchor 1 whatever the other lights do.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: what rtsh_filter_*_light_list* refuse of a list; NULL params, positions,
 *     normals, visibility, visibility_out or lengths_out; some but not all of the four prev_* NULL; max_length 0 or above 255; a
 *     normal_cos_min, plane_eps, eye_delta, basis or scale component that is not finite; a scale that is not > 0; W or H equal to 0 or
 *     above 65536 (so that (float)W * 32 and ix stay exact); visibility_out == prev_visibility or lengths_out == prev_lengths (the pass
 *     gathers from neighbours: history must ping-pong); a NULL ctx.
 *   * visibility_out == visibility IS allowed: a pixel reads only its own current value, and reads it before it writes.
 *   * planes of any buffer from `count` up are never touched.  Only `count` of the list matters; it is the list the visibility combine
 *     takes.
 *   * host form: multi-threaded (threads: 0 = all host threads).  Device form: DEVICE buffers, asynchronous on `stream`, allocates
 *     nothing and reads nothing back; under graph capture ONE kernel node, list and params by value (params is read during the call).
 *     No BVH, no alignment of any buffer beyond its element type's.
 *   * OUT OF SCOPE: (moving geometry is followed by the motion forms at the end of this header, DESIGN.md 4.29;) variance clamping of
 *     the history (a mean +- k sigma box needs a square root; the min/max box is rtsh_accumulate_visibility_list_clamped below),
 *     accumulating distance planes (the count planes' moments: rtsh_accumulate_moments_soft_light_list below), row ranges and
 *     stripes, a frame term in the jitter hash. */
typedef struct rtsh_temporal_params {
    float    eye_delta[3];                             /* current eye - previous eye */
    float    prev_right[3], prev_up[3], prev_fwd[3];   /* the previous camera's basis */
    float    prev_scale_x, prev_scale_y;               /* its tanHalf * aspect and tanHalf: finite, > 0 */
    float    normal_cos_min;                           /* a tap needs N_p . N'_q >= this */
    float    plane_eps;                                /* ... and |N_p . (P'_q - Q)| <= this (world units) */
    uint32_t max_length;                               /* 1 .. 255 */
    uint32_t reset_lights;                             /* bit l: light l takes no history this frame */
    uint32_t reserved_[2];                             /* ignored */
} rtsh_temporal_params;                                                            /* 80 bytes */
/* The camera the primary pass (rtsh_primary_gbuffer*) builds from (eye, target, fovy, W, H), exactly: out = eye[3], fwd[3], right[3],
 * up[3], tanHalf, aspect.  RTS_ERR_INVALID_ARG for a NULL pointer or W == 0 or H == 0. */
int rtsh_camera_basis(const float eye[3], const float target[3], float fovy, uint32_t W, uint32_t H, float out[14]);
int rtsh_accumulate_visibility_list(const rts_light_list* list, const rtsh_temporal_params* params, const float* positions,
                                    const float* normals, const uint8_t* lights_map, const float* visibility, const float* prev_positions,
                                    const float* prev_normals, const float* prev_visibility, const uint8_t* prev_lengths, uint32_t W,
                                    uint32_t H, float* visibility_out, uint8_t* lengths_out, int threads);
int rtsh_accumulate_visibility_list_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_temporal_params* params,
                                           const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                           const float* d_visibility, const float* d_prev_positions, const float* d_prev_normals,
                                           const float* d_prev_visibility, const uint8_t* d_prev_lengths, uint32_t W, uint32_t H,
                                           float* d_visibility_out, uint8_t* d_lengths_out, void* stream);

/* THE CLAMPED FORM OF THE TEMPORAL ACCUMULATION: the pass above rejects history by the RECEIVER's geometry alone, so when an occluder or
 * a light moves it keeps blending a shadow that is no longer there (max_length 32: a pixel that has just become lit still shows 97 % of
 * it), and reset_lights throws a light's whole history away, noise reduction included.  Here a pixel's reprojected history is first
 * CLAMPED into the range its light's CURRENT visibility spans over a (2r+1) x (2r+1) window around the pixel.  The range is a minimum
 * and a maximum, so it does not depend on any order, and the host form checks the device form bit for bit as above.
 * Everything of rtsh_accumulate_visibility_list holds unchanged -- INACTIVE, REPROJECT, tap acceptance, sw, sv, m, n, the pass-through
 * cases, the canonical NaN --; ONE step is added between prev = sv / (float)sw and the lerp, so only where a value is blended (n != 1).
 *   ORDER: for a float of bits u, key(u) = u ^ ((u >> 31) ? 0xFFFFFFFF : 0x80000000), compared as unsigned integers: a total order on
 *     the non-NaN floats in which -0 < +0.  The minimum and maximum below are integer min/max of keys: no order of taps, no tiling, no
 *     staging scheme can change a bit.
 *   BOX of pixel p = (x, y) for light l: of the taps q = (x+dx, y+dy), |dx| <= r and |dy| <= r, those CONTRIBUTE for which q lies
 *     inside the frame, normals[q].xyz is not all zero, lights_map is NULL or bit l of lights_map[q] is set, and visibility[l][q] is
 *     not a NaN (v != v).  (The middle two exclude the +0.0f that inactive pixels hold.)  The centre is a tap like any other: active
 *     by the INACTIVE rule, it contributes unless it is a NaN.  lo and hi are the contributing values of the smallest and the largest
 *     key; where in the window they lie is never looked at.
 *   CLAMP: with no contributing tap, prev is used as it is.  Otherwise lo_m = lo - margin and hi_m = hi + margin (one rounded
 *     operation each) and prev' = prev < lo_m ? lo_m : (prev > hi_m ? hi_m : prev); a NaN prev fails both comparisons and stays.  The
 *     lerp reads v = prev' + (cur - prev') * (1.0f / (float)n).  lengths_out is what the unclamped rule gives: the clamp does not
 *     shorten a history.
 * ANCHORS: (1) Over finite planes, a margin so large that lo_m <= prev <= hi_m everywhere (3.0e38f over planes in [0, 1]) gives the
 * unclamped pass's bits, wherever every blended pixel has a contributing tap -- true when the current planes hold no NaN, the centre
 * being one.  (With a plane value or a history beyond +-(FLT_MAX - margin) the sums overflow or round and the anchor ends.)
 * (2) radius 0 with margin 0: lo_m = hi_m = cur, so prev' = cur and visibility_out == visibility, bit for bit, at every blended pixel
 * whose current value is finite and not -0 and whose prev is not a NaN: cur + (cur - cur) * k is cur.  -0 is excepted because
 * hi_m = -0 + 0 is +0 (and a prev above it then gives +0 + (-0 - +0) * k = +0, not -0); the infinities because Inf - Inf is a NaN,
 * stored as the canonical one; a NaN prev because it stays.  (3) The pass-through cases -- the first frame, max_length 1, a light in
 * reset_lights, a pixel with no accepted tap -- keep the current bits exactly as above: the clamp never touches them.  (4) THE STEP:
 * history 1.0f of length >= 1 everywhere, current 0.0f everywhere, a still camera, margin 0: the result is exactly +0.0f at any radius
 * and any max_length, where the unclamped pass gives 1 - 1/n.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: everything the unclamped form refuses; a NULL clamp; radius above
 *     RTSH_CLAMP_MAX_RADIUS; a margin that is negative or not finite; visibility_out == visibility -- the unclamped form allows it,
 *     this one reads its neighbours' current values and cannot (overlap other than equality is the caller's error, as everywhere).
 *   * reserved_ is ignored.  Planes from `count` up are never touched.  Host form: multi-threaded.  Device form: DEVICE buffers,
 *     asynchronous on `stream`, allocates nothing, reads nothing back; under graph capture ONE kernel node, list, params and clamp by
 *     value.  No BVH, no alignment of any buffer beyond its element type's. */
enum { RTSH_CLAMP_MAX_RADIUS = 4 };
typedef struct rtsh_history_clamp {
    uint32_t radius;                                   /* r, 0 .. RTSH_CLAMP_MAX_RADIUS: the window is (2r+1) x (2r+1) pixels */
    float    margin;                                   /* finite, >= 0: the box is widened by this on both sides */
    uint32_t reserved_[2];                             /* ignored */
} rtsh_history_clamp;                                                              /* 16 bytes */
int rtsh_accumulate_visibility_list_clamped(const rts_light_list* list, const rtsh_temporal_params* params, const float* positions,
                                            const float* normals, const uint8_t* lights_map, const float* visibility,
                                            const float* prev_positions, const float* prev_normals, const float* prev_visibility,
                                            const uint8_t* prev_lengths, uint32_t W, uint32_t H, float* visibility_out,
                                            uint8_t* lengths_out, const rtsh_history_clamp* clamp, int threads);
int rtsh_accumulate_visibility_list_clamped_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_temporal_params* params,
                                                   const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                   const float* d_visibility, const float* d_prev_positions, const float* d_prev_normals,
                                                   const float* d_prev_visibility, const uint8_t* d_prev_lengths, uint32_t W, uint32_t H,
                                                   float* d_visibility_out, uint8_t* d_lengths_out, const rtsh_history_clamp* clamp,
                                                   void* stream);

/* THE WIDE FILTER OF A LIGHT LIST'S PLANES: an a-trous filter -- up to five passes of one 5 x 5 kernel whose taps lie 1, 2, 4, 8 and 16
 * pixels apart -- from the count planes of a soft light list (or the mask of a hard one) to one float visibility plane per light.  Its
 * cost grows with the logarithm of its reach (2 * (2^passes - 1) pixels: 2, 6, 14, 30, 62), where rtsh_filter_*_light_list* above walk
 * every tap of a (2R+1)^2 window.  It is ANOTHER filter, not a faster form of that one: the two agree only where the anchors below say
 * so.  The result is a function of the inputs alone: the planes between passes are 16-BIT FIXED POINT and every sum across pixels is an
 * INTEGER sum -- a float intermediate would make the result depend on the order of a float sum over taps --, floats appear in per-tap
 * comparisons and in one division per light at the end; so no order of taps, no tiling and no staging form can change a bit, and the
 * host form checks the device form bit for bit.  All buffers are whole frames of W x H.
 *   typedef struct rtsh_wide_filter_params: passes (0 .. RTSH_WIDE_FILTER_MAX_PASSES), normal_cos_min, plane_eps, reserved_ (ignored).
 * For light l < count:  n_l = max(1, nsamples_l) (1 for a hard list);  S_l = 65535 / n_l by integer division (65535 for a hard light,
 * 16383 for 4 samples, 1365 for 48);  on(q, l), bg(q), N_q, P_q and c_l(q) are the filter's above.
 *   INPUT: V_0(q, l) = min(c_l(q), n_l) * S_l.  The CLAMP to n_l is this filter's own (the filter above reads the byte unclamped): it
 *     makes V fit 16 bits at full precision for every n_l, and the traces never write more than n_l.
 *   PASS k (k = 0 .. passes - 1, step s = 1 << k), for an ACTIVE pixel p = (x, y) -- not bg(p), and on(p, l) --: over the taps
 *     q = (x + dx * s, y + dy * s), dx, dy in -2 .. 2, INSIDE THE FRAME, each of the integer weight w = b[|dx|] * b[|dy|],
 *     b = {6, 4, 1} (the 25 weights sum to 256):  the centre tap is always accepted; another tap is accepted when geom(p, q) -- the
 *     filter's expression above: not bg(q), the normal test against normal_cos_min, the plane test against plane_eps, a NaN rejects;
 *     evaluated once per tap for all lights -- and on(q, l) hold.  num = sum of w * V_k(q, l), den = sum of w over the accepted taps
 *     (num <= 65535 * 256 < 2^24: everything fits 32 bits), and V_(k+1)(p, l) = (2 * num + den) / (2 * den) by integer division: the
 *     ROUNDED MEAN.  An INACTIVE pixel carries V = 0 in every pass and is never accepted.
 *   OUTPUT: visibility[l * W * H + p] = (float)V_passes / (float)(n_l * S_l), one correctly rounded division of two integers below
 *     2^16, formed by the last pass itself; +0.0f at an inactive pixel.
 * ANCHORS: (1) passes == 0, or thresholds that accept no neighbour at any pass: (float)(c * S_l) / (float)(n_l * S_l), which is
 * (float)c / (float)n_l bit for bit (c the clamped byte) -- the R = 0 filter's plane wherever c <= n_l, so the visibility combine over
 * it gives the list combine's bytes.  (2) Where every accepted tap of every pass carries the same value, the rounded mean of equal
 * values is that value and the result is the centre's quotient.  (3) RANGE: every V_(k+1)(p) lies between the smallest and the largest
 * accepted V_k; visibility never leaves [0, 1].
 *   * lights_map may be NULL; positions is always required.  visibility: count * W * H floats; planes of any buffer from `count` up are
 *     never touched.
 *   * host forms: multi-threaded (threads: 0 = all host threads); they allocate their own intermediates.
 *   * device forms: DEVICE buffers, asynchronous on `stream`, allocate nothing and read nothing back.  d_scratch: 2 * count * W * H
 *     uint16_t (rtsh_wide_filter_scratch_bytes), aligned to 2 bytes and no more, used as two ping-pong sets of count planes (the second
 *     begins count * W * H elements in); it may be NULL when passes <= 1, and nothing of it is touched then.  Under graph capture a
 *     call adds exactly max(1, passes) KERNEL nodes on one chain, list and parameters by value (params is read during the call).  No
 *     BVH, no alignment of any other buffer beyond its element type's.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: what rtsh_filter_*_light_list* refuse of a list; NULL params, positions,
 *     normals, mask / counts or visibility; passes > RTSH_WIDE_FILTER_MAX_PASSES; a normal_cos_min or plane_eps that is not finite;
 *     W == 0 or H == 0, W or H above 0x7FFFFFF0; in the device forms a NULL ctx, H above 16 * 65535 (the grid), a NULL d_scratch with
 *     passes >= 2, and d_visibility equal to d_scratch or to its second half (overlap other than equality is the caller's error).
 *   * OUT OF SCOPE: distance planes as a guide (the spread guide of the filter above degenerated at these resolutions, and no useful
 *     spread is known), row ranges and stripes.  (Variance guidance is rtsh_wide_filter_guided_soft_light_list below.) */
enum { RTSH_WIDE_FILTER_MAX_PASSES = 5 };
typedef struct rtsh_wide_filter_params {
    uint32_t passes;          /* 0 .. RTSH_WIDE_FILTER_MAX_PASSES (5): pass k has its taps 1 << k pixels apart */
    float    normal_cos_min;  /* a tap needs N_p . N_q >= this */
    float    plane_eps;       /* ... and |N_p . (P_q - P_p)| <= this (world units) */
    uint32_t reserved_[5];    /* ignored */
} rtsh_wide_filter_params;                                                         /* 32 bytes */
/* 2 * count * W * H * sizeof(uint16_t): the bytes of d_scratch; 0 where count is outside 1 .. 8 or W or H is 0. */
size_t rtsh_wide_filter_scratch_bytes(uint32_t count, uint32_t W, uint32_t H);
int rtsh_wide_filter_light_list(const rts_light_list* list, const rtsh_wide_filter_params* params, const float* positions,
                                const float* normals, const uint8_t* lights_map, const uint8_t* mask, uint32_t W, uint32_t H,
                                float* visibility, int threads);
int rtsh_wide_filter_soft_light_list(const rts_soft_light_list* list, const rtsh_wide_filter_params* params, const float* positions,
                                     const float* normals, const uint8_t* lights_map, const uint8_t* counts, uint32_t W, uint32_t H,
                                     float* visibility, int threads);
int rtsh_wide_filter_light_list_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_wide_filter_params* params,
                                       const float* d_positions, const float* d_normals, const uint8_t* d_lights_map, const uint8_t* d_mask,
                                       uint32_t W, uint32_t H, float* d_visibility, uint16_t* d_scratch, void* stream);
int rtsh_wide_filter_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_wide_filter_params* params,
                                            const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                            const uint8_t* d_counts, uint32_t W, uint32_t H, float* d_visibility, uint16_t* d_scratch,
                                            void* stream);

/* THE WIDE FILTER OF THE BENT PLANE: the a-trous filter above over rts_trace_ambient_occlusion_bent*'s plane -- W x H
 * RGBA32F, (frame * sum of free directions, count) per pixel --, so that the direction an ambient term is aimed by is as smooth as the
 * AO term beside it.  The world-space vector is QUANTISED ONCE, to 16-bit signed integers, and from there every sum across pixels is an
 * INTEGER sum: the rule above with signed values, and as order-free.  One geometry test and one byte decide a tap for all four
 * channels.  Inputs: rtsh_wide_filter_params (unchanged); nsamples, n = max(1, nsamples) <= RTS_AO_MAX_SAMPLES (the trace's sample
 * count: |bent.xyz| <= n up to rounding, bent.w = the count); positions, normals; `active`, W x H bytes or NULL; `bent`, any float allowed.
 *   ACTIVE: a pixel is active when it is not bg(p) and (active == NULL or active[p] != 0).  bg, geom(p, q), the 25 taps, the weights
 *     b = {6, 4, 1} and the in-frame rule are the wide filter's above, word for word.  A tap is accepted when it is the centre, or when
 *     geom(p, q) holds and q is active.  An INACTIVE pixel carries four zeros in every pass and is never accepted.
 *   INPUT: S_b = 32767 / n, S_l = 65535 / n, both by integer division.  Per component c of xyz: t = bent.c * (float)S_b, ONE rounded
 *     multiply, no contraction; a NaN gives 0; clamp to [-(n * S_b), n * S_b]; X_0.c = (int32) rint(t), ties to even: it fits int16.
 *     For .w: a NaN gives 0; clamp to [0, n]; rint; V_0 = that * S_l -- uint16, the wide filter's V_0 of the count.
 *   PASS k (step 1 << k): den = sum of w over the accepted taps; per signed component num = sum of w * X_k.c (|num| <= 32767 * 256 <
 *     2^23) and X_(k+1).c = sign(num) * ((2 * |num| + den) / (2 * den)) by integer division: the ROUNDED MEAN, HALF AWAY FROM ZERO, so
 *     that negating the input negates the output.  The .w channel is the wide filter's pass unchanged.
 *   OUTPUT (formed by the last pass; from X_0 when passes == 0): out[p].c = (float)X.c / (float)(n * S_b), one correctly rounded
 *     division, a zero numerator gives +0;  out[p].w = (float)V / (float)(n * S_l);  ao[p], when given, holds out[p].w's bits.  An
 *     inactive pixel gets four +0 (and ao[p] = +0).  So out.xyz is the mean free direction PER SAMPLE, inside [-1, 1], out.w the AO
 *     visibility in [0, 1], and |xyz| / w keeps the trace's measure of how narrow the open cone is.
 * ANCHORS: (1) out.w and ao equal, bit for bit, rtsh_wide_filter_soft_light_list*'s plane of the bent trace's own `counts` under a
 * one-entry soft list of n samples, the same parameters and a map of 0 / 1 bytes, for every passes.  (2) Negating every bent.xyz negates
 * every out.xyz exactly (a zero stays +0: the division gives it).  (3) RANGE: every X_(k+1).c lies between the smallest and the largest
 * accepted X_k.c.  (4) Thresholds that accept no neighbour give the passes == 0 plane at any passes.  (5) Equal accepted texels give
 * that texel.  (6) rtsh_combine_visibility_list_ao_bent* over (ao, out) with passes == 0 gives the h of the raw plane wherever the raw
 * vector quantises exactly; NOT BIT-EQUAL IN GENERAL: the direction is rounded to 1 / (n S_b).
 *   * out: W x H RGBA32F, required; ao: W x H floats or NULL.  Host form: multi-threaded (threads: 0 = all host threads), allocates
 *     its own intermediates.
 *   * device form: DEVICE buffers, asynchronous on `stream`, allocates nothing and reads nothing back.  d_scratch:
 *     rtsh_wide_filter_bent_scratch_bytes(W, H) = 2 * W * H * 8 bytes, ALIGNED TO 8 BYTES: two ping-pong planes of one 8-byte texel per
 *     pixel (int16 x, y, z and uint16 V; the second begins W * H texels in); NULL allowed when passes <= 1, nothing of it is touched
 *     then, and passes == 2 leaves its second half untouched.  d_bent and d_out are ALIGNED TO 16 BYTES (they are read and written as
 *     whole texels).  Under graph capture a call adds exactly max(1, passes) KERNEL nodes on one chain, parameters by value.  No BVH.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: everything the wide filter above refuses of its parameters and sizes;
 *     NULL positions, normals, bent or out; nsamples > RTS_AO_MAX_SAMPLES; in the device form a NULL ctx, H above 16 * 65535, a NULL
 *     d_scratch with passes >= 2, d_out or d_ao equal to d_bent, to d_scratch or to its second half, a d_bent or d_out that is not
 *     aligned to 16 bytes, a d_scratch not aligned to 8.
 *   * OUT OF SCOPE: ~~temporal accumulation of the bent plane~~ (rtsh_accumulate_bent* and rtsh_wide_filter_bent_mean* below, DESIGN.md
 *     4.39), variance guidance, a bent form of the adaptive or distance traces, stripes and row ranges. */
size_t rtsh_wide_filter_bent_scratch_bytes(uint32_t W, uint32_t H);   /* 2 * W * H * 8; 0 where W or H is 0 */
int rtsh_wide_filter_bent(const rtsh_wide_filter_params* params, uint32_t nsamples, const float* positions, const float* normals,
                          const uint8_t* active, const float* bent, uint32_t W, uint32_t H, float* out, float* ao, int threads);
int rtsh_wide_filter_bent_device(rts_ctx* ctx, const rtsh_wide_filter_params* params, uint32_t nsamples, const float* d_positions,
                                 const float* d_normals, const uint8_t* d_active, const float* d_bent, uint32_t W, uint32_t H, float* d_out,
                                 float* d_ao, void* d_scratch, void* stream);

/* THE TEMPORAL ACCUMULATION OF THE BENT TEXEL: the wide bent filter's 8-byte texel over reprojected frames, in FIXED
 * POINT -- what rtsh_accumulate_moments_soft_light_list* (further down) does for a count plane, for the vector that aims the sky tint.  A
 * spatial filter cannot remove an error every pixel of a surface shares (a trace without a direction table); different directions on
 * different frames, averaged at the same surface point, can: the caller varies rts_ao_params.dirs per frame, no frame term is added to the
 * trace.  The current value is an integer and the bilinear weights are integers, so every sum is an integer sum: THE RESULT DOES NOT
 * DEPEND ON THE ORDER OF THE TAPS, and the host form checks the device form bit for bit.
 *   THE TEXEL, owned by the caller from here on: 8 bytes, int16 x, y, z then uint16 V, lowest bits first (little endian: a uint64_t
 *     whose bits 0..15 are x, 16..31 y, 32..47 z, 48..63 V).  x, y, z: the bent vector in units of 1 / S_b, S_b = 32767 / n; V: the count
 *     in units of 1 / S_l, S_l = 65535 / n; both by integer division -- the wide bent filter's fixed point above.
 *   CURRENT frame: params (rtsh_temporal_params, the struct and the meaning of rtsh_accumulate_visibility_list); nsamples, n = max(1,
 *     nsamples) <= RTS_AO_MAX_SAMPLES; positions, normals; `active`, W x H bytes or NULL: a pixel is ACTIVE when it is not bg(p) and
 *     (active == NULL or active[p] != 0), the wide bent filter's rule; `bent`: the trace's W x H RGBA32F plane, any float allowed.
 *   PREVIOUS frame: prev_positions, prev_normals, prev_texels (W x H texels), prev_lengths (W x H bytes).  All four NULL: the FIRST
 *     FRAME; all four or none.  Any 8 bytes are legal in the history, components 0x8000 and a V above n * S_l included.
 *   Outputs: texels_out (W x H texels), lengths_out (W x H bytes).
 *   CURRENT VALUE: X_0 and V_0 are the wide bent filter's INPUT rule exactly: per component one rounded multiply by S_b, a NaN gives 0,
 *     the clamp to +-(n * S_b), rint; .w: a NaN gives 0, the clamp to [0, n], rint, times S_l.
 *   GEOMETRY: INACTIVE (above), REPROJECT, the four taps in their order, their integer weights and the acceptance of a tap are
 *     rtsh_accumulate_visibility_list's, word for word, with ONE plane: prev_lengths[q] != 0 stands in for the per-light length, bit 0 of
 *     reset_lights is the reset.  An inactive pixel gets an all-zero texel and length 0.
 *   PASS-THROUGH: on the first frame, with the reset bit, off screen, with no accepted tap, or with n_f == 1: pack(X_0, V_0), length 1.
 *   BLEND: sw = the sum of the accepted weights, m = the smallest accepted length, n_f = min(m + 1, max_length), lengths_out = n_f;
 *     den = n_f * sw < 2^18.  Per signed component c: s = the integer sum of w * X'(q).c over the accepted taps (|s| <= 2^25),
 *     num = (n_f - 1) * s + sw * X_0.c (|num| < 2^34), out.c = sign(num) * ((2 * |num| + den) / (2 * den)) by integer division: the
 *     ROUNDED MEAN, HALF AWAY FROM ZERO, so that the pass commutes with negation.  V: the moments pass's mean rule unchanged,
 *     (2 * ((n_f - 1) * s + sw * V_0) + den) / (2 * den).  Everything fits 64 bits.
 * ANCHORS: (1) lengths_out and the V channel equal, byte for byte, lengths_out and mean_out of rtsh_accumulate_moments_soft_light_list*
 * over the trace's own `counts` under a one-entry soft list of n samples, a map of 0 / 1 bytes made from `active`, the same reset bit
 * and a history whose V channel is that prev_mean.  (2) Negating every bent.xyz and every history x, y, z negates every output x, y, z
 * (no history component being -32768, which has no negative).  (3) A still camera (one tap of weight 1024) gives, per component,
 * h_k = sign * ((2 * |(n_f - 1) * h_(k-1) + cur| + n_f) / (2 * n_f)).  (4) max_length == 1, the reset bit and the first frame give
 * pack(X_0, V_0) and length 1 at active pixels.  (5) RANGE: every output component lies between the smallest and the largest of its
 * accepted history values and the current one; so the output stays inside int16 / uint16.  (6) Equal accepted values give that value.
 *   * motion forms: prev_points and prev_point_normals of this frame's motion G-buffer pass; REPROJECT and TAP ACCEPTANCE change as in
 *     rtsh_accumulate_visibility_list_motion, word for word (Q = prev_points[p], the taps are tested with M_p = prev_point_normals[p], a
 *     background M_p accepts no tap).
 *   * host forms: multi-threaded (threads: 0 = all host threads).  Device forms: DEVICE buffers, asynchronous on `stream`, allocate
 *     nothing, read nothing back; under graph capture ONE kernel node, params by value.  No BVH.  d_bent is ALIGNED TO 16 BYTES, both
 *     texel planes TO 8 (they are read and written whole).
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: what rtsh_accumulate_moments_soft_light_list* refuses of params, the frame
 *     and the buffers (bent in the place of counts, the texel planes in the place of the mean planes); nsamples > RTS_AO_MAX_SAMPLES;
 *     some but not all of the four prev_*; texels_out == prev_texels or lengths_out == prev_lengths (history must ping-pong); in the
 *     device forms a NULL ctx, a d_bent not aligned to 16 bytes, a texel plane not aligned to 8, H above 16 * 65535; in the motion forms,
 *     with a history, a NULL prev_points or prev_point_normals.
 *   * OUT OF SCOPE: a second moment or variance guidance for the vector, a history clamp for it, a frame term inside the trace's table
 *     hash, bent forms of the adaptive or distance traces, stripes and row ranges. */
int rtsh_accumulate_bent(const rtsh_temporal_params* params, uint32_t nsamples, const float* positions, const float* normals,
                         const uint8_t* active, const float* bent, const float* prev_positions, const float* prev_normals,
                         const void* prev_texels, const uint8_t* prev_lengths, uint32_t W, uint32_t H, void* texels_out,
                         uint8_t* lengths_out, int threads);
int rtsh_accumulate_bent_device(rts_ctx* ctx, const rtsh_temporal_params* params, uint32_t nsamples, const float* d_positions,
                                const float* d_normals, const uint8_t* d_active, const float* d_bent, const float* d_prev_positions,
                                const float* d_prev_normals, const void* d_prev_texels, const uint8_t* d_prev_lengths, uint32_t W,
                                uint32_t H, void* d_texels_out, uint8_t* d_lengths_out, void* stream);
int rtsh_accumulate_bent_motion(const rtsh_temporal_params* params, uint32_t nsamples, const float* positions, const float* normals,
                                const uint8_t* active, const float* bent, const float* prev_positions, const float* prev_normals,
                                const void* prev_texels, const uint8_t* prev_lengths, const float* prev_points,
                                const float* prev_point_normals, uint32_t W, uint32_t H, void* texels_out, uint8_t* lengths_out,
                                int threads);
int rtsh_accumulate_bent_motion_device(rts_ctx* ctx, const rtsh_temporal_params* params, uint32_t nsamples, const float* d_positions,
                                       const float* d_normals, const uint8_t* d_active, const float* d_bent,
                                       const float* d_prev_positions, const float* d_prev_normals, const void* d_prev_texels,
                                       const uint8_t* d_prev_lengths, const float* d_prev_points, const float* d_prev_point_normals,
                                       uint32_t W, uint32_t H, void* d_texels_out, uint8_t* d_lengths_out, void* stream);

/* THE WIDE BENT FILTER FED FROM THE ACCUMULATED TEXEL: SVGF's order -- integrate over time, then filter.
 * rtsh_wide_filter_bent*'s rule word for word with ONE change, of INPUT: at an active pixel X_0'.c = clamp(texel.c, -(n * S_b), n * S_b)
 * and V_0' = min(texel.V, n * S_l), read from the 8-byte plane `texels` (rtsh_accumulate_bent*'s output for THIS frame) at active pixels
 * only.  The CLAMP is this form's own: the accumulate never writes more (its RANGE anchor), but any 8 bytes are allowed and out.xyz must
 * stay in [-1, 1], out.w in [0, 1].  The argument list is the parent's with `const void* texels` in the place of bent; the scratch
 * (rtsh_wide_filter_bent_scratch_bytes), the refusals and the max(1, passes) kernel nodes are unchanged; only the first kernel differs.
 * ANCHORS: (1) over the texels of a first-frame accumulate, out and ao are bit for bit rtsh_wide_filter_bent*'s of the float plane, for
 * every passes.  (2) passes == 0 gives the two quotients of the clamped texel.  (3) The parent's negation, range, closed-threshold and
 * equal-texel anchors hold.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: everything the parent refuses (texels in the place of bent); in the device
 *     form a d_texels not aligned to 8 bytes, or equal to d_out, d_ao, d_scratch or its second half. */
int rtsh_wide_filter_bent_mean(const rtsh_wide_filter_params* params, uint32_t nsamples, const float* positions, const float* normals,
                               const uint8_t* active, const void* texels, uint32_t W, uint32_t H, float* out, float* ao, int threads);
int rtsh_wide_filter_bent_mean_device(rts_ctx* ctx, const rtsh_wide_filter_params* params, uint32_t nsamples, const float* d_positions,
                                      const float* d_normals, const uint8_t* d_active, const void* d_texels, uint32_t W, uint32_t H,
                                      float* d_out, float* d_ao, void* d_scratch, void* stream);

/* THE VARIANCE-GUIDED WIDE FILTER OF A SOFT LIGHT LIST'S PLANES: rtsh_wide_filter_soft_light_list above with SVGF's luminance stop, so
 * that the passes blur noise and stop at a sharp shadow edge.  A tap is accepted for a light only if its value lies within a tolerance
 * T of the centre's, and T comes from the count plane itself: a pixel with c of n samples unoccluded has a Bernoulli variance
 * proportional to c * (n - c) -- an integer, a function of the inputs alone, no history.  Where the samples of a neighbourhood are
 * unanimous T is 0 and the edge stays; where they disagree the filter blurs.  Everything of the unguided filter holds (16-bit planes,
 * integer sums, bit-for-bit host and device forms); the notation -- n_l, S_l, V_0, geom, on, bg, b = {6, 4, 1} -- is its own.
 *   typedef struct rtsh_wide_guide_params: passes, normal_cos_min, plane_eps as in rtsh_wide_filter_params; guide_k4: the tolerance k
 *     in QUARTER units, 0 .. 255 (k = 3 standard deviations is 12); reserved_ (ignored).
 *   ENERGY: E(q, l) = V_0(q, l) * (n_l * S_l - V_0(q, l)) = c (n - c) S^2, at most about 2^30.
 *   NEIGHBOURHOOD SUM, for an active pixel p and a light with n_l >= 2: over the 3 x 3 pixels q around p that are INSIDE THE FRAME, not
 *     bg(q), and have on(q, l), weights w = {1, 2, 1} x {1, 2, 1}:  G = sum of w * E(q, l),  D = sum of w (the centre always counts:
 *     D >= 4).  There is NO geom TEST here: the worst a pixel of a foreign surface can do is RAISE the tolerance; it never makes the
 *     filter cross a geometry edge -- the pass below still applies geom to every tap --, and leaving the test out keeps the sum to
 *     nine integer loads.
 *   THRESHOLD: T(p, l) = min(65535, isqrt((guide_k4^2 * G) / (16 * D * n_l))), the division an integer division, isqrt the exact
 *     integer square root; everything fits unsigned 64 bits (guide_k4^2 < 2^16, G < 2^35).  It is k * S_l * sqrt(mean of c (n - c) / n)
 *     rounded down.  For n_l <= 1 (a hard light inside a soft list) the estimate carries no information: T = 65535, and that light is
 *     filtered exactly as the unguided filter does.
 *   PASS k: the unguided filter's pass with one change: a tap other than the centre is accepted for light l when geom(p, q) and
 *     on(q, l) hold AND |V_k(q, l) - V_k(p, l)| <= T(p, l).  Acceptance, num and den are per light; the rounded mean
 *     (2 * num + den) / (2 * den) and the final quotient are unchanged.  T comes from V_0 and is THE SAME AT EVERY PASS.
 * There is NO guided form for a hard list: its c (1 - c) is 0 everywhere.
 * ANCHORS: (1) guide_k4 == 0 gives the passes == 0 plane bit for bit whatever passes is: with T = 0 only equal values are accepted, and
 * the rounded mean of equal values is that value.  (2) Plane l of a light with n_l <= 1 is bit for bit the plane of
 * rtsh_wide_filter_soft_light_list for the same inputs.  (3) A pixel whose 3 x 3 neighbourhood is unanimous for light l -- every
 * counted c is 0 or n_l -- keeps its own quotient through every pass.  (4) RANGE: every V_(k+1)(p) lies between the smallest and the
 * largest accepted V_k.  (5) passes == 0 is the unguided conversion, (float)min(c, n_l) / (float)n_l.
 *   * buffers, lights_map, threads, stream and graph capture as for rtsh_wide_filter_soft_light_list*: a device call adds exactly
 *     max(1, passes) KERNEL nodes on one chain, list and parameters by value.  The FIRST pass computes T; for passes >= 2 it writes T to
 *     a THIRD set of count planes of d_scratch, of which later passes read one uint16_t per pixel and light.
 *   * d_scratch: 3 * count * W * H uint16_t (rtsh_wide_filter_guided_scratch_bytes): the two ping-pong sets, then the planes of T; it
 *     may be NULL when passes <= 1, and nothing of it is touched then.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: everything rtsh_wide_filter_soft_light_list* refuse (d_visibility equal
 *     to the start of any of the three sets of d_scratch included); guide_k4 > 255; a NULL d_scratch with passes >= 2.
 *   * OUT OF SCOPE: ~~variance propagated through the passes~~ (T is the first pass's at every pass HERE; propagated:
 *     rtsh_wide_filter_propagated_mean_soft_light_list below), a guide for the tent filter
 *     rtsh_filter_*_light_list*.  (A temporal variance from accumulated moments: rtsh_wide_filter_guided_temporal_soft_light_list
 *     below.) */
enum { RTSH_WIDE_GUIDE_MAX_K4 = 255 };
typedef struct rtsh_wide_guide_params {
    uint32_t passes;          /* 0 .. RTSH_WIDE_FILTER_MAX_PASSES (5) */
    float    normal_cos_min;  /* a tap needs N_p . N_q >= this */
    float    plane_eps;       /* ... and |N_p . (P_q - P_p)| <= this (world units) */
    uint32_t guide_k4;        /* the tolerance in quarter standard deviations, 0 .. RTSH_WIDE_GUIDE_MAX_K4 (255) */
    uint32_t reserved_[4];    /* ignored */
} rtsh_wide_guide_params;                                                          /* 32 bytes */
/* 3 * count * W * H * sizeof(uint16_t): the bytes of d_scratch; 0 where count is outside 1 .. 8 or W or H is 0. */
size_t rtsh_wide_filter_guided_scratch_bytes(uint32_t count, uint32_t W, uint32_t H);
/* T of the rule above from its parts (G < 2^35, 4 <= D <= 16, 2 <= n <= 48, guide_k4 <= 255): what host twin and kernels evaluate. */
uint32_t rtsh_wide_guide_threshold(uint64_t G, uint32_t D, uint32_t n, uint32_t guide_k4);
int rtsh_wide_filter_guided_soft_light_list(const rts_soft_light_list* list, const rtsh_wide_guide_params* params, const float* positions,
                                            const float* normals, const uint8_t* lights_map, const uint8_t* counts, uint32_t W,
                                            uint32_t H, float* visibility, int threads);
int rtsh_wide_filter_guided_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_wide_guide_params* params,
                                                   const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                   const uint8_t* d_counts, uint32_t W, uint32_t H, float* d_visibility,
                                                   uint16_t* d_scratch, void* stream);

/* THE TEMPORAL ACCUMULATION OF A SOFT LIGHT LIST'S COUNT MOMENTS: the first and second moment of V_0 = min(c, n_l) * S_l -- the wide
 * filter's own 16-bit input, its notation -- over reprojected frames, in FIXED POINT.  It is what SVGF drives its luminance stop with:
 * rtsh_wide_filter_guided_temporal_soft_light_list below takes its tolerance from these planes where a pixel's history is long enough.
 * Counts are integers and the bilinear weights of rtsh_accumulate_visibility_list are integers, so every sum here is an integer sum:
 * THE RESULT DOES NOT DEPEND ON THE ORDER OF THE TAPS, and the host form checks the device form bit for bit.
 *   CURRENT frame: positions, normals, lights_map (may be NULL), counts (count uint8_t planes).
 *   PREVIOUS frame: prev_positions, prev_normals, prev_mean (count uint16_t planes), prev_square (count uint32_t planes), prev_lengths
 *     (count uint8_t planes).  All five NULL: the FIRST FRAME; all five or none.
 *   Outputs: mean_out (uint16_t), square_out (uint32_t), lengths_out (uint8_t), count planes each.
 *   params: rtsh_temporal_params, the struct and the meaning of rtsh_accumulate_visibility_list, max_length and reset_lights included.
 * For pixel p and light l < count:  cur1 = V_0(p, l) (at most 65535), cur2 = cur1 * cur1 (below 2^32).
 *   GEOMETRY: INACTIVE, REPROJECT, the four taps, their integer weights and the acceptance of a tap are rtsh_accumulate_visibility_list's,
 *     word for word (prev_lengths in the place of its prev_lengths).  An inactive (pixel, light) holds 0, 0 and length 0.
 *   PASS-THROUGH: on the first frame, off screen, with no accepted tap, or with n == 1: cur1, cur2 and length 1.
 *   BLEND: sw = the sum of the accepted weights, m = the smallest accepted length, n = min(m + 1, max_length), lengths_out = n; for X in
 *     {mean, square}: s = the integer sum of w * prev_X[l][q] over the accepted taps, num = (n - 1) * s + sw * cur_X, den = n * sw,
 *     out_X = (2 * num + den) / (2 * den) by integer division: ONE rounded mean in place of the float pass's two steps.
 *   WIDTH: s < 2^42, 2 * num + den < 2^52, 2 * den < 2^19: everything fits unsigned 64 bits (and a double, exactly).
 * ANCHORS: (1) lengths_out is byte for byte what rtsh_accumulate_visibility_list writes for the same G-buffers, params, map and
 * prev_lengths.  (2) A still camera (anchor 2 there: one tap of weight 1024) gives h_k = (2 * ((n - 1) * h_(k-1) + cur) + n) / (2 * n),
 * n = min(k, max_length), per pixel and moment.  (3) Where every accepted history value and the current one are the same value, the
 * output is that value, for any weights; so a pixel whose count never changed has square == mean * mean exactly.  (4) max_length == 1,
 * an all-ones reset_lights and the first frame give cur1, cur2 and 1 at active pixels.  (5) RANGE: every output lies between the
 * smallest and the largest of its accepted history values and the current one.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: what rtsh_accumulate_visibility_list refuses (of params, the frame and the
 *     buffers, counts in the place of visibility); what rtsh_wide_filter_soft_light_list refuses of a soft list; some but not all of the
 *     five prev_*; mean_out == prev_mean, square_out == prev_square or lengths_out == prev_lengths (history must ping-pong); a NULL ctx.
 *   * planes of any buffer from `count` up are never touched.  No buffer needs alignment beyond its element type's.
 *   * host form: multi-threaded.  Device form: DEVICE buffers, asynchronous on `stream`, allocates nothing, reads nothing back; under
 *     graph capture ONE kernel node, list and params by value.  No BVH.
 *   * OUT OF SCOPE: (moving geometry: the motion form at the end of this header;) (a clamp of the moments' history: the clamped forms at
 *     the end of this header, DESIGN.md 4.30;) hard lists (their variance is 0), row ranges and stripes. */
int rtsh_accumulate_moments_soft_light_list(const rts_soft_light_list* list, const rtsh_temporal_params* params, const float* positions,
                                            const float* normals, const uint8_t* lights_map, const uint8_t* counts,
                                            const float* prev_positions, const float* prev_normals, const uint16_t* prev_mean,
                                            const uint32_t* prev_square, const uint8_t* prev_lengths, uint32_t W, uint32_t H,
                                            uint16_t* mean_out, uint32_t* square_out, uint8_t* lengths_out, int threads);
int rtsh_accumulate_moments_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_temporal_params* params,
                                                   const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                   const uint8_t* d_counts, const float* d_prev_positions, const float* d_prev_normals,
                                                   const uint16_t* d_prev_mean, const uint32_t* d_prev_square,
                                                   const uint8_t* d_prev_lengths, uint32_t W, uint32_t H, uint16_t* d_mean_out,
                                                   uint32_t* d_square_out, uint8_t* d_lengths_out, void* stream);

/* THE GUIDED WIDE FILTER WITH A TEMPORAL THRESHOLD: rtsh_wide_filter_guided_soft_light_list with ONE change, in ENERGY -- where a pixel's
 * moments (the planes above, for THIS frame) have a history of at least min_history frames, its energy is the variance seen over those
 * frames, not the one frame's Bernoulli estimate.  Under a jittered trace of few samples whole 3 x 3 neighbourhoods hold only 0 or n_l:
 * the spatial estimate is 0 there and the guided filter keeps the noise; the temporal one sees the pixel change from frame to frame.
 *   typedef struct rtsh_wide_guide_temporal_params: passes, normal_cos_min, plane_eps, guide_k4 as in rtsh_wide_guide_params;
 *     min_history 1 .. 255; reserved_ (ignored).
 *   ENERGY: E*(q, l) = n_l * max(0, square[l][q] - mean[l][q]^2) where lengths[l][q] >= min_history, else E(q, l) of the guided filter.
 *     (n_l times the variance of V is in the units of E: E / n_l is the binomial variance of V.)  Arbitrary plane contents are allowed:
 *     E* < 48 * 2^32, so G < 2^42 and guide_k4^2 * G < 2^58, inside 64 bits; rtsh_wide_guide_threshold is exact for such G too (its
 *     integer fix-up multiplies r * r * d < 2^46).
 *   G, D and the 3 x 3 weights, T = min(65535, isqrt((guide_k4^2 * G) / (16 * D * n_l))), T = 65535 for n_l <= 1, the pass, the rounded
 *     mean and the output are the guided filter's, unchanged.
 * ANCHORS: (1) where every counted lengths value is below min_history the result is bit for bit the guided filter's for the same inputs.
 * (2) From first-frame moments (square == mean^2, length 1) with min_history == 1 every T is 0: the passes == 0 plane for every light
 * with n_l >= 2.  (3) guide_k4 == 0 gives the passes == 0 plane.  (4) A light with n_l <= 1 gives rtsh_wide_filter_soft_light_list's
 * plane.  (5) RANGE as in the guided filter.
 *   * buffers, scratch (rtsh_wide_filter_guided_scratch_bytes), threads, stream and graph capture as for the guided filter: max(1, passes)
 *     KERNEL nodes on one chain; only the first differs from the guided filter's.  mean, square, lengths: count planes each, read at
 *     counted pixels only, each on its element type's alignment.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: everything the guided filter refuses; a NULL mean, square or lengths;
 *     min_history 0 or above 255.
 *   * OUT OF SCOPE: ~~variance propagated through the passes~~ (rtsh_wide_filter_propagated_mean_soft_light_list below, DESIGN.md
 *     4.31), a guide for the tent filter, row ranges and stripes, hard
 *     lists.  (Filtering the accumulated mean plane in place of this frame's counts: rtsh_wide_filter_mean_soft_light_list and
 *     rtsh_wide_filter_guided_temporal_mean_soft_light_list below.) */
typedef struct rtsh_wide_guide_temporal_params {
    uint32_t passes;          /* 0 .. RTSH_WIDE_FILTER_MAX_PASSES (5) */
    float    normal_cos_min;  /* a tap needs N_p . N_q >= this */
    float    plane_eps;       /* ... and |N_p . (P_q - P_p)| <= this (world units) */
    uint32_t guide_k4;        /* the tolerance in quarter standard deviations, 0 .. RTSH_WIDE_GUIDE_MAX_K4 (255) */
    uint32_t min_history;     /* 1 .. 255: a pixel of at least this many frames of history gives its temporal variance */
    uint32_t reserved_[3];    /* ignored */
} rtsh_wide_guide_temporal_params;                                                 /* 32 bytes */
int rtsh_wide_filter_guided_temporal_soft_light_list(const rts_soft_light_list* list, const rtsh_wide_guide_temporal_params* params,
                                                     const float* positions, const float* normals, const uint8_t* lights_map,
                                                     const uint8_t* counts, const uint16_t* mean, const uint32_t* square,
                                                     const uint8_t* lengths, uint32_t W, uint32_t H, float* visibility, int threads);
int rtsh_wide_filter_guided_temporal_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                            const rtsh_wide_guide_temporal_params* params, const float* d_positions,
                                                            const float* d_normals, const uint8_t* d_lights_map, const uint8_t* d_counts,
                                                            const uint16_t* d_mean, const uint32_t* d_square, const uint8_t* d_lengths,
                                                            uint32_t W, uint32_t H, float* d_visibility, uint16_t* d_scratch, void* stream);

/* THE WIDE FILTERS FED FROM THE ACCUMULATED MEAN: SVGF's order -- integrate over time first, then run the a-trous passes over the
 * integrated signal.  rtsh_accumulate_moments_soft_light_list* above writes, per light, a uint16_t `mean` plane in the wide filter's own
 * fixed point; the two families here run the wide filter and the temporally guided wide filter over THAT plane in the place of this
 * frame's count bytes.  Everything of those filters holds (16-bit planes, integer sums, bit-for-bit host and device forms); the notation
 * -- n_l, S_l, on, bg, geom, b = {6, 4, 1}, V_0 -- is the wide filter's.
 *   INPUT: V_0'(q, l) = min(mean[l][q], n_l * S_l) at an active (pixel, light), 0 elsewhere.  mean: count planes of uint16_t, the
 *     moments pass's output for THIS frame.  The CLAMP is this family's own: the moments pass never writes more than n_l * S_l (its
 *     RANGE anchor), but arbitrary plane contents are allowed and visibility must stay in [0, 1] (65535 > n_l * S_l for n_l = 48: 65520).
 *     mean is read only where on(q, l) holds and q is not background.
 * rtsh_wide_filter_mean_soft_light_list*: THE UNGUIDED FILTER.  rtsh_wide_filter_soft_light_list's rule word for word with V_0' in the
 *   place of V_0: PASS k over the 5 x 5 taps 1 << k apart, integer weights b[|dx|] * b[|dy|], the centre always accepted, another tap
 *   where geom(p, q) and on(q, l) hold, V_(k+1) = (2 * num + den) / (2 * den), the ROUNDED MEAN; OUTPUT
 *   visibility[l * W * H + p] = (float)V_passes / (float)(n_l * S_l), +0.0f at an inactive pixel.  The argument list is that
 *   function's with `const uint16_t* mean` in the place of counts; rtsh_wide_filter_params, the scratch
 *   (rtsh_wide_filter_scratch_bytes: two ping-pong sets) and the refusals are unchanged.
 * rtsh_wide_filter_guided_temporal_mean_soft_light_list*: THE GUIDED FILTER.  rtsh_wide_filter_guided_temporal_soft_light_list's rule
 *   with the same ONE change of input; its argument list, rtsh_wide_guide_temporal_params and the three scratch sets
 *   (rtsh_wide_filter_guided_scratch_bytes).  ENERGY E*, G, D and T are exactly that filter's:
 *     E*(q, l) = n_l * max(0, square[l][q] - mean[l][q]^2), from the UNCLAMPED planes, where lengths[l][q] >= min_history;
 *     E*(q, l) = V_0(q, l) * (n_l * S_l - V_0(q, l)) = c (n - c) S^2 from THIS frame's count byte elsewhere -- which is why counts stays
 *     in the argument list; a count byte is read only at a counted pixel whose length is below min_history;
 *     G, D over the 3 x 3 with weights {1, 2, 1} x {1, 2, 1}, no geom test; T = min(65535, isqrt((guide_k4^2 * G) / (16 * D * n_l))),
 *     65535 for n_l <= 1.  Only the values that the passes AVERAGE and COMPARE against T are V_0' (and the planes that follow from it):
 *     a tap other than the centre is accepted for light l when geom(p, q) and on(q, l) hold and |V_k(q, l) - V_k(p, l)| <= T(p, l).
 *     T DOES NOT SHRINK WITH THE HISTORY'S LENGTH: it is the spread of one frame's V_0 about the mean, while the mean of m frames
 *     scatters by about 1 / sqrt(m) of that -- so at equal guide_k4 this form accepts more than the count-input form.  Dividing the
 *     variance by the length is out of scope HERE (below): by_length of rtsh_wide_filter_propagated_mean_soft_light_list does it.
 * ANCHORS: (1) Where mean[l][q] == min(c_l(q), n_l) * S_l at every active (pixel, light), both functions give bit for bit the planes of
 * their count-input counterparts (rtsh_wide_filter_soft_light_list*, rtsh_wide_filter_guided_temporal_soft_light_list*) for the same
 * inputs: first-frame moments are such a case, so is max_length 1.  (2) passes == 0 gives (float)min(mean, n S) / (float)(n S).
 * (3) Where every accepted tap of every pass carries one value, the result is that value's quotient.  (4) RANGE: every V_(k+1)(p) lies
 * between the smallest and the largest accepted V_k, and visibility stays in [0, 1] whatever the mean plane holds.  (5) The guided
 * form: guide_k4 == 0 gives the passes == 0 plane of every light with n_l >= 2; a light with n_l <= 1 gives rtsh_wide_filter_mean_soft_light_list's plane; every
 * counted length below min_history together with anchor 1's condition gives rtsh_wide_filter_guided_soft_light_list's bits.
 *   * lights_map may be NULL.  mean needs 2-byte alignment and no more, square 4, every byte plane none.  Planes of any buffer from
 *     `count` up are never touched.  Host forms: multi-threaded, they allocate their own intermediates.
 *   * device forms: DEVICE buffers, asynchronous on `stream`, allocate nothing, read nothing back.  Under graph capture a call adds
 *     exactly max(1, passes) KERNEL nodes on one chain, list and parameters by value; only the FIRST differs from the counterpart's.
 *     d_scratch may be NULL when passes <= 1, and nothing of it is touched then; in the guided form the first pass writes T to the
 *     third set for passes >= 2.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: everything the counterpart refuses, with mean in the place of counts;
 *     a NULL mean; d_visibility equal to the start of any scratch set (two for the unguided form, three for the guided one).
 *   * OUT OF SCOPE: ~~variance divided by the history's length or propagated through the passes~~ (both:
 *     rtsh_wide_filter_propagated_mean_soft_light_list below), (a clamp of the moments' history: the
 *     clamped forms at the end of this header,) motion vectors, the tent filter, hard lists, row ranges and stripes, an LDS-staged form of the moments, and feeding the float visibility
 *     history of rtsh_accumulate_visibility_list to the a-trous passes (it is not fixed point). */
int rtsh_wide_filter_mean_soft_light_list(const rts_soft_light_list* list, const rtsh_wide_filter_params* params, const float* positions,
                                          const float* normals, const uint8_t* lights_map, const uint16_t* mean, uint32_t W, uint32_t H,
                                          float* visibility, int threads);
int rtsh_wide_filter_mean_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_wide_filter_params* params,
                                                 const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                 const uint16_t* d_mean, uint32_t W, uint32_t H, float* d_visibility, uint16_t* d_scratch,
                                                 void* stream);
int rtsh_wide_filter_guided_temporal_mean_soft_light_list(const rts_soft_light_list* list, const rtsh_wide_guide_temporal_params* params,
                                                          const float* positions, const float* normals, const uint8_t* lights_map,
                                                          const uint8_t* counts, const uint16_t* mean, const uint32_t* square,
                                                          const uint8_t* lengths, uint32_t W, uint32_t H, float* visibility, int threads);
int rtsh_wide_filter_guided_temporal_mean_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                                 const rtsh_wide_guide_temporal_params* params, const float* d_positions,
                                                                 const float* d_normals, const uint8_t* d_lights_map,
                                                                 const uint8_t* d_counts, const uint16_t* d_mean, const uint32_t* d_square,
                                                                 const uint8_t* d_lengths, uint32_t W, uint32_t H, float* d_visibility,
                                                                 uint16_t* d_scratch, void* stream);

/* THE GUIDED MEAN FILTER WITH A PROPAGATED VARIANCE: rtsh_wide_filter_guided_temporal_mean_soft_light_list above with
 * SVGF's second half -- a per-pixel VARIANCE plane is filtered along with the signal, Var' = sum w^2 Var / (sum w)^2, and the edge stop
 * is re-derived from it at every pass, so the tolerance tightens as the signal gets cleaner.  Moments and tap weights are integers, so
 * this is exact: host and device forms agree bit for bit.  Notation as above: n_l, S_l, V_0' = min(mean, n_l * S_l), geom, on, bg,
 * b = {6, 4, 1}; "active pair" = a (pixel, light) with not bg(q) and on(q, l).
 *   typedef struct rtsh_wide_guide_propagated_params: passes, normal_cos_min, plane_eps, guide_k4, min_history as in
 *     rtsh_wide_guide_temporal_params; by_length 0 or 1; reserved_ (ignored).
 *   R: at an active pair with lengths[l][q] >= min_history, R(q, l) = max(0, square[l][q] - mean[l][q]^2), from the UNCLAMPED planes.
 *   Q_0(q, l), a uint32_t in V^2 units: R(q, l) where the history suffices -- R(q, l) / lengths[l][q] by integer division there if
 *     by_length is set --; (V_0 * (n_l * S_l - V_0)) / n_l by integer division elsewhere, V_0 = min(c, n_l) * S_l from THIS frame's
 *     count byte: the Bernoulli energy in the same units; 0 at an inactive pair.
 *   T_0(p, l): with by_length == 0 the guided mean filter's T word for word -- E* = n_l * R in the temporal branch, V_0 * (n_l * S_l - V_0)
 *     elsewhere, G and D over the 3 x 3 with weights {1, 2, 1} x {1, 2, 1}, no geom test,
 *     T = min(65535, isqrt((guide_k4^2 * G) / (16 * D * n_l))).  With by_length == 1 the same expression with E* = n_l * Q_0 in the
 *     temporal branch (the other branch keeps its E: n_l * Q_0 would round there).
 *   PASS k, k = 0 .. passes - 1, VALUES: the guided filter's pass with T_k: taps 1 << k apart, the centre always accepted, another tap
 *     where geom(p, q) and on(q, l) hold and |V_k(q, l) - V_k(p, l)| <= T_k(p, l); V_(k+1) = (2 * num + den) / (2 * den).
 *   PASS k, VARIANCE: over EXACTLY the taps accepted for light l, the centre included, w = b[|dx|] * b[|dy|]:
 *     numQ = sum of w^2 * Q_k(q, l), den = sum of w (the values' den), Q_(k+1)(p, l) = (2 * numQ + den^2) / (2 * den^2) by integer
 *     division; 0 at an inactive pair.  sum of w^2 <= 70^2, so numQ < 2^45; den^2 <= 2^16: rtsh_wide_variance_step evaluates it, the
 *     same source on host and device, without a 64-bit division.  The last pass writes no Q.
 *   T_k(p, l) for k >= 1, formed by pass k before its taps: over the 3 x 3 ADJACENT pixels q (one pixel apart whatever k is) that are
 *     inside the frame, not bg(q) and have on(q, l), weights {1, 2, 1} x {1, 2, 1}, no geom test, the centre always counts:
 *     G_k = sum of w * Q_k(q, l) < 2^36, D_k = sum of w, T_k = rtsh_wide_guide_threshold(G_k, D_k, 1, guide_k4) =
 *     min(65535, isqrt((guide_k4^2 * G_k) / (16 * D_k))): Q is the variance of V itself, so n_l leaves the divisor.  0 where l is not
 *     on at p.
 *   ONE-SAMPLE LIGHTS: n_l <= 1 gives T = 65535 at every pass; that light's Q is never read and is written as 0.
 *   OUTPUT: visibility[l * W * H + p] = (float)V_passes / (float)(n_l * S_l), formed by the last pass; passes == 0 converts V_0'.
 * ANCHORS: (1) passes <= 1 with by_length == 0 gives rtsh_wide_filter_guided_temporal_mean_soft_light_list's plane bit for bit.
 * (2) guide_k4 == 0 gives the passes == 0 plane of every light with n_l >= 2.  (3) A light with n_l <= 1 gives
 * rtsh_wide_filter_mean_soft_light_list's plane.  (4) RANGE: every V_(k+1)(p) lies between the smallest and the largest accepted V_k,
 * and visibility stays in [0, 1] whatever the planes hold.  (5) Q_(k+1)(p) is at most the largest accepted Q_k (sum w^2 <= (sum w)^2),
 * and a pixel that accepts only its centre keeps its Q exactly (1296 Q / 36^2).  (6) Where lengths >= min_history and
 * square == mean^2 hold at every active pair, every Q and every T is 0 and every pixel keeps its own quotient through every pass.
 * (7) by_length == 1 with every counted length equal to 1 gives the by_length == 0 bits.
 *   * argument lists: rtsh_wide_filter_guided_temporal_mean_soft_light_list*'s, with `void* d_scratch` in the device form.  Buffers,
 *     lights_map, alignment, threads, stream as there; planes from `count` up are never touched.
 *   * d_scratch: rtsh_wide_filter_propagated_scratch_bytes(count, W, H) = 12 * count * W * H bytes, aligned to 4: two ping-pong sets of
 *     count uint16_t planes, then -- 4 * count * W * H bytes in, a multiple of 4 -- two ping-pong sets of count uint32_t planes of Q.
 *     There is no plane of T: each pass recomputes T_k.  Pass k < passes - 1 writes V_(k+1) and Q_(k+1) to sets k & 1.  It may be NULL
 *     when passes <= 1, and nothing of it is touched then.
 *   * under graph capture a device call adds exactly max(1, passes) KERNEL nodes on one chain, list and parameters by value.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: everything the guided mean filter refuses; by_length > 1; a d_scratch that
 *     is not a multiple of 4; d_visibility equal to the start of any of the four sets of d_scratch.
 *   * OUT OF SCOPE: the count-input form (a caller without history passes first-frame moments: anchor 1 of the mean family), the tent
 *     filter, hard lists, row ranges and stripes, the effective sample count of an exponential history (lengths is capped at
 *     max_length, and by_length divides by that). */
typedef struct rtsh_wide_guide_propagated_params {
    uint32_t passes;          /* 0 .. RTSH_WIDE_FILTER_MAX_PASSES (5) */
    float    normal_cos_min;  /* a tap needs N_p . N_q >= this */
    float    plane_eps;       /* ... and |N_p . (P_q - P_p)| <= this (world units) */
    uint32_t guide_k4;        /* the tolerance in quarter standard deviations, 0 .. RTSH_WIDE_GUIDE_MAX_K4 (255) */
    uint32_t min_history;     /* 1 .. 255: a pixel of at least this many frames of history gives its temporal variance */
    uint32_t by_length;       /* 0, or 1: the temporal variance is divided by the history's length (the variance OF THE MEAN) */
    uint32_t reserved_[2];    /* ignored */
} rtsh_wide_guide_propagated_params;                                               /* 32 bytes */
/* 12 * count * W * H: the bytes of d_scratch; 0 where count is outside 1 .. 8 or W or H is 0. */
size_t rtsh_wide_filter_propagated_scratch_bytes(uint32_t count, uint32_t W, uint32_t H);
/* Q_(k+1) of the rule above from its parts (1 <= den <= 256, numQ <= den^2 * (2^32 - 1)); 0xFFFFFFFF outside that domain. */
uint32_t rtsh_wide_variance_step(uint64_t numQ, uint32_t den);
int rtsh_wide_filter_propagated_mean_soft_light_list(const rts_soft_light_list* list, const rtsh_wide_guide_propagated_params* params,
                                                     const float* positions, const float* normals, const uint8_t* lights_map,
                                                     const uint8_t* counts, const uint16_t* mean, const uint32_t* square,
                                                     const uint8_t* lengths, uint32_t W, uint32_t H, float* visibility, int threads);
int rtsh_wide_filter_propagated_mean_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                            const rtsh_wide_guide_propagated_params* params, const float* d_positions,
                                                            const float* d_normals, const uint8_t* d_lights_map, const uint8_t* d_counts,
                                                            const uint16_t* d_mean, const uint32_t* d_square, const uint8_t* d_lengths,
                                                            uint32_t W, uint32_t H, float* d_visibility, void* d_scratch, void* stream);

/* OBJ ingest.  rtsh_obj_load parses `path` and expands it to the reference's flat
 * Vertex stream: 8 floats per vertex (position.xyz, normal.xyz, texcoord.uv), indices[i] = i.
 * Call with vertices == NULL to query *vertex_count (3 per triangle) first.  Returns RTS_OK,
 * RTS_ERR_INVALID_ARG (cannot open / fails objValidate) or RTS_ERR_CAPACITY. */
int rtsh_obj_load(const char* path, float* vertices, size_t vertex_capacity, uint32_t* vertex_count,
                  float bbox_min[3], float bbox_max[3]);

/* The parser's number reader (objparser.cpp:62-131), exposed so tests can pin it. */
float rtsh_obj_parse_float(const char* text, int* consumed);

/* Host logic of rts_ctx_plan_splits, reachable without a device (tests): the order of a split table's front records for n tiles
 * {life_us[i], tiles[i] = bx | by << 16} with front_share 1 and no splits -- half-octave bands of life, longest first, image order
 * inside a band; life_block B > 1: a tile counts as long as the longest tile of its B x B block; xcd_square S > 0: inside a band,
 * record first_record + r is taken from the tiles of XCD ((first_record + r) mod 8)'s S x S squares while it has any (include/rts.h,
 * rts_split_plan).  order_out[r] = index of the tile that becomes record first_record + r. */
int rtsh_split_front_order(const float* life_us, const uint32_t* tiles, size_t n, uint32_t first_record, uint32_t xcd_square,
                           uint32_t life_block, uint32_t* order_out);

/* Follow mode's order (include/rts.h, rts_ctx_read_follow) on the host: the checker of the device planner.  life_ticks[t]: the life of
 * tile t = bx + by * blocks_x of a blocks_x x blocks_y dispatch in 100 MHz ticks; a tile's band is rts_ctx_plan_splits' half-octave of
 * ticks * 0.01f us (of the longest tile of its life_block x life_block block, 0 / 1: itself; at most 64); xcd_square S > 0: each band
 * dealt by the DEAL rule of include/rts.h.  order_out[r] = tile id of record first_record + r.  With S = 0 the order equals
 * rtsh_split_front_order's for the same lives and life_block. */
int rtsh_follow_order(const uint32_t* life_ticks, uint32_t blocks_x, uint32_t blocks_y, uint32_t first_record, uint32_t xcd_square,
                      uint32_t life_block, uint32_t* order_out);

/* The device planner of follow mode (rts_follow.hip) on lives the caller gives: what a trace in follow mode queues after its mask
 * kernel, run on tile t's stamps {start_ticks[t], start_ticks[t] + life_ticks[t]} (mod 2^32; start_ticks NULL: 0) in buffers sized
 * and carved as a stream's follow state is, with "follow_square" xcd_square and "follow_block" life_block.  order_out[i] = the
 * tile of record i as bx | by << 16 (as rts_ctx_read_follow; first record 0).  Synchronous, on the default stream; refused
 * (RTS_ERR_INVALID_ARG) while that stream is being captured, for the arguments rtsh_follow_order refuses and for a side of more
 * than 65 536 tiles; zero tiles: RTS_OK.  Touches no stream's follow state, no counter and no option. */
int rtsh_follow_plan_device(rts_ctx* ctx, const uint32_t* life_ticks, const uint32_t* start_ticks /* nullable: 0 */,
                            uint32_t blocks_x, uint32_t blocks_y, uint32_t xcd_square, uint32_t life_block,
                            uint32_t* order_out /* record i -> bx | by << 16, as rts_ctx_read_follow */);

/* MOTION VECTORS: TEMPORAL ACCUMULATION THAT FOLLOWS REFITTED GEOMETRY.  The temporal passes above reproject through
 * the CAMERA's motion alone; a pixel on geometry that a refit moved fails their plane test and restarts every frame, and a face that
 * slides in its own plane blends the history of another surface point.  A refit keeps every node index (include/rts.h), and the
 * closest hit knows its leaf, so the surface point a pixel sees can be looked up in the PREVIOUS frame's stream at the same leaf index:
 * two streams of one topology are all that is needed.
 *
 * THE MOTION G-BUFFER PASS: rtsh_primary_gbuffer* plus prev_packed (the previous frame's stream: prev_count_vec4 == count_vec4, a refit
 * sibling of `packed`) and prev_eye.  positions, normals (nullable) and hit_count are rtsh_primary_gbuffer*'s, bit for bit.  New planes:
 *   prev_points         W*H*4 floats: the seen surface point where it was last frame, relative to the PREVIOUS eye; .w = 1 STATIC,
 *                       2 MOVED, 0 background.
 *   prev_point_normals  W*H*4 floats: that surface's normal last frame, .w = 0.
 *   leaves              W*H uint32_t, nullable: the hit leaf's node index, 0xFFFFFFFF for background.
 * Per pixel, with d and hit = the closest hit as in rtsh_primary_gbuffer*:
 *   BACKGROUND: all four floats of both new texels are +0, leaves = 0xFFFFFFFF.
 *   HIT of leaf L: e0, e1, v0 = its nine words in the current stream -- words 0..2 and 4..6 of node L and words 0..2 of the tail at
 *     index a[3] --, e0', e1', v0' = the words at the SAME indices of prev_packed.  The tail index is always the CURRENT stream's, so a
 *     prev_packed of the right size is never read out of bounds, whatever it holds.
 *   STATIC (the nine words are bit-identical): prev_point.xyz = position.xyz + eye_delta, eye_delta[k] = eye[k] - prev_eye[k] formed
 *     once on the host; prev_point.w = 1; prev_point_normal = normal, bit for bit.  This is REPROJECT's Q above.
 *   MOVED (any word differs): with o = eye, s1 = cross(d, e1), det = dot(s1, e0), invd = 1 / det, dd = o - v0, b1 = dot(dd, s1) * invd,
 *     s2 = cross(dd, e0), b2 = dot(d, s2) * invd (the closest hit's own expressions), per component
 *       prev_point = (v0' + (e0' * b1 + e1' * b2)) - prev_eye,   every operation rounded once, in this grouping, no contraction;
 *     prev_point.w = 2.  n' = cross(e0', e1'), s' = dot(n', n') > 0 ? 1 / sqrtf(dot(n', n')) : 0, negated exactly where the current
 *     normal was (dot(cross(e0, e1), d) > 0: the same side of the triangle, not a new decision); prev_point_normal = n' * s', .w = 0.
 *     A triangle that was degenerate last frame gives a zero normal: "no history" to the passes below.
 *     The host and the device form agree bit for bit on every component that is not a NaN.  A component of a MOVED texel can be a
 *     NaN only where the nine words of prev_packed hold a NaN or an Inf; it is then a NaN in both forms, but WHICH NaN is not defined
 *     (which NaN Inf * 0 or Inf - Inf returns is the one thing hosts and the GPU disagree on; measured on poisoned streams, a third
 *     of the NaN components differ in their bits, all of them in prev_point_normals).  The passes below reject every NaN alike.
 *   * RTS_ERR_INVALID_ARG, nothing written, nothing launched: everything rtsh_primary_gbuffer* refuses; a NULL prev_packed, prev_eye,
 *     prev_points or prev_point_normals; a prev_eye that is not finite; prev_count_vec4 != count_vec4 (device form: != the installed
 *     stream's).  Host form: a prev_packed whose tag and link words differ from packed's is RTS_ERR_BAD_BVH.  Device form: equal
 *     topology is the caller's contract; the index rule keeps a violation memory-safe.
 *   * device form: the same 8 x 8 tile grid and RTSH_GBUFFER_MAX_HEIGHT; ONE kernel node under capture; allocates nothing, reads
 *     nothing back; every buffer on its element type's alignment. */
int rtsh_primary_gbuffer_motion(const rts_vec4u* packed, size_t count_vec4, const rts_vec4u* prev_packed, size_t prev_count_vec4,
                                const float eye[3], const float prev_eye[3], const float target[3], float fovy, uint32_t W, uint32_t H,
                                float* positions, float* normals, float* prev_points, float* prev_point_normals, uint32_t* leaves,
                                uint64_t* hit_count, int threads);
int rtsh_primary_gbuffer_motion_device(rts_ctx* ctx, const rts_vec4u* d_prev_packed, size_t prev_count_vec4, const float eye[3],
                                       const float prev_eye[3], const float target[3], float fovy, uint32_t W, uint32_t H,
                                       float* d_positions, float* d_normals, float* d_prev_points, float* d_prev_point_normals,
                                       uint32_t* d_leaves, void* stream);

/* The installed stream, copied into a caller's DEVICE buffer of capacity_vec4 vec4: one asynchronous device-to-device copy on `stream`
 * (ONE memcpy node under capture), so that a frame loop is snapshot -> rts_ctx_refit_bvh_device -> motion G-buffer with no host round
 * trip.  ORDER: rts_ctx_refit_bvh_device runs on the DEFAULT stream and waits for no stream of rts_stream_create (those do not
 * synchronise with the default one): the copy is ordered before the refit when `stream` is the default stream (NULL), as the frame
 * loop of tools/render.py issues it, or when the caller has synchronised `stream` before it calls the refit.  The refit returns when
 * its kernels are done, so whatever is issued after it, on any stream, sees the refitted stream and a finished default-stream copy.
 * RTS_ERR_NO_BVH before rts_ctx_set_bvh; RTS_ERR_INVALID_ARG for a
 * NULL ctx or buffer or too small a capacity, with nothing copied. */
int rtsh_ctx_snapshot_bvh_device(rts_ctx* ctx, rts_vec4u* d_out, size_t capacity_vec4, void* stream);
/* The installed stream's size in vec4, 0 before rts_ctx_set_bvh. */
size_t rtsh_ctx_bvh_count(rts_ctx* ctx);

/* THE MOTION FORMS OF THE THREE TEMPORAL PASSES: each is its parent's signature plus prev_points and prev_point_normals, THIS frame's
 * planes from the motion G-buffer pass.  Everything of the parent rule holds word for word except:
 *   REPROJECT: Q = prev_points[p].xyz in place of P_p + eye_delta.  params->eye_delta is not used but must still be finite.
 *   TAP ACCEPTANCE: M_p = prev_point_normals[p].xyz stands in place of N_p in both geometric tests -- dot3(M_p, N'_q) >= normal_cos_min
 *     and fabsf(dot3(M_p, P'_q - Q)) <= plane_eps: the surface is compared with what the previous frame saw, in the previous frame's
 *     orientation, so a rotating object keeps its history.  Where M_p is all zero at an active pixel no tap is accepted and the pixel
 *     restarts.  INACTIVE is still decided by the CURRENT normal and map.  A NaN anywhere in Q or M_p rejects, as every comparison does.
 * ANCHOR: over the planes of a motion G-buffer pass with prev_packed == packed (every hit STATIC) and eye_delta = eye - prev_eye, each
 * motion form gives its parent's bits.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: the parents' refusals; prev_points or prev_point_normals NULL while the
 *     prev_* history is given (on the first frame both may be NULL and are not read).
 *   * device forms: the parents' shape, ONE kernel node under capture; the two texels are read once, by their own pixel. */
int rtsh_accumulate_visibility_list_motion(const rts_light_list* list, const rtsh_temporal_params* params, const float* positions,
                                           const float* normals, const uint8_t* lights_map, const float* visibility,
                                           const float* prev_positions, const float* prev_normals, const float* prev_visibility,
                                           const uint8_t* prev_lengths, const float* prev_points, const float* prev_point_normals,
                                           uint32_t W, uint32_t H, float* visibility_out, uint8_t* lengths_out, int threads);
int rtsh_accumulate_visibility_list_motion_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_temporal_params* params,
                                                  const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                  const float* d_visibility, const float* d_prev_positions, const float* d_prev_normals,
                                                  const float* d_prev_visibility, const uint8_t* d_prev_lengths,
                                                  const float* d_prev_points, const float* d_prev_point_normals, uint32_t W, uint32_t H,
                                                  float* d_visibility_out, uint8_t* d_lengths_out, void* stream);
int rtsh_accumulate_visibility_list_clamped_motion(const rts_light_list* list, const rtsh_temporal_params* params, const float* positions,
                                                   const float* normals, const uint8_t* lights_map, const float* visibility,
                                                   const float* prev_positions, const float* prev_normals, const float* prev_visibility,
                                                   const uint8_t* prev_lengths, const float* prev_points,
                                                   const float* prev_point_normals, uint32_t W, uint32_t H, float* visibility_out,
                                                   uint8_t* lengths_out, const rtsh_history_clamp* clamp, int threads);
int rtsh_accumulate_visibility_list_clamped_motion_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_temporal_params* params,
                                                          const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                          const float* d_visibility, const float* d_prev_positions,
                                                          const float* d_prev_normals, const float* d_prev_visibility,
                                                          const uint8_t* d_prev_lengths, const float* d_prev_points,
                                                          const float* d_prev_point_normals, uint32_t W, uint32_t H,
                                                          float* d_visibility_out, uint8_t* d_lengths_out,
                                                          const rtsh_history_clamp* clamp, void* stream);
int rtsh_accumulate_moments_soft_light_list_motion(const rts_soft_light_list* list, const rtsh_temporal_params* params,
                                                   const float* positions, const float* normals, const uint8_t* lights_map,
                                                   const uint8_t* counts, const float* prev_positions, const float* prev_normals,
                                                   const uint16_t* prev_mean, const uint32_t* prev_square, const uint8_t* prev_lengths,
                                                   const float* prev_points, const float* prev_point_normals, uint32_t W, uint32_t H,
                                                   uint16_t* mean_out, uint32_t* square_out, uint8_t* lengths_out, int threads);
int rtsh_accumulate_moments_soft_light_list_motion_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                          const rtsh_temporal_params* params, const float* d_positions,
                                                          const float* d_normals, const uint8_t* d_lights_map, const uint8_t* d_counts,
                                                          const float* d_prev_positions, const float* d_prev_normals,
                                                          const uint16_t* d_prev_mean, const uint32_t* d_prev_square,
                                                          const uint8_t* d_prev_lengths, const float* d_prev_points,
                                                          const float* d_prev_point_normals, uint32_t W, uint32_t H,
                                                          uint16_t* d_mean_out, uint32_t* d_square_out, uint8_t* d_lengths_out,
                                                          void* stream);

/* THE CLAMPED FORMS OF THE MOMENTS PASS: rtsh_accumulate_moments_soft_light_list and its motion form reject history by the RECEIVER's
 * geometry alone, so a shadow that changes on a receiver that does not -- a moving occluder's cast shadow, a drifting light -- lags
 * (max_length 32: 97 % of the stale mean), and reset_lights throws a light's whole history away.  Here a pair's reprojected tap sums are
 * first CLAMPED into a box built from THIS frame's counts over a (2r+1) x (2r+1) window: the window's [min, max] INTERSECTED with its
 * mean +- sigma_k4/4 standard deviations.  V_0 is a 16-bit integer, so the window's sums are integer sums and the square root is an
 * exact integer one: no order of taps, no tiling and no staging scheme can change a bit, and the host forms check the device forms bit
 * for bit.  Everything of the parent rule holds unchanged -- INACTIVE, REPROJECT (or the motion forms' Q and M_p), tap acceptance, sw,
 * s, m, n, PASS-THROUGH, lengths_out --; ONE step is added between the tap sums and the quotient, so only at a BLENDED (pixel, light).
 *   WINDOW of pixel p = (x, y) for light l: of the taps q = (x+dx, y+dy), |dx| <= r and |dy| <= r, those CONTRIBUTE that lie inside the
 *     frame, whose normals[q].xyz is not all zero, and for which lights_map is NULL or bit l of lights_map[q] is set (the activity
 *     conditions of rtsh_accumulate_visibility_list_clamped; no NaN case: the values are integers).  A tap's value is v_q = V_0(q, l)
 *     of THIS frame's counts; the window lies on THIS frame's pixel grid in the motion form too.  The centre of a blended pair always
 *     contributes.  Over the contributing taps: m = their number (at most 81), S1 = sum v (< 2^23), S2 = sum v^2 (< 2^39), lo = min v,
 *     hi = max v.
 *   BOX (unsigned 64-bit integers throughout): D = m * S2 - S1^2 (never negative, < 2^43); x = sigma_k4^2 * D (< 2^59);
 *     R = ceil(sqrt(x)) = isqrt(x), plus one where isqrt(x)^2 < x; Rc = (R + 3) / 4; A = S1 - Rc saturating at 0, B = S1 + Rc;
 *     L_m = max(m * lo, A), H_m = min(m * hi, B); Lv = L_m / m (floor), Hv = (H_m + m - 1) / m (ceiling): rounded OUTWARD to whole
 *     units of V_0; Lv' = Lv - margin saturating at 0, Hv' = min(65535, Hv + margin).  (m * mean = S1 and m * sigma = sqrt(D): the
 *     box is mean +- (sigma_k4 / 4) sigma in units of 1/m, cut to the range.)  rtsh_moments_clamp_bounds evaluates exactly this from
 *     its parts: the host twin, the kernels and the tests share that one source.  Outside the widths above (m == 0 or above 81,
 *     sigma_k4 above 255, hi above 65535, lo above hi, S1 >= 2^23, S2 >= 2^39, m * S2 < S1^2) it gives Lv' = 0 and Hv' = 65535.
 *   CLAMP: s1' = min(max(s1, sw * Lv'), sw * Hv'), s2' = min(max(s2, sw * Lv'^2), sw * Hv'^2) (at most 2^42); then num, den and the
 *     single rounded quotient of the parent rule on s1' and s2'.  Every width of the parent rule still holds.
 * ANCHORS: (1) margin 65535 gives the unclamped pass's three planes bit for bit, for any radius and sigma_k4, over a history whose
 * squares are at most 65535^2 -- every plane this pass or its parent wrote is, by RANGE; a foreign prev_square above it is cut to
 * sw * 65535^2 like any other value above the box.  (2) radius 0 with
 * margin 0 gives mean_out = cur1 and square_out = cur2 at every blended pair, and the unclamped lengths.  (3) Pass-through and inactive
 * pairs are the unclamped rule's bits: the first frame, max_length 1 and a light in reset_lights are all pass-through.  (4) THE STEP:
 * history mean 65535 and square 65535^2 of any length, current counts all 0, a still camera, margin 0: mean 0 and square 0 exactly, at
 * any radius, sigma_k4 and max_length, where the unclamped pass gives round(65535 * (n - 1) / n).  (5) sigma_k4 >= 36 is the range box
 * alone: by Samuelson's inequality no value lies further than sqrt(m - 1) < 9 deviations from its window's mean; so sigma_k4 36 and
 * 255 agree bit for bit.  At sigma_k4 0 the box is the window's mean rounded outward: Hv - Lv <= 1.  Always lo <= Lv <= Hv <= hi.
 * (6) RANGE: every mean_out lies between min(Lv', cur1) and max(Hv', cur1), every square_out between min(Lv'^2, cur2) and
 * max(Hv'^2, cur2).
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: everything the unclamped form (and, for the motion forms, the motion form)
 *     refuses; a NULL clamp; radius above RTSH_MOMENTS_CLAMP_MAX_RADIUS; sigma_k4 above 255; margin above 65535.  `counts` is only read
 *     and no output has its type: there is no counterpart of the float clamp's visibility_out == visibility refusal.
 *   * reserved_ is ignored.  Planes from `count` up are never touched.  Host forms: multi-threaded.  Device forms: DEVICE buffers,
 *     asynchronous on `stream`, allocate nothing, read nothing back; under graph capture ONE kernel node, list, params and clamp by
 *     value.  No BVH, no alignment of any buffer beyond its element type's.
 *   * OUT OF SCOPE: a sigma box for the float pass (rtsh_accumulate_visibility_list_clamped keeps its min/max box), a data-dependent
 *     skip per block, row ranges and stripes. */
enum { RTSH_MOMENTS_CLAMP_MAX_RADIUS = 4 };
typedef struct rtsh_moments_clamp {
    uint32_t radius;                                   /* r, 0 .. RTSH_MOMENTS_CLAMP_MAX_RADIUS: the window is (2r+1) x (2r+1) pixels */
    uint32_t sigma_k4;                                 /* 0 .. 255: the box is mean +- sigma_k4/4 deviations, cut to [min, max] */
    uint32_t margin;                                   /* 0 .. 65535, in units of V_0: widens the box on both sides */
    uint32_t reserved_;                                /* ignored */
} rtsh_moments_clamp;                                                              /* 16 bytes */
void rtsh_moments_clamp_bounds(uint32_t m, uint64_t S1, uint64_t S2, uint32_t lo, uint32_t hi, uint32_t sigma_k4, uint32_t margin,
                               uint32_t* Lv, uint32_t* Hv);
int rtsh_accumulate_moments_soft_light_list_clamped(const rts_soft_light_list* list, const rtsh_temporal_params* params,
                                                    const float* positions, const float* normals, const uint8_t* lights_map,
                                                    const uint8_t* counts, const float* prev_positions, const float* prev_normals,
                                                    const uint16_t* prev_mean, const uint32_t* prev_square, const uint8_t* prev_lengths,
                                                    uint32_t W, uint32_t H, uint16_t* mean_out, uint32_t* square_out, uint8_t* lengths_out,
                                                    const rtsh_moments_clamp* clamp, int threads);
int rtsh_accumulate_moments_soft_light_list_clamped_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_temporal_params* params,
                                                           const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                                           const uint8_t* d_counts, const float* d_prev_positions,
                                                           const float* d_prev_normals, const uint16_t* d_prev_mean,
                                                           const uint32_t* d_prev_square, const uint8_t* d_prev_lengths, uint32_t W,
                                                           uint32_t H, uint16_t* d_mean_out, uint32_t* d_square_out, uint8_t* d_lengths_out,
                                                           const rtsh_moments_clamp* clamp, void* stream);
int rtsh_accumulate_moments_soft_light_list_clamped_motion(const rts_soft_light_list* list, const rtsh_temporal_params* params,
                                                           const float* positions, const float* normals, const uint8_t* lights_map,
                                                           const uint8_t* counts, const float* prev_positions, const float* prev_normals,
                                                           const uint16_t* prev_mean, const uint32_t* prev_square,
                                                           const uint8_t* prev_lengths, const float* prev_points,
                                                           const float* prev_point_normals, uint32_t W, uint32_t H, uint16_t* mean_out,
                                                           uint32_t* square_out, uint8_t* lengths_out, const rtsh_moments_clamp* clamp,
                                                           int threads);
int rtsh_accumulate_moments_soft_light_list_clamped_motion_device(rts_ctx* ctx, const rts_soft_light_list* list,
                                                                  const rtsh_temporal_params* params, const float* d_positions,
                                                                  const float* d_normals, const uint8_t* d_lights_map,
                                                                  const uint8_t* d_counts, const float* d_prev_positions,
                                                                  const float* d_prev_normals, const uint16_t* d_prev_mean,
                                                                  const uint32_t* d_prev_square, const uint8_t* d_prev_lengths,
                                                                  const float* d_prev_points, const float* d_prev_point_normals,
                                                                  uint32_t W, uint32_t H, uint16_t* d_mean_out, uint32_t* d_square_out,
                                                                  uint8_t* d_lengths_out, const rtsh_moments_clamp* clamp, void* stream);

/* HALF-RESOLUTION LIGHT LISTS: trace a quarter of the pixels and reconstruct the rest from the G-buffer.  Three passes around the
 * EXISTING traces -- subsample the G-buffer, (trace it at w x h with rts_trace_soft_light_list* / rts_trace_light_list*,) mark the pixels
 * no traced neighbour can stand for, (trace those at full resolution with the mark as lights_map,) upsample the rest -- whose result is
 * COUNT PLANES again, uint8_t per light at W x H (one mask byte for a hard list), which every later stage takes unchanged.  A dense
 * half-resolution frame keeps the 8 x 8 packets of the trace full, where a checkerboard map would idle half of each.  The result is
 * a function of the inputs alone: integer weights, integer sums, one integer quotient per light; floats appear in per-tap comparisons
 * only; so the host forms check the device forms byte for byte.
 *   typedef struct rtsh_upsample_params: phase_x, phase_y (0 or 1), normal_cos_min, plane_eps (world units), reserved_ (ignored).
 * THE LATTICE: low-resolution pixel (X, Y) IS full-resolution pixel s(X, Y) = (2X + phase_x, 2Y + phase_y); the low-resolution frame
 *   is w x h with w = (W + 1 - phase_x) >> 1 and h = (H + 1 - phase_y) >> 1 (rtsh_subsampled_size): exactly the sampled pixels inside
 *   the frame, nothing is ever clamped.  A caller may rotate the phase per frame so that a temporal stage sees all four pixels of a quad.
 * on(p, l), bg(p), N_p, P_p and geom(p, q) are the filter's above (rtsh_filter_*_light_list); c_l(q) = the byte of LOW-RESOLUTION
 *   plane l at q (lo_counts[l * w * h + q]; bit l of lo_mask[q] as 0 or 1), unclamped.
 * rtsh_subsample_gbuffer: lo_positions[q], lo_normals[q] (four floats each, copied as they are) and, where lights_map is not NULL,
 *   lo_lights_map[q] = those of s(q).  lights_map == NULL: lo_lights_map is not touched (and may be NULL).
 * TAPS of p = (x, y): u = x - phase_x, X0 = u >> 1 (arithmetic: -1 for u = -1), ax = u & 1; v = y - phase_y, Y0 = v >> 1, ay = v & 1.
 *   Four taps IN THIS ORDER: (X0, Y0), (X0+1, Y0), (X0, Y0+1), (X0+1, Y0+1), of the INTEGER weights (2-ax)*(2-ay), ax*(2-ay), (2-ax)*ay,
 *   ax*ay, which sum to 4.  A tap of weight 0, or outside w x h, DOES NOT EXIST.  A tap whose sampled pixel is p itself (ax == ay == 0:
 *   the one tap, of weight 4) is always accepted for every light; its map bit is not looked at.  Any other tap q is ACCEPTED for light
 *   l when geom(p, q) holds -- the one shared function of the wide filters: not bg(q), the normal test against normal_cos_min, the plane
 *   test against plane_eps, in that order, a NaN rejects; p's data from the full-resolution G-buffer, q's from the low-resolution one
 *   -- and on(q, l) holds in lo_lights_map (NULL: every light).
 * rtsh_upsample_retrace_map: bit l < count of retrace[p] is set exactly where p is not background, on(p, l) holds, p is not a sampled
 *   pixel and no tap of p is accepted for light l; every other bit is 0.  Given to a full-resolution trace as lights_map, that trace
 *   writes the planes: the traced byte where the bit is set, 0 where it is clear.
 * rtsh_upsample_soft_light_list / rtsh_upsample_light_list, for p and l < count, in this order:
 *   KEEP: where keep != NULL and bit l of keep[p] is set, plane l at p is NOT TOUCHED (a hard list: bit l of mask[p] stays, the byte is
 *     read and rewritten) and nothing else of p is looked at for that light.  With keep = the retrace map the pass merges in place
 *     behind the masked trace: no temporary, no merge pass.
 *   INACTIVE: where bg(p) or not on(p, l), the byte is 0 and nothing else is read.
 *   QUOTIENT: num = sum of w * c_l(q), den = sum of w over the accepted taps; byte = (2 * num + den) / (2 * den) in unsigned integers:
 *     the mean rounded half up.  A hard list uses the same formula on bits.
 *   FALLBACK: with no accepted tap, the byte c_l(q) of the existing tap with on(q, l) of the LARGEST weight, the FIRST such in tap
 *     order; 0 if there is none.  (Its geometry is not looked at: every existing tap failed it.)
 *   Bits of a hard list's mask from `count` up are written 0 wherever the byte is written (it is not where every light below count
 *   is kept); planes of a soft list from `count` up are never touched.
 * ANCHORS: (1) a sampled pixel active for light l gets its low-resolution byte exactly ((8c + 4) / 8 = c).  (2) Where every accepted
 * tap carries the same byte c the result is c ((2 * c * den + den) / (2 * den) = c).  (3) With keep = the retrace map of the same
 * params and maps, no written (pixel, light) takes the fallback.  (4) With a list without jitter tables and plane_eps = -1.0f (no
 * neighbour is accepted): subsample, trace at w x h, retrace map, trace at W x H under it, upsample with keep -- equals the plain trace
 * at W x H byte for byte, in every phase: a pixel's count depends on its position and the list alone, and a pixel is either sampled
 * or retraced.  (At background pixels this needs a map that clears them, as rtsh_facing_lights' does: WITHOUT a map the plain trace
 * traces a background pixel's cleared texel like any other, and the INACTIVE rule gives it 0.)
 *   * lights_map, lo_lights_map and keep may each be NULL.  All other buffers are required.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: what rtsh_filter_*_light_list* refuse of a list (the retrace map takes
 *     `count` alone: 0 or above RTS_MAX_LIST_LIGHTS); NULL params, G-buffers (full or low) or planes (full or low); a phase above 1; a
 *     normal_cos_min or plane_eps that is not finite; W, H, w or h equal to 0 (phase 1 on a frame one pixel wide); W or H above
 *     0x7FFFFFF0; output planes equal to the low-resolution planes; in rtsh_subsample_gbuffer a lights_map without lo_lights_map; in
 *     the device forms a NULL ctx and, in the two full-resolution passes, H above 8 * 65535 (the grid).
 *   * host forms: multi-threaded (threads: 0 = all host threads).  Device forms: DEVICE buffers, asynchronous on `stream`, allocate
 *     nothing and read nothing back, need no BVH and no alignment of any buffer beyond its element type's; under graph capture each
 *     adds ONE kernel node, parameters by value (params is read during the call).  One low-resolution pixel per lane in the
 *     subsample, one full-resolution pixel per lane in the other two.
 *   * OUT OF SCOPE: distance planes; the adaptive and jittered list forms (a jitter hash takes the index in the frame traced); factors
 *     other than 2; row ranges and stripes. */
typedef struct rtsh_upsample_params {
    uint32_t phase_x, phase_y;  /* 0 or 1: low-resolution (X, Y) is full-resolution (2X + phase_x, 2Y + phase_y) */
    float    normal_cos_min;    /* a tap needs N_p . N_q >= this */
    float    plane_eps;         /* ... and |N_p . (P_q - P_p)| <= this (world units) */
    uint32_t reserved_[4];      /* ignored */
} rtsh_upsample_params;                                                            /* 32 bytes */
int rtsh_subsampled_size(uint32_t W, uint32_t H, uint32_t phase_x, uint32_t phase_y, uint32_t* w, uint32_t* h);
int rtsh_subsample_gbuffer(const rtsh_upsample_params* params, const float* positions, const float* normals, const uint8_t* lights_map,
                           uint32_t W, uint32_t H, float* lo_positions, float* lo_normals, uint8_t* lo_lights_map);
int rtsh_subsample_gbuffer_device(rts_ctx* ctx, const rtsh_upsample_params* params, const float* d_positions, const float* d_normals,
                                  const uint8_t* d_lights_map, uint32_t W, uint32_t H, float* d_lo_positions, float* d_lo_normals,
                                  uint8_t* d_lo_lights_map, void* stream);
int rtsh_upsample_retrace_map(uint32_t count, const rtsh_upsample_params* params, const float* positions, const float* normals,
                              const uint8_t* lights_map, const float* lo_positions, const float* lo_normals, const uint8_t* lo_lights_map,
                              uint32_t W, uint32_t H, uint8_t* retrace, int threads);
int rtsh_upsample_retrace_map_device(rts_ctx* ctx, uint32_t count, const rtsh_upsample_params* params, const float* d_positions,
                                     const float* d_normals, const uint8_t* d_lights_map, const float* d_lo_positions,
                                     const float* d_lo_normals, const uint8_t* d_lo_lights_map, uint32_t W, uint32_t H, uint8_t* d_retrace,
                                     void* stream);
int rtsh_upsample_light_list(const rts_light_list* list, const rtsh_upsample_params* params, const float* positions, const float* normals,
                             const uint8_t* lights_map, const float* lo_positions, const float* lo_normals, const uint8_t* lo_lights_map,
                             const uint8_t* lo_mask, const uint8_t* keep, uint32_t W, uint32_t H, uint8_t* mask, int threads);
int rtsh_upsample_soft_light_list(const rts_soft_light_list* list, const rtsh_upsample_params* params, const float* positions,
                                  const float* normals, const uint8_t* lights_map, const float* lo_positions, const float* lo_normals,
                                  const uint8_t* lo_lights_map, const uint8_t* lo_counts, const uint8_t* keep, uint32_t W, uint32_t H,
                                  uint8_t* counts, int threads);
int rtsh_upsample_light_list_device(rts_ctx* ctx, const rts_light_list* list, const rtsh_upsample_params* params, const float* d_positions,
                                    const float* d_normals, const uint8_t* d_lights_map, const float* d_lo_positions,
                                    const float* d_lo_normals, const uint8_t* d_lo_lights_map, const uint8_t* d_lo_mask,
                                    const uint8_t* d_keep, uint32_t W, uint32_t H, uint8_t* d_mask, void* stream);
int rtsh_upsample_soft_light_list_device(rts_ctx* ctx, const rts_soft_light_list* list, const rtsh_upsample_params* params,
                                         const float* d_positions, const float* d_normals, const uint8_t* d_lights_map,
                                         const float* d_lo_positions, const float* d_lo_normals, const uint8_t* d_lo_lights_map,
                                         const uint8_t* d_lo_counts, const uint8_t* d_keep, uint32_t W, uint32_t H, uint8_t* d_counts,
                                         void* stream);

/* COMPACTED LIGHT MAPS: a light map -> the dense LIST of its marked pixels, for the sparse list traces (rts.h, SPARSE LIGHT LISTS).  A
 * masked block trace opens every 8 x 8 tile that holds one marked pixel; a mark that sets 1 % of the bits along every silhouette costs
 * a fifth to a third of a whole trace.  The list lets a trace put 64 marked pixels into every wave.  Integers only, no float anywhere.
 * THE RULE, for a map of W x H bytes and count = 1..8 lights:
 *   MARKED: pixel p = y * W + x is marked when lights_map[p] & ((1 << count) - 1) is not 0.
 *   TILE ORDER: the frame is cut into tiles of 8 x 8 pixels, tile (tx, ty) = the pixels x in [8 tx, 8 tx + 8), y in [8 ty, 8 ty + 8)
 *     that lie inside the frame; there are ceil(W / 8) x ceil(H / 8) tiles.  The tiles are taken in row-major order (ty ascending, then
 *     tx ascending), the pixels of a tile in row-major order (y ascending, then x ascending).  The list holds the marked pixels in that
 *     order, as 32-bit indices p.  So 64 consecutive entries come from one tile or from neighbouring tiles of a tile row (and, at a
 *     row's end, the next row's first tiles): a wave's rays stay near each other.
 *   *n receives the number of marked pixels of the WHOLE frame; it may exceed capacity.  pixels[0 .. min(n, capacity)) receive the first
 *   entries of the list.  No entry from min(n, capacity) on is touched.  The order is fixed by the rule: the host form, the device form
 *   and a restatement from this text agree word for word.
 *   * RTS_ERR_INVALID_ARG, nothing launched, nothing written: count 0 or above 8; a NULL map, list or n; W or H equal to 0; W * H above
 *     2^31; capacity 0; in the device form a NULL ctx or scratch.
 *   * rtsh_compact_scratch_bytes(W, H): the bytes of d_scratch, 4 * (tiles + ceil(tiles / 1024)); 0 for a frame that is refused.
 *   * device form: DEVICE buffers, asynchronous on `stream`, allocates nothing and reads nothing back, needs no BVH; d_scratch and d_n
 *     need 4-byte alignment.  FOUR kernels (rtsh_compact_nodes()): a count per tile (one wave per tile: ballot and popcount), an
 *     exclusive sum inside groups of 1024 tiles, an exclusive sum of the groups' totals by ONE workgroup (which also writes *d_n), the
 *     write pass (one wave per tile again).  No workgroup waits for another one: each kernel reads what the kernel in front of it has
 *     finished.  Under graph capture it adds those four kernel nodes and no other node; the pointers are captured, so a replay compacts
 *     whatever map the buffer holds then.
 *   * SIZING capacity: W * H always suffices.  A renderer that knows its mark sizes it from the mark; a frame whose
 *     list does not fit is seen from *n > capacity, and the first `capacity` entries are still valid. */
size_t rtsh_compact_scratch_bytes(uint32_t W, uint32_t H);
int rtsh_compact_nodes(void);
int rtsh_compact_light_map(uint32_t count, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t* pixels, uint32_t capacity,
                           uint32_t* n_out);
int rtsh_compact_light_map_device(rts_ctx* ctx, uint32_t count, const uint8_t* d_lights_map, uint32_t W, uint32_t H, uint32_t* d_pixels,
                                  uint32_t capacity, uint32_t* d_n, void* d_scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RTS_SCENE_H */
