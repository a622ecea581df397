/* =============================================================================
 * rts.h -- C ABI of the MI355X-native shadow-ray path (librts.so).
 *
 * Drop-in boundary for the ONE hot path of kayru/RayTracedShadows:
 *     BVHBuilder::build  ->  packed vec4 node stream  ->  any-hit shadow kernel
 * Plain pointers and sizes only; no C++/torch types cross this line.  Every entry
 * returns an int status (RTS_OK == 0) and never throws.
 *
 * Each declaration cites the reference interface it replaces (paths relative to
 * the reference checkout).  The reference-side binding a maintainer would add is
 * shown in INTEGRATION.md.
 * ========================================================================== */
#ifndef RTS_H
#define RTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
enum {
    RTS_OK              = 0,
    RTS_ERR_INVALID_ARG = 1, /* NULL pointer, prim_count == 0, bad row range ...           */
    RTS_ERR_CAPACITY    = 2, /* output buffer too small                                    */
    RTS_ERR_NONFINITE   = 3, /* NaN/Inf vertex (reference: unbounded recursion, SURVEY E-4) */
    RTS_ERR_NO_BVH      = 4, /* trace called before rts_ctx_set_bvh                         */
    RTS_ERR_BAD_BVH     = 5, /* packed buffer fails structural validation                   */
    RTS_ERR_DEGENERATE  = 6, /* finite vertices whose extents overflow the SAH cost to +inf: no split position
                                exists (reference: unbounded recursion, SURVEY E-4/E-5); RTS_GPU_BUILD_SAH also: a
                                tree deeper than 262 144 levels (hundreds of thousands of triangles with EQUAL boxes split
                                off one per level; the reference recurses as deep as that chain is long)        */
    RTS_ERR_HIP         = 100 /* 100 + hipError_t                                           */
};
const char* rts_status_string(int status);

/* ---- data contract -------------------------------------------------------- */

/* Source/BVHBuilder.h:22-25 `struct BVHPackedNode {u32 a,b,c,d;}` == GLSL `vec4 bvhNodes[]`
 * (Source/Shaders/RayTracedShadows.comp:23-26).  Layout of the whole buffer: SURVEY.md Appendix A. */
typedef struct rts_vec4u { uint32_t a, b, c, d; } rts_vec4u;

/* Source/BVHBuilder.h:8-20 `struct BVHNode` (unpacked, DFS order; prim==0xFFFFFFFF <=> inner). */
typedef struct rts_bvh_node {
    float bboxMin[3]; uint32_t prim;
    float bboxMax[3]; uint32_t next;
} rts_bvh_node;

/* Source/RayTracedShadows.h:56-62 `struct RayTracingConstants` == UBO `Constants`
 * (RayTracedShadows.comp:3-9).  Only cameraPosition.xyz and lightDirection.xyz are read. */
typedef struct rts_constants {
    float cameraPosition[4];
    float cameraDirection[4];
    float lightDirection[4];
    float renderTargetSize[4];
} rts_constants;

/* RayTracedShadows.comp:28-32 `struct Ray { vec4 o; vec4 d; }`: o.w = tmax, d.w unused. */
typedef struct rts_ray { float o[4]; float d[4]; } rts_ray;

/* Light model.  type RTS_LIGHT_DIRECTIONAL with xyz = constants.lightDirection.xyz is exactly the
 * reference (RayTracedShadows.comp:134-146).  RTS_LIGHT_POINT and nsamples > 1 are the extensions
 * BASELINE.json's configs ask for:
 *   point : o0 = cam + rel; bias as comp:138-140; dn = (L-o0)/|L-o0|; o = o0 + dn*bias;
 *           d = L - o (un-normalised); tmax = 1
 *   nsamples in [2,64]: sample j uses L + offsets[j].xyz; the output byte is the number of
 *   UNoccluded samples (0..nsamples) instead of 0/1.  `table` != 0: per-pixel jitter, see the field. */
enum { RTS_LIGHT_DIRECTIONAL = 0, RTS_LIGHT_POINT = 1 };
typedef struct rts_light {
    uint32_t type;
    uint32_t nsamples;      /* 0 or 1 = hard shadow */
    float    xyz[3];
    uint32_t table;         /* 0: sample j uses offsets[j] in every pixel (one coherent pass per sample).
                               T in [nsamples, 64]: PER-PIXEL jitter -- offsets[] holds T entries and pixel p = y*W + x of the
                               frame uses offsets[(start(p) + j) mod T], start(p) = (hash32(p) * T) >> 32 with
                               hash32(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16
                               (32-bit wrap-around): integer arithmetic only, the same on every device and in every
                               stripe.  Neighbouring pixels then aim at different points of the light in the same pass,
                               which is what stresses ray packets (BASELINE configs[4]).  (The field was `reserved`, 0.) */
    float    offsets[64][4];
} rts_light;

typedef struct rts_ctx rts_ctx;

/* ---- producer: replaces BVHBuilder::build (Source/BVHBuilder.h:31, BVHBuilder.cpp:248-368;
 *      call site Source/RayTracedShadows.cpp:1031-1037) ---------------------- */

/* m_packedNodes.size() for prim_count triangles = 2*(2P-1) + P = 5P-2 (BVHBuilder.cpp:308-367). */
size_t rts_bvh_packed_count(uint32_t prim_count);
/* m_nodes.size() = 2P-1. */
size_t rts_bvh_node_count(uint32_t prim_count);

/* vertices/stride/indices/prim_count: identical meaning to BVHBuilder::build -- `stride_floats`
 * is in floats (the reference passes sizeof(Vertex)/sizeof(float) == 8).  out_packed receives
 * m_packedNodes (capacity in vec4 >= rts_bvh_packed_count); out_nodes (nullable) receives m_nodes.
 * Tail .d words are 0 (reference: uninitialised). */
int rts_bvh_build(const float* vertices, uint32_t stride_floats, const uint32_t* indices,
                  uint32_t prim_count, rts_vec4u* out_packed, size_t out_capacity_vec4,
                  rts_bvh_node* out_nodes);

/* Same with the two knobs the reference hard-codes: sah_prim_limit (1000000 at BVHBuilder.cpp:83;
 * ranges larger than this use the spatial-median split) and the number of host threads
 * (0 = all; the tree does not depend on it). */
int rts_bvh_build_ex(const float* vertices, uint32_t stride_floats, const uint32_t* indices,
                     uint32_t prim_count, uint32_t sah_prim_limit, int threads,
                     rts_vec4u* out_packed, size_t out_capacity_vec4, rts_bvh_node* out_nodes);

/* Structural validation of a packed buffer from ANY producer (ours or the reference's):
 * count == 5P-2, leaf/inner tags, strictly-forward miss links, tail pointers in range. */
int rts_bvh_validate(const rts_vec4u* packed, size_t count_vec4, uint32_t* prim_count_out);

/* BVH build ON THE GPU: four producers of the same packed layout with the reference's layout rules
 * (larger-area child first, DFS numbering, miss links, tail; BVHBuilder.cpp:202-244, 308-367).
 * rts_bvh_build_device = RTS_GPU_BUILD_SAH (BVHBuilder's tree); rts_bvh_build_device_ex picks the topology:
 *   RTS_GPU_BUILD_LBVH  Karras hierarchy + bottom-up bounds (fastest build)
 *   RTS_GPU_BUILD_PLOC  parallel locally-ordered clustering, `radius` = Morton neighbours searched each way (0 = 16)
 *   RTS_GPU_BUILD_PLOC_SAH  PLOC down to <= 65 536 clusters, then the top of the tree over the clusters' boxes by the
 *                       reference's split rule (full-sweep SAH, BVHBuilder.cpp:78-156, weighted by triangle counts) on
 *                       the host: ~10x the build time of PLOC, a tree closer to BVHBuilder's
 *   RTS_GPU_BUILD_SAH   BVHBuilder's own rule for every node, level by level on the device: full-sweep SAH on three
 *                       axes (cpp:78-156), spatial median above `radius` triangles per range (cpp:157-178; 0 = the
 *                       reference's 1 000 000), larger-area child first.  Triangles with EQUAL centroids on an axis are
 *                       ordered by triangle id where the reference's std::sort leaves them unspecified: on a mesh
 *                       without such ties the stream is byte-identical to rts_bvh_build's, otherwise a tree of the
 *                       same quality.  RTS_ERR_DEGENERATE where the reference would not terminate.
 * vertex_floats = number of floats in `vertices`.  `vertices` and `indices` may be host pointers (copied to the device) or
 * device pointers on the context's device (used where they lie: a renderer's vertex and index buffers).  out_packed (host, nullable) receives the 5P-2 vec4; install != 0
 * makes the stream the context's BVH without a host round trip.  build_ms (nullable): device time of the build.
 * The builders' working memory (about 0.6 KB per triangle) stays with the context until rts_ctx_destroy, so that a rebuild
 * per frame allocates nothing. */
enum { RTS_GPU_BUILD_LBVH = 0, RTS_GPU_BUILD_PLOC = 1, RTS_GPU_BUILD_PLOC_SAH = 2, RTS_GPU_BUILD_SAH = 3 };
int rts_bvh_build_device(rts_ctx* ctx, const float* vertices, size_t vertex_floats, uint32_t stride_floats,
                         const uint32_t* indices, uint32_t prim_count, rts_vec4u* out_packed,
                         size_t out_capacity_vec4, int install, float* build_ms);
int rts_bvh_build_device_ex(rts_ctx* ctx, const float* vertices, size_t vertex_floats, uint32_t stride_floats,
                            const uint32_t* indices, uint32_t prim_count, int algorithm, uint32_t radius,
                            rts_vec4u* out_packed, size_t out_capacity_vec4, int install, float* build_ms);

/* ---- refit: moving geometry keeps its tree (an extension: the reference's geometry is static) ----------------------------
 * A refit keeps a stream's topology -- every tag and link word, hence every node index -- and recomputes its boxes and leaf
 * data from new vertex positions for the same prim_count: leaf e0 = v1 - v0, e1 = v2 - v0 and tail v0 (.d = 0) as the builder
 * writes them (BVHBuilder.cpp:324-341), inner bboxMin / bboxMax = the per-axis minimum / maximum over the vertices of the
 * triangles in the node's subtree [i, link(i)) (END: N), taken in the total order of the order-preserving integer encoding
 * (-0.0 < +0.0): no reduction order changes a byte, and with no -0.0 coordinate a refit with the vertices a stream was built
 * from returns it unchanged.  Refused, with nothing changed: a NaN / Inf vertex referenced by the indices -> RTS_ERR_NONFINITE;
 * an index outside vertex_floats, count_vec4 != 5 * prim_count - 2 or (device form) prim_count != the installed stream's ->
 * RTS_ERR_INVALID_ARG; a stream that is not a pre-order binary tree with the reference's miss links -> RTS_ERR_BAD_BVH.
 * Edges that overflow to +-Inf from finite vertices are not an error (as for a build).  DESIGN.md 4.9. */

/* Host, in place on a caller's blob (any producer's): the CPU form, and the checker of the device form. */
int rts_bvh_refit(const float* vertices, size_t vertex_floats, uint32_t stride_floats, const uint32_t* indices,
                  uint32_t prim_count, rts_vec4u* packed, size_t count_vec4);
/* The context's installed stream, on the device, in place.  vertices / indices: host or device pointers as in
 * rts_bvh_build_device_ex.  out_packed (host, nullable) receives the refitted stream; refit_ms (nullable): device time;
 * cost_ratio (nullable): the SAH cost proxy -- sum over inner nodes of surfaceArea(box) / surfaceArea(root), surfaceArea as
 * BVHBuilder.cpp:24-28 -- after this refit, divided by the same for the stream as it was installed (taken at the first refit):
 * how far the tree has degraded, for a renderer that decides when to rebuild instead (a heuristic: no exactness claim).
 * The context ends as rts_ctx_set_bvh of the refitted bytes would leave it ("bvh_finite" / "bvh_ordered" / "bvh_enclosed"
 * decided again; the private copy of kernel 8 refreshed in place, dropped with the split table when the flags no longer
 * allow it, derived when they allow it again), except that the split table, the planned tile order, every option and the
 * stream's allocation are kept: they hold node indices and tile coordinates, which a refit does not change.  What depends on
 * the topology alone (the check, the schedule, the cost baseline) is derived at the first refit after an install and kept
 * until the next one: a steady refit per frame allocates nothing.  Synchronous, default stream, like rts_bvh_build_device. */
int rts_ctx_refit_bvh_device(rts_ctx* ctx, const float* vertices, size_t vertex_floats, uint32_t stride_floats,
                             const uint32_t* indices, uint32_t prim_count, rts_vec4u* out_packed,
                             size_t out_capacity_vec4, float* refit_ms, float* cost_ratio);

/* ---- consumer: replaces the bind-group + dispatch of
 *      RayTracedShadowsApp::renderShadowMaskCompute (Source/RayTracedShadows.cpp:570-595) and the
 *      BVH upload (Source/RayTracedShadows.cpp:1039-1044) ---------------------- */

/* One context per device; not thread-safe; owns the device copy of the BVH. */
int rts_ctx_create(int device_ordinal, rts_ctx** out);
int rts_ctx_destroy(rts_ctx* ctx);

/* == Gfx_CreateBuffer(Storage, stride 16, count, m_packedNodes.data()) (cpp:1039-1044).
 * Validates the structure on the host, copies H2D once (the device copy is the same Appendix-A bytes), then decides on
 * the device what the kernels may assume (finite, ordered, enclosing boxes) and derives the private copy of kernel 8. */
int rts_ctx_set_bvh(rts_ctx* ctx, const rts_vec4u* packed, size_t count_vec4);

/* Tuning knobs.  Results never depend on any of them (tests/test_gpu_parity.py).  Unknown key or bad value ->
 * RTS_ERR_INVALID_ARG.
 *   "kernel"        -1 = auto (default: variant 7 below 256 K pixels, the packet kernel 3 from there, the wide packet 8 for
 *                   one-sample dispatches of >= 4 M pixels when the stream has a private copy); 0 straight,
 *                   1 while-while, 2 postpone, 3 packet (8x8 px / wave), 4 packet2 (16x8), 5 packet4 (16x16),
 *                   6 packet + successor prefetch, 7 lane-per-ray with work sharing, 8 WIDE packet (a private copy of the
 *                   stream with four boxes per node: one dependent fetch decides two levels of the reference's walk; a
 *                   stream without a private copy runs 3), 9 the same with the loop compiled instead of hand-written.
 *                   get "kernel_count" = 10.  rts_ctx_autotune picks between 3, 8 and 7 by timing them on the frame.
 *   "wide_copy"     1 (default): derive the private copy for kernel 8 whenever a stream is installed (on the device,
 *                   about 0.2 KB per triangle; needs a finite stream of ordered, enclosing boxes, at most 512 levels deep,
 *                   at most 2^24 triangles -- otherwise there simply is none); 0: never
 *   "wide_lane"     0 (default): a dissolved wide packet continues lane per ray over the stream, stackless; 1: over the wide
 *                   nodes with a 16-entry stack per lane in LDS (4 KB per wave: a CU then holds 28 instead of 32 waves)
 *   "soft_split"    1 (default): soft shadows (nsamples > 1) with kernel 3 or 8 run 4 waves per tile, each a quarter of the
 *                   samples (the counts meet in LDS); 0: one wave walks a pixel's samples one after the other
 *   "packet_budget" side-steps between two coherence checks of a packet (default 16)
 *   "packet_share"  a packet dissolves when it picks up fewer than share/16 of its live rays per side-step (default 4)
 *   "block_waves"   waves per workgroup of the packet kernels: 1 (default) or 4
 *   "xcd_swizzle"   1 = contiguous image chunk per XCD (default 0: measured slower)
 *   "row_order"     order in which the tile rows of a frame are dispatched: 0 first to last (default), 1 last to first,
 *                   2 middle row outwards (the rows dispatched last are the kernel's tail; which order wins depends on
 *                   where the scene's long rays are: profiles/r02/row_order_sweep.log)
 *   "tile_splits"   1 (default): traces use an installed split table (rts_ctx_plan_splits); 0: they ignore it
 *   "tune_for_motion" 0 (default): rts_ctx_autotune picks the fastest table for THIS frame; 1: only a table that keeps over a
 *                   camera path -- the whole dispatch in table order sorted by blocks of 16 x 16 tiles (rts_split_plan:
 *                   life_block, xcd_square), no pieces, no front lists
 *   "follow"        0 (default); 1: FOLLOW MODE -- one-sample traces in a frame loop run the whole dispatch in an order planned on
 *                   the device from the tile lives of the stream's last trace of the same dispatch (rts_ctx_read_follow below)
 *   "follow_block"  life_block B of follow mode's order, 1..64 (default 8)
 *   "follow_square" xcd_square S of follow mode's order, 0..65535 (default 32; 0: no deal over the XCDs)
 *                   get only: "follow_streams" (streams that hold follow state), "follow_traces" (traces that recorded lives),
 *                   "follow_ordered" (traces that ran a rolling order)
 *   "piece_stats"   diagnostics, see rts_ctx_read_piece_stats;  get only: "split_tiles", "front_tiles", "split_pieces"
 *   "lds_pad"       experiment: extra dynamic LDS bytes per one-wave packet workgroup (throttles occupancy; default 0)
 *   "wave_stats"    diagnostics, see rts_ctx_read_wave_stats
 *   "clock_probe"   diagnostics, see rts_ctx_read_clock_probe
 *   "refit_treelet" nodes per workgroup of the device refit's treelet pass, 32..2048 (default 1024; speed only)
 *   "builder_scratch" set 0: release the working memory the GPU builders keep between builds; get: MiB held
 *   get only: "bvh_finite", "bvh_ordered", "bvh_enclosed" (what the installed stream allows: decided by one kernel over all
 *   nodes at upload / adoption), "wide_nodes", "wide_levels" (size of the private copy, 0 = none) */
int rts_ctx_set_option(rts_ctx* ctx, const char* key, int value);
int rts_ctx_get_option(rts_ctx* ctx, const char* key, int* value);

/* == Gfx_Dispatch(divUp(W,8), divUp(H,8), 1) of RayTracedShadows.comp (cpp:576-592) restricted to
 * rows [row_begin,row_end) (row stripes for multi-GPU).
 *   constants : the 64-byte UBO; cameraPosition.xyz is read.  light == NULL means the reference's
 *               directional light taken from constants->lightDirection.xyz.
 *   positions : binding 2, RGBA32F W x H, row-major, camera-relative world position (Model.frag:35)
 *   mask      : binding 3, W x H bytes; 1 = lit, 0 = occluded (comp:148; polarity of the
 *               reference); rows outside the range are not touched.
 * HOST pointers; copies in, traces, copies out, synchronises. */
int rts_trace_shadow_mask(rts_ctx* ctx, const rts_constants* constants, const rts_light* light,
                          const float* positions, uint32_t W, uint32_t H,
                          uint32_t row_begin, uint32_t row_end, uint8_t* mask);

/* Same with DEVICE pointers, asynchronous on `stream` (a hipStream_t, NULL = default stream).
 * GRAPH CAPTURE (tests/test_gpu_graph.py): this call, the stripes form, the active forms, rts_trace_rays_device and the device
 * passes of rts_scene.h may be issued on a stream under hipStreamBeginCapture.  Each adds kernel nodes only -- one per trace, plus
 * the planner's four in follow mode (three with "follow_block" 1) -- and no memcpy, memset or allocation node; nothing is allocated, cleared or read back.
 * constants, light and every option travel in the kernel arguments BY VALUE as they are at the call: a replay traces the captured
 * light and camera whatever the host structs hold by then, from the positions (and map) the device buffers hold at the replay. */
int rts_trace_shadow_mask_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light,
                                 const float* d_positions, uint32_t W, uint32_t H,
                                 uint32_t row_begin, uint32_t row_end, uint8_t* d_mask, void* stream);

/* Interleaved row stripes in ONE dispatch (multi-GPU strong scaling): the frame is cut
 * into bands of band_rows rows (a multiple of the kernel's workgroup height: 8 for the default packet kernel, 16 or 32 for
 * the others -- 32 always works) dealt round-robin to n_stripes devices; this call
 * traces the bands stripe, stripe + n_stripes, ... and touches no other row of d_mask.  A stripe that owns no band (a frame
 * of fewer bands than n_stripes) launches nothing; the tuning and planning calls for its dispatch return RTS_OK and tune,
 * plan and write nothing (no split table, no tile order, launch options unchanged, *ms = 0). */
int rts_trace_shadow_mask_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light,
                                         const float* d_positions, uint32_t W, uint32_t H, uint32_t band_rows,
                                         uint32_t n_stripes, uint32_t stripe, uint8_t* d_mask, void* stream);

/* ACTIVE MAPS: trace only the pixels the caller marks.  A deferred renderer multiplies the mask by max(0, N.L) and discards the
 * background, so the byte traced for a surface that faces away from the light, or for a background pixel, never reaches the image;
 * light range, spot cones, stencilled regions and checkerboard tracing are the same mechanism with another mark.
 *   active : W x H bytes, row-major like the mask: non-zero = trace this pixel as the call without a map does, zero = send no ray.
 * The three calls are the three above with that one argument more:
 *   * for every pixel of the rows the call owns, mask[p] = active[p] ? (the byte the call without a map writes) : 0.  Zero is
 *     "occluded" in the reference's polarity and "no unoccluded sample" for nsamples > 1; it IS written, so the mask is defined
 *     wherever the plain call defines it.  Rows outside the range / stripe are not touched.  The positions of an inactive pixel may
 *     hold anything (NaN included) and change no other pixel's byte.
 *   * active == NULL is exactly the call without a map (the same launch of the same kernel).
 *   * results never depend on an option.  An active trace honours "kernel" by FAMILY, one tile (or block) per workgroup: 0, 1, 2, 7
 *     (and -1 below 256 K pixels) run the lane-per-ray walk with work sharing over 16 x 16 blocks -- an inactive pixel's lane
 *     works on its neighbours' rays --, 3..6 the stackless packet over 8 x 8 tiles, 8 and 9 the wide packet when the stream has a
 *     private copy, else the stackless one.  A band of the stripes form is a multiple of 16 rows for the first family, of 8 for the
 *     others.  "soft_split", "packet_budget", "packet_share", "xcd_swizzle" and "row_order" apply as to the plain trace.
 *     A packet wave whose tile holds no active pixel stores its zeros and ends before it sets up a ray.
 *   * this version: an active trace ignores an installed split table, a planned or caller-set tile order, follow mode, "block_waves"
 *     and "wide_lane" (tables and orders were planned on the lives of full tiles), and records no wave statistics and no clock
 *     probe.  It never drops or alters any of them: the next plain trace uses them as before.
 *   * get-only option "active_traces": launches with a map so far; rts_ctx_last_kernel_name then names
 *     "shadowMaskActiveShareKernel", "shadowMaskActivePacketKernel<1>" or "shadowMaskActivePacketKernel<1,wide>".
 *   * the device forms are asynchronous, allocate nothing and read nothing back (capturable like the plain trace); the host form
 *     copies in, traces, copies out, synchronises.
 * include/rts_scene.h has a mark made from the G-buffer (rtsh_facing_active); INTEGRATION.md shows where a renderer writes it. */
int rts_trace_shadow_mask_active(rts_ctx* ctx, const rts_constants* constants, const rts_light* light, const float* positions,
                                 const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                 uint8_t* mask);
int rts_trace_shadow_mask_active_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light,
                                        const float* d_positions, const uint8_t* d_active, uint32_t W, uint32_t H,
                                        uint32_t row_begin, uint32_t row_end, uint8_t* d_mask, void* stream);
int rts_trace_shadow_mask_active_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light,
                                                const float* d_positions, const uint8_t* d_active, uint32_t W, uint32_t H,
                                                uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_mask,
                                                void* stream);

/* Generic rays (the shader's `Ray`): out[i] = 1 if ray i is NOT occluded.  Host / device forms. */
int rts_trace_rays(rts_ctx* ctx, const rts_ray* rays, size_t n, uint8_t* out);
int rts_trace_rays_device(rts_ctx* ctx, const rts_ray* d_rays, size_t n, uint8_t* d_out, void* stream);

/* OCCLUDER DISTANCE: the nearest blocker's ray parameter beside the shadow byte (hit distance for shadow denoisers, contact-
 * hardening penumbrae -- (1 - t) / t x light size for a point-light ray, which runs from the surface, t = 0, to the light, t = 1 --,
 * distance-based fading).
 * DEFINITION, exact: walk the node stream as intersectAny does (comp:75-111), same box test, same triangle test, but do not
 * return at a hit -- a leaf that hits goes on through its miss link like one that misses.  (The box test never looks at tmax,
 * comp:61-73, so the leaves visited do not depend on any hit.)  Every triangle the test accepts contributes c = (t > 0) ? t : +0,
 * t as intersectRayTri computes it (an accepted NaN or -0 counts as +0); distance = the minimum, +Inf (0x7F800000) if there is
 * none.  Equivalently: the smallest T >= +0 for which the reference's any-hit with tmax = min(T, the ray's tmax) reports a hit.
 * No box is culled against the best t so far (boxes and triangles round differently: a cull could change a bit), so an occluded
 * ray costs what a lit one costs.  Units are the ray parameter's: directional light = world distance along lightDirection as
 * given (tmax 1e9), point light = fraction of the segment surface -> light (tmax 1).
 *   rts_trace_rays_distance*: out_t[i] for generic ray i (n floats).
 *   rts_trace_shadow_distance*: the ray is the one rts_trace_shadow_mask* sets up (same bias, same light model).
 *     distance : W x H floats, row-major like the mask.  Every pixel of the rows the call owns is written: the ray's distance where
 *                the pixel is active, +0.0f where it is not.  Rows outside the range / stripe are not touched.
 *     active   : as in rts_trace_shadow_mask_active*, or NULL = every pixel.  Inactive positions may hold anything and change no
 *                other pixel.
 *     mask     : NULL, or W x H bytes that receive exactly what rts_trace_shadow_mask_active* writes -- so
 *                mask[p] == (distance[p] == +Inf) everywhere, inactive pixels (0, +0) included.
 *   * light->nsamples > 1 returns RTS_ERR_INVALID_ARG: several samples are rts_trace_soft_distance* (below).
 *   * the stripes form: as for the mask traces, a stripe that owns no band launches nothing, writes nothing and returns RTS_OK.
 *   * results never depend on an option.  "kernel" picks the FAMILY: 0, 1, 2, 7 (and -1 below 256 K pixels), and every wave that
 *     must take the exact path, run the lane-per-ray walk with work sharing (16 x 16 blocks; a stripe's band is then a multiple of
 *     16 rows); 3..6 (and -1 from 256 K pixels) the stackless packet over 8 x 8 tiles.  THIS VERSION: 8 and 9 run the stackless
 *     packet too -- the wide walk culls with a conservative test and confirms single hits; its distance form is a follow-up.
 *     Generic rays always run lane per ray.  "packet_budget", "packet_share", "xcd_swizzle" and "row_order" apply (speed only).
 *   * a distance trace ignores split tables, tile orders, follow mode, "block_waves", "wide_lane", wave statistics and the clock
 *     probe, and never drops or alters any of them.
 *   * the device forms are asynchronous, allocate nothing and read nothing back; under graph capture each adds ONE kernel node and
 *     nothing else, constants, light and options by value as for the mask traces.  The host forms copy in, trace, copy out.
 *   * get-only option "distance_traces": distance launches so far; rts_ctx_last_kernel_name then names "shadowDistanceShareKernel",
 *     "traceRaysDistanceKernel", or the packet instantiation launched: "shadowDistancePacketKernel<rows>" (a row range on a 2-D
 *     grid), "shadowDistancePacketKernel<bands>" (a stripe of power-of-two bands) or "shadowDistancePacketKernel<general>". */
int rts_trace_rays_distance(rts_ctx* ctx, const rts_ray* rays, size_t n, float* out_t);
int rts_trace_rays_distance_device(rts_ctx* ctx, const rts_ray* d_rays, size_t n, float* d_out_t, void* stream);
int rts_trace_shadow_distance(rts_ctx* ctx, const rts_constants* constants, const rts_light* light, const float* positions,
                              const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                              float* distance, uint8_t* mask);
int rts_trace_shadow_distance_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light,
                                     const float* d_positions, const uint8_t* d_active, uint32_t W, uint32_t H,
                                     uint32_t row_begin, uint32_t row_end, float* d_distance, uint8_t* d_mask, void* stream);
int rts_trace_shadow_distance_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light,
                                             const float* d_positions, const uint8_t* d_active, uint32_t W, uint32_t H,
                                             uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, float* d_distance,
                                             uint8_t* d_mask, void* stream);

/* SOFT-SHADOW OCCLUDER DISTANCE: the nearest blocker over ALL of an area light's samples, beside the count of unoccluded ones (what a
 * shadow denoiser and a contact-hardening penumbra estimate want of a soft shadow).  For pixel p and a light of n = nsamples in [2, 64]:
 *   sample j's ray is the one rts_trace_shadow_mask* sets up for (p, j): light position xyz + offsets[j], or with `table` != 0
 *   offsets[(start(p) + j) mod table] -- start(p) hashed from p's index y*W + x in the caller's FULL frame (rts_light.table);
 *   d_j = that ray's distance as defined above (OCCLUDER DISTANCE);
 *   distance[p] = min_j d_j -- every d_j is a bit pattern >= +0, so this is an integer minimum that does not depend on the order of
 *                 the samples; +Inf exactly when every sample is unoccluded;
 *   mask[p]     = #{ j : d_j == +Inf }: the byte rts_trace_shadow_mask_active* writes for the same light.
 * Hence mask[p] == n exactly where distance[p] == +Inf, and mask[p] < n exactly where it is finite.  Inactive pixels get +0.0f and 0,
 * and their positions are never looked at; rows outside the range / stripe are not touched.  active and mask may be NULL.
 * (The MEAN blocker distance is not offered: a float sum has no order-free definition -- DESIGN.md 4.13.)
 *   * nsamples 0 or 1 (or light == NULL) IS rts_trace_shadow_distance*: the same launch of the same kernel, the same bytes, counted
 *     by "distance_traces".  nsamples > 64, type > RTS_LIGHT_POINT, or a table outside nsamples <= table <= 64 with nsamples >= 2:
 *     RTS_ERR_INVALID_ARG.  (rts_trace_shadow_distance* itself keeps refusing nsamples > 1.)
 *   * results never depend on an option.  "kernel" picks the FAMILY as for a distance trace: 0, 1, 2, 7 (and -1 below 256 K pixels)
 *     the lane-per-ray walk over 16 x 16 blocks, the samples one after the other; 3..6, 8, 9 (and -1 from 256 K pixels) the stackless
 *     packet over 8 x 8 tiles -- with "soft_split" 1 (default) four waves per tile, wave w walking the samples w, w + 4, ..., their
 *     minima and counts joined in LDS; with 0 one wave walks every sample.  A stripe's band is a multiple of 16 rows for the first
 *     family, of 8 for the second; a stripe that owns no band launches nothing, writes nothing and returns RTS_OK.
 *   * like a distance trace it ignores split tables, tile orders, follow mode, "block_waves", "wide_lane", wave statistics and the
 *     clock probe, and never drops or alters any of them.
 *   * the device forms are asynchronous, allocate nothing and read nothing back; under graph capture each adds ONE kernel node,
 *     constants, light and options by value.  The host form copies in its rows only, traces, copies out.
 *   * get-only option "soft_distance_traces": soft distance launches so far ("distance_traces" does not move for them);
 *     rts_ctx_last_kernel_name then names "shadowSoftDistanceShareKernel" or "shadowSoftDistancePacketKernel<S,geom>", S = 4 or 1
 *     waves per tile, geom = rows, bands or general as for "shadowDistancePacketKernel". */
int rts_trace_soft_distance(rts_ctx* ctx, const rts_constants* constants, const rts_light* light, const float* positions,
                            const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                            float* distance, uint8_t* mask);
int rts_trace_soft_distance_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light,
                                   const float* d_positions, const uint8_t* d_active, uint32_t W, uint32_t H,
                                   uint32_t row_begin, uint32_t row_end, float* d_distance, uint8_t* d_mask, void* stream);
int rts_trace_soft_distance_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light,
                                           const float* d_positions, const uint8_t* d_active, uint32_t W, uint32_t H,
                                           uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, float* d_distance,
                                           uint8_t* d_mask, void* stream);

/* AMBIENT OCCLUSION: short segment rays from the surface over the hemisphere around the normal, the unoccluded ones counted -- the
 * any-hit walk of the shadow traces aimed by the G-buffer's normal instead of a light.  For pixel p of the rows the
 * call owns, N = normals[p].xyz, rel = positions[p].xyz, n = max(1, ao->nsamples):
 *   INACTIVE: N all zero (background), or active != NULL && active[p] == 0: counts[p] = 0, and the position is never read (NaN allowed).
 *   FRAME (Duff et al.'s branchless basis; every operation ONE rounded float operation, parenthesised as written, no contraction):
 *     sg = -1.0f if the sign bit of N.z is set, else 1.0f;   a = -1.0f / (sg + N.z);   b = (N.x * N.y) * a;
 *     T = (1.0f + (sg * (N.x * N.x)) * a,  sg * b,  -(sg * N.x));      B = (b,  sg + (N.y * N.y) * a,  -N.y)
 *   SAMPLE j < n: s = dirs[idx], idx = j with table == 0, else (start(p) + j) mod table -- start(p) hashed from p's index y*W + x in
 *     the caller's FULL frame exactly as for rts_light.table;  per component c:
 *     dir.c = ((T.c * s.x) + (B.c * s.y)) + (N.c * s.z);   o0.c = cam.c + rel.c;   L.c = o0.c + (radius * dir.c)
 *     the ray is the one rts_trace_shadow_mask* sets up at p for the hard point light { RTS_LIGHT_POINT, 1 sample, xyz = L }: the same
 *     bias, d = L - o, tmax = 1 -- a segment of about `radius` world units.  u_j = its any-hit byte (1: unoccluded).
 *   counts[p] = u_0 + ... + u_(n-1): a sum of bytes that are functions of (pixel, sample) alone, so no order of the samples, no deal
 *   over waves and no option can change it.  Any float is allowed in dirs (z <= 0 is legal: the rule defines the result).
 *   * RTS_ERR_INVALID_ARG, nothing written, no counter moved: NULL ao, normals, positions, counts or constants; nsamples >
 *     RTS_AO_MAX_SAMPLES; a table that is neither 0 nor in nsamples..RTS_AO_MAX_DIRS with nsamples >= 2; a radius that is Inf or NaN; a
 *     bad row range or band, as rts_trace_soft_distance* refuses them.
 *   * "kernel" picks the FAMILY as for a soft distance trace: the lane-per-ray walk over 16 x 16 blocks, samples in order, or the
 *     stackless packet over 8 x 8 tiles -- "soft_split" 1 (default): four waves per tile, wave w walking the samples w, w + 4, ...,
 *     their counts added in LDS; 0: one wave walks every sample.  A tile without an active non-background pixel stores its zeros and
 *     sets up no ray.  Bands: a multiple of 16 rows for the first family, of 8 for the second; a stripe that owns no band launches
 *     nothing, writes nothing and returns RTS_OK.
 *   * like the other block traces it ignores split tables, tile orders, follow mode, "block_waves", "wide_lane", wave statistics and
 *     the clock probe, and never drops or alters any of them.
 *   * the device forms are asynchronous, allocate nothing and read nothing back; under graph capture each adds ONE kernel node, `ao`,
 *     constants and options by value.  The host form copies in its rows only, traces, copies out.
 *   * get-only option "ao_traces": AO launches so far (no other trace counter moves); rts_ctx_last_kernel_name then names
 *     "ambientOcclusionShareKernel" or "ambientOcclusionPacketKernel<S,geom>", S = 4 or 1 waves per tile, geom = rows, bands or general.
 * The count plane is a soft list's plane of n samples to everything downstream: the filters, the moments pass and the upsample read it
 * under a one-entry rts_soft_light_list of the same nsamples (they read nothing else of a light when `distances` is NULL).
 * rtsh_ambient_occlusion (rts_scene.h) is the host twin, rtsh_ao_rays the same rays as rts_ray records for rts_trace_rays*. */
enum { RTS_AO_MAX_SAMPLES = 48, RTS_AO_MAX_DIRS = 64 };
typedef struct rts_ao_params {
    uint32_t nsamples;   /* 1..48 (0 counts as 1) */
    uint32_t table;      /* 0, or nsamples..64 with nsamples >= 2: per-pixel start as rts_light.table */
    float    radius;     /* finite; world units: the length of every AO segment */
    uint32_t reserved_;  /* ignored */
    float    dirs[64][4];/* tangent-space directions (x, y: tangent plane, z: along the normal); .w ignored */
} rts_ao_params;         /* 1040 bytes */
int rts_trace_ambient_occlusion(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao, const float* positions,
                                const float* normals, const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin,
                                uint32_t row_end, uint8_t* counts);
int rts_trace_ambient_occlusion_device(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao, const float* d_positions,
                                       const float* d_normals, const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t row_begin,
                                       uint32_t row_end, uint8_t* d_counts, void* stream);
int rts_trace_ambient_occlusion_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao,
                                               const float* d_positions, const float* d_normals, const uint8_t* d_active, uint32_t W,
                                               uint32_t H, uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_counts,
                                               void* stream);

/* ADAPTIVE AMBIENT OCCLUSION: a probe of a few AO samples per pixel, the remaining samples only where the probe disagrees -- inside
 * ONE dispatch, so the rays of open surface and of closed corners beyond the probe are never sent.  This is
 * rts_trace_ambient_occlusion*'s definition with rts_trace_shadow_mask_adaptive*'s decision on top.  For n = ao->nsamples in [2, 48],
 * a probe count k in [1, n - 1] and pixel p of the rows the call owns:
 *   u_j = sample j's any-hit byte exactly as AMBIENT OCCLUSION above defines it: the same frame, the same idx with or without a table,
 *   the same point light's ray at L;   c_k = u_0 + ... + u_(k-1),   c_n = u_0 + ... + u_(n-1);
 *   counts[p]  = 0    where p is inactive (N all zero, or active != NULL && active[p] == 0; the position is never read, NaN allowed),
 *                0    where c_k == 0,
 *                n    where c_k == k,
 *                c_n  otherwise;
 *   refined[p] = 1 exactly where the c_n case applied, else 0 (inactive pixels included).  refined may be NULL.
 * Hence counts[p] == rts_trace_ambient_occlusion's byte wherever refined[p] == 1, and elsewhere it is 0 or n.  A pixel whose probe is
 * unanimous although its full count is not keeps the probe's verdict: that is the quality cost of the call (a pixel with one or two
 * occluded samples of 16 often passes a probe of 4 as fully open), which is why it is a call of its own; a table makes neighbouring
 * pixels probe different directions.  All of it is integer counting of bytes that depend on (pixel, sample) alone, so no byte depends
 * on the kernel family, on "soft_split", on the order the samples are walked in or on any other option.  Rows outside the range /
 * stripe are not touched.
 *   * RTS_ERR_INVALID_ARG, nothing written, no counter moved: everything rts_trace_ambient_occlusion* refuses; nsamples < 2;
 *     probe == 0 or probe >= nsamples.
 *   * "kernel" picks the FAMILY as for an AO trace: the lane-per-ray walk over 16 x 16 blocks, each wave deciding for its own 8 x 8
 *     quarter, or the stackless packet over 8 x 8 tiles -- "soft_split" 1 (default): four waves per tile that deal the probe samples,
 *     join their counts in LDS, decide alike, and deal the remaining samples over the refining pixels; 0: one wave does both.  A tile
 *     without an active non-background pixel ends before a ray is set up; a tile without a refining pixel ends after its probe.  Bands:
 *     a multiple of 16 rows for the first family, of 8 for the second; a stripe that owns no band launches nothing, writes nothing
 *     and returns RTS_OK.
 *   * like the other block traces it ignores split tables, tile orders, follow mode, "block_waves", "wide_lane", wave statistics and
 *     the clock probe, and never drops or alters any of them.
 *   * the device forms are asynchronous, allocate nothing and read nothing back; under graph capture each adds ONE kernel node, `ao`,
 *     probe, constants and options by value.  The host form copies in its rows only, traces, copies out.
 *   * get-only option "ao_adaptive_traces": launches so far ("ao_traces" and "adaptive_traces" do not move for them);
 *     rts_ctx_last_kernel_name then names "ambientOcclusionAdaptiveShareKernel" or "ambientOcclusionAdaptivePacketKernel<S,geom>",
 *     S and geom as for "ambientOcclusionPacketKernel".
 * The plane is a count plane of n samples like rts_trace_ambient_occlusion's to everything downstream.
 * rtsh_ambient_occlusion_adaptive (rts_scene.h) is the host twin. */
int rts_trace_ambient_occlusion_adaptive(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao, const float* positions,
                                         const float* normals, const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin,
                                         uint32_t row_end, uint32_t probe, uint8_t* counts, uint8_t* refined);
int rts_trace_ambient_occlusion_adaptive_device(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao,
                                                const float* d_positions, const float* d_normals, const uint8_t* d_active, uint32_t W,
                                                uint32_t H, uint32_t row_begin, uint32_t row_end, uint32_t probe, uint8_t* d_counts,
                                                uint8_t* d_refined, void* stream);
int rts_trace_ambient_occlusion_adaptive_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao,
                                                        const float* d_positions, const float* d_normals, const uint8_t* d_active,
                                                        uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_stripes, uint32_t stripe,
                                                        uint32_t probe, uint8_t* d_counts, uint8_t* d_refined, void* stream);

/* BENT NORMALS: the AO trace with the DIRECTION the hemisphere is open in beside the count -- per pixel the frame applied to the sum of
 * the unoccluded samples' directions, what an ambient term lit from a sky or an environment is aimed by.  The rays
 * are rts_trace_ambient_occlusion*'s own.  For pixel p of the rows the call owns, u_j, idx(p, j), N, T and B are exactly those of
 * AMBIENT OCCLUSION above, n = max(1, ao->nsamples):
 *   Q(v)  = 0 if v is NaN, else (int32) rint(min(max(v, -1.0f), 1.0f) * 16384.0f): the product is exact, ties round to even,
 *           infinities clamp to +-16384;
 *   q_j   = (Q(s.x), Q(s.y), Q(s.z)) for s = dirs[idx(p, j)]: a function of the table entry alone;
 *   S     = sum over j of u_j * q_j, an INTEGER vector;  c = sum u_j, the AO trace's byte;  |S.c| <= 48 * 16384 < 2^24;
 *   f     = ((float)S.x * 0x1p-14f, (float)S.y * 0x1p-14f, (float)S.z * 0x1p-14f): both steps exact;
 *   bent[p].c = ((T.c * f.x) + (B.c * f.y)) + (N.c * f.z) per component c of xyz, each operation ONE rounded float operation, no
 *           contraction;   bent[p].w = (float)c.
 *   INACTIVE (N all zero, or active != NULL && active[p] == 0): counts[p] = 0, bent[p] = (+0, +0, +0, +0); the position is never read.
 * WHY THE SUM IS TAKEN IN TANGENT SPACE: the frame is linear, so the sum of the samples' world directions IS the frame applied to the
 * sum of their tangent-space directions -- but only the latter can be added over integers.  Summing per-sample world directions in
 * float would make the result depend on the order the samples are walked in and on which wave walked which; integer addition is
 * associative, so S is as order-free as the count is, and the frame meets it ONCE, in the written order.  Hence no byte of `bent` or
 * `counts` depends on the kernel family, on "soft_split" or on any other option.  (An active pixel with c == 0 gets the frame applied
 * to the zero vector: every component is a zero, whose sign is the written operations' -- -0 where all three products are -0.)
 * The vector is NOT normalised: its length over c says how narrow the open cone is; rtsh_combine_visibility_list_ao_bent normalises.
 * `bent`: W x H RGBA32F, required.  `counts`: W x H bytes or NULL; where given it is byte for byte the plane
 * rts_trace_ambient_occlusion* writes.  Rows outside the range / stripe are not touched in either plane.
 *   * RTS_ERR_INVALID_ARG, nothing written, no counter moved: everything rts_trace_ambient_occlusion* refuses except NULL counts; NULL
 *     bent.
 *   * families, "soft_split", bands, the ignored options and the behaviour under capture are rts_trace_ambient_occlusion*'s: ONE
 *     kernel node per call, `ao`, constants and options by value; the four waves of a tile add their integer words in LDS.
 *   * get-only option "ao_bent_traces": launches so far ("ao_traces" and "ao_adaptive_traces" do not move for them);
 *     rts_ctx_last_kernel_name then names "ambientOcclusionBentShareKernel" or "ambientOcclusionBentPacketKernel<S,geom>", S and
 *     geom as for "ambientOcclusionPacketKernel".
 * rtsh_ambient_occlusion_bent (rts_scene.h) is the host twin. */
int rts_trace_ambient_occlusion_bent(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao, const float* positions,
                                     const float* normals, const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin,
                                     uint32_t row_end, uint8_t* counts, float* bent);
int rts_trace_ambient_occlusion_bent_device(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao,
                                            const float* d_positions, const float* d_normals, const uint8_t* d_active, uint32_t W,
                                            uint32_t H, uint32_t row_begin, uint32_t row_end, uint8_t* d_counts, float* d_bent,
                                            void* stream);
int rts_trace_ambient_occlusion_bent_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao,
                                                    const float* d_positions, const float* d_normals, const uint8_t* d_active,
                                                    uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_stripes, uint32_t stripe,
                                                    uint8_t* d_counts, float* d_bent, void* stream);

/* AO DISTANCE AND FALLOFF: the AO trace with the NEAREST BLOCKER over the hemisphere and a WEIGHTED obscurance beside the count -- a
 * blocker at 99 % of the radius no longer darkens a pixel as much as one at 1 %, and the hit distance is there for the denoiser and
 * for contact darkening.  The rays, the frame, idx(p, j) and INACTIVE are word for word those of AMBIENT OCCLUSION
 * above.  For pixel p of the rows the call owns, n = max(1, ao->nsamples):
 *   d_j   = the OCCLUDER DISTANCE of sample j's ray as defined above: the walk does not return at a hit; the smallest accepted t as a
 *           bit pattern >= +0, +Inf if there is none.  The ray is the point light's segment, so t is the fraction of the segment from
 *           the surface (0) to L (1);
 *   u_j   = (d_j == +Inf);   c = sum u_j;   counts[p] = c, byte for byte the plane of rts_trace_ambient_occlusion*;
 *   distance[p] = min_j d_j, an integer minimum of bit patterns as in SOFT-SHADOW OCCLUDER DISTANCE; +Inf exactly where c == n;
 *   b_j   = min(63u, (uint32_t)(min(d_j, 1.0f) * 64.0f)) for a blocked sample: the product is exact, the conversion truncates;
 *   a_j   = 255 where u_j, else falloff->weight[b_j]: weight[b] says how OPEN a sample counts whose nearest blocker lies in the b-th
 *           64th of the segment -- 0 a full occluder, 255 no occlusion.  A falloff rises with b, but any bytes are legal;
 *   A     = sum a_j, an integer <= 48 * 255;   S = 65535 / n by integer division (the wide filter's S_l, rts_scene.h);
 *   obscurance[p] = (2 * A * S + 255) / 510, an integer quotient: the intermediate stays below 2^26, the value never exceeds n * S.
 *   INACTIVE: counts[p] = 0, distance[p] = +0.0f, obscurance[p] = 0, and the position is never read.  Rows outside the range / stripe
 *   are not touched in any plane.
 * Every quantity that crosses samples is an integer sum or an integer minimum of functions of (pixel, sample) alone -- a weighted sum of
 * float distances would have no order-free definition; a sum of integer weights looked up from a QUANTISED distance
 * has one --, so no byte depends on the kernel family, on "soft_split", on the order of the samples or on any option.
 * ANCHORS: (1) counts is the AO trace's plane, and distance is finite exactly where counts < n.  (2) weight all 0: obscurance ==
 * counts * S, the wide filter's V_0 of the count plane.  (3) weight all 255: obscurance == n * S at every active pixel.
 * (4) obscurance >= counts * S always, and raising any weight[b] never lowers any pixel.  (5) n == 1: distance is bit for bit what
 * rts_trace_shadow_distance* gives at that pixel for the hard point light at L.
 * DOWNSTREAM: obscurance IS a plane in the wide filter's fixed point: it goes into rtsh_wide_filter_mean_soft_light_list* as `mean`
 * under a one-entry rts_soft_light_list of n samples without a conversion pass; passes == 0 gives the float plane V / (n S) that
 * rtsh_combine_visibility_list_ao* and rtsh_accumulate_visibility_list* take.  Nothing downstream changes.
 * counts, distance (W x H floats) and obscurance (W x H uint16_t) may each be NULL, but at least one of distance and obscurance is
 * given; falloff may be NULL only when obscurance is (it is not read then).
 *   * RTS_ERR_INVALID_ARG, nothing written, no counter moved: everything rts_trace_ambient_occlusion* refuses except NULL counts; both
 *     outputs NULL; obscurance without falloff; an obscurance pointer that is not 2-byte aligned; a distance pointer that is not
 *     4-byte aligned.
 *   * families, "soft_split", bands, stripes and the ignored options are rts_trace_ambient_occlusion*'s; under graph capture a call is
 *     ONE kernel node, `ao`, `falloff`, constants and options by value; the four waves of a tile join their integer words in LDS.
 *   * get-only option "ao_distance_traces": launches so far (no other counter moves); rts_ctx_last_kernel_name then names
 *     "ambientOcclusionDistanceShareKernel" or "ambientOcclusionDistancePacketKernel<S,geom>", S and geom as for
 *     "ambientOcclusionPacketKernel".
 * A distance walk never stops at its first hit: where neither plane is wanted, stay with rts_trace_ambient_occlusion*.
 * rtsh_ambient_occlusion_distance (rts_scene.h) is the host twin. */
typedef struct rts_ao_falloff { uint8_t weight[64]; } rts_ao_falloff;   /* 64 bytes */
int rts_trace_ambient_occlusion_distance(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao,
                                         const rts_ao_falloff* falloff, const float* positions, const float* normals,
                                         const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                         uint8_t* counts, float* distance, uint16_t* obscurance);
int rts_trace_ambient_occlusion_distance_device(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao,
                                                const rts_ao_falloff* falloff, const float* d_positions, const float* d_normals,
                                                const uint8_t* d_active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                                uint8_t* d_counts, float* d_distance, uint16_t* d_obscurance, void* stream);
int rts_trace_ambient_occlusion_distance_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_ao_params* ao,
                                                        const rts_ao_falloff* falloff, const float* d_positions,
                                                        const float* d_normals, const uint8_t* d_active, uint32_t W, uint32_t H,
                                                        uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_counts,
                                                        float* d_distance, uint16_t* d_obscurance, void* stream);

/* LIGHT LISTS: up to 8 hard lights in ONE dispatch, one bit per light in the mask byte -- one read of the G-buffer texel, one launch and
 * one mask plane for all of a frame's shadow-casting lights.  For pixel p of the rows the call owns and l < list->count:
 *   mask[p] bit l = (lights_map == NULL || (lights_map[p] >> l) & 1)
 *                   ? the byte rts_trace_shadow_mask* writes at p for the hard light { lights[l].type, nsamples 1, lights[l].xyz } alone
 *                   : 0
 *   bits l >= count are 0, whatever the map holds.  Directional and point lights may be mixed in one list.
 * So bit l equals rts_trace_shadow_mask_active* for light l alone with active[p] = bit l of lights_map[p], byte for byte.  Every pixel
 * of the owned rows is written; a pixel whose map byte has no bit below count gets 0, its position is never looked at (NaN allowed)
 * and changes no other pixel; rows outside the range / stripe are not touched.  The result does not depend on the order the lights
 * are walked in nor on which wave walked which: bits are joined by an integer OR.
 *   * lights_map: NULL, or W x H bytes (rtsh_facing_lights* makes the one a deferred renderer wants: bit l = the surface faces light l).
 *   * list == NULL, count == 0, count > RTS_MAX_LIST_LIGHTS or a type > RTS_LIGHT_POINT: RTS_ERR_INVALID_ARG, nothing written.
 *     reserved_ is ignored.  Hard lights only (soft lights in a list: rts_trace_soft_light_list* below).
 *   * results never depend on an option.  "kernel" picks the FAMILY as for a distance trace: 0, 1, 2, 7 (and -1 below 256 K pixels) the
 *     lane-per-ray walk over 16 x 16 blocks, the lights one after the other; 3..6, 8, 9 (and -1 from 256 K pixels) the stackless packet
 *     over 8 x 8 tiles -- with "soft_split" 1 (default) four waves per tile, wave w walking the lights w and w + 4, their bytes ORed in
 *     LDS; with 0 one wave walks every light.  8 and 9 run the stackless packet too in this version: the wide walk's segment form is
 *     chosen at compile time per light type and a list mixes types (the wide form is a follow-up).  A stripe's band is a multiple of 16
 *     rows for the first family, of 8 for the second; a stripe that owns no band launches nothing, writes nothing and returns RTS_OK.
 *     "packet_budget", "packet_share", "xcd_swizzle" and "row_order" apply, for speed only.
 *   * a light no pixel of a wave's tile is marked for costs that wave nothing: it is skipped before any ray is set up.
 *   * like a distance trace it ignores split tables, tile orders, follow mode, "block_waves", "wide_lane", wave statistics and the
 *     clock probe, and never drops or alters any of them.
 *   * the device forms are asynchronous, allocate nothing and read nothing back; under graph capture each adds ONE kernel node,
 *     constants, list and options by value.  The host form copies in its rows only, traces, copies out and synchronises.
 *   * get-only option "light_list_traces": list launches so far ("active_traces", "distance_traces" and "soft_distance_traces" do not
 *     move for them); rts_ctx_last_kernel_name then names "shadowLightListShareKernel" or "shadowLightListPacketKernel<S,geom>",
 *     S = 4 or 1 waves per tile, geom = rows, bands or general as for "shadowSoftDistancePacketKernel". */
enum { RTS_MAX_LIST_LIGHTS = 8 };
typedef struct rts_light_entry { uint32_t type; float xyz[3]; } rts_light_entry;   /* 16 bytes; type, xyz as in rts_light, one sample */
typedef struct rts_light_list {
    uint32_t count;
    uint32_t reserved_[3];
    rts_light_entry lights[RTS_MAX_LIST_LIGHTS];
} rts_light_list;                                                                  /* 144 bytes */
int rts_trace_light_list(rts_ctx* ctx, const rts_constants* constants, const rts_light_list* list, const float* positions,
                         const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, uint8_t* mask);
int rts_trace_light_list_device(rts_ctx* ctx, const rts_constants* constants, const rts_light_list* list, const float* d_positions,
                                const uint8_t* d_lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                uint8_t* d_mask, void* stream);
int rts_trace_light_list_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_light_list* list,
                                        const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                        uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_mask, void* stream);

/* ADAPTIVE SOFT SHADOWS: a probe of a few samples per pixel, the remaining samples only where the probe disagrees -- inside ONE
 * dispatch, so the rays of the umbra and of the fully lit area beyond the probe are never sent.  For a light of n = nsamples in
 * [2, 64], a probe count k in [1, n - 1] and pixel p of the rows the call owns:
 *   sample j's ray is the one rts_trace_shadow_mask* sets up for (p, j) of THIS light: light position xyz + offsets[j], or with
 *   `table` != 0 offsets[(start(p) + j) mod table] -- start(p) hashed from p's index y*W + x in the caller's FULL frame;
 *   u_j in {0, 1} = that sample's any-hit byte (1: unoccluded);  c_k = u_0 + ... + u_(k-1),  c_n = u_0 + ... + u_(n-1) -- c_n is
 *   the byte the soft mask trace writes;
 *   mask[p]    = 0    where active[p] == 0 (the position is never looked at: NaN allowed),
 *                0    where c_k == 0,
 *                n    where c_k == k,
 *                c_n  otherwise;
 *   refined[p] = 1 exactly where the c_n case applied, else 0 (inactive pixels included).
 * Hence mask[p] == c_n wherever refined[p] == 1, and elsewhere mask[p] is 0 or n: a value the full trace could have written for a
 * unanimous pixel.  A pixel whose probe is unanimous although its full count is not keeps the probe's verdict: that is the quality
 * cost, and what the per-pixel table is for (neighbouring pixels probe different points of the light).  All of it is integer counting
 * of bytes that depend on (pixel, sample) alone, so the result does not depend on the order of the samples, on which wave walked which,
 * or on any option.  Rows outside the range / stripe are not touched.  active and refined may be NULL.
 *   * light == NULL, nsamples < 2 or > 64, type > RTS_LIGHT_POINT, a table outside nsamples <= table <= 64, probe == 0 or
 *     probe >= nsamples: RTS_ERR_INVALID_ARG, nothing written.
 *   * "kernel" picks the FAMILY as for a distance trace: 0, 1, 2, 7 (and -1 below 256 K pixels) the lane-per-ray walk over 16 x 16
 *     blocks, each wave deciding for its own 8 x 8 quarter; 3..6, 8, 9 (and -1 from 256 K pixels) the stackless packet over 8 x 8
 *     tiles -- with "soft_split" 1 (default) four waves per tile that deal the probe samples, join their counts in LDS, decide alike,
 *     and deal the remaining samples over the penumbra pixels; with 0 one wave does both.  A stripe's band is a multiple of 16 rows for
 *     the first family, of 8 for the second; a stripe that owns no band launches nothing, writes nothing and returns RTS_OK.
 *     "packet_budget", "packet_share", "xcd_swizzle" and "row_order" apply, for speed only.
 *   * a tile without an active pixel ends before a ray is set up; a tile without a penumbra pixel ends after its probe.
 *   * like a distance trace it ignores split tables, tile orders, follow mode, "block_waves", "wide_lane", wave statistics and the
 *     clock probe, and never drops or alters any of them.
 *   * the device forms are asynchronous, allocate nothing and read nothing back; under graph capture each adds ONE kernel node,
 *     constants, light, probe and options by value.  The host form copies in its rows only, traces, copies out and synchronises.
 *   * get-only option "adaptive_traces": adaptive launches so far ("active_traces", "distance_traces", "soft_distance_traces" and
 *     "light_list_traces" do not move for them); rts_ctx_last_kernel_name then names "shadowMaskAdaptiveShareKernel" or
 *     "shadowMaskAdaptivePacketKernel<S,geom>", S = 4 or 1 waves per tile, geom = rows, bands or general as for
 *     "shadowSoftDistancePacketKernel". */
int rts_trace_shadow_mask_adaptive(rts_ctx* ctx, const rts_constants* constants, const rts_light* light, const float* positions,
                                   const uint8_t* active, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end,
                                   uint32_t probe, uint8_t* mask, uint8_t* refined);
int rts_trace_shadow_mask_adaptive_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light,
                                          const float* d_positions, const uint8_t* d_active, uint32_t W, uint32_t H,
                                          uint32_t row_begin, uint32_t row_end, uint32_t probe, uint8_t* d_mask, uint8_t* d_refined,
                                          void* stream);
int rts_trace_shadow_mask_adaptive_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_light* light,
                                                  const float* d_positions, const uint8_t* d_active, uint32_t W, uint32_t H,
                                                  uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint32_t probe,
                                                  uint8_t* d_mask, uint8_t* d_refined, void* stream);

/* SOFT LIGHT LISTS: up to 8 lights, each hard or soft, in ONE dispatch, one COUNT PLANE per light -- one read of the G-buffer texel,
 * one launch and one light map for all of a frame's area lights.  The lights share one table of RTS_SOFT_LIST_OFFSETS sample offsets;
 * light l uses the nsamples entries from `first` on, scaled by its radius (ranges may overlap or coincide).  For pixel p of the rows
 * the call owns and l < list->count, light l stands for the derived rts_light
 *   { type, nsamples, xyz, table 0, offsets'[j][c] = radius * offsets[first + j][c] }       (j < nsamples, c < 3)
 * -- the product ONE rounded float multiply per component, which the set-up then adds to xyz as for any rts_light (the library is
 * built without FMA contraction, so the product is never fused into that add; radius 1.0f gives the table's entries themselves) -- and
 *   counts[l * W * H + p] = (lights_map == NULL || (lights_map[p] >> l) & 1)
 *                           ? the byte rts_trace_shadow_mask_active* writes at p for that derived light alone
 *                           : 0
 * So plane l lies in 0 .. max(1, nsamples_l): the number of unoccluded samples.  A hard entry (nsamples 0 or 1) ignores first, radius
 * and the table in what it computes: its plane is bit l of rts_trace_light_list* for { type, xyz }, as 0 or 1.  Planes l >= count are
 * never touched; rows outside the range / stripe are not touched in any plane.  A pixel whose map byte has no bit below count gets 0
 * in every plane, its position is never looked at (NaN allowed) and changes no other pixel.  The per-pixel jitter table
 * (rts_light.table) is offered by rts_trace_soft_light_list_jittered* below, not by these calls.  A count is a sum of bytes that depend on (pixel, light, sample) alone:
 * no order of the pairs, no deal over waves and no option can change a byte.
 *   * counts: count * W * H bytes, plane l at counts + l * W * H.  lights_map: NULL, or W x H bytes (rtsh_facing_lights* makes it from
 *     the rts_light_list of the same types and positions).
 *   * RTS_ERR_INVALID_ARG, nothing written, no counter moved: list == NULL, count == 0 or > RTS_MAX_LIST_LIGHTS, a type >
 *     RTS_LIGHT_POINT, nsamples > RTS_SOFT_LIST_OFFSETS, nsamples >= 2 with first + nsamples > RTS_SOFT_LIST_OFFSETS, a radius that is
 *     not finite (in any entry, also a hard one), counts == NULL, a bad row range or a bad band as rts_trace_light_list* refuses them.
 *     reserved_ is ignored.
 *   * results never depend on an option.  "kernel" picks the FAMILY as for a light list: 0, 1, 2, 7 (and -1 below 256 K pixels) the
 *     lane-per-ray walk over 16 x 16 blocks, lights in order and samples in order; 3..6, 8, 9 (and -1 from 256 K pixels) the stackless
 *     packet over 8 x 8 tiles -- with "soft_split" 1 (default) four waves per tile: the (light, sample) PAIRS of the list, flattened in
 *     list order, are dealt r = w, w + 4, ... over the waves, so a list of many small lights and a list of one large light both keep
 *     four waves busy; the waves' counts are joined in LDS.  With 0 one wave walks every pair.  8 and 9 run the stackless packet too.
 *     A stripe's band is a multiple of 16 rows for the first family, of 8 for the second; a stripe that owns no band launches nothing,
 *     writes nothing and returns RTS_OK.  "packet_budget", "packet_share", "xcd_swizzle" and "row_order" apply, for speed only.
 *   * a light no pixel of a wave's tile is marked for costs that wave nothing: it is skipped before any ray is set up.
 *   * like the other block traces it ignores split tables, tile orders, follow mode, "block_waves", "wide_lane", wave statistics and
 *     the clock probe, and never drops or alters any of them.
 *   * the device forms are asynchronous, allocate nothing and read nothing back; under graph capture each adds ONE kernel node,
 *     constants, list and options by value.  The host form copies in its rows only, traces, copies out and synchronises.
 *   * get-only option "soft_light_list_traces": soft list launches so far (no other counter moves for them); rts_ctx_last_kernel_name
 *     then names "shadowSoftLightListShareKernel" or "shadowSoftLightListPacketKernel<S,geom>", S = 4 or 1 waves per tile, geom =
 *     rows, bands or general as for "shadowSoftDistancePacketKernel". */
enum { RTS_SOFT_LIST_OFFSETS = 48 };
typedef struct rts_soft_light_entry {      /* 32 bytes */
    uint32_t type;       /* RTS_LIGHT_DIRECTIONAL / RTS_LIGHT_POINT */
    uint32_t nsamples;   /* 0 or 1 = hard; 2..48 = soft */
    uint32_t first;      /* first entry of offsets[] this light uses; first + nsamples <= 48 when nsamples >= 2 */
    float    radius;     /* scales the shared offsets for this light */
    float    xyz[3];
    uint32_t reserved_;  /* ignored */
} rts_soft_light_entry;
typedef struct rts_soft_light_list {
    uint32_t count;                       /* 1..RTS_MAX_LIST_LIGHTS */
    uint32_t reserved_[3];                /* ignored */
    rts_soft_light_entry lights[RTS_MAX_LIST_LIGHTS];
    float offsets[RTS_SOFT_LIST_OFFSETS][4];   /* one sample table shared by all lights; ranges may overlap */
} rts_soft_light_list;                                                             /* 1040 bytes */
int rts_trace_soft_light_list(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list, const float* positions,
                              const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, uint8_t* counts);
int rts_trace_soft_light_list_device(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                     const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                                     uint32_t row_end, uint8_t* d_counts, void* stream);
int rts_trace_soft_light_list_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                             const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                             uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_counts, void* stream);

/* SPARSE LIGHT LISTS: the two list traces over a LIST of pixels instead of a row range -- for a mark that sets few bits (the retrace
 * map of a half-resolution list, rts_scene.h; spot cones, light range, stencilled regions).  The block traces give a wave one 8 x 8
 * tile, so a tile that holds ONE marked pixel costs a wave; here lane i of the launch owns entry i of the list (rtsh_compact_light_map*
 * makes it from a map), 64 marked pixels per wave.  The arguments are those of rts_trace_soft_light_list_device and
 * rts_trace_light_list_device without row range and stripes; in their place d_pixels (32-bit pixel indices y * W + x), d_n (ONE
 * 32-bit word: the list's length) -- both ON THE DEVICE, read by the kernel, never read back -- and capacity (the entries d_pixels
 * has room for).  The host forms take pixels and n from host memory.
 *   Take every entry p = pixels[i] with i < min(*d_n, capacity) and p < W * H, and every l < count with on(p, l): lights_map == NULL
 *   or bit l of lights_map[p] set.
 *     soft list: counts[l * W * H + p] is the byte rts_trace_soft_light_list* writes there under the same map;
 *     hard list: bit l of mask[p] is the bit rts_trace_light_list* writes; the other bits of that byte keep what they held (the byte is
 *                read, changed and stored by the one lane that owns the entry).
 *   EVERY OTHER BYTE of the planes is NOT TOUCHED: pixels not listed, pairs whose bit is clear, planes from count up.  That is what
 *   rtsh_upsample_*_light_list* with `keep` expects in front of it.  An entry of W * H or above is skipped: nothing is read or written
 *   for it.  A list that names a pixel twice gives the same bytes.  A listed pixel's position is read; an unlisted one's never is (NaN
 *   allowed).  The result depends on no option and not on the order of the list: each byte is a function of (pixel, light, sample)
 *   alone.
 *   * RTS_ERR_INVALID_ARG, nothing written, no counter moved: what rts_trace_soft_light_list* / rts_trace_light_list* refuse of the
 *     list, the planes and the frame; NULL pixels or n; capacity 0.  Behind those, without a BVH: RTS_ERR_NO_BVH.
 *   * ONE kernel, the lane-per-ray walk with work sharing of "shadowSoftLightListShareKernel" / "shadowLightListShareKernel" -- lights in
 *     order, samples in order, the same ray set-up, so every ray has the same bits -- launched as ceil(capacity / 256) workgroups of
 *     four waves; a wave whose first entry lies at or beyond min(*d_n, capacity) leaves at once.  Every exit is wave-uniform, there is
 *     no workgroup barrier.  "kernel", "soft_split" and every other option choose nothing here.
 *   * FROM WHAT SHARE OF MARKED PIXELS the masked block trace is the better call: AT EVERY SHARE MEASURED, 0.06 % to 66 % of the frame
 *     (DESIGN.md 4.33's tables, MI355X, one run): compaction plus the sparse trace took 1.5-5.3 times the masked trace on retrace maps
 *     of 0.06-0.54 % and 1.9-2.7 times on dense maps.  The list's few waves each walk lights x samples rays one after the other with the
 *     lane-per-ray walk; the masked packet trace opens more tiles but its waves are short and many.  These calls are exact and kept for
 *     marks and walks to come; today rts_trace_*_light_list* under the map is the faster call.
 *   * the device forms are asynchronous, allocate nothing and read nothing back; under graph capture each adds ONE kernel node --
 *     constants, list, options and capacity by value, the POINTERS d_pixels and d_n captured: a replay traces whatever list the buffers
 *     hold then.  The host forms copy in the frame, the caller's planes and the list, trace, copy out the planes and synchronise; n == 0
 *     is RTS_OK and nothing is copied.
 *   * get-only option "sparse_list_traces": launches of either kernel so far (no other counter moves for them);
 *     rts_ctx_last_kernel_name then names "shadowSoftLightListSparseKernel" or "shadowLightListSparseKernel".
 *   * OUT OF SCOPE: the distance, adaptive and jittered forms; row ranges and stripes. */
int rts_trace_light_list_sparse(rts_ctx* ctx, const rts_constants* constants, const rts_light_list* list, const float* positions,
                                const uint8_t* lights_map, uint32_t W, uint32_t H, const uint32_t* pixels, uint32_t n, uint8_t* mask);
int rts_trace_light_list_sparse_device(rts_ctx* ctx, const rts_constants* constants, const rts_light_list* list, const float* d_positions,
                                       const uint8_t* d_lights_map, uint32_t W, uint32_t H, const uint32_t* d_pixels, const uint32_t* d_n,
                                       uint32_t capacity, uint8_t* d_mask, void* stream);
int rts_trace_soft_light_list_sparse(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list, const float* positions,
                                     const uint8_t* lights_map, uint32_t W, uint32_t H, const uint32_t* pixels, uint32_t n,
                                     uint8_t* counts);
int rts_trace_soft_light_list_sparse_device(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                            const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                            const uint32_t* d_pixels, const uint32_t* d_n, uint32_t capacity, uint8_t* d_counts,
                                            void* stream);

/* SOFT LIGHT LIST DISTANCE: a soft light list with the NEAREST BLOCKER per light beside its count -- one DISTANCE PLANE per light, what
 * contact-hardening penumbrae, a distance-guided denoiser or a distance fade want of several area lights, without one
 * rts_trace_soft_distance* dispatch per light.  The arguments are those of rts_trace_soft_light_list*, with `distances` in front of
 * `counts`.  For pixel p of the rows the call owns and l < list->count, with the derived rts_light of entry l as defined above
 * (SOFT LIGHT LISTS) and on = (lights_map == NULL || (lights_map[p] >> l) & 1):
 *   distances[l * W * H + p] = on ? the float rts_trace_soft_distance* writes at p for that derived light alone -- the minimum over the
 *                                   light's samples of the one-ray distance (SOFT-SHADOW OCCLUDER DISTANCE), +Inf exactly when every
 *                                   sample is unoccluded; a hard entry (nsamples 0 or 1) gives the one-ray distance of
 *                                   rts_trace_shadow_distance*, its ray aimed at xyz as given
 *                                 : +0.0f
 *   counts[l * W * H + p]    = byte for byte what rts_trace_soft_light_list* writes.
 * Hence, where on, counts == max(1, nsamples_l) exactly where the distance is +Inf.  Planes l >= count are never touched in either
 * output; rows outside the range / stripe are not touched in any plane.  A pixel whose map byte has no bit below count gets +0.0f and 0
 * in every plane, its position is never looked at (NaN allowed) and changes no other pixel.  Every one-ray distance is a bit pattern
 * >= +0 whose unsigned order is the float order, so a light's minimum is an integer minimum per (pixel, light) and its count an integer
 * sum: no order of the pairs, no deal over waves and no option can change a bit.  The per-pixel jitter table and
 * probes are not offered here, nor is the MEAN blocker distance.
 *   * distances: count * W * H floats, plane l at distances + l * W * H.  counts: NULL, or count * W * H bytes.  lights_map as above.
 *   * RTS_ERR_INVALID_ARG, nothing written, no counter moved: everything rts_trace_soft_light_list* refuses of the list, the row range,
 *     the band and the stripe; distances == NULL.
 *   * results never depend on an option.  "kernel" picks the FAMILY as for a soft light list: 0, 1, 2, 7 (and -1 below 256 K pixels)
 *     the lane-per-ray walk over 16 x 16 blocks, lights in order and samples in order; 3..6, 8, 9 (and -1 from 256 K pixels) the
 *     stackless packet over 8 x 8 tiles -- with "soft_split" 1 (default) four waves per tile that deal the (light, sample) pairs as the
 *     soft light list does and join their minima and counts in LDS, with 0 one wave walks every pair.  A stripe's band is a multiple of
 *     16 rows for the first family, of 8 for the second; a stripe that owns no band launches nothing, writes nothing and returns
 *     RTS_OK.  "packet_budget", "packet_share", "xcd_swizzle" and "row_order" apply, for speed only.
 *   * a light no pixel of a wave's tile is marked for costs that wave nothing: it is skipped before any ray is set up.  Unlike the
 *     counts alone, a distance needs every accepted triangle of every sample: no walk ends at its first hit.
 *   * like the other block traces it ignores split tables, tile orders, follow mode, "block_waves", "wide_lane", wave statistics and
 *     the clock probe, and never drops or alters any of them.
 *   * the device forms are asynchronous, allocate nothing and read nothing back; under graph capture each adds ONE kernel node,
 *     constants, list and options by value.  The host form copies in its rows only, traces, copies out both outputs and synchronises.
 *   * get-only option "soft_list_distance_traces": launches so far (no other counter moves for them); rts_ctx_last_kernel_name then
 *     names "shadowSoftLightListDistanceShareKernel" or "shadowSoftLightListDistancePacketKernel<S,geom>", S = 4 or 1 waves per tile,
 *     geom = rows, bands or general as for "shadowSoftDistancePacketKernel". */
int rts_trace_soft_light_list_distance(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                       const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                                       uint32_t row_end, float* distances, uint8_t* counts);
int rts_trace_soft_light_list_distance_device(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                              const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                              uint32_t row_begin, uint32_t row_end, float* d_distances, uint8_t* d_counts, void* stream);
int rts_trace_soft_light_list_distance_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                                      const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                                      uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, float* d_distances,
                                                      uint8_t* d_counts, void* stream);

/* ADAPTIVE SOFT LIGHT LISTS: a soft light list with a probe count per light -- the two traces above joined inside ONE dispatch: every
 * light's probe is walked first, and a light's remaining samples only over the pixels whose probe of THAT light disagrees.  The
 * arguments are those of rts_trace_soft_light_list*, plus `probes` (list->count entries on the host, read by value at the call, under
 * graph capture too) and the optional plane `refined`.  With n_l = max(1, nsamples_l) and k_l = probes[l], for pixel p of the rows
 * the call owns and l < list->count:
 *   k_l == 0            light l is traced in full: counts[l * W * H + p] is byte for byte what rts_trace_soft_light_list* writes, and
 *                       bit l of refined[p] is 0.
 *   1 <= k_l <= n_l - 1 (only a soft entry has such a k) counts[l * W * H + p] is the byte rts_trace_shadow_mask_adaptive* writes at p
 *                       for the derived light of entry l (above: xyz + radius * offsets[first + j], table 0) with probe k_l and the
 *                       active byte (lights_map == NULL ? 1 : (lights_map[p] >> l) & 1); bit l of refined[p] is that call's refined
 *                       byte.
 * refined is ONE plane of W * H bytes for the whole list (NULL: not wanted): bit l set exactly where light l took its full count; bits
 * at and above count are 0.  A pixel whose map byte has no bit below count gets 0 in refined and in every plane; its position is never
 * looked at (NaN allowed).  Planes at and above count, and rows outside the range / stripe, are not touched in counts or in refined.
 * Every byte is integer counting of bytes that depend on (pixel, light, sample) alone: no order of the pairs, no deal over waves and no
 * option can change one.  The per-pixel jitter table: rts_trace_soft_light_list_jittered* below.
 *   * RTS_ERR_INVALID_ARG, nothing written, no counter moved: everything rts_trace_soft_light_list* refuses; probes == NULL;
 *     probes[l] >= n_l for any l < count -- a hard entry therefore accepts 0 alone.  probes[] from count up is not read.
 *   * "kernel" picks the FAMILY as for a soft light list: 0, 1, 2, 7 (and -1 below 256 K pixels) the lane-per-ray walk over 16 x 16
 *     blocks, the lights in order, each wave deciding per light for its own 8 x 8 quarter; 3..6, 8, 9 (and -1 from 256 K pixels) the
 *     stackless packet over 8 x 8 tiles -- with "soft_split" 1 (default) four waves per tile that deal the probe pairs (l, j < k_l) --
 *     all n_l samples where k_l == 0 --, join their counts in LDS, decide alike, and deal the remaining pairs over each light's own
 *     penumbra pixels; with 0 one wave does both.  Bands, "packet_budget", "packet_share", "xcd_swizzle" and "row_order" as for a soft
 *     light list, for speed only.
 *   * a tile with no bit below count ends before a ray is set up; a tile without a penumbra pixel of any light ends after its probes;
 *     a light without a penumbra pixel in a tile costs that tile nothing beyond its probe.
 *   * like the other block traces it ignores split tables, tile orders, follow mode, "block_waves", "wide_lane", wave statistics and
 *     the clock probe, and never drops or alters any of them.
 *   * the device forms are asynchronous, allocate nothing and read nothing back; under graph capture each adds ONE kernel node,
 *     constants, list, probes and options by value.  The host form copies in its rows only, traces, copies out and synchronises.
 *   * get-only option "soft_list_adaptive_traces": launches so far (no other counter moves for them); rts_ctx_last_kernel_name then
 *     names "shadowSoftLightListAdaptiveShareKernel" or "shadowSoftLightListAdaptivePacketKernel<S,geom>", S = 4 or 1 waves per tile,
 *     geom = rows, bands or general as for "shadowSoftDistancePacketKernel". */
int rts_trace_soft_light_list_adaptive(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                       const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                                       uint32_t row_end, uint8_t* counts, const uint32_t* probes, uint8_t* refined);
int rts_trace_soft_light_list_adaptive_device(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                              const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                              uint32_t row_begin, uint32_t row_end, uint8_t* d_counts, const uint32_t* probes,
                                              uint8_t* d_refined, void* stream);
int rts_trace_soft_light_list_adaptive_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                                      const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                                      uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_counts,
                                                      const uint32_t* probes, uint8_t* d_refined, void* stream);

/* JITTERED SOFT LIGHT LISTS: the adaptive soft light list with a PER-PIXEL JITTER TABLE per light (rts_light.table, in a list).  The
 * arguments are those of rts_trace_soft_light_list_adaptive*, plus `tables` after `probes`: list->count entries on the host, read by
 * value at the call, under graph capture too.  With n_l = max(1, nsamples_l), k_l = probes[l] and T_l = tables[l]:
 *   T_l == 0   light l is exactly what rts_trace_soft_light_list_adaptive* makes of it.
 *   T_l != 0   (a soft entry only) light l stands for the derived rts_light
 *                { type, nsamples_l, xyz, table T_l, offsets'[i][c] = radius * offsets[first + i][c] }      (i < T_l, c < 3)
 *              -- the product one rounded multiply, as above.  So pixel p aims sample j at offsets'[(start(p) + j) mod T_l], start(p) =
 *              (hash32(p) * T_l) >> 32, p = y * W + x in the caller's FULL frame: the rule of rts_light.table, unchanged, in a row
 *              range, in a stripe and in the host form alike.  Plane l is byte for byte what the one-light trace writes for that
 *              derived light under bit l of the light map: rts_trace_shadow_mask_adaptive* with probe k_l where k_l >= 1, bit l of
 *              refined that call's refined byte; rts_trace_shadow_mask_active* where k_l == 0, the refined bit 0.
 * Neighbouring pixels then probe different points of the light, so a thin penumbra that one fixed probe pattern misses everywhere is
 * caught in some pixels.  Everything else is the adaptive list's contract: planes at and above count and rows outside the range /
 * stripe are untouched; a pixel whose map byte has no bit below count gets zeros and its position is never read; every byte is integer
 * counting of bytes that depend on (pixel, light, sample) alone, so no order, deal or option can change one.
 *   * tables == NULL or all zeros below count IS rts_trace_soft_light_list_adaptive*: the same launch of the same kernel, counted by
 *     "soft_list_adaptive_traces".
 *   * RTS_ERR_INVALID_ARG, nothing written, no counter moved: everything rts_trace_soft_light_list_adaptive* refuses; tables[l] != 0 on
 *     a hard entry; tables[l] < nsamples_l; first + tables[l] > RTS_SOFT_LIST_OFFSETS.  tables[] from count up is not read.
 *   * families, "soft_split", bands and the speed-only options as for the adaptive list; split tables, tile orders, follow mode and
 *     the wide packet are ignored as by every block trace.  The device forms are asynchronous, allocate nothing and read nothing
 *     back; under graph capture each adds ONE kernel node, constants, list, probes, tables and options by value.  The host form
 *     stages its rows as the adaptive list's host form does.
 *   * get-only option "soft_list_jitter_traces": launches with some table so far (no other counter moves for them);
 *     rts_ctx_last_kernel_name then names "shadowSoftLightListAdaptiveShareKernel<jitter>" or
 *     "shadowSoftLightListAdaptivePacketKernel<S,geom,jitter>".
 *   * a list with every probe 0 and some table is the full jittered list trace; it runs this family, first phase only. */
int rts_trace_soft_light_list_jittered(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                       const float* positions, const uint8_t* lights_map, uint32_t W, uint32_t H, uint32_t row_begin,
                                       uint32_t row_end, uint8_t* counts, const uint32_t* probes, const uint32_t* tables,
                                       uint8_t* refined);
int rts_trace_soft_light_list_jittered_device(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                              const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                              uint32_t row_begin, uint32_t row_end, uint8_t* d_counts, const uint32_t* probes,
                                              const uint32_t* tables, uint8_t* d_refined, void* stream);
int rts_trace_soft_light_list_jittered_stripes_device(rts_ctx* ctx, const rts_constants* constants, const rts_soft_light_list* list,
                                                      const float* d_positions, const uint8_t* d_lights_map, uint32_t W, uint32_t H,
                                                      uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_counts,
                                                      const uint32_t* probes, const uint32_t* tables, uint8_t* d_refined, void* stream);

/* ---- device-memory and timing plumbing (so callers need no HIP headers) ------ */
int rts_device_count(int* count);
int rts_device_malloc(rts_ctx* ctx, void** d_ptr, size_t bytes);
int rts_device_free(rts_ctx* ctx, void* d_ptr);
int rts_memcpy_h2d(rts_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int rts_memcpy_d2h(rts_ctx* ctx, void* dst, const void* d_src, size_t bytes);
int rts_stream_synchronize(rts_ctx* ctx, void* stream);
/* A stream of the context's device for the `stream` arguments above (a renderer passes its own hipStream_t).  Dispatches on
 * different streams may overlap: with two frames in flight the tail of one frame's dispatch runs beside the next one's. */
int rts_stream_create(rts_ctx* ctx, void** stream);
int rts_stream_destroy(rts_ctx* ctx, void* stream);
/* hipEvent pair on `stream` == Gfx_BeginTimer/EndTimer(Timestamp_Shadows) (cpp:572,594).
 * rts_timer_end records the stop event; rts_timer_elapsed_ms synchronises on it. */
int rts_timer_begin(rts_ctx* ctx, void* stream);
int rts_timer_end(rts_ctx* ctx, void* stream);
int rts_timer_elapsed_ms(rts_ctx* ctx, float* ms);
/* Per-launch timing: hipEvents in numbered slots (0..65535, created on first use).  rts_timer_mark records slot `slot`
 * on `stream`; rts_timer_between_ms synchronises on slot_b and returns the time from slot_a to slot_b.  A mark before
 * every dispatch of a frame loop gives the per-frame GPU times whose median the reference shows
 * (120-frame average of Timestamp_Shadows, cpp:263-265). */
int rts_timer_mark(rts_ctx* ctx, void* stream, uint32_t slot);
int rts_timer_between_ms(rts_ctx* ctx, uint32_t slot_a, uint32_t slot_b, float* ms);
/* Name of the kernel the last trace launched (for matching rocprofv3 rows). */
const char* rts_ctx_last_kernel_name(rts_ctx* ctx);
/* Dispatch order of the image tiles for traces whose workgroup count equals `count`: workgroup i works on tile
 * order[i] (a permutation of 0..count-1; NULL or 0 restores the natural order).  Speed only. */
int rts_ctx_set_tile_order(rts_ctx* ctx, const uint32_t* order, size_t count);
/* ... planned from one measured launch of THIS dispatch (any light, any number of samples; stripes as in
 * rts_trace_shadow_mask_stripes_device, n_stripes 1 = the whole frame): the order a whole-dispatch split table runs in -- half-
 * octave bands of measured tile life, longest first, each band dealt over the 8 XCDs by xcd_square x xcd_square-tile image squares
 * (0: not), a tile counted as long as the longest of its life_block x life_block block (0 / 1: itself) --, for the launches that
 * carry no table: soft shadows (16 samples on the city - 5.6 %, on the courtyard - 6.3 %).  rts_ctx_autotune does this for
 * dispatches of more than one sample and keeps it when it gains 1 %.  *tiles = tiles ordered (0: none -- not a dispatch of one
 * 8x8 tile per workgroup).  An order planned on a dispatch of several samples is used by such dispatches only: one-sample traces
 * of the same size keep their everyday launch (and their split table).  Options: "tile_order" 0 makes traces ignore the
 * installed order; get "tile_order_tiles", "tile_order_planned", "tile_order_square", "tile_order_block".  Synchronous, default
 * stream.  Speed only. */
int rts_ctx_plan_tile_order(rts_ctx* ctx, const rts_constants* constants, const rts_light* light, const float* d_positions,
                            uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_mask,
                            uint32_t xcd_square, uint32_t life_block, uint32_t* tiles);
/* Free and total device memory in bytes (hipMemGetInfo on the context's device); either pointer may be NULL. */
int rts_device_mem_info(rts_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
/* Diagnostics (tools/wave_stats.py): after rts_ctx_set_option(ctx, "wave_stats", n_waves) the packet
 * kernels record 4 x u64 per wave: start clock, end clock, {dissolved flag (bit 0) | lane-per-ray iterations after the
 * dissolve (bits 8-31) | clocks from start to the dissolve (32-63)}, {tile x (48-63) | tile y (32-47) | lane-steps in
 * those iterations (0-31)};
 * this copies them out. */
int rts_ctx_read_wave_stats(rts_ctx* ctx, uint64_t* out, size_t waves);
/* After rts_ctx_set_option(ctx, "clock_probe", tile_rows) every launch of a packet kernel on a 2-D grid -- the everyday
 * instantiation included, so the launches that are TIMED -- stamps, for the first wave of each tile row, {shader clock at
 * start, at end, 100 MHz clock at start, at end} (4 x u64 per row): clock held = sum(d shader) / sum(d 100 MHz) * 100 MHz. */
int rts_ctx_read_clock_probe(rts_ctx* ctx, uint64_t* out, size_t rows);
/* Picks the kernel for this frame by timing the candidates on it (lane-per-ray with work sharing for small frames, the
 * packet kernel, the wide packet kernel) -- what a renderer does once per scene and resolution; then, for a packet kernel,
 * the dissolve threshold ("packet_share" 4 or 6) and the order in which the tile rows are started ("row_order" 0 or 1), each
 * kept only if it gains 1.5 %; then seven split tables (rts_ctx_plan_splits below) planned from one set of wave statistics -- the
 * tiles that lived longer than a quarter of the frame split or not, the longest 3 % / third / all of the tiles started first --,
 * the fastest kept on the same condition (any table installed before is dropped).  Leaves the options "kernel", "packet_share" and "row_order" set to the winners and the winning table installed
 * (*chosen = the kernel, median of five launches in *ms; both nullable).  Device pointers, default stream, synchronous.
 * Results never depend on any of it. */
int rts_ctx_autotune(rts_ctx* ctx, const rts_constants* constants, const rts_light* light, const float* d_positions,
                     uint32_t W, uint32_t H, uint8_t* d_mask, int* chosen, float* ms);
/* The same for the dispatch of rts_trace_shadow_mask_stripes_device with these band_rows / n_stripes / stripe: what rank
 * `stripe` of an n_stripes-GPU frame launches is what it tunes -- kernel, dissolve threshold, and the split
 * table for its own rows (one eighth of a 4K frame is two rounds of the chip's wave slots: its time is its longest waves). */
int rts_ctx_autotune_stripes(rts_ctx* ctx, const rts_constants* constants, const rts_light* light, const float* d_positions,
                             uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_mask,
                             int* chosen, float* ms);
/* ---- split tiles: the few tiles that are measured to be LONG walked by several waves -------------------------------------
 * The reference maps one 8x8 tile to one 64-thread group (RayTracedShadows.comp:127, dispatch RayTracedShadows.cpp:590-592) and
 * so does every kernel here; a frame's time is then often its few longest waves.  A split table breaks that mapping for
 * exactly those tiles: each is walked by S one-wave workgroups ("pieces"), every piece over ONE index range of the node
 * stream with all 64 rays (any-hit is an OR over the ranges; exactness: rts_kernels.hip, "SPLIT TILES").  The pieces are
 * the first workgroups of the SAME dispatch (the longest work starts first), the split tiles' own waves end in their
 * prologue, and launches without a table run the unchanged everyday kernels.
 *
 * rts_ctx_plan_splits measures and installs the table for ONE dispatch geometry (frame size and row range, or stripe):
 *   1. wave statistics of the dispatch (one launch with "wave_stats"), or the caller's statistics of an EARLIER frame
 *      (prev_stats / prev_realtime as rts_ctx_read_wave_stats / rts_ctx_read_wave_realtime return them, prev_waves entries).
 *      Records with end <= start and tiles right of the dispatch are ignored; statistics that name a tile below the
 *      dispatch, or one tile in two records, are refused (RTS_ERR_INVALID_ARG, no table).  A tile without a record is
 *      launched as usual: the table covers the whole dispatch -- no tile rows -- only when every one of its tiles has one;
 *   2. the tiles whose wave lived longer than min_life_us and ended later than end_after_us (the longest max_tiles of
 *      them) are walked once more, alone, with
 *      their visited node indices logged; tile t gets S = ceil(life / piece_us) pieces (2 .. max_pieces), its ranges cut at
 *      the j/S quantiles of its log.
 * Every later trace with the same geometry, one sample per pixel and kernel 3 or 8 uses the table (option "tile_splits" 0
 * switches that off; get "split_tiles" / "split_pieces" = the table's size); rts_ctx_set_bvh and rts_ctx_clear_splits drop
 * it.  The table only holds node indices and tile coordinates: a camera or light that moves makes it less well balanced,
 * never wrong.  Needs the private copy of kernel 8 (without one no table is made: *tiles = 0).  Synchronous, default stream;
 * device pointers.  Each stream that traces with the table gets a small state buffer at its first such trace (at most 8 streams;
 * further ones trace without the table).  A trace under graph capture never allocates: a stream whose first trace with the table is
 * being captured traces -- and replays -- without the table; trace once on the stream before capturing to have the table in the
 * graph.  Results never depend on any of it (tests/test_gpu_parity.py, tests/test_gpu_graph.py). */
typedef struct rts_split_plan {
    float    min_life_us;        /* > 0 */
    float    end_after_us;       /* >= 0: ... and only the tiles whose wave ENDED later than this after the dispatch's first wave
                                    started (the waves that end last are the dispatch's tail; 0 = every long tile) */
    float    piece_us;           /* > 0 */
    float    front_life_us;      /* 0, or < min_life_us: the tiles that lived longer than this but are not split are FRONT tiles -- walked
                                    by their own wave, unchanged, but dispatched at the head of the grid (after the pieces, longest
                                    first): what is long starts early, and the dispatch ends with short waves */
    float    front_share;        /* 0..1: ... or, given as a share: the longest front_share of all tiles of the dispatch start first (the
                                    larger of the two thresholds counts when both are given).  1 = every tile: the WHOLE dispatch runs
                                    in table order -- half-octaves of measured life, longest first, image order inside one -- and no
                                    tile rows are launched at all.  rts_ctx_autotune tries 0.03, 1/3 and 1 */
    uint32_t max_pieces;         /* 2..64 */
    uint32_t max_tiles;          /* 0 = 4096 */
    uint32_t xcd_square;         /* 0, or S: inside a band of the front order, record i (which the dispatcher places on XCD i mod 8) is taken
                                    from the S x S-tile squares of the image that belong to that XCD -- each XCD's L2 then holds the part of
                                    the tree its squares see.  Balanced by construction (equal numbers of equally long tiles per XCD);
                                    rts_ctx_autotune uses 32 with front_share 1 */
    uint32_t life_block;         /* 0 / 1, or B: the front order takes a tile to be as long as the longest tile of its block of B x B tiles.
                                    A table sorted by single tiles fits ONE camera (a step of 0.1 % of the view distance moves what is long by
                                    a tile, and a stale order is slower than none); sorted by blocks of 16 it gives up a third of its gain
                                    and keeps the rest over a camera path (rts_ctx option "tune_for_motion") */
    uint32_t reserved_;          /* 0 */
    const uint64_t* prev_stats;  /* all three NULL / 0: measure now */
    const uint64_t* prev_realtime;
    size_t   prev_waves;
} rts_split_plan;
int rts_ctx_plan_splits(rts_ctx* ctx, const rts_constants* constants, const rts_light* light, const float* d_positions,
                        uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end, uint8_t* d_mask,
                        const rts_split_plan* plan, uint32_t* tiles, uint32_t* pieces);
/* ... for the dispatch of rts_trace_shadow_mask_stripes_device with the same band_rows / n_stripes / stripe */
int rts_ctx_plan_splits_stripes(rts_ctx* ctx, const rts_constants* constants, const rts_light* light, const float* d_positions,
                                uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_stripes, uint32_t stripe, uint8_t* d_mask,
                                const rts_split_plan* plan, uint32_t* tiles, uint32_t* pieces);
int rts_ctx_clear_splits(rts_ctx* ctx);
/* The parameters the installed table was planned with (prev_* NULL): what a caller that tunes in one process and renders in
 * another hands to rts_ctx_plan_splits there.  RTS_ERR_INVALID_ARG without a table. */
int rts_ctx_get_split_plan(rts_ctx* ctx, rts_split_plan* out);
/* Diagnostics (tools/piece_stats.py): the first `pieces` records of the installed table -- 8 x u32 {tile x | tile y << 16, first
 * node, end node, state slot | pieces of the tile << 24, byte offset of the wide node the piece starts at, 0, 0, 0} -- and, after rts_ctx_set_option(ctx, "piece_stats", n), 8 x u64 per
 * piece of the last launch that used the table: 100 MHz clock at {start, end, rays ready, end of the packet phase, start of the
 * lane-per-ray phase, end of the walk}, {wide nodes entered | stack entries at the dissolve << 32}, lanes found occluded.
 * Either pointer may be NULL. */
int rts_ctx_read_piece_stats(rts_ctx* ctx, uint32_t* records, uint64_t* clocks, size_t pieces);
/* ---- follow mode (option "follow" 1): a split-table order that follows a moving camera, planned on the device -------------
 * A table planned on one frame fits that frame; a camera that moves 0.1 % of its view distance per frame makes it stale.  In follow
 * mode every one-sample trace where an installed split table could apply today (kernel 3 or 8, one tile per workgroup on a 2-D grid,
 * the private copy, no "wave_stats", no "wide_lane"; stripes with power-of-two bands and -- for follow mode alone: a stripe is always
 * launched first row to last, and an installed table applies to it whatever the option says -- the option "row_order" 0) and none does -- an installed
 * table or a caller's tile order always wins -- records how long each tile's wave lived, and kernels on the same stream then plan
 * from those lives the order the NEXT trace of the same dispatch on that stream runs in: the front-only table with every tile in
 * it (rts_split_plan front_share 1, no pieces) -- half-octave bands of life, longest first, row-major inside a band, a tile as long
 * as the longest of its follow_block x follow_block block, each band dealt over the XCDs by follow_square squares:
 *   DEAL.  Inside a band of L records that starts at record R, XCD x's own tiles (those of the squares (sx + 3 sy) mod 8 = x, in
 *   image order) fill the band's positions q with (R + q) mod 8 = x, in order, until the tiles or the positions run out.  The
 *   tiles left over, in XCD order and then image order, fill the positions still vacant in increasing order.  (Prefix sums
 *   compute it -- unlike rts_ctx_plan_splits' greedy deal, which also differs when an XCD runs out.)
 * Nothing is read back, nothing waits on the host, and a steady frame allocates nothing.  The first trace of a geometry on a stream
 * runs the everyday launch (and records); later ones the stream's rolling order.  State is per stream, for one dispatch geometry
 * (W, H, row range, stripe: another one starts the stream over), at most 8 streams (the least recently used is evicted); frames in
 * flight on two streams never share a buffer.  rts_stream_destroy releases the stream's state; rts_ctx_set_bvh, a GPU build's
 * install, "follow" 0 and rts_ctx_destroy drop all of it; rts_ctx_refit_bvh_device keeps it (tile coordinates do not change).  A
 * trace on a stream under graph capture never allocates: without state it runs the everyday launch.  Results never depend on it.
 *
 * Diagnostics: synchronises `stream` and returns the life of every tile of its last traced dispatch in 100 MHz ticks (row-major
 * tile id; either pointer may be NULL) and the order the next trace runs (record i -> bx | by << 16).  RTS_ERR_INVALID_ARG when the
 * stream holds no state or `tiles` is not the dispatch's tile count.  rtsh_follow_order (rts_scene.h) is the same order on the host. */
int rts_ctx_read_follow(rts_ctx* ctx, void* stream, uint32_t* lives, uint32_t* order, size_t tiles);
/* Self-test behind one of the kernels' shortcuts: 1.0f / x (comp:44, comp:77) is computed as v_rcp_f32 + one Newton step in
 * fma arithmetic when 2^-100 <= |x| <= 2^100 in a whole wave.  That this is the correctly rounded quotient is checked HERE for
 * every bit pattern of the range on the context's device: out[0] = patterns checked (3 355 443 200), out[1] = patterns whose
 * result differs from the IEEE division -- 0 on gfx950 --, out[2] = one such pattern.  A fraction of a second. */
int rts_selftest_reciprocal(rts_ctx* ctx, uint64_t out[3]);
/* Same launch, 4 x u64 per wave: s_memrealtime (the constant 100 MHz counter) at the wave's start and end, shader clocks
 * from the wave's start to its first ray being ready (G-buffer texel in, ray set up), XCC id.  With the start/end shader
 * clocks above: clock held under load = sum(end - start clocks) / sum(end - start realtime) * 100 MHz. */
int rts_ctx_read_wave_realtime(rts_ctx* ctx, uint64_t* out, size_t waves);

#ifdef __cplusplus
}
#endif
#endif /* RTS_H */
