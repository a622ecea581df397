// BVH refit on the device (rts_ctx_refit_bvh_device): the installed stream keeps its topology, its boxes and leaf data are
// recomputed from new vertex positions.  The bytes are those of the host form (bvh_refit.cpp, the contract: DESIGN.md 4.9):
// inner boxes are per-axis min / max in the total order of the order-preserving integer encoding, so the reduction order
// below -- any order -- gives the same bytes.
//
// Synchronisation: the rule of rts_lbvh.hip holds -- every dependency between nodes crosses a kernel boundary or stays inside
// one workgroup.  No flags or spin-waits between workgroups (the per-XCD L2s are not coherent).
//
//   check     one thread per triangle: index range and finiteness of the referenced vertices -> status.err.  Every kernel
//             after it that writes reads status.err first and writes nothing when it is set: a refused refit leaves the
//             stream and the private copy as they were, without a host round trip in between.
//   treelets  a subtree is a contiguous node range, so every subtree of at most T nodes whose parent's is larger ("treelet
//             root", from the schedule the host derived once from the topology) is one workgroup's job: its leaves write
//             e0 / e1 / tail and put their encoded boxes into LDS; the box of an inner node i of the range is the min / max
//             over the range [i, end(i)) of those boxes -- a range query, answered with a sparse table built by doubling in
//             LDS (level k covers windows of 2^k slots; a range of length L is two windows of 2^floor(log2 L)).  Barriers
//             only.  T = 1024 (option "refit_treelet").
//   top       the inner nodes above the treelet roots, one workgroup, in order of height (barrier between heights); a
//             child's box is read back from the stream (decode / encode is a bijection: exact) or, for a leaf child,
//             from its vertices.
//   wide      the private copy of kernel 8 in place (its layout and record order depend on the topology only, rts_wide.hip):
//             one thread per wide node re-reads its slot boxes, one per triangle record its v0 / e0 / e1 and parent box.
//   validate  validateKernel (rts_wide.hip) -> status.valid; cost: sum of surfaceArea(inner box) -> status.cost.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "rts_refit.h"

namespace rts {

hipError_t validateStreamAsync(const void* d_packed, uint32_t P, uint32_t* d_word);     // rts_wide.hip

namespace {

constexpr uint32_t END = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t encodeOrdered(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t decodeOrdered(uint32_t e) { return (e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e; }
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

struct Refit {
    uint32_t* w;                 // the stream as dwords (8 per node, then 4 per tail vec4)
    uint32_t P, N;
    const float* verts; uint32_t stride; const uint32_t* indices;
    RefitStatus* status;
};

__device__ __forceinline__ const float* vertexOf(const Refit& r, uint32_t prim, uint32_t c) {
    return r.verts + (size_t)r.stride * r.indices[(size_t)prim * 3 + c];
}

// leaf node n: e0 / e1 into the stream (tag and link untouched), the tail of its triangle, its encoded box into box[6]
__device__ __forceinline__ void refitLeaf(const Refit& r, uint32_t n, uint32_t tag, uint32_t box[6]) {
    const uint32_t prim = tag - 2 * r.N;
    const float* v0 = vertexOf(r, prim, 0);
    const float* v1 = vertexOf(r, prim, 1);
    const float* v2 = vertexOf(r, prim, 2);
    uint32_t* o = r.w + (size_t)n * 8;
    o[0] = __float_as_uint(v1[0] - v0[0]); o[1] = __float_as_uint(v1[1] - v0[1]); o[2] = __float_as_uint(v1[2] - v0[2]);
    o[4] = __float_as_uint(v2[0] - v0[0]); o[5] = __float_as_uint(v2[1] - v0[1]); o[6] = __float_as_uint(v2[2] - v0[2]);
    uint32_t* t = r.w + ((size_t)2 * r.N + prim) * 4;
    t[0] = __float_as_uint(v0[0]); t[1] = __float_as_uint(v0[1]); t[2] = __float_as_uint(v0[2]); t[3] = 0;
    for (int k = 0; k < 3; ++k) {
        const uint32_t a = encodeOrdered(__float_as_uint(v0[k])), b = encodeOrdered(__float_as_uint(v1[k])),
                       c = encodeOrdered(__float_as_uint(v2[k]));
        box[k] = umin(umin(a, b), c);
        box[3 + k] = umax(umax(a, b), c);
    }
}

__device__ __forceinline__ void storeBox(const Refit& r, uint32_t n, const uint32_t box[6]) {
    uint32_t* o = r.w + (size_t)n * 8;
    o[0] = decodeOrdered(box[0]); o[1] = decodeOrdered(box[1]); o[2] = decodeOrdered(box[2]);
    o[4] = decodeOrdered(box[3]); o[5] = decodeOrdered(box[4]); o[6] = decodeOrdered(box[5]);
}

__global__ void checkKernel(Refit r, size_t vertexFloats) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= r.P) return;
    uint32_t err = 0;
    uint32_t idx[3];
    for (int c = 0; c < 3; ++c) {
        idx[c] = r.indices[(size_t)p * 3 + c];
        if ((size_t)idx[c] * r.stride + 3 > vertexFloats) err |= REFIT_ERR_INDEX;
    }
    if (!err)
        for (int c = 0; c < 3; ++c) {
            const float* v = r.verts + (size_t)r.stride * idx[c];
            for (int k = 0; k < 3; ++k) if (!(__builtin_fabsf(v[k]) < __builtin_inff())) err |= REFIT_ERR_NONFINITE;
        }
    if (err) atomicOr(&r.status->err, err);
}

// One workgroup per treelet root; dynamic LDS: two sparse-table levels of 6 x T encoded words, then T range lengths.
__global__ __launch_bounds__(256) void treeletKernel(Refit r, const uint32_t* roots, uint32_t T) {
    if (r.status->err) return;
    extern __shared__ uint32_t lds[];
    uint32_t* level[2] = { lds, lds + 6 * T };
    uint32_t* len = lds + 12 * T;
    const uint32_t root = roots[blockIdx.x];
    const uint32_t rootLink = r.w[(size_t)root * 8 + 7];
    const uint32_t size = (rootLink == END ? r.N : rootLink) - root;          // <= T (schedule)
    for (uint32_t j = threadIdx.x; j < size; j += blockDim.x) {
        const uint32_t n = root + j;
        const uint32_t tag = r.w[(size_t)n * 8 + 3];
        uint32_t box[6] = { END, END, END, 0, 0, 0 };                          // the identity of min / max
        if (tag != END) {
            refitLeaf(r, n, tag, box);
            len[j] = 0;
        } else {
            const uint32_t link = r.w[(size_t)n * 8 + 7];
            len[j] = (link == END ? r.N : link) - n;
        }
        for (int k = 0; k < 6; ++k) level[0][k * T + j] = box[k];
    }
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t k = 0; (1u << k) <= size; ++k) {
        const uint32_t win = 1u << k;
        const uint32_t* m = level[cur];
        // inner nodes whose range length L has floor(log2 L) == k: [j, j + L) = [j, j + win) u [j + L - win, j + L)
        for (uint32_t j = threadIdx.x; j < size; j += blockDim.x) {
            const uint32_t L = len[j];
            if (L == 0 || 31u - __builtin_clz(L) != k) continue;
            const uint32_t b = j + L - win;
            uint32_t box[6];
            for (int a = 0; a < 3; ++a) {
                box[a] = umin(m[a * T + j], m[a * T + b]);
                box[3 + a] = umax(m[(3 + a) * T + j], m[(3 + a) * T + b]);
            }
            storeBox(r, root + j, box);
        }
        if ((win << 1) > size) break;                                           // no range is that long
        uint32_t* out = level[cur ^ 1];
        for (uint32_t j = threadIdx.x; j < size; j += blockDim.x) {
            const bool pair = j + win < size;
            for (int a = 0; a < 3; ++a) {
                const uint32_t lo = m[a * T + j], hi = m[(3 + a) * T + j];
                out[a * T + j] = pair ? umin(lo, m[a * T + j + win]) : lo;
                out[(3 + a) * T + j] = pair ? umax(hi, m[(3 + a) * T + j + win]) : hi;
            }
        }
        __syncthreads();
        cur ^= 1;
    }
}

__device__ __forceinline__ void childBox(const Refit& r, uint32_t c, uint32_t box[6]) {
    const uint32_t* a = r.w + (size_t)c * 8;
    const uint32_t tag = a[3];
    if (tag == END) {
        for (int k = 0; k < 3; ++k) { box[k] = encodeOrdered(a[k]); box[3 + k] = encodeOrdered(a[4 + k]); }
        return;
    }
    const uint32_t prim = tag - 2 * r.N;
    for (int k = 0; k < 3; ++k) { box[k] = END; box[3 + k] = 0; }
    for (uint32_t v = 0; v < 3; ++v) {
        const float* p = vertexOf(r, prim, v);
        for (int k = 0; k < 3; ++k) {
            const uint32_t e = encodeOrdered(__float_as_uint(p[k]));
            box[k] = umin(box[k], e);
            box[3 + k] = umax(box[3 + k], e);
        }
    }
}

// The nodes above the treelet roots, lowest height first; one workgroup (its stores are visible to its own waves after
// the barrier).  A degenerate chain has as many heights as nodes: correct, slow.
__global__ __launch_bounds__(1024) void topKernel(Refit r, const uint32_t* top, const uint32_t* levelOff, uint32_t levels) {
    if (r.status->err) return;
    for (uint32_t h = 0; h < levels; ++h) {
        const uint32_t first = levelOff[h], last = levelOff[h + 1];
        for (uint32_t t = first + threadIdx.x; t < last; t += blockDim.x) {
            const uint32_t i = top[t], left = i + 1, right = r.w[(size_t)left * 8 + 7];
            uint32_t l[6], rb[6], box[6];
            childBox(r, left, l);
            childBox(r, right, rb);
            for (int k = 0; k < 3; ++k) { box[k] = umin(l[k], rb[k]); box[3 + k] = umax(l[3 + k], rb[3 + k]); }
            storeBox(r, i, box);
        }
        __syncthreads();
    }
}

// Wide node w (layout: rts_wide.hip): slot k's node is dword 28 + k (k >= 1) or, for slot 0, n + 1 when that is a leaf and
// n + 2 otherwise; an inner slot carries its own box, a leaf slot (reference with the low bit set) its parent's.
__global__ void wideRefreshKernel(Refit r, uint32_t* wide, uint32_t wideCount, const uint32_t* parents) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= wideCount || r.status->err) return;
    uint32_t* o = wide + (size_t)w * 32;
    const uint32_t n = o[28];
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t ref = o[24 + k];
        if (ref == END) continue;
        const uint32_t node = k ? o[28 + k] : (r.w[(size_t)(n + 1) * 8 + 3] != END ? n + 1 : n + 2);
        const uint32_t* b = r.w + (size_t)((ref & 1u) ? parents[node] : node) * 8;
        o[6 * k + 0] = b[0]; o[6 * k + 1] = b[1]; o[6 * k + 2] = b[2];
        o[6 * k + 3] = b[4]; o[6 * k + 4] = b[5]; o[6 * k + 5] = b[6];
    }
}

// Triangle record j: {v0, e0, e1, leaf node, parent's box}; the leaf node (dword 9) does not change.
__global__ void trisRefreshKernel(Refit r, uint32_t* tris, const uint32_t* parents) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= r.P || r.status->err) return;
    uint32_t* o = tris + (size_t)j * 16;
    const uint32_t n = o[9];
    const uint32_t* a = r.w + (size_t)n * 8;
    const uint32_t* v0 = r.w + (size_t)a[3] * 4;
    const uint32_t* pb = r.w + (size_t)parents[n] * 8;
    o[0] = v0[0]; o[1] = v0[1]; o[2] = v0[2];
    o[3] = a[0]; o[4] = a[1]; o[5] = a[2];
    o[6] = a[4]; o[7] = a[5]; o[8] = a[6];
    o[10] = pb[0]; o[11] = pb[1]; o[12] = pb[2];
    o[13] = pb[4]; o[14] = pb[5]; o[15] = pb[6];
}

// SAH cost proxy: sum over inner nodes of surfaceArea(box) (BVHBuilder.cpp:24-28), and the root's; any order.
__global__ void costKernel(const uint32_t* w, uint32_t N, double* sum, double* rootArea) {
    __shared__ double part[256];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    double v = 0.0;
    if (i < N && w[(size_t)i * 8 + 3] == END) {
        const uint32_t* a = w + (size_t)i * 8;
        const float ex = __uint_as_float(a[4]) - __uint_as_float(a[0]), ey = __uint_as_float(a[5]) - __uint_as_float(a[1]),
                    ez = __uint_as_float(a[6]) - __uint_as_float(a[2]);
        const float sa = (ex * ey + ey * ez + ez * ex) * 2.0f;
        v = (double)sa;
        if (i == 0) *rootArea = v;
    }
    part[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t s = 128; s; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0] != 0.0) atomicAdd(sum, part[0]);
}

} // namespace

size_t refitLdsBytes(uint32_t T) { return (size_t)13 * T * 4; }

hipError_t refitLaunch(const RefitLaunch& L) {
    Refit r{ (uint32_t*)L.d_packed, L.P, 2 * L.P - 1, L.verts, L.stride, L.indices, L.status };
    const dim3 block(256);
    hipError_t e = hipMemsetAsync(L.status, 0, L.baseline ? sizeof(RefitStatus) : offsetof(RefitStatus, baseCost), nullptr);
    if (e != hipSuccess) return e;
    const uint32_t gridN = (r.N + 255) / 256;
    if (L.baseline)                                                           // the stream as installed, before any box changes
        hipLaunchKernelGGL(costKernel, dim3(gridN), block, 0, nullptr, r.w, r.N, &L.status->baseCost, &L.status->baseRootArea);
    hipLaunchKernelGGL(checkKernel, dim3((L.P + 255) / 256), block, 0, nullptr, r, L.vertexFloats);
    hipLaunchKernelGGL(treeletKernel, dim3(L.nRoots), block, refitLdsBytes(L.treelet), nullptr, r, L.roots, L.treelet);
    if (L.nLevels)
        hipLaunchKernelGGL(topKernel, dim3(1), dim3(1024), 0, nullptr, r, L.top, L.levelOff, L.nLevels);
    if (L.wideCount) {
        hipLaunchKernelGGL(wideRefreshKernel, dim3((L.wideCount + 255) / 256), block, 0, nullptr, r, (uint32_t*)L.d_wide, L.wideCount,
                           L.d_parents);
        hipLaunchKernelGGL(trisRefreshKernel, dim3((L.P + 255) / 256), block, 0, nullptr, r, (uint32_t*)L.d_tris, L.d_parents);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = validateStreamAsync(L.d_packed, L.P, &L.status->valid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(costKernel, dim3(gridN), block, 0, nullptr, r.w, r.N, &L.status->cost, &L.status->rootArea);
    return hipGetLastError();
}

hipError_t refitSetLds(uint32_t T) {
    return hipFuncSetAttribute((const void*)treeletKernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)refitLdsBytes(T));
}

} // namespace rts
