// Follow mode (option "follow"): the order the NEXT trace of a dispatch runs in, planned on the device from the
// tile lives the last trace recorded (shadowMaskFollowKernel), in the stream, without a host round trip.  The order is the
// front-only split table with every tile in it (front_share 1, no pieces): half-octave bands of life, longest first, row-major
// inside a band; blocks of B x B tiles count as long as their longest tile (life_block); with xcd_square S each band is dealt
// over the 8 XCDs by the rule of include/rts.h (a rule prefix sums compute, unlike the host planner's greedy dealOverXcds).
// rtsh_follow_order (rts_api.cpp) is the same order on the host: the checker of this file.
//
//   blockMax  (B > 1) one wave per block of B x B tiles: the longest life of the block.
//   rank      one workgroup per chunk of 1024 tiles: key = band slot * 8 + XCD (XCD 0 without S), its band from
//             the per-band lower bounds of the tick count the host computed with its own lifeBand (integer compares only);
//             the tile's rank among the chunk's tiles of the same key in image order (ballots per wave, counts per wave in
//             LDS); the chunk's count per key.
//   scan      one wave per key: the exclusive prefix of the chunks' counts (in place) and the key's total.
//   scatter   every workgroup first derives each band slot's first record from the totals (in LDS); then one thread per tile:
//             rank in (band, XCD) = chunk prefix + rank in chunk; its record by the deal; the tile's
//             dword at the record's slot of the front map.  Every record gets exactly one tile: a permutation by construction.
//
// Synchronisation: every dependency crosses a kernel boundary or stays inside one workgroup (barriers only).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "rts_device.h"

namespace rts {

namespace {

constexpr uint32_t KEYS = FOLLOW_BANDS * 8u;
constexpr uint32_t CHUNK = 1024u;              // tiles per workgroup of the rank pass: one tile per thread
constexpr uint32_t RANK_THREADS = 1024u;

struct Scratch {                               // carved from one allocation (followScratchBytes)
    uint32_t* blockMax;                        // one word per tile (a block count never exceeds the tile count)
    uint32_t* keyRank;                         // key << 16 | rank in chunk, per tile
    uint32_t* hist;                            // [KEYS][chunks]: counts, then exclusive prefixes
    uint32_t* total;                           // [KEYS]: tiles per key
};

__host__ __device__ inline size_t alignUp(size_t v) { return (v + 255u) & ~(size_t)255u; }

Scratch carve(void* base, uint32_t tiles) {
    const uint32_t chunks = (tiles + CHUNK - 1) / CHUNK;
    char* b = (char*)base;
    Scratch s;
    s.blockMax = (uint32_t*)b; b += alignUp((size_t)tiles * 4);
    s.keyRank = (uint32_t*)b; b += alignUp((size_t)tiles * 4);
    s.hist = (uint32_t*)b; b += alignUp((size_t)KEYS * chunks * 4);
    s.total = (uint32_t*)b;
    return s;
}

__device__ __forceinline__ uint32_t lifeOf(const uint32_t* lives, uint32_t t) { return lives[2u * t + 1u] - lives[2u * t]; }

// one wave per block of B x B tiles: its lanes take the block's tiles in turn, then a max over the wave (no atomics)
__global__ __launch_bounds__(256) void followBlockMaxKernel(const uint32_t* lives, uint32_t blocksX, uint32_t blocksY, uint32_t B,
                                                            uint32_t* blockMax) {
    const uint32_t gx = (blocksX + B - 1) / B, gy = (blocksY + B - 1) / B;
    const uint32_t blk = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (blk >= gx * gy) return;
    const uint32_t x0 = (blk % gx) * B, y0 = (blk / gx) * B;
    uint32_t m = 0;
    for (uint32_t i = lane; i < B * B; i += 64u) {
        const uint32_t x = x0 + i % B, y = y0 + i / B;
        if (x < blocksX && y < blocksY) { const uint32_t v = lifeOf(lives, y * blocksX + x); m = v > m ? v : m; }
    }
    for (uint32_t d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)m, (int)d, 64); m = o > m ? o : m; }
    if (lane == 0) blockMax[blk] = m;
}

__global__ __launch_bounds__(RANK_THREADS) void followRankKernel(const uint32_t* lives, const uint32_t* blockMax, uint32_t blocksX,
                                                                 uint32_t tiles, uint32_t B, uint32_t S, FollowBands bands,
                                                                 uint32_t* keyRank, uint32_t* hist, uint32_t chunks) {
    __shared__ uint32_t minTicks[FOLLOW_BANDS];
    __shared__ uint16_t waveCount[RANK_THREADS / 64][KEYS];         // tiles per key in each wave
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t i = tid; i < FOLLOW_BANDS; i += RANK_THREADS) minTicks[i] = bands.minTicks[i];
    for (uint32_t i = tid; i < KEYS * (RANK_THREADS / 64); i += RANK_THREADS) waveCount[i / KEYS][i % KEYS] = 0;
    const uint32_t t = blockIdx.x * CHUNK + tid;
    const bool valid = t < tiles;
    const uint32_t bx = valid ? t % blocksX : 0u, by = valid ? t / blocksX : 0u;
    const uint32_t life = !valid ? 0u : (B > 1 ? blockMax[(by / B) * ((blocksX + B - 1) / B) + bx / B] : lifeOf(lives, t));
    __syncthreads();
    uint32_t key = 0;
    if (valid) {
        uint32_t lo = 0, hi = FOLLOW_BANDS - 1;                      // the highest band whose lower bound the life reaches
        while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (minTicks[mid] <= life) lo = mid; else hi = mid - 1; }
        const uint32_t slot = FOLLOW_BANDS - 1 - lo;                // (slot 0: the longest band)
        const uint32_t xcd = S ? ((bx / S) + (by / S) * 3u) & 7u : 0u;
        key = slot * 8u + xcd;
    }
    // rank among the wave's lanes of the same key: one ballot per distinct key of the wave
    uint64_t todo = __builtin_amdgcn_ballot_w64(valid);
    uint32_t rank = 0;
    const uint64_t below = (1ull << lane) - 1ull;
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t k = __builtin_amdgcn_readlane(key, leader);
        const uint64_t same = __builtin_amdgcn_ballot_w64(valid && key == k);
        if (valid && key == k) rank = (uint32_t)__builtin_popcountll(same & below);
        if (lane == leader) waveCount[wave][k] = (uint16_t)__builtin_popcountll(same);
        todo &= ~same;
    }
    __syncthreads();
    if (valid) {
        uint32_t r = rank;
        for (uint32_t w = 0; w < wave; ++w) r += waveCount[w][key];
        keyRank[t] = (key << 16) | r;
    }
    for (uint32_t k = tid; k < KEYS; k += RANK_THREADS) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < RANK_THREADS / 64; ++w) sum += waveCount[w][k];
        hist[(size_t)k * chunks + blockIdx.x] = sum;
    }
}

// one wave per key: the exclusive prefix of its chunks' counts, 64 chunks at a time (a scan across the wave), and its total
__global__ __launch_bounds__(256) void followScanKernel(uint32_t* hist, uint32_t chunks, uint32_t* total) {
    const uint32_t key = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (key >= KEYS) return;
    uint32_t* h = hist + (size_t)key * chunks;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < chunks; c0 += 64u) {
        const uint32_t v = c0 + lane < chunks ? h[c0 + lane] : 0u;
        uint32_t incl = v;
        for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= d) incl += o; }
        if (c0 + lane < chunks) h[c0 + lane] = carry + incl - v;
        carry += (uint32_t)__shfl((int)incl, 63, 64);
    }
    if (lane == 0) total[key] = carry;
}

// positions q of a band of L records from record R with (R + q) mod 8 == y: q = ((y - R) mod 8) + 8 k, k < slots(y)
__device__ __forceinline__ uint32_t slotsOf(uint32_t off, uint32_t L) { return L > off ? (L - 1u - off) / 8u + 1u : 0u; }

__global__ __launch_bounds__(256) void followScatterKernel(const uint32_t* keyRank, const uint32_t* hist, uint32_t chunks, const uint32_t* total,
                                                           uint32_t blocksX, uint32_t tiles, uint32_t S, uint32_t* frontMap,
                                                           uint32_t frontStride) {
    __shared__ uint32_t tot[KEYS];
    __shared__ uint32_t start[FOLLOW_BANDS];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t kr = t < tiles ? keyRank[t] : 0u;
    for (uint32_t k = threadIdx.x; k < KEYS; k += 256u) tot[k] = total[k];
    __syncthreads();
    if (threadIdx.x < 64) {                                           // the first record of every band slot: a scan across one wave
        const uint32_t lane = threadIdx.x;
        uint32_t n = 0;
        if (lane < FOLLOW_BANDS) for (uint32_t x = 0; x < 8; ++x) n += tot[lane * 8u + x];
        uint32_t incl = n;
        for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= d) incl += o; }
        if (lane < FOLLOW_BANDS) start[lane] = incl - n;
    }
    __syncthreads();
    if (t >= tiles) return;
    const uint32_t key = kr >> 16, slot = key >> 3, x = key & 7u;
    const uint32_t j = hist[(size_t)key * chunks + t / CHUNK] + (kr & 0xFFFFu);          // rank among the band's tiles of XCD x
    const uint32_t* bi = tot + slot * 8u;
    const uint32_t R = start[slot];
    uint32_t q = j;
    if (S) {
        uint32_t c[8], L = 0;
        for (uint32_t y = 0; y < 8; ++y) { c[y] = bi[y]; L += c[y]; }
        const uint32_t offX = (x - R) & 7u, mX = slotsOf(offX, L);
        if (j < mX) q = offX + 8u * j;                                // on its own XCD
        else {                                                        // a leftover: the l-th vacant position
            uint32_t l = j - mX, m[8];
            for (uint32_t y = 0; y < 8; ++y) {
                m[y] = slotsOf((y - R) & 7u, L);
                if (y < x && c[y] > m[y]) l += c[y] - m[y];
            }
            // vacancies in rows [0, K): sum over y of max(0, min(K, m_y) - c_y); the first K with more than l
            uint32_t lo = 0, hi = (L + 7u) / 8u;                      // row of the answer in [lo, hi)
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                uint32_t v = 0;
                for (uint32_t y = 0; y < 8; ++y) { const uint32_t e = mid < m[y] ? mid : m[y]; v += e > c[y] ? e - c[y] : 0u; }
                if (v <= l) lo = mid; else hi = mid;
            }
            uint32_t before = 0;
            for (uint32_t y = 0; y < 8; ++y) { const uint32_t e = lo < m[y] ? lo : m[y]; before += e > c[y] ? e - c[y] : 0u; }
            uint32_t off = 0;
            for (uint32_t o = 0; o < 8; ++o) {                        // row lo, in position order
                const uint32_t y = (R + o) & 7u;
                if (c[y] <= lo && lo < m[y]) { if (before == l) { off = o; break; } ++before; }
            }
            q = 8u * lo + off;
        }
    }
    const uint32_t rec = R + q;
    const uint32_t bx = t % blocksX, by = t / blocksX;
    frontMap[(size_t)(rec & 7u) * frontStride + (rec >> 3)] = bx | (by << 16);
}

} // namespace

size_t followScratchBytes(uint32_t tiles) {
    const uint32_t chunks = (tiles + CHUNK - 1) / CHUNK;
    return alignUp((size_t)tiles * 4) * 2 + alignUp((size_t)KEYS * chunks * 4) + alignUp((size_t)KEYS * 4);
}

hipError_t launchFollowPlan(const uint32_t* d_lives, uint32_t blocksX, uint32_t blocksY, uint32_t xcdSquare, uint32_t lifeBlock,
                            const FollowBands& bands, void* d_scratch, uint32_t* d_frontMap, uint32_t frontStride, hipStream_t stream) {
    const uint32_t tiles = blocksX * blocksY, chunks = (tiles + CHUNK - 1) / CHUNK, B = lifeBlock > 1 ? lifeBlock : 1u;
    if (!tiles) return hipSuccess;
    const Scratch s = carve(d_scratch, tiles);
    if (B > 1) {
        const uint32_t blocks = ((blocksX + B - 1) / B) * ((blocksY + B - 1) / B);
        hipLaunchKernelGGL(followBlockMaxKernel, dim3((blocks + 3u) / 4u), dim3(256), 0, stream, d_lives, blocksX, blocksY, B, s.blockMax);
    }
    hipLaunchKernelGGL(followRankKernel, dim3(chunks), dim3(RANK_THREADS), 0, stream, d_lives, s.blockMax, blocksX, tiles, B, xcdSquare,
                       bands, s.keyRank, s.hist, chunks);
    hipLaunchKernelGGL(followScanKernel, dim3((KEYS + 3u) / 4u), dim3(256), 0, stream, s.hist, chunks, s.total);
    hipLaunchKernelGGL(followScatterKernel, dim3((tiles + 255u) / 256u), dim3(256), 0, stream, s.keyRank, s.hist, chunks, s.total, blocksX,
                       tiles, xcdSquare, d_frontMap, frontStride);
    return hipGetLastError();
}

} // namespace rts
