// Host-only check of the light map compaction (tests/test_list_sparse_host.py, built with -fsanitize=address,undefined together with
// raytracedshadows_amd/csrc/rts_scene.cpp).  Frames of 1 x 1, 7 x 9, 8 x 8, 9 x 8, 17 x 5, 70 x 33 and the two around one scan group's
// 1024 tiles (8192 x 8, 8200 x 8); maps all zero, all set, bits from `count` up only, one marked pixel in the last tile, about 1 % and
// about 50 % marked; capacities n - 1, n, n + 1 and 1.  The map and the list are heap blocks of exactly the stated size, so an index
// outside the frame or an entry from min(n, capacity) on that is touched is a sanitizer report.  The sanitizers are the first check.
// The second: the list against a restatement of the header's rule (four nested loops: tile row, tile column, row, column),
// the entries past min(n, capacity) unchanged, n exact; every refusal with nothing written.  Prints the first case that differs and
// exits 1; "ok <cases>" otherwise.
#include "../../include/rts_scene.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int rts_bvh_validate(const rts_vec4u*, size_t, uint32_t*) { return RTS_ERR_BAD_BVH; }   // (no pass here takes a stream)

static unsigned long cases = 0;
#define CHECK(cond, ...) \
    do { ++cases; if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

template <class T> static T* block(size_t n) { return (T*)std::malloc((n ? n : 1) * sizeof(T)); }

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static void frame(uint32_t W, uint32_t H, int kind, uint32_t count) {
    const size_t n = (size_t)W * H;
    const uint32_t below = (1u << count) - 1u;
    uint8_t* map = block<uint8_t>(n);
    uint32_t seed = W * 131u + H * 7u + count + (uint32_t)kind;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t bits = 1u + rnd(seed) % 255u, roll = rnd(seed) % 1000u;
        switch (kind) {
        case 0: map[i] = 0; break;
        case 1: map[i] = 0xFF; break;
        case 2: map[i] = (uint8_t)(bits & ~below); break;
        case 3: map[i] = (uint8_t)(i == n - 1 ? 1u : 0u); break;
        case 4: map[i] = (uint8_t)(roll < 10u ? bits : bits & ~below); break;
        default: map[i] = (uint8_t)(roll < 500u ? bits : bits & ~below); break;
        }
    }
    // the rule, restated from the header: tile rows, tile columns, then the rows and the columns inside the tile
    std::vector<uint32_t> want;
    for (uint32_t ty = 0; ty * 8u < H; ++ty)
        for (uint32_t tx = 0; tx * 8u < W; ++tx)
            for (uint32_t y = ty * 8u; y < ty * 8u + 8u && y < H; ++y)
                for (uint32_t x = tx * 8u; x < tx * 8u + 8u && x < W; ++x)
                    if (map[(size_t)y * W + x] & below) want.push_back(y * W + x);
    const uint32_t total = (uint32_t)want.size();
    const uint32_t capacities[4] = { total - 1u, total, total + 1u, 1u };
    for (uint32_t capacity : capacities) {
        if (capacity == 0u || capacity == 0xFFFFFFFFu) continue;
        uint32_t* list = block<uint32_t>(capacity);                       // exactly `capacity` entries
        for (uint32_t i = 0; i < capacity; ++i) list[i] = 0xABABABABu;
        uint32_t got = 0xABABABABu;
        const int s = rtsh_compact_light_map(count, map, W, H, list, capacity, &got);
        CHECK(s == RTS_OK && got == total, "%ux%u kind %d count %u capacity %u: status %d, n %u, want %u", W, H, kind, count, capacity, s, got, total);
        const uint32_t k = total < capacity ? total : capacity;
        for (uint32_t i = 0; i < capacity; ++i)
            CHECK(list[i] == (i < k ? want[i] : 0xABABABABu), "%ux%u kind %d count %u capacity %u: entry %u is %u", W, H, kind, count, capacity, i,
                  list[i]);
        std::free(list);
    }
    std::free(map);
}

static void refusals() {
    uint8_t* map = block<uint8_t>(17 * 5);
    std::memset(map, 0xFF, 17 * 5);
    uint32_t* list = block<uint32_t>(4);
    for (int i = 0; i < 4; ++i) list[i] = 0xABABABABu;
    uint32_t n = 0xABABABABu;
    CHECK(rtsh_compact_light_map(0, map, 17, 5, list, 4, &n) == RTS_ERR_INVALID_ARG, "count 0");
    CHECK(rtsh_compact_light_map(9, map, 17, 5, list, 4, &n) == RTS_ERR_INVALID_ARG, "count 9");
    CHECK(rtsh_compact_light_map(3, nullptr, 17, 5, list, 4, &n) == RTS_ERR_INVALID_ARG, "no map");
    CHECK(rtsh_compact_light_map(3, map, 17, 5, nullptr, 4, &n) == RTS_ERR_INVALID_ARG, "no list");
    CHECK(rtsh_compact_light_map(3, map, 17, 5, list, 4, nullptr) == RTS_ERR_INVALID_ARG, "no n");
    CHECK(rtsh_compact_light_map(3, map, 0, 5, list, 4, &n) == RTS_ERR_INVALID_ARG, "W 0");
    CHECK(rtsh_compact_light_map(3, map, 17, 0, list, 4, &n) == RTS_ERR_INVALID_ARG, "H 0");
    CHECK(rtsh_compact_light_map(3, map, 17, 5, list, 0, &n) == RTS_ERR_INVALID_ARG, "capacity 0");
    CHECK(rtsh_compact_light_map(3, map, 1u << 16, (1u << 15) + 1u, list, 4, &n) == RTS_ERR_INVALID_ARG, "W * H above 2^31");
    CHECK(rtsh_compact_light_map(3, map, 0xFFFFFFFFu, 0xFFFFFFFFu, list, 4, &n) == RTS_ERR_INVALID_ARG, "W * H far above 2^31");
    for (int i = 0; i < 4; ++i) CHECK(list[i] == 0xABABABABu, "a refusal wrote entry %d", i);
    CHECK(n == 0xABABABABu, "a refusal wrote n");
    CHECK(rtsh_compact_scratch_bytes(0, 5) == 0 && rtsh_compact_scratch_bytes(1u << 16, (1u << 15) + 1u) == 0, "scratch of a refused frame");
    CHECK(rtsh_compact_scratch_bytes(8192, 8) == 4u * 1025u && rtsh_compact_scratch_bytes(8200, 8) == 4u * 1027u, "scratch around one group");
    CHECK(rtsh_compact_light_map(3, map, 17, 5, list, 4, &n) == RTS_OK && n == 85u && list[3] == 3u, "the good call");
    std::free(list);
    std::free(map);
}

int main() {
    const uint32_t frames[8][2] = { { 1, 1 }, { 7, 9 }, { 8, 8 }, { 9, 8 }, { 17, 5 }, { 70, 33 }, { 8192, 8 }, { 8200, 8 } };
    for (const auto& f : frames)
        for (int kind = 0; kind < 6; ++kind)
            for (uint32_t count : { 1u, 3u, 8u }) {
                if (f[0] > 1000u && count == 3u) continue;                // (the wide frames: two counts are enough)
                frame(f[0], f[1], kind, count);
            }
    refusals();
    std::printf("ok %lu\n", cases);
    return 0;
}
