// Host-only check of rts_dispatch.h (tests/test_host_logic.py, built with -fsanitize=address,undefined): rows(), bandShift(), grid()
// and operator== of a Dispatch against restatements written the slow way -- bands counted one by one, shifts tried one by one, blocks
// stepped over one by one.  Prints the first case that differs and exits 1; "ok <cases>" otherwise.
#include "../../raytracedshadows_amd/csrc/rts_dispatch.h"
#include <cstdio>
#include <cstdlib>

using rts::Dispatch;

static unsigned long cases = 0;

#define CHECK(got, want, ...) \
    do { ++cases; if ((got) != (want)) { std::printf(__VA_ARGS__); std::printf(": got %u, want %u\n", (unsigned)(got), (unsigned)(want)); std::exit(1); } } while (0)

// the bands b = stripe, stripe + n, ... below H, one by one: whole bands (what the dispatch launches) and the rows of them inside the frame
static void ownedSlow(uint32_t H, uint32_t band, uint32_t n, uint32_t stripe, uint64_t* whole, uint64_t* inside) {
    *whole = *inside = 0;
    for (uint64_t b = 0; b * band < H; ++b) {
        if (b % n != stripe) continue;
        *whole += band;
        *inside += (b + 1) * band <= H ? band : H - b * band;
    }
}

static uint32_t bandShiftSlow(uint32_t band, uint32_t n) {
    if (n <= 1 || band % 8 != 0) return 0xFFFFFFFFu;
    const uint32_t tiles = band / 8;
    for (uint32_t sh = 0; sh < 32; ++sh) {
        if ((1u << sh) == tiles) return sh;
        if ((1u << sh) > tiles) break;
    }
    return 0xFFFFFFFFu;
}

static uint32_t blocksSlow(uint32_t pixels, uint32_t block) {
    uint32_t n = 0;
    for (uint64_t at = 0; at < pixels; at += block) ++n;
    return n;
}

int main() {
    const uint32_t Hs[] = { 1, 7, 8, 9, 15, 16, 17, 131, 1080, 2160, 65535u * 8u, (1u << 31) / 3840u };
    const uint32_t bands[] = { 8, 16, 24, 32, 40, 64, 2160 };
    const uint32_t ns[] = { 1, 2, 3, 4, 8 };

    // rows(): every stripe, those without a band included (0); the last band cut by H still counts whole
    for (uint32_t H : Hs) for (uint32_t band : bands) for (uint32_t n : ns) for (uint32_t stripe = 0; stripe < n; ++stripe) {
        uint64_t whole, inside;
        ownedSlow(H, band, n, stripe, &whole, &inside);
        const Dispatch g = Dispatch::ofStripe(3840, H, band, n, stripe);
        if (n == 1) {
            CHECK(inside, H, "one stripe owns the frame H %u band %u", H, band);
            CHECK(g.rows(), H, "rows() H %u band %u n 1", H, band);
            CHECK(g.bandRows, 0u, "one stripe is a dispatch of rows H %u band %u", H, band);
        } else {
            CHECK(g.rows(), whole, "rows() H %u band %u n %u stripe %u", H, band, n, stripe);
            CHECK(whole - inside < band, true, "at most the last band is cut H %u band %u n %u stripe %u", H, band, n, stripe);
            CHECK(g.rows() == 0, (uint64_t)stripe * band >= H, "no band, no rows H %u band %u n %u stripe %u", H, band, n, stripe);
        }
        CHECK(rts::stripeRows(H, band, n, stripe), whole, "stripeRows H %u band %u n %u stripe %u", H, band, n, stripe);
    }
    for (uint32_t H : Hs) {                                       // row ranges of an unstriped dispatch
        const uint32_t cuts[] = { 0, H / 3, H / 2, H };
        for (uint32_t b : cuts) for (uint32_t e : cuts) if (b <= e) CHECK(Dispatch::ofRows(7, H, b, e).rows(), e - b, "rows() H %u [%u, %u)", H, b, e);
    }

    // bandShift(): the log2 of a band of 2^k tiles of stripes, 0xFFFFFFFF for everything else
    const uint32_t shiftBands[] = { 0, 8, 16, 24, 32, 40, 64, 2160, 1, 4, 7, 9, 12, 20, 36, 100, 2164, 1u << 20, 0x80000000u, 0xFFFFFFF8u };
    for (uint32_t band : shiftBands) for (uint32_t n : ns) for (uint32_t stripe = 0; stripe < n; ++stripe) {
        const Dispatch g{ 3840, 2160, 0, 2160, band, n, stripe };
        CHECK(g.bandShift(), bandShiftSlow(band, n), "bandShift() band %u n %u stripe %u", band, n, stripe);
    }
    CHECK((Dispatch{ 8, 8, 0, 8, 64, 1, 0 }).bandShift(), 0xFFFFFFFFu, "bandShift() of one stripe");
    CHECK((Dispatch{ 8, 8, 0, 8, 64, 2, 0 }).bandShift(), 3u, "bandShift() of 64-row bands");

    // grid(): blocks stepped over one by one; the swizzle alone rounds the launch up to 8
    const uint32_t Ws[] = { 1, 7, 8, 9, 3840, 65535u * 8u + 1u };
    const uint32_t rowsOf[] = { 1, 7, 8, 9, 15, 16, 17, 131, 1080 };
    const uint32_t blockSides[] = { 8, 16 };
    for (uint32_t block : blockSides) for (uint32_t W : Ws) for (uint32_t rows : rowsOf) for (int swizzle = 0; swizzle < 2; ++swizzle) {
        const rts::Grid got = Dispatch::ofRows(W, rows + 5, 5, rows + 5).grid(block, block, swizzle != 0);
        const uint32_t bx = blocksSlow(W, block), by = blocksSlow(rows, block);
        uint32_t launched = bx * by;
        while (swizzle && launched % 8 != 0) ++launched;
        CHECK(got.blocksX, bx, "grid().blocksX block %u W %u", block, W);
        CHECK(got.blocksY, by, "grid().blocksY block %u rows %u", block, rows);
        CHECK(got.nBlocks, bx * by, "grid().nBlocks block %u W %u rows %u", block, W, rows);
        CHECK(got.gridBlocks, launched, "grid().gridBlocks block %u W %u rows %u swizzle %d", block, W, rows, swizzle);
    }
    {   // a stripe's grid covers its virtual rows; blocks need not be square
        const rts::Grid got = Dispatch::ofStripe(100, 131, 24, 3, 1).grid(8, 32, false);      // bands 1 and 4 of 6: 48 rows
        CHECK(got.blocksX, 13u, "stripe grid blocksX");
        CHECK(got.blocksY, 2u, "stripe grid blocksY");
    }

    // operator==: equal when all seven fields are, unequal when any one differs
    const Dispatch a{ 64, 64, 0, 64, 8, 2, 0 };
    Dispatch same = a;
    CHECK(a == same, true, "equal dispatches");
    const char* names[7] = { "W", "H", "rowBegin", "rowEnd", "bandRows", "nStripes", "stripe" };
    uint32_t Dispatch::* const fields[7] = { &Dispatch::W, &Dispatch::H, &Dispatch::rowBegin, &Dispatch::rowEnd, &Dispatch::bandRows,
                                             &Dispatch::nStripes, &Dispatch::stripe };
    for (int i = 0; i < 7; ++i) {
        Dispatch other = a;
        other.*fields[i] += 1;
        CHECK(a == other, false, "dispatches that differ in %s", names[i]);
        CHECK(other == a, false, "dispatches that differ in %s, the other way round", names[i]);
    }

    // stripeArgsOk: a nonzero multiple of 8, a stripe of the n
    CHECK(rts::stripeArgsOk(8, 1, 0) && rts::stripeArgsOk(2160, 8, 7), true, "stripeArgsOk accepts");
    CHECK(rts::stripeArgsOk(0, 2, 0) || rts::stripeArgsOk(12, 2, 0) || rts::stripeArgsOk(8, 0, 0) || rts::stripeArgsOk(8, 2, 2), false, "stripeArgsOk refuses");
    std::printf("ok %lu\n", cases);
    return 0;
}
