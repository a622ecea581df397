// Host-only check of rts_args.h (tests/test_host_logic.py, built with -fsanitize=address,undefined): the hard light's rule, the soft
// light's rule, lightListOk and the frame check against restatements of include/rts.h written the slow way -- the allowed values
// tried one by one.  Prints the first case that differs and exits 1; "ok <cases>" otherwise.
#include "../../raytracedshadows_amd/csrc/rts_args.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static unsigned long cases = 0;

#define CHECK(got, want, ...) \
    do { ++cases; if ((got) != (want)) { std::printf(__VA_ARGS__); std::printf(": got %d, want %d\n", (int)(got), (int)(want)); std::exit(1); } } while (0)

static bool knownType(uint32_t type) {
    const uint32_t known[] = { RTS_LIGHT_DIRECTIONAL, RTS_LIGHT_POINT };
    for (uint32_t t : known) if (type == t) return true;
    return false;
}

// include/rts.h, rts_trace_shadow_distance*: a known type; nsamples 0 or 1 = a hard shadow, more is refused
static bool hardSlow(const rts_light& l) {
    if (!knownType(l.type)) return false;
    for (uint32_t n = 0; n <= 1; ++n) if (l.nsamples == n) return true;
    return false;
}

// include/rts.h, rts_light: a known type; nsamples 0 or 1 (hard) or in [2, 64]; table 0, or T in [nsamples, 64] with nsamples >= 2
static bool softSlow(const rts_light& l) {
    if (!knownType(l.type)) return false;
    for (uint32_t n = 0; n <= 64; ++n) {
        if (l.nsamples != n) continue;
        if (l.table == 0) return true;
        if (n < 2) return false;
        for (uint32_t T = n; T <= 64; ++T) if (l.table == T) return true;
    }
    return false;
}

int main() {
    // the light rules: every (type, nsamples, table) around the allowed ranges, and NULL
    CHECK(rts::hardLightOk(nullptr), true, "hardLightOk(NULL)");
    CHECK(rts::softLightOk(nullptr), true, "softLightOk(NULL)");
    for (uint32_t type = 0; type <= 2; ++type) for (uint32_t ns = 0; ns <= 66; ++ns) for (uint32_t table = 0; table <= 66; ++table) {
        rts_light l;
        std::memset(&l, 0, sizeof(l));
        l.type = type; l.nsamples = ns; l.table = table;
        CHECK(rts::softLightOk(&l), softSlow(l), "softLightOk type %u nsamples %u table %u", type, ns, table);
        CHECK(rts::hardLightOk(&l), hardSlow(l), "hardLightOk type %u nsamples %u table %u", type, ns, table);
    }
    {   // far outside the ranges
        rts_light l;
        std::memset(&l, 0, sizeof(l));
        l.type = 0xFFFFFFFFu;
        CHECK(rts::softLightOk(&l) || rts::hardLightOk(&l), false, "type 0xFFFFFFFF");
        l.type = RTS_LIGHT_POINT; l.nsamples = 0xFFFFFFFFu;
        CHECK(rts::softLightOk(&l) || rts::hardLightOk(&l), false, "nsamples 0xFFFFFFFF");
        l.nsamples = 4; l.table = 0xFFFFFFFFu;
        CHECK(rts::softLightOk(&l), false, "table 0xFFFFFFFF");
    }

    // lightListOk: 1..RTS_MAX_LIST_LIGHTS lights of known types; a bad type counts only below the count
    CHECK(rts::lightListOk(nullptr), false, "lightListOk(NULL)");
    const uint32_t badTypes[] = { 2u, 0xFFFFFFFFu };
    for (uint32_t count = 0; count <= 9; ++count) {
        rts_light_list list;
        std::memset(&list, 0, sizeof(list));
        list.count = count;
        for (uint32_t l = 0; l < RTS_MAX_LIST_LIGHTS; ++l) list.lights[l].type = (l & 1u) ? RTS_LIGHT_POINT : RTS_LIGHT_DIRECTIONAL;
        bool countOk = false;
        for (uint32_t n = 1; n <= RTS_MAX_LIST_LIGHTS; ++n) countOk = countOk || count == n;
        CHECK(rts::lightListOk(&list), countOk, "lightListOk count %u, known types", count);
        for (uint32_t bad : badTypes) for (uint32_t at = 0; at < RTS_MAX_LIST_LIGHTS; ++at) {
            const uint32_t kept = list.lights[at].type;
            list.lights[at].type = bad;
            bool read = false;                                     // light `at` is one of the list's
            for (uint32_t l = 0; l < count && l < RTS_MAX_LIST_LIGHTS; ++l) read = read || l == at;
            CHECK(rts::lightListOk(&list), countOk && !read, "lightListOk count %u, type %u at %u", count, bad, at);
            list.lights[at].type = kept;
        }
    }

    // the frame check: W, H nonzero, row_begin <= row_end <= H (an empty range is a frame's)
    const uint32_t sizes[] = { 0, 1, 7, 2160, 0xFFFFFFFFu };
    for (uint32_t W : sizes) for (uint32_t H : sizes) {
        const uint32_t rows[] = { 0, 1, H / 2, H - 1, H, H + 1, 0xFFFFFFFFu };      // (H - 1, H + 1 wrap at the ends: still rows to try)
        for (uint32_t b : rows) for (uint32_t e : rows) {
            bool want = W > 0 && H > 0;
            if (b > e) want = false;                               // row_begin > row_end
            if (e > H) want = false;                               // row_end == H + 1 and beyond
            CHECK(rts::frameRowsOk(W, H, b, e), want, "frameRowsOk W %u H %u rows [%u, %u)", W, H, b, e);
        }
    }
    CHECK(rts::frameRowsOk(61, 37, 30, 30), true, "an empty range inside the frame");
    CHECK(rts::frameRowsOk(61, 37, 37, 37), true, "an empty range at the frame's end");
    CHECK(rts::frameRowsOk(61, 37, 3, 37), true, "row_end == H");
    CHECK(rts::frameRowsOk(61, 37, 3, 38), false, "row_end == H + 1");
    CHECK(rts::frameRowsOk(61, 37, 31, 30), false, "row_begin > row_end");
    CHECK(rts::frameRowsOk(0, 37, 0, 37), false, "W 0");
    CHECK(rts::frameRowsOk(61, 0, 0, 0), false, "H 0");
    std::printf("ok %lu\n", cases);
    return 0;
}
