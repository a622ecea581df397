// Host-only check of rts_args.h's rule for the per-pixel jitter tables of a jittered soft light list trace
// (tests/test_soft_list_jitter_host.py, built with -fsanitize=address,undefined): softListTablesOk against a restatement of
// include/rts.h written the slow way -- the allowed table sizes tried one by one -- over every (nsamples, first, table) around the
// allowed ranges in the first and the last entry, hard entries, lists and probes the older rules refuse, NULL for each argument,
// values at the ends of uint32 (first + table wraps), and a tables array of exactly `count` entries on the heap.  Prints the first
// case that differs and exits 1; "ok <cases>" otherwise.
#include "../../raytracedshadows_amd/csrc/rts_args.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

static unsigned long cases = 0;

#define CHECK(got, want, ...) \
    do { ++cases; if ((got) != (want)) { std::printf(__VA_ARGS__); std::printf(": got %d, want %d\n", (int)(got), (int)(want)); std::exit(1); } } while (0)

// include/rts.h, rts_trace_soft_light_list_jittered*: everything the adaptive call refuses (softListProbesOk, pinned by
// tests/cpp/soft_list_probes_host.cpp); per entry below count a table of 0 is allowed, and on a soft entry so is every T with
// nsamples <= T and first + T <= 48 -- tried one by one, in 64 bits
static bool tablesSlow(const rts_soft_light_list* list, const uint32_t* probes, const uint32_t* tables) {
    if (!rts::softListProbesOk(list, probes)) return false;
    if (!tables) return true;
    for (uint32_t l = 0; l < list->count; ++l) {
        const rts_soft_light_entry& e = list->lights[l];
        bool ok = tables[l] == 0;
        if (e.nsamples >= 2)
            for (uint64_t T = e.nsamples; (uint64_t)e.first + T <= 48; ++T) ok = ok || tables[l] == T;
        if (!ok) return false;
    }
    return true;
}

int main() {
    static_assert(RTS_SOFT_LIST_OFFSETS == 48 && RTS_MAX_LIST_LIGHTS == 8, "the limits of include/rts.h");
    const uint32_t far[] = { 49u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFD0u, 0xFFFFFFFEu, 0xFFFFFFFFu };
    rts_soft_light_list* s = (rts_soft_light_list*)std::malloc(sizeof(rts_soft_light_list));
    if (!s) return 2;
    const uint32_t zeros[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    const auto good = [&](uint32_t count) {
        std::memset(s, 0, sizeof(*s));
        s->count = count;
        for (uint32_t l = 0; l < 8; ++l) { s->lights[l].type = l & 1u; s->lights[l].nsamples = 2 + 5 * l; s->lights[l].first = l; s->lights[l].radius = 0.5f; }
    };
    // (the tables live on the heap, exactly `count` entries: a rule that read tables[count] would be seen)
    const auto check = [&](const char* what, uint32_t a, uint32_t b, uint32_t at, uint32_t value) {
        const uint32_t entries = (s->count >= 1 && s->count <= 8) ? s->count : 1;      // (a refused count: one entry, never read)
        uint32_t* tables = (uint32_t*)std::malloc(sizeof(uint32_t) * entries);
        if (!tables) std::exit(2);
        for (uint32_t l = 0; l < entries; ++l) tables[l] = 0;
        if (at < entries) tables[at] = value;
        CHECK(rts::softListTablesOk(s, zeros, tables), tablesSlow(s, zeros, tables), "%s %u %u entry %u table %u", what, a, b, at, value);
        std::free(tables);
    };
    good(3);
    CHECK(rts::softListTablesOk(nullptr, zeros, zeros), false, "softListTablesOk(NULL, probes, tables)");
    CHECK(rts::softListTablesOk(s, nullptr, zeros), false, "softListTablesOk(list, NULL, tables)");
    CHECK(rts::softListTablesOk(s, zeros, nullptr), true, "tables == NULL is all zeros");
    CHECK(rts::softListTablesOk(s, zeros, zeros), true, "all zeros");
    CHECK(rts::softListHasTable(s, nullptr), false, "no tables, none set");
    CHECK(rts::softListHasTable(s, zeros), false, "zeros, none set");
    { const uint32_t t[8] = { 0, 0, 0, 7, 7, 7, 7, 7 }; CHECK(rts::softListHasTable(s, t), false, "tables beyond the count are not looked at"); }
    { const uint32_t t[3] = { 0, 0, 12 }; CHECK(rts::softListHasTable(s, t), true, "the last entry's table"); }
    // every (nsamples, first, table) around the ranges, in the first and in the last entry of a list
    for (uint32_t ns = 0; ns <= 49; ++ns) for (uint32_t first : { 0u, 1u, 24u, 46u, 47u, 48u }) for (uint32_t T = 0; T <= 50; ++T)
        for (uint32_t count : { 1u, 8u }) for (uint32_t at : { 0u, count - 1u }) {
            good(count);
            s->lights[at].nsamples = ns; s->lights[at].first = first;
            check("nsamples, first", ns, first, at, T);
            const bool listOk = ns <= 48 && (ns < 2 || first + ns <= 48);
            const bool want = listOk && (T == 0 || (ns >= 2 && T >= ns && first + T <= 48));
            uint32_t tables[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
            tables[at] = T;
            CHECK(rts::softListTablesOk(s, zeros, tables), want, "nsamples %u first %u table %u entry %u of %u", ns, first, T, at, count);
        }
    // a hard entry accepts 0 alone, whatever its `first`
    for (uint32_t ns : { 0u, 1u }) for (uint32_t T : { 0u, 1u, 2u, 48u }) for (uint32_t first : { 0u, 47u, 0xFFFFFFFFu }) {
        good(2); s->lights[1].nsamples = ns; s->lights[1].first = first;
        const uint32_t tables[2] = { 0, T };
        CHECK(rts::softListTablesOk(s, zeros, tables), T == 0, "a hard entry of nsamples %u first %u, table %u", ns, first, T);
    }
    // far values: refused in an entry below the count (first + table may wrap in 32 bits), not looked at beyond it
    for (uint32_t v : far) {
        good(3);
        const uint32_t beyond[8] = { 0, 0, 0, v, v, v, v, v };
        CHECK(rts::softListTablesOk(s, zeros, beyond), true, "a table %u beyond the count", v);
        for (uint32_t at : { 0u, 2u }) {
            check("far table", v, 0, at, v);
            uint32_t t[3] = { 0, 0, 0 };
            t[at] = v;
            CHECK(rts::softListTablesOk(s, zeros, t), false, "table %u in entry %u", v, at);
        }
    }
    good(1); s->lights[0].nsamples = 2; s->lights[0].first = 20;
    { const uint32_t t[1] = { 0xFFFFFFFFu - 19u }; CHECK(rts::softListTablesOk(s, zeros, t), false, "first + table == 2^32"); }
    { const uint32_t t[1] = { 0xFFFFFFFFu - 18u }; CHECK(rts::softListTablesOk(s, zeros, t), false, "first + table == 2^32 + 1"); }
    // what the older rules refuse is refused whatever the tables
    for (uint32_t count : { 0u, 9u, 0xFFFFFFFFu }) { good(count); check("count", count, 0, 0, 0); CHECK(rts::softListTablesOk(s, zeros, zeros), false, "count %u", count); }
    good(8); s->lights[7].type = 2;
    CHECK(rts::softListTablesOk(s, zeros, zeros), false, "a type of 2");
    good(8); s->lights[0].radius = std::numeric_limits<float>::quiet_NaN();
    CHECK(rts::softListTablesOk(s, zeros, zeros), false, "a NaN radius");
    good(3);
    { const uint32_t p[3] = { 2, 0, 0 }; CHECK(rts::softListTablesOk(s, p, zeros), false, "probe 2 of 2"); }
    // the ends of the ranges
    good(1); s->lights[0].nsamples = 48; s->lights[0].first = 0;
    { const uint32_t t[1] = { 48 }; CHECK(rts::softListTablesOk(s, zeros, t), true, "48 of 48"); }
    { const uint32_t t[1] = { 47 }; CHECK(rts::softListTablesOk(s, zeros, t), false, "47 under 48 samples"); }
    s->lights[0].nsamples = 2; s->lights[0].first = 46;
    { const uint32_t t[1] = { 2 }; CHECK(rts::softListTablesOk(s, zeros, t), true, "2 from 46"); }
    { const uint32_t t[1] = { 3 }; CHECK(rts::softListTablesOk(s, zeros, t), false, "3 from 46"); }
    s->lights[0].nsamples = 16; s->lights[0].first = 8;
    { const uint32_t t[1] = { 40 }; CHECK(rts::softListTablesOk(s, zeros, t), true, "40 from 8"); }
    { const uint32_t t[1] = { 41 }; CHECK(rts::softListTablesOk(s, zeros, t), false, "41 from 8"); }
    std::free(s);
    std::printf("ok %lu\n", cases);
    return 0;
}
