// Host-only check of rts_args.h's adaptive rule (tests/test_adaptive_args_host.py, built with -fsanitize=address,undefined):
// adaptiveLightOk against a restatement of include/rts.h written the slow way -- the allowed values tried one by one -- over every
// (type, nsamples, table, probe) around the allowed ranges, NULL, and values far outside.  Prints the first case that differs and
// exits 1; "ok <cases>" otherwise.
#include "../../raytracedshadows_amd/csrc/rts_args.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static unsigned long cases = 0;

#define CHECK(got, want, ...) \
    do { ++cases; if ((got) != (want)) { std::printf(__VA_ARGS__); std::printf(": got %d, want %d\n", (int)(got), (int)(want)); std::exit(1); } } while (0)

// include/rts.h, rts_trace_shadow_mask_adaptive*: a known type; nsamples n in [2, 64]; table 0, or T in [n, 64]; probe k in [1, n - 1]
static bool adaptiveSlow(const rts_light& l, uint32_t probe) {
    if (l.type != RTS_LIGHT_DIRECTIONAL && l.type != RTS_LIGHT_POINT) return false;
    for (uint32_t n = 2; n <= 64; ++n) {
        if (l.nsamples != n) continue;
        bool tableOk = l.table == 0;
        for (uint32_t T = n; T <= 64; ++T) tableOk = tableOk || l.table == T;
        if (!tableOk) return false;
        for (uint32_t k = 1; k + 1 <= n; ++k) if (probe == k) return true;
    }
    return false;
}

int main() {
    const uint32_t far[] = { 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu };
    for (uint32_t probe = 0; probe <= 66; ++probe) CHECK(rts::adaptiveLightOk(nullptr, probe), false, "adaptiveLightOk(NULL, %u)", probe);
    // (the light lives on the heap, exactly sized: a rule that read past an rts_light would be seen)
    rts_light* l = (rts_light*)std::malloc(sizeof(rts_light));
    if (!l) return 2;
    for (uint32_t type = 0; type <= 2; ++type) for (uint32_t ns = 0; ns <= 66; ++ns) for (uint32_t table = 0; table <= 66; ++table) {
        std::memset(l, 0, sizeof(*l));
        l->type = type; l->nsamples = ns; l->table = table;
        for (uint32_t probe = 0; probe <= 66; ++probe)
            CHECK(rts::adaptiveLightOk(l, probe), adaptiveSlow(*l, probe), "adaptiveLightOk type %u nsamples %u table %u probe %u", type, ns, table, probe);
        for (uint32_t probe : far)
            CHECK(rts::adaptiveLightOk(l, probe), false, "adaptiveLightOk type %u nsamples %u table %u probe %u", type, ns, table, probe);
    }
    for (uint32_t v : far) {
        std::memset(l, 0, sizeof(*l));
        l->type = RTS_LIGHT_POINT; l->nsamples = 16;
        CHECK(rts::adaptiveLightOk(l, 4), true, "the flagship light");
        l->type = v;
        CHECK(rts::adaptiveLightOk(l, 4), false, "type %u", v);
        l->type = RTS_LIGHT_POINT; l->nsamples = v;
        CHECK(rts::adaptiveLightOk(l, 4), false, "nsamples %u", v);
        CHECK(rts::adaptiveLightOk(l, v - 1u), false, "nsamples %u probe %u", v, v - 1u);     // probe < nsamples is not enough
        l->nsamples = 16; l->table = v;
        CHECK(rts::adaptiveLightOk(l, 4), false, "table %u", v);
    }
    // the ends of the probe range, with and without a table
    std::memset(l, 0, sizeof(*l));
    l->type = RTS_LIGHT_DIRECTIONAL; l->nsamples = 2;
    CHECK(rts::adaptiveLightOk(l, 1), true, "2 samples, probe 1");
    CHECK(rts::adaptiveLightOk(l, 2), false, "2 samples, probe 2");
    l->nsamples = 64; l->table = 64;
    CHECK(rts::adaptiveLightOk(l, 63), true, "64 of 64, probe 63");
    CHECK(rts::adaptiveLightOk(l, 64), false, "64 of 64, probe 64");
    l->nsamples = 65; l->table = 0;
    CHECK(rts::adaptiveLightOk(l, 4), false, "65 samples");
    std::free(l);
    std::printf("ok %lu\n", cases);
    return 0;
}
