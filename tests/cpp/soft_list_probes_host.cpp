// Host-only check of rts_args.h's rule for the probe counts of an adaptive soft light list trace (tests/test_soft_list_probes_host.py,
// built with -fsanitize=address,undefined): softListProbesOk against a restatement of include/rts.h written the slow way -- the
// allowed probes tried one by one -- over every (nsamples, probe) around the allowed ranges in every entry position, lists the list
// rule itself refuses, NULL for either argument, values at the ends of uint32, and a probes array of exactly `count` entries on the
// heap.  Prints the first case that differs and exits 1; "ok <cases>" otherwise.
#include "../../raytracedshadows_amd/csrc/rts_args.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

static unsigned long cases = 0;

#define CHECK(got, want, ...) \
    do { ++cases; if ((got) != (want)) { std::printf(__VA_ARGS__); std::printf(": got %d, want %d\n", (int)(got), (int)(want)); std::exit(1); } } while (0)

// include/rts.h, rts_trace_soft_light_list*: the list's own rule, restated as in tests/cpp/soft_list_args_host.cpp
static bool entrySlow(const rts_soft_light_entry& e) {
    if (e.type != RTS_LIGHT_DIRECTIONAL && e.type != RTS_LIGHT_POINT) return false;
    if (std::isnan(e.radius) || std::isinf(e.radius)) return false;
    if (e.nsamples == 0 || e.nsamples == 1) return true;
    for (uint32_t n = 2; n <= 48; ++n)
        for (uint32_t first = 0; first + n <= 48; ++first)
            if (e.nsamples == n && e.first == first) return true;
    return false;
}
static bool listSlow(const rts_soft_light_list* list) {
    if (!list) return false;
    bool countOk = false;
    for (uint32_t c = 1; c <= 8; ++c) countOk = countOk || list->count == c;
    if (!countOk) return false;
    for (uint32_t l = 0; l < list->count; ++l) if (!entrySlow(list->lights[l])) return false;
    return true;
}
// include/rts.h, rts_trace_soft_light_list_adaptive*: probes must be there; per entry below count 0 is allowed, and so is every
// k with 1 <= k <= n - 1 where n = max(1, nsamples) -- tried one by one
static bool probesSlow(const rts_soft_light_list* list, const uint32_t* probes) {
    if (!probes || !listSlow(list)) return false;
    for (uint32_t l = 0; l < list->count; ++l) {
        const uint32_t ns = list->lights[l].nsamples, n = ns < 1 ? 1 : ns;
        bool ok = probes[l] == 0;
        for (uint32_t k = 1; k + 1 <= n; ++k) ok = ok || probes[l] == k;
        if (!ok) return false;
    }
    return true;
}

int main() {
    static_assert(RTS_SOFT_LIST_OFFSETS == 48 && RTS_MAX_LIST_LIGHTS == 8, "the limits of include/rts.h");
    const uint32_t far[] = { 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFD0u, 0xFFFFFFFEu, 0xFFFFFFFFu };
    rts_soft_light_list* s = (rts_soft_light_list*)std::malloc(sizeof(rts_soft_light_list));
    if (!s) return 2;
    const auto good = [&](uint32_t count) {
        std::memset(s, 0, sizeof(*s));
        s->count = count;
        for (uint32_t l = 0; l < 8; ++l) { s->lights[l].type = l & 1u; s->lights[l].nsamples = 2 + 5 * l; s->lights[l].first = l; s->lights[l].radius = 0.5f; }
    };
    // (the probes live on the heap, exactly `count` entries: a rule that read probes[count] would be seen)
    const auto check = [&](const char* what, uint32_t a, uint32_t b, uint32_t at, uint32_t value) {
        const uint32_t entries = (s->count >= 1 && s->count <= 8) ? s->count : 1;      // (a refused count: one entry, never read)
        uint32_t* probes = (uint32_t*)std::malloc(sizeof(uint32_t) * entries);
        if (!probes) std::exit(2);
        for (uint32_t l = 0; l < entries; ++l) probes[l] = 1;            // (allowed in every entry of good())
        if (at < entries) probes[at] = value;
        CHECK(rts::softListProbesOk(s, probes), probesSlow(s, probes), "%s %u %u entry %u probe %u", what, a, b, at, value);
        std::free(probes);
    };
    good(3);
    {
        const uint32_t zeros[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        CHECK(rts::softListProbesOk(nullptr, zeros), false, "softListProbesOk(NULL, probes)");
        CHECK(rts::softListProbesOk(s, nullptr), false, "softListProbesOk(list, NULL)");
        CHECK(rts::softListProbesOk(nullptr, nullptr), false, "softListProbesOk(NULL, NULL)");
        CHECK(rts::softListProbesOk(s, zeros), true, "all zeros");
    }
    // every (nsamples, probe) around the ranges, in the first and in the last entry of a list
    for (uint32_t ns = 0; ns <= 50; ++ns) for (uint32_t k = 0; k <= 51; ++k)
        for (uint32_t count : { 1u, 3u, 8u }) for (uint32_t at : { 0u, count - 1u }) {
            good(count);
            s->lights[at].nsamples = ns; s->lights[at].first = 0;
            check("nsamples, probe", ns, k, at, k);
            const bool want = ns <= 48 && (k == 0 || k + 1 <= (ns < 1 ? 1 : ns));
            good(count);
            s->lights[at].nsamples = ns; s->lights[at].first = 0;
            uint32_t probes[8] = { 1, 1, 1, 1, 1, 1, 1, 1 };
            probes[at] = k;
            CHECK(rts::softListProbesOk(s, probes), want, "nsamples %u probe %u entry %u of %u", ns, k, at, count);
        }
    // a hard entry accepts 0 alone
    for (uint32_t ns : { 0u, 1u }) for (uint32_t k : { 0u, 1u, 2u }) {
        good(2); s->lights[1].nsamples = ns;
        uint32_t probes[2] = { 1, k };
        CHECK(rts::softListProbesOk(s, probes), k == 0, "a hard entry of nsamples %u, probe %u", ns, k);
    }
    // a probe beyond the count is not looked at
    for (uint32_t v : far) {
        good(3);
        uint32_t probes[8] = { 1, 1, 1, v, v, v, v, v };
        CHECK(rts::softListProbesOk(s, probes), true, "a probe %u beyond the count", v);
        for (uint32_t at : { 0u, 2u }) {
            check("far probe", v, 0, at, v);
            uint32_t p2[3] = { 1, 1, 1 };
            p2[at] = v;
            CHECK(rts::softListProbesOk(s, p2), false, "probe %u in entry %u", v, at);
        }
    }
    // lists the list rule refuses are refused whatever the probes
    for (uint32_t count : { 0u, 9u, 0xFFFFFFFFu }) { good(count); check("count", count, 0, 0, 0); CHECK(rts::softListOk(s), false, "count %u", count); }
    {
        const uint32_t zeros[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        good(8); s->lights[7].type = 2;
        CHECK(rts::softListProbesOk(s, zeros), false, "a type of 2");
        good(8); s->lights[3].nsamples = 49;
        CHECK(rts::softListProbesOk(s, zeros), false, "49 samples");
        good(8); s->lights[3].nsamples = 2; s->lights[3].first = 47;
        CHECK(rts::softListProbesOk(s, zeros), false, "a range past slot 48");
        good(8); s->lights[0].radius = std::numeric_limits<float>::infinity();
        CHECK(rts::softListProbesOk(s, zeros), false, "an infinite radius");
        good(8); s->lights[0].radius = std::numeric_limits<float>::quiet_NaN();
        CHECK(rts::softListProbesOk(s, zeros), false, "a NaN radius");
    }
    // the ends of the ranges
    good(1); s->lights[0].nsamples = 48; s->lights[0].first = 0;
    { uint32_t p[1] = { 47 }; CHECK(rts::softListProbesOk(s, p), true, "probe 47 of 48"); }
    { uint32_t p[1] = { 48 }; CHECK(rts::softListProbesOk(s, p), false, "probe 48 of 48"); }
    s->lights[0].nsamples = 2; s->lights[0].first = 46;
    { uint32_t p[1] = { 1 }; CHECK(rts::softListProbesOk(s, p), true, "probe 1 of 2"); }
    { uint32_t p[1] = { 2 }; CHECK(rts::softListProbesOk(s, p), false, "probe 2 of 2"); }
    std::free(s);
    std::printf("ok %lu\n", cases);
    return 0;
}
