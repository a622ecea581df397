// Host-only check of rts_args.h's soft light list rule (tests/test_soft_list_args_host.py, built with -fsanitize=address,undefined):
// softListOk against a restatement of include/rts.h written the slow way -- the allowed values tried one by one -- over every
// (count, type, nsamples, first) around the allowed ranges in every entry position, radii of every class, NULL, and values far
// outside.  Prints the first case that differs and exits 1; "ok <cases>" otherwise.
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

// include/rts.h, rts_trace_soft_light_list*: count in [1, 8]; per entry below count a known type, nsamples 0..48, a soft entry's
// range inside the 48 slots, a radius that is a number and not an infinity
static bool entrySlow(const rts_soft_light_entry& e) {
    if (e.type != RTS_LIGHT_DIRECTIONAL && e.type != RTS_LIGHT_POINT) return false;
    if (std::isnan(e.radius) || std::isinf(e.radius)) return false;
    if (e.nsamples == 0 || e.nsamples == 1) return true;                 // hard: first is not looked at
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

int main() {
    static_assert(sizeof(rts_soft_light_entry) == 32 && sizeof(rts_soft_light_list) == 16 + 8 * 32 + 48 * 16, "the layout of include/rts.h");
    static_assert(RTS_SOFT_LIST_OFFSETS == 48 && RTS_MAX_LIST_LIGHTS == 8, "the limits of include/rts.h");
    const uint32_t far[] = { 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFD0u, 0xFFFFFFFEu, 0xFFFFFFFFu };
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float radii[] = { 0.0f, -0.0f, 1.0f, -2.5f, 0.3f, std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max(),
                            -std::numeric_limits<float>::max(), inf, -inf, nan, -nan };
    CHECK(rts::softListOk(nullptr), false, "softListOk(NULL)");
    // (the list lives on the heap, exactly sized: a rule that read past an rts_soft_light_list would be seen)
    rts_soft_light_list* s = (rts_soft_light_list*)std::malloc(sizeof(rts_soft_light_list));
    if (!s) return 2;
    const auto good = [&](uint32_t count) {
        std::memset(s, 0, sizeof(*s));
        s->count = count;
        for (uint32_t l = 0; l < 8; ++l) { s->lights[l].type = l & 1u; s->lights[l].nsamples = 2 + 5 * l; s->lights[l].first = l; s->lights[l].radius = 0.5f; }
    };
    // every (type, nsamples, first) around the ranges, in the first and in the last entry of a list, and beyond its count
    for (uint32_t type = 0; type <= 2; ++type) for (uint32_t ns = 0; ns <= 50; ++ns) for (uint32_t first = 0; first <= 50; ++first)
        for (uint32_t count : { 1u, 3u, 8u }) for (uint32_t at : { 0u, count - 1u, count }) {
            if (at >= 8) continue;
            good(count);
            s->lights[at].type = type; s->lights[at].nsamples = ns; s->lights[at].first = first;
            const bool want = listSlow(s);
            if (at == count && !want) { std::printf("an entry beyond the count was looked at by the restatement\n"); return 1; }
            CHECK(rts::softListOk(s), want, "softListOk count %u entry %u type %u nsamples %u first %u", count, at, type, ns, first);
        }
    for (uint32_t count = 0; count <= 10; ++count) { good(count); CHECK(rts::softListOk(s), listSlow(s), "count %u", count); }
    for (uint32_t v : far) {
        good(v);
        CHECK(rts::softListOk(s), false, "count %u", v);
        for (uint32_t at : { 0u, 7u }) {
            good(8); s->lights[at].type = v;
            CHECK(rts::softListOk(s), false, "type %u", v);
            good(8); s->lights[at].nsamples = v;
            CHECK(rts::softListOk(s), false, "nsamples %u", v);
            good(8); s->lights[at].first = v;                            // (first + nsamples wraps around for the largest values)
            CHECK(rts::softListOk(s), false, "first %u", v);
            good(8); s->lights[at].nsamples = 1; s->lights[at].first = v;
            CHECK(rts::softListOk(s), true, "a hard entry's first %u", v);
            good(8); s->lights[at].reserved_ = v; s->reserved_[at & 1u] = v;
            CHECK(rts::softListOk(s), true, "reserved_ %u", v);
        }
    }
    for (float r : radii) for (uint32_t ns : { 0u, 1u, 2u, 48u }) for (uint32_t at : { 0u, 4u, 5u }) {
        good(5); s->lights[at].nsamples = ns; s->lights[at].first = 0; s->lights[at].radius = r;
        CHECK(rts::softListOk(s), listSlow(s), "radius %g nsamples %u entry %u", (double)r, ns, at);
        CHECK(rts::softListOk(s), at >= 5 || std::isfinite(r), "radius %g entry %u", (double)r, at);
    }
    // the ends of the ranges
    good(1); s->lights[0].nsamples = 48; s->lights[0].first = 0;
    CHECK(rts::softListOk(s), true, "48 samples from 0");
    s->lights[0].first = 1;
    CHECK(rts::softListOk(s), false, "48 samples from 1");
    s->lights[0].nsamples = 2; s->lights[0].first = 46;
    CHECK(rts::softListOk(s), true, "2 samples from 46");
    s->lights[0].first = 47;
    CHECK(rts::softListOk(s), false, "2 samples from 47");
    s->lights[0].nsamples = 49; s->lights[0].first = 0;
    CHECK(rts::softListOk(s), false, "49 samples");
    std::free(s);
    std::printf("ok %lu\n", cases);
    return 0;
}
