// The argument rules of include/rts.h that the library (rts_api.cpp) and its host twins (rts_scene.cpp) both apply, written once.
// Host only: nothing of HIP (tests/cpp/args_host.cpp checks them against slow restatements).
#pragma once
#include <string.h>
#include "../../include/rts.h"

namespace rts {

// a hard light: NULL (the constants' directional light), or a known type with one sample
inline bool hardLightOk(const rts_light* light) {
    return !light || (light->type <= RTS_LIGHT_POINT && light->nsamples <= 1);
}

// a light of up to 64 samples; a table (per-pixel jitter) holds nsamples..64 entries and needs at least 2 samples
inline bool softLightOk(const rts_light* light) {
    return !light || (light->type <= RTS_LIGHT_POINT && light->nsamples <= 64 &&
                      (!light->table || (light->table <= 64 && light->table >= light->nsamples && light->nsamples >= 2)));
}

// an adaptive trace: a light that MUST be there, of 2..64 samples (softLightOk's type and table rules), and a probe of 1..nsamples - 1
inline bool adaptiveLightOk(const rts_light* light, uint32_t probe) {
    return light && light->nsamples >= 2 && softLightOk(light) && probe >= 1 && probe < light->nsamples;
}

// a light list: 1..RTS_MAX_LIST_LIGHTS lights of known types
inline bool lightListOk(const rts_light_list* list) {
    if (!list || list->count == 0 || list->count > RTS_MAX_LIST_LIGHTS) return false;
    for (uint32_t l = 0; l < list->count; ++l) if (list->lights[l].type > RTS_LIGHT_POINT) return false;
    return true;
}

// a soft light list: 1..RTS_MAX_LIST_LIGHTS entries of known types, each of at most RTS_SOFT_LIST_OFFSETS samples with a finite radius;
// a soft entry's range [first, first + nsamples) lies inside the shared table (a hard entry's `first` is not looked at)
inline bool softListOk(const rts_soft_light_list* list) {
    if (!list || list->count == 0 || list->count > RTS_MAX_LIST_LIGHTS) return false;
    for (uint32_t l = 0; l < list->count; ++l) {
        const rts_soft_light_entry& e = list->lights[l];
        if (e.type > RTS_LIGHT_POINT || e.nsamples > RTS_SOFT_LIST_OFFSETS) return false;
        if (e.nsamples >= 2 && (uint64_t)e.first + e.nsamples > RTS_SOFT_LIST_OFFSETS) return false;
        uint32_t bits;
        memcpy(&bits, &e.radius, sizeof(bits));
        if ((bits & 0x7F800000u) == 0x7F800000u) return false;           // Inf or NaN: every exponent bit set
    }
    return true;
}

// the probe counts of an adaptive soft light list trace, one per entry below the count of a list softListOk accepts: 0 (the light is
// traced in full) or 1 .. max(1, nsamples) - 1 -- so a hard entry accepts 0 alone.  Entries of probes[] from the count up are not read.
inline bool softListProbesOk(const rts_soft_light_list* list, const uint32_t* probes) {
    if (!probes || !softListOk(list)) return false;
    for (uint32_t l = 0; l < list->count; ++l) {
        const uint32_t n = list->lights[l].nsamples > 1u ? list->lights[l].nsamples : 1u;
        if (probes[l] >= n) return false;
    }
    return true;
}

// the probe counts and the per-pixel table sizes of a jittered soft light list trace: softListProbesOk, and per entry below the count
// a table of 0 (none), or on a SOFT entry one of nsamples .. RTS_SOFT_LIST_OFFSETS - first entries -- the table starts at the light's
// `first` and must hold every sample and end inside the shared table.  tables == NULL stands for all zeros.  Entries of tables[] from
// the count up are not read.
inline bool softListTablesOk(const rts_soft_light_list* list, const uint32_t* probes, const uint32_t* tables) {
    if (!softListProbesOk(list, probes)) return false;
    for (uint32_t l = 0; tables && l < list->count; ++l) {
        const rts_soft_light_entry& e = list->lights[l];
        if (tables[l] == 0u) continue;
        if (e.nsamples < 2u || tables[l] < e.nsamples || (uint64_t)e.first + tables[l] > RTS_SOFT_LIST_OFFSETS) return false;
    }
    return true;
}

// whether any entry below the count has a table (a list softListTablesOk accepts)
inline bool softListHasTable(const rts_soft_light_list* list, const uint32_t* tables) {
    for (uint32_t l = 0; tables && l < list->count; ++l) if (tables[l] != 0u) return true;
    return false;
}

// an ambient occlusion trace: at most RTS_AO_MAX_SAMPLES samples, a finite radius, and softLightOk's table rule over RTS_AO_MAX_DIRS
inline bool aoParamsOk(const rts_ao_params* ao) {
    if (!ao || ao->nsamples > RTS_AO_MAX_SAMPLES) return false;
    if (ao->table && (ao->table > RTS_AO_MAX_DIRS || ao->table < ao->nsamples || ao->nsamples < 2)) return false;
    uint32_t bits;
    memcpy(&bits, &ao->radius, sizeof(bits));
    return (bits & 0x7F800000u) != 0x7F800000u;                          // Inf or NaN: every exponent bit set
}

// an adaptive ambient occlusion trace: aoParamsOk's rules, at least 2 samples, and a probe of 1..nsamples - 1
inline bool aoAdaptiveOk(const rts_ao_params* ao, uint32_t probe) {
    return aoParamsOk(ao) && ao->nsamples >= 2 && probe >= 1 && probe < ao->nsamples;
}

// the pixel list of a sparse list trace: the list and its length (on the device in the device forms) and room for at least one entry
inline bool sparseListOk(const uint32_t* pixels, const uint32_t* n, uint32_t capacity) {
    return pixels && n && capacity != 0;
}

// a frame and its row range [row_begin, row_end), which may be empty
inline bool frameRowsOk(uint32_t W, uint32_t H, uint32_t row_begin, uint32_t row_end) {
    return W != 0 && H != 0 && row_begin <= row_end && row_end <= H;
}

} // namespace rts
