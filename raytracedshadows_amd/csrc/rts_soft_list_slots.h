// The slots of a soft light list in the 64 x 4 floats of TraceParams::offsets (rts_soft_light_list.h, rts_soft_light_list_adaptive.h:
// what travels where), as the C-ABI layer writes them and as every soft list launcher checks them before it launches.  Host only and
// nothing of HIP: the block is passed as it is, so tests/cpp/soft_list_slots_host.cpp checks the guard under the host sanitizers.
// The kernels' readers (makeSoftListRay, softListSamples, softListProbe, softListTable, softListSampleAt) index the same slots.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/rts.h"

namespace rts {

constexpr uint32_t SOFT_LIST_SLOT = 48;                  // offsets[48 + 2 l], [48 + 2 l + 1]: light l; the shared table lies below

// { x, y, z, radius } and the bit patterns of { type, samples, first, k_l = 0 } of light l
inline void setSoftListEntry(float (*offsets)[4], uint32_t l, uint32_t type, uint32_t samples, uint32_t first, float radius, const float* xyz) {
    float* a = offsets[SOFT_LIST_SLOT + 2u * l];
    a[0] = xyz[0]; a[1] = xyz[1]; a[2] = xyz[2]; a[3] = radius;
    const uint32_t bits[4] = { type, samples, first, 0u };
    memcpy(offsets[SOFT_LIST_SLOT + 2u * l + 1u], bits, sizeof(bits));
}

// A list softListOk accepts (rts_args.h): the shared table, then the two slots of every light -- a hard entry as one sample from 0
inline void setSoftList(float (*offsets)[4], const rts_soft_light_list* list) {
    static_assert(sizeof(list->offsets) == sizeof(float) * 4 * RTS_SOFT_LIST_OFFSETS && RTS_SOFT_LIST_OFFSETS == SOFT_LIST_SLOT &&
                  RTS_SOFT_LIST_OFFSETS + 2 * RTS_MAX_LIST_LIGHTS == 64, "48 sample slots and two slots per light fill TraceParams::offsets");
    memcpy(offsets, list->offsets, sizeof(list->offsets));
    for (uint32_t l = 0; l < list->count; ++l) {
        const rts_soft_light_entry& e = list->lights[l];
        const bool soft = e.nsamples >= 2;
        setSoftListEntry(offsets, l, e.type, soft ? e.nsamples : 1u, soft ? e.first : 0u, e.radius, e.xyz);
    }
}

// k_l, the probe count of light l: after setSoftListEntry, which writes 0 there
inline void setSoftListProbe(float (*offsets)[4], uint32_t l, uint32_t probe) {
    memcpy(&offsets[SOFT_LIST_SLOT + 2u * l + 1u][3], &probe, sizeof(probe));
}

// T_l, the table size of light l, in the .w of the shared table's entry l: after the table was copied in
inline void setSoftListTable(float (*offsets)[4], uint32_t l, uint32_t table) {
    memcpy(&offsets[l][3], &table, sizeof(table));
}

// What keeps every index of the kernels inside the block: 1..8 lights, each of a known type and 1..48 samples, a soft light's range
// [first, first + samples) below slot 48.  probes: k_l < samples as well.  tables: T_l is looked at too -- 0, or samples .. 48 - first
// on a soft entry, so that first + sampleIndexOf(...) < SOFT_LIST_SLOT for every pixel.
inline bool softListSlotsOk(const float (*offsets)[4], uint32_t count, bool probes, bool tables) {
    if (count < 1 || count > 8) return false;
    for (uint32_t l = 0; l < count; ++l) {
        uint32_t bits[4], table;                                         // { type, samples, first, k_l }
        memcpy(bits, offsets[SOFT_LIST_SLOT + 2u * l + 1u], sizeof(bits));
        memcpy(&table, &offsets[l][3], sizeof(table));
        if (bits[0] > 1u || bits[1] < 1u || bits[1] > SOFT_LIST_SLOT || (bits[1] > 1u && (uint64_t)bits[2] + bits[1] > SOFT_LIST_SLOT))
            return false;
        if (probes && bits[3] >= bits[1]) return false;
        if (tables && table != 0u && (bits[1] < 2u || table < bits[1] || (uint64_t)bits[2] + table > SOFT_LIST_SLOT)) return false;
    }
    return true;
}

} // namespace rts
