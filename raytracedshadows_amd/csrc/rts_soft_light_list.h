// Internal interface between the C-ABI layer (rts_api.cpp) and the soft light list kernels (rts_soft_light_list.inc, compiled with
// rts_kernels.hip): beside rts_device.h, whose text is part of the kernel-build hash that the committed counter profiles carry.
#pragma once
#include "rts_device.h"
#include "rts_soft_list_slots.h"

namespace rts {

// soft light list traces (include/rts.h).  TraceParams keeps its size and layout; the list travels in the 64 sample offsets:
//   p.nsamples                          = the number of lights, 1..8 (RTS_MAX_LIST_LIGHTS)
//   p.offsets[j], j < 48                = the list's shared sample table (RTS_SOFT_LIST_OFFSETS entries; .w is not read)
//   p.offsets[48 + 2 l]                 = { x, y, z, radius } of light l
//   p.offsets[48 + 2 l + 1]             = the bit patterns of { type, samples = max(1, nsamples), first (0 for a hard entry), 0 }
// (rts_soft_list_slots.h writes the two slots of light l, setSoftListEntry, and has the launchers' guard of them, softListSlotsOk.)
// p.activeMap = the per-pixel light map (bit l: light l sends its rays here) or NULL (every light everywhere); p.mask = the count
// planes, plane l at p.mask + l * W * H: the number of unoccluded samples of light l.  p.lightTable is 0: a list's per-pixel jitter
// tables, where it has any, travel per light (rts_soft_light_list_adaptive.h).  V_SHARE, or V_PACKET with 4 waves per tile (p.softSplit) or one.  *name: the kernel's stable name.
hipError_t launchShadowSoftLightList(int variant, const TraceParams& p, hipStream_t stream, const char** name);

} // namespace rts
