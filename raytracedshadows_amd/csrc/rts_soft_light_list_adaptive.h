// Internal interface between the C-ABI layer (rts_api.cpp) and the adaptive soft light list kernels (rts_soft_light_list_adaptive.inc,
// compiled with rts_kernels.hip): beside rts_device.h, whose text is part of the kernel-build hash that the committed counter profiles carry.
#pragma once
#include "rts_soft_light_list.h"

namespace rts {

// adaptive soft light list traces (include/rts.h).  TraceParams keeps its size and layout; the list travels as in
// rts_soft_light_list.h, and the two values this trace adds in slots that trace leaves alone:
//   p.offsets[48 + 2 l + 1][3] = the bit pattern of k_l, the probe count of light l: 0 (every sample, no decision) or 1 .. samples - 1
//                                (setSoftListEntry writes 0 there and the soft list kernels never read it; setSoftListProbe writes k_l
//                                 AFTER setSoftListEntry)
//   p.out                      = the refined plane, W x H bytes, bit l = light l took its full count here, or NULL (the generic rays'
//                                output, as in rts_adaptive.h)
// The jittered form (rts_trace_soft_light_list_jittered*) adds a third, the table size T_l of light l.  The two slots of a light are
// full -- { x, y, z, radius }, { type, samples, first, k_l } --, and TraceParams keeps its size, so T_l travels in the shared table:
//   p.offsets[l][3], l < p.nsamples = the bit pattern of T_l: 0 (no table) or samples .. 48 - first on a soft entry
// The .w of the 48 table entries is never read as an offset (rts_soft_light_list.h), by any list kernel; setSoftListTable writes T_l
// AFTER the table was copied in, and only the JITTER instantiations read it.  The other candidate, packing T_l beside k_l (both are
// below 64), would have changed what the existing kernels load for k_l and with it their text.
// p.pixelBase = the index in the caller's frame of the dispatch's pixel 0: the hash is the full frame's (rts_light.table).
// p.mask = the count planes, p.activeMap = the light map or NULL.  The launcher re-checks every entry and every k_l against the 64
// slots before it launches (softListSlotsOk).  V_SHARE, or V_PACKET with 4 waves per tile (p.softSplit) or one.  *name: the kernel's stable name.
hipError_t launchShadowSoftLightListAdaptive(int variant, const TraceParams& p, hipStream_t stream, const char** name);
// the same with the tables honoured: the JITTER instantiations, named "...ShareKernel<jitter>" and "...PacketKernel<S,geom,jitter>";
// the launcher checks first + T_l <= 48 as well.
hipError_t launchShadowSoftLightListJittered(int variant, const TraceParams& p, hipStream_t stream, const char** name);

} // namespace rts
