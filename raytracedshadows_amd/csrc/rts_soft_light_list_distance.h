// Internal interface between the C-ABI layer (rts_api.cpp) and the soft light list distance kernels (rts_soft_light_list_distance.inc,
// compiled with rts_kernels.hip): beside rts_device.h, whose text is part of the kernel-build hash that the committed counter profiles carry.
#pragma once
#include "rts_device.h"

namespace rts {

// soft light list distance traces (include/rts.h).  TraceParams keeps its size and layout; the list travels in the slots of
// rts_soft_light_list.h (p.nsamples the number of lights, the shared table and two slots per light in p.offsets, setSoftListEntry),
// the light map in p.activeMap (or NULL).  p.distance = the distance planes, plane l at p.distance + l * W * H floats: the minimum of
// light l's samples' one-ray distances; p.mask = the count planes of the soft light list, or NULL.  V_SHARE, or V_PACKET with 4 waves
// per tile (p.softSplit) or one.  *name: the kernel's stable name.
hipError_t launchShadowSoftLightListDistance(int variant, const TraceParams& p, hipStream_t stream, const char** name);

} // namespace rts
