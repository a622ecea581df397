// Internal interface between the C-ABI layer (rts_api.cpp) and the light list kernels (rts_light_list.inc, compiled with
// rts_kernels.hip): beside rts_device.h, whose text is part of the kernel-build hash that the committed counter profiles carry.
#pragma once
#include "rts_device.h"

namespace rts {

// light list traces: p.nsamples = the number of lights (1..8 = RTS_MAX_LIST_LIGHTS), light l in p.offsets[l] = {x, y, z, 0.0f directional / 1.0f point},
// p.activeMap = the per-pixel light map (bit l: light l sends a ray here) or NULL (every light everywhere); bit l of p.mask[pixel] =
// light l's shadow byte.  V_SHARE, or V_PACKET with 4 waves per tile (p.softSplit) or one.  *name: the kernel's stable name.
hipError_t launchShadowLightList(int variant, const TraceParams& p, hipStream_t stream, const char** name);

} // namespace rts
