// Internal interface between the C-ABI layer (rts_api.cpp) and the soft distance kernels (rts_soft_distance.inc, compiled with
// rts_kernels.hip): beside rts_device.h, whose text is part of the kernel-build hash that the committed counter profiles carry.
#pragma once
#include "rts_device.h"

namespace rts {

// soft distance traces, p.nsamples in [2, 64]: the minimum over the light's samples to p.distance, the count of unoccluded samples
// to p.mask (nullable).  V_SHARE, or V_PACKET with 4 waves per tile (p.softSplit) or one.  *name: the kernel's stable name.
hipError_t launchShadowSoftDistance(int variant, const TraceParams& p, hipStream_t stream, const char** name);

} // namespace rts
