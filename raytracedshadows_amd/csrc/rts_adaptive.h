// Internal interface between the C-ABI layer (rts_api.cpp) and the adaptive soft-shadow kernels (rts_adaptive.inc, compiled with
// rts_kernels.hip): beside rts_device.h, whose text is part of the kernel-build hash that the committed counter profiles carry.
#pragma once
#include "rts_device.h"

namespace rts {

// adaptive soft mask traces, p.nsamples in [2, 64]: the first `probe` samples of every live pixel, the others only where the probe
// disagrees (include/rts.h).  TraceParams keeps its layout; the two values this trace adds travel in slots no pixel trace reads:
//   p.nrays = probe, in [1, p.nsamples - 1]                     (the generic rays' count)
//   p.out   = the refined plane, W x H bytes, or NULL           (the generic rays' output; so neither follow mode's lives nor a
//                                                                distance plane exists in such a launch: the same union)
// p.mask is written, p.activeMap may be NULL.  V_SHARE, or V_PACKET with 4 waves per tile (p.softSplit) or one.  *name: the kernel's
// stable name.
hipError_t launchShadowMaskAdaptive(int variant, const TraceParams& p, hipStream_t stream, const char** name);

} // namespace rts
