// Internal interface between the C-ABI layer (rts_api.cpp) and the bent-normal ambient occlusion kernels (rts_ao_bent.inc, compiled
// with rts_kernels.hip): beside rts_device.h, whose text is part of the kernel-build hash that the committed counter profiles carry.
#pragma once
#include "rts_ao.h"

namespace rts {

// bent AO traces, p.nsamples in [1, 48]: the AO trace's count (to p.mask, which may be NULL here) and, per pixel, the frame applied to
// the integer sum of the unoccluded samples' quantised directions (include/rts.h).  TraceParams keeps its size and its text.  The slots
// of an AO launch stay what rts_ao.h says; the one value this trace adds travels in a slot no AO kernel reads:
//   p.pieceClock = the bent plane, W x H RGBA32F, never NULL  (the piece path's diagnostics pointer: only a split table's piece walk in
//                                                              the mask kernels reads it, and a block trace never runs one -- the slot
//                                                              the adaptive form's refined plane takes, rts_ao_adaptive.h)
inline void setAoBent(TraceParams& p, float* d_bent) { p.pieceClock = (uint64_t*)d_bent; }

// V_SHARE, or V_PACKET with 4 waves per tile (p.softSplit) or one.  *name: the kernel's stable name.
hipError_t launchAmbientOcclusionBent(int variant, const TraceParams& p, hipStream_t stream, const char** name);

} // namespace rts
