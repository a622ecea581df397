// Internal interface between the C-ABI layer (rts_api.cpp) and the adaptive ambient occlusion kernels (rts_ao_adaptive.inc, compiled
// with rts_kernels.hip): beside rts_device.h, whose text is part of the kernel-build hash that the committed counter profiles carry.
#pragma once
#include "rts_ao.h"

namespace rts {

// adaptive AO traces, p.nsamples in [2, 48]: the first `probe` samples of every live pixel, the others only where the probe disagrees
// (include/rts.h).  TraceParams keeps its size and its text.  The slots of an AO launch stay what rts_ao.h says (the normals in
// p.distance, the counts in p.mask, the radius in p.light[0], the directions in p.offsets, the table in p.lightTable, the active map in
// p.activeMap); the two values this trace adds travel in slots no block trace reads:
//   p.nrays      = probe, in [1, p.nsamples - 1]            (the generic rays' count, as in rts_adaptive.h)
//   p.pieceClock = the refined plane, W x H bytes, or NULL  (the piece path's diagnostics pointer: only a split table's piece walk in
//                                                            the mask kernels reads it, and a block trace never runs one)
// rts_adaptive.h carries its refined plane in p.out; here that union holds the normals, and the generic rays' input pointer shares
// its slot with the active map -- hence a third one.
inline void setAoRefined(TraceParams& p, uint8_t* d_refined) { p.pieceClock = (uint64_t*)d_refined; }

// V_SHARE, or V_PACKET with 4 waves per tile (p.softSplit) or one.  *name: the kernel's stable name.
hipError_t launchAmbientOcclusionAdaptive(int variant, const TraceParams& p, hipStream_t stream, const char** name);

} // namespace rts
