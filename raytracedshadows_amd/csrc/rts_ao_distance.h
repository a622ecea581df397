// Internal interface between the C-ABI layer (rts_api.cpp) and the AO distance kernels (rts_ao_distance.inc, compiled with
// rts_kernels.hip): beside rts_device.h, whose text is part of the kernel-build hash that the committed counter profiles carry.
#pragma once
#include <string.h>
#include "rts_ao.h"

namespace rts {

// AO distance traces, p.nsamples in [1, 48]: the AO trace's count (to p.mask, which may be NULL here), the nearest blocker over the
// pixel's samples and the falloff-weighted obscurance (include/rts.h).  TraceParams keeps its size and its text.  The slots of an AO
// launch stay what rts_ao.h says -- the normals keep the distances' slot --; what this trace adds travels in slots no AO kernel reads:
//   p.pieceClock       = the distance plane, W x H floats, or NULL    (the piece path's diagnostics pointer: only a split table's piece
//                                                                      walk in the mask kernels reads it, and a block trace never runs
//                                                                      one -- the slot of the adaptive form's refined plane and of the
//                                                                      bent plane, rts_ao_adaptive.h, rts_ao_bent.h)
//   p.nrays            = the obscurance plane, W x H uint16_t, or NULL (the generic rays' count, 64 bits: the adaptive forms carry their
//                                                                      probe count in it; no other block trace reads it)
//   p.offsets[b][3]    = falloff->weight[b] as a uint32_t, b < 64      (the .w of the 64 direction entries: every AO kernel reads x, y
//                                                                      and z of an entry alone.  All 64 are written, whatever the table
//                                                                      size; zeros without an obscurance plane)
// At least one of the two planes is given; the kernels branch on either pointer per wave.
inline void setAoDistance(TraceParams& p, float* d_distance, uint16_t* d_obscurance, const uint8_t* weight64) {
    p.pieceClock = (uint64_t*)d_distance;
    p.nrays = (uint64_t)(uintptr_t)d_obscurance;
    for (int b = 0; b < 64; ++b) {
        const uint32_t w = (d_obscurance && weight64) ? weight64[b] : 0u;
        memcpy(&p.offsets[b][3], &w, 4);
    }
}

// V_SHARE, or V_PACKET with 4 waves per tile (p.softSplit) or one.  *name: the kernel's stable name.
hipError_t launchAmbientOcclusionDistance(int variant, const TraceParams& p, hipStream_t stream, const char** name);

} // namespace rts
