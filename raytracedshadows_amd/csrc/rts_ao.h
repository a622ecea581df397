// Internal interface between the C-ABI layer (rts_api.cpp) and the ambient occlusion kernels (rts_ao.inc, compiled with
// rts_kernels.hip): beside rts_device.h, whose text is part of the kernel-build hash that the committed counter profiles carry.
#pragma once
#include "rts_device.h"

namespace rts {

// The slots of an AO launch in the argument block, which keeps its size and its text: the NORMALS (W x H RGBA32F) travel in the slot
// of the generic rays' output / the distances (p.distance), which no AO kernel writes -- counts go out through p.mask alone --; the
// radius in p.light[0]; the sample count in p.nsamples; the directions in p.offsets and their table size in p.lightTable, so the
// pixel's start is the mask kernels' own sampleIndex (with p.pixelBase); the active map in p.activeMap; p.lightType is RTS_LIGHT_POINT.
inline void setAoNormals(TraceParams& p, const float* d_normals) { p.distance = const_cast<float*>(d_normals); }

// ambient occlusion traces, p.nsamples in [1, 48]: the count of unoccluded hemisphere segments to p.mask.  V_SHARE, or V_PACKET with
// 4 waves per tile (p.softSplit) or one.  *name: the kernel's stable name.
hipError_t launchAmbientOcclusion(int variant, const TraceParams& p, hipStream_t stream, const char** name);

} // namespace rts
