// Internal interface between the C-ABI layer (rts_api.cpp) and the sparse light list kernels (rts_light_list_sparse.inc, compiled with
// rts_kernels.hip): beside rts_device.h, whose text is part of the kernel-build hash that the committed counter profiles carry.
#pragma once
#include "rts_device.h"

namespace rts {

// sparse list traces (include/rts.h): p as launchShadowLightList / launchShadowSoftLightList take it -- the lights, the map, the
// planes, W and H; the grid's and the row range's members are not read -- and beside it, as kernel arguments of their own, the list of
// pixel indices, its length (both on the device, read by the kernel) and the capacity.  ceil(capacity / 256) workgroups of 256 lanes,
// lane i owns pixels[i] for i < min(*d_n, capacity).  *name: the kernel's stable name.
hipError_t launchShadowLightListSparse(const TraceParams& p, const uint32_t* d_pixels, const uint32_t* d_n, uint32_t capacity,
                                       hipStream_t stream, const char** name);
hipError_t launchShadowSoftLightListSparse(const TraceParams& p, const uint32_t* d_pixels, const uint32_t* d_n, uint32_t capacity,
                                           hipStream_t stream, const char** name);

} // namespace rts
