// Interface between rts_api.cpp (the context, the schedule) and the refit kernels (rts_refit.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rts {

enum { REFIT_ERR_NONFINITE = 1u, REFIT_ERR_INDEX = 2u };

// What one refit leaves on the device; read back in one copy at its end.
struct RefitStatus {
    uint32_t err;                // REFIT_ERR_*: nothing was written
    uint32_t valid;              // validateKernel's flags of the refitted stream (rts_wide.hip)
    uint32_t pad[2];
    double cost, rootArea;       // sum of surfaceArea over inner nodes, the root's, after the refit
    double baseCost, baseRootArea;   // the same before it (only with RefitLaunch::baseline)
};

struct RefitLaunch {
    void* d_packed; uint32_t P;
    const float* verts; size_t vertexFloats; uint32_t stride; const uint32_t* indices;   // device pointers
    const uint32_t* roots; uint32_t nRoots; uint32_t treelet;        // treelet roots (subtrees of <= treelet nodes)
    const uint32_t* top; const uint32_t* levelOff; uint32_t nLevels;  // inner nodes above them, grouped by height
    void* d_wide; uint32_t wideCount; void* d_tris; const uint32_t* d_parents;   // the private copy (wideCount 0: none)
    RefitStatus* status;
    bool baseline;               // also the cost proxy of the stream as it is before the refit
};

size_t refitLdsBytes(uint32_t treelet);
hipError_t refitSetLds(uint32_t treelet);          // once per treelet size above 1024 (more than 64 KB of LDS)
hipError_t refitLaunch(const RefitLaunch& launch); // default stream, asynchronous

} // namespace rts
