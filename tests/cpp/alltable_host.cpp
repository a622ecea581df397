// Host-only view of raytracedshadows_amd/csrc/rts_alltable.h for tests/test_alltable_host.py (built as a small shared object, no
// HIP headers): the selection rule of the ALLTABLE instantiation and the per-scene constants of a root node.
#include "../../raytracedshadows_amd/csrc/rts_alltable.h"

extern "C" {

// facts: {wavesPerBlock, nsamples, wideLane, follow, table, hasPieces, allInTable, frontMap, stripes, waveStats, sceneBounds,
//         nPieces, blocksX, pieceRows}
int alltable_rule(const uint32_t* f) {
    rts::AllTableFacts a{};
    a.wavesPerBlock = f[0]; a.nsamples = f[1]; a.wideLane = f[2] != 0; a.follow = f[3] != 0; a.table = f[4] != 0; a.hasPieces = f[5] != 0;
    a.allInTable = f[6] != 0; a.frontMap = f[7] != 0; a.stripes = f[8] != 0; a.waveStats = f[9] != 0; a.sceneBounds = f[10] != 0;
    a.nPieces = f[11]; a.blocksX = f[12]; a.pieceRows = f[13];
    return rts::allTableRule(a) ? 1 : 0;
}

void alltable_scene_bounds(const uint32_t* root8, uint32_t* out9) { rts::sceneBoundsOf(root8, out9); }

uint32_t alltable_scene_bounds_dwords(void) { return rts::SCENE_BOUNDS_DWORDS; }

}
