// Shared by the two refit forms (bvh_refit.cpp on the host, rts_ctx_refit_bvh_device in rts_api.cpp).
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/rts.h"

namespace rts {

constexpr uint32_t kRefitEnd = 0xFFFFFFFFu;

// Topology check of a packed stream of P triangles (5P-2 vec4), one O(N) pass: a pre-order binary tree with the reference's
// miss links -- the root's link END, links strictly forward, a leaf's tail pointer in [2N, 2N+P) and its link the next node
// (END for the last), an inner node's left child i+1 and right child link(i+1) with link(right) == link(i).  Then the subtree
// of node i is exactly [i, end[i]), end[i] = link(i) or N.  RTS_OK or RTS_ERR_BAD_BVH; `end` (nullable) receives end[].
int refitTopology(const rts_vec4u* packed, uint32_t P, std::vector<uint32_t>* end);

} // namespace rts
