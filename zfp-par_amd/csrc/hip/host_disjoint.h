// Host shim: do any two of these block boxes intersect?  The exact test behind
// the batched region encode's rule that no block belongs to two entries
// (kernels_boxes_enc.h).  No HIP call: compiles on the CPU (tests/emu).
//
// A box is an entry's range of blocks in the coded box's block grid, per axis
// [b0, b0 + nb), nb >= 1; axes the field does not have are [0, 1).
//
// Sweep along one axis (the slowest the field has): the entry numbers are
// sorted by their first block on it, and an active list holds the entries
// whose last block on that axis is not below the current entry's first.
// Whatever is in the list intersects the current entry on the sweep axis, so
// it is tested against it on the other axes, box against box.
//
// Cost: the sort's O(n log n) plus one box test per (entry, active entry)
// pair.  Batches spread along the sweep axis keep the list short.  The worst
// case is n entries that all share a plane of the sweep axis without sharing a
// block (coplanar tiles, or any 1D-thin batch laid out along another axis):
// the list never shrinks and the test count is n (n - 1) / 2, 2.1e9 for the
// 65,536 entries a call may have.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace zfp_amd {

struct BlockBox {
  uint32_t b0[3];  // first block per axis
  uint32_t nb[3];  // blocks per axis (>= 1)
};

inline bool block_boxes_meet(const BlockBox& p, const BlockBox& q)
{
  for (int a = 0; a < 3; a++)
    if ((uint64_t)p.b0[a] + p.nb[a] <= q.b0[a] || (uint64_t)q.b0[a] + q.nb[a] <= p.b0[a])
      return false;
  return true;
}

// True when two of the n boxes share a block; *ia < *ib are then the entry
// numbers of the first such pair the sweep meets (a true intersection, not
// necessarily the pair with the lowest numbers).  axis: the sweep axis, 0..2.
inline bool first_shared_block(const BlockBox* box, size_t n, int axis, size_t* ia, size_t* ib)
{
  if (n < 2)  // (a single entry needs no test)
    return false;
  std::vector<uint32_t> order(n);
  for (size_t i = 0; i < n; i++)
    order[i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    return box[x].b0[axis] != box[y].b0[axis] ? box[x].b0[axis] < box[y].b0[axis] : x < y;
  });
  std::vector<uint32_t> active;
  for (size_t k = 0; k < n; k++) {
    const uint32_t e = order[k];
    const uint64_t first = box[e].b0[axis];
    size_t keep = 0;
    for (size_t m = 0; m < active.size(); m++) {
      const uint32_t o = active[m];
      if ((uint64_t)box[o].b0[axis] + box[o].nb[axis] <= first)  // ended below: dropped for good
        continue;
      if (block_boxes_meet(box[o], box[e])) {
        *ia = std::min(o, e);
        *ib = std::max(o, e);
        return true;
      }
      active[keep++] = o;
    }
    active.resize(keep);
    active.push_back(e);
  }
  return false;
}

}  // namespace zfp_amd
