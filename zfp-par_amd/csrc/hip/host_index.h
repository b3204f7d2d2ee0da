// Host shim: the block index of a variable-rate stream and its device storage.
#pragma once

#include <algorithm>
#include <cstdint>

#include "host_error.h"
#include "zfp_hip.h"

// block index (variable-rate streams)
// An index describes one stream: it records the codec settings, the layout
// and a fingerprint of the stream's words (stream_fingerprint), and is used
// only for a stream that matches all of them (index_matches) -- another
// stream of the same shape, a changed mode or a rewritten buffer is scanned.
// What the launchers read and write of an index: the layout and the two device
// arrays, which it borrows.  It is the whole of a zfp_hip_index, or the part of
// one that a slab covers (index_view); only a zfp_hip_index owns, grows and
// frees the arrays (index_reserve, index_release take nothing else).
struct IndexView {
  int device = -1;
  uint64_t nblocks = 0;
  uint64_t nwaves = 0;
  uint32_t per_wave = 0;       // blocks per wave of the layout it was made for (64: 3D, 16: 4D)
  uint64_t total_bits = 0;
  uint16_t* d_len = nullptr;   // per-block bit length
  uint64_t* d_base = nullptr;  // per-wave start bit relative to the stream's first block
};

struct zfp_hip_index : IndexView {
  uint64_t start_bit = ~0ull;  // stream bit offset of block 0 it was made for
  uint64_t fp = 0;             // stream_fingerprint of the stream it was made for
  uint32_t minbits = 0, maxbits = 0, maxprec = 0;
  int32_t minexp = 0;
  int32_t type = 0, dims = 0;
  size_t cap_blocks = 0, cap_waves = 0;
  // Start table of the region decoder (host_region.h): the start bit of every
  // block, 8 bytes each.  A cache of what d_len and d_base say, so a call that
  // only reads the index may build it: built on first use, dropped whenever
  // the arrays are about to be refilled (index_reserve), freed in index_release.
  mutable uint64_t* d_start = nullptr;
  mutable size_t cap_start = 0;
  mutable bool start_valid = false;
};

static int index_reserve(zfp_hip_index* x, uint64_t nblocks, uint64_t nwaves)
{
  x->start_valid = false;  // whoever refills the arrays reserves first
  if (x->cap_blocks < nblocks) {
    if (x->d_len) (void)hipFree(x->d_len);
    x->d_len = nullptr;
    x->cap_blocks = 0;
    if (hipMalloc(&x->d_len, std::max<uint64_t>(nblocks, 1) * sizeof(uint16_t)) != hipSuccess)
      return fail("hipMalloc of the block index (%llu blocks) failed", (unsigned long long)nblocks);
    x->cap_blocks = nblocks;
  }
  if (x->cap_waves < nwaves) {
    if (x->d_base) (void)hipFree(x->d_base);
    x->d_base = nullptr;
    x->cap_waves = 0;
    if (hipMalloc(&x->d_base, std::max<uint64_t>(nwaves, 1) * sizeof(uint64_t)) != hipSuccess)
      return fail("hipMalloc of the block index (%llu waves) failed", (unsigned long long)nwaves);
    x->cap_waves = nwaves;
  }
  return 1;
}

static void index_release(zfp_hip_index* x)
{
  if (x->d_len) (void)hipFree(x->d_len);
  if (x->d_base) (void)hipFree(x->d_base);
  if (x->d_start) (void)hipFree(x->d_start);
  x->d_len = nullptr;
  x->d_base = nullptr;
  x->d_start = nullptr;
  x->cap_blocks = x->cap_waves = x->cap_start = 0;
  x->start_valid = false;
  x->nblocks = x->nwaves = 0;
  x->start_bit = ~0ull;
  x->fp = 0;
}
