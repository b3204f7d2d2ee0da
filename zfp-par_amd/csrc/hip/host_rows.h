// Host shim: the rows of a region in a strided host array <-> the region's
// packed image (x fastest, no gaps).  No HIP call in here: region_to_host and
// region_from_host put the device copy around it, and tests/emu/rows_emu.cpp
// runs it on the CPU.
#pragma once

#include <cstdint>
#include <cstring>

// ext: the region's extents, x first, 1 on the axes from `dims` on; hs: the
// host array's element strides (hs[k] for k >= dims is not read).
static bool region_is_dense(const uint64_t ext[3], int dims, const int64_t* hs)
{
  return hs[0] == 1 && (dims < 2 || hs[1] == (int64_t)ext[0]) && (dims < 3 || hs[2] == (int64_t)(ext[0] * ext[1]));
}

// to_host: packed -> host, else host -> packed.  `host` points at the region's
// first element; only the region's bytes are read or written there.
static void region_rows(const uint64_t ext[3], int dims, size_t es, const int64_t* hs, void* host, void* packed,
                        bool to_host)
{
  const size_t row = (size_t)ext[0] * es;
  const int64_t sy = dims > 1 ? hs[1] : 0, sz = dims > 2 ? hs[2] : 0;
  for (uint64_t z = 0; z < ext[2]; z++)
    for (uint64_t y = 0; y < ext[1]; y++) {
      char* p = (char*)packed + (z * ext[1] + y) * row;
      char* h = (char*)host + ((int64_t)y * sy + (int64_t)z * sz) * (int64_t)es;
      if (hs[0] == 1) {
        to_host ? memcpy(h, p, row) : memcpy(p, h, row);
        continue;
      }
      for (uint64_t x = 0; x < ext[0]; x++) {
        char* hx = h + (int64_t)x * hs[0] * (int64_t)es;
        to_host ? memcpy(hx, p + x * es, es) : memcpy(p + x * es, hx, es);
      }
    }
}
