// Host run of the region row walker (host_rows.h) against direct enumeration.
//
// Every extent in {1, 2, 3, 5} per axis, for 1D, 2D and 3D and element sizes 4
// and 8, through six host layouts: dense, a padded y stride, x stride 2, a
// negative y stride, a negative z stride, and x stride 2 with a negative y
// stride.  The host array carries a guard band on either side and the pointer
// is placed so that every element lies inside it; strides of axes the region
// does not have hold a value that would leave the array if it were read.
//
// To-host: every region element must hold the packed image's value and every
// other byte must still be the sentinel.  From-host: the packed image must
// equal direct enumeration.  region_is_dense may say yes only where the host
// layout is the packed image's, and must say yes for the packed strides.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "host_rows.h"

constexpr unsigned char kSentinel = 0xA5;
constexpr int64_t kGuard = 7;             // elements on either side
constexpr int64_t kUnread = 1000003;      // the stride of an axis the region does not have

struct Layout {
  const char* name;
  int sx, pad_y;
  bool neg_y, neg_z;
};
static const Layout kLayouts[] = {
  {"dense", 1, 0, false, false},       {"padded y", 1, 3, false, false},  {"x stride 2", 2, 0, false, false},
  {"negative y", 1, 0, true, false},   {"negative z", 1, 1, false, true}, {"x stride 2, negative y", 2, 1, true, false},
};

static long g_cases = 0, g_bad = 0;

static void bad(const char* what, const Layout& l, int dims, size_t es, const uint64_t* ext)
{
  if (g_bad++ < 10)
    printf("BAD %s: %s, %dD, %zu-byte elements, extents %llu %llu %llu\n", what, l.name, dims, es,
           (unsigned long long)ext[0], (unsigned long long)ext[1], (unsigned long long)ext[2]);
}

static void run(const Layout& l, int dims, size_t es, const uint64_t ext[3])
{
  const int64_t ypitch = l.sx * (int64_t)ext[0] + l.pad_y, zpitch = ypitch * (int64_t)ext[1] + (l.neg_z ? 2 : 0);
  int64_t hs[4] = {l.sx, l.neg_y ? -ypitch : ypitch, l.neg_z ? -zpitch : zpitch, kUnread};
  for (int k = dims; k < 3; k++)
    hs[k] = kUnread;
  // the first element's place: above the guard band and the rows that lie below it
  int64_t first = kGuard;
  if (dims > 1 && l.neg_y) first += ((int64_t)ext[1] - 1) * ypitch;
  if (dims > 2 && l.neg_z) first += ((int64_t)ext[2] - 1) * zpitch;
  const size_t count = (size_t)(ext[0] * ext[1] * ext[2]);
  const size_t host_elems = (size_t)(2 * kGuard + zpitch * (int64_t)ext[2]);
  auto offset = [&](uint64_t x, uint64_t y, uint64_t z) {
    int64_t o = first + (int64_t)x * hs[0];
    if (dims > 1) o += (int64_t)y * hs[1];
    if (dims > 2) o += (int64_t)z * hs[2];
    if (o < kGuard || o >= (int64_t)host_elems - kGuard) {
      printf("rows_emu: layout places an element in the guard band\n");
      exit(2);
    }
    return (size_t)o * es;
  };
  std::vector<unsigned char> image(count * es), host(host_elems * es), want;
  for (size_t i = 0; i < image.size(); i++)
    image[i] = (unsigned char)(1 + i % 163);  // (never the sentinel)

  // packed -> host
  std::fill(host.begin(), host.end(), kSentinel);
  want = host;
  for (uint64_t z = 0; z < ext[2]; z++)
    for (uint64_t y = 0; y < ext[1]; y++)
      for (uint64_t x = 0; x < ext[0]; x++)
        memcpy(&want[offset(x, y, z)], &image[((z * ext[1] + y) * ext[0] + x) * es], es);
  region_rows(ext, dims, es, hs, host.data() + (size_t)first * es, image.data(), true);
  g_cases++;
  if (host != want)
    bad("to host", l, dims, es, ext);

  // host -> packed
  for (size_t i = 0; i < host.size(); i++)
    host[i] = (unsigned char)(i * 131 + (i >> 8) * 17 + 3);
  std::vector<unsigned char> got(count * es, kSentinel);
  want.assign(count * es, 0);
  for (uint64_t z = 0; z < ext[2]; z++)
    for (uint64_t y = 0; y < ext[1]; y++)
      for (uint64_t x = 0; x < ext[0]; x++)
        memcpy(&want[((z * ext[1] + y) * ext[0] + x) * es], &host[offset(x, y, z)], es);
  region_rows(ext, dims, es, hs, host.data() + (size_t)first * es, got.data(), false);
  g_cases++;
  if (got != want)
    bad("from host", l, dims, es, ext);

  // dense: one copy of count * es bytes from the first element must be the walk
  if (region_is_dense(ext, dims, hs))
    for (uint64_t z = 0; z < ext[2]; z++)
      for (uint64_t y = 0; y < ext[1]; y++)
        for (uint64_t x = 0; x < ext[0]; x++)
          if (offset(x, y, z) != ((size_t)first + (z * ext[1] + y) * ext[0] + x) * es) {
            bad("dense", l, dims, es, ext);
            return;
          }
}

int main()
{
  const uint64_t sizes[4] = {1, 2, 3, 5};
  for (int dims = 1; dims <= 3; dims++)
    for (size_t es : {(size_t)4, (size_t)8})
      for (uint64_t nz : sizes)
        for (uint64_t ny : sizes)
          for (uint64_t nx : sizes) {
            if ((dims < 3 && nz != 1) || (dims < 2 && ny != 1))
              continue;
            const uint64_t ext[3] = {nx, ny, nz};
            for (const Layout& l : kLayouts)
              run(l, dims, es, ext);
            const int64_t packed[3] = {1, (int64_t)nx, (int64_t)(nx * ny)};
            g_cases++;
            if (!region_is_dense(ext, dims, packed))
              bad("packed strides not recognised as dense", kLayouts[0], dims, es, ext);
          }
  printf("mismatches %ld of %ld\n", g_bad, g_cases);
  return g_bad ? 1 : 0;
}
