// Region decode kernels (kernels_region.h): every instantiation the host can
// select -- float and double 3D through decode_block3 (double also with planes
// 32..63 only), 1D/2D of every scalar type and 3D integers through
// decode_block_n -- and the start-table kernel.
#include "kernels_region.h"

namespace zfp_amd {

namespace {

struct RegionLaunch {
  hipStream_t stream;
  dim3 grid;
  size_t lds;
  void* dst;
  const Geometry& g;
  const CodecParams& cp;
  const RegionGeom& rg;
  const RegionArgs& a;
};

template <typename S, bool HI, int D>
void region_kernel(const RegionLaunch& l, bool rev)
{
  if (rev)
    hipLaunchKernelGGL((decode3_region<S, true, HI, D>), l.grid, dim3(256), l.lds, l.stream, (S*)l.dst, l.g, l.cp, l.rg,
                       l.a);
  else
    hipLaunchKernelGGL((decode3_region<S, false, HI, D>), l.grid, dim3(256), l.lds, l.stream, (S*)l.dst, l.g, l.cp,
                       l.rg, l.a);
}

template <typename S>
void region_by_dims(const RegionLaunch& l, int dims, bool rev, bool hi)
{
  if (dims == 1)
    return region_kernel<S, false, 1>(l, rev);
  if (dims == 2)
    return region_kernel<S, false, 2>(l, rev);
  if constexpr (std::is_same<S, double>::value) {
    if (hi)
      return region_kernel<S, true, 3>(l, rev);
  }
  region_kernel<S, false, 3>(l, rev);
}

}  // namespace

void launch_decode_region(int type, int dims, bool rev, bool hi, hipStream_t stream, dim3 grid, size_t lds, void* dst,
                          const Geometry& g, const CodecParams& cp, const RegionGeom& rg, const RegionArgs& a)
{
  const RegionLaunch l{stream, grid, lds, dst, g, cp, rg, a};
  switch (type) {
    case 1: return region_by_dims<int32_t>(l, dims, rev, hi);
    case 2: return region_by_dims<int64_t>(l, dims, rev, hi);
    case 3: return region_by_dims<float>(l, dims, rev, hi);
    default: return region_by_dims<double>(l, dims, rev, hi);
  }
}

void launch_start_table(hipStream_t stream, const uint16_t* len, const uint64_t* base, uint64_t nblocks,
                        uint64_t nwaves, uint32_t per_wave, uint64_t* start)
{
  const unsigned groups = (unsigned)((nwaves + kWavesPerGroup - 1) / kWavesPerGroup);
  hipLaunchKernelGGL(build_start_table, dim3(groups), dim3(256), 0, stream, len, base, nblocks, nwaves, per_wave,
                     start);
}

}  // namespace zfp_amd
