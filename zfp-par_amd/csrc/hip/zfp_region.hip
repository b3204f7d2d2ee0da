// Region decode kernels (kernels_region.h): every instantiation the host can
// select -- float and double 3D through decode_block3 (double also with planes
// 32..63 only), 1D/2D of every scalar type and 3D integers through
// decode_block_n, the set that region_dispatch.h spells out -- and the
// start-table kernel.
#include "kernels_region.h"
#include "region_dispatch.h"

namespace zfp_amd {

void launch_decode_region(int type, int dims, bool rev, bool hi, hipStream_t stream, dim3 grid, size_t lds, void* dst,
                          const Geometry& g, const CodecParams& cp, const RegionGeom& rg, const RegionArgs& a)
{
  by_region_kernel(type, dims, hi, [&](auto tag, auto hi_tag, auto dims_tag) {
    using S = std::remove_pointer_t<decltype(tag)>;
    constexpr bool HI = decltype(hi_tag)::value;
    constexpr int D = decltype(dims_tag)::value;
    if (rev)
      hipLaunchKernelGGL((decode3_region<S, true, HI, D>), grid, dim3(256), lds, stream, (S*)dst, g, cp, rg, a);
    else
      hipLaunchKernelGGL((decode3_region<S, false, HI, D>), grid, dim3(256), lds, stream, (S*)dst, g, cp, rg, a);
  });
}

void launch_start_table(hipStream_t stream, const uint16_t* len, const uint64_t* base, uint64_t nblocks,
                        uint64_t nwaves, uint32_t per_wave, uint64_t* start)
{
  const unsigned groups = (unsigned)((nwaves + kWavesPerGroup - 1) / kWavesPerGroup);
  hipLaunchKernelGGL(build_start_table, dim3(groups), dim3(256), 0, stream, len, base, nblocks, nwaves, per_wave,
                     start);
}

}  // namespace zfp_amd
