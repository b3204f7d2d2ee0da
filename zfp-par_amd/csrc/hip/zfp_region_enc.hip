// Region encode kernels (kernels_region_enc.h): every instantiation the host
// can select -- float and double 3D through decode_block3 / encode_block3
// (double also with planes 32..63 only), 1D/2D of every scalar type and 3D
// integers through the generic per-lane codec (region_dispatch.h).  Fixed rate
// only: there is no reversible form.
#include "kernels_region_enc.h"
#include "region_dispatch.h"

namespace zfp_amd {

void launch_encode_region(int type, int dims, bool hi, hipStream_t stream, dim3 grid, size_t lds, const void* src,
                          const Geometry& g, const CodecParams& cp, const RegionGeom& rg, const RegionEncArgs& a)
{
  by_region_kernel(type, dims, hi, [&](auto tag, auto hi_tag, auto dims_tag) {
    using S = std::remove_pointer_t<decltype(tag)>;
    constexpr bool HI = decltype(hi_tag)::value;
    constexpr int D = decltype(dims_tag)::value;
    hipLaunchKernelGGL((encode3_region<S, HI, D>), grid, dim3(256), lds, stream, (const S*)src, g, cp, rg, a);
  });
}

}  // namespace zfp_amd
