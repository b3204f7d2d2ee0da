// Batched region decode kernels (kernels_boxes.h): the instantiations of
// zfp_region.hip (region_dispatch.h) -- float and double 3D through
// decode_block3 (double also with planes 32..63 only), 1D/2D of every scalar
// type and 3D integers through decode_block_n.
#include "kernels_boxes.h"
#include "region_dispatch.h"

namespace zfp_amd {

void launch_decode_boxes(int type, int dims, bool rev, bool hi, hipStream_t stream, dim3 grid, size_t lds,
                         const BoxesArgs& b, const Geometry& g, const CodecParams& cp, const RegionArgs& a)
{
  by_region_kernel(type, dims, hi, [&](auto tag, auto hi_tag, auto dims_tag) {
    using S = std::remove_pointer_t<decltype(tag)>;
    constexpr bool HI = decltype(hi_tag)::value;
    constexpr int D = decltype(dims_tag)::value;
    if (rev)
      hipLaunchKernelGGL((decode3_boxes<S, true, HI, D>), grid, dim3(256), lds, stream, b, g, cp, a);
    else
      hipLaunchKernelGGL((decode3_boxes<S, false, HI, D>), grid, dim3(256), lds, stream, b, g, cp, a);
  });
}

}  // namespace zfp_amd
