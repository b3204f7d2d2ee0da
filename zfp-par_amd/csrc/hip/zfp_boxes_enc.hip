// Batched region encode kernels (kernels_boxes_enc.h): the instantiations of
// zfp_region_enc.hip (region_dispatch.h) -- float and double 3D through
// decode_block3 / encode_block3 (double also with planes 32..63 only), 1D/2D
// of every scalar type and 3D integers through the generic per-lane codec.
#include "kernels_boxes_enc.h"
#include "region_dispatch.h"

namespace zfp_amd {

void launch_encode_boxes(int type, int dims, bool hi, hipStream_t stream, dim3 grid, size_t lds, const BoxesArgs& b,
                         const Geometry& g, const CodecParams& cp, const RegionEncArgs& a)
{
  by_region_kernel(type, dims, hi, [&](auto tag, auto hi_tag, auto dims_tag) {
    using S = std::remove_pointer_t<decltype(tag)>;
    constexpr bool HI = decltype(hi_tag)::value;
    constexpr int D = decltype(dims_tag)::value;
    hipLaunchKernelGGL((encode3_boxes<S, HI, D>), grid, dim3(256), lds, stream, b, g, cp, a);
  });
}

}  // namespace zfp_amd
