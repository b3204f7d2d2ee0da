// Batched region decode kernels (kernels_boxes.h): the instantiations of
// zfp_region.hip -- float and double 3D through decode_block3 (double also with
// planes 32..63 only), 1D/2D of every scalar type and 3D integers through
// decode_block_n.
#include "kernels_boxes.h"

namespace zfp_amd {

namespace {

struct BoxesLaunch {
  hipStream_t stream;
  dim3 grid;
  size_t lds;
  const BoxesArgs& b;
  const Geometry& g;
  const CodecParams& cp;
  const RegionArgs& a;
};

template <typename S, bool HI, int D>
void boxes_kernel(const BoxesLaunch& l, bool rev)
{
  if (rev)
    hipLaunchKernelGGL((decode3_boxes<S, true, HI, D>), l.grid, dim3(256), l.lds, l.stream, l.b, l.g, l.cp, l.a);
  else
    hipLaunchKernelGGL((decode3_boxes<S, false, HI, D>), l.grid, dim3(256), l.lds, l.stream, l.b, l.g, l.cp, l.a);
}

template <typename S>
void boxes_by_dims(const BoxesLaunch& l, int dims, bool rev, bool hi)
{
  if (dims == 1)
    return boxes_kernel<S, false, 1>(l, rev);
  if (dims == 2)
    return boxes_kernel<S, false, 2>(l, rev);
  if constexpr (std::is_same<S, double>::value) {
    if (hi)
      return boxes_kernel<S, true, 3>(l, rev);
  }
  boxes_kernel<S, false, 3>(l, rev);
}

}  // namespace

void launch_decode_boxes(int type, int dims, bool rev, bool hi, hipStream_t stream, dim3 grid, size_t lds,
                         const BoxesArgs& b, const Geometry& g, const CodecParams& cp, const RegionArgs& a)
{
  const BoxesLaunch l{stream, grid, lds, b, g, cp, a};
  switch (type) {
    case 1: return boxes_by_dims<int32_t>(l, dims, rev, hi);
    case 2: return boxes_by_dims<int64_t>(l, dims, rev, hi);
    case 3: return boxes_by_dims<float>(l, dims, rev, hi);
    default: return boxes_by_dims<double>(l, dims, rev, hi);
  }
}

}  // namespace zfp_amd
