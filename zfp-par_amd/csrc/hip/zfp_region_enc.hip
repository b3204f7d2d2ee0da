// Region encode kernels (kernels_region_enc.h): every instantiation the host
// can select -- float and double 3D through decode_block3 / encode_block3
// (double also with planes 32..63 only), 1D/2D of every scalar type and 3D
// integers through the generic per-lane codec.  Fixed rate only: there is no
// reversible form.
#include "kernels_region_enc.h"

namespace zfp_amd {

namespace {

struct RegionEncLaunch {
  hipStream_t stream;
  dim3 grid;
  size_t lds;
  const void* src;
  const Geometry& g;
  const CodecParams& cp;
  const RegionGeom& rg;
  const RegionEncArgs& a;
};

template <typename S, bool HI, int D>
void region_enc_kernel(const RegionEncLaunch& l)
{
  hipLaunchKernelGGL((encode3_region<S, HI, D>), l.grid, dim3(256), l.lds, l.stream, (const S*)l.src, l.g, l.cp, l.rg,
                     l.a);
}

template <typename S>
void region_enc_by_dims(const RegionEncLaunch& l, int dims, bool hi)
{
  if (dims == 1)
    return region_enc_kernel<S, false, 1>(l);
  if (dims == 2)
    return region_enc_kernel<S, false, 2>(l);
  if constexpr (std::is_same<S, double>::value) {
    if (hi)
      return region_enc_kernel<S, true, 3>(l);
  }
  region_enc_kernel<S, false, 3>(l);
}

}  // namespace

void launch_encode_region(int type, int dims, bool hi, hipStream_t stream, dim3 grid, size_t lds, const void* src,
                          const Geometry& g, const CodecParams& cp, const RegionGeom& rg, const RegionEncArgs& a)
{
  const RegionEncLaunch l{stream, grid, lds, src, g, cp, rg, a};
  switch (type) {
    case 1: return region_enc_by_dims<int32_t>(l, dims, hi);
    case 2: return region_enc_by_dims<int64_t>(l, dims, hi);
    case 3: return region_enc_by_dims<float>(l, dims, hi);
    default: return region_enc_by_dims<double>(l, dims, hi);
  }
}

}  // namespace zfp_amd
