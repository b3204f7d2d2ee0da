// Which instantiations of the region kernels exist: the one selection ladder
// of the region decode, batched region decode, region encode and batched region
// encode launch units (zfp_region.hip, zfp_boxes.hip, zfp_region_enc.hip,
// zfp_boxes_enc.hip).  It knows nothing about
// the kernels: each unit passes a callable that launches its own.
#pragma once

#include <cstdint>
#include <type_traits>

namespace zfp_amd {

// f(tag, HI, D): tag a null S* (S the scalar type of `type`: 1 int32, 2 int64,
// 3 float, 4 double), HI a std::bool_constant (planes 32..63 only: double 3D),
// D a std::integral_constant<int> (the dimensionality).  1D and 2D of every
// scalar type and 3D of every type without HI, double 3D also with it.
template <typename F>
void by_region_kernel(int type, int dims, bool hi, F&& f)
{
  auto by_dims = [&](auto tag) {
    using S = std::remove_pointer_t<decltype(tag)>;
    if (dims == 1)
      return f(tag, std::false_type{}, std::integral_constant<int, 1>{});
    if (dims == 2)
      return f(tag, std::false_type{}, std::integral_constant<int, 2>{});
    if constexpr (std::is_same<S, double>::value) {
      if (hi)
        return f(tag, std::true_type{}, std::integral_constant<int, 3>{});
    }
    f(tag, std::false_type{}, std::integral_constant<int, 3>{});
  };
  switch (type) {
    case 1: return by_dims((int32_t*)nullptr);
    case 2: return by_dims((int64_t*)nullptr);
    case 3: return by_dims((float*)nullptr);
    default: return by_dims((double*)nullptr);
  }
}

}  // namespace zfp_amd
