// mma.hpp — device primitives shared by the 16-bit MFMA convolution kernels (conv_ae.hip,
// conv_c1_mfma.hip, conv_narrow.hip, conv_rows.hip, decoder_tail.hip, tail_rows_g.hip): the
// vector types, the 16x16x32 MFMA, the packed dot product, the conversions and the fp32 -> T
// pair packing. Everything is __device__ __forceinline__: a kernel's code is what its own
// body makes of them.
//
// Two floats are packed into one word of T pairs (round to nearest even, first argument in
// the low half) by THREE source forms that round alike but are not the same code to the
// compiler; a file keeps the form it was measured with:
//   pack2_cvt   __builtin_convertvector of a float pair           conv_rows.hip
//   pack2_vec   two scalar converts in a vector initialiser       conv_ae.hip, conv_c1_mfma.hip
//   pack2_bits  two scalar converts, a shift and an or            decoder_tail.hip,
//                                                                 tail_rows_g.hip, relu_pack
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "specenh.h"

namespace specenh {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// acc + A x B on v_mfma_f32_16x16x32_{f16,bf16}: a lane's 8 K-elements of A and of B as any
// 16-byte value (uint4, eight raw shorts, V8<T>, a typed 8-vector). By reference on purpose:
// taken by value, the register allocation of nearly every calling kernel comes out different.
template <typename T, typename V>
__device__ __forceinline__ f32x4 mfma16x16x32(const V& a, const V& b, f32x4 acc) {
  static_assert(sizeof(T) == 2 && sizeof(V) == 16, "eight 16-bit elements per lane");
  if constexpr (__is_same(T, _Float16))
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a),
                                                  __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

// c + a.lo*b.lo + a.hi*b.hi for two packed 16-bit values of T
template <typename T>
__device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c) {
  if constexpr (__is_same(T, _Float16)) {
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), c,
                                  false);
  } else {  // v_dot2c_f32_bf16 (gfx950)
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a),
                                           __builtin_bit_cast(bf16x2, b), c, false);
  }
}

// max(a, b) without the NaN-quieting canonicalisation fmaxf gets (operands are
// accumulators: finite unless the inputs hold NaN/Inf) as v_med3_f32(a, b, +inf): a
// builtin, not inline asm, so the compiler's hazard recognizer sees the read of an MFMA
// result and pads the XDL-write -> VALU-read wait states (inside an asm statement it
// does not)
__device__ __forceinline__ float vmax(float a, float b) {
  return __builtin_amdgcn_fmed3f(a, b, __builtin_inff());
}

// the layer's activation, chosen at run time (SPECENH_ACT_*)
__device__ __forceinline__ float act_f(float v, int act) {
  if (act == SPECENH_ACT_RELU) return fmaxf(v, 0.f);
  if (act == SPECENH_ACT_SIGMOID) return 1.f / (1.f + __expf(-v));
  return v;
}

__device__ __forceinline__ float to_f(float x) { return x; }
__device__ __forceinline__ float to_f(__bf16 x) { return (float)x; }
__device__ __forceinline__ float to_f(_Float16 x) { return (float)x; }
template <typename T>
__device__ __forceinline__ T from_f(float x);
template <>
__device__ __forceinline__ float from_f<float>(float x) { return x; }
template <>
__device__ __forceinline__ __bf16 from_f<__bf16>(float x) { return (__bf16)x; }
template <>
__device__ __forceinline__ _Float16 from_f<_Float16>(float x) { return (_Float16)x; }

// an element's raw bits in the low end of a word
__device__ __forceinline__ uint32_t bits(float x) { return __float_as_uint(x); }
__device__ __forceinline__ uint32_t bits(__bf16 x) {
  return (uint32_t)__builtin_bit_cast(unsigned short, x);
}
__device__ __forceinline__ uint32_t bits(_Float16 x) {
  return (uint32_t)__builtin_bit_cast(unsigned short, x);
}

// The three packing forms (file comment), each with the instructions gfx950 -O3 makes of a
// lone call. The first two agree there; they are still different IR (one vector convert
// against two scalar converts that the back end has to pair up again), so swapping them
// inside a kernel is a code change to be measured, not a rename.
//
// fp16: v_cvt_pk_f16_f32; bf16: v_cvt_pk_bf16_f32 (one instruction). Used by conv_rows.hip.
template <typename T>
__device__ __forceinline__ uint32_t pack2_cvt(float lo, float hi) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef T t2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{lo, hi}, t2));
}
// fp16: v_cvt_pk_f16_f32; bf16: v_cvt_pk_bf16_f32 (the two converts paired into one
// instruction). Used by conv_ae.hip and conv_c1_mfma.hip.
template <typename T>
__device__ __forceinline__ uint32_t pack2_vec(float lo, float hi) {
  if constexpr (__is_same(T, __bf16)) {
    return __builtin_bit_cast(uint32_t, bf16x2{(__bf16)lo, (__bf16)hi});
  } else {
    return __builtin_bit_cast(uint32_t, f16x2{(_Float16)lo, (_Float16)hi});
  }
}
// fp16: v_cvt_f16_f32, v_cvt_f16_f32 (SDWA, into the high half), v_or_b32; bf16: two
// v_cvt_pk_bf16_f32 (one value each), v_lshlrev_b32 16, v_or_b32 (SDWA). Used by
// decoder_tail.hip and tail_rows_g.hip, directly and through relu_pack.
template <typename T>
__device__ __forceinline__ uint32_t pack2_bits(float lo, float hi) {
  const T a = (T)lo, b = (T)hi;
  return (uint32_t)__builtin_bit_cast(unsigned short, a) |
         ((uint32_t)__builtin_bit_cast(unsigned short, b) << 16);
}

// bias + ReLU of four fp32 accumulators -> four T packed in 8 bytes (the decoder tails). The
// accumulators start at the bias (folded into the MFMA chain); ReLU commutes with the
// monotone rounding, so for fp16 it runs on the packed halves (v_pk_max_f16: 2 instead of
// 4 VALU).
template <typename T>
__device__ __forceinline__ uint2 relu_pack(const f32x4& v) {
  if constexpr (__is_same(T, _Float16)) {
    const f16x2 lo = f16x2{(_Float16)v[0], (_Float16)v[1]};
    const f16x2 hi = f16x2{(_Float16)v[2], (_Float16)v[3]};
    const f16x2 z = f16x2{(_Float16)0.f, (_Float16)0.f};
    return uint2{__builtin_bit_cast(uint32_t, __builtin_elementwise_max(lo, z)),
                 __builtin_bit_cast(uint32_t, __builtin_elementwise_max(hi, z))};
  } else {
    return uint2{pack2_bits<T>(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f)),
                 pack2_bits<T>(fmaxf(v[2], 0.f), fmaxf(v[3], 0.f))};
  }
}

}  // namespace specenh
