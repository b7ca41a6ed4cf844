// wave.hpp — device helpers shared by the kernel files: the LDS-only workgroup barrier, wave
// and workgroup sums, 64-bit lane moves, fp64 reciprocal refinements and the buffer
// descriptor. One copy of each; every body is the one the kernels were tuned with.
#pragma once

#include <hip/hip_runtime.h>

namespace specenh {

// Workgroup barrier that orders LDS only: waits for this wave's LDS ops (lgkmcnt) and
// meets the other waves, but leaves global loads (the register prefetch) and global
// stores in flight. __syncthreads() would add s_waitcnt vmcnt(0) and serialise both.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---------------------------------------------------------------- lane moves
// DPP move (row_mask = bank_mask = 0xF). BOUND is bound_ctrl: a lane whose source is
// invalid reads 0 when set, keeps the `old` operand (also 0) when clear; the encodings differ.
template <int CTRL, bool BOUND>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, BOUND));
}
template <int CTRL, bool BOUND>
__device__ __forceinline__ double dpp(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, BOUND);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, BOUND);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// lane l's v (wave-uniform l)
__device__ __forceinline__ double readlane64(double v, int l) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, l);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// ---------------------------------------------------------------- sums
// Sum over the 64 lanes of a wave, result in every lane. Two orders of addition, not
// interchangeable bit for bit: the __shfl_xor butterfly, and DPP inside rows of 16 (quad
// swaps, half-row and row mirrors) followed by the four row sums (every lane active; no LDS
// traffic).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double wave_sum_dpp(double v) {
  v += dpp<0xB1, false>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp<0x4E, false>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp<0x141, false>(v);  // row_half_mirror
  v += dpp<0x140, false>(v);  // row_mirror
  return (readlane64(v, 0) + readlane64(v, 16)) + (readlane64(v, 32) + readlane64(v, 48));
}
// Sum over a workgroup of 256 threads, result in every thread; red: 4 doubles of LDS,
// reusable call after call.
__device__ __forceinline__ double block_sum256(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();  // red is reused call after call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------- fp64 1/x, 1/sqrt(x)
// v_rcp_f64 / v_rsq_f64 plus Newton steps instead of the IEEE division and sqrt sequences.
// Two steps give full fp64 precision for finite x != 0 / x > 0; one step of rsq serves
// factors that only need to be consistent with each other, not correctly rounded. The one-
// and two-step forms of rsq write the step differently and are kept as they were.
__device__ __forceinline__ double rcp64_2(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(r, fma(-x, r, 1.0), r);
  return fma(r, fma(-x, r, 1.0), r);
}
template <int STEPS>
__device__ __forceinline__ double rsq64(double x) {
  static_assert(STEPS == 1 || STEPS == 2, "one or two Newton steps");
  double r = __builtin_amdgcn_rsq(x);
  if constexpr (STEPS == 1) {
    return r * fma(-0.5 * x * r, r, 1.5);
  } else {
    r = fma(r * fma(-0.5 * x, r * r, 0.5), 1.0, r);  // r (1 + (1 - x r^2) / 2)
    return fma(r * fma(-0.5 * x, r * r, 0.5), 1.0, r);
  }
}

// Buffer descriptor over [base, base + bytes) (wave-uniform base, 32-bit offsets): a load
// or store is then one VGPR offset + a scalar offset + an immediate, not a 64-bit address
// pair, and an offset past `bytes` reads 0 / is not stored.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* base, long long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0,
                                           (int)(bytes < 0x7fffffffll ? bytes : 0x7fffffffll),
                                           0x00020000);
}

}  // namespace specenh
