// bf16_slice.h — an fp32 number as the sum of three bf16-representable fp32 numbers (gemm.hip wgrad_tile, sliced body).
//
//   hi  = x with the low 16 bits cleared          (sign, exponent, top 7 fraction bits: truncation, never overflows)
//   mid = (x - hi) with the low 16 bits cleared    (x - hi is exact: at most 16 significant bits)
//   lo  = (x - hi) - mid                           (exact: at most 8 significant bits)
//
// hi + mid + lo == x exactly for every finite x, in any order of the two additions.  hi and mid have their low 16 bits clear by
// construction.  lo has them clear whenever x is a multiple of 2^-133 (the spacing of bf16 subnormals): every |x| >= 2^-110 and
// every coarser small value, FLT_MIN included.  Below that, lo can carry bits under 2^-133 which a bf16 cannot hold; slice_pack()
// drops them (truncation), an absolute error below 2^-133 per operand.
// Non-finite x: hi = x & 0xFFFF0000 (an infinity, or a NaN whose payload lies in the low 16 bits, gives an infinity), x - hi is
// inf - inf = NaN, so mid and lo are NaN: a product with such an operand is NaN where the exact fp32 product gives +-inf or NaN.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BLVM_HD __host__ __device__
#else
#define BLVM_HD
#endif

namespace blvm {

struct Slices3 {
  float hi, mid, lo;
};

BLVM_HD inline uint32_t slice_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
BLVM_HD inline float slice_trunc(float x) { return __builtin_bit_cast(float, slice_bits(x) & 0xFFFF0000u); }

BLVM_HD inline Slices3 slice3(float x) {
  Slices3 s;
  s.hi = slice_trunc(x);
  const float r = x - s.hi;
  s.mid = slice_trunc(r);
  s.lo = r - s.mid;
  return s;
}

// two slices as one register of two bf16: e0 in the low half (the element with the lower k), e1 in the high half
BLVM_HD inline uint32_t slice_pack(float e0, float e1) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(slice_bits(e1), slice_bits(e0), 0x07060302u);  // one v_perm_b32: bytes 3:2 of e1, bytes 3:2 of e0
#else
  return (slice_bits(e1) & 0xFFFF0000u) | (slice_bits(e0) >> 16);
#endif
}

}  // namespace blvm
