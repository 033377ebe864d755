// k_fp8.h -- fp32 -> OCP fp8 (e4m3fn / e5m2) bits, the way torch's CPU cast rounds.
//
// No HIP headers: the same code compiles for gfx950 (k_decode.h stores decoded values into fp8 destinations with it) and
// for the host, where tests/test_fp8_host.py holds it against torch's `.to(torch.float8_*)` with a plain C++ compiler.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#ifndef LMC_DTYPE_FP8_E4M3
#define LMC_DTYPE_FP8_E4M3 2
#define LMC_DTYPE_FP8_E5M2 3
#endif

// c10's fp8e4m3fn_from_fp32_value / fp8e5m2_from_fp32_value, bit for bit: round to nearest even, subnormals through
// one fp32 add (whose own RNE places the bits), e4m3fn overflow (|x| >= 480, or a rounding up into 0x7f) -> NaN, e5m2
// overflow (|x| >= 61440 after rounding) -> inf.  One difference: every NaN comes out as the positive 0x7f (torch keeps
// the sign bit of the input).  Integer arithmetic and one add, not v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32: the result has
// to be torch's, whatever the instruction does at the edges.
template <int DT>
__host__ __device__ inline uint32_t lmc_f32_to_fp8(float f) {
  uint32_t fb = __builtin_bit_cast(uint32_t, f);
  const uint32_t sign = fb & 0x80000000u;
  fb ^= sign;
  uint32_t r;
  if constexpr (DT == LMC_DTYPE_FP8_E4M3) {
    if (fb >= 0x43f00000u) return 0x7fu;  // |x| >= 480, inf, NaN
    if (fb < (121u << 23)) {              // below 2^-6: the subnormal range
      const uint32_t dm = 141u << 23;
      r = __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, fb) + __builtin_bit_cast(float, dm)) - dm;
    } else {
      r = (fb + ((uint32_t)(7 - 127) << 23) + 0x7ffffu + ((fb >> 20) & 1u)) >> 20;
    }
    r &= 0xffu;
    if (r == 0x7fu) return 0x7fu;  // rounded up into the NaN code
  } else {
    if (fb > 0x7f800000u) return 0x7fu;                   // NaN
    if (fb >= (143u << 23)) return 0x7cu | (sign >> 24);  // |x| >= 65536, inf
    if (fb < (113u << 23)) {                              // below 2^-14
      const uint32_t dm = 134u << 23;
      r = __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, fb) + __builtin_bit_cast(float, dm)) - dm;
    } else {
      r = (fb + ((uint32_t)(15 - 127) << 23) + 0xfffffu + ((fb >> 21) & 1u)) >> 21;
    }
    r &= 0xffu;
  }
  return r | (sign >> 24);
}
