// arith_harness.hip -- test-only kernels around the device helpers whose results rest on a hardware approximation or a
// proved shortcut (tests/test_gpu_device_arith.py).  Every kernel is "load the inputs, call the product's function,
// store what it returned": no formula of the product is written down here, so a change to a helper, to the flags the
// library is built with (tests/arith_harness.py takes native.HIPCC_FLAGS as they are) or to the compiler's lowering
// shows in the numbers the tests compare.
//
// One extern "C" entry per kernel: device pointers, a case count, a stream; returns the launch's hipError_t.
// Element kernels: one thread per case (pair kernels: per two cases), threads past the count return at once.
// Wave kernels (the CDF columns, the bit transpose): one 64-lane workgroup per case, every lane in use.
#include "../../lmcache_amd/csrc/lmc_device.h"
#include "../../lmcache_amd/csrc/k_quantize.h"
#include "../../lmcache_amd/csrc/k_bits.h"
#include "../../lmcache_amd/csrc/k_copy_split.h"

#define AH_BLOCK 256
#define AH_GRID(n) (unsigned)(((n) + AH_BLOCK - 1) / AH_BLOCK)
#define AH_INDEX(n)                                                      \
  const long long i = (long long)blockIdx.x * AH_BLOCK + threadIdx.x;    \
  if (i >= (n)) return
#define AH_LAUNCH(kernel, grid, block, ...)                              \
  do {                                                                   \
    if (n <= 0) return (int)hipSuccess;                                  \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
    return (int)hipGetLastError();                                       \
  } while (0)

// ---- the row factor ---------------------------------------------------------------------------------------------------
// case i: a row max as its 16-bit pattern, MAX as an integer.  in_range: the range test; short_bits: the four-instruction
// division; div_bits: the division as the quantisers write it when the range test fails.
__global__ void ahk_row_factor(const u32* max_bits, const u32* max_int, int dtype, u32* in_range, u32* short_bits, u32* div_bits,
                               long long n) {
  AH_INDEX(n);
  const float maxf = (float)max_int[i];
  const float sf = h2f_rt(max_bits[i], dtype);
  in_range[i] = row_div_in_range(max_bits[i], dtype) ? 1u : 0u;
  short_bits[i] = __float_as_uint(row_div_short(maxf, sf));
  div_bits[i] = __float_as_uint(maxf / sf);
}
extern "C" int ah_row_factor(const u32* max_bits, const u32* max_int, int dtype, u32* in_range, u32* short_bits, u32* div_bits,
                             long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_row_factor, AH_GRID(n), AH_BLOCK, max_bits, max_int, dtype, in_range, short_bits, div_bits, n);
}

// ---- the quantise step ------------------------------------------------------------------------------------------------
// One MAX per launch, x as fp32, the factor per row.  ah_quant_pair: a thread takes cases 2i and 2i + 1 (quant_z2 is a
// packed pair; n is even); cvt[p * n + case] = v_cvt_pk_u8_f32 of quant_z2's value into byte p of a dword that held
// 0xa5a5a5a5.  ah_quant_single: the one-at-a-time forms as they return.  (Two kernels, so that the packed multiply and
// add are compiled for their own sake as they are in the quantisers' regular path.)
__global__ void ahk_quant_pair(const float* x, const u32* row, const float* row_factor, float maxf, u32* cvt, long long n) {
  const long long i = ((long long)blockIdx.x * AH_BLOCK + threadIdx.x) * 2;
  if (i + 1 >= n) return;
  const f32x2_t f2 = {row_factor[row[i]], row_factor[row[i + 1]]}, maxf2 = {maxf, maxf};
  const f32x2_t z = quant_z2(x[i], x[i + 1], f2, maxf2);
  cvt[0 * n + i] = __builtin_amdgcn_cvt_pk_u8_f32(z.x, 0, 0xa5a5a5a5u);
  cvt[1 * n + i] = __builtin_amdgcn_cvt_pk_u8_f32(z.x, 1, 0xa5a5a5a5u);
  cvt[2 * n + i] = __builtin_amdgcn_cvt_pk_u8_f32(z.x, 2, 0xa5a5a5a5u);
  cvt[3 * n + i] = __builtin_amdgcn_cvt_pk_u8_f32(z.x, 3, 0xa5a5a5a5u);
  cvt[0 * n + i + 1] = __builtin_amdgcn_cvt_pk_u8_f32(z.y, 0, 0xa5a5a5a5u);
  cvt[1 * n + i + 1] = __builtin_amdgcn_cvt_pk_u8_f32(z.y, 1, 0xa5a5a5a5u);
  cvt[2 * n + i + 1] = __builtin_amdgcn_cvt_pk_u8_f32(z.y, 2, 0xa5a5a5a5u);
  cvt[3 * n + i + 1] = __builtin_amdgcn_cvt_pk_u8_f32(z.y, 3, 0xa5a5a5a5u);
}
extern "C" int ah_quant_pair(const float* x, const u32* row, const float* row_factor, float maxf, u32* cvt, long long n,
                             hipStream_t stream) {
  if (n & 1) return (int)hipErrorInvalidValue;
  AH_LAUNCH(ahk_quant_pair, AH_GRID(n / 2), AH_BLOCK, x, row, row_factor, maxf, cvt, n);
}
__global__ void ahk_quant_single(const float* x, const u32* row, const float* row_factor, float maxf, u32* fast, u32* special,
                                 long long n) {
  AH_INDEX(n);
  const float f = row_factor[row[i]];
  fast[i] = quant_fast(x[i], f, maxf);
  special[i] = quant_special(x[i], f, maxf);
}
extern "C" int ah_quant_single(const float* x, const u32* row, const float* row_factor, float maxf, u32* fast, u32* special,
                               long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_quant_single, AH_GRID(n), AH_BLOCK, x, row, row_factor, maxf, fast, special, n);
}
// quant_special alone (rows with a zero, tiny, inf or NaN max): its value as it returns it
__global__ void ahk_quant_special(const float* x, const u32* row, const float* row_factor, const float* row_maxf, u32* special,
                                  long long n) {
  AH_INDEX(n);
  special[i] = quant_special(x[i], row_factor[row[i]], row_maxf[row[i]]);
}
extern "C" int ah_quant_special(const float* x, const u32* row, const float* row_factor, const float* row_maxf, u32* special,
                                long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_quant_special, AH_GRID(n), AH_BLOCK, x, row, row_factor, row_maxf, special, n);
}

// ---- the coder's division ---------------------------------------------------------------------------------------------
__global__ void ahk_rans(const u32* x, const u32* f, const u32* st, u32* q, u32* r, u32* put, long long n) {
  AH_INDEX(n);
  u32 qq, rr;
  divmod_est(x[i], f[i], qq, rr);
  q[i] = qq;
  r[i] = rr;
  put[i] = rans_put(x[i], f[i], 65536u - f[i], st[i]);
}
extern "C" int ah_rans(const u32* x, const u32* f, const u32* st, u32* q, u32* r, u32* put, long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_rans, AH_GRID(n), AH_BLOCK, x, f, st, q, r, put, n);
}

// ---- the CDF arithmetic -----------------------------------------------------------------------------------------------
__global__ void ahk_rne_div(const u32* v, const u32* T, const u32* magic, u32* out, long long n) {
  AH_INDEX(n);
  out[i] = rne_div_u32(v[i], T[i], magic[i]);
}
extern "C" int ah_rne_div(const u32* v, const u32* T, const u32* magic, u32* out, long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_rne_div, AH_GRID(n), AH_BLOCK, v, T, magic, out, n);
}
// one wave per case: hreg[case][k][lane] in, the table as the helper left it in LDS out ([33][64] u16 / 1024 dwords)
__global__ void __launch_bounds__(64) ahk_cdf_column(const u32* hreg_in, const u32* T, const u32* nsym, u16* out) {
  __shared__ u16 tab[33 * 64];
  const int lane = threadIdx.x;
  const long long c = blockIdx.x;
  u32 hreg[16];
#pragma unroll
  for (int k = 0; k < 16; k++) hreg[k] = hreg_in[(c * 16 + k) * 64 + lane];
  cdf_column_to_lds(hreg, T[c], nsym[c], tab, lane);
  __syncthreads();
  for (int e = lane; e < 33 * 64; e += 64) out[c * (33 * 64) + e] = tab[e];
}
extern "C" int ah_cdf_column(const u32* hreg, const u32* T, const u32* nsym, u16* out, long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_cdf_column, (unsigned)n, 64, hreg, T, nsym, out);
}
__global__ void __launch_bounds__(64) ahk_cdf_column_wide(const u32* hreg_in, const u32* T, const u32* nsym, u32* out) {
  __shared__ u32 tab32[4 * 256];
  const int lane = threadIdx.x;
  const long long c = blockIdx.x;
  u32 hreg[16];
#pragma unroll
  for (int k = 0; k < 16; k++) hreg[k] = hreg_in[(c * 16 + k) * 64 + lane];
  cdf_column_to_lds_wide(hreg, T[c], nsym[c], tab32, lane);
  __syncthreads();
  for (int e = lane; e < 4 * 256; e += 64) out[c * (4 * 256) + e] = tab32[e];
}
extern "C" int ah_cdf_column_wide(const u32* hreg, const u32* T, const u32* nsym, u32* out, long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_cdf_column_wide, (unsigned)n, 64, hreg, T, nsym, out);
}

// ---- small exact pieces -----------------------------------------------------------------------------------------------
__global__ void ahk_divmod_small(const u32* e, const u32* R, const float* rcpR, u32* q, u32* r, long long n) {
  AH_INDEX(n);
  u32 qq, rr;
  divmod_small(e[i], R[i], rcpR[i], qq, rr);
  q[i] = qq;
  r[i] = rr;
}
extern "C" int ah_divmod_small(const u32* e, const u32* R, const float* rcpR, u32* q, u32* r, long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_divmod_small, AH_GRID(n), AH_BLOCK, e, R, rcpR, q, r, n);
}
__global__ void ahk_split_divmod(const u32* e, const u32* R, const float* rcpR, u32* q, u32* r, long long n) {
  AH_INDEX(n);
  u32 qq, rr;
  split_divmod(e[i], R[i], rcpR[i], qq, rr);
  q[i] = qq;
  r[i] = rr;
}
extern "C" int ah_split_divmod(const u32* e, const u32* R, const float* rcpR, u32* q, u32* r, long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_split_divmod, AH_GRID(n), AH_BLOCK, e, R, rcpR, q, r, n);
}
// the counts model's scaling as the kernels write it: the multiply-high of x << 8 with the device magic of T
__global__ void ahk_counts_scale(const u32* x, const u32* T, u32* scaled, u32* magic, long long n) {
  AH_INDEX(n);
  const u32 m = lmc_counts_scale_magic_dev(T[i]);
  magic[i] = m;
  scaled[i] = __umulhi(x[i] << 8, m);
}
extern "C" int ah_counts_scale(const u32* x, const u32* T, u32* scaled, u32* magic, long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_counts_scale, AH_GRID(n), AH_BLOCK, x, T, scaled, magic, n);
}
__global__ void ahk_f2bf16(const u32* fbits, u32* out, long long n) {
  AH_INDEX(n);
  out[i] = f2bf16(__uint_as_float(fbits[i]));
}
extern "C" int ah_f2bf16(const u32* fbits, u32* out, long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_f2bf16, AH_GRID(n), AH_BLOCK, fbits, out, n);
}
__global__ void ahk_f2fp16(const u32* fbits, u32* out, long long n) {
  AH_INDEX(n);
  out[i] = f2fp16(__uint_as_float(fbits[i]));
}
extern "C" int ah_f2fp16(const u32* fbits, u32* out, long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_f2fp16, AH_GRID(n), AH_BLOCK, fbits, out, n);
}
// the widening the quantisers read their elements with
__global__ void ahk_h2f(const u32* bits, int dtype, u32* out, long long n) {
  AH_INDEX(n);
  out[i] = __float_as_uint(h2f_rt(bits[i], dtype));
}
extern "C" int ah_h2f(const u32* bits, int dtype, u32* out, long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_h2f, AH_GRID(n), AH_BLOCK, bits, dtype, out, n);
}
// one wave per matrix: lane l loads row l, stores what it holds afterwards
__global__ void __launch_bounds__(64) ahk_transpose64(const u64* rows, u64* out) {
  const int lane = threadIdx.x;
  const long long c = blockIdx.x;
  const u64 v = rows[c * 64 + lane];
  u32 lo = (u32)v, hi = (u32)(v >> 32);
  transpose64(lo, hi, lane);
  out[c * 64 + lane] = ((u64)hi << 32) | (u64)lo;
}
extern "C" int ah_transpose64(const u64* rows, u64* out, long long n, hipStream_t stream) {
  AH_LAUNCH(ahk_transpose64, (unsigned)n, 64, rows, out);
}
