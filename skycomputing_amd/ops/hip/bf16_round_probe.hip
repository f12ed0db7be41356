// Exhaustive probe of the fp32 -> bf16 rounding in common.h: one launch walks
// all 2^32 float bit patterns and compares f32_to_bf16 (the scalar form) and
// both lanes of f32x2_to_bf16x2 (the packed form) with the integer
// round-to-nearest-even formula the kernels used before the hardware
// convert, which is kept here as the reference.
//
// counts[0]: non-NaN inputs for which any of the three results differs from
//            the formula's bits;
// counts[1]: NaN inputs for which any of the three results is not a NaN
//            (the formula itself turns some NaN payloads into +-0 / +-Inf;
//            the hardware keeps a NaN, the one permitted difference);
// counts[2]: inputs examined, so that two zeroes mean something: 2^32.
// tests/test_bf16_round_gpu.py requires 0, 0 and 2^32.

#include "common.h"

DEV ushort_t bf16_round_formula(unsigned int i) {
  const unsigned int lsb = (i >> 16) & 1u;
  i += 0x7fffu + lsb;
  return (ushort_t)(i >> 16);
}

DEV bool bf16_is_nan(ushort_t b) { return (b & 0x7fffu) > 0x7f80u; }

// 2^20 threads x 4096 patterns; thread t takes t, t + 2^20, ...
constexpr unsigned PROBE_BLOCKS = 4096;

__global__ __launch_bounds__(256) void bf16_round_probe_kernel(
    unsigned long long* __restrict__ counts) {
  const unsigned int t = blockIdx.x * 256u + threadIdx.x;
  unsigned int bad = 0, nan_lost = 0, seen = 0;
  for (unsigned int k = 0; k < 4096u; ++k) {
    const unsigned int i = t + (k << 20);
    const float f = __builtin_bit_cast(float, i);
    // the other lane's input: some unrelated value, so neither lane of the
    // packed convert can be folded into the scalar one
    const float g = __builtin_bit_cast(float, i * 2654435761u + 0x3f800001u);
    const ushort_t ref = bf16_round_formula(i);
    const ushort_t sc = f32_to_bf16(f);
    const ushort_t lo = (ushort_t)f32x2_to_bf16x2(f, g);
    const ushort_t hi = (ushort_t)(f32x2_to_bf16x2(g, f) >> 16);
    if ((i & 0x7fffffffu) > 0x7f800000u) {
      if (!bf16_is_nan(sc) || !bf16_is_nan(lo) || !bf16_is_nan(hi)) ++nan_lost;
    } else {
      if (sc != ref || lo != ref || hi != ref) ++bad;
    }
    ++seen;
  }
  // at most three atomics per wave
  for (int off = 32; off > 0; off >>= 1) {
    bad += __shfl_xor(bad, off, 64);
    nan_lost += __shfl_xor(nan_lost, off, 64);
    seen += __shfl_xor(seen, off, 64);
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    if (bad) atomicAdd(&counts[0], (unsigned long long)bad);
    if (nan_lost) atomicAdd(&counts[1], (unsigned long long)nan_lost);
    atomicAdd(&counts[2], (unsigned long long)seen);
  }
}

// counts: three uint64 on the device; zeroed here, then filled by the launch.
SKY_EXPORT int sky_probe_bf16_round(uint64_t stream, uint64_t counts) {
  if (counts == 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e =
      hipMemsetAsync((void*)counts, 0, 3 * sizeof(unsigned long long), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(bf16_round_probe_kernel, dim3(PROBE_BLOCKS), dim3(256), 0,
                     s, (unsigned long long*)counts);
  LAUNCH_CHECK();
  return 0;
}
