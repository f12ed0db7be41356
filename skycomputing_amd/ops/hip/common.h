// Common helpers for skycomputing_amd gfx950 (CDNA4) kernels.
//
// Conventions (per /opt/skills/guides/cdna_hip_programming.md):
//   * wave = 64 lanes, hard-coded;
//   * 256-thread blocks (multiple of 64);
//   * bf16 I/O is vectorized as ushort4/ushort8 reinterprets (scalar bf16
//     loads are ~2-2.5x slower, guide G13);
//   * fp32 accumulation everywhere.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <type_traits>

#define WAVE 64
#define DEV __device__ __forceinline__

typedef unsigned short ushort_t;
typedef __attribute__((ext_vector_type(2))) unsigned short ushort2_t;
typedef __attribute__((ext_vector_type(4))) unsigned short ushort4_t;
typedef __attribute__((ext_vector_type(8))) unsigned short ushort8_t;
typedef __attribute__((ext_vector_type(4))) float float4_t;

DEV float bf16_to_f32(ushort_t u) {
  union { unsigned int i; float f; } v;
  v.i = ((unsigned int)u) << 16;
  return v.f;
}

// fp32 -> bf16, round-to-nearest-even, by the hardware convert
// (v_cvt_pk_bf16_f32). For every non-NaN input the bits are those of the
// integer formula ((i + 0x7fff + ((i >> 16) & 1)) >> 16) these kernels used
// before; a NaN stays a NaN, where the formula carried some payloads over
// into +-0 or +-Inf (tests/test_bf16_round_gpu.py walks all 2^32 inputs).
typedef __attribute__((ext_vector_type(2))) float float2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) unsigned int uint2_t;
typedef __attribute__((ext_vector_type(4))) unsigned int uint4_t;

DEV ushort_t f32_to_bf16(float f) {
  return __builtin_bit_cast(ushort_t, (__bf16)f);
}

// Two neighbouring values in one instruction: lo in bits 0..15, hi in
// bits 16..31, i.e. the little-endian image of {bf16(lo), bf16(hi)}.
DEV unsigned int f32x2_to_bf16x2(float lo, float hi) {
  const float2_t v = {lo, hi};
  return __builtin_bit_cast(unsigned int,
                            __builtin_convertvector(v, bf16x2_t));
}

// Four values as a ushort4 (the 8-byte P/dS packs of the attention kernels)
DEV ushort4_t f32x4_to_bf16x4(float a, float b, float c, float d) {
  const uint2_t v = {f32x2_to_bf16x2(a, b), f32x2_to_bf16x2(c, d)};
  return __builtin_bit_cast(ushort4_t, v);
}

// dtype tags matching hiplib._DT
enum { DT_F32 = 0, DT_BF16 = 1 };

// 8-element vector I/O (16 B/lane for bf16 — the coalescing sweet spot,
// guide G13; fp32 goes through two float4). Index i8 is in units of 8
// elements; pointers must be 16-byte aligned at those offsets.
template <int DT> struct Vec8;
template <> struct Vec8<DT_BF16> {
  static DEV void load(const void* p, int64_t i8, float f[8]) {
    ushort8_t v = ((const ushort8_t*)p)[i8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = bf16_to_f32(v[j]);
  }
  static DEV void store(void* p, int64_t i8, const float f[8]) {
    uint4_t v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = f32x2_to_bf16x2(f[2 * j], f[2 * j + 1]);
    ((uint4_t*)p)[i8] = v;
  }
};
template <> struct Vec8<DT_F32> {
  static DEV void load(const void* p, int64_t i8, float f[8]) {
    float4_t a = ((const float4_t*)p)[i8 * 2];
    float4_t b = ((const float4_t*)p)[i8 * 2 + 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[4 + j] = b[j]; }
  }
  static DEV void store(void* p, int64_t i8, const float f[8]) {
    float4_t a, b;
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[j] = f[j]; b[j] = f[4 + j]; }
    ((float4_t*)p)[i8 * 2] = a;
    ((float4_t*)p)[i8 * 2 + 1] = b;
  }
};

// generic element load/store through a dtype tag (scalar path)
template <int DT> DEV float load_elem(const void* p, int64_t i);
template <> DEV float load_elem<DT_F32>(const void* p, int64_t i) {
  return ((const float*)p)[i];
}
template <> DEV float load_elem<DT_BF16>(const void* p, int64_t i) {
  return bf16_to_f32(((const ushort_t*)p)[i]);
}
template <int DT> DEV void store_elem(void* p, int64_t i, float v);
template <> DEV void store_elem<DT_F32>(void* p, int64_t i, float v) {
  ((float*)p)[i] = v;
}
template <> DEV void store_elem<DT_BF16>(void* p, int64_t i, float v) {
  ((ushort_t*)p)[i] = f32_to_bf16(v);
}

// wave-wide reductions (64 lanes)
DEV float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
DEV float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// block-wide reductions through LDS (BLOCK threads = BLOCK/64 waves)
template <int BLOCK>
DEV float block_sum(float v, float* lds /* >= BLOCK/64 floats */) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  v = wave_sum(v);
  if (lane == 0) lds[wid] = v;
  __syncthreads();
  float r = 0.f;
  if (wid == 0) {
    r = (lane < BLOCK / WAVE) ? lds[lane] : 0.f;
    r = wave_sum(r);
    if (lane == 0) lds[0] = r;
  }
  __syncthreads();
  r = lds[0];
  __syncthreads();
  return r;
}

// counter-based RNG: splitmix64 -> uniform [0,1)
DEV uint64_t rng_hash(uint64_t seed, uint64_t q) {
  uint64_t z = seed + q * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// per-launch seed: the op's salt mixed with the device step counter
// (null state = counter 0), so masks vary under hipGraph replay
DEV uint64_t rng_seed(uint64_t salt, const unsigned long long* state) {
  return salt + (state ? *state : 0ull) * 0xD1B54A32D192ED03ull;
}

DEV float rng_uniform(uint64_t seed, uint64_t idx) {
  return (float)(rng_hash(seed, idx) >> 40) * 0x1.0p-24f;
}

// dropout keep decision: one splitmix hash feeds FOUR consecutive indices
// (16-bit thresholds) — 4x fewer hashes when a lane owns consecutive
// elements. keep16 = keep * 65536 (keep == 1 -> always true).
// rng_keep16 (one element) and RNG_DROP8 (a lane's 8) are the two spellings
// of the LINEAR index scheme: element e keeps iff slice e & 3 of
// rng_hash(seed, e >> 2) is below keep16.
DEV bool rng_keep16(uint64_t seed, uint64_t idx, unsigned keep16) {
  uint64_t z = rng_hash(seed, idx >> 2);
  return (unsigned)((z >> (16 * (idx & 3))) & 0xFFFFu) < keep16;
}

// The same decisions for the 8 consecutive elements 8*i8 .. 8*i8+7 (exactly
// two hash quads): float v[8] becomes v[j] * inv_keep where kept and 0 where
// dropped; bit j of the unsigned lvalue `bits` is element j's keep decision.
//
// A statement macro, not a function, on purpose. These kernels are compiled
// with fp contraction on, so which multiplies become FMAs is settled only
// after the SLP vectoriser has paired the lanes' 8 values, and that pairing
// changes when this loop reaches the kernel already unrolled, as it does
// through any inlined function (by pointer, by reference or by value):
// 49 of layernorm.hip's 112 kernels then compile differently and their
// outputs move by an ulp (profiles/r06_notes.md). Expanded in place, the
// kernels' results do not depend on where this text lives.
#define RNG_DROP8(seed, i8, keep16, inv_keep, v, bits)                        \
  do {                                                                        \
    const uint64_t z0_ = rng_hash(seed, (uint64_t)(i8) * 2);                  \
    const uint64_t z1_ = rng_hash(seed, (uint64_t)(i8) * 2 + 1);              \
    bits = 0;                                                                 \
    _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) {                        \
      const uint64_t zz_ = j_ < 4 ? z0_ : z1_;                                \
      const bool kb_ =                                                        \
          (unsigned)((zz_ >> (16 * (j_ & 3))) & 0xFFFFu) < (keep16);          \
      bits |= (unsigned)kb_ << j_;                                            \
      (v)[j_] = kb_ ? (v)[j_] * (inv_keep) : 0.f;                             \
    }                                                                         \
  } while (0)

DEV unsigned keep_to_16(float keep) {
  return keep >= 1.f ? 0x20000u : (unsigned)(keep * 65536.f + 0.5f);
}

// erf-formula GELU and its derivative (fp32)
// Branch-free erf (Abramowitz & Stegun 7.1.26, |err| <= 1.5e-7 absolute —
// far below bf16 resolution): ~12 VALU ops vs OCML erff's ~30 with range
// branches. Feeds the exact (erf) GELU, not the tanh approximation.
//
// The reciprocal is one v_rcp_f32 (1 ulp) where an IEEE divide is about 11
// instructions; gelu_grad_f evaluates exp(-x^2/2) once and hands it to the
// erf as well as the pdf ((x/sqrt 2)^2 and x^2/2 differ by the rounding of
// k only). -DSKY_GELU_IEEE_MATH restores the divide and the two
// exponentials, i.e. the earlier bits: it exists to check the rest of a
// change for identity against an older build, not for users.

// erf(x) given e = exp(-x*x)
DEV float erf_fast_e(float x, float e) {
  const float ax = fabsf(x);
#ifdef SKY_GELU_IEEE_MATH
  const float t = 1.f / fmaf(0.3275911f, ax, 1.f);
#else
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.f));
#endif
  const float p = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f),
                                           1.421413741f), -0.284496736f),
                           0.254829592f);
  const float r = 1.f - p * e;
  return copysignf(r, x);
}
DEV float erf_fast(float x) {
  const float ax = fabsf(x);
  return erf_fast_e(x, __expf(-ax * ax));
}
DEV float gelu_f(float x) { return 0.5f * x * (1.f + erf_fast(x * 0.70710678118654752f)); }
DEV float gelu_grad_f(float x) {
  const float k = 0.70710678118654752f;       // 1/sqrt(2)
  const float c = 0.3989422804014327f;        // 1/sqrt(2*pi)
#ifdef SKY_GELU_IEEE_MATH
  float cdf = 0.5f * (1.f + erf_fast(x * k));
  float pdf = c * __expf(-0.5f * x * x);
#else
  const float e = __expf(-0.5f * x * x);
  float cdf = 0.5f * (1.f + erf_fast_e(x * k, e));
  float pdf = c * e;
#endif
  return cdf + x * pdf;
}

// Slab reduction shared by the two-stage column sums (defined in
// elementwise.hip): out[c] = sum over the nslabs rows of the fp32 scratch
// [nslabs][cols], written as dtout (a DT_* tag). One launch.
void sky_launch_colsum_final(hipStream_t s, const float* scratch, void* out,
                             int64_t cols, int64_t nslabs, int dtout);

// A slab reduction whose producer has run but whose final has not: scratch
// holds nslabs slabs of [nv][cols] fp32, and out[v][c] = sum over the slabs
// of scratch[(slab*nv + v)*cols + c], written as dtout (a DT_* tag). The
// *_parts entry points fill one of these instead of launching their final
// (nv = 0: nothing pending, the producer finished its own outputs);
// sky_colsum_finish runs up to SKY_FINISH_MAX_JOBS of them in one launch.
// Mirrored by ops/hiplib.py: FinishJob.
struct SkyFinishJob {
  uint64_t scratch;
  uint64_t out[3];
  int64_t nslabs;
  int64_t cols;
  int32_t nv;
  int32_t dtout;
};
constexpr int SKY_FINISH_MAX_JOBS = 4;

static inline void sky_finish_job_set(SkyFinishJob* job, uint64_t scratch,
                                      uint64_t o0, uint64_t o1, uint64_t o2,
                                      int64_t nslabs, int64_t cols, int nv,
                                      int dtout) {
  *job = SkyFinishJob{scratch, {o0, o1, o2}, nslabs, cols, nv, dtout};
}

// Most slabs any two-stage column reduction writes: callers size the fp32
// scratch for MAX_SLABS slabs (ops/functions.py: _CS_SLABS).
constexpr int MAX_SLABS = 1024;

// Runtime (dt, has_res, drop, ch) -> compile-time tags: calls
// f(DT, HAS_RES, DROP, CH) with std::integral_constant arguments, usable
// directly as template arguments. ch (chunks of 512 elements per row) picks
// CH = 2, 4 or 8; a ch above MAXCH launches nothing (the caller has checked
// the width). Callers without a dropout or chunk axis pass false / 0 and
// ignore the tag.
template <int MAXCH = 8, class F>
static inline void dispatch_tags(int dt, bool has_res, bool drop, int ch,
                                 F&& f) {
  using std::integral_constant;
  auto by_ch = [&](auto DT, auto HR, auto DR) {
    if (ch <= 2) f(DT, HR, DR, integral_constant<int, 2>{});
    else if (ch <= 4) f(DT, HR, DR, integral_constant<int, 4>{});
    else if constexpr (MAXCH >= 8) f(DT, HR, DR, integral_constant<int, 8>{});
  };
  auto by_flags = [&](auto DT) {
    if (has_res) drop ? by_ch(DT, std::true_type{}, std::true_type{})
                      : by_ch(DT, std::true_type{}, std::false_type{});
    else drop ? by_ch(DT, std::false_type{}, std::true_type{})
              : by_ch(DT, std::false_type{}, std::false_type{});
  };
  if (dt == DT_F32) by_flags(integral_constant<int, DT_F32>{});
  else by_flags(integral_constant<int, DT_BF16>{});
}

#define LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

#define SKY_EXPORT extern "C" __attribute__((visibility("default")))
