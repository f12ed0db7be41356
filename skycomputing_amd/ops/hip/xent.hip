// Softmax cross-entropy over wide rows (a vocabulary) for gfx950: the loss of
// masked-LM pretraining, fused so that the logits cross HBM once forward
// and once in each direction backward, and rows without a label not at all.
//
//   logits [N, ld]  bf16 or fp32, rows ld elements apart; columns 0..V-1
//                   are the classes, columns V..ld-1 are padding (a GEMM-
//                   friendly width) that is never read forward and gets
//                   gradient 0
//   labels [N]      int64. A row is VALID iff 0 <= label < V and
//                   label != ignore_index. Every other row — the ignore
//                   index and any out-of-range label alike — is ignored:
//                   loss 0, gradient 0, and its logits are never read. No
//                   label is ever used as an index before that test.
//
// One step is sky_xent_fwd, sky_xent_finish, [autograd,] sky_xent_bwd on one
// stream. The scalars that depend on the labels live in a device block of
// two fp32 words, so a step captured once in a hipGraph stays right when
// replayed on labels with another valid count:
//
//   word  name       written by
//   0     loss       sky_xent_finish: sum of row losses / valid count
//   1     inv_count  sky_xent_finish: 1 / valid count
//   count == 0 gives loss = 0 and inv_count = 0 (torch gives NaN there).
//
// Forward, one 256-thread block per row, ONLINE (max, sum): each thread
// folds its vectors into a running pair (m, s = sum exp(z - m)), rescaling s
// when m grows, and the pairs merge by the same formula across the wave and
// the block in a fixed order. The alternative, a register-resident row, is
// 120 fp32 registers per thread at V = 30522 and caps occupancy; the online
// form costs one extra exponential per 8 elements and keeps ~20 registers,
// which is what a streaming kernel wants (many waves, many loads in flight).
// Per row it leaves rowmax = m, logsum = log(s) and
//   rowloss = logsum - (z[label] - rowmax),
// the SHIFTED form: both terms are O(log V). (rowmax + logsum) - z[label]
// rounds rowmax + logsum to an ulp of |rowmax| first and loses the loss when
// the row has one large logit. The log and that last expression are taken in
// double by the row's one finishing thread (rounded to fp32 once).
//
// Backward: dlogits[r][j] = (exp((z - rowmax) - logsum) - [j == label])
//                           * gout * inv_count
// for valid rows and j < V, zero elsewhere; gout (the incoming gradient of
// the mean) and inv_count are read from device memory. Each element is read
// and then written by the same thread, so dlogits may be the logits buffer.
//
// Rows are not assumed to start 16-byte aligned or to have ld % 8 == 0 (at
// ld = 30522 in bf16 the row start walks through 0, 4, 8, 12 mod 16): every
// row has a scalar head up to its first 16-byte boundary, a Vec8 body and a
// scalar tail. exp and log are expf/logf, not the fast intrinsics: the
// accuracy rule of tests/xent_checks.py is then met with room. Measured
// (profiles/r10_notes.md): the backward runs at the memory rate, the
// forward at 3.16 TB/s, bound by expf; __expf there is open.

#include "common.h"
#include <float.h>

template <int DT> struct ElemSize { static constexpr int value = DT == DT_F32 ? 4 : 2; };

DEV bool xent_valid(int64_t label, int64_t V, int64_t ignore) {
  return label >= 0 && label < V && label != ignore;
}

// elements of a row starting at p that lie before its first 16-byte
// boundary, at most width
template <int DT> DEV int xent_head(const void* p, int64_t width) {
  const int h = (int)(((16 - ((uintptr_t)p & 15)) & 15) / ElemSize<DT>::value);
  return (int64_t)h < width ? h : (int)width;
}

// (m, s) <- the pair of the union of two sets. m starts at -FLT_MAX, not
// -inf, so that two empty pairs merge to an empty pair (exp(0) * 0) and
// not to NaN.
DEV void xent_merge(float& m, float& s, float mo, float so) {
  const float mn = fmaxf(m, mo);
  s = s * expf(m - mn) + so * expf(mo - mn);
  m = mn;
}

DEV void xent_fold1(float& m, float& s, float x) {
  const float mn = fmaxf(m, x);
  s = s * expf(m - mn) + expf(x - mn);
  m = mn;
}

DEV void xent_fold8(float& m, float& s, const float x[8]) {
  float g = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])),
                  fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
  const float mn = fmaxf(m, g);
  float e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = expf(x[j] - mn);
  s = s * expf(m - mn) +
      (((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7])));
  m = mn;
}

template <int DT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void xent_fwd_kernel(
    const void* __restrict__ logits, const int64_t* __restrict__ labels,
    float* __restrict__ rowmax, float* __restrict__ logsum,
    float* __restrict__ rowloss, int64_t V, int64_t ld, int64_t ignore) {
  __shared__ float lds_m[BLOCK / WAVE];
  __shared__ float lds_s[BLOCK / WAVE];
  const int64_t r = blockIdx.x;
  const int64_t label = labels[r];
  if (!xent_valid(label, V, ignore)) {  // the whole block leaves together
    if (threadIdx.x == 0) {
      rowmax[r] = 0.f;
      logsum[r] = 0.f;
      rowloss[r] = 0.f;
    }
    return;
  }
  const char* row = (const char*)logits + r * ld * ElemSize<DT>::value;
  const int head = xent_head<DT>(row, V);
  const void* body = row + head * ElemSize<DT>::value;
  const int64_t n8 = (V - head) / 8;
  const int64_t tail0 = head + n8 * 8;

  float m = -FLT_MAX, s = 0.f;
  // two vectors per trip, both loads issued before either is used; the
  // second index is clamped (a repeated load) so that no load sits behind
  // a branch
  for (int64_t i8 = threadIdx.x; i8 < n8; i8 += 2 * BLOCK) {
    const int64_t k8 = i8 + BLOCK;
    const bool two = k8 < n8;
    float a[8], b[8];
    Vec8<DT>::load(body, i8, a);
    Vec8<DT>::load(body, two ? k8 : i8, b);
    xent_fold8(m, s, a);
    if (two) xent_fold8(m, s, b);
  }
  if ((int)threadIdx.x < head) xent_fold1(m, s, load_elem<DT>(row, threadIdx.x));
  if (tail0 + threadIdx.x < V)
    xent_fold1(m, s, load_elem<DT>(row, tail0 + threadIdx.x));

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float mo = __shfl_xor(m, off, 64);
    const float so = __shfl_xor(s, off, 64);
    xent_merge(m, s, mo, so);
  }
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  if (lane == 0) {
    lds_m[wid] = m;
    lds_s[wid] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < BLOCK / WAVE; ++w) xent_merge(m, s, lds_m[w], lds_s[w]);
    // The row's three scalars meet in double, on this one thread: in fp32
    // z[label] - m and the subtraction from the log each round to an ulp
    // of the loss, which is a whole ulp where torch's fp32 loss can happen
    // to be exact. This way the loss is rounded once.
    const double lse = log((double)s);
    const double zl = (double)load_elem<DT>(row, label);
    rowmax[r] = m;
    logsum[r] = (float)lse;
    rowloss[r] = (float)(lse - (zl - (double)m));
  }
}

SKY_EXPORT int sky_xent_fwd(uint64_t stream, uint64_t logits, uint64_t labels,
                            uint64_t rowmax, uint64_t logsum, uint64_t rowloss,
                            int64_t N, int64_t V, int64_t ld, int64_t ignore,
                            int dt) {
  constexpr int BLOCK = 256;
  if (N < 0 || N > 0x7fffffffLL || V < 1 || V > ld) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)N);
  if (dt == DT_F32)
    hipLaunchKernelGGL((xent_fwd_kernel<DT_F32, BLOCK>), grid, dim3(BLOCK), 0, s,
                       (const void*)logits, (const int64_t*)labels,
                       (float*)rowmax, (float*)logsum, (float*)rowloss, V, ld,
                       ignore);
  else
    hipLaunchKernelGGL((xent_fwd_kernel<DT_BF16, BLOCK>), grid, dim3(BLOCK), 0, s,
                       (const void*)logits, (const int64_t*)labels,
                       (float*)rowmax, (float*)logsum, (float*)rowloss, V, ld,
                       ignore);
  LAUNCH_CHECK();
  return 0;
}

// One block adds the row losses and counts the valid rows in a fixed order
// (no atomics), like gradnorm_finish_kernel, and leaves the mean and
// 1/count in the device block.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void xent_finish_kernel(
    const float* __restrict__ rowloss, const int64_t* __restrict__ labels,
    int64_t N, int64_t V, int64_t ignore, float* __restrict__ block) {
  __shared__ float lds[BLOCK / WAVE];
  __shared__ int lds_n[BLOCK / WAVE];
  float acc = 0.f;
  int cnt = 0;
  for (int64_t i = threadIdx.x; i < N; i += BLOCK) {
    acc += rowloss[i];  // ignored rows hold 0
    cnt += xent_valid(labels[i], V, ignore) ? 1 : 0;
  }
  acc = block_sum<BLOCK>(acc, lds);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if ((threadIdx.x & (WAVE - 1)) == 0) lds_n[threadIdx.x / WAVE] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / WAVE; ++w) n += lds_n[w];
    block[0] = n > 0 ? acc / (float)n : 0.f;
    block[1] = n > 0 ? 1.f / (float)n : 0.f;
  }
}

SKY_EXPORT int sky_xent_finish(uint64_t stream, uint64_t rowloss,
                               uint64_t labels, uint64_t block, int64_t N,
                               int64_t V, int64_t ignore) {
  constexpr int BLOCK = 256;
  if (N < 0 || N > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((xent_finish_kernel<BLOCK>), dim3(1), dim3(BLOCK), 0,
                     (hipStream_t)stream, (const float*)rowloss,
                     (const int64_t*)labels, N, V, ignore, (float*)block);
  LAUNCH_CHECK();
  return 0;
}

template <int DT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void xent_bwd_kernel(
    const void* logits, const int64_t* __restrict__ labels,
    const float* __restrict__ rowmax, const float* __restrict__ logsum,
    const float* __restrict__ block, const float* __restrict__ gout,
    void* dlogits, int64_t V, int64_t ld, int64_t ignore) {
  // logits and dlogits may be one buffer: no __restrict__ on either
  const int64_t r = blockIdx.x;
  const int64_t label = labels[r];
  const char* row = (const char*)logits + r * ld * ElemSize<DT>::value;
  char* orow = (char*)dlogits + r * ld * ElemSize<DT>::value;
  // the host has checked that both rows sit alike mod 16
  const int head = xent_head<DT>(orow, ld);
  const void* body = row + head * ElemSize<DT>::value;
  void* obody = orow + head * ElemSize<DT>::value;
  const int64_t n8 = (ld - head) / 8;
  const int64_t tail0 = head + n8 * 8;

  if (!xent_valid(label, V, ignore)) {  // zeros, written without a read
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t i8 = threadIdx.x; i8 < n8; i8 += BLOCK)
      Vec8<DT>::store(obody, i8, z);
    if ((int)threadIdx.x < head) store_elem<DT>(orow, threadIdx.x, 0.f);
    if (tail0 + threadIdx.x < ld) store_elem<DT>(orow, tail0 + threadIdx.x, 0.f);
    return;
  }

  const float m = rowmax[r];
  const float lse = logsum[r];
  const float scale = gout[0] * block[1];

  // pad columns inside the row are loaded with their vector and dropped by
  // the select: whatever they hold, they get 0
#define XENT_GRAD8(v, col0)                                                   \
  do {                                                                        \
    const int64_t lj_ = label - (col0);                                       \
    const int64_t vj_ = V - (col0);                                           \
    _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) {                        \
      const float p_ = expf(((v)[j_] - m) - lse);                             \
      const float g_ = (p_ - (j_ == lj_ ? 1.f : 0.f)) * scale;                \
      (v)[j_] = j_ < vj_ ? g_ : 0.f;                                          \
    }                                                                         \
  } while (0)

  for (int64_t i8 = threadIdx.x; i8 < n8; i8 += 2 * BLOCK) {
    const int64_t k8 = i8 + BLOCK;
    const bool two = k8 < n8;
    float a[8], b[8];
    Vec8<DT>::load(body, i8, a);
    Vec8<DT>::load(body, two ? k8 : i8, b);
    XENT_GRAD8(a, head + i8 * 8);
    Vec8<DT>::store(obody, i8, a);
    if (two) {
      XENT_GRAD8(b, head + k8 * 8);
      Vec8<DT>::store(obody, k8, b);
    }
  }
#undef XENT_GRAD8
  if ((int)threadIdx.x < head) {
    const int64_t c = threadIdx.x;  // head <= ld, and c < V is tested
    float g = 0.f;
    if (c < V)
      g = (expf((load_elem<DT>(row, c) - m) - lse) - (c == label ? 1.f : 0.f)) * scale;
    store_elem<DT>(orow, c, g);
  }
  if (tail0 + threadIdx.x < ld) {
    const int64_t c = tail0 + threadIdx.x;
    float g = 0.f;
    if (c < V)
      g = (expf((load_elem<DT>(row, c) - m) - lse) - (c == label ? 1.f : 0.f)) * scale;
    store_elem<DT>(orow, c, g);
  }
}

SKY_EXPORT int sky_xent_bwd(uint64_t stream, uint64_t logits, uint64_t labels,
                            uint64_t rowmax, uint64_t logsum, uint64_t block,
                            uint64_t gout, uint64_t dlogits, int64_t N,
                            int64_t V, int64_t ld, int64_t ignore, int dt) {
  constexpr int BLOCK = 256;
  if (N < 0 || N > 0x7fffffffLL || V < 1 || V > ld) return (int)hipErrorInvalidValue;
  // one head/body/tail split serves the loads and the stores
  if ((logits ^ dlogits) & 15) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)N);
  if (dt == DT_F32)
    hipLaunchKernelGGL((xent_bwd_kernel<DT_F32, BLOCK>), grid, dim3(BLOCK), 0, s,
                       (const void*)logits, (const int64_t*)labels,
                       (const float*)rowmax, (const float*)logsum,
                       (const float*)block, (const float*)gout, (void*)dlogits,
                       V, ld, ignore);
  else
    hipLaunchKernelGGL((xent_bwd_kernel<DT_BF16, BLOCK>), grid, dim3(BLOCK), 0, s,
                       (const void*)logits, (const int64_t*)labels,
                       (const float*)rowmax, (const float*)logsum,
                       (const float*)block, (const float*)gout, (void*)dlogits,
                       V, ld, ignore);
  LAUNCH_CHECK();
  return 0;
}
