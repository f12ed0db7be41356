// Multi-tensor fused AdamW for gfx950, with the gradient clip folded in.
//
// Same launch shape as sgd.hip: the host packs one descriptor per slab into
// a device int64 array (ops/multi_tensor.py) and each block updates one
// slab. What differs is where the step's scalars live. Every value that
// changes from step to step is read from a small device "hyper block", so a
// step captured once in a hipGraph keeps counting, clipping and following
// the schedule when it is replayed with frozen launch arguments:
//
//   word  type   name       written by
//   0     float  lr         the host (a stream-ordered fill)
//   1     float  clip       sky_gradnorm_finish; stays 1 without clipping
//   2     float  gnorm      sky_gradnorm_finish (the unclipped L2 norm)
//   3     float  bc1        sky_adamw_tick: 1 - beta1^t
//   4     float  rsqrt_bc2  sky_adamw_tick: 1 / sqrt(1 - beta2^t)
//   5     -      unused
//   6     int32  t          sky_adamw_tick: the step count, advanced on the
//                           device; the host zeroes or restores it
//   7     -      unused
//
// One step is: [sky_gradnorm_partials, sky_gradnorm_finish,] sky_adamw_tick,
// sky_adamw_step, all on one stream. The norm stays two kernels so that a
// cross-rank sum of the one scalar can go between them.
//
// Per element, g loaded as fp32 and multiplied by clip (torch.optim.AdamW's
// semantics, eps outside the square root):
//   p  = p * (1 - lr*wd_slab)        wd_slab = 0 where the descriptor says so
//   m  = beta1*m + (1-beta1)*g
//   v  = beta2*v + (1-beta2)*g*g
//   p -= (lr/bc1) * m / (sqrt(v)*rsqrt_bc2 + eps)
// m and v are fp32 whatever the parameter's dtype. With fp32 masters the
// update runs on the master and the bf16 parameter is refreshed in the same
// pass: 2 (g) + 3*8 (master, m, v read and written) + 2 (p) = 28 B/element.
//
// I/O is plain write-back and the body is unrolled twice, the variant that
// won in-app for the SGD kernel (sgd.hip); there are no environment knobs.

#include "common.h"

struct AdamWDesc {
  uint64_t p, g, master, m, v;
  int64_t n;
  int64_t flags;  // bit 0: no weight decay for this tensor
};

struct AdamWHyper {
  float lr, clip, gnorm, bc1, rsqrt_bc2, pad0;
  int t;
  int pad1;
};

// The powers are taken once per step here, in double, so the update kernel
// stays memory-bound (a powf per element would make it VALU-bound).
__global__ void adamw_tick_kernel(AdamWHyper* h, double beta1, double beta2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int t = h->t + 1;
  h->t = t;
  h->bc1 = (float)(1.0 - pow(beta1, (double)t));
  h->rsqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(beta2, (double)t)));
}

SKY_EXPORT int sky_adamw_tick(uint64_t stream, uint64_t hyper, double beta1,
                              double beta2) {
  hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, (AdamWHyper*)hyper, beta1, beta2);
  LAUNCH_CHECK();
  return 0;
}

// partials[b] = sum of g^2 over descriptor b's slab, fp32. Each thread keeps
// one accumulator per vector element, and block_sum adds them in a fixed
// order: the same gradients give the same bits.
template <int DT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void gradnorm_partials_kernel(
    const AdamWDesc* __restrict__ descs, float* __restrict__ partials) {
  __shared__ float lds[BLOCK / WAVE];
  const AdamWDesc d = descs[blockIdx.x];
  const void* g = (const void*)d.g;
  const int64_t n8 = d.n / 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int64_t i8 = threadIdx.x; i8 < n8; i8 += BLOCK) {
    float gv[8];
    Vec8<DT>::load(g, i8, gv);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += gv[j] * gv[j];
  }
  for (int64_t i = n8 * 8 + threadIdx.x; i < d.n; i += BLOCK) {
    const float gv = load_elem<DT>(g, i);
    acc[0] += gv * gv;
  }
  float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) +
            ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  s = block_sum<BLOCK>(s, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

SKY_EXPORT int sky_gradnorm_partials(uint64_t stream, uint64_t descs,
                                     int64_t n_descs, uint64_t partials,
                                     int dt) {
  constexpr int BLOCK = 256;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)n_descs);
  if (dt == DT_F32)
    hipLaunchKernelGGL((gradnorm_partials_kernel<DT_F32, BLOCK>), grid,
                       dim3(BLOCK), 0, s, (const AdamWDesc*)descs,
                       (float*)partials);
  else
    hipLaunchKernelGGL((gradnorm_partials_kernel<DT_BF16, BLOCK>), grid,
                       dim3(BLOCK), 0, s, (const AdamWDesc*)descs,
                       (float*)partials);
  LAUNCH_CHECK();
  return 0;
}

// One block adds all partials in a fixed order (no atomics) and leaves the
// norm and torch.nn.utils.clip_grad_norm_'s factor in the hyper block.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void gradnorm_finish_kernel(
    const float* __restrict__ partials, int64_t n, AdamWHyper* h,
    float max_norm) {
  __shared__ float lds[BLOCK / WAVE];
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += BLOCK) acc += partials[i];
  acc = block_sum<BLOCK>(acc, lds);
  if (threadIdx.x == 0) {
    const float gnorm = sqrtf(acc);
    h->gnorm = gnorm;
    h->clip = fminf(1.f, max_norm / (gnorm + 1e-6f));
  }
}

SKY_EXPORT int sky_gradnorm_finish(uint64_t stream, uint64_t partials,
                                   int64_t n_descs, uint64_t hyper,
                                   float max_norm) {
  constexpr int BLOCK = 256;
  hipLaunchKernelGGL((gradnorm_finish_kernel<BLOCK>), dim3(1), dim3(BLOCK), 0,
                     (hipStream_t)stream, (const float*)partials, n_descs,
                     (AdamWHyper*)hyper, max_norm);
  LAUNCH_CHECK();
  return 0;
}

template <int DT, int BLOCK, bool MASTER>
__global__ __launch_bounds__(BLOCK) void adamw_kernel(
    const AdamWDesc* __restrict__ descs, const AdamWHyper* __restrict__ hyper,
    float beta1, float omb1, float beta2, float omb2, float eps, float wd) {
  constexpr int UNROLL = 2;
  const AdamWDesc d = descs[blockIdx.x];
  void* p = (void*)d.p;
  const void* g = (const void*)d.g;
  float* master = (float*)d.master;
  float* mbuf = (float*)d.m;
  float* vbuf = (float*)d.v;
  // the step's scalars, once per thread and in double: 1 - lr*wd and
  // lr/bc1 then carry one rounding each, whatever the compiler contracts
  const double lr = (double)hyper->lr;
  const float clip = hyper->clip;
  const float rs2 = hyper->rsqrt_bc2;
  const float step = (float)(lr / (double)hyper->bc1);
  const float decay = (float)(1.0 - lr * ((d.flags & 1) ? 0.0 : (double)wd));
  const int64_t n8 = d.n / 8;
  // vectorized body (slab bases are 16B-aligned; tail handled below)
  for (int64_t i8 = threadIdx.x; i8 < n8; i8 += UNROLL * BLOCK) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t k8 = i8 + u * BLOCK;
      if (k8 >= n8) break;
      float gv[8], pv[8], mv[8], vv[8];
      Vec8<DT>::load(g, k8, gv);
      if (MASTER) Vec8<DT_F32>::load(master, k8, pv);
      else Vec8<DT>::load(p, k8, pv);
      Vec8<DT_F32>::load(mbuf, k8, mv);
      Vec8<DT_F32>::load(vbuf, k8, vv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gg = gv[j] * clip;
        mv[j] = beta1 * mv[j] + omb1 * gg;
        vv[j] = beta2 * vv[j] + omb2 * gg * gg;
        pv[j] = pv[j] * decay - step * mv[j] / (sqrtf(vv[j]) * rs2 + eps);
      }
      Vec8<DT_F32>::store(mbuf, k8, mv);
      Vec8<DT_F32>::store(vbuf, k8, vv);
      if (MASTER) Vec8<DT_F32>::store(master, k8, pv);
      Vec8<DT>::store(p, k8, pv);
    }
  }
  for (int64_t i = n8 * 8 + threadIdx.x; i < d.n; i += BLOCK) {
    const float gg = load_elem<DT>(g, i) * clip;
    float pv = MASTER ? master[i] : load_elem<DT>(p, i);
    const float m = beta1 * mbuf[i] + omb1 * gg;
    const float v = beta2 * vbuf[i] + omb2 * gg * gg;
    pv = pv * decay - step * m / (sqrtf(v) * rs2 + eps);
    mbuf[i] = m;
    vbuf[i] = v;
    if (MASTER) master[i] = pv;
    store_elem<DT>(p, i, pv);
  }
}

// flags bit 0: the descriptors carry fp32 masters. beta1 and beta2 arrive as
// doubles so that 1 - beta is rounded to fp32 once (1.f - 0.999f is off by
// 1.3e-5 of itself).
SKY_EXPORT int sky_adamw_step(uint64_t stream, uint64_t descs, int64_t n_descs,
                              uint64_t hyper, double beta1, double beta2,
                              float eps, float wd, int dt, int flags) {
  constexpr int BLOCK = 256;
  const bool has_master = flags & 1;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)n_descs);
#define ADAMW(DT, MA)                                                        \
  hipLaunchKernelGGL((adamw_kernel<DT, BLOCK, MA>), grid, dim3(BLOCK), 0, s, \
                     (const AdamWDesc*)descs, (const AdamWHyper*)hyper,      \
                     (float)beta1, (float)(1.0 - beta1), (float)beta2,       \
                     (float)(1.0 - beta2), eps, wd)
  if (dt == DT_F32) {
    if (has_master) ADAMW(DT_F32, true); else ADAMW(DT_F32, false);
  } else {
    if (has_master) ADAMW(DT_BF16, true); else ADAMW(DT_BF16, false);
  }
#undef ADAMW
  LAUNCH_CHECK();
  return 0;
}
