// Multi-tensor fused LAMB for gfx950: Adam's direction, scaled per tensor by
// the trust ratio ||p|| / ||u||.
//
// The update of one element depends on two norms over its whole tensor, and
// a tensor is spread over many slabs, so over many blocks. The step is
// therefore two passes over the slabs with a small per-tensor kernel
// between them, and the update direction u is never stored: a scratch
// buffer for it would be 4 B per parameter (8 GB at the 160-layer model).
// Stage 2 recomputes u from the moments that stage 1 left, through the same
// inline expression (lamb_update), whose roundings are spelled out so that
// both kernels get the same bits whatever the compiler contracts.
//
// One step is: [sky_gradnorm_partials, sky_gradnorm_finish,] sky_adamw_tick
// (all three from adamw.hip, unchanged), sky_lamb_stage1, sky_lamb_ratios,
// sky_lamb_stage2, on one stream. The descriptor table has AdamW's row
// layout, which is why the gradient-norm kernels run on it as it is; LAMB
// adds the tensor index in the high half of the flags word. The step's
// scalars come from AdamW's device hyper block (layout in adamw.hip): lr,
// clip, bc1, rsqrt_bc2. No launch argument changes between steps, so a step
// captured once stays live under replay.
//
// Per element, with g loaded as fp32 and multiplied by clip:
//   m = beta1*m + (1-beta1)*g
//   v = beta2*v + (1-beta2)*g*g
//   u = (m/bc1) / (sqrt(v)*rsqrt_bc2 + eps) + wd_T*p     wd_T = 0: no_decay
//   r_T = ||p|| / ||u||  if T adapts and both norms are > 0, else 1
//   p -= lr * r_T * u
// p is the fp32 master where there is one; the norms are taken over it.
//
//   sky_lamb_stage1  one block per slab. Reads g, m, v, p; writes m and v
//                    (final); leaves the slab's sum of p^2 and of u^2.
//   sky_lamb_ratios  one wave per tensor. Adds the tensor's slab partials
//                    and writes r_T, ||p|| and ||u||.
//   sky_lamb_stage2  one block per slab. Reads m, v, p; writes p (and the
//                    bf16 parameter next to its master).
// All sums are taken in a fixed order (one accumulator per vector lane, a
// fixed tree, block_sum; lane-strided, wave_sum) and there are no atomics:
// the same inputs give the same bits.
//
// Bytes per element with masters and bf16 parameters: stage 1 reads
// 2 (g) + 4 (master) + 8 (m, v) = 14 and writes 8; stage 2 reads 12 and
// writes 4 + 2 = 6. 40 B/element in all, against AdamW's 28: the price of
// not keeping u is reading m, v and p a second time.

#include "common.h"

// adamw.hip's AdamWDesc, row for row (the host builds both tables with the
// same splitter); flags bit 0: no weight decay, bits 32..62: tensor index
struct LambDesc {
  uint64_t p, g, master, m, v;
  int64_t n;
  int64_t flags;
};
static_assert(sizeof(LambDesc) == 56, "row layout shared with AdamWDesc");

// adamw.hip's AdamWHyper
struct LambHyper {
  float lr, clip, gnorm, bc1, rsqrt_bc2, pad0;
  int t;
  int pad1;
};
static_assert(sizeof(LambHyper) == 32, "the AdamW hyper block");

DEV int lamb_tensor_of(const LambDesc& d) { return (int)(d.flags >> 32); }

// u for one element. Every multiply-add is an explicit fmaf and the other
// products feed a divide, so nothing is left for fp contraction to decide.
DEV float lamb_update(float m, float v, float p, float inv_bc1, float rs2,
                      float eps, float wd) {
  return fmaf(wd, p, (m * inv_bc1) / fmaf(sqrtf(v), rs2, eps));
}

// the scalars both stages derive from the hyper block, once per thread
struct LambScalars {
  float inv_bc1, rs2, wd;
};
DEV LambScalars lamb_scalars(const LambHyper* h, const LambDesc& d, float wd) {
  LambScalars s;
  s.inv_bc1 = (float)(1.0 / (double)h->bc1);
  s.rs2 = h->rsqrt_bc2;
  s.wd = (d.flags & 1) ? 0.f : wd;
  return s;
}

DEV float tree8(const float a[8]) {
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// partials[2*b] = sum p^2, partials[2*b + 1] = sum u^2 over slab b
template <int DT, int BLOCK, bool MASTER>
__global__ __launch_bounds__(BLOCK) void lamb_stage1_kernel(
    const LambDesc* __restrict__ descs, const LambHyper* __restrict__ hyper,
    float* __restrict__ partials, float beta1, float omb1, float beta2,
    float omb2, float eps, float wd) {
  constexpr int UNROLL = 2;
  __shared__ float lds[BLOCK / WAVE];
  const LambDesc d = descs[blockIdx.x];
  const void* p = (const void*)d.p;
  const void* g = (const void*)d.g;
  const float* master = (const float*)d.master;
  float* mbuf = (float*)d.m;
  float* vbuf = (float*)d.v;
  const float clip = hyper->clip;
  const LambScalars s = lamb_scalars(hyper, d, wd);
  float accp[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float accu[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int64_t n8 = d.n / 8;
  // vectorized body (slab bases are 16B-aligned; tail handled below)
  for (int64_t i8 = threadIdx.x; i8 < n8; i8 += UNROLL * BLOCK) {
#pragma unroll
    for (int r = 0; r < UNROLL; ++r) {
      const int64_t k8 = i8 + r * BLOCK;
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
        mv[j] = fmaf(beta1, mv[j], omb1 * gg);
        vv[j] = fmaf(beta2, vv[j], (omb2 * gg) * gg);
        const float u =
            lamb_update(mv[j], vv[j], pv[j], s.inv_bc1, s.rs2, eps, s.wd);
        accp[j] = fmaf(pv[j], pv[j], accp[j]);
        accu[j] = fmaf(u, u, accu[j]);
      }
      Vec8<DT_F32>::store(mbuf, k8, mv);
      Vec8<DT_F32>::store(vbuf, k8, vv);
    }
  }
  for (int64_t i = n8 * 8 + threadIdx.x; i < d.n; i += BLOCK) {
    const float gg = load_elem<DT>(g, i) * clip;
    const float pv = MASTER ? master[i] : load_elem<DT>(p, i);
    const float m = fmaf(beta1, mbuf[i], omb1 * gg);
    const float v = fmaf(beta2, vbuf[i], (omb2 * gg) * gg);
    const float u = lamb_update(m, v, pv, s.inv_bc1, s.rs2, eps, s.wd);
    accp[0] = fmaf(pv, pv, accp[0]);
    accu[0] = fmaf(u, u, accu[0]);
    mbuf[i] = m;
    vbuf[i] = v;
  }
  const float sp = block_sum<BLOCK>(tree8(accp), lds);
  const float su = block_sum<BLOCK>(tree8(accu), lds);
  if (threadIdx.x == 0) {
    partials[2 * (int64_t)blockIdx.x] = sp;
    partials[2 * (int64_t)blockIdx.x + 1] = su;
  }
}

// Tensor T owns the slabs first[T] .. first[T+1]-1. Its wave adds their
// partials lane-strided (a tensor with more than 64 slabs makes it loop),
// then across the lanes. out is three planes of n_tensors floats: the trust
// ratio, ||p|| and ||u||.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void lamb_ratios_kernel(
    const float* __restrict__ partials, const int* __restrict__ first,
    const int* __restrict__ adapt, float* __restrict__ out, int n_tensors) {
  const int t = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  if (t >= n_tensors) return;  // the whole wave leaves together
  const int lane = threadIdx.x & (WAVE - 1);
  const int end = first[t + 1];
  float sp = 0.f, su = 0.f;
  for (int b = first[t] + lane; b < end; b += WAVE) {
    sp += partials[2 * (int64_t)b];
    su += partials[2 * (int64_t)b + 1];
  }
  sp = wave_sum(sp);
  su = wave_sum(su);
  if (lane == 0) {
    const float pn = sqrtf(sp), un = sqrtf(su);
    out[t] = (adapt[t] && pn > 0.f && un > 0.f) ? pn / un : 1.f;
    out[n_tensors + t] = pn;
    out[2 * n_tensors + t] = un;
  }
}

template <int DT, int BLOCK, bool MASTER>
__global__ __launch_bounds__(BLOCK) void lamb_stage2_kernel(
    const LambDesc* __restrict__ descs, const LambHyper* __restrict__ hyper,
    const float* __restrict__ ratios, float eps, float wd) {
  constexpr int UNROLL = 2;
  const LambDesc d = descs[blockIdx.x];
  void* p = (void*)d.p;
  float* master = (float*)d.master;
  const float* mbuf = (const float*)d.m;
  const float* vbuf = (const float*)d.v;
  const LambScalars s = lamb_scalars(hyper, d, wd);
  const float nstep = -(hyper->lr * ratios[lamb_tensor_of(d)]);
  const int64_t n8 = d.n / 8;
  for (int64_t i8 = threadIdx.x; i8 < n8; i8 += UNROLL * BLOCK) {
#pragma unroll
    for (int r = 0; r < UNROLL; ++r) {
      const int64_t k8 = i8 + r * BLOCK;
      if (k8 >= n8) break;
      float pv[8], mv[8], vv[8];
      if (MASTER) Vec8<DT_F32>::load(master, k8, pv);
      else Vec8<DT>::load(p, k8, pv);
      Vec8<DT_F32>::load(mbuf, k8, mv);
      Vec8<DT_F32>::load(vbuf, k8, vv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float u =
            lamb_update(mv[j], vv[j], pv[j], s.inv_bc1, s.rs2, eps, s.wd);
        pv[j] = fmaf(nstep, u, pv[j]);
      }
      if (MASTER) Vec8<DT_F32>::store(master, k8, pv);
      Vec8<DT>::store(p, k8, pv);
    }
  }
  for (int64_t i = n8 * 8 + threadIdx.x; i < d.n; i += BLOCK) {
    float pv = MASTER ? master[i] : load_elem<DT>(p, i);
    const float u =
        lamb_update(mbuf[i], vbuf[i], pv, s.inv_bc1, s.rs2, eps, s.wd);
    pv = fmaf(nstep, u, pv);
    if (MASTER) master[i] = pv;
    store_elem<DT>(p, i, pv);
  }
}

// flags bit 0: the descriptors carry fp32 masters. beta1 and beta2 arrive as
// doubles so that 1 - beta is rounded to fp32 once, as in sky_adamw_step.
SKY_EXPORT int sky_lamb_stage1(uint64_t stream, uint64_t descs, int64_t n_descs,
                               uint64_t hyper, uint64_t partials, double beta1,
                               double beta2, float eps, float wd, int dt,
                               int flags) {
  constexpr int BLOCK = 256;
  const bool has_master = flags & 1;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)n_descs);
#define LAMB1(DT, MA)                                                        \
  hipLaunchKernelGGL((lamb_stage1_kernel<DT, BLOCK, MA>), grid, dim3(BLOCK), \
                     0, s, (const LambDesc*)descs, (const LambHyper*)hyper,  \
                     (float*)partials, (float)beta1, (float)(1.0 - beta1),   \
                     (float)beta2, (float)(1.0 - beta2), eps, wd)
  if (dt == DT_F32) {
    if (has_master) LAMB1(DT_F32, true); else LAMB1(DT_F32, false);
  } else {
    if (has_master) LAMB1(DT_BF16, true); else LAMB1(DT_BF16, false);
  }
#undef LAMB1
  LAUNCH_CHECK();
  return 0;
}

SKY_EXPORT int sky_lamb_ratios(uint64_t stream, uint64_t partials,
                               uint64_t first, uint64_t adapt, uint64_t out,
                               int64_t n_tensors) {
  constexpr int BLOCK = 256;
  constexpr int PER_BLOCK = BLOCK / WAVE;
  dim3 grid((unsigned)((n_tensors + PER_BLOCK - 1) / PER_BLOCK));
  hipLaunchKernelGGL((lamb_ratios_kernel<BLOCK>), grid, dim3(BLOCK), 0,
                     (hipStream_t)stream, (const float*)partials,
                     (const int*)first, (const int*)adapt, (float*)out,
                     (int)n_tensors);
  LAUNCH_CHECK();
  return 0;
}

SKY_EXPORT int sky_lamb_stage2(uint64_t stream, uint64_t descs, int64_t n_descs,
                               uint64_t hyper, uint64_t ratios, float eps,
                               float wd, int dt, int flags) {
  constexpr int BLOCK = 256;
  const bool has_master = flags & 1;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)n_descs);
#define LAMB2(DT, MA)                                                        \
  hipLaunchKernelGGL((lamb_stage2_kernel<DT, BLOCK, MA>), grid, dim3(BLOCK), \
                     0, s, (const LambDesc*)descs, (const LambHyper*)hyper,  \
                     (const float*)ratios, eps, wd)
  if (dt == DT_F32) {
    if (has_master) LAMB2(DT_F32, true); else LAMB2(DT_F32, false);
  } else {
    if (has_master) LAMB2(DT_BF16, true); else LAMB2(DT_BF16, false);
  }
#undef LAMB2
  LAUNCH_CHECK();
  return 0;
}
