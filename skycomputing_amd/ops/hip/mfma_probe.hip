// MFMA fragment-layout probe for gfx950: computes one 16x16 tile
// D = A(16x32) @ B(32x16) with v_mfma_f32_16x16x32_bf16 using the assumed
// lane->element mappings, so the GPU test can verify them against torch.
//
// Assumed mappings (verified by tests/test_ops_gpu.py::test_mfma_layout):
//   A[i][k]: lane l holds i = l%16, k = 8*(l/16) + j  (j = 0..7)
//   B[k][n]: lane l holds n = l%16, k = 8*(l/16) + j
//   D[i][n]: lane l holds n = l%16, i = 4*(l/16) + r  (r = 0..3)

#include "attn_common.h"

__global__ __launch_bounds__(64) void mfma_probe_kernel(
    const ushort_t* __restrict__ A, const ushort_t* __restrict__ B,
    float* __restrict__ D) {
  const int l = threadIdx.x;
  bf16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int i = l % 16, k = 8 * (l / 16) + j;
    a[j] = (short)A[i * 32 + k];
    int n = l % 16;
    b[j] = (short)B[k * 16 + n];
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int i = 4 * (l / 16) + r, n = l % 16;
    D[i * 16 + n] = acc[r];
  }
}

SKY_EXPORT int sky_mfma_probe(uint64_t stream, uint64_t A, uint64_t B,
                              uint64_t D) {
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, (const ushort_t*)A,
                     (const ushort_t*)B, (float*)D);
  LAUNCH_CHECK();
  return 0;
}

// Chained-MFMA probe: the D tiles of one MFMA as the B operand of the next,
// as the keys-on-rows attention kernels chain them. D = A(32x32) @ B(32x16)
// is two stacked D tiles T0 (rows 0..15) and T1; att_pack_dpair makes them a
// B operand whose slot (lg, j) stands for row (j < 4 ? 0 : 16) + lg*4 + (j & 3)
// of D, and abf_tr_rows64_2 reads the matching A operand from the row-major
// [k][64] sw7 image of A2^T (A2 is [16][32], i x k). D2 = A2 @ bf16(D).
__global__ __launch_bounds__(64) void mfma_chain_probe_kernel(
    const ushort_t* __restrict__ A, const ushort_t* __restrict__ B,
    const ushort_t* __restrict__ A2, float* __restrict__ D2) {
  __shared__ __attribute__((aligned(16))) char img[32 * 128];
  const int l = threadIdx.x;
  const int lm = l & 15, lg = l >> 4;
  // image row k, column i of A2^T (columns 16..63 unused, zeroed)
  for (int u = l; u < 32 * 64; u += 64) {
    const int k = u >> 6, i = u & 63;
    *(ushort_t*)lds_at(img, swz(k * 128 + i * 2, k, 7)) =
        i < 16 ? A2[i * 32 + k] : (ushort_t)0;
  }
  __syncthreads();
  bf16x8 b;
#pragma unroll
  for (int j = 0; j < 8; ++j) b[j] = (short)B[(8 * lg + j) * 16 + lm];
  f32x4 t[2];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    bf16x8 a;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (short)A[(tt * 16 + lm) * 32 + 8 * lg + j];
    t[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    t[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, t[tt], 0, 0, 0);
  }
  const bf16x8 bd = att_pack_dpair(t[0], t[1]);
  const bf16x8 a2 = abf_tr_rows64_2(img, 0, lg * 4, 16 + lg * 4, 0, lm);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, bd, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) D2[(4 * lg + r) * 16 + lm] = acc[r];
}

SKY_EXPORT int sky_mfma_chain_probe(uint64_t stream, uint64_t A, uint64_t B,
                                    uint64_t A2, uint64_t D2) {
  hipLaunchKernelGGL(mfma_chain_probe_kernel, dim3(1), dim3(64), 0,
                     (hipStream_t)stream, (const ushort_t*)A,
                     (const ushort_t*)B, (const ushort_t*)A2, (float*)D2);
  LAUNCH_CHECK();
  return 0;
}

// glds semantics probe: copy 4 KB global -> LDS via global_load_lds with a
// per-lane (mode 0) or wave-uniform (mode 1) LDS pointer, then write the
// LDS back out so the host can check which addressing lands correctly.
typedef const __attribute__((address_space(1))) unsigned int* gp_u32;
typedef __attribute__((address_space(3))) unsigned int* lp_u32;

__global__ __launch_bounds__(256) void glds_probe_kernel(
    const ushort_t* __restrict__ src, ushort_t* __restrict__ dst, int mode) {
  __shared__ __attribute__((aligned(16))) char lbuf[4096];
  const int tid = threadIdx.x;
  const int w = tid >> 6;
  const ushort_t* g = src + tid * 8;
  if (mode == 0) {
    __builtin_amdgcn_global_load_lds((gp_u32)g, (lp_u32)(lbuf + tid * 16), 16, 0, 0);
  } else {
    __builtin_amdgcn_global_load_lds((gp_u32)g, (lp_u32)(lbuf + w * 64 * 16), 16, 0, 0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  *(ushort8_t*)(dst + tid * 8) = *(const ushort8_t*)(lbuf + tid * 16);
}

SKY_EXPORT int sky_glds_probe(uint64_t stream, uint64_t src, uint64_t dst,
                              int mode) {
  hipLaunchKernelGGL(glds_probe_kernel, dim3(1), dim3(256), 0,
                     (hipStream_t)stream, (const ushort_t*)src,
                     (ushort_t*)dst, mode);
  LAUNCH_CHECK();
  return 0;
}
