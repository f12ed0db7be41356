// Fused multi-head attention forward for gfx950 (MFMA 16x16x32 bf16).
//
// Computes out = dropout(softmax(scale * Q K^T + mask)) V for one (batch,
// head) per workgroup, S <= 128, d = 64 (BERT-large heads) — replacing the
// reference's QK^T GEMM + mask-add + softmax + dropout + PV GEMM + head
// permutes (reference: scaelum/model/bert_layers.py:249-275) with ONE
// kernel. The S x S score matrix never touches HBM; row max / row sum are
// saved (fp32) so backward recomputes probabilities with sky_attn_probs.
//
// Layouts (chosen so no transpose copies happen anywhere in the layer):
//   qkv  [B, S, 3, h, d]  — straight out of the fused QKV GEMM
//   out  [B, S, h, d]     — views as [B, S, h*d] for the output projection
//
// Structure per workgroup (4 waves, 256 threads):
//   * K tile staged to LDS [S][64] (XOR-swizzled), V staged TRANSPOSED to
//     LDS [64][S] so PV's B-fragments are contiguous ds_read_b128;
//   * each wave owns 32 query rows: QK^T via mfma_f32_16x16x32_bf16
//     (A = Q fragments straight from global, B = K from LDS), softmax in
//     registers (subwave shuffles), dropout via the counter RNG, P written
//     to a per-wave LDS tile, PV via MFMA (A = P, B = V^T from LDS).
//
// Fragment mappings verified on hardware by sky_mfma_probe
// (tests/test_ops_gpu.py::test_mfma_layout).
//
// attn_fwd_kernel (the structure above) serves probs mode and
// SKY_ATTN_KROWS=0; the default forward is attn_fwd_krows_kernel below.

#include "attn_common.h"

// LDS layout (bytes): K [128][64]bf16 at 0 (16K); P per wave [32][128]
// at 16K + w*8K (32K). After QK^T, V^T [64][128] ALIASES K's region
// (K is dead) — total 48K, so 3 workgroups fit per CU (160K LDS) instead
// of 2, +50% latency-hiding concurrency.
#define K_OFF 0
#define VT_OFF 0
#define P_OFF (16 * 1024)
#define ATT_LDS_BYTES (48 * 1024)

template <bool HAS_MASK, bool SAVE_ML, bool PROBS_MODE, bool TRV = false>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ mask,
    ushort_t* __restrict__ out, float* __restrict__ m_io,
    float* __restrict__ l_io, ushort_t* __restrict__ p_out,
    ushort_t* __restrict__ pd_out, int B, int S, int h, float scale,
    float keep, uint64_t salt, const unsigned long long* __restrict__ state) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int l = tid & 63;
  const int w = tid >> 6;
  const int bh = blockIdx.x;
  const int b = bh / h;
  const int hh = bh % h;
  const int ts = 3 * h * ATT_D;  // token stride in qkv
  const int NT = (S + 15) / 16;  // 16-token k tiles
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* qbase = qkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
  const ushort_t* kbase = qbase + (size_t)h * ATT_D;
  const ushort_t* vbase = qbase + (size_t)2 * h * ATT_D;

  // ---- zero LDS when S < full tile coverage (avoid NaN poisoning) ----
  if (S < ATT_SMAX) {
    for (int u = tid; u < ATT_LDS_BYTES / 16; u += 256)
      *(ushort8_t*)lds_at(lds, u * 16) = (ushort8_t)(ushort_t)0;
    __syncthreads();
  }

  // ---- stage K into LDS [S][64] via global_load_lds ----
  att_glds_rows(kbase, ts, 0, S, false, S, lds, K_OFF, tid);
  // ---- per-wave constants (issued BEFORE the barrier so the global
  // loads land under the staging latency) ----
  const int qt0 = 2 * w;
  const int lm = l & 15;
  const int lg = l >> 4;  // lane group 0..3

  // additive mask values for this lane's k columns (col = kt*16 + lm)
  float mval[8];
  att_mask_cols<HAS_MASK>(mval, mask, b, S, lm);
  // Q fragments for both q tiles (independent of LDS)
  bf16x8 aq_all[2][2];
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    int qtok = (qt0 + qi) * 16 + lm;
    if (qtok >= S) qtok = S - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      aq_all[qi][ks] = *(const bf16x8*)(qbase + (size_t)qtok * ts + ks * 32 + lg * 8);
  }
  __syncthreads();

#pragma clang loop unroll(disable)
  for (int qi = 0; qi < 2; ++qi) {
    const int qtile = qt0 + qi;
    const int qtok_base = qtile * 16;
    if (qtok_base >= S) break;
    // A fragments of Q (preloaded before the barrier)
    bf16x8 aq[2] = {aq_all[qi][0], aq_all[qi][1]};
    f32x4 sacc[8];
    att_zero(sacc);
    att_score_tile(sacc, aq, lds, K_OFF, NT, lm, lg);
    // softmax over this wave's 4 rows per (lg, r); the transformed
    // scores overwrite sacc in place (register budget)
    float mx[4], sm[4], inv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) mx[r] = -3.0e38f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      if (kt >= NT) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float zz = sacc[kt][r] * scale + mval[kt];
        sacc[kt][r] = zz;
        mx[r] = fmaxf(mx[r], zz);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) mx[r] = row16_max(mx[r]);
    float mrow[4], lrow[4];
    if (PROBS_MODE) {
      // use saved statistics for exact recomputation
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = qtok_base + lg * 4 + r;
        const int rr = row < S ? row : S - 1;
        mrow[r] = m_io[((size_t)bh) * S + rr];
        lrow[r] = l_io[((size_t)bh) * S + rr];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) sm[r] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      if (kt >= NT) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = __expf(sacc[kt][r] - (PROBS_MODE ? mrow[r] : mx[r]));
        sacc[kt][r] = p;
        sm[r] += p;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sm[r] = row16_sum(sm[r]);
      inv[r] = 1.f / (PROBS_MODE ? lrow[r] : sm[r]);
    }
    if (SAVE_ML && lm == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = qtok_base + lg * 4 + r;
        if (row < S) {
          m_io[((size_t)bh) * S + row] = mx[r];
          l_io[((size_t)bh) * S + row] = sm[r];
        }
      }
    }
    // normalize, dropout, write P (LDS in fwd mode; global in probs mode).
    // The fused backward kernels regenerate this mask (att_drop_hash /
    // att_drop_keep); the decomposed backward reads it off Pd != 0.
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = qtok_base + lg * 4 + r;
      uint64_t z[2] = {0, 0};
      if (keep < 1.f) att_drop_hash(z, seed, bh, S, row, lm);
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        if (kt >= NT) continue;
        const int col = kt * 16 + lm;
        float p = sacc[kt][r] * inv[r];
        float pd = p;
        if (keep < 1.f) pd = att_drop_keep(z, kt, keep16) ? p * inv_keep : 0.f;
        if (PROBS_MODE) {
          if (row < S && col < S) {
            p_out[((size_t)bh * S + row) * S + col] = f32_to_bf16(p);
            pd_out[((size_t)bh * S + row) * S + col] = f32_to_bf16(pd);
          }
        } else {
          const int rl = qi * 16 + lg * 4 + r;  // local row 0..31
          *(ushort_t*)lds_at(
              lds, swz(P_OFF + w * 8192 + rl * 256 + col * 2, rl, 15)) =
              f32_to_bf16((row < S && col < S) ? pd : 0.f);
        }
      }
    }
  }

  if (PROBS_MODE) return;

  // PV accumulators live only from here (declaring them earlier keeps 32
  // VGPRs hot through the scores/softmax phase and forces spills)
  f32x4 oacc[2][4];
  att_zero(oacc[0]);
  att_zero(oacc[1]);

  // ---- stage V over K's (now dead) region ----
  __syncthreads();  // all waves done reading K and writing their P tiles
  if (TRV) {
    // DIRECT [tok][64] sw7 row image via glds; PV reads it TRANSPOSED
    // with ds_read_b64_tr_b16 (garbage rows tok>=S multiply P zeros)
    att_glds_rows(vbase, ts, 0, 128, true, S, lds, VT_OFF, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    if (S < ATT_SMAX) {
      for (int u = tid; u < (16 * 1024) / 16; u += 256)
        *(ushort8_t*)lds_at(lds, VT_OFF + u * 16) = (ushort8_t)(ushort_t)0;
      __syncthreads();  // zero before scattered staging writes land
    }
    for (int u = tid; u < S * 8; u += 256) {
      const int tok = u >> 3;
      const int c16 = u & 7;
      ushort8_t v = *(const ushort8_t*)(vbase + (size_t)tok * ts + c16 * 8);
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int j = (jj + tok) & 7;  // bank-spread write order (see bwd2)
        const int c = c16 * 8 + j;
        *(ushort_t*)lds_at(lds, swz(VT_OFF + c * 256 + tok * 2, c, 15)) = v[j];
      }
    }
  }
  __syncthreads();

  // ---- PV: O[32 rows][64] per wave ----
  // (same-wave LDS write->read; compiler inserts the lgkm waits)
  for (int qi = 0; qi < 2; ++qi) {
    if ((qt0 + qi) * 16 >= S) break;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (ks * 32 >= S) break;
      // A fragment: P rows
      const int rl = qi * 16 + lm;
      bf16x8 ap = *(const bf16x8*)lds_at(
          lds, swz(P_OFF + w * 8192 + rl * 256 + (ks * 32 + lg * 8) * 2, rl, 15));
#pragma unroll
      for (int dvt = 0; dvt < 4; ++dvt) {
        bf16x8 bv;
        if (TRV) {
          bv = abf_tr_rows64(lds, VT_OFF, ks * 32 + lg * 8, dvt * 4, lm);
        } else {
          const int dv = dvt * 16 + lm;
          bv = *(const bf16x8*)lds_at(
              lds, swz(VT_OFF + dv * 256 + (ks * 32 + lg * 8) * 2, dv, 15));
        }
        oacc[qi][dvt] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap, bv, oacc[qi][dvt], 0, 0, 0);
      }
    }
  }
  // write out [B,S,h,d]
  ushort_t* obase = out + ((size_t)b * S * h + hh) * ATT_D;
#pragma unroll
  for (int qi = 0; qi < 2; ++qi)
    att_store_rows16(obase, h * ATT_D, oacc[qi], (qt0 + qi) * 16, S, lm, lg);
}

// ---------------------------------------------------------------------------
// Forward with the KEYS on the MFMA rows (the default; SKY_ATTN_KROWS=0
// restores attn_fwd_kernel). S^T = K Q^T comes out of the MFMA with a lane
// holding four consecutive keys of ONE query, which is a B operand of
// O^T = V^T Pd^T as it stands (att_pack_dpair), so P never goes to LDS:
//   * K and V are both staged up front by glds, one barrier in the kernel;
//   * m, l are per-lane scalars: the lane's own registers + two shuffles;
//   * O^T leaves a lane with four consecutive d of its token: 8-byte stores.
// One block per (b, h, 64*QPW-query block); a wave owns QPW 16-query tiles
// 64 queries apart. LDS: K [128][64] sw7 @0, V @16K, key mask fp32 @32K.
#define KR_K_OFF KR_IMG0_OFF
#define KR_V_OFF KR_IMG1_OFF
#define KR_MASK_OFF KR_AUX_OFF
#define KR_LDS_BYTES (KR_AUX_OFF + 512)

template <bool HAS_MASK, int QPW>
__global__ __launch_bounds__(256, 4) void attn_fwd_krows_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ mask,
    ushort_t* __restrict__ out, float* __restrict__ m_io,
    float* __restrict__ l_io, int B, int S, int h, float scale, float keep,
    uint64_t salt, const unsigned long long* __restrict__ state) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int l = tid & 63;
  const int w = tid >> 6;
  const int lm = l & 15;
  const int lg = l >> 4;
  const int QB = (S + 64 * QPW - 1) / (64 * QPW);
  const int bh = blockIdx.x / QB;
  const int qb = blockIdx.x % QB;
  const int b = bh / h;
  const int hh = bh % h;
  const int ts = 3 * h * ATT_D;
  const int NT = (S + 15) / 16;
  const int NP = (S + 31) / 32;  // key-tile pairs = PV contraction steps
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* qbase = qkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
  const ushort_t* kbase = qbase + (size_t)h * ATT_D;
  const ushort_t* vbase = qbase + (size_t)2 * h * ATT_D;
  float* mk = (float*)lds_at(lds, KR_MASK_OFF);

  // whole tile pairs are staged; tokens >= S re-read token S-1, finite
  // values that the -3e38 mask (scores) and the zero P (PV) null
  att_glds_rows(kbase, ts, 0, NP * 32, true, S, lds, KR_K_OFF, tid);
  att_glds_rows(vbase, ts, 0, NP * 32, true, S, lds, KR_V_OFF, tid);
  att_mask_keys_lds(mk, HAS_MASK, mask, b, S, tid);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  ushort_t* obase = out + ((size_t)b * S * h + hh) * ATT_D;
#pragma clang loop unroll(disable)
  for (int qi = 0; qi < QPW; ++qi) {
    const int qtok_base = (qb * QPW + qi) * 64 + w * 16;
    if (qtok_base >= S) break;
    const int q = qtok_base + lm;  // this lane's query
    const int qc = q < S ? q : S - 1;
    bf16x8 bq[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      bq[ks] = *(const bf16x8*)(qbase + (size_t)qc * ts + ks * 32 + lg * 8);
    f32x4 sacc[8];
    att_zero(sacc);
    att_score_tile_t(sacc, bq, lds, KR_K_OFF, NT, lm, lg);
    float mx = -3.0e38f;
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
      if (mt >= NT) continue;
      const f32x4 mv = att_mask_keys4(mk, mt, lg);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float zz = sacc[mt][r] * scale + mv[r];
        sacc[mt][r] = zz;
        mx = fmaxf(mx, zz);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sm = 0.f;
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
      if (mt >= NT) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = __expf(sacc[mt][r] - mx);
        sacc[mt][r] = p;
        sm += p;
      }
    }
    sm += __shfl_xor(sm, 16, 64);
    sm += __shfl_xor(sm, 32, 64);
    const float inv = 1.f / sm;
    if (lg == 0 && q < S) {
      m_io[(size_t)bh * S + q] = mx;
      l_io[(size_t)bh * S + q] = sm;
    }
    // normalize + dropout in place; keys >= S hold exact zeros already
    uint64_t z[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    if (keep < 1.f) att_drop_hash_krows(z, seed, bh, S, q, lg);
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
      if (mt >= NT) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = sacc[mt][r] * inv;
        if (keep < 1.f) p = att_drop_keep(z[r], mt, keep16) ? p * inv_keep : 0.f;
        sacc[mt][r] = p;
      }
    }
    // O^T = V^T Pd^T: B = the score registers, A = V^T by tr16
    f32x4 oacc[4];
    att_zero(oacc);
#pragma unroll
    for (int kp = 0; kp < 4; ++kp) {
      if (kp >= NP) continue;
      const bf16x8 bp = att_pack_dpair(sacc[2 * kp], sacc[2 * kp + 1]);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const bf16x8 av = abf_tr_rows64_2(lds, KR_V_OFF, kp * 32 + lg * 4,
                                          kp * 32 + 16 + lg * 4, ct * 4, lm);
        oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bp, oacc[ct], 0, 0, 0);
      }
    }
    att_store_cols16(obase, h * ATT_D, oacc, qtok_base, S, lm, lg);
  }
}

// pack dQ/dK/dV (each [B,h,S,d] contiguous) into dqkv [B,S,3,h,d] in one
// pass — replaces three permute-copies in the attention backward.
template <int DT>
__global__ __launch_bounds__(256) void pack3_kernel(
    const void* __restrict__ s0, const void* __restrict__ s1,
    const void* __restrict__ s2, void* __restrict__ dst, int64_t B,
    int64_t S, int64_t h, int64_t d8) {
  const int64_t n = B * h * S * d8;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n;
       u += (int64_t)gridDim.x * 256) {
    int64_t t = u;
    const int64_t di = t % d8; t /= d8;
    const int64_t tok = t % S; t /= S;
    const int64_t hh = t % h;
    const int64_t b = t / h;
    const int64_t src_off = u;  // [B,h,S,d] contiguous
    const int64_t dst_base = (((b * S + tok) * 3) * h + hh) * d8 + di;
    float v[8];
    Vec8<DT>::load(s0, src_off, v);
    Vec8<DT>::store(dst, dst_base, v);
    Vec8<DT>::load(s1, src_off, v);
    Vec8<DT>::store(dst, dst_base + h * d8, v);
    Vec8<DT>::load(s2, src_off, v);
    Vec8<DT>::store(dst, dst_base + 2 * h * d8, v);
  }
}

SKY_EXPORT int sky_pack3(uint64_t stream, uint64_t s0, uint64_t s1,
                         uint64_t s2, uint64_t dst, int64_t B, int64_t S,
                         int64_t h, int64_t d, int dt) {
  if (d % 8 != 0) return (int)hipErrorInvalidValue;
  const int64_t n = B * h * S * (d / 8);
  unsigned grid = (unsigned)((n + 255) / 256);
  if (grid > 2048u) grid = 2048u;
  hipStream_t s = (hipStream_t)stream;
  if (dt == DT_F32)
    hipLaunchKernelGGL((pack3_kernel<DT_F32>), dim3(grid), dim3(256), 0, s,
                       (const void*)s0, (const void*)s1, (const void*)s2,
                       (void*)dst, B, S, h, d / 8);
  else
    hipLaunchKernelGGL((pack3_kernel<DT_BF16>), dim3(grid), dim3(256), 0, s,
                       (const void*)s0, (const void*)s1, (const void*)s2,
                       (void*)dst, B, S, h, d / 8);
  LAUNCH_CHECK();
  return 0;
}

static int attn_launch(uint64_t stream, uint64_t qkv, uint64_t mask,
                       uint64_t out, uint64_t m, uint64_t lsum, uint64_t p,
                       uint64_t pd, int64_t B, int64_t S, int64_t h,
                       int64_t d, float scale, float keep, uint64_t salt,
                       uint64_t state, bool probs_mode) {
  if (d != ATT_D || S > ATT_SMAX) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)(B * h));
  size_t lds_bytes = ATT_LDS_BYTES;
  bool hm = mask != 0;
  // (a split-q forward variant — 2 blocks per (b,h), 32K LDS — measured
  // SLOWER than this one-block kernel: 29.2 vs 27.2 us; the duplicated K
  // staging doesn't pay without an occupancy gain, and the fwd register
  // budget pins 2 waves/SIMD either way. See profiles/r01_notes.md.)
  // Default: stage V DIRECT via glds and read PV fragments with
  // ds_read_b64_tr_b16 — measured 27.0 vs 30.3 us standalone and
  // -0.55 ms/step in-app over the register-transpose V^T staging.
  // SKY_ATTN_TRV=0 restores the old staging for A/B.
  const char* trve = getenv("SKY_ATTN_TRV");
  const bool trv = !(trve && trve[0] == '0');
  // Default: the keys-on-rows kernel, one block per (b, h, 64-query block).
  // SKY_ATTN_KROWS=0 restores attn_fwd_kernel; =2 runs the keys-on-rows
  // kernel with one block per (b, h, 128 queries), K and V staged once per
  // head, for A/B (profiles/r11_notes.md). Probs mode keeps attn_fwd_kernel.
  const char* kre = getenv("SKY_ATTN_KROWS");
  if (!probs_mode && !(kre && kre[0] == '0')) {
    const bool wide = kre && kre[0] == '2';
    const int qspan = wide ? 128 : 64;
    dim3 kgrid((unsigned)(B * h * ((S + qspan - 1) / qspan)));
#define ATTK(QPW)                                                             \
  ATT_LAUNCH_HM(hm, (attn_fwd_krows_kernel<HM, QPW>), kgrid, KR_LDS_BYTES, s, \
                (const ushort_t*)qkv, (const ushort_t*)mask, (ushort_t*)out,  \
                (float*)m, (float*)lsum, (int)B, (int)S, (int)h, scale, keep, \
                salt, (const unsigned long long*)state)
    if (wide) ATTK(2); else ATTK(1);
#undef ATTK
    LAUNCH_CHECK();
    return 0;
  }
#define ATT(SML, PM, TRV)                                                     \
  ATT_LAUNCH_HM(hm, (attn_fwd_kernel<HM, SML, PM, TRV>), grid, lds_bytes, s,  \
                (const ushort_t*)qkv, (const ushort_t*)mask, (ushort_t*)out,  \
                (float*)m, (float*)lsum, (ushort_t*)p, (ushort_t*)pd, (int)B, \
                (int)S, (int)h, scale, keep, salt,                            \
                (const unsigned long long*)state)
  if (probs_mode) { if (trv) ATT(false, true, true); else ATT(false, true, false); }
  else            { if (trv) ATT(true, false, true); else ATT(true, false, false); }
#undef ATT
  LAUNCH_CHECK();
  return 0;
}

SKY_EXPORT int sky_attn_fwd(uint64_t stream, uint64_t qkv, uint64_t mask,
                            uint64_t out, uint64_t m, uint64_t lsum,
                            int64_t B, int64_t S, int64_t h, int64_t d,
                            float scale, float keep, uint64_t salt,
                            uint64_t state) {
  return attn_launch(stream, qkv, mask, out, m, lsum, 0, 0, B, S, h, d,
                     scale, keep, salt, state, false);
}

SKY_EXPORT int sky_attn_probs(uint64_t stream, uint64_t qkv, uint64_t mask,
                              uint64_t m, uint64_t lsum, uint64_t p,
                              uint64_t pd, int64_t B, int64_t S, int64_t h,
                              int64_t d, float scale, float keep,
                              uint64_t salt, uint64_t state) {
  return attn_launch(stream, qkv, mask, 0, m, lsum, p, pd, B, S, h, d, scale,
                     keep, salt, state, true);
}
