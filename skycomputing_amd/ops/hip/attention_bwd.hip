// ============================================================================
// Fully-fused attention backward (two kernels).
//
// B1, per (b,h) and 64-query block: recompute scores -> P (saved m/l) +
//   dropout mask; compute
//   dPd = dO V^T (MFMA, A = dO straight from global), dP, the softmax
//   row-dot, dS = scale*P*(dP - rowdot); write dS row-major to per-wave LDS
//   and dS^T / Pd^T TRANSPOSED to global scratch; compute
//   dQ = dS K (A = dS from LDS, B = K^T read transposed from the K image)
//   -> dqkv[:,:,0].
// B2, per (b,h): dV = Pd^T dO and dK = dS^T Q, reading the transposed
//   scratch directly as MFMA A-fragments (contiguous q per lane) and
//   staging Q^T / dO^T in LDS -> dqkv[:,:,1:3].
//
// Replaces: sky_attn_probs + 4 hipBLASLt bmms + softmax-bwd + dropout-bwd
// + permute copies + the dqkv pack (FusedAttentionFn.backward fast path).
//
// B1 + B2 run with SKY_ATTN_KROWS=0 and for S = 1; the default pair is
// attn_bwd_dq_krows_kernel + attn_bwd_dkv_krows_kernel further down.
// ============================================================================

#include "attn_common.h"

// B1 is split over q: (S+63)/64 blocks per (b,h), each covering 64 query
// rows (one 16-row tile per wave, no qi loop). One block per (b,h) needs
// 80 KB LDS and a 32-row register footprint, which pins it at 2 blocks/CU
// and 2 waves/SIMD, latency-bound; with a 16-row per-wave dS buffer the
// block fits 48 KB LDS -> 3 blocks/CU at 3+ waves/SIMD and 2x the
// workgroups (bwd pair 60.8 -> 49.2 us, profiles/r01_notes.md).
//
// DBIAS (sky_attn_bwd_dbias): the block also writes the column sums of its
// stored dQ tile, 64 floats, to columns hh*64.. of slab b*QB + qb of the
// fp32 scratch dbscr [B*QB][3*h*64]; with attn_bwd2_kernel's dK/dV sums
// every (slab, column) is written exactly once, so the scratch needs no
// memset and the slab reduction (colsum_final) is deterministic.
template <bool HAS_MASK, bool DBIAS>
__global__ __launch_bounds__(256, 3) void attn_bwd1s_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ dout,
    const ushort_t* __restrict__ mask, const float* __restrict__ m_io,
    const float* __restrict__ l_io, ushort_t* __restrict__ pdT,
    ushort_t* __restrict__ dsT, ushort_t* __restrict__ dqkv, int B, int S,
    int h, float scale, float keep, uint64_t salt,
    const unsigned long long* __restrict__ state, float* __restrict__ dbscr) {
  // LDS: V [128][64] sw7 @0 (16K), K [128][64] sw7 @16K, per-wave dS
  // [16][128] sw15 @32K + w*4K. Total 48K. DBIAS reuses the first 1 KB of
  // the V image, dead once phase A is over, for the per-wave column sums.
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int l = tid & 63;
  const int w = tid >> 6;
  const int lm = l & 15;
  const int lg = l >> 4;
  const int QB = (S + 63) / 64;
  const int bh = blockIdx.x / QB;
  const int qb = blockIdx.x % QB;
  const int b = bh / h;
  const int hh = bh % h;
  const int ts = 3 * h * ATT_D;
  const int NT = (S + 15) / 16;
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* qbase = qkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
  const ushort_t* kbase = qbase + (size_t)h * ATT_D;
  const ushort_t* vbase = qbase + (size_t)2 * h * ATT_D;
  const ushort_t* dobase = dout + ((size_t)b * S * h + hh) * ATT_D;
  const int dots = h * ATT_D;

  const int qtok_base = qb * 64 + w * 16;
  const bool active = qtok_base < S;

  if (S < ATT_SMAX) {
    for (int u = tid; u < (48 * 1024) / 16; u += 256)
      *(ushort8_t*)lds_at(lds, u * 16) = (ushort8_t)(ushort_t)0;
    __syncthreads();
  }
  // stage V [tok][64] sw7 @0 and K [tok][64] sw7 @16K
  for (int u = tid; u < S * 8; u += 256) {
    const int tok = u >> 3;
    const int c16 = u & 7;
    *(ushort8_t*)lds_at(lds, swz(0 + tok * 128 + c16 * 16, tok, 7)) =
        *(const ushort8_t*)(vbase + (size_t)tok * ts + c16 * 8);
    *(ushort8_t*)lds_at(lds, swz(16384 + tok * 128 + c16 * 16, tok, 7)) =
        *(const ushort8_t*)(kbase + (size_t)tok * ts + c16 * 8);
  }
  // preload this wave's Q / dO fragments + mask column values
  float mval[8];
  att_mask_cols<HAS_MASK>(mval, mask, b, S, lm);
  int qtok = qtok_base + lm;
  if (qtok >= S) qtok = S - 1;
  bf16x8 aq[2], ado[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    aq[ks] = *(const bf16x8*)(qbase + (size_t)qtok * ts + ks * 32 + lg * 8);
    ado[ks] = *(const bf16x8*)(dobase + (size_t)qtok * dots + ks * 32 + lg * 8);
  }
  __syncthreads();

  // phase A: scores + dPd
  f32x4 sacc[8], dacc[8];
  att_zero(sacc);
  att_zero(dacc);
  if (active) {
    att_score_tile(sacc, aq, lds, 16384, NT, lm, lg);  // Q K^T
    att_score_tile(dacc, ado, lds, 0, NT, lm, lg);     // dO V^T
  }

  if (active) {
    // P, dP, rowdot, dS. Register budget: p/pd/dp are NOT kept in arrays
    // (3x32 VGPRs would spill); the store loop recomputes them from the
    // still-live sacc/dacc and the cached dropout hashes.
    float mrow[4], lrow[4], dot[4];
    uint64_t zs[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = qtok_base + lg * 4 + r;
      const int rr = row < S ? row : S - 1;
      mrow[r] = m_io[(size_t)bh * S + rr];
      lrow[r] = 1.f / l_io[(size_t)bh * S + rr];
      dot[r] = 0.f;
      zs[r][0] = zs[r][1] = 0;
      if (keep < 1.f) att_drop_hash(zs[r], seed, bh, S, row, lm);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = qtok_base + lg * 4 + r;
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        if (kt >= NT) continue;
        const int col = kt * 16 + lm;
        const float p = att_prob(sacc[kt][r], scale, mval[kt], mrow[r],
                                 lrow[r], row < S && col < S);
        float dp = dacc[kt][r];
        if (keep < 1.f) dp = att_drop_keep(zs[r], kt, keep16) ? dp * inv_keep : 0.f;
        dot[r] += dp * p;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dot[r] = row16_sum(dot[r]);
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      if (kt >= NT) continue;
      const int col = kt * 16 + lm;
      ushort4_t ds4, pd4;
      float dsf[4], pdf[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = qtok_base + lg * 4 + r;
        const float p = att_prob(sacc[kt][r], scale, mval[kt], mrow[r],
                                 lrow[r], row < S && col < S);
        float pd = p, dp = dacc[kt][r];
        if (keep < 1.f) {
          const bool kbit = att_drop_keep(zs[r], kt, keep16);
          pd = kbit ? p * inv_keep : 0.f;
          dp = kbit ? dp * inv_keep : 0.f;
        }
        const float ds = scale * p * (dp - dot[r]);
        dsf[r] = ds;
        pdf[r] = pd;
      }
      ds4 = f32x4_to_bf16x4(dsf[0], dsf[1], dsf[2], dsf[3]);
      pd4 = f32x4_to_bf16x4(pdf[0], pdf[1], pdf[2], pdf[3]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = lg * 4 + r;
        *(ushort_t*)lds_at(lds, swz(32768 + w * 4096 + rl * 256 + col * 2, rl, 15)) =
            ds4[r];
      }
      if (col < S) {
        const size_t o = ((size_t)bh * S + col) * S + qtok_base + lg * 4;
        if (qtok_base + lg * 4 + 3 < S) {
          *(ushort4_t*)(dsT + o) = ds4;
          *(ushort4_t*)(pdT + o) = pd4;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (qtok_base + lg * 4 + r < S) {
              dsT[o + r] = ds4[r];
              pdT[o + r] = pd4[r];
            }
        }
      }
    }
  }
  __syncthreads();  // dS tiles complete before the dQ MFMAs read them

  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  if (active) {
    // dQ = dS K : A = this wave's dS rows (LDS), B = K^T via tr16
    f32x4 qacc[4];
    att_zero(qacc);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (ks * 32 >= S) break;
      bf16x8 asr = *(const bf16x8*)lds_at(
          lds, swz(32768 + w * 4096 + lm * 256 + (ks * 32 + lg * 8) * 2, lm, 15));
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        bf16x8 bkt = abf_tr_rows64(lds, 16384, ks * 32 + lg * 8, ct * 4, lm);
        qacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(asr, bkt, qacc[ct], 0, 0, 0);
      }
    }
    ushort_t* dq = dqkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
    att_store_rows16(dq, ts, qacc, qtok_base, S, lm, lg);
    if constexpr (DBIAS) att_colsum_rows16(cs, qacc, qtok_base, S, lg);
  }
  if constexpr (DBIAS) {
    // every wave has passed the barrier above, so nobody reads V any more;
    // inactive waves contribute their zeros and must reach the barrier too
    float* wsum = (float*)lds_at(lds, 0);  // [4 waves][64 cols]
    att_colsum_wave(cs);
    if (lg == 0) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) wsum[w * 64 + ct * 16 + lm] = cs[ct];
    }
    __syncthreads();
    if (tid < 64)
      dbscr[((size_t)b * QB + qb) * ts + (size_t)hh * ATT_D + tid] =
          (wsum[tid] + wsum[64 + tid]) + (wsum[128 + tid] + wsum[192 + tid]);
  }
}

// DBIAS: the block writes the column sums of its stored dK and dV tiles to
// slab b*QB of dbscr (see attn_bwd1s_kernel) and zeros to the same columns
// of the batch's other QB-1 slabs. Launched with 2 KB more LDS for the
// per-wave sums [4 waves][dK 64 | dV 64] @32K.
template <bool DBIAS>
__global__ __launch_bounds__(256) void attn_bwd2_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ dout,
    const ushort_t* __restrict__ pdT, const ushort_t* __restrict__ dsT,
    ushort_t* __restrict__ dqkv, int B, int S, int h,
    float* __restrict__ dbscr) {
  // LDS: Qt [64][128] sw15 @0 (16K), dOt [64][128] sw15 @16K. Total 32K
  // (+ 2K of column sums @32K with DBIAS).
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int l = tid & 63;
  const int w = tid >> 6;
  const int lm = l & 15;
  const int lg = l >> 4;
  const int bh = blockIdx.x;
  const int b = bh / h;
  const int hh = bh % h;
  const int ts = 3 * h * ATT_D;
  const int dots = h * ATT_D;

  const ushort_t* qbase = qkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
  const ushort_t* dobase = dout + ((size_t)b * S * h + hh) * ATT_D;

  // Q and dO staged DIRECT [tok][64] sw7 via glds; the dV/dK B-fragments
  // read them transposed with ds_read_b64_tr_b16 (v2 — replaces the
  // register-scatter Qt/dOt build and its residual bank conflicts).
  // A-side zeros (pdT/dsT rows beyond S) null any garbage tail rows.
  att_glds_rows(qbase, ts, 0, S, false, S, lds, 0, tid);
  att_glds_rows(dobase, dots, 0, S, false, S, lds, 16384, tid);
  // rows >= S must be ZERO: the pdT/dsT A-fragment reads of a partial
  // 32-q block run past row S into the next k-row's data (row stride S),
  // and only a zero B side nulls that contribution.
  for (int u = S * 8 + tid; u < 128 * 8; u += 256) {
    *(ushort8_t*)lds_at(lds, 0 + u * 16) = (ushort8_t)(ushort_t)0;
    *(ushort8_t*)lds_at(lds, 16384 + u * 16) = (ushort8_t)(ushort_t)0;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int kt0 = 2 * w;  // this wave's two 16-row k tiles
  float ck[4] = {0.f, 0.f, 0.f, 0.f}, cv[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ki = 0; ki < 2; ++ki) {
    const int ktok_base = (kt0 + ki) * 16;
    if (ktok_base >= S) break;
    int ktok = ktok_base + lm;
    if (ktok >= S) ktok = S - 1;
    f32x4 vacc[4], kacc[4];
    att_zero(vacc);
    att_zero(kacc);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (ks * 32 >= S) break;
      // A fragments from the transposed global scratch (contiguous q)
      const size_t abase = ((size_t)bh * S + ktok) * S + ks * 32 + lg * 8;
      bf16x8 apd = *(const bf16x8*)(pdT + abase);
      bf16x8 ads = *(const bf16x8*)(dsT + abase);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        bf16x8 bdo = abf_tr_rows64(lds, 16384, ks * 32 + lg * 8, ct * 4, lm);
        vacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(apd, bdo, vacc[ct], 0, 0, 0);
        bf16x8 bq = abf_tr_rows64(lds, 0, ks * 32 + lg * 8, ct * 4, lm);
        kacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ads, bq, kacc[ct], 0, 0, 0);
      }
    }
    ushort_t* dk = dqkv + (size_t)b * S * ts + (size_t)(h + hh) * ATT_D;
    ushort_t* dv = dqkv + (size_t)b * S * ts + (size_t)(2 * h + hh) * ATT_D;
    att_store_rows16x2(dk, dv, ts, kacc, vacc, ktok_base, S, lm, lg);
    if constexpr (DBIAS) {
      att_colsum_rows16(ck, kacc, ktok_base, S, lg);
      att_colsum_rows16(cv, vacc, ktok_base, S, lg);
    }
  }
  if constexpr (DBIAS) {
    float* wsum = (float*)lds_at(lds, 32768);
    att_colsum_wave(ck);
    att_colsum_wave(cv);
    if (lg == 0) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        wsum[w * 128 + ct * 16 + lm] = ck[ct];
        wsum[w * 128 + 64 + ct * 16 + lm] = cv[ct];
      }
    }
    __syncthreads();
    if (tid < 128) {
      const int QB = (S + 63) / 64;
      // tid < 64: dK column tid; otherwise dV column tid - 64
      const size_t col = (size_t)((tid < 64 ? h : 2 * h) + hh) * ATT_D + (tid & 63);
      float* dst = dbscr + (size_t)b * QB * ts + col;
      dst[0] = (wsum[tid] + wsum[128 + tid]) + (wsum[256 + tid] + wsum[384 + tid]);
      for (int q = 1; q < QB; ++q) dst[(size_t)q * ts] = 0.f;
    }
  }
}

// ---------------------------------------------------------------------------
// Fully-fused attention backward (S <= 128): ONE kernel per (b,h) computes
// dQ, dK, dV with P and dS living ONLY in LDS — the bwd1s/bwd2 pair's
// transposed pdT/dsT scratch (2 x S x S bf16 per (b,h), written scattered
// and re-read next kernel) never touches HBM, and Q/dO are staged once
// instead of twice. Transposed operand fragments (Kt for dQ; pd^T/dS^T,
// Q^T, dO^T for dK/dV) are read with ds_read_b64_tr_b16 (lane mapping
// derived on HW, tools/tr16_probe.hip) straight from row-major images.
//
// LDS (80 KB -> 2 WGs/CU): K[128][64]sw7 @0, Q @16K, dO @32K (all glds-
// staged), dS[64 q][128 k]sw15 @48K, pd @64K (per-pass tiles; q rows are
// processed in two 64-row passes, dK/dV accumulate in registers across
// passes; each wave owns one 16-row q tile per pass and k-tiles 2w,2w+1).
#define ABF_K 0
#define ABF_Q (16 * 1024)
#define ABF_DO (32 * 1024)
#define ABF_DS (48 * 1024)
#define ABF_PD (64 * 1024)
#define ABF_LDS (80 * 1024)

template <bool HAS_MASK>
__global__ __launch_bounds__(256, 1) void attn_bwd_fused_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ dout,
    const ushort_t* __restrict__ mask, const float* __restrict__ m_io,
    const float* __restrict__ l_io, ushort_t* __restrict__ dqkv, int B,
    int S, int h, float scale, float keep, uint64_t salt,
    const unsigned long long* __restrict__ state) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int l = tid & 63;
  const int w = tid >> 6;
  const int lm = l & 15;
  const int lg = l >> 4;
  const int bh = blockIdx.x;
  const int b = bh / h;
  const int hh = bh % h;
  const int ts = 3 * h * ATT_D;
  const int dots = h * ATT_D;
  const int NT = (S + 15) / 16;
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* qbase = qkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
  const ushort_t* kbase = qbase + (size_t)h * ATT_D;
  const ushort_t* vbase = qbase + (size_t)2 * h * ATT_D;
  const ushort_t* dobase = dout + ((size_t)b * S * h + hh) * ATT_D;

  // ---- stage K, Q, dO row images via glds (source-side swizzle) ----
  att_glds_rows(kbase, ts, 0, 128, true, S, lds, ABF_K, tid);
  att_glds_rows(qbase, ts, 0, 128, true, S, lds, ABF_Q, tid);
  att_glds_rows(dobase, dots, 0, 128, true, S, lds, ABF_DO, tid);
  // mask column values (pass-independent)
  float mval[8];
  att_mask_cols<HAS_MASK>(mval, mask, b, S, lm);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // persistent dK/dV accumulators: wave w owns k-tiles 2w and 2w+1
  f32x4 kacc[2][4], vacc[2][4];
#pragma unroll
  for (int ki = 0; ki < 2; ++ki) {
    att_zero(kacc[ki]);
    att_zero(vacc[ki]);
  }

  const int npass = (S + 63) / 64;
  for (int pass = 0; pass < npass; ++pass) {
    const int qtok_base = pass * 64 + w * 16;
    const bool active = qtok_base < S;
    // ---- phase A: scores (K from LDS) + dPd (V fragments from global);
    // A fragments (this wave's q rows of Q / dO) read per-use from the
    // staged LDS row images — no held registers ----
    const int qrow = qtok_base + lm;
    const int qrl = qrow < S ? qrow : S - 1;
    f32x4 sacc[8], dacc[8];
    att_zero(sacc);
    att_zero(dacc);
    if (active) {
      bf16x8 aq[2], ado[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        aq[ks] = *(const bf16x8*)lds_at(
            lds, swz(ABF_Q + qrl * 128 + (ks * 32 + lg * 8) * 2, qrl, 7));
        ado[ks] = *(const bf16x8*)lds_at(
            lds, swz(ABF_DO + qrl * 128 + (ks * 32 + lg * 8) * 2, qrl, 7));
      }
      att_score_tile(sacc, aq, lds, ABF_K, NT, lm, lg);
      // dPd stays local: V is not staged, its B fragments come from global
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        if (kt >= NT) continue;
        const int ktok = kt * 16 + lm;
        const int vtok = ktok < S ? ktok : S - 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          bf16x8 bv = *(const bf16x8*)(vbase + (size_t)vtok * ts + ks * 32 + lg * 8);
          dacc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ado[ks], bv, dacc[kt], 0, 0, 0);
        }
      }
    }
    // ---- P, dP, rowdot, dS/pd tiles (EVERY wave writes its 16 rows) ----
    float mrow[4], lrow[4], dot[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = qtok_base + lg * 4 + r;
      const int rr = row < S ? row : S - 1;
      mrow[r] = m_io[(size_t)bh * S + rr];
      lrow[r] = 1.f / l_io[(size_t)bh * S + rr];
      dot[r] = 0.f;
    }
    // dot pass: p and the dropout-masked dp are PARKED in the pd/dS tile
    // slots (bf16) so sacc/dacc die here — the register peak would
    // otherwise spill (sacc+dacc 64 + kacc/vacc 64 persistent).
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = qtok_base + lg * 4 + r;
      const int rl = lg * 4 + r;
      uint64_t z[2] = {0, 0};
      if (keep < 1.f) att_drop_hash(z, seed, bh, S, row, lm);
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        const int col = kt * 16 + lm;
        const float p = att_prob(sacc[kt][r], scale, mval[kt], mrow[r],
                                 lrow[r], kt < NT && row < S && col < S);
        float dp = dacc[kt][r];
        if (keep < 1.f) dp = att_drop_keep(z, kt, keep16) ? dp * inv_keep : 0.f;
        dot[r] += dp * p;
        *(ushort_t*)lds_at(lds, swz(ABF_PD + (w * 16 + rl) * 256 + col * 2, rl, 15)) =
            f32_to_bf16(p);
        *(ushort_t*)lds_at(lds, swz(ABF_DS + (w * 16 + rl) * 256 + col * 2, rl, 15)) =
            f32_to_bf16(dp);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dot[r] = row16_sum(dot[r]);
    // finish pass: read the parked p/dp back, apply dropout to p -> pd,
    // ds = scale * p * (dp - dot); overwrite the same slots in place.
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = qtok_base + lg * 4 + r;
      const int rl = lg * 4 + r;
      uint64_t z[2] = {0, 0};
      if (keep < 1.f) att_drop_hash(z, seed, bh, S, row, lm);
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        const int col = kt * 16 + lm;
        const float p = bf16_to_f32(*(const ushort_t*)lds_at(
            lds, swz(ABF_PD + (w * 16 + rl) * 256 + col * 2, rl, 15)));
        const float dp = bf16_to_f32(*(const ushort_t*)lds_at(
            lds, swz(ABF_DS + (w * 16 + rl) * 256 + col * 2, rl, 15)));
        float pd = p;
        if (keep < 1.f) pd = att_drop_keep(z, kt, keep16) ? p * inv_keep : 0.f;
        const float ds = scale * p * (dp - dot[r]);
        *(ushort_t*)lds_at(lds, swz(ABF_DS + (w * 16 + rl) * 256 + col * 2, rl, 15)) =
            f32_to_bf16(ds);
        *(ushort_t*)lds_at(lds, swz(ABF_PD + (w * 16 + rl) * 256 + col * 2, rl, 15)) =
            f32_to_bf16(pd);
      }
    }
    __syncthreads();  // tiles complete for cross-wave reads

    // ---- dQ = dS K (A = own tile rows, direct b128; B = Kt via tr16) ----
    if (active) {
      f32x4 qacc[4];
      att_zero(qacc);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks * 32 >= S) break;
        bf16x8 asr = *(const bf16x8*)lds_at(
            lds, swz(ABF_DS + (w * 16 + lm) * 256 + (ks * 32 + lg * 8) * 2, lm, 15));
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          bf16x8 bkt = abf_tr_rows64(lds, ABF_K, ks * 32 + lg * 8, ct * 4, lm);
          qacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(asr, bkt, qacc[ct], 0, 0, 0);
        }
      }
      ushort_t* dq = dqkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
      att_store_rows16(dq, ts, qacc, qtok_base, S, lm, lg);
    }

    // ---- dK += dS^T Q, dV += pd^T dO over this pass's 64 q rows ----
    // wave's k-tiles: 2w, 2w+1; A frags via tr16 on the tiles, B frags
    // via tr16 on the Q/dO row images (k-dim = global q row).
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const int q0t = ks2 * 32 + lg * 8;             // tile-local q base
      bf16x8 apd[2], ads[2];
#pragma unroll
      for (int ki = 0; ki < 2; ++ki) {
        const int kt = 2 * w + ki;
        apd[ki] = abf_tr_rows128(lds, ABF_PD, q0t, kt * 4, lm);
        ads[ki] = abf_tr_rows128(lds, ABF_DS, q0t, kt * 4, lm);
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        bf16x8 bq = abf_tr_rows64(lds, ABF_Q, pass * 64 + q0t, ct * 4, lm);
        bf16x8 bdo = abf_tr_rows64(lds, ABF_DO, pass * 64 + q0t, ct * 4, lm);
#pragma unroll
        for (int ki = 0; ki < 2; ++ki) {
          vacc[ki][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(apd[ki], bdo, vacc[ki][ct], 0, 0, 0);
          kacc[ki][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ads[ki], bq, kacc[ki][ct], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // tiles free for the next pass
  }

  // ---- write dK/dV (wave's 32 k rows) ----
  ushort_t* dk = dqkv + (size_t)b * S * ts + (size_t)(h + hh) * ATT_D;
  ushort_t* dv = dqkv + (size_t)b * S * ts + (size_t)(2 * h + hh) * ATT_D;
#pragma unroll
  for (int ki = 0; ki < 2; ++ki)
    att_store_rows16x2(dk, dv, ts, kacc[ki], vacc[ki], (2 * w + ki) * 16, S,
                       lm, lg);
}

SKY_EXPORT int sky_attn_bwd_fused(uint64_t stream, uint64_t qkv,
                                  uint64_t dout, uint64_t mask, uint64_t m,
                                  uint64_t lsum, uint64_t dqkv, int64_t B,
                                  int64_t S, int64_t h, int64_t d,
                                  float scale, float keep, uint64_t salt,
                                  uint64_t state) {
  if (d != ATT_D || S > ATT_SMAX) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)(B * h));
  ATT_LAUNCH_HM(mask != 0, (attn_bwd_fused_kernel<HM>), grid, ABF_LDS, s,
                (const ushort_t*)qkv, (const ushort_t*)dout,
                (const ushort_t*)mask, (const float*)m, (const float*)lsum,
                (ushort_t*)dqkv, (int)B, (int)S, (int)h, scale, keep, salt,
                (const unsigned long long*)state);
  LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// The default backward pair (SKY_ATTN_KROWS=0 restores bwd1s + bwd2): P and
// dS stay in the registers their MFMA left them in. Each product is
// computed in the orientation the next one wants (att_pack_dpair), so no
// dS tile goes through LDS and no dS^T / Pd^T goes through global scratch;
// the second kernel recomputes them from Q, K, V, dO and the row statistics.
//
// dQ, per (b, h, 64-query block), keys on the MFMA rows: S^T = K Q^T and
// dPd^T = V dO^T, a lane owns ONE query (m, 1/l and the row dot are lane
// scalars), P overwrites the scores (one __expf per element), dS^T
// overwrites them again and is the B operand of dQ^T = K^T dS^T. Also
// writes dot[bh*S + q] (fp32) for the second kernel, and with DBIAS the
// block's 64 dQ column sums to slab b*QB + qb like attn_bwd1s_kernel.
// LDS: K [128][64] sw7 @0, V @16K, key mask fp32 @32K, DBIAS sums @32.5K.
#define KRB_K_OFF KR_IMG0_OFF
#define KRB_V_OFF KR_IMG1_OFF
#define KRB_MASK_OFF KR_AUX_OFF
#define KRB_SUM_OFF (KR_AUX_OFF + 512)
#define KRB_DQ_LDS (KR_AUX_OFF + 512 + 1024)

template <bool HAS_MASK, bool DBIAS>
__global__ __launch_bounds__(256, 4) void attn_bwd_dq_krows_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ dout,
    const ushort_t* __restrict__ mask, const float* __restrict__ m_io,
    const float* __restrict__ l_io, float* __restrict__ dot_out,
    ushort_t* __restrict__ dqkv, int B, int S, int h, float scale, float keep,
    uint64_t salt, const unsigned long long* __restrict__ state,
    float* __restrict__ dbscr) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int l = tid & 63;
  const int w = tid >> 6;
  const int lm = l & 15;
  const int lg = l >> 4;
  const int QB = (S + 63) / 64;
  const int bh = blockIdx.x / QB;
  const int qb = blockIdx.x % QB;
  const int b = bh / h;
  const int hh = bh % h;
  const int ts = 3 * h * ATT_D;
  const int dots = h * ATT_D;
  const int NT = (S + 15) / 16;
  const int NP = (S + 31) / 32;
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* qbase = qkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
  const ushort_t* kbase = qbase + (size_t)h * ATT_D;
  const ushort_t* vbase = qbase + (size_t)2 * h * ATT_D;
  const ushort_t* dobase = dout + ((size_t)b * S * h + hh) * ATT_D;
  float* mk = (float*)lds_at(lds, KRB_MASK_OFF);

  const int qtok_base = qb * 64 + w * 16;
  const bool active = qtok_base < S;
  const int q = qtok_base + lm;  // this lane's query
  const int qc = q < S ? q : S - 1;

  att_glds_rows(kbase, ts, 0, NP * 32, true, S, lds, KRB_K_OFF, tid);
  att_glds_rows(vbase, ts, 0, NP * 32, true, S, lds, KRB_V_OFF, tid);
  att_mask_keys_lds(mk, HAS_MASK, mask, b, S, tid);
  bf16x8 bq[2], bdo[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bq[ks] = *(const bf16x8*)(qbase + (size_t)qc * ts + ks * 32 + lg * 8);
    bdo[ks] = *(const bf16x8*)(dobase + (size_t)qc * dots + ks * 32 + lg * 8);
  }
  const float mrow = m_io[(size_t)bh * S + qc];
  const float lrow = 1.f / l_io[(size_t)bh * S + qc];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  float cs = 0.f;
  if (active) {
    f32x4 sacc[8], dacc[8];
    att_zero(sacc);
    att_zero(dacc);
    att_score_tile_t(sacc, bq, lds, KRB_K_OFF, NT, lm, lg);   // K Q^T
    att_score_tile_t(dacc, bdo, lds, KRB_V_OFF, NT, lm, lg);  // V dO^T
    uint64_t z[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    if (keep < 1.f) att_drop_hash_krows(z, seed, bh, S, q, lg);
    // P -> sacc, dropout-masked dP -> dacc, row dot
    float dot = 0.f;
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
      if (mt >= NT) continue;
      const f32x4 mv = att_mask_keys4(mk, mt, lg);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = mt * 16 + lg * 4 + r;
        const float p = att_prob(sacc[mt][r], scale, mv[r], mrow, lrow,
                                 q < S && key < S);
        float dp = dacc[mt][r];
        if (keep < 1.f)
          dp = att_drop_keep(z[r], mt, keep16) ? dp * inv_keep : 0.f;
        dot += dp * p;
        sacc[mt][r] = p;
        dacc[mt][r] = dp;
      }
    }
    dot += __shfl_xor(dot, 16, 64);
    dot += __shfl_xor(dot, 32, 64);
    if (lg == 0 && q < S) dot_out[(size_t)bh * S + q] = dot;
    // dS^T over P, then dQ^T = K^T dS^T
    f32x4 qacc[4];
    att_zero(qacc);
#pragma unroll
    for (int kp = 0; kp < 4; ++kp) {
      if (kp >= NP) continue;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sacc[2 * kp + t][r] =
              scale * sacc[2 * kp + t][r] * (dacc[2 * kp + t][r] - dot);
      }
      const bf16x8 bds = att_pack_dpair(sacc[2 * kp], sacc[2 * kp + 1]);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const bf16x8 ak = abf_tr_rows64_2(lds, KRB_K_OFF, kp * 32 + lg * 4,
                                          kp * 32 + 16 + lg * 4, ct * 4, lm);
        qacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak, bds, qacc[ct], 0, 0, 0);
      }
    }
    ushort_t* dq = dqkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
    att_store_cols16(dq, ts, qacc, qtok_base, S, lm, lg);
    if constexpr (DBIAS) cs = att_colsum_cols16(qacc, qtok_base, S, lm);
  }
  if constexpr (DBIAS) {
    // inactive waves contribute their zeros and must reach the barrier too
    float* wsum = (float*)lds_at(lds, KRB_SUM_OFF);  // [4 waves][64 cols]
    wsum[w * 64 + att_colsum_cols16_col(lm, lg)] = cs;
    __syncthreads();
    if (tid < 64)
      dbscr[((size_t)b * QB + qb) * ts + (size_t)hh * ATT_D + tid] =
          (wsum[tid] + wsum[64 + tid]) + (wsum[128 + tid] + wsum[192 + tid]);
  }
}

// dK/dV, per (b, h, 64-key block), queries on the MFMA rows, launched after
// the dQ kernel: a wave owns 16 keys (K and V fragments from global) and
// walks the queries in pairs of 16-row tiles: S = Q K^T and dPd = dO V^T
// from the Q / dO images in LDS, P, Pd and dS from the saved m, 1/l and the
// dQ kernel's dot, and the packed pair is the B operand of
// dV^T += dO^T Pd and dK^T += Q^T dS. With DBIAS the block writes its dK
// and dV column sums to slab b*QB + kb: one key block per query block, so
// every (slab, column) is written exactly once and nothing is zero-filled.
// LDS: Q [128][64] sw7 @0, dO @16K, m | 1/l | dot fp32 [128] each @32K,
// keep bits (att_drop_bits_lds) @33.5K, DBIAS sums [4][dK 64 | dV 64] @35.5K.
#define KRB_Q_OFF KR_IMG0_OFF
#define KRB_DO_OFF KR_IMG1_OFF
#define KRB_STAT_OFF KR_AUX_OFF
#define KRB_BITS_OFF (KR_AUX_OFF + 1536)
#define KRB_SUM2_OFF (KR_AUX_OFF + 1536 + 2048)
#define KRB_DKV_LDS (KR_AUX_OFF + 1536 + 2048 + 2048)

template <bool HAS_MASK, bool DBIAS>
__global__ __launch_bounds__(256, 4) void attn_bwd_dkv_krows_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ dout,
    const ushort_t* __restrict__ mask, const float* __restrict__ m_io,
    const float* __restrict__ l_io, const float* __restrict__ dot_in,
    ushort_t* __restrict__ dqkv, int B, int S, int h, float scale, float keep,
    uint64_t salt, const unsigned long long* __restrict__ state,
    float* __restrict__ dbscr) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int l = tid & 63;
  const int w = tid >> 6;
  const int lm = l & 15;
  const int lg = l >> 4;
  const int QB = (S + 63) / 64;
  const int bh = blockIdx.x / QB;
  const int kb = blockIdx.x % QB;
  const int b = bh / h;
  const int hh = bh % h;
  const int ts = 3 * h * ATT_D;
  const int dots = h * ATT_D;
  const int NT = (S + 15) / 16;
  const int NP = (S + 31) / 32;
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* qbase = qkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
  const ushort_t* kbase = qbase + (size_t)h * ATT_D;
  const ushort_t* vbase = qbase + (size_t)2 * h * ATT_D;
  const ushort_t* dobase = dout + ((size_t)b * S * h + hh) * ATT_D;
  float* st = (float*)lds_at(lds, KRB_STAT_OFF);
  unsigned char* bits = (unsigned char*)lds_at(lds, KRB_BITS_OFF);

  const int ktok_base = kb * 64 + w * 16;
  const bool active = ktok_base < S;
  const int key = ktok_base + lm;  // this lane's key
  const int kc = key < S ? key : S - 1;

  att_glds_rows(qbase, ts, 0, NP * 32, true, S, lds, KRB_Q_OFF, tid);
  att_glds_rows(dobase, dots, 0, NP * 32, true, S, lds, KRB_DO_OFF, tid);
  // rows >= S: 1/l = 0 and a false valid flag null P, dot = 0 keeps dS finite
  if (tid < ATT_SMAX) {
    const bool live = tid < S;
    st[tid] = live ? m_io[(size_t)bh * S + tid] : 0.f;
    st[128 + tid] = live ? 1.f / l_io[(size_t)bh * S + tid] : 0.f;
    st[256 + tid] = live ? dot_in[(size_t)bh * S + tid] : 0.f;
  }
  if (keep < 1.f)
    att_drop_bits_lds(bits, seed, bh, S, kb, NP * 32, keep16, tid);
  bf16x8 bk[2], bv[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bk[ks] = *(const bf16x8*)(kbase + (size_t)kc * ts + ks * 32 + lg * 8);
    bv[ks] = *(const bf16x8*)(vbase + (size_t)kc * ts + ks * 32 + lg * 8);
  }
  float mv = 0.f;
  if (HAS_MASK && key < S) mv = bf16_to_f32(mask[(size_t)b * S + key]);
  if (key >= S) mv = -3.0e38f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  float ck = 0.f, cv = 0.f;
  if (active) {
    f32x4 kacc[4], vacc[4];
    att_zero(kacc);
    att_zero(vacc);
#pragma unroll
    for (int qp = 0; qp < 4; ++qp) {
      if (qp >= NP) continue;
      f32x4 pd[2], ds[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int qt = 2 * qp + t;
        pd[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        ds[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (qt >= NT) continue;
        const int qrow = qt * 16 + lm;  // < NP*32: a staged (clamped) row
        f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, d4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 aq = *(const bf16x8*)lds_at(
              lds, swz(KRB_Q_OFF + qrow * 128 + (ks * 32 + lg * 8) * 2, qrow, 7));
          const bf16x8 ado = *(const bf16x8*)lds_at(
              lds, swz(KRB_DO_OFF + qrow * 128 + (ks * 32 + lg * 8) * 2, qrow, 7));
          s4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq, bk[ks], s4, 0, 0, 0);
          d4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ado, bv[ks], d4, 0, 0, 0);
        }
        const f32x4 m4 = *(const f32x4*)(st + qt * 16 + lg * 4);
        const f32x4 il4 = *(const f32x4*)(st + 128 + qt * 16 + lg * 4);
        const f32x4 dot4 = *(const f32x4*)(st + 256 + qt * 16 + lg * 4);
        unsigned kbits = 0xFFFFFFFFu;
        if (keep < 1.f)
          kbits = *(const unsigned*)(bits + ((qt * 4 + lg) * 16 + lm) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qq = qt * 16 + lg * 4 + r;
          const float p = att_prob(s4[r], scale, mv, m4[r], il4[r],
                                   qq < S && key < S);
          const bool kbit = (kbits >> (8 * r + w)) & 1u;
          float pdv = p, dp = d4[r];
          if (keep < 1.f) {
            pdv = kbit ? p * inv_keep : 0.f;
            dp = kbit ? dp * inv_keep : 0.f;
          }
          pd[t][r] = pdv;
          ds[t][r] = scale * p * (dp - dot4[r]);
        }
      }
      const bf16x8 bpd = att_pack_dpair(pd[0], pd[1]);
      const bf16x8 bds = att_pack_dpair(ds[0], ds[1]);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const bf16x8 adot = abf_tr_rows64_2(lds, KRB_DO_OFF, qp * 32 + lg * 4,
                                            qp * 32 + 16 + lg * 4, ct * 4, lm);
        vacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(adot, bpd, vacc[ct], 0, 0, 0);
        const bf16x8 aqt = abf_tr_rows64_2(lds, KRB_Q_OFF, qp * 32 + lg * 4,
                                           qp * 32 + 16 + lg * 4, ct * 4, lm);
        kacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aqt, bds, kacc[ct], 0, 0, 0);
      }
    }
    ushort_t* dk = dqkv + (size_t)b * S * ts + (size_t)(h + hh) * ATT_D;
    ushort_t* dv = dqkv + (size_t)b * S * ts + (size_t)(2 * h + hh) * ATT_D;
    att_store_cols16(dk, ts, kacc, ktok_base, S, lm, lg);
    att_store_cols16(dv, ts, vacc, ktok_base, S, lm, lg);
    if constexpr (DBIAS) {
      ck = att_colsum_cols16(kacc, ktok_base, S, lm);
      cv = att_colsum_cols16(vacc, ktok_base, S, lm);
    }
  }
  if constexpr (DBIAS) {
    float* wsum = (float*)lds_at(lds, KRB_SUM2_OFF);  // [4][dK 64 | dV 64]
    const int c = att_colsum_cols16_col(lm, lg);
    wsum[w * 128 + c] = ck;
    wsum[w * 128 + 64 + c] = cv;
    __syncthreads();
    if (tid < 128) {
      // tid < 64: dK column tid; otherwise dV column tid - 64
      const size_t col = (size_t)((tid < 64 ? h : 2 * h) + hh) * ATT_D + (tid & 63);
      dbscr[((size_t)b * QB + kb) * ts + col] =
          (wsum[tid] + wsum[128 + tid]) + (wsum[256 + tid] + wsum[384 + tid]);
    }
  }
}

// the default pair: dQ + dot, then dK/dV. dot (fp32 [B*h*S]) lives at the
// head of the pdT scratch the entry points receive (2*S*S bytes per (b,h)
// cover 4*S for S >= 2); nothing else of pdT / dsT is touched.
template <bool DBIAS>
static void launch_attn_bwd_krows(hipStream_t s, uint64_t qkv, uint64_t dout,
                                  uint64_t mask, uint64_t m, uint64_t lsum,
                                  uint64_t pdT, uint64_t dqkv, int64_t B,
                                  int64_t S, int64_t h, float scale,
                                  float keep, uint64_t salt, uint64_t state,
                                  float* dbscr) {
  dim3 grid((unsigned)(B * h * ((S + 63) / 64)));
  ATT_LAUNCH_HM(mask != 0, (attn_bwd_dq_krows_kernel<HM, DBIAS>), grid,
                KRB_DQ_LDS, s, (const ushort_t*)qkv, (const ushort_t*)dout,
                (const ushort_t*)mask, (const float*)m, (const float*)lsum,
                (float*)pdT, (ushort_t*)dqkv, (int)B, (int)S, (int)h, scale,
                keep, salt, (const unsigned long long*)state, dbscr);
  ATT_LAUNCH_HM(mask != 0, (attn_bwd_dkv_krows_kernel<HM, DBIAS>), grid,
                KRB_DKV_LDS, s, (const ushort_t*)qkv, (const ushort_t*)dout,
                (const ushort_t*)mask, (const float*)m, (const float*)lsum,
                (const float*)pdT, (ushort_t*)dqkv, (int)B, (int)S, (int)h,
                scale, keep, salt, (const unsigned long long*)state, dbscr);
}

// SKY_ATTN_KROWS=0, read at launch like SKY_ATTN_TRV, restores the
// bwd1s + bwd2 pair; S = 1 always runs it (the dot hand-off needs S >= 2).
static bool attn_bwd_use_krows(int64_t S) {
  const char* e = getenv("SKY_ATTN_KROWS");
  return S >= 2 && !(e && e[0] == '0');
}

// the bwd1s + bwd2 pair; DBIAS also fills the column-partial scratch
template <bool DBIAS>
static void launch_attn_bwd_pair(hipStream_t s, uint64_t qkv, uint64_t dout,
                                 uint64_t mask, uint64_t m, uint64_t lsum,
                                 uint64_t pdT, uint64_t dsT, uint64_t dqkv,
                                 int64_t B, int64_t S, int64_t h, float scale,
                                 float keep, uint64_t salt, uint64_t state,
                                 float* dbscr) {
  dim3 grid((unsigned)(B * h * ((S + 63) / 64)));
  ATT_LAUNCH_HM(mask != 0, (attn_bwd1s_kernel<HM, DBIAS>), grid, 48 * 1024, s,
                (const ushort_t*)qkv, (const ushort_t*)dout,
                (const ushort_t*)mask, (const float*)m, (const float*)lsum,
                (ushort_t*)pdT, (ushort_t*)dsT, (ushort_t*)dqkv, (int)B,
                (int)S, (int)h, scale, keep, salt,
                (const unsigned long long*)state, dbscr);
  hipLaunchKernelGGL(attn_bwd2_kernel<DBIAS>, dim3((unsigned)(B * h)),
                     dim3(256), (DBIAS ? 34 : 32) * 1024, s,
                     (const ushort_t*)qkv, (const ushort_t*)dout,
                     (const ushort_t*)pdT, (const ushort_t*)dsT,
                     (ushort_t*)dqkv, (int)B, (int)S, (int)h, dbscr);
}

SKY_EXPORT int sky_attn_bwd(uint64_t stream, uint64_t qkv, uint64_t dout,
                            uint64_t mask, uint64_t m, uint64_t lsum,
                            uint64_t pdT, uint64_t dsT, uint64_t dqkv,
                            int64_t B, int64_t S, int64_t h, int64_t d,
                            float scale, float keep, uint64_t salt,
                            uint64_t state) {
  if (d != ATT_D || S > ATT_SMAX) return (int)hipErrorInvalidValue;
  if (attn_bwd_use_krows(S))
    launch_attn_bwd_krows<false>((hipStream_t)stream, qkv, dout, mask, m, lsum,
                                 pdT, dqkv, B, S, h, scale, keep, salt, state,
                                 nullptr);
  else
    launch_attn_bwd_pair<false>((hipStream_t)stream, qkv, dout, mask, m, lsum,
                                pdT, dsT, dqkv, B, S, h, scale, keep, salt,
                                state, nullptr);
  LAUNCH_CHECK();
  return 0;
}

// sky_attn_bwd that also returns dbias[3*h*64] = the column sums of dqkv
// over its B*S rows, i.e. the bias gradient of the linear that produced
// qkv, taken from the kernels' registers instead of a re-read of dqkv.
// scratch: fp32 [B * ceil(S/64)][3*h*64], no memset needed; dbias_dt is
// the DT_* tag of the dbias buffer.
// job == nullptr: the slab reduction runs here; otherwise it is left
// pending in *job.
static int attn_bwd_dbias_impl(uint64_t stream, uint64_t qkv, uint64_t dout,
                               uint64_t mask, uint64_t m, uint64_t lsum,
                               uint64_t pdT, uint64_t dsT, uint64_t dqkv,
                               int64_t B, int64_t S, int64_t h, int64_t d,
                               float scale, float keep, uint64_t salt,
                               uint64_t state, uint64_t scratch,
                               uint64_t dbias, int dbias_dt,
                               SkyFinishJob* job) {
  if (d != ATT_D || S > ATT_SMAX || scratch == 0 || dbias == 0)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (attn_bwd_use_krows(S))
    launch_attn_bwd_krows<true>(s, qkv, dout, mask, m, lsum, pdT, dqkv, B, S, h,
                                scale, keep, salt, state, (float*)scratch);
  else
    launch_attn_bwd_pair<true>(s, qkv, dout, mask, m, lsum, pdT, dsT, dqkv, B,
                               S, h, scale, keep, salt, state, (float*)scratch);
  const int64_t cols = 3 * h * ATT_D, nslabs = B * ((S + 63) / 64);
  if (job)
    sky_finish_job_set(job, scratch, dbias, 0, 0, nslabs, cols, 1, dbias_dt);
  else
    sky_launch_colsum_final(s, (const float*)scratch, (void*)dbias, cols,
                            nslabs, dbias_dt);
  LAUNCH_CHECK();
  return 0;
}

SKY_EXPORT int sky_attn_bwd_dbias(uint64_t stream, uint64_t qkv, uint64_t dout,
                                  uint64_t mask, uint64_t m, uint64_t lsum,
                                  uint64_t pdT, uint64_t dsT, uint64_t dqkv,
                                  int64_t B, int64_t S, int64_t h, int64_t d,
                                  float scale, float keep, uint64_t salt,
                                  uint64_t state, uint64_t scratch,
                                  uint64_t dbias, int dbias_dt) {
  return attn_bwd_dbias_impl(stream, qkv, dout, mask, m, lsum, pdT, dsT, dqkv,
                             B, S, h, d, scale, keep, salt, state, scratch,
                             dbias, dbias_dt, nullptr);
}

// sky_attn_bwd_dbias without its final: dqkv and the column-partial scratch
// are written, dbias's slab reduction is described in *job (a host
// SkyFinishJob) for sky_colsum_finish.
SKY_EXPORT int sky_attn_bwd_dbias_parts(
    uint64_t stream, uint64_t qkv, uint64_t dout, uint64_t mask, uint64_t m,
    uint64_t lsum, uint64_t pdT, uint64_t dsT, uint64_t dqkv, int64_t B,
    int64_t S, int64_t h, int64_t d, float scale, float keep, uint64_t salt,
    uint64_t state, uint64_t scratch, uint64_t dbias, int dbias_dt,
    uint64_t job) {
  if (job == 0) return (int)hipErrorInvalidValue;
  ((SkyFinishJob*)job)->nv = 0;
  return attn_bwd_dbias_impl(stream, qkv, dout, mask, m, lsum, pdT, dsT, dqkv,
                             B, S, h, d, scale, keep, salt, state, scratch,
                             dbias, dbias_dt, (SkyFinishJob*)job);
}
