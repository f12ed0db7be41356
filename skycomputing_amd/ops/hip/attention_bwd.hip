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
  launch_attn_bwd_pair<true>(s, qkv, dout, mask, m, lsum, pdT, dsT, dqkv, B, S,
                             h, scale, keep, salt, state, (float*)scratch);
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
