// ============================================================================
// Flash-style attention forward for ARBITRARY sequence length (d = 64).
//
// Online-softmax over 128-key kv tiles: one workgroup per
// (batch, head, 128-query block); running row max m / row sum l with a
// rescale of the O accumulator at every tile (plain rescale, no defer —
// the guide's T13 hazard does not apply). The S x S matrix never exists;
// row stats are saved so the Python backward can recompute probabilities.
// Dropout uses LINEAR element indices ((bh*S+row)*S+col) so the generic
// dropout kernels regenerate the same mask in the decomposed backward.
//
// LDS reuses the S<=128 kernel's 48 KB layout per kv tile: K staged via
// global_load_lds with a source-side XOR swizzle, V^T aliased over K after
// QK^T (two barriers per tile), per-wave P tile.
// ============================================================================

#include "attn_common.h"

// Flash forward v2: one workgroup covers QPW 128-query blocks of one
// (batch, head) — K and V^T live in SEPARATE LDS regions staged ONCE per
// kv tile and reused across the q blocks (the v1 kernel aliased V over K
// and restaged both for every q block: S/128x K/V read amplification,
// 176 vs 107 us at S=512 against the decomposed path). Consecutive
// blockIdx values = same (b,h), so with the XCD-contiguous remap a head's
// K/V streams from its XCD's L2 across its q-block workgroups.
// LDS: K [128][64] @0 (16K), V^T [64][128] @16K, P per wave @32K+w*8K.
#define F2_K_OFF 0
#define F2_VT_OFF (16 * 1024)
#define F2_P_OFF (32 * 1024)
#define F2_LDS_BYTES (64 * 1024)

template <int QPW>
__global__ __launch_bounds__(256, 1) void attn_flash_fwd_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ mask,
    ushort_t* __restrict__ out, float* __restrict__ m_io,
    float* __restrict__ l_io, int B, int S, int h, float scale, float keep,
    uint64_t salt, const unsigned long long* __restrict__ state) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int l = tid & 63;
  const int w = tid >> 6;
  const int nqb = (S + 127) / 128;
  const int nchunk = (nqb + QPW - 1) / QPW;
  int bid = blockIdx.x;
  {  // XCD-contiguous remap (bijective): consecutive ids share an XCD
    const int nwg = gridDim.x;
    const int q = nwg / 8, rr = nwg % 8;
    const int xcd = bid % 8, idx = bid / 8;
    bid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx;
  }
  const int bh = bid / nchunk;
  const int qc = bid % nchunk;
  const int b = bh / h;
  const int hh = bh % h;
  const int ts = 3 * h * ATT_D;
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* qbase = qkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
  const ushort_t* kbase = qbase + (size_t)h * ATT_D;
  const ushort_t* vbase = qbase + (size_t)2 * h * ATT_D;

  const int lm = l & 15;
  const int lg = l >> 4;
  const int q0 = qc * QPW * 128;    // first query row of this chunk
  const int qt0 = 2 * w;            // wave's first q tile within a block

  // Q fragments for the wave's 2 tiles in each of the QPW blocks
  bf16x8 aq_all[QPW][2][2];
#pragma unroll
  for (int blk = 0; blk < QPW; ++blk)
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
      int qtok = q0 + blk * 128 + (qt0 + qi) * 16 + lm;
      if (qtok >= S) qtok = S - 1;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        aq_all[blk][qi][ks] =
            *(const bf16x8*)(qbase + (size_t)qtok * ts + ks * 32 + lg * 8);
    }

  float mx[QPW][2][4], sm[QPW][2][4];
  f32x4 oacc[QPW][2][4];
#pragma unroll
  for (int blk = 0; blk < QPW; ++blk)
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
      att_zero(oacc[blk][qi]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mx[blk][qi][r] = -3.0e38f;
        sm[blk][qi][r] = 0.f;
      }
    }

  const int nkv = (S + 127) / 128;
  for (int kv = 0; kv < nkv; ++kv) {
    const int k0 = kv * 128;
    const int ktiles = min(8, (S - k0 + 15) / 16);
    __syncthreads();  // previous tile's K/Vt reads complete before overwrite
    // ---- stage K tile [128][64] via glds (clamped rows masked off via
    // mval) ----
    att_glds_rows(kbase, ts, k0, 128, true, S, lds, F2_K_OFF, tid);
    // ---- stage V^T [64 d][128 tok] (register transpose) ----
    for (int u = tid; u < 128 * 8; u += 256) {
      const int tok = u >> 3;
      const int gtok = k0 + tok;
      const int c16 = u & 7;
      ushort8_t v;
      if (gtok < S)
        v = *(const ushort8_t*)(vbase + (size_t)gtok * ts + c16 * 8);
      else
        v = (ushort8_t)(ushort_t)0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c16 * 8 + j;
        *(ushort_t*)lds_at(lds, swz(F2_VT_OFF + c * 256 + tok * 2, c, 15)) = v[j];
      }
    }
    // additive mask values for this tile's columns
    float mval[8];
    att_mask_cols(mval, mask != nullptr, mask, b, S, lm, k0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

#pragma clang loop unroll(disable)
    for (int blk = 0; blk < QPW; ++blk) {
      if (q0 + blk * 128 >= S) break;
#pragma clang loop unroll(disable)
      for (int qi = 0; qi < 2; ++qi) {
        const int qrow_base = q0 + blk * 128 + (qt0 + qi) * 16;
        if (qrow_base >= S) break;
        f32x4 sacc[8];
        att_zero(sacc);
        att_score_tile(sacc, aq_all[blk][qi], lds, F2_K_OFF, ktiles, lm, lg);
        // online softmax update for this tile
        float tmx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) tmx[r] = -3.0e38f;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) {
          if (kt >= ktiles) continue;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float zz = sacc[kt][r] * scale + mval[kt];
            sacc[kt][r] = zz;
            tmx[r] = fmaxf(tmx[r], zz);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          tmx[r] = row16_max(tmx[r]);
          const float mn = fmaxf(mx[blk][qi][r], tmx[r]);
          const float f = __expf(mx[blk][qi][r] - mn);
          mx[blk][qi][r] = mn;
          sm[blk][qi][r] *= f;
#pragma unroll
          for (int dv = 0; dv < 4; ++dv) oacc[blk][qi][dv][r] *= f;
        }
        float tsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) {
          if (kt >= ktiles) continue;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float p = __expf(sacc[kt][r] - mx[blk][qi][r]);
            sacc[kt][r] = p;
            tsum[r] += p;
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sm[blk][qi][r] += row16_sum(tsum[r]);
        }
        // dropout + UNNORMALIZED P tile to per-wave LDS (linear-index RNG)
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) {
          const int col = k0 + kt * 16 + lm;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = qrow_base + lg * 4 + r;
            float p = (kt < ktiles) ? sacc[kt][r] : 0.f;
            if (keep < 1.f && p != 0.f && row < S && col < S) {
              const uint64_t idx = ((uint64_t)bh * S + row) * S + col;
              p = rng_keep16(seed, idx, keep16) ? p * inv_keep : 0.f;
            }
            const int rl = qi * 16 + lg * 4 + r;
            *(ushort_t*)lds_at(
                lds,
                swz(F2_P_OFF + w * 8192 + rl * 256 + (kt * 16 + lm) * 2, rl, 15)) =
                f32_to_bf16((row < S && col < S) ? p : 0.f);
          }
        }
        // ---- PV for this qi straight away (V^T resident, P per-wave) ----
        // same-wave LDS RAW on the P tile: wait the ds_writes explicitly
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        {
          const int rl = qi * 16 + lm;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            bf16x8 ap = *(const bf16x8*)lds_at(
                lds, swz(F2_P_OFF + w * 8192 + rl * 256 + (ks * 32 + lg * 8) * 2,
                         rl, 15));
#pragma unroll
            for (int dvt = 0; dvt < 4; ++dvt) {
              const int dv = dvt * 16 + lm;
              bf16x8 bv = *(const bf16x8*)lds_at(
                  lds, swz(F2_VT_OFF + dv * 256 + (ks * 32 + lg * 8) * 2, dv, 15));
              oacc[blk][qi][dvt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  ap, bv, oacc[blk][qi][dvt], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  // ---- epilogue: normalize by l, write out + stats (local store loop:
  // the 1/l scale and the stats store ride in it) ----
#pragma unroll
  for (int blk = 0; blk < QPW; ++blk) {
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
      const int qrow_base = q0 + blk * 128 + (qt0 + qi) * 16;
      if (qrow_base >= S) break;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = qrow_base + lg * 4 + r;
        const float inv = 1.f / sm[blk][qi][r];
        if (lm == 0 && row < S) {
          m_io[(size_t)bh * S + row] = mx[blk][qi][r];
          l_io[(size_t)bh * S + row] = sm[blk][qi][r];
        }
#pragma unroll
        for (int dvt = 0; dvt < 4; ++dvt) {
          const int dv = dvt * 16 + lm;
          if (row < S)
            out[(((size_t)b * S + row) * h + hh) * ATT_D + dv] =
                f32_to_bf16(oacc[blk][qi][dvt][r] * inv);
        }
      }
    }
  }
}

SKY_EXPORT int sky_attn_flash_fwd(uint64_t stream, uint64_t qkv,
                                  uint64_t mask, uint64_t out, uint64_t m,
                                  uint64_t lsum, int64_t B, int64_t S,
                                  int64_t h, int64_t d, float scale,
                                  float keep, uint64_t salt, uint64_t state) {
  if (d != ATT_D) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int nqb = (int)((S + 127) / 128);
  // 2 query blocks per workgroup where the grid stays >= 256 WGs
  int qpw = (nqb >= 2 && B * h * ((nqb + 1) / 2) >= 512) ? 2 : 1;
  const int nchunk = (nqb + qpw - 1) / qpw;
  dim3 grid((unsigned)(B * h * nchunk));
#define F2L(QPW)                                                               \
  hipLaunchKernelGGL((attn_flash_fwd_kernel<QPW>), grid, dim3(256),            \
                     F2_LDS_BYTES, s, (const ushort_t*)qkv,                    \
                     (const ushort_t*)mask, (ushort_t*)out, (float*)m,         \
                     (float*)lsum, (int)B, (int)S, (int)h, scale, keep, salt,  \
                     (const unsigned long long*)state)
  if (qpw == 2) F2L(2);
  else F2L(1);
#undef F2L

  LAUNCH_CHECK();
  return 0;
}
