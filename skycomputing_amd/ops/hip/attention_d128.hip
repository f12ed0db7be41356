// Attention at head dim 128 (bf16, 1 <= S <= 4096): one chunked keys-on-rows
// family for the whole range, forward, dQ and dK/dV. The design is that of
// attention_long.hip with every d-dependent quantity doubled: K, V, Q and dO
// rows are 256 B, staged into [64][128] sw15 images (att_glds_rows128), a
// score tile contracts 128 values in four mfma_f32_16x16x32_bf16 steps
// (att_score_tile_t128), and O^T, dQ^T, dK^T and dV^T are eight f32x4 per
// lane each, read back from the images by tr16 (abf_tr_rows128_2).
//   * forward: a lane owns ONE query; (m, l) are two lane scalars and the
//     rescale of O^T touches only the lane's own 32 registers;
//   * dQ: dot = dO . O over the stored bf16 O up front (the diagonal of one
//     16 x 16 tile O dO^T, four MFMA steps), written to dot [B*h*S] fp32, the
//     only scratch; P from the saved m and 1/l, dS^T overwrites it and feeds
//     dQ^T += K^T dS^T from registers;
//   * dK/dV: a wave owns 16 keys, dK^T and dV^T stay in registers across the
//     walk over the query chunks.
// No S x S tensor exists anywhere.
//
// Chunk length: 64 tokens. Two images are 32 KB, so the forward and the dQ
// kernel keep the four blocks per CU (128 VGPRs) of the d = 64 kernels; with
// 128-token chunks the images alone would be 64 KB and the eight score tiles
// of a chunk another 16 registers next to the 32 of O^T. The dK/dV kernel
// holds K and V fragments (32), dK^T and dV^T (64) and a pair of P / dS tiles
// (16) at once and cannot fit 128 registers whatever the chunk length; it is
// bounded to three blocks per CU (168 VGPRs), which its 34 KB of LDS allow.
// A 64-key chunk is also the unit of the dropout index (key / 64), one hash
// per (row, key % 16, chunk), and of the causal walk: the diagonal chunk of
// 64-token block i is chunk i.
//
// Compiler figures at --offload-arch=gfx950 (resource-usage remarks), every
// instantiation, scratch 0 in all of them:
//   attn_d128_fwd_kernel     106 / 107 / 108 VGPRs, LDS 33280 B, 4 waves/SIMD
//   attn_d128_bwd_dq_kernel  128 / 128 / 128 VGPRs, LDS 33280 B, 4 waves/SIMD
//   attn_d128_bwd_dkv_kernel 163 / 163 / 164 VGPRs, LDS 34560 B, 3 waves/SIMD
// (mask / no mask / causal; no AGPRs; LDS is dynamic, the launch's figure;
// profiles/r17_notes.md has the same table.)
//
// Grouped-query attention (template parameter GQA, sky_attn_d128_gqa_*): h
// query heads on h_kv shared K/V heads over the packed layout
// [B, S, h + 2*h_kv, 128] (AtdHeads). Forward and dQ: a block per query head
// as above, only the K/V base pointers and the token stride differ. dK/dV: a
// block per (b, K/V head, 64-key block) walks the group's G = h / h_kv query
// heads one after the other into the same dK^T and dV^T registers (see the
// kernel). The GQA = false instantiations are the figures above; GQA = true:
//   attn_d128_fwd_kernel     106 / 107 / 108 VGPRs, LDS 33280 B, 4 waves/SIMD
//   attn_d128_bwd_dq_kernel  128 / 128 / 128 VGPRs, LDS 33280 B, 4 waves/SIMD
//   attn_d128_bwd_dkv_kernel 164 / 164 / 165 VGPRs, LDS 34560 B, 3 waves/SIMD
// scratch 0, no AGPRs; the dK/dV kernel keeps 14 / 14 / 8 scalars in lanes of
// one VGPR, read once per head outside the chunk walk
// (profiles/r18_notes.md).
//
// Dropout: att_drop_hash_c64 + att_drop_keep (attn_common.h), index
// ((bh*S + row)*16 + key%16) * NC + key/64, slice (key/16) & 3: no d in it, so
// for equal (salt, state, B, S, h) the keep mask is the d = 64 long kernels'
// bit for bit. Both backward kernels regenerate it; nothing is stored.

#include "attn_common.h"

#define ATD_SMAX 4096
#define ATD_C 64  // chunk length in tokens, and the 64-token block of a grid entry

// As attention_long.hip: without the packed fp32 VALU ops; with them the
// score loops are packed into register pairs and the kernels spill.
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass does not know the feature
#define ATD_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define ATD_NO_PK_F32
#endif
#define ATD_KERNEL ATD_NO_PK_F32 __global__ __launch_bounds__(256, 4)
#define ATD_KERNEL3 ATD_NO_PK_F32 __global__ __launch_bounds__(256, 3)

// lm / lg made opaque once per chunk, so that the LDS addresses built from
// them are recomputed per chunk and not hoisted out of the chunk loop into
// registers that spill (atl_chunk_lanes of attention_long.hip)
DEV void atd_chunk_lanes(int& lmc, int& lgc, int lm, int lg) {
  lmc = lm;
  lgc = lg;
  asm volatile("" : "+v"(lmc), "+v"(lgc));
}

// the tiles of a chunk a wave visits under the triangle: up to the one that
// holds its first query, rel = 16-aligned query base minus the chunk's first
// key (>= 0)
DEV int atd_tri_tiles(int nt, int rel) {
  const int d = (rel >> 4) + 1;
  return nt < d ? nt : d;
}

// the lane's four hashes for 64-key chunk kc: hash r covers keys
// kc*64 + mt*16 + lg*4 + r, mt = 0..3 its four 16-bit slices
DEV void atd_drop_hash_chunk(uint64_t (&z)[4], uint64_t seed, int bh, int S,
                             int q, int lg, int kc) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    z[r] = att_drop_hash_c64(seed, bh, S, q, lg * 4 + r, kc);
}
DEV bool atd_drop_keep(uint64_t z, int mt, unsigned keep16) {
  const uint64_t zz[2] = {z, 0};
  return att_drop_keep(zz, mt, keep16);
}

// the diagonal of the wave's 16 x 16 tile O dO^T as dot[q] on every lane of
// column lm = q: from the same MFMA and in the same order over j as
// dPd^T = V dO^T, so that dP - dot cancels exactly where one key holds all
// of a row's weight (attention_long.hip's dQ kernel has the argument)
DEV float atd_row_dot(const ushort_t* __restrict__ orow,
                      const bf16x8 (&bdo)[4], int lm, int lg) {
  f32x4 dd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const bf16x8 ao = *(const bf16x8*)(orow + ks * 32 + lg * 8);
    dd = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ao, bdo[ks], dd, 0, 0, 0);
  }
  // element (lm, lm) is register lm & 3 of the lane (lg = lm >> 2, lm)
  const float dsel = (lm & 2) ? ((lm & 1) ? dd[3] : dd[2]) : ((lm & 1) ? dd[1] : dd[0]);
  return __shfl(dsel, ((lm >> 2) << 4) | lm, 64);
}

// The head arithmetic of the packed layout [B, S, h + 2*h_kv, 128]: query
// head hh at column hh, key head g at h + g, value head g at h + h_kv + g
// (columns of 128 values), query head hh on K/V head hh / G, G = h / h_kv.
// GQA = false is multi-head attention, [B, S, 3, h, 128]: h_kv is not read
// and every expression folds to the one in h alone. All of it is computed
// from kernel arguments and the block index: wave-uniform scalars.
template <bool GQA>
struct AtdHeads {
  int h, hkv, G, ts;
  DEV AtdHeads(int h_, int h_kv)
      : h(h_), hkv(GQA ? h_kv : h_), G(GQA ? h_ / h_kv : 1),
        ts((h_ + 2 * (GQA ? h_kv : h_)) * ATT_D128) {}
  DEV int kcol(int g) const { return h + g; }
  DEV int vcol(int g) const { return h + hkv + g; }
};

// LDS of the forward and the dQ kernel: K chunk @0, V chunk @16K, the
// chunk's key mask fp32 @32K (att_mask_keys_lds_at writes 128 values, the
// chunk's 64 and the next chunk's): 33280 B, four blocks per CU,
// single-buffered: co-resident blocks cover each other's load phase.
#define ATD_K_OFF KR_IMG0_OFF
#define ATD_V_OFF KR_IMG1_OFF
#define ATD_MASK_OFF KR_AUX_OFF
#define ATD_FWD_LDS (KR_AUX_OFF + 512)

// ---------------------------------------------------------------------------
// Forward. One block per (b, h, 64-query block), a wave owns 16 queries (Q
// fragments from global, four bf16x8).
// CAUSAL (no additive mask): q sees k iff k <= q. Block qb stops at chunk qb,
// its diagonal chunk; inside it wave w stops at tile w, its own.
template <bool HAS_MASK, bool CAUSAL, bool GQA>
ATD_KERNEL void attn_d128_fwd_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ mask,
    ushort_t* __restrict__ out, float* __restrict__ m_io,
    float* __restrict__ l_io, int B, int S, int h, float scale, float keep,
    uint64_t salt, const unsigned long long* __restrict__ state, int h_kv) {
  static_assert(!CAUSAL || !HAS_MASK, "causal mode takes no additive mask");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int l = tid & 63;
  const int w = tid >> 6;
  const int lm = l & 15;
  const int lg = l >> 4;
  const int QB = (S + ATD_C - 1) / ATD_C;
  const int bh = blockIdx.x / QB;
  const int qb = blockIdx.x % QB;
  const int b = bh / h;
  const int hh = bh % h;
  const AtdHeads<GQA> hd(h, h_kv);
  const int ts = hd.ts;
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* tokb = qkv + (size_t)b * S * ts;
  const ushort_t* qbase = tokb + (size_t)hh * ATT_D128;
  const ushort_t* kbase = tokb + (size_t)hd.kcol(hh / hd.G) * ATT_D128;
  const ushort_t* vbase = tokb + (size_t)hd.vcol(hh / hd.G) * ATT_D128;
  float* mk = (float*)lds_at(lds, ATD_MASK_OFF);

  const int qtok_base = qb * ATD_C + w * 16;
  const bool active = qtok_base < S;  // wave-uniform
  const int q = qtok_base + lm;       // this lane's query
  const int qc = q < S ? q : S - 1;
  bf16x8 bq[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    bq[ks] = *(const bf16x8*)(qbase + (size_t)qc * ts + ks * 32 + lg * 8);
  // the chunks past a query block's diagonal chunk are never staged
  const int kc1 = CAUSAL ? qb + 1 : QB;

  // Why m is a real score after the first visited chunk, at 64-key chunks:
  // the walk starts at chunk 0, which always holds key 0, and additive masks
  // are finite (-10000), so after chunk 0 m is a real score. Before it,
  // m = -3e38 gives alpha = exp(-3e38 - m_new) = 0 against l = 0 and O = 0;
  // later, a jump of m by 1e4 (chunks of masked keys followed by a visible
  // one) gives alpha = 0 as well, the correct weight of the terms so far.
  // Keys >= S carry -3e38 against a real m: p = exp(-3e38 - m) = 0 exactly.
  // No inf - inf can form: m and every score are finite, never infinite.
  // CAUSAL: key 0 is visible to every query, so the same holds after chunk
  // 0; every later chunk kc <= qb starts at key 64*kc <= 64*qb <= q, and the
  // tiles a wave visits in its diagonal chunk begin with that key, so no lane
  // meets a chunk without a visible key, and the keys above the diagonal are
  // -3e38 against a real m: exact zeros. Lanes past S hold the clamped
  // query's finite values and store nothing.
  float m = -3.0e38f, lsum = 0.f;
  f32x4 oacc[8];
  att_zero(oacc);

#pragma clang loop unroll(disable)
  for (int kc = 0; kc < kc1; ++kc) {
    const int k0 = kc * ATD_C;
    const int nk = S - k0 < ATD_C ? S - k0 : ATD_C;
    const int NT = (nk + 15) / 16;
    const int NP = (nk + 31) / 32;  // key-tile pairs = PV contraction steps
    if (kc != 0) __syncthreads();   // every wave is done with the last chunk
    // whole tile pairs are staged; tokens >= S re-read token S-1, finite
    // values that the -3e38 mask (scores) and the zero P (PV) null
    att_glds_rows128(kbase, ts, k0, NP * 32, S, lds, ATD_K_OFF, tid);
    att_glds_rows128(vbase, ts, k0, NP * 32, S, lds, ATD_V_OFF, tid);
    if constexpr (!CAUSAL) att_mask_keys_lds_at(mk, HAS_MASK, mask, b, S, k0, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) continue;
    int lmc, lgc;
    atd_chunk_lanes(lmc, lgc, lm, lg);
    // CAUSAL: the wave's tiles end with its diagonal tile (wave-uniform; NT
    // in every chunk before the diagonal one); a skipped tile keeps
    // att_zero's zeros through to the PV pair that holds it
    const int NTw = CAUSAL ? atd_tri_tiles(NT, qtok_base - k0) : NT;
    const int NPw = CAUSAL ? (NTw + 1) >> 1 : NP;

    f32x4 sacc[4];
    att_zero(sacc);
    att_score_tile_t128(sacc, bq, lds, ATD_K_OFF, 0, 0, NTw, lmc, lgc);
    float mx = -3.0e38f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      if (mt >= NTw) continue;
      f32x4 mv;
      if constexpr (CAUSAL)
        mv = att_tri_mask4<false>(nullptr, mt, lgc, 0, q - k0, nk);
      else mv = att_mask_keys4(mk, mt, lgc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float zz = sacc[mt][r] * scale + mv[r];
        sacc[mt][r] = zz;
        mx = fmaxf(mx, zz);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx);
    const float alpha = __expf(m - m_new);
    m = m_new;
    uint64_t z[4] = {0, 0, 0, 0};
    if (keep < 1.f) atd_drop_hash_chunk(z, seed, bh, S, q, lg, kc);
    // unnormalised p (the sum takes it before dropout), dropped in place;
    // keys >= S come out as exact zeros. 1/keep is not applied here but to
    // O^T at the end, with 1/l: the bf16 Pd operand then holds p itself, and
    // the row's largest key, p = 1, is exact there where 1/keep is not (a
    // row that one key dominates, the first rows under the triangle, would
    // carry that rounding into O and into the dQ kernel's dot = dO . O).
    float sm = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      if (mt >= NTw) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = __expf(sacc[mt][r] - m_new);
        sm += p;
        if (keep < 1.f) p = atd_drop_keep(z[r], mt, keep16) ? p : 0.f;
        sacc[mt][r] = p;
      }
    }
    sm += __shfl_xor(sm, 16, 64);
    sm += __shfl_xor(sm, 32, 64);
    lsum = lsum * alpha + sm;
    // the O^T column lm is this lane's query: the rescale is lane-local
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) oacc[ct] *= alpha;
    // O^T += V^T Pd^T: B = the score registers, A = V^T by tr16
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
      if (kp >= NPw) continue;
      const bf16x8 bp = att_pack_dpair(sacc[2 * kp], sacc[2 * kp + 1]);
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        const bf16x8 av = abf_tr_rows128_2(lds, ATD_V_OFF, kp * 32 + lgc * 4,
                                           kp * 32 + 16 + lgc * 4, ct * 4, lmc);
        oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bp, oacc[ct], 0, 0, 0);
      }
    }
  }
  if (!active) return;
  const float inv = inv_keep / lsum;  // inv_keep = 1 exactly without dropout
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) oacc[ct] *= inv;
  if (lg == 0 && q < S) {
    m_io[(size_t)bh * S + q] = m;
    l_io[(size_t)bh * S + q] = lsum;
  }
  ushort_t* obase = out + ((size_t)b * S * h + hh) * ATT_D128;
  att_store_cols16_d128(obase, h * ATT_D128, oacc, qtok_base, S, lm, lg);
}

// ---------------------------------------------------------------------------
// Backward dQ. One block per (b, h, 64-query block); K and V come in chunks
// as in the forward. Per pair of key tiles: S^T and dPd^T (four MFMA steps
// each per tile), P from the saved statistics, dS^T over the scores,
// dQ^T += K^T dS^T; only the pair is live. Writes dot[bh*S + q] for the
// dK/dV kernel. LDS as the forward.
template <bool HAS_MASK, bool CAUSAL, bool GQA>
ATD_KERNEL void attn_d128_bwd_dq_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ dout,
    const ushort_t* __restrict__ out, const ushort_t* __restrict__ mask,
    const float* __restrict__ m_io, const float* __restrict__ l_io,
    float* __restrict__ dot_out, ushort_t* __restrict__ dqkv, int B, int S,
    int h, float scale, float keep, uint64_t salt,
    const unsigned long long* __restrict__ state, int h_kv) {
  static_assert(!CAUSAL || !HAS_MASK, "causal mode takes no additive mask");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int l = tid & 63;
  const int w = tid >> 6;
  const int lm = l & 15;
  const int lg = l >> 4;
  const int QB = (S + ATD_C - 1) / ATD_C;
  const int bh = blockIdx.x / QB;
  const int qb = blockIdx.x % QB;
  const int b = bh / h;
  const int hh = bh % h;
  const AtdHeads<GQA> hd(h, h_kv);
  const int ts = hd.ts;
  const int dots = h * ATT_D128;
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* tokb = qkv + (size_t)b * S * ts;
  const ushort_t* qbase = tokb + (size_t)hh * ATT_D128;
  const ushort_t* kbase = tokb + (size_t)hd.kcol(hh / hd.G) * ATT_D128;
  const ushort_t* vbase = tokb + (size_t)hd.vcol(hh / hd.G) * ATT_D128;
  const ushort_t* dobase = dout + ((size_t)b * S * h + hh) * ATT_D128;
  const ushort_t* obase = out + ((size_t)b * S * h + hh) * ATT_D128;
  float* mk = (float*)lds_at(lds, ATD_MASK_OFF);

  const int qtok_base = qb * ATD_C + w * 16;
  const bool active = qtok_base < S;
  const int q = qtok_base + lm;  // this lane's query
  const int qc = q < S ? q : S - 1;

  bf16x8 bq[4], bdo[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    bq[ks] = *(const bf16x8*)(qbase + (size_t)qc * ts + ks * 32 + lg * 8);
    bdo[ks] = *(const bf16x8*)(dobase + (size_t)qc * dots + ks * 32 + lg * 8);
  }
  const float dot = atd_row_dot(obase + (size_t)qc * dots, bdo, lm, lg);
  if (active && lg == 0 && q < S) dot_out[(size_t)bh * S + q] = dot;
  const float mrow = m_io[(size_t)bh * S + qc];
  const float lrow = 1.f / l_io[(size_t)bh * S + qc];
  const int kc1 = CAUSAL ? qb + 1 : QB;

  f32x4 qacc[8];
  att_zero(qacc);
#pragma clang loop unroll(disable)
  for (int kc = 0; kc < kc1; ++kc) {
    const int k0 = kc * ATD_C;
    const int nk = S - k0 < ATD_C ? S - k0 : ATD_C;
    const int NT = (nk + 15) / 16;
    const int NP = (nk + 31) / 32;
    if (kc != 0) __syncthreads();
    att_glds_rows128(kbase, ts, k0, NP * 32, S, lds, ATD_K_OFF, tid);
    att_glds_rows128(vbase, ts, k0, NP * 32, S, lds, ATD_V_OFF, tid);
    if constexpr (!CAUSAL) att_mask_keys_lds_at(mk, HAS_MASK, mask, b, S, k0, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) continue;
    int lmc, lgc;
    atd_chunk_lanes(lmc, lgc, lm, lg);
    // CAUSAL: tiles and pairs up to the wave's diagonal tile, as the forward
    const int NTw = CAUSAL ? atd_tri_tiles(NT, qtok_base - k0) : NT;
    const int NPw = CAUSAL ? (NTw + 1) >> 1 : NP;

    uint64_t z[4] = {0, 0, 0, 0};
    if (keep < 1.f) atd_drop_hash_chunk(z, seed, bh, S, q, lg, kc);
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
      if (kp >= NPw) continue;
      f32x4 s2[2], d2[2];
      att_zero(s2);
      att_zero(d2);
      att_score_tile_t128(s2, bq, lds, ATD_K_OFF, 2 * kp, 0, NTw, lmc, lgc);   // K Q^T
      att_score_tile_t128(d2, bdo, lds, ATD_V_OFF, 2 * kp, 0, NTw, lmc, lgc);  // V dO^T
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int mt = 2 * kp + t;
        if (mt >= NTw) continue;  // s2[t] stays zero: a null dS tile
        f32x4 mv;
        if constexpr (CAUSAL)
          mv = att_tri_mask4<false>(nullptr, mt, lgc, 0, q - k0, nk);
        else mv = att_mask_keys4(mk, mt, lgc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + mt * 16 + lg * 4 + r;
          const float p = att_prob(s2[t][r], scale, mv[r], mrow, lrow,
                                   q < S && key < S);
          float dp = d2[t][r];
          if (keep < 1.f)
            dp = atd_drop_keep(z[r], mt, keep16) ? dp * inv_keep : 0.f;
          s2[t][r] = scale * p * (dp - dot);
        }
      }
      const bf16x8 bds = att_pack_dpair(s2[0], s2[1]);
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        const bf16x8 ak = abf_tr_rows128_2(lds, ATD_K_OFF, kp * 32 + lgc * 4,
                                           kp * 32 + 16 + lgc * 4, ct * 4, lmc);
        qacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak, bds, qacc[ct], 0, 0, 0);
      }
    }
  }
  if (!active) return;
  ushort_t* dq = dqkv + (size_t)b * S * ts + (size_t)hh * ATT_D128;
  att_store_cols16_d128(dq, ts, qacc, qtok_base, S, lm, lg);
}

// ---------------------------------------------------------------------------
// Backward dK/dV. One block per (b, h, 64-key block), launched after the dQ
// kernel (it reads dot). A wave owns 16 keys, K and V fragments from global
// (four bf16x8 each); dK^T and dV^T stay in registers while the queries go by
// in chunks of 64: Q and dO images, m | 1/l | dot and the chunk's keep bits
// in LDS, and inside a chunk pairs of 16-row tiles.
// LDS: Q chunk @0, dO chunk @16K, m | 1/l | dot fp32 [64] each @32K, keep
// bits (att_drop_bits_lds_long, 64 rows) @32K + 768: 34560 B.
// CAUSAL: key block kb begins with query chunk kb, its diagonal chunk, and in
// it wave w begins with tile w.
// GQA: one block per (b, K/V head g, 64-key block), grid B * h_kv * ceil(S/64).
// The wave's K and V fragments are loaded once and the block takes the walk
// above once per query head of the group, g*G .. g*G + G-1, into the same
// dK^T and dV^T: one fp32 sum over the group, one rounding, one store, no
// atomics and no partials. G times the work in a block over G times fewer
// blocks; the LDS and the registers are those of the one-head walk.
#define ATD_Q_OFF KR_IMG0_OFF
#define ATD_DO_OFF KR_IMG1_OFF
#define ATD_STAT_OFF KR_AUX_OFF
#define ATD_BITS_OFF (KR_AUX_OFF + 768)
#define ATD_DKV_LDS (KR_AUX_OFF + 768 + 1024)

template <bool HAS_MASK, bool CAUSAL, bool GQA>
ATD_KERNEL3 void attn_d128_bwd_dkv_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ dout,
    const ushort_t* __restrict__ mask, const float* __restrict__ m_io,
    const float* __restrict__ l_io, const float* __restrict__ dot_in,
    ushort_t* __restrict__ dqkv, int B, int S, int h, float scale, float keep,
    uint64_t salt, const unsigned long long* __restrict__ state, int h_kv) {
  static_assert(!CAUSAL || !HAS_MASK, "causal mode takes no additive mask");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x;
  const int l = tid & 63;
  const int w = tid >> 6;
  const int lm = l & 15;
  const int lg = l >> 4;
  const int QB = (S + ATD_C - 1) / ATD_C;
  const AtdHeads<GQA> hd(h, h_kv);
  const int bg = blockIdx.x / QB;  // b * h_kv + g
  const int kb = blockIdx.x % QB;
  const int b = bg / hd.hkv;
  const int g = bg % hd.hkv;
  const int ts = hd.ts;
  const int dots = h * ATT_D128;
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* tokb = qkv + (size_t)b * S * ts;
  const ushort_t* kbase = tokb + (size_t)hd.kcol(g) * ATT_D128;
  const ushort_t* vbase = tokb + (size_t)hd.vcol(g) * ATT_D128;
  float* st = (float*)lds_at(lds, ATD_STAT_OFF);
  unsigned char* bits = (unsigned char*)lds_at(lds, ATD_BITS_OFF);

  const int ktok_base = kb * ATD_C + w * 16;
  const bool active = ktok_base < S;
  const int key = ktok_base + lm;  // this lane's key
  const int kcl = key < S ? key : S - 1;

  bf16x8 bk[4], bv[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    bk[ks] = *(const bf16x8*)(kbase + (size_t)kcl * ts + ks * 32 + lg * 8);
    bv[ks] = *(const bf16x8*)(vbase + (size_t)kcl * ts + ks * 32 + lg * 8);
  }
  float mv = 0.f;
  if (HAS_MASK && key < S) mv = bf16_to_f32(mask[(size_t)b * S + key]);
  if (key >= S) mv = -3.0e38f;
  // CAUSAL: the chunks before a key block's diagonal chunk are never staged
  const int qc0 = CAUSAL ? kb : 0;

  f32x4 kacc[8], vacc[8];
  att_zero(kacc);
  att_zero(vacc);
  // The group's G query heads one after the other (MHA: the one head g), each
  // with its own walk over the query chunks; kacc and vacc run through all
  // G * (QB - qc0) visits, so dK and dV of the shared head are summed in fp32
  // and rounded once. Head, bh and the two base pointers come from the block
  // index and the loop counter: scalars.
#pragma clang loop unroll(disable)
  for (int j = 0; j < hd.G; ++j) {
    const int hh = g * hd.G + j;
    const int bh = b * h + hh;  // the query head's: statistics, dot, dropout
    const ushort_t* qbase = tokb + (size_t)hh * ATT_D128;
    const ushort_t* dobase = dout + ((size_t)b * S * h + hh) * ATT_D128;
#pragma clang loop unroll(disable)
    for (int qch = qc0; qch < QB; ++qch) {
      const int q0 = qch * ATD_C;
      const int nq = S - q0 < ATD_C ? S - q0 : ATD_C;
      const int NT = (nq + 15) / 16;
      const int NP = (nq + 31) / 32;
      // the one barrier before LDS is reused, on every visit but the block's
      // first: the first chunk of head j + 1 overwrites what the last chunk of
      // head j is still being read from. Waves without keys (!active) skip the
      // work below and take every barrier of every head.
      if (j != 0 || qch != qc0) __syncthreads();
      att_glds_rows128(qbase, ts, q0, NP * 32, S, lds, ATD_Q_OFF, tid);
      att_glds_rows128(dobase, dots, q0, NP * 32, S, lds, ATD_DO_OFF, tid);
      // rows >= S: 1/l = 0 and a false valid flag null P, dot = 0 keeps dS finite
      if (tid < ATD_C) {
        const int row = q0 + tid;
        const bool live = row < S;
        st[tid] = live ? m_io[(size_t)bh * S + row] : 0.f;
        st[ATD_C + tid] = live ? 1.f / l_io[(size_t)bh * S + row] : 0.f;
        st[2 * ATD_C + tid] = live ? dot_in[(size_t)bh * S + row] : 0.f;
      }
      if (keep < 1.f)
        att_drop_bits_lds_long(bits, seed, bh, S, kb, q0, NP * 32, keep16, tid);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (!active) continue;
      int lmc, lgc;
      atd_chunk_lanes(lmc, lgc, lm, lg);
      // CAUSAL: in the diagonal chunk the wave starts at its own tile (0 in
      // every later chunk); wave-uniform, no barrier below
      const int tw0 = CAUSAL && ktok_base > q0 ? (ktok_base - q0) >> 4 : 0;

#pragma unroll
      for (int qp = 0; qp < 2; ++qp) {
        if (qp >= NP) continue;
        if constexpr (CAUSAL) if (qp < tw0 >> 1) continue;
        f32x4 pd[2], ds[2];
        att_zero(pd);
        att_zero(ds);
        // Q K^T and dO V^T: the images are the A side here, the wave's K and V
        // fragments the B side, so a lane holds queries qt*16 + lg*4 + r
        // against ITS key
        att_score_tile_t128(pd, bk, lds, ATD_Q_OFF, 2 * qp, tw0, NT, lmc, lgc);
        att_score_tile_t128(ds, bv, lds, ATD_DO_OFF, 2 * qp, tw0, NT, lmc, lgc);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int qt = 2 * qp + t;
          if (qt >= NT) continue;
          if constexpr (CAUSAL) if (qt < tw0) continue;
          const f32x4 m4 = *(const f32x4*)(st + qt * 16 + lgc * 4);
          const f32x4 il4 = *(const f32x4*)(st + ATD_C + qt * 16 + lgc * 4);
          const f32x4 dot4 = *(const f32x4*)(st + 2 * ATD_C + qt * 16 + lgc * 4);
          unsigned kbits = 0xFFFFFFFFu;
          if (keep < 1.f)
            kbits = *(const unsigned*)(bits + ((qt * 4 + lgc) * 16 + lmc) * 4);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int qq = q0 + qt * 16 + lg * 4 + r;
            // the lane's token is the key here: the triangle compare turns round
            const float mvr = (CAUSAL && qq < key) ? -3.0e38f : mv;
            const float p = att_prob(pd[t][r], scale, mvr, m4[r], il4[r],
                                     qq < S && key < S);
            const bool kbit = (kbits >> (8 * r + w)) & 1u;
            // Pd without its 1/keep, which dV^T takes at the end (as the
            // forward's O^T does)
            float pdv = p, dp = ds[t][r];
            if (keep < 1.f) {
              pdv = kbit ? p : 0.f;
              dp = kbit ? dp * inv_keep : 0.f;
            }
            pd[t][r] = pdv;
            ds[t][r] = scale * p * (dp - dot4[r]);
          }
        }
        const bf16x8 bpd = att_pack_dpair(pd[0], pd[1]);
        const bf16x8 bds = att_pack_dpair(ds[0], ds[1]);
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) {
          const bf16x8 adot = abf_tr_rows128_2(lds, ATD_DO_OFF, qp * 32 + lgc * 4,
                                               qp * 32 + 16 + lgc * 4, ct * 4, lmc);
          vacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(adot, bpd, vacc[ct], 0, 0, 0);
          const bf16x8 aqt = abf_tr_rows128_2(lds, ATD_Q_OFF, qp * 32 + lgc * 4,
                                              qp * 32 + 16 + lgc * 4, ct * 4, lmc);
          kacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aqt, bds, kacc[ct], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) vacc[ct] *= inv_keep;
  // stored once, at the K/V head's own columns
  ushort_t* dk = dqkv + (size_t)b * S * ts + (size_t)hd.kcol(g) * ATT_D128;
  ushort_t* dv = dqkv + (size_t)b * S * ts + (size_t)hd.vcol(g) * ATT_D128;
  att_store_cols16_d128(dk, ts, kacc, ktok_base, S, lm, lg);
  att_store_cols16_d128(dv, ts, vacc, ktok_base, S, lm, lg);
}

// ---------------------------------------------------------------------------
// Entry points: d = 128 and 1 <= S <= 4096; argument lists as their
// sky_attn_long_* counterparts, the causal pair without ids and bounds. The
// sky_attn_d128_gqa_* forms take h_kv after h and the packed layout
// [B, S, h + 2*h_kv, 128], 1 <= h_kv, h % h_kv == 0; out, m, l and dot are
// indexed by the query head as in the multi-head forms.
template <bool GQA>
static bool atd_shape_ok(int64_t S, int64_t h, int64_t h_kv, int64_t d,
                         bool causal) {
  if (GQA && (h_kv < 1 || h % h_kv != 0)) return false;
  return d == ATT_D128 && S >= (causal ? 2 : 1) && S <= ATD_SMAX;
}
// heads = h (forward, dQ: a block per query head) or h_kv (the GQA dK/dV)
static dim3 atd_grid(int64_t B, int64_t S, int64_t heads) {
  return dim3((unsigned)(B * heads * ((S + ATD_C - 1) / ATD_C)));
}

template <bool CAUSAL, bool GQA>
static int atd_fwd(uint64_t stream, uint64_t qkv, uint64_t mask, uint64_t out,
                   uint64_t m, uint64_t lsum, int64_t B, int64_t S, int64_t h,
                   int64_t h_kv, int64_t d, float scale, float keep,
                   uint64_t salt, uint64_t state) {
  if (!atd_shape_ok<GQA>(S, h, h_kv, d, CAUSAL) || qkv == 0 || out == 0 ||
      m == 0 || lsum == 0)
    return (int)hipErrorInvalidValue;
  ATT_LAUNCH_HM(!CAUSAL && mask != 0,
                (attn_d128_fwd_kernel<HM && !CAUSAL, CAUSAL, GQA>),
                atd_grid(B, S, h), ATD_FWD_LDS, (hipStream_t)stream,
                (const ushort_t*)qkv, (const ushort_t*)mask, (ushort_t*)out,
                (float*)m, (float*)lsum, (int)B, (int)S, (int)h, scale, keep,
                salt, (const unsigned long long*)state, (int)h_kv);
  LAUNCH_CHECK();
  return 0;
}

// dQ + dot, then dK/dV. out: the forward's output [B,S,h,128]; dot: fp32
// [B*h*S], written by the dQ kernel and read by the dK/dV kernel.
template <bool CAUSAL, bool GQA>
static int atd_bwd(uint64_t stream, uint64_t qkv, uint64_t dout, uint64_t out,
                   uint64_t mask, uint64_t m, uint64_t lsum, uint64_t dot,
                   uint64_t dqkv, int64_t B, int64_t S, int64_t h,
                   int64_t h_kv, int64_t d, float scale, float keep,
                   uint64_t salt, uint64_t state) {
  if (!atd_shape_ok<GQA>(S, h, h_kv, d, CAUSAL) || qkv == 0 || dout == 0 ||
      out == 0 || m == 0 || lsum == 0 || dot == 0 || dqkv == 0)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  ATT_LAUNCH_HM(!CAUSAL && mask != 0,
                (attn_d128_bwd_dq_kernel<HM && !CAUSAL, CAUSAL, GQA>),
                atd_grid(B, S, h), ATD_FWD_LDS, s, (const ushort_t*)qkv,
                (const ushort_t*)dout, (const ushort_t*)out,
                (const ushort_t*)mask, (const float*)m, (const float*)lsum,
                (float*)dot, (ushort_t*)dqkv, (int)B, (int)S, (int)h, scale,
                keep, salt, (const unsigned long long*)state, (int)h_kv);
  ATT_LAUNCH_HM(!CAUSAL && mask != 0,
                (attn_d128_bwd_dkv_kernel<HM && !CAUSAL, CAUSAL, GQA>),
                atd_grid(B, S, GQA ? h_kv : h), ATD_DKV_LDS, s,
                (const ushort_t*)qkv, (const ushort_t*)dout,
                (const ushort_t*)mask, (const float*)m, (const float*)lsum,
                (const float*)dot, (ushort_t*)dqkv, (int)B, (int)S, (int)h,
                scale, keep, salt, (const unsigned long long*)state,
                (int)h_kv);
  LAUNCH_CHECK();
  return 0;
}

SKY_EXPORT int sky_attn_d128_fwd(uint64_t stream, uint64_t qkv, uint64_t mask,
                                 uint64_t out, uint64_t m, uint64_t lsum,
                                 int64_t B, int64_t S, int64_t h, int64_t d,
                                 float scale, float keep, uint64_t salt,
                                 uint64_t state) {
  return atd_fwd<false, false>(stream, qkv, mask, out, m, lsum, B, S, h, h, d,
                               scale, keep, salt, state);
}

SKY_EXPORT int sky_attn_d128_bwd(uint64_t stream, uint64_t qkv, uint64_t dout,
                                 uint64_t out, uint64_t mask, uint64_t m,
                                 uint64_t lsum, uint64_t dot, uint64_t dqkv,
                                 int64_t B, int64_t S, int64_t h, int64_t d,
                                 float scale, float keep, uint64_t salt,
                                 uint64_t state) {
  return atd_bwd<false, false>(stream, qkv, dout, out, mask, m, lsum, dot,
                               dqkv, B, S, h, h, d, scale, keep, salt, state);
}

// The causal forms (q attends k iff k <= q), 2 <= S <= 4096: no mask, no ids.
SKY_EXPORT int sky_attn_d128_causal_fwd(uint64_t stream, uint64_t qkv,
                                        uint64_t out, uint64_t m, uint64_t lsum,
                                        int64_t B, int64_t S, int64_t h,
                                        int64_t d, float scale, float keep,
                                        uint64_t salt, uint64_t state) {
  return atd_fwd<true, false>(stream, qkv, 0, out, m, lsum, B, S, h, h, d,
                              scale, keep, salt, state);
}

SKY_EXPORT int sky_attn_d128_causal_bwd(uint64_t stream, uint64_t qkv,
                                        uint64_t dout, uint64_t out, uint64_t m,
                                        uint64_t lsum, uint64_t dot,
                                        uint64_t dqkv, int64_t B, int64_t S,
                                        int64_t h, int64_t d, float scale,
                                        float keep, uint64_t salt,
                                        uint64_t state) {
  return atd_bwd<true, false>(stream, qkv, dout, out, 0, m, lsum, dot, dqkv, B,
                              S, h, h, d, scale, keep, salt, state);
}

// Grouped-query forms: the four above with h_kv after h.
SKY_EXPORT int sky_attn_d128_gqa_fwd(uint64_t stream, uint64_t qkv,
                                     uint64_t mask, uint64_t out, uint64_t m,
                                     uint64_t lsum, int64_t B, int64_t S,
                                     int64_t h, int64_t h_kv, int64_t d,
                                     float scale, float keep, uint64_t salt,
                                     uint64_t state) {
  return atd_fwd<false, true>(stream, qkv, mask, out, m, lsum, B, S, h, h_kv,
                              d, scale, keep, salt, state);
}

SKY_EXPORT int sky_attn_d128_gqa_bwd(uint64_t stream, uint64_t qkv,
                                     uint64_t dout, uint64_t out, uint64_t mask,
                                     uint64_t m, uint64_t lsum, uint64_t dot,
                                     uint64_t dqkv, int64_t B, int64_t S,
                                     int64_t h, int64_t h_kv, int64_t d,
                                     float scale, float keep, uint64_t salt,
                                     uint64_t state) {
  return atd_bwd<false, true>(stream, qkv, dout, out, mask, m, lsum, dot, dqkv,
                              B, S, h, h_kv, d, scale, keep, salt, state);
}

SKY_EXPORT int sky_attn_d128_gqa_causal_fwd(uint64_t stream, uint64_t qkv,
                                            uint64_t out, uint64_t m,
                                            uint64_t lsum, int64_t B, int64_t S,
                                            int64_t h, int64_t h_kv, int64_t d,
                                            float scale, float keep,
                                            uint64_t salt, uint64_t state) {
  return atd_fwd<true, true>(stream, qkv, 0, out, m, lsum, B, S, h, h_kv, d,
                             scale, keep, salt, state);
}

SKY_EXPORT int sky_attn_d128_gqa_causal_bwd(uint64_t stream, uint64_t qkv,
                                            uint64_t dout, uint64_t out,
                                            uint64_t m, uint64_t lsum,
                                            uint64_t dot, uint64_t dqkv,
                                            int64_t B, int64_t S, int64_t h,
                                            int64_t h_kv, int64_t d, float scale,
                                            float keep, uint64_t salt,
                                            uint64_t state) {
  return atd_bwd<true, true>(stream, qkv, dout, out, 0, m, lsum, dot, dqkv, B,
                             S, h, h_kv, d, scale, keep, salt, state);
}

