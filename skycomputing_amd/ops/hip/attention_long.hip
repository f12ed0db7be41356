// Attention for 128 < S <= 4096 (d = 64, bf16): the keys-on-rows kernels of
// attention.hip / attention_bwd.hip turned into flash kernels. The S <= 128
// kernels hold a whole row of scores in registers; here the other side of
// each product arrives in chunks of 128 tokens, staged into the same two
// [128][64] sw7 images, and what a lane carries from chunk to chunk is per
// lane:
//   * forward: with keys on the MFMA rows a lane owns ONE query in both
//     S^T = K Q^T and O^T = V^T Pd^T, so the online-softmax state (m, l) is
//     two lane scalars and the rescale oacc *= exp(m - m_new) touches only
//     the lane's own registers: no shuffle, no LDS;
//   * dQ: the row dot cannot wait for the last chunk, so it is taken up
//     front as sum_j dO[q,j] * O[q,j] (equal to sum_k dP * P, dropout
//     included), the diagonal of one 16 x 16 MFMA tile O dO^T; P comes from
//     the saved m and 1/l, dS^T overwrites it and feeds dQ^T += K^T dS^T;
//   * dK/dV: a wave owns 16 keys, dK^T and dV^T stay in registers across
//     the walk over the queries.
// No S x S tensor and no scratch beyond dot [B*h*S] fp32 exists anywhere.
// Dropout: att_drop_hash_c64 + att_drop_keep (attn_common.h), regenerated
// in both backward kernels from (salt, state).
// Segment mode (SEG, packed sequences): query q sees key k iff their segment
// ids are equal, and equal ids form one contiguous run per row. A 64-token
// block then walks only the chunks between the run start of its first token
// and the run end of its last one (attn_seg_bounds_kernel's table; the
// relation is symmetric, so the table serves query and key blocks alike).
// The dropout hashes take absolute (row, key) indices: skipping a chunk
// moves no mask bit.

#include "attn_common.h"

#define ATL_SMAX 4096

typedef __attribute__((ext_vector_type(4))) int i32x4;

// Every kernel of this file is compiled without the packed fp32 VALU ops
// (v_pk_mul_f32, v_pk_fma_f32, v_pk_add_f32). With them the compiler packs
// the score loops of the forward into register pairs and the kernel goes
// from 102 VGPRs to 128 with some 3300 spilled registers; zero scratch is a
// requirement here, so the feature is switched off in the source and not
// left to a build flag.
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass does not know the feature
#define ATL_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define ATL_NO_PK_F32
#endif
#define ATL_KERNEL ATL_NO_PK_F32 __global__ __launch_bounds__(256, 4)

// lm / lg made opaque once per chunk. Inside a chunk loop every LDS address
// is loop-invariant; the compiler hoists them all out of the loop and the
// ~50 registers that hold them spill. Addresses built from the opaque copies
// are recomputed per chunk, which is what the S <= 128 kernels pay once.
// Global indices (hashes, masks, rows) keep the plain lm / lg.
DEV void atl_chunk_lanes(int& lmc, int& lgc, int lm, int lg) {
  lmc = lm;
  lgc = lg;
  asm volatile("" : "+v"(lmc), "+v"(lgc));
}

// two adjacent transposed score tiles (2*kp, 2*kp + 1) of a [128][64] sw7
// image: att_score_tile_t restricted to one pair, so that only the pair is
// live while its dS goes into the next MFMA. Tiles >= nt keep their zeros.
DEV void atl_score_pair_t(f32x4 (&acc)[2], const bf16x8 (&b)[2], char* lds,
                          int off, int kp, int nt, int lm, int lg) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (2 * kp + t >= nt) continue;
    const int tok = (2 * kp + t) * 16 + lm;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 at = *(const bf16x8*)lds_at(
          lds, swz(off + tok * 128 + (ks * 32 + lg * 8) * 2, tok, 7));
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at, b[ks], acc[t], 0, 0, 0);
    }
  }
}

// the lane's hashes for chunk kc: z[r][half] covers keys
// kc*128 + half*64 + (mt & 3)*16 + lg*4 + r, read as att_drop_keep(z[r], mt)
DEV void atl_drop_hash_chunk(uint64_t (&z)[4][2], uint64_t seed, int bh, int S,
                             int q, int lg, int kc) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    z[r][0] = att_drop_hash_c64(seed, bh, S, q, lg * 4 + r, kc * 2);
    z[r][1] = att_drop_hash_c64(seed, bh, S, q, lg * 4 + r, kc * 2 + 1);
  }
}

// SEG: the segment ids of the 128-key chunk at k0 in the LDS slot of the
// fp32 key mask, as int32; keys >= S repeat key S-1 (atl_seg_mask4 nulls
// them by position)
DEV void atl_seg_ids_lds_at(int* sk, const int* __restrict__ ids, int b, int S,
                            int k0, int tid) {
  if (tid < ATT_SMAX) {
    const int key = k0 + tid;
    sk[tid] = ids[(size_t)b * S + (key < S ? key : S - 1)];
  }
}
// the additive mask of tile mt's four keys lg*4.. against the lane's own id:
// 0 for the same segment, -3e38 (the out-of-range key value) for another
// segment and for chunk positions >= nk
DEV f32x4 atl_seg_mask4(const int* sk, int mt, int lg, int own, int nk) {
  const i32x4 id = *(const i32x4*)(sk + mt * 16 + lg * 4);
  f32x4 mv;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    mv[r] = (id[r] == own && mt * 16 + lg * 4 + r < nk) ? 0.f : -3.0e38f;
  return mv;
}
// SEG: the chunk range [c0, c1) of 64-token block blk of batch row b, from
// the bounds table [B][QB][lo, hi); clamped to the row, so that no table
// content can send a walk out of bounds
DEV void atl_seg_chunks(int& c0, int& c1, const int* __restrict__ bounds,
                        int b, int QB, int blk, int NCH) {
  const int* bd = bounds + ((size_t)b * QB + blk) * 2;
  const int lo = bd[0], hi = bd[1];
  c0 = lo > 0 ? lo / 128 : 0;
  c1 = (hi + 127) / 128;
  c1 = c1 < NCH ? c1 : NCH;
}

// ---------------------------------------------------------------------------
// Forward. One block per (b, h, 64-query block), a wave owns 16 queries
// (fragments from global). LDS: K chunk @0, V chunk @16K, the chunk's key
// mask fp32 @32K: 33 KB, four blocks per CU, single-buffered: co-resident
// blocks cover each other's load phase.
#define ATL_K_OFF KR_IMG0_OFF
#define ATL_V_OFF KR_IMG1_OFF
#define ATL_MASK_OFF KR_AUX_OFF
#define ATL_FWD_LDS (KR_AUX_OFF + 512)

// The chunk range of 64-token block blk under the triangle, cut from [c0, c1):
// a query block ends with the chunk that holds its last query (the chunks past
// its diagonal are never staged), a key block begins with the chunk that holds
// its first key. Block-uniform: the chunk loops hold barriers.
DEV int atl_tri_last_chunk(int c1, int blk) {
  const int d = (blk * 64 + 63) / 128 + 1;
  return c1 < d ? c1 : d;
}
DEV int atl_tri_first_chunk(int c0, int blk) {
  const int d = blk * 64 / 128;
  return c0 > d ? c0 : d;
}
// the tiles of a chunk a wave visits: up to the one that holds its first
// query, rel = 16-aligned query base minus the chunk's first key (>= 0)
DEV int atl_tri_tiles(int nt, int rel) {
  const int d = (rel >> 4) + 1;
  return nt < d ? nt : d;
}

// SEG: mask points at the int32 segment ids [B][S], bounds at the table.
// CAUSAL (no additive mask, with or without SEG): q sees k iff k <= q. The
// block stops at its diagonal chunk, and inside it a wave stops at its own
// diagonal tile; without ids neither mask nor bounds is read.
template <bool HAS_MASK, bool SEG = false, bool CAUSAL = false>
ATL_KERNEL void attn_fwd_long_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ mask,
    ushort_t* __restrict__ out, float* __restrict__ m_io,
    float* __restrict__ l_io, int B, int S, int h, float scale, float keep,
    uint64_t salt, const unsigned long long* __restrict__ state,
    const int* __restrict__ bounds) {
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
  const int NCH = (S + 127) / 128;
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* qbase = qkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
  const ushort_t* kbase = qbase + (size_t)h * ATT_D;
  const ushort_t* vbase = qbase + (size_t)2 * h * ATT_D;
  float* mk = (float*)lds_at(lds, ATL_MASK_OFF);

  const int qtok_base = qb * 64 + w * 16;
  const bool active = qtok_base < S;  // wave-uniform
  const int q = qtok_base + lm;       // this lane's query
  const int qc = q < S ? q : S - 1;
  bf16x8 bq[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
    bq[ks] = *(const bf16x8*)(qbase + (size_t)qc * ts + ks * 32 + lg * 8);
  const int* ids = (const int*)mask;
  int kc0 = 0, kc1 = NCH, qid = 0;
  if constexpr (SEG) {
    atl_seg_chunks(kc0, kc1, bounds, b, QB, qb, NCH);
    qid = ids[(size_t)b * S + qc];
  }
  static_assert(!CAUSAL || !HAS_MASK, "causal mode takes no additive mask");
  if constexpr (CAUSAL) kc1 = atl_tri_last_chunk(kc1, qb);

  // Chunk 0 always holds key 0 and additive masks are finite (-10000), so m
  // is a real score after chunk 0. Before it, m = -3e38 gives alpha =
  // exp(-3e38 - m_new) = 0 against l = 0 and O = 0; later, a jump of m by
  // 1e4 (a chunk of masked keys followed by a visible one) gives alpha = 0
  // as well, which is the correct weight of the terms so far.
  // SEG: the walk may start past chunk 0, and a lane can meet chunks with no
  // key of its segment before its run begins (the block's range starts at
  // the run of its FIRST token). There every score is exactly -3e38, m_new
  // stays at the finite -3e38 (alpha = exp(0) = 1 against l = 0 and O = 0),
  // and the exponent base is held at >= -1e30, so p = exp(-3e38 + 1e30) is
  // an exact 0 where exp(-3e38 - m_new) would be 1: l and oacc reach the
  // lane's first visible chunk as exact zeros, and no inf - inf can form
  // because m is never infinite. With a visible key m_new is a real score
  // and the clamp does nothing.
  // CAUSAL without ids: the walk starts at chunk 0, whose key 0 every query
  // sees, so m is a real score after it as in the dense case; every later
  // chunk the block visits starts at or before the block's first query, so
  // no lane ever meets a chunk without a visible key, and the keys above the
  // diagonal are -3e38 against a real m: exact zeros. With ids the SEG
  // argument applies unchanged: the triangle only removes keys, the lane's
  // own key (the diagonal) is in its run and in the walk, and a chunk left
  // with no visible key is the case the clamp covers.
  float m = -3.0e38f, lsum = 0.f;
  f32x4 oacc[4];
  att_zero(oacc);

#pragma clang loop unroll(disable)
  for (int kc = kc0; kc < kc1; ++kc) {
    const int k0 = kc * 128;
    const int nk = S - k0 < 128 ? S - k0 : 128;
    const int NT = (nk + 15) / 16;
    const int NP = (nk + 31) / 32;  // key-tile pairs = PV contraction steps
    if (kc != kc0) __syncthreads();  // every wave is done with the last chunk
    // whole tile pairs are staged; tokens >= S re-read token S-1, finite
    // values that the -3e38 mask (scores) and the zero P (PV) null
    att_glds_rows(kbase, ts, k0, NP * 32, true, S, lds, ATL_K_OFF, tid);
    att_glds_rows(vbase, ts, k0, NP * 32, true, S, lds, ATL_V_OFF, tid);
    if constexpr (SEG) atl_seg_ids_lds_at((int*)mk, ids, b, S, k0, tid);
    else if constexpr (!CAUSAL) att_mask_keys_lds_at(mk, HAS_MASK, mask, b, S, k0, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) continue;
    int lmc, lgc;
    atl_chunk_lanes(lmc, lgc, lm, lg);
    // CAUSAL: the wave's tiles end with its diagonal tile (wave-uniform; NT
    // again in every chunk before the diagonal one); a skipped tile keeps
    // att_zero's zeros through to the PV pair that holds it
    const int NTw = CAUSAL ? atl_tri_tiles(NT, qtok_base - k0) : NT;
    const int NPw = CAUSAL ? (NTw + 1) >> 1 : NP;

    f32x4 sacc[8];
    att_zero(sacc);
    att_score_tile_t(sacc, bq, lds, ATL_K_OFF, NTw, lmc, lgc);
    float mx = -3.0e38f;
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
      if (mt >= NTw) continue;
      f32x4 mv;
      if constexpr (CAUSAL)
        mv = att_tri_mask4<SEG>((const int*)mk, mt, lgc, qid, q - k0, nk);
      else if constexpr (SEG) mv = atl_seg_mask4((const int*)mk, mt, lgc, qid, nk);
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
    const float m_exp = SEG ? fmaxf(m_new, -1.0e30f) : m_new;
    uint64_t z[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    if (keep < 1.f) atl_drop_hash_chunk(z, seed, bh, S, q, lg, kc);
    // unnormalised p (the sum takes it before dropout), dropped in place;
    // keys >= S come out as exact zeros
    float sm = 0.f;
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
      if (mt >= NTw) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = __expf(sacc[mt][r] - m_exp);
        sm += p;
        if (keep < 1.f) p = att_drop_keep(z[r], mt, keep16) ? p * inv_keep : 0.f;
        sacc[mt][r] = p;
      }
    }
    sm += __shfl_xor(sm, 16, 64);
    sm += __shfl_xor(sm, 32, 64);
    lsum = lsum * alpha + sm;
    // the O^T column lm is this lane's query: the rescale is lane-local
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) oacc[ct] *= alpha;
    // O^T += V^T Pd^T: B = the score registers, A = V^T by tr16
#pragma unroll
    for (int kp = 0; kp < 4; ++kp) {
      if (kp >= NPw) continue;
      const bf16x8 bp = att_pack_dpair(sacc[2 * kp], sacc[2 * kp + 1]);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const bf16x8 av = abf_tr_rows64_2(lds, ATL_V_OFF, kp * 32 + lgc * 4,
                                          kp * 32 + 16 + lgc * 4, ct * 4, lmc);
        oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bp, oacc[ct], 0, 0, 0);
      }
    }
  }
  if (!active) return;
  const float inv = 1.f / lsum;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) oacc[ct] *= inv;
  if (lg == 0 && q < S) {
    m_io[(size_t)bh * S + q] = m;
    l_io[(size_t)bh * S + q] = lsum;
  }
  ushort_t* obase = out + ((size_t)b * S * h + hh) * ATT_D;
  att_store_cols16(obase, h * ATT_D, oacc, qtok_base, S, lm, lg);
}

// ---------------------------------------------------------------------------
// Backward dQ. One block per (b, h, 64-query block); K and V come in chunks
// as in the forward. Per pair of key tiles: S^T and dPd^T, P from the saved
// statistics, dS^T over the scores, dQ^T += K^T dS^T; only the pair is live.
// Writes dot[bh*S + q] for the dK/dV kernel; with DBIAS the block's 64 dQ
// column sums go to slab b*QB + qb. LDS as the forward + DBIAS sums @32.5K.
#define ATL_SUM_OFF (KR_AUX_OFF + 512)
#define ATL_DQ_LDS (KR_AUX_OFF + 512 + 1024)

template <bool HAS_MASK, bool DBIAS, bool SEG = false, bool CAUSAL = false>
ATL_KERNEL void attn_bwd_dq_long_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ dout,
    const ushort_t* __restrict__ out, const ushort_t* __restrict__ mask,
    const float* __restrict__ m_io, const float* __restrict__ l_io,
    float* __restrict__ dot_out, ushort_t* __restrict__ dqkv, int B, int S,
    int h, float scale, float keep, uint64_t salt,
    const unsigned long long* __restrict__ state, float* __restrict__ dbscr,
    const int* __restrict__ bounds) {
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
  const int NCH = (S + 127) / 128;
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* qbase = qkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
  const ushort_t* kbase = qbase + (size_t)h * ATT_D;
  const ushort_t* vbase = qbase + (size_t)2 * h * ATT_D;
  const ushort_t* dobase = dout + ((size_t)b * S * h + hh) * ATT_D;
  const ushort_t* obase = out + ((size_t)b * S * h + hh) * ATT_D;
  float* mk = (float*)lds_at(lds, ATL_MASK_OFF);

  const int qtok_base = qb * 64 + w * 16;
  const bool active = qtok_base < S;
  const int q = qtok_base + lm;  // this lane's query
  const int qc = q < S ? q : S - 1;

  bf16x8 bq[2], bdo[2];
  // dot[q] = sum_j dO[q,j] * O[q,j] as the diagonal of the wave's 16 x 16
  // tile O dO^T, from the same MFMA and in the same order over j as
  // dPd^T = V dO^T below. A VALU sum of the 64 products differs from the
  // MFMA's in the last bits; where one key holds all of a row's weight
  // (O = that key's V row) dP - dot must cancel exactly, and it does only if
  // both come out of the same arithmetic.
  f32x4 dd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bq[ks] = *(const bf16x8*)(qbase + (size_t)qc * ts + ks * 32 + lg * 8);
    bdo[ks] = *(const bf16x8*)(dobase + (size_t)qc * dots + ks * 32 + lg * 8);
    const bf16x8 ao = *(const bf16x8*)(obase + (size_t)qc * dots + ks * 32 + lg * 8);
    dd = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ao, bdo[ks], dd, 0, 0, 0);
  }
  // element (lm, lm) is register lm & 3 of the lane (lg = lm >> 2, lm)
  const float dsel = (lm & 2) ? ((lm & 1) ? dd[3] : dd[2]) : ((lm & 1) ? dd[1] : dd[0]);
  const float dot = __shfl(dsel, ((lm >> 2) << 4) | lm, 64);
  if (active && lg == 0 && q < S) dot_out[(size_t)bh * S + q] = dot;
  const float mrow = m_io[(size_t)bh * S + qc];
  const float lrow = 1.f / l_io[(size_t)bh * S + qc];
  // SEG: a key of another segment gets the additive -3e38, so P, rebuilt
  // from the saved m and 1/l, is exp(-huge) = 0 and dS with it
  const int* ids = (const int*)mask;
  int kc0 = 0, kc1 = NCH, qid = 0;
  if constexpr (SEG) {
    atl_seg_chunks(kc0, kc1, bounds, b, QB, qb, NCH);
    qid = ids[(size_t)b * S + qc];
  }
  static_assert(!CAUSAL || !HAS_MASK, "causal mode takes no additive mask");
  if constexpr (CAUSAL) kc1 = atl_tri_last_chunk(kc1, qb);

  f32x4 qacc[4];
  att_zero(qacc);
#pragma clang loop unroll(disable)
  for (int kc = kc0; kc < kc1; ++kc) {
    const int k0 = kc * 128;
    const int nk = S - k0 < 128 ? S - k0 : 128;
    const int NT = (nk + 15) / 16;
    const int NP = (nk + 31) / 32;
    if (kc != kc0) __syncthreads();
    att_glds_rows(kbase, ts, k0, NP * 32, true, S, lds, ATL_K_OFF, tid);
    att_glds_rows(vbase, ts, k0, NP * 32, true, S, lds, ATL_V_OFF, tid);
    if constexpr (SEG) atl_seg_ids_lds_at((int*)mk, ids, b, S, k0, tid);
    else if constexpr (!CAUSAL) att_mask_keys_lds_at(mk, HAS_MASK, mask, b, S, k0, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) continue;
    int lmc, lgc;
    atl_chunk_lanes(lmc, lgc, lm, lg);
    // CAUSAL: tiles and pairs up to the wave's diagonal tile, as the forward
    const int NTw = CAUSAL ? atl_tri_tiles(NT, qtok_base - k0) : NT;
    const int NPw = CAUSAL ? (NTw + 1) >> 1 : NP;

    uint64_t z[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    if (keep < 1.f) atl_drop_hash_chunk(z, seed, bh, S, q, lg, kc);
#pragma unroll
    for (int kp = 0; kp < 4; ++kp) {
      if (kp >= NPw) continue;
      f32x4 s2[2], d2[2];
      atl_score_pair_t(s2, bq, lds, ATL_K_OFF, kp, NTw, lmc, lgc);   // K Q^T
      atl_score_pair_t(d2, bdo, lds, ATL_V_OFF, kp, NTw, lmc, lgc);  // V dO^T
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int mt = 2 * kp + t;
        if (mt >= NTw) continue;  // s2[t] stays zero: a null dS tile
        f32x4 mv;
        if constexpr (CAUSAL)
          mv = att_tri_mask4<SEG>((const int*)mk, mt, lgc, qid, q - k0, nk);
        else if constexpr (SEG) mv = atl_seg_mask4((const int*)mk, mt, lgc, qid, nk);
        else mv = att_mask_keys4(mk, mt, lgc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + mt * 16 + lg * 4 + r;
          const float p = att_prob(s2[t][r], scale, mv[r], mrow, lrow,
                                   q < S && key < S);
          float dp = d2[t][r];
          if (keep < 1.f)
            dp = att_drop_keep(z[r], mt, keep16) ? dp * inv_keep : 0.f;
          s2[t][r] = scale * p * (dp - dot);
        }
      }
      const bf16x8 bds = att_pack_dpair(s2[0], s2[1]);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const bf16x8 ak = abf_tr_rows64_2(lds, ATL_K_OFF, kp * 32 + lgc * 4,
                                          kp * 32 + 16 + lgc * 4, ct * 4, lmc);
        qacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak, bds, qacc[ct], 0, 0, 0);
      }
    }
  }
  float cs = 0.f;
  if (active) {
    ushort_t* dq = dqkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
    att_store_cols16(dq, ts, qacc, qtok_base, S, lm, lg);
    if constexpr (DBIAS) cs = att_colsum_cols16(qacc, qtok_base, S, lm);
  }
  if constexpr (DBIAS) {
    // inactive waves contribute their zeros and must reach the barrier too
    float* wsum = (float*)lds_at(lds, ATL_SUM_OFF);  // [4 waves][64 cols]
    wsum[w * 64 + att_colsum_cols16_col(lm, lg)] = cs;
    __syncthreads();
    if (tid < 64)
      dbscr[((size_t)b * QB + qb) * ts + (size_t)hh * ATT_D + tid] =
          (wsum[tid] + wsum[64 + tid]) + (wsum[128 + tid] + wsum[192 + tid]);
  }
}

// ---------------------------------------------------------------------------
// Backward dK/dV. One block per (b, h, 64-key block), launched after the dQ
// kernel (it reads dot). A wave owns 16 keys, K and V fragments from global;
// dK^T and dV^T stay in registers while the queries go by in chunks of 128:
// Q and dO images, m | 1/l | dot and the chunk's keep bits in LDS, and inside
// a chunk pairs of 16-row tiles as in attn_bwd_dkv_krows_kernel. With DBIAS
// the dK and dV column sums go to slab b*QB + kb.
// LDS: Q chunk @0, dO chunk @16K, m | 1/l | dot fp32 [128] each @32K, keep
// bits (att_drop_bits_lds_long) @33.5K, DBIAS sums [4][dK 64 | dV 64] @35.5K.
#define ATL_Q_OFF KR_IMG0_OFF
#define ATL_DO_OFF KR_IMG1_OFF
#define ATL_STAT_OFF KR_AUX_OFF
#define ATL_BITS_OFF (KR_AUX_OFF + 1536)
#define ATL_SUM2_OFF (KR_AUX_OFF + 1536 + 2048)
#define ATL_DKV_LDS (KR_AUX_OFF + 1536 + 2048 + 2048)
// SEG: the chunk's query ids, int32 [128], one more word array @37.5K
#define ATL_QID_OFF ATL_DKV_LDS
#define ATL_DKV_SEG_LDS (ATL_DKV_LDS + 512)

template <bool HAS_MASK, bool DBIAS, bool SEG = false, bool CAUSAL = false>
ATL_KERNEL void attn_bwd_dkv_long_kernel(
    const ushort_t* __restrict__ qkv, const ushort_t* __restrict__ dout,
    const ushort_t* __restrict__ mask, const float* __restrict__ m_io,
    const float* __restrict__ l_io, const float* __restrict__ dot_in,
    ushort_t* __restrict__ dqkv, int B, int S, int h, float scale, float keep,
    uint64_t salt, const unsigned long long* __restrict__ state,
    float* __restrict__ dbscr, const int* __restrict__ bounds) {
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
  const int NCH = (S + 127) / 128;
  const uint64_t seed = rng_seed(salt, state);
  const float inv_keep = 1.f / keep;
  const unsigned keep16 = keep_to_16(keep);

  const ushort_t* qbase = qkv + (size_t)b * S * ts + (size_t)hh * ATT_D;
  const ushort_t* kbase = qbase + (size_t)h * ATT_D;
  const ushort_t* vbase = qbase + (size_t)2 * h * ATT_D;
  const ushort_t* dobase = dout + ((size_t)b * S * h + hh) * ATT_D;
  float* st = (float*)lds_at(lds, ATL_STAT_OFF);
  unsigned char* bits = (unsigned char*)lds_at(lds, ATL_BITS_OFF);

  const int ktok_base = kb * 64 + w * 16;
  const bool active = ktok_base < S;
  const int key = ktok_base + lm;  // this lane's key
  const int kc = key < S ? key : S - 1;

  bf16x8 bk[2], bv[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bk[ks] = *(const bf16x8*)(kbase + (size_t)kc * ts + ks * 32 + lg * 8);
    bv[ks] = *(const bf16x8*)(vbase + (size_t)kc * ts + ks * 32 + lg * 8);
  }
  float mv = 0.f;
  if (HAS_MASK && key < S) mv = bf16_to_f32(mask[(size_t)b * S + key]);
  if (key >= S) mv = -3.0e38f;
  // SEG: the query chunks of key block kb's range; the lane's key id from
  // global, as the key mask above
  const int* ids = (const int*)mask;
  int* sq = (int*)lds_at(lds, ATL_QID_OFF);
  int qc0 = 0, qc1 = NCH, kid = 0;
  if constexpr (SEG) {
    atl_seg_chunks(qc0, qc1, bounds, b, QB, kb, NCH);
    kid = ids[(size_t)b * S + kc];
  }
  static_assert(!CAUSAL || !HAS_MASK, "causal mode takes no additive mask");
  // CAUSAL: the key block's queries begin in the chunk that holds its first key
  if constexpr (CAUSAL) qc0 = atl_tri_first_chunk(qc0, kb);

  f32x4 kacc[4], vacc[4];
  att_zero(kacc);
  att_zero(vacc);
#pragma clang loop unroll(disable)
  for (int qch = qc0; qch < qc1; ++qch) {
    const int q0 = qch * 128;
    const int nq = S - q0 < 128 ? S - q0 : 128;
    const int NT = (nq + 15) / 16;
    const int NP = (nq + 31) / 32;
    if (qch != qc0) __syncthreads();  // the one barrier before LDS is reused
    att_glds_rows(qbase, ts, q0, NP * 32, true, S, lds, ATL_Q_OFF, tid);
    att_glds_rows(dobase, dots, q0, NP * 32, true, S, lds, ATL_DO_OFF, tid);
    // rows >= S: 1/l = 0 and a false valid flag null P, dot = 0 keeps dS finite
    if (tid < ATT_SMAX) {
      const int row = q0 + tid;
      const bool live = row < S;
      st[tid] = live ? m_io[(size_t)bh * S + row] : 0.f;
      st[128 + tid] = live ? 1.f / l_io[(size_t)bh * S + row] : 0.f;
      st[256 + tid] = live ? dot_in[(size_t)bh * S + row] : 0.f;
      if constexpr (SEG) sq[tid] = ids[(size_t)b * S + (live ? row : S - 1)];
    }
    if (keep < 1.f)
      att_drop_bits_lds_long(bits, seed, bh, S, kb, q0, NP * 32, keep16, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) continue;
    int lmc, lgc;
    atl_chunk_lanes(lmc, lgc, lm, lg);
    // CAUSAL: in the diagonal chunk the wave starts at its own tile (0 in
    // every later chunk); wave-uniform, no barrier below
    const int tw0 = CAUSAL && ktok_base > q0 ? (ktok_base - q0) >> 4 : 0;

#pragma unroll
    for (int qp = 0; qp < 4; ++qp) {
      if (qp >= NP) continue;
      if constexpr (CAUSAL) if (qp < tw0 >> 1) continue;
      f32x4 pd[2], ds[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int qt = 2 * qp + t;
        pd[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        ds[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (qt >= NT) continue;
        if constexpr (CAUSAL) if (qt < tw0) continue;
        const int qrow = qt * 16 + lmc;  // < NP*32: a staged (clamped) row
        f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, d4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 aq = *(const bf16x8*)lds_at(
              lds, swz(ATL_Q_OFF + qrow * 128 + (ks * 32 + lgc * 8) * 2, qrow, 7));
          const bf16x8 ado = *(const bf16x8*)lds_at(
              lds, swz(ATL_DO_OFF + qrow * 128 + (ks * 32 + lgc * 8) * 2, qrow, 7));
          s4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq, bk[ks], s4, 0, 0, 0);
          d4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ado, bv[ks], d4, 0, 0, 0);
        }
        const f32x4 m4 = *(const f32x4*)(st + qt * 16 + lgc * 4);
        const f32x4 il4 = *(const f32x4*)(st + 128 + qt * 16 + lgc * 4);
        const f32x4 dot4 = *(const f32x4*)(st + 256 + qt * 16 + lgc * 4);
        unsigned kbits = 0xFFFFFFFFu;
        if (keep < 1.f)
          kbits = *(const unsigned*)(bits + ((qt * 4 + lgc) * 16 + lmc) * 4);
        i32x4 qid4 = {0, 0, 0, 0};
        if constexpr (SEG) qid4 = *(const i32x4*)(sq + qt * 16 + lgc * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qq = q0 + qt * 16 + lg * 4 + r;
          // the lane's token is the key here: the triangle compare turns round
          const float mvr = ((SEG && qid4[r] != kid) || (CAUSAL && qq < key))
                                ? -3.0e38f : mv;
          const float p = att_prob(s4[r], scale, mvr, m4[r], il4[r],
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
        const bf16x8 adot = abf_tr_rows64_2(lds, ATL_DO_OFF, qp * 32 + lgc * 4,
                                            qp * 32 + 16 + lgc * 4, ct * 4, lmc);
        vacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(adot, bpd, vacc[ct], 0, 0, 0);
        const bf16x8 aqt = abf_tr_rows64_2(lds, ATL_Q_OFF, qp * 32 + lgc * 4,
                                           qp * 32 + 16 + lgc * 4, ct * 4, lmc);
        kacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aqt, bds, kacc[ct], 0, 0, 0);
      }
    }
  }
  float ck = 0.f, cv = 0.f;
  if (active) {
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
    float* wsum = (float*)lds_at(lds, ATL_SUM2_OFF);  // [4][dK 64 | dV 64]
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

// ---------------------------------------------------------------------------
// Entry points: d = 64 and 128 < S <= 4096 only (S <= 128 belongs to
// sky_attn_fwd / sky_attn_bwd*).
static bool atl_shape_ok(int64_t S, int64_t d) {
  return d == ATT_D && S > ATT_SMAX && S <= ATL_SMAX;
}

SKY_EXPORT int sky_attn_long_fwd(uint64_t stream, uint64_t qkv, uint64_t mask,
                                 uint64_t out, uint64_t m, uint64_t lsum,
                                 int64_t B, int64_t S, int64_t h, int64_t d,
                                 float scale, float keep, uint64_t salt,
                                 uint64_t state) {
  if (!atl_shape_ok(S, d)) return (int)hipErrorInvalidValue;
  dim3 grid((unsigned)(B * h * ((S + 63) / 64)));
  ATT_LAUNCH_HM(mask != 0, (attn_fwd_long_kernel<HM>), grid, ATL_FWD_LDS,
                (hipStream_t)stream, (const ushort_t*)qkv,
                (const ushort_t*)mask, (ushort_t*)out, (float*)m, (float*)lsum,
                (int)B, (int)S, (int)h, scale, keep, salt,
                (const unsigned long long*)state, (const int*)nullptr);
  LAUNCH_CHECK();
  return 0;
}

// dQ + dot, then dK/dV; DBIAS also fills the column-partial slabs
template <bool DBIAS>
static void launch_attn_long_bwd(hipStream_t s, uint64_t qkv, uint64_t dout,
                                 uint64_t out, uint64_t mask, uint64_t m,
                                 uint64_t lsum, uint64_t dot, uint64_t dqkv,
                                 int64_t B, int64_t S, int64_t h, float scale,
                                 float keep, uint64_t salt, uint64_t state,
                                 float* dbscr) {
  dim3 grid((unsigned)(B * h * ((S + 63) / 64)));
  ATT_LAUNCH_HM(mask != 0, (attn_bwd_dq_long_kernel<HM, DBIAS>), grid,
                ATL_DQ_LDS, s, (const ushort_t*)qkv, (const ushort_t*)dout,
                (const ushort_t*)out, (const ushort_t*)mask, (const float*)m,
                (const float*)lsum, (float*)dot, (ushort_t*)dqkv, (int)B,
                (int)S, (int)h, scale, keep, salt,
                (const unsigned long long*)state, dbscr, (const int*)nullptr);
  ATT_LAUNCH_HM(mask != 0, (attn_bwd_dkv_long_kernel<HM, DBIAS>), grid,
                ATL_DKV_LDS, s, (const ushort_t*)qkv, (const ushort_t*)dout,
                (const ushort_t*)mask, (const float*)m, (const float*)lsum,
                (const float*)dot, (ushort_t*)dqkv, (int)B, (int)S, (int)h,
                scale, keep, salt, (const unsigned long long*)state, dbscr,
                (const int*)nullptr);
}

// out: the forward's output [B,S,h,d]; dot: fp32 [B*h*S], written by the
// dQ kernel and read by the dK/dV kernel.
SKY_EXPORT int sky_attn_long_bwd(uint64_t stream, uint64_t qkv, uint64_t dout,
                                 uint64_t out, uint64_t mask, uint64_t m,
                                 uint64_t lsum, uint64_t dot, uint64_t dqkv,
                                 int64_t B, int64_t S, int64_t h, int64_t d,
                                 float scale, float keep, uint64_t salt,
                                 uint64_t state) {
  if (!atl_shape_ok(S, d) || out == 0 || dot == 0)
    return (int)hipErrorInvalidValue;
  launch_attn_long_bwd<false>((hipStream_t)stream, qkv, dout, out, mask, m,
                              lsum, dot, dqkv, B, S, h, scale, keep, salt,
                              state, nullptr);
  LAUNCH_CHECK();
  return 0;
}

// sky_attn_long_bwd that also returns dbias[3*h*64], the column sums of dqkv
// as stored; scratch: fp32 [B * ceil(S/64)][3*h*64], every element written.
// job == nullptr: the slab reduction runs here; otherwise it is left
// pending in *job (as attn_bwd_dbias_impl, attention_bwd.hip).
static int attn_long_bwd_dbias_impl(uint64_t stream, uint64_t qkv,
                                    uint64_t dout, uint64_t out, uint64_t mask,
                                    uint64_t m, uint64_t lsum, uint64_t dot,
                                    uint64_t dqkv, int64_t B, int64_t S,
                                    int64_t h, int64_t d, float scale,
                                    float keep, uint64_t salt, uint64_t state,
                                    uint64_t scratch, uint64_t dbias,
                                    int dbias_dt, SkyFinishJob* job) {
  if (!atl_shape_ok(S, d) || out == 0 || dot == 0 || scratch == 0 || dbias == 0)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  launch_attn_long_bwd<true>(s, qkv, dout, out, mask, m, lsum, dot, dqkv, B, S,
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

SKY_EXPORT int sky_attn_long_bwd_dbias(
    uint64_t stream, uint64_t qkv, uint64_t dout, uint64_t out, uint64_t mask,
    uint64_t m, uint64_t lsum, uint64_t dot, uint64_t dqkv, int64_t B,
    int64_t S, int64_t h, int64_t d, float scale, float keep, uint64_t salt,
    uint64_t state, uint64_t scratch, uint64_t dbias, int dbias_dt) {
  return attn_long_bwd_dbias_impl(stream, qkv, dout, out, mask, m, lsum, dot,
                                  dqkv, B, S, h, d, scale, keep, salt, state,
                                  scratch, dbias, dbias_dt, nullptr);
}

SKY_EXPORT int sky_attn_long_bwd_dbias_parts(
    uint64_t stream, uint64_t qkv, uint64_t dout, uint64_t out, uint64_t mask,
    uint64_t m, uint64_t lsum, uint64_t dot, uint64_t dqkv, int64_t B,
    int64_t S, int64_t h, int64_t d, float scale, float keep, uint64_t salt,
    uint64_t state, uint64_t scratch, uint64_t dbias, int dbias_dt,
    uint64_t job) {
  if (job == 0) return (int)hipErrorInvalidValue;
  ((SkyFinishJob*)job)->nv = 0;
  return attn_long_bwd_dbias_impl(stream, qkv, dout, out, mask, m, lsum, dot,
                                  dqkv, B, S, h, d, scale, keep, salt, state,
                                  scratch, dbias, dbias_dt, (SkyFinishJob*)job);
}

// ---------------------------------------------------------------------------
// Segment bounds. One block per batch row; thread t owns tokens 16t..16t+15
// (S <= 4096). A neighbour compare marks run starts and run ends; the latest
// start at or before a token is a prefix-max over positions, the earliest end
// after it a suffix-min, both scanned over the 256 thread totals in LDS.
// bounds[b][blk] = {run start of token 64*blk, run end (exclusive) of token
// min(64*blk + 63, S - 1)}: 0 <= lo <= 64*blk < hi <= S for any ids.
ATL_NO_PK_F32 __global__ __launch_bounds__(256) void attn_seg_bounds_kernel(
    const int* __restrict__ ids, int* __restrict__ bounds, int S) {
  __shared__ int pmax[256], smin[256];
  const int tid = threadIdx.x;
  const int* row = ids + (size_t)blockIdx.x * S;
  int tmax = 0, tmin = S;  // the identities: token 0 starts a run, S - 1 ends one
  for (int i = tid * 16; i < tid * 16 + 16 && i < S; ++i) {
    const int id = row[i];
    if (i > 0 && row[i - 1] != id) tmax = i;  // ascending: the last one stays
    if (tmin == S && i + 1 < S && row[i + 1] != id) tmin = i + 1;
  }
  pmax[tid] = tmax;
  smin[tid] = tmin;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int a = tid >= off ? pmax[tid - off] : 0;
    const int c = tid + off < 256 ? smin[tid + off] : S;
    __syncthreads();
    pmax[tid] = pmax[tid] > a ? pmax[tid] : a;
    smin[tid] = smin[tid] < c ? smin[tid] : c;
    __syncthreads();
  }
  const int QB = (S + 63) / 64;
  if (tid < QB) {
    // block tid = tokens f..e, threads 4*tid..4*tid + 3
    const int f = tid * 64;
    const int e = f + 63 < S ? f + 63 : S - 1;
    int lo = f, hi = e + 1;
    if (f > 0 && row[f - 1] == row[f]) lo = pmax[4 * tid - 1];
    if (e + 1 < S && row[e + 1] == row[e]) hi = smin[4 * tid + 4];
    int* bd = bounds + ((size_t)blockIdx.x * QB + tid) * 2;
    bd[0] = lo;
    bd[1] = hi;
  }
}

// ids: int32 [B][S]; bounds: int32 [B][ceil(S/64)][2], every element written
SKY_EXPORT int sky_attn_seg_bounds(uint64_t stream, uint64_t ids,
                                   uint64_t bounds, int64_t B, int64_t S) {
  if (!atl_shape_ok(S, ATT_D) || ids == 0 || bounds == 0)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_seg_bounds_kernel, dim3((unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, (const int*)ids, (int*)bounds, (int)S);
  LAUNCH_CHECK();
  return 0;
}

// The segment forms of sky_attn_long_fwd / sky_attn_long_bwd: ids in the
// place of the additive mask, bounds from sky_attn_seg_bounds on the same ids.
SKY_EXPORT int sky_attn_long_seg_fwd(uint64_t stream, uint64_t qkv,
                                     uint64_t ids, uint64_t bounds,
                                     uint64_t out, uint64_t m, uint64_t lsum,
                                     int64_t B, int64_t S, int64_t h, int64_t d,
                                     float scale, float keep, uint64_t salt,
                                     uint64_t state) {
  if (!atl_shape_ok(S, d) || ids == 0 || bounds == 0)
    return (int)hipErrorInvalidValue;
  dim3 grid((unsigned)(B * h * ((S + 63) / 64)));
  hipLaunchKernelGGL((attn_fwd_long_kernel<false, true>), grid, dim3(256),
                     ATL_FWD_LDS, (hipStream_t)stream, (const ushort_t*)qkv,
                     (const ushort_t*)ids, (ushort_t*)out, (float*)m,
                     (float*)lsum, (int)B, (int)S, (int)h, scale, keep, salt,
                     (const unsigned long long*)state, (const int*)bounds);
  LAUNCH_CHECK();
  return 0;
}

// the segment pair: dQ + dot, then dK/dV; DBIAS also fills the slabs.
// CAUSAL: the triangle pair, with ids and bounds (SEG) or with neither.
template <bool DBIAS, bool SEG = true, bool CAUSAL = false>
static void launch_attn_long_seg_bwd(hipStream_t s, uint64_t qkv, uint64_t dout,
                                     uint64_t out, uint64_t ids, uint64_t bounds,
                                     uint64_t m, uint64_t lsum, uint64_t dot,
                                     uint64_t dqkv, int64_t B, int64_t S,
                                     int64_t h, float scale, float keep,
                                     uint64_t salt, uint64_t state,
                                     float* dbscr) {
  dim3 grid((unsigned)(B * h * ((S + 63) / 64)));
  hipLaunchKernelGGL((attn_bwd_dq_long_kernel<false, DBIAS, SEG, CAUSAL>), grid,
                     dim3(256), ATL_DQ_LDS, s, (const ushort_t*)qkv,
                     (const ushort_t*)dout, (const ushort_t*)out,
                     (const ushort_t*)ids, (const float*)m, (const float*)lsum,
                     (float*)dot, (ushort_t*)dqkv, (int)B, (int)S, (int)h, scale,
                     keep, salt, (const unsigned long long*)state, dbscr,
                     (const int*)bounds);
  hipLaunchKernelGGL((attn_bwd_dkv_long_kernel<false, DBIAS, SEG, CAUSAL>), grid,
                     dim3(256), SEG ? ATL_DKV_SEG_LDS : ATL_DKV_LDS, s,
                     (const ushort_t*)qkv,
                     (const ushort_t*)dout, (const ushort_t*)ids,
                     (const float*)m, (const float*)lsum, (const float*)dot,
                     (ushort_t*)dqkv, (int)B, (int)S, (int)h, scale, keep, salt,
                     (const unsigned long long*)state, dbscr,
                     (const int*)bounds);
}

SKY_EXPORT int sky_attn_long_seg_bwd(uint64_t stream, uint64_t qkv,
                                     uint64_t dout, uint64_t out, uint64_t ids,
                                     uint64_t bounds, uint64_t m, uint64_t lsum,
                                     uint64_t dot, uint64_t dqkv, int64_t B,
                                     int64_t S, int64_t h, int64_t d,
                                     float scale, float keep, uint64_t salt,
                                     uint64_t state) {
  if (!atl_shape_ok(S, d) || out == 0 || dot == 0 || ids == 0 || bounds == 0)
    return (int)hipErrorInvalidValue;
  launch_attn_long_seg_bwd<false>((hipStream_t)stream, qkv, dout, out, ids,
                                  bounds, m, lsum, dot, dqkv, B, S, h, scale,
                                  keep, salt, state, nullptr);
  LAUNCH_CHECK();
  return 0;
}

// sky_attn_long_seg_bwd that also returns dbias[3*h*64]: the segment forms of
// sky_attn_long_bwd_dbias / _parts, scratch and job as there
static int attn_long_seg_bwd_dbias_impl(
    uint64_t stream, uint64_t qkv, uint64_t dout, uint64_t out, uint64_t ids,
    uint64_t bounds, uint64_t m, uint64_t lsum, uint64_t dot, uint64_t dqkv,
    int64_t B, int64_t S, int64_t h, int64_t d, float scale, float keep,
    uint64_t salt, uint64_t state, uint64_t scratch, uint64_t dbias,
    int dbias_dt, SkyFinishJob* job, bool causal = false) {
  // causal: ids and bounds both set or both 0
  const bool seg = ids != 0 && bounds != 0;
  if (!atl_shape_ok(S, d) || out == 0 || dot == 0 || scratch == 0 ||
      dbias == 0 || (causal ? (ids != 0) != (bounds != 0) : !seg))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (!causal)
    launch_attn_long_seg_bwd<true>(s, qkv, dout, out, ids, bounds, m, lsum, dot,
                                   dqkv, B, S, h, scale, keep, salt, state,
                                   (float*)scratch);
  else if (seg)
    launch_attn_long_seg_bwd<true, true, true>(s, qkv, dout, out, ids, bounds, m,
                                               lsum, dot, dqkv, B, S, h, scale,
                                               keep, salt, state, (float*)scratch);
  else
    launch_attn_long_seg_bwd<true, false, true>(s, qkv, dout, out, 0, 0, m, lsum,
                                                dot, dqkv, B, S, h, scale, keep,
                                                salt, state, (float*)scratch);
  const int64_t cols = 3 * h * ATT_D, nslabs = B * ((S + 63) / 64);
  if (job)
    sky_finish_job_set(job, scratch, dbias, 0, 0, nslabs, cols, 1, dbias_dt);
  else
    sky_launch_colsum_final(s, (const float*)scratch, (void*)dbias, cols,
                            nslabs, dbias_dt);
  LAUNCH_CHECK();
  return 0;
}

SKY_EXPORT int sky_attn_long_seg_bwd_dbias(
    uint64_t stream, uint64_t qkv, uint64_t dout, uint64_t out, uint64_t ids,
    uint64_t bounds, uint64_t m, uint64_t lsum, uint64_t dot, uint64_t dqkv,
    int64_t B, int64_t S, int64_t h, int64_t d, float scale, float keep,
    uint64_t salt, uint64_t state, uint64_t scratch, uint64_t dbias,
    int dbias_dt) {
  return attn_long_seg_bwd_dbias_impl(stream, qkv, dout, out, ids, bounds, m,
                                      lsum, dot, dqkv, B, S, h, d, scale, keep,
                                      salt, state, scratch, dbias, dbias_dt,
                                      nullptr);
}

SKY_EXPORT int sky_attn_long_seg_bwd_dbias_parts(
    uint64_t stream, uint64_t qkv, uint64_t dout, uint64_t out, uint64_t ids,
    uint64_t bounds, uint64_t m, uint64_t lsum, uint64_t dot, uint64_t dqkv,
    int64_t B, int64_t S, int64_t h, int64_t d, float scale, float keep,
    uint64_t salt, uint64_t state, uint64_t scratch, uint64_t dbias,
    int dbias_dt, uint64_t job) {
  if (job == 0) return (int)hipErrorInvalidValue;
  ((SkyFinishJob*)job)->nv = 0;
  return attn_long_seg_bwd_dbias_impl(stream, qkv, dout, out, ids, bounds, m,
                                      lsum, dot, dqkv, B, S, h, d, scale, keep,
                                      salt, state, scratch, dbias, dbias_dt,
                                      (SkyFinishJob*)job);
}

// ---------------------------------------------------------------------------
// The causal forms (q attends k iff k <= q): arguments as the segment forms
// above, but ids and bounds may both be 0 (no packing), which selects the
// SEG = false instantiations; only one of the two set is an error.
static bool atl_causal_ok(int64_t S, int64_t d, uint64_t ids, uint64_t bounds) {
  return atl_shape_ok(S, d) && (ids != 0) == (bounds != 0);
}

SKY_EXPORT int sky_attn_long_causal_fwd(uint64_t stream, uint64_t qkv,
                                        uint64_t ids, uint64_t bounds,
                                        uint64_t out, uint64_t m, uint64_t lsum,
                                        int64_t B, int64_t S, int64_t h,
                                        int64_t d, float scale, float keep,
                                        uint64_t salt, uint64_t state) {
  if (!atl_causal_ok(S, d, ids, bounds)) return (int)hipErrorInvalidValue;
  dim3 grid((unsigned)(B * h * ((S + 63) / 64)));
#define ATLC(SEG)                                                             \
  hipLaunchKernelGGL((attn_fwd_long_kernel<false, SEG, true>), grid,          \
                     dim3(256), ATL_FWD_LDS, (hipStream_t)stream,             \
                     (const ushort_t*)qkv, (const ushort_t*)ids,              \
                     (ushort_t*)out, (float*)m, (float*)lsum, (int)B, (int)S, \
                     (int)h, scale, keep, salt,                               \
                     (const unsigned long long*)state, (const int*)bounds)
  if (ids) ATLC(true); else ATLC(false);
#undef ATLC
  LAUNCH_CHECK();
  return 0;
}

SKY_EXPORT int sky_attn_long_causal_bwd(uint64_t stream, uint64_t qkv,
                                        uint64_t dout, uint64_t out,
                                        uint64_t ids, uint64_t bounds,
                                        uint64_t m, uint64_t lsum, uint64_t dot,
                                        uint64_t dqkv, int64_t B, int64_t S,
                                        int64_t h, int64_t d, float scale,
                                        float keep, uint64_t salt,
                                        uint64_t state) {
  if (!atl_causal_ok(S, d, ids, bounds) || out == 0 || dot == 0)
    return (int)hipErrorInvalidValue;
  if (ids)
    launch_attn_long_seg_bwd<false, true, true>(
        (hipStream_t)stream, qkv, dout, out, ids, bounds, m, lsum, dot, dqkv, B,
        S, h, scale, keep, salt, state, nullptr);
  else
    launch_attn_long_seg_bwd<false, false, true>(
        (hipStream_t)stream, qkv, dout, out, 0, 0, m, lsum, dot, dqkv, B, S, h,
        scale, keep, salt, state, nullptr);
  LAUNCH_CHECK();
  return 0;
}

SKY_EXPORT int sky_attn_long_causal_bwd_dbias(
    uint64_t stream, uint64_t qkv, uint64_t dout, uint64_t out, uint64_t ids,
    uint64_t bounds, uint64_t m, uint64_t lsum, uint64_t dot, uint64_t dqkv,
    int64_t B, int64_t S, int64_t h, int64_t d, float scale, float keep,
    uint64_t salt, uint64_t state, uint64_t scratch, uint64_t dbias,
    int dbias_dt) {
  return attn_long_seg_bwd_dbias_impl(stream, qkv, dout, out, ids, bounds, m,
                                      lsum, dot, dqkv, B, S, h, d, scale, keep,
                                      salt, state, scratch, dbias, dbias_dt,
                                      nullptr, true);
}

SKY_EXPORT int sky_attn_long_causal_bwd_dbias_parts(
    uint64_t stream, uint64_t qkv, uint64_t dout, uint64_t out, uint64_t ids,
    uint64_t bounds, uint64_t m, uint64_t lsum, uint64_t dot, uint64_t dqkv,
    int64_t B, int64_t S, int64_t h, int64_t d, float scale, float keep,
    uint64_t salt, uint64_t state, uint64_t scratch, uint64_t dbias,
    int dbias_dt, uint64_t job) {
  if (job == 0) return (int)hipErrorInvalidValue;
  ((SkyFinishJob*)job)->nv = 0;
  return attn_long_seg_bwd_dbias_impl(stream, qkv, dout, out, ids, bounds, m,
                                      lsum, dot, dqkv, B, S, h, d, scale, keep,
                                      salt, state, scratch, dbias, dbias_dt,
                                      (SkyFinishJob*)job, true);
}
