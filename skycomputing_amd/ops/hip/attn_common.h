// Shared tile math of the attention kernels (attention.hip,
// attention_bwd.hip, attention_flash.hip): types, LDS addressing and one
// DEV helper per block the kernels have in common. All helpers assume the
// kernels' lane split lm = lane & 15 (MFMA column), lg = lane >> 4 (row
// group), 256-thread blocks, d = 64.
#pragma once

#include "common.h"

typedef const __attribute__((address_space(1))) unsigned int* att_gas;
typedef __attribute__((address_space(3))) unsigned int* att_las;

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define ATT_SMAX 128
#define ATT_D 64

// LDS layout shared by the keys-on-rows kernels: two [128][64] sw7 row
// images (K | V in the forward and the dQ kernel, Q | dO in the dK/dV
// kernel), then each kernel's small arrays from KR_AUX_OFF on.
#define KR_IMG0_OFF 0
#define KR_IMG1_OFF (16 * 1024)
#define KR_AUX_OFF (32 * 1024)

DEV void* lds_at(char* base, int byte) { return (void*)(base + byte); }

DEV int swz(int byte_addr, int row, int rmask) {
  return byte_addr ^ ((row & rmask) << 4);
}

typedef __attribute__((ext_vector_type(4))) short s16x4_a;
typedef __attribute__((address_space(3))) s16x4_a* abf_las4;

// tr16 read of an MFMA fragment from a row-major [row][64] sw7 image:
// lane lm indexes the fragment's 16 output columns (cquad base cq0),
// regs j = 4 consecutive image rows starting at r0 + (per-lane s>>2).
DEV bf16x8 abf_tr_rows64(const char* lds_base, int off, int r0, int cq0,
                         int s4) {
  s16x4_a v[2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int row = r0 + half * 4 + (s4 >> 2);
    const int byte = (off + row * 128 + (cq0 + (s4 & 3)) * 8) ^ ((row & 7) << 4);
    v[half] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (abf_las4)(lds_base + byte));
  }
  return (bf16x8){v[0][0], v[0][1], v[0][2], v[0][3],
                  v[1][0], v[1][1], v[1][2], v[1][3]};
}

// The same read with the two halves' row bases given separately: regs
// j = 0..3 are image rows ra.., regs j = 4..7 image rows rb... This is the
// A operand that goes with att_pack_dpair's B operand: for the stacked
// 16-row tiles T0 and T1, ra = T0*16 + lg*4 and rb = T1*16 + lg*4.
DEV bf16x8 abf_tr_rows64_2(const char* lds_base, int off, int ra, int rb,
                           int cq0, int s4) {
  s16x4_a v[2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int row = (half ? rb : ra) + (s4 >> 2);
    const int byte = (off + row * 128 + (cq0 + (s4 & 3)) * 8) ^ ((row & 7) << 4);
    v[half] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (abf_las4)(lds_base + byte));
  }
  return (bf16x8){v[0][0], v[0][1], v[0][2], v[0][3],
                  v[1][0], v[1][1], v[1][2], v[1][3]};
}

// Two stacked MFMA D tiles as the next MFMA's B operand, with no lane
// movement: a D lane holds rows lg*4 .. lg*4+3 of column lm, a B lane holds
// 8 contraction indices of column lm, and the order of those indices is free
// as long as A agrees. Slot (lg, j) stands for contraction index
// (j < 4 ? T0 : T1)*16 + lg*4 + (j & 3); abf_tr_rows64_2 reads the matching
// A operand (tests/test_attn_krows_gpu.py::test_mfma_chain pins both).
DEV bf16x8 att_pack_dpair(const f32x4& t0, const f32x4& t1) {
  const uint4_t v = {f32x2_to_bf16x2(t0[0], t0[1]), f32x2_to_bf16x2(t0[2], t0[3]),
                     f32x2_to_bf16x2(t1[0], t1[1]), f32x2_to_bf16x2(t1[2], t1[3])};
  return __builtin_bit_cast(bf16x8, v);
}

// same for the [64 q][128 k] sw15 tiles (256-B rows)
DEV bf16x8 abf_tr_rows128(const char* lds_base, int off, int r0, int cq0,
                          int s4) {
  s16x4_a v[2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int row = r0 + half * 4 + (s4 >> 2);
    const int byte = (off + (row & 63) * 256 + (cq0 + (s4 & 3)) * 8) ^
                     ((row & 15) << 4);
    v[half] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (abf_las4)(lds_base + byte));
  }
  return (bf16x8){v[0][0], v[0][1], v[0][2], v[0][3],
                  v[1][0], v[1][1], v[1][2], v[1][3]};
}

template <int N> DEV void att_zero(f32x4 (&acc)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// additive mask values for this lane's 8 key columns (col0 + kt*16 + lm);
// columns past S get -3e38 so they vanish from max and sum.
DEV void att_mask_cols(float (&mval)[8], bool has_mask,
                       const ushort_t* __restrict__ mask, int b, int S,
                       int lm, int col0) {
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    const int col = col0 + kt * 16 + lm;
    float mv = 0.f;
    if (has_mask && col < S) mv = bf16_to_f32(mask[(size_t)b * S + col]);
    mval[kt] = (col < S) ? mv : -3.0e38f;
  }
}
template <bool HAS_MASK>
DEV void att_mask_cols(float (&mval)[8], const ushort_t* __restrict__ mask,
                       int b, int S, int lm) {
  att_mask_cols(mval, HAS_MASK, mask, b, S, lm, 0);
}

// reductions over the 16 lanes that share one MFMA output row
DEV float row16_sum(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
DEV float row16_max(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// score tile: acc[kt] += A B^T for the first nt 16-token tiles of a
// [tok][64] sw7 LDS image at byte offset off (A = a 16-row fragment pair)
DEV void att_score_tile(f32x4 (&acc)[8], const bf16x8 (&a)[2], char* lds,
                        int off, int nt, int lm, int lg) {
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    if (kt >= nt) continue;
    const int ktok = kt * 16 + lm;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 bk = *(const bf16x8*)lds_at(
          lds, swz(off + ktok * 128 + (ks * 32 + lg * 8) * 2, ktok, 7));
      acc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], bk, acc[kt], 0, 0, 0);
    }
  }
}

// transposed score tile (keys on the MFMA rows): acc[mt] += T B^T with the
// operands of att_score_tile swapped, A = 16-token tile mt of the LDS image,
// B = the wave's 16-row fragment pair b. A lane then holds tokens
// mt*16 + lg*4 + r of the image against ITS row lm of b.
DEV void att_score_tile_t(f32x4 (&acc)[8], const bf16x8 (&b)[2], char* lds,
                          int off, int nt, int lm, int lg) {
#pragma unroll
  for (int mt = 0; mt < 8; ++mt) {
    if (mt >= nt) continue;
    const int tok = mt * 16 + lm;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 at = *(const bf16x8*)lds_at(
          lds, swz(off + tok * 128 + (ks * 32 + lg * 8) * 2, tok, 7));
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at, b[ks], acc[mt], 0, 0, 0);
    }
  }
}

// keys on rows: the 128 additive key values of batch b as fp32 in LDS
// (keys past S get -3e38), written by threads 0..127 before the staging
// barrier; a lane reads tile mt's four keys lg*4.. with att_mask_keys4.
DEV void att_mask_keys_lds(float* mk, bool has_mask,
                           const ushort_t* __restrict__ mask, int b, int S,
                           int tid) {
  if (tid < ATT_SMAX) {
    float mv = 0.f;
    if (has_mask && tid < S) mv = bf16_to_f32(mask[(size_t)b * S + tid]);
    mk[tid] = (tid < S) ? mv : -3.0e38f;
  }
}
DEV f32x4 att_mask_keys4(const float* mk, int mt, int lg) {
  return *(const f32x4*)(mk + mt * 16 + lg * 4);
}

// stage nrows rows of a [tok][64] bf16 row image (token stride tstride,
// first token tok0) to LDS offset off via global_load_lds. The XOR swizzle
// moves to the SOURCE address (lane-linear LDS image == sw7 layout). With
// clamp, tokens >= S re-read token S-1 (the consumer nulls those rows).
DEV void att_glds_rows(const ushort_t* src, int tstride, int tok0, int nrows,
                       bool clamp, int S, char* lds, int off, int tid) {
  for (int u = tid; u < nrows * 8; u += 256) {
    const int tok = u >> 3;
    int gtok = tok0 + tok;
    if (clamp && gtok >= S) gtok = S - 1;
    const int c16s = (u & 7) ^ (tok & 7);  // pre-swizzled source column
    __builtin_amdgcn_global_load_lds(
        (att_gas)(src + (size_t)gtok * tstride + c16s * 8),
        (att_las)lds_at(lds, off + u * 16), 16, 0, 0);
  }
}

// probability recomputed from the saved row statistics (inv_l = 1 / l)
DEV float att_prob(float s, float scale, float mv, float m, float inv_l,
                   bool valid) {
  float p = __expf(s * scale + mv - m) * inv_l;
  if (!valid) p = 0.f;
  return p;
}

// Dropout of the S <= 128 kernels: lane-local indices, two hashes per
// (row, lane) cover the lane's 8 key tiles (one 16-bit slice per kt).
// The forward, probs mode and EVERY backward must draw their keep bits
// through att_drop_hash + att_drop_keep and nothing else — the mask is
// regenerated, never stored, so a second definition is a silent bug.
// half 0 covers key tiles kt = 0..3, half 1 kt = 4..7
DEV uint64_t att_drop_hash_half(uint64_t seed, int bh, int S, int row, int lm,
                                int half) {
  const uint64_t base = ((uint64_t)bh * S + row) * 16 + lm;
  return rng_hash(seed, base * 2 + half);
}
DEV void att_drop_hash(uint64_t (&z)[2], uint64_t seed, int bh, int S,
                       int row, int lm) {
  z[0] = att_drop_hash_half(seed, bh, S, row, lm, 0);
  z[1] = att_drop_hash_half(seed, bh, S, row, lm, 1);
}
DEV bool att_drop_keep(const uint64_t (&z)[2], int kt, unsigned keep16) {
  const uint64_t zz = kt < 4 ? z[0] : z[1];
  return (unsigned)((zz >> (16 * (kt & 3))) & 0xFFFFu) < keep16;
}
// Keys on rows: a lane owns query q and, in tile mt, keys mt*16 + lg*4 + r.
// Element (q, key) draws the bit of (row q, lm = key % 16, kt = key / 16), so
// the lane hashes (q, lg*4 + r) for r = 0..3 and takes slice kt = mt:
// att_drop_keep(z[r], mt, keep16). Eight hashes per 16-query tile, as with
// queries on rows.
DEV void att_drop_hash_krows(uint64_t (&z)[4][2], uint64_t seed, int bh,
                             int S, int q, int lg) {
#pragma unroll
  for (int r = 0; r < 4; ++r) att_drop_hash(z[r], seed, bh, S, q, lg * 4 + r);
}
// One 64-key block's keep bits for all query rows, shared by its four
// waves through LDS: bit w of byte (q >> 2)*64 + lm*4 + (q & 3) is the keep
// bit of (row q, key kb*64 + w*16 + lm). Those four keys are the four
// slices of ONE hash, att_drop_hash_half(.., kb & 1), so a thread pays one hash
// per byte and eight for S = 128. A lane reads its tile's four rows
// lg*4 + r as the dword at ((qt*4 + lg)*16 + lm)*4.
DEV void att_drop_bits_lds(unsigned char* bits, uint64_t seed, int bh, int S,
                           int kb, int nrows, unsigned keep16, int tid) {
  for (int u = tid; u < nrows * 16; u += 256) {
    const int q = u >> 4, lm = u & 15;
    uint64_t z[2] = {0, 0};
    z[kb & 1] = att_drop_hash_half(seed, bh, S, q, lm, kb & 1);
    unsigned v = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      v |= (unsigned)att_drop_keep(z, (kb & 1) * 4 + w, keep16) << w;
    bits[(q >> 2) * 64 + lm * 4 + (q & 3)] = (unsigned char)v;
  }
}

// store a 16-row x 64-col accumulator tile (MFMA C layout) as bf16 rows
// row0.. of dst (row stride rstride elements); rows >= S are skipped
DEV void att_store_rows16(ushort_t* __restrict__ dst, int rstride,
                          const f32x4 (&acc)[4], int row0, int S, int lm,
                          int lg) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    // a lane's rows r and r + 1 share one packed convert
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const int row = row0 + lg * 4 + r;
      const unsigned int v2 = f32x2_to_bf16x2(acc[ct][r], acc[ct][r + 1]);
      if (row < S) dst[(size_t)row * rstride + ct * 16 + lm] = (ushort_t)v2;
      if (row + 1 < S)
        dst[(size_t)(row + 1) * rstride + ct * 16 + lm] = (ushort_t)(v2 >> 16);
    }
  }
}

// the same for two tiles on the same rows (dK and dV): each row's two
// stores issue together, which measures faster than two single calls
DEV void att_store_rows16x2(ushort_t* __restrict__ d0,
                            ushort_t* __restrict__ d1, int rstride,
                            const f32x4 (&a0)[4], const f32x4 (&a1)[4],
                            int row0, int S, int lm, int lg) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const int row = row0 + lg * 4 + r;
      const int c = ct * 16 + lm;
      const unsigned int v0 = f32x2_to_bf16x2(a0[ct][r], a0[ct][r + 1]);
      const unsigned int v1 = f32x2_to_bf16x2(a1[ct][r], a1[ct][r + 1]);
      if (row < S) {
        d0[(size_t)row * rstride + c] = (ushort_t)v0;
        d1[(size_t)row * rstride + c] = (ushort_t)v1;
      }
      if (row + 1 < S) {
        d0[(size_t)(row + 1) * rstride + c] = (ushort_t)(v0 >> 16);
        d1[(size_t)(row + 1) * rstride + c] = (ushort_t)(v1 >> 16);
      }
    }
  }
}

// Column sums of a stored 16-row x 64-col tile, for the bias gradient of
// the linear that produced the tile's tensor: cs[ct] += over the lane's 4
// rows (rows < S only) of the value AS att_store_rows16 STORES IT (rounded
// to bf16), so the sum is over exactly what the weight-gradient GEMM reads.
DEV void att_colsum_rows16(float (&cs)[4], const f32x4 (&acc)[4], int row0,
                           int S, int lg) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (row0 + lg * 4 + r < S) cs[ct] += bf16_to_f32(f32_to_bf16(acc[ct][r]));
  }
}

// Fold the four lg row groups of a wave: afterwards every lane holds the
// wave's sum for its column ct*16 + lm.
DEV void att_colsum_wave(float (&cs)[4]) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    cs[ct] += __shfl_xor(cs[ct], 16, 64);
    cs[ct] += __shfl_xor(cs[ct], 32, 64);
  }
}

// store a TRANSPOSED 64-col x 16-row accumulator tile: acc[ct][r] is column
// ct*16 + lg*4 + r of row row0 + lm, so a lane's four values of one ct are
// 8 contiguous bytes of its row. Rows >= S are skipped.
DEV void att_store_cols16(ushort_t* __restrict__ dst, int rstride,
                          const f32x4 (&acc)[4], int row0, int S, int lm,
                          int lg) {
  const int row = row0 + lm;
  if (row >= S) return;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
    *(ushort4_t*)(dst + (size_t)row * rstride + ct * 16 + lg * 4) =
        f32x4_to_bf16x4(acc[ct][0], acc[ct][1], acc[ct][2], acc[ct][3]);
}

// Column sums of such a tile AS STORED (rounded to bf16, rows < S only),
// over the wave's 16 rows. The rows are on the 16 lm lanes, so this is a
// reduce-scatter butterfly: each step hands half of the lane's columns to
// its partner and adds the partner's other half, 8 + 4 + 2 + 1 shuffles,
// and lane lm ends with column index c = lm of (c = ct*4 + r), i.e. column
// (lm >> 2)*16 + lg*4 + (lm & 3). The order of the adds is fixed.
DEV float att_colsum_cols16(const f32x4 (&acc)[4], int row0, int S, int lm) {
  const bool live = row0 + lm < S;
  float v8[8], v4[4], v2[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float lo = live ? bf16_to_f32(f32_to_bf16(acc[i >> 2][i & 3])) : 0.f;
    const float hi =
        live ? bf16_to_f32(f32_to_bf16(acc[2 + (i >> 2)][i & 3])) : 0.f;
    v8[i] = ((lm & 8) ? hi : lo) + __shfl_xor((lm & 8) ? lo : hi, 8, 64);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    v4[i] = ((lm & 4) ? v8[4 + i] : v8[i]) +
            __shfl_xor((lm & 4) ? v8[i] : v8[4 + i], 4, 64);
#pragma unroll
  for (int i = 0; i < 2; ++i)
    v2[i] = ((lm & 2) ? v4[2 + i] : v4[i]) +
            __shfl_xor((lm & 2) ? v4[i] : v4[2 + i], 2, 64);
  return ((lm & 1) ? v2[1] : v2[0]) + __shfl_xor((lm & 1) ? v2[0] : v2[1], 1, 64);
}
// the column that att_colsum_cols16 leaves on lane (lm, lg)
DEV int att_colsum_cols16_col(int lm, int lg) {
  return (lm >> 2) * 16 + lg * 4 + (lm & 3);
}

// Launch KERNEL, an expression in the constexpr bool HM such as
// (attn_bwd1s_kernel<HM>), as its HAS_MASK instantiation picked by the
// runtime bool has_mask; 256 threads, the argument list written once.
#define ATT_LAUNCH_HM(has_mask, KERNEL, grid, lds_bytes, stream, ...)         \
  do {                                                                        \
    if (has_mask) {                                                           \
      constexpr bool HM = true;                                               \
      hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds_bytes, stream,          \
                         __VA_ARGS__);                                        \
    } else {                                                                  \
      constexpr bool HM = false;                                              \
      hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds_bytes, stream,          \
                         __VA_ARGS__);                                        \
    }                                                                         \
  } while (0)
