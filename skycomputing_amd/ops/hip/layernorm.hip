// Fused (residual-add +) LayerNorm forward/backward for gfx950.
//
// Replaces the reference's optional apex FusedLayerNormAffineFunction
// (reference: scaelum/model/bert_layers.py:128-168) and fuses the
// preceding residual add (bert_layers.py:283-288,321-326) into the pass.
//
// Fast path (cols % 8 == 0, cols <= 4096): WAVE-PER-ROW, 16 B/lane
// vectorized loads, values register-cached across the stats/normalize
// passes, reductions via 64-lane shuffles only — no LDS, no barriers.
// Backward splits into a wave-per-row dx kernel plus a column-parallel
// dweight/dbias reduction kernel (coalesced down-column traversal, few
// atomics) instead of row-serial LDS accumulation.
// Generic fallback (odd cols): block-per-row scalar kernels.

#include "common.h"

#define LN_MAXCH 8  // max chunks of 512 elements -> cols <= 4096 fast path

// ---------------- forward (vectorized, wave per row) ----------------

// 64-lane sum through DPP row shifts and row broadcasts (VALU only) instead
// of wave_sum's six dependent LDS-crossbar shuffles. The forward needs its
// two sums one after the other (mean, then the centred squares), so the
// reduction's latency is on the critical path twice. Lanes a shift has no
// source for, and rows a broadcast is masked off for, add 0.
template <int CTRL, int ROW_MASK>
DEV float dpp_add(float v) {
  const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL,
                                            ROW_MASK, 0xf, true);
  return v + __int_as_float(t);
}
DEV float wave_sum_dpp(float v) {
  v = dpp_add<0x111, 0xf>(v);  // row_shr:1
  v = dpp_add<0x112, 0xf>(v);  // row_shr:2
  v = dpp_add<0x114, 0xf>(v);  // row_shr:4
  v = dpp_add<0x118, 0xf>(v);  // row_shr:8 -> lane 15 of a row: the row's sum
  v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
  v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Per-launch dropout constants of the vectorized kernels.
struct LnDrop {
  uint64_t seed;
  unsigned keep16;
  float inv_keep;
  DEV LnDrop(bool drop, float keep, uint64_t salt,
             const unsigned long long* state)
      : seed(drop ? rng_seed(salt, state) : 0),
        keep16(keep_to_16(keep)),
        inv_keep(1.f / keep) {}
};

// A lane's 8 values of the LayerNorm input xs = dropout(x) + res at vec8
// index i8 (LINEAR scheme: row * cols8 + column vec8). Dropout is applied
// BEFORE the residual add (the BERT pattern LN(dropout(dense(x)) + residual),
// reference bert_layers.py:283-288). Fills float v[8]; with DROP also sets
// the unsigned lvalue kbits to the 8 keep bits, from which the backward
// masks dx. Reads the enclosing kernel's DT, HAS_RES and DROP, and is a
// statement macro for RNG_DROP8's reason (ops/hip/common.h).
#define LN_LOAD_ROW(x, res, i8, drop, v, kbits)                               \
  do {                                                                        \
    Vec8<DT>::load(x, i8, v);                                                 \
    if (DROP)                                                                 \
      RNG_DROP8((drop).seed, i8, (drop).keep16, (drop).inv_keep, v, kbits);   \
    if (HAS_RES) {                                                            \
      float r_[8];                                                            \
      Vec8<DT>::load(res, i8, r_);                                            \
      _Pragma("unroll") for (int k_ = 0; k_ < 8; ++k_) (v)[k_] += r_[k_];     \
    }                                                                         \
  } while (0)

// DROP: the mask is regenerated from (salt,state,element index) in backward.
template <int DT, bool HAS_RES, bool DROP, int CH>
__global__ __launch_bounds__(256) void ln_fwd_vec_kernel(
    const void* __restrict__ x, const void* __restrict__ res,
    const void* __restrict__ w, const void* __restrict__ b,
    void* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int64_t rows, int64_t cols, float eps,
    float keep, uint64_t salt, const unsigned long long* __restrict__ state) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int64_t cols8 = cols / 8;
  const LnDrop drop(DROP, keep, salt, state);
  float v[CH][8];
  for (int64_t row = (int64_t)blockIdx.x * 4 + wid; row < rows;
       row += (int64_t)gridDim.x * 4) {
    const int64_t base8 = row * cols8;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int64_t i8 = (int64_t)c * WAVE + lane;
      if (i8 < cols8) {
        [[maybe_unused]] unsigned kbits;
        LN_LOAD_ROW(x, res, base8 + i8, drop, v[c], kbits);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[c][j];
      }
    }
    s = wave_sum_dpp(s);
    const float mean = s / (float)cols;
    // variance from centred values: E[x^2] - mean^2 cancels to nothing
    // once |mean| >> std (fp32 x-hat error 2.4e-3 at mean 64, std 1); the
    // row is in registers, so the second pass costs no memory traffic
    float s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int64_t i8 = (int64_t)c * WAVE + lane;
      if (i8 < cols8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = v[c][j] - mean;
          s2 += d * d;
        }
      }
    }
    s2 = wave_sum_dpp(s2);
    const float rstd = rsqrtf(s2 / (float)cols + eps);
    if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int64_t i8 = (int64_t)c * WAVE + lane;
      if (i8 < cols8) {
        float wv[8], bv[8], o[8];
        Vec8<DT>::load(w, i8, wv);
        Vec8<DT>::load(b, i8, bv);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o[j] = (v[c][j] - mean) * rstd * wv[j] + bv[j];
        Vec8<DT>::store(y, base8 + i8, o);
      }
    }
  }
}

// generic scalar fallback (block per row)
template <int DT, int BLOCK, bool HAS_RES>
__global__ __launch_bounds__(BLOCK) void ln_fwd_kernel(
    const void* __restrict__ x, const void* __restrict__ res,
    const void* __restrict__ w, const void* __restrict__ b,
    void* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int64_t rows, int64_t cols, float eps) {
  __shared__ float lds[BLOCK / WAVE > 2 ? BLOCK / WAVE : 2];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t base = row * cols;
    float s = 0.f;
    for (int64_t c = threadIdx.x; c < cols; c += BLOCK) {
      float v = load_elem<DT>(x, base + c);
      if (HAS_RES) v += load_elem<DT>(res, base + c);
      s += v;
    }
    s = block_sum<BLOCK>(s, lds);
    const float mean = s / (float)cols;
    // centred variance (see ln_fwd_vec_kernel); the row is re-read anyway.
    // The centred values also sum to what rounding left out of `mean`
    // (delta, up to half an ulp of the mean: 4e-6 at 64, too small to
    // change the stored mean). This path is on no hot loop, so it spends a
    // third block_sum to take delta off x - mean, which keeps y at fp32
    // relative accuracy for any row mean; the vector kernel stays at the
    // two-pass accuracy of its two reductions.
    float s1 = 0.f, s2 = 0.f;
    for (int64_t c = threadIdx.x; c < cols; c += BLOCK) {
      float v = load_elem<DT>(x, base + c);
      if (HAS_RES) v += load_elem<DT>(res, base + c);
      const float d = v - mean;
      s1 += d;
      s2 += d * d;
    }
    s1 = block_sum<BLOCK>(s1, lds);
    s2 = block_sum<BLOCK>(s2, lds);
    const float delta = s1 / (float)cols;
    const float rstd =
        rsqrtf(fmaxf(s2 / (float)cols - delta * delta, 0.f) + eps);
    if (threadIdx.x == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
    for (int64_t c = threadIdx.x; c < cols; c += BLOCK) {
      float v = load_elem<DT>(x, base + c);
      if (HAS_RES) v += load_elem<DT>(res, base + c);
      store_elem<DT>(y, base + c,
                     ((v - mean) - delta) * rstd * load_elem<DT>(w, c) +
                         load_elem<DT>(b, c));
    }
  }
}

static inline bool ln_fast_ok(int64_t cols) {
  return (cols % 8 == 0) && cols <= 64 * 8 * LN_MAXCH;
}

// chunks of 512 elements (one vec8 per lane) a wave needs for a row
static inline int ln_chunks(int64_t cols) {
  return (int)((cols / 8 + WAVE - 1) / WAVE);
}

SKY_EXPORT int sky_layernorm_fwd(uint64_t stream, uint64_t x, uint64_t res,
                                 uint64_t w, uint64_t b, uint64_t y,
                                 uint64_t mean, uint64_t rstd, int64_t rows,
                                 int64_t cols, float eps, int dt, float keep,
                                 uint64_t salt, uint64_t state) {
  hipStream_t s = (hipStream_t)stream;
  bool has_res = res != 0;
  bool drop = keep < 1.f;
  if (drop && !ln_fast_ok(cols)) return (int)hipErrorInvalidValue;
  if (ln_fast_ok(cols)) {
    unsigned grid = (unsigned)((rows + 3) / 4);
    if (grid > 8192u) grid = 8192u;
    dispatch_tags(dt, has_res, drop, ln_chunks(cols),
                  [&](auto DT, auto HR, auto DR, auto CH) {
      hipLaunchKernelGGL((ln_fwd_vec_kernel<DT, HR, DR, CH>), dim3(grid),
                         dim3(256), 0, s, (const void*)x, (const void*)res,
                         (const void*)w, (const void*)b, (void*)y,
                         (float*)mean, (float*)rstd, rows, cols, eps, keep,
                         salt, (const unsigned long long*)state);
    });
  } else {
    dim3 grid((unsigned)(rows < 4096 ? rows : 4096));
    dispatch_tags(dt, has_res, false, 0, [&](auto DT, auto HR, auto, auto) {
      hipLaunchKernelGGL((ln_fwd_kernel<DT, 256, HR>), grid, dim3(256), 0, s,
                         (const void*)x, (const void*)res, (const void*)w,
                         (const void*)b, (void*)y, (float*)mean, (float*)rstd,
                         rows, cols, eps);
    });
  }
  LAUNCH_CHECK();
  return 0;
}

// ---------------- backward ----------------
// dxhat = dy * w
// dx = rstd * (dxhat - mean_c(dxhat) - xhat * mean_c(dxhat * xhat))
// dw[c] += sum_r dy * xhat ; db[c] += sum_r dy

// Vectorized dx with NS column sums (0, 2 or 3), wave per row.
//
// DROP: x is the PRE-dropout tensor; the mask is regenerated to rebuild
// xs = dropout(x)+res for the statistics, dx gets the mask/keep factor,
// and (when dres != null) the residual grad d_xs is written separately.
//
// NS = 2 fuses the dw/db column partials into the pass: it already holds dy
// and xhat in registers for every element, and a wave's lane covers the SAME
// column slices on every row it processes — so the partial sums accumulate
// in registers for free and wb_part's 16-24 MB re-read of dy/x disappears.
// The block's 4 waves merge through LDS into ONE scratch slab
// (slab = blockIdx); the grid is capped so nslabs <= MAX_SLABS.
//
// NS = 3 adds a third column partial: the sum over rows of the value stored
// to dx (after the dropout mask and 1/keep scaling), accumulated in fp32
// from the value AS STORED, i.e. rounded to the output dtype first. When
// the LayerNorm's input is a linear's output, that sum is the linear's
// bias gradient, and it is then the column sum of exactly the dy that the
// linear's dgrad and wgrad GEMMs read — what a separate column-sum pass or
// the BGRADB epilogue computes. (Summing the unrounded fp32 values instead
// differed from those by the accumulated input rounding, up to 0.05 over
// 256 rows of unit-scale bf16 gradients.) It costs a few VALU ops per
// element here and saves the linear a pass over its dy. Slab layout is
// [NS*cols]: dw, db(, dxsum).
//
// NS = 0 (SKY_LN_SPLIT_WB) is the dx pass alone: no accumulators, no LDS
// merge, and scratch is not touched.
//
// PMERGE (CH <= 2 only) merges in one barrier: every wave writes its
// NS x CH*512 partials to an LDS region of its own (4 x 12 KB at NS = 3),
// and after the barrier each thread sums its columns over waves 0, 1, 2, 3
// in that order from 0.f, which is the order and the arithmetic of the
// serial merge (zeroed LDS, then the waves add in turn), and stores the
// slab values from registers, 16 bytes at a time. The serial merge costs
// five barriers and three passes over the LDS image; it stays for CH = 4,
// whose four regions would need 96 KB, and under SKY_LN_MERGE_SERIAL=1.
// So do the kernels without dropout: at 114 to 128 VGPRs they run four
// blocks per CU, the region writes cost them the registers for that
// (132 to 138) and four 48 KB regions would not fit the 160 KB of LDS
// either, and the merge is not worth a block of occupancy. With dropout the
// VGPRs (130 to 158) allow three blocks with either merge.
#define LN_PMERGE_OK(DROP, CH, NS) ((CH) <= 2 && (NS) > 0 && (DROP))
template <int DT, bool HAS_RES, bool DROP, int CH, int NS, bool PMERGE = false>
__global__ __launch_bounds__(256) void ln_bwd_dx_cs_kernel(
    const void* __restrict__ dy, const void* __restrict__ x,
    const void* __restrict__ res, const void* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    void* __restrict__ dx, void* __restrict__ dres,
    float* __restrict__ scratch, int64_t rows, int64_t cols, float keep,
    uint64_t salt, const unsigned long long* __restrict__ state) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int64_t cols8 = cols / 8;
  const LnDrop drop(DROP, keep, salt, state);
  float xh[CH][8], dxh[CH][8];
  float sw[NS ? CH : 1][8], sb[NS ? CH : 1][8], sx[NS == 3 ? CH : 1][8];
  if constexpr (NS > 0) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sw[c][j] = 0.f;
        sb[c][j] = 0.f;
        if constexpr (NS == 3) sx[c][j] = 0.f;
      }
  }
  unsigned kbits[CH];
  for (int64_t row = (int64_t)blockIdx.x * 4 + wid; row < rows;
       row += (int64_t)gridDim.x * 4) {
    const int64_t base8 = row * cols8;
    const float mu = mean[row], rs = rstd[row];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int64_t i8 = (int64_t)c * WAVE + lane;
      if (i8 < cols8) {
        float xv[8], dyv[8], wv[8];
        LN_LOAD_ROW(x, res, base8 + i8, drop, xv, kbits[c]);
        Vec8<DT>::load(dy, base8 + i8, dyv);
        Vec8<DT>::load(w, i8, wv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xh[c][j] = (xv[j] - mu) * rs;
          dxh[c][j] = dyv[j] * wv[j];
          s1 += dxh[c][j];
          s2 += dxh[c][j] * xh[c][j];
          if constexpr (NS > 0) {
            sw[c][j] += dyv[j] * xh[c][j];
            sb[c][j] += dyv[j];
          }
        }
      }
    }
    s1 = wave_sum(s1) / (float)cols;
    s2 = wave_sum(s2) / (float)cols;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int64_t i8 = (int64_t)c * WAVE + lane;
      if (i8 < cols8) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o[j] = rs * (dxh[c][j] - s1 - xh[c][j] * s2);
        if (DROP && dres != nullptr) Vec8<DT>::store(dres, base8 + i8, o);
        if (DROP) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            o[j] = ((kbits[c] >> j) & 1u) ? o[j] * drop.inv_keep : 0.f;
        }
        if constexpr (NS == 3) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            sx[c][j] += DT == DT_BF16 ? bf16_to_f32(f32_to_bf16(o[j])) : o[j];
        }
        Vec8<DT>::store(dx, base8 + i8, o);
      }
    }
  }
  if constexpr (NS > 0 && PMERGE) {
    static_assert(LN_PMERGE_OK(DROP, CH, NS), "see LN_PMERGE_OK");
    __shared__ __attribute__((aligned(16))) float part[4][NS][CH * 512];
    // The partials pass through an opaque register constraint first, so
    // that the 16-byte LDS writes below do not reach back into the row loop:
    // with contraction on, the SLP vectoriser would otherwise pair that
    // loop's accumulations by these vectors and fuse other multiplies into
    // FMAs than the serial-merge kernel does (see RNG_DROP8 in common.h),
    // and the fp32 kernels' slabs would move by an ulp. What the vectoriser
    // does is the compiler's choice, not the language's:
    // tests/test_ln_merge_gpu.py compares this kernel's slabs and outputs
    // with the serial kernel's, bit for bit, fp32 included, and is what
    // notices if a compiler decides otherwise.
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        asm volatile("" : "+v"(sw[c][j]), "+v"(sb[c][j]));
        if constexpr (NS == 3) asm volatile("" : "+v"(sx[c][j]));
      }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int64_t i8 = (int64_t)c * WAVE + lane;
      if (i8 < cols8) {
        float4_t* pw = (float4_t*)&part[wid][0][i8 * 8];
        float4_t* pb = (float4_t*)&part[wid][1][i8 * 8];
        pw[0] = float4_t{sw[c][0], sw[c][1], sw[c][2], sw[c][3]};
        pw[1] = float4_t{sw[c][4], sw[c][5], sw[c][6], sw[c][7]};
        pb[0] = float4_t{sb[c][0], sb[c][1], sb[c][2], sb[c][3]};
        pb[1] = float4_t{sb[c][4], sb[c][5], sb[c][6], sb[c][7]};
        if constexpr (NS == 3) {
          float4_t* px = (float4_t*)&part[wid][2][i8 * 8];
          px[0] = float4_t{sx[c][0], sx[c][1], sx[c][2], sx[c][3]};
          px[1] = float4_t{sx[c][4], sx[c][5], sx[c][6], sx[c][7]};
        }
      }
    }
    __syncthreads();
    // cols % 8 == 0, so a row of the slab is cols / 4 whole float4s, all of
    // them written above (i8 < cols8 covers every column below cols)
    float* base = scratch + (int64_t)blockIdx.x * NS * cols8 * 8;
    const int n4 = (int)(cols8 * 2);
    for (int i4 = threadIdx.x; i4 < n4; i4 += 256) {
#pragma unroll
      for (int v = 0; v < NS; ++v) {
        float4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) a += *(const float4_t*)&part[k][v][i4 * 4];
        *(float4_t*)(base + (int64_t)v * cols8 * 8 + (int64_t)i4 * 4) = a;
      }
    }
  } else if constexpr (NS > 0) {
    // merge the 4 waves' partials through LDS (halves the slab count vs
    // per-wave slabs -> half the scratch the final stage must re-read),
    // then ONE slab write per block.
    __shared__ float mrg[NS][CH * 512];
    for (int i = threadIdx.x; i < NS * CH * 512; i += 256)
      (&mrg[0][0])[i] = 0.f;
    __syncthreads();
    for (int k = 0; k < 4; ++k) {
      if (wid == k) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int64_t i8 = (int64_t)c * WAVE + lane;
          if (i8 < cols8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              mrg[0][i8 * 8 + j] += sw[c][j];
              mrg[1][i8 * 8 + j] += sb[c][j];
              if constexpr (NS == 3) mrg[2][i8 * 8 + j] += sx[c][j];
            }
          }
        }
      }
      __syncthreads();
    }
    float* base = scratch + (int64_t)blockIdx.x * NS * cols8 * 8;
    for (int i = threadIdx.x; i < cols8 * 8; i += 256) {
      base[i] = mrg[0][i];
      base[cols8 * 8 + i] = mrg[1][i];
      if constexpr (NS == 3) base[2 * cols8 * 8 + i] = mrg[2][i];
    }
  }
}

// column-parallel dw/db, two-stage, no atomics, outputs need no zero-init:
// stage 1 writes per-slab partials to scratch [nslabs][2*cols] fp32
// (dw partial at [y][c], db partial at [y][cols+c]); stage 2 reduces.
template <int DT, bool HAS_RES, bool DROP, int BLOCK>
__global__ __launch_bounds__(BLOCK) void ln_bwd_wb_part_kernel(
    const void* __restrict__ dy, const void* __restrict__ x,
    const void* __restrict__ res, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ scratch,
    int64_t rows, int64_t cols8, int64_t rows_per_slab, float keep,
    uint64_t salt, const unsigned long long* __restrict__ state) {
  const int64_t c8 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (c8 >= cols8) return;
  const int64_t slab = blockIdx.y;
  const int64_t r0 = slab * rows_per_slab;
  const int64_t r1 = min(rows, r0 + rows_per_slab);
  const LnDrop drop(DROP, keep, salt, state);
  float sw[8] = {0.f}, sb[8] = {0.f};
  for (int64_t r = r0; r < r1; ++r) {
    const float mu = mean[r], rs = rstd[r];
    float xv[8], dyv[8];
    [[maybe_unused]] unsigned kbits;
    LN_LOAD_ROW(x, res, r * cols8 + c8, drop, xv, kbits);
    Vec8<DT>::load(dy, r * cols8 + c8, dyv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sw[j] += dyv[j] * (xv[j] - mu) * rs;
      sb[j] += dyv[j];
    }
  }
  float* base = scratch + slab * 2 * cols8 * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    base[c8 * 8 + j] = sw[j];
    base[cols8 * 8 + c8 * 8 + j] = sb[j];
  }
}

// two-level: a 1024-thread block covers 16 columns x 64 slab-groups,
// parallel LDS tree, one write per column (see colsum_final_kernel).
// NV = vectors per slab: 2 (dw, db) or 3 (dw, db, dxsum). (A 4-column,
// 256-slab-group variant was measured as the 3-vector final at 512 slabs
// and lost, 23.8 vs 18.6 us for dx_cs + final: profiles/r03_notes.md.)
template <int BLOCK, int DTOUT, int NV>
__global__ __launch_bounds__(1024) void ln_bwd_wb_final_kernel(
    const float* __restrict__ scratch, void* __restrict__ dw,
    void* __restrict__ db, void* __restrict__ dxsum, int64_t cols,
    int64_t nslabs) {
  __shared__ float lds[NV][64][17];
  const int c = threadIdx.x & 15;
  const int g = threadIdx.x >> 4;  // 0..63
  const int64_t col = (int64_t)blockIdx.x * 16 + c;
  const int64_t per = (nslabs + 63) / 64;
  float s[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) s[v] = 0.f;
  if (col < cols) {
    const int64_t y1 = min(nslabs, (int64_t)(g + 1) * per);
    for (int64_t y = (int64_t)g * per; y < y1; ++y) {
#pragma unroll
      for (int v = 0; v < NV; ++v) s[v] += scratch[(y * NV + v) * cols + col];
    }
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) lds[v][g][c] = s[v];
  __syncthreads();
  for (int st = 32; st >= 1; st >>= 1) {
    if (g < st) {
#pragma unroll
      for (int v = 0; v < NV; ++v) lds[v][g][c] += lds[v][g + st][c];
    }
    __syncthreads();
  }
  if (g == 0 && col < cols) {
    store_elem<DTOUT>(dw, col, lds[0][0][c]);
    store_elem<DTOUT>(db, col, lds[1][0][c]);
    if constexpr (NV == 3) store_elem<DTOUT>(dxsum, col, lds[NV - 1][0][c]);
  }
}

template <int DT, bool HAS_RES, int BLOCK>
__global__ __launch_bounds__(BLOCK) void ln_bwd_wb_kernel(
    const void* __restrict__ dy, const void* __restrict__ x,
    const void* __restrict__ res, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ dw,
    float* __restrict__ db, int64_t rows, int64_t cols, int64_t rows_per_slab) {
  const int64_t col = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (col >= cols) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab;
  const int64_t r1 = min(rows, r0 + rows_per_slab);
  float sw = 0.f, sb = 0.f;
  for (int64_t r = r0; r < r1; ++r) {
    float xv = load_elem<DT>(x, r * cols + col);
    if (HAS_RES) xv += load_elem<DT>(res, r * cols + col);
    float dyv = load_elem<DT>(dy, r * cols + col);
    sw += dyv * (xv - mean[r]) * rstd[r];
    sb += dyv;
  }
  atomicAdd(&dw[col], sw);
  atomicAdd(&db[col], sb);
}

// generic scalar fallback dx (block per row)
template <int DT, int BLOCK, bool HAS_RES>
__global__ __launch_bounds__(BLOCK) void ln_bwd_dx_kernel(
    const void* __restrict__ dy, const void* __restrict__ x,
    const void* __restrict__ res, const void* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    void* __restrict__ dx, int64_t rows, int64_t cols) {
  __shared__ float lds[BLOCK / WAVE > 2 ? BLOCK / WAVE : 2];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t base = row * cols;
    const float mu = mean[row], rs = rstd[row];
    float s1 = 0.f, s2 = 0.f;
    for (int64_t c = threadIdx.x; c < cols; c += BLOCK) {
      float xv = load_elem<DT>(x, base + c);
      if (HAS_RES) xv += load_elem<DT>(res, base + c);
      float dxhat = load_elem<DT>(dy, base + c) * load_elem<DT>(w, c);
      s1 += dxhat;
      s2 += dxhat * (xv - mu) * rs;
    }
    s1 = block_sum<BLOCK>(s1, lds) / (float)cols;
    s2 = block_sum<BLOCK>(s2, lds) / (float)cols;
    for (int64_t c = threadIdx.x; c < cols; c += BLOCK) {
      float xv = load_elem<DT>(x, base + c);
      if (HAS_RES) xv += load_elem<DT>(res, base + c);
      float xhat = (xv - mu) * rs;
      float dxhat = load_elem<DT>(dy, base + c) * load_elem<DT>(w, c);
      store_elem<DT>(dx, base + c, rs * (dxhat - s1 - xhat * s2));
    }
  }
}

// widest chunk count the three-sum dx kernel is built for: CH=2 and CH=4
// compile without scratch; CH=8 is at the VGPR limit with two sums already
// and is not offered.
#define LN_XSUM_MAXCH 4

// what every backward launch below needs of the entry points' arguments
struct LnBwdArgs {
  hipStream_t s;
  uint64_t dy, x, res, w, mean, rstd, dx, dres, scratch;
  int64_t rows, cols;
  int dt;
  float keep;
  uint64_t salt, state;
};

// The vectorized dx kernel with NS column sums; returns its grid, which for
// NS > 0 is the number of slabs it wrote ([NS*cols] fp32 each).
template <int NS>
static int64_t ln_bwd_dx_launch(const LnBwdArgs& a) {
  unsigned gmax = 8192;
  if (NS > 0) {
    // one slab per BLOCK (LDS-merged): grid 512 keeps the dx streaming fed
    // (256 starved it: 16.9 vs 9.9 us) while the final re-reads only
    // 512 slabs (SKY_LN_CS_GRID overrides for sweeps)
    gmax = 512;
    if (const char* e = getenv("SKY_LN_CS_GRID")) gmax = (unsigned)atoi(e);
    if (gmax > (unsigned)MAX_SLABS) gmax = MAX_SLABS;
    if (gmax < 1) gmax = 1;
  }
  unsigned grid = (unsigned)((a.rows + 3) / 4);
  if (grid > gmax) grid = gmax;
  // one-barrier merge where LN_PMERGE_OK allows it; SKY_LN_MERGE_SERIAL set
  // (to any value, as with SKY_LN_SPLIT_WB) keeps the serial merge for A/B,
  // and so does a scratch that the 16-byte slab stores could not address
  [[maybe_unused]] const bool serial =
      NS > 0 &&
      (getenv("SKY_LN_MERGE_SERIAL") != nullptr || (a.scratch & 15) != 0);
  dispatch_tags<NS == 3 ? LN_XSUM_MAXCH : LN_MAXCH>(
      a.dt, a.res != 0, a.keep < 1.f, ln_chunks(a.cols),
      [&](auto DT, auto HR, auto DR, auto CH) {
        auto launch = [&](auto kern) {
          hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, a.s,
                             (const void*)a.dy, (const void*)a.x,
                             (const void*)a.res, (const void*)a.w,
                             (const float*)a.mean, (const float*)a.rstd,
                             (void*)a.dx, (void*)a.dres, (float*)a.scratch,
                             a.rows, a.cols, a.keep, a.salt,
                             (const unsigned long long*)a.state);
        };
        if constexpr (LN_PMERGE_OK(DR, CH, NS)) {
          if (!serial) {
            launch(ln_bwd_dx_cs_kernel<DT, HR, DR, CH, NS, true>);
            return;
          }
        }
        launch(ln_bwd_dx_cs_kernel<DT, HR, DR, CH, NS, false>);
      });
  return (int64_t)grid;
}

// The final slab reduction: dw, db (and dxsum for NV = 3) from nslabs slabs
// of [NV*cols] fp32, written in the param dtype.
template <int NV>
static void ln_bwd_wb_final_launch(const LnBwdArgs& a, uint64_t dw,
                                   uint64_t db, uint64_t dxsum,
                                   int64_t nslabs) {
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.cols + 15) / 16)), dim3(1024),
                       0, a.s, (const float*)a.scratch, (void*)dw, (void*)db,
                       (void*)dxsum, a.cols, nslabs);
  };
  if (a.dt == DT_BF16) launch(ln_bwd_wb_final_kernel<256, DT_BF16, NV>);
  else launch(ln_bwd_wb_final_kernel<256, DT_F32, NV>);
}

// Fused backward: dx (+dres) and the per-block column partials in one
// kernel, then the final slab reduction. NS = 3 also produces dxsum[cols],
// the column sum of the stored dx.
// With a job, the final is left pending in *job for sky_colsum_finish.
template <int NS>
static int ln_bwd_cs_launch(const LnBwdArgs& a, uint64_t dw, uint64_t db,
                            uint64_t dxsum, SkyFinishJob* job = nullptr) {
  const int64_t nslabs = ln_bwd_dx_launch<NS>(a);  // one slab per block
  if (job)
    sky_finish_job_set(job, a.scratch, dw, db, dxsum, nslabs, a.cols, NS,
                       a.dt);
  else
    ln_bwd_wb_final_launch<NS>(a, dw, db, dxsum, nslabs);
  LAUNCH_CHECK();
  return 0;
}

SKY_EXPORT int sky_layernorm_bwd(uint64_t stream, uint64_t dy, uint64_t x,
                                 uint64_t res, uint64_t w, uint64_t mean,
                                 uint64_t rstd, uint64_t dx, uint64_t dw,
                                 uint64_t db, uint64_t scratch, int64_t rows,
                                 int64_t cols, int dt, float keep,
                                 uint64_t salt, uint64_t state,
                                 uint64_t dres) {
  const LnBwdArgs a{(hipStream_t)stream, dy, x, res, w, mean, rstd, dx, dres,
                    scratch, rows, cols, dt, keep, salt, state};
  hipStream_t s = a.s;
  bool has_res = res != 0;
  bool drop = keep < 1.f;
  if (drop && !ln_fast_ok(cols)) return (int)hipErrorInvalidValue;
  // fused path: the dx kernel also produces the dw/db column partials
  // (kills wb_part's re-read of dy/x); SKY_LN_SPLIT_WB=1 restores the
  // separate 3-kernel chain for A/B.
  const bool fused_wb =
      ln_fast_ok(cols) && scratch != 0 && !getenv("SKY_LN_SPLIT_WB");
  if (fused_wb) return ln_bwd_cs_launch<2>(a, dw, db, 0);
  if (ln_fast_ok(cols)) {
    ln_bwd_dx_launch<0>(a);
  } else {
    dim3 grid((unsigned)(rows < 4096 ? rows : 4096));
    dispatch_tags(dt, has_res, false, 0, [&](auto DT, auto HR, auto, auto) {
      hipLaunchKernelGGL((ln_bwd_dx_kernel<DT, 256, HR>), grid, dim3(256), 0,
                         s, (const void*)dy, (const void*)x, (const void*)res,
                         (const void*)w, (const float*)mean,
                         (const float*)rstd, (void*)dx, rows, cols);
    });
  }
  if (cols % 8 == 0 && scratch != 0) {
    constexpr int BLOCK = 128;
    const int64_t cols8 = cols / 8;
    // ~1024 workgroups total (see launch_colsum): more slabs only where
    // the column dimension is too narrow to fill the chip
    const int64_t gx = (cols8 + BLOCK - 1) / BLOCK;
    int64_t nslabs = 1024 / gx;
    if (nslabs < 128) nslabs = 128;
    if (nslabs > MAX_SLABS) nslabs = MAX_SLABS;
    if (nslabs > rows) nslabs = rows;
    const int64_t slab = (rows + nslabs - 1) / nslabs;
    dim3 grid((unsigned)gx, (unsigned)nslabs);
    dispatch_tags(dt, has_res, drop, 0, [&](auto DT, auto HR, auto DR, auto) {
      hipLaunchKernelGGL((ln_bwd_wb_part_kernel<DT, HR, DR, BLOCK>), grid,
                         dim3(BLOCK), 0, s, (const void*)dy, (const void*)x,
                         (const void*)res, (const float*)mean,
                         (const float*)rstd, (float*)scratch, rows, cols8,
                         slab, keep, salt, (const unsigned long long*)state);
    });
    ln_bwd_wb_final_launch<2>(a, dw, db, 0, nslabs);
  } else {
    constexpr int BLOCK = 256;
    // slab sized so the grid fills 256 CUs (cols/256 col-blocks * row-slabs)
    int64_t slab = 64;
    while ((cols + BLOCK - 1) / BLOCK * ((rows + slab - 1) / slab) > 2048 && slab < rows)
      slab *= 2;
    dim3 grid((unsigned)((cols + BLOCK - 1) / BLOCK),
              (unsigned)((rows + slab - 1) / slab));
    dispatch_tags(dt, has_res, false, 0, [&](auto DT, auto HR, auto, auto) {
      hipLaunchKernelGGL((ln_bwd_wb_kernel<DT, HR, BLOCK>), grid, dim3(BLOCK),
                         0, s, (const void*)dy, (const void*)x,
                         (const void*)res, (const float*)mean,
                         (const float*)rstd, (float*)dw, (float*)db, rows,
                         cols, slab);
    });
  }
  LAUNCH_CHECK();
  return 0;
}

// 1 if sky_layernorm_bwd_xsum supports this row width.
SKY_EXPORT int sky_layernorm_bwd_xsum_ok(int64_t cols) {
  return cols > 0 && cols % 8 == 0 && cols <= 64 * 8 * LN_XSUM_MAXCH;
}

// sky_layernorm_bwd plus dxsum[cols] = column sum of the stored dx (param
// dtype, like dw/db): the bias gradient of a linear feeding this LayerNorm.
// Always the fused dx + column-partials path; needs scratch of
// [MAX_SLABS][3*cols] fp32. Unsupported widths return an error so the
// caller composes the two ops instead.
SKY_EXPORT int sky_layernorm_bwd_xsum(uint64_t stream, uint64_t dy, uint64_t x,
                                      uint64_t res, uint64_t w, uint64_t mean,
                                      uint64_t rstd, uint64_t dx, uint64_t dw,
                                      uint64_t db, uint64_t scratch,
                                      int64_t rows, int64_t cols, int dt,
                                      float keep, uint64_t salt, uint64_t state,
                                      uint64_t dres, uint64_t dxsum) {
  if (!sky_layernorm_bwd_xsum_ok(cols) || scratch == 0 || dxsum == 0)
    return (int)hipErrorInvalidValue;
  const LnBwdArgs a{(hipStream_t)stream, dy, x, res, w, mean, rstd, dx, dres,
                    scratch, rows, cols, dt, keep, salt, state};
  return ln_bwd_cs_launch<3>(a, dw, db, dxsum);
}

// sky_layernorm_bwd (dxsum == 0) or sky_layernorm_bwd_xsum (dxsum != 0)
// without the final of the fused dx + column-partials path: dx (and dres)
// are written, and the slab reduction that yields dw, db (and dxsum) is
// described in *job (a host SkyFinishJob) for sky_colsum_finish. Where the
// two-sum call is not on that path (width, no scratch, SKY_LN_SPLIT_WB) it
// runs sky_layernorm_bwd whole and job->nv is 0; the three-sum call refuses
// what sky_layernorm_bwd_xsum refuses.
SKY_EXPORT int sky_layernorm_bwd_parts(uint64_t stream, uint64_t dy,
                                       uint64_t x, uint64_t res, uint64_t w,
                                       uint64_t mean, uint64_t rstd,
                                       uint64_t dx, uint64_t dw, uint64_t db,
                                       uint64_t scratch, int64_t rows,
                                       int64_t cols, int dt, float keep,
                                       uint64_t salt, uint64_t state,
                                       uint64_t dres, uint64_t dxsum,
                                       uint64_t job) {
  if (job == 0) return (int)hipErrorInvalidValue;
  SkyFinishJob* jb = (SkyFinishJob*)job;
  jb->nv = 0;
  const LnBwdArgs a{(hipStream_t)stream, dy, x, res, w, mean, rstd, dx, dres,
                    scratch, rows, cols, dt, keep, salt, state};
  if (dxsum != 0) {
    if (!sky_layernorm_bwd_xsum_ok(cols) || scratch == 0)
      return (int)hipErrorInvalidValue;
    return ln_bwd_cs_launch<3>(a, dw, db, dxsum, jb);
  }
  if (ln_fast_ok(cols) && scratch != 0 && !getenv("SKY_LN_SPLIT_WB"))
    return ln_bwd_cs_launch<2>(a, dw, db, 0, jb);
  return sky_layernorm_bwd(stream, dy, x, res, w, mean, rstd, dx, dw, db,
                           scratch, rows, cols, dt, keep, salt, state, dres);
}
