// The bf16 engine's LayerNorm family (one wave64 per row or per R rows, 16-byte vector accesses, fp32 statistics):
//   layernorm_rows / layernorm_rows_full          BertLayerNorm over a row that already holds dense(h)+bias+residual (the
//                                                 GEMM epilogue added them): (x-u)/sqrt(var+eps)*w+b, biased variance,
//                                                 eps inside the sqrt -- BertSelfOutput / BertOutput,
//                                                 oscar/modeling_bert.py:94,120; also the optional image LayerNorm,
//                                                 tasks/viewpoint_select/encoder.py:280-281      (vt_layernorm_dispatch)
//   embed_layernorm                               BertEmbeddings: word + position + token_type gather-sum -> LayerNorm,
//                                                 encoder.py:267-269; writes rows b*S+t of the [B,S,H] sequence buffer
//                                                 directly (no torch.cat, :287)                  (vt_embed_layernorm_dispatch)
//   layernorm_bwd_rows / layernorm_bwd_rows_full  their backward: dx, and dgamma / dbeta as one partial row per workgroup
//   ln_bwd_reduce                                 ... summed in a fixed order                    (vt_layernorm_bwd_dispatch)
//   embed_layernorm_bwd                           backward of embed_layernorm up to d_e          (vt_embed_layernorm_bwd_dispatch)
//   prefetch_ranges                               the weight prefetch as a launch of its own, where the chunked forward
//                                                 kernel has no spare workgroups to carry it (common.hpp, vt_prefetch_role)
// The fp32 path's LayerNorms are in fp32_path.hip / fp32_train.hip, the deferred one of inference in ln_deferred.hip.
#include "dispatch.hpp"
#include "switches.hpp"

__global__ __launch_bounds__(256) void prefetch_ranges(PrefetchArgs a) { vt_prefetch_role(a, blockIdx.x, gridDim.x); }

struct LnArgs {
  const bf16_t* x; long ldx;   // bf16, or fp16 (template parameter XF16: the training layer's pre-LayerNorm sums)
  bf16_t* y; long ldy;
  uint16_t* yh; long ldyh;     // optional second output: the same rows as fp16 (the next sub-layer's residual operand)
  const float* gamma; const float* beta;
  float* mean; float* rstd;  // optional [M] outputs for backward
  int M, H;
  int grp_rows, grp_stride;  // row remap as in the GEMM (0: identity); applies to x and y
  float eps;
  // layernorm_rows_full only: workgroups n_main .. gridDim.x - 1 do not normalise rows but read `pf`'s ranges (the weights of
  // the GEMMs that follow: vt_prefetch_role); n_main == gridDim.x and pf.n == 0 without a prefetch
  int n_main;
  PrefetchArgs pf;
};

template <int CH, bool XF16>
__global__ __launch_bounds__(256) void layernorm_rows(LnArgs a) {
  auto lo = [](uint32_t w) { return XF16 ? f16lo(w) : bf16lo(w); };
  auto hi = [](uint32_t w) { return XF16 ? f16hi(w) : bf16hi(w); };
  // One wave = LN_ROWS consecutive rows at once: their loads are all in flight together and the scale / shift vectors
  // (6 KiB of fp32 against 1.5 KiB per row) are fetched once per wave instead of once per row.
  constexpr int LN_ROWS = 4;
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * LN_ROWS;
  if (row0 >= a.M) return;
  u32x4 w[LN_ROWS][CH];
  long prow[LN_ROWS];
#pragma unroll
  for (int r = 0; r < LN_ROWS; ++r) {
    const int row = row0 + r < a.M ? row0 + r : a.M - 1;   // the tail repeats the last row (its store is skipped)
    prow[r] = a.grp_rows ? (long)(row / a.grp_rows) * a.grp_stride + (row % a.grp_rows) : (long)row;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int col = (lane + 64 * c) * 8;
      w[r][c] = col < a.H ? *(const u32x4*)(a.x + prow[r] * a.ldx + col) : (u32x4){0u, 0u, 0u, 0u};
    }
  }
  float gam[CH][8], bet[CH][8];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int col = (lane + 64 * c) * 8;
    if (col < a.H) {
      const f32x4 g0 = *(const f32x4*)(a.gamma + col), g1 = *(const f32x4*)(a.gamma + col + 4);
      const f32x4 b0 = *(const f32x4*)(a.beta + col), b1 = *(const f32x4*)(a.beta + col + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) { gam[c][i] = g0[i]; gam[c][4 + i] = g1[i]; bet[c][i] = b0[i]; bet[c][4 + i] = b1[i]; }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) { gam[c][i] = 0.f; bet[c][i] = 0.f; }
    }
  }
  const float invH = 1.0f / (float)a.H;
  float u[LN_ROWS], rs[LN_ROWS];
#pragma unroll
  for (int r = 0; r < LN_ROWS; ++r) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) s += lo(w[r][c][i]) + hi(w[r][c][i]);   // columns past H hold zeros
    u[r] = s;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int r = 0; r < LN_ROWS; ++r) u[r] += __shfl_xor(u[r], o, 64);
#pragma unroll
  for (int r = 0; r < LN_ROWS; ++r) {
    u[r] *= invH;
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int col = (lane + 64 * c) * 8;
      if (col < a.H) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float d0 = lo(w[r][c][i]) - u[r], d1 = hi(w[r][c][i]) - u[r];
          ss += d0 * d0 + d1 * d1;
        }
      }
    }
    rs[r] = ss;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int r = 0; r < LN_ROWS; ++r) rs[r] += __shfl_xor(rs[r], o, 64);
#pragma unroll
  for (int r = 0; r < LN_ROWS; ++r) {
    const int row = row0 + r;
    if (row >= a.M) break;
    const float rstd = 1.0f / sqrtf(rs[r] * invH + a.eps);
    if (lane == 0) {
      if (a.mean) a.mean[row] = u[r];
      if (a.rstd) a.rstd[row] = rstd;
    }
    bf16_t* yp = a.y + prow[r] * a.ldy;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int col = (lane + 64 * c) * 8;
      if (col < a.H) {
        u32x4 o4, h4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float o0 = (lo(w[r][c][i]) - u[r]) * rstd * gam[c][2 * i] + bet[c][2 * i];
          const float o1 = (hi(w[r][c][i]) - u[r]) * rstd * gam[c][2 * i + 1] + bet[c][2 * i + 1];
          o4[i] = pack_bf16x2(o0, o1);
          h4[i] = pack_f16x2(o0, o1);
        }
        *(u32x4*)(yp + col) = o4;
        if (a.yh) *(u32x4*)(a.yh + prow[r] * a.ldyh + col) = h4;
      }
    }
  }
}

// The same forward for H == 512 * C8 + 256 * C4 exactly and no row remap, laid out like layernorm_bwd_rows_full below: every
// lane owns 8 * C8 + 4 * C4 columns (H = 768: 12 columns on all 64 lanes instead of 8 + 8 with half the wave idle in the second
// chunk), a wave walks rows R at a time over a fixed grid with the next R rows' loads issued before the current rows'
// arithmetic, and the two reductions per row run on the vector ALU (wave_sum_valu).
template <int C8, int C4, int R, bool XF16>
__global__ __launch_bounds__(256) void layernorm_rows_full(LnArgs a) {
  constexpr int E = 8 * C8 + 4 * C4, H = 512 * C8 + 256 * C4, W = E / 2;
  if ((int)blockIdx.x >= a.n_main) {   // a spare workgroup: the weight prefetch riding along (uniform per workgroup)
    vt_prefetch_role(a.pf, (int)blockIdx.x - a.n_main, (int)gridDim.x - a.n_main);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col4 = 512 * C8 + lane * 4;
  float gam[E], bet[E];
#pragma unroll
  for (int c = 0; c < C8; ++c) {
    const int col = (lane + 64 * c) * 8;
    const f32x4 g0 = *(const f32x4*)(a.gamma + col), g1 = *(const f32x4*)(a.gamma + col + 4);
    const f32x4 b0 = *(const f32x4*)(a.beta + col), b1 = *(const f32x4*)(a.beta + col + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { gam[8 * c + i] = g0[i]; gam[8 * c + 4 + i] = g1[i]; bet[8 * c + i] = b0[i]; bet[8 * c + 4 + i] = b1[i]; }
  }
  if (C4) {
    const f32x4 g0 = *(const f32x4*)(a.gamma + col4), b0 = *(const f32x4*)(a.beta + col4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { gam[8 * C8 + i] = g0[i]; bet[8 * C8 + i] = b0[i]; }
  }
  const float invH = 1.0f / (float)H;
  const long ngroups = ((long)a.M + R - 1) / R, stride = (long)a.n_main * 4;
  uint32_t xw[R][W];
  auto load_rows = [&](long g) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      long row = g * R + r;
      row = row < a.M ? row : (long)a.M - 1;   // the tail repeats the last row (its stores are skipped)
      const bf16_t* px = a.x + row * a.ldx;
#pragma unroll
      for (int c = 0; c < C8; ++c) {
        const u32x4 vx = *(const u32x4*)(px + (lane + 64 * c) * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i) xw[r][4 * c + i] = vx[i];
      }
      if (C4) {
        const u32x2 vx = *(const u32x2*)(px + col4);
        xw[r][4 * C8] = vx[0]; xw[r][4 * C8 + 1] = vx[1];
      }
    }
  };
  long g = (long)blockIdx.x * 4 + wave;
  if (g < ngroups) load_rows(g);
  for (; g < ngroups; g += stride) {
    float xv[R][E];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < W; ++k) {
        xv[r][2 * k] = XF16 ? f16lo(xw[r][k]) : bf16lo(xw[r][k]);
        xv[r][2 * k + 1] = XF16 ? f16hi(xw[r][k]) : bf16hi(xw[r][k]);
      }
    if (g + stride < ngroups) load_rows(g + stride);
    float u[R], rs[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) s += xv[r][e];
      u[r] = s;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) u[r] = wave_sum_valu(u[r]) * invH;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) { const float d = xv[r][e] - u[r]; ss += d * d; }
      rs[r] = ss;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) rs[r] = 1.0f / sqrtf(wave_sum_valu(rs[r]) * invH + a.eps);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long row = g * R + r;
      if (row < a.M) {
        if (lane == 0) {
          if (a.mean) a.mean[row] = u[r];
          if (a.rstd) a.rstd[row] = rs[r];
        }
        float o[E];
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = (xv[r][e] - u[r]) * rs[r] * gam[e] + bet[e];
        bf16_t* yp = a.y + row * a.ldy;
        uint16_t* hp = a.yh ? a.yh + row * a.ldyh : nullptr;
#pragma unroll
        for (int c = 0; c < C8; ++c) {
          const int col = (lane + 64 * c) * 8;
          u32x4 o4, h4;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            o4[i] = pack_bf16x2(o[8 * c + 2 * i], o[8 * c + 2 * i + 1]);
            h4[i] = pack_f16x2(o[8 * c + 2 * i], o[8 * c + 2 * i + 1]);
          }
          *(u32x4*)(yp + col) = o4;
          if (hp) *(u32x4*)(hp + col) = h4;
        }
        if (C4) {
          *(u32x2*)(yp + col4) = (u32x2){pack_bf16x2(o[8 * C8], o[8 * C8 + 1]), pack_bf16x2(o[8 * C8 + 2], o[8 * C8 + 3])};
          if (hp) *(u32x2*)(hp + col4) = (u32x2){pack_f16x2(o[8 * C8], o[8 * C8 + 1]), pack_f16x2(o[8 * C8 + 2], o[8 * C8 + 3])};
        }
      }
    }
  }
}

int vt_layernorm_dispatch(const void* x, long ldx, void* y, long ldy, const float* gamma, const float* beta,
                          float* mean, float* rstd, int M, int H, float eps, int grp_rows, int grp_stride,
                          hipStream_t stream, int x_f16, void* y_f16, long ldyh, const PrefetchArgs* pf) {
  if (!x || !y || !gamma || !beta) return VT_ERR_NULL;
  if (M <= 0 || H <= 0 || (H % 8) || H > 64 * 8 * 4) return VT_ERR_BAD_SHAPE;
  if ((ldx % 8) || (ldy % 8) || (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) & 15)) return VT_ERR_BAD_ALIGN;
  if (y_f16 && ((ldyh % 8) || ((uintptr_t)y_f16 & 15))) return VT_ERR_BAD_ALIGN;
  LnArgs a;
  a.x = (const bf16_t*)x; a.ldx = ldx; a.y = (bf16_t*)y; a.ldy = ldy; a.gamma = gamma; a.beta = beta;
  a.yh = (uint16_t*)y_f16; a.ldyh = ldyh;
  a.mean = mean; a.rstd = rstd; a.M = M; a.H = H; a.grp_rows = grp_rows; a.grp_stride = grp_stride; a.eps = eps;
  // VT_LN_FWD_ROWS: rows a wave holds at once (1 or 2; 0 = the chunked kernel above).  Measured at M = 50 820, H = 768, two
  // outputs: cold operands (tools/ln_bench.py) chunked 49.0 us, 1 row 44.2, 2 rows 44.7 (1 024 / 2 048 / 4 096 workgroups
  // within 2 us of each other); inside the pretrain step on one box (tools/experiments/ln_fwd_ab.sh) 41.8-42.1 / 39.4 / 38.1.
  static const int rows_per_wave = (int)vt_switch(VT_LN_FWD_ROWS);
  if (rows_per_wave > 0 && grp_rows == 0 && (H == 768 || H == 512 || H == 1024 || H == 256)) {
    const int R = rows_per_wave >= 2 ? 2 : 1;
    long nb = (((long)M + R - 1) / R + 3) / 4;
    static const int max_blocks = (int)vt_switch(VT_LN_FWD_BLOCKS);
    if (nb > max_blocks) nb = max_blocks;
    a.n_main = (int)nb;
    a.pf.n = 0;
    if (pf && pf->n > 0) {   // spare workgroups behind the row workgroups read the ranges (16 KiB per workgroup and pass)
      long extra = 0;
      for (int i = 0; i < pf->n; ++i) extra += (pf->bytes[i] + 16383) >> 14;
      a.pf = *pf;
      nb += extra < 1 ? 1 : (extra > 640 ? 640 : extra);
    }
#define VT_LNF_LAUNCH(C8, C4, RR)                                                                                          \
    do {                                                                                                                   \
      if (x_f16) hipLaunchKernelGGL((layernorm_rows_full<C8, C4, RR, true>), dim3((unsigned)nb), dim3(256), 0, stream, a);  \
      else hipLaunchKernelGGL((layernorm_rows_full<C8, C4, RR, false>), dim3((unsigned)nb), dim3(256), 0, stream, a);      \
    } while (0)
#define VT_LNF_SHAPE(RR)                                                                                                   \
    do {                                                                                                                   \
      if (H == 768) VT_LNF_LAUNCH(1, 1, RR); else if (H == 512) VT_LNF_LAUNCH(1, 0, RR);                                   \
      else if (H == 1024) VT_LNF_LAUNCH(2, 0, RR); else VT_LNF_LAUNCH(0, 1, RR);                                           \
    } while (0)
    if (R == 2) VT_LNF_SHAPE(2); else VT_LNF_SHAPE(1);
#undef VT_LNF_SHAPE
#undef VT_LNF_LAUNCH
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
  }
  if (pf && pf->n > 0) hipLaunchKernelGGL(prefetch_ranges, dim3(256), dim3(256), 0, stream, *pf);   // (no spare workgroups in the chunked kernel)
  const dim3 grid((M + 15) / 16), block(256);   // 4 waves x 4 rows per workgroup
  const int ch = (H + 511) / 512;
#define VT_LN_LAUNCH(CH_)                                                                     \
  if (x_f16) hipLaunchKernelGGL((layernorm_rows<CH_, true>), grid, block, 0, stream, a);      \
  else hipLaunchKernelGGL((layernorm_rows<CH_, false>), grid, block, 0, stream, a)
  if (ch == 1) { VT_LN_LAUNCH(1); }
  else if (ch == 2) { VT_LN_LAUNCH(2); }
  else if (ch == 3) { VT_LN_LAUNCH(3); }
  else { VT_LN_LAUNCH(4); }
#undef VT_LN_LAUNCH
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------
struct EmbArgs {
  const int64_t* ids; const int64_t* type_ids; const int64_t* pos_ids;  // [B,T]; type/pos may be null
  const float* word; const float* pos; const float* type;               // fp32 tables [*, H]
  const float* gamma; const float* beta;
  bf16_t* y; long ldy;                                                  // row b*S + t
  int B, T, S, H;
  int n_word, n_pos, n_type;
  float eps;
  int* err;  // set to 1 when an index is out of range (the torch reference would raise)
  DropCfg drop;  // BertEmbeddings.dropout after the LayerNorm; element index = token * H + col
};

template <int CH>
__global__ __launch_bounds__(256) void embed_layernorm(EmbArgs a) {
  const int lane = threadIdx.x & 63;
  const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= a.B * a.T) return;
  const int b = tok / a.T, t = tok - b * a.T;
  long wi = a.ids[tok];
  long pi = a.pos_ids ? a.pos_ids[tok] : (long)t;
  long ti = a.type_ids ? a.type_ids[tok] : 0L;
  if (wi < 0 || wi >= a.n_word || pi < 0 || pi >= a.n_pos || ti < 0 || ti >= a.n_type) {
    if (lane == 0 && a.err) *a.err = 1;
    wi = wi < 0 ? 0 : (wi >= a.n_word ? a.n_word - 1 : wi);
    pi = pi < 0 ? 0 : (pi >= a.n_pos ? a.n_pos - 1 : pi);
    ti = ti < 0 ? 0 : (ti >= a.n_type ? a.n_type - 1 : ti);
  }
  const float* wp = a.word + wi * a.H;
  const float* pp = a.pos + pi * a.H;
  const float* tp = a.type + ti * a.H;
  float v[CH][8];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int col = (lane + 64 * c) * 8;
    if (col < a.H) {
#pragma unroll
      for (int hlf = 0; hlf < 2; ++hlf) {
        const f32x4 w4 = *(const f32x4*)(wp + col + 4 * hlf);
        const f32x4 p4 = *(const f32x4*)(pp + col + 4 * hlf);
        const f32x4 t4 = *(const f32x4*)(tp + col + 4 * hlf);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[c][4 * hlf + i] = (w4[i] + p4[i]) + t4[i]; s += v[c][4 * hlf + i]; }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[c][i] = 0.f;
    }
  }
  const float invH = 1.0f / (float)a.H;
  const float u = wave_sum(s) * invH;
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int col = (lane + 64 * c) * 8;
    if (col < a.H) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float d = v[c][i] - u; ss += d * d; }
    }
  }
  const float rs = 1.0f / sqrtf(wave_sum(ss) * invH + a.eps);
  bf16_t* yp = a.y + ((long)b * a.S + t) * a.ldy;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int col = (lane + 64 * c) * 8;
    if (col < a.H) {
      const f32x4 g0 = *(const f32x4*)(a.gamma + col), g1 = *(const f32x4*)(a.gamma + col + 4);
      const f32x4 b0 = *(const f32x4*)(a.beta + col), b1 = *(const f32x4*)(a.beta + col + 4);
      float o[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i] = (v[c][i] - u) * rs * g0[i] + b0[i];
        o[4 + i] = (v[c][4 + i] - u) * rs * g1[i] + b1[i];
      }
      if (a.drop.thresh) {
        const uint32_t e0 = (uint32_t)tok * (uint32_t)a.H + (uint32_t)col;
        vt_drop_run<8>(a.drop, e0, o);
      }
      u32x4 w;
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(o[2 * i], o[2 * i + 1]);
      *(u32x4*)(yp + col) = w;
    }
  }
}

int vt_embed_layernorm_dispatch(const int64_t* ids, const int64_t* type_ids, const int64_t* pos_ids, const float* word,
                                const float* pos, const float* type, const float* gamma, const float* beta, void* y,
                                long ldy, int B, int T, int S, int H, int n_word, int n_pos, int n_type, float eps,
                                int* err_flag, hipStream_t stream, const DropCfg* drop) {
  if (!ids || !word || !pos || !type || !gamma || !beta || !y) return VT_ERR_NULL;
  if (B <= 0 || T <= 0 || S < T || H <= 0 || (H % 8) || H > 2048) return VT_ERR_BAD_SHAPE;
  if ((ldy % 8) || (((uintptr_t)word | (uintptr_t)pos | (uintptr_t)type | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15))
    return VT_ERR_BAD_ALIGN;
  EmbArgs a;
  a.ids = ids; a.type_ids = type_ids; a.pos_ids = pos_ids; a.word = word; a.pos = pos; a.type = type;
  a.gamma = gamma; a.beta = beta; a.y = (bf16_t*)y; a.ldy = ldy; a.B = B; a.T = T; a.S = S; a.H = H;
  a.n_word = n_word; a.n_pos = n_pos; a.n_type = n_type; a.eps = eps; a.err = err_flag;
  a.drop = drop ? *drop : vt_no_drop();
  const dim3 grid((B * T + 3) / 4), block(256);
  const int ch = (H + 511) / 512;
  if (ch == 1) hipLaunchKernelGGL(embed_layernorm<1>, grid, block, 0, stream, a);
  else if (ch == 2) hipLaunchKernelGGL(embed_layernorm<2>, grid, block, 0, stream, a);
  else if (ch == 3) hipLaunchKernelGGL(embed_layernorm<3>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(embed_layernorm<4>, grid, block, 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------
// LayerNorm backward (autograd of BertLayerNorm inside loss.backward(), pretrain.py:191):
//   xhat = (x - u) * rstd;  g = dy * gamma;  dx = rstd * (g - mean(g) - xhat * mean(g * xhat))
//   dgamma = sum_rows dy * xhat;  dbeta = sum_rows dy
// One wave per row (statistics recomputed from x: no saved mean/rstd needed), rows strided over a
// fixed grid; each wave keeps its dgamma/dbeta partial sums in registers, the block combines them
// through LDS and writes ONE partial row per block (no atomics: reproducible); ln_bwd_reduce sums
// the partial rows.
struct LnBwdArgs {
  const bf16_t* x; long ldx;
  const bf16_t* dy; long ldy;
  const float* gamma;
  bf16_t* dx; long lddx;
  bf16_t* dx2; long lddx2;   // optional: dx * dropout mask * scale (gradient of the dense output that was dropped
  DropCfg drop;              // out before the residual add); element index = row * H + col
  float* partial;  // [gridDim.x][2][H]
  int M, H;
  float eps;
};

// PG = false is the dx-only form (a frozen LayerNorm: dgamma / dbeta are not wanted): no partial sums are kept, no partial row is
// written and nothing is reduced afterwards; dx goes through the same instructions in the same order, so it is bit for bit the
// full kernel's.
template <int CH, bool XF16, bool PG = true>
__global__ __launch_bounds__(256) void layernorm_bwd_rows(LnBwdArgs a) {
  __shared__ float red[PG ? 4 : 1][2][PG ? CH * 512 : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float gam[CH][8], dg[CH][8], db[CH][8];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int col = (lane + 64 * c) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      dg[c][i] = 0.f; db[c][i] = 0.f;
      gam[c][i] = col < a.H ? a.gamma[col + i] : 0.f;
    }
  }
  const float invH = 1.0f / (float)a.H;
  for (long row = (long)blockIdx.x * 4 + wave; row < a.M; row += (long)gridDim.x * 4) {
    float xv[CH][8], gv[CH][8];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int col = (lane + 64 * c) * 8;
      if (col < a.H) {
        const u32x4 w = *(const u32x4*)(a.x + row * a.ldx + col);
        const u32x4 d = *(const u32x4*)(a.dy + row * a.ldy + col);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xv[c][2 * i] = XF16 ? f16lo(w[i]) : bf16lo(w[i]); xv[c][2 * i + 1] = XF16 ? f16hi(w[i]) : bf16hi(w[i]);
          gv[c][2 * i] = bf16lo(d[i]); gv[c][2 * i + 1] = bf16hi(d[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) s += xv[c][i];
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) { xv[c][i] = 0.f; gv[c][i] = 0.f; }
      }
    }
    const float u = wave_sum(s) * invH;
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int col = (lane + 64 * c) * 8;
      if (col < a.H) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float d = xv[c][i] - u; ss += d * d; }
      }
    }
    const float rs = 1.0f / sqrtf(wave_sum(ss) * invH + a.eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int col = (lane + 64 * c) * 8;
      if (col < a.H) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float xh = (xv[c][i] - u) * rs;
          const float dyv = gv[c][i];
          if (PG) {
            dg[c][i] += dyv * xh;
            db[c][i] += dyv;
          }
          const float gg = dyv * gam[c][i];
          xv[c][i] = xh;
          gv[c][i] = gg;
          s1 += gg;
          s2 += gg * xh;
        }
      }
    }
    const float m1 = wave_sum(s1) * invH, m2 = wave_sum(s2) * invH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int col = (lane + 64 * c) * 8;
      if (col < a.H) {
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = rs * (gv[c][i] - m1 - xv[c][i] * m2);
        u32x4 w;
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(o[2 * i], o[2 * i + 1]);
        *(u32x4*)(a.dx + row * a.lddx + col) = w;
        if (a.dx2) {
          const uint32_t e0 = (uint32_t)row * (uint32_t)a.H + (uint32_t)col;
          vt_drop_run<8>(a.drop, e0, o);   // thresh 0: everything kept, scale 1
#pragma unroll
          for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(o[2 * i], o[2 * i + 1]);
          *(u32x4*)(a.dx2 + row * a.lddx2 + col) = w;
        }
      }
    }
  }
  if (!PG) return;
  // block combine: 4 waves -> one partial row
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      red[wave][0][(lane + 64 * c) * 8 + i] = dg[c][i];
      red[wave][1][(lane + 64 * c) * 8 + i] = db[c][i];
    }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 2 * a.H; idx += 256) {
    const int which = idx / a.H, col = idx - which * a.H;
    const float v = red[0][which][col] + red[1][which][col] + red[2][which][col] + red[3][which][col];
    a.partial[((long)blockIdx.x * 2 + which) * a.H + col] = v;
  }
}

// The same backward for H == 512 * C8 + 256 * C4 exactly (768 = 512 + 256, 512, 1024, 256), built for the memory system
// instead of around it:
//  * every lane owns E = 8 * C8 + 4 * C4 columns of a row -- chunk c < C8: columns (lane + 64 c) * 8 .. + 8 (16-byte
//    accesses), then 4 columns at 512 * C8 + lane * 4 (8-byte accesses): at H = 768 all 64 lanes carry 12 columns (the
//    chunked form leaves half the wave idle in its second chunk and pays the full vector-issue time for it);
//  * a wave works on R consecutive rows at once and loads the NEXT R rows (raw words) before it starts on the current ones:
//    with one row per wave and four dependent reductions between its loads and the next row's, the kernel kept ~ 30 KB per CU
//    in flight where 8 TB/s needs ~ 64 KB;
//  * the four reductions per row run on the vector ALU (wave_sum_valu) instead of 24 LDS-crossbar shuffles.
// Same arithmetic per element as layernorm_bwd_rows; the in-lane summation order differs (last-bit differences in dx).
// (PG = false: the dx-only form, as in layernorm_bwd_rows.)
template <int C8, int C4, int R, bool XF16, bool PG = true>
__global__ __launch_bounds__(256) void layernorm_bwd_rows_full(LnBwdArgs a) {
  constexpr int E = 8 * C8 + 4 * C4, H = 512 * C8 + 256 * C4, W = E / 2;
  __shared__ float red[PG ? 4 : 1][2][PG ? H : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col4 = 512 * C8 + lane * 4;
  float gam[E], dg[E], db[E];
#pragma unroll
  for (int c = 0; c < C8; ++c) {
    const int col = (lane + 64 * c) * 8;
    const f32x4 g0 = *(const f32x4*)(a.gamma + col), g1 = *(const f32x4*)(a.gamma + col + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { gam[8 * c + i] = g0[i]; gam[8 * c + 4 + i] = g1[i]; }
  }
  if (C4) {
    const f32x4 g0 = *(const f32x4*)(a.gamma + col4);
#pragma unroll
    for (int i = 0; i < 4; ++i) gam[8 * C8 + i] = g0[i];
  }
#pragma unroll
  for (int e = 0; e < E; ++e) { dg[e] = 0.f; db[e] = 0.f; }
  const float invH = 1.0f / (float)H;
  const long ngroups = ((long)a.M + R - 1) / R, stride = (long)gridDim.x * 4;
  uint32_t xw[R][W], dw[R][W];
  auto load_rows = [&](long g) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      long row = g * R + r;
      row = row < a.M ? row : (long)a.M - 1;   // the tail repeats the last row: no contribution, no store (below)
      const bf16_t* px = a.x + row * a.ldx;
      const bf16_t* pd = a.dy + row * a.ldy;
#pragma unroll
      for (int c = 0; c < C8; ++c) {
        const int col = (lane + 64 * c) * 8;
        const u32x4 vx = *(const u32x4*)(px + col), vd = *(const u32x4*)(pd + col);
#pragma unroll
        for (int i = 0; i < 4; ++i) { xw[r][4 * c + i] = vx[i]; dw[r][4 * c + i] = vd[i]; }
      }
      if (C4) {
        const u32x2 vx = *(const u32x2*)(px + col4), vd = *(const u32x2*)(pd + col4);
        xw[r][4 * C8] = vx[0]; xw[r][4 * C8 + 1] = vx[1]; dw[r][4 * C8] = vd[0]; dw[r][4 * C8 + 1] = vd[1];
      }
    }
  };
  long g = (long)blockIdx.x * 4 + wave;
  if (g < ngroups) load_rows(g);
  for (; g < ngroups; g += stride) {
    float xv[R][E], gv[R][E];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool valid = g * R + r < a.M;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        xv[r][2 * k] = XF16 ? f16lo(xw[r][k]) : bf16lo(xw[r][k]);
        xv[r][2 * k + 1] = XF16 ? f16hi(xw[r][k]) : bf16hi(xw[r][k]);
        gv[r][2 * k] = valid ? bf16lo(dw[r][k]) : 0.f;
        gv[r][2 * k + 1] = valid ? bf16hi(dw[r][k]) : 0.f;
      }
    }
    if (g + stride < ngroups) load_rows(g + stride);
    float u[R], rs[R], m1[R], m2[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) s += xv[r][e];
      u[r] = s;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) u[r] = wave_sum_valu(u[r]) * invH;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) { const float d = xv[r][e] - u[r]; ss += d * d; }
      rs[r] = ss;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) rs[r] = 1.0f / sqrtf(wave_sum_valu(rs[r]) * invH + a.eps);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float xh = (xv[r][e] - u[r]) * rs[r];
        const float dyv = gv[r][e];
        if (PG) {
          dg[e] += dyv * xh;
          db[e] += dyv;
        }
        const float gg = dyv * gam[e];
        xv[r][e] = xh;
        gv[r][e] = gg;
        s1 += gg;
        s2 += gg * xh;
      }
      m1[r] = s1; m2[r] = s2;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) { m1[r] = wave_sum_valu(m1[r]) * invH; m2[r] = wave_sum_valu(m2[r]) * invH; }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long row = g * R + r;
      if (row < a.M) {
        bf16_t* po = a.dx + row * a.lddx;
        bf16_t* po2 = a.dx2 ? a.dx2 + row * a.lddx2 : nullptr;
        const uint32_t erow = (uint32_t)row * (uint32_t)H;
#pragma unroll
        for (int c = 0; c < C8; ++c) {
          const int col = (lane + 64 * c) * 8;
          float o[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) o[i] = rs[r] * (gv[r][8 * c + i] - m1[r] - xv[r][8 * c + i] * m2[r]);
          u32x4 w;
#pragma unroll
          for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(o[2 * i], o[2 * i + 1]);
          *(u32x4*)(po + col) = w;
          if (po2) {
            vt_drop_run<8>(a.drop, erow + (uint32_t)col, o);   // thresh 0: everything kept, scale 1
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(o[2 * i], o[2 * i + 1]);
            *(u32x4*)(po2 + col) = w;
          }
        }
        if (C4) {
          float o[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = rs[r] * (gv[r][8 * C8 + i] - m1[r] - xv[r][8 * C8 + i] * m2[r]);
          *(u32x2*)(po + col4) = (u32x2){pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
          if (po2) {
            vt_drop_run<4>(a.drop, erow + (uint32_t)col4, o);
            *(u32x2*)(po2 + col4) = (u32x2){pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
          }
        }
      }
    }
  }
  if (!PG) return;
  // block combine: 4 waves -> one partial row
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int col = e < 8 * C8 ? (lane + 64 * (e >> 3)) * 8 + (e & 7) : col4 + (e - 8 * C8);
    red[wave][0][col] = dg[e];
    red[wave][1][col] = db[e];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 2 * H; idx += 256) {
    const int which = idx >= H ? 1 : 0, col = idx - which * H;
    const float v = red[0][which][col] + red[1][which][col] + red[2][which][col] + red[3][which][col];
    a.partial[((long)blockIdx.x * 2 + which) * H + col] = v;
  }
}

// out[j] (+)= sum_b partial[b][j], j < n  (n = 2H: dgamma | dbeta; n % 4 == 0).  A block owns 16 columns (4 lanes x
// 16 bytes); its 64 row groups each sum every 64th partial row with independent 16-byte loads (1024 partial rows = 16
// loads per thread, all in flight), then combine through LDS.  (The first form -- 32 columns x 8 row groups, 128
// dependent-latency loads per thread on 48 workgroups -- took 12 us per call, as much as the LayerNorm backward itself
// at a small batch.)
__global__ __launch_bounds__(256) void ln_bwd_reduce(const float* __restrict__ partial, int nblocks, int n,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta, int H,
                                                     int accumulate, int n_main, PrefetchArgs pf) {
  __shared__ f32x4 red[64][4];
  if ((int)blockIdx.x >= n_main) {   // a spare workgroup: the weight prefetch riding along (see LnArgs::pf)
    vt_prefetch_role(pf, (int)blockIdx.x - n_main, (int)gridDim.x - n_main);
    return;
  }
  const int cg = threadIdx.x & 3, part = threadIdx.x >> 2;
  const int j = blockIdx.x * 16 + cg * 4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (j < n) {
    int b = part;
    for (; b + 192 < nblocks; b += 256) {
      const f32x4 v0 = *(const f32x4*)(partial + (long)b * n + j), v1 = *(const f32x4*)(partial + (long)(b + 64) * n + j);
      const f32x4 v2 = *(const f32x4*)(partial + (long)(b + 128) * n + j), v3 = *(const f32x4*)(partial + (long)(b + 192) * n + j);
      s += (v0 + v1) + (v2 + v3);
    }
    for (; b < nblocks; b += 64) s += *(const f32x4*)(partial + (long)b * n + j);
  }
  red[part][cg] = s;
  __syncthreads();
  for (int h = 32; h > 0; h >>= 1) {   // tree over the 64 row groups: a fixed order, reproducible
    if (part < h) red[part][cg] += red[part + h][cg];
    __syncthreads();
  }
  if (part == 0 && j < n) {
    const f32x4 t = red[0][cg];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int jj = j + k;
      float* dst = jj < H ? dgamma + jj : dbeta + (jj - H);
      *dst = accumulate ? *dst + t[k] : t[k];
    }
  }
}

#define LN_BWD_MAX_BLOCKS 1024
int vt_layernorm_bwd_dispatch(const void* x, long ldx, const void* dy, long ldy, const float* gamma, void* dx, long lddx,
                              float* dgamma, float* dbeta, float* partial_ws, int M, int H, float eps, int accumulate,
                              hipStream_t stream, void* dx2, long lddx2, const DropCfg* drop, int x_f16,
                              const PrefetchArgs* pf) {
  // dgamma == dbeta == NULL: dx only (the LayerNorm's parameters are frozen) -- the kernels' PG = false forms, no reduce launch,
  // partial_ws not touched (may be NULL) and the weight prefetch that rides in the reduce launch dropped with it
  const bool pg = dgamma != nullptr || dbeta != nullptr;
  if (!x || !dy || !gamma || !dx || (pg && (!dgamma || !dbeta || !partial_ws))) return VT_ERR_NULL;
  if (M <= 0 || H <= 0 || (H % 8) || H > 1024) return VT_ERR_BAD_SHAPE;
  if ((ldx % 8) || (ldy % 8) || (lddx % 8) || (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15)) return VT_ERR_BAD_ALIGN;
  LnBwdArgs a;
  a.x = (const bf16_t*)x; a.ldx = ldx; a.dy = (const bf16_t*)dy; a.ldy = ldy; a.gamma = gamma;
  a.dx = (bf16_t*)dx; a.lddx = lddx; a.partial = partial_ws; a.M = M; a.H = H; a.eps = eps;
  a.dx2 = (bf16_t*)dx2; a.lddx2 = lddx2;
  a.drop = drop ? *drop : vt_no_drop();
  if (dx2 && ((lddx2 % 8) || ((uintptr_t)dx2 & 15))) return VT_ERR_BAD_ALIGN;
  int nblocks = (M + 3) / 4;
  if (nblocks > LN_BWD_MAX_BLOCKS) nblocks = LN_BWD_MAX_BLOCKS;
  // VT_LN_BWD_ROWS: rows a wave holds at once (1, 2 or 4; 0 = the chunked kernel).  Measured at M = 50 820, H = 768 with the
  // masked second copy, cold operands, reduce kernel included (tools/ln_bench.py): chunked 74.9 us, 1 row 66.6 (122 registers,
  // four waves per SIMD), 2 rows 70.3 (182), 4 rows 78.3 (302); in the pretrain step 65.3 -> 51.5 us per launch.
  static const int rows_per_wave = (int)vt_switch(VT_LN_BWD_ROWS);
  if (rows_per_wave > 0 && (H == 768 || H == 512 || H == 1024 || H == 256) && (((uintptr_t)gamma) & 15) == 0) {
    const int R = rows_per_wave >= 4 ? 4 : rows_per_wave >= 2 ? 2 : 1;
    nblocks = (int)((((long)M + R - 1) / R + 3) / 4);
    if (nblocks > LN_BWD_MAX_BLOCKS) nblocks = LN_BWD_MAX_BLOCKS;
#define VT_LNB_LAUNCH_PG(C8, C4, RR, PG)                                                                                   \
    do {                                                                                                                   \
      if (x_f16) hipLaunchKernelGGL((layernorm_bwd_rows_full<C8, C4, RR, true, PG>), dim3(nblocks), dim3(256), 0, stream, a); \
      else hipLaunchKernelGGL((layernorm_bwd_rows_full<C8, C4, RR, false, PG>), dim3(nblocks), dim3(256), 0, stream, a);   \
    } while (0)
#define VT_LNB_LAUNCH(C8, C4, RR)                                                                                        \
    do {                                                                                                                 \
      if (pg) VT_LNB_LAUNCH_PG(C8, C4, RR, true); else VT_LNB_LAUNCH_PG(C8, C4, RR, false);                              \
    } while (0)
#define VT_LNB_SHAPE(RR)                                                                                                 \
    do {                                                                                                                 \
      if (H == 768) VT_LNB_LAUNCH(1, 1, RR); else if (H == 512) VT_LNB_LAUNCH(1, 0, RR);                                 \
      else if (H == 1024) VT_LNB_LAUNCH(2, 0, RR); else VT_LNB_LAUNCH(0, 1, RR);                                         \
    } while (0)
    if (R == 4) VT_LNB_SHAPE(4); else if (R == 2) VT_LNB_SHAPE(2); else VT_LNB_SHAPE(1);
#undef VT_LNB_SHAPE
#undef VT_LNB_LAUNCH
#undef VT_LNB_LAUNCH_PG
  } else {
#define VT_LNB_CHUNKED(CH, PG)                                                                                           \
    do {                                                                                                                 \
      if (x_f16) hipLaunchKernelGGL((layernorm_bwd_rows<CH, true, PG>), dim3(nblocks), dim3(256), 0, stream, a);         \
      else hipLaunchKernelGGL((layernorm_bwd_rows<CH, false, PG>), dim3(nblocks), dim3(256), 0, stream, a);              \
    } while (0)
    if (H <= 512) { if (pg) VT_LNB_CHUNKED(1, true); else VT_LNB_CHUNKED(1, false); }
    else { if (pg) VT_LNB_CHUNKED(2, true); else VT_LNB_CHUNKED(2, false); }
#undef VT_LNB_CHUNKED
  }
  if (pg) {
    const int n_main = (2 * H + 15) / 16;
    PrefetchArgs none;
    none.n = 0;
    for (int i = 0; i < 4; ++i) { none.p[i] = nullptr; none.bytes[i] = 0; }
    long extra = 0;
    if (pf && pf->n > 0) {
      for (int i = 0; i < pf->n; ++i) extra += (pf->bytes[i] + 16383) >> 14;
      extra = extra < 1 ? 1 : (extra > 640 ? 640 : extra);
    }
    hipLaunchKernelGGL(ln_bwd_reduce, dim3((unsigned)(n_main + extra)), dim3(256), 0, stream, partial_ws, nblocks, 2 * H, dgamma,
                       dbeta, H, accumulate, n_main, extra ? *pf : none);
  }
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
// workspace floats needed by vt_layernorm_bwd: LN_BWD_MAX_BLOCKS * 2 * H

// ---------------------------------------------------------------------------------------------
// Backward of embed_layernorm: recompute e = word + pos + type (fp32, as the forward did), run the
// LayerNorm backward against the incoming gradient rows b*S+t of g, and emit d_e (fp32 [B*T,H]) for
// the three table scatter-adds, plus dgamma/dbeta partial rows (same scheme as layernorm_bwd_rows).
struct EmbBwdArgs {
  const int64_t* ids; const int64_t* type_ids; const int64_t* pos_ids;
  const float* word; const float* pos; const float* type;
  const float* gamma;
  const bf16_t* g; long ldg;   // gradient rows b*S + t
  float* de;                   // [B*T, H]
  float* partial;              // [gridDim.x][2][H]
  int B, T, S, H;
  int n_word, n_pos, n_type;
  float eps;
  DropCfg drop;  // same mask as the forward: the incoming gradient is masked and scaled first
};

template <int CH>
__global__ __launch_bounds__(256) void embed_layernorm_bwd(EmbBwdArgs a) {
  __shared__ float red[4][2][CH * 512];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float gam[CH][8], dg[CH][8], db[CH][8];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int col = (lane + 64 * c) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      dg[c][i] = 0.f; db[c][i] = 0.f;
      gam[c][i] = col < a.H ? a.gamma[col + i] : 0.f;
    }
  }
  const float invH = 1.0f / (float)a.H;
  const long ntok = (long)a.B * a.T;
  for (long tok = (long)blockIdx.x * 4 + wave; tok < ntok; tok += (long)gridDim.x * 4) {
    const int b = (int)(tok / a.T), t = (int)(tok - (long)b * a.T);
    long wi = a.ids[tok];
    long pi = a.pos_ids ? a.pos_ids[tok] : (long)t;
    long ti = a.type_ids ? a.type_ids[tok] : 0L;
    wi = wi < 0 ? 0 : (wi >= a.n_word ? a.n_word - 1 : wi);
    pi = pi < 0 ? 0 : (pi >= a.n_pos ? a.n_pos - 1 : pi);
    ti = ti < 0 ? 0 : (ti >= a.n_type ? a.n_type - 1 : ti);
    const float* wp = a.word + wi * a.H;
    const float* pp = a.pos + pi * a.H;
    const float* tp = a.type + ti * a.H;
    const bf16_t* gp = a.g + ((long)b * a.S + t) * a.ldg;
    float xv[CH][8], gv[CH][8];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int col = (lane + 64 * c) * 8;
      if (col < a.H) {
#pragma unroll
        for (int hlf = 0; hlf < 2; ++hlf) {
          const f32x4 w4 = *(const f32x4*)(wp + col + 4 * hlf);
          const f32x4 p4 = *(const f32x4*)(pp + col + 4 * hlf);
          const f32x4 t4 = *(const f32x4*)(tp + col + 4 * hlf);
#pragma unroll
          for (int i = 0; i < 4; ++i) { xv[c][4 * hlf + i] = (w4[i] + p4[i]) + t4[i]; s += xv[c][4 * hlf + i]; }
        }
        const u32x4 d = *(const u32x4*)(gp + col);
#pragma unroll
        for (int i = 0; i < 4; ++i) { gv[c][2 * i] = bf16lo(d[i]); gv[c][2 * i + 1] = bf16hi(d[i]); }
        if (a.drop.thresh) {
          const uint32_t e0 = (uint32_t)tok * (uint32_t)a.H + (uint32_t)col;
          vt_drop_run<8>(a.drop, e0, gv[c]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) { xv[c][i] = 0.f; gv[c][i] = 0.f; }
      }
    }
    const float u = wave_sum(s) * invH;
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int col = (lane + 64 * c) * 8;
      if (col < a.H) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float d = xv[c][i] - u; ss += d * d; }
      }
    }
    const float rs = 1.0f / sqrtf(wave_sum(ss) * invH + a.eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int col = (lane + 64 * c) * 8;
      if (col < a.H) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float xh = (xv[c][i] - u) * rs;
          const float dyv = gv[c][i];
          dg[c][i] += dyv * xh;
          db[c][i] += dyv;
          const float gg = dyv * gam[c][i];
          xv[c][i] = xh;
          gv[c][i] = gg;
          s1 += gg;
          s2 += gg * xh;
        }
      }
    }
    const float m1 = wave_sum(s1) * invH, m2 = wave_sum(s2) * invH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int col = (lane + 64 * c) * 8;
      if (col < a.H) {
        float* op = a.de + tok * a.H + col;
        f32x4 o0, o1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          o0[i] = rs * (gv[c][i] - m1 - xv[c][i] * m2);
          o1[i] = rs * (gv[c][4 + i] - m1 - xv[c][4 + i] * m2);
        }
        *(f32x4*)op = o0;
        *(f32x4*)(op + 4) = o1;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      red[wave][0][(lane + 64 * c) * 8 + i] = dg[c][i];
      red[wave][1][(lane + 64 * c) * 8 + i] = db[c][i];
    }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 2 * a.H; idx += 256) {
    const int which = idx / a.H, col = idx - which * a.H;
    a.partial[((long)blockIdx.x * 2 + which) * a.H + col] =
        red[0][which][col] + red[1][which][col] + red[2][which][col] + red[3][which][col];
  }
}

int vt_embed_layernorm_bwd_dispatch(const int64_t* ids, const int64_t* type_ids, const int64_t* pos_ids, const float* word,
                                    const float* pos, const float* type, const float* gamma, const void* g, long ldg,
                                    float* de, float* dgamma, float* dbeta, float* partial_ws, int B, int T, int S, int H,
                                    int n_word, int n_pos, int n_type, float eps, int accumulate, hipStream_t stream,
                                    const DropCfg* drop) {
  if (!ids || !word || !pos || !type || !gamma || !g || !de || !dgamma || !dbeta || !partial_ws) return VT_ERR_NULL;
  if (B <= 0 || T <= 0 || S < T || H <= 0 || (H % 8) || H > 1024) return VT_ERR_BAD_SHAPE;
  if ((ldg % 8) || (((uintptr_t)word | (uintptr_t)pos | (uintptr_t)type | (uintptr_t)g | (uintptr_t)de) & 15)) return VT_ERR_BAD_ALIGN;
  EmbBwdArgs a;
  a.ids = ids; a.type_ids = type_ids; a.pos_ids = pos_ids; a.word = word; a.pos = pos; a.type = type; a.gamma = gamma;
  a.g = (const bf16_t*)g; a.ldg = ldg; a.de = de; a.partial = partial_ws; a.B = B; a.T = T; a.S = S; a.H = H;
  a.n_word = n_word; a.n_pos = n_pos; a.n_type = n_type; a.eps = eps;
  a.drop = drop ? *drop : vt_no_drop();
  long nb = ((long)B * T + 3) / 4;
  const int nblocks = (int)(nb > LN_BWD_MAX_BLOCKS ? LN_BWD_MAX_BLOCKS : nb);
  if (H <= 512) hipLaunchKernelGGL(embed_layernorm_bwd<1>, dim3(nblocks), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(embed_layernorm_bwd<2>, dim3(nblocks), dim3(256), 0, stream, a);
  PrefetchArgs none;
  none.n = 0;
  for (int i = 0; i < 4; ++i) { none.p[i] = nullptr; none.bytes[i] = 0; }
  hipLaunchKernelGGL(ln_bwd_reduce, dim3((2 * H + 15) / 16), dim3(256), 0, stream, partial_ws, nblocks, 2 * H, dgamma,
                     dbeta, H, accumulate, (2 * H + 15) / 16, none);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
