// Row kernels of the fp32 training step (PretrainEngine(..., precision="fp32"), visitron_amd/training_f32.py).
//
// The reference trains in fp32 (tasks/viewpoint_select/pretrain.py:191, no AMP).  The products of that step run on
// gemm_f32_128 (fp32_path.hip: A-transposed operand, K split, dropout / pre-activation epilogue); what is not a product is
// here, fp32 everywhere, with no float atomics (every reduction has a fixed order, so a step is bitwise reproducible):
//
//   colsum_f32          out (+)= column sums of x [rows, cols]: bias gradients, and the LayerNorm dgamma / dbeta partials
//   ln_bwd_f32          BertLayerNorm backward from the saved input: dx, optionally dx * keep / (1 - p) of a dropout site
//                       (the dense output's gradient), an input dropout mask on g (the embedding / image sites), and the
//                       per-block dgamma / dbeta partials
//   attn_softmax_train  x / 8 + mask -> softmax P (kept for the backward) and P * keep / (1 - p) * head_mask (the product's
//                       operand), the reference's (1 - m) * -10000 mask arithmetic (oscar/modeling_bert.py:53-66)
//   attn_softmax_bwd    dS = P (g - rowsum(g P)) / 8 with g = dP * keep / (1 - p) * head_mask
//   dgelu_f32           g * GELU'(pre) of the erf form
//   embed_sum_f32       word + position + token_type rows (the embedding LayerNorm's input, saved for its backward)
//   dropout_rows_f32    y = x * keep / (1 - p) with a row remap on the input (the image rows' gradient)
#include "dispatch.hpp"

#define CS_ROWS 256   // rows per partial of colsum_f32: the partial count is a function of the row count only

// partial[chunk][col] = sum of rows chunk * 256 .. + 255 of column col, 4 row groups combined in a fixed order
__global__ __launch_bounds__(256) void colsum_partial_f32(const float* __restrict__ x, long ldx, long rows, int cols,
                                                          float* __restrict__ partial) {
  __shared__ float red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + tx;
  const long r0 = (long)blockIdx.y * CS_ROWS;
  float s = 0.f;
  if (col < cols) {
    for (int i = ty; i < CS_ROWS; i += 4) {
      const long r = r0 + i;
      if (r < rows) s += x[r * ldx + col];
    }
  }
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && col < cols) partial[(long)blockIdx.y * cols + col] = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
}

__global__ __launch_bounds__(256) void colsum_final_f32(const float* __restrict__ partial, int nchunk, int cols,
                                                        float* __restrict__ out, int accumulate) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= cols) return;
  float s = 0.f;
  for (int k = 0; k < nchunk; ++k) s += partial[(long)k * cols + col];
  out[col] = accumulate ? out[col] + s : s;
}

int vt_colsum_f32_dispatch(const float* x, long ldx, long rows, int cols, float* out, int accumulate, float* ws,
                           hipStream_t stream) {
  if (!x || !out || !ws) return VT_ERR_NULL;
  if (rows <= 0 || cols <= 0 || ldx < cols) return VT_ERR_BAD_SHAPE;
  const long nchunk = (rows + CS_ROWS - 1) / CS_ROWS;
  if (nchunk > 65535) return VT_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(colsum_partial_f32, dim3((unsigned)((cols + 63) / 64), (unsigned)nchunk), dim3(256), 0, stream, x, ldx, rows,
                     cols, ws);
  hipLaunchKernelGGL(colsum_final_f32, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, stream, ws, (int)nchunk, cols, out,
                     accumulate);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm backward, one wave per row (a block's 4 waves walk the rows with a stride of 4 * gridDim.x):
//   g' = g[remap(row)] * keep_in / (1 - p_in)                         (optional input dropout: the embedding / image sites)
//   xhat = (x - u) * rstd,  dxhat = g' * gamma
//   dx = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat))
//   dx_drop = dx * keep_out / (1 - p_out)                              (optional: the gradient of a dropped dense output)
//   partial[block] = [sum g' xhat | sum g'] over the block's rows (fixed order; colsum_f32 sums the blocks)
struct LnBwdF32Args {
  const float* x; long ldx;
  const float* g; long ldg; int grp_rows, grp_stride;   // g row of row r: (r / grp_rows) * grp_stride + r % grp_rows
  const float* gamma;
  float* dx; long lddx;
  float* dx_drop; long ldd;
  float* partial;   // [gridDim.x, 2H]
  long M; int H; float eps;
  DropCfg din, dout;
};

#define LNB_MAXC 4   // H <= 64 * 4 * 4 = 1024

__global__ __launch_bounds__(256) void ln_bwd_f32(LnBwdF32Args a) {
  __shared__ float red[4][2 * 64 * 4 * LNB_MAXC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float dg[LNB_MAXC][4], db[LNB_MAXC][4];
#pragma unroll
  for (int c = 0; c < LNB_MAXC; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) { dg[c][i] = 0.f; db[c][i] = 0.f; }
  for (long row = (long)blockIdx.x * 4 + wave; row < a.M; row += 4L * gridDim.x) {
    const long grow = a.grp_rows ? (row / a.grp_rows) * a.grp_stride + (row % a.grp_rows) : row;
    float xv[LNB_MAXC][4], gv[LNB_MAXC][4];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < LNB_MAXC; ++c) {
      const int col = (lane + 64 * c) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) { xv[c][i] = 0.f; gv[c][i] = 0.f; }
      if (col < a.H) {
        const f32x4 t = *(const f32x4*)(a.x + row * a.ldx + col);
        const f32x4 u = *(const f32x4*)(a.g + grow * a.ldg + col);
#pragma unroll
        for (int i = 0; i < 4; ++i) { xv[c][i] = t[i]; gv[c][i] = u[i]; s += t[i]; }
        if (a.din.thresh) {
#pragma unroll
          for (int i = 0; i < 4; ++i) gv[c][i] = vt_keep(a.din, (uint32_t)(row * a.H + col + i)) ? gv[c][i] * a.din.scale : 0.f;
        }
      }
    }
    const float mu = wave_sum(s) / (float)a.H;
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < LNB_MAXC; ++c) {
      const int col = (lane + 64 * c) * 4;
      if (col < a.H) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float d = xv[c][i] - mu; ss += d * d; }
      }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)a.H + a.eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < LNB_MAXC; ++c) {
      const int col = (lane + 64 * c) * 4;
      if (col < a.H) {
        const f32x4 g4 = *(const f32x4*)(a.gamma + col);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xv[c][i] = (xv[c][i] - mu) * rstd;                // xhat
          dg[c][i] += gv[c][i] * xv[c][i];
          db[c][i] += gv[c][i];
          gv[c][i] *= g4[i];                                // dxhat
          s1 += gv[c][i];
          s2 += gv[c][i] * xv[c][i];
        }
      }
    }
    const float m1 = wave_sum(s1) / (float)a.H, m2 = wave_sum(s2) / (float)a.H;
#pragma unroll
    for (int c = 0; c < LNB_MAXC; ++c) {
      const int col = (lane + 64 * c) * 4;
      if (col < a.H) {
        f32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = rstd * (gv[c][i] - m1 - xv[c][i] * m2);
        if (a.dx) *(f32x4*)(a.dx + row * a.lddx + col) = o;
        if (a.dx_drop) {
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = vt_keep(a.dout, (uint32_t)(row * a.H + col + i)) ? o[i] * a.dout.scale : 0.f;
          *(f32x4*)(a.dx_drop + row * a.ldd + col) = o;
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < LNB_MAXC; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int col = (lane + 64 * c) * 4 + i;
      red[wave][col] = dg[c][i];
      red[wave][64 * 4 * LNB_MAXC + col] = db[c][i];
    }
  __syncthreads();
  for (int j = threadIdx.x; j < 2 * a.H; j += 256) {
    const int src = j < a.H ? j : 64 * 4 * LNB_MAXC + (j - a.H);
    a.partial[(long)blockIdx.x * 2 * a.H + j] = ((red[0][src] + red[1][src]) + red[2][src]) + red[3][src];
  }
}

// the block count of ln_bwd_f32 (a function of the row count only: the dgamma / dbeta sums keep their order)
int vt_ln_bwd_f32_blocks(long M) {
  const long b = (M + 3) / 4;
  return (int)(b < 512 ? b : 512);
}

int vt_ln_bwd_f32_dispatch(const float* x, long ldx, const float* g, long ldg, int grp_rows, int grp_stride, const float* gamma,
                           float* dx, long lddx, float* dx_drop, long ldd, float* partial, long M, int H, float eps, DropCfg din,
                           DropCfg dout, hipStream_t stream) {
  if (!x || !g || !gamma || !partial) return VT_ERR_NULL;
  if (M <= 0 || H <= 0 || (H % 4) || H > 64 * 4 * LNB_MAXC) return VT_ERR_BAD_SHAPE;
  if (grp_rows < 0 || (grp_rows > 0 && grp_stride < grp_rows)) return VT_ERR_BAD_SHAPE;
  if ((ldx % 4) || (ldg % 4) || (dx && (lddx % 4)) || (dx_drop && (ldd % 4))) return VT_ERR_BAD_ALIGN;
  if ((((uintptr_t)x | (uintptr_t)g | (uintptr_t)gamma | (uintptr_t)dx | (uintptr_t)dx_drop) & 15)) return VT_ERR_BAD_ALIGN;
  LnBwdF32Args a;
  a.x = x; a.ldx = ldx; a.g = g; a.ldg = ldg; a.grp_rows = grp_rows; a.grp_stride = grp_stride; a.gamma = gamma;
  a.dx = dx; a.lddx = lddx; a.dx_drop = dx_drop; a.ldd = ldd; a.partial = partial; a.M = M; a.H = H; a.eps = eps;
  a.din = din; a.dout = dout;
  hipLaunchKernelGGL(ln_bwd_f32, dim3((unsigned)vt_ln_bwd_f32_blocks(M)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------------------------
// Attention probabilities of a training step, one wave per row r = (b * nh + h) * S + q of the scores x [rows, S] (in place):
//   P = softmax(x * scale + mask)           -> x   (kept for the backward)
//   Pd = P * keep / (1 - p) * head_scale[h] -> pd  (the operand of the context product)
// mask_mode: -1 none, 0 raw [B, S] -> (1 - m) * -10000 (encoder.py:238-241), 2 additive per query [B, S, S].
// keep: the attention site's decision for (b, h, q, k): hash stream vt_hash32(site seed, b * nh + h), element q * pitch + k,
// pitch = S rounded up to a multiple of 4 -- the bf16 kernels' decisions on their padded layout (vt_keep_attn).
struct AttnTrainArgs {
  float* x; float* pd; long ld; long rows; int S, nh;
  float scale;
  const float* mask; int mask_mode;
  const float* head_scale;
  DropCfg drop;
};

__device__ __forceinline__ bool attn_keep_row(const DropCfg& d, uint32_t head_seed, uint32_t idx) {
  DropCfg dh = d;
  dh.seed = head_seed;
  return vt_keep_attn(dh, idx);
}

__global__ __launch_bounds__(256) void attn_softmax_train_f32(AttnTrainArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const long bh = row / a.S;
  const int q = (int)(row - bh * a.S);
  const int b = (int)(bh / a.nh), h = (int)(bh - (long)b * a.nh);
  float* xp = a.x + row * a.ld;
  float* pp = a.pd + row * a.ld;
  const float* mp = nullptr;
  if (a.mask_mode == 0) mp = a.mask + (long)b * a.S;
  else if (a.mask_mode == 2) mp = a.mask + ((long)b * a.S + q) * a.S;
  float mx = -INFINITY;
  for (int c = lane; c < a.S; c += 64) {
    float v = xp[c] * a.scale;
    if (mp) v += (a.mask_mode == 0) ? (1.0f - mp[c]) * -10000.0f : mp[c];
    xp[c] = v;
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int c = lane; c < a.S; c += 64) {
    const float e = expf(xp[c] - mx);
    xp[c] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  const float hs = a.head_scale ? a.head_scale[h] : 1.0f;
  const uint32_t hseed = vt_hash32(a.drop.seed, (uint32_t)bh);
  const int pitch = (a.S + 3) & ~3;
  for (int c = lane; c < a.S; c += 64) {
    const float p = xp[c] / sum;
    xp[c] = p;
    float v = p;
    if (a.drop.thresh) v = attn_keep_row(a.drop, hseed, (uint32_t)(q * pitch + c)) ? v * a.drop.scale : 0.f;
    pp[c] = v * hs;
  }
}

// dS = P (g - rowsum(g P)) * scale, g = dPd * keep / (1 - p) * head_scale; in place on dp
__global__ __launch_bounds__(256) void attn_softmax_bwd_f32(AttnTrainArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const long bh = row / a.S;
  const int q = (int)(row - bh * a.S);
  const int b = (int)(bh / a.nh), h = (int)(bh - (long)b * a.nh);
  const float* P = a.x + row * a.ld;
  float* dp = a.pd + row * a.ld;
  const float hs = a.head_scale ? a.head_scale[h] : 1.0f;
  const uint32_t hseed = vt_hash32(a.drop.seed, (uint32_t)bh);
  const int pitch = (a.S + 3) & ~3;
  float dot = 0.f;
  for (int c = lane; c < a.S; c += 64) {
    float g = dp[c];
    if (a.drop.thresh) g = attn_keep_row(a.drop, hseed, (uint32_t)(q * pitch + c)) ? g * a.drop.scale : 0.f;
    g *= hs;
    dp[c] = g;
    dot += g * P[c];
  }
  dot = wave_sum(dot);
  for (int c = lane; c < a.S; c += 64) dp[c] = P[c] * (dp[c] - dot) * a.scale;
}

int vt_attn_softmax_f32_dispatch(int backward, float* x, float* pd, long ld, int B, int nh, int S, float scale, const float* mask,
                                 int mask_mode, const float* head_scale, DropCfg drop, hipStream_t stream) {
  if (!x || !pd) return VT_ERR_NULL;
  if (B <= 0 || nh <= 0 || S <= 0 || ld < S) return VT_ERR_BAD_SHAPE;
  if (mask_mode != -1 && mask_mode != 0 && mask_mode != 2) return VT_ERR_UNSUPPORTED;
  if (mask_mode >= 0 && !mask) return VT_ERR_NULL;
  AttnTrainArgs a;
  a.x = x; a.pd = pd; a.ld = ld; a.rows = (long)B * nh * S; a.S = S; a.nh = nh; a.scale = scale; a.mask = mask;
  a.mask_mode = mask ? mask_mode : -1; a.head_scale = head_scale; a.drop = drop;
  const dim3 grid((unsigned)((a.rows + 3) / 4));
  if (backward) hipLaunchKernelGGL(attn_softmax_bwd_f32, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(attn_softmax_train_f32, grid, dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------------------------
// out = g * GELU'(pre), GELU(x) = x / 2 (1 + erf(x / sqrt 2)): GELU'(x) = (1 + erf(x / sqrt 2)) / 2 + x exp(-x^2 / 2) / sqrt(2 pi)
__global__ __launch_bounds__(256) void dgelu_f32(const float* __restrict__ g, const float* __restrict__ pre, float* __restrict__ out,
                                                 long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = pre[i];
  const float d = 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * expf(-0.5f * x * x) * 0.39894228040143268f;
  out[i] = g[i] * d;
}

int vt_dgelu_f32_dispatch(const float* g, const float* pre, float* out, long n, hipStream_t stream) {
  if (!g || !pre || !out) return VT_ERR_NULL;
  if (n <= 0) return VT_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(dgelu_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, g, pre, out, n);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------------------------
// e[b*T + t] = (word[id] + pos[pid]) + type[tid] (BertEmbeddings' sum, encoder.py:267-269; the order of embed_layernorm_f32)
struct EmbSumArgs {
  const int64_t* ids; const int64_t* type_ids; const int64_t* pos_ids;
  const float* word; const float* pos; const float* type;
  float* e; int B, T, H, n_word, n_pos, n_type;
  int* err;
};

__global__ __launch_bounds__(256) void embed_sum_f32(EmbSumArgs a) {
  const int tok = blockIdx.x;
  const int t = tok % a.T;
  long wi = a.ids[tok];
  long pi = a.pos_ids ? a.pos_ids[tok] : (long)t;
  long ti = a.type_ids ? a.type_ids[tok] : 0L;
  if (wi < 0 || wi >= a.n_word || pi < 0 || pi >= a.n_pos || ti < 0 || ti >= a.n_type) {
    if (threadIdx.x == 0 && a.err) *a.err = 1;
    wi = wi < 0 ? 0 : (wi >= a.n_word ? a.n_word - 1 : wi);
    pi = pi < 0 ? 0 : (pi >= a.n_pos ? a.n_pos - 1 : pi);
    ti = ti < 0 ? 0 : (ti >= a.n_type ? a.n_type - 1 : ti);
  }
  for (int c = threadIdx.x; c < a.H; c += 256)
    a.e[(long)tok * a.H + c] = (a.word[wi * a.H + c] + a.pos[pi * a.H + c]) + a.type[ti * a.H + c];
}

int vt_embed_sum_f32_dispatch(const int64_t* ids, const int64_t* type_ids, const int64_t* pos_ids, const float* word,
                              const float* pos, const float* type, float* e, int B, int T, int H, int n_word, int n_pos,
                              int n_type, int* err, hipStream_t stream) {
  if (!ids || !word || !pos || !type || !e) return VT_ERR_NULL;
  if (B <= 0 || T <= 0 || H <= 0) return VT_ERR_BAD_SHAPE;
  EmbSumArgs a;
  a.ids = ids; a.type_ids = type_ids; a.pos_ids = pos_ids; a.word = word; a.pos = pos; a.type = type; a.e = e;
  a.B = B; a.T = T; a.H = H; a.n_word = n_word; a.n_pos = n_pos; a.n_type = n_type; a.err = err;
  hipLaunchKernelGGL(embed_sum_f32, dim3((unsigned)(B * T)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------------------------
// y[r] = x[remap(r)] * keep / (1 - p), element index r * cols + c (x row of r: (r / grp_rows) * grp_stride + r % grp_rows)
__global__ __launch_bounds__(256) void dropout_rows_f32(const float* __restrict__ x, long ldx, int grp_rows, int grp_stride,
                                                        float* __restrict__ y, long ldy, long rows, int cols, DropCfg d) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cols) return;
  const long r = i / cols, c = i - r * cols;
  const long xr = grp_rows ? (r / grp_rows) * grp_stride + (r % grp_rows) : r;
  const float v = x[xr * ldx + c];
  y[r * ldy + c] = (d.thresh == 0 || vt_keep(d, (uint32_t)i)) ? v * d.scale : 0.f;
}

int vt_dropout_rows_f32_dispatch(const float* x, long ldx, int grp_rows, int grp_stride, float* y, long ldy, long rows, int cols,
                                 DropCfg d, hipStream_t stream) {
  if (!x || !y) return VT_ERR_NULL;
  if (rows <= 0 || cols <= 0 || (grp_rows > 0 && grp_stride < grp_rows)) return VT_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(dropout_rows_f32, dim3((unsigned)((rows * cols + 255) / 256)), dim3(256), 0, stream, x, ldx, grp_rows,
                     grp_stride, y, ldy, rows, cols, d);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
