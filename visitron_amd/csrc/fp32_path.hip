// fp32 parity path of the encoder hot path (BASELINE north_star: "logits within 1e-3 of the CPU reference").
//
// The reference computes in fp32 throughout (tasks/viewpoint_select/encoder.py:238-240, no AMP anywhere); the bf16
// kernels of this library cannot meet 1e-3 (bf16 weights alone put ~8e-3 RMS on sequence_output).  These kernels keep
// EVERY operand, activation and accumulation in fp32 -- the matrix products run on the exact-fp32 matrix cores of
// gfx950 (v_mfma_f32_32x32x2_f32) -- and are selected per model (`visitron_amd.set_precision(model, "fp32")`).
// They are a correctness mode: plainly tiled, not tuned like the bf16 kernels.
//
//   gemm_f32_128        C = act(alpha * A . op(W) + bias) (+ R)     every nn.Linear (oscar/modeling_bert.py:43-45, :94,
//                       :119, :120; encoder.py:277-279, :296, :377-391) and, batched over (batch, head), the two
//                       attention products torch.matmul(q, k^T) / torch.matmul(probs, v) (oscar/modeling_bert.py:52,68)
//   softmax_rows_f32    x/sqrt(d) + mask -> Softmax(dim=-1) [* head_mask]   (oscar/modeling_bert.py:53-66); also the token
//                       head's nn.Softmax (encoder.py:323-326)
//   layernorm_rows_f32  BertLayerNorm, fp32 or bf16 rows in, fp32 or bf16 rows out
//   embed_layernorm_f32 BertEmbeddings (encoder.py:267-269) with fp32 output
//
// Training (PretrainEngine(..., precision="fp32"), fp32_train.hip) reuses gemm_f32_128 for every product of the step: the
// A-transposed operand (a_is_km) gives the weight gradients dW = dY^T . X and the attention's dK = dS^T . Q / dV = P^T . dC,
// a fixed-order split of the K range (partial planes, summed in order by gemm_f32_split_reduce) keeps a long token-row
// reduction on the whole chip, and the epilogue can save the pre-activation, apply a dropout site and accumulate into C.
#include "dispatch.hpp"

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

struct GemmF32Args {
  const float* A; long lda; long sA_b, sA_h;
  const float* W; long ldw; long sW_b, sW_h;
  const float* bias; const float* R; long ldr;
  float* C; long ldc; long sC_b, sC_h;
  int M, N, K;
  int act;          // VT_ACT_NONE / VT_ACT_GELU / VT_ACT_TANH
  int w_is_kn;      // 0: W is [N, K] (row n holds the K weights of output n -- nn.Linear.weight); 1: W is [K, N]
  int heads;        // blockIdx.z = b * heads + h
  int grp_rows, grp_stride;   // output row remap as in the bf16 GEMM (0: identity)
  int vec_a, vec_w; // 16-byte loads allowed (aligned base, stride and K / N multiples of 4)
  float alpha;
  // training forms (fp32_train.hip; all zero / null in the inference entry points)
  int a_is_km;      // 0: A is [M, K]; 1: A is [K, M] (element (m, k) at A[k * lda + m]: dY^T of a weight gradient)
  int accumulate;   // C += result (C's old value is added after the residual)
  int split, kchunk;  // blockIdx.z = (b * heads + h) * split + s; split s covers K range [s * kchunk, (s + 1) * kchunk)
  float* ws;        // split > 1: partial plane s at ws + s * M * N (row-major [M, N], alpha applied, nothing else)
  float* pre;       // saved alpha * acc + bias before the activation (same layout as C), or null
  DropCfg drop;     // dropout of act(...) before the residual add, element index = row * N + col (row before the remap)
};

#define GF_BM 128
#define GF_BN 128
#define GF_BK 16
#define GF_LD 132   // LDS row pitch in floats: 16-byte aligned rows, conflict-free transposed stores

__device__ __forceinline__ float gf_act(float v, int act) {
  if (act == 1) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));   // erf-GELU (hidden_act == "gelu")
  if (act == 2) return tanhf(v);
  return v;
}

__global__ __launch_bounds__(256) void gemm_f32_128(GemmF32Args g) {
  __shared__ __attribute__((aligned(16))) float As[2][GF_BK][GF_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2][GF_BK][GF_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * GF_BM, n0 = blockIdx.x * GF_BN;
  const int zs = blockIdx.z % g.split, zbh = blockIdx.z / g.split;
  const int zb = zbh / g.heads, zh = zbh - zb * g.heads;
  const int kbeg = zs * g.kchunk, kend = min(g.K, kbeg + g.kchunk);
  const float* A = g.A + zb * g.sA_b + zh * g.sA_h;
  const float* W = g.W + zb * g.sW_b + zh * g.sW_h;
  float* C = g.C + zb * g.sC_b + zh * g.sC_h;

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

  // global -> register staging: rows x 16 k-values; a thread owns two (row, k-quad) pieces: row = tid/4 (+64), kq = tid%4
  float ra[2][4], rb[2][4];
  const int ld_row = tid >> 2, ld_kq = (tid & 3) * 4;
  auto load_rowmajor = [&](const float* base, long ld, int row0, int nrows, int k0, bool vec, float (&r)[2][4]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int row = row0 + ld_row + 64 * p;
      const int k = k0 + ld_kq;
      if (row < nrows && vec && k + 3 < kend) {
        const f32x4 v = *(const f32x4*)(base + (long)row * ld + k);
        r[p][0] = v[0]; r[p][1] = v[1]; r[p][2] = v[2]; r[p][3] = v[3];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) r[p][i] = (row < nrows && k + i < kend) ? base[(long)row * ld + k + i] : 0.f;
      }
    }
  };
  // W given as [K, N]: a thread owns two (k, n-quad) pieces: k = tid/32 (+8), n = (tid%32)*4
  // an operand given as [K, cols] (W with w_is_kn, A with a_is_km): a thread owns two (k, col-quad) pieces: k = tid/32 (+8),
  // col = (tid%32)*4
  auto load_kx = [&](const float* base, long ld, int c0, int ncols, bool vec, int k0, float (&r)[2][4]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int k = k0 + (tid >> 5) + 8 * p;
      const int n = c0 + (tid & 31) * 4;
      if (k < kend && vec && n + 3 < ncols) {
        const f32x4 v = *(const f32x4*)(base + (long)k * ld + n);
        r[p][0] = v[0]; r[p][1] = v[1]; r[p][2] = v[2]; r[p][3] = v[3];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) r[p][i] = (k < kend && n + i < ncols) ? base[(long)k * ld + n + i] : 0.f;
      }
    }
  };
  auto load_kn = [&](int k0, float (&r)[2][4]) { load_kx(W, g.ldw, n0, g.N, g.vec_w != 0, k0, r); };
  auto load_a = [&](int k0) {
    if (g.a_is_km) load_kx(A, g.lda, m0, g.M, g.vec_a != 0, k0, ra);
    else load_rowmajor(A, g.lda, m0, g.M, k0, g.vec_a != 0, ra);
  };
  auto store_tile = [&](int buf) {
    if (g.a_is_km) {
#pragma unroll
      for (int p = 0; p < 2; ++p) *(f32x4*)&As[buf][(tid >> 5) + 8 * p][(tid & 31) * 4] = (f32x4){ra[p][0], ra[p][1], ra[p][2], ra[p][3]};
    } else {
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) As[buf][ld_kq + i][ld_row + 64 * p] = ra[p][i];
    }
    if (g.w_is_kn) {
#pragma unroll
      for (int p = 0; p < 2; ++p) *(f32x4*)&Bs[buf][(tid >> 5) + 8 * p][(tid & 31) * 4] = (f32x4){rb[p][0], rb[p][1], rb[p][2], rb[p][3]};
    } else {
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[buf][ld_kq + i][ld_row + 64 * p] = rb[p][i];
    }
  };

  const int nk = (kend - kbeg + GF_BK - 1) / GF_BK;
  load_a(kbeg);
  if (g.w_is_kn) load_kn(kbeg, rb); else load_rowmajor(W, g.ldw, n0, g.N, kbeg, g.vec_w != 0, rb);
  store_tile(0);
  __syncthreads();
  const int fr = lane & 31, fk = lane >> 5;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) {
      const int kn = kbeg + (kt + 1) * GF_BK;
      load_a(kn);
      if (g.w_is_kn) load_kn(kn, rb); else load_rowmajor(W, g.ldw, n0, g.N, kn, g.vec_w != 0, rb);
    }
#pragma unroll
    for (int kk = 0; kk < GF_BK; kk += 2) {
      const float a0 = As[buf][kk + fk][wm * 64 + fr], a1 = As[buf][kk + fk][wm * 64 + 32 + fr];
      const float b0 = Bs[buf][kk + fk][wn * 64 + fr], b1 = Bs[buf][kk + fk][wn * 64 + 32 + fr];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tile(buf ^ 1);   // the other buffer: its last readers passed the barrier below one step ago
    __syncthreads();
  }

  // epilogue: accumulator v of lane l = C[8 (v/4) + 4 (l/32) + v%4][l%32] of its 32x32 tile
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 64 + 32 * j + fr;
      if (col >= g.N) continue;
      const float bv = g.bias ? g.bias[col] : 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = m0 + wm * 64 + 32 * i + 8 * (v >> 2) + 4 * fk + (v & 3);
        if (row >= g.M) continue;
        if (g.split > 1) {   // a partial plane: summed in split order by gemm_f32_split_reduce
          g.ws[((long)zs * g.M + row) * g.N + col] = acc[i][j][v] * g.alpha;
          continue;
        }
        const float pv = acc[i][j][v] * g.alpha + bv;
        const long orow = g.grp_rows ? (long)(row / g.grp_rows) * g.grp_stride + (row % g.grp_rows) : (long)row;
        if (g.pre) g.pre[orow * g.ldc + col] = pv;
        float x = gf_act(pv, g.act);
        if (g.drop.thresh) x = vt_keep(g.drop, (uint32_t)((long)row * g.N + col)) ? x * g.drop.scale : 0.f;
        if (g.R) x += g.R[(long)row * g.ldr + col];
        if (g.accumulate) x += C[orow * g.ldc + col];
        C[orow * g.ldc + col] = x;
      }
    }
}

int vt_gemm_f32_dispatch(const float* A, long lda, long sA_b, long sA_h, const float* W, long ldw, long sW_b, long sW_h,
                         int w_is_kn, const float* bias, const float* R, long ldr, float* C, long ldc, long sC_b, long sC_h,
                         int M, int N, int K, int act, float alpha, int batch, int heads, int grp_rows, int grp_stride,
                         hipStream_t stream) {
  if (!A || !W || !C) return VT_ERR_NULL;
  if (M <= 0 || N <= 0 || K <= 0 || batch <= 0 || heads <= 0 || (long)batch * heads > 65535) return VT_ERR_BAD_SHAPE;
  if (act != 0 && act != 1 && act != 2) return VT_ERR_UNSUPPORTED;
  if (grp_rows < 0 || (grp_rows > 0 && grp_stride < grp_rows)) return VT_ERR_BAD_SHAPE;
  GemmF32Args g;
  g.A = A; g.lda = lda; g.sA_b = sA_b; g.sA_h = sA_h; g.W = W; g.ldw = ldw; g.sW_b = sW_b; g.sW_h = sW_h;
  g.bias = bias; g.R = R; g.ldr = ldr; g.C = C; g.ldc = ldc; g.sC_b = sC_b; g.sC_h = sC_h;
  g.M = M; g.N = N; g.K = K; g.act = act; g.w_is_kn = w_is_kn; g.heads = heads; g.grp_rows = grp_rows; g.grp_stride = grp_stride;
  g.alpha = alpha;
  g.a_is_km = 0; g.accumulate = 0; g.split = 1; g.kchunk = (K + GF_BK - 1) / GF_BK * GF_BK; g.ws = nullptr; g.pre = nullptr;
  g.drop = vt_no_drop();
  auto ok4 = [](const void* p, long ld, long s0, long s1) { return (((uintptr_t)p & 15) == 0) && (ld % 4 == 0) && (s0 % 4 == 0) && (s1 % 4 == 0); };
  g.vec_a = ok4(A, lda, sA_b, sA_h) ? 1 : 0;
  g.vec_w = ok4(W, ldw, sW_b, sW_h) ? 1 : 0;
  const dim3 grid((N + GF_BN - 1) / GF_BN, (M + GF_BM - 1) / GF_BM, batch * heads);
  if (grid.y > 65535) return VT_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(gemm_f32_128, grid, dim3(256), 0, stream, g);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// C (+)= sum_s ws[s] in split order (the weight gradients' K split): bitwise the same result for the same shape and split.
__global__ __launch_bounds__(256) void gemm_f32_split_reduce(const float* __restrict__ ws, int split, int M, int N,
                                                             float* __restrict__ C, long ldc, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)M * N) return;
  const long row = i / N, col = i - row * N;
  float s = accumulate ? C[row * ldc + col] : 0.f;
  float t = ws[i];
  for (int k = 1; k < split; ++k) t += ws[(long)k * M * N + i];
  C[row * ldc + col] = s + t;
}

// How many K ranges a product of this shape is split into (a function of the shape only): enough workgroups to cover the
// 256 CUs about twice when the [M, N] tiles alone cannot, each range at least 512 deep, at most 16 ranges.
int vt_gemm_f32_split_for(int M, int N, int K) {
  const long tiles = (long)((M + GF_BM - 1) / GF_BM) * ((N + GF_BN - 1) / GF_BN);
  int s = (int)(512 / tiles);
  s = s < K / 512 ? s : K / 512;
  return s < 1 ? 1 : (s > 16 ? 16 : s);
}

int vt_gemm_f32_ex_dispatch(const float* A, long lda, long sA_b, long sA_h, int a_is_km, const float* W, long ldw, long sW_b,
                            long sW_h, int w_is_kn, const float* bias, const float* R, long ldr, float* C, long ldc, long sC_b,
                            long sC_h, float* pre, int M, int N, int K, int act, float alpha, int batch, int heads,
                            int grp_rows, int grp_stride, int accumulate, int split, float* ws, DropCfg drop,
                            hipStream_t stream) {
  if (!A || !W || !C) return VT_ERR_NULL;
  if (M <= 0 || N <= 0 || K <= 0 || batch <= 0 || heads <= 0) return VT_ERR_BAD_SHAPE;
  if (act != 0 && act != 1 && act != 2) return VT_ERR_UNSUPPORTED;
  if (grp_rows < 0 || (grp_rows > 0 && grp_stride < grp_rows)) return VT_ERR_BAD_SHAPE;
  if (split <= 0) split = vt_gemm_f32_split_for(M, N, K);
  if (split > 1) {
    // partial planes carry alpha * A . op(W) only: the rest of the epilogue has no place in a K split
    if (!ws) return VT_ERR_NULL;
    if (batch * heads != 1 || bias || R || pre || act || grp_rows || drop.thresh) return VT_ERR_UNSUPPORTED;
  }
  if ((long)batch * heads * split > 65535) return VT_ERR_BAD_SHAPE;
  GemmF32Args g;
  g.A = A; g.lda = lda; g.sA_b = sA_b; g.sA_h = sA_h; g.W = W; g.ldw = ldw; g.sW_b = sW_b; g.sW_h = sW_h;
  g.bias = bias; g.R = R; g.ldr = ldr; g.C = C; g.ldc = ldc; g.sC_b = sC_b; g.sC_h = sC_h;
  g.M = M; g.N = N; g.K = K; g.act = act; g.w_is_kn = w_is_kn; g.heads = heads; g.grp_rows = grp_rows; g.grp_stride = grp_stride;
  g.alpha = alpha;
  g.a_is_km = a_is_km ? 1 : 0; g.accumulate = accumulate ? 1 : 0; g.split = split; g.ws = ws; g.pre = pre; g.drop = drop;
  g.kchunk = ((K + split - 1) / split + GF_BK - 1) / GF_BK * GF_BK;
  auto ok4 = [](const void* p, long ld, long s0, long s1) { return (((uintptr_t)p & 15) == 0) && (ld % 4 == 0) && (s0 % 4 == 0) && (s1 % 4 == 0); };
  g.vec_a = ok4(A, lda, sA_b, sA_h) ? 1 : 0;
  g.vec_w = ok4(W, ldw, sW_b, sW_h) ? 1 : 0;
  const dim3 grid((N + GF_BN - 1) / GF_BN, (M + GF_BM - 1) / GF_BM, batch * heads * split);
  if (grid.y > 65535) return VT_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(gemm_f32_128, grid, dim3(256), 0, stream, g);
  if (split > 1) {
    const long n = (long)M * N;
    hipLaunchKernelGGL(gemm_f32_split_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws, split, M, N, C, ldc,
                       g.accumulate);
  }
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------------------------
// In-place row softmax of x [rows, cols] (row pitch ld): x * scale + bias(row, col) -> softmax -> * head_scale.
// Attention use: rows = B * nh * S, row r = ((b * nh + h) * S + q); mask_mode 0: raw mask [B, cols] turned into
// (1 - m) * -10000 (encoder.py:238-241), 1: additive [B, cols], 2: additive per query [B, S, cols]; -1: no mask.
struct SoftmaxArgs {
  float* x; long ld; long rows; int cols;
  float scale;
  const float* mask; int mask_mode;
  const float* head_scale;   // [nh] or null
  int nh, S;                 // row decomposition (nh = S = 1 when there is none)
};

__global__ __launch_bounds__(256) void softmax_rows_f32(SoftmaxArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const long bh = row / a.S;
  const int q = (int)(row - bh * a.S);
  const int b = (int)(bh / a.nh), h = (int)(bh - (long)b * a.nh);
  float* xp = a.x + row * a.ld;
  const float* mp = nullptr;
  if (a.mask_mode == 0 || a.mask_mode == 1) mp = a.mask + (long)b * a.cols;
  else if (a.mask_mode == 2) mp = a.mask + ((long)b * a.S + q) * a.cols;
  float mx = -INFINITY;
  for (int c = lane; c < a.cols; c += 64) {
    float v = xp[c] * a.scale;
    if (mp) v += (a.mask_mode == 0) ? (1.0f - mp[c]) * -10000.0f : mp[c];
    xp[c] = v;
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int c = lane; c < a.cols; c += 64) {
    const float e = expf(xp[c] - mx);
    xp[c] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  const float hs = a.head_scale ? a.head_scale[h] : 1.0f;
  for (int c = lane; c < a.cols; c += 64) xp[c] = (xp[c] / sum) * hs;   // the reference's order: softmax, then * head_mask
}

int vt_softmax_rows_f32_dispatch(float* x, long ld, long rows, int cols, float scale, const float* mask, int mask_mode,
                                 const float* head_scale, int nh, int S, hipStream_t stream) {
  if (!x) return VT_ERR_NULL;
  if (rows <= 0 || cols <= 0 || nh <= 0 || S <= 0 || rows > 4L * 2147483647L) return VT_ERR_BAD_SHAPE;
  if (mask_mode < -1 || mask_mode > 2 || (mask_mode >= 0 && !mask)) return VT_ERR_NULL;
  SoftmaxArgs a;
  a.x = x; a.ld = ld; a.rows = rows; a.cols = cols; a.scale = scale; a.mask = mask; a.mask_mode = mask ? mask_mode : -1;
  a.head_scale = head_scale; a.nh = nh; a.S = S;
  hipLaunchKernelGGL(softmax_rows_f32, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------------------------
// BertLayerNorm, one wave per row: (x - u) / sqrt(var + eps) * w + b, biased variance, two passes over registers.
struct LnF32Args {
  const void* x; long ldx; void* y; long ldy;
  const float* gamma; const float* beta;
  long M; int H; float eps;
  int grp_rows, grp_stride;
  DropCfg drop;   // fp32 output only: dropout after the LayerNorm, element index = row * H + col (row before the remap)
  int x_compact;  // 1: x rows are not remapped (x [M, H] compact, only y rows are); 0: both (in place)
};

template <bool IN_F32, bool OUT_F32>
__global__ __launch_bounds__(256) void layernorm_rows_f32(LnF32Args a) {
  constexpr int MAXC = 16;   // H <= 64 * 4 * 16 = 4096
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.M) return;
  const long prow = a.grp_rows ? (row / a.grp_rows) * a.grp_stride + (row % a.grp_rows) : row;
  float v[MAXC][4];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int col = (lane + 64 * c) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[c][i] = 0.f;
    if (col < a.H) {
      if (IN_F32) {
        const f32x4 t = *(const f32x4*)((const float*)a.x + (a.x_compact ? row : prow) * a.ldx + col);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[c][i] = t[i];
      } else {
        const uint2 t = *(const uint2*)((const bf16_t*)a.x + (a.x_compact ? row : prow) * a.ldx + col);
        v[c][0] = bf16lo(t.x); v[c][1] = bf16hi(t.x); v[c][2] = bf16lo(t.y); v[c][3] = bf16hi(t.y);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) s += v[c][i];
    }
  }
  const float u = wave_sum(s) / (float)a.H;
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int col = (lane + 64 * c) * 4;
    if (col < a.H) {
#pragma unroll
      for (int i = 0; i < 4; ++i) { const float d = v[c][i] - u; ss += d * d; }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)a.H + a.eps);
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int col = (lane + 64 * c) * 4;
    if (col < a.H) {
      const f32x4 g4 = *(const f32x4*)(a.gamma + col), b4 = *(const f32x4*)(a.beta + col);
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (v[c][i] - u) * rstd * g4[i] + b4[i];
      if (OUT_F32 && a.drop.thresh) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = vt_keep(a.drop, (uint32_t)(row * a.H + col + i)) ? o[i] * a.drop.scale : 0.f;
      }
      if (OUT_F32) {
        *(f32x4*)((float*)a.y + prow * a.ldy + col) = (f32x4){o[0], o[1], o[2], o[3]};
      } else {
        uint2 w;
        w.x = pack_bf16x2(o[0], o[1]); w.y = pack_bf16x2(o[2], o[3]);
        *(uint2*)((bf16_t*)a.y + prow * a.ldy + col) = w;
      }
    }
  }
}

int vt_layernorm_f32_dispatch(const void* x, long ldx, int x_is_f32, void* y, long ldy, int y_is_f32, const float* gamma,
                              const float* beta, long M, int H, float eps, int grp_rows, int grp_stride, hipStream_t stream) {
  return vt_layernorm_f32_drop_dispatch(x, ldx, x_is_f32, y, ldy, y_is_f32, gamma, beta, M, H, eps, grp_rows, grp_stride,
                                        vt_no_drop(), stream, 0);
}

// drop_entry (vt_layernorm_drop_f32): x rows compact, y rows remapped; 0 (vt_layernorm_rows): both remapped (in place)
int vt_layernorm_f32_drop_dispatch(const void* x, long ldx, int x_is_f32, void* y, long ldy, int y_is_f32, const float* gamma,
                                   const float* beta, long M, int H, float eps, int grp_rows, int grp_stride, DropCfg drop,
                                   hipStream_t stream, int drop_entry) {
  if (drop.thresh && !y_is_f32) return VT_ERR_UNSUPPORTED;
  if (!x || !y || !gamma || !beta) return VT_ERR_NULL;
  if (M <= 0 || H <= 0 || (H % 4) || H > 4096) return VT_ERR_BAD_SHAPE;
  const int ax = x_is_f32 ? 15 : 7, ay = y_is_f32 ? 15 : 7;
  if ((ldx % 4) || (ldy % 4) || ((uintptr_t)x & ax) || ((uintptr_t)y & ay) || (((uintptr_t)gamma | (uintptr_t)beta) & 15)) return VT_ERR_BAD_ALIGN;
  LnF32Args a;
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.gamma = gamma; a.beta = beta; a.M = M; a.H = H; a.eps = eps;
  a.grp_rows = grp_rows; a.grp_stride = grp_stride; a.drop = drop; a.x_compact = drop_entry;
  const dim3 grid((unsigned)((M + 3) / 4)), block(256);
  if (x_is_f32 && y_is_f32) hipLaunchKernelGGL((layernorm_rows_f32<true, true>), grid, block, 0, stream, a);
  else if (x_is_f32) hipLaunchKernelGGL((layernorm_rows_f32<true, false>), grid, block, 0, stream, a);
  else if (y_is_f32) hipLaunchKernelGGL((layernorm_rows_f32<false, true>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((layernorm_rows_f32<false, false>), grid, block, 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------------------------
// BertEmbeddings in fp32: word + position + token_type -> LayerNorm -> rows b*S + t of y [B*S, H] fp32.
struct EmbF32Args {
  const int64_t* ids; const int64_t* type_ids; const int64_t* pos_ids;
  const float* word; const float* pos; const float* type; const float* gamma; const float* beta;
  float* y; long ldy;
  int B, T, S, H, n_word, n_pos, n_type;
  float eps;
  int* err;
};

__global__ __launch_bounds__(256) void embed_layernorm_f32(EmbF32Args a) {
  constexpr int MAXC = 16;
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
  float v[MAXC][4];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int col = (lane + 64 * c) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[c][i] = 0.f;
    if (col < a.H) {
      const f32x4 w4 = *(const f32x4*)(a.word + wi * a.H + col);
      const f32x4 p4 = *(const f32x4*)(a.pos + pi * a.H + col);
      const f32x4 t4 = *(const f32x4*)(a.type + ti * a.H + col);
#pragma unroll
      for (int i = 0; i < 4; ++i) { v[c][i] = (w4[i] + p4[i]) + t4[i]; s += v[c][i]; }
    }
  }
  const float u = wave_sum(s) / (float)a.H;
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int col = (lane + 64 * c) * 4;
    if (col < a.H) {
#pragma unroll
      for (int i = 0; i < 4; ++i) { const float d = v[c][i] - u; ss += d * d; }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)a.H + a.eps);
  float* yp = a.y + ((long)b * a.S + t) * a.ldy;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int col = (lane + 64 * c) * 4;
    if (col < a.H) {
      const f32x4 g4 = *(const f32x4*)(a.gamma + col), b4 = *(const f32x4*)(a.beta + col);
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (v[c][i] - u) * rstd * g4[i] + b4[i];
      *(f32x4*)(yp + col) = o;
    }
  }
}

int vt_embed_layernorm_f32_dispatch(const int64_t* ids, const int64_t* type_ids, const int64_t* pos_ids, const float* word,
                                    const float* pos, const float* type, const float* gamma, const float* beta, float* y,
                                    long ldy, int B, int T, int S, int H, int n_word, int n_pos, int n_type, float eps,
                                    int* err_flag, hipStream_t stream) {
  if (!ids || !word || !pos || !type || !gamma || !beta || !y) return VT_ERR_NULL;
  if (B <= 0 || T <= 0 || S < T || H <= 0 || (H % 4) || H > 4096) return VT_ERR_BAD_SHAPE;
  if ((ldy % 4) || (((uintptr_t)word | (uintptr_t)pos | (uintptr_t)type | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15))
    return VT_ERR_BAD_ALIGN;
  EmbF32Args a;
  a.ids = ids; a.type_ids = type_ids; a.pos_ids = pos_ids; a.word = word; a.pos = pos; a.type = type; a.gamma = gamma;
  a.beta = beta; a.y = y; a.ldy = ldy; a.B = B; a.T = T; a.S = S; a.H = H; a.n_word = n_word; a.n_pos = n_pos;
  a.n_type = n_type; a.eps = eps; a.err = err_flag;
  hipLaunchKernelGGL(embed_layernorm_f32, dim3((B * T + 3) / 4), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
