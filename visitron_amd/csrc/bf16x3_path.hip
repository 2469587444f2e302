// bf16x3: the fp32 route's matrix products on the bf16 matrix cores (visitron_amd.set_precision(model, "bf16x3")).
//
// gfx950 runs v_mfma_f32_32x32x2_f32 (fp32_path.hip) at 1/16 of the bf16 MFMA rate and has no xf32 form.  This kernel
// takes the SAME fp32 operands from memory and splits each element into two bf16 terms while it stages the tile from
// registers into LDS:
//
//   hi = bf16_rne(x)            lo = bf16_rne(x - hi)           x = hi + lo + r,  |r| <= 2^-16 |x|  (x - hi is exact in fp32)
//
// and forms every product as  lo.hi + hi.lo + hi.hi  -- three v_mfma_f32_32x32x16_bf16 into one fp32 accumulator, smallest
// terms first -- so each operand keeps 16 significant bits instead of 8:  |a.b - (ah.bh + ah.bl + al.bh)| <= 3 * 2^-16 |a||b|
// to first order (the dropped lo.lo term is 2^-16 |a||b| on its own).  Three bf16 MFMAs (3 x 32 cycles per 32x32x16) stand
// for sixteen fp32 MFMA issue slots of the same work: 16/3 = 5.3x is the ceiling on product time.
//
//   gemm_bf16x3_128     C = act(alpha * A . op(W) + bias) (+ R)     the inference forms of gemm_f32_128: A fp32 [M, K], W fp32
//                       [N, K] or [K, N] (w_is_kn), optional bias / residual / output-row remap, (batch, head) element
//                       strides on all three operands, C fp32; any M, N, K (tails zero-filled); bases / strides that are
//                       not 16-byte aligned take scalar loads.  No training forms (fp32_train.hip keeps gemm_f32_128).
//
// 128x128 tile, 256 threads, 2x2 tiles of 32x32 per wave, BK = 32, double-buffered LDS.  LDS holds a hi plane and a lo plane
// per operand ([128 rows][32 k] bf16, k contiguous: a lane's MFMA fragment is one 16-byte read); the two planes together are
// the bytes of the fp32 tile.  The [K, N]-given operand (V in probs . v) is transposed by its LDS store.  Nothing is cached
// between calls: no pre-split weights, no workspace, no atomics.
//
// Non-finite operands: an inf or NaN element may make the output elements it reaches non-finite (inf splits into hi = inf,
// lo = inf - inf = NaN, so an output that fp32 would leave at inf can come out NaN).  Finite operands inside bf16's range
// (|x| <= 3.3895e38) never produce a non-finite result on their own: hi is finite, x - hi is exact, and |lo| <= 2^-8 |hi|.
#include "dispatch.hpp"

struct GemmX3Args {
  const float* A; long lda; long sA_b, sA_h;
  const float* W; long ldw; long sW_b, sW_h;
  const float* bias; const float* R; long ldr;
  float* C; long ldc; long sC_b, sC_h;
  int M, N, K;
  int act;          // VT_ACT_NONE / VT_ACT_GELU / VT_ACT_TANH
  int w_is_kn;      // 0: W is [N, K]; 1: W is [K, N]
  int heads;        // blockIdx.z = b * heads + h
  int grp_rows, grp_stride;   // output row remap as in gemm_f32_128 (0: identity)
  int vec_a, vec_w; // 16-byte loads allowed (aligned base and strides)
  float alpha;
};

#define GX_BM 128
#define GX_BN 128
#define GX_BK 32
#define GX_PLANE (128 * GX_BK)   // bf16 elements of one plane

// element (row, k) of a plane: 64-byte rows; the 16-byte chunk k / 8 of row r sits at chunk (k / 8) ^ ((r / 4) % 4), so the
// sixteen rows a fragment read covers per lane group fall on sixteen different 16-byte slots of the 256-byte bank row
__device__ __forceinline__ int gx_off(int row, int k) { return row * GX_BK + ((((k >> 3) ^ (row >> 2)) & 3) << 3) + (k & 7); }

// (x0, x1) -> one dword of hi and one of lo (v_cvt_pk_bf16_f32, round to nearest even, twice)
__device__ __forceinline__ void gx_split2(float x0, float x1, uint32_t& hi, uint32_t& lo) {
  hi = pack_bf16x2(x0, x1);
  lo = pack_bf16x2(x0 - bf16lo(hi), x1 - bf16hi(hi));
}

__device__ __forceinline__ float gx_act(float v, int act) {
  if (act == 1) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));   // erf-GELU, as gemm_f32_128
  if (act == 2) return tanhf(v);
  return v;
}

__global__ __launch_bounds__(256) void gemm_bf16x3_128(GemmX3Args g) {
  // [buffer][operand: A, W][plane: hi, lo]
  __shared__ __attribute__((aligned(16))) bf16_t lds[2][2][2][GX_PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * GX_BM, n0 = blockIdx.x * GX_BN;
  const int zb = blockIdx.z / g.heads, zh = blockIdx.z - zb * g.heads;
  const float* A = g.A + zb * g.sA_b + zh * g.sA_h;
  const float* W = g.W + zb * g.sW_b + zh * g.sW_h;
  float* C = g.C + zb * g.sC_b + zh * g.sC_h;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

  // global -> registers.  A [rows, K]-given operand: a thread owns four (row, k-quad) pieces, row = tid/8 + 32 p,
  // k = (tid%8) * 4.  The [K, N]-given operand: two (k-pair, n-quad) pieces, k = 2 (tid/32 + 8 p) and k + 1 in r[2p], r[2p+1],
  // n = (tid%32) * 4 -- a k pair is one dword of a transposed plane.
  float ra[4][4], rb[4][4];
  auto load_rowmajor = [&](const float* base, long ld, int row0, int nrows, int k0, bool vec, float (&r)[4][4]) {
    const int k = k0 + (tid & 7) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row = row0 + (tid >> 3) + 32 * p;
      if (row < nrows && vec && k + 3 < g.K) {
        const f32x4 v = *(const f32x4*)(base + (long)row * ld + k);
        r[p][0] = v[0]; r[p][1] = v[1]; r[p][2] = v[2]; r[p][3] = v[3];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) r[p][i] = (row < nrows && k + i < g.K) ? base[(long)row * ld + k + i] : 0.f;
      }
    }
  };
  auto load_kn = [&](int k0, float (&r)[4][4]) {
    const int n = n0 + (tid & 31) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int k = k0 + 2 * ((tid >> 5) + 8 * (p >> 1)) + (p & 1);
      if (k < g.K && g.vec_w && n + 3 < g.N) {
        const f32x4 v = *(const f32x4*)(W + (long)k * g.ldw + n);
        r[p][0] = v[0]; r[p][1] = v[1]; r[p][2] = v[2]; r[p][3] = v[3];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) r[p][i] = (k < g.K && n + i < g.N) ? W[(long)k * g.ldw + n + i] : 0.f;
      }
    }
  };
  auto load_tiles = [&](int k0) {
    load_rowmajor(A, g.lda, m0, g.M, k0, g.vec_a != 0, ra);
    if (g.w_is_kn) load_kn(k0, rb); else load_rowmajor(W, g.ldw, n0, g.N, k0, g.vec_w != 0, rb);
  };
  // registers -> split -> LDS
  auto store_rowmajor = [&](bf16_t* hi, bf16_t* lo, const float (&r)[4][4]) {
    const int k = (tid & 7) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int off = gx_off((tid >> 3) + 32 * p, k);
      uint32_t h0, l0, h1, l1;
      gx_split2(r[p][0], r[p][1], h0, l0);
      gx_split2(r[p][2], r[p][3], h1, l1);
      *(u32x2*)(hi + off) = (u32x2){h0, h1};
      *(u32x2*)(lo + off) = (u32x2){l0, l1};
    }
  };
  auto store_kn = [&](bf16_t* hi, bf16_t* lo, const float (&r)[4][4]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int k = 2 * ((tid >> 5) + 8 * p);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int off = gx_off((tid & 31) * 4 + i, k);
        uint32_t h, l;
        gx_split2(r[2 * p][i], r[2 * p + 1][i], h, l);
        *(uint32_t*)(hi + off) = h;
        *(uint32_t*)(lo + off) = l;
      }
    }
  };
  auto store_tiles = [&](int buf) {
    store_rowmajor(lds[buf][0][0], lds[buf][0][1], ra);
    if (g.w_is_kn) store_kn(lds[buf][1][0], lds[buf][1][1], rb); else store_rowmajor(lds[buf][1][0], lds[buf][1][1], rb);
  };

  const int nk = (g.K + GX_BK - 1) / GX_BK;
  load_tiles(0);
  store_tiles(0);
  __syncthreads();
  // fragment of lane l for k-step s: row l%32 of its 32-row tile, k = 16 s + 8 (l/32) .. + 7 (cdna MFMA bf16 operand map)
  const int fr = lane & 31, fk = lane >> 5;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load_tiles((kt + 1) * GX_BK);
#pragma unroll
    for (int s = 0; s < GX_BK / 16; ++s) {
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int oa = gx_off(wm * 64 + 32 * i + fr, 16 * s + 8 * fk);
        const int ob = gx_off(wn * 64 + 32 * i + fr, 16 * s + 8 * fk);
        ah[i] = *(const bf16x8*)(lds[buf][0][0] + oa);
        al[i] = *(const bf16x8*)(lds[buf][0][1] + oa);
        bh[i] = *(const bf16x8*)(lds[buf][1][0] + ob);
        bl[i] = *(const bf16x8*)(lds[buf][1][1] + ob);
      }
      // smallest terms first; four independent accumulators between two MFMAs on the same one
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tiles(buf ^ 1);   // the other buffer: its last readers passed the barrier below one step ago
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
        const long orow = g.grp_rows ? (long)(row / g.grp_rows) * g.grp_stride + (row % g.grp_rows) : (long)row;
        float x = gx_act(acc[i][j][v] * g.alpha + bv, g.act);
        if (g.R) x += g.R[(long)row * g.ldr + col];
        C[orow * g.ldc + col] = x;
      }
    }
}

int vt_gemm_bf16x3_dispatch(const float* A, long lda, long sA_b, long sA_h, const float* W, long ldw, long sW_b, long sW_h,
                            int w_is_kn, const float* bias, const float* R, long ldr, float* C, long ldc, long sC_b, long sC_h,
                            int M, int N, int K, int act, float alpha, int batch, int heads, int grp_rows, int grp_stride,
                            hipStream_t stream) {
  if (!A || !W || !C) return VT_ERR_NULL;
  if (M <= 0 || N <= 0 || K <= 0 || batch <= 0 || heads <= 0 || (long)batch * heads > 65535) return VT_ERR_BAD_SHAPE;
  if (act != 0 && act != 1 && act != 2) return VT_ERR_UNSUPPORTED;
  if (grp_rows < 0 || (grp_rows > 0 && grp_stride < grp_rows)) return VT_ERR_BAD_SHAPE;
  GemmX3Args g;
  g.A = A; g.lda = lda; g.sA_b = sA_b; g.sA_h = sA_h; g.W = W; g.ldw = ldw; g.sW_b = sW_b; g.sW_h = sW_h;
  g.bias = bias; g.R = R; g.ldr = ldr; g.C = C; g.ldc = ldc; g.sC_b = sC_b; g.sC_h = sC_h;
  g.M = M; g.N = N; g.K = K; g.act = act; g.w_is_kn = w_is_kn ? 1 : 0; g.heads = heads; g.grp_rows = grp_rows;
  g.grp_stride = grp_stride; g.alpha = alpha;
  auto ok4 = [](const void* p, long ld, long s0, long s1) { return (((uintptr_t)p & 15) == 0) && (ld % 4 == 0) && (s0 % 4 == 0) && (s1 % 4 == 0); };
  g.vec_a = ok4(A, lda, sA_b, sA_h) ? 1 : 0;
  g.vec_w = ok4(W, ldw, sW_b, sW_h) ? 1 : 0;
  const dim3 grid((N + GX_BN - 1) / GX_BN, (M + GX_BM - 1) / GX_BM, batch * heads);
  if (grid.y > 65535) return VT_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(gemm_bf16x3_128, grid, dim3(256), 0, stream, g);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
