// The glue between the big kernels: HBM-bound element and row kernels, 16-byte vector accesses where the layout allows.
//   pack_concat_bf16                            [src0 | src1 | 0-pad] fp32 -> one bf16 K-concatenated GEMM operand
//   dgelu_mul_bf16                              g * gelu'(saved): backward through the MLM-head transform's GELU
//   scale_heads_bf16                            head_mask on a context tensor and on its gradient
//   cast_scale_f32_bf16                         the bf16 communication copy of a gradient-slab range
//   transpose_bf16, transpose_batch_bf16        the transposed weight copies the dgrad GEMMs read
//   apply_dropout_bf16, dropout_mask_dump       a site's dropout mask applied in place / written out for the tests
//   embed_table_grad_runs, embed_table_grad_join  table gradients of an embedding lookup without atomics
//   center_mask_rows                            the per-key attention mask as the attention kernels take it
//   batch_row_counts, batch_row_lists, batch_seq_starts  a training batch's supervised and kept rows, on the device
// LayerNorm lives in layernorm.hip, the loss heads in loss_heads.hip, the optimizers in optim.hip.
#include "dispatch.hpp"

// ---------------------------------------------------------------------------------------------
// out[row, :] = bf16([src0[row, 0:d0] | src1[row, 0:d1] | zeros up to kpad]); 8 columns per thread.  A group that lies
// inside one source reads it as four float2 (d0 = 2054: the rows of the region features are 8-byte, not 16-byte, aligned);
// only the group that straddles the seam (and any source with an odd width) takes the element-wise path.
template <bool PAIRS>
__global__ __launch_bounds__(256) void pack_concat_bf16(const float* __restrict__ s0, int d0, const float* __restrict__ s1,
                                                        int d1, bf16_t* __restrict__ out, int kpad, long rows) {
  const int cpr = kpad >> 3;  // 8-column groups per row
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= rows * cpr) return;
  const long row = gid / cpr;
  const int col = (int)(gid - row * cpr) * 8;
  float v[8];
  const float* src = nullptr;
  if (PAIRS) {
    if (col + 8 <= d0) src = s0 + row * d0 + col;
    else if (col >= d0 && col + 8 <= d0 + d1) src = s1 + row * d1 + (col - d0);
  }
  if (src) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float2 t = *(const float2*)(src + 2 * i);
      v[2 * i] = t.x;
      v[2 * i + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = col + i;
      float x = 0.f;
      if (c < d0) x = s0[row * d0 + c];
      else if (c < d0 + d1) x = s1[row * d1 + (c - d0)];
      v[i] = x;
    }
  }
  u32x4 w;
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
  *(u32x4*)(out + row * kpad + col) = w;
}

int vt_pack_concat_dispatch(const float* s0, int d0, const float* s1, int d1, void* out, int kpad, long rows,
                            hipStream_t stream) {
  if (!s0 || !out || (d1 > 0 && !s1)) return VT_ERR_NULL;
  if (rows <= 0 || d0 <= 0 || d1 < 0 || kpad < d0 + d1 || (kpad % 8)) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)out) & 15) return VT_ERR_BAD_ALIGN;
  const long n = rows * (kpad >> 3);
  // float2 reads need even widths (every row and the seam then start on 8 bytes) and 8-byte aligned bases
  const bool pairs = !(d0 & 1) && !(d1 & 1) && !(((uintptr_t)s0 | (uintptr_t)s1) & 7);
  if (pairs) hipLaunchKernelGGL(pack_concat_bf16<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, s0, d0, s1, d1,
                                (bf16_t*)out, kpad, rows);
  else hipLaunchKernelGGL(pack_concat_bf16<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, s0, d0, s1, d1,
                          (bf16_t*)out, kpad, rows);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// out = g * d elementwise (bf16, 8 per thread), d = saved gelu'(pre-activation): backward through the
// MLM-head transform's GELU.
__global__ __launch_bounds__(256) void dgelu_mul_bf16(const bf16_t* __restrict__ g, const bf16_t* __restrict__ h,
                                                      bf16_t* __restrict__ out, long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const u32x4 gv = ((const u32x4*)g)[i], hv = ((const u32x4*)h)[i];
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    o[k] = pack_bf16x2(bf16lo(gv[k]) * bf16lo(hv[k]), bf16hi(gv[k]) * bf16hi(hv[k]));
  ((u32x4*)out)[i] = o;
}

int vt_dgelu_mul_dispatch(const void* g, const void* h, void* out, long n, hipStream_t stream) {
  if (!g || !h || !out) return VT_ERR_NULL;
  if (n <= 0 || (n % 8)) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)g | (uintptr_t)h | (uintptr_t)out) & 15) return VT_ERR_BAD_ALIGN;
  const long n8 = n / 8;
  hipLaunchKernelGGL(dgelu_mul_bf16, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)g,
                     (const bf16_t*)h, (bf16_t*)out, n8);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// out[r, 64 h + d] = x[r, 64 h + d] * scale[h]: head_mask applied to a context tensor (oscar/modeling_bert.py:65-66 scales
// the probabilities of head h, i.e. that head's 64 context columns) -- the training path's forward copy and its
// gradient's way back.  One thread = 8 columns.
__global__ __launch_bounds__(256) void scale_heads_bf16(const bf16_t* __restrict__ x, long ldx, bf16_t* __restrict__ out, long ldo,
                                                        long rows, int nh, const float* __restrict__ scale) {
  const int cpr = nh * 8;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cpr) return;
  const long row = i / cpr;
  const int c = (int)(i - row * cpr);
  const float sc = scale[c >> 3];
  const u32x4 v = *(const u32x4*)(x + row * ldx + c * 8);
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = pack_bf16x2(bf16lo(v[k]) * sc, bf16hi(v[k]) * sc);
  *(u32x4*)(out + row * ldo + c * 8) = o;
}

int vt_scale_heads_dispatch(const void* x, long ldx, void* out, long ldo, long rows, int nh, const float* scale, hipStream_t stream) {
  if (!x || !out || !scale) return VT_ERR_NULL;
  if (rows <= 0 || nh <= 0) return VT_ERR_BAD_SHAPE;
  if ((ldx % 8) || (ldo % 8) || (((uintptr_t)x | (uintptr_t)out) & 15)) return VT_ERR_BAD_ALIGN;
  const long n = rows * nh * 8;
  hipLaunchKernelGGL(scale_heads_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)x, ldx,
                     (bf16_t*)out, ldo, rows, nh, scale);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// y = bf16(x * scale), flat: the communication copy of a gradient-slab range (half the all-reduce bytes)
__global__ __launch_bounds__(256) void cast_scale_f32_bf16(const float* __restrict__ x, bf16_t* __restrict__ y, long n8, float scale) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const f32x4 a = ((const f32x4*)x)[2 * i], b = ((const f32x4*)x)[2 * i + 1];
    u32x4 o;
    o[0] = pack_bf16x2(a[0] * scale, a[1] * scale); o[1] = pack_bf16x2(a[2] * scale, a[3] * scale);
    o[2] = pack_bf16x2(b[0] * scale, b[1] * scale); o[3] = pack_bf16x2(b[2] * scale, b[3] * scale);
    ((u32x4*)y)[i] = o;
  }
}

int vt_cast_scale_dispatch(const float* x, void* y, long n, float scale, hipStream_t stream) {
  if (!x || !y) return VT_ERR_NULL;
  if (n <= 0 || (n % 8)) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)x & 15) || ((uintptr_t)y & 15)) return VT_ERR_BAD_ALIGN;
  const long n8 = n / 8;
  long blocks = (n8 + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(cast_scale_f32_bf16, dim3((unsigned)blocks), dim3(256), 0, stream, x, (bf16_t*)y, n8, scale);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// out[c][r] = in[r][c], bf16, 64x64 tiles through LDS (both sides 16-byte coalesced).  Refreshes the
// transposed weight copies the dgrad GEMMs read after every optimizer step.
__global__ __launch_bounds__(256) void transpose_bf16(const bf16_t* __restrict__ in, long ldi, bf16_t* __restrict__ out,
                                                      long ldo, int R, int C) {
  __shared__ bf16_t tile[64][72];  // [c][r], pitch 72 elements = 144 B keeps 16-B row reads aligned
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int t = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int chunk = t + 256 * it;          // 512 chunks of 8 elements
    const int r = chunk >> 3, cc = (chunk & 7) * 8;
    u32x4 v = (u32x4){0u, 0u, 0u, 0u};
    if (r0 + r < R && c0 + cc < C) v = *(const u32x4*)(in + (long)(r0 + r) * ldi + c0 + cc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      tile[cc + 2 * i][r] = (bf16_t)(v[i] & 0xffffu);
      tile[cc + 2 * i + 1][r] = (bf16_t)(v[i] >> 16);
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int chunk = t + 256 * it;
    const int c = chunk >> 3, rr = (chunk & 7) * 8;
    if (c0 + c < C && r0 + rr < R) *(u32x4*)(out + (long)(c0 + c) * ldo + r0 + rr) = *(const u32x4*)(&tile[c][rr]);
  }
}

int vt_transpose_dispatch(const void* in, long ldi, void* out, long ldo, int R, int C, hipStream_t stream) {
  if (!in || !out) return VT_ERR_NULL;
  if (R <= 0 || C <= 0 || (R % 8) || (C % 8)) return VT_ERR_BAD_SHAPE;
  if ((ldi % 8) || (ldo % 8) || (((uintptr_t)in | (uintptr_t)out) & 15)) return VT_ERR_BAD_ALIGN;
  hipLaunchKernelGGL(transpose_bf16, dim3((C + 63) / 64, (R + 63) / 64), dim3(256), 0, stream, (const bf16_t*)in, ldi,
                     (bf16_t*)out, ldo, R, C);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// The same for a batch of matrices in ONE launch (blockIdx.z = matrix): after an optimizer step the 48 layer weights
// are re-transposed, and 48 five-microsecond launches cost more in gaps than in work.
struct TransposeBatch {
  const bf16_t* in[64];
  bf16_t* out[64];
  int ldi[64], ldo[64], R[64], C[64];
  int blk_begin[65];   // first workgroup of each matrix in the 1-D grid (64x64-element tiles, column-tile fastest)
};
__global__ __launch_bounds__(256) void transpose_batch_bf16(TransposeBatch b, int n) {
  __shared__ bf16_t tile[64][72];
  int z = 0;
  for (int i = 1; i < n; ++i)   // wave-uniform scan
    if ((int)blockIdx.x >= b.blk_begin[i]) z = i;
  const int R = b.R[z], C = b.C[z];
  const int local = blockIdx.x - b.blk_begin[z];
  const int bx = (C + 63) >> 6;
  const int r0 = (local / bx) * 64, c0 = (local % bx) * 64;
  const bf16_t* __restrict__ in = b.in[z];
  bf16_t* __restrict__ out = b.out[z];
  const long ldi = b.ldi[z], ldo = b.ldo[z];
  const int t = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int chunk = t + 256 * it;
    const int r = chunk >> 3, cc = (chunk & 7) * 8;
    u32x4 v = (u32x4){0u, 0u, 0u, 0u};
    if (r0 + r < R && c0 + cc < C) v = *(const u32x4*)(in + (long)(r0 + r) * ldi + c0 + cc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      tile[cc + 2 * i][r] = (bf16_t)(v[i] & 0xffffu);
      tile[cc + 2 * i + 1][r] = (bf16_t)(v[i] >> 16);
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int chunk = t + 256 * it;
    const int c = chunk >> 3, rr = (chunk & 7) * 8;
    if (c0 + c < C && r0 + rr < R) *(u32x4*)(out + (long)(c0 + c) * ldo + r0 + rr) = *(const u32x4*)(&tile[c][rr]);
  }
}

int vt_transpose_batch_dispatch(const void* const* in, const long* ldi, void* const* out, const long* ldo, const int* R,
                                const int* C, int n, hipStream_t stream) {
  if (!in || !out || !ldi || !ldo || !R || !C) return VT_ERR_NULL;
  if (n <= 0) return VT_ERR_BAD_SHAPE;
  for (int base = 0; base < n; base += 64) {
    const int cnt = n - base < 64 ? n - base : 64;
    TransposeBatch b;
    int blocks = 0;
    for (int i = 0; i < 64; ++i) {
      const int j = base + (i < cnt ? i : 0);
      if (!in[j] || !out[j]) return VT_ERR_NULL;
      // a row count that is not a multiple of 8 is served when the output rows have room for the rounded-up count
      // (the tail of the last 8-element group is written as zeros: padding columns of the transposed copy)
      if (R[j] <= 0 || C[j] <= 0 || (C[j] % 8) || ldo[j] < ((R[j] + 7) & ~7)) return VT_ERR_BAD_SHAPE;
      if ((ldi[j] % 8) || (ldo[j] % 8) || (((uintptr_t)in[j] | (uintptr_t)out[j]) & 15)) return VT_ERR_BAD_ALIGN;
      b.in[i] = (const bf16_t*)in[j]; b.out[i] = (bf16_t*)out[j]; b.ldi[i] = (int)ldi[j]; b.ldo[i] = (int)ldo[j];
      b.R[i] = R[j]; b.C[i] = C[j];
      b.blk_begin[i] = blocks;
      if (i < cnt) blocks += ((R[j] + 63) / 64) * ((C[j] + 63) / 64);
    }
    b.blk_begin[64] = blocks;
    hipLaunchKernelGGL(transpose_batch_bf16, dim3(blocks), dim3(256), 0, stream, b, cnt);
    if (hipGetLastError() != hipSuccess) return VT_ERR_HIP;
  }
  return VT_OK;
}

// x *= dropout mask * scale in place (bf16 [rows, cols], element index = row * cols + col): masks the
// compacted image-row gradient with the mask the region-projection epilogue used.
__global__ __launch_bounds__(256) void apply_dropout_bf16(bf16_t* __restrict__ x, long ld, long rows, int cols, DropCfg d) {
  const int cpr = cols >> 3;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cpr) return;
  const long row = i / cpr;
  const int col = (int)(i - row * cpr) * 8;
  u32x4 w = *(u32x4*)(x + row * ld + col);
  const uint32_t e0 = (uint32_t)row * (uint32_t)cols + (uint32_t)col;
  float v[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[2 * k] = bf16lo(w[k]); v[2 * k + 1] = bf16hi(w[k]); }
  vt_drop_run<8>(d, e0, v);
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = pack_bf16x2(v[2 * k], v[2 * k + 1]);
  *(u32x4*)(x + row * ld + col) = w;
}

int vt_apply_dropout_dispatch(void* x, long ld, long rows, int cols, const DropCfg& d, hipStream_t stream) {
  if (!x) return VT_ERR_NULL;
  if (rows <= 0 || cols <= 0 || (cols % 8) || (ld % 8) || rows * cols >= (1L << 32)) return VT_ERR_BAD_SHAPE;
  if (!d.thresh) return VT_OK;
  const long n = rows * (cols >> 3);
  hipLaunchKernelGGL(apply_dropout_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (bf16_t*)x, ld, rows, cols, d);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// out[i] = 1 if element i of the site is kept (tests: lets the CPU oracle run with the SAME masks)
// ATTN: the attention sites' function (a hash word per four keys, 8-bit thresholds: vt_keep_attn)
template <bool ATTN>
__global__ __launch_bounds__(256) void dropout_mask_dump(uint8_t* __restrict__ out, long n, DropCfg d) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (ATTN ? vt_keep_attn(d, (uint32_t)i) : vt_keep(d, (uint32_t)i)) ? 1 : 0;
}

int vt_dropout_mask_dispatch(uint8_t* out, long n, const DropCfg& d, hipStream_t stream, int attn) {
  if (!out) return VT_ERR_NULL;
  if (n <= 0 || n >= (1L << 32)) return VT_ERR_BAD_SHAPE;
  if (attn) hipLaunchKernelGGL(dropout_mask_dump<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, out, n, d);
  else hipLaunchKernelGGL(dropout_mask_dump<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, out, n, d);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---- table gradients of an embedding lookup without atomics ------------------------------------------------------
// grad[id[i], :] += sum of de[perm[j], :] over the rows j whose id equals id[i], for the sorted id list `sorted_ids`
// (perm = the stable sort's permutation): the scatter-add of BertEmbeddings' backward (torch: index_add_ = 25 M float
// atomics for the word table at B = 256, 179 us, and an order of additions that changes from run to run).  No atomics
// here: a table row is written by one wave, the rows of a run added in their original order (bitwise reproducible); the
// padding index `skip_id`, whose row torch.nn.Embedding leaves without gradient, is passed over.  Most runs are short (a
// token id seldom repeats in a batch), [CLS] repeats B times, and [MASK] may repeat thousands of times: hence the segments.
#define ETG_SEG 32   // rows one wave adds at most: a run of equal ids is cut at the multiples of ETG_SEG of the sorted order

// the rows [i, e) of the sorted order (one id), added in their original order into acc[3] (columns c0 + 256 k + 4 lane):
// 64 permutation entries per vector load, four rows in flight at a time
__device__ __forceinline__ void etg_sum_rows(const long* __restrict__ perm, const float* __restrict__ de, long ld_de, long i, long len,
                                             int c0, int H, int lane, f32x4 (&acc)[3]) {
  for (long j0 = 0; j0 < len; j0 += 64) {
    const long left = len - j0 < 64 ? len - j0 : 64;
    const long pv = lane < left ? perm[i + j0 + lane] : 0;
    for (int j = 0; j < (int)left; j += 4) {
      f32x4 v[4][3];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = j + r < (int)left;
        const long pr = ((long)__builtin_amdgcn_readlane((int)(pv >> 32), on ? j + r : 0) << 32) |
                        (unsigned)__builtin_amdgcn_readlane((int)pv, on ? j + r : 0);
        const float* row = de + pr * ld_de;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int c = c0 + 256 * k + 4 * lane;
          v[r][k] = (on && c < H) ? *(const f32x4*)(row + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[k][e] += v[r][k][e];
    }
  }
}

// Pass 1, one WAVE per sorted position (four per workgroup).  A position works if it starts a SEGMENT: a run of equal ids, cut
// at every multiple of ETG_SEG of the sorted order (so that a token repeated thousands of times in a batch -- [MASK] -- is
// added by many waves, not by one).  A run that is one segment is added straight into its table row (plain loads and
// stores: the wave owns the row); the segments of a longer run park their sums in `scratch` (row = the segment's first
// sorted position) for pass 2.
__global__ __launch_bounds__(256) void embed_table_grad_runs(const int* __restrict__ sorted_ids, const long* __restrict__ perm,
                                                             const float* __restrict__ de, long ld_de, float* __restrict__ grad,
                                                             long ld_grad, long n, int H, long n_rows_table, long skip_id,
                                                             float* __restrict__ scratch, int* __restrict__ any_long) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const long id = sorted_ids[i];
  if (id == skip_id || id < 0 || id >= n_rows_table) return;          // uniform per wave
  const bool run_head = i == 0 || sorted_ids[i - 1] != id;
  if (!run_head && (i % ETG_SEG) != 0) return;                        // not the first row of a segment
  const long bound = (i / ETG_SEG + 1) * ETG_SEG < n ? (i / ETG_SEG + 1) * ETG_SEG : n;
  long e = i + 1;
  while (e < bound && sorted_ids[e] == id) ++e;                       // (uniform scalar loop, <= ETG_SEG steps)
  const bool run_ends = e == n || sorted_ids[e] != id;
  const bool whole_run = run_head && run_ends;
  if (!whole_run && lane == 0) *any_long = 1;
  float* dst = whole_run ? grad + id * ld_grad : scratch + i * (long)H;
  for (int c0 = 0; c0 < H; c0 += 768) {
    f32x4 acc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int c = c0 + 256 * k + 4 * lane;
      acc[k] = (whole_run && c < H) ? *(const f32x4*)(dst + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    etg_sum_rows(perm, de, ld_de, i, e - i, c0, H, lane, acc);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int c = c0 + 256 * k + 4 * lane;
      if (c < H) *(f32x4*)(dst + c) = acc[k];
    }
  }
}

// Pass 2 (does nothing unless pass 1 met a run of several segments): the head of such a run adds its segments' sums, in
// the order of the segments, into the table row.
__global__ __launch_bounds__(256) void embed_table_grad_join(const int* __restrict__ sorted_ids, float* __restrict__ grad, long ld_grad,
                                                             long n, int H, long n_rows_table, long skip_id,
                                                             const float* __restrict__ scratch, const int* __restrict__ any_long) {
  if (*any_long == 0) return;
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const long id = sorted_ids[i];
  if (id == skip_id || id < 0 || id >= n_rows_table) return;
  if (i > 0 && sorted_ids[i - 1] == id) return;                       // not a run head
  const long b1 = (i / ETG_SEG + 1) * ETG_SEG;                        // the run's second segment would start here
  if (b1 >= n || sorted_ids[b1] != id) return;                        // one segment: pass 1 added it straight into the table
  float* gr = grad + id * ld_grad;
  for (int c0 = 0; c0 < H; c0 += 768) {
    f32x4 acc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int c = c0 + 256 * k + 4 * lane;
      acc[k] = c < H ? *(const f32x4*)(gr + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // the first segment starts at i, the others at the multiples of ETG_SEG after it; four sums in flight at a time
    long sgm = i;
    while (sgm < n && sorted_ids[sgm] == id) {
      f32x4 v[4][3];
      bool on[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        on[r] = sgm < n && sorted_ids[sgm] == id;
        const float* src = scratch + (on[r] ? sgm : i) * (long)H;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int c = c0 + 256 * k + 4 * lane;
          v[r][k] = (on[r] && c < H) ? *(const f32x4*)(src + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        if (on[r]) sgm = (sgm / ETG_SEG + 1) * ETG_SEG;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (on[r])
#pragma unroll
          for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[k][e] += v[r][k][e];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int c = c0 + 256 * k + 4 * lane;
      if (c < H) *(f32x4*)(gr + c) = acc[k];
    }
  }
}

int vt_embed_table_grad_dispatch(const int* sorted_ids, const long* perm, const float* de, long ld_de, float* grad, long ld_grad,
                                 long n, int H, long n_rows_table, long skip_id, float* scratch, int* flag, hipStream_t stream) {
  if (!sorted_ids || !perm || !de || !grad || !scratch || !flag) return VT_ERR_NULL;
  if (n <= 0 || H <= 0 || (H & 3) || n_rows_table <= 0 || n > 0x7fffffffL) return VT_ERR_BAD_SHAPE;
  if ((ld_de & 3) || (ld_grad & 3) || (((uintptr_t)de | (uintptr_t)grad | (uintptr_t)scratch) & 15)) return VT_ERR_BAD_ALIGN;
  if (hipMemsetAsync(flag, 0, sizeof(int), stream) != hipSuccess) return VT_ERR_HIP;
  const unsigned nwg = (unsigned)((n + 3) / 4);
  hipLaunchKernelGGL(embed_table_grad_runs, dim3(nwg), dim3(256), 0, stream, sorted_ids, perm, de, ld_de, grad, ld_grad, n, H,
                     n_rows_table, skip_id, scratch, flag);
  hipLaunchKernelGGL(embed_table_grad_join, dim3(nwg), dim3(256), 0, stream, sorted_ids, grad, ld_grad, n, H, n_rows_table, skip_id,
                     scratch, flag);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---- the per-key attention mask as the kernels take it ---------------------------------------------------------------
// out[b, :] = float(mask[b, :]) - max_s float(mask[b, s]) + 1 (modeling._centered_mask: one constant per sequence off the
// additive bias (1 - m) * -10000 of encoder.py:238-241, a bitwise no-op for a 0/1 mask with a kept key), from the dtypes
// callers pass (float32, int64, int32, one-byte bool / uint8): one launch where torch took a cast, amax, sub and add.
template <typename T>
__global__ __launch_bounds__(256) void center_mask_rows(const T* __restrict__ m, long ldm, float* __restrict__ out, int S) {
  __shared__ float red[4];
  const T* row = m + (long)blockIdx.x * ldm;
  float mx = -INFINITY;
  for (int s = threadIdx.x; s < S; s += 256) mx = fmaxf(mx, (float)row[s]);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  for (int s = threadIdx.x; s < S; s += 256) out[(long)blockIdx.x * S + s] = ((float)row[s] - mx) + 1.0f;
}

// kind: 0 float32, 1 int64, 2 int32, 3 one byte (bool / uint8)
int vt_center_mask_dispatch(const void* mask, int kind, long ldm, float* out, int B, int S, hipStream_t stream) {
  if (!mask || !out) return VT_ERR_NULL;
  if (B <= 0 || S <= 0 || ldm < S) return VT_ERR_BAD_SHAPE;
  switch (kind) {
    case 0: hipLaunchKernelGGL(center_mask_rows<float>, dim3(B), dim3(256), 0, stream, (const float*)mask, ldm, out, S); break;
    case 1: hipLaunchKernelGGL(center_mask_rows<long>, dim3(B), dim3(256), 0, stream, (const long*)mask, ldm, out, S); break;
    case 2: hipLaunchKernelGGL(center_mask_rows<int>, dim3(B), dim3(256), 0, stream, (const int*)mask, ldm, out, S); break;
    case 3: hipLaunchKernelGGL(center_mask_rows<unsigned char>, dim3(B), dim3(256), 0, stream, (const unsigned char*)mask, ldm, out, S); break;
    default: return VT_ERR_UNSUPPORTED;
  }
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---- what the host must know about a training batch, and its row lists -------------------------------------------
// The pretrain step runs its heads on the supervised rows only (labels != -1, token_labels != -1: encoder.py:377-385,
// CrossEntropyLoss(ignore_index=-1)) and its encoder on the rows with a non-zero attention mask only; the host needs the
// three counts to size those launches.  batch_row_counts reduces them -- with the verdict on the compacted layout (a 0/1
// mask, every [CLS] and every supervised position kept) and the embedding kernel's out-of-range flag -- into five words the
// host reads back in one synchronisation; batch_row_lists then writes the row lists (ascending), the padded -> compact
// map and the per-sequence start / length.  Three short launches where torch needed ~25 (sum, any, nonzero, cumsum, where ...).
// one workgroup per tile of 1024 positions (one position per thread: coalesced)
__global__ __launch_bounds__(1024) void batch_row_counts(BatchRowsArgs a) {
  __shared__ int red[16][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long i = (long)blockIdx.x * 1024 + tid;
  int w = 0, t = 0, k = 0, bad = 0;
  if (i < a.M) {
    w = a.lab && a.lab[i] != -1;
    t = a.tl && a.tl[i] != -1;
    k = 1;
    if (a.mask) {
      const float m = a.mask[i];
      k = m != 0.f;
      if ((k && m != 1.f) || ((w || t) && !k) || (!k && (i % a.S) == 0)) bad = 1;
    }
  }
  const int nw = __builtin_popcountll(__builtin_amdgcn_ballot_w64(w != 0)), nt = __builtin_popcountll(__builtin_amdgcn_ballot_w64(t != 0));
  const int nk = __builtin_popcountll(__builtin_amdgcn_ballot_w64(k != 0)), nb = __builtin_amdgcn_ballot_w64(bad != 0) != 0;
  if (lane == 0) { red[wave][0] = nw; red[wave][1] = nt; red[wave][2] = nk; red[wave][3] = nb; }
  __syncthreads();
  if (tid == 0) {
    int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int v = 0; v < 16; ++v) { s0 += red[v][0]; s1 += red[v][1]; s2 += red[v][2]; s3 |= red[v][3]; }
    a.tile_counts[3 * blockIdx.x + 0] = s0; a.tile_counts[3 * blockIdx.x + 1] = s1; a.tile_counts[3 * blockIdx.x + 2] = s2;
    // (integer atomics: the totals do not depend on the order)
    if (s0) atomicAdd((unsigned long long*)&a.counts[1], (unsigned long long)s0);
    if (s1) atomicAdd((unsigned long long*)&a.counts[2], (unsigned long long)s1);
    if (s2) atomicAdd((unsigned long long*)&a.counts[3], (unsigned long long)s2);
    if (s3) atomicOr((unsigned long long*)&a.counts[4], 1ull);
    if (blockIdx.x == 0 && a.err) a.counts[0] = (long)a.err[0];
  }
}

// grid (ntiles, 3): blockIdx.y 0 = labels list, 1 = token-labels list, 2 = kept rows + inverse map.  A tile's first output
// slot is the sum of the earlier tiles' counts; inside the tile the slots follow the positions (ballot prefix per wave,
// the waves' totals through LDS).
__global__ __launch_bounds__(1024) void batch_row_lists(BatchRowsArgs a) {
  __shared__ int wsum[16];
  __shared__ long s_base;
  const int which = blockIdx.y;
  if ((which == 0 && !a.lab) || (which == 1 && !a.tl) || (which == 2 && !a.mask)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // base: counts of the tiles before this one (<= a few hundred values)
  long part = 0;
  for (int t = tid; t < (int)blockIdx.x; t += 1024) part += a.tile_counts[3 * t + which];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane == 0) wsum[wave] = (int)part;
  __syncthreads();
  if (tid == 0) { long b = 0; for (int v = 0; v < 16; ++v) b += wsum[v]; s_base = b; }
  __syncthreads();
  const long base = s_base;
  const long i = (long)blockIdx.x * 1024 + tid;
  bool f = false;
  if (i < a.M) f = which == 0 ? a.lab[i] != -1 : (which == 1 ? a.tl[i] != -1 : a.mask[i] != 0.f);
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(f);
  const int before = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
  __syncthreads();                       // (wsum is reused)
  if (lane == 0) wsum[wave] = __builtin_popcountll(bal);
  __syncthreads();
  int wbase = 0;
  for (int v = 0; v < wave; ++v) wbase += wsum[v];
  const long pos = base + wbase + before;
  long* out = which == 0 ? a.idx_w : (which == 1 ? a.idx_t : a.index);
  const long cap = which == 0 ? a.n_w : (which == 1 ? a.n_t : a.n_keep);   // (a stale count must not write past a list)
  if (f && pos < cap) out[pos] = i;
  if (which == 2 && i < a.M) a.inverse[i] = f ? pos : -1;
}

// per-sequence first compact row and number of kept rows, from the finished inverse map ([CLS] of every sequence kept)
__global__ __launch_bounds__(256) void batch_seq_starts(BatchRowsArgs a) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const long s0 = a.inverse[(long)b * a.S];
  const long s1 = b + 1 < a.B ? a.inverse[(long)(b + 1) * a.S] : a.n_keep;
  a.start[b] = (int)s0;
  a.length[b] = (int)(s1 - s0);
}

int vt_batch_rows_dispatch(const BatchRowsArgs& a, int lists, hipStream_t stream) {
  if (a.M <= 0 || a.S <= 0 || a.B <= 0 || (long)a.B * a.S != a.M) return VT_ERR_BAD_SHAPE;
  if (!a.tile_counts) return VT_ERR_NULL;
  const unsigned ntiles = (unsigned)((a.M + 1023) / 1024);
  if (!lists) {
    if (!a.counts) return VT_ERR_NULL;
    hipLaunchKernelGGL(batch_row_counts, dim3(ntiles), dim3(1024), 0, stream, a);
  } else {
    if ((a.lab && a.n_w > 0 && !a.idx_w) || (a.tl && a.n_t > 0 && !a.idx_t) ||
        (a.mask && ((a.n_keep > 0 && !a.index) || !a.inverse || !a.start || !a.length))) return VT_ERR_NULL;
    if (a.n_w < 0 || a.n_t < 0 || a.n_keep < 0) return VT_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(batch_row_lists, dim3(ntiles, 3), dim3(1024), 0, stream, a);
    if (a.mask) hipLaunchKernelGGL(batch_seq_starts, dim3((a.B + 255) / 256), dim3(256), 0, stream, a);
  }
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
