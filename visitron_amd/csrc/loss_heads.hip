// The three loss heads: per supervised row one launch gives the loss, the argmax and the gradient row (bf16 for the bf16
// engine, fp32 for the fp32 training step: the dispatch functions' dz_f32):
//   ce_softmax_rows / ce_softmax_rows_reg<8|32>  softmax cross-entropy over the MLM logits; ce_softmax_launch picks the
//                                                kernel by the padded width                    (vt_ce_softmax_dispatch)
//   ce_double_softmax_rows                       the masked-region-token head, whose criterion applies log-softmax to
//                                                a Softmax output                              (vt_ce_double_softmax_dispatch)
//   action_head_rows                             the 1-in-A action head: loss, accuracy and gradient of the whole batch in
//                                                one workgroup                                 (vt_action_head_dispatch)
// ce_store / ce_store1 write a gradient row in either format; block_sum_256 is ce_double_softmax_rows' block reduction.
#include "dispatch.hpp"

// gradient rows of the loss kernels: bf16 (the bf16 engine) or fp32 (the fp32 training step), N consecutive values
template <int N>
__device__ __forceinline__ void ce_store(bf16_t* p, const float* g) {
  if (N == 8) {
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = pack_bf16x2(g[2 * i], g[2 * i + 1]);
    *(u32x4*)p = o;
  } else {
    u32x2 o;
    o[0] = pack_bf16x2(g[0], g[1]);
    o[1] = pack_bf16x2(g[2], g[3]);
    *(u32x2*)p = o;
  }
}
template <int N>
__device__ __forceinline__ void ce_store(float* p, const float* g) {
#pragma unroll
  for (int i = 0; i < N; i += 4) *(f32x4*)(p + i) = (f32x4){g[i], g[i + 1], g[i + 2], g[i + 3]};
}
__device__ __forceinline__ void ce_store1(bf16_t* p, float v) { *p = f32_to_bf16(v); }
__device__ __forceinline__ void ce_store1(float* p, float v) { *p = v; }

// ---------------------------------------------------------------------------------------------
// Fused softmax cross-entropy over the MLM logits (tasks/viewpoint_select/encoder.py:387-389 + the
// argmax of :399 + the backward of the criterion): per supervised row, ONE kernel produces
//   loss_row = logsumexp(z) - z[y],  argmax(z),  dz = (softmax(z) - onehot(y)) * scale   (bf16, zero-padded)
// instead of torch's log_softmax / exp / scatter / mul / cast passes over a [rows, 30522] fp32 tensor.
// One 256-thread workgroup per row; the row (<= 122 KB) is read twice (second pass from L2).
template <typename DZ>
__global__ __launch_bounds__(256) void ce_softmax_rows(const float* __restrict__ z, long ldz, const int64_t* __restrict__ y,
                                                       float* __restrict__ loss_row, int64_t* __restrict__ amax,
                                                       DZ* __restrict__ dz, long lddz, int V, int Vpad, float scale) {
  __shared__ float red_m[4], red_s[4], red_bv[4];
  __shared__ int red_bi[4];
  const long row = blockIdx.x;
  const float* zp = z + row * ldz;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // pass 1: online max / sum-exp, and argmax (first index on ties, as torch.argmax)
  float m = -INFINITY, s = 0.f, bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = tid * 4; c < V; c += 1024) {
    float v[4];
    if (c + 4 <= V) {
      const f32x4 t = *(const f32x4*)(zp + c);
      v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (c + i < V) ? zp[c + i] : -INFINITY;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (v[i] > bv) { bv = v[i]; bi = c + i; }
      const float mn = fmaxf(m, v[i]);
      s = s * __expf(m - mn) + __expf(v[i] - mn);
      m = mn;
    }
  }
  // wave reduce (m, s) and (bv, bi)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    const float mn = fmaxf(m, m2);
    s = (mn == -INFINITY) ? 0.f : s * __expf(m - mn) + s2 * __expf(m2 - mn);
    m = mn;
    const float bv2 = __shfl_xor(bv, o, 64);
    const int bi2 = __shfl_xor(bi, o, 64);
    if (bv2 > bv || (bv2 == bv && bi2 < bi)) { bv = bv2; bi = bi2; }
  }
  if (lane == 0) { red_m[wave] = m; red_s[wave] = s; red_bv[wave] = bv; red_bi[wave] = bi; }
  __syncthreads();
  m = red_m[0]; s = red_s[0]; bv = red_bv[0]; bi = red_bi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const float mn = fmaxf(m, red_m[w]);
    s = s * __expf(m - mn) + red_s[w] * __expf(red_m[w] - mn);
    m = mn;
    if (red_bv[w] > bv || (red_bv[w] == bv && red_bi[w] < bi)) { bv = red_bv[w]; bi = red_bi[w]; }
  }
  const float lse = m + __logf(s);
  const int64_t label = y[row];
  if (tid == 0) {
    loss_row[row] = lse - zp[label];
    amax[row] = bi;
  }
  // pass 2: gradient row (skipped when the caller wants the loss and the argmax only: dz == nullptr)
  if (!dz) return;
  DZ* dp = dz + row * lddz;
  for (int c = tid * 8; c < Vpad; c += 2048) {
    float g[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int col = c + i;
      float p = 0.f;
      if (col < V) {
        p = __expf(zp[col] - lse);
        if (col == (int)label) p -= 1.0f;
        p *= scale;
      }
      g[i] = p;
    }
    ce_store<8>(dp + c, g);
  }
}

// The same with the row held in registers (V <= 32 768: 32 x f32x4 per thread of a 256-thread workgroup): the logits are
// read from HBM ONCE, the maximum is taken without exponentials, exp(z - max) is computed once per element and kept, the
// gradient is that value times scale / sum (no second exponential, no second read).  Against the two-pass kernel above
// (one exponential pair per element in the online pass, a third in the gradient pass, the row read twice): 440 -> ~170 us
// for [4 272, 30 522] at B = 256.
template <int NV, typename DZ>
__global__ __launch_bounds__(256) void ce_softmax_rows_reg(const float* __restrict__ z, long ldz, const int64_t* __restrict__ y,
                                                           float* __restrict__ loss_row, int64_t* __restrict__ amax,
                                                           DZ* __restrict__ dz, long lddz, int V, int Vpad, float scale) {
  __shared__ float red_a[4], red_b[4];
  __shared__ int red_i[4];
  const long row = blockIdx.x;
  const float* zp = z + row * ldz;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  f32x4 v[NV];
  float bv = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = tid * 4 + k * 1024;
    if (c + 4 <= V) v[k] = *(const f32x4*)(zp + c);
    else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[k][i] = (c + i < V) ? zp[c + i] : -INFINITY;
    }
  }
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (v[k][i] > bv) { bv = v[k][i]; bi = tid * 4 + k * 1024 + i; }   // (ascending columns per thread: first maximum)
  // block argmax (value, then smaller index: torch.argmax's first maximum)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float bv2 = __shfl_xor(bv, o, 64);
    const int bi2 = __shfl_xor(bi, o, 64);
    if (bv2 > bv || (bv2 == bv && bi2 < bi)) { bv = bv2; bi = bi2; }
  }
  if (lane == 0) { red_a[wave] = bv; red_i[wave] = bi; }
  __syncthreads();
  bv = red_a[0]; bi = red_i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (red_a[w] > bv || (red_a[w] == bv && red_i[w] < bi)) { bv = red_a[w]; bi = red_i[w]; }
  const float m = bv;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[k][i] = __expf(v[k][i] - m); s += v[k][i]; }   // (-inf columns: 0)
  s = wave_sum(s);
  if (lane == 0) red_b[wave] = s;
  __syncthreads();
  s = red_b[0] + red_b[1] + red_b[2] + red_b[3];
  const float lse = m + __logf(s);
  const int64_t label = y[row];
  if (tid == 0) {
    loss_row[row] = lse - zp[label];
    amax[row] = bi;
  }
  if (!dz) return;
  DZ* dp = dz + row * lddz;
  const float f = scale / s;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = tid * 4 + k * 1024;
    if (c < Vpad) {
      float g[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) g[i] = (c + i < V) ? v[k][i] * f - ((c + i == (int)label) ? scale : 0.f) : 0.f;
      ce_store<4>(dp + c, g);
    }
  }
}

template <typename DZ>
static void ce_softmax_launch(const float* z, long ldz, const int64_t* y, float* loss_row, int64_t* amax, DZ* dz, long lddz,
                              long rows, int V, int Vpad, float scale, hipStream_t stream) {
  const int need = (Vpad + 1023) / 1024;   // f32x4 per thread
  if (need <= 8)
    hipLaunchKernelGGL((ce_softmax_rows_reg<8, DZ>), dim3((unsigned)rows), dim3(256), 0, stream, z, ldz, y, loss_row, amax, dz,
                       lddz, V, Vpad, scale);
  else if (need <= 32)
    hipLaunchKernelGGL((ce_softmax_rows_reg<32, DZ>), dim3((unsigned)rows), dim3(256), 0, stream, z, ldz, y, loss_row, amax, dz,
                       lddz, V, Vpad, scale);
  else
    hipLaunchKernelGGL((ce_softmax_rows<DZ>), dim3((unsigned)rows), dim3(256), 0, stream, z, ldz, y, loss_row, amax, dz, lddz,
                       V, Vpad, scale);
}

// dz_f32: the gradient rows are fp32 (the fp32 training step) instead of bf16
int vt_ce_softmax_dispatch(const float* z, long ldz, const int64_t* y, float* loss_row, int64_t* amax, void* dz, long lddz,
                           long rows, int V, int Vpad, float scale, int dz_f32, hipStream_t stream) {
  if (!z || !y || !loss_row || !amax) return VT_ERR_NULL;
  if (!dz) { Vpad = (V + 7) / 8 * 8; lddz = Vpad; dz_f32 = 0; }   // no gradient row wanted
  if (rows <= 0 || V <= 0 || Vpad < V || (Vpad % 8) || lddz < Vpad) return VT_ERR_BAD_SHAPE;
  if ((ldz % 4) || (lddz % 8) || (((uintptr_t)z | (uintptr_t)dz) & 15)) return VT_ERR_BAD_ALIGN;
  if (dz_f32) ce_softmax_launch(z, ldz, y, loss_row, amax, (float*)dz, lddz, rows, V, Vpad, scale, stream);
  else ce_softmax_launch(z, ldz, y, loss_row, amax, (bf16_t*)dz, lddz, rows, V, Vpad, scale, stream);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// The masked-region-token head's loss (tasks/viewpoint_select/encoder.py:323-326, 380-385): token_head = Linear +
// Softmax, and the criterion applies log-softmax AGAIN, so per supervised row
//     p = softmax(z),   loss = logsumexp(p) - p[y],   argmax = argmax(p) = argmax(z),
//     dL/dp_i = softmax(p)_i - onehot_i,   dL/dz_j = p_j (dL/dp_j - sum_i dL/dp_i p_i).
// One workgroup per row, the row (V <= 2048 classes) held in registers, three block reductions.
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

template <typename DZ>
__global__ __launch_bounds__(256) void ce_double_softmax_rows(const float* __restrict__ z, long ldz, const int64_t* __restrict__ y,
                                                              float* __restrict__ loss_row, int64_t* __restrict__ amax,
                                                              DZ* __restrict__ dz, long lddz, int V, int Vpad, float scale) {
  __shared__ float red[4];
  __shared__ float red_bv[4];
  __shared__ int red_bi[4];
  const long row = blockIdx.x;
  const float* zp = z + row * ldz;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = tid * 8;
  float v[8];
  float bv = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = (c0 + i < V) ? zp[c0 + i] : -INFINITY;
    if (v[i] > bv) { bv = v[i]; bi = c0 + i; }
  }
  // max and argmax (first index on ties, as torch.argmax)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float bv2 = __shfl_xor(bv, o, 64);
    const int bi2 = __shfl_xor(bi, o, 64);
    if (bv2 > bv || (bv2 == bv && bi2 < bi)) { bv = bv2; bi = bi2; }
  }
  if (lane == 0) { red_bv[wave] = bv; red_bi[wave] = bi; }
  __syncthreads();
  bv = red_bv[0]; bi = red_bi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (red_bv[w] > bv || (red_bv[w] == bv && red_bi[w] < bi)) { bv = red_bv[w]; bi = red_bi[w]; }
  // p = softmax(z)
  float s1 = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) { v[i] = (c0 + i < V) ? __expf(v[i] - bv) : 0.f; s1 += v[i]; }
  const float inv = 1.0f / block_sum_256(s1, red);
  // second softmax over p: s2 = sum exp(p), t = sum exp(p) p
  float s2 = 0.f, t = 0.f;
  float e[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] *= inv;
    e[i] = (c0 + i < V) ? __expf(v[i]) : 0.f;
    s2 += e[i];
    t += e[i] * v[i];
  }
  s2 = block_sum_256(s2, red);
  t = block_sum_256(t, red);
  const int label = (int)y[row];
  const float lse2 = __logf(s2);
  // p[label] lives in thread label / 8
  __shared__ float p_label;
  if (label >= c0 && label < c0 + 8) {
    float pl = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) pl = (c0 + i == label) ? v[i] : pl;
    p_label = pl;
  }
  __syncthreads();
  const float py = p_label;
  if (tid == 0) {
    loss_row[row] = lse2 - py;
    amax[row] = bi;
  }
  const float dot = t / s2 - py;   // sum_i (softmax(p)_i - onehot_i) p_i
  if (!dz) return;                 // loss and argmax only
  DZ* dp = dz + row * lddz;
  if (c0 < Vpad) {
    float gz[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float dpi = e[i] / s2 - ((c0 + i == label) ? 1.0f : 0.f);
      gz[i] = (c0 + i < V) ? v[i] * (dpi - dot) * scale : 0.f;
    }
    ce_store<8>(dp + c0, gz);
  }
}

int vt_ce_double_softmax_dispatch(const float* z, long ldz, const int64_t* y, float* loss_row, int64_t* amax, void* dz, long lddz,
                                  long rows, int V, int Vpad, float scale, int dz_f32, hipStream_t stream) {
  if (!z || !y || !loss_row || !amax) return VT_ERR_NULL;
  if (!dz) { Vpad = (V + 7) / 8 * 8; lddz = Vpad; dz_f32 = 0; }   // no gradient row wanted
  if (rows <= 0 || V <= 0 || Vpad < V || (Vpad % 8) || lddz < Vpad) return VT_ERR_BAD_SHAPE;
  if (Vpad > 2048) return VT_ERR_UNSUPPORTED;   // the row is held in registers: 256 threads x 8 classes
  if ((lddz % 8) || ((uintptr_t)dz & 15)) return VT_ERR_BAD_ALIGN;
  if (dz_f32)
    hipLaunchKernelGGL(ce_double_softmax_rows<float>, dim3((unsigned)rows), dim3(256), 0, stream, z, ldz, y, loss_row, amax,
                       (float*)dz, lddz, V, Vpad, scale);
  else
    hipLaunchKernelGGL(ce_double_softmax_rows<bf16_t>, dim3((unsigned)rows), dim3(256), 0, stream, z, ldz, y, loss_row, amax,
                       (bf16_t*)dz, lddz, V, Vpad, scale);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---- the 1-in-A action head's loss, accuracy and gradient in one launch ------------------------------------------
// NextActionPrediction = Linear + LogSoftmax (tasks/viewpoint_select/encoder.py:142-151) and the criterion
// CrossEntropyLoss(ignore_index=-1) applies log_softmax AGAIN (encoder.py:387-391): on logits z [B, A] with targets y,
//   l = log_softmax(z), m = log_softmax(l), loss = -sum_{valid b} m[b, y_b] / n_valid, accuracy = #(argmax l == y) / B,
//   dz = g - exp(l) * rowsum(g),  g = (exp(m) - onehot(y)) * valid * grad_scale / n_valid
// (torch: two log_softmax, gather, clamp, exp, scatter_add, several multiplies and reductions = ~20 launches on a [256, 36]
// tensor).  One workgroup, one wave per row in turn; A <= 64.  n_valid = 0 gives the NaN loss torch gives and, as torch,
// a gradient of zeros (an ignored row never gets a gradient).
template <typename DZ>
__global__ __launch_bounds__(1024) void action_head_rows(const float* __restrict__ z, long ldz, const long* __restrict__ y, int B,
                                                         int A, float grad_scale, DZ* __restrict__ dz, long lddz, int Ap,
                                                         float* __restrict__ out /* loss, accuracy */) {
  __shared__ float red[16][2];
  __shared__ int redn[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int nv = 0;
  for (int b = tid; b < B; b += 1024) nv += y[b] != -1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o, 64);
  if (lane == 0) redn[wave] = nv;
  __syncthreads();
  int n_valid = 0;
  for (int w = 0; w < 16; ++w) n_valid += redn[w];
  const float inv_n = 1.0f / (float)n_valid;          // inf when nothing is valid: loss 0 * inf = NaN, as torch's 0 / 0
  float loss = 0.f, hits = 0.f;
  for (int b = wave; b < B; b += 16) {
    const float v = lane < A ? z[b * ldz + lane] : -INFINITY;
    const float mx = wave_max(v);
    const float e = lane < A ? __expf(v - mx) : 0.f;
    const float l = v - mx - __logf(wave_sum(e));                     // log_softmax(z)
    const float lm = lane < A ? l : -INFINITY;
    const float mx2 = wave_max(lm);
    const float e2 = lane < A ? __expf(lm - mx2) : 0.f;
    const float m = lm - mx2 - __logf(wave_sum(e2));                  // log_softmax(log_softmax(z))
    const long yb = y[b];
    const bool valid = yb != -1;
    const int yc = yb < 0 ? 0 : (int)yb;                              // torch: clamp(min=0) for the gather
    // argmax of l (first maximum, as torch.argmax)
    const unsigned long long atmax = __builtin_amdgcn_ballot_w64(lane < A && lm == mx2);
    const int amax = __builtin_ctzll(atmax);
    const float m_y = __shfl(m, yc < A ? yc : 0, 64);
    if (lane == 0) {
      if (valid) loss -= m_y;
      hits += (long)amax == yb ? 1.f : 0.f;
    }
    // (exp(m) - onehot) * (grad_scale / n_valid) on a valid row; an ignored row has weight 0 whatever n_valid is (torch's nll_loss
    // backward writes only the rows that are not ignored: with n_valid = 0 the loss is NaN and the gradient exactly 0)
    const float g = lane < A ? (__expf(m) - (lane == yc ? 1.f : 0.f)) * (valid ? grad_scale * inv_n : 0.f) : 0.f;
    const float gs = wave_sum(g);
    const float d = g - __expf(l) * gs;
    if (lane < Ap) ce_store1(dz + b * lddz + lane, lane < A ? d : 0.f);
  }
  if (lane == 0) { red[wave][0] = loss; red[wave][1] = hits; }
  __syncthreads();
  if (tid == 0) {
    float ls = 0.f, hs = 0.f;
    for (int w = 0; w < 16; ++w) { ls += red[w][0]; hs += red[w][1]; }
    out[0] = ls * inv_n;
    out[1] = hs / (float)B;
  }
}

int vt_action_head_dispatch(const float* z, long ldz, const long* y, int B, int A, float grad_scale, void* dz, long lddz, int Ap,
                            float* out, int dz_f32, hipStream_t stream) {
  if (!z || !y || !dz || !out) return VT_ERR_NULL;
  if (B <= 0 || A <= 0 || A > 64 || Ap < A || Ap > 64 || ldz < A || lddz < Ap) return VT_ERR_BAD_SHAPE;
  if (dz_f32)
    hipLaunchKernelGGL(action_head_rows<float>, dim3(1), dim3(1024), 0, stream, z, ldz, y, B, A, grad_scale, (float*)dz, lddz, Ap,
                       out);
  else
    hipLaunchKernelGGL(action_head_rows<bf16_t>, dim3(1), dim3(1024), 0, stream, z, ldz, y, B, A, grad_scale, (bf16_t*)dz, lddz,
                       Ap, out);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
