// Kernels of the turn-based task's decoder step (tasks/turn_based/agent_models.py:277-319, agent.py:307-338):
//   * the LSTM cell fused with its input projection: embedding gather, concat, both GEMV-shaped products, gate arithmetic
//   * the action head around the step: blocked logits, cross entropy with ignore_index, next action (teacher / argmax /
//     sample), and its gradient
#include "dispatch.hpp"
#include "row_loads.hpp"

__device__ __forceinline__ float tb_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tb_tanh(float x) {
  const float e = __expf(-2.0f * fabsf(x));
  return copysignf((1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e), x);
}

// ---------------------------------------------------------------------------------------------
// gates = [emb | feature] . W_ih^T + h_prev . W_hh^T + bias, then the arithmetic of lstm_step_kernel (rollout.hip).
// Decomposition as there: one workgroup = 16 hidden units x 4 gates x 16 batch rows.  The K axis is the 32-wide steps of
// the padded input width (Kpad / 32 of them) followed by the hs / 32 steps of the recurrent product; the 4 waves take
// every fourth step, a step's activation fragment serves the 4 gates' MFMAs, and the partial sums meet in LDS.
//
// Input columns: column c < E comes from the embedding row (table row ids[b], or row b of a ready block), E <= c < E + F
// from the feature row, c >= E + F is zero.  Neither row has an alignment the kernel may assume (a 2054-float row is
// 8-byte aligned on every other row), so a group of 4 columns is read with one 16-byte load only when it lies inside one
// source and its address is 16-byte aligned, with two 8-byte loads when 8-byte aligned, and element by element
// otherwise; no load touches an element outside columns [0, E) / [0, F) of its row.

// (load4_cat, row_loads.hpp: 4 consecutive columns of the virtual concatenated row)

__global__ __launch_bounds__(256) void tb_lstm_cell_kernel(TbCellArgs a) {
  __shared__ f32x4 part[4][4][64];   // [wave][gate][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const int hs = a.hs, E = a.E, K = a.E + a.F;
  const int kl = (lane >> 4) * 8;               // the lane's 8 consecutive k inside a 32-wide MFMA step
  const int brow = b0 + (lane & 15);
  const bool bvalid = brow < a.B;
  const float* ep = nullptr;
  const float* fp = nullptr;
  const float* hp = nullptr;
  if (bvalid) {
    if (a.ids) {
      const long id = a.ids[brow];
      if (id >= 0 && id < a.A) ep = a.table + id * a.ld_t;
      else if (a.err && blockIdx.x == 0 && wave == 0 && lane < 16) *a.err = 1;   // the row's embedding counts as zero
    } else {
      ep = a.x_emb + (long)brow * a.ld_e;
    }
    fp = a.feature + (long)brow * a.ld_f;
    hp = a.h_prev + (long)brow * hs;
  }
  const bf16_t* wih = a.w_ih + (long)(h0 + (lane & 15)) * a.ldw + kl;
  const bf16_t* whh = a.w_hh + (long)(h0 + (lane & 15)) * hs + kl;
  const int nx = a.Kpad >> 5, nsteps = nx + (hs >> 5);
  f32x4 acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int s = wave; s < nsteps; s += 4) {
    f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = {0.f, 0.f, 0.f, 0.f};
    const bf16_t* wp;
    long gstride;
    if (s < nx) {
      const int c = s * 32 + kl;
      if (bvalid) { x0 = load4_cat(ep, E, fp, K, c); x1 = load4_cat(ep, E, fp, K, c + 4); }
      wp = wih + s * 32;
      gstride = (long)hs * a.ldw;
    } else {
      const int k = (s - nx) * 32;
      if (bvalid) { x0 = *(const f32x4*)(hp + k + kl); x1 = *(const f32x4*)(hp + k + kl + 4); }
      wp = whh + k;
      gstride = (long)hs * hs;
    }
    u32x4 xb;
    xb[0] = pack_bf16x2(x0[0], x0[1]); xb[1] = pack_bf16x2(x0[2], x0[3]);
    xb[2] = pack_bf16x2(x1[0], x1[1]); xb[3] = pack_bf16x2(x1[2], x1[3]);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const u32x4 wv = *(const u32x4*)(wp + g * gstride);
      acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wv), __builtin_bit_cast(bf16x8, xb),
                                                       acc[g], 0, 0, 0);
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) part[wave][g][lane] = acc[g];
  __syncthreads();
  // thread (lane, r = wave): element hidden = h0 + 4*(lane/16) + r, batch = b0 + lane%16
  const int r = wave;
  const int hid = h0 + 4 * (lane >> 4) + r;
  if (!bvalid) return;
  const long e = (long)brow * hs + hid;
  float gate[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float s = a.bias[g * hs + hid];
#pragma unroll
    for (int w = 0; w < 4; ++w) s += ((const float*)&part[w][g][lane])[r];
    gate[g] = s;
  }
  const float ig = tb_sigmoid(gate[0]), fg = tb_sigmoid(gate[1]), gg = tb_tanh(gate[2]), og = tb_sigmoid(gate[3]);
  const float cp = a.c_prev[e];
  const float cn = fg * cp + ig * gg;
  if (a.sv_gates) {   // training: what lstm_step_bwd_kernel reads
    float* sg = a.sv_gates + (long)brow * 4 * hs + hid;
    sg[0] = ig; sg[hs] = fg; sg[2 * hs] = gg; sg[3 * hs] = og;
  }
  if (a.sv_c) a.sv_c[e] = cp;
  if (a.sv_h) a.sv_h[e] = f32_to_bf16(a.h_prev[e]);
  a.c_out[e] = cn;
  a.h_out[e] = og * tb_tanh(cn);
}

int vt_tb_lstm_cell_dispatch(const TbCellArgs& a, hipStream_t stream) {
  if (!a.feature || !a.h_prev || !a.c_prev || !a.w_ih || !a.w_hh || !a.bias || !a.h_out || !a.c_out) return VT_ERR_NULL;
  if (a.ids ? (!a.table || a.x_emb) : !a.x_emb) return VT_ERR_NULL;   // exactly one form of the first operand
  if (a.B <= 0 || a.E < 1 || a.F < 1 || a.hs <= 0 || (a.hs % 128) != 0 || (a.ids && a.A < 1)) return VT_ERR_BAD_SHAPE;
  if ((a.Kpad & 31) || a.Kpad < a.E + a.F || a.ldw < a.Kpad) return VT_ERR_BAD_SHAPE;
  if (a.ld_f < a.F || (a.ids ? a.ld_t < a.E : a.ld_e < a.E)) return VT_ERR_BAD_SHAPE;
  if ((const void*)a.h_prev == (const void*)a.h_out) return VT_ERR_UNSUPPORTED;   // other workgroups still read it
  if ((a.ldw & 7) || ((((uintptr_t)a.h_prev) | ((uintptr_t)a.w_ih) | ((uintptr_t)a.w_hh)) & 15)) return VT_ERR_BAD_ALIGN;
  if ((((uintptr_t)a.feature) | ((uintptr_t)a.table) | ((uintptr_t)a.x_emb)) & 3) return VT_ERR_BAD_ALIGN;
  if ((a.B + 15) / 16 > 65535) return VT_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(tb_lstm_cell_kernel, dim3(a.hs / 16, (a.B + 15) / 16), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------
// The action head of one step (agent.py:316-338): l = logit with the blocked entries at -inf;
//   loss = mean over the counted rows (target != ignore_index) of logsumexp(l) - l[target]
//   a_t  = target | lowest index of the row maximum | inverse CDF in index order at u = (hash32(seed, row) >> 8) 2^-24
// One wave per row, one lane per action (A <= 64), reductions inside the wave.  One workgroup of 16 waves walks all rows:
// wave w takes rows w, w + 16, ... in order and thread 0 adds the 16 partial sums in order, so the loss is reproducible.

__device__ __forceinline__ float tb_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float tb_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

#define TB_HEAD_WAVES 16
__global__ __launch_bounds__(64 * TB_HEAD_WAVES) void tb_action_head_kernel(TbHeadArgs a) {
  __shared__ float psum[TB_HEAD_WAVES], pcnt[TB_HEAD_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float sum = 0.f, cnt = 0.f;
  for (int row = wave; row < a.B; row += TB_HEAD_WAVES) {
    const bool in = lane < a.A;
    const bool blk = in && a.blocked && a.blocked[(long)row * a.ld_blk + lane] != 0;
    const float l = (in && !blk) ? a.logit[(long)row * a.ld + lane] : -INFINITY;
    const float m = tb_wave_max(l);
    const float ex = in ? expf(l - m) : 0.f;        // every entry blocked: -inf - -inf = NaN, as torch's softmax gives
    const float z = tb_wave_sum(ex);
    const long tgt = a.target[row];
    bool counted = tgt != a.ignore_index;
    if (counted && (tgt < 0 || tgt >= a.A)) {       // torch asserts on the device; here: the row is left out, flag raised
      counted = false;
      if (a.err && lane == 0) *a.err = 1;
    }
    if (counted) {
      const float lt = __shfl(l, (int)tgt, 64);
      sum += (logf(z) + m) - lt;                    // a blocked target: +inf
      cnt += 1.f;
    }
    long pick = tgt;
    if (a.mode == 1) {
      const unsigned long long eq = __ballot(in && l == m);
      pick = eq ? (long)__ffsll((long long)eq) - 1 : 0;
    } else if (a.mode == 2) {
      float cum = ex;                                // inclusive scan in index order
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(cum, o, 64);
        if (lane >= o) cum += up;
      }
      const float total = __shfl(cum, a.A - 1, 64);
      const float u = (float)(vt_hash32(a.seed, (uint32_t)row) >> 8) * 5.9604644775390625e-08f;   // 2^-24
      const float thr = u * total;
      const unsigned long long hit = __ballot(in && cum > thr);
      const unsigned long long open = __ballot(in && !blk);
      if (hit) pick = (long)__ffsll((long long)hit) - 1;
      else pick = open ? 63 - (long)__clzll((long long)open) : 0;   // rounding left none: the last unblocked entry
    }
    if (a.a_t && lane == 0) a.a_t[row] = pick;
  }
  if (lane == 0) { psum[wave] = sum; pcnt[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f, c = 0.f;
    for (int w = 0; w < TB_HEAD_WAVES; ++w) { s += psum[w]; c += pcnt[w]; }
    a.loss[0] = s / c;                               // no counted row: 0 / 0 = NaN, as torch's mean reduction gives
    a.count[0] = c;
  }
}

int vt_tb_action_head_dispatch(const TbHeadArgs& a, hipStream_t stream) {
  if (!a.logit || !a.target || !a.loss || !a.count) return VT_ERR_NULL;
  if (a.B <= 0 || a.A < 1 || a.A > 64 || a.ld < a.A || (a.blocked && a.ld_blk < a.A)) return VT_ERR_BAD_SHAPE;
  if (a.mode < 0 || a.mode > 2) return VT_ERR_UNSUPPORTED;
  if (a.mode != 0 && !a.a_t) return VT_ERR_NULL;
  hipLaunchKernelGGL(tb_action_head_kernel, dim3(1), dim3(64 * TB_HEAD_WAVES), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// dlogit = g (softmax(l) - onehot(target)) / n_counted on the counted rows, 0 on the others and on every blocked entry
// (the block is a fill: no gradient passes it).  g and n_counted are read on the device (no host round trip).
__global__ __launch_bounds__(256) void tb_action_head_bwd_kernel(TbHeadBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B) return;
  const bool in = lane < a.A;
  const bool blk = in && a.blocked && a.blocked[(long)row * a.ld_blk + lane] != 0;
  const float l = (in && !blk) ? a.logit[(long)row * a.ld + lane] : -INFINITY;
  const float m = tb_wave_max(l);
  const float ex = in ? expf(l - m) : 0.f;
  const float z = tb_wave_sum(ex);
  const long tgt = a.target[row];
  const bool counted = tgt != a.ignore_index && tgt >= 0 && tgt < a.A;
  float d = 0.f;
  if (counted && !blk) d = (a.g[0] / a.count[0]) * (ex / z - (lane == tgt ? 1.f : 0.f));
  if (in) a.dlogit[(long)row * a.ld_d + lane] = d;
}

int vt_tb_action_head_bwd_dispatch(const TbHeadBwdArgs& a, hipStream_t stream) {
  if (!a.logit || !a.target || !a.g || !a.count || !a.dlogit) return VT_ERR_NULL;
  if (a.B <= 0 || a.A < 1 || a.A > 64 || a.ld < a.A || a.ld_d < a.A || (a.blocked && a.ld_blk < a.A)) return VT_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(tb_action_head_bwd_kernel, dim3((a.B + 3) / 4), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
