// Backward of the fused self-attention (head size 64): given dCtx, recompute P from Q, K and
// the forward's log-sum-exp and produce dQ | dK | dV in the packed [B*S, 3H] layout.  This is the
// autograd of oscar/modeling_bert.py:47-72 inside `loss.backward()` (tasks/viewpoint_select/
// pretrain.py:191):
//     P  = softmax(QK^T/8 + mask)      dV = P^T dO        dP = dO V^T
//     dS = P * (dP - delta)            dQ = dS K / 8      dK = dS^T Q / 8,   delta = rowsum(dO * O)
// The S x S matrices never exist in HBM.
//
// This file holds the host side -- validate, fill AttnBwdArgs, route (attn_bwd_route below: the one place that says which
// kernel serves a call), launch and round -- and the three small kernels around the launch.  The kernels proper live one
// family per file, each with its design comment, LDS map, kernel table and host launcher (attention_bwd_common.hpp):
//   attention_bwd_keyblock.hip   one workgroup per (head, batch, block of 256 keys), 4 or 8 waves: every shape.  Up to 256
//                                keys dQ is complete in the workgroup; beyond, the key blocks' dQ partials are summed in an
//                                fp32 workspace (atomics, or the planes below) that attn_dq_round[_planes] rounds to bf16
//   attention_bwd_w16.hip        16 waves, one (batch, head) pair per workgroup: S <= 256
//   attention_bwd_w16p.hip       the same made persistent and LDS-DMA pipelined: the shipped kernel at S <= 256
//
// Deterministic mode (vt_set_deterministic(1); S > 256 only -- below that nothing changes).  From three key blocks on the
// atomic sum depends on the order in which the workgroups arrive.  Under the switch the workspace is nkb = ceil(S / 256)
// PLANES of fp32 [rows, nh*64] (rows = B*S, or the compacted row count), plane kb at float offset kb * rows * nh*64, and
//   * the workgroup of key block kb STORES its dQ partial of every query row of its sequence into plane kb: the same
//     256-byte-per-row wave-instruction, a plain store instead of an add.  It does so for every row below the sequence's
//     length, also where all of its keys are masked (the partial is then 0 or tiny, but written), and a workgroup whose key
//     block lies past a short sequence of a compacted batch stores zeros there -- so every (plane, row) is written by
//     exactly one workgroup, nothing is zeroed beforehand and the memset is dropped;
//   * attn_dq_round_planes forms ((p0 + p1) + p2) + ... in ascending kb in fp32 and rounds once to bf16.
// The plane layout and this order are CONTRACT (tests/test_gpu_deterministic.py recomputes the sum from the planes).  dK and
// dV never leave their workgroup and are the same bits in both modes.
#include "attention_bwd_common.hpp"

// delta[b,h,s] = mul * sum_d dO[b,s,h,d] * O[b,s,h,d]   (one wave per token row; 64 d per head = 8 lanes x 8).
// grid = (ceil(S / 4), B): row s of sequence b, which starts at seq_start[b] (or b * S) and has seq_len[b] (or S) rows.
__global__ __launch_bounds__(256) void attn_delta_rows(const bf16_t* __restrict__ d_o, long ld_d, const bf16_t* __restrict__ o,
                                                       long ld_o, float* __restrict__ delta, int B, int S, int nh,
                                                       const int* __restrict__ seq_start, const int* __restrict__ seq_len,
                                                       float mul) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.y, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int len = seq_len ? seq_len[b] : S;
  if (s >= len) return;
  const long row = (seq_start ? (long)seq_start[b] : (long)b * S) + s;
  const int nchunks = nh * 8;  // 8-element chunks per row
  for (int c = lane; c < nchunks; c += 64) {
    const u32x4 x = *(const u32x4*)(d_o + row * ld_d + c * 8);
    const u32x4 y = *(const u32x4*)(o + row * ld_o + c * 8);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc += bf16lo(x[i]) * bf16lo(y[i]) + bf16hi(x[i]) * bf16hi(y[i]);
    // reduce the 8 lanes of a head (c>>3 == head): lanes are consecutive
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if ((c & 7) == 0) delta[((long)b * nh + (c >> 3)) * S + s] = acc * mul;   // mul = 1 - p (see the backward's dS)
  }
}

// dq (bf16, columns 0..H-1 of the packed dqkv rows) = round(dq32)
__global__ __launch_bounds__(256) void attn_dq_round(const float* __restrict__ dq32, bf16_t* __restrict__ dqkv, long ld_dqkv,
                                                     long rows, int H) {
  const int cpr = H >> 3;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cpr) return;
  const long row = i / cpr;
  const int col = (int)(i - row * cpr) * 8;
  const f32x4 x0 = *(const f32x4*)(dq32 + row * H + col), x1 = *(const f32x4*)(dq32 + row * H + col + 4);
  u32x4 o;
  o[0] = pack_bf16x2(x0[0], x0[1]); o[1] = pack_bf16x2(x0[2], x0[3]);
  o[2] = pack_bf16x2(x1[0], x1[1]); o[3] = pack_bf16x2(x1[2], x1[3]);
  *(u32x4*)(dqkv + row * ld_dqkv + col) = o;
}

// deterministic mode: dq = round(((p0 + p1) + p2) + ...), planes in ascending key-block order, fp32, one rounding to bf16
__global__ __launch_bounds__(256) void attn_dq_round_planes(const float* __restrict__ dq32, long plane, int nkb,
                                                            bf16_t* __restrict__ dqkv, long ld_dqkv, long rows, int H) {
  const int cpr = H >> 3;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cpr) return;
  const long row = i / cpr;
  const int col = (int)(i - row * cpr) * 8;
  const float* p = dq32 + row * H + col;
  f32x4 x0 = *(const f32x4*)p, x1 = *(const f32x4*)(p + 4);
  for (int kb = 1; kb < nkb; ++kb) {
    x0 += *(const f32x4*)(p + kb * plane);
    x1 += *(const f32x4*)(p + kb * plane + 4);
  }
  u32x4 o;
  o[0] = pack_bf16x2(x0[0], x0[1]); o[1] = pack_bf16x2(x0[2], x0[3]);
  o[2] = pack_bf16x2(x1[0], x1[1]); o[3] = pack_bf16x2(x1[2], x1[3]);
  *(u32x4*)(dqkv + row * ld_dqkv + col) = o;
}

// The dQ workspace a backward over S keys needs in the CURRENT mode, in bytes: 0 up to 256 keys (one key block, no
// workspace), else rows * nh*64 fp32 -- one slab for the atomic sum, ceil(S / 256) planes under vt_set_deterministic(1).
long vt_attention_bwd_ws_bytes_impl(int B, int S, int nh, long rows) {
  if (B <= 0 || S <= 256 || nh <= 0 || rows <= 0) return 0;
  const long slab = rows * nh * 64 * (long)sizeof(float);
  return vt_deterministic() ? slab * ((S + 255) / 256) : slab;
}

// The accepted values of vt_debug_set_attn_bwd_waves / ops.set_attn_bwd_waves (anything else: the default).  They are
// compared in attn_bwd_route and nowhere else.
enum AttnBwdSetting {
  ATTN_BWD_SET_W4 = 4,           // the 4-wave key-block kernel behind a separate attn_delta_rows pass
  ATTN_BWD_SET_W8 = 8,           // the 8-wave key-block kernel forming delta = rowsum(dO o O) itself
  ATTN_BWD_SET_W8_DELTA_PASS = 10,   // the same kernel behind a separate attn_delta_rows pass (the form before round 3's last
                                     // change: 330-338 against 320 us per launch at B = 256)
  ATTN_BWD_SET_W16 = 16,         // the 16-wave kernel, one (batch, head) pair per workgroup, where it serves
  ATTN_BWD_SET_W16P = 17,        // (default) its persistent, software-pipelined form where that serves
};
static std::atomic<int> g_attn_bwd_waves{ATTN_BWD_SET_W16P};
void vt_attn_bwd_set_waves(int w) {
  const bool known = w == ATTN_BWD_SET_W4 || w == ATTN_BWD_SET_W8 || w == ATTN_BWD_SET_W8_DELTA_PASS || w == ATTN_BWD_SET_W16;
  g_attn_bwd_waves.store(known ? w : ATTN_BWD_SET_W16P, std::memory_order_relaxed);
}

enum class AttnBwdFamily { KeyBlock4, KeyBlock8, W16, W16P };
struct AttnBwdRoute {
  AttnBwdFamily family;
  bool delta;   // the kernel forms delta itself; false: attn_delta_rows runs first
};

// Which kernel serves a call.  nkb = ceil(S / 256) key blocks; mask_mode 2 = the per-query bias [B, S, S]; keep_words: the
// forward's keep words were handed over; dropout: the forward dropped attention probabilities.
//   * Setting 4: always the 4-wave key-block kernel, delta from the separate pass (it reads neither keep words nor ctx).
//   * Setting 8 and 10: always the 8-wave key-block kernel; 8 forms delta in the kernel, 10 takes it from the pass.
//   * Setting 16 and 17 ask for a 16-wave kernel.  Those serve one key block (S <= 256), no per-query bias, and dropout
//     only through the forward's keep words (they do not re-derive the hash).  A call outside that -- S > 256, mask_mode 2,
//     or dropout without keep words -- FALLS BACK to the 8-wave key-block kernel exactly as under setting 8 (delta in the
//     kernel).  S = 300 with a per-query bias under setting 17 is therefore the 8-wave kernel over two key blocks.
//   * Inside that, 16 is the one-pair-per-workgroup kernel and 17 the persistent one -- unless the batch exceeds the
//     persistent kernel's limits (B * nh <= 65535 pairs, B <= 1024 sequences: attention_bwd_common.hpp), where 17 FALLS
//     BACK to the one-pair-per-workgroup kernel.  Both form delta themselves.
// The deterministic switch does not route: it selects the plane-storing instantiation of whichever key-block kernel was
// chosen, and only from two key blocks on.
static AttnBwdRoute attn_bwd_route(int setting, int nkb, int mask_mode, bool keep_words, bool dropout, int B, int nh) {
  if (setting == ATTN_BWD_SET_W4) return {AttnBwdFamily::KeyBlock4, false};
  const bool w16_serves = nkb == 1 && mask_mode != 2 && (keep_words || !dropout);
  if (setting < ATTN_BWD_SET_W16 || !w16_serves) return {AttnBwdFamily::KeyBlock8, setting != ATTN_BWD_SET_W8_DELTA_PASS};
  const bool persistent_serves = (long)B * nh <= VT_ATTN_BWD_W16P_MAX_PAIRS && B <= VT_ATTN_BWD_W16P_MAX_B;
  return {setting == ATTN_BWD_SET_W16P && persistent_serves ? AttnBwdFamily::W16P : AttnBwdFamily::W16, true};
}

int vt_attention_bwd_dispatch(const void* qkv, long ld_qkv, const void* dctx, long ld_d, const void* ctx, long ld_ctx,
                              const float* mask, int mask_additive, const float* lse, float* delta_ws, void* dqkv,
                              long ld_dqkv, float* dq32_ws, int B, int S, int nh, int head_size, hipStream_t stream,
                              const DropCfg* drop, const int* seq_start, const int* seq_len, long rows_total,
                              const uint32_t* keep_bits) {
  // ---- validate
  if (mask_additive == 2 && (!mask || seq_start)) return VT_ERR_NULL;   // per-query bias [B, S, S]
  if (!qkv || !dctx || !ctx || !lse || !delta_ws || !dqkv) return VT_ERR_NULL;
  if (head_size != 64) return VT_ERR_UNSUPPORTED;
  const int nkb = (S + 255) / 256;
  if (nkb > 1 && !dq32_ws) return VT_ERR_NULL;
  if (nkb > 65535) return VT_ERR_BAD_SHAPE;
  if (B <= 0 || S <= 0 || nh <= 0 || B > 65535 || nh > 65535) return VT_ERR_BAD_SHAPE;
  if ((ld_qkv % 8) || (ld_d % 8) || (ld_ctx % 8) || (ld_dqkv % 8)) return VT_ERR_BAD_ALIGN;
  if (((uintptr_t)qkv | (uintptr_t)dctx | (uintptr_t)ctx | (uintptr_t)dqkv) & 15) return VT_ERR_BAD_ALIGN;
  if ((seq_start == nullptr) != (seq_len == nullptr)) return VT_ERR_NULL;
  if (seq_start && (mask || rows_total <= 0)) return VT_ERR_UNSUPPORTED;   // compacted rows carry no masked keys

  // ---- fill the arguments
  const long rows = seq_start ? rows_total : (long)B * S;
  // deterministic mode: one plane per key block, every (plane, row) stored by exactly one workgroup -- nothing to zero
  const bool det = nkb > 1 && vt_deterministic();
  AttnBwdArgs a;
  a.qkv = (const bf16_t*)qkv; a.dctx = (const bf16_t*)dctx; a.mask = mask; a.mask_additive = mask_additive;
  a.lse = lse; a.delta = delta_ws; a.dqkv = (bf16_t*)dqkv;
  a.dq32 = nkb > 1 ? dq32_ws : nullptr;
  a.dq_plane = det ? rows * nh * 64 : 0;
  a.ld_qkv = ld_qkv; a.ld_d = ld_d; a.ld_dqkv = ld_dqkv; a.B = B; a.S = S; a.nh = nh;
  a.seq_start = seq_start; a.seq_len = seq_len;
  a.scale = 1.0f / sqrtf((float)head_size);
  a.drop = drop ? *drop : vt_no_drop();
  a.keep_bits = a.drop.thresh ? keep_bits : nullptr;
  a.ctx = (const bf16_t*)ctx; a.ld_ctx = ld_ctx; a.delta_mul = a.drop.thresh ? 1.0f / a.drop.scale : 1.0f;
  const bool bits = a.keep_bits != nullptr;

  // ---- route
  const AttnBwdRoute r = attn_bwd_route(g_attn_bwd_waves.load(std::memory_order_relaxed), nkb, mask_additive,
                                        keep_bits != nullptr, a.drop.thresh != 0, B, nh);

  // ---- launch and round: the delta pass where the kernel wants it, the slab's zeros, the kernel, the rounding of dQ
  if (!r.delta)
    hipLaunchKernelGGL(attn_delta_rows, dim3((unsigned)((S + 3) / 4), B), dim3(256), 0, stream, (const bf16_t*)dctx, ld_d,
                       (const bf16_t*)ctx, ld_ctx, delta_ws, B, S, nh, seq_start, seq_len, a.delta_mul);
  if (nkb > 1 && !det && hipMemsetAsync(dq32_ws, 0, (size_t)rows * nh * 64 * sizeof(float), stream) != hipSuccess) return VT_ERR_HIP;
  int rc = VT_OK;
  switch (r.family) {
    case AttnBwdFamily::W16P: rc = vt_attn_bwd_w16p_launch(a, bits, stream); break;
    case AttnBwdFamily::W16: rc = vt_attn_bwd_w16_launch(a, bits, stream); break;
    case AttnBwdFamily::KeyBlock8: rc = vt_attn_bwd_keyblock_launch(a, true, det, bits, r.delta, stream); break;
    case AttnBwdFamily::KeyBlock4: rc = vt_attn_bwd_keyblock_launch(a, false, det, false, false, stream); break;
  }
  if (rc != VT_OK) return rc;
  if (nkb > 1) {
    const long n = rows * (nh * 8);
    if (det) hipLaunchKernelGGL(attn_dq_round_planes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dq32_ws, a.dq_plane,
                                nkb, (bf16_t*)dqkv, ld_dqkv, rows, nh * 64);
    else hipLaunchKernelGGL(attn_dq_round, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dq32_ws, (bf16_t*)dqkv, ld_dqkv,
                            rows, nh * 64);
  }
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
