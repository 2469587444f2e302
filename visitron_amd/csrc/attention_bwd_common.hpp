// What the attention backward's translation units share (attention_bwd.hip: the mathematics, the dispatcher and its route;
// attention_bwd_keyblock.hip, attention_bwd_w16.hip, attention_bwd_w16p.hip: one kernel family each): the argument struct,
// five small device helpers, and the families' host launchers.  A kernel is named only in the file that defines it.
#pragma once
#include "dispatch.hpp"
#include <type_traits>

#define LOG2E 1.4426950408889634f

// A sequence's row count as the kernels use it: 1 .. S.  The engine always keeps the [CLS] row (seq_len >= 1) and never
// exceeds the padded length; a C-ABI caller that hands 0 or more than S would otherwise turn the unsigned "last row" clamps
// below (S - 1) into ~4 G rows of offset in LDS-DMA loads that are not range-checked.  Out-of-contract lengths therefore
// compute (meaningless but in-bounds) rows instead of faulting; include/visitron_hip.h states the contract.
__device__ __forceinline__ int vt_clamp_len(int len, int S) { return len < 1 ? 1 : (len > S ? S : len); }

struct AttnBwdArgs {
  const bf16_t* qkv;    // [B*S, ld_qkv]
  const bf16_t* dctx;   // [B*S, ld_d]   gradient of the context
  const float* mask;    // [B,S] raw or additive (as forward), or null
  int mask_additive;
  const float* lse;     // [B, nh, S] natural-log LSE from the forward
  const float* delta;   // [B, nh, S] rowsum(dO * O)
  bf16_t* dqkv;         // [B*S, ld_dqkv]  dq | dk | dv
  float* dq32;          // [B*S, nh*64] fp32 accumulation slab (zeroed) when S > 256, else null
  long ld_qkv, ld_d, ld_dqkv;
  int B, S, nh;
  const int* seq_start;   // compacted rows (see attention_fwd.hip): sequence b = rows seq_start[b] .. + seq_len[b];
  const int* seq_len;     // lse / delta keep their [B, nh, S] layout.  Null: sequence b = rows b*S .. b*S + S
  float scale;          // 1 / sqrt(head_size)
  DropCfg drop;         // the forward's attention-probability dropout (same seed / indexing)
  // the forward's keep decisions (AttnArgs::keep_bits in attention_fwd.hip): word [((b*nh + h) * nqb + qb) * kpitch + key],
  // bit j = keep(query 32 qb + j, key).  Null: the 8-wave kernel re-derives them from the hash like the 4-wave kernel does.
  const uint32_t* keep_bits;
  // the forward's context rows [B*S, ld_ctx] for the kernels that form delta = rowsum(dO o O) themselves (8-wave, DELTA)
  const bf16_t* ctx; long ld_ctx; float delta_mul;
  long dq_plane;        // deterministic mode (the DET instantiations): floats per plane (rows * nh*64), key block kb stores into plane kb
};

typedef __attribute__((ext_vector_type(8))) short short8v;

__device__ __forceinline__ bf16x8 tr_pair_b(unsigned addr, int second_off) {
  short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)addr);
  short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(addr + second_off));
  short8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ bf16x8 pack8(const f32x16& v, int s2) {
  u32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = pack_bf16x2(v[8 * s2 + 2 * j], v[8 * s2 + 2 * j + 1]);
  return __builtin_bit_cast(bf16x8, r);
}

// Keep flags of a lane's 16 score elements in the backward tiles, re-derived from the hash (the path without the forward's
// keep words: tests, VT_ATTN_KEEP_BITS=0): element i = query qbase + (i&3) + 8*(i>>2), this lane's key.  The attention
// sites' function (common.hpp, vt_keep_attn): byte key & 3 of the hash word of (query, key >> 2), row pitch Sp = the
// sequence's length rounded up to a multiple of 4.  The word index is linear in the query, so the hash's first multiply is
// taken once and the other queries are reached by adding multiples of (Sp / 4) * C1.
// Exact-p mode (vt_attn_wide: 16-bit fields, two keys per word): the same walk with key >> 1 / Sp >> 1 and field key & 1.
__device__ __forceinline__ void attn_bwd_keep16(const DropCfg& dr, uint32_t qbase, uint32_t key, uint32_t Sp, bool (&keep)[16]) {
  const bool wide = vt_attn_wide(dr);
  const uint32_t lg = wide ? 1u : 2u;
  const uint32_t sh = wide ? 16u * (key & 1u) : 8u * (key & 3u);
  const uint32_t fmask = wide ? 0xffffu : 0xffu, th = wide ? dr.thresh >> 16 : dr.thresh;
  const uint32_t qstep = (Sp >> lg) * VT_HASH_C1;
  const uint32_t x0 = vt_hash_pre(dr.seed, qbase * (Sp >> lg) + (key >> lg));
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t h = vt_hash_fin(x0 + (uint32_t)((i & 3) + 8 * (i >> 2)) * qstep);
    keep[i] = ((h >> sh) & fmask) >= th;
  }
}

// Deterministic mode: a key block past a short sequence contributes nothing, and says so -- zeros in its plane for this
// head's 64 columns of the sequence's `len` rows (one wave-instruction = one row's 256 bytes, as the partials are stored).
__device__ __forceinline__ void attn_bwd_zero_plane_rows(float* p, int len, int H) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (int q = wave; q < len; q += nwaves) p[(long)q * H + lane] = 0.f;
}

// An entry of a family's kernel table: the kernel and the flag of its LDS attribute (set for the kernel about to be launched)
struct AttnBwdKernel { void (*fn)(AttnBwdArgs); VtLdsAttrOnce lds; };

// ---- the families' host launchers.  Each takes the filled arguments and the selectors of its kernel table, sets the
// kernel's LDS attribute, computes its own grid and block and launches on `stream`: VT_OK, or VT_ERR_HIP where the
// attribute (or, for the persistent kernel, the device's CU count) could not be had -- nothing is launched then.
// Which family serves a call is decided in attention_bwd.hip (attn_bwd_route) and nowhere else.

// attention_bwd_keyblock.hip: one workgroup per (head, batch, block of 256 keys), any S.  eight_waves: the 8-wave kernel
// [det][bits][delta], else the 4-wave pair [det] (which knows neither keep words nor an in-kernel delta: bits and delta
// are ignored).  det: plane stores (a.dq_plane set); bits: a.keep_bits; delta: the kernel forms delta from a.ctx itself.
int vt_attn_bwd_keyblock_launch(const AttnBwdArgs& a, bool eight_waves, bool det, bool bits, bool delta, hipStream_t stream);
// attention_bwd_w16.hip: 16 waves, one (batch, head) per workgroup.  S <= 256, no per-query bias, delta in the kernel.
int vt_attn_bwd_w16_launch(const AttnBwdArgs& a, bool bits, hipStream_t stream);
// attention_bwd_w16p.hip: the persistent form of the same, one workgroup per compute unit.  Beyond what the 16-wave kernel
// asks, it serves B * nh <= VT_ATTN_BWD_W16P_MAX_PAIRS pairs of B <= VT_ATTN_BWD_W16P_MAX_B sequences (the latter sizes
// the per-sequence metadata of its LDS map, AP_META); the route sends larger batches to the 16-wave kernel.
constexpr long VT_ATTN_BWD_W16P_MAX_PAIRS = 65535;
constexpr int VT_ATTN_BWD_W16P_MAX_B = 1024;
int vt_attn_bwd_w16p_launch(const AttnBwdArgs& a, bool bits, hipStream_t stream);
