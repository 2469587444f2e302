// Rectangular multi-head attention, head size 64: Sq queries over Sk >= Sq keys, forward and backward.
//
// Serves encoder_history_states (oscar/modeling_bert.py:37-41, 148-155): keys and values come from cat([history, hidden], 1),
// queries from the hidden positions alone.  The packed layout of the square kernels is kept: qkv is [B*Sk, ld] = q | k | v,
// sequence b owns rows b*Sk .. b*Sk+Sk-1, its Sh = Sk - Sq history rows come first and its queries are the LAST Sq rows
// (the q columns of history rows are never read).  ctx, dctx and lse are indexed by the query: [B*Sq, nh*64], [B, nh, Sq].
//
// Written for correctness first, as fp32_path.hip was: one wave per workgroup, v_mfma_f32_16x16x32_bf16, every operand
// fragment addressed by the instruction's lane map and nothing else (lane l, c = l & 15, g = l >> 4):
//   A[row c][k = 8g + j],  B[k = 8g + j][col c]  (j = 0 .. 7),   C/D[row 4g + reg][col c]  (reg = 0 .. 3).
// All three kernels share one shape.  A wave OWNS 16 rows (forward and dQ: queries; dK/dV: keys) which stay on the lane's
// column c, and walks the OTHER side (keys; queries) in blocks of 32:
//   X^T[other][own] = Other . Own^T     A = rows of the other side, B = the wave's own rows: 16-byte loads from the rows
//   Out^T[d][own]  += W^T[d][other] . X^T[other][own]
// The second product sums over X^T's ROW index, so the two 16-row tiles of a block, converted to bf16, ARE its B operand
// (no LDS, no lane movement): element j of lane group g is other-row 16 (j >> 2) + 4g + (j & 3) of the block, and the A
// operand W^T takes the same order, read element-wise from a row-major LDS copy of the block's W rows.
// No atomics and no workspace: dK / dV are formed by one pass per key tile over all queries, dQ by one pass per query tile
// over all keys, both recomputing P from lse, each with its own rowsum(dO o ctx); the history rows' dQ is written as zeros
// by workgroups of the dQ launch.  Every sum has a fixed order: the backward is bitwise reproducible in any mode.
//
// Softmax in fp32 on s = fma(q.k, 1/8, bias).  Forward: a first pass over the keys takes the row maximum, a second forms
// p = exp(s - max), sums the UNROUNDED p into the normaliser, drops, rounds p to bf16 once and accumulates P.V; 1 / l,
// dropout's 1 / (1 - p) and the head scale multiply the fp32 accumulators (the bound of tests/helpers_attention.py).
// Dropout: the attention sites' form (common.hpp, vt_keep_attn): per (b, h) the seed is hash32(seed, b*nh + h), the element
// index is query * Sk' + key with the query counted from the first NEW position and Sk' = Sk rounded up to a multiple of 4
// (Sq == Sk: the square kernels' index).
#include "dispatch.hpp"

struct RectArgs {
  const bf16_t* qkv;        // [B*Sk, ld_qkv]
  const float* mask;        // null; [B, Sk] raw (mode 0) or additive (1); additive per query [B, Sq, Sk] (2)
  int mask_mode;
  const float* head_scale;  // [nh] or null (forward)
  bf16_t* ctx;              // [B*Sq, ld_ctx]: forward output, backward input
  float* lse;               // [B, nh, Sq]: forward output (or null), backward input
  const bf16_t* dctx;       // [B*Sq, ld_d]
  bf16_t* dqkv;             // [B*Sk, ld_dqkv]
  // keep words, one per (batch, head, 32-query block, key): word ((b*nh + h) * nqb + qb) * kpitch + key, bit j = keep(query
  // 32 qb + j, key), nqb = ceil(Sq / 32), kpitch = Sk rounded up to 32.  Forward: written when non-null and dropout is on.
  // Backward: read when non-null, else the decisions are taken from the hash again.
  uint32_t* keep_bits;
  long ld_qkv, ld_ctx, ld_d, ld_dqkv;
  int B, Sq, Sk, nh;
  DropCfg drop;
};

#define RECT_LOG2E 1.4426950408889634f
#define RECT_PITCH 68   // bf16 per row of an LDS tile (64 + 4: the four lane groups' rows fall into different banks)

typedef __attribute__((ext_vector_type(8))) short rect_short8;

__device__ __forceinline__ float rect_bias(const RectArgs& a, int b, int q, int key) {
  if (!a.mask) return 0.f;
  if (a.mask_mode == 2) return a.mask[((long)b * a.Sq + q) * a.Sk + key];
  const float m = a.mask[(long)b * a.Sk + key];
  return a.mask_mode ? m : (1.0f - m) * -10000.0f;
}

// rows row0 .. row0 + 31 (clamped to last) of a [*, ld] bf16 matrix, 64 columns from col0 -> LDS tile[32][RECT_PITCH]
__device__ __forceinline__ void rect_stage32(const bf16_t* src, long ld, long first, int row0, int last, bf16_t* tile, int lane) {
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const int chunk = lane + 64 * n;        // 8-byte chunks, 16 per row
    const int row = chunk >> 4, c8 = chunk & 15;
    int r = row0 + row;
    r = r < last ? r : last;
    const u32x2 v = *(const u32x2*)(src + (first + r) * ld + 4 * c8);
    *(u32x2*)(tile + row * RECT_PITCH + 4 * c8) = v;
  }
}

// A operand W^T[row d = d0 + c][k = other-row 16 (j >> 2) + 4g + (j & 3)] from a row-major LDS tile of the block's W rows
__device__ __forceinline__ bf16x8 rect_tfrag(const bf16_t* tile, int g, int d) {
  rect_short8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (short)tile[(16 * (j >> 2) + 4 * g + (j & 3)) * RECT_PITCH + d];
  return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ bf16x8 rect_pack8(const float (&x)[8]) {
  u32x4 w;
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = pack_bf16x2(x[2 * j], x[2 * j + 1]);
  return __builtin_bit_cast(bf16x8, w);
}

__device__ __forceinline__ f32x4 rect_dot64(const bf16x8 (&a)[2], const bf16x8 (&b)[2]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], acc, 0, 0, 0);
  return acc;
}

// the two k-steps of a 64-wide row as an operand fragment: elements 32 step + 8g .. + 7
__device__ __forceinline__ void rect_rowfrag(const bf16_t* row, int g, bf16x8 (&f)[2]) {
  f[0] = *(const bf16x8*)(row + 8 * g);
  f[1] = *(const bf16x8*)(row + 32 + 8 * g);
}

__device__ __forceinline__ bool rect_keep(const RectArgs& a, const DropCfg& dr, const uint32_t* words, int q, int key,
                                          uint32_t skp) {
  if (words) return (words[(long)(q >> 5) * ((a.Sk + 31) & ~31) + key] >> (q & 31)) & 1u;
  return vt_keep_attn(dr, (uint32_t)q * skp + (uint32_t)key);
}

// ---- forward: one wave = 32 queries (two 16-query tiles, so a keep word is written whole by one wave) ----------------------
__global__ __launch_bounds__(64) void attention_rect_fwd_d64(RectArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t vt_tile[32 * RECT_PITCH];
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * 32;
  const int Sq = a.Sq, Sk = a.Sk, Sh = Sk - Sq, H = a.nh * 64;
  const bf16_t* base = a.qkv + head * 64;
  const long first = (long)b * Sk;

  int qi[2];
  bf16x8 qf[2][2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = q0 + 16 * qt + c;
    qi[qt] = q < Sq ? q : Sq - 1;
    rect_rowfrag(base + (first + Sh + qi[qt]) * a.ld_qkv, g, qf[qt]);
  }

  // pass 1: the row maximum
  float m[2] = {-INFINITY, -INFINITY};
  for (int k0 = 0; k0 < Sk; k0 += 16) {
    const int kr = k0 + c < Sk ? k0 + c : Sk - 1;
    bf16x8 kf[2];
    rect_rowfrag(base + H + (first + kr) * a.ld_qkv, g, kf);
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const f32x4 acc = rect_dot64(kf, qf[qt]);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int key = k0 + 4 * g + reg;
        if (key < Sk) m[qt] = fmaxf(m[qt], fmaf(acc[reg], 0.125f, rect_bias(a, b, qi[qt], key)));
      }
    }
  }
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    m[qt] = fmaxf(m[qt], __shfl_xor(m[qt], 16, 64));
    m[qt] = fmaxf(m[qt], __shfl_xor(m[qt], 32, 64));
  }

  // pass 2: p, the normaliser, dropout, P.V
  DropCfg dr = a.drop;
  dr.seed = vt_hash32(a.drop.seed, (uint32_t)(b * a.nh + head));
  const uint32_t skp = (uint32_t)(Sk + 3) & ~3u;
  const bool write_keep = a.keep_bits && dr.thresh;
  uint32_t* words = write_keep ? a.keep_bits + (((long)b * a.nh + head) * ((Sq + 31) >> 5) + blockIdx.x) * ((Sk + 31) & ~31) : nullptr;
  float l[2] = {0.f, 0.f};
  f32x4 o[2][4];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[qt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int kb = 0; kb < Sk; kb += 32) {
    __syncthreads();
    rect_stage32(base + 2 * H, a.ld_qkv, first, kb, Sk - 1, vt_tile, lane);
    __syncthreads();
    float p[2][8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kr = kb + 16 * t + c < Sk ? kb + 16 * t + c : Sk - 1;
      bf16x8 kf[2];
      rect_rowfrag(base + H + (first + kr) * a.ld_qkv, g, kf);
      const f32x4 acc0 = rect_dot64(kf, qf[0]), acc1 = rect_dot64(kf, qf[1]);   // [key 4g + reg][query c]
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int key = kb + 16 * t + 4 * g + reg;
        const int keyc = key < Sk ? key : Sk - 1;
        bool kp[2] = {true, true};
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          float pv = 0.f;
          if (key < Sk) {
            const float s = fmaf(qt ? acc1[reg] : acc0[reg], 0.125f, rect_bias(a, b, qi[qt], key));
            pv = __builtin_amdgcn_exp2f((s - m[qt]) * RECT_LOG2E);
          }
          l[qt] += pv;                      // the normaliser sums every probability, dropped or not, unrounded
          if (dr.thresh) kp[qt] = vt_keep_attn(dr, (uint32_t)qi[qt] * skp + (uint32_t)keyc);
          p[qt][4 * t + reg] = kp[qt] ? pv : 0.f;
        }
        if (write_keep) {   // uniform
          // lanes 16g .. 16g + 15 hold this key (4g + reg of the tile) for queries 0 .. 15 of each query tile
          const uint64_t m0 = __builtin_amdgcn_ballot_w64(kp[0]), m1 = __builtin_amdgcn_ballot_w64(kp[1]);
          const uint32_t w = (uint32_t)((m0 >> (16 * g)) & 0xffffu) | ((uint32_t)((m1 >> (16 * g)) & 0xffffu) << 16);
          if (c == 0 && key < Sk) words[key] = w;
        }
      }
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const bf16x8 vf = rect_tfrag(vt_tile, g, 16 * dt + c);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
        o[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, rect_pack8(p[qt]), o[qt][dt], 0, 0, 0);
    }
  }

#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float lt = l[qt] + __shfl_xor(l[qt], 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    const int q = q0 + 16 * qt + c;
    if (q >= Sq) continue;
    float inv = 1.0f / lt;
    if (dr.thresh) inv *= dr.scale;
    if (a.head_scale) inv *= a.head_scale[head];
    if (a.lse && g == 0) a.lse[((long)b * a.nh + head) * Sq + q] = m[qt] + logf(lt);
    bf16_t* op = a.ctx + ((long)b * Sq + q) * a.ld_ctx + head * 64 + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      u32x2 w;
      w[0] = pack_bf16x2(o[qt][dt][0] * inv, o[qt][dt][1] * inv);
      w[1] = pack_bf16x2(o[qt][dt][2] * inv, o[qt][dt][3] * inv);
      *(u32x2*)(op + 16 * dt) = w;
    }
  }
}

// ---- backward, dK and dV: one wave = 16 keys, over all queries in blocks of 32 -----------------------------------------------
__global__ __launch_bounds__(64) void attention_rect_bwd_dkv_d64(RectArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t q_tile[32 * RECT_PITCH];
  __shared__ __attribute__((aligned(16))) bf16_t do_tile[32 * RECT_PITCH];
  __shared__ float delta_s[32];
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, head = blockIdx.y, k0 = blockIdx.x * 16;
  const int Sq = a.Sq, Sk = a.Sk, Sh = Sk - Sq, H = a.nh * 64;
  const bf16_t* base = a.qkv + head * 64;
  const long first = (long)b * Sk, qfirst = (long)b * Sq;
  const int key = k0 + c, keyc = key < Sk ? key : Sk - 1;

  bf16x8 kf[2], vf[2];   // B operands: the wave's own keys on the column
  rect_rowfrag(base + H + (first + keyc) * a.ld_qkv, g, kf);
  rect_rowfrag(base + 2 * H + (first + keyc) * a.ld_qkv, g, vf);

  DropCfg dr = a.drop;
  dr.seed = vt_hash32(a.drop.seed, (uint32_t)(b * a.nh + head));
  const uint32_t skp = (uint32_t)(Sk + 3) & ~3u;
  const uint32_t* words = (a.keep_bits && dr.thresh) ? a.keep_bits + ((long)b * a.nh + head) * ((Sq + 31) >> 5) * ((Sk + 31) & ~31) : nullptr;
  const float cdrop = dr.thresh ? dr.scale : 1.0f;
  const float* lse = a.lse + ((long)b * a.nh + head) * Sq;

  f32x4 dk[4], dv[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) { dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

  for (int qb = 0; qb < Sq; qb += 32) {
    __syncthreads();
    rect_stage32(base, a.ld_qkv, first + Sh, qb, Sq - 1, q_tile, lane);
    rect_stage32(a.dctx + head * 64, a.ld_d, qfirst, qb, Sq - 1, do_tile, lane);
    __syncthreads();
    {   // delta = rowsum(dO o ctx) of the block's queries: two lanes per query, 32 columns each
      const int row = lane >> 1, half = lane & 1;
      const int q = qb + row < Sq ? qb + row : Sq - 1;
      const bf16_t* cp = a.ctx + (qfirst + q) * a.ld_ctx + head * 64 + 32 * half;
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 32; ++i) s = fmaf(bf16_to_f32(do_tile[row * RECT_PITCH + 32 * half + i]), bf16_to_f32(cp[i]), s);
      s += __shfl_xor(s, 1, 64);
      if (half == 0) delta_s[row] = s;
    }
    __syncthreads();
    float pk[8], ds[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int qr = qb + 16 * t + c < Sq ? qb + 16 * t + c : Sq - 1;
      bf16x8 qa[2], da[2];   // A operands: the block's queries on the row
      rect_rowfrag(base + (first + Sh + qr) * a.ld_qkv, g, qa);
      rect_rowfrag(a.dctx + head * 64 + (qfirst + qr) * a.ld_d, g, da);
      const f32x4 sacc = rect_dot64(qa, kf);    // [query 4g + reg][key c]
      const f32x4 dpacc = rect_dot64(da, vf);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int ql = 16 * t + 4 * g + reg, q = qb + ql;
        const int qc = q < Sq ? q : Sq - 1;
        float p = 0.f;
        if (q < Sq && key < Sk) {
          const float s = fmaf(sacc[reg], 0.125f, rect_bias(a, b, qc, keyc));
          p = __builtin_amdgcn_exp2f((s - lse[qc]) * RECT_LOG2E);
        }
        const bool keep = dr.thresh ? rect_keep(a, dr, words, qc, keyc, skp) : true;
        const float dp = keep ? dpacc[reg] * cdrop : 0.f;
        pk[4 * t + reg] = keep ? p : 0.f;
        ds[4 * t + reg] = p * (dp - delta_s[ql]);
      }
    }
    const bf16x8 pb = rect_pack8(pk), dsb = rect_pack8(ds);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rect_tfrag(do_tile, g, 16 * dt + c), pb, dv[dt], 0, 0, 0);
      dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rect_tfrag(q_tile, g, 16 * dt + c), dsb, dk[dt], 0, 0, 0);
    }
  }

  if (key >= Sk) return;
  bf16_t* op = a.dqkv + (first + key) * a.ld_dqkv + head * 64 + 4 * g;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    u32x2 w;
    w[0] = pack_bf16x2(dk[dt][0] * 0.125f, dk[dt][1] * 0.125f);
    w[1] = pack_bf16x2(dk[dt][2] * 0.125f, dk[dt][3] * 0.125f);
    *(u32x2*)(op + H + 16 * dt) = w;
    w[0] = pack_bf16x2(dv[dt][0] * cdrop, dv[dt][1] * cdrop);
    w[1] = pack_bf16x2(dv[dt][2] * cdrop, dv[dt][3] * cdrop);
    *(u32x2*)(op + 2 * H + 16 * dt) = w;
  }
}

// ---- backward, dQ: one wave = 16 queries over all keys in blocks of 32; the workgroups past the query tiles write the zeros
// of the history rows' dQ, 16 rows each ------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void attention_rect_bwd_dq_d64(RectArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t k_tile[32 * RECT_PITCH];
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, head = blockIdx.y;
  const int Sq = a.Sq, Sk = a.Sk, Sh = Sk - Sq, H = a.nh * 64;
  const long first = (long)b * Sk, qfirst = (long)b * Sq;
  const int nqt = (Sq + 15) >> 4;
  if ((int)blockIdx.x >= nqt) {   // uniform
    const int row = ((int)blockIdx.x - nqt) * 16 + (lane >> 2);
    if (row < Sh) {
      bf16_t* zp = a.dqkv + (first + row) * a.ld_dqkv + head * 64 + 16 * (lane & 3);
      const u32x4 z = {0u, 0u, 0u, 0u};
      ((u32x4*)zp)[0] = z;
      ((u32x4*)zp)[1] = z;
    }
    return;
  }
  const bf16_t* base = a.qkv + head * 64;
  const int q = blockIdx.x * 16 + c, qc = q < Sq ? q : Sq - 1;

  bf16x8 qf[2], df[2];   // B operands: the wave's own queries on the column
  rect_rowfrag(base + (first + Sh + qc) * a.ld_qkv, g, qf);
  rect_rowfrag(a.dctx + head * 64 + (qfirst + qc) * a.ld_d, g, df);
  float delta = 0.f;     // rowsum(dO o ctx) of query c: 16 columns per lane group
  {
    const bf16_t* dp = a.dctx + head * 64 + (qfirst + qc) * a.ld_d + 16 * g;
    const bf16_t* cp = a.ctx + head * 64 + (qfirst + qc) * a.ld_ctx + 16 * g;
#pragma unroll
    for (int i = 0; i < 16; ++i) delta = fmaf(bf16_to_f32(dp[i]), bf16_to_f32(cp[i]), delta);
    delta += __shfl_xor(delta, 16, 64);
    delta += __shfl_xor(delta, 32, 64);
  }
  const float lse_q = a.lse[((long)b * a.nh + head) * Sq + qc];

  DropCfg dr = a.drop;
  dr.seed = vt_hash32(a.drop.seed, (uint32_t)(b * a.nh + head));
  const uint32_t skp = (uint32_t)(Sk + 3) & ~3u;
  const uint32_t* words = (a.keep_bits && dr.thresh) ? a.keep_bits + ((long)b * a.nh + head) * ((Sq + 31) >> 5) * ((Sk + 31) & ~31) : nullptr;
  const float cdrop = dr.thresh ? dr.scale : 1.0f;

  f32x4 dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int kb = 0; kb < Sk; kb += 32) {
    __syncthreads();
    rect_stage32(base + H, a.ld_qkv, first, kb, Sk - 1, k_tile, lane);
    __syncthreads();
    float ds[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kr = kb + 16 * t + c < Sk ? kb + 16 * t + c : Sk - 1;
      bf16x8 ka[2], va[2];   // A operands: the block's keys on the row
      rect_rowfrag(base + H + (first + kr) * a.ld_qkv, g, ka);
      rect_rowfrag(base + 2 * H + (first + kr) * a.ld_qkv, g, va);
      const f32x4 sacc = rect_dot64(ka, qf);    // [key 4g + reg][query c]
      const f32x4 dpacc = rect_dot64(va, df);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int key = kb + 16 * t + 4 * g + reg;
        const int keyc = key < Sk ? key : Sk - 1;
        float p = 0.f;
        if (key < Sk && q < Sq) {
          const float s = fmaf(sacc[reg], 0.125f, rect_bias(a, b, qc, keyc));
          p = __builtin_amdgcn_exp2f((s - lse_q) * RECT_LOG2E);
        }
        const bool keep = dr.thresh ? rect_keep(a, dr, words, qc, keyc, skp) : true;
        const float dp = keep ? dpacc[reg] * cdrop : 0.f;
        ds[4 * t + reg] = p * (dp - delta);
      }
    }
    const bf16x8 dsb = rect_pack8(ds);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rect_tfrag(k_tile, g, 16 * dt + c), dsb, dq[dt], 0, 0, 0);
  }

  if (q >= Sq) return;
  bf16_t* op = a.dqkv + (first + Sh + q) * a.ld_dqkv + head * 64 + 4 * g;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    u32x2 w;
    w[0] = pack_bf16x2(dq[dt][0] * 0.125f, dq[dt][1] * 0.125f);
    w[1] = pack_bf16x2(dq[dt][2] * 0.125f, dq[dt][3] * 0.125f);
    *(u32x2*)(op + 16 * dt) = w;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int rect_check(const RectArgs& a, int head_size) {
  if (head_size != 64) return VT_ERR_UNSUPPORTED;
  if (a.B <= 0 || a.nh <= 0 || a.B > 65535 || a.nh > 65535) return VT_ERR_BAD_SHAPE;
  if (a.Sq < 1 || a.Sq > a.Sk || a.Sk > 1024) return VT_ERR_UNSUPPORTED;   // the forward bound counts sums of <= 1 025 terms
  if (a.mask && (a.mask_mode < 0 || a.mask_mode > 2)) return VT_ERR_UNSUPPORTED;
  if ((a.ld_qkv % 8) || (a.ld_ctx % 8) || a.ld_qkv < 3L * a.nh * 64 || a.ld_ctx < (long)a.nh * 64) return VT_ERR_BAD_ALIGN;
  if (((uintptr_t)a.qkv | (uintptr_t)a.ctx) & 15) return VT_ERR_BAD_ALIGN;
  return VT_OK;
}

int vt_attention_rect_fwd_dispatch(const void* qkv, long ld_qkv, const float* mask, int mask_mode, const float* head_scale,
                                   void* ctx, long ld_ctx, float* lse, int B, int Sq, int Sk, int nh, int head_size,
                                   const DropCfg& drop, uint32_t* keep_bits, hipStream_t stream) {
  if (!qkv || !ctx) return VT_ERR_NULL;
  RectArgs a = {};
  a.qkv = (const bf16_t*)qkv; a.mask = mask; a.mask_mode = mask_mode; a.head_scale = head_scale; a.ctx = (bf16_t*)ctx; a.lse = lse;
  a.keep_bits = keep_bits; a.ld_qkv = ld_qkv; a.ld_ctx = ld_ctx; a.B = B; a.Sq = Sq; a.Sk = Sk; a.nh = nh; a.drop = drop;
  const int rc = rect_check(a, head_size);
  if (rc != VT_OK) return rc;
  hipLaunchKernelGGL(attention_rect_fwd_d64, dim3((Sq + 31) / 32, nh, B), dim3(64), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

int vt_attention_rect_bwd_dispatch(const void* qkv, long ld_qkv, const void* dctx, long ld_d, const void* ctx, long ld_ctx,
                                   const float* mask, int mask_mode, const float* lse, void* dqkv, long ld_dqkv, int B, int Sq,
                                   int Sk, int nh, int head_size, const DropCfg& drop, const uint32_t* keep_bits,
                                   hipStream_t stream) {
  if (!qkv || !dctx || !ctx || !lse || !dqkv) return VT_ERR_NULL;
  RectArgs a = {};
  a.qkv = (const bf16_t*)qkv; a.mask = mask; a.mask_mode = mask_mode; a.ctx = (bf16_t*)const_cast<void*>(ctx);
  a.lse = const_cast<float*>(lse); a.dctx = (const bf16_t*)dctx; a.dqkv = (bf16_t*)dqkv;
  a.keep_bits = const_cast<uint32_t*>(keep_bits);
  a.ld_qkv = ld_qkv; a.ld_ctx = ld_ctx; a.ld_d = ld_d; a.ld_dqkv = ld_dqkv; a.B = B; a.Sq = Sq; a.Sk = Sk; a.nh = nh; a.drop = drop;
  const int rc = rect_check(a, head_size);
  if (rc != VT_OK) return rc;
  if ((ld_d % 8) || (ld_dqkv % 8) || ld_d < (long)nh * 64 || ld_dqkv < 3L * nh * 64) return VT_ERR_BAD_ALIGN;
  if (((uintptr_t)dctx | (uintptr_t)dqkv) & 15) return VT_ERR_BAD_ALIGN;
  hipLaunchKernelGGL(attention_rect_bwd_dkv_d64, dim3((Sk + 15) / 16, nh, B), dim3(64), 0, stream, a);
  if (hipGetLastError() != hipSuccess) return VT_ERR_HIP;
  hipLaunchKernelGGL(attention_rect_bwd_dq_d64, dim3((Sq + 15) / 16 + (Sk - Sq + 15) / 16, nh, B), dim3(64), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
