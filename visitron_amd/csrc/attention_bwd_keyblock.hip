// Attention backward, the key-block kernels: one workgroup per (head, batch, block of 256 keys), 4 waves
// (attn_bwd_body_4w) or 8 (attn_bwd_body_w8).  They serve every shape -- S > 256, the per-query bias, dropout from the
// hash -- and, as the DET instantiations, the deterministic mode's planes; attention_bwd.hip has the mathematics, the
// deterministic contract and the rule that routes a call here.
//
// gfx950 design.  One workgroup = 4 waves = one (batch, head); wave w owns keys 64w..64w+63 for the
// whole kernel: their K and V fragments live in registers (MFMA B operands) and their dK^T / dV^T
// (64 d x 64 keys each) accumulate in 128 registers, so dK and dV need no cross-wave or cross-
// workgroup sum.  The workgroup sweeps 32-query slices (Q and dO slices double-buffered in LDS by
// global_load_lds).  All score-shaped products keep the KEY on the MFMA lane (v_mfma_f32_32x32x16_bf16):
//   S[q][key]  = Q . K^T       dP[q][key] = dO . V^T        (A = LDS rows, B = registers)
// so P and dS tiles are, as they stand in the accumulators, the B operands of
//   dV^T[d][key] += dO^T . P   dK^T[d][key] += Q^T . dS     (A = ds_read_b64_tr_b16 of the slices)
// Only dS crosses LDS, once per slice, as a [4-query group][key] image that every wave then reads
// (transposed) to form dQ^T[d][q] = K^T . dS^T over ALL keys -- wave w produces d rows 16w..16w+15
// with v_mfma_f32_16x16x32_bf16 -- so dQ needs no reduction either, and for S <= 256 everything is
// bitwise reproducible (no atomics).  For S > 256 the keys are split into blocks of 256 with one
// workgroup each (grid.z); dK/dV stay private, and the dQ partials of the key blocks are combined by
// fp32 atomics into a scratch [B*S,H] slab: each slice's dQ^T is transposed through LDS so that a
// wave-instruction adds 256 contiguous bytes of one row (the full-rate atomic shape), then a small
// kernel rounds the slab to bf16.
#include "attention_bwd_common.hpp"

// LDS map (bytes)
#define AB_K 0                      // [256 keys][128 B], 32-B groups XOR ((row>>1)&1 | ((row>>3)&1)<<1)
#define AB_Q (32768)                // 2 x [32 q][128 B], chunk XOR (row>>1)&7
#define AB_DO (AB_Q + 2 * 4096)     // 2 x [32 q][128 B], same
#define AB_DS (AB_DO + 2 * 4096)    // 2 x [8 q-groups][256 keys][8 B]
#define AB_ROW (AB_DS + 2 * 16384)  // 2 x (lse[32] | delta[32]) fp32
#define AB_DQ (AB_ROW + 2 * 256)     // [32 q][64 d] fp32 staging for the atomic dQ path
#define AB_LDS_BYTES (AB_DQ + 8192)

// The kernel's body.  DET: deterministic mode (several key blocks only: plane stores instead of atomics); its kernels are
// attention_det_bwd_4w / attention_det_bwd_w8 below, the default kernels are the body with DET = false, the code as it was.
template <bool DET>
__device__ __forceinline__ void attn_bwd_body_4w(const AttnBwdArgs& a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h2 = lane >> 5;
  const int b = blockIdx.y, head = blockIdx.x;
  const int kb0 = blockIdx.z * 256;   // first key of this workgroup's key block
  const int Smax = a.S, H = a.nh * 64;
  const int S = a.seq_len ? vt_clamp_len(a.seq_len[b], a.S) : a.S;                       // this sequence's rows
  const long row0 = a.seq_start ? (long)a.seq_start[b] : (long)b * a.S;
  if (kb0 >= S) {                                                     // uniform: a key block past a short sequence
    if (DET) attn_bwd_zero_plane_rows(a.dq32 + blockIdx.z * a.dq_plane + row0 * H + head * 64, S, H);
    return;
  }
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  const bf16_t* base = a.qkv + row0 * a.ld_qkv + head * 64;
  const bf16_t* dobase = a.dctx + row0 * a.ld_d + head * 64;
  const float* lse_p = a.lse + ((long)b * a.nh + head) * Smax;
  const float* del_p = a.delta + ((long)b * a.nh + head) * Smax;
  const int nslices = (S + 31) >> 5;
  DropCfg dr = a.drop;
  dr.seed = vt_hash32(a.drop.seed, (uint32_t)(b * a.nh + head));
  const float ds_scale = a.scale * dr.scale;   // 1 / sqrt(d) times dropout's 1 / (1-p) (1 when off)
  const int kcount = (S - kb0) < 256 ? (S - kb0) : 256;
  const int nkt = (kcount + 31) >> 5;  // 32-key steps of this key block for dQ

  // ---- K tile (all keys) -> LDS for the dQ product ----
  for (int j = wave; j < nkt * 4; j += 4) {  // 8-row pieces
    const int row = 8 * j + (lane >> 3);
    int kr = (kb0 + row) < S ? (kb0 + row) : S - 1;
    const int cs = lane & 7;
    const int sw = (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1;  // 32-B group XOR, in 16-B chunk units
    glds16(base + (long)kr * a.ld_qkv + H + ((cs ^ sw) << 3), smem + AB_K + j * 1024);
  }
  // ---- slice loader: Q and dO rows q0..q0+31 (one 1-KiB piece = 8 rows; waves 0..3 take rows 8w..8w+7) ----
  // The row constants (lse | delta) are fetched BEFORE the DMA is issued (vmcnt retires in order: a
  // later register load would make the wave wait for the DMA too) and written to LDS by store_rows().
  auto load_rows = [&](int sl) -> float {
    float v = 0.f;
    if (tid < 64) {
      const int qq = sl * 32 + (tid & 31);
      if (tid < 32) v = qq < S ? lse_p[qq] : INFINITY;  // +inf => P = 0 for padded queries
      else v = qq < S ? del_p[qq] : 0.f;
    }
    return v;
  };
  auto store_rows = [&](float v, int buf) {
    if (tid < 64) ((float*)(smem + AB_ROW + buf * 256))[tid] = v;
  };
  auto load_slice = [&](int sl, int buf) {
    const int row = 8 * wave + (lane >> 3);
    int q = sl * 32 + row;
    q = q < S ? q : S - 1;
    const int c = (lane & 7) ^ ((row >> 1) & 7);
    glds16(base + (long)q * a.ld_qkv + (c << 3), smem + AB_Q + buf * 4096 + wave * 1024);
    glds16(dobase + (long)q * a.ld_d + (c << 3), smem + AB_DO + buf * 4096 + wave * 1024);
  };
  store_rows(load_rows(0), 0);
  load_slice(0, 0);

  // ---- this wave's K and V fragments (B operands; lane = key) and its key biases ----
  bf16x8 kf[2][4], vf[2][4];
  float kbias[2];
  const float* mq3[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = kb0 + 64 * wave + 32 * kt + r;
    const int kr = key < S ? key : S - 1;
    const bf16_t* kp = base + (long)kr * a.ld_qkv + H + 8 * h2;
    const bf16_t* vp = base + (long)kr * a.ld_qkv + 2 * H + 8 * h2;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      kf[kt][ds] = *(const bf16x8*)(kp + 16 * ds);
      vf[kt][ds] = *(const bf16x8*)(vp + 16 * ds);
    }
    float add = -INFINITY;
    if (key < S) {
      add = 0.f;
      if (a.mask && a.mask_additive != 2) {
        const float mval = a.mask[(long)b * Smax + key];
        add = a.mask_additive ? mval : (1.0f - mval) * -10000.0f;
      }
    }
    kbias[kt] = add;
    // mask_additive == 2: an additive bias per (query, key) [B, S, S] (the reference's 3-D attention masks,
    // encoder.py:228-229): this lane's key column; the query row is added per element below
    mq3[kt] = (a.mask && a.mask_additive == 2) ? a.mask + (long)b * Smax * Smax + kr : nullptr;
  }

  f32x16 dv[2][2], dk[2][2];  // [d-tile][key-tile]: lane = key, reg <-> d = 32dt + 16h2 + reg
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) { dv[i][j][e] = 0.f; dk[i][j][e] = 0.f; }

  // lane-constant addressing
  const int a_row = r * 128;                                  // Q / dO row read (A operand of S, dP)
  const int a_swz = (r >> 1) & 7;
  const int i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3, dhalf = (lane >> 4) & 1, g = lane >> 4;
  // transposed slice reads (A operand of dV^T / dK^T): rows q = 16*s2 + 4*h2 + q4 (+8), cols d-perm
  const int t_row = 4 * h2 + q4;
  const int t_col = 2 * (16 * (p4 & 1) + 8 * dhalf + 4 * (p4 >> 1));  // + 64*dt, within the 128-B row
  // slices use the 16-B chunk swizzle (row>>1)&7: as a byte XOR on bits 4..6
  const int t_sw0 = (((t_row) >> 1) & 7) << 4;          // rows 4h2+q4        (s2 = 0)
  const int t_sw1 = (((t_row + 8) >> 1) & 7) << 4;      // rows +8
  const int t_sw2 = (((t_row + 16) >> 1) & 7) << 4;     // s2 = 1
  const int t_sw3 = (((t_row + 24) >> 1) & 7) << 4;

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int sl = 0; sl < nslices; ++sl) {
    const int buf = sl & 1;

    const char* sQ = smem + AB_Q + buf * 4096;
    const char* sDO = smem + AB_DO + buf * 4096;
    const float* rowv = (const float*)(smem + AB_ROW + buf * 256);
    char* sDS = smem + AB_DS + buf * 16384;

    // A fragments of this slice: Q and dO rows (lane (r, h2): row r, d = 16ds + 8h2 ..)
    bf16x8 qa[4], da[4];
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      qa[ds] = *(const bf16x8*)(sQ + a_row + (((2 * ds + h2) ^ a_swz) << 4));
      da[ds] = *(const bf16x8*)(sDO + a_row + (((2 * ds + h2) ^ a_swz) << 4));
    }
    // per-register row constants: q = (reg&3) + 8(reg>>2) + 4h2
    f32x4 lse4[4], del4[4];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      lse4[g4] = *(const f32x4*)(rowv + 8 * g4 + 4 * h2);
      del4[g4] = *(const f32x4*)(rowv + 32 + 8 * g4 + 4 * h2);
    }
    // transposed A operands of the slice: [s2][dt] for dO^T (dV) and Q^T (dK)
    bf16x8 doT[2][2], qT[2][2];
    {
      const unsigned bq = lds0 + AB_Q + buf * 4096 + t_row * 128;
      const unsigned bd = lds0 + AB_DO + buf * 4096 + t_row * 128;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int cb = t_col + 64 * dt;
        // rows +8 => +1024 bytes, but the swizzle differs between the two blocks: two explicit reads
        short4v q0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bq + (cb ^ t_sw0)));
        short4v q1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bq + 1024 + (cb ^ t_sw1)));
        short4v q2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bq + 2048 + (cb ^ t_sw2)));
        short4v q3 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bq + 3072 + (cb ^ t_sw3)));
        qT[0][dt] = __builtin_bit_cast(bf16x8, (short8v){q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]});
        qT[1][dt] = __builtin_bit_cast(bf16x8, (short8v){q2[0], q2[1], q2[2], q2[3], q3[0], q3[1], q3[2], q3[3]});
        short4v d0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bd + (cb ^ t_sw0)));
        short4v d1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bd + 1024 + (cb ^ t_sw1)));
        short4v d2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bd + 2048 + (cb ^ t_sw2)));
        short4v d3 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bd + 3072 + (cb ^ t_sw3)));
        doT[0][dt] = __builtin_bit_cast(bf16x8, (short8v){d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]});
        doT[1][dt] = __builtin_bit_cast(bf16x8, (short8v){d2[0], d2[1], d2[2], d2[3], d3[0], d3[1], d3[2], d3[3]});
      }
    }

    // prefetch the next slice now that this slice's operands are in registers (issuing the DMA before
    // those LDS reads would make hipcc wait for it first); buffer buf^1 was last read in slice sl-1,
    // which every wave left through the barrier below
    float next_rowv = 0.f;
    if (sl + 1 < nslices) {
      next_rowv = load_rows(sl + 1);
      load_slice(sl + 1, buf ^ 1);
    }

#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      // S = Q K^T and dP = dO V^T for keys 64w + 32kt .. +31 (lane = key)
      f32x16 sacc, dpacc;
#pragma unroll
      for (int e = 0; e < 16; ++e) { sacc[e] = 0.f; dpacc[e] = 0.f; }
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) {
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[ds], kf[kt][ds], sacc, 0, 0, 0);
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da[ds], vf[kt][ds], dpacc, 0, 0, 0);
      }
      // P = exp(s/8 + mask - lse);  dS = P (dP - delta) / 8
      f32x16 pacc;
      bool keep[16];
      if (dr.thresh) attn_bwd_keep16(dr, (uint32_t)(sl * 32 + 4 * h2), (uint32_t)(kb0 + 64 * wave + 32 * kt + r), (uint32_t)(S + 3) & ~3u, keep);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g4 + e;
          float s = fmaf(sacc[i], a.scale, kbias[kt]);
          if (mq3[kt]) {   // per-query bias row of element i's query (clamped: rows past S carry dO = 0)
            const int qi = sl * 32 + (i & 3) + 8 * (i >> 2) + 4 * h2;
            s += mq3[kt][(long)(qi < S ? qi : S - 1) * Smax];
          }
          const float p = __builtin_amdgcn_exp2f((s - lse4[g4][e]) * LOG2E);
          float dpv = dpacc[i], pv = p;
          if (dr.thresh) {  // O = (P * mask / (1-p)) V: dP and the P that feeds dV carry the mask, dS keeps P
            dpv = keep[i] ? dpv : 0.f;
            pv = keep[i] ? p : 0.f;
          }
          // dropout's uniform 1 / (1-p) is not applied per element: dV takes it once at the end, and in
          // dS = P (mask dP / (1-p) - delta) / 8 it moves outside the bracket: ds_scale = 1 / (8 (1-p)), the row constant arrives
          // as delta (1-p) (attn_delta_rows)
          pacc[i] = pv;
          sacc[i] = p * (dpv - del4[g4][e]) * ds_scale;  // dS' (scales folded in)
        }
      // dV^T += dO^T P ; dK^T += Q^T dS'   (k = q, 2 steps of 16)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pb = pack8(pacc, s2);
        const bf16x8 sb = pack8(sacc, s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(doT[s2][dt], pb, dv[dt][kt], 0, 0, 0);
          dk[dt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qT[s2][dt], sb, dk[dt][kt], 0, 0, 0);
        }
      }
      // dS' -> LDS image [q-group G][key][4 q] (8 B per (G,key)), key index XOR-swizzled by G
      {
        const int key = 64 * wave + 32 * kt + r;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int G = 2 * g4 + h2;
          const int kx = key ^ (((G >> 1) & 1) << 2) ^ ((G & 1) << 4);
          u32x2 w;
          w[0] = pack_bf16x2(sacc[4 * g4 + 0], sacc[4 * g4 + 1]);
          w[1] = pack_bf16x2(sacc[4 * g4 + 2], sacc[4 * g4 + 3]);
          *(u32x2*)(sDS + (G * 256 + kx) * 8) = w;
        }
      }
    }

    if (sl + 1 < nslices) store_rows(next_rowv, buf ^ 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // next slice's DMA (issued above) has landed
    __syncthreads();                                   // ... and every wave's dS' is in the image

    // ---- dQ^T[d][q] = sum_key K^T[d][key] dS'^T[key][q]; wave w: d = 16w .. 16w+15, both 16-q tiles ----
    f32x4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = {0.f, 0.f, 0.f, 0.f};
    {
      const unsigned kbase = lds0 + AB_K;
      const unsigned dsb = lds0 + AB_DS + buf * 16384;
      for (int ks = 0; ks < nkt; ++ks) {
        const int krow = 32 * ks + 8 * g + q4;  // first block row; second block = +4
        const int ksw = ((((krow >> 1) & 1) | (((krow >> 3) & 1) << 1)) << 5);
        const int ksw2 = (((((krow + 4) >> 1) & 1) | ((((krow + 4) >> 3) & 1) << 1)) << 5);
        const int kcol = 2 * (16 * wave) + 8 * p4;
        short4v k0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(kbase + krow * 128 + (kcol ^ ksw)));
        short4v k1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(kbase + (krow + 4) * 128 + (kcol ^ ksw2)));
        const bf16x8 ka = __builtin_bit_cast(bf16x8, (short8v){k0[0], k0[1], k0[2], k0[3], k1[0], k1[1], k1[2], k1[3]});
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          const int G = 4 * qt + p4;
          const int gsw = (((G >> 1) & 1) << 2) ^ ((G & 1) << 4);
          short4v s0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(dsb + (G * 256 + (krow ^ gsw)) * 8));
          short4v s1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(dsb + (G * 256 + ((krow + 4) ^ gsw)) * 8));
          const bf16x8 sbq = __builtin_bit_cast(bf16x8, (short8v){s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]});
          if (qt == 0) dq0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, sbq, dq0, 0, 0, 0);
          else dq1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, sbq, dq1, 0, 0, 0);
        }
      }
    }
    // store dQ: lane (q_local = lane&15, g): d = 16w + 4g .. +3
    if (a.dq32 == nullptr) {
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int q = sl * 32 + 16 * qt + (lane & 15);
        if (q < S) {
          const f32x4 v = qt == 0 ? dq0 : dq1;
          u32x2 w;
          w[0] = pack_bf16x2(v[0], v[1]);
          w[1] = pack_bf16x2(v[2], v[3]);
          *(u32x2*)(a.dqkv + (row0 + q) * a.ld_dqkv + head * 64 + 16 * wave + 4 * g) = w;
        }
      }
    } else {
      // several key blocks: transpose the slice's dQ^T through LDS, then add whole 256-byte row
      // segments atomically (lane = d) -- the atomic shape that runs at the full chip-wide rate
      float* st = (float*)(smem + AB_DQ);
      *(f32x4*)(st + (lane & 15) * 64 + 16 * wave + 4 * g) = dq0;
      *(f32x4*)(st + (16 + (lane & 15)) * 64 + 16 * wave + 4 * g) = dq1;
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const int ql = 8 * wave + rr;
        const int q = sl * 32 + ql;
        if (q < S) {
          float* dst = a.dq32 + (row0 + q) * H + head * 64 + lane;
          if (DET) dst[blockIdx.z * a.dq_plane] = st[ql * 64 + lane];   // deterministic mode: plane kb, plain store
          else atomicAdd(dst, st[ql * 64 + lane]);
        }
      }
      // the staging tile is rewritten only after the next slice's barrier, which every wave reaches
      // after these reads
    }
    // no barrier needed here: the next slice writes the OTHER dS image / reads the other Q,dO buffers,
    // and the barrier inside the next slice orders this slice's dQ reads before the image is reused.
  }

  // ---- dK, dV of this wave's keys: lane = key, reg <-> d = 32dt + 16h2 + reg ----
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = kb0 + 64 * wave + 32 * kt + r;
    if (key >= S) continue;
    bf16_t* orow = a.dqkv + (row0 + key) * a.ld_dqkv + head * 64 + 16 * h2;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      u32x4 k0, k1, v0, v1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        k0[i] = pack_bf16x2(dk[dt][kt][2 * i], dk[dt][kt][2 * i + 1]);
        k1[i] = pack_bf16x2(dk[dt][kt][8 + 2 * i], dk[dt][kt][8 + 2 * i + 1]);
        v0[i] = pack_bf16x2(dv[dt][kt][2 * i] * dr.scale, dv[dt][kt][2 * i + 1] * dr.scale);
        v1[i] = pack_bf16x2(dv[dt][kt][8 + 2 * i] * dr.scale, dv[dt][kt][8 + 2 * i + 1] * dr.scale);
      }
      ((u32x4*)(orow + H + 32 * dt))[0] = k0;
      ((u32x4*)(orow + H + 32 * dt))[1] = k1;
      ((u32x4*)(orow + 2 * H + 32 * dt))[0] = v0;
      ((u32x4*)(orow + 2 * H + 32 * dt))[1] = v1;
    }
  }
}

// 8-wave form: wave w owns keys 32w..32w+31 (one key tile), <= 256 VGPRs, two waves per SIMD.
// BITS: the dropout keep flags come from the words the forward wrote (one 4-byte load per lane and slice, one bit-field
// extract and two ands per element) instead of the hash (about ten vector instructions per element, a third of the loop)
// DELTA: the row constant delta = rowsum(dO o O) (x (1-p) under dropout) is formed here, a slice ahead, from 8 bytes of dO
// and of O per thread (16 threads per query), instead of by a separate pass over both tensors (attn_delta_rows)
__global__ __launch_bounds__(256, 1) void attention_bwd_d64(AttnBwdArgs a) { attn_bwd_body_4w<false>(a); }
__global__ __launch_bounds__(256, 1) void attention_det_bwd_4w(AttnBwdArgs a) { attn_bwd_body_4w<true>(a); }

// DET: deterministic mode, as in attn_bwd_body_4w
template <bool BITS, bool DELTA, bool DET>
__device__ __forceinline__ void attn_bwd_body_w8(const AttnBwdArgs& a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h2 = lane >> 5;
  const int b = blockIdx.y, head = blockIdx.x;
  const int kb0 = blockIdx.z * 256;   // first key of this workgroup's key block
  const int Smax = a.S, H = a.nh * 64;
  const int S = a.seq_len ? vt_clamp_len(a.seq_len[b], a.S) : a.S;                       // this sequence's rows
  const long row0 = a.seq_start ? (long)a.seq_start[b] : (long)b * a.S;
  if (kb0 >= S) {                                                     // uniform: a key block past a short sequence
    if (DET) attn_bwd_zero_plane_rows(a.dq32 + blockIdx.z * a.dq_plane + row0 * H + head * 64, S, H);
    return;
  }
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  const bf16_t* base = a.qkv + row0 * a.ld_qkv + head * 64;
  const bf16_t* dobase = a.dctx + row0 * a.ld_d + head * 64;
  const float* lse_p = a.lse + ((long)b * a.nh + head) * Smax;
  const float* del_p = a.delta + ((long)b * a.nh + head) * Smax;
  const int nslices = (S + 31) >> 5;
  DropCfg dr = a.drop;
  dr.seed = vt_hash32(a.drop.seed, (uint32_t)(b * a.nh + head));
  const float ds_scale = a.scale * dr.scale;   // 1 / sqrt(d) times dropout's 1 / (1-p) (1 when off): applied to dK once at the
                                               // end and to each slice's four dQ values, not to every dS element
  const int kcount = (S - kb0) < 256 ? (S - kb0) : 256;
  const int nkt = (kcount + 31) >> 5;  // 32-key steps of this key block for dQ

  // ---- K tile (all keys) -> LDS for the dQ product ----
  for (int j = wave; j < nkt * 4; j += 8) {  // 8-row pieces
    const int row = 8 * j + (lane >> 3);
    int kr = (kb0 + row) < S ? (kb0 + row) : S - 1;
    const int cs = lane & 7;
    const int sw = (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1;  // 32-B group XOR, in 16-B chunk units
    glds16(base + (long)kr * a.ld_qkv + H + ((cs ^ sw) << 3), smem + AB_K + j * 1024);
  }
  // ---- slice loader: Q and dO rows q0..q0+31 (one 1-KiB piece = 8 rows; waves 0..3 take rows 8w..8w+7) ----
  // The row constants (lse | delta) are fetched BEFORE the DMA is issued (vmcnt retires in order: a
  // later register load would make the wave wait for the DMA too) and written to LDS by store_rows().
  auto load_rows = [&](int sl) -> float {
    float v = 0.f;
    if (tid < 64) {
      const int qq = sl * 32 + (tid & 31);
      if (tid < 32) v = qq < S ? lse_p[qq] : INFINITY;  // +inf => P = 0 for padded queries
      else if (!DELTA) v = qq < S ? del_p[qq] : 0.f;
    }
    return v;
  };
  auto store_rows = [&](float v, int buf) {
    if (tid < (DELTA ? 32 : 64)) ((float*)(smem + AB_ROW + buf * 256))[tid] = v;
  };
  // DELTA: thread t = (query t >> 4 of the slice, 4 head columns 4 (t & 15)): its 8 bytes of dO and of O
  const bf16_t* obase = DELTA ? a.ctx + row0 * a.ld_ctx + head * 64 + 4 * (tid & 15) : nullptr;
  auto load_do_o = [&](int sl, u32x2& xd, u32x2& xo) {
    int q = sl * 32 + (tid >> 4);
    q = q < S ? q : S - 1;
    xd = *(const u32x2*)(dobase + (long)q * a.ld_d + 4 * (tid & 15));
    xo = *(const u32x2*)(obase + (long)q * a.ld_ctx);
  };
  auto store_delta = [&](u32x2 xd, u32x2 xo, int buf) {
    float v = bf16lo(xd[0]) * bf16lo(xo[0]) + bf16hi(xd[0]) * bf16hi(xo[0]) + bf16lo(xd[1]) * bf16lo(xo[1]) + bf16hi(xd[1]) * bf16hi(xo[1]);
    // sum over the 16 lanes of a query (one DPP row): xor 1, xor 2, mirror within 8, mirror within 16
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true));
    if ((tid & 15) == 0) ((float*)(smem + AB_ROW + buf * 256))[32 + (tid >> 4)] = v * a.delta_mul;
  };
  auto load_slice = [&](int sl, int buf) {
    const int pw = wave & 3;
    const int row = 8 * pw + (lane >> 3);
    int q = sl * 32 + row;
    q = q < S ? q : S - 1;
    const int c = (lane & 7) ^ ((row >> 1) & 7);
    if (wave < 4) glds16(base + (long)q * a.ld_qkv + (c << 3), smem + AB_Q + buf * 4096 + pw * 1024);
    else glds16(dobase + (long)q * a.ld_d + (c << 3), smem + AB_DO + buf * 4096 + pw * 1024);
  };
  // the keep words of this lane's key: one per 32-query slice, fetched a slice ahead like the row constants
  const uint32_t* keep_p = nullptr;
  if (BITS) {
    const long nqb = (Smax + 31) >> 5, kpitch = nqb << 5;
    const long key = kb0 + 32 * wave + r;
    keep_p = a.keep_bits + ((long)b * a.nh + head) * nqb * kpitch + (key < kpitch ? key : kpitch - 1);
  }
  const long keep_step = (long)((Smax + 31) >> 5) << 5;
  uint32_t kw_next = BITS ? keep_p[0] : 0u;
  u32x2 nd = {0u, 0u}, no = {0u, 0u};
  if (DELTA) { load_do_o(0, nd, no); store_delta(nd, no, 0); }
  store_rows(load_rows(0), 0);
  load_slice(0, 0);

  // ---- this wave's K and V fragments (B operands; lane = key) and its key biases ----
  bf16x8 kf[1][4], vf[1][4];
  float kbias[1];
  const float* mq3[1];
#pragma unroll
  for (int kt = 0; kt < 1; ++kt) {
    const int key = kb0 + 32 * wave + r;
    const int kr = key < S ? key : S - 1;
    const bf16_t* kp = base + (long)kr * a.ld_qkv + H + 8 * h2;
    const bf16_t* vp = base + (long)kr * a.ld_qkv + 2 * H + 8 * h2;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      kf[kt][ds] = *(const bf16x8*)(kp + 16 * ds);
      vf[kt][ds] = *(const bf16x8*)(vp + 16 * ds);
    }
    float add = -INFINITY;
    if (key < S) {
      add = 0.f;
      if (a.mask && a.mask_additive != 2) {
        const float mval = a.mask[(long)b * Smax + key];
        add = a.mask_additive ? mval : (1.0f - mval) * -10000.0f;
      }
    }
    kbias[kt] = add;
    // mask_additive == 2: an additive bias per (query, key) [B, S, S] (the reference's 3-D attention masks,
    // encoder.py:228-229): this lane's key column; the query row is added per element below
    mq3[kt] = (a.mask && a.mask_additive == 2) ? a.mask + (long)b * Smax * Smax + kr : nullptr;
  }

  f32x16 dv[2][1], dk[2][1];  // [d-tile][key-tile]: lane = key, reg <-> d = 32dt + 16h2 + reg
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 1; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) { dv[i][j][e] = 0.f; dk[i][j][e] = 0.f; }

  // lane-constant addressing
  const int a_row = r * 128;                                  // Q / dO row read (A operand of S, dP)
  const int a_swz = (r >> 1) & 7;
  const int i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3, dhalf = (lane >> 4) & 1, g = lane >> 4;
  // transposed slice reads (A operand of dV^T / dK^T): rows q = 16*s2 + 4*h2 + q4 (+8), cols d-perm
  const int t_row = 4 * h2 + q4;
  const int t_col = 2 * (16 * (p4 & 1) + 8 * dhalf + 4 * (p4 >> 1));  // + 64*dt, within the 128-B row
  // slices use the 16-B chunk swizzle (row>>1)&7: as a byte XOR on bits 4..6
  const int t_sw0 = (((t_row) >> 1) & 7) << 4;          // rows 4h2+q4        (s2 = 0)
  const int t_sw1 = (((t_row + 8) >> 1) & 7) << 4;      // rows +8
  const int t_sw2 = (((t_row + 16) >> 1) & 7) << 4;     // s2 = 1
  const int t_sw3 = (((t_row + 24) >> 1) & 7) << 4;

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int sl = 0; sl < nslices; ++sl) {
    const int buf = sl & 1;

    const char* sQ = smem + AB_Q + buf * 4096;
    const char* sDO = smem + AB_DO + buf * 4096;
    const float* rowv = (const float*)(smem + AB_ROW + buf * 256);
    char* sDS = smem + AB_DS + buf * 16384;

    // A fragments of this slice: Q and dO rows (lane (r, h2): row r, d = 16ds + 8h2 ..)
    bf16x8 qa[4], da[4];
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      qa[ds] = *(const bf16x8*)(sQ + a_row + (((2 * ds + h2) ^ a_swz) << 4));
      da[ds] = *(const bf16x8*)(sDO + a_row + (((2 * ds + h2) ^ a_swz) << 4));
    }
    // per-register row constants (q = (reg&3) + 8(reg>>2) + 4h2) are read from LDS where they are used:
    // holding them across the MFMA chains costs 32 registers this kernel does not have
    // transposed A operands of the slice: [s2][dt] for dO^T (dV) and Q^T (dK)
    bf16x8 doT[2][2], qT[2][2];
    {
      const unsigned bq = lds0 + AB_Q + buf * 4096 + t_row * 128;
      const unsigned bd = lds0 + AB_DO + buf * 4096 + t_row * 128;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int cb = t_col + 64 * dt;
        // rows +8 => +1024 bytes, but the swizzle differs between the two blocks: two explicit reads
        short4v q0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bq + (cb ^ t_sw0)));
        short4v q1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bq + 1024 + (cb ^ t_sw1)));
        short4v q2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bq + 2048 + (cb ^ t_sw2)));
        short4v q3 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bq + 3072 + (cb ^ t_sw3)));
        qT[0][dt] = __builtin_bit_cast(bf16x8, (short8v){q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]});
        qT[1][dt] = __builtin_bit_cast(bf16x8, (short8v){q2[0], q2[1], q2[2], q2[3], q3[0], q3[1], q3[2], q3[3]});
        short4v d0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bd + (cb ^ t_sw0)));
        short4v d1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bd + 1024 + (cb ^ t_sw1)));
        short4v d2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bd + 2048 + (cb ^ t_sw2)));
        short4v d3 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(bd + 3072 + (cb ^ t_sw3)));
        doT[0][dt] = __builtin_bit_cast(bf16x8, (short8v){d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]});
        doT[1][dt] = __builtin_bit_cast(bf16x8, (short8v){d2[0], d2[1], d2[2], d2[3], d3[0], d3[1], d3[2], d3[3]});
      }
    }

    // prefetch the next slice now that this slice's operands are in registers (issuing the DMA before
    // those LDS reads would make hipcc wait for it first); buffer buf^1 was last read in slice sl-1,
    // which every wave left through the barrier below
    float next_rowv = 0.f;
    const uint32_t kw_cur = kw_next >> (4 * h2);   // bit (i&3) + 8(i>>2) = element i's query
    if (sl + 1 < nslices) {
      next_rowv = load_rows(sl + 1);
      if (DELTA) load_do_o(sl + 1, nd, no);
      if (BITS) kw_next = keep_p[(long)(sl + 1) * keep_step];
      load_slice(sl + 1, buf ^ 1);
    }

#pragma unroll
    for (int kt = 0; kt < 1; ++kt) {
      // S = Q K^T and dP = dO V^T for keys 32w .. 32w+31 (lane = key)
      f32x16 sacc, dpacc;
#pragma unroll
      for (int e = 0; e < 16; ++e) { sacc[e] = 0.f; dpacc[e] = 0.f; }
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) {
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[ds], kf[kt][ds], sacc, 0, 0, 0);
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da[ds], vf[kt][ds], dpacc, 0, 0, 0);
      }
      // P = exp(s/8 + mask - lse);  dS = P (dP - delta) / 8
      f32x16 pacc;
      // hash path (no keep words): the flags of a group of four queries are derived right before their use -- sixteen flags
      // held across the tile cost three spilled registers at this kernel's 128-register budget
      uint32_t hx0 = 0, hstep = 0, hsh = 0, hmask = 0xffu, hth = dr.thresh;
      if (!BITS && dr.thresh) {
        const bool wide = vt_attn_wide(dr);   // exact-p mode: 16-bit fields, two keys per word
        const uint32_t lg = wide ? 1u : 2u;
        const uint32_t Sp4 = ((uint32_t)(S + 3) & ~3u) >> lg, key = (uint32_t)(kb0 + 32 * wave + r);
        hsh = wide ? 16u * (key & 1u) : 8u * (key & 3u);
        hmask = wide ? 0xffffu : 0xffu;
        hth = wide ? dr.thresh >> 16 : dr.thresh;
        hstep = Sp4 * VT_HASH_C1;
        hx0 = vt_hash_pre(dr.seed, (uint32_t)(sl * 32 + 4 * h2) * Sp4 + (key >> lg));
      }
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 lse4_g = *(const f32x4*)(rowv + 8 * g4 + 4 * h2);
        const f32x4 del4_g = *(const f32x4*)(rowv + 32 + 8 * g4 + 4 * h2);
        bool keep[16];
        if (!BITS && dr.thresh) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            keep[4 * g4 + e] = ((vt_hash_fin(hx0 + (uint32_t)(e + 8 * g4) * hstep) >> hsh) & hmask) >= hth;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g4 + e;
          float s = fmaf(sacc[i], a.scale, kbias[kt]);
          if (mq3[kt]) {   // per-query bias row of element i's query (clamped: rows past S carry dO = 0)
            const int qi = sl * 32 + (i & 3) + 8 * (i >> 2) + 4 * h2;
            s += mq3[kt][(long)(qi < S ? qi : S - 1) * Smax];
          }
          const float p = __builtin_amdgcn_exp2f((s - lse4_g[e]) * LOG2E);
          float dpv = dpacc[i], pv = p;
          if (BITS) {   // (launched only with dropout on)
            const int km = __builtin_amdgcn_sbfe((int)kw_cur, (i & 3) + 8 * (i >> 2), 1);   // 0 / -1
            dpv = __int_as_float(__float_as_int(dpv) & km);
            pv = __int_as_float(__float_as_int(p) & km);
          } else if (dr.thresh) {  // O = (P * mask / (1-p)) V: dP and the P that feeds dV carry the mask, dS keeps P
            dpv = keep[i] ? dpv : 0.f;
            pv = keep[i] ? p : 0.f;
          }
          // dropout's uniform 1 / (1-p) is not applied per element: dV takes it once at the end, and in
          // dS = P (mask dP / (1-p) - delta) / 8 it moves outside the bracket: ds_scale = 1 / (8 (1-p)), the row constant arrives
          // as delta (1-p) (attn_delta_rows); ds_scale itself multiplies the dK accumulators at the end and dQ per slice
          // (348 -> 337 us per launch at B = 256; measured on the same box and NOT taken: log2(e) folded into scale / bias / lse
          // -- 16 multiplies fewer, 364-374 us, as in round 2 --, dS as fma(P o M, dP, -P delta) 340-349 us, the previous
          // slice's dQ product issued under this slice's element-wise work 384 us at 256 registers)
          pacc[i] = pv;
          sacc[i] = p * (dpv - del4_g[e]);   // dS' up to ds_scale
        }
      }
      // dV^T += dO^T P ; dK^T += Q^T dS'   (k = q, 2 steps of 16)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pb = pack8(pacc, s2);
        const bf16x8 sb = pack8(sacc, s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(doT[s2][dt], pb, dv[dt][kt], 0, 0, 0);
          dk[dt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qT[s2][dt], sb, dk[dt][kt], 0, 0, 0);
        }
      }
      // dS' -> LDS image [q-group G][key][4 q] (8 B per (G,key)), key index XOR-swizzled by G
      {
        const int key = 32 * wave + r;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int G = 2 * g4 + h2;
          const int kx = key ^ (((G >> 1) & 1) << 2) ^ ((G & 1) << 4);
          u32x2 w;
          w[0] = pack_bf16x2(sacc[4 * g4 + 0], sacc[4 * g4 + 1]);
          w[1] = pack_bf16x2(sacc[4 * g4 + 2], sacc[4 * g4 + 3]);
          *(u32x2*)(sDS + (G * 256 + kx) * 8) = w;
        }
      }
    }

    if (sl + 1 < nslices) {
      store_rows(next_rowv, buf ^ 1);
      if (DELTA) store_delta(nd, no, buf ^ 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // next slice's DMA (issued above) has landed
    __syncthreads();                                   // ... and every wave's dS' is in the image

    // ---- dQ^T[d][q] = sum_key K^T[d][key] dS'^T[key][q]; wave w: d = 16w .. 16w+15, both 16-q tiles ----
    f32x4 dq0 = {0.f, 0.f, 0.f, 0.f};
    const int dqd = wave >> 1, dqq = wave & 1;   // this wave's 16(d) x 16(q) tile of dQ^T
    {
      const unsigned kbase = lds0 + AB_K;
      const unsigned dsb = lds0 + AB_DS + buf * 16384;
      for (int ks = 0; ks < nkt; ++ks) {
        const int krow = 32 * ks + 8 * g + q4;  // first block row; second block = +4
        const int ksw = ((((krow >> 1) & 1) | (((krow >> 3) & 1) << 1)) << 5);
        const int ksw2 = (((((krow + 4) >> 1) & 1) | ((((krow + 4) >> 3) & 1) << 1)) << 5);
        const int kcol = 2 * (16 * dqd) + 8 * p4;
        short4v k0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(kbase + krow * 128 + (kcol ^ ksw)));
        short4v k1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(kbase + (krow + 4) * 128 + (kcol ^ ksw2)));
        const bf16x8 ka = __builtin_bit_cast(bf16x8, (short8v){k0[0], k0[1], k0[2], k0[3], k1[0], k1[1], k1[2], k1[3]});
        {
          const int qt = dqq;
          const int G = 4 * qt + p4;
          const int gsw = (((G >> 1) & 1) << 2) ^ ((G & 1) << 4);
          short4v s0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(dsb + (G * 256 + (krow ^ gsw)) * 8));
          short4v s1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(dsb + (G * 256 + ((krow + 4) ^ gsw)) * 8));
          const bf16x8 sbq = __builtin_bit_cast(bf16x8, (short8v){s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]});
          dq0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, sbq, dq0, 0, 0, 0);
        }
      }
    }
    // store dQ: lane (q_local = lane&15, g): d = 16w + 4g .. +3
    dq0 *= ds_scale;
    if (a.dq32 == nullptr) {
      const int q = sl * 32 + 16 * dqq + (lane & 15);
      if (q < S) {
        u32x2 w;
        w[0] = pack_bf16x2(dq0[0], dq0[1]);
        w[1] = pack_bf16x2(dq0[2], dq0[3]);
        *(u32x2*)(a.dqkv + (row0 + q) * a.ld_dqkv + head * 64 + 16 * dqd + 4 * g) = w;
      }
    } else {
      // several key blocks: transpose the slice's dQ^T through LDS, then add whole 256-byte row
      // segments atomically (lane = d) -- the atomic shape that runs at the full chip-wide rate
      float* st = (float*)(smem + AB_DQ);
      *(f32x4*)(st + (16 * dqq + (lane & 15)) * 64 + 16 * dqd + 4 * g) = dq0;
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int ql = 4 * wave + rr;
        const int q = sl * 32 + ql;
        if (q < S) {
          float* dst = a.dq32 + (row0 + q) * H + head * 64 + lane;
          if (DET) dst[blockIdx.z * a.dq_plane] = st[ql * 64 + lane];   // deterministic mode: plane kb, plain store
          else atomicAdd(dst, st[ql * 64 + lane]);
        }
      }
      // the staging tile is rewritten only after the next slice's barrier, which every wave reaches
      // after these reads
    }
    // no barrier needed here: the next slice writes the OTHER dS image / reads the other Q,dO buffers,
    // and the barrier inside the next slice orders this slice's dQ reads before the image is reused.
  }

  // ---- dK, dV of this wave's keys: lane = key, reg <-> d = 32dt + 16h2 + reg ----
#pragma unroll
  for (int kt = 0; kt < 1; ++kt) {
    const int key = kb0 + 32 * wave + r;
    if (key >= S) continue;
    bf16_t* orow = a.dqkv + (row0 + key) * a.ld_dqkv + head * 64 + 16 * h2;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      u32x4 k0, k1, v0, v1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        k0[i] = pack_bf16x2(dk[dt][kt][2 * i] * ds_scale, dk[dt][kt][2 * i + 1] * ds_scale);
        k1[i] = pack_bf16x2(dk[dt][kt][8 + 2 * i] * ds_scale, dk[dt][kt][8 + 2 * i + 1] * ds_scale);
        v0[i] = pack_bf16x2(dv[dt][kt][2 * i] * dr.scale, dv[dt][kt][2 * i + 1] * dr.scale);
        v1[i] = pack_bf16x2(dv[dt][kt][8 + 2 * i] * dr.scale, dv[dt][kt][8 + 2 * i + 1] * dr.scale);
      }
      ((u32x4*)(orow + H + 32 * dt))[0] = k0;
      ((u32x4*)(orow + H + 32 * dt))[1] = k1;
      ((u32x4*)(orow + 2 * H + 32 * dt))[0] = v0;
      ((u32x4*)(orow + 2 * H + 32 * dt))[1] = v1;
    }
  }
}

template <bool BITS, bool DELTA>
__global__ __launch_bounds__(512, 2) void attention_bwd_d64_w8(AttnBwdArgs a) { attn_bwd_body_w8<BITS, DELTA, false>(a); }
template <bool BITS, bool DELTA>
__global__ __launch_bounds__(512, 2) void attention_det_bwd_w8(AttnBwdArgs a) { attn_bwd_body_w8<BITS, DELTA, true>(a); }

// The kernels by what selects them, beside each the flag of its LDS attribute (set for the kernel about to be launched):
// the 8-wave family [det][bits][delta] (plane stores of the deterministic mode, keep words, delta formed in the kernel) and
// the 4-wave pair [det]
static AttnBwdKernel g_attn_bwd_w4[2] = {{attention_bwd_d64}, {attention_det_bwd_4w}};
static AttnBwdKernel g_attn_bwd_w8[2][2][2] = {
    {{{attention_bwd_d64_w8<false, false>}, {attention_bwd_d64_w8<false, true>}},
     {{attention_bwd_d64_w8<true, false>}, {attention_bwd_d64_w8<true, true>}}},
    {{{attention_det_bwd_w8<false, false>}, {attention_det_bwd_w8<false, true>}},
     {{attention_det_bwd_w8<true, false>}, {attention_det_bwd_w8<true, true>}}}};

int vt_attn_bwd_keyblock_launch(const AttnBwdArgs& a, bool eight_waves, bool det, bool bits, bool delta, hipStream_t stream) {
  AttnBwdKernel* k = eight_waves ? &g_attn_bwd_w8[det][bits][delta] : &g_attn_bwd_w4[det];
  if (!k->lds.set((const void*)k->fn, AB_LDS_BYTES)) return VT_ERR_HIP;
  hipLaunchKernelGGL(k->fn, dim3(a.nh, a.B, (a.S + 255) / 256), dim3(eight_waves ? 512 : 256), AB_LDS_BYTES, stream, a);
  return VT_OK;
}
