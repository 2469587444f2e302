// Pretraining's region rows gathered from a device region store: what PretrainDataset._extract_img_features and the tail of
// _preprocess_item do per item on the host (tasks/viewpoint_select/data_loader_pretrain.py:615-634, 654-712), for a whole
// batch in one launch.  Pure byte movers, shaped as observations.hip: one wave per output row, four rows per workgroup, and
// the four rows of a workgroup belong to one item.
//
// The store is [N, 36, P, ld] with ld = round_up(D, 8), fp32 or bf16, and counts [N, 36] says how many of a view's P rows
// exist.  Item b's regions are the rows of views 0..35 in order; their row map needs the running sum of the item's 36 counts,
// which wave 0 of every workgroup forms by a wave scan and leaves in LDS for the other three.  Output row r is region
// start + r, start = max(n - R, 0) (the LAST R rows are kept); its view is the number of running sums <= start + r.
//
// The packed row is bf16 [features D | location 128 | zeros to kpad], kpad % 8 == 0, written in 16-byte pieces of 8 columns.
// Pieces 0 .. D/8 - 1 lie inside the feature row, whose store row starts 16-byte aligned in both dtypes: a lane loads one
// 16-byte piece (bf16 store: the bits as they are) or two (fp32 store: rounded once, as pack_concat_bf16 rounds), up to 8
// rounds of them before the first store.  Every piece from D/8 on -- the one that straddles the seam (column 2054 = 8 * 256
// + 6), the location pieces (shifted against the fp32 table by D % 8 floats) and the zero tail, 25 pieces at the shipped
// width -- is formed column by column in the registers of one lane and stored once; its loads are issued before the body's.
// Every access is predicated on the row's own bounds: feature loads end at ld, location loads at 128, stores at kpad.
#include "dispatch.hpp"

#define RG_ROUNDS 8
#define RG_VIEWS 36

// what a workgroup knows about its item after the scan
struct RgItem {
  bool bad;     // slot / view out of range or a count above P: all rows zero, mask 0
  int n;        // region rows of the item (0 when bad)
  int start;    // first kept row
};

// Called by all 256 threads.  pre[v] = rows of the views before v, pre[36] = n.
__device__ __forceinline__ RgItem rg_item(const RegionGatherArgs& a, int b, int* pre, int* flag) {
  const int lane = threadIdx.x & 63;
  const int slot = a.rows[2 * b], cur = a.rows[2 * b + 1];
  const bool bad0 = slot < 0 || slot >= a.N || cur < 0 || cur >= RG_VIEWS;
  if (threadIdx.x < 64) {
    int c = 0;
    if (!bad0 && lane < RG_VIEWS) c = a.counts[(long)slot * RG_VIEWS + lane];
    const bool over = c > a.P;
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    const bool bad = bad0 || __ballot(over) != 0;
    if (lane < RG_VIEWS) pre[lane + 1] = bad ? 0 : incl;
    if (lane == 0) { pre[0] = 0; *flag = bad ? 1 : 0; }
  }
  __syncthreads();
  RgItem it;
  it.bad = *flag != 0;
  it.n = pre[RG_VIEWS];
  it.start = it.n > a.R ? it.n - a.R : 0;
  return it;
}

// the view that holds region j < n: the number of views whose rows all come before or at j
__device__ __forceinline__ int rg_view_of(const int* pre, int j, int lane) {
  const bool before = lane < RG_VIEWS && pre[lane + 1] <= j;
  return __builtin_popcountll(__ballot(before));
}

// ---- one body piece: 8 feature columns as loaded, and as the 16 bytes to store ----------------------------------------
template <bool BF16> struct RgRaw { f32x4 lo, hi; };
template <> struct RgRaw<true> { u32x4 w; };

template <bool BF16>
__device__ __forceinline__ RgRaw<BF16> rg_load(const void* src, int q) {
  RgRaw<BF16> r;
  if constexpr (BF16) {
    r.w = ((const u32x4*)src)[q];
  } else {
    r.lo = ((const f32x4*)src)[2 * q];
    r.hi = ((const f32x4*)src)[2 * q + 1];
  }
  return r;
}

template <bool BF16>
__device__ __forceinline__ u32x4 rg_bits(const RgRaw<BF16>& r) {
  if constexpr (BF16) {
    return r.w;
  } else {
    return (u32x4){pack_bf16x2(r.lo[0], r.lo[1]), pack_bf16x2(r.lo[2], r.lo[3]), pack_bf16x2(r.hi[0], r.hi[1]),
                   pack_bf16x2(r.hi[2], r.hi[3])};
  }
}

template <bool BF16>
__device__ __forceinline__ void rg_floats(const RgRaw<BF16>& r, float* v) {
  if constexpr (BF16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = bf16lo(r.w[i]); v[2 * i + 1] = bf16hi(r.w[i]); }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = r.lo[i]; v[4 + i] = r.hi[i]; }
  }
}

// One packed output row.  src: the store row (ld elements, 16-byte aligned) or null for a zero row; loc: the 128 floats of
// the row's location embedding (unused for a zero row).
template <bool BF16>
__device__ __forceinline__ void rg_pack_row(const void* __restrict__ src, const float* __restrict__ loc,
                                            bf16_t* __restrict__ dst, int D, int kpad, int lane) {
  u32x4* d4 = (u32x4*)dst;
  const int np = kpad >> 3;   // pieces of the row
  const int nb = D >> 3;      // of them inside the feature row
  if (!src) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int q = lane; q < np; q += 64) d4[q] = z;
    return;
  }
  // the pieces from the seam on: one per lane (25 at D = 2054, kpad = 2240); a wider pad takes further turns below
  const int qt = nb + lane;
  RgRaw<BF16> seam = {};
  float lv[8];
  if (qt < np) {
    if (lane == 0 && (D & 7)) seam = rg_load<BF16>(src, nb);   // columns 8 nb .. ld - 1: inside the store row's padding
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = qt * 8 + i - D;
      lv[i] = (c >= 0 && c < 128) ? loc[c] : 0.f;
    }
  }
  int p0 = 0;
  for (; p0 + 64 * RG_ROUNDS <= nb; p0 += 64 * RG_ROUNDS) {   // whole groups of rounds: no predicate inside
    RgRaw<BF16> r[RG_ROUNDS];
#pragma unroll
    for (int k = 0; k < RG_ROUNDS; ++k) r[k] = rg_load<BF16>(src, p0 + k * 64 + lane);
#pragma unroll
    for (int k = 0; k < RG_ROUNDS; ++k) d4[p0 + k * 64 + lane] = rg_bits<BF16>(r[k]);
  }
  // the rest, fewer than 8 rounds: the round count is the wave's, the last round's idle lanes are switched off
  const int nr = (nb - p0 + 63) >> 6;
  if (nr > 0) {
    RgRaw<BF16> r[RG_ROUNDS - 1];
#pragma unroll
    for (int k = 0; k < RG_ROUNDS - 1; ++k) {
      if (k < nr - 1) r[k] = rg_load<BF16>(src, p0 + k * 64 + lane);
    }
    const int pl = p0 + (nr - 1) * 64 + lane;
    RgRaw<BF16> last = {};
    if (pl < nb) last = rg_load<BF16>(src, pl);
#pragma unroll
    for (int k = 0; k < RG_ROUNDS - 1; ++k) {
      if (k < nr - 1) d4[p0 + k * 64 + lane] = rg_bits<BF16>(r[k]);
    }
    if (pl < nb) d4[pl] = rg_bits<BF16>(last);
  }
  if (qt < np) {
    float fv[8];
    rg_floats<BF16>(seam, fv);
    u32x4 w;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = qt * 8 + 2 * i;
      w[i] = pack_bf16x2(c < D ? fv[2 * i] : lv[2 * i], c + 1 < D ? fv[2 * i + 1] : lv[2 * i + 1]);
    }
    d4[qt] = w;
  }
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (int q = qt + 64; q < np; q += 64) d4[q] = z;   // a pad of 64 pieces or more: columns >= D + 505, past the location row
}

// One unpacked output row: D fp32 features (pairs where PAIRS: D even, 8-byte aligned output) and 128 location floats.
template <bool BF16, bool PAIRS>
__device__ __forceinline__ void rg_plain_row(const void* __restrict__ src, const float* __restrict__ loc,
                                             float* __restrict__ fo, float* __restrict__ lo, int D, int lane) {
  if (PAIRS) {
    f32x2* o2 = (f32x2*)fo;
    for (int c = lane; c < (D >> 1); c += 64) {
      f32x2 v = {0.f, 0.f};
      if (src) {
        if constexpr (BF16) {
          const uint32_t w = ((const uint32_t*)src)[c];
          v = (f32x2){bf16lo(w), bf16hi(w)};
        } else {
          v = ((const f32x2*)src)[c];
        }
      }
      o2[c] = v;
    }
  } else {
    for (int c = lane; c < D; c += 64) {
      float v = 0.f;
      if (src) v = BF16 ? bf16_to_f32(((const bf16_t*)src)[c]) : ((const float*)src)[c];
      fo[c] = v;
    }
  }
  if (lane < 32) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (src) v = ((const f32x4*)loc)[lane];
    ((f32x4*)lo)[lane] = v;
  }
}

template <bool BF16, bool PACKED, bool PAIRS>
__global__ __launch_bounds__(256) void region_gather_kernel(RegionGatherArgs a) {
  __shared__ int pre[RG_VIEWS + 1];
  __shared__ int flag;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int R = a.R, T = a.T, G = (R + 3) >> 2;   // row workgroups per item; one more copies the text part
  const int b = blockIdx.x / (G + 1), g = blockIdx.x - b * (G + 1);
  const RgItem it = rg_item(a, b, pre, &flag);
  const long S = (long)T + R;
  if (g == G) {   // the [B, T + R] tensors of the item: the text part copied, the region part from the row map
    for (int t = threadIdx.x; t < T; t += 256) {
      a.labels[b * S + t] = a.text_labels[(long)b * T + t];
      a.mask[b * S + t] = a.text_mask[(long)b * T + t] ? 1 : 0;
      if (a.token_labels) a.token_labels[b * S + t] = a.text_token_classes[(long)b * T + t];
    }
    for (int r = threadIdx.x; r < R; r += 256) {
      a.labels[b * S + T + r] = -1;
      a.mask[b * S + T + r] = it.start + r < it.n ? 1 : 0;
      if (a.token_labels) a.token_labels[b * S + T + r] = -1;
    }
    if (it.bad && a.err && threadIdx.x == 0) *a.err = 1;
    return;
  }
  const int r = g * 4 + wave;
  if (r >= R) return;
  const int j = it.start + r;
  const void* src = nullptr;
  const float* loc = nullptr;
  if (j < it.n) {   // (n = 0 for a bad item)
    const int v = rg_view_of(pre, j, lane);
    const int p = j - pre[v];
    const long ld = ((long)a.D + 7) & ~7L;
    const long row = (((long)a.rows[2 * b] * RG_VIEWS + v) * a.P + p) * ld;
    src = BF16 ? (const void*)((const bf16_t*)a.store + row) : (const void*)((const float*)a.store + row);
    loc = a.loc_table + ((long)a.rows[2 * b + 1] * RG_VIEWS + v) * 128;
  }
  const long orow = (long)b * R + r;
  if (PACKED) rg_pack_row<BF16>(src, loc, (bf16_t*)a.packed + orow * a.kpad, a.D, a.kpad, lane);
  else rg_plain_row<BF16, PAIRS>(src, loc, a.feats + orow * a.D, a.loc + orow * 128, a.D, lane);
}

int vt_region_gather_dispatch(const RegionGatherArgs& a, hipStream_t stream) {
  if (!a.store || !a.counts || !a.loc_table || !a.rows || !a.text_labels || !a.text_mask || !a.labels || !a.mask) return VT_ERR_NULL;
  if ((a.token_labels != nullptr) != (a.text_token_classes != nullptr)) return VT_ERR_NULL;
  const bool packed = a.packed != nullptr;
  if (a.R > 0 && !packed && (!a.feats || !a.loc)) return VT_ERR_NULL;
  if (a.N < 1 || a.N > 0x7fffffffL || a.V != RG_VIEWS || a.P < 1 || a.P > 255 || a.D < 1 || a.B < 1 || a.T < 1 || a.R < 0) return VT_ERR_BAD_SHAPE;
  if (packed && ((a.kpad & 7) || a.kpad < a.D + 128)) return VT_ERR_BAD_SHAPE;
  if ((((uintptr_t)a.store) | ((uintptr_t)a.loc_table)) & 15) return VT_ERR_BAD_ALIGN;
  if (((uintptr_t)a.rows) & 3) return VT_ERR_BAD_ALIGN;
  if ((((uintptr_t)a.labels) | ((uintptr_t)a.mask) | ((uintptr_t)a.token_labels) | ((uintptr_t)a.text_labels) |
       ((uintptr_t)a.text_mask) | ((uintptr_t)a.text_token_classes)) & 7) return VT_ERR_BAD_ALIGN;
  if (packed ? (((uintptr_t)a.packed) & 15) != 0 : ((((uintptr_t)a.loc) & 15) != 0 || (((uintptr_t)a.feats) & 3) != 0)) return VT_ERR_BAD_ALIGN;
  const long groups = (long)a.B * (((long)a.R + 3) / 4 + 1);
  if (groups > 0x7fffffffL) return VT_ERR_BAD_SHAPE;
  const bool pairs = !packed && (a.D & 1) == 0 && (((uintptr_t)a.feats) & 7) == 0;
  const dim3 grid((unsigned)groups), block(256);
  if (packed) {
    if (a.store_bf16) hipLaunchKernelGGL((region_gather_kernel<true, true, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((region_gather_kernel<false, true, false>), grid, block, 0, stream, a);
  } else if (pairs) {
    if (a.store_bf16) hipLaunchKernelGGL((region_gather_kernel<true, false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((region_gather_kernel<false, false, true>), grid, block, 0, stream, a);
  } else {
    if (a.store_bf16) hipLaunchKernelGGL((region_gather_kernel<true, false, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((region_gather_kernel<false, false, false>), grid, block, 0, stream, a);
  }
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
