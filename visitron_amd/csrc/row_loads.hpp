// Loads from fp32 rows whose alignment the kernel may not assume (rollout.hip, turn_based.hip): a 2058- or 2054-float row
// is 8-byte aligned when its base is, a row of odd width on every other row at best.  The width of a load follows the
// address, and no load touches an element outside the columns it was asked for.
#pragma once
#include "common.hpp"

// 4 consecutive columns c .. c+3 of the virtual row [ep[0 .. E) | fp[0 .. K - E)], zero from column K on.  One 16-byte load
// when the group lies inside one source and its address is 16-byte aligned, two 8-byte loads when 8-byte aligned, element
// by element otherwise and where the group straddles the seam between the sources or the end of the row.  ep == nullptr: the
// first source counts as zero.
__device__ __forceinline__ f32x4 load4_cat(const float* ep, int E, const float* fp, int K, int c) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (c >= K) return v;
  const float* p = nullptr;
  if (c + 4 <= E) p = ep ? ep + c : nullptr;
  else if (c >= E && c + 4 <= K) p = fp + (c - E);
  if (p) {
    const uintptr_t ad = (uintptr_t)p;
    if ((ad & 15) == 0) return *(const f32x4*)p;
    if ((ad & 7) == 0) {
      const f32x2 lo = *(const f32x2*)p, hi = *(const f32x2*)(p + 2);
      return (f32x4){lo[0], lo[1], hi[0], hi[1]};
    }
    return (f32x4){p[0], p[1], p[2], p[3]};
  }
  if (c + 4 <= E) return v;   // a first source that counts as zero
#pragma unroll
  for (int j = 0; j < 4; ++j) {   // the group straddles the seam between the two sources, or the end of the row
    const int cc = c + j;
    if (cc < E) v[j] = ep ? ep[cc] : 0.f;
    else if (cc < K) v[j] = fp[cc - E];
  }
  return v;
}

// W consecutive floats (W = 1, or 2 at an 8-byte aligned address) as one load / one store
template <int W> struct RowPiece;
template <> struct RowPiece<1> {
  float v[1];
  __device__ __forceinline__ static RowPiece ld(const float* p) { return RowPiece{{p[0]}}; }
  __device__ __forceinline__ void st(float* p) const { p[0] = v[0]; }
};
template <> struct RowPiece<2> {
  float v[2];
  __device__ __forceinline__ static RowPiece ld(const float* p) {
    const f32x2 t = *(const f32x2*)p;
    return RowPiece{{t[0], t[1]}};
  }
  __device__ __forceinline__ void st(float* p) const { *(f32x2*)p = (f32x2){v[0], v[1]}; }
};
