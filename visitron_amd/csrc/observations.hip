// The rollout's observation tensors gathered from a device feature store (tasks/viewpoint_select/agent.py:186-228 fed by
// data_loader.py:516-642; tasks/turn_based/agent.py:197-210).  Pure byte movers: one wave per output row, four waves per
// workgroup, and the four rows of a workgroup belong to one agent, so they read one store slot.
//
// A row is D image floats from store[slot, view, :] followed by 4 angle floats.  With D % 4 == 0 and 16-byte aligned bases
// every source and destination row starts 16-byte aligned: a lane moves 16-byte pieces, up to 8 of them are loaded before the
// first is stored (8 rounds x 64 lanes x 16 bytes = the shipped 2048-float row in one go, without a predicate or a branch
// between the 8 loads and the 8 stores; a width that leaves fewer than 8 rounds over takes them in a second, predicated
// group, whose stores the compiler separates by full waits), and the angle tail is one more 16-byte store by the lane whose
// turn it is.  An even D that is no multiple of 4 (the reference's default 2054) with 8-byte aligned bases leaves every row
// 8-byte aligned: the same shape with 8-byte pieces (W = 2: 8 rounds x 64 lanes x 8 bytes, two such groups and a rest for
// 2054 floats) and the tail as two 8-byte stores.  An odd D, or outputs aligned to less, goes element by element.  A zero
// row (END, padding, bad index) is stores only.  Every access is predicated on the row's own bounds: no piece index reaches
// D / W on the source side, and the tail ends at D + 4 on the destination side.
#include "dispatch.hpp"

#define OBS_ROUNDS 8

// sin h, cos h, sin e, cos e in float64, rounded once.  Called by the whole wave: lane `owner` evaluates the heading while
// its neighbour (owner ^ 1) evaluates the elevation in the same instructions; the result is valid on lane `owner`.
__device__ __forceinline__ f32x4 obs_angle(double h, double e, int lane, int owner) {
  double s = 0.0, c = 1.0;
  if ((lane | 1) == (owner | 1)) sincos(lane == owner ? h : e, &s, &c);
  const float sf = (float)s, cf = (float)c;
  return (f32x4){sf, cf, __shfl(sf, owner ^ 1, 64), __shfl(cf, owner ^ 1, 64)};
}

// One output row: the image part (src is null for a zero row) and, where h and e point at a candidate's heading and
// elevation, the row's angle tail, evaluated after the first loads have been issued and before they are stored, so the
// float64 arithmetic runs under the loads' latency.  -> the tail on lane `owner`.
template <int W> struct ObsPiece { typedef float type; };
template <> struct ObsPiece<4> { typedef f32x4 type; };
template <> struct ObsPiece<2> { typedef f32x2 type; };

// W = floats per piece: 4, 2 or 1 (element by element)
template <int W>
__device__ __forceinline__ f32x4 obs_copy_row(const float* __restrict__ src, float* __restrict__ dst, int D, int lane,
                                              f32x4 tail, const double* h, const double* e, int owner) {
  typedef typename ObsPiece<W>::type piece;
  bool pending = h != nullptr;
  if (W > 1) {
    const int np = D / W;
    const piece* s4 = (const piece*)src;
    piece* d4 = (piece*)dst;
    if (!src) {
      const piece z = {};
      for (int p = lane; p < np; p += 64) d4[p] = z;
      return tail;
    }
    int p0 = 0;
    for (; p0 + 64 * OBS_ROUNDS <= np; p0 += 64 * OBS_ROUNDS) {   // whole groups of rounds: no predicate inside
      piece r[OBS_ROUNDS];
#pragma unroll
      for (int k = 0; k < OBS_ROUNDS; ++k) r[k] = s4[p0 + k * 64 + lane];
      if (pending) { tail = obs_angle(*h, *e, lane, owner); pending = false; }
#pragma unroll
      for (int k = 0; k < OBS_ROUNDS; ++k) d4[p0 + k * 64 + lane] = r[k];
    }
    // the rest, fewer than 8 rounds: the round count is the wave's, the last round's idle lanes are switched off
    const int nr = (np - p0 + 63) >> 6;
    if (nr > 0) {
      piece r[OBS_ROUNDS - 1];
#pragma unroll
      for (int k = 0; k < OBS_ROUNDS - 1; ++k) {
        const int p = p0 + k * 64 + lane;
        if (k < nr - 1) r[k] = s4[p];
      }
      const int pl = p0 + (nr - 1) * 64 + lane;
      piece last = {};
      if (pl < np) last = s4[pl];
      if (pending) { tail = obs_angle(*h, *e, lane, owner); pending = false; }
#pragma unroll
      for (int k = 0; k < OBS_ROUNDS - 1; ++k) {
        const int p = p0 + k * 64 + lane;
        if (k < nr - 1) d4[p] = r[k];
      }
      if (pl < np) d4[pl] = last;
    }
  } else {
    for (int c = lane; c < D; c += 64) dst[c] = src ? src[c] : 0.f;
  }
  if (pending) tail = obs_angle(*h, *e, lane, owner);
  return tail;
}

// the 4 floats behind the image part, held by lane `owner`: one 16-byte store, two 8-byte stores or four 4-byte stores
template <int W>
__device__ __forceinline__ void obs_store_tail(float* dst, int D, f32x4 v, int lane, int owner) {
  if (lane != owner) return;
  if (W == 4) {
    *(f32x4*)(dst + D) = v;
  } else if (W == 2) {
    *(f32x2*)(dst + D) = (f32x2){v[0], v[1]};
    *(f32x2*)(dst + D + 2) = (f32x2){v[2], v[3]};
  } else {
    dst[D] = v[0]; dst[D + 1] = v[1]; dst[D + 2] = v[2]; dst[D + 3] = v[3];
  }
}

template <int W>
__global__ __launch_bounds__(256) void obs_gather_kernel(ObsGatherArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V, D = a.D, Cmax = a.Cmax;
  const int R = V + Cmax, G = (R + 3) >> 2;     // rows and workgroups per agent
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const int r = g * 4 + wave;
  const int slot = a.rows[3 * b], view = a.rows[3 * b + 1], count = a.rows[3 * b + 2];
  const int* pts = a.pts + (long)b * Cmax;
  bool bad = slot < 0 || slot >= a.N || view < 0 || view >= V || count < 0 || count >= Cmax;
  if (!bad) {   // every wave of the agent looks at all of its candidate views: a bad one zeroes the whole agent
    bool out = false;
    for (int j = lane; j < count; j += 64) {
      const int q = pts[j];
      out = out || q < 0 || q >= V;
    }
    bad = __ballot(out) != 0;
  }
  const int owner = W > 1 ? ((D / W) & 63) : 0;   // the lane that holds and stores the row's tail
  if (r < R) {
    const long ldo = (long)D + 4;
    float* dst;
    const float* src = nullptr;
    const double* h = nullptr;
    const double* e = nullptr;
    f32x4 tail = {0.f, 0.f, 0.f, 0.f};
    if (r < V) {
      dst = a.f_t + ((long)b * V + r) * ldo;
      if (!bad) {
        src = a.store + ((long)slot * V + r) * D;
        const float* t = a.table + ((long)view * V + r) * 4;
        if (lane == owner) tail = W > 1 ? *(const f32x4*)t : (f32x4){t[0], t[1], t[2], t[3]};   // (the table is 16-byte aligned)
      }
    } else {
      const int j = r - V;
      dst = a.cand + ((long)b * Cmax + j) * ldo;
      if (!bad && j < count) {
        src = a.store + ((long)slot * V + pts[j]) * D;
        h = a.cand_h + (long)b * Cmax + j;
        e = a.cand_e + (long)b * Cmax + j;
      }
    }
    tail = obs_copy_row<W>(src, dst, D, lane, tail, h, e, owner);
    obs_store_tail<W>(dst, D, tail, lane, owner);
  }
  if (g == 0 && wave == 0) {   // the per-agent outputs, behind this wave's row
    const int leng = (count < 0 ? 0 : (count >= Cmax ? Cmax - 1 : count)) + 1;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!bad) v = obs_angle(a.agent[2 * b], a.agent[2 * b + 1], lane, 0);
    if (lane == 0) {
      a.leng[b] = leng;
      if (bad && a.err) *a.err = 1;
      float* at = a.a_t + 4 * (long)b;
      at[0] = v[0]; at[1] = v[1]; at[2] = v[2]; at[3] = v[3];
    }
    for (int j = lane; j < Cmax; j += 64) a.mask[(long)b * Cmax + j] = j >= leng ? 1 : 0;
  }
}

int vt_obs_gather_dispatch(const ObsGatherArgs& a, hipStream_t stream) {
  if (!a.store || !a.table || !a.rows || !a.a_t || !a.f_t || !a.cand || !a.leng || !a.mask) return VT_ERR_NULL;
  if (a.N < 1 || a.N > 0x7fffffffL || a.V < 1 || a.D <= 0 || a.B <= 0 || a.Cmax < 1) return VT_ERR_BAD_SHAPE;
  if ((((uintptr_t)a.store) | ((uintptr_t)a.table)) & 15) return VT_ERR_BAD_ALIGN;
  if ((((uintptr_t)a.a_t) | ((uintptr_t)a.f_t) | ((uintptr_t)a.cand) | ((uintptr_t)a.leng)) & 3) return VT_ERR_BAD_ALIGN;
  const long groups = (long)a.B * (((long)a.V + a.Cmax + 3) / 4);
  if (groups > 0x7fffffffL) return VT_ERR_BAD_SHAPE;
  const bool vec = (a.D & 3) == 0 && ((((uintptr_t)a.f_t) | ((uintptr_t)a.cand)) & 15) == 0;
  const bool vec2 = !vec && (a.D & 1) == 0 && ((((uintptr_t)a.f_t) | ((uintptr_t)a.cand)) & 7) == 0;
  if (vec) hipLaunchKernelGGL(obs_gather_kernel<4>, dim3((unsigned)groups), dim3(256), 0, stream, a);
  else if (vec2) hipLaunchKernelGGL(obs_gather_kernel<2>, dim3((unsigned)groups), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(obs_gather_kernel<1>, dim3((unsigned)groups), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------
// out[b, :] = store[slot_b, view_b, :]: one wave per row, four rows per workgroup
template <int W>
__global__ __launch_bounds__(256) void obs_view_kernel(ObsViewArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = blockIdx.x * 4 + wave;
  if (row >= a.B) return;
  const int slot = a.rows[2 * row], view = a.rows[2 * row + 1];
  const bool bad = slot < 0 || slot >= a.N || view < 0 || view >= a.V;
  if (bad && a.err && lane == 0) *a.err = 1;
  const float* src = bad ? nullptr : a.store + ((long)slot * a.V + view) * a.D;
  obs_copy_row<W>(src, a.out + (long)row * a.ld_out, a.D, lane, (f32x4){0.f, 0.f, 0.f, 0.f}, nullptr, nullptr, 0);
}

int vt_obs_gather_view_dispatch(const ObsViewArgs& a, hipStream_t stream) {
  if (!a.store || !a.rows || !a.out) return VT_ERR_NULL;
  if (a.N < 1 || a.N > 0x7fffffffL || a.V < 1 || a.D <= 0 || a.B <= 0 || a.ld_out < a.D) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)a.store) & 15) return VT_ERR_BAD_ALIGN;
  if ((((uintptr_t)a.rows) | ((uintptr_t)a.out)) & 3) return VT_ERR_BAD_ALIGN;
  const bool vec = (a.D & 3) == 0 && (a.ld_out & 3) == 0 && (((uintptr_t)a.out) & 15) == 0;
  const bool vec2 = !vec && (a.D & 1) == 0 && (a.ld_out & 1) == 0 && (((uintptr_t)a.out) & 7) == 0;
  const unsigned groups = (unsigned)((a.B + 3) / 4);
  if (vec) hipLaunchKernelGGL(obs_view_kernel<4>, dim3(groups), dim3(256), 0, stream, a);
  else if (vec2) hipLaunchKernelGGL(obs_view_kernel<2>, dim3(groups), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(obs_view_kernel<1>, dim3(groups), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
