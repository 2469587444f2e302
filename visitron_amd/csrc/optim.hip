// Multi-tensor optimizer kernels: Adam / AdamW, the gradient norm and the clip of the reference's own loops
// (tasks/viewpoint_select/pretrain.py:128-130,192: pytorch-transformers AdamW; agent.py:129,511-518: two
// clip_grad_norm at 40.0 and two torch.optim.Adam).  One launch serves a whole parameter list of any shape.
//
// The list arrives as a device-resident CHUNK TABLE of n_chunks entries of VT_OPTIM_ENTRY_WORDS uint64 each:
//   [0] p  [1] g  [2] m  [3] v   byte addresses of the chunk's first element (fp32; 0 where the kernel does not use it)
//   [4] n                        elements of the chunk, 1 .. VT_OPTIM_CHUNK
//   [5] slot                     index of the chunk's hyper-parameter slot (vt_multi_adam only)
// The host cuts every tensor at multiples of VT_OPTIM_CHUNK elements, so a chunk is as aligned as its tensor.  The grid
// is capped and workgroups stride over the table: the launch count never depends on the list.  A chunk whose addresses
// are all multiples of 16 moves 16 bytes per lane and finishes its last n % 4 elements one per lane; any other chunk
// (a view that starts 4 bytes into a buffer) moves one element per lane.  The branch is uniform over the workgroup.
#include "dispatch.hpp"

namespace {

constexpr int kEntry = VT_OPTIM_ENTRY_WORDS;
constexpr int kHyper = VT_OPTIM_HYPER_FLOATS;
constexpr int kThreads = 256;
constexpr int kMaxGrid = 2048;   // 256 CUs x 8 workgroups of 256 threads: a memory-bound kernel gains nothing beyond

struct Hyper {
  float b1, omb1, b2, omb2, step_size, rsbc2, eps, lrwd;
};

// One element of either rule; the host's constants select it (rsbc2 = 1: pytorch-transformers AdamW; lrwd = 0 and
// rsbc2 = 1 / sqrt(1 - b2^t): torch.optim.Adam).  1 - b1 and 1 - b2 come from the host, formed in double: 1.0f - 0.999f
// is 1.3e-5 off.  Every product and sum is written out as the fma it is meant to be, so the 16-byte and the one-element
// paths round alike.
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const Hyper& h, float grad_coef) {
  const float gg = g * grad_coef;
  m = __builtin_fmaf(h.b1, m, h.omb1 * gg);
  v = __builtin_fmaf(h.b2, v, (h.omb2 * gg) * gg);
  const float den = __builtin_fmaf(sqrtf(v), h.rsbc2, h.eps);
  float x = __builtin_fmaf(-h.step_size, m / den, p);
  if (h.lrwd > 0.f) x = __builtin_fmaf(-h.lrwd, x, x);
  p = x;
}

__device__ __forceinline__ bool aligned16(uint64_t bits) { return (bits & 15) == 0; }

__global__ __launch_bounds__(kThreads) void multi_adam(const uint64_t* __restrict__ table, long n_chunks,
                                                       const float* __restrict__ hyper, float grad_coef,
                                                       const float* __restrict__ grad_coef_dev) {
  const float coef = grad_coef_dev ? *grad_coef_dev : grad_coef;
  for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t* e = table + c * kEntry;
    float* __restrict__ p = (float*)e[0];
    const float* __restrict__ g = (const float*)e[1];
    float* __restrict__ m = (float*)e[2];
    float* __restrict__ v = (float*)e[3];
    const int n = (int)e[4];
    const float* hs = hyper + e[5] * kHyper;
    const Hyper h = {hs[0], hs[1], hs[2], hs[3], hs[4], hs[5], hs[6], hs[7]};
    if (aligned16(e[0] | e[1] | e[2] | e[3])) {
      const int n4 = n >> 2;
      for (int i = threadIdx.x; i < n4; i += kThreads) {
        f32x4 pv = ((f32x4*)p)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
        const f32x4 gv = ((const f32x4*)g)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float pk = pv[k], mk = mv[k], vk = vv[k];
          adam_element(pk, gv[k], mk, vk, h, coef);
          pv[k] = pk;
          mv[k] = mk;
          vv[k] = vk;
        }
        ((f32x4*)p)[i] = pv;
        ((f32x4*)m)[i] = mv;
        ((f32x4*)v)[i] = vv;
      }
      const int i = 4 * n4 + threadIdx.x;
      if (i < n) adam_element(p[i], g[i], m[i], v[i], h, coef);
    } else {
      for (int i = threadIdx.x; i < n; i += kThreads) adam_element(p[i], g[i], m[i], v[i], h, coef);
    }
  }
}

// Sum over the workgroup in a fixed order: butterfly inside each wave, then the four waves' sums in wave order.
__device__ __forceinline__ double block_sum(double s, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  const double t = (lds[0] + lds[1]) + (lds[2] + lds[3]);
  __syncthreads();
  return t;
}

// partials[c] = sum of g^2 over chunk c.  Every square is formed and added in fp64 (exact products of fp32 values), so no
// fp32 accumulation chain exists at all; one value per chunk and no atomics: the same input gives the same bits.
__global__ __launch_bounds__(kThreads) void multi_sumsq(const uint64_t* __restrict__ table, long n_chunks,
                                                        double* __restrict__ partials) {
  __shared__ double lds[kThreads / 64];
  for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t* e = table + c * kEntry;
    const float* __restrict__ g = (const float*)e[1];
    const int n = (int)e[4];
    double s = 0.0;
    if (aligned16(e[1])) {
      const int n4 = n >> 2;
      for (int i = threadIdx.x; i < n4; i += kThreads) {
        const f32x4 gv = ((const f32x4*)g)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) s = __builtin_fma((double)gv[k], (double)gv[k], s);
      }
      const int i = 4 * n4 + threadIdx.x;
      if (i < n) s = __builtin_fma((double)g[i], (double)g[i], s);
    } else {
      for (int i = threadIdx.x; i < n; i += kThreads) s = __builtin_fma((double)g[i], (double)g[i], s);
    }
    s = block_sum(s, lds);
    if (threadIdx.x == 0) partials[c] = s;
  }
}

// One workgroup: the partials in a fixed order in fp64, then torch.nn.utils.clip_grad_norm_'s rule in fp32:
// out[0] = total_norm = sqrt(sum), out[1] = clip_coef = min(1, max_norm / (total_norm + 1e-6)).  The quotient is taken in
// fp64 and rounded once, which is the correctly rounded fp32 quotient whatever the build's division is.
__global__ __launch_bounds__(kThreads) void norm_finish(const double* __restrict__ partials, long n_chunks, float max_norm,
                                                        float* __restrict__ out) {
  __shared__ double lds[kThreads / 64];
  double s = 0.0;
  for (long c = threadIdx.x; c < n_chunks; c += kThreads) s += partials[c];
  s = block_sum(s, lds);
  if (threadIdx.x == 0) {
    const float total = (float)sqrt(s);
    const float den = total + 1e-6f;
    const float coef = (float)((double)max_norm / (double)den);
    out[0] = total;
    out[1] = coef > 1.0f ? 1.0f : coef;   // (a NaN norm gives a NaN coefficient, as torch's clamp does)
  }
}

__global__ __launch_bounds__(kThreads) void multi_scale(const uint64_t* __restrict__ table, long n_chunks,
                                                        const float* __restrict__ coef_dev) {
  const float coef = *coef_dev;
  for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t* e = table + c * kEntry;
    float* __restrict__ g = (float*)e[1];
    const int n = (int)e[4];
    if (aligned16(e[1])) {
      const int n4 = n >> 2;
      for (int i = threadIdx.x; i < n4; i += kThreads) {
        f32x4 gv = ((f32x4*)g)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) gv[k] *= coef;
        ((f32x4*)g)[i] = gv;
      }
      const int i = 4 * n4 + threadIdx.x;
      if (i < n) g[i] *= coef;
    } else {
      for (int i = threadIdx.x; i < n; i += kThreads) g[i] *= coef;
    }
  }
}

unsigned grid_for(long n_chunks) { return (unsigned)(n_chunks < kMaxGrid ? n_chunks : kMaxGrid); }

int launched() { return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP; }

}  // namespace

int vt_multi_adam_dispatch(const uint64_t* table, long n_chunks, const float* hyper, float grad_coef,
                           const float* grad_coef_dev, hipStream_t stream) {
  if (!table || !hyper) return VT_ERR_NULL;
  if (n_chunks <= 0) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)table & 7) || ((uintptr_t)hyper & 3) || ((uintptr_t)grad_coef_dev & 3)) return VT_ERR_BAD_ALIGN;
  hipLaunchKernelGGL(multi_adam, dim3(grid_for(n_chunks)), dim3(kThreads), 0, stream, table, n_chunks, hyper, grad_coef,
                     grad_coef_dev);
  return launched();
}

int vt_multi_sumsq_dispatch(const uint64_t* table, long n_chunks, void* partials, hipStream_t stream) {
  if (!table || !partials) return VT_ERR_NULL;
  if (n_chunks <= 0) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)table & 7) || ((uintptr_t)partials & 7)) return VT_ERR_BAD_ALIGN;
  hipLaunchKernelGGL(multi_sumsq, dim3(grid_for(n_chunks)), dim3(kThreads), 0, stream, table, n_chunks, (double*)partials);
  return launched();
}

int vt_norm_finish_dispatch(const void* partials, long n_chunks, float max_norm, float* out, hipStream_t stream) {
  if (!out || (n_chunks > 0 && !partials)) return VT_ERR_NULL;
  if (n_chunks < 0) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)partials & 7) || ((uintptr_t)out & 3)) return VT_ERR_BAD_ALIGN;
  hipLaunchKernelGGL(norm_finish, dim3(1), dim3(kThreads), 0, stream, (const double*)partials, n_chunks, max_norm, out);
  return launched();
}

int vt_multi_scale_dispatch(const uint64_t* table, long n_chunks, const float* coef_dev, hipStream_t stream) {
  if (!table || !coef_dev) return VT_ERR_NULL;
  if (n_chunks <= 0) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)table & 7) || ((uintptr_t)coef_dev & 3)) return VT_ERR_BAD_ALIGN;
  hipLaunchKernelGGL(multi_scale, dim3(grid_for(n_chunks)), dim3(kThreads), 0, stream, table, n_chunks, coef_dev);
  return launched();
}
