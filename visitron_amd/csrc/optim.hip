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
//
// Also here: shard_adamw / shard_settle, the optimizer sharded over data-parallel ranks (their own tables, below), and at
// the end of the file adamw_flat, the pretrain engine's AdamW over one flat slab, whose bits shard_adamw reproduces.
// adamw_flat stands at file scope, outside the anonymous namespace: recorded kernel statistics key on its symbol.
#include "dispatch.hpp"

namespace {

constexpr int kEntry = VT_OPTIM_ENTRY_WORDS;
constexpr int kHyper = VT_OPTIM_HYPER_FLOATS;
constexpr int kShardAdamWords = 7;     // vt_shard_adamw's table entry (include/visitron_hip.h)
constexpr int kShardSettleWords = 4;   // vt_shard_settle's
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

// ---- the optimizer sharded over data-parallel ranks: this rank's segments of the flat slabs -----------------------------
// Chunk table of kShardAdamWords uint64 per entry:
//   [0] p  [1] g  [2] m  [3] v  [4] mirror   byte addresses (p, m, v fp32; g fp32 or bf16; mirror bf16)
//   [5] n                                    elements, a multiple of 4
//   [6] decay                                non-zero: the chunk lies in the weight-decay group
// m and v point into the rank's shard-sized moment storage, the rest into the full slabs.  A lane moves 16 bytes of every
// fp32 operand and 8 bytes of every bf16 one; the element arithmetic is adamw_flat's own (adamw_flat_x4, common.hpp), so a
// sharded step leaves the bits the whole-slab launch leaves.
template <bool G16>
__global__ __launch_bounds__(kThreads) void shard_adamw(const uint64_t* __restrict__ table, long n_chunks, float lr,
                                                        float step_size, float b1, float b2, float eps, float wd,
                                                        float grad_scale) {
  for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t* e = table + c * kShardAdamWords;
    float* __restrict__ p = (float*)e[0];
    const void* __restrict__ g = (const void*)e[1];
    float* __restrict__ m = (float*)e[2];
    float* __restrict__ v = (float*)e[3];
    bf16_t* __restrict__ mirror = (bf16_t*)e[4];
    const int n4 = (int)(e[5] >> 2);
    const float wd_c = e[6] ? wd : 0.f;
    for (int i = threadIdx.x; i < n4; i += kThreads) {
      f32x4 pv = ((f32x4*)p)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
      f32x4 gv;
      if (G16) {
        const u32x2 w = ((const u32x2*)g)[i];
        gv = (f32x4){bf16lo(w[0]), bf16hi(w[0]), bf16lo(w[1]), bf16hi(w[1])};
      } else {
        gv = ((const f32x4*)g)[i];
      }
      adamw_flat_x4(pv, gv, mv, vv, lr, step_size, b1, b2, eps, wd_c, grad_scale);
      ((f32x4*)p)[i] = pv;
      ((f32x4*)m)[i] = mv;
      ((f32x4*)v)[i] = vv;
      u32x2 o;
      o[0] = pack_bf16x2(pv[0], pv[1]);
      o[1] = pack_bf16x2(pv[2], pv[3]);
      ((u32x2*)mirror)[i] = o;
    }
  }
}

// After the gather: the segments this rank does not own hold the owner's bits in ONE of the two copies; the other is made
// from it.  Chunk table of kShardSettleWords uint64: [0] p  [1] mirror  [2] n (a multiple of 4)  [3] direction --
// 0: p = float(mirror) (the weights travelled as bf16), 1: mirror = bf16(p) (they travelled as fp32).
__global__ __launch_bounds__(kThreads) void shard_settle(const uint64_t* __restrict__ table, long n_chunks) {
  for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t* e = table + c * kShardSettleWords;
    float* __restrict__ p = (float*)e[0];
    bf16_t* __restrict__ mirror = (bf16_t*)e[1];
    const int n4 = (int)(e[2] >> 2);
    if (e[3] == 0) {
      for (int i = threadIdx.x; i < n4; i += kThreads) {
        const u32x2 w = ((const u32x2*)mirror)[i];
        ((f32x4*)p)[i] = (f32x4){bf16lo(w[0]), bf16hi(w[0]), bf16lo(w[1]), bf16hi(w[1])};
      }
    } else {
      for (int i = threadIdx.x; i < n4; i += kThreads) {
        const f32x4 pv = ((const f32x4*)p)[i];
        u32x2 o;
        o[0] = pack_bf16x2(pv[0], pv[1]);
        o[1] = pack_bf16x2(pv[2], pv[3]);
        ((u32x2*)mirror)[i] = o;
      }
    }
  }
}

unsigned grid_for(long n_chunks) { return (unsigned)(n_chunks < kMaxGrid ? n_chunks : kMaxGrid); }

int launched() { return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP; }

}  // namespace

// The tables live in device memory, so the entry points check the HOST copy the caller built them from (the same words):
// a null or misaligned address or a count that is no multiple of 4 is refused before anything is launched.
int vt_shard_adamw_dispatch(const uint64_t* table, const uint64_t* host_table, long n_chunks, int g_is_bf16, float lr,
                            float step_size, float b1, float b2, float eps, float wd, float grad_scale, hipStream_t stream) {
  if (!table || !host_table) return VT_ERR_NULL;
  if (n_chunks <= 0) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)table & 7) || ((uintptr_t)host_table & 7)) return VT_ERR_BAD_ALIGN;
  for (long c = 0; c < n_chunks; ++c) {
    const uint64_t* e = host_table + c * kShardAdamWords;
    if (!e[0] || !e[1] || !e[2] || !e[3] || !e[4]) return VT_ERR_NULL;
    if (e[5] == 0 || (e[5] & 3) || e[5] > (uint64_t)0x7fffffff) return VT_ERR_BAD_SHAPE;
    if (((e[0] | e[2] | e[3]) & 15) || (e[1] & (g_is_bf16 ? 7 : 15)) || (e[4] & 7)) return VT_ERR_BAD_ALIGN;
  }
  if (g_is_bf16)
    hipLaunchKernelGGL(shard_adamw<true>, dim3(grid_for(n_chunks)), dim3(kThreads), 0, stream, table, n_chunks, lr, step_size,
                       b1, b2, eps, wd, grad_scale);
  else
    hipLaunchKernelGGL(shard_adamw<false>, dim3(grid_for(n_chunks)), dim3(kThreads), 0, stream, table, n_chunks, lr, step_size,
                       b1, b2, eps, wd, grad_scale);
  return launched();
}

int vt_shard_settle_dispatch(const uint64_t* table, const uint64_t* host_table, long n_chunks, hipStream_t stream) {
  if (!table || !host_table) return VT_ERR_NULL;
  if (n_chunks <= 0) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)table & 7) || ((uintptr_t)host_table & 7)) return VT_ERR_BAD_ALIGN;
  for (long c = 0; c < n_chunks; ++c) {
    const uint64_t* e = host_table + c * kShardSettleWords;
    if (!e[0] || !e[1]) return VT_ERR_NULL;
    if (e[2] == 0 || (e[2] & 3) || e[2] > (uint64_t)0x7fffffff || e[3] > 1) return VT_ERR_BAD_SHAPE;
    if ((e[0] & 15) || (e[1] & 7)) return VT_ERR_BAD_ALIGN;
  }
  hipLaunchKernelGGL(shard_settle, dim3(grid_for(n_chunks)), dim3(kThreads), 0, stream, table, n_chunks);
  return launched();
}

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

// ---------------------------------------------------------------------------------------------
// Fused AdamW step over a flat fp32 parameter slab, the pytorch-transformers rule used by
// tasks/viewpoint_select/pretrain.py:128-130,192:
//   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= step_size * m / (sqrt(v) + eps);  p -= lr*wd*p
// with step_size = lr * sqrt(1-b2^t) / (1-b1^t) computed on the host (eps is added to the UN-corrected
// sqrt(v); the decoupled decay uses the already-moved p).  Also refreshes the bf16 working copy the
// GEMMs read.  grad_scale multiplies g first (1/world_size for the data-parallel mean).
// G16: the gradients arrive as bf16 (the data-parallel all-reduce ran on a bf16 copy of the slab: half the bytes over
// xGMI); moments and master weights stay fp32.
template <bool G16>
__global__ __launch_bounds__(256) void adamw_flat(float* __restrict__ p, const void* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, bf16_t* __restrict__ p_bf16, long n4, float lr,
                                                  float step_size, float b1, float b2, float eps, float wd,
                                                  float grad_scale) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = ((f32x4*)p)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
    f32x4 gv;
    if (G16) {
      const u32x2 w = ((const u32x2*)g)[i];
      gv = (f32x4){bf16lo(w[0]), bf16hi(w[0]), bf16lo(w[1]), bf16hi(w[1])};
    } else {
      gv = ((const f32x4*)g)[i];
    }
    adamw_flat_x4(pv, gv, mv, vv, lr, step_size, b1, b2, eps, wd, grad_scale);
    ((f32x4*)p)[i] = pv;
    ((f32x4*)m)[i] = mv;
    ((f32x4*)v)[i] = vv;
    if (p_bf16) {
      u32x2 o;
      o[0] = pack_bf16x2(pv[0], pv[1]);
      o[1] = pack_bf16x2(pv[2], pv[3]);
      ((u32x2*)p_bf16)[i] = o;
    }
  }
}

int vt_adamw_dispatch(float* p, const void* g, int g_is_bf16, float* m, float* v, void* p_bf16, long n, float lr,
                      float step_size, float b1, float b2, float eps, float wd, float grad_scale, hipStream_t stream) {
  if (!p || !g || !m || !v) return VT_ERR_NULL;
  if (n <= 0 || (n % 4)) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15 || ((uintptr_t)g & (g_is_bf16 ? 7 : 15)) || ((uintptr_t)p_bf16 & 7)) return VT_ERR_BAD_ALIGN;
  const long n4 = n / 4;
  long blocks = (n4 + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  if (g_is_bf16)
    hipLaunchKernelGGL(adamw_flat<true>, dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v, (bf16_t*)p_bf16, n4, lr,
                       step_size, b1, b2, eps, wd, grad_scale);
  else
    hipLaunchKernelGGL(adamw_flat<false>, dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v, (bf16_t*)p_bf16, n4, lr,
                       step_size, b1, b2, eps, wd, grad_scale);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}
