// Deferred-LayerNorm GEMMs of the inference path (GemmArgs::ln_mode 1 / 2, see gemm_common.hpp): launchers of the
// 256x256-tile kernels of gemm_v7_kernels.hpp with the epilogues of gemm_v7_ln_epilogue.hpp.  One translation unit of
// its own so that it compiles beside gemm_v7.hip.
#include "gemm_v7_kernels.hpp"

template <int ACT, int LNM>
static int launch_ln(const GemmArgs& g, int persistent, int mtn, hipStream_t stream, bool shared_tiles) {
  GemmArgs ga = g;
  if (shared_tiles && !persistent) return VT_ERR_UNSUPPORTED;
  if (shared_tiles && mtn <= 5 && !vt_gemm_v8_take_region(ga)) return VT_ERR_UNSUPPORTED;   // (the region: 160- / 128-row tiles only)
  ga.tiles_n = (g.N + 255) / 256;
  ga.tiles_m = (g.M + 32 * mtn - 1) / (32 * mtn);
  const int tiles = ga.tiles_m * ga.tiles_n;
  void (*kern)(GemmArgs) = nullptr;
  int grid = tiles;
  if (persistent) {
    grid = vt_gemm_v8_grid(tiles, ga.sk_parts);
    if (grid <= 0) return VT_ERR_HIP;
    switch (mtn) {
      case 8: kern = gemm_nt_bf16_v8<ACT, false, true, false, 8, LNM>; break;
      case 7: kern = gemm_nt_bf16_v8<ACT, false, true, false, 7, LNM>; break;
      case 6: kern = gemm_nt_bf16_v8<ACT, false, true, false, 6, LNM>; break;
      case 5: kern = gemm_nt_bf16_v8<ACT, false, true, false, 5, LNM>; break;
      case 4: kern = gemm_nt_bf16_v8<ACT, false, true, false, 4, LNM>; break;
      default: return VT_ERR_UNSUPPORTED;
    }
  } else {
    switch (mtn) {
      case 8: kern = gemm_nt_bf16_v7<ACT, false, true, false, 8, LNM>; break;
      case 7: kern = gemm_nt_bf16_v7<ACT, false, true, false, 7, LNM>; break;
      case 6: kern = gemm_nt_bf16_v7<ACT, false, true, false, 6, LNM>; break;
      default: return VT_ERR_UNSUPPORTED;
    }
  }
  if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, V7_LDS_BYTES_LN) != hipSuccess) return VT_ERR_HIP;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), V7_LDS_BYTES_LN, stream, ga);
  return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_HIP;
}

// variant: a number of gemm_variants.def with LN_EPILOGUE (vt_gemm_ln_dispatch sends the others to the persistent 256-row kernel)
int vt_gemm_ln_launch(const GemmArgs& g, int act, int variant, hipStream_t stream) {
  const gv::Variant* v = gv::find(variant);
  if (!v || !(v->flags & gv::LN_EPILOGUE)) return VT_ERR_UNSUPPORTED;
  const int persistent = (v->flags & gv::PERSISTENT) ? 1 : 0, mtn = v->mtn;
  const bool sk = v->family == gv::V8_SHARED;   // the persistent kernel sharing its left-over tiles (gemm_v7.hip)
  if (g.K < 128 || (g.N & 127) || !v7_operands_fit(g)) return VT_ERR_UNSUPPORTED;
  if (g.ln_mode == 1) {
    if (act == ACT_NONE) return launch_ln<ACT_NONE, 1>(g, persistent, mtn, stream, sk);
    if (act == ACT_GELU) return launch_ln<ACT_GELU, 1>(g, persistent, mtn, stream, sk);
    return VT_ERR_UNSUPPORTED;
  }
  if (g.ln_mode == 2 && act == ACT_NONE) return launch_ln<ACT_NONE, 2>(g, persistent, mtn, stream, sk);
  return VT_ERR_UNSUPPORTED;
}
