// The C-ABI entry points declared in include/visitron_hip.h, and nothing else.  Thin: argument checks, loops and whatever
// the host side remembers between calls live in the *_dispatch functions next to each kernel.
#include "dispatch.hpp"

// the structs of the header as the ctypes binding measures them (tests/test_capi_symbols.py pins the same numbers)
static_assert(sizeof(vt_layer_weights) == 96 && sizeof(vt_layer_acts) == 136 && sizeof(vt_layer_weights_ln) == 96 &&
              sizeof(vt_layer_weights_t) == 32 && sizeof(vt_layer_grads) == 96 && sizeof(vt_bwd_workspace) == 80 &&
              sizeof(vt_wgrad_problem) == 72, "struct layout of include/visitron_hip.h changed: bump the ABI");

extern "C" {

const char* vt_error_string(int code) {
  switch (code) {
    case VT_OK: return "ok";
    case VT_ERR_BAD_SHAPE: return "bad shape";
    case VT_ERR_BAD_ALIGN: return "bad alignment or leading dimension";
    case VT_ERR_NULL: return "null pointer";
    case VT_ERR_UNSUPPORTED: return "unsupported configuration";
    case VT_ERR_HIP: return "HIP launch error";
    default: return "unknown error";
  }
}

int vt_abi_version(void) { return 22; }

// deterministic training mode (common.hpp): one word for the process, read by every dispatch at launch time
void vt_set_deterministic(int on) { vt_deterministic_word().store(on ? 1 : 0, std::memory_order_relaxed); }
int vt_get_deterministic(void) { return vt_deterministic() ? 1 : 0; }
int64_t vt_attention_bwd_ws_bytes(int B, int S, int nh, int64_t rows) { return vt_attention_bwd_ws_bytes_impl(B, S, nh, (long)rows); }

// attention-probability dropout in 16-bit (default) or 8-bit fields: one word for the run (vt_attn_drop_bits_word, common.hpp)
int vt_set_attn_dropout_bits(int bits) {
  if (bits != 8 && bits != 16) return VT_ERR_UNSUPPORTED;
  vt_attn_drop_bits_word().store(bits, std::memory_order_relaxed);
  return VT_OK;
}
int vt_get_attn_dropout_bits(void) { return vt_attn_drop_bits(); }
float vt_attn_dropout_effective(float p) { return vt_attn_drop_ok(p, vt_attn_drop_bits()) ? vt_attn_drop_p(p, vt_attn_drop_bits()) : -1.0f; }

int vt_batch_row_counts(const int64_t* labels, const int64_t* token_labels, const float* mask, const int32_t* err_flag, int B,
                        int S, int64_t* counts, int32_t* tile_counts, vt_stream_t stream) {
  BatchRowsArgs a = {(const long*)labels, (const long*)token_labels, mask, (const int*)err_flag, (long)B * S, S, B, (long*)counts,
                     (int*)tile_counts, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
  return vt_batch_rows_dispatch(a, 0, (hipStream_t)stream);
}

int vt_batch_row_lists(const int64_t* labels, const int64_t* token_labels, const float* mask, int B, int S, int64_t n_w,
                       int64_t n_t, int64_t n_keep, const int32_t* tile_counts, int64_t* idx_w, int64_t* idx_t, int64_t* index,
                       int64_t* inverse, int32_t* start, int32_t* length, vt_stream_t stream) {
  BatchRowsArgs a = {(const long*)labels, (const long*)token_labels, mask, nullptr, (long)B * S, S, B, nullptr,
                     (int*)tile_counts, (long*)idx_w, (long*)idx_t, (long*)index, (long*)inverse, (int*)start, (int*)length, n_w,
                     n_t, n_keep};
  return vt_batch_rows_dispatch(a, 1, (hipStream_t)stream);
}

int vt_action_head_f32(const float* logits, int64_t ld, const int64_t* next_action, int B, int A, float grad_scale, void* dlogits,
                       int64_t ldd, int Ap, float* loss_acc, vt_stream_t stream) {
  return vt_action_head_dispatch(logits, ld, (const long*)next_action, B, A, grad_scale, dlogits, ldd, Ap, loss_acc, 0,
                                 (hipStream_t)stream);
}

int vt_linear_splitk_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, void* y, int64_t ldy, float* ws, int M, int N,
                          int K, int ksplit, vt_stream_t stream) {
  return vt_gemm_splitk_dispatch(x, ldx, w, ldw, y, ldy, ws, M, N, K, ksplit, (hipStream_t)stream);
}

int vt_embed_table_grad(const int32_t* sorted_ids, const int64_t* perm, const float* de, int64_t ld_de, float* grad,
                        int64_t ld_grad, int64_t n, int H, int64_t n_rows_table, int64_t skip_id, float* scratch, int32_t* flag,
                        vt_stream_t stream) {
  return vt_embed_table_grad_dispatch((const int*)sorted_ids, (const long*)perm, de, ld_de, grad, ld_grad, n, H, n_rows_table,
                                      skip_id, scratch, (int*)flag, (hipStream_t)stream);
}

void vt_debug_set_gemm_variant(int variant) { vt_gemm_set_variant(variant); }
void vt_debug_set_gemm_trace(void* buf) { vt_gemm_set_trace(buf); }
void vt_debug_set_wgrad_kernel(int mode) {
  // 0: automatic; 128 / 256: the 128(k)-tile kernel with that n-tile width; 8: the persistent kernel wherever it is eligible
  // (also below its row threshold); -8: never the persistent kernel
  vt_wgrad_set_tile(mode == 128 || mode == 256 || mode == 8 ? mode : 0);
  vt_wgrad_v8_enable(mode == -8 ? 0 : 1);
}
void vt_gemm_tune(int M, int N, int K, int kind, int variant) { vt_gemm_tune_set(M, N, K, kind, variant); }
void vt_debug_set_attn_bwd_waves(int waves) { vt_attn_bwd_set_waves(waves); }
void vt_gemm_reserve_cus(int k) { vt_gemm_set_reserved_cus(k); }
int vt_gemm_set_workspace(void* base, int64_t bytes) { return vt_gemm_set_workspace_impl(base, (long)bytes); }
int64_t vt_gemm_workspace_region_bytes(void) { return (int64_t)vt_gemm_workspace_region_bytes_impl(); }
int vt_gemm_shared_tile_timeouts(unsigned* host_count) {
  if (!host_count) return VT_ERR_NULL;
  return vt_gemm_shared_tile_timeouts_impl(host_count);
}

int vt_linear_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const void* R,
                   int64_t ldr, void* C, int64_t ldc, int M, int N, int K, int act, int out_f32, int grp_rows,
                   int grp_stride, vt_stream_t stream) {
  return vt_gemm_dispatch(A, lda, W, ldw, bias, R, ldr, C, ldc, M, N, K, act, out_f32, grp_rows, grp_stride,
                          (hipStream_t)stream);
}

int vt_linear_bf16_ex(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const void* R,
                      int64_t ldr, void* C, int64_t ldc, void* C2, int64_t ldc2, int M, int N, int K, int act,
                      int out_f32, int grp_rows, int grp_stride, float drop_p, uint64_t drop_seed, uint32_t drop_site,
                      vt_stream_t stream) {
  const DropCfg d = vt_make_drop(drop_p, drop_seed, drop_site);
  return vt_gemm_dispatch(A, lda, W, ldw, bias, R, ldr, C, ldc, M, N, K, act, out_f32, grp_rows, grp_stride,
                          (hipStream_t)stream, C2, ldc2, &d);
}

int vt_linear_lnres_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const void* Rv,
                         int64_t ldr, const float* mean, const float* rstd, const float* gamma, const float* beta, void* C,
                         int64_t ldc, int M, int N, int K, int out_f16, float drop_p, uint64_t drop_seed,
                         uint32_t drop_site, vt_stream_t stream) {
  if (!Rv) return VT_ERR_NULL;
  const DropCfg d = vt_make_drop(drop_p, drop_seed, drop_site);
  const VtLnResidual rln = {mean, rstd, gamma, beta};
  return vt_gemm_dispatch(A, lda, W, ldw, bias, Rv, ldr, C, ldc, M, N, K, VT_ACT_NONE, (out_f16 ? 2 : 0) | 4, 0, 0,
                          (hipStream_t)stream, nullptr, 0, &d, &rln);
}

int vt_apply_dropout_bf16(void* x, int64_t ld, int64_t rows, int cols, float drop_p, uint64_t drop_seed, uint32_t drop_site,
                          vt_stream_t stream) {
  return vt_apply_dropout_dispatch(x, ld, rows, cols, vt_make_drop(drop_p, drop_seed, drop_site), (hipStream_t)stream);
}

int vt_debug_dropout_mask(uint8_t* out, int64_t n, float drop_p, uint64_t drop_seed, uint32_t drop_site, int head_index,
                          vt_stream_t stream) {
  if (head_index >= 0) {   // attention sites: one stream per (b, h), a hash word per four keys, 8-bit thresholds (common.hpp)
    if (!vt_attn_drop_ok(drop_p, vt_attn_drop_bits())) return VT_ERR_UNSUPPORTED;
    DropCfg d = vt_make_drop_attn(drop_p, drop_seed, drop_site, vt_attn_drop_bits());
    d.seed = vt_hash32(d.seed, (uint32_t)head_index);
    return vt_dropout_mask_dispatch(out, n, d, (hipStream_t)stream, 1);
  }
  return vt_dropout_mask_dispatch(out, n, vt_make_drop(drop_p, drop_seed, drop_site), (hipStream_t)stream, 0);
}

int vt_attention_bwd_bf16(const void* qkv, int64_t ld_qkv, const void* dctx, int64_t ld_d, const void* ctx,
                          int64_t ld_ctx, const float* mask, int mask_additive, const float* lse, float* delta_ws,
                          void* dqkv, int64_t ld_dqkv, float* dq32_ws, int B, int S, int nh, int head_size,
                          float drop_p, uint64_t drop_seed, uint32_t drop_site, const uint32_t* keep_bits,
                          vt_stream_t stream) {
  if (!vt_attn_drop_ok(drop_p, vt_attn_drop_bits())) return VT_ERR_UNSUPPORTED;
  const DropCfg d = vt_make_drop_attn(drop_p, drop_seed, drop_site, vt_attn_drop_bits());
  return vt_attention_bwd_dispatch(qkv, ld_qkv, dctx, ld_d, ctx, ld_ctx, mask, mask_additive, lse, delta_ws, dqkv,
                                   ld_dqkv, dq32_ws, B, S, nh, head_size, (hipStream_t)stream, &d, nullptr, nullptr, 0,
                                   keep_bits);
}

int vt_attention_bwd_seq_bf16(const void* qkv, int64_t ld_qkv, const void* dctx, int64_t ld_d, const void* ctx,
                              int64_t ld_ctx, const float* lse, float* delta_ws, void* dqkv, int64_t ld_dqkv,
                              float* dq32_ws, int B, int S, int nh, int head_size, float drop_p, uint64_t drop_seed,
                              uint32_t drop_site, const int32_t* seq_start, const int32_t* seq_len, int64_t rows,
                              const uint32_t* keep_bits, vt_stream_t stream) {
  if (!seq_start || !seq_len) return VT_ERR_NULL;
  if (!vt_attn_drop_ok(drop_p, vt_attn_drop_bits())) return VT_ERR_UNSUPPORTED;
  const DropCfg d = vt_make_drop_attn(drop_p, drop_seed, drop_site, vt_attn_drop_bits());
  return vt_attention_bwd_dispatch(qkv, ld_qkv, dctx, ld_d, ctx, ld_ctx, nullptr, 0, lse, delta_ws, dqkv, ld_dqkv, dq32_ws,
                                   B, S, nh, head_size, (hipStream_t)stream, &d, seq_start, seq_len, rows, keep_bits);
}

int vt_layernorm_bwd_bf16(const void* x, int64_t ldx, const void* dy, int64_t ldy, const float* gamma, void* dx,
                          int64_t lddx, float* dgamma, float* dbeta, float* partial_ws, int M, int H, float eps,
                          int accumulate, void* dx_dropped, int64_t lddxd, float drop_p, uint64_t drop_seed,
                          uint32_t drop_site, vt_stream_t stream) {
  const DropCfg d = vt_make_drop(drop_p, drop_seed, drop_site);
  return vt_layernorm_bwd_dispatch(x, ldx, dy, ldy, gamma, dx, lddx, dgamma, dbeta, partial_ws, M, H, eps, accumulate,
                                   (hipStream_t)stream, dx_dropped, lddxd, &d);
}

int vt_layernorm_bwd_h_bf16(const void* x_f16, int64_t ldx, const void* dy, int64_t ldy, const float* gamma, void* dx,
                            int64_t lddx, float* dgamma, float* dbeta, float* partial_ws, int M, int H, float eps,
                            int accumulate, void* dx_dropped, int64_t lddxd, float drop_p, uint64_t drop_seed,
                            uint32_t drop_site, vt_stream_t stream) {
  const DropCfg d = vt_make_drop(drop_p, drop_seed, drop_site);
  return vt_layernorm_bwd_dispatch(x_f16, ldx, dy, ldy, gamma, dx, lddx, dgamma, dbeta, partial_ws, M, H, eps, accumulate,
                                   (hipStream_t)stream, dx_dropped, lddxd, &d, 1);
}

int vt_embed_layernorm_bwd(const int64_t* ids, const int64_t* type_ids, const int64_t* pos_ids, const float* word,
                           const float* pos, const float* type, const float* gamma, const void* g, int64_t ldg, float* de,
                           float* dgamma, float* dbeta, float* partial_ws, int B, int T, int S, int H, int n_word, int n_pos,
                           int n_type, float eps, int accumulate, float drop_p, uint64_t drop_seed, vt_stream_t stream) {
  const DropCfg d = vt_make_drop(drop_p, drop_seed, VT_SITE_EMB);
  return vt_embed_layernorm_bwd_dispatch(ids, type_ids, pos_ids, word, pos, type, gamma, g, ldg, de, dgamma, dbeta, partial_ws,
                                         B, T, S, H, n_word, n_pos, n_type, eps, accumulate, (hipStream_t)stream, &d);
}

int vt_adamw_flat(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float step_size, float b1,
                  float b2, float eps, float wd, float grad_scale, vt_stream_t stream) {
  return vt_adamw_dispatch(p, g, 0, m, v, p_bf16, n, lr, step_size, b1, b2, eps, wd, grad_scale, (hipStream_t)stream);
}

int vt_adamw_flat_g16(float* p, const void* g_bf16, float* m, float* v, void* p_bf16, int64_t n, float lr, float step_size,
                      float b1, float b2, float eps, float wd, float grad_scale, vt_stream_t stream) {
  return vt_adamw_dispatch(p, g_bf16, 1, m, v, p_bf16, n, lr, step_size, b1, b2, eps, wd, grad_scale, (hipStream_t)stream);
}

// ---- multi-tensor optimizer step, gradient norm and clip (ABI 14) --------------------------------------------------
int vt_multi_adam(const uint64_t* table, int64_t n_chunks, const float* hyper, float grad_coef, const float* grad_coef_dev,
                  vt_stream_t stream) {
  return vt_multi_adam_dispatch(table, n_chunks, hyper, grad_coef, grad_coef_dev, (hipStream_t)stream);
}

int vt_multi_sumsq(const uint64_t* table, int64_t n_chunks, void* partials, vt_stream_t stream) {
  return vt_multi_sumsq_dispatch(table, n_chunks, partials, (hipStream_t)stream);
}

int vt_norm_finish(const void* partials, int64_t n_chunks, float max_norm, float* out, vt_stream_t stream) {
  return vt_norm_finish_dispatch(partials, n_chunks, max_norm, out, (hipStream_t)stream);
}

int vt_multi_scale(const uint64_t* table, int64_t n_chunks, const float* coef_dev, vt_stream_t stream) {
  return vt_multi_scale_dispatch(table, n_chunks, coef_dev, (hipStream_t)stream);
}

// ---- AdamW sharded over data-parallel ranks (ABI 17) ------------------------------------------------------------------
int vt_shard_adamw(const uint64_t* table, const uint64_t* host_table, int64_t n_chunks, int g_is_bf16, float lr,
                   float step_size, float b1, float b2, float eps, float wd, float grad_scale, vt_stream_t stream) {
  return vt_shard_adamw_dispatch(table, host_table, n_chunks, g_is_bf16, lr, step_size, b1, b2, eps, wd, grad_scale,
                                 (hipStream_t)stream);
}

int vt_shard_settle(const uint64_t* table, const uint64_t* host_table, int64_t n_chunks, vt_stream_t stream) {
  return vt_shard_settle_dispatch(table, host_table, n_chunks, (hipStream_t)stream);
}

int vt_mask_tokens(const int64_t* input_ids, const uint8_t* special_mask, const int64_t* token_classes, const float* u_mask,
                   const float* u_replace, const float* u_random, const int64_t* random_words, int64_t* out_ids,
                   int64_t* labels, int64_t* attention_mask, int64_t n, int64_t pad_id, int64_t mask_id,
                   float mlm_probability, vt_stream_t stream) {
  return vt_mask_tokens_dispatch(input_ids, special_mask, token_classes, u_mask, u_replace, u_random, random_words, out_ids,
                                 labels, attention_mask, n, pad_id, mask_id, mlm_probability, (hipStream_t)stream);
}

int vt_assemble_regions(const float* img_feats, const int64_t* region_counts, const int64_t* region_view_ids,
                        const int64_t* current_view, const float* loc_table, const int64_t* text_labels,
                        const int64_t* text_mask, const int64_t* text_token_classes, float* feats_out, float* loc_out,
                        int64_t* labels_out, int64_t* mask_out, int64_t* token_labels_out, int B, int T, int R, int R_in,
                        int D, vt_stream_t stream) {
  return vt_assemble_regions_dispatch(img_feats, region_counts, region_view_ids, current_view, loc_table, text_labels,
                                      text_mask, text_token_classes, feats_out, loc_out, labels_out, mask_out,
                                      token_labels_out, B, T, R, R_in, D, (hipStream_t)stream);
}

int vt_scale_heads_bf16(const void* x, int64_t ldx, void* out, int64_t ldo, int64_t rows, int nh, const float* head_scale,
                        vt_stream_t stream) {
  return vt_scale_heads_dispatch(x, ldx, out, ldo, rows, nh, head_scale, (hipStream_t)stream);
}

int vt_cast_f32_to_bf16(const float* src, void* dst_bf16, int64_t n, float scale, vt_stream_t stream) {
  return vt_cast_scale_dispatch(src, dst_bf16, n, scale, (hipStream_t)stream);
}

int vt_ce_softmax_rows(const float* z, int64_t ldz, const int64_t* y, float* loss_row, int64_t* amax, void* dz, int64_t lddz,
                       int64_t rows, int V, int Vpad, float scale, vt_stream_t stream) {
  return vt_ce_softmax_dispatch(z, ldz, y, loss_row, amax, dz, lddz, rows, V, Vpad, scale, 0, (hipStream_t)stream);
}

int vt_ce_double_softmax_rows(const float* z, int64_t ldz, const int64_t* y, float* loss_row, int64_t* amax, void* dz,
                              int64_t lddz, int64_t rows, int V, int Vpad, float scale, vt_stream_t stream) {
  return vt_ce_double_softmax_dispatch(z, ldz, y, loss_row, amax, dz, lddz, rows, V, Vpad, scale, 0, (hipStream_t)stream);
}

int vt_lstm_step_train_f32(const float* xproj, int64_t ldx, const float* h_prev, float* h_out, float* c, const void* w_hh,
                           const int32_t* lengths, float* seq_out, int64_t ld_seq, int B, int hs, int t, float* sv_gates,
                           float* sv_c, void* sv_h, vt_stream_t stream) {
  LstmStepArgs a;
  a.xproj = xproj; a.ldx = ldx; a.h_prev = h_prev; a.h_out = h_out; a.c = c; a.w_hh = (const bf16_t*)w_hh;
  a.lengths = lengths; a.seq_out = seq_out; a.ld_seq = ld_seq; a.B = B; a.hs = hs; a.t = t;
  a.xrow_start = nullptr; a.ldx_row = 0;
  a.sv_gates = sv_gates; a.ld_svg = 4L * hs; a.sv_c = sv_c; a.ld_svc = hs; a.sv_h = (bf16_t*)sv_h; a.ld_svh = hs;
  return vt_lstm_step_dispatch(a, (hipStream_t)stream);
}

int vt_lstm_step_f32(const float* xproj, int64_t ldx, const float* h_prev, float* h_out, float* c, const void* w_hh,
                     const int32_t* lengths, float* seq_out, int64_t ld_seq, int B, int hs, int t, vt_stream_t stream) {
  return vt_lstm_step_train_f32(xproj, ldx, h_prev, h_out, c, w_hh, lengths, seq_out, ld_seq, B, hs, t, nullptr, nullptr,
                                nullptr, stream);
}

int vt_lstm_sequence_f32(const float* xproj, int64_t ldx_b, int64_t ldx_t, float* h2_0, float* h2_1, float* c,
                         const void* w_hh, const int32_t* lengths, float* seq_out, int64_t lds_b, int64_t lds_t,
                         int B, int hs, int T, int reverse, vt_stream_t stream) {
  return vt_lstm_sequence_dispatch(xproj, ldx_b, ldx_t, h2_0, h2_1, c, w_hh, lengths, seq_out, lds_b, lds_t, B, hs, T, reverse,
                                   (hipStream_t)stream, nullptr);
}

int vt_lstm_sequence_train_f32(const float* xproj, int64_t ldx_b, int64_t ldx_t, float* h2_0, float* h2_1, float* c,
                               const void* w_hh, const int32_t* lengths, float* seq_out, int64_t lds_b, int64_t lds_t,
                               int B, int hs, int T, int reverse, float* sv_gates, float* sv_c, void* sv_h, int64_t S_sv,
                               vt_stream_t stream) {
  if (!sv_gates || !sv_c || !sv_h) return VT_ERR_NULL;
  return vt_lstm_sequence_dispatch(xproj, ldx_b, ldx_t, h2_0, h2_1, c, w_hh, lengths, seq_out, lds_b, lds_t, B, hs, T, reverse,
                                   (hipStream_t)stream, nullptr, sv_gates, sv_c, sv_h, S_sv);
}

int vt_lstm_step_bwd_f32(const void* dg_next, int64_t ld_dgn, const void* w_hh_t, const float* dh_final, const float* d_out,
                         int64_t ld_dout, float* dc, const float* sv_gates, int64_t ld_svg, const float* sv_c,
                         int64_t ld_svc, void* dg_out, int64_t ld_dg, float* dg_out_f32, int64_t ld_dgf,
                         const int32_t* lengths, int B, int hs, int t, int t_next, vt_stream_t stream) {
  LstmBwdArgs a;
  a.dg_next = (const bf16_t*)dg_next; a.ld_dgn = ld_dgn; a.w_hh_t = (const bf16_t*)w_hh_t; a.dh_final = dh_final;
  a.d_out = d_out; a.ld_dout = ld_dout; a.dc = dc; a.sv_gates = sv_gates; a.ld_svg = ld_svg; a.sv_c = sv_c;
  a.ld_svc = ld_svc; a.dg_out = (bf16_t*)dg_out; a.ld_dg = ld_dg; a.dg_out_f32 = dg_out_f32; a.ld_dgf = ld_dgf;
  a.lengths = lengths; a.B = B; a.hs = hs; a.t = t; a.t_next = t_next;
  return vt_lstm_step_bwd_dispatch(a, (hipStream_t)stream);
}

int vt_lstm_sequence_bwd_f32(const float* d_seq_out, int64_t ldd_b, int64_t ldd_t, const float* dh_final, float* dc,
                             const void* w_hh_t, const int32_t* lengths, const float* sv_gates, const float* sv_c,
                             void* dgates, int64_t S_sv, int B, int hs, int T, int reverse, vt_stream_t stream) {
  return vt_lstm_sequence_bwd_dispatch(d_seq_out, ldd_b, ldd_t, dh_final, dc, w_hh_t, lengths, sv_gates, sv_c, dgates, S_sv, B,
                                       hs, T, reverse, (hipStream_t)stream);
}

int vt_lstm_sequence_rows_f32(const float* xproj, int64_t ldx_row, const int32_t* row_start, float* h2_0, float* h2_1,
                              float* c, const void* w_hh, const int32_t* lengths, float* seq_out, int64_t lds_b,
                              int64_t lds_t, int B, int hs, int T, int reverse, vt_stream_t stream) {
  if (!row_start) return VT_ERR_NULL;
  return vt_lstm_sequence_dispatch(xproj, 0, ldx_row, h2_0, h2_1, c, w_hh, lengths, seq_out, lds_b, lds_t, B, hs, T, reverse,
                                   (hipStream_t)stream, row_start);
}

int64_t vt_lstm_sequence_persistent_ws_bytes(int B, int hs) { return vt_lstm_persistent_ws_bytes(B, hs); }

int vt_lstm_sequence_persistent_f32(const float* xproj, int64_t ldx_b, int64_t ldx_t, const int32_t* row_start, float* h,
                                    float* c, const void* w_hh, const int32_t* lengths, float* seq_out, int64_t lds_b,
                                    int64_t lds_t, int B, int hs, int T, int reverse, void* ws, int64_t ws_bytes,
                                    vt_stream_t stream) {
  LstmPersistArgs a;
  a.xproj = xproj; a.ldx_b = ldx_b; a.ldx_t = ldx_t; a.xrow_start = row_start; a.h = h; a.c = c;
  a.w_hh = (const bf16_t*)w_hh; a.lengths = lengths; a.seq_out = seq_out; a.lds_b = lds_b; a.lds_t = lds_t;
  a.xchg = nullptr; a.sync = nullptr; a.B = B; a.hs = hs; a.T = T; a.reverse = reverse;
  return vt_lstm_persistent_dispatch(a, ws, ws_bytes, (hipStream_t)stream);
}

int vt_skinny_linear_f32(const float* x0, int64_t ld0, int K0, const float* x1, int64_t ld1, int K1, const void* w,
                         int64_t ldw, const float* bias, float* out, int64_t ldo, int M, int N, int Kpad, int act,
                         vt_stream_t stream) {
  SkinnyArgs a;
  a.x0 = x0; a.ld0 = ld0; a.K0 = K0; a.x1 = x1; a.ld1 = ld1; a.K1 = K1; a.w = (const bf16_t*)w; a.ldw = ldw;
  a.bias = bias; a.out = out; a.ldo = ldo; a.M = M; a.N = N; a.Kpad = Kpad; a.act = act;
  return vt_skinny_linear_dispatch(a, (hipStream_t)stream);
}

int vt_softdot_attention_bwd_f32(const float* target, const float* context, int64_t ld_batch, int64_t ld_row,
                                 const uint8_t* mask, const float* d_weighted, const float* d_attn, float* d_target,
                                 float* d_context, int B, int L, int D, int output_prob, vt_stream_t stream) {
  SoftDotBwdArgs a;
  a.target = target; a.context = context; a.ld_batch = ld_batch; a.ld_row = ld_row; a.mask = mask;
  a.d_weighted = d_weighted; a.d_attn = d_attn; a.d_target = d_target; a.d_context = d_context;
  a.B = B; a.L = L; a.D = D; a.output_prob = output_prob;
  return vt_softdot_bwd_dispatch(a, (hipStream_t)stream);
}

int64_t vt_softdot_attention_bwd_split_ws_floats(int B, int L, int D) { return vt_softdot_bwd_split_ws_floats(B, L, D); }

int vt_softdot_attention_bwd_split_f32(const float* target, const float* context, int64_t ld_batch, int64_t ld_row,
                                       const uint8_t* mask, const float* d_weighted, const float* d_attn, float* d_context,
                                       float* ws, int B, int L, int D, int output_prob, vt_stream_t stream) {
  SoftDotBwdArgs a;
  a.target = target; a.context = context; a.ld_batch = ld_batch; a.ld_row = ld_row; a.mask = mask;
  a.d_weighted = d_weighted; a.d_attn = d_attn; a.d_target = nullptr; a.d_context = d_context;
  a.B = B; a.L = L; a.D = D; a.output_prob = output_prob;
  return vt_softdot_bwd_split_dispatch(a, ws, (hipStream_t)stream);
}

int vt_softdot_attention_f32(const float* target, const float* context, int64_t ld_batch, int64_t ld_row,
                             const uint8_t* mask, float* weighted, float* attn, int B, int L, int D, int output_prob,
                             vt_stream_t stream) {
  SoftDotArgs a;
  a.target = target; a.context = context; a.ld_batch = ld_batch; a.ld_row = ld_row; a.mask = mask;
  a.weighted = weighted; a.attn = attn; a.B = B; a.L = L; a.D = D; a.output_prob = output_prob;
  return vt_softdot_dispatch(a, (hipStream_t)stream);
}

int vt_turn_lstm_cell_f32(const int64_t* ids, const float* table, int64_t ld_t, int A, const float* x_emb, int64_t ld_e, int E,
                          const float* feature, int64_t ld_f, int F, const float* h_prev, const float* c_prev, const void* w_ih,
                          int64_t ldw, int Kpad, const void* w_hh, const float* bias, float* h_out, float* c_out,
                          float* sv_gates, float* sv_c, void* sv_h, int32_t* err_flag, int B, int hs, vt_stream_t stream) {
  TbCellArgs a;
  a.ids = (const long*)ids; a.table = table; a.ld_t = ld_t; a.A = A; a.x_emb = x_emb; a.ld_e = ld_e; a.feature = feature;
  a.ld_f = ld_f; a.E = E; a.F = F; a.h_prev = h_prev; a.c_prev = c_prev; a.w_ih = (const bf16_t*)w_ih; a.ldw = ldw;
  a.Kpad = Kpad; a.w_hh = (const bf16_t*)w_hh; a.bias = bias; a.h_out = h_out; a.c_out = c_out; a.sv_gates = sv_gates;
  a.sv_c = sv_c; a.sv_h = (bf16_t*)sv_h; a.err = (int*)err_flag; a.B = B; a.hs = hs;
  return vt_tb_lstm_cell_dispatch(a, (hipStream_t)stream);
}

int vt_turn_action_head_f32(const float* logit, int64_t ld, const int64_t* target, const uint8_t* blocked, int64_t ld_blk,
                            int64_t ignore_index, int B, int A, int mode, uint32_t seed, float* loss, float* count,
                            int64_t* a_t, int32_t* err_flag, vt_stream_t stream) {
  TbHeadArgs a;
  a.logit = logit; a.ld = ld; a.target = (const long*)target; a.blocked = blocked; a.ld_blk = ld_blk;
  a.ignore_index = ignore_index; a.B = B; a.A = A; a.mode = mode; a.seed = seed; a.loss = loss; a.count = count;
  a.a_t = (long*)a_t; a.err = (int*)err_flag;
  return vt_tb_action_head_dispatch(a, (hipStream_t)stream);
}

int vt_turn_action_head_bwd_f32(const float* logit, int64_t ld, const int64_t* target, const uint8_t* blocked, int64_t ld_blk,
                                int64_t ignore_index, int B, int A, const float* g, const float* count, float* dlogit,
                                int64_t ld_d, vt_stream_t stream) {
  TbHeadBwdArgs a;
  a.logit = logit; a.ld = ld; a.target = (const long*)target; a.blocked = blocked; a.ld_blk = ld_blk;
  a.ignore_index = ignore_index; a.B = B; a.A = A; a.g = g; a.count = count; a.dlogit = dlogit; a.ld_d = ld_d;
  return vt_tb_action_head_bwd_dispatch(a, (hipStream_t)stream);
}

int vt_obs_gather_f32(const float* store, int64_t N, int V, int D, const float* table, const void* record, int B, int Cmax,
                      float* input_a_t, float* f_t, float* candidate_feat, int32_t* candidate_leng, uint8_t* candidate_mask,
                      int32_t* err_flag, vt_stream_t stream) {
  if (!record) return VT_ERR_NULL;
  if (B <= 0 || Cmax < 1) return VT_ERR_BAD_SHAPE;
  if (((uintptr_t)record) & 7) return VT_ERR_BAD_ALIGN;
  // the record's layout (include/visitron_hip.h): int32 rows[B][3], int32 cand_point[B][Cmax], then the doubles, 8-byte aligned
  const char* rec = (const char*)record;
  const long nb = (long)B, nc = (long)B * Cmax;
  const long off_f64 = (12 * nb + 4 * nc + 7) & ~7L;
  ObsGatherArgs a;
  a.store = store; a.N = N; a.V = V; a.D = D; a.table = table;
  a.rows = (const int*)rec; a.pts = (const int*)(rec + 12 * nb);
  a.agent = (const double*)(rec + off_f64); a.cand_h = a.agent + 2 * nb; a.cand_e = a.cand_h + nc;
  a.B = B; a.Cmax = Cmax; a.a_t = input_a_t; a.f_t = f_t; a.cand = candidate_feat; a.leng = (int*)candidate_leng;
  a.mask = candidate_mask; a.err = (int*)err_flag;
  return vt_obs_gather_dispatch(a, (hipStream_t)stream);
}

int vt_obs_gather_view_f32(const float* store, int64_t N, int V, int D, const int32_t* rows, int B, float* out,
                           int64_t ld_out, int32_t* err_flag, vt_stream_t stream) {
  ObsViewArgs a;
  a.store = store; a.N = N; a.V = V; a.D = D; a.rows = (const int*)rows; a.B = B; a.out = out; a.ld_out = ld_out;
  a.err = (int*)err_flag;
  return vt_obs_gather_view_dispatch(a, (hipStream_t)stream);
}

static RegionGatherArgs region_args(const void* store, int store_bf16, int64_t N, int V, int P, int D, const uint8_t* counts,
                                    const float* loc_table, const int32_t* rows, const int64_t* text_labels,
                                    const int64_t* text_mask, const int64_t* text_token_classes, int B, int T, int R,
                                    int64_t* labels_out, int64_t* mask_out, int64_t* token_labels_out, int32_t* err_flag) {
  RegionGatherArgs a;
  a.store = store; a.store_bf16 = store_bf16; a.N = N; a.V = V; a.P = P; a.D = D; a.counts = counts; a.loc_table = loc_table;
  a.rows = (const int*)rows; a.text_labels = (const long*)text_labels; a.text_mask = (const long*)text_mask;
  a.text_token_classes = (const long*)text_token_classes; a.B = B; a.T = T; a.R = R;
  a.feats = nullptr; a.loc = nullptr; a.packed = nullptr; a.kpad = 0;
  a.labels = (long*)labels_out; a.mask = (long*)mask_out; a.token_labels = (long*)token_labels_out; a.err = (int*)err_flag;
  return a;
}

int vt_region_gather_f32(const void* store, int store_bf16, int64_t N, int V, int P, int D, const uint8_t* counts,
                         const float* loc_table, const int32_t* rows, const int64_t* text_labels, const int64_t* text_mask,
                         const int64_t* text_token_classes, int B, int T, int R, float* feats_out, float* loc_out,
                         int64_t* labels_out, int64_t* mask_out, int64_t* token_labels_out, int32_t* err_flag,
                         vt_stream_t stream) {
  RegionGatherArgs a = region_args(store, store_bf16, N, V, P, D, counts, loc_table, rows, text_labels, text_mask,
                                   text_token_classes, B, T, R, labels_out, mask_out, token_labels_out, err_flag);
  if (R > 0 && (!feats_out || !loc_out)) return VT_ERR_NULL;
  a.feats = feats_out; a.loc = loc_out;
  return vt_region_gather_dispatch(a, (hipStream_t)stream);
}

int vt_region_gather_pack_bf16(const void* store, int store_bf16, int64_t N, int V, int P, int D, const uint8_t* counts,
                               const float* loc_table, const int32_t* rows, const int64_t* text_labels,
                               const int64_t* text_mask, const int64_t* text_token_classes, int B, int T, int R,
                               void* packed_out, int kpad, int64_t* labels_out, int64_t* mask_out,
                               int64_t* token_labels_out, int32_t* err_flag, vt_stream_t stream) {
  RegionGatherArgs a = region_args(store, store_bf16, N, V, P, D, counts, loc_table, rows, text_labels, text_mask,
                                   text_token_classes, B, T, R, labels_out, mask_out, token_labels_out, err_flag);
  if (R > 0 && !packed_out) return VT_ERR_NULL;
  if (kpad < 8) return VT_ERR_BAD_SHAPE;
  a.packed = packed_out; a.kpad = kpad;
  return vt_region_gather_dispatch(a, (hipStream_t)stream);
}

int vt_transpose_bf16(const void* in, int64_t ldi, void* out, int64_t ldo, int R, int C, vt_stream_t stream) {
  return vt_transpose_dispatch(in, ldi, out, ldo, R, C, (hipStream_t)stream);
}

int vt_transpose_batch_bf16(const void* const* in, const int64_t* ldi, void* const* out, const int64_t* ldo, const int* R,
                            const int* C, int n, vt_stream_t stream) {
  return vt_transpose_batch_dispatch(in, (const long*)ldi, out, (const long*)ldo, R, C, n, (hipStream_t)stream);
}

int vt_dgelu_mul_bf16(const void* g, const void* h, void* out, int64_t n, vt_stream_t stream) {
  return vt_dgelu_mul_dispatch(g, h, out, n, (hipStream_t)stream);
}

int vt_attention_fwd_bf16(const void* qkv, int64_t ld_qkv, const float* mask, int mask_additive, const float* head_scale, void* ctx,
                          int64_t ld_ctx, float* lse, int B, int S, int nh, int head_size, float drop_p, uint64_t drop_seed,
                          uint32_t drop_site, uint32_t* keep_bits, vt_stream_t stream) {
  if (!vt_attn_drop_ok(drop_p, vt_attn_drop_bits())) return VT_ERR_UNSUPPORTED;
  const DropCfg d = vt_make_drop_attn(drop_p, drop_seed, drop_site, vt_attn_drop_bits());
  return vt_attention_fwd_dispatch(qkv, ld_qkv, mask, mask_additive, head_scale, ctx, ld_ctx, lse, B, S, nh, head_size,
                                   (hipStream_t)stream, &d, nullptr, nullptr, keep_bits);
}

int vt_attention_fwd_seq_bf16(const void* qkv, int64_t ld_qkv, const float* head_scale, void* ctx, int64_t ld_ctx,
                              float* lse, int B, int S, int nh, int head_size, float drop_p, uint64_t drop_seed,
                              uint32_t drop_site, const int32_t* seq_start, const int32_t* seq_len, uint32_t* keep_bits,
                              vt_stream_t stream) {
  if (!seq_start || !seq_len) return VT_ERR_NULL;
  if (!vt_attn_drop_ok(drop_p, vt_attn_drop_bits())) return VT_ERR_UNSUPPORTED;
  const DropCfg d = vt_make_drop_attn(drop_p, drop_seed, drop_site, vt_attn_drop_bits());
  return vt_attention_fwd_dispatch(qkv, ld_qkv, nullptr, 0, head_scale, ctx, ld_ctx, lse, B, S, nh, head_size,
                                   (hipStream_t)stream, &d, seq_start, seq_len, keep_bits);
}

int vt_attention_rect_fwd_bf16(const void* qkv, int64_t ld_qkv, const float* mask, int mask_additive, const float* head_scale,
                               void* ctx, int64_t ld_ctx, float* lse, int B, int Sq, int Sk, int nh, int head_size, float drop_p,
                               uint64_t drop_seed, uint32_t drop_site, uint32_t* keep_bits, vt_stream_t stream) {
  if (!vt_attn_drop_ok(drop_p, vt_attn_drop_bits())) return VT_ERR_UNSUPPORTED;
  const DropCfg d = vt_make_drop_attn(drop_p, drop_seed, drop_site, vt_attn_drop_bits());
  return vt_attention_rect_fwd_dispatch(qkv, ld_qkv, mask, mask_additive, head_scale, ctx, ld_ctx, lse, B, Sq, Sk, nh, head_size,
                                        d, keep_bits, (hipStream_t)stream);
}

int vt_attention_rect_bwd_bf16(const void* qkv, int64_t ld_qkv, const void* dctx, int64_t ld_d, const void* ctx, int64_t ld_ctx,
                               const float* mask, int mask_additive, const float* lse, void* dqkv, int64_t ld_dqkv, int B,
                               int Sq, int Sk, int nh, int head_size, float drop_p, uint64_t drop_seed, uint32_t drop_site,
                               const uint32_t* keep_bits, vt_stream_t stream) {
  if (!vt_attn_drop_ok(drop_p, vt_attn_drop_bits())) return VT_ERR_UNSUPPORTED;
  const DropCfg d = vt_make_drop_attn(drop_p, drop_seed, drop_site, vt_attn_drop_bits());
  return vt_attention_rect_bwd_dispatch(qkv, ld_qkv, dctx, ld_d, ctx, ld_ctx, mask, mask_additive, lse, dqkv, ld_dqkv, B, Sq, Sk,
                                        nh, head_size, d, keep_bits, (hipStream_t)stream);
}

int vt_attention_probs_f32(const void* qkv, int64_t ld_qkv, const float* mask, int mask_additive, const float* head_scale,
                           const float* lse, float* probs, int B, int S, int nh, int head_size, vt_stream_t stream) {
  return vt_attention_probs_dispatch(qkv, ld_qkv, mask, mask_additive, head_scale, lse, probs, B, S, nh, head_size,
                                     (hipStream_t)stream);
}

int vt_layernorm_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, const float* gamma, const float* beta,
                      float* mean, float* rstd, int M, int H, float eps, int grp_rows, int grp_stride,
                      vt_stream_t stream) {
  return vt_layernorm_dispatch(x, ldx, y, ldy, gamma, beta, mean, rstd, M, H, eps, grp_rows, grp_stride,
                               (hipStream_t)stream);
}

int vt_layernorm_h_bf16(const void* x_f16, int64_t ldx, void* y, int64_t ldy, void* y_f16, int64_t ldyh, const float* gamma,
                        const float* beta, float* mean, float* rstd, int M, int H, float eps, vt_stream_t stream) {
  return vt_layernorm_dispatch(x_f16, ldx, y, ldy, gamma, beta, mean, rstd, M, H, eps, 0, 0, (hipStream_t)stream, 1, y_f16, ldyh);
}

int vt_embed_layernorm(const int64_t* ids, const int64_t* type_ids, const int64_t* pos_ids, const float* word,
                       const float* pos, const float* type, const float* gamma, const float* beta, void* y,
                       int64_t ldy, int B, int T, int S, int H, int n_word, int n_pos, int n_type, float eps,
                       int* err_flag, float drop_p, uint64_t drop_seed, vt_stream_t stream) {
  const DropCfg d = vt_make_drop(drop_p, drop_seed, VT_SITE_EMB);
  return vt_embed_layernorm_dispatch(ids, type_ids, pos_ids, word, pos, type, gamma, beta, y, ldy, B, T, S, H, n_word,
                                     n_pos, n_type, eps, err_flag, (hipStream_t)stream, &d);
}

int vt_pack_concat_bf16(const float* s0, int d0, const float* s1, int d1, void* out, int kpad, int64_t rows,
                        vt_stream_t stream) {
  return vt_pack_concat_dispatch(s0, d0, s1, d1, out, kpad, rows, (hipStream_t)stream);
}

int vt_center_mask(const void* mask, int kind, int64_t ldm, float* out, int B, int S, vt_stream_t stream) {
  return vt_center_mask_dispatch(mask, kind, ldm, out, B, S, (hipStream_t)stream);
}

// ---- fp32 parity path (fp32_path.hip) ----------------------------------------------------------------------------
int vt_linear_f32(const float* a, int64_t lda, const float* w, int64_t ldw, int w_is_kn, const float* bias,
                  const float* residual, int64_t ldr, float* out, int64_t ldc, int M, int N, int K, int act, float alpha,
                  int grp_rows, int grp_stride, vt_stream_t stream) {
  return vt_gemm_f32_dispatch(a, lda, 0, 0, w, ldw, 0, 0, w_is_kn, bias, residual, ldr, out, ldc, 0, 0, M, N, K, act, alpha,
                              1, 1, grp_rows, grp_stride, (hipStream_t)stream);
}

int vt_bmm_f32(const float* a, int64_t lda, int64_t a_stride_b, int64_t a_stride_h, const float* w, int64_t ldw,
               int64_t w_stride_b, int64_t w_stride_h, int w_is_kn, float* out, int64_t ldc, int64_t c_stride_b,
               int64_t c_stride_h, int M, int N, int K, float alpha, int batch, int heads, vt_stream_t stream) {
  return vt_gemm_f32_dispatch(a, lda, a_stride_b, a_stride_h, w, ldw, w_stride_b, w_stride_h, w_is_kn, nullptr, nullptr, 0,
                              out, ldc, c_stride_b, c_stride_h, M, N, K, VT_ACT_NONE, alpha, batch, heads, 0, 0,
                              (hipStream_t)stream);
}

int vt_linear_bf16x3(const float* a, int64_t lda, const float* w, int64_t ldw, int w_is_kn, const float* bias,
                     const float* residual, int64_t ldr, float* out, int64_t ldc, int M, int N, int K, int act, float alpha,
                     int grp_rows, int grp_stride, vt_stream_t stream) {
  return vt_gemm_bf16x3_dispatch(a, lda, 0, 0, w, ldw, 0, 0, w_is_kn, bias, residual, ldr, out, ldc, 0, 0, M, N, K, act, alpha,
                                 1, 1, grp_rows, grp_stride, (hipStream_t)stream);
}

int vt_bmm_bf16x3(const float* a, int64_t lda, int64_t a_stride_b, int64_t a_stride_h, const float* w, int64_t ldw,
                  int64_t w_stride_b, int64_t w_stride_h, int w_is_kn, float* out, int64_t ldc, int64_t c_stride_b,
                  int64_t c_stride_h, int M, int N, int K, float alpha, int batch, int heads, vt_stream_t stream) {
  return vt_gemm_bf16x3_dispatch(a, lda, a_stride_b, a_stride_h, w, ldw, w_stride_b, w_stride_h, w_is_kn, nullptr, nullptr, 0,
                                 out, ldc, c_stride_b, c_stride_h, M, N, K, VT_ACT_NONE, alpha, batch, heads, 0, 0,
                                 (hipStream_t)stream);
}

int vt_softmax_rows_f32(float* x, int64_t ld, int64_t rows, int cols, float scale, const float* mask, int mask_mode,
                        const float* head_scale, int nh, int S, vt_stream_t stream) {
  return vt_softmax_rows_f32_dispatch(x, ld, rows, cols, scale, mask, mask_mode, head_scale, nh, S, (hipStream_t)stream);
}

int vt_layernorm_rows(const void* x, int64_t ldx, int x_is_f32, void* y, int64_t ldy, int y_is_f32, const float* gamma,
                      const float* beta, int64_t M, int H, float eps, int grp_rows, int grp_stride, vt_stream_t stream) {
  return vt_layernorm_f32_dispatch(x, ldx, x_is_f32, y, ldy, y_is_f32, gamma, beta, M, H, eps, grp_rows, grp_stride,
                                   (hipStream_t)stream);
}

int vt_embed_layernorm_f32(const int64_t* input_ids, const int64_t* token_type_ids, const int64_t* position_ids,
                           const float* word, const float* pos, const float* type, const float* gamma, const float* beta,
                           float* out, int64_t ld_out, int B, int T, int S, int H, int n_word, int n_pos, int n_type,
                           float eps, int* err_flag, vt_stream_t stream) {
  return vt_embed_layernorm_f32_dispatch(input_ids, token_type_ids, position_ids, word, pos, type, gamma, beta, out, ld_out,
                                         B, T, S, H, n_word, n_pos, n_type, eps, err_flag, (hipStream_t)stream);
}

// ---- fp32 training step (ABI 13) ---------------------------------------------------------------------------------
int vt_gemm_f32_ex(const float* a, int64_t lda, int64_t a_stride_b, int64_t a_stride_h, int a_is_km, const float* w,
                   int64_t ldw, int64_t w_stride_b, int64_t w_stride_h, int w_is_kn, const float* bias, const float* residual,
                   int64_t ldr, float* out, int64_t ldc, int64_t c_stride_b, int64_t c_stride_h, float* pre_act, int M, int N,
                   int K, int act, float alpha, int batch, int heads, int grp_rows, int grp_stride, int accumulate, int split,
                   float* split_ws, float drop_p, uint64_t drop_seed, uint32_t drop_site, vt_stream_t stream) {
  if (!(drop_p >= 0.f && drop_p < 1.f)) return VT_ERR_UNSUPPORTED;
  return vt_gemm_f32_ex_dispatch(a, lda, a_stride_b, a_stride_h, a_is_km, w, ldw, w_stride_b, w_stride_h, w_is_kn, bias, residual,
                                 ldr, out, ldc, c_stride_b, c_stride_h, pre_act, M, N, K, act, alpha, batch, heads, grp_rows,
                                 grp_stride, accumulate, split, split_ws, vt_make_drop(drop_p, drop_seed, drop_site),
                                 (hipStream_t)stream);
}

int vt_gemm_f32_split_count(int M, int N, int K) { return vt_gemm_f32_split_for(M, N, K); }

int vt_colsum_f32(const float* x, int64_t ldx, int64_t rows, int cols, float* out, int accumulate, float* ws,
                  vt_stream_t stream) {
  return vt_colsum_f32_dispatch(x, ldx, rows, cols, out, accumulate, ws, (hipStream_t)stream);
}

int64_t vt_layernorm_bwd_f32_ws_floats(int64_t M, int H) {
  const long nb = vt_ln_bwd_f32_blocks(M);
  return nb * 2L * H + 2L * ((nb + 255) / 256) * H;
}

int vt_layernorm_bwd_f32(const float* x, int64_t ldx, const float* g, int64_t ldg, int grp_rows, int grp_stride,
                         const float* gamma, float eps, float* dx, int64_t lddx, float* dx_drop, int64_t ldd, float* dgamma,
                         float* dbeta, int accumulate, float* ws, int64_t M, int H, float p_in, uint32_t site_in, float p_out,
                         uint32_t site_out, uint64_t drop_seed, vt_stream_t stream) {
  if (!dgamma || !dbeta || !ws) return VT_ERR_NULL;
  if (!(p_in >= 0.f && p_in < 1.f && p_out >= 0.f && p_out < 1.f)) return VT_ERR_UNSUPPORTED;
  const long nb = vt_ln_bwd_f32_blocks(M);
  float* partial = ws;
  float* cws = ws + nb * 2L * H;
  int rc = vt_ln_bwd_f32_dispatch(x, ldx, g, ldg, grp_rows, grp_stride, gamma, dx, lddx, dx_drop, ldd, partial, M, H, eps,
                                  vt_make_drop(p_in, drop_seed, site_in), vt_make_drop(p_out, drop_seed, site_out),
                                  (hipStream_t)stream);
  if (rc == VT_OK) rc = vt_colsum_f32_dispatch(partial, 2L * H, nb, H, dgamma, accumulate, cws, (hipStream_t)stream);
  if (rc == VT_OK) rc = vt_colsum_f32_dispatch(partial + H, 2L * H, nb, H, dbeta, accumulate, cws + ((nb + 255) / 256) * H,
                                               (hipStream_t)stream);
  return rc;
}

int vt_layernorm_drop_f32(const float* x, int64_t ldx, float* y, int64_t ldy, const float* gamma, const float* beta, int64_t M,
                          int H, float eps, int grp_rows, int grp_stride, float drop_p, uint64_t drop_seed, uint32_t drop_site,
                          vt_stream_t stream) {
  if (!(drop_p >= 0.f && drop_p < 1.f)) return VT_ERR_UNSUPPORTED;
  return vt_layernorm_f32_drop_dispatch(x, ldx, 1, y, ldy, 1, gamma, beta, M, H, eps, grp_rows, grp_stride,
                                        vt_make_drop(drop_p, drop_seed, drop_site), (hipStream_t)stream, 1);
}

int vt_attn_softmax_train_f32(int backward, float* probs, float* probs_dropped, int64_t ld, int B, int nh, int S, float scale,
                              const float* mask, int mask_mode, const float* head_scale, float drop_p, uint64_t drop_seed,
                              uint32_t drop_site, vt_stream_t stream) {
  if (!vt_attn_drop_ok(drop_p, vt_attn_drop_bits())) return VT_ERR_UNSUPPORTED;
  return vt_attn_softmax_f32_dispatch(backward, probs, probs_dropped, ld, B, nh, S, scale, mask, mask_mode, head_scale,
                                      vt_make_drop_attn(drop_p, drop_seed, drop_site, vt_attn_drop_bits()), (hipStream_t)stream);
}

int vt_dgelu_f32(const float* g, const float* pre, float* out, int64_t n, vt_stream_t stream) {
  return vt_dgelu_f32_dispatch(g, pre, out, n, (hipStream_t)stream);
}

int vt_embed_sum_f32(const int64_t* input_ids, const int64_t* token_type_ids, const int64_t* position_ids, const float* word,
                     const float* pos, const float* type, float* out, int B, int T, int H, int n_word, int n_pos, int n_type,
                     int* err_flag, vt_stream_t stream) {
  return vt_embed_sum_f32_dispatch(input_ids, token_type_ids, position_ids, word, pos, type, out, B, T, H, n_word, n_pos, n_type,
                                   err_flag, (hipStream_t)stream);
}

int vt_dropout_rows_f32(const float* x, int64_t ldx, int grp_rows, int grp_stride, float* y, int64_t ldy, int64_t rows, int cols,
                        float drop_p, uint64_t drop_seed, uint32_t drop_site, vt_stream_t stream) {
  if (!(drop_p >= 0.f && drop_p < 1.f)) return VT_ERR_UNSUPPORTED;
  return vt_dropout_rows_f32_dispatch(x, ldx, grp_rows, grp_stride, y, ldy, rows, cols, vt_make_drop(drop_p, drop_seed, drop_site),
                                      (hipStream_t)stream);
}

int vt_ce_softmax_rows_g32(const float* z, int64_t ldz, const int64_t* y, float* loss_row, int64_t* amax, float* dz, int64_t lddz,
                           int64_t rows, int V, int Vpad, float scale, vt_stream_t stream) {
  return vt_ce_softmax_dispatch(z, ldz, y, loss_row, amax, dz, lddz, rows, V, Vpad, scale, 1, (hipStream_t)stream);
}

int vt_ce_double_softmax_rows_g32(const float* z, int64_t ldz, const int64_t* y, float* loss_row, int64_t* amax, float* dz,
                                  int64_t lddz, int64_t rows, int V, int Vpad, float scale, vt_stream_t stream) {
  return vt_ce_double_softmax_dispatch(z, ldz, y, loss_row, amax, dz, lddz, rows, V, Vpad, scale, 1, (hipStream_t)stream);
}

int vt_action_head_g32(const float* logits, int64_t ld, const int64_t* next_action, int B, int A, float grad_scale, float* dlogits,
                       int64_t ldd, int Ap, float* loss_acc, vt_stream_t stream) {
  return vt_action_head_dispatch(logits, ld, (const long*)next_action, B, A, grad_scale, dlogits, ldd, Ap, loss_acc, 1,
                                 (hipStream_t)stream);
}

// the two bounded-wait counters of the current device in one launch (gemm_wgrad_v8.hip)
int vt_step_counters(int64_t* out2, vt_stream_t stream) { return vt_step_counters_dispatch((long long*)out2, (hipStream_t)stream); }

int vt_wgrad_turn_timeouts(unsigned* host_count) {
  if (!host_count) return VT_ERR_NULL;
  return vt_wgrad_v8_timeouts(host_count);
}

int vt_wgrad_bf16(const vt_wgrad_problem* problems, int nprob, int M, vt_stream_t stream) {
  if (!problems) return VT_ERR_NULL;
  if (nprob <= 0 || nprob > WG_MAX_PROBLEMS) return VT_ERR_BAD_SHAPE;
  WgradArgs a;
  a.nprob = nprob;
  a.M = M;
  for (int i = 0; i < nprob; ++i) {
    const vt_wgrad_problem& q = problems[i];
    WgradProblem& P = a.p[i];
    P.dY = (const bf16_t*)q.dY; P.ldy = q.ldy; P.X = (const bf16_t*)q.X; P.ldx = q.ldx;
    P.dW = q.dW; P.ldw = q.ldw; P.db = q.db; P.N = q.N; P.K = q.K; P.accumulate = q.accumulate;
    P.tiles_k = 0; P.tile_begin = 0;
  }
  for (int i = nprob; i < WG_MAX_PROBLEMS; ++i) a.p[i] = a.p[0];
  return vt_wgrad_dispatch(a, (hipStream_t)stream);
}

// ---- deferred-LayerNorm inference path ------------------------------------------------------------------------------
int vt_linear_ln_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* colv,
                      const float* stats_in, int np, int64_t stat_rows, float ln_eps, int ln_mode, const void* R_f16,
                      int64_t ldrs, void* C, int64_t ldc, void* C_f16, int64_t ldcs, float* stats_out, int M, int N, int K,
                      int act, vt_stream_t stream) {
  return vt_gemm_ln_dispatch(A, lda, W, ldw, bias, colv, stats_in, np, stat_rows, ln_eps, ln_mode, R_f16, ldrs, C, ldc, C_f16,
                             ldcs, stats_out, M, N, K, act, (hipStream_t)stream);
}

int vt_ln_apply(const void* v, int64_t ldv, const float* stats, int np, int64_t stat_rows, const float* gamma,
                const float* beta, float ln_eps, void* y_bf16, int64_t ldy16, float* y_f32, int64_t ldy32, int64_t M, int H,
                vt_stream_t stream) {
  return vt_ln_apply_dispatch(v, ldv, stats, np, stat_rows, gamma, beta, ln_eps, y_bf16, ldy16, y_f32, ldy32, M, H,
                              (hipStream_t)stream);
}

int vt_ln_stream_init(const float* x, int64_t ldx, void* x_f16, int64_t lds, void* x_bf16, int64_t ldy, float* stats, int np,
                      int64_t stat_rows, int64_t M, int H, float ln_eps, vt_stream_t stream) {
  return vt_ln_stream_init_dispatch(x, ldx, x_f16, lds, x_bf16, ldy, stats, np, stat_rows, M, H, ln_eps, (hipStream_t)stream);
}

// ---- the encoder stack's layer loops (encoder_loops.hip) --------------------------------------------------------------
int vt_encoder_forward_ln_bf16(const vt_layer_weights_ln* layers, int num_layers, void* s16_a, void* sf_a, float* stats_a,
                               void* s16_b, void* sf_b, float* stats_b, void* qkv, void* ctx, void* mid, const float* mask,
                               int mask_additive, const float* head_scale, int B, int S, int H, int nh, int I, float ln_eps,
                               int64_t stat_rows, vt_stream_t stream) {
  return vt_encoder_forward_ln_dispatch(layers, num_layers, s16_a, sf_a, stats_a, s16_b, sf_b, stats_b, qkv, ctx, mid, mask,
                                        mask_additive, head_scale, B, S, H, nh, I, ln_eps, stat_rows, (hipStream_t)stream, 0,
                                        nullptr, nullptr);
}

int vt_encoder_forward_ln_seq_bf16(const vt_layer_weights_ln* layers, int num_layers, void* s16_a, void* sf_a, float* stats_a,
                                   void* s16_b, void* sf_b, float* stats_b, void* qkv, void* ctx, void* mid,
                                   const float* head_scale, int B, int S, int H, int nh, int I, float ln_eps, int64_t stat_rows,
                                   int64_t rows, const int32_t* seq_start, const int32_t* seq_len, vt_stream_t stream) {
  if (rows <= 0) return VT_ERR_BAD_SHAPE;
  return vt_encoder_forward_ln_dispatch(layers, num_layers, s16_a, sf_a, stats_a, s16_b, sf_b, stats_b, qkv, ctx, mid, nullptr,
                                        0, head_scale, B, S, H, nh, I, ln_eps, stat_rows, (hipStream_t)stream, (long)rows,
                                        seq_start, seq_len);
}

int vt_encoder_forward_bf16(const vt_layer_weights* layers, const vt_layer_acts* acts, int num_layers, const void* x,
                            const float* mask, int mask_additive, const float* head_scale, int B, int S, int H, int nh,
                            int I, float ln_eps, float p_hidden, float p_attn, uint64_t drop_seed, vt_stream_t stream) {
  return vt_encoder_forward_dispatch(layers, acts, num_layers, x, mask, mask_additive, head_scale, B, S, H, nh, I, ln_eps,
                                     p_hidden, p_attn, drop_seed, (hipStream_t)stream, 0, nullptr, nullptr);
}

int vt_encoder_forward_seq_bf16(const vt_layer_weights* layers, const vt_layer_acts* acts, int num_layers, const void* x,
                                const float* head_scale, int B, int S, int H, int nh, int I, float ln_eps, float p_hidden,
                                float p_attn, uint64_t drop_seed, int64_t rows, const int32_t* seq_start,
                                const int32_t* seq_len, vt_stream_t stream) {
  if (rows <= 0) return VT_ERR_BAD_SHAPE;
  return vt_encoder_forward_dispatch(layers, acts, num_layers, x, nullptr, 0, head_scale, B, S, H, nh, I, ln_eps, p_hidden,
                                     p_attn, drop_seed, (hipStream_t)stream, (long)rows, seq_start, seq_len);
}

// Weight prefetch of the layer loops: training 0 off, 4 (default) in the LayerNorm kernels' spare workgroups; inference 0 off,
// 3 (default) in the attention kernel's spare workgroups.  -1 keeps a setting; any other number is refused.
int vt_set_weight_prefetch(int training_mode, int inference_mode) { return vt_weight_prefetch_set(training_mode, inference_mode); }
int vt_get_weight_prefetch(int inference) { return vt_weight_prefetch_get(inference); }

int vt_encoder_backward_bf16(const vt_layer_weights* layers, const vt_layer_weights_t* layers_t,
                             const vt_layer_acts* acts, const vt_layer_grads* grads, int num_layers, const void* x,
                             const float* mask, int mask_additive, void* g, const vt_bwd_workspace* ws, int B, int S,
                             int H, int nh, int I, float ln_eps, int accumulate, float p_hidden, float p_attn,
                             uint64_t drop_seed, int layer0, vt_stream_t stream) {
  return vt_encoder_backward_dispatch(layers, layers_t, acts, grads, num_layers, x, mask, mask_additive, g, ws, nullptr, B, S,
                                      H, nh, I, ln_eps, accumulate, p_hidden, p_attn, drop_seed, layer0, (hipStream_t)stream,
                                      nullptr);
}

int vt_encoder_backward_overlap_bf16(const vt_layer_weights* layers, const vt_layer_weights_t* layers_t,
                                     const vt_layer_acts* acts, const vt_layer_grads* grads, int num_layers,
                                     const void* x, const float* mask, int mask_additive, void* g,
                                     const vt_bwd_workspace* ws, const vt_bwd_workspace* ws_b, int B, int S, int H, int nh,
                                     int I, float ln_eps, int accumulate, float p_hidden, float p_attn,
                                     uint64_t drop_seed, int layer0, vt_stream_t stream, vt_stream_t side_stream) {
  return vt_encoder_backward_dispatch(layers, layers_t, acts, grads, num_layers, x, mask, mask_additive, g, ws, ws_b, B, S, H,
                                      nh, I, ln_eps, accumulate, p_hidden, p_attn, drop_seed, layer0, (hipStream_t)stream,
                                      (hipStream_t)side_stream);
}

int vt_encoder_backward_seq_bf16(const vt_layer_weights* layers, const vt_layer_weights_t* layers_t,
                                 const vt_layer_acts* acts, const vt_layer_grads* grads, int num_layers, const void* x,
                                 void* g, const vt_bwd_workspace* ws, const vt_bwd_workspace* ws_b, int B, int S, int H,
                                 int nh, int I, float ln_eps, int accumulate, float p_hidden, float p_attn,
                                 uint64_t drop_seed, int layer0, int64_t rows, const int32_t* seq_start,
                                 const int32_t* seq_len, vt_stream_t stream, vt_stream_t side_stream) {
  if (rows <= 0) return VT_ERR_BAD_SHAPE;
  return vt_encoder_backward_dispatch(layers, layers_t, acts, grads, num_layers, x, nullptr, 0, g, ws, ws_b, B, S, H, nh, I,
                                      ln_eps, accumulate, p_hidden, p_attn, drop_seed, layer0, (hipStream_t)stream,
                                      (hipStream_t)side_stream, (long)rows, seq_start, seq_len);
}

int vt_encoder_backward_partial_bf16(const vt_layer_weights* layers, const vt_layer_weights_t* layers_t,
                                     const vt_layer_acts* acts, const vt_layer_grads* grads, int num_layers, const void* x,
                                     const float* mask, int mask_additive, void* g, const vt_bwd_workspace* ws,
                                     const vt_bwd_workspace* ws_b, int B, int S, int H, int nh, int I, float ln_eps,
                                     int accumulate, float p_hidden, float p_attn, uint64_t drop_seed, int layer0,
                                     int64_t rows, const int32_t* seq_start, const int32_t* seq_len, int need_input_grad,
                                     vt_stream_t stream, vt_stream_t side_stream) {
  if (rows < 0) return VT_ERR_BAD_SHAPE;
  return vt_encoder_backward_dispatch(layers, layers_t, acts, grads, num_layers, x, mask, mask_additive, g, ws, ws_b, B, S, H,
                                      nh, I, ln_eps, accumulate, p_hidden, p_attn, drop_seed, layer0, (hipStream_t)stream,
                                      (hipStream_t)side_stream, (long)rows, seq_start, seq_len, need_input_grad);
}

}  // the C ABI
