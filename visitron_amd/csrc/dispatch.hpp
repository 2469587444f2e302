// Every host function and argument block that crosses a translation unit, declared once: the *_dispatch functions
// and setters each .hip file defines for the C-ABI layer (capi.hip) and for each other.  Default arguments live here
// and only here.  The launchers that take GemmArgs are in gemm_common.hpp, vt_wgrad_v8_dispatch in wgrad_common.hpp.
#pragma once
#include "common.hpp"
#include "wgrad_common.hpp"
#include "rollout_args.hpp"

// vt_batch_rows_dispatch (rowops.hip: batch_row_counts / batch_row_lists)
struct BatchRowsArgs {
  const long* lab; const long* tl;      // [M] or null
  const float* mask;                    // [B*S] fp32 or null (no compaction wanted)
  const int* err;                       // the embedding kernel's flag or null
  long M; int S; int B;
  long* counts;                         // [5]: err, n_w, n_t, n_keep, bad   (zeroed by the caller)
  int* tile_counts;                     // [ntiles][3]: per 1024-position tile (written by the counts kernel, read by the lists kernel)
  long* idx_w; long* idx_t;             // row lists
  long* index; long* inverse;           // kept rows; padded position -> compact row or -1
  int* start; int* length;              // [B]
  long n_w, n_t, n_keep;                // capacities of the three lists (the counts batch_row_counts reported)
};

// ---- attention_bwd.hip: the dispatcher and its route (the kernel families' launchers: attention_bwd_common.hpp, one each
// for attention_bwd_keyblock.hip, attention_bwd_w16.hip and attention_bwd_w16p.hip)
void vt_attn_bwd_set_waves(int w);
int vt_attention_bwd_dispatch(const void* qkv, long ld_qkv, const void* dctx, long ld_d, const void* ctx, long ld_ctx,
                              const float* mask, int mask_additive, const float* lse, float* delta_ws, void* dqkv,
                              long ld_dqkv, float* dq32_ws, int B, int S, int nh, int head_size, hipStream_t stream,
                              const DropCfg* drop = nullptr, const int* seq_start = nullptr, const int* seq_len = nullptr,
                              long rows_total = 0, const uint32_t* keep_bits = nullptr);
// deterministic mode (the switch itself: vt_deterministic() / vt_deterministic_word() in common.hpp, set by capi.hip's
// vt_set_deterministic): bytes of dq32_ws the backward needs in the current mode, 0 where it needs none
long vt_attention_bwd_ws_bytes_impl(int B, int S, int nh, long rows);

// ---- attention_fwd.hip
int vt_attention_fwd_dispatch(const void* qkv, long ld_qkv, const float* mask, int mask_additive, const float* head_scale, void* ctx,
                              long ld_ctx, float* lse, int B, int S, int nh, int head_size, hipStream_t stream,
                              const DropCfg* drop = nullptr, const int* seq_start = nullptr, const int* seq_len = nullptr,
                              uint32_t* keep_bits = nullptr, const PrefetchArgs* pf = nullptr);
int vt_attention_probs_dispatch(const void* qkv, long ld_qkv, const float* mask, int mask_additive, const float* head_scale,
                                const float* lse, float* probs, int B, int S, int nh, int head_size, hipStream_t stream);

// ---- attention_rect.hip: Sq queries over Sk >= Sq keys (encoder_history_states)
int vt_attention_rect_fwd_dispatch(const void* qkv, long ld_qkv, const float* mask, int mask_mode, const float* head_scale,
                                   void* ctx, long ld_ctx, float* lse, int B, int Sq, int Sk, int nh, int head_size,
                                   const DropCfg& drop, uint32_t* keep_bits, hipStream_t stream);
int vt_attention_rect_bwd_dispatch(const void* qkv, long ld_qkv, const void* dctx, long ld_d, const void* ctx, long ld_ctx,
                                   const float* mask, int mask_mode, const float* lse, void* dqkv, long ld_dqkv, int B, int Sq,
                                   int Sk, int nh, int head_size, const DropCfg& drop, const uint32_t* keep_bits,
                                   hipStream_t stream);

// ---- datapipe.hip: the data pipeline's token masking and region assembly
int vt_mask_tokens_dispatch(const int64_t* ids, const uint8_t* special, const int64_t* token_classes, const float* u_mask,
                            const float* u_replace, const float* u_random, const int64_t* random_words, int64_t* out_ids,
                            int64_t* labels, int64_t* attention_mask, long n, int64_t pad_id, int64_t mask_id,
                            float mlm_probability, hipStream_t stream);
int vt_assemble_regions_dispatch(const float* img_feats, const int64_t* region_counts, const int64_t* region_view_ids,
                                 const int64_t* current_view, const float* loc_table, const int64_t* text_labels,
                                 const int64_t* text_mask, const int64_t* text_token_classes, float* feats_out, float* loc_out,
                                 int64_t* labels_out, int64_t* mask_out, int64_t* token_labels_out, int B, int T, int R,
                                 int R_in, int D, hipStream_t stream);

// ---- encoder_loops.hip: the encoder stack's layer loops and their weight-prefetch policy
int vt_encoder_forward_ln_dispatch(const vt_layer_weights_ln* layers, int num_layers, void* s16_a, void* sf_a, float* stats_a,
                                   void* s16_b, void* sf_b, float* stats_b, void* qkv, void* ctx, void* mid, const float* mask,
                                   int mask_additive, const float* head_scale, int B, int S, int H, int nh, int I, float ln_eps,
                                   long stat_rows, hipStream_t stream, long rows, const int* seq_start, const int* seq_len);
int vt_encoder_forward_dispatch(const vt_layer_weights* layers, const vt_layer_acts* acts, int num_layers, const void* x,
                                const float* mask, int mask_additive, const float* head_scale, int B, int S, int H, int nh,
                                int I, float ln_eps, float p_hidden, float p_attn, uint64_t drop_seed, hipStream_t stream,
                                long rows, const int* seq_start, const int* seq_len);
int vt_encoder_backward_dispatch(const vt_layer_weights* layers, const vt_layer_weights_t* layers_t, const vt_layer_acts* acts,
                                 const vt_layer_grads* grads, int num_layers, const void* x, const float* mask,
                                 int mask_additive, void* g, const vt_bwd_workspace* ws_a, const vt_bwd_workspace* ws_b, int B,
                                 int S, int H, int nh, int I, float ln_eps, int accumulate, float p_hidden, float p_attn,
                                 uint64_t drop_seed, int layer0, hipStream_t stream, hipStream_t side, long rows = 0,
                                 const int* seq_start = nullptr, const int* seq_len = nullptr, int need_input_grad = 1);
int vt_weight_prefetch_set(int training_mode, int inference_mode);
int vt_weight_prefetch_get(int inference);

// ---- fp32_path.hip: the fp32 inference path (and the fp32 training step's GEMM and LayerNorm)
int vt_gemm_f32_dispatch(const float* A, long lda, long sA_b, long sA_h, const float* W, long ldw, long sW_b, long sW_h,
                         int w_is_kn, const float* bias, const float* R, long ldr, float* C, long ldc, long sC_b, long sC_h,
                         int M, int N, int K, int act, float alpha, int batch, int heads, int grp_rows, int grp_stride,
                         hipStream_t stream);
int vt_gemm_f32_split_for(int M, int N, int K);
int vt_gemm_f32_ex_dispatch(const float* A, long lda, long sA_b, long sA_h, int a_is_km, const float* W, long ldw, long sW_b,
                            long sW_h, int w_is_kn, const float* bias, const float* R, long ldr, float* C, long ldc, long sC_b,
                            long sC_h, float* pre, int M, int N, int K, int act, float alpha, int batch, int heads,
                            int grp_rows, int grp_stride, int accumulate, int split, float* ws, DropCfg drop,
                            hipStream_t stream);
int vt_softmax_rows_f32_dispatch(float* x, long ld, long rows, int cols, float scale, const float* mask, int mask_mode,
                                 const float* head_scale, int nh, int S, hipStream_t stream);
int vt_layernorm_f32_dispatch(const void* x, long ldx, int x_is_f32, void* y, long ldy, int y_is_f32, const float* gamma,
                              const float* beta, long M, int H, float eps, int grp_rows, int grp_stride, hipStream_t stream);
int vt_layernorm_f32_drop_dispatch(const void* x, long ldx, int x_is_f32, void* y, long ldy, int y_is_f32, const float* gamma,
                                   const float* beta, long M, int H, float eps, int grp_rows, int grp_stride, DropCfg drop,
                                   hipStream_t stream, int drop_entry = 1);
int vt_embed_layernorm_f32_dispatch(const int64_t* ids, const int64_t* type_ids, const int64_t* pos_ids, const float* word,
                                    const float* pos, const float* type, const float* gamma, const float* beta, float* y,
                                    long ldy, int B, int T, int S, int H, int n_word, int n_pos, int n_type, float eps,
                                    int* err_flag, hipStream_t stream);

// ---- bf16x3_path.hip: the fp32 route's products as three bf16 MFMAs per term pair (arguments as vt_gemm_f32_dispatch)
int vt_gemm_bf16x3_dispatch(const float* A, long lda, long sA_b, long sA_h, const float* W, long ldw, long sW_b, long sW_h,
                            int w_is_kn, const float* bias, const float* R, long ldr, float* C, long ldc, long sC_b, long sC_h,
                            int M, int N, int K, int act, float alpha, int batch, int heads, int grp_rows, int grp_stride,
                            hipStream_t stream);

// ---- fp32_train.hip: what only the fp32 training step runs
int vt_colsum_f32_dispatch(const float* x, long ldx, long rows, int cols, float* out, int accumulate, float* ws,
                           hipStream_t stream);
int vt_ln_bwd_f32_blocks(long M);
int vt_ln_bwd_f32_dispatch(const float* x, long ldx, const float* g, long ldg, int grp_rows, int grp_stride, const float* gamma,
                           float* dx, long lddx, float* dx_drop, long ldd, float* partial, long M, int H, float eps, DropCfg din,
                           DropCfg dout, hipStream_t stream);
int vt_attn_softmax_f32_dispatch(int backward, float* x, float* pd, long ld, int B, int nh, int S, float scale, const float* mask,
                                 int mask_mode, const float* head_scale, DropCfg drop, hipStream_t stream);
int vt_dgelu_f32_dispatch(const float* g, const float* pre, float* out, long n, hipStream_t stream);
int vt_embed_sum_f32_dispatch(const int64_t* ids, const int64_t* type_ids, const int64_t* pos_ids, const float* word,
                              const float* pos, const float* type, float* e, int B, int T, int H, int n_word, int n_pos,
                              int n_type, int* err, hipStream_t stream);
int vt_dropout_rows_f32_dispatch(const float* x, long ldx, int grp_rows, int grp_stride, float* y, long ldy, long rows, int cols,
                                 DropCfg d, hipStream_t stream);

// ---- gemm_bf16.hip: the NT GEMM's host entries and tuning hooks
void vt_gemm_set_trace(void* p);
void vt_gemm_set_variant(int v);
void vt_gemm_tune_set(int M, int N, int K, int kind, int variant);
int vt_gemm_dispatch(const void* A, long lda, const void* W, long ldw, const float* bias, const void* R, long ldr,
                     void* C, long ldc, int M, int N, int K, int act, int out_mode, int grp_rows, int grp_stride,
                     hipStream_t stream, void* C2 = nullptr, long ldc2 = 0, const DropCfg* drop = nullptr,
                     const VtLnResidual* rln = nullptr);
int vt_gemm_ln_dispatch(const void* A, long lda, const void* W, long ldw, const float* bias, const float* colv,
                        const float* stats_in, int np, long stat_rows, float eps, int ln_mode, const void* Rs, long ldrs,
                        void* C, long ldc, void* Cs, long ldcs, float* stats_out, int M, int N, int K, int act,
                        hipStream_t stream);
int vt_gemm_splitk_dispatch(const void* A, long lda, const void* W, long ldw, void* C, long ldc, float* ws, int M, int N, int K,
                            int ksplit, hipStream_t stream);

// ---- gemm_v7.hip: reserved CUs and the caller-owned GEMM workspace
void vt_gemm_set_reserved_cus(int k);
int vt_gemm_set_workspace_impl(void* base, long bytes);
long vt_gemm_workspace_region_bytes_impl();
int vt_gemm_shared_tile_timeouts_impl(unsigned* out);
int vt_gemm_sk_counter_ptrs(unsigned** ptrs, int max);

// ---- gemm_wgrad.hip
void vt_wgrad_set_tile(int tn);
int vt_wgrad_dispatch(WgradArgs& a, hipStream_t stream);

// ---- gemm_wgrad_v8.hip: the persistent weight-gradient kernel's switch and timeout counter; the step's two counters in one launch
void vt_wgrad_v8_enable(int on);
int vt_wgrad_v8_timeouts(unsigned* out);
int vt_step_counters_dispatch(long long* out2, hipStream_t stream);

// ---- ln_deferred.hip: the inference path's deferred LayerNorm
int vt_ln_apply_dispatch(const void* v, long ldv, const float* stats, int np, long stat_rows, const float* gamma,
                         const float* beta, float eps, void* y16, long ldy16, float* y32, long ldy32, long M, int H,
                         hipStream_t stream);
int vt_ln_stream_init_dispatch(const float* x, long ldx, void* s16, long lds, void* y16, long ldy, float* stats, int np,
                               long stat_rows, long M, int H, float eps, hipStream_t stream);

// ---- lstm_persistent.hip
long vt_lstm_persistent_ws_bytes(int B, int hs);
int vt_lstm_persistent_dispatch(LstmPersistArgs a, void* ws, long ws_bytes, hipStream_t stream);

// ---- optim.hip: AdamW over one flat slab; multi-tensor Adam / AdamW, gradient norm and clip over a chunk table
int vt_adamw_dispatch(float* p, const void* g, int g_is_bf16, float* m, float* v, void* p_bf16, long n, float lr,
                      float step_size, float b1, float b2, float eps, float wd, float grad_scale, hipStream_t stream);
int vt_multi_adam_dispatch(const uint64_t* table, long n_chunks, const float* hyper, float grad_coef,
                           const float* grad_coef_dev, hipStream_t stream);
int vt_multi_sumsq_dispatch(const uint64_t* table, long n_chunks, void* partials, hipStream_t stream);
int vt_norm_finish_dispatch(const void* partials, long n_chunks, float max_norm, float* out, hipStream_t stream);
int vt_multi_scale_dispatch(const uint64_t* table, long n_chunks, const float* coef_dev, hipStream_t stream);
// ... and the optimizer sharded over data-parallel ranks: AdamW on this rank's segments, then the non-owned segments settled
int vt_shard_adamw_dispatch(const uint64_t* table, const uint64_t* host_table, long n_chunks, int g_is_bf16, float lr,
                            float step_size, float b1, float b2, float eps, float wd, float grad_scale, hipStream_t stream);
int vt_shard_settle_dispatch(const uint64_t* table, const uint64_t* host_table, long n_chunks, hipStream_t stream);

// ---- rollout.hip
int vt_lstm_step_dispatch(const LstmStepArgs& a, hipStream_t stream);
int vt_lstm_step_bwd_dispatch(const LstmBwdArgs& a, hipStream_t stream);
int vt_softdot_dispatch(const SoftDotArgs& a, hipStream_t stream);
long vt_softdot_bwd_split_ws_floats(int B, int L, int D);
int vt_softdot_bwd_split_dispatch(const SoftDotBwdArgs& a, float* ws, hipStream_t stream);
int vt_softdot_bwd_dispatch(const SoftDotBwdArgs& a, hipStream_t stream);
int vt_skinny_linear_dispatch(const SkinnyArgs& a, hipStream_t stream);
// the T steps of a sequence, one launch per position; sv_*: optional training saves laid out like the padded sequence
int vt_lstm_sequence_dispatch(const float* xproj, long ldx_b, long ldx_t, float* h2_0, float* h2_1, float* c, const void* w_hh,
                              const int* lengths, float* seq_out, long lds_b, long lds_t, int B, int hs, int T, int reverse,
                              hipStream_t stream, const int* xrow_start, float* sv_gates = nullptr, float* sv_c = nullptr,
                              void* sv_h = nullptr, long S_sv = 0);
int vt_lstm_sequence_bwd_dispatch(const float* d_seq_out, long ldd_b, long ldd_t, const float* dh_final, float* dc,
                                  const void* w_hh_t, const int* lengths, const float* sv_gates, const float* sv_c, void* dgates,
                                  long S_sv, int B, int hs, int T, int reverse, hipStream_t stream);

// ---- turn_based.hip
int vt_tb_lstm_cell_dispatch(const TbCellArgs& a, hipStream_t stream);
int vt_tb_action_head_dispatch(const TbHeadArgs& a, hipStream_t stream);
int vt_tb_action_head_bwd_dispatch(const TbHeadBwdArgs& a, hipStream_t stream);

// ---- observations.hip
int vt_obs_gather_dispatch(const ObsGatherArgs& a, hipStream_t stream);
int vt_obs_gather_view_dispatch(const ObsViewArgs& a, hipStream_t stream);

// ---- regions.hip: pretraining's region rows gathered from the device region store
struct RegionGatherArgs {
  const void* store; int store_bf16; long N; int V, P, D;   // [N, V, P, round_up(D, 8)] fp32 or bf16
  const unsigned char* counts;               // [N, V] rows present per view
  const float* loc_table;                    // [36, 36, 128]
  const int* rows;                           // [B][2] slot, current view
  const long* text_labels; const long* text_mask; const long* text_token_classes;   // [B, T] (token classes may be null)
  int B, T, R;
  float* feats; float* loc;                  // the unpacked form: [B, R, D], [B, R, 128] ...
  void* packed; int kpad;                    // ... or the packed one: bf16 [B * R, kpad]
  long* labels; long* mask; long* token_labels;   // [B, T + R] (token labels may be null)
  int* err;                                  // device flag raised by a bad index, or null
};
int vt_region_gather_dispatch(const RegionGatherArgs& a, hipStream_t stream);

// ---- layernorm.hip: the bf16 engine's LayerNorm and embedding LayerNorm, forward and backward
int vt_layernorm_dispatch(const void* x, long ldx, void* y, long ldy, const float* gamma, const float* beta,
                          float* mean, float* rstd, int M, int H, float eps, int grp_rows, int grp_stride,
                          hipStream_t stream, int x_f16 = 0, void* y_f16 = nullptr, long ldyh = 0,
                          const PrefetchArgs* pf = nullptr);
int vt_embed_layernorm_dispatch(const int64_t* ids, const int64_t* type_ids, const int64_t* pos_ids, const float* word,
                                const float* pos, const float* type, const float* gamma, const float* beta, void* y,
                                long ldy, int B, int T, int S, int H, int n_word, int n_pos, int n_type, float eps,
                                int* err_flag, hipStream_t stream, const DropCfg* drop = nullptr);
int vt_layernorm_bwd_dispatch(const void* x, long ldx, const void* dy, long ldy, const float* gamma, void* dx, long lddx,
                              float* dgamma, float* dbeta, float* partial_ws, int M, int H, float eps, int accumulate,
                              hipStream_t stream, void* dx2 = nullptr, long lddx2 = 0, const DropCfg* drop = nullptr,
                              int x_f16 = 0, const PrefetchArgs* pf = nullptr);
int vt_embed_layernorm_bwd_dispatch(const int64_t* ids, const int64_t* type_ids, const int64_t* pos_ids, const float* word,
                                    const float* pos, const float* type, const float* gamma, const void* g, long ldg,
                                    float* de, float* dgamma, float* dbeta, float* partial_ws, int B, int T, int S, int H,
                                    int n_word, int n_pos, int n_type, float eps, int accumulate, hipStream_t stream,
                                    const DropCfg* drop = nullptr);

// ---- loss_heads.hip: loss, argmax and gradient rows of the three heads (dz_f32: fp32 gradient rows instead of bf16)
int vt_ce_softmax_dispatch(const float* z, long ldz, const int64_t* y, float* loss_row, int64_t* amax, void* dz, long lddz,
                           long rows, int V, int Vpad, float scale, int dz_f32, hipStream_t stream);
int vt_ce_double_softmax_dispatch(const float* z, long ldz, const int64_t* y, float* loss_row, int64_t* amax, void* dz, long lddz,
                                  long rows, int V, int Vpad, float scale, int dz_f32, hipStream_t stream);
int vt_action_head_dispatch(const float* z, long ldz, const long* y, int B, int A, float grad_scale, void* dz, long lddz, int Ap,
                            float* out, int dz_f32, hipStream_t stream);

// ---- rowops.hip: the glue kernels (packing, casts, transposes, dropout, table gradients, mask centring, batch row lists)
int vt_pack_concat_dispatch(const float* s0, int d0, const float* s1, int d1, void* out, int kpad, long rows,
                            hipStream_t stream);
int vt_dgelu_mul_dispatch(const void* g, const void* h, void* out, long n, hipStream_t stream);
int vt_scale_heads_dispatch(const void* x, long ldx, void* out, long ldo, long rows, int nh, const float* scale, hipStream_t stream);
int vt_cast_scale_dispatch(const float* x, void* y, long n, float scale, hipStream_t stream);
int vt_transpose_dispatch(const void* in, long ldi, void* out, long ldo, int R, int C, hipStream_t stream);
int vt_transpose_batch_dispatch(const void* const* in, const long* ldi, void* const* out, const long* ldo, const int* R,
                                const int* C, int n, hipStream_t stream);
int vt_apply_dropout_dispatch(void* x, long ld, long rows, int cols, const DropCfg& d, hipStream_t stream);
int vt_dropout_mask_dispatch(uint8_t* out, long n, const DropCfg& d, hipStream_t stream, int attn);
int vt_embed_table_grad_dispatch(const int* sorted_ids, const long* perm, const float* de, long ld_de, float* grad, long ld_grad,
                                 long n, int H, long n_rows_table, long skip_id, float* scratch, int* flag, hipStream_t stream);
int vt_center_mask_dispatch(const void* mask, int kind, long ldm, float* out, int B, int S, hipStream_t stream);
int vt_batch_rows_dispatch(const BatchRowsArgs& a, int lists, hipStream_t stream);
