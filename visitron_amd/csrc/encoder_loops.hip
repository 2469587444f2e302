// The encoder stack's layer loops (inference with deferred LayerNorms, training forward, training backward) and what they
// keep between calls: the weight-prefetch policy and the backward's events.  capi.hip's vt_encoder_* entry points forward here.
#include "dispatch.hpp"

// ---- weight prefetch (the why: common.hpp, at vt_prefetch_role) ---------------------------------------
// The loops read the next GEMMs' weights ahead of time in spare workgroups of kernels that are launched anyway.  Training:
// mode 4 (default), in the LayerNorm forward kernels and the LayerNorm backward's reduce kernels, below VT_PREFETCH_MAX_ROWS
// token rows (default 16 384: at B = 256 the K loops run three rounds per CU at the chip's power-limited rate and hide the
// first touch).  Inference: mode 3 (default), in the attention kernel's spare z-slices (buffers shared by all layers; the
// twelve layers' weights do not survive a forward's traffic in the Infinity Cache at small batch either: measured -6 ... -9 %
// at B <= 16).  0 is off, and so is any other number the environment names (launches of their own and a side stream were
// measured and left: profiles/r06/prefetch_ab.txt).  One word each for the run, read from the environment once.
static std::atomic<int>& prefetch_mode_word() {
  static std::atomic<int> mode{(int)vt_switch(VT_PREFETCH_WEIGHTS)};
  return mode;
}
static std::atomic<int>& prefetch_infer_word() {
  static std::atomic<int> mode{(int)vt_switch(VT_PREFETCH_INFER)};
  return mode;
}
static bool prefetch_training(long rows) {
  static const long max_rows = vt_switch(VT_PREFETCH_MAX_ROWS);
  return prefetch_mode_word().load(std::memory_order_relaxed) == 4 && rows <= max_rows;
}
static bool prefetch_inference() { return prefetch_infer_word().load(std::memory_order_relaxed) == 3; }
// -1 keeps a setting; a number that is not a mode is refused and changes nothing
int vt_weight_prefetch_set(int training_mode, int inference_mode) {
  if ((training_mode != -1 && training_mode != 0 && training_mode != 4) ||
      (inference_mode != -1 && inference_mode != 0 && inference_mode != 3))
    return VT_ERR_UNSUPPORTED;
  if (training_mode >= 0) prefetch_mode_word().store(training_mode, std::memory_order_relaxed);
  if (inference_mode >= 0) prefetch_infer_word().store(inference_mode, std::memory_order_relaxed);
  return VT_OK;
}
int vt_weight_prefetch_get(int inference) {
  return (inference ? prefetch_infer_word() : prefetch_mode_word()).load(std::memory_order_relaxed);
}
static PrefetchArgs prefetch_args(const void* p0, long b0, const void* p1, long b1, const void* p2 = nullptr, long b2 = 0,
                                  const void* p3 = nullptr, long b3 = 0) {
  PrefetchArgs a;
  a.n = 0;
  const void* p[4] = {p0, p1, p2, p3};
  const long b[4] = {b0, b1, b2, b3};
  for (int i = 0; i < 4; ++i)
    if (p[i] && b[i] > 0 && !((uintptr_t)p[i] & 15)) { a.p[a.n] = p[i]; a.bytes[a.n] = b[i]; ++a.n; }
  for (int i = a.n; i < 4; ++i) { a.p[i] = nullptr; a.bytes[i] = 0; }
  return a;
}

// CaptionBertEncoder.forward (oscar/modeling_bert.py:140-169) in eval mode with the LayerNorms deferred: five launches per
// layer (no LayerNorm pass; the residual stream stays fp16):
//   qkv GEMM (LN of the incoming stream folded in) -> fused attention -> out-proj GEMM (+ LN(stream) as residual; new
//   stream + statistics) -> FFN-up GEMM (LN folded in, GELU) -> FFN-down GEMM (+ LN(stream); new stream + statistics)
// rows != 0: the streams hold `rows` compacted token rows, sequence b = rows seq_start[b] .. + seq_len[b], every key of a
// sequence attended (no mask) -- the layout of vt_encoder_forward_seq_bf16.
int vt_encoder_forward_ln_dispatch(const vt_layer_weights_ln* layers, int num_layers, void* s16_a, void* sf_a, float* stats_a,
                                   void* s16_b, void* sf_b, float* stats_b, void* qkv, void* ctx, void* mid, const float* mask,
                                   int mask_additive, const float* head_scale, int B, int S, int H, int nh, int I, float ln_eps,
                                   long stat_rows, hipStream_t stream, long rows, const int* seq_start, const int* seq_len) {
  if (!layers || !s16_a || !sf_a || !stats_a || !s16_b || !sf_b || !stats_b || !qkv || !ctx || !mid) return VT_ERR_NULL;
  if (num_layers <= 0 || B <= 0 || S <= 0 || nh <= 0 || H != nh * 64 || (H % 128) || (I % 128) || H > 1024) return VT_ERR_BAD_SHAPE;
  if (rows && (!seq_start || !seq_len || mask || rows < 0 || rows > (long)B * S)) return VT_ERR_BAD_SHAPE;
  const int M = rows ? (int)rows : B * S, np = H / 128;
  if (stat_rows < M) return VT_ERR_BAD_SHAPE;
  const bool prefetch = prefetch_inference();
  for (int l = 0; l < num_layers; ++l) {
    const vt_layer_weights_ln& w = layers[l];
    int rc;
    const long b_qkv = 6L * H * H, b_ao = 2L * H * H, b_ffn = 2L * H * I;
    rc = vt_gemm_ln_dispatch(s16_a, H, w.w_qkv, H, w.h_qkv, w.g_qkv, stats_a, np, stat_rows, ln_eps, 1, nullptr, 0, qkv, 3L * H,
                             nullptr, 0, nullptr, M, 3 * H, H, VT_ACT_NONE, stream);
    if (rc) return rc;
    const DropCfg nodrop = vt_make_drop(0.f, 0, 0);
    // riding in the attention kernel: the three weights the rest of this layer reads, and the next layer's first
    const PrefetchArgs pf_att = prefetch_args(w.w_ao, b_ao, w.w_in, b_ffn, w.w_out, b_ffn,
                                              l + 1 < num_layers ? layers[l + 1].w_qkv : nullptr, b_qkv);
    rc = vt_attention_fwd_dispatch(qkv, 3L * H, mask, mask_additive, head_scale ? head_scale + (long)l * nh : nullptr, ctx, H,
                                   nullptr, B, S, nh, 64, stream, &nodrop, rows ? seq_start : nullptr, rows ? seq_len : nullptr,
                                   nullptr, prefetch ? &pf_att : nullptr);
    if (rc) return rc;
    rc = vt_gemm_ln_dispatch(ctx, H, w.w_ao, H, w.cb_ao, w.gamma_in, stats_a, np, stat_rows, ln_eps, 2, sf_a, H, s16_b, H, sf_b,
                             H, stats_b, M, H, H, VT_ACT_NONE, stream);
    if (rc) return rc;
    rc = vt_gemm_ln_dispatch(s16_b, H, w.w_in, H, w.h_in, w.g_in, stats_b, np, stat_rows, ln_eps, 1, nullptr, 0, mid, I, nullptr, 0,
                             nullptr, M, I, H, VT_ACT_GELU, stream);
    if (rc) return rc;
    rc = vt_gemm_ln_dispatch(mid, I, w.w_out, I, w.cb_out, w.ln1_g, stats_b, np, stat_rows, ln_eps, 2, sf_b, H, s16_a, H, sf_a, H,
                             stats_a, M, H, I, VT_ACT_NONE, stream);
    if (rc) return rc;
  }
  return VT_OK;
}

// CaptionBertEncoder.forward (oscar/modeling_bert.py:140-169): the Python loop over layers, each
// layer = CaptionBertLayer.forward (:112-124) as 7 launches on one stream:
//   qkv GEMM -> fused attention -> out-proj GEMM(+bias+residual) -> LayerNorm
//   -> FFN-up GEMM(+bias+GELU) -> FFN-down GEMM(+bias+residual) -> LayerNorm
// rows != 0: the activations hold `rows` compacted token rows (no padding rows), sequence b = rows seq_start[b] ..
// seq_start[b] + seq_len[b]; every key of a sequence is attended (no mask).  rows == 0: B * S rows, sequence b at b * S.
int vt_encoder_forward_dispatch(const vt_layer_weights* layers, const vt_layer_acts* acts, int num_layers, const void* x,
                                const float* mask, int mask_additive, const float* head_scale, int B, int S, int H, int nh,
                                int I, float ln_eps, float p_hidden, float p_attn, uint64_t drop_seed, hipStream_t stream,
                                long rows, const int* seq_start, const int* seq_len) {
  if (!layers || !acts || !x) return VT_ERR_NULL;
  if (num_layers <= 0 || B <= 0 || S <= 0 || nh <= 0 || H != nh * 64 || (H % 64) || (I % 64)) return VT_ERR_BAD_SHAPE;
  if (rows && (!seq_start || !seq_len || mask || rows < 0 || rows > (long)B * S)) return VT_ERR_BAD_SHAPE;
  const int M = rows ? (int)rows : B * S;
  const bool prefetch = prefetch_training(M);
  const void* cur = x;
  const void* cur_h = nullptr;   // fp16 copy of `cur` (the previous layer's output), when that layer kept one -- or, with
                                 // cur_ln set, the previous layer's fp16 pre-LayerNorm sum whose LayerNorm `cur` is
  VtLnResidual cur_ln = {nullptr, nullptr, nullptr, nullptr};
  for (int l = 0; l < num_layers; ++l) {
    const vt_layer_weights& w = layers[l];
    const vt_layer_acts& a = acts[l];
    if (!a.qkv || !a.ctx || !a.attn_pre || !a.attn_out || !a.mid || !a.out_pre || !a.out) return VT_ERR_NULL;
    int rc;
    const long b_qkv = 6L * H * H, b_ao = 2L * H * H, b_ffn = 2L * H * I;   // bytes of the layer's four bf16 weight matrices
    rc = vt_gemm_dispatch(cur, H, w.w_qkv, H, w.b_qkv, nullptr, 0, a.qkv, 3L * H, M, 3 * H, H, VT_ACT_NONE, 0, 0, 0, stream);
    if (rc) return rc;
    if (!vt_attn_drop_ok(p_attn, vt_attn_drop_bits())) return VT_ERR_UNSUPPORTED;
    const DropCfg d_att = vt_make_drop_attn(p_attn, drop_seed, VT_SITE_ATTN(l), vt_attn_drop_bits());
    const DropCfg d_so = vt_make_drop(p_hidden, drop_seed, VT_SITE_SELFOUT(l));
    const DropCfg d_out = vt_make_drop(p_hidden, drop_seed, VT_SITE_OUT(l));
    rc = vt_attention_fwd_dispatch(a.qkv, 3L * H, mask, mask_additive, head_scale ? head_scale + (long)l * nh : nullptr, a.ctx, H,
                                   a.lse, B, S, nh, 64, stream, &d_att, rows ? seq_start : nullptr, rows ? seq_len : nullptr,
                                   a.keep_bits);
    if (rc) return rc;
    // The residual stream.  Plain form: every tensor bf16.  With the layer's fp16 copies present (ln1_h / ln2_h non-null,
    // vt_layer_acts): the pre-LayerNorm sums attn_pre / out_pre are written and read as fp16, each LayerNorm writes its
    // output twice -- bf16 for the next GEMM's A operand (and the backward), fp16 for the next sub-layer's residual add --
    // so the stream itself is rounded to 11 significant bits instead of 8 (north_star's 5e-2 on the hidden states of the
    // path training runs: 5.8e-2 with the bf16 stream on the stress weights).
    // ln_residual_mode 1: the fp16 copies are never written -- a residual add reads the previous sub-layer's fp16 SUM and
    // reconstructs its LayerNorm from the row statistics that LayerNorm's kernel wrote (GemmArgs::r_mean); the LayerNorm
    // kernel then has one output instead of two.
    const bool rln = a.ln_residual_mode == 1;
    if (rln && (!a.ln1_mean || !a.ln1_rstd || !a.ln2_mean || !a.ln2_rstd)) return VT_ERR_NULL;
    if (a.ln_residual_mode != 0 && !rln) return VT_ERR_UNSUPPORTED;
    const bool h16 = rln || (a.ln1_h && a.ln2_h);
    const void* res = cur_h ? cur_h : cur;
    rc = vt_gemm_dispatch(a.ctx, H, w.w_ao, H, w.b_ao, res, H, a.attn_pre, H, M, H, H, VT_ACT_NONE,
                          (h16 ? 2 : 0) | (cur_h ? 4 : 0), 0, 0, stream, nullptr, 0, &d_so, cur_ln.mean ? &cur_ln : nullptr);
    if (rc) return rc;
    // the LayerNorm kernels carry the prefetch in spare workgroups -- LayerNorm 1 the two FFN weights, LayerNorm 2 the
    // next layer's attention weights (no launch of its own)
    const PrefetchArgs pf_ln1 = prefetch_args(w.w_in, b_ffn, w.w_out, b_ffn);
    const PrefetchArgs pf_ln2 = l + 1 < num_layers ? prefetch_args(layers[l + 1].w_qkv, b_qkv, layers[l + 1].w_ao, b_ao)
                                                   : prefetch_args(nullptr, 0, nullptr, 0);
    rc = vt_layernorm_dispatch(a.attn_pre, H, a.attn_out, H, w.ln1_g, w.ln1_b, a.ln1_mean, a.ln1_rstd, M, H, ln_eps, 0, 0, stream,
                               h16 ? 1 : 0, (h16 && !rln) ? a.ln1_h : nullptr, H, prefetch ? &pf_ln1 : nullptr);
    if (rc) return rc;
    rc = vt_gemm_dispatch(a.attn_out, H, w.w_in, H, w.b_in, nullptr, 0, a.mid, I, M, I, H, VT_ACT_GELU, 0, 0, 0, stream,
                          a.mid_pre, I);
    if (rc) return rc;
    const VtLnResidual ln1 = {a.ln1_mean, a.ln1_rstd, w.ln1_g, w.ln1_b};
    rc = vt_gemm_dispatch(a.mid, I, w.w_out, I, w.b_out, rln ? a.attn_pre : (h16 ? a.ln1_h : a.attn_out), H, a.out_pre, H, M, H, I,
                          VT_ACT_NONE, h16 ? 6 : 0, 0, 0, stream, nullptr, 0, &d_out, rln ? &ln1 : nullptr);
    if (rc) return rc;
    rc = vt_layernorm_dispatch(a.out_pre, H, a.out, H, w.ln2_g, w.ln2_b, a.ln2_mean, a.ln2_rstd, M, H, ln_eps, 0, 0, stream,
                               h16 ? 1 : 0, (h16 && !rln) ? a.ln2_h : nullptr, H, prefetch ? &pf_ln2 : nullptr);
    if (rc) return rc;
    cur = a.out;
    cur_h = rln ? a.out_pre : (h16 ? a.ln2_h : nullptr);
    cur_ln = rln ? VtLnResidual{a.ln2_mean, a.ln2_rstd, w.ln2_g, w.ln2_b} : VtLnResidual{nullptr, nullptr, nullptr, nullptr};
  }
  return VT_OK;
}

// Backward of CaptionBertEncoder (oscar/modeling_bert.py:140-169) = the reverse layer loop; per layer
// 4 dgrad GEMMs (residual adds and the dGELU fused in their epilogues), 2 LayerNorm backwards, the
// fused attention backward and ONE grouped weight-gradient launch for the layer's four matrices
// (bias gradients ride along in it).

// Events that order the weight-gradient launches on the side stream against the dgrad chain (one pair per layer of
// a call; created once per device, never destroyed: a few dozen host-side handles).
#define VT_BWD_MAX_LAYERS 64
struct BwdEvents {
  hipEvent_t ev[2][VT_BWD_MAX_LAYERS];
  bool ok = true;
  BwdEvents() {
    for (int k = 0; k < 2; ++k)
      for (int i = 0; ok && i < VT_BWD_MAX_LAYERS; ++i) ok = hipEventCreateWithFlags(&ev[k][i], hipEventDisableTiming) == hipSuccess;
  }
};
static hipEvent_t* bwd_events(int which) {
  static VtPerDevice<BwdEvents> store;
  BwdEvents* e = store.get();
  return e && e->ok ? e->ev[which] : nullptr;
}

// The reverse layer loop.  With a second workspace set (ws_b) and a side stream the four weight gradients of layer l
// run on the side stream while the main stream goes on with layer l-1: the grouped wgrad launch keeps 216 of the 256
// CUs busy (108 tiles x 2 row ranges), the next layer's LayerNorm backward and whatever else is not a persistent
// kernel fills the rest.  Layer l works in workspace set (layer0 + l) & 1, so the buffers a wgrad still reads are
// rewritten two layers later, behind a wait on that wgrad's completion event; before returning the main stream waits
// for every wgrad of the call.
// A layer whose vt_layer_grads holds twelve null pointers is FROZEN: it launches no weight gradient (and records no event:
// the waits below look at what was recorded in this call only) and its two LayerNorm backwards run dx-only.
// need_input_grad == 0: nobody reads dL/d(x) -- layers[0] skips its last dgrad GEMM (a frozen layers[0] is skipped
// altogether) and g is left undefined.
int vt_encoder_backward_dispatch(const vt_layer_weights* layers, const vt_layer_weights_t* layers_t,
                                 const vt_layer_acts* acts, const vt_layer_grads* grads, int num_layers, const void* x,
                                 const float* mask, int mask_additive, void* g, const vt_bwd_workspace* ws_a,
                                 const vt_bwd_workspace* ws_b, int B, int S, int H, int nh, int I, float ln_eps,
                                 int accumulate, float p_hidden, float p_attn, uint64_t drop_seed, int layer0,
                                 hipStream_t stream, hipStream_t side, long rows, const int* seq_start,
                                 const int* seq_len, int need_input_grad) {
  if (!layers || !layers_t || !acts || !grads || !x || !g || !ws_a) return VT_ERR_NULL;
  if (rows && (!seq_start || !seq_len || mask || rows < 0 || rows > (long)B * S)) return VT_ERR_BAD_SHAPE;
  const bool overlap = ws_b != nullptr && side != nullptr && side != stream;
  for (int k = 0; k < (overlap ? 2 : 1); ++k) {
    const vt_bwd_workspace* ws = k ? ws_b : ws_a;
    if (p_hidden > 0.f && (!ws->g_pre_d || !ws->g_pre2_d)) return VT_ERR_NULL;
    if (!ws->g_pre || !ws->g_pre2 || !ws->g_mid || !ws->g_ctx || !ws->g_qkv || !ws->delta || !ws->ln_partial) return VT_ERR_NULL;
  }
  if (num_layers <= 0 || B <= 0 || S <= 0 || nh <= 0 || H != nh * 64 || (I % 64)) return VT_ERR_BAD_SHAPE;
  if (overlap && num_layers > VT_BWD_MAX_LAYERS) return VT_ERR_BAD_SHAPE;
  hipEvent_t* ev_in = overlap ? bwd_events(0) : nullptr;    // E[l]: layer l's wgrad operands are complete (main)
  hipEvent_t* ev_done = overlap ? bwd_events(1) : nullptr;  // F[l]: layer l's wgrad has finished (side)
  if (overlap && (!ev_in || !ev_done)) return VT_ERR_HIP;
  const int M = rows ? (int)rows : B * S;
  const bool prefetch = prefetch_training(M);
  bool recorded[VT_BWD_MAX_LAYERS] = {};   // layers whose wgrad went to the side stream in THIS call
  int last_recorded = -1;
  for (int l = num_layers - 1; l >= 0; --l) {
    const vt_layer_weights& w = layers[l];
    const vt_layer_weights_t& wt = layers_t[l];
    const vt_layer_acts& a = acts[l];
    const vt_layer_grads& d = grads[l];
    float* const dptr[12] = {d.d_w_qkv, d.d_b_qkv, d.d_w_ao, d.d_b_ao, d.d_ln1_g, d.d_ln1_b,
                             d.d_w_in, d.d_b_in, d.d_w_out, d.d_b_out, d.d_ln2_g, d.d_ln2_b};
    int nset = 0;
    for (int i = 0; i < 12; ++i) nset += dptr[i] != nullptr;
    if (nset != 0 && nset != 12) return VT_ERR_NULL;   // a layer is trainable (all twelve) or frozen (none)
    const bool frozen = nset == 0;
    const bool input_grad = l > 0 || need_input_grad != 0;
    if (frozen && !input_grad) continue;
    if (!a.mid_pre || !a.lse) return VT_ERR_NULL;
    const void* x_in = l == 0 ? x : acts[l - 1].out;
    const vt_bwd_workspace* ws = (overlap && ((layer0 + l) & 1)) ? ws_b : ws_a;
    // this layer rewrites the set that the wgrad of layer l + 2 reads
    if (overlap && l + 2 < num_layers && recorded[l + 2] && hipStreamWaitEvent(stream, ev_done[l + 2], 0) != hipSuccess)
      return VT_ERR_HIP;
    int rc;
    // dropout sites of this layer (the forward used layer index layer0 + l)
    if (!vt_attn_drop_ok(p_attn, vt_attn_drop_bits())) return VT_ERR_UNSUPPORTED;
    const DropCfg d_att = vt_make_drop_attn(p_attn, drop_seed, VT_SITE_ATTN(layer0 + l), vt_attn_drop_bits());
    const DropCfg d_so = vt_make_drop(p_hidden, drop_seed, VT_SITE_SELFOUT(layer0 + l));
    const DropCfg d_out = vt_make_drop(p_hidden, drop_seed, VT_SITE_OUT(layer0 + l));
    // with hidden dropout the gradient of a dense output is the pre-LayerNorm gradient times the mask
    void* g_pre_dn = p_hidden > 0.f ? ws->g_pre_d : ws->g_pre;
    void* g_pre2_dn = p_hidden > 0.f ? ws->g_pre2_d : ws->g_pre2;
    const long b_qkv = 6L * H * H, b_ao = 2L * H * H, b_ffn = 2L * H * I;   // the transposed copies have the same sizes
    // LayerNorm 2 backward: dL/d(out_pre)
    const int h16 = ((a.ln1_h && a.ln2_h) || a.ln_residual_mode == 1) ? 1 : 0;   // the forward kept the pre-LayerNorm sums as fp16 (see vt_encoder_forward_dispatch)
    const PrefetchArgs pf_ln2 = prefetch_args(wt.wt_out, b_ffn, wt.wt_in, b_ffn);   // riding in the two LayerNorm backwards' reduce kernels: the transposed weights of the dgrad GEMMs behind each
    const PrefetchArgs pf_ln1 = prefetch_args(wt.wt_ao, b_ao, wt.wt_qkv, b_qkv);
    rc = vt_layernorm_bwd_dispatch(a.out_pre, H, g, H, w.ln2_g, ws->g_pre, H, d.d_ln2_g, d.d_ln2_b, ws->ln_partial, M, H,
                                   ln_eps, accumulate, stream, p_hidden > 0.f ? ws->g_pre_d : nullptr, H, &d_out, h16,
                                   prefetch ? &pf_ln2 : nullptr);
    if (rc) return rc;
    // through output.dense and the GELU: g_mid = (g_pre . W_out) * gelu'(pre-activation) (saved in mid_pre)
    rc = vt_gemm_dispatch(g_pre_dn, H, wt.wt_out, H, nullptr, a.mid_pre, I, ws->g_mid, I, M, I, H, VT_ACT_MUL, 0, 0, 0, stream);
    if (rc) return rc;
    // through intermediate.dense, plus the residual branch: dL/d(attn_out) -> g
    rc = vt_gemm_dispatch(ws->g_mid, I, wt.wt_in, I, nullptr, ws->g_pre, H, g, H, M, H, I, VT_ACT_NONE, 0, 0, 0, stream);
    if (rc) return rc;
    // LayerNorm 1 backward: dL/d(attn_pre)
    rc = vt_layernorm_bwd_dispatch(a.attn_pre, H, g, H, w.ln1_g, ws->g_pre2, H, d.d_ln1_g, d.d_ln1_b, ws->ln_partial, M, H,
                                   ln_eps, accumulate, stream, p_hidden > 0.f ? ws->g_pre2_d : nullptr, H, &d_so, h16,
                                   prefetch ? &pf_ln1 : nullptr);
    if (rc) return rc;
    // through attention.output.dense: dL/d(ctx)
    rc = vt_gemm_dispatch(g_pre2_dn, H, wt.wt_ao, H, nullptr, nullptr, 0, ws->g_ctx, H, M, H, H, VT_ACT_NONE, 0, 0, 0, stream);
    if (rc) return rc;
    rc = vt_attention_bwd_dispatch(a.qkv, 3L * H, ws->g_ctx, H, a.ctx, H, mask, mask_additive, a.lse, ws->delta, ws->g_qkv,
                                   3L * H, ws->dq32, B, S, nh, 64, stream, &d_att, rows ? seq_start : nullptr,
                                   rows ? seq_len : nullptr, rows, a.keep_bits);
    if (rc) return rc;
    // through the packed q|k|v projection, plus the residual branch: dL/d(layer input) -> g
    if (input_grad) {
      rc = vt_gemm_dispatch(ws->g_qkv, 3L * H, wt.wt_qkv, 3L * H, nullptr, ws->g_pre2, H, g, H, M, H, 3 * H, VT_ACT_NONE, 0, 0, 0, stream);
      if (rc) return rc;
    }
    if (frozen) continue;
    // the four weight (+bias) gradients of this layer in one grouped launch
    WgradArgs wa;
    wa.nprob = 4;
    wa.M = M;
    auto set = [&](int i, const void* dY, long ldy, const void* X, long ldx, float* dW, float* db, int N, int K) {
      WgradProblem& P = wa.p[i];
      P.dY = (const bf16_t*)dY; P.ldy = ldy; P.X = (const bf16_t*)X; P.ldx = ldx; P.dW = dW; P.ldw = K; P.db = db;
      P.N = N; P.K = K; P.accumulate = accumulate; P.tiles_k = 0; P.tile_begin = 0;
    };
    set(0, ws->g_mid, I, a.attn_out, H, d.d_w_in, d.d_b_in, I, H);
    set(1, g_pre_dn, H, a.mid, I, d.d_w_out, d.d_b_out, H, I);
    set(2, ws->g_qkv, 3L * H, x_in, H, d.d_w_qkv, d.d_b_qkv, 3 * H, H);
    set(3, g_pre2_dn, H, a.ctx, H, d.d_w_ao, d.d_b_ao, H, H);
    for (int i = 4; i < WG_MAX_PROBLEMS; ++i) wa.p[i] = wa.p[0];
    if (overlap) {
      if (hipEventRecord(ev_in[l], stream) != hipSuccess || hipStreamWaitEvent(side, ev_in[l], 0) != hipSuccess) return VT_ERR_HIP;
      rc = vt_wgrad_dispatch(wa, side);
      if (rc) return rc;
      if (hipEventRecord(ev_done[l], side) != hipSuccess) return VT_ERR_HIP;
      recorded[l] = true;
      last_recorded = l;
    } else {
      rc = vt_wgrad_dispatch(wa, stream);
      if (rc) return rc;
    }
  }
  if (overlap) {   // the caller's next work on the main stream (all-reduce, optimizer) sees every weight gradient
    for (int l = (num_layers < 2 ? num_layers : 2) - 1; l >= 0; --l)
      if (recorded[l] && hipStreamWaitEvent(stream, ev_done[l], 0) != hipSuccess) return VT_ERR_HIP;
    // (the side stream runs in order: where layers 0 and 1 recorded nothing, the last event recorded covers the call)
    if (last_recorded >= 2 && hipStreamWaitEvent(stream, ev_done[last_recorded], 0) != hipSuccess) return VT_ERR_HIP;
  }
  return VT_OK;
}
