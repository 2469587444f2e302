"""The turn-based fine-tuning task (tasks/turn_based), served by the HIP library.

Drop-ins for tasks/turn_based/agent_models.py: `OscarEncoder` (:117-235, the same class as the viewpoint task's, re-exported
from visitron_amd.rollout), `SoftDotAttention` (:238-274) and `AttnDecoderLSTM` (:277-319) -- same constructor arguments,
parameter names (the reference's state dicts load) and return values -- and `action_feedback`, one launch for what
tasks/turn_based/agent.py:316-338 does to the logits of a step (blocked actions, CrossEntropyLoss(ignore_index), next action).

Routing follows `rollout._grad_mode`.  Forward-only calls (eval, or p == 0, without a graph to build) run the decoder's
embedding + cat + nn.LSTMCell as ONE kernel (vt_turn_lstm_cell_f32: ids and table in, h_1 / c_1 out).  Calls that need a
graph or a dropout draw run autograd nodes whose forward is the same kernel fed with the dropped rows and whose backward is
vt_lstm_step_bwd_f32, the dense kernels on the transposed packs and one grouped vt_wgrad_bf16.  `nn.Embedding` and
`nn.Dropout` are torch ops on the device there.  No CPU fallback.
"""
import torch
import torch.nn as nn

from . import ops, rollout, switches
from . import rollout_autograd as ra
from .ops import ACT_NONE, BF16, round_up
from .rollout import OscarEncoder, _dense, _f32c, _grad_mode, _pad_weight, _Packed   # noqa: F401  (OscarEncoder: re-export)


def _post_flag(err):
    """The project's embedding convention (modeling._post_index_flag): the device flag travels to the host behind the launch
    and raises IndexError at the end of this call if it has landed, else at the next one or at modeling.check_errors()."""
    from . import modeling

    if torch.cuda.is_current_stream_capturing():
        return
    modeling._post_index_flag(err)
    modeling._poll_index_flags(block=switches.on("VT_SYNC_ERRORS"))


def _rows_f32(x):
    """fp32 rows with a contiguous last dimension; a strided view stays a view (the cell kernel takes row strides)."""
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    return x if x.stride(-1) == 1 else x.contiguous()


class SoftDotAttention(rollout.SoftDotAttention):
    """agent_models.py:238-274: one width for query and context; `forward(h, context, mask=None) -> (h_tilde, attn)` with
    attn always the probabilities.  mask: any dtype, non-zero = masked (the caller passes the uint8 seq_mask)."""

    def __init__(self, dim):
        super().__init__(dim, dim)

    def forward(self, h, context, mask=None):
        return super().forward(h, context, mask, True, True)


class _TurnCell(torch.autograd.Function):
    """[x_emb | feature] -> nn.LSTMCell, training form: the fused kernel with the saves, vt_lstm_step_bwd_f32 backwards."""

    @staticmethod
    def forward(ctx, x_emb, feature, h_prev, c_prev, w_ih, w_hh, b_ih, b_hh, packs):
        w_ih_pad, w_ih_t, w_hh16, w_hh_t = packs
        xe, xf, hp, cp = _rows_f32(x_emb), _rows_f32(feature), _f32c(h_prev), _f32c(c_prev)
        bias = (b_ih.detach().float() + b_hh.detach().float()).contiguous()
        h1, c1, saved = ops.turn_lstm_cell(xe, xf, hp, cp, w_ih_pad, w_hh16, bias, save=True)
        E, F = xe.shape[1], xf.shape[1]
        # the weight gradient's bf16 operand, zero-padded to a multiple of 8 columns (2118 -> 2120): vt_wgrad_bf16 takes
        # row strides in multiples of 8 and widths in multiples of 4
        x16 = torch.zeros((xe.shape[0], round_up(E + F, 8)), dtype=BF16, device=xe.device)
        x16[:, :E] = xe
        x16[:, E:E + F] = xf
        ctx.packs, ctx.dims = (w_ih_t, w_hh_t), (E, F)
        ctx.save_for_backward(x16, *saved)
        ctx.set_materialize_grads(False)
        return h1, c1

    @staticmethod
    def backward(ctx, dh, dc):
        if dh is None and dc is None:
            return (None,) * 9
        x16, sv_g, sv_c, sv_h = ctx.saved_tensors
        w_ih_t, w_hh_t = ctx.packs
        E, F = ctx.dims
        B, hs = sv_c.shape
        dg32, dg16, dc_prev = ops.lstm_step_bwd(dh, dc, (sv_g, sv_c, sv_h), w_hh_t)
        dxe = dxf = dh_prev = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dx = _dense((dg32,), w_ih_t)
            dxe = dx[:, :E] if ctx.needs_input_grad[0] else None
            dxf = dx[:, E:E + F] if ctx.needs_input_grad[1] else None
        if ctx.needs_input_grad[2]:
            dh_prev = _dense((dg32,), w_hh_t)
        G, Kp = 4 * hs, x16.shape[1]
        dev = dg16.device
        p_ih = dict(dy=dg16, x=x16, dw=torch.empty((G, Kp), dtype=torch.float32, device=dev),
                    db=torch.empty((G,), dtype=torch.float32, device=dev))
        p_hh = dict(dy=dg16, x=sv_h, dw=torch.empty((G, hs), dtype=torch.float32, device=dev), db=None)
        ops.wgrad([p_ih, p_hh], B)
        dw_ih = p_ih["dw"] if Kp == E + F else p_ih["dw"][:, :E + F]
        return dxe, dxf, dh_prev, (dc_prev if ctx.needs_input_grad[3] else None), dw_ih, p_hh["dw"], p_ih["db"], p_ih["db"], None


class AttnDecoderLSTM(nn.Module):
    """agent_models.py:277-319: one decoder step of the turn-based agent -- the previous action's embedding and one image
    feature per row through an LSTM cell, attention over the instruction, a linear head over the low-level actions.

    `forward(action, feature, h_0, c_0, ctx, ctx_mask=None) -> (h_1, c_1, alpha, logit)`; action int64 [B, 1] or [B].  A batch
    of one row is served as one row (the reference's `.squeeze()` drops the batch axis there and its `torch.cat` fails).  The
    caller's h_0 / c_0 are never written."""

    def __init__(self, input_action_size, output_action_size, embedding_size, hidden_size, dropout_ratio, feature_size=2048):
        super().__init__()
        self.embedding_size = embedding_size
        self.feature_size = feature_size
        self.hidden_size = hidden_size
        self.embedding = nn.Embedding(input_action_size, embedding_size)
        self.drop = nn.Dropout(p=dropout_ratio)
        self.lstm = nn.LSTMCell(embedding_size + feature_size, hidden_size)   # parameter container
        self.attention_layer = SoftDotAttention(hidden_size)
        self.decoder2action = nn.Linear(hidden_size, output_action_size)
        self._pk = _Packed()
        self._pk_t = _Packed()

    def _weights(self):
        cell, head = self.lstm, self.decoder2action

        def build():
            return dict(table=_f32c(self.embedding.weight), w_ih=_pad_weight(cell.weight_ih),
                        b=(cell.bias_ih.detach().float() + cell.bias_hh.detach().float()).contiguous(),
                        w_hh=cell.weight_hh.detach().to(BF16).contiguous(), w_head=_pad_weight(head.weight),
                        b_head=_f32c(head.bias))

        return self._pk.get((self.embedding.weight, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh, head.weight,
                             head.bias), build)

    def _check(self, ids, feature, h_0, c_0):
        B = ids.shape[0]
        if feature.dim() != 2 or feature.shape != (B, self.feature_size):
            raise RuntimeError("feature must be [%d, %d], got %s" % (B, self.feature_size, tuple(feature.shape)))
        for s in (h_0, c_0):
            if tuple(s.shape) != (B, self.hidden_size):
                raise RuntimeError("h_0 / c_0 must be [%d, %d], got %s" % (B, self.hidden_size, tuple(s.shape)))

    def _forward_autograd(self, ids, feature, h_0, c_0, ctx, ctx_mask):
        """:309-318 as autograd nodes.  `drop` on the embedded rows and on the feature separately: element-wise the same
        distribution as dropping their concatenation (:314)."""
        cell, head = self.lstm, self.decoder2action
        packs = self._pk_t.get((cell.weight_ih, cell.weight_hh, head.weight),
                               lambda: (ra.packed_lstm(cell.weight_ih, cell.weight_hh), ra.packed_linear(head.weight)))
        x_emb = self.drop(self.embedding(ids))
        x_feat = self.drop(feature.float())
        h_1, c_1 = _TurnCell.apply(x_emb, x_feat, h_0, c_0, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh,
                                   packs[0])
        h_tilde, alpha = self.attention_layer(self.drop(h_1), ctx, ctx_mask)
        logit = ra.dense(h_tilde, head.weight, head.bias, ACT_NONE, packs[1])
        return h_1, c_1, alpha, logit

    def forward(self, action, feature, h_0, c_0, ctx, ctx_mask=None):
        ops._require_hip(action, feature, h_0, c_0, ctx)
        if action.dtype != torch.int64 or action.dim() not in (1, 2) or (action.dim() == 2 and action.shape[1] != 1):
            raise RuntimeError("action must be int64 [B, 1] or [B]")
        ids = action.reshape(-1).contiguous()
        self._check(ids, feature, h_0, c_0)
        if _grad_mode(self, feature, h_0, c_0, ctx):
            return self._forward_autograd(ids, feature, h_0, c_0, ctx, ctx_mask)
        w = self._weights()
        err = torch.zeros(1, dtype=torch.int32, device=ids.device)
        h_1, c_1, _ = ops.turn_lstm_cell((ids, w["table"]), _rows_f32(feature), _f32c(h_0), _f32c(c_0), w["w_ih"], w["w_hh"],
                                         w["b"], err_flag=err)                                           # :309-315
        h_tilde, alpha = self.attention_layer(h_1, ctx, ctx_mask)                                        # :316-317
        logit = _dense((h_tilde,), w["w_head"], w["b_head"])                                             # :318
        _post_flag(err)
        return h_1, c_1, alpha, logit


# ---- the action head around the step (agent.py:316-338) ----------------------------------------------------------------
_seed_count = [0]


def _next_seed():
    """A fresh 32-bit seed per call from the process seed and a counter (the engines' dropout seeds are drawn the same way:
    torch.initial_seed() plus a call count), so torch.manual_seed reproduces a run."""
    _seed_count[0] += 1
    return (int(torch.initial_seed()) * 0x9E3779B1 + _seed_count[0]) & 0xFFFFFFFF


class _ActionHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, target, blocked, ignore_index, mode, seed, err):
        lg = logit.detach()
        if lg.dtype != torch.float32 or lg.stride(1) != 1:
            lg = lg.float().contiguous()
        loss, count, a_t = ops.turn_action_head(lg, target, blocked, ignore_index, mode, seed, err_flag=err)
        ctx.blocked, ctx.ignore_index = blocked, ignore_index
        ctx.save_for_backward(lg, target, count)
        ctx.mark_non_differentiable(a_t)
        return loss.view(()), a_t

    @staticmethod
    def backward(ctx, g, _):
        lg, target, count = ctx.saved_tensors
        g = g.detach().to(torch.float32).reshape(1).contiguous()
        return ops.turn_action_head_bwd(lg, target, ctx.blocked, ctx.ignore_index, g, count), None, None, None, None, None, None


def action_feedback(logit, target, blocked=None, ignore_index=-100, feedback="teacher", seed=None):
    """One step's loss and next action in one launch (agent.py:316-338) -> (loss, a_t).

    logit fp32 [B, A], 1 <= A <= 64; target int64 [B]; blocked bool / uint8 [B, A], non-zero = that logit counts as -inf (the
    reference's per-row `logit[i, forward] = -inf` writes gathered into one host-built tensor).  `logit` is NOT modified --
    the reference fills it in place; here the block is applied inside the kernel, and no gradient reaches a blocked entry.

    loss: 0-dim fp32 autograd result = CrossEntropyLoss(ignore_index)(blocked logits, target): the mean over the rows whose
    target is not ignore_index; +inf when such a row's target is blocked; NaN when no row counts (as torch gives).
    a_t int64 [B]: "teacher" = target; "argmax" = the lowest index of the row maximum; "sample" = inverse CDF in index order
    at u = (hash32(seed, row) >> 8) * 2^-24 -- the smallest a with sum_{j<=a} e_j > u * sum_j e_j, e_j = exp(l_j - max) in
    fp32, never a blocked entry.  seed=None draws a fresh seed from the module's counter.  A target outside [0, A) that is
    not ignore_index raises IndexError like an embedding id (modeling.check_errors())."""
    ops._require_hip(logit, target, blocked)
    if feedback not in ops.TURN_FEEDBACK:
        raise ValueError("Invalid feedback option %r" % (feedback,))
    if logit.dim() != 2 or not 1 <= logit.shape[1] <= 64:
        raise RuntimeError("logit must be [B, A] with 1 <= A <= 64, got %s" % (tuple(logit.shape),))
    mode = ops.TURN_FEEDBACK[feedback]
    if mode == 2 and seed is None:
        seed = _next_seed()
    tgt = target if (target.dtype == torch.int64 and target.is_contiguous()) else target.to(torch.int64).contiguous()
    err = torch.zeros(1, dtype=torch.int32, device=logit.device)
    loss, a_t = _ActionHead.apply(logit, tgt, blocked, int(ignore_index), mode, 0 if seed is None else int(seed), err)
    _post_flag(err)
    return loss, (tgt if mode == 0 else a_t)
