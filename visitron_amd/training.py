"""Training path of the hot loop: tasks/viewpoint_select/pretrain.py:150-193 on HIP kernels.

``PretrainEngine`` owns what the reference's step does around ``model(**batch)``:

    model.zero_grad(); loss, ... = model(**batch); [all-reduce]; loss.backward(); optimizer.step(); scheduler.step()

* parameters are re-pointed into ONE flat fp32 slab (decay group first, then the no-decay group of
  pretrain.py:109-127), gradients into a second slab of the same layout (``p.grad`` are views), and
  a bf16 mirror of the parameter slab is what the GEMM kernels read; query/key/value weights (and
  biases) are laid out adjacently so the packed [3H,H] projection and its gradient are plain views;
* forward saves per-layer activations; backward = hand-written HIP kernels (encoder: one C call);
* the MLM / token heads are evaluated on the SUPERVISED rows only (labels != -1): the 7-tuple the
  reference returns depends on nothing else (encoder.py:377-431), so the result is identical while
  the 30522-wide decoder GEMM shrinks by ~12x;
* the optimizer is a fused AdamW kernel with the pytorch-transformers update rule;
* data parallelism: one process per GPU, bucketed all-reduce of the flat gradient slab
  (``torch.distributed``; backend "nccl" = RCCL over xGMI), see ``visitron_amd.distributed``.
"""
import collections
import ctypes
import math

import torch
import torch.nn.functional as F

from . import _lib, distributed, ops, switches, training_f32
from .modeling import BertImgModelwithLocationEmbeds, PreTrainOscar, _i64, invalidate_packed_weights
from .ops import ACT_MUL, ACT_GELU, ACT_NONE, ACT_TANH, BF16, round_up

ALIGN = 64  # elements; keeps every parameter view 256-byte aligned inside the slabs


def _is_no_decay(name):
    return ("bias" in name) or ("LayerNorm.weight" in name)  # pretrain.py:109


class FlatParams(object):
    """Flat fp32 parameter / gradient / moment slabs + bf16 mirror for a PreTrainOscar."""

    def __init__(self, model, attach_grads=True, moments=True):
        # moments=False: no full-size m and v slabs (an engine whose optimizer is sharded over the ranks keeps shard-sized ones)
        self.attach_grads = attach_grads
        named = list(model.named_parameters())
        dev = named[0][1].device
        # order: decay params then no-decay params; model order inside each group already puts
        # query, key, value (weights, and separately their biases) of a layer next to each other
        decay = [(n, p) for n, p in named if not _is_no_decay(n)]
        nodecay = [(n, p) for n, p in named if _is_no_decay(n)]
        self.entries, off = [], 0
        for grp, items in ((0, decay), (1, nodecay)):
            for n, p in items:
                # q|k|v must be exactly adjacent: no padding between them
                adjacent = n.endswith(("attention.self.key.weight", "attention.self.value.weight",
                                       "attention.self.key.bias", "attention.self.value.bias"))
                if not adjacent:
                    off = round_up(off, ALIGN)
                self.entries.append((n, p, off, p.numel(), grp))
                off += p.numel()
            off = round_up(off, ALIGN)
            if grp == 0:
                self.n_decay = off
        self.total = off
        self.p = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.g = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.m = torch.zeros(self.total, dtype=torch.float32, device=dev) if moments else None
        self.v = torch.zeros(self.total, dtype=torch.float32, device=dev) if moments else None
        self.mirror = torch.zeros(self.total, dtype=BF16, device=dev)
        self.off = {}
        for n, p, o, cnt, _ in self.entries:
            self.p[o:o + cnt].copy_(p.data.reshape(-1))
            p.data = self.p[o:o + cnt].view(p.shape)
            self.off[n] = (o, cnt, tuple(p.shape))
        # an entry's span: its elements and the padding up to the next entry (the padding belongs to no parameter and holds zeros)
        starts = [o for _, _, o, _, _ in self.entries] + [self.total]
        self.span = {n: (o, nxt) for (n, _, o, _, _), nxt in zip(self.entries, starts[1:])}
        self._params = [p for _, p, _, _, _ in self.entries]
        self.reattach_grads()
        self.refresh_mirror()

    def flags(self):
        """requires_grad of every entry, in slab order (read at every step: PretrainEngine._sync_trainable)."""
        return tuple([p.requires_grad for p in self._params])

    def owns_params(self):
        """False once something re-pointed a parameter's storage (another engine built over the same parameters -- the
        full model's and the bare trunk's -- or model.to / load with assign): this slab is then stale."""
        base = self.p.data_ptr()
        return all(p.data_ptr() == base + 4 * o for _, p, o, _, _ in self.entries)

    def refresh_mirror(self):
        self.mirror.copy_(self.p)
        self._versions = self._version_key()

    def _version_key(self):
        return tuple(p._version for _, p, _, _, _ in self.entries)

    def mirror_is_stale(self):
        return self._version_key() != self._versions

    def mark_fresh(self):
        self._versions = self._version_key()

    def view(self, slab, name, count=None, shape=None):
        o, cnt, shp = self.off[name]
        if count is not None:
            return slab[o:o + count].view(shape)
        return slab[o:o + cnt].view(shp)

    def reattach_grads(self):
        """optimizer.zero_grad(set_to_none=True) drops p.grad; point them back at the slab.  A parameter that does not
        require grad has no gradient: its p.grad is None (its range of the slab is scratch nobody exposes)."""
        if not self.attach_grads:
            return
        for n, p, o, cnt, _ in self.entries:
            if not p.requires_grad:
                p.grad = None
            elif p.grad is None or p.grad.data_ptr() != self.g.data_ptr() + 4 * o:
                p.grad = self.g[o:o + cnt].view(p.shape)


# VT_ATTN_KEEP_BITS=0: the attention backward re-derives the dropout mask from the hash instead of reading the words the
# forward wrote (same mask either way; A/B switch)
KEEP_BITS = switches.on("VT_ATTN_KEEP_BITS")


# One encoder layer: table field -> parameter name under "bert.encoder.layer.<l>.".  The "w_*" fields are GEMM weights (the
# bf16 engine reads them through the mirror and keeps a transposed copy "wt_*" of each), the others fp32 vectors.
_LAYER_FIELDS = dict(
    w_ao="attention.output.dense.weight", b_ao="attention.output.dense.bias",
    ln1_g="attention.output.LayerNorm.weight", ln1_b="attention.output.LayerNorm.bias",
    w_in="intermediate.dense.weight", b_in="intermediate.dense.bias",
    w_out="output.dense.weight", b_out="output.dense.bias",
    ln2_g="output.LayerNorm.weight", ln2_b="output.LayerNorm.bias")
# ... and the packed projection: query | key | value lie adjacent in the slabs (FlatParams), so [3H, H] / [3H] are views
# that start at the query's entry
_LAYER_PACKED = dict(w_qkv="attention.self.%s.weight", b_qkv="attention.self.%s.bias")
_QKV = ("query", "key", "value")


def _layer_views(flat, l, w_slab, v_slab):
    """{field: view} of encoder layer l, the GEMM weights taken from w_slab and the vectors from v_slab."""
    pre = "bert.encoder.layer.%d." % l
    out = {}
    for k, pat in _LAYER_PACKED.items():
        o, cnt, shp = flat.off[pre + pat % _QKV[0]]
        out[k] = (w_slab if k.startswith("w_") else v_slab)[o:o + 3 * cnt].view((3 * shp[0],) + shp[1:])
    for k, name in _LAYER_FIELDS.items():
        out[k] = flat.view(w_slab if k.startswith("w_") else v_slab, pre + name)
    return out


# the layer's GEMM weights by name (what _layer_views takes from w_slab)
_LAYER_WEIGHTS = [_LAYER_PACKED["w_qkv"] % x for x in _QKV] + [n for k, n in _LAYER_FIELDS.items() if k.startswith("w_")]


# The head, pooler and region-projection parameters: (group, attribute path on the model, transposed copy).  A weight with a
# transposed copy (a key of PretrainEngine.head_t; "" = none kept) is a GEMM operand the bf16 step reads through the mirror;
# None marks what is read as fp32.  The groups are what one supervision signal feeds: without it (no supervised MLM row, no
# token row, no next_action, no regions) the group's gradients are zero.  Rows outside "bert." exist with the heads only.
_HEAD_TABLE = (
    ("pooler", "bert.pooler.dense.weight", "pool"), ("pooler", "bert.pooler.dense.bias", None),
    ("mlm", "mlmhead.predictions.transform.dense.weight", "tr"), ("mlm", "mlmhead.predictions.transform.dense.bias", None),
    ("mlm", "mlmhead.predictions.transform.LayerNorm.weight", None), ("mlm", "mlmhead.predictions.transform.LayerNorm.bias", None),
    ("mlm", "mlmhead.predictions.bias", None),
    ("mlm", "mlmhead.predictions.decoder.weight", "dec"),   # tied: the word table itself (PretrainEngine._head_group)
    ("token", "token_head.0.weight", "tok"), ("token", "token_head.0.bias", None),
    ("action", "next_action.linear.weight", "act"), ("action", "next_action.linear.bias", None),
    ("region", "bert.img_embedding.weight", ""), ("region", "bert.img_embedding.bias", None),
    ("region", "bert.location_embeds.weight", ""), ("region", "bert.location_embeds.bias", None),
    ("region", "bert.LayerNorm.weight", None), ("region", "bert.LayerNorm.bias", None),   # (with use_img_layernorm only)
)
_HEAD_GROUPS = ("mlm", "token", "action", "pooler")   # final before the encoder backward starts; "region" is not

# ---- requires_grad: what a frozen parameter costs is decided per UNIT, the parameters one backward launch group feeds -- an
# encoder layer (its 16 tensors), the embedding block (word / position / type tables and their LayerNorm; a tied MLM decoder IS
# the word table), and _HEAD_TABLE's groups.  A unit with no trainable member is not computed; a mixed one is computed whole
# and only its trainable members are exposed, reduced and stepped.
SHARD_FROZEN_MSG = ("shard_optimizer=True serves a model whose parameters all require grad: the ownership plan cuts the whole "
                    "slab, and a frozen parameter would be reduced, updated and gathered with it")
SHARD_STEPS_MSG = ("shard_optimizer=True serves parameters that all took the same number of updates (one bias correction "
                   "per launch); this state counts them differently (it comes from a run that unfroze parameters later)")


def unit_flags(names, flags, num_layers, tied_decoder=True):
    """Which units have a trainable member -> dict(layers=[bool] * L, emb=, region=, mlm=, token=, action=, pooler=).
    names / flags: the slab entries' names and requires_grad.  tied_decoder: the MLM decoder weight is the word table
    (it has no entry of its own), so a trainable word table keeps the "mlm" group computed -- its decoder launch feeds it."""
    group_of = {path: grp for grp, path, _ in _HEAD_TABLE}
    units = dict(layers=[False] * num_layers, emb=False, **{grp: False for grp in _HEAD_GROUPS + ("region",)})
    for n, fl in zip(names, flags):
        if not fl:
            continue
        if n.startswith("bert.encoder.layer."):
            units["layers"][int(n.split(".")[3])] = True
        elif n.startswith("bert.embeddings."):
            units["emb"] = True
            if tied_decoder and n == "bert.embeddings.word_embeddings.weight":
                units["mlm"] = True
        elif n in group_of:
            units[group_of[n]] = True
        else:
            raise KeyError("parameter %s belongs to no unit" % n)
    return units


def backward_stop(layer_flags, below, history_need=None):
    """Where the reverse layer loop may stop -> (lo, need_input_grad): it runs layers L-1 .. lo (none when lo == L), and
    layer lo must produce dL/d(its input) only with need_input_grad.  below: something under the layers wants the gradient
    (a trainable embedding block or region group, a caller's d_hidden); history_need[l]: the history tensor of layer l
    requires grad (its gradient comes out of layer l's last dgrad, which that layer then runs for it)."""
    if below:
        return 0, True
    for l, fl in enumerate(layer_flags):
        if fl or (history_need is not None and history_need[l]):
            return l, False
    return len(layer_flags), False


def merge_spans(spans):
    """[start, end) spans sorted and merged where they touch or overlap."""
    out = []
    for s_, e_ in sorted(spans):
        if out and s_ <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], e_))
        elif e_ > s_:
            out.append((s_, e_))
    return out


def intersect_ranges(ranges, spans):
    """The parts of `ranges` (in their order) inside the sorted disjoint `spans`."""
    out = []
    for s_, e_ in ranges:
        for a_, b_ in spans:
            lo, hi = max(s_, a_), min(e_, b_)
            if hi > lo:
                out.append((lo, hi))
    return out


def step_segments(entries, flags, steps):
    """AdamW's launches over the trainable entries: maximal runs of adjacent spans whose parameters took the same number of
    updates -> [(start, end, updates so far)].  entries: (name, (start, end)) in slab order."""
    segs = []
    for (n, (s_, e_)), fl in zip(entries, flags):
        if not fl:
            continue
        if segs and segs[-1][1] == s_ and segs[-1][2] == steps[n]:
            segs[-1] = (segs[-1][0], e_, steps[n])
        else:
            segs.append((s_, e_, steps[n]))
    return segs


class TrunkState(object):
    """What a trunk forward leaves for its consumers: the heads, the trunk backward, trunk_forward's outputs, the autograd
    nodes and the fp32 step (training_f32 fills the same class).  Nothing else of a forward outlives it: a tensor whose
    address a later launch reads is a field here or belongs to `bufs`.  Fields a path does not use stay None."""

    __slots__ = (
        # ---- shapes
        "B",              # batch size
        "T",              # text positions per sequence
        "R",              # region positions per sequence (0 without img_feats)
        "S",              # T + R
        "H",              # hidden size
        "I",              # intermediate size
        "nh",             # attention heads
        "L",              # encoder layers
        "M",              # B * S, the padded row count
        "Mr",             # rows the encoder ran on: M, or the compacted layout's count
        # ---- layout
        "dev",            # the step's device
        "bufs",           # the (B, S) _TrainBuffers holding the saved activations
        "lay",            # ops.SeqLayout of the compacted rows, None on the padded layout
        "cls_rows",       # int64 [B]: row of each sequence's [CLS] in the layout in use
        "serial",         # number of this forward: a backward must belong to the engine's latest one
        # ---- masks
        "enc_mask",       # what the attention kernels take: centered 2-D mask, additive 3-D bias, None (no mask / compacted)
        "mask_additive",  # enc_mask is the additive [B, S, St] form
        "hs",             # head_mask as per-layer head scales [L, ...], or None
        "mask",           # fp32 step: the mask as its softmax kernel takes it
        "mode",           # fp32 step: that kernel's mask mode (-1 none, 0 [B, S], 2 additive [B, S, S])
        # ---- dropout
        "p_h", "p_a",     # hidden / attention dropout probability of this forward (0 in eval)
        "seed",           # seed of this forward / backward pair
        # ---- inputs
        "ids",            # input_ids int64 [B, T]
        "tt", "pos_ids",  # token_type_ids / position_ids, int64 or None
        "img",            # img_feats as given, None for a text-only batch
        "a_img",          # region projection's packed operand [B*R, kpad] (fp32 step: [B*R, D + 128])
        # ---- kept activations (beside those in bufs)
        "img_pre",        # region rows in front of the image LayerNorm [B*R, H], None without use_img_layernorm
        "x_enc",          # the encoder's input rows in the layout in use
        "seq",            # the last layer's output rows (bf16; fp32 step: fp32 [M, H])
        "cls_seq",        # compacted layout: the [CLS] rows of seq, gathered [B, H]
        "pooled",         # pooler output fp32 [B, H]
        "pooled_bf",      # its bf16 copy, the action head's operand
        "e",              # fp32 step: the embedding sum in front of its LayerNorm [B*T, H]
        "x0",             # fp32 step: the embedding output [M, H] (layer 0's saved input; read through layers[0]["x"])
        "layers",         # fp32 step: per layer the dict of saved activations
        # ---- supervised rows (forward_backward only)
        "lab", "tl",            # labels / token_labels flattened, int64 [M]
        "idx_w", "idx_t",       # the padded rows that carry a label / a token label
        "rows_w", "rows_t",     # the same rows in the layout in use
        "Ml", "Mt",             # their counts
        # ---- history
        "hist",           # _history_state of a forward with encoder_history_states, else None
        "d_history",      # after trunk_backward: per layer dL/d(history[l]) fp32 [B, Sh, H] or None
    )

    def __init__(self, **fields):
        for name in self.__slots__:
            setattr(self, name, fields.pop(name, None))
        if fields:
            raise TypeError("TrunkState has no field %s" % ", ".join(sorted(fields)))


class _TrainBuffers(object):
    """Per-(B,S) activation store and gradient scratch, plus the ctypes tables for the C loops."""

    # the workspace buffers with one row per token (a caller that runs fewer rows slices these); the others are sized otherwise
    ws_rowed = ("g_pre", "g_pre2", "g_mid", "g_ctx", "g_qkv", "g_pre_d", "g_pre2_d")

    def __init__(self, L, M, B, S, H, I, nh, dev):
        mk = lambda n: torch.empty((M, n), dtype=BF16, device=dev)
        # the residual stream at fp16 precision (ops.F16_STREAM): the pre-LayerNorm sums are fp16 tensors (the LayerNorm
        # backward reads them) and every LayerNorm output has a second, fp16 copy that the next residual add reads -- those
        # copies are transient: ONE pair of buffers serves all layers (include/visitron_hip.h, vt_layer_acts::ln1_h)
        mkpre = (lambda: torch.empty((M, H), dtype=ops.F16, device=dev)) if ops.F16_STREAM else (lambda: mk(H))
        # ops.LN_RESIDUAL: no fp16 copies at all -- the residual adds rebuild each LayerNorm from its fp16 input and the row
        # statistics its kernel wrote (4 x [M] fp32 per layer; vt_layer_acts::ln_residual_mode)
        self.ln_residual = bool(ops.LN_RESIDUAL)
        self.ln_h = (mkpre(), mkpre()) if (ops.F16_STREAM and not self.ln_residual) else None
        self.layers = []
        self.acts = (_lib.LayerActs * L)()
        for i in range(L):
            d = dict(qkv=mk(3 * H), ctx=mk(H), attn_pre=mkpre(), attn_out=mk(H), mid_pre=mk(I), mid=mk(I),
                     out_pre=mkpre(), out=mk(H), lse=torch.empty((B, nh, S), dtype=torch.float32, device=dev))
            if self.ln_h is not None:
                d["ln1_h"], d["ln2_h"] = self.ln_h
            if self.ln_residual:
                for k in ("ln1_mean", "ln1_rstd", "ln2_mean", "ln2_rstd"):
                    d[k] = torch.empty(M, dtype=torch.float32, device=dev)
                self.acts[i].ln_residual_mode = 1
            if KEEP_BITS:   # the attention dropout's keep decisions, forward -> backward (25 MB per layer at B = 256)
                d["keep_bits"] = torch.empty(ops.keep_words(B, nh, S), dtype=torch.int32, device=dev)
            self.layers.append(d)
            for k, v in d.items():
                setattr(self.acts[i], k, v.data_ptr())
        self._mk, self._ctx_raw = mk, {}
        self._H = H
        self.x0 = mk(H)
        self.x0c = mk(H)      # compacted copy of x0 (real rows only), the encoder's input in the compact path
        self.g = mk(H)
        self.g_pad = mk(H)    # dL/dx0 scattered back to the padded row order for the embedding / region backward
        self.g_seq32 = torch.empty((M, H), dtype=torch.float32, device=dev)
        self.ws_t = dict(g_pre=mk(H), g_pre2=mk(H), g_mid=mk(I), g_ctx=mk(H), g_qkv=mk(3 * H),
                         g_pre_d=mk(H), g_pre2_d=mk(H),   # dropout-masked copies (hidden dropout > 0)
                         delta=torch.empty((B, nh, S), dtype=torch.float32, device=dev),
                         ln_partial=torch.empty(ops.LN_BWD_WS_ROWS * 2 * H, dtype=torch.float32, device=dev))
        self._dq32_shape = (B, S, nh, M)
        need = ops.attention_bwd_ws_bytes(B, S, nh, M)
        if need:  # attention backward over several key blocks: dQ in fp32 (one slab; one plane per key block when deterministic)
            self.ws_t["dq32"] = torch.empty(need // 4, dtype=torch.float32, device=dev)
        # second set of the buffers a layer's weight-gradient launch reads: with it the wgrad of layer l runs on a side
        # stream beside layer l-1's dgrad chain (vt_encoder_backward_overlap_bf16); the rest is shared
        self.ws_t_b = dict(self.ws_t)
        for k in self.ws_rowed:
            if k != "g_ctx":   # (read by the dgrad chain only)
                self.ws_t_b[k] = mk(self.ws_t[k].shape[1])
        self.ws, self.ws_b = self._workspace(self.ws_t), self._workspace(self.ws_t_b)

    @staticmethod
    def _workspace(tab, ws=None):
        """The library's table of a workspace dict's addresses (a fresh one, or `ws` pointed at the dict's present tensors)."""
        ws = _lib.BwdWorkspace() if ws is None else ws
        for k, v in tab.items():
            setattr(ws, k, v.data_ptr())
        return ws

    def fit_dq32(self):
        """The dQ workspace follows ops.set_deterministic: called in front of every backward, it asks the library what the
        current mode needs and grows the buffer (both workspace tables point at it) when the switch was turned on after the
        buffers were built."""
        need = ops.attention_bwd_ws_bytes(*self._dq32_shape)
        have = self.ws_t.get("dq32")
        if need and (have is None or have.numel() * 4 < need):
            self.ws_t["dq32"] = self.ws_t_b["dq32"] = torch.empty(need // 4, dtype=torch.float32, device=self.x0.device)
            self._workspace(self.ws_t, self.ws)
            self._workspace(self.ws_t_b, self.ws_b)

    def ctx_raw(self, layer):
        """Per-layer buffer for the attention kernel's unscaled context (head_mask in training), allocated on first use."""
        if layer not in self._ctx_raw:
            self._ctx_raw[layer] = self._mk(self._H)
        return self._ctx_raw[layer]


def _history_state(history, B, H, L, dev):
    """encoder_history_states as the unrolled layer sequences carry them: the bf16 rows each layer prepends ("src"), which
    tensors want a gradient ("need"), and per layer what the forward keeps for the backward -- the extended rows "xs"
    [B*St, H], their projection "qkv" [B*St, 3H], the rectangular attention's keep words -- and what the backward leaves,
    "d": fp32 [B, Sh, H] per layer, None where the history tensor does not require grad."""
    history = list(history)
    if len(history) != L:
        raise RuntimeError("encoder_history_states must hold one tensor per layer (%d), got %d" % (L, len(history)))
    Sh = history[0].shape[1]
    for h in history:
        ops._require_hip(h)
        if tuple(h.shape) != (B, Sh, H):
            raise RuntimeError("every encoder_history_states tensor must be [batch, Sh, hidden] = [%d, %d, %d], got %s"
                               % (B, Sh, H, tuple(h.shape)))
    return dict(Sh=Sh, src=[h.detach().to(device=dev, dtype=BF16).contiguous() for h in history],
                need=[bool(h.requires_grad) for h in history], xs=[None] * L, qkv=[None] * L, keep=[None] * L, d=[None] * L)


# one encoder layer of the bf16 engine: t = what the forward reads (GEMM weights in the mirror, vectors in the fp32 slab), gr =
# the same fields in the gradient slab, wt = the transposed copies of the GEMM weights the dgrad GEMMs read
_LayerViews = collections.namedtuple("_LayerViews", "t gr wt")


class _TrunkOnly(torch.nn.Module):
    """A bare BertImgModelwithLocationEmbeds presented to the engine under the parameter names it has inside a
    PreTrainOscar ("bert." + name): train.py:47 hands `model.bert` to the rollout agent, which trains through it."""

    def __init__(self, trunk):
        super().__init__()
        self.bert = trunk
        self.config = trunk.config


class PretrainEngine(object):
    """The training step of a PreTrainOscar (or of its bare trunk) on the HIP kernels; see the module docstring.

    shard_optimizer=True (default False; nothing changes when it is off, and one rank runs the plain step): AdamW sharded
    over the data-parallel ranks.  The gradient all-reduce is a reduce-scatter plus an all-gather; the update sits between
    the halves, so each rank updates 1 / world of the slab, keeps 1 / world of the two moment slabs, and the bytes on the
    wire stay what they were.  Ownership is static (distributed.ShardPlan); world sizes 2, 4 and 8, anything else raises
    ValueError.  The contract, after every step, on every rank:
      * flat.mirror is bit-identical to the replicated engine's;
      * every parameter the step reads as fp32 (the no-decay group, the word / position / token-type tables) is exact;
      * the parameters the step reads only through the mirror (the GEMM weights) are exact on their owner and
        float(bf16(.)) elsewhere: a rank's parameters are always what its own forward computes with, and a later
        refresh_mirror() from them is idempotent;
      * consolidate() -- a COLLECTIVE every rank must call -- all-gathers the owners' fp32 values: all parameters are then
        exact everywhere.  Required before model.state_dict() is written as a checkpoint and before fp32-route inference
        on these weights;
      * state_dict() is a collective too (it gathers the moments) and returns exactly the replicated engine's name-keyed
        format; load_state_dict takes that format and keeps this rank's pieces: the two kinds of run interchange states;
      * all_reduce_grads() raises; optimizer_step() is the un-overlapped collective (reduce-scatter, update, gather).
    Backend nccl: reduce_scatter_tensor / all_gather_into_tensor in place on the slab; any other backend: the bucketed
    all-reduce of the replicated step and the list form of all_gather.  Rehearsed with ranks sharing one device under
    gloo; never run on distinct devices."""

    def __init__(self, model, lr=5e-5, weight_decay=0.05, eps=1e-8, betas=(0.9, 0.999), correct_bias=True,
                 schedule="linear", warmup_steps=0, t_total=20000, process_group=None, bucket_mb=64,
                 loss_scale_by_world=True, attach_grads=True, grad_comm_dtype=None, precision="bf16", shard_optimizer=False):
        # precision: "bf16" (default: the bf16 kernels above) or "fp32" (the reference's training arithmetic: every operand,
        # activation and gradient in fp32 on the fp32 matrix cores, visitron_amd.training_f32).  Independent of
        # set_precision, which selects the inference arithmetic.
        if precision not in ("bf16", "fp32"):
            raise ValueError("precision must be 'bf16' or 'fp32', got %r" % (precision,))
        self.precision = precision
        if isinstance(model, BertImgModelwithLocationEmbeds):
            model = _TrunkOnly(model)    # trunk-level training (the rollout's OscarEncoder owns just the trunk)
        assert isinstance(model, (PreTrainOscar, _TrunkOnly))
        self.has_heads = isinstance(model, PreTrainOscar)
        cfg = model.config
        if cfg.hidden_size != 64 * cfg.num_attention_heads:
            raise NotImplementedError("the HIP training path serves head size 64")
        for p_ in (cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob):
            if not 0.0 <= p_ < 1.0:
                raise ValueError("dropout probability must be in [0, 1)")
        # the attention sites run p in steps of 1 / 65536 (1 / 256 under VT_ATTN_DROPOUT_BITS=8; ops.attn_drop_p raises where a
        # p is not served): the value the
        # step actually uses is recorded in state_dict()["hyper"] and in bench.py's line, not only the configured one
        self.attention_dropout_effective = ops.attn_drop_p(float(cfg.attention_probs_dropout_prob))
        self.model, self.cfg = model, cfg
        self.lr, self.wd, self.eps, self.betas, self.correct_bias = lr, weight_decay, eps, betas, correct_bias
        self.schedule, self.warmup_steps, self.t_total = schedule, warmup_steps, t_total
        self.step_count = 0       # optimizer steps taken (Adam's t)
        self.sched_step = 0       # scheduler.step() calls (LambdaLR's last_epoch)
        self.pg = process_group
        self.world = 1
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(process_group)
        # shard_optimizer: AdamW sharded over the data-parallel ranks (see the class docstring); one rank runs the plain step
        self.shard_optimizer = bool(shard_optimizer)
        self.shard = self.shard_optimizer and self.world > 1
        if self.shard:
            if self.world not in distributed.SHARD_WORLDS:
                raise ValueError("shard_optimizer=True serves world sizes %s (a bucket is cut into `world` pieces of whole "
                                 "8-element groups, and %d does not divide ALIGN / 8 = %d), not %d"
                                 % (distributed.SHARD_WORLDS, self.world, ALIGN // 8, self.world))
        if precision == "fp32" and self.world > 1:
            raise NotImplementedError("PretrainEngine(precision='fp32') serves one rank")
        self.flat = FlatParams(model, attach_grads=attach_grads, moments=not self.shard)
        # updates each parameter has taken (torch's per-parameter state["step"]: a parameter unfrozen later starts its bias
        # correction at its own first update); the tables below follow requires_grad, read at every step (_sync_trainable)
        self.param_steps = {n: 0 for n, _, _, _, _ in self.flat.entries}
        self._flags = None
        self.bucket_elems = int(bucket_mb * 1024 * 1024 // 4)
        self.loss_scale_by_world = loss_scale_by_world
        # data-parallel gradient exchange: the reference's DDP moves 452 MB of fp32 buckets per step (pretrain.py:96-102);
        # here each range of the fp32 gradient slab is cast to a bf16 communication copy as soon as its backward kernels
        # are enqueued, THAT is all-reduced (226 MB: on xGMI a ring is bound per link), and the fused
        # AdamW reads the reduced bf16 gradients into its fp32 moments.  VT_GRAD_COMM=fp32 / grad_comm_dtype="fp32": the
        # fp32 slab itself is all-reduced.
        if grad_comm_dtype is None:
            grad_comm_dtype = switches.text("VT_GRAD_COMM")
        if grad_comm_dtype not in ("bf16", "fp32"):
            raise ValueError("grad_comm_dtype must be 'bf16' or 'fp32'")
        self.grad_comm_dtype = grad_comm_dtype
        self.gemm_policy = "persistent GEMM on every CU (one rank, no collective beside it)"
        self.g16 = None
        if self.world > 1 and grad_comm_dtype == "bf16":
            self.g16 = torch.zeros(self.flat.total, dtype=BF16, device=self.flat.p.device)
        self._bufs = {}
        self._tables = None
        # dropout: masks come from a counter-based hash of (seed, site, element); the seed of a
        # forward/backward pair = base (torch's seed, decorrelated per rank) + number of pairs so far
        rank = torch.distributed.get_rank(process_group) if self.world > 1 else 0
        self.drop_seed_base = (int(torch.initial_seed()) + 0x9E3779B97F4A7C15 * (rank + 1)) & 0xFFFFFFFFFFFFFFFF
        self.fb_count = 0
        self.last_drop_seed = 0
        self._wt_dirty = True
        self._wt_batch = None
        self._wt_batch_moved = None   # (flags, the batch over the matrices with a trainable source)
        # weight gradients on a side stream beside the next layer's dgrad chain: opt-in (VT_OVERLAP_WGRAD=1 or the
        # attribute).  Measured on one GPU: +1 % when the GEMMs are the one-tile-per-workgroup kernels, -1 % with the
        # persistent kernel (its workgroups queue behind the wgrad's and still do a full share each); with a second
        # process on the same GPU it lost a lot, and beside RCCL's kernels it could not be measured here.
        self.overlap_wgrad = switches.on("VT_OVERLAP_WGRAD")
        # one rank: AdamW per parameter range on a side stream under the backward (_train_step_adamw_under_backward)
        self.overlap_adamw = switches.on("VT_OVERLAP_ADAMW")
        self._adam_stream = None
        # the training step on the real rows only (no padding rows; vt_encoder_*_seq_bf16): same losses and gradients
        # as the padded run (tests/test_gpu_train.py); VT_COMPACT_ROWS=0 or the attribute turns it off
        self.compact_rows = switches.on("VT_COMPACT_ROWS")
        self.last_rows = None
        self.last_layout = None
        self._tuned_rows = set()
        # (padded) token rows below which the step stays on the padded layout.  Rounds 2 - 5: 16 384 -- the layout then cost
        # two launches and a host synchronisation of its own.  Since the row counts and lists ride on the step's one
        # synchronisation it wins at every batch measured (round 6, profiles/r06/compaction_by_batch.txt: B = 4 ... 36 x 228
        # +0.2 ... +3.6 %, 8 x 767 +3.2 %), so the default is 0; VT_COMPACT_MIN_ROWS restores a threshold
        self.compact_min_rows = switches.integer("VT_COMPACT_MIN_ROWS")
        self._side_stream = None
        self._fwd_serial = 0      # forwards issued: a backward must belong to the latest one (the buffers are shared)
        if precision == "fp32":
            self.overlap_adamw = False
            training_f32.setup(self)
        else:
            self._build_tables()
        self._sync_trainable()
        self.plan = None
        if self.shard:
            self._shard_setup()

    # ------------------------------------------------------------------------------ tables
    def _sync_trainable(self):
        """requires_grad is read at every step: when the tuple of flags changed (or on the first call) the tables that depend
        on it are rebuilt -- the unit flags, the layer gradient table of the C loop (a frozen layer: null pointers), the
        trainable spans of the slab (what is all-reduced) and AdamW's segments (what is stepped, with which update count)."""
        f = self.flat
        flags = f.flags()
        if self.shard_optimizer and not all(flags):
            raise NotImplementedError(SHARD_FROZEN_MSG)
        if flags == self._flags:
            return
        self._flags = flags
        names = [n for n, _, _, _, _ in f.entries]
        self._trainable = dict(zip(names, flags))
        self.units = unit_flags(names, flags, self.cfg.num_hidden_layers, self.has_heads and self._decoder_tied())
        self.train_spans = merge_spans([f.span[n] for n in names if self._trainable[n]])
        self._rebuild_segments()
        f.reattach_grads()   # a parameter frozen since the last step loses its .grad, an unfrozen one gets its slab view
        if self.precision == "bf16":
            for i, lv in enumerate(self._layers):
                for k, v in lv.gr.items():
                    setattr(self.g_tab[i], "d_" + k, v.data_ptr() if self.units["layers"][i] else None)

    def _rebuild_segments(self):
        f = self.flat
        self.adam_segments = step_segments([(n, f.span[n]) for n, _, _, _, _ in f.entries], self._flags, self.param_steps)
        if self.shard_optimizer and len(set(self.param_steps.values())) > 1:
            raise NotImplementedError(SHARD_STEPS_MSG)

    def _trainable_ranges(self, ranges):
        """The trainable parts of slab ranges (a frozen parameter's range is neither all-reduced nor stepped)."""
        return intersect_ranges(ranges, self.train_spans)

    def _is_trainable(self, param):
        return self._trainable[self._name_of(param)]

    def _build_tables(self):
        self._wt_batch = None
        m, f, cfg = self.model, self.flat, self.cfg
        L, H = cfg.num_hidden_layers, cfg.hidden_size
        self.w_tab = (_lib.LayerWeights * L)()
        self.wt_tab = (_lib.LayerWeightsT * L)()
        self.g_tab = (_lib.LayerGrads * L)()
        self._layers = []        # per layer: _LayerViews of the tensors the three tables point at
        self.layer_ranges = []   # per layer: [(start, end) in the decay region, (start, end) in the no-decay region]
        for i in range(L):
            pre = "bert.encoder.layer.%d." % i
            offs = [(o, o + c) for n_, _, o, c, _ in f.entries if n_.startswith(pre)]
            dec = [r_ for r_ in offs if r_[0] < f.n_decay]
            nod = [r_ for r_ in offs if r_[0] >= f.n_decay]
            self.layer_ranges.append([(min(a_ for a_, _ in dec), max(b_ for _, b_ in dec)),
                                      (min(a_ for a_, _ in nod), max(b_ for _, b_ in nod))])
            t, gr = _layer_views(f, i, f.mirror, f.p), _layer_views(f, i, f.g, f.g)
            wt = {"wt_" + k[2:]: torch.empty(v.shape[::-1], dtype=BF16, device=f.p.device)
                  for k, v in t.items() if k.startswith("w_")}
            self._layers.append(_LayerViews(t, gr, wt))
            for row, views, pre_ in ((self.w_tab[i], t, ""), (self.g_tab[i], gr, "d_"), (self.wt_tab[i], wt, "")):
                for k, v in views.items():
                    setattr(row, pre_ + k, v.data_ptr())
        # non-encoder weights: transposed copies [H, rows padded to the GEMM tile] (a zero column tail) of _HEAD_TABLE's operands
        dev = f.p.device
        # ([H, H] for the square ones; a head's few output rows are padded to the GEMM tile, the column tail stays zero)
        self.head_t = {key: (torch.empty((H, H), dtype=BF16, device=dev) if prm.shape[0] == H else
                             torch.zeros((H, round_up(prm.shape[0], 64)), dtype=BF16, device=dev))
                       for _, prm, key in self._head_rows() if key}
        if self.has_heads:
            self.Vp, self.Cp, self.Ap = (self.head_t[k].shape[1] for k in ("dec", "tok", "act"))
        D = m.bert.img_dim
        self.kpad = round_up(D + 128, 64)
        self.w_img = torch.zeros((H, self.kpad), dtype=BF16, device=dev)
        self.b_img = torch.zeros(H, dtype=torch.float32, device=dev)
        self.dw_img = torch.zeros((H, self.kpad), dtype=torch.float32, device=dev)
        self.db_img = torch.zeros(H, dtype=torch.float32, device=dev)

    def _head_rows(self, *groups):
        """_HEAD_TABLE's rows (group, parameter, transposed copy) that exist in this model, of the named groups (all if none)."""
        m, rows = self.model, []
        for grp, path, key in _HEAD_TABLE:
            if (groups and grp not in groups) or not (self.has_heads or path.startswith("bert.")):
                continue
            if path.startswith("bert.LayerNorm.") and not getattr(m.bert, "use_img_layernorm", None):
                continue
            rows.append((grp, m.get_parameter(path), key))
        return rows

    def _decoder_tied(self):
        return self.model.mlmhead.predictions.decoder.weight is self.model.bert.embeddings.word_embeddings.weight

    def _head_group(self, *groups):
        """The parameters of the named _HEAD_TABLE groups whose gradients belong to that group alone: a tied MLM decoder IS
        the word table, whose gradient the embedding backward also adds to -- it is zeroed, reduced and updated with the
        embeddings, never with the heads."""
        word = self.model.bert.embeddings.word_embeddings.weight
        return [prm for _, prm, _ in self._head_rows(*groups) if prm is not word]

    def _zero_head_grads(self, *groups):
        """Zero gradients for the named groups: nothing in this step supervises them (both engines)."""
        for prm in self._head_group(*groups):
            self._grad(prm).zero_()

    def _name_of(self, param):
        for n, p, _, _, _ in self.flat.entries:
            if p is param:
                return n
        raise KeyError("parameter not in the flat layout")

    def _mirror(self, param):
        return self.flat.view(self.flat.mirror, self._name_of(param))

    def _grad(self, param):
        return self.flat.view(self.flat.g, self._name_of(param))

    def refresh_derived_weights(self):
        """Transposed / packed bf16 copies that the dgrad GEMMs and the region projection read.  _wt_dirty: True = all of them
        (a new engine, parameters written from outside the step); a tuple of flags = the engine's own AdamW ran under those
        requires_grad flags, so only the copies of matrices with a source that was trainable THEN changed -- a frozen
        matrix's copy is not rebuilt."""
        if self.flat.mirror_is_stale():
            self.flat.refresh_mirror()
            self._wt_dirty = True
        if not self._wt_dirty:
            return
        m, D = self.model, self.model.bert.img_dim
        if self._wt_batch is None:   # all layers' four matrices + the head matrices: one launch
            self._wt_batch = ops.TransposeBatch([(src, dst) for src, dst, _ in self._transpose_pairs(self._flags)])
        stepped = self._wt_dirty
        moved_only = stepped is not True and not all(stepped)
        region_moved = True
        if moved_only:
            if self._wt_batch_moved is None or self._wt_batch_moved[0] != stepped:
                pairs = [(src, dst) for src, dst, moved in self._transpose_pairs(stepped) if moved]
                self._wt_batch_moved = (stepped, ops.TransposeBatch(pairs) if pairs else None)
            if self._wt_batch_moved[1] is not None:
                self._wt_batch_moved[1].run()
            region_moved = any(fl for (n, _, _, _, _), fl in zip(self.flat.entries, stepped)
                               if n.startswith(("bert.img_embedding.", "bert.location_embeds.")))
        else:
            self._wt_batch.run()
        if region_moved:
            self.w_img[:, :D].copy_(self._mirror(m.bert.img_embedding.weight))
            self.w_img[:, D:D + 128].copy_(self._mirror(m.bert.location_embeds.weight))
            torch.add(m.bert.img_embedding.bias.detach(), m.bert.location_embeds.bias.detach(), out=self.b_img)
        self._wt_dirty = False

    def _transpose_pairs(self, flags):
        """(source in the mirror, transposed copy, does a parameter trainable under `flags` lie in the source) for every
        layer's four matrices and the head matrices, in the batch's order."""
        out, trainable = [], dict(zip((n for n, _, _, _, _ in self.flat.entries), flags))
        for l, lv in enumerate(self._layers):
            pre = "bert.encoder.layer.%d." % l
            for k, dst in lv.wt.items():
                field = "w_" + k[3:]
                names = [_LAYER_PACKED[field] % x for x in _QKV] if field in _LAYER_PACKED else [_LAYER_FIELDS[field]]
                out.append((lv.t[field], dst, any(trainable[pre + n] for n in names)))
        out += [(self._mirror(prm), self.head_t[key], trainable[self._name_of(prm)]) for _, prm, key in self._head_rows() if key]
        return out

    def _buffers(self, B, S):
        key = (B, S)
        b = self._bufs.get(key)
        if b is None:
            cfg = self.cfg
            if len(self._bufs) >= 2:
                self._bufs.clear()
            b = _TrainBuffers(cfg.num_hidden_layers, B * S, B, S, cfg.hidden_size, cfg.intermediate_size,
                              cfg.num_attention_heads, self.flat.p.device)
            if self.world > 1 or switches.on("VT_FORCE_MULTI_RANK_GEMM"):
                # collectives share the CUs with the backward: ops.multi_rank_gemm_policy decides once whether the persistent
                # GEMM keeps running (on CUs - k workgroups: opt-in, VT_GEMM_RESERVE_CUS=k) or stands down for the
                # one-tile-per-workgroup kernels (default); bench.py prints the choice.  VT_FORCE_MULTI_RANK_GEMM=1 applies the
                # policy on ONE rank: the profiled single-rank twin of each multi-GPU kernel mix (profiles/r05/bench_b36_*.json)
                k, self.gemm_policy = ops.multi_rank_gemm_policy()
                if k > 0:
                    _lib.load().vt_gemm_reserve_cus(k)
                else:
                    ops.PERSISTENT_GEMM_OK = False
            self._bufs[key] = b
        # GEMM choices of the padded row count, once per mode: under ops.set_deterministic they come from the committed table
        # (no timing launches), so a switch turned on later re-registers them
        tkey = ("padded", B * S, ops.is_deterministic())
        if tkey not in self._tuned_rows:
            ops.autotune_encoder_shapes(B * S, self.cfg.hidden_size, self.cfg.intermediate_size, training=True,
                                        device=self.flat.p.device)
            self._tuned_rows.add(tkey)
        return b

    # ------------------------------------------------------------------------------ schedule
    def lr_factor(self):
        s = self.sched_step
        if self.schedule == "constant":
            return float(s) / float(max(1.0, self.warmup_steps)) if s < self.warmup_steps else 1.0
        if s < self.warmup_steps:
            return float(s) / float(max(1, self.warmup_steps))
        return max(0.0, float(self.t_total - s) / float(max(1.0, self.t_total - self.warmup_steps)))

    # ------------------------------------------------------------------------------ forward + backward
    def _trunk_fwd(self, batch, head_mask, labels, token_labels, training, allow_compact, comm=None, history=None):
        """The trunk's forward (embeddings, region projection, encoder layers, pooler) with every activation the backward
        needs kept in the (B, S) buffer set; returns the step's state (a TrunkState, filled field by field at the end).  labels /
        token_labels (optional): the supervised rows are located here, where the host synchronises anyway.
        history (optional): encoder_history_states, one [B, Sh, H] tensor per layer -- layer l's keys and values run over
        cat([history[l], hidden], 1) (oscar/modeling_bert.py:37-41, 148-155) and the mask covers those Sh + S keys."""
        m, cfg, f = self.model, self.cfg, self.flat
        self._require_ownership()
        f.reattach_grads()
        ids = _i64(batch["input_ids"])
        dev = ids.device
        B, T = ids.shape
        img = batch.get("img_feats")
        R = 0 if img is None else img.shape[1]
        packed = batch.get("img_packed")
        if packed is not None:   # the region projection's operand as RegionStore.pretrain_batch(packed=True) wrote it
            R = ops.packed_region_rows(packed, batch.get("img_rows"), img, B, self.kpad, dev)
            img = packed if R > 0 else None   # (read only as "this batch has regions")
        S, H, I, nh, L = T + R, cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_hidden_layers
        M = B * S
        hist = None
        if history:
            assert img is None, "Cannot take image features while using encoder history states"   # encoder.py:271-274
            if allow_compact:
                raise NotImplementedError("encoder_history_states together with row compaction (unmasked_only) is not served")
            if comm is not None:
                raise NotImplementedError("encoder_history_states together with the chunked data-parallel backward is not served")
            hist = _history_state(history, B, H, L, dev)
        St = S + (0 if hist is None else hist["Sh"])
        am = batch.get("attention_mask")
        mask = None if am is None else am.to(torch.float32).contiguous()
        mask_additive = False
        if mask is not None and mask.dim() == 3:   # per-query mask -> additive bias [B, S, S] (encoder.py:228-229, :238-241)
            if mask.shape != (B, S, St):
                raise RuntimeError("3-D attention_mask must be [batch, text+region, text+region]" if hist is None else
                                   "3-D attention_mask must be [batch, text, history+text]")
            mask = ((1.0 - mask) * -10000.0).contiguous()
            mask_additive = True
        elif mask is not None and mask.shape != (B, St):
            raise RuntimeError("attention_mask must be [batch, text+region]" if hist is None else
                               "attention_mask must be [batch, history+text]")
        from .modeling import _centered_mask, _head_scale
        if mask is not None and not mask_additive:
            mask = _centered_mask(mask)   # one constant per sequence off the additive bias: same softmax, well-scaled numbers
        hs = _head_scale(head_mask, cfg.num_hidden_layers, cfg.num_attention_heads, ids.device)
        if hs is not None and comm is not None:
            raise NotImplementedError("head_mask together with the chunked data-parallel backward")
        tt, pos_ids = _i64(batch.get("token_type_ids")), _i64(batch.get("position_ids"))
        bufs = self._buffers(B, S)
        emb = m.bert.embeddings
        eps = emb.LayerNorm.variance_epsilon
        # dropout (nn.Dropout follows the module's training flag): same (p, seed) in forward and backward
        p_h = float(cfg.hidden_dropout_prob) if training else 0.0
        p_a = float(cfg.attention_probs_dropout_prob) if training else 0.0
        seed = (self.drop_seed_base + self.fb_count) & 0xFFFFFFFFFFFFFFFF
        self.fb_count += 1
        self.last_drop_seed = seed
        # the text embeddings go first: their out-of-range flag is then ready when the host synchronises below
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.embed_layernorm(ids, tt, pos_ids, emb.word_embeddings.weight.detach(), emb.position_embeddings.weight.detach(),
                            emb.token_type_embeddings.weight.detach(), emb.LayerNorm.weight.detach(),
                            emb.LayerNorm.bias.detach(), eps, bufs.x0, S, err_flag=err, drop=(p_h, seed, ops.SITE_EMB))
        # Everything the host must know about this batch before it can size the step -- the numbers of supervised rows
        # (the heads run on those only), the number of rows with a non-zero mask and whether the batch qualifies for the
        # compacted layout, the embedding kernel's out-of-range flag -- is reduced on the device and read back in ONE
        # synchronisation, at the start of the step (ops.batch_row_counts); the row lists and the compacted layout are then
        # written to their known sizes by a second launch (ops.batch_row_lists).
        lab = tl = idx_w = idx_t = None
        Ml = Mt = 0
        if labels is not None:
            lab, tl = _i64(labels.reshape(-1)), _i64(token_labels.reshape(-1))
        # rows nothing in the step reads: positions with attention mask 0.  As keys they weigh exactly 0, so their
        # hidden states reach no loss and their gradient is exactly 0 -- drop them from every row-wise kernel.  Needs a
        # 0/1 mask, the [CLS] position and every supervised position kept; otherwise the padded path below.
        try_compact = (allow_compact and self.compact_rows and mask is not None and mask.dim() == 2 and hs is None
                       and M >= self.compact_min_rows)
        cmask = mask.contiguous() if try_compact else None
        early = not switches.on("VT_STEP_OVERLAP_READBACK")   # A/B switch: the transposes first, as before round 6
        if early:
            self.refresh_derived_weights()
        counts = ops.batch_row_counts_begin(lab, tl, cmask, err, B, S)   # the step's one host synchronisation ...
        # ... and while its seven numbers travel to the host on a side stream, the device transposes the step's weights (the
        # copies the dgrad GEMMs read: ~95 us that used to run BEFORE the counting kernel, with the GPU idle behind it for the
        # 250 us the host needed for this read-back, three more blocking 4-byte reads and the launches that follow)
        if not early:
            self.refresh_derived_weights()
        vals, tiles = ops.batch_row_counts_end(counts)
        # out-of-range input_ids / position_ids / token_type_ids: the reference's embedding lookup raises IndexError
        # (checked before anything indexes the gradient tables with those ids)
        if vals[0] != 0:
            raise IndexError("index out of range in BertEmbeddings (input_ids / position_ids / token_type_ids)")
        # the previous step's weight gradients: a workgroup of the persistent wgrad kernel that gave up its bounded wait
        # for a dW tile added out of turn (never seen; a preempted / shared GPU could do it) -- fail loudly
        late = int(vals[5])       # (vt_step_counters: read and cleared on the device, delivered with the row counts)
        if late:
            raise RuntimeError("vt_wgrad_bf16: %d workgroup(s) ran out of their turn wait in an earlier launch; the weight "
                               "gradients of that step are unreliable" % late)
        late = int(vals[6])       # the same for the persistent GEMM's shared tiles (kernel variants 28 .. 32)
        if late:
            raise RuntimeError("vt_linear: %d finishing workgroup(s) of shared GEMM tiles ran out of their wait in an earlier "
                               "launch; that step's activations / gradients are unreliable" % late)
        Ml, Mt = (int(vals[1]), int(vals[2])) if labels is not None else (0, 0)
        compact = try_compact and int(vals[3]) < M and not vals[4]
        det = ops.is_deterministic()   # read per step (the tuned-shape keys below carry it: a later switch re-registers)
        lay = None
        if labels is not None or compact:   # one launch: the supervised-row lists and the compacted layout
            idx_w, idx_t, lay = ops.batch_row_lists(lab, tl, cmask if compact else None, B, S, Ml, Mt, int(vals[3]), tiles)
        Mr = M if lay is None else lay.rows
        self.last_rows = Mr
        self.last_layout = lay
        if lay is not None:
            # the tile quantisation changes with the row count: tune once per bucket of 256 rows (512 below 16 384 rows), at
            # the bucket's upper edge; the library then takes the nearest tuned M.  Rounds 2 - 5 used 2048-row buckets, whose
            # upper edge is another tile count altogether: 7 091 real rows of a B = 36 batch are 28 row tiles of 256, 8 192 are
            # 32 (QKV: 252 tiles = one round against 288 = two); 50 845 rows of the B = 256 batch are 199, 51 200 are 200 (QKV:
            # 1 791 tiles = 7.00 rounds against 1 800 = 7.03, i.e. eight).  profiles/r06/tune_bucket_ab.txt: +1.9 % / +0.6 %.
            bucket = round_up(Mr, switches.integer("VT_TUNE_BUCKET_LARGE" if Mr >= 16384 else "VT_TUNE_BUCKET_SMALL"))
            if (bucket, det) not in self._tuned_rows and bucket < M:
                ops.autotune_encoder_shapes(bucket, H, I, training=True, device=dev)
                self._tuned_rows.add((bucket, det))
        # the MLM head's two wide GEMMs ([Ml, 768] x [768, 30528] and back) are tuned like the encoder's, once per bucket of
        # 512 supervised rows (the row count changes from batch to batch; the library takes the nearest tuned M)
        if Ml:
            hb = round_up(Ml, 512)
            if ("head", hb, det) not in self._tuned_rows:
                ops.autotune_linear(hb, self.Vp, H, device=dev, out_f32=True)
                ops.autotune_linear(hb, H, self.Vp, device=dev)
                self._tuned_rows.add(("head", hb, det))
        rows_w = rows_t = None
        if labels is not None:   # supervised rows in the layout in use
            rows_w = idx_w if lay is None else lay.inverse.index_select(0, idx_w)
            rows_t = idx_t if lay is None else lay.inverse.index_select(0, idx_t)
        cls_rows = (torch.arange(B, device=dev) * S) if lay is None else lay.start.to(torch.int64)

        # ---------------- forward ----------------
        x0 = bufs.x0
        a_img = img_pre = None
        if img is not None:
            a_img = packed if packed is not None else ops.pack_concat(
                img.reshape(B * R, -1).float().contiguous(),
                batch["img_location_embeddings"].reshape(B * R, -1).float().contiguous(), self.kpad)
            if getattr(m.bert, "use_img_layernorm", None):
                # encoder.py:280-284: LayerNorm on the summed image embedding, THEN dropout; the pre-LayerNorm rows are
                # kept (compact [B*R, H]) for the backward pass
                ln = m.bert.LayerNorm
                img_pre = ops.linear(a_img, self.w_img, self.b_img)
                img_ln = ops.layernorm(img_pre, ln.weight.detach(), ln.bias.detach(), ln.variance_epsilon)
                if p_h > 0.0:
                    ops.apply_dropout(img_ln, (p_h, seed, ops.SITE_IMG))
                x0.view(B, S, H)[:, T:].copy_(img_ln.view(B, R, H))
            else:
                ops.linear(a_img, self.w_img, self.b_img, out=x0[T:], ldc=H, grp_rows=R, grp_stride=S,
                           drop=(p_h, seed, ops.SITE_IMG))
        x_enc, enc_mask = x0, mask
        if lay is not None:
            x_enc, enc_mask = bufs.x0c[:Mr], None
            torch.index_select(x0, 0, lay.index, out=x_enc)
        if hist is not None or ops.profiling() or hs is not None:
            self._encoder_forward_unrolled(bufs, x_enc, enc_mask, B, S, p_h, p_a, seed, lay, mask_additive, hs, hist=hist)
        else:
            ops.encoder_forward(self.w_tab, bufs.acts, x_enc, enc_mask, mask_additive, None, B, S, H, nh, I,
                                cfg.layer_norm_eps, p_hidden=p_h, p_attn=p_a, drop_seed=seed, seq=lay)
        seq = bufs.layers[-1]["out"][:Mr]
        # the [CLS] rows: every S-th row of the padded layout (a row stride), gathered from the compacted one
        cls_seq = None if lay is None else seq.index_select(0, cls_rows)
        pooled = ops.linear(seq if lay is None else cls_seq, self._mirror(m.bert.pooler.dense.weight),
                            m.bert.pooler.dense.bias.detach(), act=ACT_TANH, out_f32=True,
                            **(dict(M=B, lda=S * H) if lay is None else {}))
        self._fwd_serial += 1
        return TrunkState(
            B=B, T=T, R=R, S=S, H=H, I=I, nh=nh, L=L, M=M, Mr=Mr,
            dev=dev, bufs=bufs, lay=lay, cls_rows=cls_rows, serial=self._fwd_serial,
            enc_mask=enc_mask, mask_additive=mask_additive, hs=hs, p_h=p_h, p_a=p_a, seed=seed,
            ids=ids, tt=tt, pos_ids=pos_ids, img=img, a_img=a_img, img_pre=img_pre,
            x_enc=x_enc, seq=seq, cls_seq=cls_seq, pooled=pooled, pooled_bf=pooled.to(BF16),
            lab=lab, tl=tl, idx_w=idx_w, idx_t=idx_t, rows_w=rows_w, rows_t=rows_t, Ml=Ml, Mt=Mt, hist=hist)

    def forward_backward(self, batch, grad_scale=1.0, accumulate=False, comm=None, head_mask=None, backward=True):
        """One forward + backward; gradients of `grad_scale * loss` land in the flat slab (p.grad).
        Returns the reference's 7-tuple (0-d fp32 tensors).  attention_mask: [B, S] (any numeric values, the reference's
        (1 - m) * -10000 arithmetic) or the reference's 3-D form [B, S, S] (encoder.py:228-229); head_mask as the
        reference takes it (encoder.py:248-265; the layer loop then runs op by op: the head scaling sits between the
        attention kernel and the output projection in both directions).  backward=False: the forward and its 7-tuple only."""
        self._sync_trainable()
        if self.precision == "fp32":   # (honours requires_grad in what it exposes and steps; computes every gradient)
            if comm is not None:
                raise NotImplementedError("PretrainEngine(precision='fp32') serves one rank")
            return training_f32.forward_backward(self, batch, grad_scale, accumulate, head_mask, backward)
        st = self._trunk_fwd(batch, head_mask, batch["labels"], batch["token_labels"], self.model.training, True, comm)
        out, kept = self._heads_forward(st, batch, grad_scale)
        if not backward:   # train() under torch.no_grad(): the forward with its dropout, nothing else
            return out
        acc = bool(accumulate)
        self._heads_backward(st, kept, acc)
        if comm is not None:
            # data-parallel: the head / pooler gradients are final here, before the encoder backward has started -- their
            # all-reduce goes out first and hides under the whole backward (round 3 reduced them last, with the embeddings)
            rng = self._param_ranges(self._head_params())
            comm["launch"](rng)
            comm["done"].extend(rng)
        self._trunk_bwd(st, None, acc, comm, word_grad_ready=True)
        return out

    def _heads_forward(self, st, batch, grad_scale):
        """The heads on the supervised rows only -> (the reference's 7-tuple, what _heads_backward reads: per head a dict of
        its operands and of d(grad_scale * loss) / d(logits), None for a head nothing supervises in this batch)."""
        m, cfg, dev, seq = self.model, self.cfg, st.dev, st.seq
        Ml, Mt, H = st.Ml, st.Mt, st.H
        V, C, A = cfg.vocab_size, cfg.detector_classes, cfg.action_space
        pr = m.mlmhead.predictions
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        mlm = tok = act = None
        if Ml > 0:
            seq_w = seq.index_select(0, st.rows_w)
            y_w = st.lab.index_select(0, st.idx_w)
            h_t = torch.empty((Ml, H), dtype=BF16, device=dev)
            t1 = ops.linear(seq_w, self._mirror(pr.transform.dense.weight), pr.transform.dense.bias.detach(), act=ACT_GELU,
                            pre_act_out=h_t)
            t2 = ops.layernorm(t1, pr.transform.LayerNorm.weight.detach(), pr.transform.LayerNorm.bias.detach(),
                               pr.transform.LayerNorm.variance_epsilon)
            logits = torch.empty((Ml, self.Vp), dtype=torch.float32, device=dev)
            ops.linear(t2, self._mirror(pr.decoder.weight), pr.bias.detach(), out=logits, out_f32=True)
            # fused CE: per-row loss, argmax and the gradient (softmax - onehot) * grad_scale / Ml in one kernel
            dl = torch.empty((Ml, self.Vp), dtype=BF16, device=dev)
            loss_rows, amax_w = ops.ce_softmax_rows(logits, y_w, V, dl, float(grad_scale) / Ml)
            mask_loss = loss_rows.mean()
            words_acc = (amax_w == y_w).sum().float() / Ml
            mlm = dict(x=seq_w, h_t=h_t, t1=t1, t2=t2, dl=dl)
        else:
            mask_loss, words_acc = zero / zero, zero / zero  # CrossEntropyLoss over no valid target is nan, as in the reference
        lin_tok = m.token_head[0]
        if Mt > 0:
            seq_t = seq.index_select(0, st.rows_t)
            y_t = st.tl.index_select(0, st.idx_t)
            lt = torch.empty((Mt, self.Cp), dtype=torch.float32, device=dev)
            ops.linear(seq_t, self._mirror(lin_tok.weight), lin_tok.bias.detach(), out=lt, out_f32=True)
            # token_head = Linear + Softmax and the criterion applies log-softmax AGAIN: loss, argmax and the gradient
            # through both softmaxes in one kernel
            dlt = torch.empty((Mt, self.Cp), dtype=BF16, device=dev)
            tok_rows, amax_t = ops.ce_double_softmax_rows(lt, y_t, C, dlt, float(grad_scale) / Mt)
            token_loss = tok_rows.mean()
            token_acc = (amax_t == y_t).sum().float() / Mt
            tok = dict(x=seq_t, dl=dlt)
        else:
            token_loss, token_acc = zero / zero, zero / zero
        la = torch.empty((st.B, self.Ap), dtype=torch.float32, device=dev)
        ops.linear(st.pooled_bf, self._mirror(m.next_action.linear.weight), m.next_action.linear.bias.detach(), out=la,
                   out_f32=True)
        next_action = batch.get("next_action")
        if next_action is not None:
            # LogSoftmax head under a CrossEntropyLoss that applies log_softmax again (encoder.py:142-151, 387-391): loss,
            # accuracy and d(grad_scale * loss)/d(logits) in one launch
            next_loss, action_acc, dla_bf = ops.action_head(la, _i64(next_action), A, float(grad_scale), self.Ap)
            act = dict(dl=dla_bf)
        else:
            next_loss, action_acc = 0, 0
        loss = mask_loss + next_loss + token_loss
        return (loss, mask_loss, next_loss, token_loss, words_acc, action_acc, token_acc), (mlm, tok, act)

    def _heads_backward(self, st, kept, acc):
        """Back through the heads: their gradients into the flat slab (a head without supervision: zeros, unless the step
        accumulates) and dL/d(sequence output) into bufs.g, where the trunk backward reads it."""
        m, cfg, bufs = self.model, self.cfg, st.bufs
        B, S, H, Ml, Mt, seq = st.B, st.S, st.H, st.Ml, st.Mt, st.seq
        V, C, A = cfg.vocab_size, cfg.detector_classes, cfg.action_space
        mlm, tok, act = kept
        pr, lin_tok, emb = m.mlmhead.predictions, m.token_head[0], m.bert.embeddings
        # frozen units: a head group without a trainable member launches no weight gradient, and where nothing in the trunk
        # wants dL/d(sequence output) either (st-independent: _trunk_wants_grad) the head's dgrad is not launched
        un, below = self.units, self._trunk_wants_grad(st)
        # dL/d(sequence output): zero except at the supervised / [CLS] rows.  Assembled directly in the bf16 buffer the
        # encoder backward reads (a row normally belongs to one head; where two heads meet the sum is formed in bf16)
        g16 = bufs.g[:st.Mr]
        g16.zero_()
        wg = lambda dy, x, dw, db: dict(dy=dy, x=x, dw=dw, db=db, accumulate=acc)
        dec_w_is_tied = self._decoder_tied()
        word_grad = self._grad(emb.word_embeddings.weight)
        # The word table's gradient receives the embedding backward's run sums later on (_trunk_bwd), so it must hold
        # defined values before that: with a tied decoder and supervised rows the decoder's weight gradient -- the first
        # thing written into it -- simply overwrites all of it (no 94 MB fill, no read-back by an accumulating launch)
        dec_overwrites = dec_w_is_tied and Ml > 0 and pr.decoder.weight.shape[0] == emb.word_embeddings.weight.shape[0]
        # (a frozen word table: its range of the slab is scratch that nothing exposes, reduces or steps -- the 94 MB fill is
        # dropped; a mixed "mlm" group or embedding block still writes into it, as units are computed whole)
        if not acc and not dec_overwrites:
            if self._is_trainable(emb.word_embeddings.weight):
                word_grad.zero_()
            if dec_w_is_tied and un["mlm"]:
                self._grad(pr.bias).zero_()  # shares the accumulate flag of the tied decoder weight below
        if mlm is not None and not (un["mlm"] or below):
            pass   # frozen head over a trunk that wants nothing from it
        elif mlm is not None and not un["mlm"]:
            # frozen head, trainable trunk: the dgrad chain alone (the LayerNorm backward in its dx-only form)
            dl, t1 = mlm["dl"], mlm["t1"]
            ks = ops.splitk_for(Ml, H, self.Vp)
            g_t2 = ops.linear_splitk(dl, self.head_t["dec"], ks) if ks else ops.linear(dl, self.head_t["dec"])
            g_t1 = ops.layernorm_bwd(t1, g_t2, pr.transform.LayerNorm.weight.detach(), pr.transform.LayerNorm.variance_epsilon,
                                     None, None)
            g_ht = ops.dgelu_mul(g_t1, mlm["h_t"])
            g16.index_add_(0, st.rows_w, ops.linear(g_ht, self.head_t["tr"]))
        elif mlm is not None:
            dl, t1, t2 = mlm["dl"], mlm["t1"], mlm["t2"]
            dec_grad = self._grad(pr.decoder.weight)
            ops.wgrad([dict(dy=dl[:, :V], x=t2, dw=dec_grad, db=self._grad(pr.bias),
                            accumulate=acc or (dec_w_is_tied and not dec_overwrites))], Ml)
            # d(logits)[Ml, Vp] . W_dec[Vp, H]: 51 output tiles for 477 K-steps -- the K-steps are split over the chip
            ks = ops.splitk_for(Ml, H, self.Vp)
            g_t2 = ops.linear_splitk(dl, self.head_t["dec"], ks) if ks else ops.linear(dl, self.head_t["dec"])
            g_t1 = ops.layernorm_bwd(t1, g_t2, pr.transform.LayerNorm.weight.detach(), pr.transform.LayerNorm.variance_epsilon,
                                     self._grad(pr.transform.LayerNorm.weight), self._grad(pr.transform.LayerNorm.bias),
                                     ws=bufs.ws_t["ln_partial"], accumulate=acc)
            g_ht = ops.dgelu_mul(g_t1, mlm["h_t"])
            ops.wgrad([wg(g_ht, mlm["x"], self._grad(pr.transform.dense.weight), self._grad(pr.transform.dense.bias))], Ml)
            if below:
                g16.index_add_(0, st.rows_w, ops.linear(g_ht, self.head_t["tr"]))
        elif not acc:
            # no supervised MLM row (the loss is NaN, as the reference's): the head's gradients must not keep the
            # previous step's values (a tied decoder's weight -- the word table -- was zeroed above)
            self._zero_head_grads("mlm")
        if tok is not None:
            if un["token"]:
                ops.wgrad([wg(tok["dl"][:, :C], tok["x"], self._grad(lin_tok.weight), self._grad(lin_tok.bias))], Mt)
            if below:
                g16.index_add_(0, st.rows_t, ops.linear(tok["dl"], self.head_t["tok"]))
        elif not acc:
            self._zero_head_grads("token")
        if act is not None:
            dla_bf, pooled = act["dl"], st.pooled
            if un["action"]:
                ops.wgrad([wg(dla_bf[:, :A], st.pooled_bf, self._grad(m.next_action.linear.weight),
                              self._grad(m.next_action.linear.bias))], B)
            if un["pooler"] or below:
                g_pooled = ops.linear(dla_bf, self.head_t["act"], out_f32=True)
                g_z = (g_pooled * (1.0 - pooled * pooled)).to(BF16)
            if un["pooler"]:
                ops.wgrad([wg(g_z, seq.view(B, S * H)[:, :H] if st.lay is None else st.cls_seq,
                              self._grad(m.bert.pooler.dense.weight), self._grad(m.bert.pooler.dense.bias))], B)
            if below:
                g16.index_add_(0, st.cls_rows, ops.linear(g_z, self.head_t["pool"]))
        elif not acc:
            self._zero_head_grads("action", "pooler")

    def _head_params(self):
        """The head / pooler parameters whose gradients are final before the encoder backward starts."""
        return self._head_group(*_HEAD_GROUPS)

    def _param_ranges(self, params):
        """Slab ranges [start, end) of the trainable ones among the given parameters, ends rounded up to the alignment
        granule (the padding belongs to no parameter), sorted and merged where they touch."""
        f, spans = self.flat, []
        for prm in params:
            name = self._name_of(prm)
            if not self._trainable[name]:
                continue
            o, cnt, _ = f.off[name]
            spans.append((o, min(round_up(o + cnt, ALIGN), f.total)))
        return merge_spans(spans)

    def _layer_chunk_ranges(self, lo, hi):
        """The decay and the no-decay slab range of layers [lo, hi), ends rounded up to the slab's alignment granule (the
        padding belongs to no parameter) -- their trainable parts."""
        return self._trainable_ranges(
            [(self.layer_ranges[lo][k][0], min(round_up(self.layer_ranges[hi - 1][k][1], ALIGN), self.flat.total))
             for k in (0, 1)])

    def _trunk_wants_grad(self, st, d_hidden=None):
        """Does anything in the trunk read dL/d(sequence output)?  A trainable layer, embedding block or region group (the
        latter with regions in the batch only), a caller's d_hidden, a history tensor that requires grad."""
        un = self.units
        return bool(any(un["layers"]) or un["emb"] or (un["region"] and st.img is not None) or d_hidden is not None
                    or (st.hist is not None and any(st.hist["need"])))

    def _backward_stop(self, st, d_hidden=None):
        """backward_stop for the forward `st`: (lowest layer the backward visits, whether it must produce dL/d(its input))."""
        un = self.units
        below = un["emb"] or (un["region"] and st.img is not None) or d_hidden is not None
        return backward_stop(un["layers"], below, None if st.hist is None else st.hist["need"])

    def _trunk_bwd(self, st, g32, acc, comm=None, word_grad_ready=False, d_hidden=None):
        """Back through the trunk: g32 fp32 [rows, H] = dL/d(sequence output) in the layout of the forward (st), or None
        when the caller has already put it (bf16) into bufs.g; the gradients of the encoder layers, the embeddings and the
        region projection land in the flat slab.  Frozen units are not computed, and the layer loop stops at the lowest
        layer under which nothing wants a gradient (_backward_stop)."""
        if st.serial != self._fwd_serial:
            raise RuntimeError("the activations of this forward were overwritten by a later forward of the same engine; "
                               "run backward before the next forward")
        m, bufs = self.model, st.bufs
        emb = m.bert.embeddings
        B, T, R, S, H, L, Mr, lay = st.B, st.T, st.R, st.S, st.H, st.L, st.Mr, st.lay
        p_h, seed, ids, tt, pos_ids, img = st.p_h, st.seed, st.ids, st.tt, st.pos_ids, st.img
        un = self.units
        stop, need_dx = self._backward_stop(st, d_hidden)
        word_grad = self._grad(emb.word_embeddings.weight)
        if not acc and not word_grad_ready and self._is_trainable(emb.word_embeddings.weight):
            word_grad.zero_()
        g = bufs.g[:Mr]
        if g32 is not None:
            g.copy_(g32)
        bufs.fit_dq32()   # (the deterministic switch is read here, per backward: no copy of it is kept)
        if d_hidden is not None and comm is not None:
            raise NotImplementedError("gradients of intermediate hidden states together with the chunked data-parallel backward")
        if st.hist is not None and comm is not None:
            raise NotImplementedError("encoder_history_states together with the chunked data-parallel backward is not served")
        if st.hist is not None or ops.profiling() or st.hs is not None:
            self._encoder_backward_unrolled(bufs, st.x_enc, st.enc_mask, g, B, S, acc, p_h, st.p_a, seed, lay, st.mask_additive,
                                            st.hs, inject=d_hidden, hist=st.hist, stop=stop, need_dx=need_dx)
        else:
            # The C loop, last layers first: all layers in one call, or
            #  * data-parallel (comm): in chunks of layers -- as soon as a chunk's kernels are enqueued its gradient ranges are
            #    all-reduced on the communicator's stream, under the backward of the earlier layers;
            #  * a caller's gradients with respect to intermediate hidden states (output_hidden_states in trunk-level training,
            #    oscar/modeling_bert.py:146-158): one layer at a time, d_hidden[l + 1] (the output of layer l; bf16 rows in the
            #    forward's layout) added to the running gradient in front of layer l's backward, d_hidden[0] (the embedding
            #    output) behind layer 0's.  (d_hidden[L] is part of g already.)
            step = 1 if d_hidden is not None else max(1, L if comm is None else int(comm["layers_per_chunk"]))
            for hi in range(L, stop, -step):
                lo = max(stop, hi - step)
                if d_hidden is not None and hi < L and d_hidden[hi] is not None:
                    g.add_(d_hidden[hi])
                self._encoder_backward_layers(st, g, acc, lo, hi, need_dx or lo > stop)
                if comm is not None:
                    rng = self._layer_chunk_ranges(lo, hi)
                    comm["launch"](rng)
                    comm["done"].extend(rng)
            if d_hidden is not None and d_hidden[0] is not None:
                g.add_(d_hidden[0])
        want_reg = img is not None and un["region"]
        if not (un["emb"] or want_reg):   # nothing under the layers is trainable: no embedding / region backward at all
            return
        if lay is not None:   # dL/dx0 back in the padded row order (zero at the padding rows, as in the padded run)
            # gathers: padded row -> its compact row, or the zero row kept behind the compact rows (Mr < M here); the text
            # and the region positions land in two contiguous blocks (what the embedding and the region backward read)
            bufs.g[Mr].zero_()
            gi_text, gi_reg = lay.gather_index_split(Mr, T)
            g_text = torch.index_select(bufs.g[:Mr + 1], 0, gi_text, out=bufs.g_pad[:B * T])
            g_reg = torch.index_select(bufs.g[:Mr + 1], 0, gi_reg, out=bufs.g_pad[B * T:B * S]) if img is not None else None
            g_pitch = T
        else:
            g_text, g_reg, g_pitch = g, None, S
        if un["emb"]:
            self._embedding_backward(st, g_text, g_pitch, acc)
        if want_reg:
            self._region_backward(st, g, g_reg, acc)

    def _embedding_backward(self, st, g_text, g_pitch, acc):
        """The embedding block's gradients (its LayerNorm and the three tables) from the text rows' dL/dx0."""
        emb, bufs = self.model.bert.embeddings, st.bufs
        B, T, H, p_h, seed, ids, tt, pos_ids = st.B, st.T, st.H, st.p_h, st.seed, st.ids, st.tt, st.pos_ids
        word_grad = self._grad(emb.word_embeddings.weight)
        # embeddings: text rows
        de = ops.embed_layernorm_bwd(ids, tt, pos_ids, emb.word_embeddings.weight.detach(),
                                     emb.position_embeddings.weight.detach(), emb.token_type_embeddings.weight.detach(),
                                     emb.LayerNorm.weight.detach(), emb.LayerNorm.variance_epsilon, g_text, g_pitch,
                                     self._grad(emb.LayerNorm.weight),
                                     self._grad(emb.LayerNorm.bias), ws=bufs.ws_t["ln_partial"], accumulate=acc,
                                     drop=(p_h, seed, ops.SITE_EMB))
        pos_grad, type_grad = self._grad(emb.position_embeddings.weight), self._grad(emb.token_type_embeddings.weight)
        if not acc:
            pos_grad.zero_()
            type_grad.zero_()
        # the three table gradients without float atomics (sorted ids, one workgroup per run: ops.embed_table_grad); the
        # default position / type ids need no lookup at all: position t collects the batch's rows t, type 0 everything
        ops.embed_table_grad(ids.reshape(-1), de, word_grad, skip_id=emb.word_embeddings.padding_idx)
        pos_sum = None
        if pos_ids is None:
            pos_sum = de.view(B, T, H).sum(0)
            pos_grad[:T].add_(pos_sum)
        else:
            ops.embed_table_grad(pos_ids.reshape(-1), de, pos_grad)
        if tt is None:
            type_grad[0].add_(pos_sum.sum(0) if pos_sum is not None else de.sum(0))
        else:
            ops.embed_table_grad(tt.reshape(-1), de, type_grad)

    def _region_backward(self, st, g, g_reg, acc):
        """The region group's gradients from the region rows' dL/dx0 (g_reg: those rows gathered from a compacted layout)."""
        m, bufs = self.model, st.bufs
        B, T, R, S, H, p_h, seed = st.B, st.T, st.R, st.S, st.H, st.p_h, st.seed
        # region projection
        g_img = g_reg if g_reg is not None else g.view(B, S, H)[:, T:].reshape(B * R, H)
        if p_h > 0.0:
            ops.apply_dropout(g_img, (p_h, seed, ops.SITE_IMG))   # g is not read again after this point
        if st.img_pre is not None:   # back through the image LayerNorm
            ln = m.bert.LayerNorm
            g_img = ops.layernorm_bwd(st.img_pre, g_img.contiguous(), ln.weight.detach(), ln.variance_epsilon,
                                      self._grad(ln.weight), self._grad(ln.bias), ws=bufs.ws_t["ln_partial"],
                                      accumulate=acc)
        ops.wgrad([dict(dy=g_img, x=st.a_img, dw=self.dw_img, db=self.db_img)], B * R)
        D, bt = m.bert.img_dim, m.bert   # (the K-concatenated operand's columns are the two weights' gradients)
        for prm, src in ((bt.img_embedding.weight, self.dw_img[:, :D]), (bt.location_embeds.weight, self.dw_img[:, D:D + 128]),
                         (bt.img_embedding.bias, self.db_img), (bt.location_embeds.bias, self.db_img)):
            getattr(self._grad(prm), "add_" if acc else "copy_")(src)

    def _encoder_backward_layers(self, st, g, acc, lo, hi, need_dx=True):
        """Layers [lo, hi) of the forward `st` through the C loop (one library call), last layer first: g, the running
        gradient, enters as dL/d(output of layer hi - 1) and leaves as dL/d(input of layer lo) -- unless need_dx is False:
        nothing reads it, and layer lo does not launch its last dgrad."""
        bufs = st.bufs
        sub = lambda arr, typ: (typ * (hi - lo)).from_address(ctypes.addressof(arr) + lo * ctypes.sizeof(typ))
        ops.encoder_backward(sub(self.w_tab, _lib.LayerWeights), sub(self.wt_tab, _lib.LayerWeightsT),
                             sub(bufs.acts, _lib.LayerActs), sub(self.g_tab, _lib.LayerGrads),
                             st.x_enc if lo == 0 else bufs.layers[lo - 1]["out"], st.enc_mask, st.mask_additive, g, bufs.ws,
                             st.B, st.S, st.H, st.nh, st.I, self.cfg.layer_norm_eps, accumulate=acc, p_hidden=st.p_h,
                             p_attn=st.p_a, drop_seed=st.seed, layer0=lo, seq=st.lay, need_input_grad=need_dx,
                             **self._overlap_kw(bufs))

    # ------------------------------------------------------------------------------ trunk-level training
    def trunk_forward(self, batch, head_mask=None, training=None, unmasked_only=False, want_hidden=False, want_attn=False,
                      history=None):
        """BertImgModelwithLocationEmbeds.forward for a caller that back-propagates through it (the rollout's
        OscarEncoder, agent.py:493-518): -> (sequence_output fp32 [B,S,H], pooled_output fp32 [B,H], state).
        unmasked_only: the caller vouches that it reads sequence_output only at positions whose attention mask is not
        zero (OscarEncoder: pack_padded_sequence drops the rest); the step may then run on those rows alone (the row
        compaction of forward_backward) and the other positions of sequence_output are zero.
        history: encoder_history_states, one [B, Sh, H] tensor per layer (text-only batches; the attention mask covers the
        Sh + S keys, [B, Sh+S] or per query [B, S, Sh+S]); trunk_backward then leaves their gradients in st.d_history."""
        if training is None:
            training = self.model.bert.training
        self._sync_trainable()
        if self.precision == "fp32":
            if history:
                raise NotImplementedError("PretrainEngine(precision='fp32') does not serve encoder_history_states")
            if unmasked_only or want_hidden or want_attn:
                raise NotImplementedError("PretrainEngine(precision='fp32') serves trunk_forward without unmasked_only, "
                                          "want_hidden and want_attn")
            st = training_f32.trunk_forward(self, batch, head_mask, bool(training))
            return st.seq.view(st.B, st.S, st.H).clone(), st.pooled.clone(), st
        st = self._trunk_fwd(batch, head_mask, None, None, bool(training), bool(unmasked_only), history=history)
        n = st.seq.shape[0]

        def out32(l):
            """Layer l's output rows at fp32, from the best copy kept: the fp16 copy of the last LayerNorm's output where the
            layers keep one; under LN_RESIDUAL (the default) rebuilt from the LayerNorm's fp16 input and the row statistics
            its kernel wrote, as the residual adds do (8 more significant bits than the bf16 rows, which stay the heads' /
            pooler's GEMM operand); the bf16 rows otherwise."""
            d = st.bufs.layers[l]
            if st.bufs.ln_h is not None and l == st.L - 1:
                return st.bufs.ln_h[1][:n].float()
            if not st.bufs.ln_residual:
                return d["out"][:n].float()
            ln = self.model.bert.encoder.layer[l].output.LayerNorm
            return ((d["out_pre"][:n].float() - d["ln2_mean"][:n, None]) * d["ln2_rstd"][:n, None] * ln.weight.detach().float()
                    + ln.bias.detach().float())

        def padded(rows32):
            if st.lay is None:
                return rows32.view(st.B, st.S, st.H)
            out = torch.zeros((st.M, st.H), dtype=torch.float32, device=st.dev)
            out.index_copy_(0, st.lay.index, rows32)
            return out.view(st.B, st.S, st.H)

        seq = padded(out32(st.L - 1))
        attn = None
        if want_attn:
            # all_attentions (oscar/modeling_bert.py:62-79, 160-167): per layer the probabilities AFTER dropout and head_mask,
            # fp32 [B, heads, S, S] -- recomputed from the layer's saved projection and log-sum-exp, the dropout decisions read
            # back from the keep words the forward wrote.  Values only: no gradient flows into them (autograd_trunk_forward
            # marks them non-differentiable).
            if st.lay is not None:
                raise NotImplementedError("output_attentions on compacted rows")
            nh_, pa = st.nh, st.p_a
            attn = []
            for l, d in enumerate(st.bufs.layers):
                if st.hist is not None:
                    attn.append(self._history_probs(st, l, d))
                    continue
                pr = ops.attention_probs(d["qkv"][:n], d["lse"], st.B, st.S, nh_, mask=st.enc_mask, mask_additive=st.mask_additive,
                                         head_scale=None if st.hs is None else st.hs[l].contiguous())
                if pa > 0.0:
                    if "keep_bits" not in d:
                        raise NotImplementedError("output_attentions in training with attention dropout needs the keep words "
                                                  "(VT_ATTN_KEEP_BITS=1, the default)")
                    keep = ops.unpack_keep_bits(d["keep_bits"], st.B, nh_, st.S)
                    pr = pr * keep / (1.0 - ops.attn_drop_p(pa))
                attn.append(pr)
        if not want_hidden:
            return (seq, st.pooled.clone(), st) + ((None, attn) if want_attn else ())
        # all_hidden_states (oscar/modeling_bert.py:146-158): the embedding output, then every layer's output
        hidden = [padded(st.x_enc[:n].float())] + [padded(out32(l)) for l in range(st.L - 1)]
        hidden.append(seq.clone())
        return (seq, st.pooled.clone(), st, hidden) + ((attn,) if want_attn else ())

    def _history_probs(self, st, l, d):
        """all_attentions of layer l of a forward with history states: fp32 [B, heads, S, Sh+S], after dropout and head_mask.
        The probabilities kernel is square: it runs over the extended projection with the saved log-sum-exp in the query
        rows (the history rows' own queries get 0 and are dropped, as the inference path drops them)."""
        B, S, nh, Sh = st.B, st.S, st.nh, st.hist["Sh"]
        St = Sh + S
        lse = torch.zeros((B, nh, St), dtype=torch.float32, device=st.dev)
        lse[:, :, Sh:] = d["lse"]
        mask = st.enc_mask
        if mask is not None and mask.dim() == 3:
            mask = torch.cat([mask.new_zeros((B, Sh, St)), mask], 1).contiguous()
        pr = ops.attention_probs(st.hist["qkv"][l], lse, B, St, nh, mask=mask, mask_additive=st.mask_additive,
                                 head_scale=None if st.hs is None else st.hs[l].contiguous())[:, :, Sh:, :].contiguous()
        if st.p_a > 0.0:
            keep = ops.unpack_keep_bits_rect(st.hist["keep"][l], B, nh, S, St)
            pr = pr * keep / (1.0 - ops.attn_drop_p(st.p_a))
        return pr

    def trunk_backward(self, st, d_seq, d_pooled=None, accumulate=False, d_hidden=None):
        """Gradients of the trunk's parameters into the flat slab, given dL/d(sequence_output) [B,S,H] and / or
        dL/d(pooled_output) [B,H] (either may be None).  The pooler's gradients are zeroed when d_pooled is None, the
        region projection's when the forward had no regions.  After a forward with history states, st.d_history holds
        dL/d(history[l]) as fp32 [B, Sh, H] per layer (None for a tensor that does not require grad)."""
        if self.precision == "fp32":
            if d_hidden is not None:
                raise NotImplementedError("PretrainEngine(precision='fp32') serves trunk_backward without d_hidden")
            return self._trunk_backward_f32(st, d_seq, d_pooled, bool(accumulate))
        bufs, acc = st.bufs, bool(accumulate)
        B, S, H, M, Mr, lay = st.B, st.S, st.H, st.M, st.Mr, st.lay
        g32 = bufs.g_seq32[:Mr]
        rows = lambda t: (t.detach().reshape(M, H).float() if lay is None
                          else t.detach().reshape(M, H).float().index_select(0, lay.index))
        extra = None
        if d_hidden is not None and any(t is not None for t in d_hidden):
            # d_hidden: L + 1 entries (None where the caller read nothing): the last one is dL/d(sequence_output) again
            if d_hidden[-1] is not None:
                d_seq = d_hidden[-1] if d_seq is None else d_seq + d_hidden[-1]
            if any(t is not None for t in d_hidden[:-1]):
                extra = [None if t is None else rows(t).to(BF16) for t in d_hidden[:-1]] + [None]
        if d_seq is None:
            g32.zero_()
        elif lay is None:
            g32.copy_(d_seq.detach().reshape(M, H))
        else:
            torch.index_select(d_seq.detach().reshape(M, H).float(), 0, lay.index, out=g32)
        pw, pb = self._head_group("pooler")
        if d_pooled is not None:
            g_z = (d_pooled.detach().float() * (1.0 - st.pooled * st.pooled)).to(BF16)
            x_cls = st.seq.view(B, S * H)[:, :H] if lay is None else st.cls_seq
            if self.units["pooler"]:
                ops.wgrad([dict(dy=g_z, x=x_cls, dw=self._grad(pw), db=self._grad(pb), accumulate=acc)], B)
            g32.index_add_(0, st.cls_rows, ops.linear(g_z, self.head_t["pool"]).float())
        elif not acc:
            self._zero_head_grads("pooler")
        self._trunk_bwd(st, g32, acc, d_hidden=extra)
        if st.hist is not None:
            st.d_history = list(st.hist["d"])
        if st.img is None and not acc:
            self._zero_head_grads("region")

    def _trunk_backward_f32(self, st, d_seq, d_pooled, acc):
        g = (torch.zeros((st.M, st.H), dtype=torch.float32, device=st.dev) if d_seq is None
             else d_seq.detach().reshape(st.M, st.H).float().clone())
        if d_pooled is not None:
            training_f32.pooler_backward(self, st, g, d_pooled.detach().float(), acc)
        elif not acc:
            self._zero_head_grads("pooler")
        training_f32.trunk_backward(self, st, g, acc)

    # ---- the launch sequences of vt_encoder_forward/backward_bf16 issued op by op (bench.py's per-kernel timing)
    def _encoder_forward_unrolled(self, bufs, x0, mask, B, S, p_h=0.0, p_a=0.0, seed=0, lay=None, mask_additive=False,
                                  hs=None, hist=None):
        """hist (_history_state): layer l projects cat([history[l], layer input], 1) and attends with its S queries over
        those St = Sh + S keys (ops.attention_rect_fwd); the extended rows and their projection are kept in hist for the
        backward.  The rest of the layer is the same."""
        cfg = self.cfg
        nh, eps = cfg.num_attention_heads, cfg.layer_norm_eps
        cur, cur_h, cur_ln = x0, None, None
        n = x0.shape[0]
        for l, ((t, _, _), a) in enumerate(zip(self._layers, bufs.layers)):
            a = {k: (v if k in ("lse", "keep_bits") else v[:n]) for k, v in a.items()}   # the rows in use (all, or the compacted ones)
            # head_mask (oscar/modeling_bert.py:65-66): the attention kernel's own context is kept for the backward (ctx_raw),
            # its per-head scaled copy is what the output projection sees
            raw = a["ctx"] if hs is None else bufs.ctx_raw(l)[:n]
            if hist is None:
                ops.linear(cur, t["w_qkv"], t["b_qkv"], out=a["qkv"])
                ops.attention_fwd(a["qkv"], B, S, nh, mask=mask, mask_additive=mask_additive, out=raw, lse=a["lse"],
                                  drop=(p_a, seed, ops.site_attn(l)), seq=lay, keep_bits=a.get("keep_bits") if p_a > 0.0 else None)
            else:
                St, H = hist["Sh"] + S, cur.shape[1]
                xs = torch.cat([hist["src"][l], cur.view(B, S, H)], 1).reshape(B * St, H)
                qkv = ops.linear(xs, t["w_qkv"], t["b_qkv"])
                kbr = torch.empty(ops.keep_words_rect(B, nh, S, St), dtype=torch.int32, device=cur.device) if p_a > 0.0 else None
                hist["xs"][l], hist["qkv"][l], hist["keep"][l] = xs, qkv, kbr
                ops.attention_rect_fwd(qkv, B, S, St, nh, mask=mask, mask_additive=mask_additive, out=raw, lse=a["lse"],
                                       drop=(p_a, seed, ops.site_attn(l)), keep_bits=kbr)
            if hs is not None:
                ops.scale_heads(raw, hs[l].contiguous(), out=a["ctx"])
            # the residual stream (ops.F16_STREAM: attn_pre / out_pre are fp16 sums -- the library learns it from the dtypes): a
            # residual add reads the fp16 copy ln1_h / ln2_h of the LayerNorm output where the layer keeps one, or rebuilds the
            # LayerNorm from its fp16 input and the statistics its kernel wrote (ops.LN_RESIDUAL; the same arithmetic as the C
            # loop's ln_residual_mode 1)
            res = bufs.ln_residual
            ops.linear(a["ctx"], t["w_ao"], t["b_ao"], residual=cur if cur_h is None else cur_h, out=a["attn_pre"],
                       drop=(p_h, seed, ops.site_selfout(l)), residual_ln=cur_ln)
            ops.layernorm(a["attn_pre"], t["ln1_g"], t["ln1_b"], eps, out=a["attn_out"], mean=a.get("ln1_mean"),
                          rstd=a.get("ln1_rstd"), out_h=a.get("ln1_h"))
            ops.linear(a["attn_out"], t["w_in"], t["b_in"], act=ACT_GELU, out=a["mid"], pre_act_out=a["mid_pre"])
            ops.linear(a["mid"], t["w_out"], t["b_out"], residual=a["attn_pre"] if res else a.get("ln1_h", a["attn_out"]),
                       out=a["out_pre"], drop=(p_h, seed, ops.site_out(l)),
                       residual_ln=(a["ln1_mean"], a["ln1_rstd"], t["ln1_g"], t["ln1_b"]) if res else None)
            ops.layernorm(a["out_pre"], t["ln2_g"], t["ln2_b"], eps, out=a["out"], mean=a.get("ln2_mean"),
                          rstd=a.get("ln2_rstd"), out_h=a.get("ln2_h"))
            cur, cur_h = a["out"], a["out_pre"] if res else a.get("ln2_h")
            cur_ln = (a["ln2_mean"], a["ln2_rstd"], t["ln2_g"], t["ln2_b"]) if res else None

    def _overlap_kw(self, bufs):
        """Second workspace set + side stream for the wgrad / dgrad overlap (off: overlap_wgrad = False)."""
        if not self.overlap_wgrad:
            return {}
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=self.flat.p.device)
        return dict(ws_b=bufs.ws_b, side_stream=self._side_stream)

    def _encoder_backward_unrolled(self, bufs, x0, mask, g, B, S, acc, p_h=0.0, p_a=0.0, seed=0, lay=None,
                                   mask_additive=False, hs=None, inject=None, hist=None, stop=0, need_dx=True):
        """stop / need_dx (_backward_stop): the loop visits layers L-1 .. stop, and layer `stop` launches its last dgrad only
        with need_dx (or for a history tensor's gradient); a frozen layer runs its dgrad chain, its attention backward and
        its two LayerNorm backwards dx-only, and nothing else.
        hist (_history_state of the forward): the rectangular attention backward gives the gradient of the extended
        projection [B*St, 3H]; one dgrad GEMM over those rows yields the hidden rows' gradient (joined with the residual
        gradient) and, in fp32, d_history[l] (kept in hist["d"] for history tensors that require grad); the packed QKV
        weight gradient is a launch of its own over the B*St rows (the dq columns of history rows are zero, so the query
        weights see the hidden rows only; key and value biases apply to history rows as in the reference)."""
        cfg = self.cfg
        nh, eps, M = cfg.num_attention_heads, cfg.layer_norm_eps, x0.shape[0]
        w = {k: (v[:M] if k in bufs.ws_rowed else v) for k, v in bufs.ws_t.items()}
        for l in range(cfg.num_hidden_layers - 1, stop - 1, -1):
            if inject is not None and l + 1 < cfg.num_hidden_layers and inject[l + 1] is not None:
                g.add_(inject[l + 1])   # dL/d(output of layer l) from a caller that read the intermediate hidden states
            (t, gr, wt), a = self._layers[l], bufs.layers[l]
            train, dx = self.units["layers"][l], need_dx or l > stop
            if not train:   # frozen: no parameter gradients from the LayerNorm backwards, no weight-gradient launch
                gr = dict.fromkeys(gr)
            a = {k: (v if k in ("lse", "keep_bits") else v[:M]) for k, v in a.items()}
            x_in = x0 if l == 0 else bufs.layers[l - 1]["out"][:M]
            hd = p_h > 0.0   # with hidden dropout the dense outputs' gradients are the masked copies
            g_pre_dn, g_pre2_dn = (w["g_pre_d"], w["g_pre2_d"]) if hd else (w["g_pre"], w["g_pre2"])
            ops.layernorm_bwd(a["out_pre"], g, t["ln2_g"], eps, gr["ln2_g"], gr["ln2_b"], dx=w["g_pre"],
                              ws=w["ln_partial"], accumulate=acc, dx_dropped=w["g_pre_d"] if hd else None,
                              drop=(p_h, seed, ops.site_out(l)))
            ops.linear(g_pre_dn, wt["wt_out"], residual=a["mid_pre"], act=ACT_MUL, out=w["g_mid"])
            ops.linear(w["g_mid"], wt["wt_in"], residual=w["g_pre"], out=g)
            ops.layernorm_bwd(a["attn_pre"], g, t["ln1_g"], eps, gr["ln1_g"], gr["ln1_b"], dx=w["g_pre2"],
                              ws=w["ln_partial"], accumulate=acc, dx_dropped=w["g_pre2_d"] if hd else None,
                              drop=(p_h, seed, ops.site_selfout(l)))
            ops.linear(g_pre2_dn, wt["wt_ao"], out=w["g_ctx"])
            g_ctx, ctx_l = w["g_ctx"], a["ctx"]
            # the layer's weight-gradient problems (the packed projection's joins them below)
            prob = lambda dy, x, k: dict(dy=dy, x=x, dw=gr["w_" + k], db=gr["b_" + k], accumulate=acc)
            ffn, ao = [prob(w["g_mid"], a["attn_out"], "in"), prob(g_pre_dn, a["mid"], "out")], prob(g_pre2_dn, a["ctx"], "ao")
            if hs is not None:   # back through the head scaling: dL/d(raw context) = head_mask * dL/d(scaled context)
                g_ctx = ops.scale_heads(w["g_ctx"], hs[l].contiguous())
                ctx_l = bufs.ctx_raw(l)[:M]
            if hist is not None:
                Sh, H = hist["Sh"], g.shape[1]
                St = Sh + S
                g_ext = ops.attention_rect_bwd(hist["qkv"][l], g_ctx, ctx_l, a["lse"], B, S, St, nh, mask=mask,
                                               mask_additive=mask_additive, drop=(p_a, seed, ops.site_attn(l)),
                                               keep_bits=hist["keep"][l] if p_a > 0.0 else None)
                if dx or hist["need"][l]:
                    gx = ops.linear(g_ext, wt["wt_qkv"], out_f32=True).view(B, St, H)
                    g.copy_((gx[:, Sh:] + w["g_pre2"].view(B, S, H).float()).reshape(M, H))
                    if hist["need"][l]:
                        hist["d"][l] = gx[:, :Sh].clone()
                if train:
                    ops.wgrad([prob(g_ext, hist["xs"][l], "qkv")], B * St)
                    ops.wgrad(ffn + [ao], M)
                continue
            ops.attention_bwd(a["qkv"], g_ctx, ctx_l, a["lse"], B, S, nh, mask=mask, mask_additive=mask_additive,
                              out=w["g_qkv"], delta_ws=w["delta"], dq32_ws=w.get("dq32"), drop=(p_a, seed, ops.site_attn(l)),
                              seq=lay, keep_bits=a.get("keep_bits") if p_a > 0.0 else None)
            if dx:
                ops.linear(w["g_qkv"], wt["wt_qkv"], residual=w["g_pre2"], out=g)
            if train:
                ops.wgrad(ffn + [prob(w["g_qkv"], x_in, "qkv"), ao], M)
        if inject is not None and inject[0] is not None:
            g.add_(inject[0])           # ... and with respect to the embedding output

    # ------------------------------------------------------------------------------ optimizer
    def _require_ownership(self):
        """The model's parameters must still live in THIS engine's flat slab.  Building another engine over the same
        parameters (the trunk-level engine behind a training-mode `model.bert(...)` call, `model.to(...)`, a load with
        assign) re-points `p.data` elsewhere without touching `_version`: this engine would then read and update a stale
        slab and mirror while the model's real parameters never change.  Refused loudly instead."""
        if not self.flat.owns_params():
            raise RuntimeError(
                "this PretrainEngine no longer owns the model's parameters (their storage was re-pointed: another engine was "
                "built over them -- e.g. by a training-mode call through model.bert -- or the model was moved); build a new "
                "PretrainEngine(model) and carry the optimizer state over with state_dict() / load_state_dict()")

    def _adam_begin(self):
        """Advance Adam's step counter -- the global one and every trainable parameter's own -- and return this step's
        constants (lr after the schedule, the step size bias-corrected for a parameter updated at every step so far)."""
        self._require_ownership()
        self._sync_trainable()
        self.step_count += 1
        for n, fl in self._trainable.items():
            if fl:
                self.param_steps[n] += 1
        self.adam_segments = [(s_, e_, t + 1) for s_, e_, t in self.adam_segments]
        lr = self.lr * self.lr_factor()
        b1, b2 = self.betas
        return lr, self._step_size(lr, self.step_count), b1, b2

    def _adam_abort(self):
        """Take back _adam_begin's counting: no update was completed on behalf of the step."""
        self.step_count -= 1
        for n, fl in self._trainable.items():
            if fl:
                self.param_steps[n] -= 1
        self.adam_segments = [(s_, e_, t - 1) for s_, e_, t in self.adam_segments]

    def _step_size(self, lr, t):
        """lr with Adam's bias correction after t updates."""
        if not self.correct_bias:
            return lr
        b1, b2 = self.betas
        return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)

    def _adam_ranges(self, consts, ranges, grad_scale, grads=None):
        """The fused AdamW on the trainable parts of [start, end) ranges of the flat slabs (weight decay by region:
        pretrain.py:109-127), each segment with the bias correction of its own update count."""
        f = self.flat
        lr, _, b1, b2 = consts
        g = f.g if grads is None else grads   # fp32 slab, or the all-reduced bf16 communication copy
        nd = f.n_decay
        for s_, e_ in ranges:
            for a_, b_, t in self.adam_segments:
                s0, e0 = max(s_, a_), min(e_, b_)
                if e0 <= s0:
                    continue
                step_size = self._step_size(lr, t)
                for lo, hi, wd in ((s0, min(e0, nd), self.wd), (max(s0, nd), e0, 0.0)):
                    if hi > lo:
                        ops.adamw_flat(f.p[lo:hi], g[lo:hi], f.m[lo:hi], f.v[lo:hi], f.mirror[lo:hi], lr, step_size, b1, b2,
                                       self.eps, wd, grad_scale)

    def _adam_end(self):
        self.sched_step += 1
        self.flat.mark_fresh()
        # the transposed copies of what AdamW just stepped are stale (a pending full rebuild stays one; two steps under
        # different flags without a forward between them: everything)
        if self._wt_dirty is False:
            self._wt_dirty = self._flags
        elif self._wt_dirty != self._flags:
            self._wt_dirty = True
        # the fused kernel wrote the slab through raw pointers: no parameter's _version moved, so the packed bf16
        # copies the inference path caches (encoder layers, region projection, rollout modules) are told explicitly
        invalidate_packed_weights()

    def optimizer_step(self, grad_scale=1.0, grads=None):
        """AdamW.step() + scheduler.step() (pretrain.py:192-193) as two fused launches (decay / no-decay).  With the optimizer
        sharded over several ranks it is a COLLECTIVE: reduce-scatter of the gradient slab, this rank's update, all-gather
        of the updated weights (the sum over the ranks times grad_scale is what AdamW sees)."""
        if self.shard:
            if grads is not None:
                raise ValueError("the sharded optimizer_step() reduces the gradient slab itself; it takes no `grads`")
            return self._shard_step_unoverlapped(grad_scale)
        self._adam_ranges(self._adam_begin(), [(0, self.flat.total)], grad_scale, grads)
        self._adam_end()

    def _train_step_adamw_under_backward(self, batch, scale, layers_per_chunk):
        """One rank: the fused AdamW of a parameter range runs on a side stream as soon as that range's gradients are final
        -- the heads' before the encoder backward starts, a chunk of encoder layers' while the earlier layers' backward
        runs (pretrain.py:191-193 has no gradient clipping between backward and step: a range's update needs nothing but
        its own gradients).  The update is HBM-bound (30 bytes per parameter) and finds its CUs beside the kernels that do
        not fill the chip (the grouped weight-gradient launch runs 216 of 256 workgroups; attention, LayerNorm and the
        heads are not persistent).  A layer's weights are not read again once its backward is enqueued (dgrad reads the
        transposed copies, rebuilt at the start of the next step); embeddings, region projection and everything else follow
        on the main stream, which then waits for the side stream."""
        if self._adam_stream is None:
            self._adam_stream = torch.cuda.Stream(device=self.flat.p.device)
        side = self._adam_stream
        consts = self._adam_begin()
        try:
            def launch(rng):
                ev = torch.cuda.Event()
                ev.record()
                side.wait_event(ev)
                with torch.cuda.stream(side):
                    self._adam_ranges(consts, rng, 1.0)

            comm = dict(layers_per_chunk=layers_per_chunk, launch=launch, done=[])
            out = self.forward_backward(batch, grad_scale=scale, comm=comm)
        except BaseException:
            self._adam_abort()   # no update was completed on behalf of this step's counters
            torch.cuda.current_stream().wait_stream(side)
            raise
        self._adam_ranges(consts, distributed.complement_ranges(self.flat.total, comm["done"]), 1.0)
        torch.cuda.current_stream().wait_stream(side)
        self._adam_end()
        return out

    # ------------------------------------------------------------------------------ optimizer sharded over the ranks
    def shard_atoms(self):
        """The ranges forward_backward hands to comm["launch"] with one layer per chunk, in slab order: the heads' ranges,
        every layer's decay and no-decay range (ends rounded up to ALIGN, as _trunk_bwd rounds them), and what is left."""
        done = self._param_ranges(self._head_params()) if self.has_heads else []
        done = done + [r_ for l in range(len(self.layer_ranges)) for r_ in self._layer_chunk_ranges(l, l + 1)]
        return sorted(done + distributed.complement_ranges(self.flat.total, done))

    def shard_launch_ranges(self):
        """The launches of one overlapped step with one layer per chunk, in launch order: heads, layers last first, tail."""
        heads = self._param_ranges(self._head_params()) if self.has_heads else []
        layers = [self._layer_chunk_ranges(l, l + 1) for l in reversed(range(len(self.layer_ranges)))]
        done = heads + [r_ for l_ in layers for r_ in l_]
        return [r_ for r_ in [heads] + layers + [distributed.complement_ranges(self.flat.total, done)] if r_]

    def mirror_only_names(self):
        """The slab entries the step reads ONLY through the bf16 mirror: what the layer tables point at in flat.mirror and
        what the heads, the pooler and the region projection take via _mirror(...) -- minus every entry that some kernel
        also takes as the fp32 parameter itself (the three embedding tables; the tied MLM decoder IS the word table)."""
        emb = self.model.bert.embeddings
        as_fp32 = [emb.word_embeddings.weight, emb.position_embeddings.weight, emb.token_type_embeddings.weight]
        names = {"bert.encoder.layer.%d.%s" % (l, n) for l in range(self.cfg.num_hidden_layers) for n in _LAYER_WEIGHTS}
        names |= {self._name_of(prm) for _, prm, key in self._head_rows() if key is not None}
        return names - {self._name_of(p_) for p_ in as_fp32}

    def fp32_spans(self):
        """Slab ranges whose updated values travel back as fp32: every entry that is not mirror-only (the whole no-decay
        group among them), each with the padding behind it."""
        f, only16 = self.flat, self.mirror_only_names()
        assert not any(grp for n, _, _, _, grp in f.entries if n in only16)   # biases / LayerNorms are read as fp32
        spans = []
        starts = [o for _, _, o, _, _ in f.entries] + [f.total]
        for (n, _, o, _, _), nxt in zip(f.entries, starts[1:]):
            if n not in only16:
                if spans and spans[-1][1] == o:
                    spans[-1] = (spans[-1][0], nxt)
                else:
                    spans.append((o, nxt))
        return spans

    def shard_plan(self, world, rank, bucket_elems=None):
        """The static ownership plan of this engine's slab for `world` ranks (any engine can compute any rank's)."""
        f = self.flat
        be = self.bucket_elems if bucket_elems is None else int(bucket_elems)
        return distributed.ShardPlan(f.total, f.n_decay, self.shard_atoms(), self.fp32_spans(), world, rank, be)

    def _shard_setup(self):
        f = self.flat
        self.plan = self.shard_plan(self.world, torch.distributed.get_rank(self.pg))
        # AdamW's moments of the owned pieces only, back to back in slab order (1 / world of the two slabs)
        self.m_sh = torch.zeros(self.plan.owned, dtype=torch.float32, device=f.p.device)
        self.v_sh = torch.zeros(self.plan.owned, dtype=torch.float32, device=f.p.device)
        self._shard_tables = {}

    def _shard_table(self, launch, grads):
        key = (tuple(launch.ranges), grads.data_ptr())
        tab = self._shard_tables.get(key)
        if tab is None:
            f = self.flat
            tab = self._shard_tables[key] = ops.shard_adamw_table(
                f.p, grads, self.m_sh, self.v_sh, f.mirror, [(s_, e_, dec, mo) for s_, e_, dec, _, mo in launch.own])
        return tab

    def _comm_copy(self, ranges):
        """What the communicator reduces for these ranges of the gradient slab -> (buffer, elements per bucket): the fp32 slab
        itself, or the bf16 communication copy with the ranges cast into it (same bytes per bucket)."""
        if self.g16 is None:
            return self.flat.g, self.bucket_elems
        for s_, e_ in ranges:
            if e_ > s_:
                ops.cast_to_bf16(self.flat.g[s_:e_], self.g16[s_:e_])
        return self.g16, 2 * self.bucket_elems

    def _shard_reduce(self, launch, handles):
        """Communication copy and reduce-scatter of one launch's ranges; returns the buffer AdamW reads."""
        buf, per_bucket = self._comm_copy(launch.ranges)
        distributed.reduce_scatter_buckets(buf, launch, self.plan, per_bucket, self.pg, handles)
        return buf

    def _shard_update(self, consts, launch, grad_scale, grads):
        """AdamW on this rank's segments of one launch: one kernel launch."""
        lr, step_size, b1, b2 = consts
        ops.shard_adamw(self._shard_table(launch, grads), grads.dtype == BF16, lr, step_size, b1, b2, self.eps, self.wd, grad_scale)

    def _shard_gather(self, launch, handles):
        """All-gather of one launch's updated pieces: the mirror where a bucket holds bf16-class elements, the fp32
        parameters where it holds fp32-class ones."""
        f = self.flat
        distributed.all_gather_buckets(f.mirror, [b for b in launch.buckets if b[2]], self.plan, self.pg, handles)
        distributed.all_gather_buckets(f.p, [b for b in launch.buckets if b[3]], self.plan, self.pg, handles)

    def _shard_settle(self):
        """The segments this rank does not own, once all gathers have arrived: p = float(mirror) where the weights
        travelled as bf16, mirror = bf16(p) where they travelled as fp32.  One launch over the whole plan."""
        tab = self._shard_tables.get("settle")
        if tab is None:
            segs = [(s_, e_, int(f32)) for s_, e_, f32 in self.plan.everything().others]
            tab = self._shard_tables["settle"] = ops.shard_settle_table(self.flat.p, self.flat.mirror, segs)
        ops.shard_settle(tab)

    def _shard_step_unoverlapped(self, grad_scale):
        """The three phases one after the other over the whole plan (optimizer_step(), train_step(overlap=False)); the
        launches are those of an overlapped step with one layer per chunk."""
        launches = [self.plan.launch(r_) for r_ in self.shard_launch_ranges()]
        handles, bufs = [], []
        for la in launches:
            bufs.append(self._shard_reduce(la, handles))
        for h in handles:
            h.wait()
        consts = self._adam_begin()
        for la, buf in zip(launches, bufs):
            self._shard_update(consts, la, grad_scale, buf)
        handles = []
        for la in launches:
            self._shard_gather(la, handles)
        for h in handles:
            h.wait()
        self._shard_settle()
        self._adam_end()

    def _shard_train_step(self, batch, scale, layers_per_chunk, _force_comm):
        ws = self.world
        handles, launched = [], []   # launched: (plan launch, gradient buffer, first handle, one past the last handle)

        def reduce_ranges(rng):
            la = self.plan.launch(rng)
            n0 = len(handles)
            buf = self._shard_reduce(la, handles)
            launched.append((la, buf, n0, len(handles)))

        def local_ranges(rng):   # _force_comm: the same kernels on the rank's own fp32 gradients, no collective
            launched.append((self.plan.launch(rng), self.flat.g, 0, 0))
            _force_comm(rng)

        launch = reduce_ranges if _force_comm is None else local_ranges
        comm = dict(layers_per_chunk=layers_per_chunk, launch=launch, done=[])
        out = self.forward_backward(batch, grad_scale=scale, comm=comm)
        launch(distributed.complement_ranges(self.flat.total, comm["done"]))   # embeddings, region projection
        # per arrived range, in launch order: this rank's update, then the all-gather of that range goes out and travels
        # while the next range is updated
        consts = self._adam_begin()
        gathers = []
        for la, buf, h0, h1 in launched:
            for h in handles[h0:h1]:
                h.wait()
            self._shard_update(consts, la, 1.0 / ws, buf)
            if _force_comm is None:
                self._shard_gather(la, gathers)
        for h in gathers:
            h.wait()
        self._shard_settle()
        self._adam_end()
        return out

    def consolidate(self):
        """COLLECTIVE (every rank must call it): all-gather of the owners' fp32 parameters, after which flat.p -- the
        model's parameters -- is exact on every rank.  Required before model.state_dict() is written as a checkpoint and
        before fp32-route inference on these weights.  Nothing to do where the optimizer is not sharded."""
        if not self.shard:
            return
        self._require_ownership()
        distributed.all_gather_buckets(self.flat.p, self.plan.everything().buckets, self.plan, self.pg)
        invalidate_packed_weights()

    def _shard_full_moments(self):
        """(m, v) as full slabs on every rank: a collective gather of the shard-local storage (temporaries)."""
        every = self.plan.everything()
        out = []
        for sh in (self.m_sh, self.v_sh):
            full = torch.zeros(self.flat.total, dtype=torch.float32, device=sh.device)
            for s_, e_, _, _, mo in every.own:
                full[s_:e_].copy_(sh[mo:mo + e_ - s_])
            distributed.all_gather_buckets(full, every.buckets, self.plan, self.pg)
            out.append(full)
        return out

    # ------------------------------------------------------------------------------ optimizer state (resume)
    def state_dict(self):
        """What a resumed run needs beside the model's own state_dict: AdamW's moments per parameter NAME (layout-
        independent), the step / scheduler / dropout counters and the hyper-parameters.  (The reference checkpoints weights
        only, pretrain.py:247-270; this is the fused optimizer's counterpart of torch.optim's state_dict.)"""
        f = self.flat
        # (the optimizer sharded over several ranks: a COLLECTIVE -- the moments are gathered, the format is the same)
        m_, v_ = self._shard_full_moments() if self.shard else (f.m, f.v)
        state = {n: dict(exp_avg=f.view(m_, n).detach().clone(), exp_avg_sq=f.view(v_, n).detach().clone())
                 for n, _, _, _, _ in f.entries}
        return dict(state=state, step_count=self.step_count, sched_step=self.sched_step, fb_count=self.fb_count,
                    drop_seed_base=self.drop_seed_base,
                    # updates per parameter (they differ once requires_grad changed during the run)
                    param_steps=dict(self.param_steps),
                    hyper=dict(lr=self.lr, weight_decay=self.wd, eps=self.eps, betas=tuple(self.betas),
                               correct_bias=self.correct_bias, schedule=self.schedule, warmup_steps=self.warmup_steps,
                               t_total=self.t_total,
                               # what travelled in the gradient all-reduce of the run that wrote this state (recorded, not
                               # restored: it is a property of the launch, and it changes the result at rounding level)
                               grad_comm_dtype=self.grad_comm_dtype, world_size=self.world, precision=self.precision,
                               shard_optimizer=self.shard_optimizer,   # (recorded, not restored)
                               hidden_dropout=float(self.cfg.hidden_dropout_prob),
                               attention_dropout_configured=float(self.cfg.attention_probs_dropout_prob),
                               attention_dropout_effective=self.attention_dropout_effective,
                               # ops.set_deterministic at the time of the call (recorded, not restored: a process-wide switch)
                               deterministic=ops.is_deterministic()))

    def load_state_dict(self, sd, load_hyper=True):
        f = self.flat
        missing = [n for n, _, _, _, _ in f.entries if n not in sd["state"]]
        if missing:
            raise KeyError("optimizer state has no entry for %s" % ", ".join(missing[:5]))
        # (sharded over several ranks: the same name-keyed format goes through a full-size temporary; the rank keeps its pieces)
        for key, slab, sh in (("exp_avg", f.m, getattr(self, "m_sh", None)), ("exp_avg_sq", f.v, getattr(self, "v_sh", None))):
            full = torch.zeros(f.total, dtype=torch.float32, device=f.p.device) if self.shard else slab
            for n, _, _, _, _ in f.entries:
                f.view(full, n).copy_(sd["state"][n][key])
            if self.shard:
                for s_, e_, _, _, mo in self.plan.everything().own:
                    sh[mo:mo + e_ - s_].copy_(full[s_:e_])
        self.step_count, self.sched_step = int(sd["step_count"]), int(sd["sched_step"])
        self.fb_count, self.drop_seed_base = int(sd["fb_count"]), int(sd["drop_seed_base"])
        # a state without per-parameter counts (written before they existed): every parameter from the global step
        steps = sd.get("param_steps")
        self.param_steps = {n: int(self.step_count if steps is None else steps[n]) for n, _, _, _, _ in f.entries}
        self._rebuild_segments()
        if load_hyper:
            h = sd["hyper"]
            self.lr, self.wd, self.eps, self.betas = h["lr"], h["weight_decay"], h["eps"], tuple(h["betas"])
            self.correct_bias, self.schedule = h["correct_bias"], h["schedule"]
            self.warmup_steps, self.t_total = h["warmup_steps"], h["t_total"]

    def all_reduce_grads(self):
        """Sum the flat gradient slab over the data-parallel group in fixed-size buckets (no overlap)."""
        if self.world == 1:
            return
        if self.shard:
            raise RuntimeError("with the optimizer sharded over the ranks no rank holds the whole reduced gradient slab: call "
                               "optimizer_step(), which reduce-scatters, updates and gathers")
        self._sync_trainable()
        if all(self._flags):
            distributed.all_reduce_flat(*self._comm_copy([(0, self.flat.total)]), self.pg)
            return
        buf, per_bucket = self._comm_copy(self.train_spans)   # frozen ranges stay off the wire
        distributed.all_reduce_ranges(buf, self.train_spans, per_bucket, self.pg)

    def train_step(self, batch, overlap=True, layers_per_chunk=3, _force_comm=None):
        """zero_grad -> forward -> backward -> gradient all-reduce -> AdamW -> schedule, as pretrain.py:150-193.
        The reference divides the loss by world_size before backward AND lets DDP average;
        loss_scale_by_world reproduces that extra 1/world factor.  With overlap, the all-reduce of the
        encoder layers' gradients runs under the backward of the earlier layers."""
        ws = self.world
        scale = (1.0 / ws) if (ws > 1 and self.loss_scale_by_world) else 1.0
        if ws == 1 and _force_comm is None and overlap and self.overlap_adamw:
            return self._train_step_adamw_under_backward(batch, scale, layers_per_chunk)
        if self.shard:
            if overlap:
                return self._shard_train_step(batch, scale, layers_per_chunk, _force_comm)
            out = self.forward_backward(batch, grad_scale=scale)
            self.optimizer_step(grad_scale=1.0 / ws)   # DDP's mean over ranks
            return out
        if (ws == 1 and _force_comm is None) or not overlap:
            out = self.forward_backward(batch, grad_scale=scale)
            self.all_reduce_grads()
        else:
            handles, launched = [], []   # launched: (ranges, first handle, one past the last handle) per launch call

            def reduce_ranges(rng):
                n0 = len(handles)
                buf, per_bucket = self._comm_copy(rng)
                distributed.all_reduce_ranges(buf, rng, per_bucket, self.pg, handles)
                launched.append((list(rng), n0, len(handles)))

            launch = _force_comm or reduce_ranges
            comm = dict(layers_per_chunk=layers_per_chunk, launch=launch, done=[])
            out = self.forward_backward(batch, grad_scale=scale, comm=comm)
            # embeddings, region projection, heads (and whatever is frozen, which is not reduced)
            launch(self._trainable_ranges(distributed.complement_ranges(self.flat.total, comm["done"])))
            if _force_comm is None:
                # AdamW per arrived range, in launch order (last layers first, the embeddings / heads tail last): the update
                # of the encoder's 85 M parameters runs while the tail's all-reduce is still in flight.  (wait() makes this
                # stream wait for the communicator's, not the host.)
                consts = self._adam_begin()
                for rng, h0, h1 in launched:
                    for h in handles[h0:h1]:
                        h.wait()
                    self._adam_ranges(consts, rng, 1.0 / ws, self.g16)   # 1 / ws: DDP's mean over ranks
                self._adam_end()
                return out
            for h in handles:
                h.wait()
        use16 = self.g16 is not None and _force_comm is None
        self.optimizer_step(grad_scale=1.0 / ws, grads=self.g16 if use16 else None)  # DDP's mean over ranks
        return out


class _LossWithGrads(torch.autograd.Function):
    """Bridges the engine to torch autograd for the reference's own loop (`loss.backward()` then a torch
    optimizer, tasks/viewpoint_select/pretrain.py:167-193): forward has already run the HIP forward AND
    backward for d(loss)/d(params); backward hands those gradients (times the incoming scalar) to
    autograd, which accumulates them into p.grad and fires DistributedDataParallel's hooks."""

    @staticmethod
    def forward(ctx, engine, loss, *params):
        ctx.engine = engine
        ctx.names = [engine._name_of(p) for p in params]
        ctx.fb_count = engine.fb_count      # which forward / backward pair of the engine these gradients belong to
        return loss.detach().clone()

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.engine.fb_count != ctx.fb_count:
            # the gradients live in the engine's slab and the next training forward on this module has overwritten them
            raise RuntimeError("backward() of a PreTrainOscar loss after a later training forward of the same module: the HIP "
                               "step computes the gradients with the forward and keeps ONE set per module -- call "
                               "loss.backward() before the next forward (the reference's loop does: pretrain.py:169-191)")
        f = ctx.engine.flat
        return (None, None) + tuple(f.view(f.g, n) * grad_out for n in ctx.names)


class _LossLazyGrads(torch.autograd.Function):
    """eval-mode forward with grad enabled (the reference's val(), pretrain.py:291,469-481, calls model(**batch) in
    eval() with no torch.no_grad): the values come from the inference path; the engine (its slabs and saved
    activations) is built and the HIP forward + backward run only IF `.backward()` is actually called -- dropout is
    the identity in eval mode, so the recomputation sees the same function."""

    @staticmethod
    def forward(ctx, model, batch, loss, *params):
        ctx.model, ctx.batch = model, dict(batch)
        ctx.head_mask = ctx.batch.pop("__head_mask__", None)
        ctx.params = params
        return loss.detach().clone()

    @staticmethod
    def backward(ctx, grad_out):
        model = ctx.model
        eng = _bridge_engine(model)
        was = model.training
        model.eval()
        try:
            eng.forward_backward(ctx.batch, head_mask=ctx.head_mask)
        finally:
            model.train(was)
        f = eng.flat
        return (None, None, None) + tuple(f.view(f.g, eng._name_of(p)) * grad_out for p in ctx.params)


def _trunk_param_grads(eng, st, names, d_pooled):
    """What a trunk autograd node hands back for its parameters after eng.trunk_backward: copies of the slab's gradients, None
    for the groups that backward had nothing to feed (the region projection of a text-only forward, the pooler when nothing
    read pooled_output)."""
    unused = ()
    if st.img is None:
        unused += ("bert.img_embedding.", "bert.location_embeds.", "bert.LayerNorm.")
    if d_pooled is None:
        unused += ("bert.pooler.",)
    f = eng.flat
    return tuple(None if n.startswith(unused) else f.view(f.g, n).clone() for n in names)


class _TrunkWithGrads(torch.autograd.Function):
    """The trunk as ONE autograd node for callers that train through it (OscarEncoder in the rollout, agent.py:493-518):
    forward = the engine's trunk forward (activations kept in its buffers), backward = its trunk backward, handing the
    parameter gradients to autograd."""

    @staticmethod
    def forward(ctx, engine, batch, head_mask, unmasked_only, want_hidden, want_attn, n_history, *tensors):
        # tensors: the n_history encoder_history_states (inputs with gradients of their own), then the parameters
        history, params = tensors[:n_history], tensors[n_history:]
        out = engine.trunk_forward(batch, head_mask, unmasked_only=unmasked_only, want_hidden=want_hidden, want_attn=want_attn,
                                   history=history)
        seq, pooled, st = out[:3]
        ctx.engine, ctx.st = engine, st
        ctx.history_like = [(h.dtype, h.device) for h in history]
        ctx.names = [engine._name_of(p) for p in params]
        ctx.n_hidden = len(out[3]) if want_hidden else 0
        ctx.set_materialize_grads(False)
        attn = tuple(out[4]) if want_attn else ()
        ctx.mark_non_differentiable(*attn)
        return (seq, pooled) + (tuple(out[3]) if want_hidden else ()) + attn

    @staticmethod
    def backward(ctx, d_seq, d_pooled, *d_rest):
        eng, st = ctx.engine, ctx.st
        d_hidden = d_rest[:ctx.n_hidden]
        eng.trunk_backward(st, d_seq, d_pooled, d_hidden=list(d_hidden) if d_hidden else None)
        d_history = tuple(None if d is None else d.to(device=dev, dtype=dt)
                          for d, (dt, dev) in zip(st.d_history or (), ctx.history_like))
        return (None, None, None, None, None, None, None) + d_history + _trunk_param_grads(eng, st, ctx.names, d_pooled)


class _TrunkLazyGrads(torch.autograd.Function):
    """eval() with grad enabled at trunk level (the values come from the inference path, nothing is saved): the engine's
    trunk forward + backward run only if `.backward()` is actually called -- dropout is the identity in eval mode, so the
    recomputation sees the same function (the trunk-level twin of _LossLazyGrads)."""

    @staticmethod
    def forward(ctx, trunk, batch, head_mask, seq, pooled, *params):
        ctx.trunk, ctx.batch, ctx.head_mask, ctx.params = trunk, dict(batch), head_mask, params
        ctx.set_materialize_grads(False)
        return seq.detach().clone(), pooled.detach().clone()

    @staticmethod
    def backward(ctx, d_seq, d_pooled):
        eng = _bridge_engine(ctx.trunk)
        _, _, st = eng.trunk_forward(ctx.batch, ctx.head_mask, training=False)
        eng.trunk_backward(st, d_seq, d_pooled)
        return (None, None, None, None, None) + _trunk_param_grads(eng, st, [eng._name_of(p) for p in ctx.params], d_pooled)


def lazy_autograd_trunk(trunk, batch, head_mask, seq, pooled):
    """The inference path's (sequence_output, pooled_output) made differentiable on demand (eval mode, grad enabled)."""
    params = [p for p in trunk.parameters() if p.requires_grad]
    return _TrunkLazyGrads.apply(trunk, batch, head_mask, seq, pooled, *params)


def autograd_trunk_forward(trunk, batch, head_mask=None, unmasked_only=False, want_hidden=False, want_attn=False, history=None):
    """BertImgModelwithLocationEmbeds.forward in training mode: (sequence_output, pooled_output) that back-propagate into the
    trunk's parameters through the HIP backward; under torch.no_grad() the same forward (dropout included) without a graph.
    unmasked_only: see PretrainEngine.trunk_forward.  want_hidden: one more element, the tuple of all_hidden_states
    (embedding output + every layer's output, oscar/modeling_bert.py:146-158), each differentiable like sequence_output.
    want_attn: one more, the tuple of all_attentions (per layer, after dropout and head_mask) -- values only.
    history: encoder_history_states (one [B, Sh, H] tensor per layer); the tensors among them that require grad receive
    their gradients like the parameters do."""
    eng = _bridge_engine(trunk)
    history = list(history) if history else []
    if not torch.is_grad_enabled():
        out = eng.trunk_forward(batch, head_mask, unmasked_only=unmasked_only, want_hidden=want_hidden, want_attn=want_attn,
                                history=history)
        return (out[0], out[1]) + ((tuple(out[3]),) if want_hidden else ()) + ((tuple(out[4]),) if want_attn else ())
    params = [p for p in trunk.parameters() if p.requires_grad]
    out = _TrunkWithGrads.apply(eng, batch, head_mask, bool(unmasked_only), bool(want_hidden), bool(want_attn), len(history),
                                *history, *params)
    k = 2 + (trunk.config.num_hidden_layers + 1 if want_hidden else 0)
    return (out[0], out[1]) + ((tuple(out[2:k]),) if want_hidden else ()) + ((tuple(out[k:]),) if want_attn else ())


def _bridge_engine(model):
    """The engine behind the autograd bridge (parameters stay the model's own: attach_grads=False).  An external torch
    optimizer owns the update there, and optimizers that write through `p.data` (the reference's pytorch-transformers
    AdamW: `p.data.addcdiv_`, `p.data.add_`) do not move `p._version` -- so nothing can tell whether the fp32 slab
    changed since the last call.  The bf16 mirror (one fused cast of the slab) and the transposed copies are therefore
    rebuilt on EVERY bridged forward, and the inference-side packed copies are invalidated."""
    eng = getattr(model, "_vt_engine", None)
    if eng is None or eng.flat.p.device != next(model.parameters()).device or not eng.flat.owns_params():
        eng = PretrainEngine(model, attach_grads=False)
        object.__setattr__(model, "_vt_engine", eng)
    else:
        eng.flat.refresh_mirror()
        eng._wt_dirty = True
    invalidate_packed_weights()
    return eng


def autograd_forward(model, batch, head_mask=None):
    """PreTrainOscar.forward in training mode with grad enabled: returns the 7-tuple whose first element
    back-propagates into the model's parameters."""
    eng = _bridge_engine(model)
    out = eng.forward_backward(batch, head_mask=head_mask)
    params = [p for p in model.parameters() if p.requires_grad]
    loss = _LossWithGrads.apply(eng, out[0], *params)
    return (loss,) + tuple(out[1:])


def lazy_autograd_loss(model, batch, loss, head_mask=None):
    """The inference path's loss made differentiable on demand (eval mode, grad enabled)."""
    params = [p for p in model.parameters() if p.requires_grad]
    if head_mask is not None:
        batch = dict(batch, __head_mask__=head_mask)
    return _LossLazyGrads.apply(model, batch, loss, *params)
