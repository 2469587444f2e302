"""Optimizers, schedules and gradient clipping of the reference's own training loops, on HIP kernels.

Drop-in classes for what ``tasks/viewpoint_select/pretrain.py:26-30,108-139,192`` and ``agent.py:129,511-518`` construct:

* ``AdamW`` -- the pytorch-transformers rule (``eps`` added to the UN-corrected ``sqrt(v)``, decoupled decay applied after the
  move), parameter groups, ``LambdaLR``-driven ``group["lr"]``;
* ``Adam`` -- ``torch.optim.Adam``'s rule (no weight decay, no amsgrad);
* ``clip_grad_norm_`` -- ``torch.nn.utils.clip_grad_norm_`` for the 2-norm, without a host synchronisation;
* ``WarmupLinearSchedule`` / ``WarmupConstantSchedule`` -- host-only ``LambdaLR`` subclasses.

They work over arbitrary lists of fp32 parameters on one HIP device and know nothing of ``PretrainEngine``.  A step is ONE
launch of ``vt_multi_adam`` whatever the list holds (three with ``max_grad_norm``: sum of squares, norm, update reading the
clip coefficient from device memory); ``clip_grad_norm_`` is three.  The kernels read a device-resident chunk table of
addresses which is built on the first call and rebuilt only when an address or the set of parameters with gradients changes.
There is no CPU fallback.
"""
import collections
import math

import torch
from torch.optim import Optimizer
from torch.optim.lr_scheduler import LambdaLR

from . import _lib

# the chunk table's geometry (include/visitron_hip.h)
CHUNK, ENTRY_WORDS, HYPER_FLOATS = (_lib.CONSTANTS["VT_OPTIM_" + c] for c in ("CHUNK", "ENTRY_WORDS", "HYPER_FLOATS"))


# ---- host constants: formed in double, rounded once to fp32 when they are written to the hyper buffer ----------------
def adamw_constants(lr, betas, eps, weight_decay, t, correct_bias=True):
    """(b1, 1-b1, b2, 1-b2, step_size, rsbc2, eps, lr*wd) of the pytorch-transformers rule at step t (1-based)."""
    b1, b2 = float(betas[0]), float(betas[1])
    step_size = float(lr)
    if correct_bias:
        step_size = step_size * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    return (b1, 1.0 - b1, b2, 1.0 - b2, step_size, 1.0, float(eps), float(lr) * float(weight_decay))


def adam_constants(lr, betas, eps, t):
    """The same eight for torch.optim.Adam's rule: p -= lr / (1-b1^t) * m / (sqrt(v) / sqrt(1-b2^t) + eps)."""
    b1, b2 = float(betas[0]), float(betas[1])
    return (b1, 1.0 - b1, b2, 1.0 - b2, float(lr) / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), float(eps), 0.0)


# ---- the chunk table ------------------------------------------------------------------------------------------------
def build_chunk_table(entries, chunk=CHUNK):
    """entries: (p, g, m, v byte addresses, element count, hyper slot) per tensor -> rows of ENTRY_WORDS ints, one per
    chunk of at most `chunk` fp32 elements.  An address of 0 (a tensor the kernel does not use) stays 0."""
    rows = []
    for p, g, m, v, n, slot in entries:
        for lo in range(0, n, chunk):
            off = 4 * lo
            rows.append([a + off if a else 0 for a in (p, g, m, v)] + [min(chunk, n - lo), slot])
    return rows


class ChunkTable(object):
    """The cached table of one parameter list.  update(entries) rebuilds it when, and only when, `entries` differ from
    the ones it was built from -- an address, a count, a slot, or which tensors are present."""

    def __init__(self, device=None):
        self.device = device        # None: host only (rows are kept, nothing is uploaded)
        self.key = None
        self.rows = []
        self.builds = 0
        self.dev = None             # int64 [n_chunks, ENTRY_WORDS] on the device
        self.partials = None        # fp64 [n_chunks]: vt_multi_sumsq's output
        self.numel = 0

    @property
    def n_chunks(self):
        return len(self.rows)

    def stale(self, entries):
        return self.key != tuple(entries)

    def update(self, entries):
        if not self.stale(entries):
            return False
        self.rows = build_chunk_table(entries)
        self.numel = sum(e[4] for e in entries)
        self.builds += 1
        if self.device is not None and self.rows:
            self.dev = _upload(self.rows, torch.int64, self.device)
            self.partials = torch.empty(len(self.rows), dtype=torch.float64, device=self.device)
        else:
            self.dev = self.partials = None
        self.key = tuple(entries)
        return True


def _upload(rows, dtype, device):
    """A fresh device tensor filled from pinned host memory by an asynchronous copy: the host does not wait, and a buffer
    an earlier launch may still read is never written again (each call gets its own)."""
    return torch.tensor(rows, dtype=dtype).pin_memory().to(device, non_blocking=True)


def _check(t, what, device):
    if not t.is_cuda:
        raise RuntimeError("visitron_amd.optim runs on a HIP device only (%s is a %s tensor); there is no CPU fallback"
                           % (what, t.device))
    if t.dtype != torch.float32:
        raise RuntimeError("visitron_amd.optim serves fp32 tensors (%s is %s)" % (what, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError("visitron_amd.optim serves contiguous tensors (%s has strides %s)" % (what, tuple(t.stride())))
    if t.device != device:
        raise RuntimeError("visitron_amd.optim serves one device per list (%s is on %s, the list started on %s)"
                           % (what, t.device, device))


def _dense(g, what):
    if g.layout is not torch.strided:
        raise RuntimeError("visitron_amd.optim does not serve sparse gradients (%s is %s)" % (what, g.layout))
    return g


def _norm_launches(table, max_norm, device):
    """sum of squares + finish -> fp32 [2] on the device: (total_norm, clip_coef)."""
    from . import ops

    out = torch.empty(2, dtype=torch.float32, device=device)
    ops.multi_sumsq(table.dev, table.n_chunks, table.partials, table.numel)
    ops.norm_finish(table.partials, table.n_chunks, max_norm, out)
    return out


# ---- clip_grad_norm_ ------------------------------------------------------------------------------------------------
_CLIP_TABLES = collections.OrderedDict()    # (device, entries) -> ChunkTable; a table holds addresses only
_CLIP_TABLES_MAX = 8


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_ for the 2-norm: scales the gradients in place by min(1, max_norm / (norm + 1e-6))
    and returns the norm as a 0-dim device tensor.  Three launches, no host synchronisation."""
    from . import ops

    if float(norm_type) != 2.0:
        raise ValueError("visitron_amd.optim.clip_grad_norm_ serves norm_type=2 (got %r)" % (norm_type,))
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = list(parameters)
    grads = [_dense(p.grad, "a gradient") for p in params if p.grad is not None]
    if not grads:
        return torch.zeros((), device=params[0].device if params else None)
    device = grads[0].device
    entries = tuple((0, g.data_ptr(), 0, 0, g.numel(), 0) for g in grads)
    table = _CLIP_TABLES.get((device, entries))
    if table is None:
        for g in grads:
            _check(g, "a gradient", device)
        table = ChunkTable(device)
        table.update(entries)
        _CLIP_TABLES[(device, entries)] = table
        while len(_CLIP_TABLES) > _CLIP_TABLES_MAX:
            _CLIP_TABLES.popitem(last=False)
    else:
        _CLIP_TABLES.move_to_end((device, entries))
    if table.n_chunks == 0:
        return torch.zeros((), device=device)
    with torch.cuda.device(device):
        out = _norm_launches(table, max_norm, device)
        ops.multi_scale(table.dev, table.n_chunks, out[1:], table.numel)
    return out[0]


# ---- the optimizers -------------------------------------------------------------------------------------------------
def _step_value(step):
    return int(step.item()) if isinstance(step, torch.Tensor) else int(step)


class _MultiTensorAdam(Optimizer):
    """step() over all parameter groups in one launch of vt_multi_adam.  Subclasses give the rule's host constants and
    the form of a fresh `step` counter."""

    max_grad_norm = None

    def _constants(self, group, t):
        raise NotImplementedError

    def _new_step(self):
        raise NotImplementedError

    def _table_of(self):
        table = self.__dict__.get("_table")
        if table is None:
            table = self.__dict__["_table"] = ChunkTable()
        return table

    @torch.no_grad()
    def step(self, closure=None):
        from . import ops
        from .modeling import invalidate_packed_weights

        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        entries, present, slots, hyper = [], [], {}, []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = _dense(p.grad, "a gradient")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = self._new_step()
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                t = _step_value(st["step"]) + 1
                slot = slots.get((gi, t))
                if slot is None:
                    slot = slots[(gi, t)] = len(hyper)
                    hyper.append(self._constants(group, t))
                m, v = st["exp_avg"], st["exp_avg_sq"]
                entries.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), slot))
                present.append((p, g, st))
        if not entries:
            return loss
        table = self._table_of()
        if table.stale(entries):
            device = present[0][0].device
            for p, g, st in present:
                _check(p, "a parameter", device)
                _check(g, "a gradient", device)
                _check(st["exp_avg"], "exp_avg", device)
                _check(st["exp_avg_sq"], "exp_avg_sq", device)
                if not (g.numel() == st["exp_avg"].numel() == st["exp_avg_sq"].numel() == p.numel()):
                    raise RuntimeError("visitron_amd.optim: a gradient or moment does not have its parameter's size")
            table.device = device
            table.update(entries)
        if table.n_chunks:
            device = table.device
            with torch.cuda.device(device):
                # this step's constants (the schedule's lr, t) in a device buffer of their own: see _upload
                hyper_dev = _upload(hyper, torch.float32, device)
                if self.max_grad_norm is not None:
                    out = _norm_launches(table, self.max_grad_norm, device)
                    ops.multi_adam(table.dev, table.n_chunks, hyper_dev, 1.0, out[1:], table.numel)
                    self.last_grad_norm = out[0]
                else:
                    ops.multi_adam(table.dev, table.n_chunks, hyper_dev, 1.0, None, table.numel)
        for _, _, st in present:
            st["step"] += 1
        # the kernel wrote through raw pointers: no _version moved, the packed bf16 copies of the inference path must follow
        invalidate_packed_weights()
        return loss


class AdamW(_MultiTensorAdam):
    """pytorch-transformers' AdamW (pretrain.py:128-130).  max_grad_norm: clip the global gradient norm inside the step
    (p.grad itself is left unscaled); the norm of the last step is `last_grad_norm`, a 0-dim device tensor."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True,
                 max_grad_norm=None):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: {} - should be in [0.0, 1.0[".format(betas))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias))
        self.max_grad_norm = max_grad_norm

    def _constants(self, group, t):
        return adamw_constants(group["lr"], group["betas"], group["eps"], group["weight_decay"], t, group["correct_bias"])

    def _new_step(self):
        return 0


class Adam(_MultiTensorAdam):
    """torch.optim.Adam's rule (agent.py:129).  Served: lr, betas, eps; weight_decay, amsgrad and maximize are not."""

    _SERVED = "visitron_amd.optim.Adam serves lr, betas and eps (weight_decay=0, amsgrad=False, maximize=False)"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False,
                 max_grad_norm=None):
        if weight_decay != 0:
            raise ValueError("%s: got weight_decay=%r" % (self._SERVED, weight_decay))
        if amsgrad:
            raise ValueError("%s: got amsgrad=%r" % (self._SERVED, amsgrad))
        if maximize:
            raise ValueError("%s: got maximize=%r" % (self._SERVED, maximize))
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: {}".format(betas))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False))
        self.max_grad_norm = max_grad_norm

    def _constants(self, group, t):
        # (a loaded torch.optim.Adam state_dict brings its own group keys)
        if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
            raise ValueError("%s: a parameter group asks for more" % self._SERVED)
        return adam_constants(group["lr"], group["betas"], group["eps"], t)

    def _new_step(self):
        return torch.tensor(0.0, dtype=torch.float32)      # torch.optim.Adam keeps `step` as a host tensor


# ---- schedules (host only) ------------------------------------------------------------------------------------------
class WarmupLinearSchedule(LambdaLR):
    """Linear warm-up from 0 to 1 over `warmup_steps`, then linear decay to 0 at `t_total` (pretrain.py:132-139)."""

    def __init__(self, optimizer, warmup_steps, t_total, last_epoch=-1):
        self.warmup_steps = warmup_steps
        self.t_total = t_total
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)

    def lr_lambda(self, step):
        if step < self.warmup_steps:
            return float(step) / float(max(1, self.warmup_steps))
        return max(0.0, float(self.t_total - step) / float(max(1.0, self.t_total - self.warmup_steps)))


class WarmupConstantSchedule(LambdaLR):
    """Linear warm-up from 0 to 1 over `warmup_steps`, then 1."""

    def __init__(self, optimizer, warmup_steps, last_epoch=-1):
        self.warmup_steps = warmup_steps
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)

    def lr_lambda(self, step):
        if step < self.warmup_steps:
            return float(step) / float(max(1.0, self.warmup_steps))
        return 1.0
