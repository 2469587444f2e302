"""Shared helpers for the parity tests: oracle/product model pairs on identical weights."""
import torch

from visitron_amd.synth import deterministic_state_dict


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def model_pair(oracle_cls, product_cls, cfg, seed=0, device="cuda:0", weight_std=0.05):
    ref = oracle_cls(cfg).eval()
    ref.load_state_dict(deterministic_state_dict(ref, seed=seed, weight_std=weight_std))
    prod = product_cls(cfg).eval()
    prod.load_state_dict(ref.state_dict())
    if hasattr(prod, "tie_weights"):
        prod.tie_weights()
    return ref, prod.to(device)


def maxabs(a, b):
    return float((a.detach().float().cpu() - b.detach().float().cpu()).abs().max())


_MEASURED = []


def _recorded():
    """tests/golden/parity_measured.json: the error every named check measured on an MI355X when its bound was last
    reviewed (written from profiles/r02/parity_measured.txt).  A check then passes only below
    min(stated bound, max(2 x recorded, stated bound / 10)): the stated bound is the contract (north_star's 5e-2 / 1e-3,
    or what the docstring derives), the recorded value keeps a regression from hiding inside a generous contract, and
    the floor of a tenth of the bound keeps noise-level errors (which move with the autotuner's kernel choice and the
    summation order) from failing a healthy run."""
    global _REC
    if _REC is None:
        import json
        import os

        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parity_measured.json")
        _REC = json.load(open(path)) if os.path.exists(path) else {}
    return _REC


_REC = None


# RULE for the regression guard below (round 6, after two rounds in which it moved in the loosening direction at the end of a
# round): the guard's floor (the 0.1 / 0.5 factors of effective_bound) may only be RAISED in a commit of its own that quotes
# the measured series justifying it (as c912670 did), never in a commit that also changes a kernel; the STATED bounds in
# the tests are the contract and do not move with it.
def effective_bound(name, bound, scalar=False):
    """scalar: the checked quantity is a single number (a loss of a two-sequence batch): its error is one draw of the bf16
    noise -- it moved 8e-4 -> 2.9e-3 -> 2.5e-4 between rebuilds that changed nothing but a summation order -- so the recorded
    value says little about the next draw and the floor is half the stated bound instead of a tenth."""
    import os

    # VT_PARITY_RECORD=1: the round's re-measurement run -- stated bounds only, every check recorded
    # (gpurun_out/parity_measured.txt); tools/merge_parity.py then REPLACES the committed record with this run and lists
    # every check that rose by more than 1.5 x (the list and its reason go into the commit message)
    rec = None if os.environ.get("VT_PARITY_RECORD") == "1" else _recorded().get(name)
    if rec is None:
        return bound
    return min(bound, max(2.0 * rec, (0.5 if scalar else 0.1) * bound))


def check_close(name, got, want, bound, kind="maxabs"):
    """Assert |got - want| <= bound and RECORD the measured error: every parity test prints `PARITY name measured bound`
    (run pytest with -s, or read tests' session summary written by conftest) so that a bound can be audited against
    what the kernels actually deliver.  kind: "maxabs" (absolute) or "rel_l2" (||got - want|| / ||want||)."""
    g, w = torch.as_tensor(got).detach().float().cpu(), torch.as_tensor(want).detach().float().cpu()
    g = g.reshape(w.shape)
    if kind == "maxabs":
        err = float((g - w).abs().max()) if w.numel() else 0.0
    elif kind == "rel_l2":
        err = float((g - w).norm() / (w.norm() + 1e-30))
    else:
        raise ValueError(kind)
    stated, bound = float(bound), effective_bound(name, float(bound), scalar=w.numel() <= 1)
    _MEASURED.append((name, kind, err, bound))
    print("PARITY %-58s %-7s measured %.3e  bound %.3e (stated %.1e: margin x%.1f)" % (
        name, kind, err, bound, stated, stated / err if err > 0 else float("inf")))
    assert err <= bound, "%s: %s error %.4e exceeds the bound %.4e (stated %.1e, tightened by the recorded value)" % (
        name, kind, err, bound, stated)
    return err


def measured():
    return list(_MEASURED)


class FixedMaskDropout(torch.nn.Module):
    """nn.Dropout with the keep-mask given instead of drawn: x * keep / (1 - p)."""

    def __init__(self, keep, p):
        super().__init__()
        self.keep, self.p = keep.float(), float(p)

    def forward(self, x):
        return x * self.keep.view_as(x) / (1.0 - self.p)


def inject_dropout_masks(ref, p_hidden, p_attn, seed, B, T, R, device="cuda:0", layout=None):
    """Replace every nn.Dropout of the oracle model by a FixedMaskDropout holding the keep-mask the HIP
    kernels derive from (seed, site, element index) — read back through vt_debug_dropout_mask.

    layout (ops.SeqLayout, the engine's `last_layout`): the step ran on the compacted rows (padding rows dropped).  The
    encoder's row-wise sites then index their elements by COMPACT row (row_c * H + col) and the attention site by
    sequence-relative (query, key) with the sequence's own length as the row pitch; the masks are scattered back to the
    padded [B, S] geometry the oracle computes in (positions the step never computed keep 1: nothing reads them).  The
    embedding and image sites are applied before the compaction and stay in the padded geometry."""
    from visitron_amd import ops

    cfg = ref.config
    H, nh, S = cfg.hidden_size, cfg.num_attention_heads, T + R

    def keep(n, p, site, head=-1):
        return ops.dropout_mask(n, (p, seed, site), head_index=head, device=device).cpu()

    def attn_keep(n, site, head):   # [n, n] of one (batch, head): element (q, k) = index q * n' + k, n' = n rounded up to even
        return ops.attn_dropout_mask(n, (p_attn, seed, site), head, device=device).cpu()

    def setmod(name, mod):
        parent = ref
        parts = name.split(".")
        for q in parts[:-1]:
            parent = getattr(parent, q)
        setattr(parent, parts[-1], mod)

    if layout is not None:
        index = layout.index.cpu()
        start, length = layout.start.cpu().tolist(), layout.length.cpu().tolist()
        pos = [(index[start[b]:start[b] + length[b]] - b * S) for b in range(B)]   # padded positions of b's kept rows

    def rows_site(site):
        if layout is None:
            return keep(B * S * H, p_hidden, site).view(B, S, H)
        full = torch.ones(B * S, H, dtype=torch.uint8)
        full[index] = keep(layout.rows * H, p_hidden, site).view(layout.rows, H)
        return full.view(B, S, H)

    def attn_site(site):
        if layout is None:
            return torch.stack([attn_keep(S, site, i) for i in range(B * nh)]).view(B, nh, S, S)
        full = torch.ones(B, nh, S, S, dtype=torch.uint8)
        for b in range(B):
            n = length[b]
            for h in range(nh):
                blk = attn_keep(n, site, b * nh + h)
                full[b, h][pos[b][:, None], pos[b][None, :]] = blk
        return full

    setmod("bert.embeddings.dropout", FixedMaskDropout(keep(B * T * H, p_hidden, ops.SITE_EMB).view(B, T, H), p_hidden))
    if R:
        setmod("bert.dropout", FixedMaskDropout(keep(B * R * H, p_hidden, ops.SITE_IMG).view(B, R, H), p_hidden))
    for l in range(cfg.num_hidden_layers):
        pre = "bert.encoder.layer.%d." % l
        # (the attention sites run p quantised to 1/256 and scale by the quantised value: ops.attn_drop_p)
        setmod(pre + "attention.self.dropout", FixedMaskDropout(attn_site(ops.site_attn(l)), ops.attn_drop_p(p_attn)))
        setmod(pre + "attention.output.dropout", FixedMaskDropout(rows_site(ops.site_selfout(l)), p_hidden))
        setmod(pre + "output.dropout", FixedMaskDropout(rows_site(ops.site_out(l)), p_hidden))
    return ref


# ---- which layer loop an eval forward takes -----------------------------------------------------------------------------
# The test session sends every eval forward through the deferred-LayerNorm loop (tests/conftest.py: threshold 0); the product
# sends those below DEFERRED_LN_MIN_ROWS_DEFAULT token rows through the seven-launch layer.  The inference comparisons are
# written once, as bodies that take a Route, and run under both: Route() is the session's setting and changes nothing;
# Route(shipped=True) sets the shipped threshold on every model the body builds, marks every check name and PROVES the route
# of every call (tests/test_gpu_shipped_routes.py).
SHIPPED_SUFFIX = " [shipped route]"


def _leaves(out):
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _leaves(o)]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in _leaves(out[k])]
    return [] if out is None else [torch.as_tensor(out)]


def same_bits(a, b):
    """Two (nested) outputs hold the same values bit for bit (NaN equal to NaN: the 7-tuple's corners)."""
    la, lb = _leaves(a), _leaves(b)
    return len(la) == len(lb) and all(x.shape == y.shape and x.dtype == y.dtype
                                      and torch.equal(torch.nan_to_num(x.float(), nan=12345.0), torch.nan_to_num(y.float(), nan=12345.0))
                                      and torch.equal(torch.isnan(x.float()), torch.isnan(y.float())) for x, y in zip(la, lb))


def _clone(out):
    if isinstance(out, torch.Tensor):
        return out.clone()
    if isinstance(out, (tuple, list)):
        return type(out)(_clone(o) for o in out)
    return out


def encoder_of(model):
    from visitron_amd.modeling import CaptionBertEncoder

    encs = [m for m in model.modules() if isinstance(m, CaptionBertEncoder)]
    assert len(encs) == 1, "one trunk per model"
    return encs[0]


class Route(object):
    def __init__(self, shipped=False):
        self.shipped = shipped
        self.suffix = SHIPPED_SUFFIX if shipped else ""
        self.proven = []          # (rows, "seven-launch layer" | "same route under both thresholds") per call, shipped only

    def name(self, s):
        return s + self.suffix

    def check(self, name, got, want, bound, kind="maxabs"):
        return check_close(name + self.suffix, got, want, bound, kind)

    def apply(self, model):
        """The shipped threshold on `model`'s encoder (the session's stays otherwise).  Returns the model."""
        if self.shipped:
            from visitron_amd.modeling import DEFERRED_LN_MIN_ROWS_DEFAULT

            encoder_of(model).deferred_ln_min_rows = DEFERRED_LN_MIN_ROWS_DEFAULT
        return model

    def call(self, model, rows, fn, history=None):
        """fn() -- one eval forward of `model` over `rows` token rows (the count the product's rule sees: padded B x S, or
        the kept rows of a compacted forward).  Session route: fn() as it is.  Shipped route: the rule is asked under both
        thresholds.  Where they agree (history states, per-layer outputs, >= the threshold's rows) the case has run on this
        very route in the session's test already: None is returned and the caller moves on.  Where they differ the shipped
        answer must be the seven-launch layer, fn() runs, and its output must equal, bit for bit, a second run with
        `deferred_ln = False` -- and every serves_deferred_ln call the product made on the way must have asked for `rows`."""
        if not self.shipped:
            return fn()
        from visitron_amd.modeling import DEFERRED_LN_MIN_ROWS_DEFAULT

        enc = encoder_of(model)
        assert enc.deferred_ln_min_rows == DEFERRED_LN_MIN_ROWS_DEFAULT and enc.deferred_ln, "Route.apply() the model first"
        shipped = enc.serves_deferred_ln(history=history, rows=rows)
        enc.deferred_ln_min_rows = 0
        session = enc.serves_deferred_ln(history=history, rows=rows)
        enc.deferred_ln_min_rows = DEFERRED_LN_MIN_ROWS_DEFAULT
        if shipped is session:
            assert shipped is (history is None and not enc.output_attentions and not enc.output_hidden_states), rows
            assert shipped is False or rows >= DEFERRED_LN_MIN_ROWS_DEFAULT
            self.proven.append((rows, "same route under both thresholds"))
            print("ROUTE %d rows: %s under both thresholds -- not run twice" % (
                rows, "deferred-LayerNorm loop" if shipped else "seven-launch layer"))
            return None
        assert shipped is False and session is True and rows < DEFERRED_LN_MIN_ROWS_DEFAULT, rows
        asked, rule = [], enc.serves_deferred_ln

        def spy(history=None, seq=None, rows=None):
            asked.append((rows, rule(history=history, seq=seq, rows=rows)))
            return asked[-1][1]

        enc.serves_deferred_ln = spy
        try:
            out = _clone(fn())     # (a copy: outputs may live in a workspace the next call rewrites)
        finally:
            del enc.serves_deferred_ln
        assert asked and all(a == (rows, False) for a in asked), (rows, asked)
        enc.deferred_ln = False
        try:
            seven = fn()
        finally:
            enc.deferred_ln = True
        assert same_bits(out, seven), "%d rows: not the seven-launch layer's output" % rows
        self.proven.append((rows, "seven-launch layer"))
        print("ROUTE %d rows: seven-launch layer (bitwise equal to deferred_ln = False)" % rows)
        return out
