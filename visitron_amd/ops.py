"""Tensor-level wrappers over the C ABI: torch tensors in, torch tensors out.

torch is plumbing here (device memory + the current HIP stream); all arithmetic of the
hot path runs in ``libvisitron_hip.so``.  Every function raises on CPU tensors.
"""
import ctypes
import os
import re

import torch

from . import _lib, switches

BF16 = torch.bfloat16
ACT_NONE, ACT_GELU, ACT_TANH, ACT_MUL = (_lib.CONSTANTS["VT_ACT_" + a] for a in ("NONE", "GELU", "TANH", "MUL"))
NO_DROP = (0.0, 0, 0)      # (p, step seed, site): dropout disabled
# dropout sites: VT_SITE_* of include/visitron_hip.h (tests/test_host_switches.py holds the two spellings to each other)
SITE_EMB, SITE_IMG = 0xE0, 0xE1


def site_attn(layer):
    return 8 * layer


def site_selfout(layer):
    return 8 * layer + 1


def site_out(layer):
    return 8 * layer + 2


LN_BWD_WS_ROWS = 1024  # vt_layernorm_bwd_bf16 scratch = LN_BWD_WS_ROWS * 2 * H floats


# ---- optional per-launch timing (HIP events on the launch stream); used by bench.py only ----------
_prof = None


def profile_begin():
    global _prof
    _prof = []


def profile_end():
    """-> {kernel: {"ms": total, "n": launches, "flops": algorithmic flops, "bytes": algorithmic bytes}}"""
    global _prof
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1, flops, nbytes in _prof:
        d = out.setdefault(name, {"ms": 0.0, "n": 0, "flops": 0.0, "bytes": 0.0})
        d["ms"] += e0.elapsed_time(e1)
        d["n"] += 1
        d["flops"] += flops
        d["bytes"] += nbytes
    _prof = None
    return out


def profiling():
    return _prof is not None


class _timed(object):
    def __init__(self, name, flops=0.0, nbytes=0.0):
        self.name, self.flops, self.nbytes = name, flops, nbytes

    def __enter__(self):
        if _prof is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if _prof is not None:
            self.e1.record()
            _prof.append((self.name, self.e0, self.e1, self.flops, self.nbytes))
        return False


def _require_hip(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "visitron_amd ops run on a HIP device only (got a %s tensor); there is no CPU fallback" % t.device
            )


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def round_up(x, m):
    return (x + m - 1) // m * m


F16 = torch.float16
# The seven-launch layer (training, compacted-row and diagnostic forwards) keeps its residual stream at fp16 precision: the
# pre-LayerNorm sums are written as fp16 and every LayerNorm output also as an fp16 copy that the next residual add reads
# (include/visitron_hip.h, vt_layer_acts::ln1_h).  VT_F16_STREAM=0: every tensor bf16, as through round 3 (A/B switch).
F16_STREAM = switches.on("VT_F16_STREAM")
# With the fp16 stream, the TRAINING layer does not write the LayerNorm outputs' fp16 copies at all: a residual add reads the
# previous sub-layer's fp16 sum and reconstructs its LayerNorm from the row statistics the LayerNorm kernel wrote
# (vt_layer_acts::ln_residual_mode = 1; linear(..., residual_ln=...)).  VT_LN_RESIDUAL=0: the two-output LayerNorm of round 4.
LN_RESIDUAL = F16_STREAM and switches.on("VT_LN_RESIDUAL")


def linear(a, w, bias=None, residual=None, act=ACT_NONE, out=None, out_f32=False, grp_rows=0, grp_stride=0,
           M=None, lda=None, ldc=None, pre_act_out=None, drop=NO_DROP, residual_ln=None):
    """out = act(a @ w.T + bias) (+ residual).  a [M,K] bf16 (row stride lda), w [N,K] bf16.
    pre_act_out: optional bf16 [M,N] buffer saved for backward: gelu'(a @ w.T + bias) when act == ACT_GELU,
    else a @ w.T + bias.  act == ACT_MUL: out = (a @ w.T) * residual.
    residual_ln = (mean [M], rstd [M], gamma [N], beta [N]), all fp32: `residual` is an FP16 pre-LayerNorm sum v and what is
    added is LayerNorm(v) = (v - mean) * rstd * gamma + beta (vt_linear_lnres_bf16)."""
    _require_hip(a, w, bias, residual, out, pre_act_out)
    assert a.dtype == BF16 and w.dtype == BF16
    N, K = w.shape
    if M is None:
        M = a.shape[0]
    if lda is None:
        assert a.stride(-1) == 1
        lda = a.stride(0)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32 if out_f32 else BF16, device=a.device)
    if ldc is None:
        ldc = out.stride(0)
    ldr = residual.stride(0) if residual is not None else 0
    if residual_ln is not None:
        mean, rstd, gamma, beta = residual_ln
        _require_hip(mean, rstd, gamma, beta)
        assert residual is not None and residual.dtype == F16 and act == ACT_NONE and not out_f32 and pre_act_out is None
        assert grp_rows == 0 and out.dtype in (BF16, F16)
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (mean, rstd, gamma, beta))
        assert mean.numel() >= M and rstd.numel() >= M and gamma.numel() == N and beta.numel() == N
        with _timed("gemm_nt_bf16", 2.0 * M * N * K, 2.0 * (M * K + N * K + 2 * M * N)):
            rc = _lib.load().vt_linear_lnres_bf16(
                _ptr(a), lda, _ptr(w), w.stride(0), _ptr(bias), _ptr(residual), ldr, _ptr(mean), _ptr(rstd), _ptr(gamma),
                _ptr(beta), _ptr(out), ldc, M, N, K, 1 if out.dtype == F16 else 0, float(drop[0]), int(drop[1]),
                int(drop[2]), _stream())
        _lib.check(rc, "vt_linear_lnres_bf16")
        return out
    # an fp16 `out` / `residual` (the training layer's higher-precision residual stream) is told to the library by bits 1 / 2
    # of its output-mode argument
    assert out.dtype == (torch.float32 if out_f32 else out.dtype) and out.dtype in (BF16, F16, torch.float32)
    assert residual is None or residual.dtype in (BF16, F16)
    out_f32 = (1 if out_f32 else 0) | (2 if out.dtype == F16 else 0) | (4 if (residual is not None and residual.dtype == F16) else 0)
    with _timed("gemm_nt_bf16", 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N)):
        rc = _lib.load().vt_linear_bf16_ex(
            _ptr(a), lda, _ptr(w), w.stride(0), _ptr(bias), _ptr(residual), ldr, _ptr(out), ldc,
            _ptr(pre_act_out), 0 if pre_act_out is None else pre_act_out.stride(0),
            M, N, K, act, int(out_f32), grp_rows, grp_stride, float(drop[0]), int(drop[1]), int(drop[2]), _stream())
    _lib.check(rc, "vt_linear_bf16_ex")
    return out


def linear_ln(a, w, bias, colv, stats, eps, ln_mode, act=ACT_NONE, out=None, rs=None, out_s=None, stats_out=None, M=None):
    """A GEMM of the deferred-LayerNorm inference path (vt_linear_ln_bf16; include/visitron_hip.h has the arithmetic).
    a [M,K] bf16 = the bf16 copy of the stream (mode 1) or a plain activation (mode 2); stats fp32 [np, rows, 2] = the
    partial row statistics of the stream being normalised; mode 2 also takes the fp16 stream rs [M,N] and returns the new
    stream (out: its bf16 copy, out_s: fp16, stats_out)."""
    _require_hip(a, w, bias, colv, stats, out, rs, out_s, stats_out)
    assert a.dtype == BF16 and w.dtype == BF16 and stats.dtype == torch.float32 and stats.is_contiguous()
    N, K = w.shape
    if M is None:
        M = a.shape[0]
    np_, rows = stats.shape[0], stats.shape[1]
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a.device)
    if ln_mode == 2:
        assert rs is not None and rs.dtype == F16
        if out_s is None:
            out_s = torch.empty((M, N), dtype=F16, device=a.device)
        if stats_out is None:
            stats_out = torch.empty((N // 128, rows, 2), dtype=torch.float32, device=a.device)
        assert stats_out.shape[1] == rows and stats_out.is_contiguous()
    with _timed("gemm_nt_bf16", 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N) + (4.0 * M * N if ln_mode == 2 else 0.0)):
        rc = _lib.load().vt_linear_ln_bf16(
            _ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(bias), _ptr(colv), _ptr(stats), np_, rows, float(eps), int(ln_mode),
            _ptr(rs), 0 if rs is None else rs.stride(0), _ptr(out), out.stride(0), _ptr(out_s),
            0 if out_s is None else out_s.stride(0), _ptr(stats_out), M, N, K, int(act), _stream())
    _lib.check(rc, "vt_linear_ln_bf16")
    return (out, out_s, stats_out) if ln_mode == 2 else out


def ln_apply(vs, stats, gamma, beta, eps, out16=None, out32=None, M=None):
    """LayerNorm of a stream (fp16 rows + partial statistics) written as bf16 and / or fp32."""
    _require_hip(vs, stats, gamma, beta, out16, out32)
    assert vs.dtype == F16 and stats.dtype == torch.float32 and stats.is_contiguous()
    if M is None:
        M = vs.shape[0]
    H = gamma.numel()
    with _timed("ln_apply_rows", 0.0, M * H * (2.0 + (2.0 if out16 is not None else 0.0) + (4.0 if out32 is not None else 0.0))):
        rc = _lib.load().vt_ln_apply(_ptr(vs), vs.stride(0), _ptr(stats), stats.shape[0], stats.shape[1], _ptr(gamma), _ptr(beta),
                                     float(eps), _ptr(out16), 0 if out16 is None else out16.stride(0), _ptr(out32),
                                     0 if out32 is None else out32.stride(0), M, H, _stream())
    _lib.check(rc, "vt_ln_apply")


def ln_stream_init(x32, xs, x16, stats, eps, M=None):
    """x32 fp32 [M,H] enters the deferred-LayerNorm stack as it is: the stream xs (fp16), its bf16 copy x16, identity
    statistics."""
    _require_hip(x32, xs, x16, stats)
    assert x32.dtype == torch.float32 and xs.dtype == F16 and x16.dtype == BF16 and stats.dtype == torch.float32
    assert stats.is_contiguous()
    if M is None:
        M = x32.shape[0]
    with _timed("ln_stream_init", 0.0, M * x32.shape[1] * 8.0):
        rc = _lib.load().vt_ln_stream_init(_ptr(x32), x32.stride(0), _ptr(xs), xs.stride(0), _ptr(x16), x16.stride(0), _ptr(stats),
                                           stats.shape[0], stats.shape[1], M, x32.shape[1], float(eps), _stream())
    _lib.check(rc, "vt_ln_stream_init")


def encoder_forward_ln(layer_weights, stream_a, stream_b, qkv, ctx, mid, mask, mask_additive, head_scale, B, S, H, nh, I, eps,
                       seq=None):
    """The deferred-LayerNorm layer loop in C.  stream_x = (bf16 copy, fp16 rows, statistics).  seq (SeqLayout): the
    streams hold its compacted rows (no mask)."""
    _require_hip(stream_a[0], mask, head_scale)
    rows = stream_a[2].shape[1]
    if seq is not None:
        if mask is not None:
            raise ValueError("compacted rows carry no mask")
        rc = _lib.load().vt_encoder_forward_ln_seq_bf16(
            layer_weights, len(layer_weights), _ptr(stream_a[0]), _ptr(stream_a[1]), _ptr(stream_a[2]), _ptr(stream_b[0]),
            _ptr(stream_b[1]), _ptr(stream_b[2]), _ptr(qkv), _ptr(ctx), _ptr(mid), _ptr(head_scale), B, S, H, nh, I, float(eps),
            rows, seq.rows, _ptr(seq.start), _ptr(seq.length), _stream())
        _lib.check(rc, "vt_encoder_forward_ln_seq_bf16")
        return
    rc = _lib.load().vt_encoder_forward_ln_bf16(
        layer_weights, len(layer_weights), _ptr(stream_a[0]), _ptr(stream_a[1]), _ptr(stream_a[2]), _ptr(stream_b[0]),
        _ptr(stream_b[1]), _ptr(stream_b[2]), _ptr(qkv), _ptr(ctx), _ptr(mid), _ptr(mask), _mask_mode(mask, mask_additive, B, S),
        _ptr(head_scale), B, S, H, nh, I, float(eps), rows, _stream())
    _lib.check(rc, "vt_encoder_forward_ln_bf16")


# ---- the GEMM kernel variants: csrc/gemm_variants.def is the list (one line per variant, described there) ---------------------
_VARIANT_FLAGS = ("PERSISTENT", "NEEDS_WORKSPACE", "LN_EPILOGUE", "BF16_IO_ONLY", "TUNE_CANDIDATE", "TUNE_CANDIDATE_STREAMK_ONLY")
_VARIANT_LINE = re.compile(r"VT_GEMM_VARIANT\((\d+), (\w+), (\d), (\w+(?: \| \w+)*)(?: \| PLAIN_TWIN\((\d+)\))?\)\s*(?://.*)?")


def _parse_variants(text):
    """gemm_variants.def -> {id: {"family", "mtn", "flags" (frozenset), "twin" (id or None)}} in file order, the variants of the
    experimental build (24 .. 27) included.  The line format is closed: anything else raises."""
    out = {}
    for n, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line or line.startswith("//") or line in ("#ifdef VT_EXPERIMENTAL_GEMM", "#endif"):
            continue
        m = _VARIANT_LINE.fullmatch(line)
        flags = () if not m or m.group(4) == "0" else m.group(4).split(" | ")
        if not m or int(m.group(1)) in out or set(flags) - set(_VARIANT_FLAGS):
            raise ImportError("visitron_amd: line %d of csrc/gemm_variants.def is malformed or names an unknown flag: `%s`" % (n, line))
        out[int(m.group(1))] = {"family": m.group(2), "mtn": int(m.group(3)), "flags": frozenset(flags),
                                "twin": m.group(5) and int(m.group(5))}
    return out


GEMM_VARIANTS = _parse_variants(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "gemm_variants.def")).read())
_variants_with = lambda flag: tuple(v for v, e in GEMM_VARIANTS.items() if flag in e["flags"])
# the stream-K variants measured negative on MI355X at every row count tried: opt-in candidates, never timed by default
STREAMK = switches.on("VT_GEMM_STREAMK")
GEMM_CANDIDATES = _variants_with("TUNE_CANDIDATE") + (_variants_with("TUNE_CANDIDATE_STREAMK_ONLY") if STREAMK else ())   # file order is timing order


# -1: shape table / heuristic; -2: the same plus the tail launch of the persistent kernel's last round (VT_GEMM_TAIL_SPLIT=1)
AUTO_VARIANT = -2 if switches.on("VT_GEMM_TAIL_SPLIT") else -1


def set_gemm_variant(v):
    """Tuning/test hook: force one GEMM kernel variant (-1: shape table / heuristic)."""
    if int(v) in SHARED_TILE_VARIANTS:
        ensure_gemm_workspace()
    _lib.load().vt_debug_set_gemm_variant(int(AUTO_VARIANT if v == -1 else v))
# The persistent kernel launches one workgroup per CU and needs every CU to itself (512 registers per wave, 132 KiB
# of LDS): a collective running beside it on a few CUs makes the workgroups mapped to those CUs wait for a whole kernel
# time.  Data-parallel training (gradient all-reduce overlapped with the backward) therefore tunes without it; the
# one-tile-per-workgroup forms of the same kernel are within 1 % over the step and simply queue their tiles.
PERSISTENT_GEMM_OK = True
PERSISTENT_VARIANTS = _variants_with("PERSISTENT")
SHARED_TILE_VARIANTS = _variants_with("NEEDS_WORKSPACE")   # the GEMM workspace below (stream-K region; split-K planes)


def multi_rank_gemm_policy(environ=None):
    """What the NT GEMM does under more than one rank -> (k, text).  k == 0 (the default): the persistent kernels stand down
    and the one-tile-per-workgroup forms (15, 22, 23: within 0-0.8 % over the step on one GPU) queue their tiles behind
    whatever RCCL occupies.  k > 0: they stay in the candidate list and launch on CUs - k workgroups, leaving k compute units
    to the collective's kernels -- OPT-IN through VT_GEMM_RESERVE_CUS=k only: the reservation has never been measured beside a
    real RCCL collective (no multi-GPU node in five rounds; the weight-gradient side stream competes for the same k CUs), so
    nothing switches it on by inference.  (Round 4 derived k from NCCL_MAX_NCHANNELS; withdrawn: one RCCL workgroup per
    channel is an assumption, not a measurement.)  Both policies have a profiled single-rank twin: profiles/r05/bench_b36_*.json."""
    v = switches.text("VT_GEMM_RESERVE_CUS", environ=environ)
    if v is not None and str(v).strip().lstrip("-").isdigit():
        k = max(0, int(v))
        if 0 < k <= 64:
            return k, "persistent GEMM on CUs - %d (VT_GEMM_RESERVE_CUS)" % k
        return 0, "persistent GEMM off beside the collective (VT_GEMM_RESERVE_CUS=%s): one-tile-per-workgroup kernels" % str(v).strip()
    return 0, ("persistent GEMM off beside the collective (default; VT_GEMM_RESERVE_CUS=k opts into the persistent kernels on "
               "CUs - k): one-tile-per-workgroup kernels")
_tuned = {}
_timed_keys = set()   # keys of _tuned whose variant came out of timing launches (deterministic mode re-registers those)
_forced_variant = None


def set_deterministic(flag):
    """Process-wide switch (include/visitron_hip.h, vt_set_deterministic): with it on two runs of the same training step on
    the same data agree bit for bit.  The attention backward over more than 256 keys sums its key blocks' dQ partials from
    planes in key-block order, the persistent weight-gradient kernel adds a tile's row ranges in row-range order and its
    bias gradient without atomics, and the GEMM kernel of a shape no longer depends on timing: autotune_linear takes
    VT_TUNE_FILE or the committed gemm_defaults.json, as under VT_AUTOTUNE=0, and launches nothing.  Read by every call
    when it launches (nothing caches it): set it before a step, not between a forward and its backward.  Off (default):
    every launch, workspace and result as without the switch.  Not covered: the reduction order inside RCCL."""
    _lib.load().vt_set_deterministic(1 if flag else 0)


def is_deterministic():
    return bool(_lib.load().vt_get_deterministic())


def attention_bwd_ws_bytes(B, S, nh, rows=None):
    """Bytes of the dq32 workspace attention_bwd needs for this shape in the current mode (rows: the compacted row count,
    default B * S): 0 up to 256 keys, rows * nh * 64 * 4 beyond, times ceil(S / 256) under set_deterministic(True)."""
    return int(_lib.load().vt_attention_bwd_ws_bytes(int(B), int(S), int(nh), int(B * S if rows is None else rows)))


def force_gemm_variant(v):
    """Test hook: every linear() takes kernel variant `v` and the autotuner stands down (None: back to automatic).
    With one variant everywhere two processes run the same summation order, so their results can be compared exactly."""
    global _forced_variant
    _forced_variant = None if v is None else int(v)
    if v is not None and int(v) in SHARED_TILE_VARIANTS:
        ensure_gemm_workspace()
    _lib.load().vt_debug_set_gemm_variant(AUTO_VARIANT if v is None else int(v))


def tune_kind(act, residual=False, pre_act=False, out_f32=False, ln_mode=0):
    """The epilogue part of the autotuner's key, as the library derives it from a call's arguments (VT_TUNE_KIND in
    include/visitron_hip.h; tests/test_host_switches.py holds the two to each other): act | 16 residual / factor operand |
    32 second output | 64 fp32 output | ln_mode << 8."""
    return int(act) | (16 if (residual or act == ACT_MUL) else 0) | (32 if pre_act else 0) | (64 if out_f32 else 0) | (int(ln_mode) << 8)


# the deferred-LayerNorm epilogues exist on the 256x256-tile kernels
LN_GEMM_CANDIDATES = tuple(v for v in GEMM_CANDIDATES if "LN_EPILOGUE" in GEMM_VARIANTS[v]["flags"])
TUNE_ROUNDS = 3          # interleaved timing rounds per candidate; a candidate's time is the MEDIAN of its rounds
TUNE_KEEP_DEFAULT = 0.03   # the committed default stays unless a candidate beats it by more than this fraction
_defaults = None


def _default_table():
    """visitron_amd/gemm_defaults.json: kernel choices measured on an MI355X for the path's own shapes ("M,N,K,kind" ->
    variant), committed with the package.  A box whose timings are noisy keeps them (TUNE_KEEP_DEFAULT); VT_AUTOTUNE=0
    takes them without timing anything (nearest M of the same (N, K, kind) within 25 %)."""
    global _defaults
    if _defaults is None:
        import json
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_defaults.json")
        _defaults = {}
        if os.path.exists(path):
            with open(path) as fh:
                for k, v in json.load(fh).items():
                    if not k.startswith("_"):
                        _defaults[tuple(int(x) for x in k.split(","))] = int(v)
    return _defaults


def _default_variant(key):
    tab = _default_table()
    if key in tab:
        return tab[key]
    M, N, K, kind = key
    best, best_d = None, None
    for (m, n, k, kd), v in tab.items():
        if (n, k, kd) == (N, K, kind) and 4 * abs(m - M) <= m and (best_d is None or abs(m - M) < best_d):
            best, best_d = v, abs(m - M)
    return best


def autotune_linear(M, N, K, act=ACT_NONE, residual=False, pre_act=False, device="cuda", reps=6, out_f32=False, ln_mode=0):
    """Time the GEMM kernel variants on one shape AND epilogue (random data, HIP events) and register the fastest in the
    library's table.  Every candidate is timed in TUNE_ROUNDS interleaved rounds (candidate order inside a round, rounds
    outside: drift of the clock or of a neighbour's load hits all candidates alike) and judged by its median; the committed
    default (gemm_defaults.json) is kept unless beaten by more than TUNE_KEEP_DEFAULT.  Synchronises; call it before the
    timed region / graph capture."""
    kind = tune_kind(act, residual, pre_act, out_f32, ln_mode)
    key = (M, N, K, kind)
    if _forced_variant is not None:
        return _forced_variant
    det = is_deterministic()
    if key in _tuned and not (det and key in _timed_keys):
        return _tuned[key]
    lib = _lib.load()
    have_ws = ensure_gemm_workspace(device)   # (before any variant is registered: SHARED_TILE_VARIANTS need it at launch time)
    # The training layer's residual GEMMs (out-proj, FFN-down) read an fp16 residual and write the fp16 pre-LayerNorm sum
    # (F16_STREAM); the grouped epilogue of the BF16_IO_ONLY variants cannot and the library would silently run the default
    # variant in their place -- a kernel never timed for the shape.  Such kinds are tuned with the dtypes they run with, without them.
    f16_io = F16_STREAM and residual and act == ACT_NONE and not out_f32 and not pre_act and not ln_mode
    usable = lambda v: (v is not None and (v not in PERSISTENT_VARIANTS or PERSISTENT_GEMM_OK)
                        and not (f16_io and "BF16_IO_ONLY" in GEMM_VARIANTS[v]["flags"]) and (have_ws or v not in SHARED_TILE_VARIANTS))
    saved = _tune_file_table().get("%d,%d,%d,%d" % key)
    if usable(saved):   # VT_TUNE_FILE: a previous run's choices
        lib.vt_gemm_tune(M, N, K, kind, int(saved))
        _tuned[key] = int(saved)
        return _tuned[key]
    default = _default_variant(key)
    if (det or not switches.on("VT_AUTOTUNE")) and usable(default):
        lib.vt_gemm_tune(M, N, K, kind, int(default))
        _tuned[key] = int(default)
        _timed_keys.discard(key)
        return _tuned[key]
    if det:
        # no committed choice for this (N, K, epilogue) near M: nothing is registered and the library takes its built-in
        # choice, a function of the shape and of the entries registered so far.  (A choice that timing registered for this
        # very key while the switch was off cannot be withdrawn from the library's table and stays: for two PROCESSES to
        # agree, set the switch before the first step.)
        return _tuned.get(key)
    g = torch.Generator(device=device).manual_seed(M + N + K)   # on the device: a CPU draw of M x 3072 values costs seconds
    a = torch.randn(M, K, generator=g, device=device).to(BF16)
    w = (torch.randn(N, K, generator=g, device=device) * 0.03).to(BF16)
    b = torch.zeros(N, device=device)
    if ln_mode:
        H = K if ln_mode == 1 else N
        np_, rows = H // 128, round_up(M, 16)
        stats = torch.zeros((np_, rows, 2), device=device)
        stats[0, :, 1] = float(H)
        colv = torch.ones(N, device=device)
        r16 = torch.randn(M, N, generator=g, device=device).to(F16) if ln_mode == 2 else None
        out = torch.empty((M, N), dtype=BF16, device=device)
        o16 = torch.empty((M, N), dtype=F16, device=device) if ln_mode == 2 else None
        so = torch.empty((N // 128, rows, 2), device=device) if ln_mode == 2 else None

        def run():
            linear_ln(a, w, b, colv, stats, 1e-12, ln_mode, act=act, out=out, rs=r16, out_s=o16, stats_out=so)
    else:
        r = torch.randn(M, N, generator=g, device=device).to(F16 if f16_io else BF16) if (residual or act == ACT_MUL) else None
        out = torch.empty((M, N), dtype=torch.float32 if out_f32 else (F16 if f16_io else BF16), device=device)
        pre = torch.empty((M, N), dtype=BF16, device=device) if pre_act else None
        # LN_RESIDUAL (the training layer's default): those two GEMMs run the rebuilt-LayerNorm epilogue (vt_linear_lnres_bf16:
        # four more LDS-DMA pieces and the vectors' ds_reads per slab) -- time THAT epilogue, with its operands
        rln = None
        if f16_io and LN_RESIDUAL:
            rln = (torch.randn(M, generator=g, device=device), torch.rand(M, generator=g, device=device) + 0.5,
                   torch.ones(N, device=device), torch.zeros(N, device=device))

        def run():
            linear(a, w, b, residual=r, act=act, out=out, pre_act_out=pre, out_f32=out_f32, residual_ln=rln)
    cands = [v for v in (LN_GEMM_CANDIDATES if ln_mode else GEMM_CANDIDATES) if usable(v)]
    if not ln_mode and f16_io and LN_RESIDUAL:
        cands = [v for v in cands if v != 16]   # (the library gives such a GEMM the 224-row tile: 16 would time variant 18 twice)
    times = {v: [] for v in cands}
    for rnd in range(TUNE_ROUNDS):
        for v in list(cands):
            lib.vt_debug_set_gemm_variant(v)
            try:
                for _ in range(2 if rnd == 0 else 1):
                    run()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    run()
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) / reps)
            except RuntimeError:
                cands.remove(v)
                times.pop(v, None)
    lib.vt_debug_set_gemm_variant(AUTO_VARIANT)
    med = {v: sorted(t)[len(t) // 2] for v, t in times.items() if t}
    best = min(med, key=med.get)
    if usable(default) and default in med and med[default] <= med[best] * (1.0 + TUNE_KEEP_DEFAULT):
        best = default
    if switches.on("VT_TUNE_VERBOSE"):
        for v in sorted(med):
            print("  tune M=%d N=%d K=%d kind=%d variant %2d: %8.1f us %6.0f TF  (rounds %s)%s" % (
                M, N, K, kind, v, med[v] * 1e3, 2.0 * M * N * K / (med[v] * 1e-3) * 1e-12,
                " ".join("%.1f" % (t * 1e3) for t in times[v]), "  <- chosen" if v == best else ""))
    lib.vt_gemm_tune(M, N, K, kind, best)
    _tuned[key] = best
    _timed_keys.add(key)
    _tune_file_store(key, best)
    return best


_tune_file = None


def _tune_file_table():
    """VT_TUNE_FILE=<json>: the autotuner's choices are read from / added to this file, so a later process (a profiler
    run, a serving start-up) skips the timing launches.  Unset: no file."""
    global _tune_file
    if _tune_file is None:
        _tune_file = {}
        path = switches.text("VT_TUNE_FILE")
        if path and os.path.exists(path):
            import json
            with open(path) as fh:
                _tune_file = dict(json.load(fh))
    return _tune_file


def _tune_file_store(key, best):
    path = switches.text("VT_TUNE_FILE")
    if not path:
        return
    import json
    tab = _tune_file_table()
    tab["%d,%d,%d,%d" % key] = int(best)
    with open(path, "w") as fh:
        json.dump(tab, fh, indent=0, sort_keys=True)


def autotune_encoder_shapes_ln(M, H, I, device="cuda"):
    """The five GEMM launches of one deferred-LayerNorm encoder layer at M token rows (four distinct shape / epilogue pairs)."""
    return dict(qkv=autotune_linear(M, 3 * H, H, ln_mode=1, device=device),
                attn_out=autotune_linear(M, H, H, ln_mode=2, device=device),
                ffn_up=autotune_linear(M, I, H, act=ACT_GELU, ln_mode=1, device=device),
                ffn_down=autotune_linear(M, H, I, ln_mode=2, device=device))


def autotune_encoder_shapes(M, H, I, training=False, device="cuda"):
    """Tune every GEMM shape of one encoder layer at M token rows (forward; plus the dgrads when training)."""
    res = {}
    res["qkv"] = autotune_linear(M, 3 * H, H, device=device)
    res["attn_out"] = autotune_linear(M, H, H, residual=True, device=device)
    res["ffn_up"] = autotune_linear(M, I, H, act=ACT_GELU, pre_act=training, device=device)
    res["ffn_down"] = autotune_linear(M, H, I, residual=True, device=device)
    if training:
        res["d_ffn_down"] = autotune_linear(M, I, H, act=ACT_MUL, device=device)
        res["d_qkv"] = autotune_linear(M, H, 3 * H, residual=True, device=device)
        res["d_ffn_up"] = autotune_linear(M, H, I, residual=True, device=device)    # same kernel entry as ffn_down: listed for the record
        res["d_attn_out"] = autotune_linear(M, H, H, device=device)                  # the plain dgrad: not the out-proj's entry
    return res


def _mask_mode(mask, mask_additive, B, S):
    """0: raw [B,S] mask, 1: additive [B,S] bias, 2: additive per-query bias [B,S,S] (the reference's 3-D masks)."""
    if mask is None:
        return 0
    assert mask.dtype == torch.float32 and mask.is_contiguous()
    if mask.dim() == 3:
        assert mask_additive and mask.shape == (B, S, S), "per-query masks are passed as the additive bias [B,S,S]"
        return 2
    assert mask.numel() == B * S
    return 1 if mask_additive else 0


class SeqLayout(object):
    """Compacted token rows (a batch without its padding rows): sequence b = rows start[b] .. start[b] + length[b] of
    every activation; `rows` real rows in all, at most S per sequence.  index = the kept rows' positions in the padded
    [B*S] order (int64), inverse[padded position] = compact row or -1."""

    def __init__(self, keep, rows=None):
        """rows: the number of kept positions when the caller already knows it (no host synchronisation here then)."""
        assert keep.dim() == 2 and keep.dtype == torch.bool
        B, S = keep.shape
        lens = keep.sum(1)
        self.B, self.S = B, S
        self.length = lens.to(torch.int32).contiguous()
        self.start = (torch.cumsum(lens, 0) - lens).to(torch.int32).contiguous()
        flat = keep.reshape(-1)
        if rows is None:
            self.index = torch.nonzero(flat).flatten()
            self.rows = int(self.index.numel())                 # host sync
        else:
            self.rows = int(rows)
            self.index = torch.nonzero_static(flat, size=self.rows).flatten()
        inv = torch.cumsum(flat.to(torch.int64), 0) - 1
        self.inverse = torch.where(flat, inv, torch.full_like(inv, -1))
        self._gather = None

    @classmethod
    def from_parts(cls, B, S, rows, index, inverse, start, length):
        """A layout whose tensors were built elsewhere (ops.batch_row_lists): no kernels, no synchronisation."""
        self = cls.__new__(cls)
        self.B, self.S, self.rows = int(B), int(S), int(rows)
        self.index, self.inverse, self.start, self.length = index, inverse, start, length
        self._gather = None
        return self

    def gather_index(self, zero_row):
        """int64 [B*S]: for every padded position its compact row, or `zero_row` (a row the caller keeps at zero) where the
        position was dropped -- un-compaction as ONE index_select instead of a fill + index_copy."""
        if self._gather is None or self._gather[0] != zero_row:
            self._gather = (zero_row, torch.where(self.inverse < 0, torch.full_like(self.inverse, zero_row), self.inverse))
        return self._gather[1]

    def gather_index_split(self, zero_row, T):
        """The same index as two lists: the first T positions of every sequence, and the rest (text | regions) -- each
        part then lands contiguous, [B*T, H] and [B*(S-T), H]."""
        idx = self.gather_index(zero_row).view(self.B, self.S)
        return idx[:, :T].reshape(-1), idx[:, T:].reshape(-1)


def keep_words(B, nh, S):
    """Words of a dropout keep buffer (VT_KEEP_WORDS in include/visitron_hip.h): one per (batch, head, 32-query block, key)."""
    nqb = (S + 31) // 32
    return B * nh * nqb * nqb * 32


def unpack_keep_bits(keep_bits, B, nh, S):
    """bool [B, nh, S, S] (query, key) from the keep words attention_fwd wrote (word ((b nh + h) nqb + qb) kpitch + key, bit j =
    query 32 qb + j): torch ops, for the rarely used output_attentions of a training-mode forward."""
    nqb = (S + 31) // 32
    kp = nqb * 32
    w = keep_bits[:B * nh * nqb * kp].view(B, nh, nqb, 1, kp)
    j = torch.arange(32, device=keep_bits.device, dtype=torch.int32).view(1, 1, 1, 32, 1)
    bits = torch.bitwise_and(torch.bitwise_right_shift(w, j), 1)
    return bits.reshape(B, nh, nqb * 32, kp)[:, :, :S, :S].bool()


def attention_fwd(qkv, B, S, nh, mask=None, mask_additive=False, head_scale=None, out=None, lse=None, drop=NO_DROP,
                  seq=None, keep_bits=None):
    """qkv [B*S, 3*nh*64] bf16, mask fp32 [B,S] -> context [B*S, nh*64] bf16.  seq (SeqLayout): compacted rows, no
    mask.  keep_bits (int32 [keep_words(B, nh, S)], training with dropout): receives the keep decisions for attention_bwd."""
    _require_hip(qkv, mask, head_scale, out, lse, keep_bits)
    assert qkv.dtype == BF16
    if keep_bits is not None:
        assert keep_bits.dtype == torch.int32 and keep_bits.is_contiguous() and keep_bits.numel() >= keep_words(B, nh, S)
    H = nh * 64
    if seq is not None:
        assert mask is None and seq.B == B and seq.S == S and qkv.shape[0] >= seq.rows
        if out is None:
            out = torch.empty((seq.rows, H), dtype=BF16, device=qkv.device)
        with _timed("attention_fwd_d64", 4.0 * B * nh * S * S * 64, 2.0 * seq.rows * 4 * H):
            rc = _lib.load().vt_attention_fwd_seq_bf16(
                _ptr(qkv), qkv.stride(0), _ptr(head_scale), _ptr(out), out.stride(0), _ptr(lse), B, S, nh, 64,
                float(drop[0]), int(drop[1]), int(drop[2]), _ptr(seq.start), _ptr(seq.length), _ptr(keep_bits), _stream())
        _lib.check(rc, "vt_attention_fwd_seq_bf16")
        return out
    if out is None:
        out = torch.empty((B * S, H), dtype=BF16, device=qkv.device)
    mode = _mask_mode(mask, mask_additive, B, S)
    with _timed("attention_fwd_d64", 4.0 * B * nh * S * S * 64, 2.0 * B * S * 4 * H):
        rc = _lib.load().vt_attention_fwd_bf16(
            _ptr(qkv), qkv.stride(0), _ptr(mask), mode, _ptr(head_scale), _ptr(out),
            out.stride(0), _ptr(lse), B, S, nh, 64, float(drop[0]), int(drop[1]), int(drop[2]), _ptr(keep_bits), _stream())
    _lib.check(rc, "vt_attention_fwd_bf16")
    return out


def keep_words_rect(B, nh, Sq, Sk):
    """Words of the rectangular attention's keep buffer (VT_KEEP_WORDS_RECT in include/visitron_hip.h): one per (batch, head,
    32-query block, key), the key pitch Sk rounded up to 32.  Sq == Sk: keep_words(B, nh, Sk)."""
    return B * nh * ((Sq + 31) // 32) * ((Sk + 31) // 32 * 32)


def unpack_keep_bits_rect(keep_bits, B, nh, Sq, Sk):
    """bool [B, nh, Sq, Sk] (query, key) from the keep words attention_rect_fwd wrote (word ((b nh + h) nqb + qb) kpitch + key,
    bit j = query 32 qb + j, nqb = ceil(Sq / 32), kpitch = Sk rounded up to 32)."""
    nqb = (Sq + 31) // 32
    kp = (Sk + 31) // 32 * 32
    w = keep_bits[:B * nh * nqb * kp].view(B, nh, nqb, 1, kp)
    j = torch.arange(32, device=keep_bits.device, dtype=torch.int32).view(1, 1, 1, 32, 1)
    bits = torch.bitwise_and(torch.bitwise_right_shift(w, j), 1)
    return bits.reshape(B, nh, nqb * 32, kp)[:, :, :Sq, :Sk].bool()


def _mask_mode_rect(mask, mask_additive, B, Sq, Sk):
    """_mask_mode over Sk keys: 0 raw [B,Sk], 1 additive [B,Sk], 2 additive per query [B,Sq,Sk]."""
    if mask is None:
        return 0
    assert mask.dtype == torch.float32 and mask.is_contiguous()
    if mask.dim() == 3:
        assert mask_additive and mask.shape == (B, Sq, Sk), "per-query masks are passed as the additive bias [B,Sq,Sk]"
        return 2
    assert mask.numel() == B * Sk
    return 1 if mask_additive else 0


def attention_rect_fwd(qkv, B, Sq, Sk, nh, mask=None, mask_additive=False, head_scale=None, out=None, lse=None, drop=NO_DROP,
                       keep_bits=None):
    """Sq queries over Sk >= Sq keys (encoder_history_states): qkv [B*Sk, 3*nh*64] bf16 of the extended rows, a sequence's
    queries its last Sq rows; mask fp32 over the Sk keys -> context [B*Sq, nh*64] bf16.  lse: fp32 [B, nh, Sq] or None.
    keep_bits (int32 [keep_words_rect(B, nh, Sq, Sk)], dropout on): receives the keep decisions for attention_rect_bwd."""
    _require_hip(qkv, mask, head_scale, out, lse, keep_bits)
    assert qkv.dtype == BF16 and qkv.shape[0] >= B * Sk
    if keep_bits is not None:
        assert keep_bits.dtype == torch.int32 and keep_bits.is_contiguous() and keep_bits.numel() >= keep_words_rect(B, nh, Sq, Sk)
    if lse is not None:
        assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() >= B * nh * Sq
    H = nh * 64
    if out is None:
        out = torch.empty((B * max(Sq, 0), H), dtype=BF16, device=qkv.device)
    mode = _mask_mode_rect(mask, mask_additive, B, Sq, Sk) if 1 <= Sq <= Sk else 0
    with _timed("attention_rect_fwd_d64", 4.0 * B * nh * Sq * Sk * 64, 2.0 * B * (3 * Sk + Sq) * H):
        rc = _lib.load().vt_attention_rect_fwd_bf16(
            _ptr(qkv), qkv.stride(0), _ptr(mask), mode, _ptr(head_scale), _ptr(out), out.stride(0), _ptr(lse), B, Sq, Sk, nh, 64,
            float(drop[0]), int(drop[1]), int(drop[2]), _ptr(keep_bits), _stream())
    _lib.check(rc, "vt_attention_rect_fwd_bf16")
    return out


def attention_rect_bwd(qkv, dctx, ctx, lse, B, Sq, Sk, nh, mask=None, mask_additive=False, out=None, drop=NO_DROP,
                       keep_bits=None):
    """Gradient of attention_rect_fwd w.r.t. the packed qkv: dqkv [B*Sk, 3*nh*64] bf16; the dq columns of the Sk - Sq history
    rows of every sequence are written as zeros.  No workspace, no atomics: the same bits on every run."""
    _require_hip(qkv, dctx, ctx, lse, mask, out, keep_bits)
    assert qkv.dtype == BF16 and dctx.dtype == BF16 and ctx.dtype == BF16 and lse.dtype == torch.float32
    if keep_bits is not None:
        assert keep_bits.dtype == torch.int32 and keep_bits.is_contiguous() and keep_bits.numel() >= keep_words_rect(B, nh, Sq, Sk)
    H = nh * 64
    if out is None:
        out = torch.empty((B * Sk, 3 * H), dtype=BF16, device=qkv.device)
    mode = _mask_mode_rect(mask, mask_additive, B, Sq, Sk) if 1 <= Sq <= Sk else 0
    with _timed("attention_rect_bwd_d64", 14.0 * B * nh * Sq * Sk * 64, 2.0 * B * (6 * Sk + 2 * Sq) * H):
        rc = _lib.load().vt_attention_rect_bwd_bf16(
            _ptr(qkv), qkv.stride(0), _ptr(dctx), dctx.stride(0), _ptr(ctx), ctx.stride(0), _ptr(mask), mode, _ptr(lse),
            _ptr(out), out.stride(0), B, Sq, Sk, nh, 64, float(drop[0]), int(drop[1]), int(drop[2]), _ptr(keep_bits), _stream())
    _lib.check(rc, "vt_attention_rect_bwd_bf16")
    return out


def attention_probs(qkv, lse, B, S, nh, mask=None, mask_additive=False, head_scale=None):
    """fp32 [B, nh, S, S] attention probabilities (config.output_attentions) from qkv and attention_fwd's lse."""
    _require_hip(qkv, lse, mask, head_scale)
    assert qkv.dtype == BF16 and lse.dtype == torch.float32 and lse.numel() == B * nh * S
    probs = torch.empty((B, nh, S, S), dtype=torch.float32, device=qkv.device)
    rc = _lib.load().vt_attention_probs_f32(_ptr(qkv), qkv.stride(0), _ptr(mask), _mask_mode(mask, mask_additive, B, S),
                                            _ptr(head_scale), _ptr(lse), _ptr(probs), B, S, nh, 64, _stream())
    _lib.check(rc, "vt_attention_probs_f32")
    return probs


def layernorm(x, gamma, beta, eps, out=None, mean=None, rstd=None, M=None, grp_rows=0, grp_stride=0, out_h=None):
    """BertLayerNorm over bf16 rows -> bf16; or over FP16 rows (the pre-LayerNorm sums of a layer that keeps fp16 copies of
    its residual stream) -> bf16 (out) and, with out_h, the same values as fp16 (the next sub-layer's residual operand)."""
    _require_hip(x, gamma, beta, out, out_h)
    assert x.dtype in (BF16, F16) and gamma.dtype == torch.float32
    H = gamma.numel()
    if M is None:
        M = x.shape[0]
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    if x.dtype == F16:
        assert grp_rows == 0 and (out_h is None or out_h.dtype == F16)
        with _timed("layernorm_rows", 0.0, (4.0 if out_h is None else 6.0) * M * H):
            rc = _lib.load().vt_layernorm_h_bf16(
                _ptr(x), x.stride(0), _ptr(out), out.stride(0), _ptr(out_h), 0 if out_h is None else out_h.stride(0),
                _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd), M, H, float(eps), _stream())
        _lib.check(rc, "vt_layernorm_h_bf16")
        return out
    assert out_h is None
    with _timed("layernorm_rows", 0.0, 4.0 * M * H):
        rc = _lib.load().vt_layernorm_bf16(
            _ptr(x), x.stride(0), _ptr(out), out.stride(0), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd),
            M, H, float(eps), grp_rows, grp_stride, _stream())
    _lib.check(rc, "vt_layernorm_bf16")
    return out


def embed_layernorm(ids, type_ids, pos_ids, word, pos, typ, gamma, beta, eps, out, S, err_flag=None, drop=NO_DROP):
    """Writes rows b*S + t (t < T) of ``out`` [B*S, H] bf16."""
    _require_hip(ids, word, out)
    B, T = ids.shape
    H = word.shape[1]
    for t in (ids, type_ids, pos_ids):
        assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.shape == ids.shape)
    for t in (word, pos, typ):
        assert t.dtype == torch.float32 and t.is_contiguous()
    with _timed("embed_layernorm", 0.0, B * T * H * 14.0):
        rc = _lib.load().vt_embed_layernorm(
            _ptr(ids), _ptr(type_ids), _ptr(pos_ids), _ptr(word), _ptr(pos), _ptr(typ), _ptr(gamma), _ptr(beta),
            _ptr(out), out.stride(0), B, T, S, H, word.shape[0], pos.shape[0], typ.shape[0], float(eps),
            _ptr(err_flag), float(drop[0]), int(drop[1]), _stream())
    _lib.check(rc, "vt_embed_layernorm")
    return out


_MASK_KINDS = {torch.float32: 0, torch.int64: 1, torch.int32: 2, torch.bool: 3, torch.uint8: 3}


def center_mask(mask):
    """fp32 [B, S] = mask - rowmax(mask) + 1 for a per-key attention mask of any of the dtypes callers pass (one launch;
    other dtypes are cast to fp32 first).  See modeling._centered_mask for what the shift is for."""
    _require_hip(mask)
    assert mask.dim() == 2
    if mask.dtype not in _MASK_KINDS:
        mask = mask.to(torch.float32)
    if mask.stride(1) != 1:
        mask = mask.contiguous()
    B, S = mask.shape
    out = torch.empty((B, S), dtype=torch.float32, device=mask.device)
    rc = _lib.load().vt_center_mask(_ptr(mask), _MASK_KINDS[mask.dtype], mask.stride(0), _ptr(out), B, S, _stream())
    _lib.check(rc, "vt_center_mask")
    return out


def pack_concat(s0, s1, kpad, out=None):
    """bf16([s0 | s1 | 0-pad]) row-wise; s0 [rows,d0], s1 [rows,d1] fp32 contiguous."""
    _require_hip(s0, s1, out)
    assert s0.dtype == torch.float32 and s0.is_contiguous()
    rows, d0 = s0.shape
    d1 = 0
    if s1 is not None:
        assert s1.dtype == torch.float32 and s1.is_contiguous() and s1.shape[0] == rows
        d1 = s1.shape[1]
    if out is None:
        out = torch.empty((rows, kpad), dtype=BF16, device=s0.device)
    with _timed("pack_concat_bf16", 0.0, rows * (4.0 * (d0 + d1) + 2.0 * kpad)):
        rc = _lib.load().vt_pack_concat_bf16(_ptr(s0), d0, _ptr(s1), d1, _ptr(out), kpad, rows, _stream())
    _lib.check(rc, "vt_pack_concat_bf16")
    return out


def attention_bwd(qkv, dctx, ctx, lse, B, S, nh, mask=None, mask_additive=False, out=None, delta_ws=None, dq32_ws=None,
                  drop=NO_DROP, seq=None, keep_bits=None):
    """Gradient of attention_fwd w.r.t. the packed qkv: returns dqkv [B*S, 3*nh*64] bf16 (seq: compacted rows).
    keep_bits: the buffer attention_fwd filled with the same drop (else the mask is recomputed from the hash)."""
    _require_hip(qkv, dctx, ctx, lse, mask, out, keep_bits)
    if keep_bits is not None:
        assert keep_bits.dtype == torch.int32 and keep_bits.is_contiguous() and keep_bits.numel() >= keep_words(B, nh, S)
    H = nh * 64
    nrows = B * S if seq is None else seq.rows
    if out is None:
        out = torch.empty((nrows, 3 * H), dtype=BF16, device=qkv.device)
    if delta_ws is None:
        delta_ws = torch.empty((B, nh, S), dtype=torch.float32, device=qkv.device)
    # the dQ workspace of the current mode (one fp32 slab; under set_deterministic one plane per key block): the library's
    # own figure, and a caller's buffer that is smaller is refused here -- the kernels cannot check it
    need = attention_bwd_ws_bytes(B, S, nh, nrows)
    if dq32_ws is None and need:
        dq32_ws = torch.empty(need // 4, dtype=torch.float32, device=qkv.device)
    if need:
        _require_hip(dq32_ws)
        if dq32_ws.dtype != torch.float32 or not dq32_ws.is_contiguous() or dq32_ws.numel() * 4 < need:
            raise ValueError("attention_bwd: dq32_ws must be a contiguous fp32 tensor of at least %d bytes for B=%d S=%d nh=%d "
                             "rows=%d (deterministic mode %s), got %s of %d bytes" % (
                                 need, B, S, nh, nrows, "on" if is_deterministic() else "off", dq32_ws.dtype,
                                 dq32_ws.numel() * dq32_ws.element_size()))
    if seq is not None:
        assert mask is None and seq.B == B and seq.S == S
        with _timed("attention_bwd_d64", 10.0 * B * nh * S * S * 64, 2.0 * nrows * 9 * H):
            rc = _lib.load().vt_attention_bwd_seq_bf16(
                _ptr(qkv), qkv.stride(0), _ptr(dctx), dctx.stride(0), _ptr(ctx), ctx.stride(0), _ptr(lse), _ptr(delta_ws),
                _ptr(out), out.stride(0), _ptr(dq32_ws), B, S, nh, 64, float(drop[0]), int(drop[1]), int(drop[2]),
                _ptr(seq.start), _ptr(seq.length), seq.rows, _ptr(keep_bits), _stream())
        _lib.check(rc, "vt_attention_bwd_seq_bf16")
        return out
    with _timed("attention_bwd_d64", 10.0 * B * nh * S * S * 64, 2.0 * B * S * 9 * H):
        rc = _lib.load().vt_attention_bwd_bf16(
            _ptr(qkv), qkv.stride(0), _ptr(dctx), dctx.stride(0), _ptr(ctx), ctx.stride(0), _ptr(mask),
            _mask_mode(mask, mask_additive, B, S), _ptr(lse), _ptr(delta_ws), _ptr(out), out.stride(0), _ptr(dq32_ws), B, S, nh, 64,
            float(drop[0]), int(drop[1]), int(drop[2]), _ptr(keep_bits), _stream())
    _lib.check(rc, "vt_attention_bwd_bf16")
    return out


def layernorm_bwd(x, dy, gamma, eps, dgamma, dbeta, dx=None, ws=None, accumulate=False, M=None, dx_dropped=None,
                  drop=NO_DROP):
    """dx (bf16) and dgamma/dbeta (fp32, in place) of BertLayerNorm; x = pre-LayerNorm input.
    dx_dropped (optional bf16 [M,H]) receives dx * dropout mask / (1-p) of site `drop`.
    dgamma = dbeta = None (a frozen LayerNorm): dx only -- the same dx bit for bit, no partial sums, no reduce launch, ws not
    touched (profiled as "layernorm_bwd_dx")."""
    _require_hip(x, dy, gamma, dgamma, dbeta, dx)
    if (dgamma is None) != (dbeta is None):
        raise ValueError("layernorm_bwd takes dgamma and dbeta together, or neither")
    H = gamma.numel()
    if M is None:
        M = x.shape[0]
    if dx is None:
        dx = torch.empty((M, H), dtype=BF16, device=x.device)
    if ws is None and dgamma is not None:
        ws = torch.empty(LN_BWD_WS_ROWS * 2 * H, dtype=torch.float32, device=x.device)
    fn = "vt_layernorm_bwd_h_bf16" if x.dtype == F16 else "vt_layernorm_bwd_bf16"   # x: the pre-LayerNorm sums, bf16 or fp16
    with _timed("layernorm_bwd_rows" if dgamma is not None else "layernorm_bwd_dx", 0.0, 6.0 * M * H):
        rc = getattr(_lib.load(), fn)(
            _ptr(x), x.stride(0), _ptr(dy), dy.stride(0), _ptr(gamma), _ptr(dx), dx.stride(0), _ptr(dgamma),
            _ptr(dbeta), _ptr(ws), M, H, float(eps), 1 if accumulate else 0, _ptr(dx_dropped),
            0 if dx_dropped is None else dx_dropped.stride(0), float(drop[0]), int(drop[1]), int(drop[2]), _stream())
    _lib.check(rc, fn)
    return dx


def embed_layernorm_bwd(ids, type_ids, pos_ids, word, pos, typ, gamma, eps, g, S, dgamma, dbeta, ws=None,
                        accumulate=False, drop=NO_DROP):
    """-> de fp32 [B*T, H]: gradient w.r.t. the summed embedding of every text token."""
    _require_hip(ids, word, g)
    B, T = ids.shape
    H = word.shape[1]
    de = torch.empty((B * T, H), dtype=torch.float32, device=g.device)
    if ws is None:
        ws = torch.empty(LN_BWD_WS_ROWS * 2 * H, dtype=torch.float32, device=g.device)
    rc = _lib.load().vt_embed_layernorm_bwd(
        _ptr(ids), _ptr(type_ids), _ptr(pos_ids), _ptr(word), _ptr(pos), _ptr(typ), _ptr(gamma), _ptr(g), g.stride(0),
        _ptr(de), _ptr(dgamma), _ptr(dbeta), _ptr(ws), B, T, S, H, word.shape[0], pos.shape[0], typ.shape[0],
        float(eps), 1 if accumulate else 0, float(drop[0]), int(drop[1]), _stream())
    _lib.check(rc, "vt_embed_layernorm_bwd")
    return de


_readback = {}   # per device: [side stream, pinned int64[8, 8] ring, next slot] of the step's one read-back


def batch_row_counts_begin(labels, token_labels, mask, err_flag, B, S):
    """Launch the step's counting kernel (and the one-thread kernel that reads and clears the two bounded-wait counters,
    vt_step_counters) and start copying the seven numbers to pinned host memory on a SIDE stream behind an event -- the
    caller's stream goes on with work that does not need them (the step's weight transposes) while the host waits in
    batch_row_counts_end.  Returns a handle for it."""
    _require_hip(labels, token_labels, mask, err_flag)
    ref = next(t for t in (labels, token_labels, mask, err_flag) if t is not None)
    for t in (labels, token_labels):
        assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.numel() == B * S)
    assert mask is None or (mask.dtype == torch.float32 and mask.is_contiguous() and mask.numel() == B * S)
    dev = ref.device
    out = torch.zeros(8, dtype=torch.int64, device=dev)
    tiles = torch.empty(3 * ((B * S + 1023) // 1024), dtype=torch.int32, device=dev)
    lib = _lib.load()
    rc = lib.vt_batch_row_counts(_ptr(labels), _ptr(token_labels), _ptr(mask), _ptr(err_flag), B, S, _ptr(out), _ptr(tiles),
                                 _stream())
    _lib.check(rc, "vt_batch_row_counts")
    _lib.check(lib.vt_step_counters(out.data_ptr() + 5 * 8, _stream()), "vt_step_counters")
    rb = _readback.get(dev.index)
    if rb is None:   # a side stream and a ring of eight pinned slots (read-backs begun before an earlier one was collected)
        rb = _readback[dev.index] = [torch.cuda.Stream(device=dev), torch.zeros((8, 8), dtype=torch.int64).pin_memory(), 0]
    side, host = rb[0], rb[1][rb[2] & 7]
    rb[2] += 1
    ready = torch.cuda.Event()
    ready.record()
    side.wait_event(ready)
    with torch.cuda.stream(side):
        host.copy_(out, non_blocking=True)
        done = torch.cuda.Event()
        done.record(side)
    out.record_stream(side)
    return done, host, tiles


def batch_row_counts_end(handle):
    """-> ([err, #labels != -1, #token_labels != -1, #mask != 0, bad, wgrad waits that ran out, shared-tile waits that ran
    out] as Python ints, per-tile counts for batch_row_lists): the one host synchronisation of a training step."""
    done, host, tiles = handle
    done.synchronize()
    return host[:7].tolist(), tiles


def batch_row_counts(labels, token_labels, mask, err_flag, B, S):
    """batch_row_counts_begin + batch_row_counts_end (labels / token_labels int64 [B*S] or None, mask fp32 [B,S] or None,
    err_flag int32 [1] or None)."""
    return batch_row_counts_end(batch_row_counts_begin(labels, token_labels, mask, err_flag, B, S))


def batch_row_lists(labels, token_labels, mask, B, S, n_w, n_t, n_keep, tiles):
    """The row lists to the counts batch_row_counts reported (tiles: its second return value, same labels / mask):
    (idx_w, idx_t, layout) -- idx_* int64 or None, layout a SeqLayout over the positions with a non-zero mask or None."""
    _require_hip(labels, token_labels, mask)
    ref = next(t for t in (labels, token_labels, mask) if t is not None)
    i64 = lambda n: torch.empty(int(n), dtype=torch.int64, device=ref.device)
    idx_w = i64(n_w) if labels is not None else None
    idx_t = i64(n_t) if token_labels is not None else None
    index = inverse = start = length = None
    if mask is not None:
        index, inverse = i64(n_keep), i64(B * S)
        start = torch.empty(B, dtype=torch.int32, device=ref.device)
        length = torch.empty(B, dtype=torch.int32, device=ref.device)
    rc = _lib.load().vt_batch_row_lists(_ptr(labels), _ptr(token_labels), _ptr(mask), B, S, int(n_w), int(n_t), int(n_keep),
                                        _ptr(tiles), _ptr(idx_w), _ptr(idx_t), _ptr(index), _ptr(inverse), _ptr(start),
                                        _ptr(length), _stream())
    _lib.check(rc, "vt_batch_row_lists")
    lay = SeqLayout.from_parts(B, S, n_keep, index, inverse, start, length) if mask is not None else None
    return idx_w, idx_t, lay


def action_head(logits, next_action, A, grad_scale, Ap, dz=None):
    """logits fp32 [B, >= A], next_action int64 [B] -> (loss 0-d, accuracy 0-d, dlogits bf16 [B, Ap]): the action head's
    double log-softmax cross entropy with its gradient (encoder.py:142-151, 387-391) in one launch.  dz: the gradient's
    destination, bf16 [B, Ap] with any row stride (a view of a wider buffer); a fresh tensor otherwise."""
    _require_hip(logits, next_action, dz)
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and next_action.dtype == torch.int64
    B = logits.shape[0]
    dl = torch.empty((B, Ap), dtype=BF16, device=logits.device) if dz is None else dz
    assert dl.dtype == BF16 and tuple(dl.shape) == (B, Ap) and (dl.stride(1) == 1 or Ap == 1)
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    rc = _lib.load().vt_action_head_f32(_ptr(logits), logits.stride(0), _ptr(next_action.contiguous()), B, int(A),
                                        float(grad_scale), _ptr(dl), dl.stride(0), int(Ap), _ptr(out), _stream())
    _lib.check(rc, "vt_action_head_f32")
    return out[0], out[1], dl


def linear_splitk(a, w, ksplit, out=None):
    """a [M,K] bf16, w [N,K] bf16 -> a w^T [M,N] bf16 with the reduction split over `ksplit` copies of the 256x256 tile list
    (fp32 partial planes, then a sum): for a long K and so few output tiles that one copy leaves most CUs idle."""
    _require_hip(a, w, out)
    assert a.dtype == BF16 and w.dtype == BF16 and a.stride(1) == 1 and w.stride(1) == 1 and a.shape[1] == w.shape[1]
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a.device)
    ws = torch.empty(int(ksplit) * M * N, dtype=torch.float32, device=a.device)
    with _timed("gemm_nt_bf16", 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N)):
        rc = _lib.load().vt_linear_splitk_bf16(_ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(out), out.stride(0), _ptr(ws), M, N,
                                               K, int(ksplit), _stream())
    _lib.check(rc, "vt_linear_splitk_bf16")
    return out


def splitk_for(M, N, K, cus=256):
    """How many K-ranges to give the 256x256 tile list of an [M, N] output so that it covers the chip about once (0: none --
    enough tiles already, or a short K)."""
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    if tiles * 2 > cus or K < 64 * 32 or not switches.on("VT_SPLITK"):
        return 0
    return max(2, min(cus // tiles, K // (64 * 8)))


def embed_table_grad(ids, de, grad, skip_id=None):
    """grad[ids[i], :] += de[i, :] for every row i (ids int64 [n], de fp32 [n, H], grad fp32 [rows, H]) without atomics: a
    stable sort of the ids, then one workgroup per run of equal ids (bitwise reproducible; rows with id == skip_id add
    nothing -- nn.Embedding's padding_idx)."""
    _require_hip(ids, de, grad)
    assert ids.dtype == torch.int64 and de.dtype == torch.float32 and grad.dtype == torch.float32
    assert de.stride(1) == 1 and grad.stride(1) == 1 and ids.numel() == de.shape[0] and de.shape[1] == grad.shape[1]
    sorted_ids, perm = torch.sort(ids.reshape(-1).to(torch.int32), stable=True)   # (table rows < 2^31)
    # partial sums of the runs that span several 32-row segments (rows of such segments only are touched), and one flag
    scratch = torch.empty((ids.numel(), de.shape[1]), dtype=torch.float32, device=de.device)
    flag = torch.empty(1, dtype=torch.int32, device=de.device)
    rc = _lib.load().vt_embed_table_grad(_ptr(sorted_ids), _ptr(perm), _ptr(de), de.stride(0), _ptr(grad), grad.stride(0),
                                         ids.numel(), de.shape[1], grad.shape[0], -1 if skip_id is None else int(skip_id),
                                         _ptr(scratch), _ptr(flag), _stream())
    _lib.check(rc, "vt_embed_table_grad")
    return grad


def adamw_flat(p, g, m, v, p_bf16, lr, step_size, b1, b2, eps, wd, grad_scale=1.0):
    """In-place AdamW (pytorch-transformers rule) over flat fp32 slabs; refreshes the bf16 mirror.  g: fp32, or bf16 (the
    all-reduced communication copy of the gradient slab)."""
    _require_hip(p, g, m, v, p_bf16)
    n = p.numel()
    g16 = g.dtype == BF16
    fn = _lib.load().vt_adamw_flat_g16 if g16 else _lib.load().vt_adamw_flat
    with _timed("adamw_flat", 0.0, n * ((26.0 if g16 else 28.0) + (2.0 if p_bf16 is not None else 0.0))):
        rc = fn(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p_bf16), n, float(lr), float(step_size), float(b1), float(b2),
                float(eps), float(wd), float(grad_scale), _stream())
    _lib.check(rc, "vt_adamw_flat")


# ---- AdamW sharded over data-parallel ranks (visitron_amd/distributed.py: ShardPlan) ---------------------------------
SHARD_CHUNK = 2048   # elements per table chunk: two 16-byte rounds of a workgroup; long segments and short ones then balance


class ShardTable(object):
    """A chunk table of vt_shard_adamw (7 words) or vt_shard_settle (4 words) on the device, with the host copy the entry
    point checks.  rows: int64 [n, words - 2 | words - 1] of (addresses ..., elements[, flag]) per SEGMENT; segments are cut
    here into chunks of at most `chunk` elements (a multiple of 4, so a chunk is as aligned as its segment)."""

    def __init__(self, segments, elem_sizes, device, chunk=SHARD_CHUNK):
        import numpy as np

        na = len(elem_sizes)
        seg = np.asarray(segments, dtype=np.int64).reshape(-1, na + 2)
        assert chunk > 0 and chunk % 4 == 0
        counts = (seg[:, na] + chunk - 1) // chunk
        which = np.repeat(np.arange(seg.shape[0]), counts)                     # chunk -> its segment
        first = np.cumsum(counts) - counts
        k = np.arange(which.shape[0]) - first[which]                           # chunk -> its index inside the segment
        tab = np.empty((which.shape[0], na + 2), dtype=np.int64)
        for a, size in enumerate(elem_sizes):
            tab[:, a] = seg[which, a] + k * chunk * size
        tab[:, na] = np.minimum(seg[which, na] - k * chunk, chunk)
        tab[:, na + 1] = seg[which, na + 1]
        self.host = torch.from_numpy(np.ascontiguousarray(tab))
        self.dev = self.host.to(device)
        self.n_chunks = int(tab.shape[0])
        self.numel = int(seg[:, na].sum())


def shard_adamw_table(p, g, m, v, mirror, segments, chunk=SHARD_CHUNK):
    """segments: (slab start, slab end, decay, moment offset): p, g, mirror are addressed at the slab position, m and v (the
    rank's shard-sized moment storage) at the moment offset."""
    _require_hip(p, g, m, v, mirror)
    assert p.dtype == m.dtype == v.dtype == torch.float32 and mirror.dtype == BF16 and g.dtype in (torch.float32, BF16)
    gs = g.element_size()
    rows = [(p.data_ptr() + 4 * s, g.data_ptr() + gs * s, m.data_ptr() + 4 * mo, v.data_ptr() + 4 * mo,
             mirror.data_ptr() + 2 * s, e - s, int(bool(dec))) for s, e, dec, mo in segments]
    for s, e, _, mo in segments:
        assert 0 <= s < e <= p.numel() and e <= g.numel() and e <= mirror.numel() and 0 <= mo and mo + e - s <= m.numel() == v.numel()
    return ShardTable(rows, (4, gs, 4, 4, 2), p.device, chunk)


def shard_settle_table(p, mirror, segments, chunk=SHARD_CHUNK):
    """segments: (slab start, slab end, direction) -- 0: p = float(mirror), 1: mirror = bf16(p)."""
    _require_hip(p, mirror)
    assert p.dtype == torch.float32 and mirror.dtype == BF16
    for s, e, _ in segments:
        assert 0 <= s < e <= p.numel() and e <= mirror.numel()
    rows = [(p.data_ptr() + 4 * s, mirror.data_ptr() + 2 * s, e - s, int(d)) for s, e, d in segments]
    return ShardTable(rows, (4, 2), p.device, chunk)


def shard_adamw(table, g_is_bf16, lr, step_size, b1, b2, eps, wd, grad_scale=1.0):
    """adamw_flat's update on the chunks of a ShardTable (this rank's segments of the slabs), one launch."""
    with _timed("shard_adamw", 0.0, table.numel * (28.0 if g_is_bf16 else 30.0)):
        rc = _lib.load().vt_shard_adamw(_ptr(table.dev), _ptr(table.host), table.n_chunks, int(bool(g_is_bf16)), float(lr),
                                        float(step_size), float(b1), float(b2), float(eps), float(wd), float(grad_scale),
                                        _stream())
    _lib.check(rc, "vt_shard_adamw")


def shard_settle(table):
    """The segments a rank does not own, after the gather: p = float(mirror) or mirror = bf16(p) per chunk, one launch."""
    with _timed("shard_settle", 0.0, table.numel * 6.0):
        rc = _lib.load().vt_shard_settle(_ptr(table.dev), _ptr(table.host), table.n_chunks, _stream())
    _lib.check(rc, "vt_shard_settle")


# ---- multi-tensor optimizer step, gradient norm and clip (visitron_amd/optim.py builds the tables) -------------------
def multi_adam(table, n_chunks, hyper, grad_coef=1.0, grad_coef_dev=None, numel=0):
    """One launch of the Adam / AdamW rule over a chunk table (int64 [n_chunks, 6] on the device: addresses of p, g, m, v,
    element count, hyper slot).  hyper: fp32 [slots, 8] on the device.  The gradients are multiplied by the device float
    `grad_coef_dev` where given, else by `grad_coef`.  numel: the elements the table covers (profiling only)."""
    _require_hip(table, hyper, grad_coef_dev)
    with _timed("multi_adam", 0.0, 28.0 * numel):
        rc = _lib.load().vt_multi_adam(_ptr(table), int(n_chunks), _ptr(hyper), float(grad_coef), _ptr(grad_coef_dev), _stream())
    _lib.check(rc, "vt_multi_adam")


def multi_sumsq(table, n_chunks, partials, numel=0):
    """partials[c] (fp64 [n_chunks]) = sum of g^2 over chunk c of the table."""
    _require_hip(table, partials)
    assert partials.dtype == torch.float64 and partials.numel() >= n_chunks
    with _timed("multi_sumsq", 0.0, 4.0 * numel):
        rc = _lib.load().vt_multi_sumsq(_ptr(table), int(n_chunks), _ptr(partials), _stream())
    _lib.check(rc, "vt_multi_sumsq")


def norm_finish(partials, n_chunks, max_norm, out):
    """out (fp32 [2]) = (total_norm, clip_coef) from the per-chunk sums: torch.nn.utils.clip_grad_norm_'s rule."""
    _require_hip(partials, out)
    assert out.dtype == torch.float32 and out.numel() >= 2
    with _timed("norm_finish", 0.0, 8.0 * n_chunks):
        rc = _lib.load().vt_norm_finish(_ptr(partials), int(n_chunks), float(max_norm), _ptr(out), _stream())
    _lib.check(rc, "vt_norm_finish")


def multi_scale(table, n_chunks, coef_dev, numel=0):
    """g *= coef_dev[0] over the table's gradients."""
    _require_hip(table, coef_dev)
    with _timed("multi_scale", 0.0, 8.0 * numel):
        rc = _lib.load().vt_multi_scale(_ptr(table), int(n_chunks), _ptr(coef_dev), _stream())
    _lib.check(rc, "vt_multi_scale")


def scale_heads(x, head_scale, out=None):
    """out[r, 64 h + d] = x[r, 64 h + d] * head_scale[h] (bf16 [rows, nh * 64]; head_scale fp32 [nh])."""
    _require_hip(x, head_scale, out)
    assert x.dtype == BF16 and x.stride(1) == 1 and head_scale.dtype == torch.float32 and head_scale.is_contiguous()
    nh = head_scale.numel()
    assert x.shape[1] == nh * 64
    if out is None:
        out = torch.empty_like(x)
    rc = _lib.load().vt_scale_heads_bf16(_ptr(x), x.stride(0), _ptr(out), out.stride(0), x.shape[0], nh, _ptr(head_scale),
                                         _stream())
    _lib.check(rc, "vt_scale_heads_bf16")
    return out


def cast_to_bf16(src, dst, scale=1.0):
    """dst (bf16, flat) = src (fp32, flat) * scale; element counts a multiple of 8."""
    _require_hip(src, dst)
    assert src.dtype == torch.float32 and dst.dtype == BF16 and src.numel() == dst.numel()
    rc = _lib.load().vt_cast_f32_to_bf16(_ptr(src), _ptr(dst), src.numel(), float(scale), _stream())
    _lib.check(rc, "vt_cast_f32_to_bf16")
    return dst


def ce_softmax_rows(z, y, V, dz, scale):
    """Fused CE over logits z fp32 [rows, >=V] with labels y: returns (loss_row fp32 [rows], argmax int64 [rows])
    and fills dz bf16 [rows, Vpad] with (softmax - onehot) * scale (dz None: loss and argmax only)."""
    _require_hip(z, y, dz)
    rows = z.shape[0]
    loss = torch.empty(rows, dtype=torch.float32, device=z.device)
    amax = torch.empty(rows, dtype=torch.int64, device=z.device)
    vpad, lddz = (round_up(V, 8), round_up(V, 8)) if dz is None else (dz.shape[1], dz.stride(0))
    with _timed("ce_softmax_rows", 0.0, rows * ((8.0 if dz is not None else 4.0) * V + (2.0 * vpad if dz is not None else 0.0))):
        rc = _lib.load().vt_ce_softmax_rows(_ptr(z), z.stride(0), _ptr(y), _ptr(loss), _ptr(amax), _ptr(dz), lddz,
                                            rows, V, vpad, float(scale), _stream())
    _lib.check(rc, "vt_ce_softmax_rows")
    return loss, amax


def ce_double_softmax_rows(z, y, V, dz, scale):
    """The token head's loss (Linear + Softmax, then CrossEntropy = a second log-softmax): returns (loss_row, argmax)
    and fills dz bf16 [rows, Vpad] with d(scale * loss_row)/dz (dz None: loss and argmax only)."""
    _require_hip(z, y, dz)
    rows = z.shape[0]
    loss = torch.empty(rows, dtype=torch.float32, device=z.device)
    amax = torch.empty(rows, dtype=torch.int64, device=z.device)
    vpad, lddz = (round_up(V, 8), round_up(V, 8)) if dz is None else (dz.shape[1], dz.stride(0))
    with _timed("ce_softmax_rows", 0.0, rows * (4.0 * V + (2.0 * vpad if dz is not None else 0.0))):
        rc = _lib.load().vt_ce_double_softmax_rows(_ptr(z), z.stride(0), _ptr(y), _ptr(loss), _ptr(amax), _ptr(dz),
                                                   lddz, rows, V, vpad, float(scale), _stream())
    _lib.check(rc, "vt_ce_double_softmax_rows")
    return loss, amax


def set_attn_bwd_waves(waves):
    """Tuning/test hook: 17 (default; any other value restores it) = the persistent, software-pipelined 16-wave attention
    backward kernel where it serves (one key block, per-key masks, dropout through the forward's keep words) and the 8-wave
    kernel elsewhere; 16 = the 16-wave kernel with one (batch, head) per workgroup; 8 = always the 8-wave kernel (forms
    delta = rowsum(dO o O) itself), 10 = the same behind a separate delta pass, 4 = the 4-wave kernel."""
    _lib.load().vt_debug_set_attn_bwd_waves(int(waves))


def apply_dropout(x, drop):
    """x *= mask / (1-p) in place (bf16 [rows, cols], element index row * cols + col)."""
    _require_hip(x)
    assert x.dtype == BF16 and x.stride(1) == 1
    rc = _lib.load().vt_apply_dropout_bf16(_ptr(x), x.stride(0), x.shape[0], x.shape[1], float(drop[0]), int(drop[1]),
                                           int(drop[2]), _stream())
    _lib.check(rc, "vt_apply_dropout_bf16")
    return x


def dropout_mask(n, drop, head_index=-1, device="cuda"):
    """uint8 [n]: 1 where element i of the site is kept (test hook: feed the oracle the same masks)."""
    out = torch.empty(n, dtype=torch.uint8, device=device)
    rc = _lib.load().vt_debug_dropout_mask(_ptr(out), n, float(drop[0]), int(drop[1]), int(drop[2]), int(head_index),
                                           _stream())
    _lib.check(rc, "vt_debug_dropout_mask")
    return out


def attn_dropout_mask(n, drop, head_index, device="cuda"):
    """uint8 [n, n]: the keep mask of the attention-probability dropout of one (batch, head) whose sequence has n rows
    (test hook).  The attention kernels index element (query q, key k) as q * n' + k with n' = n rounded up to a multiple of 4
    (csrc/common.hpp, vt_keep_attn: the keys 4m .. 4m + 3 of a query share a hash word, a byte each against an 8-bit
    threshold -- the drop probability runs quantised to 1/256, attn_drop_p)."""
    pitch = (n + 3) & ~3
    return dropout_mask(n * pitch, drop, head_index=head_index, device=device).view(n, pitch)[:, :n]


def attn_drop_p(p):
    """The attention-probability dropout's effective probability under the current setting (set_attn_dropout_bits): by
    default p resolved to 1/65536 (0.1 -> 0.100006), with 8-bit fields to 1/256 (0.1 -> 26/256 = 0.1016); kept
    probabilities are scaled by 1 / (1 - attn_drop_p(p)).  A p below half a step runs as one step (never silently as no
    dropout); a p that rounds to 1 is refused (the library returns VT_ERR_UNSUPPORTED: the scale would be infinite)."""
    if not p > 0:
        return 0.0
    n = float(1 << attn_dropout_bits())
    if p * n + 0.5 >= n:
        raise ValueError("attention_probs_dropout_prob %r is not served: the attention sites quantise p to n/%d, n <= %d"
                         % (p, int(n), int(n) - 1))
    return float(min(int(n) - 1, max(1, int(p * n + 0.5)))) / n


def set_weight_prefetch(training=-1, inference=-1):
    """The layer loops' weight prefetch (include/visitron_hip.h, vt_set_weight_prefetch): training 0 off or 4 riding in the
    LayerNorm kernels (default), inference 0 off or 3 riding in the attention kernel (default); -1 keeps a setting.  Any other
    number is refused (RuntimeError) and changes nothing."""
    _lib.check(_lib.load().vt_set_weight_prefetch(int(training), int(inference)), "vt_set_weight_prefetch")


def weight_prefetch():
    """(training mode, inference mode) in force: 0 / 4 and 0 / 3, or the number VT_PREFETCH_WEIGHTS / VT_PREFETCH_INFER named
    (one that is not a mode runs as off)."""
    lib = _lib.load()
    return int(lib.vt_get_weight_prefetch(0)), int(lib.vt_get_weight_prefetch(1))


def attn_dropout_bits():
    """16 (default: exact p) or 8 (rounds 4-5's faster form): the width of the attention-probability dropout's hash fields."""
    try:
        return int(_lib.load().vt_get_attn_dropout_bits())
    except Exception:   # noqa: BLE001 -- no HIP library on this host: the product path refuses elsewhere, loudly
        return 8 if switches.text("VT_ATTN_DROPOUT_BITS") == "8" else 16


def set_attn_dropout_bits(bits):
    """Process-wide: 16 (default) = exact-p attention dropout (the reference's nn.Dropout(0.1) runs as 0.100006), 8 = p in
    steps of 1/256 (0.1 runs as 0.1016; half the hash words in the attention forward: that kernel ~5 % faster, the B = 256
    step 0.15 %).  Set it before building an engine / model: forward
    and backward of a step must see the same setting (include/visitron_hip.h, vt_set_attn_dropout_bits)."""
    _lib.check(_lib.load().vt_set_attn_dropout_bits(int(bits)), "vt_set_attn_dropout_bits")


def transpose(src, out):
    """out[c, r] = src[r, c] (bf16 2-D, row strides allowed)."""
    _require_hip(src, out)
    assert src.dtype == BF16 and out.dtype == BF16 and src.stride(1) == 1 and out.stride(1) == 1
    R, C = src.shape
    rc = _lib.load().vt_transpose_bf16(_ptr(src), src.stride(0), _ptr(out), out.stride(0), R, C, _stream())
    _lib.check(rc, "vt_transpose_bf16")
    return out


class TransposeBatch(object):
    """A fixed list of (src, out) bf16 matrix pairs transposed by ONE launch (vt_transpose_batch_bf16): the argument
    arrays are built once, `run()` re-issues the launch (the tensors must keep their storage)."""

    def __init__(self, pairs):
        n = len(pairs)
        self.n, self._keep = n, list(pairs)
        self.src, self.dst = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
        self.ldi, self.ldo = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
        self.R, self.C = (ctypes.c_int * n)(), (ctypes.c_int * n)()
        for i, (s_, o_) in enumerate(pairs):
            _require_hip(s_, o_)
            assert s_.dtype == BF16 and o_.dtype == BF16 and s_.stride(1) == 1 and o_.stride(1) == 1
            assert o_.shape[0] == s_.shape[1] and o_.shape[1] >= s_.shape[0]   # wider: zero-padded column tail
            self.src[i], self.dst[i] = s_.data_ptr(), o_.data_ptr()
            self.ldi[i], self.ldo[i] = s_.stride(0), o_.stride(0)
            self.R[i], self.C[i] = s_.shape

    def run(self):
        rc = _lib.load().vt_transpose_batch_bf16(self.src, self.ldi, self.dst, self.ldo, self.R, self.C, self.n, _stream())
        _lib.check(rc, "vt_transpose_batch_bf16")


def dgelu_mul(g, h, out=None):
    """g * d (d = saved gelu' values), bf16 contiguous."""
    _require_hip(g, h, out)
    assert g.dtype == BF16 and h.dtype == BF16 and g.is_contiguous() and h.is_contiguous()
    if out is None:
        out = torch.empty_like(g)
    rc = _lib.load().vt_dgelu_mul_bf16(_ptr(g), _ptr(h), _ptr(out), g.numel(), _stream())
    _lib.check(rc, "vt_dgelu_mul_bf16")
    return out


def encoder_backward(layer_weights, layer_weights_t, layer_acts, layer_grads, x, mask, mask_additive, g, ws,
                     B, S, H, nh, I, eps, accumulate=False, p_hidden=0.0, p_attn=0.0, drop_seed=0, layer0=0,
                     ws_b=None, side_stream=None, seq=None, need_input_grad=True):
    """Reverse layer loop in C; g [B*S,H] bf16 is updated in place to dL/dx.  With a second workspace set and a side
    stream (torch.cuda.Stream) the weight gradients of a layer run beside the next layer's dgrad chain.
    A layer_grads row of null pointers is a frozen layer (no weight gradient, LayerNorm backward dx-only).
    need_input_grad=False: nobody reads dL/dx -- the first layer's last dgrad GEMM is not launched and g is left undefined."""
    _require_hip(x, mask, g)
    if not need_input_grad:
        assert seq is None or mask is None
        rc = _lib.load().vt_encoder_backward_partial_bf16(
            layer_weights, layer_weights_t, layer_acts, layer_grads, len(layer_weights), _ptr(x), _ptr(mask),
            _mask_mode(mask, mask_additive, B, S), _ptr(g), ctypes.byref(ws), None if ws_b is None else ctypes.byref(ws_b),
            B, S, H, nh, I, float(eps), 1 if accumulate else 0, float(p_hidden), float(p_attn), int(drop_seed), int(layer0),
            0 if seq is None else seq.rows, None if seq is None else _ptr(seq.start), None if seq is None else _ptr(seq.length),
            0, _stream(), None if side_stream is None else ctypes.c_void_p(side_stream.cuda_stream))
        _lib.check(rc, "vt_encoder_backward_partial_bf16")
        return
    if seq is not None:
        assert mask is None
        rc = _lib.load().vt_encoder_backward_seq_bf16(
            layer_weights, layer_weights_t, layer_acts, layer_grads, len(layer_weights), _ptr(x), _ptr(g),
            ctypes.byref(ws), None if ws_b is None else ctypes.byref(ws_b), B, S, H, nh, I, float(eps),
            1 if accumulate else 0, float(p_hidden), float(p_attn), int(drop_seed), int(layer0), seq.rows,
            _ptr(seq.start), _ptr(seq.length), _stream(),
            None if side_stream is None else ctypes.c_void_p(side_stream.cuda_stream))
        _lib.check(rc, "vt_encoder_backward_seq_bf16")
        return
    if ws_b is not None and side_stream is not None:
        rc = _lib.load().vt_encoder_backward_overlap_bf16(
            layer_weights, layer_weights_t, layer_acts, layer_grads, len(layer_weights), _ptr(x), _ptr(mask),
            _mask_mode(mask, mask_additive, B, S), _ptr(g), ctypes.byref(ws), ctypes.byref(ws_b), B, S, H, nh, I, float(eps),
            1 if accumulate else 0, float(p_hidden), float(p_attn), int(drop_seed), int(layer0), _stream(),
            ctypes.c_void_p(side_stream.cuda_stream))
        _lib.check(rc, "vt_encoder_backward_overlap_bf16")
        return
    rc = _lib.load().vt_encoder_backward_bf16(
        layer_weights, layer_weights_t, layer_acts, layer_grads, len(layer_weights), _ptr(x), _ptr(mask),
        _mask_mode(mask, mask_additive, B, S), _ptr(g), ctypes.byref(ws), B, S, H, nh, I, float(eps), 1 if accumulate else 0,
        float(p_hidden), float(p_attn), int(drop_seed), int(layer0), _stream())
    _lib.check(rc, "vt_encoder_backward_bf16")


def set_wgrad_kernel(mode):
    """Tuning/test hook: 0 automatic (persistent kernel from 12 288 rows), 128 / 256 the one-tile-per-workgroup kernel, -8 never /
    8 always (where eligible) the persistent kernel."""
    _lib.load().vt_debug_set_wgrad_kernel(int(mode))


def wgrad(problems, M):
    """Grouped weight gradients.  problems: list of dicts(dy, x, dw, db=None, accumulate=False) with
    dy [M,N] bf16, x [M,K] bf16, dw [N,K] fp32, db [N] fp32; one launch for up to 8 problems."""
    arr = (_lib.WgradProblem * len(problems))()
    flops = 0.0
    for i, p in enumerate(problems):
        dy, x, dw, db = p["dy"], p["x"], p["dw"], p.get("db")
        _require_hip(dy, x, dw, db)
        assert dy.dtype == BF16 and x.dtype == BF16 and dw.dtype == torch.float32
        N, K = dw.shape
        arr[i].dY, arr[i].ldy = dy.data_ptr(), dy.stride(0)
        arr[i].X, arr[i].ldx = x.data_ptr(), x.stride(0)
        arr[i].dW, arr[i].ldw = dw.data_ptr(), dw.stride(0)
        arr[i].db = None if db is None else db.data_ptr()
        arr[i].N, arr[i].K = N, K
        arr[i].accumulate = 1 if p.get("accumulate") else 0
        flops += 2.0 * M * N * K
    with _timed("gemm_wgrad_tn_bf16", flops, 0.0):
        rc = _lib.load().vt_wgrad_bf16(arr, len(problems), M, _stream())
    _lib.check(rc, "vt_wgrad_bf16")


_gemm_ws = {}


def ensure_gemm_workspace(device=None):
    """Register the shared-tile workspace of the persistent GEMM (vt_gemm_set_workspace) on `device`, once: VT_GEMM_WS_REGIONS
    regions (default 2; 0: none -- SHARED_TILE_VARIANTS are then refused and the autotuner leaves them out) of 64 MiB + 4 KiB
    (vt_gemm_workspace_region_bytes), zeroed, owned by this module for the life of the process."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev.index in _gemm_ws:
        return _gemm_ws[dev.index] is not None
    regions = switches.integer("VT_GEMM_WS_REGIONS")
    lib = _lib.load()
    if regions <= 0:
        _gemm_ws[dev.index] = None
        return False
    n = int(lib.vt_gemm_workspace_region_bytes()) * regions
    with torch.cuda.device(dev):
        ws = torch.zeros(n + 256, dtype=torch.uint8, device=dev)
        base = (ws.data_ptr() + 255) // 256 * 256
        torch.cuda.synchronize(dev)
        _lib.check(lib.vt_gemm_set_workspace(ctypes.c_void_p(base), n), "vt_gemm_set_workspace")
    _gemm_ws[dev.index] = ws
    return True


def gemm_shared_tile_timeouts():
    """Finishing workgroups of shared GEMM tiles that ran out of their bounded wait since the last call (0 in a healthy run).
    Blocking read-back: call it where the host synchronises anyway."""
    if not any(v is not None for v in _gemm_ws.values()):
        return 0
    n = ctypes.c_uint(0)
    _lib.check(_lib.load().vt_gemm_shared_tile_timeouts(ctypes.byref(n)), "vt_gemm_shared_tile_timeouts")
    return int(n.value)


def wgrad_turn_timeouts():
    """Workgroups of the persistent weight-gradient kernel that ran out of their bounded wait for a dW tile since the last
    call (0 in a healthy run).  Blocking 4-byte read-back: call it where the host synchronises anyway."""
    n = ctypes.c_uint(0)
    _lib.check(_lib.load().vt_wgrad_turn_timeouts(ctypes.byref(n)), "vt_wgrad_turn_timeouts")
    return int(n.value)


def encoder_forward(layer_weights, layer_acts, x, mask, mask_additive, head_scale, B, S, H, nh, I, eps,
                    p_hidden=0.0, p_attn=0.0, drop_seed=0, seq=None):
    """Run the layer loop in C.  layer_weights / layer_acts: ctypes arrays built by the caller
    (``visitron_amd.modeling`` keeps them alive together with the tensors they point into).  seq (SeqLayout): x and
    the activations hold the compacted rows, no mask."""
    _require_hip(x, mask, head_scale)
    L = len(layer_weights)
    if seq is not None:
        assert mask is None and seq.B == B and seq.S == S
        rc = _lib.load().vt_encoder_forward_seq_bf16(
            layer_weights, layer_acts, L, _ptr(x), _ptr(head_scale), B, S, H, nh, I, float(eps), float(p_hidden),
            float(p_attn), int(drop_seed), seq.rows, _ptr(seq.start), _ptr(seq.length), _stream())
        _lib.check(rc, "vt_encoder_forward_seq_bf16")
        return
    rc = _lib.load().vt_encoder_forward_bf16(
        layer_weights, layer_acts, L, _ptr(x), _ptr(mask), _mask_mode(mask, mask_additive, B, S), _ptr(head_scale),
        B, S, H, nh, I, float(eps), float(p_hidden), float(p_attn), int(drop_seed), _stream())
    _lib.check(rc, "vt_encoder_forward_bf16")


# ---- rollout caller (tasks/viewpoint_select/agent_models.py) ---------------------------------------------------
def lstm_step(xproj, h_prev, h_out, c, w_hh, t=0, lengths=None, seq_out=None):
    """One nn.LSTM / nn.LSTMCell step: xproj fp32 [B, 4*hs] view (row stride free) = x @ W_ih.T + b_ih + b_hh;
    h_prev / h_out / c fp32 [B, hs] (c in place, h ping-pong); w_hh bf16 [4*hs, hs]; lengths int32 [B] gives the
    packed-sequence rule; seq_out fp32 [B, hs] view (row stride free) of the padded output at position t."""
    _require_hip(xproj, h_prev, h_out, c, w_hh, lengths, seq_out)
    B, hs = h_prev.shape
    assert xproj.dtype == torch.float32 and xproj.shape == (B, 4 * hs) and xproj.stride(1) == 1
    assert w_hh.dtype == BF16 and w_hh.shape == (4 * hs, hs) and w_hh.is_contiguous()
    for s in (h_prev, h_out, c):
        assert s.dtype == torch.float32 and s.shape == (B, hs) and s.is_contiguous()
    if lengths is not None:
        assert lengths.dtype == torch.int32 and lengths.shape == (B,) and lengths.is_contiguous()
    if seq_out is not None:
        assert seq_out.dtype == torch.float32 and seq_out.shape == (B, hs) and seq_out.stride(1) == 1
    with _timed("lstm_step", 2.0 * B * 4 * hs * hs, 2.0 * 4 * hs * hs + 4.0 * B * hs * 8):
        rc = _lib.load().vt_lstm_step_f32(
            _ptr(xproj), xproj.stride(0), _ptr(h_prev), _ptr(h_out), _ptr(c), _ptr(w_hh), _ptr(lengths), _ptr(seq_out),
            0 if seq_out is None else seq_out.stride(0), B, hs, int(t), _stream())
    _lib.check(rc, "vt_lstm_step_f32")
    return h_out


def softdot_attention(target, context, mask=None, want_weighted=True, want_attn=True, output_prob=True):
    """SoftDotAttention after linear_in: target fp32 [B,D], context fp32 [B,L,D] (last dim contiguous, any row and batch
    stride), mask bool/uint8 [B,L] (nonzero = masked) -> (weighted fp32 [B,D] | None, attn fp32 [B,L] | None).
    Any 1 <= D <= 4096: 16-byte loads where D and the strides are multiples of 4 on 16-byte aligned bases, 8-byte loads where
    D % 4 == 2 on even strides and 8-byte aligned bases (2058), element loads otherwise; nothing outside a row's D columns is
    read.  A masked key is never multiplied into the weighted sum; a row with every key masked is NaN."""
    _require_hip(target, context, mask)
    B, L, D = context.shape
    assert target.dtype == torch.float32 and target.shape == (B, D) and target.is_contiguous()
    assert context.dtype == torch.float32 and context.stride(2) == 1
    m8 = None
    if mask is not None:
        assert mask.shape == (B, L)
        m8 = (mask if mask.dtype == torch.uint8 else mask.to(torch.bool).view(torch.uint8)).contiguous()
    weighted = torch.empty((B, D), dtype=torch.float32, device=target.device) if want_weighted else None
    attn = torch.empty((B, L), dtype=torch.float32, device=target.device) if want_attn else None
    with _timed("softdot_attention", 4.0 * B * L * D, 4.0 * B * L * D):
        rc = _lib.load().vt_softdot_attention_f32(
            _ptr(target), _ptr(context), context.stride(0), context.stride(1), _ptr(m8), _ptr(weighted), _ptr(attn),
            B, L, D, 1 if output_prob else 0, _stream())
    _lib.check(rc, "vt_softdot_attention_f32")
    return weighted, attn


# The recurrence as ONE persistent launch (csrc/lstm_persistent.hip) where the shape allows (B <= 64, hs in 128 .. 1024):
# VT_LSTM_PERSISTENT=0 keeps the one-launch-per-position form.  Scratch (exchange buffers + sync words) per (B, hs, device).
LSTM_PERSISTENT = switches.on("VT_LSTM_PERSISTENT")
_lstm_ws = {}
_LSTM_FORCE_TIMEOUT = [False]   # test hook: treat every persistent launch as timed out (exercises the restore + fallback)


def _lstm_persistent(xproj, ldx_b, ldx_t, row_start, h, c, w_hh, lengths, seq_out, T, reverse):
    """-> True if the persistent kernel served the call (h, c, seq_out updated); False: the caller issues the step launches
    (shape outside the persistent form, or a workgroup ran out of its bounded wait -- h / c are then untouched)."""
    B, hs = c.shape
    if not LSTM_PERSISTENT or B > 64 or hs not in (128, 256, 512, 1024):
        return False
    if torch.cuda.is_current_stream_capturing():
        return False   # the time-out word is read back by the host: not inside a graph capture (the step launches are)
    lib = _lib.load()
    # scratch (exchange buffers, arrival counter, time-out word) per shape, device AND stream: two streams running the
    # recurrence side by side must not share a counter
    key = (B, hs, str(c.device), int(torch.cuda.current_stream().cuda_stream))
    ws = _lstm_ws.get(key)
    if ws is None:
        ws = torch.empty(int(lib.vt_lstm_sequence_persistent_ws_bytes(B, hs)), dtype=torch.uint8, device=c.device)
        _lstm_ws[key] = ws
    # a workgroup that runs out of its bounded wait leaves the state partly advanced (the others may have finished the
    # last step): the caller's h / c are restored from these copies before the step launches take over
    h_keep, c_keep = h.clone(), c.clone()
    with _timed("lstm_persistent", 2.0 * T * B * 4 * hs * hs, T * 4.0 * B * hs * 8):
        rc = lib.vt_lstm_sequence_persistent_f32(
            _ptr(xproj), ldx_b, ldx_t, _ptr(row_start), _ptr(h), _ptr(c), _ptr(w_hh), _ptr(lengths), _ptr(seq_out),
            0 if seq_out is None else seq_out.stride(0), 0 if seq_out is None else seq_out.stride(1), B, hs, int(T),
            1 if reverse else 0, _ptr(ws), ws.numel(), _stream())
    if rc == _lib.VT_ERR_UNSUPPORTED:
        return False
    _lib.check(rc, "vt_lstm_sequence_persistent_f32")
    # the timeout word (one 4-byte read-back; the recurrence's result is consumed right after anyway)
    if int(ws[4:8].view(torch.int32).item()) != 0 or _LSTM_FORCE_TIMEOUT[0]:
        h.copy_(h_keep)
        c.copy_(c_keep)
        return False
    return True


def lstm_sequence(xproj, h2, c, w_hh, T, lengths=None, seq_out=None, reverse=False):
    """One nn.LSTM direction over a padded batch: xproj fp32 [B,S,4*hs] (last dim contiguous), h2 = (h, scratch) two
    fp32 [B,hs] buffers (h: initial state in, final state out), c fp32 [B,hs] in place, seq_out fp32 [B,T,hs] view."""
    _require_hip(xproj, h2[0], h2[1], c, w_hh, lengths, seq_out)
    B, hs = c.shape
    assert xproj.dtype == torch.float32 and xproj.dim() == 3 and xproj.shape[0] == B and xproj.shape[2] == 4 * hs
    assert xproj.stride(2) == 1 and 0 < T <= xproj.shape[1]
    assert w_hh.dtype == BF16 and w_hh.shape == (4 * hs, hs) and w_hh.is_contiguous()
    for s in (h2[0], h2[1], c):
        assert s.dtype == torch.float32 and s.shape == (B, hs) and s.is_contiguous()
    if lengths is not None:
        assert lengths.dtype == torch.int32 and lengths.shape == (B,) and lengths.is_contiguous()
    if seq_out is not None:
        assert seq_out.dtype == torch.float32 and seq_out.shape == (B, T, hs) and seq_out.stride(2) == 1
    if _lstm_persistent(xproj, xproj.stride(0), xproj.stride(1), None, h2[0], c, w_hh, lengths, seq_out, T, reverse):
        return h2[0]
    with _timed("lstm_step", 2.0 * T * B * 4 * hs * hs, T * (2.0 * 4 * hs * hs + 4.0 * B * hs * 8)):
        rc = _lib.load().vt_lstm_sequence_f32(
            _ptr(xproj), xproj.stride(0), xproj.stride(1), _ptr(h2[0]), _ptr(h2[1]), _ptr(c), _ptr(w_hh), _ptr(lengths),
            _ptr(seq_out), 0 if seq_out is None else seq_out.stride(0), 0 if seq_out is None else seq_out.stride(1),
            B, hs, int(T), 1 if reverse else 0, _stream())
    _lib.check(rc, "vt_lstm_sequence_f32")
    return h2[0]


def skinny_linear(x0, w_pad, bias=None, x1=None, act=ACT_NONE):
    """act([x0 | x1] @ W.T + bias) in fp32 for a handful of rows: x0 [M,K0], x1 [M,K1] fp32 (any widths K0 >= 1, K1 >= 0,
    any row strides: the rows are read by address, a 4-column group may straddle the two), any N, w_pad bf16 [N, Kpad]
    zero-padded past K0 + K1 (Kpad a multiple of 32, row stride a multiple of 8)."""
    _require_hip(x0, x1, w_pad, bias)
    assert x0.dtype == torch.float32 and x0.dim() == 2 and x0.stride(1) == 1
    M, K0 = x0.shape
    K1 = 0
    if x1 is not None:
        assert x1.dtype == torch.float32 and x1.shape[0] == M and x1.stride(1) == 1
        K1 = x1.shape[1]
    assert w_pad.dtype == BF16 and w_pad.stride(1) == 1
    N, Kpad = w_pad.shape
    out = torch.empty((M, N), dtype=torch.float32, device=x0.device)
    with _timed("skinny_linear", 2.0 * M * N * (K0 + K1), 2.0 * N * Kpad):
        rc = _lib.load().vt_skinny_linear_f32(
            _ptr(x0), x0.stride(0), K0, _ptr(x1), 0 if x1 is None else x1.stride(0), K1, _ptr(w_pad), w_pad.stride(0),
            _ptr(bias), _ptr(out), out.stride(0), M, N, Kpad, int(act), _stream())
    _lib.check(rc, "vt_skinny_linear_f32")
    return out


def lstm_sequence_rows(xproj, row_start, h2, c, w_hh, T, lengths, seq_out=None, reverse=False):
    """lstm_sequence over compacted input projections: xproj fp32 [rows, 4*hs] holds only the positions below each
    sequence's length, row of (b, t) = row_start[b] + t (int32 [B]); lengths int32 [B] is required."""
    _require_hip(xproj, row_start, h2[0], h2[1], c, w_hh, lengths, seq_out)
    B, hs = c.shape
    assert xproj.dtype == torch.float32 and xproj.dim() == 2 and xproj.shape[1] == 4 * hs and xproj.stride(1) == 1
    assert row_start.dtype == torch.int32 and row_start.shape == (B,) and lengths.dtype == torch.int32 and lengths.shape == (B,)
    assert w_hh.dtype == BF16 and w_hh.shape == (4 * hs, hs) and w_hh.is_contiguous()
    for s_ in (h2[0], h2[1], c):
        assert s_.dtype == torch.float32 and s_.shape == (B, hs) and s_.is_contiguous()
    if seq_out is not None:
        assert seq_out.dtype == torch.float32 and seq_out.shape == (B, T, hs) and seq_out.stride(2) == 1
    if _lstm_persistent(xproj, 0, xproj.stride(0), row_start, h2[0], c, w_hh, lengths, seq_out, T, reverse):
        return h2[0]
    with _timed("lstm_step", 2.0 * T * B * 4 * hs * hs, T * (2.0 * 4 * hs * hs + 4.0 * B * hs * 8)):
        rc = _lib.load().vt_lstm_sequence_rows_f32(
            _ptr(xproj), xproj.stride(0), _ptr(row_start), _ptr(h2[0]), _ptr(h2[1]), _ptr(c), _ptr(w_hh), _ptr(lengths),
            _ptr(seq_out), 0 if seq_out is None else seq_out.stride(0), 0 if seq_out is None else seq_out.stride(1),
            B, hs, int(T), 1 if reverse else 0, _stream())
    _lib.check(rc, "vt_lstm_sequence_rows_f32")
    return h2[0]


# ---- rollout training (agent.py:493-518 back-propagates through OscarEncoder / AttnDecoderLSTM) ------------------------
def lstm_step_train(xproj, h_prev, c_prev, w_hh):
    """nn.LSTMCell step that keeps what its backward needs -> (h_1, c_1, saved) with saved = (gates fp32 [B,4hs] activated
    i f g o, c_prev fp32, h_prev bf16)."""
    _require_hip(xproj, h_prev, c_prev, w_hh)
    B, hs = h_prev.shape
    assert xproj.dtype == torch.float32 and xproj.shape == (B, 4 * hs) and xproj.stride(1) == 1
    assert w_hh.dtype == BF16 and w_hh.shape == (4 * hs, hs) and w_hh.is_contiguous()
    assert h_prev.dtype == torch.float32 and h_prev.is_contiguous() and c_prev.shape == (B, hs)
    dev = xproj.device
    h1 = torch.empty((B, hs), dtype=torch.float32, device=dev)
    c1 = c_prev.detach().to(torch.float32).clone()
    sv_g = torch.empty((B, 4 * hs), dtype=torch.float32, device=dev)
    sv_c = torch.empty((B, hs), dtype=torch.float32, device=dev)
    sv_h = torch.empty((B, hs), dtype=BF16, device=dev)
    rc = _lib.load().vt_lstm_step_train_f32(_ptr(xproj), xproj.stride(0), _ptr(h_prev), _ptr(h1), _ptr(c1), _ptr(w_hh), None,
                                            None, 0, B, hs, 0, _ptr(sv_g), _ptr(sv_c), _ptr(sv_h), _stream())
    _lib.check(rc, "vt_lstm_step_train_f32")
    return h1, c1, (sv_g, sv_c, sv_h)


def lstm_step_bwd(dh, dc, saved, w_hh_t):
    """Gradient of one nn.LSTMCell step: dh / dc fp32 [B,hs] (either may be None) -> (dgates fp32 [B,4hs], dgates bf16,
    dc_prev fp32 [B,hs]).  The caller turns dgates into dx / dh_prev (dense products) and dW (vt_wgrad_bf16)."""
    sv_g, sv_c, _ = saved
    B, hs = sv_c.shape
    dev = sv_c.device
    _require_hip(dh, dc, sv_g, w_hh_t)
    assert w_hh_t.dtype == BF16 and w_hh_t.shape == (hs, 4 * hs) and w_hh_t.is_contiguous()
    dcb = torch.zeros((B, hs), dtype=torch.float32, device=dev) if dc is None else dc.detach().float().contiguous().clone()
    dhf = None if dh is None else dh.detach().float().contiguous()
    dg16 = torch.empty((B, 4 * hs), dtype=BF16, device=dev)
    dg32 = torch.empty((B, 4 * hs), dtype=torch.float32, device=dev)
    rc = _lib.load().vt_lstm_step_bwd_f32(None, 0, _ptr(w_hh_t), _ptr(dhf), None, 0, _ptr(dcb), _ptr(sv_g), sv_g.stride(0),
                                          _ptr(sv_c), sv_c.stride(0), _ptr(dg16), dg16.stride(0), _ptr(dg32),
                                          dg32.stride(0), None, B, hs, 0, -1, _stream())
    _lib.check(rc, "vt_lstm_step_bwd_f32")
    return dg32, dg16, dcb


def lstm_sequence_train(xproj, w_hh, T, lengths=None, reverse=False):
    """One nn.LSTM direction from a zero initial state (agent_models.py:238-254) over xproj fp32 [B,S,4hs], keeping what the
    backward needs -> (seq_out fp32 [B,T,hs], h_T, c_T, saved)."""
    _require_hip(xproj, w_hh, lengths)
    B, S, G = xproj.shape
    hs = G // 4
    assert xproj.dtype == torch.float32 and xproj.stride(2) == 1 and 0 < T <= S
    assert w_hh.dtype == BF16 and w_hh.shape == (4 * hs, hs) and w_hh.is_contiguous()
    dev = xproj.device
    h2 = (torch.zeros((B, hs), dtype=torch.float32, device=dev), torch.empty((B, hs), dtype=torch.float32, device=dev))
    c = torch.zeros((B, hs), dtype=torch.float32, device=dev)
    seq_out = torch.empty((B, T, hs), dtype=torch.float32, device=dev)
    sv_g = torch.empty((B, S, 4 * hs), dtype=torch.float32, device=dev)
    sv_c = torch.empty((B, S, hs), dtype=torch.float32, device=dev)
    sv_h = torch.zeros((B, S, hs), dtype=BF16, device=dev)     # zeros: rows the recurrence never ran multiply zero dgates
    with _timed("lstm_step", 2.0 * T * B * 4 * hs * hs, T * (2.0 * 4 * hs * hs + 4.0 * B * hs * 8)):
        rc = _lib.load().vt_lstm_sequence_train_f32(
            _ptr(xproj), xproj.stride(0), xproj.stride(1), _ptr(h2[0]), _ptr(h2[1]), _ptr(c), _ptr(w_hh), _ptr(lengths),
            _ptr(seq_out), seq_out.stride(0), seq_out.stride(1), B, hs, int(T), 1 if reverse else 0, _ptr(sv_g), _ptr(sv_c),
            _ptr(sv_h), S, _stream())
    _lib.check(rc, "vt_lstm_sequence_train_f32")
    return seq_out, h2[0], c, (sv_g, sv_c, sv_h)


def lstm_sequence_bwd(d_seq_out, dh_final, dc_final, saved, w_hh_t, T, lengths=None, reverse=False):
    """Back-propagation through the T steps of lstm_sequence_train -> dgates bf16 [B,S,4hs] (pre-activation gate gradients
    = the gradient of xproj; zero where a row was inactive)."""
    sv_g, sv_c, _ = saved
    B, S, hs = sv_c.shape
    dev = sv_c.device
    _require_hip(d_seq_out, dh_final, dc_final, w_hh_t, lengths)
    assert w_hh_t.dtype == BF16 and w_hh_t.shape == (hs, 4 * hs) and w_hh_t.is_contiguous()
    if d_seq_out is not None:
        d_seq_out = d_seq_out.detach().float()
        if d_seq_out.stride(2) != 1:
            d_seq_out = d_seq_out.contiguous()
        assert d_seq_out.shape == (B, T, hs)
    dhf = None if dh_final is None else dh_final.detach().float().contiguous()
    dc = torch.zeros((B, hs), dtype=torch.float32, device=dev) if dc_final is None else dc_final.detach().float().contiguous().clone()
    dg = torch.zeros((B, S, 4 * hs), dtype=BF16, device=dev)
    with _timed("lstm_step_bwd", 2.0 * T * B * 4 * hs * hs, T * (2.0 * 4 * hs * hs + 4.0 * B * hs * 8)):
        rc = _lib.load().vt_lstm_sequence_bwd_f32(
            _ptr(d_seq_out), 0 if d_seq_out is None else d_seq_out.stride(0), 0 if d_seq_out is None else d_seq_out.stride(1),
            _ptr(dhf), _ptr(dc), _ptr(w_hh_t), _ptr(lengths), _ptr(sv_g), _ptr(sv_c), _ptr(dg), S, B, hs, int(T),
            1 if reverse else 0, _stream())
    _lib.check(rc, "vt_lstm_sequence_bwd_f32")
    return dg


SOFTDOT_SPLIT_KEYS = 128   # contexts at least this long take the two-launch form of the soft-dot backward (shorter: slower)


def softdot_attention_bwd(target, context, mask, d_weighted, d_attn, output_prob, want_d_context):
    """Gradient of softdot_attention -> (d_target fp32 [B,D], d_context fp32 [B,L,D] | None)."""
    _require_hip(target, context, mask, d_weighted, d_attn)
    B, L, D = context.shape
    assert target.dtype == torch.float32 and target.shape == (B, D) and target.is_contiguous()
    assert context.dtype == torch.float32 and context.stride(2) == 1
    m8 = None
    if mask is not None:
        m8 = (mask if mask.dtype == torch.uint8 else mask.to(torch.bool).view(torch.uint8)).contiguous()
    dw = None if d_weighted is None else d_weighted.detach().float().contiguous()
    da = None if d_attn is None else d_attn.detach().float().contiguous()
    d_ctx = torch.empty((B, L, D), dtype=torch.float32, device=target.device) if want_d_context else None
    if L >= SOFTDOT_SPLIT_KEYS:   # a long context: two launches spread over keys instead of one workgroup per batch row
        lib = _lib.load()
        ws = torch.empty(int(lib.vt_softdot_attention_bwd_split_ws_floats(B, L, D)), dtype=torch.float32, device=target.device)
        with _timed("softdot_attention_bwd", 6.0 * B * L * D, 12.0 * B * L * D):
            rc = lib.vt_softdot_attention_bwd_split_f32(
                _ptr(target), _ptr(context), context.stride(0), context.stride(1), _ptr(m8), _ptr(dw), _ptr(da), _ptr(d_ctx),
                _ptr(ws), B, L, D, 1 if output_prob else 0, _stream())
        _lib.check(rc, "vt_softdot_attention_bwd_split_f32")
        return ws[2 * B * L:].view(B, -1, D).sum(1), d_ctx
    d_target = torch.empty((B, D), dtype=torch.float32, device=target.device)
    with _timed("softdot_attention_bwd", 6.0 * B * L * D, 12.0 * B * L * D):
        rc = _lib.load().vt_softdot_attention_bwd_f32(
            _ptr(target), _ptr(context), context.stride(0), context.stride(1), _ptr(m8), _ptr(dw), _ptr(da), _ptr(d_target),
            _ptr(d_ctx), B, L, D, 1 if output_prob else 0, _stream())
    _lib.check(rc, "vt_softdot_attention_bwd_f32")
    return d_target, d_ctx


# ---- the turn-based decoder step (tasks/turn_based/agent_models.py:277-319, agent.py:307-338; csrc/turn_based.hip) ------
def turn_lstm_cell(first, feature, h_prev, c_prev, w_ih_pad, w_hh, bias, h_out=None, c_out=None, save=False, err_flag=None):
    """nn.Embedding + cat + nn.LSTMCell in one launch.  first = (ids int64 [B], table fp32 [A, E]) or a ready fp32 [B, E]
    block; feature fp32 [B, F]; rows of table / block / feature may be strided views (last dim contiguous) of any width.
    w_ih_pad bf16 [4hs, Kpad] zero past E + F (Kpad a multiple of 32), w_hh bf16 [4hs, hs], bias fp32 [4hs] = b_ih + b_hh.
    h_prev / c_prev fp32 [B, hs] contiguous and left as they are -> (h_1, c_1, saved | None), saved = (activated gates fp32
    [B, 4hs], c_prev fp32, h_prev bf16) as ops.lstm_step_bwd reads them (save=True allocates them, a tuple is written into).  An id outside the table: the row's embedding counts
    as zero and err_flag (int32 [1]) is raised."""
    if isinstance(first, (tuple, list)):
        ids, table = first
        x_emb = None
        _require_hip(ids, table)
        assert ids.dtype == torch.int64 and ids.dim() == 1 and ids.is_contiguous()
        assert table.dtype == torch.float32 and table.dim() == 2 and table.stride(1) == 1
        A, E = table.shape
        B = ids.shape[0]
    else:
        ids = table = None
        x_emb = first
        _require_hip(x_emb)
        assert x_emb.dtype == torch.float32 and x_emb.dim() == 2 and x_emb.stride(1) == 1
        B, E = x_emb.shape
        A = 0
    _require_hip(feature, h_prev, c_prev, w_ih_pad, w_hh, bias, h_out, c_out, err_flag)
    hs = h_prev.shape[1]
    assert feature.dtype == torch.float32 and feature.dim() == 2 and feature.shape[0] == B and feature.stride(1) == 1
    F = feature.shape[1]
    for s_ in (h_prev, c_prev):
        assert s_.dtype == torch.float32 and s_.shape == (B, hs) and s_.is_contiguous()
    assert w_ih_pad.dtype == BF16 and w_ih_pad.shape[0] == 4 * hs and w_ih_pad.stride(1) == 1
    assert w_hh.dtype == BF16 and w_hh.shape == (4 * hs, hs) and w_hh.is_contiguous()
    assert bias.dtype == torch.float32 and bias.shape == (4 * hs,) and bias.is_contiguous()
    dev = h_prev.device
    if h_out is None:
        h_out = torch.empty((B, hs), dtype=torch.float32, device=dev)
    if c_out is None:
        c_out = torch.empty((B, hs), dtype=torch.float32, device=dev)
    for s_ in (h_out, c_out):
        assert s_.dtype == torch.float32 and s_.shape == (B, hs) and s_.is_contiguous()
    saved = None
    if isinstance(save, (tuple, list)):   # the caller's buffers
        saved = tuple(save)
        for s_, shp, dt in zip(saved, ((B, 4 * hs), (B, hs), (B, hs)), (torch.float32, torch.float32, BF16)):
            _require_hip(s_)
            assert s_.dtype == dt and s_.shape == shp and s_.is_contiguous()
        save = True
    elif save:
        saved = (torch.empty((B, 4 * hs), dtype=torch.float32, device=dev), torch.empty((B, hs), dtype=torch.float32, device=dev),
                 torch.empty((B, hs), dtype=BF16, device=dev))
    if err_flag is not None:
        assert err_flag.dtype == torch.int32 and err_flag.numel() == 1
    Kpad = w_ih_pad.shape[1]
    with _timed("turn_lstm_cell", 2.0 * B * 4 * hs * (E + F + hs), 2.0 * 4 * hs * (Kpad + hs)):
        rc = _lib.load().vt_turn_lstm_cell_f32(
            _ptr(ids), _ptr(table), 0 if table is None else table.stride(0), A, _ptr(x_emb),
            0 if x_emb is None else x_emb.stride(0), E, _ptr(feature), feature.stride(0), F, _ptr(h_prev), _ptr(c_prev),
            _ptr(w_ih_pad), w_ih_pad.stride(0), Kpad, _ptr(w_hh), _ptr(bias), _ptr(h_out), _ptr(c_out),
            _ptr(saved[0]) if save else None, _ptr(saved[1]) if save else None, _ptr(saved[2]) if save else None,
            _ptr(err_flag), B, hs, _stream())
    _lib.check(rc, "vt_turn_lstm_cell_f32")
    return h_out, c_out, saved


TURN_FEEDBACK = {"teacher": 0, "argmax": 1, "sample": 2}


def _blocked_u8(blocked, B, A):
    if blocked is None:
        return None
    assert blocked.shape == (B, A)
    b8 = blocked if blocked.dtype == torch.uint8 else blocked.to(torch.bool).view(torch.uint8)
    return b8 if b8.stride(1) == 1 else b8.contiguous()


def turn_action_head(logit, target, blocked, ignore_index, mode, seed, err_flag=None):
    """One step's cross entropy and next action: logit fp32 [B, A] (A <= 64, row stride free, not modified), target int64
    [B], blocked bool / uint8 [B, A] or None -> (loss fp32 [1], count fp32 [1], a_t int64 [B])."""
    _require_hip(logit, target, blocked, err_flag)
    assert logit.dtype == torch.float32 and logit.dim() == 2 and logit.stride(1) == 1
    B, A = logit.shape
    assert target.dtype == torch.int64 and target.shape == (B,) and target.is_contiguous()
    b8 = _blocked_u8(blocked, B, A)
    loss = torch.empty((1,), dtype=torch.float32, device=logit.device)
    count = torch.empty((1,), dtype=torch.float32, device=logit.device)
    a_t = torch.empty((B,), dtype=torch.int64, device=logit.device)
    with _timed("turn_action_head", 0.0, 8.0 * B * A):
        rc = _lib.load().vt_turn_action_head_f32(
            _ptr(logit), logit.stride(0), _ptr(target), _ptr(b8), 0 if b8 is None else b8.stride(0), int(ignore_index), B, A,
            int(mode), int(seed) & 0xFFFFFFFF, _ptr(loss), _ptr(count), _ptr(a_t), _ptr(err_flag), _stream())
    _lib.check(rc, "vt_turn_action_head_f32")
    return loss, count, a_t


def turn_action_head_bwd(logit, target, blocked, ignore_index, g, count):
    """dlogit fp32 [B, A] of turn_action_head's loss; g fp32 [1] (device) is the loss's gradient, count what the forward left."""
    _require_hip(logit, target, blocked, g, count)
    B, A = logit.shape
    b8 = _blocked_u8(blocked, B, A)
    assert g.dtype == torch.float32 and g.numel() == 1 and count.dtype == torch.float32 and count.numel() == 1
    dlogit = torch.empty((B, A), dtype=torch.float32, device=logit.device)
    with _timed("turn_action_head_bwd", 0.0, 8.0 * B * A):
        rc = _lib.load().vt_turn_action_head_bwd_f32(
            _ptr(logit), logit.stride(0), _ptr(target), _ptr(b8), 0 if b8 is None else b8.stride(0), int(ignore_index), B, A,
            _ptr(g), _ptr(count), _ptr(dlogit), dlogit.stride(0), _stream())
    _lib.check(rc, "vt_turn_action_head_bwd_f32")
    return dlogit


# ---- the rollout's observation tensors from a device feature store (csrc/observations.hip) ------------------------------------
def obs_record_bytes(B, Cmax):
    """Size of one step's staged record (include/visitron_hip.h, vt_obs_gather_f32) and the byte offset of its doubles."""
    off_f64 = round_up(12 * B + 4 * B * Cmax, 8)
    return off_f64 + 8 * (2 * B + 2 * B * Cmax), off_f64


def obs_gather(store, table, record, B, Cmax, out=None, err_flag=None):
    """One launch for a panoramic step's inputs.  store fp32 [N, V, D], table fp32 [V, V, 4], record uint8 [>= record bytes]
    on the device (8-byte aligned, laid out as vt_obs_gather_f32 says) -> (input_a_t fp32 [B, 4], f_t fp32 [B, V, D+4],
    candidate_feat fp32 [B, Cmax, D+4], candidate_leng int32 [B], candidate_mask bool [B, Cmax]).  out: the five tensors to
    write into (contiguous), else they are allocated."""
    _require_hip(store, table, record, err_flag)
    assert store.dtype == torch.float32 and store.dim() == 3 and store.is_contiguous()
    N, V, D = store.shape
    assert table.dtype == torch.float32 and tuple(table.shape) == (V, V, 4) and table.is_contiguous()
    assert record.dtype == torch.uint8 and record.dim() == 1 and record.numel() >= obs_record_bytes(B, Cmax)[0]
    dev = store.device
    if out is None:
        out = (torch.empty((B, 4), dtype=torch.float32, device=dev), torch.empty((B, V, D + 4), dtype=torch.float32, device=dev),
               torch.empty((B, Cmax, D + 4), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
               torch.empty((B, Cmax), dtype=torch.bool, device=dev))
    a_t, f_t, cand, leng, mask = out
    for t, shp, dt in zip(out, ((B, 4), (B, V, D + 4), (B, Cmax, D + 4), (B,), (B, Cmax)),
                          (torch.float32, torch.float32, torch.float32, torch.int32, torch.bool)):
        _require_hip(t)
        assert t.dtype == dt and tuple(t.shape) == shp and t.is_contiguous()
    if err_flag is not None:
        assert err_flag.dtype == torch.int32 and err_flag.numel() == 1
    nbytes = 4.0 * B * (V + Cmax) * (D + 4)
    with _timed("obs_gather", 0.0, 2.0 * nbytes):
        rc = _lib.load().vt_obs_gather_f32(_ptr(store), N, V, D, _ptr(table), _ptr(record), B, Cmax, _ptr(a_t), _ptr(f_t),
                                           _ptr(cand), _ptr(leng), _ptr(mask), _ptr(err_flag), _stream())
    _lib.check(rc, "vt_obs_gather_f32")
    return out


def obs_gather_view(store, rows, B, out=None, err_flag=None):
    """out[b] = store[slot_b, view_b, :].  rows int32 [B, 2] on the device; out fp32 [B, D] (row stride free)."""
    _require_hip(store, rows, out, err_flag)
    assert store.dtype == torch.float32 and store.dim() == 3 and store.is_contiguous()
    N, V, D = store.shape
    assert rows.dtype == torch.int32 and rows.numel() >= 2 * B and rows.is_contiguous()
    if out is None:
        out = torch.empty((B, D), dtype=torch.float32, device=store.device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, D) and out.stride(1) == 1
    if err_flag is not None:
        assert err_flag.dtype == torch.int32 and err_flag.numel() == 1
    with _timed("obs_gather_view", 0.0, 8.0 * B * D):
        rc = _lib.load().vt_obs_gather_view_f32(_ptr(store), N, V, D, _ptr(rows), B, _ptr(out), out.stride(0) if B > 1 else D,
                                                _ptr(err_flag), _stream())
    _lib.check(rc, "vt_obs_gather_view_f32")
    return out


# ---- pretraining's region rows from a device region store (csrc/regions.hip) ---------------------------------------------------
def region_gather(store, counts, loc_table, rows, D, text_labels, text_mask, text_token_classes, R, kpad=None, out=None,
                  err_flag=None):
    """One launch for a pretraining batch's region tensors.  store [N, 36, P, round_up(D, 8)] fp32 or bf16, counts uint8
    [N, 36], loc_table fp32 [36, 36, 128], rows int32 [B, 2] = slot, current view, the text tensors int64 [B, T] (token
    classes may be None), all on the device.  kpad None -> (img_feats fp32 [B, R, D], img_location_embeddings fp32 [B, R, 128],
    labels, attention_mask, token_labels int64 [B, T + R]); kpad given -> (img_packed bf16 [B * R, kpad], labels,
    attention_mask, token_labels).  out: the tensors to write into (contiguous), else they are allocated."""
    _require_hip(store, counts, loc_table, rows, text_labels, text_mask, text_token_classes, err_flag)
    assert store.dtype in (torch.float32, BF16) and store.dim() == 4 and store.is_contiguous()
    N, V, P, ld = store.shape
    assert ld == round_up(D, 8) and counts.dtype == torch.uint8 and tuple(counts.shape) == (N, V) and counts.is_contiguous()
    assert loc_table.dtype == torch.float32 and tuple(loc_table.shape) == (36, 36, 128) and loc_table.is_contiguous()
    assert rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[1] == 2 and rows.is_contiguous()
    B, T = text_labels.shape
    assert rows.shape[0] == B
    for t in (text_labels, text_mask, text_token_classes):
        assert t is None or (t.dtype == torch.int64 and tuple(t.shape) == (B, T) and t.is_contiguous())
    dev = store.device
    tok = text_token_classes is not None
    packed = kpad is not None
    shapes = (((B * R, kpad), BF16),) if packed else (((B, R, D), torch.float32), ((B, R, 128), torch.float32))
    shapes += (((B, T + R), torch.int64),) * 3
    if out is None:
        out = tuple(torch.empty(s, dtype=dt, device=dev) for s, dt in shapes)
        if not tok:
            out = out[:-1] + (None,)
    assert len(out) == len(shapes) and (out[-1] is not None) == tok
    for t, (s, dt) in zip(out, shapes):
        if t is not None:
            _require_hip(t)
            assert t.dtype == dt and tuple(t.shape) == s and t.is_contiguous()
    if err_flag is not None:
        assert err_flag.dtype == torch.int32 and err_flag.numel() == 1
    head = (_ptr(store), int(store.dtype == BF16), N, V, P, D, _ptr(counts), _ptr(loc_table), _ptr(rows), _ptr(text_labels),
            _ptr(text_mask), _ptr(text_token_classes), B, T, R)
    tail = (_ptr(out[-3]), _ptr(out[-2]), _ptr(out[-1]), _ptr(err_flag), _stream())
    if packed:
        with _timed("region_gather_pack", 0.0, B * R * (float(store.element_size()) * D + 2.0 * kpad)):
            rc = _lib.load().vt_region_gather_pack_bf16(*(head + (_ptr(out[0]), kpad) + tail))
        _lib.check(rc, "vt_region_gather_pack_bf16")
    else:
        with _timed("region_gather", 0.0, B * R * (float(store.element_size()) * D + 4.0 * (D + 128))):
            rc = _lib.load().vt_region_gather_f32(*(head + (_ptr(out[0]), _ptr(out[1])) + tail))
        _lib.check(rc, "vt_region_gather_f32")
    return out


def packed_region_rows(img_packed, img_rows, img_feats, B, kpad, device):
    """The checks on a batch that carries the region projection's operand ready-made (RegionStore.pretrain_batch(packed=True))
    -> R.  img_packed must be contiguous bf16 [B * img_rows, kpad] on `device`, and img_feats must not come with it."""
    if img_feats is not None:
        raise ValueError("a batch carries img_feats or img_packed, not both")
    if img_rows is None:
        raise ValueError("img_packed needs img_rows, the region positions per sequence")
    R = int(img_rows)
    if not isinstance(img_packed, torch.Tensor) or img_packed.dtype != BF16:
        raise ValueError("img_packed must be a bfloat16 tensor")
    if R < 0 or tuple(img_packed.shape) != (B * R, kpad):
        raise ValueError("img_packed must be [batch * img_rows, %d] = [%d, %d], got %s"
                         % (kpad, B * R, kpad, tuple(img_packed.shape)))
    if not img_packed.is_contiguous():
        raise ValueError("img_packed must be contiguous")
    if img_packed.device != torch.device(device):
        raise ValueError("img_packed is on %s, the model on %s" % (img_packed.device, torch.device(device)))
    return R


# ---- fp32 parity path (csrc/fp32_path.hip): every operand, activation and accumulation in fp32 -----------------------
def _f32ok(*ts):
    for t in ts:
        assert t is None or (t.dtype == torch.float32 and t.stride(-1) == 1), "fp32 path: contiguous-row fp32 tensors"


PRODUCTS = ("fp32", "bf16x3")


def _products_ok(products):
    if products not in PRODUCTS:
        raise ValueError("products must be one of %s, got %r" % (PRODUCTS, products))
    return products == "bf16x3"


def linear_f32(a, w, bias=None, residual=None, act=ACT_NONE, out=None, w_is_kn=False, alpha=1.0, grp_rows=0, grp_stride=0,
               M=None, lda=None, ldc=None, products="fp32"):
    """out = act(alpha * a @ w.T + bias) (+ residual), fp32 operands and output.  a [M,K] (row stride lda), w [N,K]
    (nn.Linear.weight) or [K,N] with w_is_kn.  products: "fp32" -- the product on the fp32 matrix cores -- or "bf16x3" --
    each operand split in the kernel into two bf16 terms, the product as three bf16 MFMAs with fp32 accumulation
    (csrc/bf16x3_path.hip: |error| <= 3 * 2^-16 * |alpha| * |a| @ |w|.T to first order)."""
    x3 = _products_ok(products)
    _require_hip(a, w, bias, residual, out)
    _f32ok(a, w, bias, residual, out)
    K = a.shape[-1]
    N = w.shape[1] if w_is_kn else w.shape[0]
    assert (w.shape[0] if w_is_kn else w.shape[1]) == K
    if M is None:
        M = a.shape[0]
    if lda is None:
        lda = a.stride(0)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    if ldc is None:
        ldc = out.stride(0)
    lib = _lib.load()
    name = "vt_linear_bf16x3" if x3 else "vt_linear_f32"
    with _timed("gemm_bf16x3" if x3 else "gemm_f32", 2.0 * M * N * K, 4.0 * (M * K + N * K + M * N)):
        rc = getattr(lib, name)(_ptr(a), lda, _ptr(w), w.stride(0), 1 if w_is_kn else 0, _ptr(bias), _ptr(residual),
                                0 if residual is None else residual.stride(0), _ptr(out), ldc, M, N, K, int(act),
                                float(alpha), grp_rows, grp_stride, _stream())
    _lib.check(rc, name)
    return out


def attention_f32(qkv, B, S, nh, mask=None, mask_additive=False, head_scale=None, want_probs=False, products="fp32"):
    """oscar/modeling_bert.py:47-72 in fp32 on the packed projection qkv fp32 [B*S, 3*nh*64]: scores = q k^T (one batched
    product), / sqrt(64) + mask, softmax, * head_mask (one row kernel, in place), context = probs v (one batched product).
    products: the arithmetic of the two products, as in linear_f32; the softmax is the same call either way.
    -> (ctx fp32 [B*S, nh*64], probs fp32 [B, nh, S, S] or None)."""
    _require_hip(qkv, mask, head_scale)
    _f32ok(qkv, mask, head_scale)
    x3 = _products_ok(products)
    H = nh * 64
    ld = qkv.stride(0)
    lib = _lib.load()
    name = "vt_bmm_bf16x3" if x3 else "vt_bmm_f32"
    bmm, tag = getattr(lib, name), ("bmm_bf16x3" if x3 else "bmm_f32")
    flops, nbytes = 2.0 * B * nh * S * S * 64, 4.0 * B * nh * (2 * S * 64 + S * S)
    probs = torch.empty((B, nh, S, S), dtype=torch.float32, device=qkv.device)
    q, k, v = qkv, qkv[:, H:], qkv[:, 2 * H:]
    with _timed(tag, flops, nbytes):
        rc = bmm(_ptr(q), ld, S * ld, 64, _ptr(k), ld, S * ld, 64, 0, _ptr(probs), S, nh * S * S, S * S, S, S, 64, 1.0,
                 B, nh, _stream())
    _lib.check(rc, name + " (q k^T)")
    mode = -1 if mask is None else _mask_mode(mask, mask_additive, B, S)
    rc = lib.vt_softmax_rows_f32(_ptr(probs), S, B * nh * S, S, 0.125, _ptr(mask), mode, _ptr(head_scale), nh, S, _stream())
    _lib.check(rc, "vt_softmax_rows_f32")
    ctx = torch.empty((B * S, H), dtype=torch.float32, device=qkv.device)
    with _timed(tag, flops, nbytes):
        rc = bmm(_ptr(probs), S, nh * S * S, S * S, _ptr(v), ld, S * ld, 64, 1, _ptr(ctx), H, S * H, 64, S, 64, S, 1.0,
                 B, nh, _stream())
    _lib.check(rc, name + " (probs v)")
    return ctx, (probs if want_probs else None)


def softmax_rows_f32(x):
    """In-place softmax over the last dim of a 2-D fp32 tensor (the token head's nn.Softmax, encoder.py:323-326)."""
    _require_hip(x)
    _f32ok(x)
    rc = _lib.load().vt_softmax_rows_f32(_ptr(x), x.stride(0), x.shape[0], x.shape[1], 1.0, None, -1, None, 1, 1, _stream())
    _lib.check(rc, "vt_softmax_rows_f32")
    return x


def layernorm_rows(x, gamma, beta, eps, out=None, out_f32=None, M=None, grp_rows=0, grp_stride=0):
    """BertLayerNorm over fp32 or bf16 rows into fp32 or bf16 rows (default: the input's type)."""
    _require_hip(x, gamma, beta, out)
    assert x.dtype in (torch.float32, BF16) and x.stride(-1) == 1
    if out is None:
        want32 = (x.dtype == torch.float32) if out_f32 is None else bool(out_f32)
        out = torch.empty(x.shape, dtype=torch.float32 if want32 else BF16, device=x.device)
    if M is None:
        M = x.shape[0]
    rc = _lib.load().vt_layernorm_rows(_ptr(x), x.stride(0), 1 if x.dtype == torch.float32 else 0, _ptr(out), out.stride(0),
                                       1 if out.dtype == torch.float32 else 0, _ptr(gamma), _ptr(beta), M, gamma.numel(),
                                       float(eps), grp_rows, grp_stride, _stream())
    _lib.check(rc, "vt_layernorm_rows")
    return out


def embed_layernorm_f32(ids, type_ids, pos_ids, word, pos, typ, gamma, beta, eps, out, S, err_flag=None):
    """BertEmbeddings with fp32 output: rows b*S + t (t < T) of ``out`` [B*S, H] fp32."""
    _require_hip(ids, word, out)
    _f32ok(word, pos, typ, gamma, beta, out)
    B, T = ids.shape
    rc = _lib.load().vt_embed_layernorm_f32(_ptr(ids), _ptr(type_ids), _ptr(pos_ids), _ptr(word), _ptr(pos), _ptr(typ),
                                            _ptr(gamma), _ptr(beta), _ptr(out), out.stride(0), B, T, S, word.shape[1],
                                            word.shape[0], pos.shape[0], typ.shape[0], float(eps), _ptr(err_flag), _stream())
    _lib.check(rc, "vt_embed_layernorm_f32")
    return out


# ---- fp32 training step (PretrainEngine(..., precision="fp32"); visitron_amd/training_f32.py) ------------------------------
def gemm_f32_ex(a, w, M, N, K, out, lda=None, ldw=None, ldc=None, a_is_km=False, w_is_kn=False, bias=None, residual=None,
                ldr=None, pre_act=None, act=ACT_NONE, alpha=1.0, batch=1, heads=1, strides=((0, 0), (0, 0), (0, 0)),
                grp_rows=0, grp_stride=0, accumulate=False, split=1, drop=NO_DROP):
    """out (+)= act(alpha * op(a) . op(w) + bias) (+ residual) in fp32 (vt_gemm_f32_ex).  op(a): a [M,K], or [K,M] with
    a_is_km (dY^T of a weight gradient); op(w): w [N,K], or [K,N] with w_is_kn.  strides: element strides ((a_b, a_h),
    (w_b, w_h), (c_b, c_h)) of a (batch, head)-batched product.  split: the K range in parts (0: the library's choice for the
    shape) summed in a fixed order.  pre_act: saved pre-activation (out's layout); drop: dropout before the residual add."""
    _require_hip(a, w, out, bias, residual, pre_act)
    _f32ok(a, w, out, bias, residual, pre_act)
    lib = _lib.load()
    if split == 0:
        split = int(lib.vt_gemm_f32_split_count(M, N, K)) if batch * heads == 1 else 1
    ws = torch.empty(split * M * N, dtype=torch.float32, device=a.device) if split > 1 else None
    (sab, sah), (swb, swh), (scb, sch) = strides
    with _timed("gemm_f32", 2.0 * M * N * K * batch * heads, 4.0 * (M * K + N * K + M * N) * batch * heads):
        rc = lib.vt_gemm_f32_ex(_ptr(a), a.stride(0) if lda is None else lda, sab, sah, 1 if a_is_km else 0, _ptr(w),
                                w.stride(0) if ldw is None else ldw, swb, swh, 1 if w_is_kn else 0, _ptr(bias), _ptr(residual),
                                0 if residual is None else (residual.stride(0) if ldr is None else ldr), _ptr(out),
                                out.stride(0) if ldc is None else ldc, scb, sch, _ptr(pre_act), M, N, K, int(act), float(alpha),
                                batch, heads, grp_rows, grp_stride, 1 if accumulate else 0, int(split), _ptr(ws),
                                float(drop[0]), int(drop[1]), int(drop[2]), _stream())
    _lib.check(rc, "vt_gemm_f32_ex")
    return out


def colsum_f32(x, out, accumulate=False):
    """out (+)= x.sum(0) over fp32 rows in a fixed order (bias gradients)."""
    _require_hip(x, out)
    _f32ok(x, out)
    rows, cols = x.shape
    ws = torch.empty(((rows + 255) // 256) * cols, dtype=torch.float32, device=x.device)
    rc = _lib.load().vt_colsum_f32(_ptr(x), x.stride(0), rows, cols, _ptr(out), 1 if accumulate else 0, _ptr(ws), _stream())
    _lib.check(rc, "vt_colsum_f32")
    return out


def wgrad_f32(dy, x, dw, db=None, accumulate=False, split=0):
    """dw (+)= dy^T . x and db (+)= dy.sum(0): dy [rows, N], x [rows, K] fp32, dw [N, K] (K-split over the rows)."""
    rows, N = dy.shape
    K = x.shape[1]
    gemm_f32_ex(dy, x, N, K, rows, dw, a_is_km=True, w_is_kn=True, accumulate=accumulate, split=split)
    if db is not None:
        colsum_f32(dy, db, accumulate=accumulate)


def layernorm_bwd_f32(x, g, gamma, eps, dgamma, dbeta, dx=None, dx_drop=None, accumulate=False, M=None, grp_rows=0,
                      grp_stride=0, drop_in=NO_DROP, drop_out=NO_DROP):
    """BertLayerNorm backward in fp32 from its saved input x [M, H]: dx (+ dx * keep / (1 - p) of drop_out's site into
    dx_drop), dgamma / dbeta (+)= their fixed-order sums.  g: dL/dy, row r at (r / grp_rows) * grp_stride + r % grp_rows;
    drop_in: g is first masked by that site (the embedding / image dropout that follows their LayerNorm)."""
    _require_hip(x, g, gamma, dx, dx_drop, dgamma, dbeta)
    _f32ok(x, g, gamma, dx, dx_drop, dgamma, dbeta)
    H = gamma.numel()
    if M is None:
        M = x.shape[0]
    lib = _lib.load()
    ws = torch.empty(int(lib.vt_layernorm_bwd_f32_ws_floats(M, H)), dtype=torch.float32, device=x.device)
    assert drop_in[0] == 0 or drop_out[0] == 0 or drop_in[1] == drop_out[1]
    seed = drop_in[1] if drop_in[0] > 0 else drop_out[1]
    rc = lib.vt_layernorm_bwd_f32(_ptr(x), x.stride(0), _ptr(g), g.stride(0), grp_rows, grp_stride, _ptr(gamma), float(eps),
                                  _ptr(dx), 0 if dx is None else dx.stride(0), _ptr(dx_drop),
                                  0 if dx_drop is None else dx_drop.stride(0), _ptr(dgamma), _ptr(dbeta), 1 if accumulate else 0,
                                  _ptr(ws), M, H, float(drop_in[0]), int(drop_in[2]), float(drop_out[0]), int(drop_out[2]),
                                  int(seed), _stream())
    _lib.check(rc, "vt_layernorm_bwd_f32")
    return dx


def layernorm_drop_f32(x, gamma, beta, eps, out, M=None, grp_rows=0, grp_stride=0, drop=NO_DROP):
    """out[remap(r)] = dropout(LayerNorm(x[r])) in fp32, element index r * H + c."""
    _require_hip(x, gamma, beta, out)
    _f32ok(x, gamma, beta, out)
    if M is None:
        M = x.shape[0]
    rc = _lib.load().vt_layernorm_drop_f32(_ptr(x), x.stride(0), _ptr(out), out.stride(0), _ptr(gamma), _ptr(beta), M,
                                           gamma.numel(), float(eps), grp_rows, grp_stride, float(drop[0]), int(drop[1]),
                                           int(drop[2]), _stream())
    _lib.check(rc, "vt_layernorm_drop_f32")
    return out


def attn_softmax_train_f32(probs, probs_dropped, B, nh, S, mask=None, mask_mode=-1, head_scale=None, drop=NO_DROP,
                           backward=False, scale=0.125):
    """Forward: probs [B*nh*S, S] holds the scores; -> P (in place) and P * keep / (1 - p) * head_scale into probs_dropped.
    Backward: probs_dropped holds dL/d(dropped probs) and becomes dL/d(scores) (the 1/8 included)."""
    _require_hip(probs, probs_dropped, mask, head_scale)
    _f32ok(probs, probs_dropped, mask, head_scale)
    assert probs.stride(0) == probs_dropped.stride(0)
    rc = _lib.load().vt_attn_softmax_train_f32(1 if backward else 0, _ptr(probs), _ptr(probs_dropped), probs.stride(0), B, nh, S,
                                               float(scale), _ptr(mask), int(mask_mode) if mask is not None else -1,
                                               _ptr(head_scale), float(drop[0]), int(drop[1]), int(drop[2]), _stream())
    _lib.check(rc, "vt_attn_softmax_train_f32")
    return probs_dropped


def dgelu_f32(g, pre, out=None):
    """out = g * GELU'(pre) (erf form), fp32, contiguous."""
    _require_hip(g, pre, out)
    assert g.is_contiguous() and pre.is_contiguous() and g.numel() == pre.numel()
    if out is None:
        out = torch.empty_like(g)
    rc = _lib.load().vt_dgelu_f32(_ptr(g), _ptr(pre), _ptr(out), g.numel(), _stream())
    _lib.check(rc, "vt_dgelu_f32")
    return out


def embed_sum_f32(ids, type_ids, pos_ids, word, pos, typ, out, err_flag=None):
    """out [B*T, H] = word[ids] + pos[pos_ids or t] + typ[type_ids or 0] (BertEmbeddings' sum before its LayerNorm)."""
    _require_hip(ids, word, out)
    _f32ok(word, pos, typ, out)
    B, T = ids.shape
    rc = _lib.load().vt_embed_sum_f32(_ptr(ids), _ptr(type_ids), _ptr(pos_ids), _ptr(word), _ptr(pos), _ptr(typ), _ptr(out), B, T,
                                      word.shape[1], word.shape[0], pos.shape[0], typ.shape[0], _ptr(err_flag), _stream())
    _lib.check(rc, "vt_embed_sum_f32")
    return out


def dropout_rows_f32(x, out, rows, grp_rows=0, grp_stride=0, drop=NO_DROP):
    """out[r] = x[remap(r)] * keep / (1 - p), element index r * cols + c."""
    _require_hip(x, out)
    _f32ok(x, out)
    rc = _lib.load().vt_dropout_rows_f32(_ptr(x), x.stride(0), grp_rows, grp_stride, _ptr(out), out.stride(0), rows,
                                         out.shape[1], float(drop[0]), int(drop[1]), int(drop[2]), _stream())
    _lib.check(rc, "vt_dropout_rows_f32")
    return out


def ce_softmax_rows_g32(z, y, V, dz, scale):
    """ce_softmax_rows with fp32 gradient rows dz [rows, Vpad]."""
    _require_hip(z, y, dz)
    rows = z.shape[0]
    loss = torch.empty(rows, dtype=torch.float32, device=z.device)
    amax = torch.empty(rows, dtype=torch.int64, device=z.device)
    rc = _lib.load().vt_ce_softmax_rows_g32(_ptr(z), z.stride(0), _ptr(y), _ptr(loss), _ptr(amax), _ptr(dz), dz.stride(0), rows, V,
                                            dz.shape[1], float(scale), _stream())
    _lib.check(rc, "vt_ce_softmax_rows_g32")
    return loss, amax


def ce_double_softmax_rows_g32(z, y, V, dz, scale):
    """ce_double_softmax_rows with fp32 gradient rows dz [rows, Vpad]."""
    _require_hip(z, y, dz)
    rows = z.shape[0]
    loss = torch.empty(rows, dtype=torch.float32, device=z.device)
    amax = torch.empty(rows, dtype=torch.int64, device=z.device)
    rc = _lib.load().vt_ce_double_softmax_rows_g32(_ptr(z), z.stride(0), _ptr(y), _ptr(loss), _ptr(amax), _ptr(dz), dz.stride(0),
                                                   rows, V, dz.shape[1], float(scale), _stream())
    _lib.check(rc, "vt_ce_double_softmax_rows_g32")
    return loss, amax


def action_head_g32(logits, next_action, A, grad_scale, Ap, dz=None):
    """action_head with an fp32 gradient: -> (loss 0-d, accuracy 0-d, dlogits fp32 [B, Ap]).  dz: the gradient's destination,
    fp32 [B, Ap] with any row stride (a view of a wider buffer); a fresh tensor otherwise."""
    _require_hip(logits, next_action, dz)
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and next_action.dtype == torch.int64
    B = logits.shape[0]
    dl = torch.empty((B, Ap), dtype=torch.float32, device=logits.device) if dz is None else dz
    assert dl.dtype == torch.float32 and tuple(dl.shape) == (B, Ap) and (dl.stride(1) == 1 or Ap == 1)
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    rc = _lib.load().vt_action_head_g32(_ptr(logits), logits.stride(0), _ptr(next_action.contiguous()), B, int(A),
                                        float(grad_scale), _ptr(dl), dl.stride(0), int(Ap), _ptr(out), _stream())
    _lib.check(rc, "vt_action_head_g32")
    return out[0], out[1], dl
