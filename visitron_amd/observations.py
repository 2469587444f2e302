"""The rollout's observation tensors, served from a feature store on the device.

The reference builds a decoder step's inputs on the host (tasks/viewpoint_select/agent.py:186-228, fed by `_get_obs` /
`make_candidate` in data_loader.py:516-642): per agent and step it concatenates a [36, D] image block with a [36, 4] angle
block and one row per candidate in numpy, stacks the batch and sends [B, 36, D+4] and [B, Cmax, D+4] to the device.  The
features are static, so `FeatureStore` keeps them on the device once and a step uploads indices and angles only: one pinned
record, one copy, one kernel (csrc/observations.hip, vt_obs_gather_f32) that writes all five tensors of the step.

    store = FeatureStore(feature_store["features"], device, view_angle_table=env.angle_feature)
    input_a_t, f_t, candidate_feat, candidate_leng = store.get_input_feat(perm_obs)     # agent.py:219-228
    candidate_mask = store.last_candidate_mask                                          # utils.length2mask(candidate_leng)

`view_features(slots, view_index)` is the turn-based task's `_feature_variable` (tasks/turn_based/agent.py:197-210): one
[D] row per agent.  A bad index (slot, view, candidate view, negative count) writes that agent's rows as zeros and raises
IndexError through `modeling.check_errors()`, as out-of-range embedding ids do; nothing outside the store is read.  The
gathers run on a HIP device only; there is no CPU fallback."""
import itertools
import math

import numpy as np
import torch

from . import ops

UPLOAD_CHUNK_BYTES = 256 << 20


def default_view_angle_table(V=36):
    """fp32 [V, V, 4] indexed [base view][view][sin h, cos h, sin e, cos e] with heading = (view % 12 - base % 12) * 30 deg and
    elevation = (view // 12 - 1) * 30 deg, computed in float64 and rounded once to fp32.

    The reference does not compute these numbers: utils.get_all_point_angle_feature() reads heading and elevation of every
    view from its simulator (utils.py:288-318), whose float arithmetic may differ from the closed form in the last bits.  A
    caller who wants the simulator's bits passes that table to FeatureStore(view_angle_table=...)."""
    t = np.empty((V, V, 4), dtype=np.float64)
    step = math.radians(30)
    for base in range(V):
        for view in range(V):
            h = (view % 12 - base % 12) * step
            e = (view // 12 - 1) * step
            t[base, view] = (math.sin(h), math.cos(h), math.sin(e), math.cos(e))
    return t.astype(np.float32)


def _int_vector(x, n, name):
    a = np.asarray(x)
    if a.shape != (n,):
        raise ValueError("%s must have shape (%d,), got %s" % (name, n, a.shape))
    if a.dtype.kind not in "iu":
        raise TypeError("%s must hold integers, got %s" % (name, a.dtype))
    if a.size and (a.max() > 0x7FFFFFFF or a.min() < -0x80000000):
        raise ValueError("%s does not fit int32" % name)
    return a


def _real_vector(x, n, name):
    a = np.asarray(x)
    if a.shape != (n,):
        raise ValueError("%s must have shape (%d,), got %s" % (name, n, a.shape))
    if a.dtype.kind not in "fiu":
        raise TypeError("%s must hold real numbers, got %s" % (name, a.dtype))
    return a


def _candidate_flat(x, counts, kinds, name):
    """The entries j < cand_count[b] of every agent, row after row, as one array.  x: a [B, >= max count] array, or a sequence
    of B per-agent sequences of at least cand_count[b] entries."""
    B = len(counts)
    keep = np.maximum(counts, 0)
    if isinstance(x, np.ndarray) and x.dtype != object:
        if x.ndim != 2 or x.shape[0] != B or x.shape[1] < int(keep.max()):
            raise ValueError("%s must be [%d, >= max(cand_count)], got %s" % (name, B, x.shape))
        flat = x[np.arange(x.shape[1])[None, :] < keep[:, None]]
    else:
        if len(x) != B:
            raise ValueError("%s must have %d rows, got %d" % (name, B, len(x)))
        try:
            lens = [len(r) for r in x]
        except TypeError:
            raise ValueError("%s must hold one sequence per agent" % name)
        want = keep.tolist()
        if lens != want:                      # longer rows are cut at the count; a shorter one is a mistake
            for b in range(B):
                if lens[b] < want[b]:
                    raise ValueError("%s[%d] must hold at least cand_count[%d] = %d entries" % (name, b, b, want[b]))
            x = [r[:n] for r, n in zip(x, want)]
        flat = np.array(list(itertools.chain.from_iterable(x))) if sum(want) else np.zeros(0, dtype=np.int64)
        if flat.ndim != 1:
            raise ValueError("%s must hold one number per candidate" % name)
    if flat.dtype.kind not in kinds:
        raise TypeError("%s: dtype %s not accepted" % (name, flat.dtype))
    return flat


def pack_record(buf, slots, view_index, heading, elevation, cand_point, cand_heading, cand_elevation, cand_count):
    """Writes one step's record into `buf` (a uint8 numpy array, 8-byte aligned, at least ops.obs_record_bytes(B, Cmax)[0]
    long) in the layout vt_obs_gather_f32 reads: int32 [B][3] slot / view_index / cand_count, int32 cand_point [B][Cmax],
    then float64 [B][2] heading / elevation, cand_heading [B][Cmax], cand_elevation [B][Cmax].  Entries at j >= cand_count[b]
    are zero.  Shape and dtype mistakes raise here, before anything is staged.  -> (B, Cmax, bytes)."""
    B = len(slots)
    if B < 1:
        raise ValueError("an empty batch")
    slots = _int_vector(slots, B, "slots")
    view_index = _int_vector(view_index, B, "view_index")
    cand_count = _int_vector(cand_count, B, "cand_count")
    heading = _real_vector(heading, B, "heading")
    elevation = _real_vector(elevation, B, "elevation")
    pts = _candidate_flat(cand_point, cand_count, "iu", "cand_point")
    chs = _candidate_flat(cand_heading, cand_count, "fiu", "cand_heading")
    ces = _candidate_flat(cand_elevation, cand_count, "fiu", "cand_elevation")
    Cmax = max(0, int(cand_count.max())) + 1
    nbytes, off = ops.obs_record_bytes(B, Cmax)
    if buf.dtype != np.uint8 or buf.ndim != 1 or buf.shape[0] < nbytes or buf.ctypes.data % 8:
        raise ValueError("the record buffer must be uint8, 8-byte aligned and hold %d bytes" % nbytes)
    rows = buf[:12 * B].view(np.int32).reshape(B, 3)
    rows[:, 0], rows[:, 1], rows[:, 2] = slots, view_index, cand_count
    p = buf[12 * B:12 * B + 4 * B * Cmax].view(np.int32).reshape(B, Cmax)
    f = buf[off:nbytes].view(np.float64)
    agent = f[:2 * B].reshape(B, 2)
    ch = f[2 * B:2 * B + B * Cmax].reshape(B, Cmax)
    ce = f[2 * B + B * Cmax:].reshape(B, Cmax)
    agent[:, 0], agent[:, 1] = heading, elevation
    p[:], ch[:], ce[:] = 0, 0.0, 0.0
    live = np.arange(Cmax)[None, :] < cand_count[:, None]
    p[live], ch[live], ce[live] = pts, chs, ces
    return B, Cmax, nbytes


def unpack_record(buf, B, Cmax):
    """The fields of a packed record as arrays (copies): slots, view_index, heading, elevation, cand_point, cand_heading,
    cand_elevation, cand_count -- the argument order of pack_record."""
    nbytes, off = ops.obs_record_bytes(B, Cmax)
    rows = buf[:12 * B].view(np.int32).reshape(B, 3).copy()
    p = buf[12 * B:12 * B + 4 * B * Cmax].view(np.int32).reshape(B, Cmax).copy()
    f = buf[off:nbytes].view(np.float64)
    agent = f[:2 * B].reshape(B, 2).copy()
    ch = f[2 * B:2 * B + B * Cmax].reshape(B, Cmax).copy()
    ce = f[2 * B + B * Cmax:].reshape(B, Cmax).copy()
    return rows[:, 0], rows[:, 1], agent[:, 0], agent[:, 1], p, ch, ce, rows[:, 2]


class _Stage(object):
    """Two pinned host buffers that alternate; each has an event recorded behind its copy and is rewritten only after that
    event has completed."""

    def __init__(self):
        self.bufs = [None, None]
        self.events = [None, None]
        self.turn = 0

    def acquire(self, nbytes):
        i = self.turn
        self.turn = 1 - i
        if self.events[i] is not None:
            self.events[i].synchronize()          # returns at once unless two steps are still in flight
        if self.bufs[i] is None or self.bufs[i].numel() < nbytes:
            self.bufs[i] = torch.empty(ops.round_up(max(nbytes, 4096), 4096), dtype=torch.uint8).pin_memory()
        return i, self.bufs[i]

    def upload(self, i, nbytes, device):
        dev = torch.empty(ops.round_up(nbytes, 16), dtype=torch.uint8, device=device)
        dev[:nbytes].copy_(self.bufs[i][:nbytes], non_blocking=True)
        if self.events[i] is None:
            self.events[i] = torch.cuda.Event()
        self.events[i].record()
        return dev


class FeatureStore(object):
    """Image features of every viewpoint as one fp32 device tensor [N, V, D], and the gathers that turn a step's indices into
    the decoder's input tensors.

    features: the reference's feature_store["features"] mapping ("<scan>_<viewpoint>" -> array [V, D]) or a pair
    (keys, array [N, V, D]).  Uploaded in chunks of at most 256 MB through a pinned buffer (no host copy of the whole set).
    view_angle_table: the caller's utils.get_all_point_angle_feature() as fp32 [V, V, 4]; default_view_angle_table() when
    omitted (see there for the difference)."""

    def __init__(self, features, device, view_angle_table=None):
        self.device = torch.device(device)
        if isinstance(features, (tuple, list)) and len(features) == 2 and not isinstance(features[1], str):
            keys, arr = features
            arr = arr if isinstance(arr, torch.Tensor) else np.asarray(arr)
            if arr.ndim != 3 or arr.shape[0] != len(keys):
                raise ValueError("features must be (keys, array [N, V, D]) with one key per slot")
            keys = list(keys)
            get = lambda lo, hi: arr[lo:hi]
            N, V, D = (int(s) for s in arr.shape)
        elif hasattr(features, "keys"):
            keys = list(features.keys())
            if not keys:
                raise ValueError("an empty feature mapping")
            first = np.asarray(features[keys[0]])
            if first.ndim != 2:
                raise ValueError("every feature must be [V, D], got %s" % (first.shape,))
            N, (V, D) = len(keys), (int(s) for s in first.shape)

            def get(lo, hi):
                rows = [np.asarray(features[k]) for k in keys[lo:hi]]
                for k, r in zip(keys[lo:hi], rows):
                    if r.shape != (V, D):
                        raise ValueError("feature %r is %s, the first one [%d, %d]" % (k, r.shape, V, D))
                return rows
        else:
            raise TypeError("features must be a mapping id -> [V, D] or a pair (keys, array [N, V, D])")
        if N < 1 or V < 1 or D < 1:
            raise ValueError("features must be [N >= 1, V >= 1, D >= 1]")
        self._slots = {k: i for i, k in enumerate(keys)}
        if len(self._slots) != N:
            raise ValueError("duplicate ids in the feature keys")
        self.N, self.V, self.D = N, V, D
        self.features = torch.empty((N, V, D), dtype=torch.float32, device=self.device)
        self._upload(get)
        table = default_view_angle_table(V) if view_angle_table is None else np.asarray(view_angle_table)
        if table.shape != (V, V, 4):
            raise ValueError("view_angle_table must be [%d, %d, 4], got %s" % (V, V, table.shape))
        if table.dtype != np.float32:
            raise TypeError("view_angle_table must be float32, got %s" % table.dtype)
        self.view_angle_table = torch.from_numpy(np.ascontiguousarray(table)).to(self.device)
        self._stage = _Stage()
        self.last_candidate_mask = None

    def _upload(self, get):
        N, V, D = self.N, self.V, self.D
        per = max(1, UPLOAD_CHUNK_BYTES // (4 * V * D))
        pinned = torch.empty((min(per, N), V, D), dtype=torch.float32)
        if self.device.type == "cuda":
            pinned = pinned.pin_memory()
        view = pinned.numpy()
        for lo in range(0, N, per):
            hi = min(N, lo + per)
            chunk = get(lo, hi)
            if isinstance(chunk, torch.Tensor):
                pinned[:hi - lo].copy_(chunk)
            elif isinstance(chunk, list):
                for i, r in enumerate(chunk):
                    view[i] = r
            else:
                view[:hi - lo] = chunk
            self.features[lo:hi].copy_(pinned[:hi - lo], non_blocking=True)
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()      # the buffer is refilled next

    @property
    def nbytes(self):
        return self.features.numel() * 4

    def slot(self, long_id):
        """The store row of "<scan>_<viewpoint>"; KeyError for an id the store does not hold."""
        return self._slots[long_id]

    def __len__(self):
        return self.N

    # ---- the panoramic step -------------------------------------------------------------------------------------------
    def step_inputs(self, slots, view_index, heading, elevation, cand_point, cand_heading, cand_elevation, cand_count):
        """-> (input_a_t [B, 4], f_t [B, V, D+4], candidate_feat [B, Cmax, D+4], candidate_leng list, candidate_mask bool
        [B, Cmax]) with the reference's semantics:

          f_t[b, v]            = [store[slots[b], v, :] | view_angle_table[view_index[b], v, :]]
          candidate_feat[b, j] = [store[slots[b], cand_point[b][j], :] | sin, cos of cand_heading[b][j], cand_elevation[b][j]]
                                 for j < cand_count[b], zero for j >= cand_count[b] (the END row and the padding)
          candidate_leng[b]    = cand_count[b] + 1, Cmax = max(candidate_leng)
          candidate_mask       = utils.length2mask(candidate_leng): j > candidate_leng[b] - 1
          input_a_t[b]         = sin, cos of heading[b], elevation[b]

        All arguments are host sequences or numpy arrays: integers for slots, view_index, cand_point, cand_count; real numbers
        for the angles; cand_* either [B, >= max count] arrays or one sequence per agent.  They travel in one pinned record
        and one non-blocking copy; the angles are evaluated on the device in float64 and rounded once."""
        nbytes = ops.obs_record_bytes(len(slots), self._cmax_hint(cand_count))[0]
        if not self.features.is_cuda:   # the host-side checks still come first; then the refusal
            pack_record(np.zeros(nbytes, dtype=np.uint8), slots, view_index, heading, elevation, cand_point, cand_heading,
                        cand_elevation, cand_count)
            ops._require_hip(self.features)
        with torch.cuda.device(self.device):
            i, host = self._stage.acquire(nbytes)
            B, Cmax, nbytes = pack_record(host.numpy(), slots, view_index, heading, elevation, cand_point, cand_heading,
                                          cand_elevation, cand_count)
            record = self._stage.upload(i, nbytes, self.device)
            err = torch.zeros(1, dtype=torch.int32, device=self.device)
            a_t, f_t, cand, _, mask = ops.obs_gather(self.features, self.view_angle_table, record, B, Cmax, err_flag=err)
            _post_flag(err)
        leng = [max(int(c), 0) + 1 for c in np.asarray(cand_count)]   # known on the host: no read-back of the device copy
        self.last_candidate_mask = mask
        return a_t, f_t, cand, leng, mask

    @staticmethod
    def _cmax_hint(cand_count):
        c = np.asarray(cand_count)
        if c.ndim != 1 or c.size < 1 or c.dtype.kind not in "iu":
            raise ValueError("cand_count must be a non-empty vector of integers")
        return max(0, int(c.max())) + 1

    def obs_fields(self, obs):
        """The eight step_inputs arguments of a list of the reference's observations.  Reads `scan`, `viewpoint`, `viewIndex`,
        `heading`, `elevation` of each ob and `pointId`, `heading`, `elevation` of each ob["candidate"] entry; never
        `feature`."""
        slots = [self.slot("%s_%s" % (ob["scan"], ob["viewpoint"])) for ob in obs]
        view_index = [int(ob["viewIndex"]) for ob in obs]
        heading = [float(ob["heading"]) for ob in obs]
        elevation = [float(ob["elevation"]) for ob in obs]
        cands = [ob["candidate"] for ob in obs]
        cand_point = [[int(c["pointId"]) for c in cs] for cs in cands]
        cand_heading = [[float(c["heading"]) for c in cs] for cs in cands]
        cand_elevation = [[float(c["elevation"]) for c in cs] for cs in cands]
        return slots, view_index, heading, elevation, cand_point, cand_heading, cand_elevation, [len(cs) for cs in cands]

    def get_input_feat(self, obs):
        """Drop-in for Agent.get_input_feat(perm_obs) (agent.py:219-228) -> (input_a_t, f_t, candidate_feat, candidate_leng);
        the mask of the same step is `last_candidate_mask`."""
        return self.step_inputs(*self.obs_fields(obs))[:4]

    # ---- the turn-based step ------------------------------------------------------------------------------------------
    def view_features(self, slots, view_index):
        """fp32 [B, D]: store[slots[b], view_index[b], :], the turn-based task's _feature_variable."""
        B = len(slots)
        if B < 1:
            raise ValueError("an empty batch")
        s, v = _int_vector(slots, B, "slots"), _int_vector(view_index, B, "view_index")
        ops._require_hip(self.features)
        with torch.cuda.device(self.device):
            i, host = self._stage.acquire(8 * B)
            rows = host.numpy()[:8 * B].view(np.int32).reshape(B, 2)
            rows[:, 0], rows[:, 1] = s, v
            record = self._stage.upload(i, 8 * B, self.device)
            err = torch.zeros(1, dtype=torch.int32, device=self.device)
            out = ops.obs_gather_view(self.features, record.view(torch.int32), B, err_flag=err)
            _post_flag(err)
        return out


def _post_flag(err):
    from .turn_based import _post_flag as post

    post(err)
