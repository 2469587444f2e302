"""Pretraining's region features, served from a region store on the device.

The reference builds every pretraining item's image input on the host (tasks/viewpoint_select/data_loader_pretrain.py:
615-634): `_extract_img_features` reads the 36 records "<scan>_<viewpoint>_<idx>" of the item's viewpoint, cuts each to its
first 5 rows and concatenates them into up to 180 rows of D floats; the tail of `_preprocess_item` (:654-712) then keeps the
last `max_img_seq_length` rows or zero-pads, looks up the location embeddings and extends labels and attention mask.  A
loader that feeds the engine that way moves B * R_in * D * 4 bytes per batch (378 MB at B = 256, R_in = 180, D = 2054).

The features are static, so `RegionStore` keeps them on the device once -- features [N, 36, P, ld], ld = round_up(D, 8), and
counts uint8 [N, 36] -- and a batch uploads one small pinned record of slots and view indices; one kernel
(csrc/regions.hip) writes the batch's tensors, either as `data.assemble_batch` returns them or, with packed=True, as the
bf16 operand of the region-projection GEMM itself (what `ops.pack_concat` would make of them), which `PretrainEngine` and
the module forwards take as `img_packed`:

    store = RegionStore(features_reader, device)                       # once
    batch = store.pretrain_batch(slots, current_view_index, input_ids, labels, text_attention_mask, next_action,
                                 max_img_seq_length, token_classes=token_classes, packed=True)
    loss = model(**batch)[0]

A slot or view index out of range (or a corrupted count) writes that item's region rows as zeros with mask 0 and raises
IndexError through `modeling.check_errors()`, as out-of-range embedding ids do; nothing outside the store is read.  The
gather runs on a HIP device only; there is no CPU fallback."""
import numpy as np
import torch

from . import ops
from .data import loc_embedding_table
from .observations import UPLOAD_CHUNK_BYTES, _int_vector, _post_flag, _Stage

VIEWS = 36


def _text(k):
    return k.decode() if isinstance(k, (bytes, bytearray)) else k


class RegionStore(object):
    """Region features of every viewpoint on the device: features [N, 36, P, ld] (ld = round_up(D, 8), the padding zero) and
    counts uint8 [N, 36], the rows each view really has.

    features: the reference's features_reader form, a mapping "<scan>_<viewpoint>_<idx>" (str or bytes keys, idx 0..35) ->
    array [n, D] of which the first `per_view` rows are kept (n may be 0); or a triple (keys, array [N, 36, P, D], counts
    [N, 36]) with keys "<scan>_<viewpoint>".  Uploaded in chunks of at most 256 MB through one pinned buffer: there is never
    a host copy of the whole set.

    dtype: torch.bfloat16 (default) holds the bf16 engine's operand precision, rounded once to nearest even as
    pack_concat_bf16 rounds; torch.float32 holds the features exactly, for the fp32 engine and for parity work.

    Memory: N * 36 * P * ld * itemsize bytes.  At N = 10 000 viewpoints, P = 5, D = 2054 (ld = 2056): 10 000 * 36 * 5 * 2056 *
    2 = 7.4 GB in bf16, 14.8 GB in fp32."""

    def __init__(self, features, device, per_view=5, dtype=torch.bfloat16):
        self.device = torch.device(device)
        if dtype not in (torch.bfloat16, torch.float32):
            raise TypeError("dtype must be torch.bfloat16 or torch.float32, got %s" % (dtype,))
        P = int(per_view)
        if P < 1 or P > 255:
            raise ValueError("per_view must be 1..255, got %r" % (per_view,))
        if isinstance(features, (tuple, list)) and len(features) == 3:
            keys, arr, cnt = features
            keys = [_text(k) for k in keys]
            arr = arr if isinstance(arr, torch.Tensor) else np.asarray(arr)
            cnt = np.asarray(cnt.cpu() if isinstance(cnt, torch.Tensor) else cnt)
            if arr.ndim != 4 or arr.shape[0] != len(keys) or arr.shape[1] != VIEWS or arr.shape[2] != P:
                raise ValueError("features must be (keys, array [N, 36, per_view, D], counts [N, 36]) with one key per slot, "
                                 "got array %s" % (tuple(arr.shape),))
            if cnt.shape != (len(keys), VIEWS) or cnt.dtype.kind not in "iu":
                raise ValueError("counts must be integers [N, 36], got %s %s" % (cnt.dtype, cnt.shape))
            if cnt.size and (cnt.min() < 0 or cnt.max() > P):
                raise ValueError("counts must lie in 0..per_view")
            N, D = int(arr.shape[0]), int(arr.shape[3])
            counts = cnt.astype(np.uint8)

            def fill(view, lo, hi):
                view[:hi - lo] = arr[lo:hi].numpy() if isinstance(arr, torch.Tensor) else arr[lo:hi]
        elif hasattr(features, "keys"):
            by_id, order = {}, []
            for k in features.keys():
                long_id, _, idx = _text(k).rpartition("_")
                if not long_id or not idx.isdigit() or int(idx) >= VIEWS:
                    raise ValueError("feature key %r is not '<scan>_<viewpoint>_<idx>' with idx 0..35" % (k,))
                if long_id not in by_id:
                    by_id[long_id] = [None] * VIEWS
                    order.append(long_id)
                if by_id[long_id][int(idx)] is not None:
                    raise ValueError("duplicate ids in the feature keys: %r" % (k,))
                by_id[long_id][int(idx)] = k
            if not order:
                raise ValueError("an empty feature mapping")
            for long_id in order:
                if None in by_id[long_id]:
                    raise ValueError("viewpoint %r lacks view %d" % (long_id, by_id[long_id].index(None)))
            keys, N = order, len(order)
            D = None
            for k in by_id[order[0]]:
                first = np.asarray(features[k])
                if first.ndim != 2:
                    raise ValueError("every feature must be [n, D], got %s for %r" % (first.shape, k))
                D = int(first.shape[1])
                break
            counts = np.zeros((N, VIEWS), dtype=np.uint8)

            def fill(view, lo, hi):
                view[:hi - lo] = 0.0
                for i in range(lo, hi):
                    for v, k in enumerate(by_id[keys[i]]):
                        r = np.asarray(features[k])
                        if r.ndim != 2 or r.shape[1] != D:
                            raise ValueError("feature %r is %s, the first one [n, %d]" % (k, r.shape, D))
                        if r.dtype.kind not in "fiu":
                            raise TypeError("feature %r holds %s" % (k, r.dtype))
                        n = min(int(r.shape[0]), P)
                        view[i - lo, v, :n] = r[:n]
                        counts[i, v] = n
        else:
            raise TypeError("features must be a mapping '<scan>_<viewpoint>_<idx>' -> [n, D] or a triple "
                            "(keys, array [N, 36, per_view, D], counts [N, 36])")
        if N < 1 or D < 1:
            raise ValueError("features must be [N >= 1, 36, per_view, D >= 1]")
        self._slots = {k: i for i, k in enumerate(keys)}
        if len(self._slots) != N:
            raise ValueError("duplicate ids in the feature keys")
        self.N, self.V, self.P, self.D, self.ld, self.dtype = N, VIEWS, P, D, ops.round_up(D, 8), dtype
        self.features = torch.zeros((N, VIEWS, P, self.ld), dtype=dtype, device=self.device)
        self._upload(fill)
        self.counts = torch.from_numpy(counts).to(self.device)
        self.loc_table = loc_embedding_table(self.device)
        self._stage = _Stage()

    def _upload(self, fill):
        N, V, P, D = self.N, self.V, self.P, self.D
        per = max(1, UPLOAD_CHUNK_BYTES // (4 * V * P * D))
        pinned = torch.empty((min(per, N), V, P, D), dtype=torch.float32)
        if self.device.type == "cuda":
            pinned = pinned.pin_memory()
        view = pinned.numpy()
        for lo in range(0, N, per):
            hi = min(N, lo + per)
            fill(view, lo, hi)
            chunk = pinned[:hi - lo].to(self.device, non_blocking=True)
            self.features[lo:hi, :, :, :D].copy_(chunk)              # the one rounding of a bf16 store (to nearest even)
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()      # the buffer is refilled next

    @property
    def nbytes(self):
        return self.N * self.V * self.P * self.ld * self.features.element_size()

    def slot(self, scan, viewpoint):
        """The store row of viewpoint `viewpoint` of `scan`; KeyError for an id the store does not hold."""
        return self._slots["%s_%s" % (_text(scan), _text(viewpoint))]

    def __len__(self):
        return self.N

    def pretrain_batch(self, slots, current_view_index, input_ids, labels, text_attention_mask, next_action,
                       max_img_seq_length, token_classes=None, no_action_grounding=False, packed=False):
        """_extract_img_features plus the tail of _preprocess_item (data_loader_pretrain.py:615-634, 654-712) for a batch.
        slots, current_view_index: host sequences of B integers (slot() of every item's viewpoint, its current view); the
        other arguments as data.assemble_batch takes them (tensors; moved to the store's device if they are not there).

        Item b's rows are the stored rows of views 0..35 in order, counts[slot_b, v] per view; more than R =
        max_img_seq_length keep the LAST R, fewer are zero-padded with attention mask 0; a kept row's location embedding is
        _static_loc_embeddings[current_view_index_b][its absolute view]; labels and token labels get -1 on every region
        position.  -> the dict data.assemble_batch returns (img_feats fp32 [B, R, D]: a bf16 store's values widened), or with
        packed=True the same without img_feats / img_location_embeddings and with img_packed bf16 [B * R, kpad], kpad =
        round_up(D + 128, 64), rows [features | location | zeros], and img_rows = R.

        One pinned record and one copy travel per call; nothing synchronises with the host."""
        B = len(slots)
        if B < 1:
            raise ValueError("an empty batch")
        s = _int_vector(slots, B, "slots")
        v = _int_vector(current_view_index, B, "current_view_index")
        R = int(max_img_seq_length)
        if R < 0:
            raise ValueError("max_img_seq_length must not be negative")
        if tuple(input_ids.shape[:1]) != (B,) or input_ids.dim() != 2:
            raise ValueError("input_ids must be [%d, T], got %s" % (B, tuple(input_ids.shape)))
        T = int(input_ids.shape[1])
        for name, t in (("labels", labels), ("text_attention_mask", text_attention_mask), ("token_classes", token_classes)):
            if t is not None and tuple(t.shape) != (B, T):
                raise ValueError("%s must be [%d, %d], got %s" % (name, B, T, tuple(t.shape)))
        ops._require_hip(self.features)
        dev = self.device
        i64 = lambda t: None if t is None else t.to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
        with torch.cuda.device(dev):
            i, host = self._stage.acquire(8 * B)
            rec = host.numpy()[:8 * B].view(np.int32).reshape(B, 2)
            rec[:, 0], rec[:, 1] = s, v
            rows = self._stage.upload(i, 8 * B, dev)[:8 * B].view(torch.int32).view(B, 2)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            out = ops.region_gather(self.features, self.counts, self.loc_table, rows, self.D, i64(labels),
                                    i64(text_attention_mask), i64(token_classes), R,
                                    kpad=ops.round_up(self.D + 128, 64) if packed else None, err_flag=err)
            _post_flag(err)
        next_action = next_action.to(dev, non_blocking=True)
        batch = dict(input_ids=input_ids.to(dev, non_blocking=True), labels=out[-3], attention_mask=out[-2])
        if packed:
            batch.update(img_packed=out[0], img_rows=R)
        else:
            batch.update(img_feats=out[0], img_location_embeddings=out[1])
        batch.update(next_action=torch.full_like(next_action, -1) if no_action_grounding else next_action, token_labels=out[-1])
        return batch
