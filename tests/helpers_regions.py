"""Shared by tests/test_host_regions.py and tests/test_gpu_regions.py: a synthetic region-feature mapping in the reference's
form, the per-item expectation (the reference's loop of data_loader_pretrain.py:615-634 -- views 0..35, first P rows,
concatenate -- fed into oracle.data.preprocess_item_tail, which tests/golden/ref_data.npz pins to the reference's own
_preprocess_item), and a numpy restatement of the row map csrc/regions.hip implements, with a table of wrong variants.

Shapes: N = 6 viewpoints, 36 views, P = 5, B = 5, T = 9.  Five items cannot hold six roles (n = 0, 0 < n < R, n == R, a cut
in the middle of a view, a cut on a view boundary, one slot twice), so every (D, R) has two batches of five over the same
six viewpoints: "lengths" = slots 0..4, one role each, and "twice" = slot 5 twice under different current views beside three
of the others.  At R = 180 no item can have more rows than R (36 * 5 = 180): the two cut roles do not exist there.

R = 0: the reference's own slice is degenerate there (x[-0:] is all of x: an item with regions keeps them all and its
tensors no longer collate); the expectation at R = 0 is the text part alone, the oracle fed zero region rows."""
import numpy as np
import torch

from oracle import data as odata

N, V, P, B, T = 6, 36, 5, 5, 9
DS = (2054, 16, 10)          # the shipped width; a multiple of 8; seam and zero tail inside the first pieces
RS = (12, 40, 180, 0)
MAX_RAW = P + 2              # some records hold more rows than the [:P] cut keeps
PATTERN = (5, 0, 3, 5, 1, 5, 2, 4, 0, 5, 5, 3)   # rows per view, cycled: running sums 0 5 5 8 13 14 19 21 25 25 30 35 38
MID_CUT, EDGE_CUT = 7, 8     # 7 rows in: inside view 2 (rows 5..7); 8 rows in: the first row of view 3
BATCHES = {"lengths": ((0, 1, 2, 3, 4), (0, 7, 35, 13, 24)), "twice": ((5, 3, 5, 1, 2), (11, 13, 30, 0, 12))}


def kpad_of(D):
    return (D + 128 + 63) // 64 * 64


def _take(n, shift):
    """36 per-view counts that sum to n: the pattern from `shift` on, raised towards P from view 0 up or emptied from view
    35 down until the sum fits (the head of the pattern, where the cuts fall, stays as it is for n >= 13)."""
    c = [PATTERN[(v + shift) % len(PATTERN)] for v in range(V)]
    v = 0
    while sum(c) < n:
        c[v] = min(P, c[v] + n - sum(c))
        v += 1
    v = V - 1
    while sum(c) > n:
        c[v] = max(0, c[v] - (sum(c) - n))
        v -= 1
    return c


def counts_for(R):
    """uint8 [N, 36] after the [:P] cut.  Slot: 0 n = 0; 1 0 < n < R; 2 n == R; 3 n = R + 7 (cut inside view 2); 4 n = R + 8 (cut
    on the edge of view 3); 5 n = R + 30 under a shifted pattern -- the last three capped at 180 rows."""
    cap = V * P
    ns = (0, R // 2, R, min(R + MID_CUT, cap), min(R + EDGE_CUT, cap), min(R + 30, cap))
    return np.array([_take(n, 5 if i == 5 else 0) for i, n in enumerate(ns)], dtype=np.uint8)


def raw_counts_for(R):
    """Rows the records hold before the cut: two more than P in every other full view."""
    c = counts_for(R).astype(np.int64)
    extra = ((np.arange(N)[:, None] + np.arange(V)[None, :]) % 2 == 0) & (c == P)
    return c + 2 * extra


def long_id(i):
    return "s%d_v%02d" % (i, i)


_base = {}


def base_features(D):
    if D not in _base:
        rng = np.random.default_rng(1000 + D)
        _base[D] = rng.standard_normal((N, V, MAX_RAW, D)).astype(np.float32)
    return _base[D]


def mapping_for(D, R, bytes_keys=False):
    """{"<scan>_<viewpoint>_<idx>": array [n, D]}, n = raw_counts_for(R)."""
    feats, raw = base_features(D), raw_counts_for(R)
    out = {}
    for i in range(N):
        for v in range(V):
            k = "%s_%d" % (long_id(i), v)
            out[k.encode() if bytes_keys else k] = feats[i, v, :raw[i, v]]
    return out


def triple_for(D, R):
    """(keys, array [N, 36, P, D], counts) of the same features; rows a view does not have are NaN."""
    arr = base_features(D)[:, :, :P].copy()
    counts = counts_for(R)
    arr[np.arange(P)[None, None, :] >= counts[:, :, None]] = np.nan
    return [long_id(i) for i in range(N)], arr, counts


_text = {}


def text_tensors():
    """input_ids, labels, text attention mask, token classes [B, T] int64 and next_action [B]."""
    if not _text:
        g = torch.Generator().manual_seed(77)
        ids = torch.randint(5, 500, (B, T), generator=g)
        att = torch.ones(B, T, dtype=torch.long)
        for b in range(B):
            att[b, T - b:] = 0
            ids[b, T - b:] = 0
        real = att == 1          # (supervised positions are real tokens: a training step may then drop the padded rows)
        labels = torch.where((torch.rand(B, T, generator=g) < 0.3) & real, ids, torch.full_like(ids, -1))
        tok = torch.where((torch.rand(B, T, generator=g) < 0.3) & real, torch.randint(0, 40, (B, T), generator=g),
                          torch.full_like(ids, -1))
        _text.update(input_ids=ids, labels=labels, att=att, token_classes=tok, next_action=torch.randint(0, 36, (B,), generator=g))
    return _text


_expect = {}


def expectation(D, R, batch, token_classes=True, no_action_grounding=False, rounded=False):
    """The oracle's tensors of one batch, stacked (cached; do not modify).  rounded: the features through bf16 first."""
    key = (D, R, batch, token_classes, no_action_grounding, rounded)
    if key in _expect:
        return _expect[key]
    mapping, tx = mapping_for(D, R), text_tensors()
    slots, curs = BATCHES[batch]
    items = []
    for b in range(B):
        feats = [mapping["%s_%d" % (long_id(slots[b]), v)][:P] for v in range(V)]   # data_loader_pretrain.py:619-626
        view_ids = [v for v in range(V) for _ in range(len(feats[v]))]
        img = np.concatenate(feats, axis=0)
        if rounded:
            img = torch.from_numpy(img).to(torch.bfloat16).float().numpy()
        if R == 0:
            img, view_ids = img[:0], []
        items.append(odata.preprocess_item_tail(tx["input_ids"][b], tx["labels"][b], tx["att"][b], img, view_ids, curs[b],
                                                int(tx["next_action"][b]), R,
                                                token_classes=tx["token_classes"][b] if token_classes else None,
                                                no_action_grounding=no_action_grounding))
    out = dict(input_ids=torch.stack([it["input_ids"] for it in items]),
               labels=torch.stack([it["labels"] for it in items]),
               attention_mask=torch.stack([it["attention_mask"].long() for it in items]),
               img_feats=torch.stack([it["img_feats"] for it in items]),
               img_location_embeddings=torch.stack([it["img_location_embeddings"] for it in items]),
               next_action=torch.tensor([it["next_action"] for it in items]),
               token_labels=torch.stack([it["token_labels"] for it in items]) if token_classes else None)
    _expect[key] = out
    return out


def packed_of(exp, D):
    """fp32 [B * R, kpad]: [features | location | zeros] of an expectation."""
    R = exp["img_feats"].shape[1]
    out = torch.zeros(B * R, kpad_of(D))
    out[:, :D] = exp["img_feats"].reshape(B * R, D)
    out[:, D:D + 128] = exp["img_location_embeddings"].reshape(B * R, 128)
    return out


# ---- the row map of csrc/regions.hip in numpy, and what it must not be -------------------------------------------------------
WRONG = ("first_R", "truncate_before_cut", "loc_by_position", "loc_transposed", "pad_mask_1", "labels_0", "off_by_one",
         "tail_unwritten")
SENTINEL = -12345.0
LOC = np.stack(odata.STATIC)     # [current view][absolute view][128]


def restate(D, R, batch, wrong=None):
    """Item b, output row r: region j = start + r of the concatenation of the views' first min(n_v, P) rows, start =
    max(n - R, 0); valid where j < n; its view = how many running sums are <= j."""
    assert wrong is None or wrong in WRONG
    mapping, tx = mapping_for(D, R), text_tensors()
    slots, curs = BATCHES[batch]
    kpad = kpad_of(D)
    feats = np.zeros((B, R, D), np.float32)
    loc = np.zeros((B, R, 128), np.float32)
    mask = np.zeros((B, T + R), np.int64)
    labels = np.full((B, T + R), 0 if wrong == "labels_0" else -1, np.int64)
    tok = np.full((B, T + R), -1, np.int64)
    packed = np.full((B * R, kpad), SENTINEL, np.float32)
    for b in range(B):
        rows = [mapping["%s_%d" % (long_id(slots[b]), v)] for v in range(V)]
        raw = np.array([len(x) for x in rows])
        c = np.minimum(raw, P)
        pre = np.concatenate([[0], np.cumsum(c)])
        n = int(pre[V])
        start = max((int(raw.sum()) if wrong == "truncate_before_cut" else n) - R, 0)
        if wrong == "first_R":
            start = 0
        if wrong == "off_by_one" and n == R and R > 0:
            start = 1
        labels[b, :T], mask[b, :T], tok[b, :T] = tx["labels"][b].numpy(), tx["att"][b].numpy(), tx["token_classes"][b].numpy()
        for r in range(R):
            j = start + r
            if j < n:
                v = int(np.sum(pre[1:] <= j))
                feats[b, r] = rows[v][j - pre[v]]
                lv = r % V if wrong == "loc_by_position" else v
                loc[b, r] = LOC[lv][curs[b]] if wrong == "loc_transposed" else LOC[curs[b]][lv]
                mask[b, T + r] = 1
            elif wrong == "pad_mask_1":
                mask[b, T + r] = 1
            row = packed[b * R + r]
            row[:D], row[D:D + 128] = feats[b, r], loc[b, r]
            if wrong != "tail_unwritten":
                row[D + 128:] = 0.0
    return dict(img_feats=feats, img_location_embeddings=loc, attention_mask=mask, labels=labels, token_labels=tok,
                packed=packed)


def agrees(D, R, batch, wrong=None):
    """Whether the restatement gives the oracle's tensors (and the packed rows made of them) exactly."""
    got, exp = restate(D, R, batch, wrong), expectation(D, R, batch)
    same = all(np.array_equal(got[k], exp[k].numpy()) for k in ("img_feats", "img_location_embeddings", "attention_mask",
                                                                 "labels", "token_labels"))
    return same and np.array_equal(got["packed"], packed_of(exp, D).numpy())
