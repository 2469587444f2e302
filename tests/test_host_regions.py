"""CPU: the region store's host side (visitron_amd/regions.py) -- construction from the reference's mapping form and from the
triple, the [:P] cut, slot lookup, the errors -- and the row map of csrc/regions.hip restated in numpy
(tests/helpers_regions.py) against the oracle expectation, with a table of wrong row maps that the cases must reject."""
import numpy as np
import pytest
import torch

import helpers_regions as hr
from visitron_amd import RegionStore

D, R = 10, 12


def _stored(store):
    return store.features[..., :store.D].float().numpy(), store.counts.numpy()


@pytest.mark.parametrize("bytes_keys", [False, True])
def test_mapping_form_keeps_the_first_rows_of_every_view(bytes_keys):
    mapping = hr.mapping_for(D, R, bytes_keys=bytes_keys)
    store = RegionStore(mapping, "cpu", dtype=torch.float32)
    arr, counts = _stored(store)
    raw = hr.raw_counts_for(R)
    assert (raw > hr.P).any() and (raw == 0).any() and ((raw > 0) & (raw < hr.P)).any()   # the cut, empty and short views
    assert len(store) == hr.N and store.features.shape == (hr.N, 36, hr.P, 16) and store.features.dtype == torch.float32
    assert np.array_equal(counts, hr.counts_for(R)) and counts.dtype == np.uint8
    assert store.nbytes == hr.N * 36 * hr.P * 16 * 4
    base = hr.base_features(D)
    for i in range(hr.N):
        assert store.slot("s%d" % i, "v%02d" % i) == i
        assert store.slot(b"s%d" % i, "v%02d" % i) == i
        for v in range(36):
            n = counts[i, v]
            assert np.array_equal(arr[i, v, :n], base[i, v, :n]) and not arr[i, v, n:].any()
    assert not store.features[..., D:].any()                     # the padding up to ld
    with pytest.raises(KeyError):
        store.slot("s0", "v01")


def test_triple_form_and_bf16_default():
    keys, arr, counts = hr.triple_for(D, R)
    store = RegionStore((keys, arr, counts), "cpu")
    assert store.features.dtype == torch.bfloat16 and store.nbytes == hr.N * 36 * hr.P * 16 * 2
    want = torch.from_numpy(arr).to(torch.bfloat16)
    assert torch.equal(torch.nan_to_num(store.features[..., :D]), torch.nan_to_num(want))
    assert np.array_equal(store.counts.numpy(), counts) and store.slot("s3", "v03") == 3
    exact = RegionStore((keys, torch.from_numpy(arr), torch.from_numpy(counts)), "cpu", dtype=torch.float32)
    assert torch.equal(torch.nan_to_num(exact.features[..., :D]), torch.nan_to_num(torch.from_numpy(arr)))


def test_construction_errors():
    keys, arr, counts = hr.triple_for(D, R)
    with pytest.raises(ValueError, match="duplicate"):
        RegionStore(([keys[0]] + keys[:-1], arr, counts), "cpu")
    both = hr.mapping_for(D, R)
    both[b"s0_v00_3"] = both["s0_v00_3"]                        # one record under a str and a bytes key
    with pytest.raises(ValueError, match="duplicate"):
        RegionStore(both, "cpu")
    with pytest.raises(ValueError):
        RegionStore((keys, arr[:, :, :4], counts), "cpu")        # per_view rows expected
    with pytest.raises(ValueError):
        RegionStore((keys, arr, counts[:, :35]), "cpu")
    with pytest.raises(ValueError):
        RegionStore((keys, arr, counts + 1), "cpu")              # a count above per_view
    with pytest.raises(ValueError):
        RegionStore((keys, arr, counts.astype(np.float32)), "cpu")
    with pytest.raises(TypeError):
        RegionStore((keys, arr, counts), "cpu", dtype=torch.float16)
    with pytest.raises(TypeError):
        RegionStore(arr, "cpu")
    with pytest.raises(ValueError):
        RegionStore({}, "cpu")
    lacking = hr.mapping_for(D, R)
    del lacking["s2_v02_17"]
    with pytest.raises(ValueError, match="lacks view 17"):
        RegionStore(lacking, "cpu")
    ragged = hr.mapping_for(D, R)
    ragged["s1_v01_0"] = np.zeros((2, D + 1), np.float32)
    with pytest.raises(ValueError):
        RegionStore(ragged, "cpu")
    with pytest.raises(ValueError):
        RegionStore({"nounderscore": np.zeros((1, D), np.float32)}, "cpu")


def test_a_host_store_refuses_to_gather():
    store = RegionStore(hr.triple_for(D, R), "cpu")
    tx = hr.text_tensors()
    with pytest.raises(ValueError):
        store.pretrain_batch([0, 1], [0], tx["input_ids"][:2], tx["labels"][:2], tx["att"][:2], tx["next_action"][:2], R)
    with pytest.raises(RuntimeError, match="HIP device only"):
        store.pretrain_batch(*hr.BATCHES["lengths"], tx["input_ids"], tx["labels"], tx["att"], tx["next_action"], R)


def test_location_table_is_the_oracles_bit_for_bit():
    from visitron_amd.data import loc_embedding_table

    assert np.array_equal(loc_embedding_table().numpy(), hr.LOC)


def test_the_case_table_holds_every_role():
    for R_ in hr.RS:
        c = hr.counts_for(R_).astype(np.int64)
        n = c.sum(1)
        pre = np.concatenate([np.zeros((hr.N, 1), np.int64), np.cumsum(c, 1)], 1)
        assert n[0] == 0 and n[2] == R_ and (R_ == 0 or 0 < n[1] < R_)
        assert (c == 0).any() and ((c > 0) & (c < hr.P)).any()
        if 0 < R_ < 180:                                         # (R = 0 keeps no row; R = 180 is every row there can be)
            assert n[3] > R_ and (n[3] - R_) not in pre[3]       # the cut falls inside a view
            assert n[4] > R_ and (n[4] - R_) in pre[4][1:]       # the cut falls on a view's first row
    slots = hr.BATCHES["twice"][0]
    assert len(slots) == hr.B == len(hr.BATCHES["lengths"][0]) and len(set(slots)) < hr.B


@pytest.mark.parametrize("batch", sorted(hr.BATCHES))
@pytest.mark.parametrize("R_", hr.RS)
def test_row_map_restatement_agrees_with_the_oracle(R_, batch):
    assert hr.agrees(D, R_, batch)


# wrong row map -> one case (R, batch) that rejects it
REJECTED_BY = {
    "first_R": (12, "lengths"),               # slots 3 and 4 hold more than R rows
    "truncate_before_cut": (12, "lengths"),   # slot 3: n = 19 > R of 23 rows before the cut
    "loc_by_position": (40, "lengths"),       # view 1 is empty: row 5 belongs to view 2
    "loc_transposed": (12, "twice"),
    "pad_mask_1": (40, "lengths"),            # slots 0 and 1 are padded
    "labels_0": (12, "lengths"),
    "off_by_one": (180, "lengths"),           # slot 2: n == R
    "tail_unwritten": (12, "twice"),          # kpad = 192 > 10 + 128
}


@pytest.mark.parametrize("wrong", hr.WRONG)
def test_wrong_row_maps_are_rejected(wrong):
    R_, batch = REJECTED_BY[wrong]
    assert not hr.agrees(D, R_, batch, wrong=wrong), "%s passes R = %d, batch %r" % (wrong, R_, batch)
