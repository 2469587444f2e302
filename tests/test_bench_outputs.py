"""bench.py's --dump-outputs and --full: the helpers that write the timed step's outputs (CPU), and plain / --full runs
of the bench on small shapes (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

SIDE_FIELDS = ("value_all_padded_rows_computed", "fwd_samples_per_sec", "fwd_b64", "b36", "collective", "roofline", "hbm",
               "cpu_baseline", "kernels_ms_per_step")


def test_fixed_sample_is_the_same_positions_in_every_call():
    t = torch.arange(1000, dtype=torch.float32)
    a, b = bench.fixed_sample(t, 64, 5), bench.fixed_sample(t.clone(), 64, 5)
    assert a.shape == (64,) and torch.equal(a, b)
    assert not torch.equal(a, bench.fixed_sample(t, 64, 6))
    assert torch.equal(bench.fixed_sample(t.view(10, 100), 1000, 0), t)      # small enough: every element, flattened


def test_write_outputs_float32_and_the_size_limit(tmp_path):
    arrays = {"a": np.arange(6, dtype=np.float16).reshape(2, 3), "b": np.float64(2.5), "c": np.zeros(3, dtype=np.int64)}
    total = bench.write_outputs(str(tmp_path), arrays)
    a, b, c = (np.load(os.path.join(str(tmp_path), n + ".npy")) for n in "abc")
    assert a.dtype == np.float32 and a.shape == (2, 3) and b.dtype == np.float64 and float(b) == 2.5
    assert c.dtype == np.float32 and total == a.nbytes + b.nbytes + c.nbytes
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_MAX_BYTES // 4 + 1, dtype=np.float32)})
    assert not os.path.exists(str(tmp_path / "big" / "x.npy"))


def test_step_and_trunk_outputs_names_and_sampling():
    lin = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 5000, bias=False))
    lin[0].weight.grad = torch.ones_like(lin[0].weight)      # the other parameters have no gradient: zeros in the dump
    res = tuple(torch.tensor(float(i)) for i in range(7))
    out = bench.step_outputs(res, lin)
    assert [out[n].item() for n in bench.STEP_OUTPUT_NAMES] == list(range(7))
    n = 6 + 2 + bench.DUMP_PARAM_SAMPLE                      # 6 + 2 elements whole, 10 000 sampled to DUMP_PARAM_SAMPLE
    assert out["params_sample"].shape == (n,) and out["grads_sample"].shape == (n,)
    assert (out["grads_sample"][:6] == 1).all() and (out["grads_sample"][6:] == 0).all()
    assert np.array_equal(out["params_sample"][:6], lin[0].weight.detach().reshape(-1).numpy())
    seq = torch.randn(2, 3, 4)
    t = bench.trunk_outputs((seq, seq[:, 0]))
    assert list(t) == ["sequence_output", "pooled_output"] and t["sequence_output"].dtype == np.float32
    assert np.array_equal(t["sequence_output"], seq.numpy()) and np.array_equal(t["pooled_output"], seq[:, 0].numpy())


def test_outputs_above_the_budget_keep_the_small_arrays_whole():
    n = bench.DUMP_MAX_ELEMS
    small, mid, big = torch.arange(10.0), torch.ones(n // 2 + 1), torch.arange(float(n))
    out = bench.fit_outputs({"big": big, "small": small, "mid": mid})
    assert list(out) == ["big", "small", "mid"] and np.array_equal(out["small"], small.numpy())
    share = (n - 10) // 2                                    # what is left after the small array, split between the two
    assert out["mid"].shape == (share,) and out["big"].shape == (n - 10 - share,)
    assert sum(a.size for a in out.values()) <= n and sum(a.nbytes for a in out.values()) <= bench.DUMP_MAX_BYTES
    again = bench.fit_outputs({"big": big, "small": small, "mid": mid})
    assert np.array_equal(out["big"], again["big"])          # the same sample positions in every call
    whole = bench.fit_outputs({"a": torch.ones(n - 10), "b": small})
    assert whole["a"].shape == (n - 10,) and whole["b"].shape == (10,)


def _bench(args, tmp_path, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


SMALL = ["--batch", "4", "--text", "24", "--regions", "8"]


@pytest.mark.gpu
def test_plain_bench_times_the_steps_and_dumps_the_train_step(dev, tmp_path):
    out_dir = str(tmp_path / "out")
    line = _bench(SMALL + ["--steps", "3", "--warmup", "2", "--dump-outputs", out_dir], tmp_path)
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step_hip_events"]["n"] == 3
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(4 * 1e3 / line["ms_per_step"], rel=1e-2)
    assert line["higher_is_better"] is True and line["unit"] == "samples/s" and line["dtype"] == "bf16"
    assert all(line[k] is None for k in SIDE_FIELDS)
    got = {n: np.load(os.path.join(out_dir, n + ".npy")) for n in bench.STEP_OUTPUT_NAMES + ("params_sample", "grads_sample")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.isfinite(got["loss"]) and float(got["loss"]) > 0
    assert float(got["loss"]) == pytest.approx(float(got["mask_loss"] + got["next_loss"] + got["token_loss"]), rel=1e-5)
    assert got["params_sample"].shape == got["grads_sample"].shape and np.isfinite(got["grads_sample"]).all()
    assert np.abs(got["grads_sample"]).max() > 0


@pytest.mark.gpu
def test_plain_bench_dumps_the_forward_and_full_adds_the_side_measurements(dev, tmp_path):
    out_dir = str(tmp_path / "out")
    line = _bench(SMALL + ["--mode", "fwd", "--steps", "2", "--warmup", "1", "--dump-outputs", out_dir], tmp_path)
    assert line["steps"] == 2 and all(line[k] is None for k in SIDE_FIELDS)
    seq = np.load(os.path.join(out_dir, "sequence_output.npy"))
    pooled = np.load(os.path.join(out_dir, "pooled_output.npy"))
    assert seq.shape == (4, 32, 768) and pooled.shape == (4, 768) and np.isfinite(seq).all()
    full = _bench(SMALL + ["--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"], tmp_path)
    assert full["steps"] == 2 and full["fwd_samples_per_sec"] > 0 and full["fwd_b64"]["samples_per_sec"] > 0
    assert full["b36"]["samples_per_sec"] > 0 and full["kernels_ms_per_step"] and full["roofline"]["achieved"] > 0
