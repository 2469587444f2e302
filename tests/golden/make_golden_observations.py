"""Writes tests/golden/ref_observations.npz from the reference's own input-building code (build container only).

The reference's source runs where it lies: tasks/viewpoint_select/agent.py and utils.py are imported from /root/reference by
path (asserted below), nothing of their text is copied.  `lmdb`, which this machine does not have and the executed functions
do not touch, gets an empty stand-in module.  Agent.get_input_feat, Agent._feature_variable, Agent._candidate_variable and
utils.length2mask run over the synthetic observations of tests/helpers_observations.py (B = 5, candidate counts 0, 1, 3, 3, 2,
D = 10; angles with 0, negative values and values above 2 pi) on a throw-away `self` that carries `args` only.

Recorded: the inputs (store, keys, table and the eight per-step fields, the ragged candidate lists padded with zeros to
[B, 3]) and the four outputs plus the mask."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import helpers_observations as ho  # noqa: E402


def _load(name, rel):
    path = os.path.join(REF, rel)
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.realpath(mod.__file__).startswith(REF + os.sep), mod.__file__
    return mod


class _Args(object):
    device = "cpu"
    views = 36
    angle_feat_size = 4
    lstm_img_feature_dim = 10


class _Self(object):
    args = _Args()


def main():
    sys.modules.setdefault("lmdb", types.ModuleType("lmdb"))
    sys.path.insert(0, os.path.join(REF, "tasks", "viewpoint_select"))
    sys.path.insert(0, REF)
    agent = _load("ref_viewpoint_agent", "tasks/viewpoint_select/agent.py")
    utils = agent.utils
    assert os.path.realpath(utils.__file__).startswith(REF + os.sep), utils.__file__

    inp = ho.synthetic_inputs(D=_Args.lstm_img_feature_dim)
    keys = ho.keys_for(inp["store"].shape[0])
    obs = ho.make_obs(inp, keys)
    me = _Self()
    me._feature_variable = lambda o: agent.Agent._feature_variable(me, o)
    me._candidate_variable = lambda o: agent.Agent._candidate_variable(me, o)
    input_a_t, f_t, candidate_feat, candidate_leng = agent.Agent.get_input_feat(me, obs)
    mask = utils.length2mask(candidate_leng, "cpu")

    B, C = len(obs), max(int(c) for c in inp["cand_count"])

    def padded(rows, dtype):
        out = np.zeros((B, C), dtype=dtype)
        for b, r in enumerate(rows):
            out[b, :len(r)] = r
        return out

    out = dict(store=inp["store"], keys=np.array(keys), table=inp["table"], slots=inp["slots"].astype(np.int64),
               view_index=inp["view_index"].astype(np.int64), heading=inp["heading"], elevation=inp["elevation"],
               cand_point=padded(inp["cand_point"], np.int64), cand_heading=padded(inp["cand_heading"], np.float64),
               cand_elevation=padded(inp["cand_elevation"], np.float64), cand_count=inp["cand_count"].astype(np.int64),
               input_a_t=input_a_t.numpy(), f_t=f_t.numpy(), candidate_feat=candidate_feat.numpy(),
               candidate_leng=np.array(candidate_leng, dtype=np.int64), candidate_mask=mask.numpy())
    path = os.path.join(HERE, "ref_observations.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 100 * 1024, size
    print("ref_observations.npz written: %d bytes, %d arrays" % (size, len(out)))


if __name__ == "__main__":
    sys.exit(main())
