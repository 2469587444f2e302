"""One child process of tests/test_gpu_layernorm_conformance.py: the LayerNorm kernels the library runs under non-default values
of VT_LN_FWD_ROWS / VT_LN_FWD_BLOCKS / VT_LN_BWD_ROWS (read once per process, so the suite's own process never runs them).

    python tests/ln_conformance_worker.py <family>        family: a key of helpers_layernorm.FAMILY_ENV

The parent sets the family's switch values in the environment.  Every case of the family goes through its visitron_amd.ops entry
point and is judged by helpers_layernorm.judge; one `RATIO <check name>\t<measured / bound>` line per check, `DONE <cases>` at the
end.  The parent re-asserts every ratio; this process only refuses to run a case the library would send to another kernel."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import helpers_layernorm as hl

    family = sys.argv[1]
    for name, value in hl.FAMILY_ENV[family].items():
        assert os.environ.get(name) == value, "%s must be %s in this process" % (name, value)
    dev = torch.device("cuda", 0)
    n = 0
    for case in hl.cases(family):
        reached = hl.case_dispatch(case, os.environ)[0]
        assert reached == case.reaches, "%s runs %s, not %s" % (case, reached, case.reaches)
        rs = hl.judge(case, hl.run(case, dev))
        for key in sorted(rs):
            print("RATIO %s %s: %s\t%r" % (family, case.name, key, abs(rs[key])))
        n += 1
    print("DONE %d" % n)


if __name__ == "__main__":
    main()
