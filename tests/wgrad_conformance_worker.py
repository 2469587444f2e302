"""One child process of tests/test_gpu_wgrad_conformance.py: the weight-gradient forms the library takes under non-default values of
VT_WGRAD_SPLIT / VT_WGRAD_ORDER / VT_WGRAD_PERSISTENT_MIN_ROWS (read once per process, so the suite's own process never runs them).

    python tests/wgrad_conformance_worker.py <family>        family: a key of helpers_wgrad.FAMILY_ENV

The parent sets the family's switch values in the environment.  Every case of the family goes through visitron_amd.ops.wgrad and is
judged by helpers_wgrad.judge; one `RATIO <check name>\t<measured / bound>` line per check, `DONE <cases>` at the end.  Under
VT_WGRAD_SPLIT=2 the 20 launches back to back and the turn form on two streams follow.  The parent re-asserts every ratio; this
process only refuses to run a case the library would send to another form."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import helpers_wgrad as hw
    from visitron_amd import ops

    family = sys.argv[1]
    for name, value in hw.FAMILY_ENV[family].items():
        assert os.environ.get(name) == value, "%s must be %s in this process" % (name, value)
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n = 0
    for case in hw.cases(family):
        if not hw.applicable(case, cus):
            continue
        reached = hw.case_dispatch(case, os.environ, cus)["form"]
        assert reached == case.reaches, "%s runs %s on %d CUs, not %s" % (case, reached, cus, case.reaches)
        outs = hw.run(case, dev)
        rs = hw.judge(case, outs, dev)
        for key in sorted(rs):
            print("RATIO %s %s: %s\t%r" % (family, case.name, key, abs(rs[key])))
        if case.data == "census" and not hw.passes(rs):
            print("CENSUS %s %s: %s" % (family, case.name, hw.census_report(case, outs, dev)))
        if case.data == "fingerprint":
            print("FINGERPRINT %s %s: %s" % (family, case.name, hw.fingerprint_values(case, outs)))
        n += 1
    print("RATIO %s turn timeouts after the table\t%r" % (family, 0.0 if ops.wgrad_turn_timeouts() == 0 else hw.INF))
    if family == "split2":
        seq = hw.sequence_cases(family)
        for tag, cs, streams in (("one stream", seq, 1), ("two streams", hw.two_stream_cases(), 2)):
            rs = hw.run_sequence(cs, dev, os.environ, streams)
            for key in sorted(rs):
                print("RATIO %s %s %s\t%r" % (family, tag, key, abs(rs[key])))
            n += len(cs)
    print("DONE %d" % n)


if __name__ == "__main__":
    main()
