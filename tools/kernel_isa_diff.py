#!/usr/bin/env python3
"""Are the gfx950 kernels of two csrc trees the same instructions?  Host only: it compiles and runs nothing.

    python tools/kernel_isa_diff.py OLD_CSRC NEW_CSRC [file.hip ...]

Every .hip file of both trees (or the named ones) is compiled to device assembly as tests/test_build_isa.py does, cut into
kernels (instructions and kernel descriptor) and compared per kernel symbol after dropping what only records WHERE in its
file a kernel stands: comments and the numbers in local labels.  A symbol that several files of a tree emit must be equal
in every copy.  Exit status 0 only if both trees emit the same kernels with the same text.
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HIPCC = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S"]
LOCAL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b")


def kernels(asm):
    """symbol -> raw text of each kernel: from its label to .end_amdhsa_kernel"""
    res = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\s*$", asm, re.M):
        begin = re.search(r"^%s:" % re.escape(m.group(1)), asm, re.M).start()
        res[m.group(1)] = asm[begin:asm.index(".end_amdhsa_kernel", m.end()) + len(".end_amdhsa_kernel")]
    return res


def normalise(text):
    """lines without comments; .LBB<f>_<n> loses <f> (the function's position in its file), .Ltmp<n>, .Lfunc_end<n> and
    their like are renumbered in order of first use inside the kernel"""
    seen = {}

    def local(m):
        return ".L%s%s" % (m.group(1), m.group(3) or seen.setdefault(m.group(0), len(seen)))

    lines = (LOCAL.sub(local, line.split(";")[0]).strip() for line in text.split("\n"))
    return [" ".join(line.split()) for line in lines if line]


def tree_kernels(csrc, names, workdir):
    """(symbol -> normalised lines, file -> kernel count, report lines for unequal copies); at most 16 compiles at a time"""
    def asm_of(name):
        out = os.path.join(workdir, name + ".s")
        subprocess.run(HIPCC + [name, "-o", out], check=True, cwd=csrc, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()

    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        texts = list(pool.map(asm_of, names))
    merged, counts, rep = {}, {}, []
    for name, asm in zip(names, texts):
        ks = {sym: normalise(text) for sym, text in kernels(asm).items()}
        counts[name] = len(ks)
        rep += ["changed  %s: the copy in %s differs from another file's" % (s, name) for s in ks if merged.get(s, ks[s]) != ks[s]]
        merged.update(ks)
    return merged, counts, rep


def compare(old, new):
    """report lines for two symbol -> normalised-lines maps; empty when they are equal"""
    rep = ["removed  " + s for s in sorted(set(old) - set(new))] + ["added    " + s for s in sorted(set(new) - set(old))]
    for s in sorted(set(old) & set(new)):
        if old[s] != new[s]:
            i = next((i for i, (a, b) in enumerate(zip(old[s], new[s])) if a != b), min(len(old[s]), len(new[s])))
            rep.append("changed  %s\n    line %d: %s\n         -> %s" % (s, i, " | ".join(old[s][i:i + 3]), " | ".join(new[s][i:i + 3])))
    return rep


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for csrc in argv[1:3]:
            names = [f for f in argv[3:] or sorted(os.listdir(csrc)) if f.endswith(".hip") and os.path.exists(os.path.join(csrc, f))]
            res.append(tree_kernels(csrc, names, tempfile.mkdtemp(dir=tmp)))
    (old, old_n, old_rep), (new, new_n, new_rep) = res
    print("%-24s %6s %6s" % ("kernels per file", "old", "new"))
    for name in sorted(set(old_n) | set(new_n)):
        print("%-24s %6s %6s" % (name, old_n.get(name, "-"), new_n.get(name, "-")))
    print("%-24s %6d %6d   (distinct symbols: %d, %d)" % ("all files", sum(old_n.values()), sum(new_n.values()), len(old), len(new)))
    rep = old_rep + new_rep + compare(old, new)
    print("\n".join(rep + ["added %d, removed %d, changed %d" % tuple(sum(r.startswith(w) for r in rep) for w in ("added", "removed", "changed"))]))
    return 1 if rep else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
