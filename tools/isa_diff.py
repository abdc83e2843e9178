#!/usr/bin/env python
"""Is the gfx950 assembly of the working tree the same as that of commit REV?  The proof that a kernel refactor moved nothing.
    python tools/isa_diff.py REV [file.hip ...]                                       (needs hipcc and git; no GPU)
REV's csrc/ and include/ are exported with `git archive` (the working tree is not touched), every named source (default: all of
_build.SOURCES) is compiled from both trees with the product flags plus `--cuda-device-only -S -fuse-cuid=none`, and the two assembly
files are compared byte for byte: one line per source, `identical` or the first differing lines.  Exit status 1 if any source differs."""
import importlib.util, io, os, subprocess, sys, tarfile, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "solver-in-the-loop_amd"
spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, PKG, "_build.py"))
b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)

if len(sys.argv) < 2:
    sys.exit(__doc__)
rev, sources = sys.argv[1], sys.argv[2:] or b.SOURCES


def compile_asm(job):
    tree, src, out = job
    cmd = [b._hipcc()] + b.FLAGS + b.EXTRA.get(src, []) + ["--cuda-device-only", "-S", "-fuse-cuid=none",
                                                           os.path.join(tree, PKG, "csrc", src), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.exit("hipcc failed for %s:\n%s" % (os.path.join(tree, PKG, "csrc", src), r.stdout))


with tempfile.TemporaryDirectory() as tmp:
    old = os.path.join(tmp, "old")
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, PKG + "/csrc", "include"], stdout=subprocess.PIPE, check=True).stdout
    tarfile.open(fileobj=io.BytesIO(tar)).extractall(old)
    asm = {s: (os.path.join(tmp, s + ".old.s"), os.path.join(tmp, s + ".new.s")) for s in sources}
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:       # the slowest source (karman_step.hip) first
        list(pool.map(compile_asm, [(t, s, asm[s][k]) for s in sources for k, t in enumerate((old, ROOT))]))
    differ = 0
    for s in sources:
        a, c = (open(p).read() for p in asm[s])
        if a == c:
            print("%-22s identical  (%d lines)" % (s, a.count("\n")))
            continue
        differ += 1
        la, lc = a.splitlines(), c.splitlines()
        i = next((k for k, (x, y) in enumerate(zip(la, lc)) if x != y), min(len(la), len(lc)))
        print("%-22s DIFFERS from line %d  (%d / %d lines)" % (s, i + 1, len(la), len(lc)))
        print("\n".join(["  - " + x for x in la[i:i + 5]] + ["  + " + y for y in lc[i:i + 5]]))
sys.exit(1 if differ else 0)
