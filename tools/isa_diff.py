#!/usr/bin/env python3
"""Device-assembly diff of two source trees, kernel by kernel (CPU only, needs hipcc).

usage: python tools/isa_diff.py OLD_TREE NEW_TREE [file.hip ...]

Each named file (default: every csrc/*.hip of either tree; a bare name is looked up under the
package's csrc/) is compiled in both trees with __graft_entry__.HIP_FLAGS, `--cuda-device-only -S`
in place of `-shared`. The listing is split at each function symbol (the text before the first,
and the register maximums, device variables and code-object metadata after the last, are compared
as `<preamble>` and `<tail>`); lines holding `__hip_cuid_` (a hash of the source text) are
dropped. Prints per file how many kernels are identical, which differ and which were added or
removed; exits 1 on any difference. A source-only refactor of a kernel file proves itself with
this against the parent commit checked out beside it (`git worktree add <dir> <parent>`)."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import HIPCC, HIP_FLAGS, PKG_NAME  # noqa: E402

FLAGS = [f for f in HIP_FLAGS if f != "-shared"] + ["--cuda-device-only", "-S"]
FUNC = re.compile(r"^\s*\.type\s+(\S+),@function")
TAIL = re.compile(r"^\s*(\.section\s+\.AMDGPU\.gpr_maximums|\.amdgpu_metadata)")


def assemble(tree, rel, out):
    """-> {symbol: [lines]} of one file's device assembly, or None where the tree has no such file."""
    src = os.path.join(tree, rel)
    if not os.path.exists(src):
        return None
    r = subprocess.run([HIPCC] + FLAGS + ["-I", os.path.join(tree, "include"), src, "-o", out],
                       capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"isa_diff: {src} does not compile\n{r.stderr}")
    syms, cur = {}, "<preamble>"
    with open(out) as f:
        for line in f:
            m = FUNC.match(line)
            if m:
                cur = m.group(1)
            elif TAIL.match(line):
                cur = "<tail>"
            if "__hip_cuid_" not in line:
                syms.setdefault(cur, []).append(line)
    return syms


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    old, new = argv[1], argv[2]
    csrc = os.path.join(PKG_NAME, "csrc")
    rels = [a if os.sep in a else os.path.join(csrc, a) for a in argv[3:]]
    if not rels:
        rels = sorted({os.path.join(csrc, n) for t in (old, new) if os.path.isdir(os.path.join(t, csrc))
                       for n in os.listdir(os.path.join(t, csrc)) if n.endswith(".hip")})
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=16) as pool:
        jobs = [(rel, [pool.submit(assemble, t, rel, os.path.join(tmp, f"{i}_{k}.s")) for k, t in enumerate((old, new))])
                for i, rel in enumerate(rels)]
        for rel, (fo, fn) in jobs:
            o, n = fo.result() or {}, fn.result() or {}
            same = [s for s in o if s in n and o[s] == n[s] and s[0] != "<"]
            differ = sorted(s for s in o if s in n and o[s] != n[s])
            removed, added = sorted(set(o) - set(n)), sorted(set(n) - set(o))
            print(f"{rel}: {len(same)} of {sum(s[0] != '<' for s in o)} kernels identical, {len(differ)} differ, "
                  f"{len(added)} added, {len(removed)} removed")
            for tag, names in (("differs", differ), ("added", added), ("removed", removed)):
                for s in names:
                    print(f"  {tag}: {s}" + (f" ({len(o[s])} -> {len(n[s])} lines)" if tag == "differs" else ""))
            bad += len(differ) + len(added) + len(removed)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
