"""Per-kernel instruction-mnemonic counts of two device assembly files, and their differences.
   python tools/isa_diff.py A/zr_kernels-hip-amdgcn-amd-amdhsa-gfx950.s B/zr_kernels-hip-amdgcn-amd-amdhsa-gfx950.s [-v]
A kernel's code is what lies between its `name:` label and its `.Lfunc_end`; comments,
labels, directives and operands are ignored, so two builds compare equal when every
kernel has the same multiset of mnemonics.  Exit status 1 when any kernel differs."""
import collections
import re
import subprocess
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        line = line.split(";", 1)[0].rstrip()
        if not line:
            continue
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and not line.startswith(".L"):
            cur = out.setdefault(m.group(1), collections.Counter())
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            cur = None
        if cur is None or s.startswith(".") or s.endswith(":"):
            continue
        cur[s.split()[0]] += 1
    return {k: v for k, v in out.items() if v}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    verbose = "-v" in sys.argv[3:]
    names = sorted(set(a) | set(b))
    nice = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    differ = 0
    for n, d in zip(names, nice):
        ca, cb = a.get(n, collections.Counter()), b.get(n, collections.Counter())
        same = ca == cb
        differ += not same
        if verbose or not same:
            print(f"{'same' if same else 'DIFF'} {sum(ca.values()):7d} {sum(cb.values()):7d}  {d[:110]}")
        if not same:
            for op in sorted(set(ca) | set(cb)):
                if ca[op] != cb[op]:
                    print(f"       {op:28s} {ca[op]:6d} -> {cb[op]:6d}")
    print(f"{len(names)} functions, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
