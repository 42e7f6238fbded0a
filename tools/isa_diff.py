#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device-assembly files of one translation unit.

    hipcc <the flags of sonar_amd/build.py> --offload-device-only -S csrc/X.hip -o X.s      (once per tree)
    python tools/isa_diff.py base/X.s tree/X.s [OLD_NAME=NEW_NAME ...]

Compares function bodies and .amdhsa_kernel descriptors; the per-file __hip_cuid_<hash> symbol is masked and local labels are
renumbered per function.  OLD=NEW pairs a kernel of the base with its new mangled name (a template parameter that went).
Exit status 1 if a kernel differs or one was added.
"""
import re
import sys


def kernels(path, rename=()):
    txt = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    for old, new in rename:
        txt = re.sub(rf"\b{re.escape(old)}\b", new, txt)
    out = {}
    for m in re.finditer(r"^(\w+):\s*(?:;.*)?\n(.*?)^\.Lfunc_end\d+:", txt, flags=re.M | re.S):
        out[m.group(1)] = m.group(2)
    for m in re.finditer(r"^\t\.amdhsa_kernel (\w+)\n(.*?)^\t\.end_amdhsa_kernel", txt, flags=re.M | re.S):
        out[m.group(1)] = out.get(m.group(1), "") + m.group(2)
    return out


def norm(s):  # local labels are numbered per file: renumber per function
    seen = {}
    return re.sub(r"\.L\w+", lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), s)


pairs = [tuple(p.split("=", 1)) for p in sys.argv[3:]]
a, b = kernels(sys.argv[1], pairs), kernels(sys.argv[2])
same = [k for k in a if k in b and norm(a[k]) == norm(b[k])]
diff = [k for k in a if k in b and norm(a[k]) != norm(b[k])]
print(f"base {len(a)} kernels, tree {len(b)}; identical {len(same)}, differing {len(diff)}, "
      f"removed {len(set(a) - set(b))}, added {len(set(b) - set(a))}")
for old, new in pairs: print("PAIRED", old, "->", new)
for k in diff: print("DIFF", k)
for k in sorted(set(a) - set(b)): print("REMOVED", k)
for k in sorted(set(b) - set(a)): print("ADDED", k)
sys.exit(1 if diff or set(b) - set(a) else 0)
