#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device-assembly files of one translation unit.

    hipcc <the flags of sonar_amd/build.py> --offload-device-only -S csrc/X.hip -o X.s      (once per tree)
    python tools/isa_diff.py base/X.s tree/X.s [OLD_NAME=NEW_NAME ...]

Compares function bodies (from the `name:` label line, with or without its `; @name` comment, to the next `.Lfunc_endN:`)
and .amdhsa_kernel descriptors; the per-file __hip_cuid_<hash> symbol is masked, local labels are renumbered per
function and the padding in front of a label line's comment is ignored.  OLD=NEW pairs a kernel of the base with its new mangled name (a template parameter that went).
Every kernel of the base is IDENTICAL, COMMUTED (equal once the two source operands of every v_add/mul/max/min_f32_e32
line are sorted -- IEEE add, mul, max and min commute; nothing else is normalised), DIFF or REMOVED; kernels only in the
tree are ADDED.  Exit status 1 if a kernel is DIFF or ADDED.
"""
import re
import sys

COMMUTATIVE = re.compile(r"^(\s*v_(?:add|mul|max|min)_f32_e32 [^,]+), ([^,;]+), ([^,;]+?)(\s*(?:;.*)?)$", re.M)


def kernels(path, rename=()):
    txt = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    for old, new in rename:
        txt = re.sub(rf"\b{re.escape(old)}\b", new, txt)
    out, name, body = {}, None, []
    for line in txt.splitlines():
        m = re.match(r"(\w+):\s*(?:;.*)?$", line)
        if m:  # a data label never reaches a .Lfunc_end: the next label line replaces it
            name, body = m.group(1), []
        elif name and re.match(r"\.Lfunc_end\d+:", line):
            out[name], name = "\n".join(body) + "\n", None
        elif name:
            body.append(line)
    for m in re.finditer(r"^\t\.amdhsa_kernel (\w+)\n(.*?)^\t\.end_amdhsa_kernel", txt, flags=re.M | re.S):
        out[m.group(1)] = out.get(m.group(1), "") + m.group(2)
    return out


def norm(s):  # local labels are numbered per file: renumber per function (comments name blocks without the .L: "Header=BB3_5")
    seen = {}
    s = re.sub(r"(?<![.\w])BB\d+_\d+", lambda m: ".L" + m.group(0), s)
    s = re.sub(r"\.L\w+", lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), s)
    return re.sub(r"^(\.L\d+:)[ \t]+;", r"\1 ;", s, flags=re.M)  # the comment column moves with the label's width (.LBB9_1 / .LBB10_1)


def commute(s):
    return COMMUTATIVE.sub(lambda m: "%s, %s, %s%s" % (m.group(1), *sorted(m.group(2, 3)), m.group(4)), s)


pairs = [tuple(p.split("=", 1)) for p in sys.argv[3:]]
a, b = ({k: norm(v) for k, v in kernels(*args).items()} for args in ((sys.argv[1], pairs), (sys.argv[2],)))
both = [k for k in a if k in b]
same = [k for k in both if a[k] == b[k]]
comm = [k for k in both if a[k] != b[k] and commute(a[k]) == commute(b[k])]
diff = [k for k in both if commute(a[k]) != commute(b[k])]
print(f"base {len(a)} kernels, tree {len(b)}; identical {len(same)}, commuted {len(comm)}, differing {len(diff)}, "
      f"removed {len(set(a) - set(b))}, added {len(set(b) - set(a))}")
for old, new in pairs: print("PAIRED", old, "->", new)
for k in same: print("IDENTICAL", k)
for k in comm: print("COMMUTED", k)
for k in diff: print("DIFF", k)
for k in sorted(set(a) - set(b)): print("REMOVED", k)
for k in sorted(set(b) - set(a)): print("ADDED", k)
sys.exit(1 if diff or set(b) - set(a) else 0)
