#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device-assembly files of one translation unit.

    hipcc <the flags of sonar_amd/build.py> --offload-device-only -S csrc/X.hip -o X.s      (once per tree)
    python tools/isa_diff.py base/X.s tree/X.s [OLD_NAME=NEW_NAME ...]

Compares function bodies (from the `name:` label line, with or without its `; @name` comment, to the next `.Lfunc_endN:`)
and .amdhsa_kernel descriptors; the per-file __hip_cuid_<hash> symbol is masked, local labels are renumbered per
function and the padding in front of a label line's comment is ignored.  OLD=NEW pairs a kernel of the base with its new mangled name (a template parameter that went).
Every kernel of the base is IDENTICAL, COMMUTED (equal once the two source operands of every v_add/mul/max/min_f32_e32,
s_add_i32/u32, s_mul_i32, s_and/or/xor_b32, s_min/max_i32/u32 and v_add_u32_e32 line are sorted, and those of a v_pk_mul_f32
whose only modifier is op_sel_hi:[x,y] together with the two bits -- IEEE add, mul, max and min and the integer operations
commute exactly, SCC and carry included; nothing else is normalised), RESCHEDULED, DIFF or
REMOVED; kernels only in the tree are ADDED.  Under a DIFF line: whether the ordered sequence (next sentence) is the base's all the
same, every descriptor resource that differs as `field base -> tree`, and the count of changed lines (the larger side of a
line diff, descriptor included) -- what a refactor that renumbers registers is judged by.  RESCHEDULED: the sequence of v_mfma*, ds_*, global_* / buffer_*, s_waitcnt*,
s_barrier and s_setprio lines, compared by mnemonic (s_waitcnt: with its counters), equals the base's, and so do the
descriptor's VGPR / AGPR / SGPR counts, scratch size and LDS size, and the two bodies hold the same lines (as a multiset,
after the COMMUTED sorting) -- only VALU / SALU address or arithmetic lines moved; a line that changed, a register
renumbered, is DIFF.  (The 256x256 GEMM engines rely on counted vmcnt waits: the order of memory operations and waits is
what must not move.)
Exit status 1 if a kernel is DIFF or ADDED.
"""
import difflib
import re
import sys

COMMUTATIVE = re.compile(r"^(\s*(?:v_(?:add|mul|max|min)_f32_e32|s_add_[iu]32|s_mul_i32|s_(?:and|or|xor)_b32|s_(?:min|max)_[iu]32|v_add_u32_e32)"
                         r" [^,]+), ([^,;]+), ([^,;]+?)(\s*(?:;.*)?)$", re.M)
# v_pk_mul_f32 d, a, b op_sel_hi:[x,y] (no other modifier): the two sources swapped TOGETHER with their op_sel_hi bits
PK_MUL = re.compile(r"^(\s*v_pk_mul_f32 [^,]+), ([^,;]+), ([^,; ]+) op_sel_hi:\[([01]),([01])\](\s*(?:;.*)?)$", re.M)
ORDERED = re.compile(r"^\s*(v_mfma\w*|ds_\w+|global_\w+|buffer_\w+|s_barrier|s_setprio|s_waitcnt\w*[^;\n]*)", re.M)  # s_waitcnt: the whole operand text
RESOURCES = re.compile(r"^\s*\.amdhsa_(?:next_free_vgpr|next_free_sgpr|accum_offset|private_segment_fixed_size|group_segment_fixed_size) .*$", re.M)


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
        if m.group(2) not in out.get(m.group(1), ""):  # (hipcc prints the descriptor behind .Lfunc_end: once, not twice)
            out[m.group(1)] = out.get(m.group(1), "") + m.group(2)
    return out


def norm(s):  # local labels are numbered per file: renumber per function (comments name blocks without the .L: "Header=BB3_5")
    seen = {}
    s = re.sub(r"(?<![.\w])BB\d+_\d+", lambda m: ".L" + m.group(0), s)
    s = re.sub(r"\.L\w+", lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), s)
    return re.sub(r"^(\.L\d+:)[ \t]+;", r"\1 ;", s, flags=re.M)  # the comment column moves with the label's width (.LBB9_1 / .LBB10_1)


def commute(s):
    s = PK_MUL.sub(lambda m: "%s, %s, %s op_sel_hi:[%s,%s]%s" % (m.group(1), *sum(zip(*sorted(zip(m.group(2, 3), m.group(4, 5)))), ()), m.group(6)), s)
    return COMMUTATIVE.sub(lambda m: "%s, %s, %s%s" % (m.group(1), *sorted(m.group(2, 3)), m.group(4)), s)


def skeleton(s):  # what a RESCHEDULED kernel shares with its base: ordered lines in order, resources, all lines as a multiset
    return ([" ".join(m.split()) for m in ORDERED.findall(s)], [" ".join(m.split()) for m in RESOURCES.findall(s)],
            sorted(commute(s).splitlines()))


pairs = [tuple(p.split("=", 1)) for p in sys.argv[3:]]
a, b = ({k: norm(v) for k, v in kernels(*args).items()} for args in ((sys.argv[1], pairs), (sys.argv[2],)))
both = [k for k in a if k in b]
same = [k for k in both if a[k] == b[k]]
comm = [k for k in both if a[k] != b[k] and commute(a[k]) == commute(b[k])]
rest = [k for k in both if commute(a[k]) != commute(b[k])]
resch = [k for k in rest if skeleton(a[k]) == skeleton(b[k])]
diff = [k for k in rest if k not in resch]
print(f"base {len(a)} kernels, tree {len(b)}; identical {len(same)}, commuted {len(comm)}, differing {len(diff)}, "
      f"removed {len(set(a) - set(b))}, added {len(set(b) - set(a))}, rescheduled {len(resch)}")
for old, new in pairs: print("PAIRED", old, "->", new)
for k in same: print("IDENTICAL", k)
for k in comm: print("COMMUTED", k)
for k in resch: print("RESCHEDULED", k)
for k in diff:
    print("DIFF", k)
    (oa, ra, _), (ob, rb, _) = skeleton(a[k]), skeleton(b[k])
    fa, fb = ({r.split()[0].replace(".amdhsa_", ""): r.split()[1] for r in rs} for rs in (ra, rb))
    moved = [f"{f} {fa.get(f, '-')} -> {fb.get(f, '-')}" for f in dict.fromkeys([*fa, *fb]) if fa.get(f) != fb.get(f)]
    marks = [d[0] for d in difflib.unified_diff(a[k].splitlines(), b[k].splitlines(), n=0, lineterm="")][2:]
    print(f"  ordered sequence {'same' if oa == ob else 'DIFFERS'} ({len(oa)} -> {len(ob)} lines); resources "
          f"{', '.join(moved) if moved else 'same'}; changed lines {max(marks.count('-'), marks.count('+'))} of {len(a[k].splitlines())}")
for k in sorted(set(a) - set(b)): print("REMOVED", k)
for k in sorted(set(b) - set(a)): print("ADDED", k)
sys.exit(1 if diff or set(b) - set(a) else 0)
