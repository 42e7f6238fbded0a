"""CPU: tools/isa_diff.py compares function BODIES, not only kernel descriptors, on small hand-written assembly."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DESC = "\t\t.amdhsa_group_segment_fixed_size 0\n\t\t.amdhsa_next_free_vgpr 8\n"


def kernel(name, body, n, comment=True, desc=DESC):
    """One function the way hipcc -S prints it: label line (with its `; @name` comment), body, descriptor, .Lfunc_end."""
    return (f"\t.globl\t{name}\n\t.type\t{name},@function\n{name}:{' ; @' + name if comment else ''}\n; %bb.0:\n"
            f"{body}.LBB{n}_1:                                ; =>This Inner Loop Header: Depth=1\n"
            f"\ts_cbranch_execnz .LBB{n}_1\n; %bb.2:                                ;   in Loop: Header=BB{n}_1 Depth=1\n\ts_endpgm\n"
            f"\t.section\t.rodata,\"a\",@progbits\n\t.amdhsa_kernel {name}\n{desc}\t.end_amdhsa_kernel\n\t.text\n"
            f".Lfunc_end{n}:\n\t.size\t{name}, .Lfunc_end{n}-{name}\n")


def unit(kernels, cuid):
    return ("\t.text\n" + "".join(kernels) +
            f"\t.type\t__hip_cuid_{cuid},@object\n\t.globl\t__hip_cuid_{cuid}\n__hip_cuid_{cuid}:\n\t.byte\t0\n")


BODY_A = "\tv_add_f32_e32 v1, v2, v3\n\tv_sub_f32_e32 v4, v1, v5\n\tv_mul_f32_e32 v6, v4, v4\n"
BODY_B = "\tglobal_load_dword v1, v0, s[0:1]\n\ts_waitcnt vmcnt(0)\n\tv_max_f32_e32 v1, v1, v2\n"


def run(tmp_path, base, tree, *pairs):
    (tmp_path / "base.s").write_text(base)
    (tmp_path / "tree.s").write_text(tree)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_diff.py"), str(tmp_path / "base.s"),
                        str(tmp_path / "tree.s"), *pairs], capture_output=True, text=True)
    assert p.returncode in (0, 1), p.stderr
    return p.returncode, p.stdout.splitlines()


def test_labels_and_cuid_do_not_count(tmp_path):
    base = unit([kernel("k_a", BODY_A, 0), kernel("k_b", BODY_B, 1)], "0123abcd")
    tree = unit([kernel("k_a", BODY_A, 4), kernel("k_b", BODY_B, 7)], "feed9876")
    rc, out = run(tmp_path, base, tree)
    assert rc == 0
    assert "IDENTICAL k_a" in out and "IDENTICAL k_b" in out
    assert out[0].startswith("base 2 kernels, tree 2; identical 2, commuted 0, differing 0, removed 0, added 0")


def test_label_width_does_not_move_a_diff(tmp_path):
    # hipcc pads a label line's comment to a fixed column: a function that becomes number 10 instead of 9 (another instantiation
    # order) has one space less in front of it
    base = unit([kernel("k_a", BODY_A, 9)], "0")
    tree = unit([kernel("k_a", BODY_A, 10).replace(".LBB10_1:                                ;", ".LBB10_1:                               ;")], "0")
    assert base.replace("BB9_", "BB10_") != tree
    rc, out = run(tmp_path, base, tree)
    assert rc == 0 and "IDENTICAL k_a" in out


def test_changed_instruction_under_commented_label_is_a_diff(tmp_path):
    # the regression: label lines carry `; @name`, ONE instruction of ONE body differs, the descriptors are equal
    base = unit([kernel("k_a", BODY_A, 0), kernel("k_b", BODY_B, 1)], "0123abcd")
    tree = unit([kernel("k_a", BODY_A, 0), kernel("k_b", BODY_B.replace("vmcnt(0)", "vmcnt(1)"), 1)], "0123abcd")
    rc, out = run(tmp_path, base, tree)
    assert rc == 1
    assert "IDENTICAL k_a" in out and "DIFF k_b" in out
    assert "identical 1, commuted 0, differing 1" in out[0]


def test_changed_instruction_under_bare_label_is_a_diff(tmp_path):
    base = unit([kernel("k_a", BODY_A, 0, comment=False)], "0")
    tree = unit([kernel("k_a", BODY_A.replace("v5", "v7"), 0, comment=False)], "0")
    rc, out = run(tmp_path, base, tree)
    assert rc == 1 and "DIFF k_a" in out


def test_changed_descriptor_is_a_diff(tmp_path):
    base = unit([kernel("k_a", BODY_A, 0)], "0")
    tree = unit([kernel("k_a", BODY_A, 0, desc=DESC.replace("vgpr 8", "vgpr 12"))], "0")
    rc, out = run(tmp_path, base, tree)
    assert rc == 1 and "DIFF k_a" in out


def test_swapped_add_operands_are_commuted(tmp_path):
    base = unit([kernel("k_a", BODY_A, 0), kernel("k_b", BODY_B, 1)], "0")
    tree = unit([kernel("k_a", BODY_A.replace("v_add_f32_e32 v1, v2, v3", "v_add_f32_e32 v1, v3, v2"), 0),
                 kernel("k_b", BODY_B, 1)], "0")
    rc, out = run(tmp_path, base, tree)
    assert rc == 0
    assert "COMMUTED k_a" in out and "IDENTICAL k_b" in out
    assert "identical 1, commuted 1, differing 0" in out[0]


def test_swapped_sub_operands_are_a_diff(tmp_path):
    base = unit([kernel("k_a", BODY_A, 0)], "0")
    tree = unit([kernel("k_a", BODY_A.replace("v_sub_f32_e32 v4, v1, v5", "v_sub_f32_e32 v4, v5, v1"), 0)], "0")
    rc, out = run(tmp_path, base, tree)
    assert rc == 1 and "DIFF k_a" in out


def test_commuted_destination_is_a_diff(tmp_path):
    base = unit([kernel("k_a", BODY_A, 0)], "0")
    tree = unit([kernel("k_a", BODY_A.replace("v_add_f32_e32 v1, v2, v3", "v_add_f32_e32 v2, v1, v3"), 0)], "0")
    rc, out = run(tmp_path, base, tree)
    assert rc == 1 and "DIFF k_a" in out


def test_swapped_scalar_and_integer_operands_are_commuted(tmp_path):
    body = ("\ts_add_i32 s5, s0, s2\n\ts_mul_i32 s6, s5, s3\n\ts_and_b32 s7, s6, s1\n\ts_max_u32 s8, s7, s4\n"
            "\tv_add_u32_e32 v1, v2, v3\n\ts_add_u32 s9, s8, s5\n")
    swapped = ("\ts_add_i32 s5, s2, s0\n\ts_mul_i32 s6, s3, s5\n\ts_and_b32 s7, s1, s6\n\ts_max_u32 s8, s4, s7\n"
               "\tv_add_u32_e32 v1, v3, v2\n\ts_add_u32 s9, s5, s8\n")
    rc, out = run(tmp_path, unit([kernel("k_a", body, 0)], "0"), unit([kernel("k_a", swapped, 0)], "0"))
    assert rc == 0 and "COMMUTED k_a" in out
    # a subtraction and a shift do not commute
    for op in ("s_sub_i32", "s_lshl_b32"):
        rc, out = run(tmp_path, unit([kernel("k_a", body + f"\t{op} s10, s9, s1\n", 0)], "0"),
                      unit([kernel("k_a", body + f"\t{op} s10, s1, s9\n", 0)], "0"))
        assert rc == 1 and "DIFF k_a" in out


def test_swapped_packed_multiply_sources_are_commuted_only_with_their_op_sel_hi_bits(tmp_path):
    line = "\tv_pk_mul_f32 v[30:31], v[32:33], v[30:31] op_sel_hi:[0,1]\n"
    both = "\tv_pk_mul_f32 v[30:31], v[30:31], v[32:33] op_sel_hi:[1,0]\n"     # sources and bits swapped together: the same product
    srcs = "\tv_pk_mul_f32 v[30:31], v[30:31], v[32:33] op_sel_hi:[0,1]\n"     # only the sources: another high half
    rc, out = run(tmp_path, unit([kernel("k_a", BODY_A + line, 0)], "0"), unit([kernel("k_a", BODY_A + both, 0)], "0"))
    assert rc == 0 and "COMMUTED k_a" in out
    rc, out = run(tmp_path, unit([kernel("k_a", BODY_A + line, 0)], "0"), unit([kernel("k_a", BODY_A + srcs, 0)], "0"))
    assert rc == 1 and "DIFF k_a" in out


# a K-loop-like body: address arithmetic between memory operations, counted waits, MFMAs
BODY_C = ("\ts_lshl_b32 s4, s2, 8\n\tv_lshlrev_b32_e32 v9, 4, v0\n\tglobal_load_dwordx4 v[2:5], v1, s[0:1]\n"
          "\tds_read_b128 v[10:13], v9\n\ts_waitcnt vmcnt(0) lgkmcnt(0)\n\tv_mfma_f32_16x16x32_f16 a[0:3], v[2:5], v[10:13], a[0:3]\n"
          "\ts_barrier\n\tv_add_u32_e32 v1, s4, v1\n\tglobal_store_dwordx4 v1, v[2:5], s[0:1]\n")
DESC_C = DESC + "\t\t.amdhsa_next_free_sgpr 16\n\t\t.amdhsa_accum_offset 16\n\t\t.amdhsa_private_segment_fixed_size 0\n"


def test_moved_valu_and_salu_lines_are_rescheduled(tmp_path):
    lines = BODY_C.splitlines(keepends=True)
    moved = "".join([lines[1], lines[0], lines[2], lines[3], lines[4], lines[5], lines[7], lines[6], lines[8]])
    assert moved != BODY_C
    base = unit([kernel("k_a", BODY_C, 0, desc=DESC_C), kernel("k_b", BODY_B, 1)], "0")
    rc, out = run(tmp_path, base, unit([kernel("k_a", moved, 0, desc=DESC_C), kernel("k_b", BODY_B, 1)], "0"))
    assert rc == 0
    assert "RESCHEDULED k_a" in out and "IDENTICAL k_b" in out
    assert out[0].endswith("identical 1, commuted 0, differing 0, removed 0, added 0, rescheduled 1")
    # the same move with one more SGPR in the descriptor, or with a register renumbered, is a DIFF
    rc, out = run(tmp_path, base, unit([kernel("k_a", moved, 0, desc=DESC_C.replace("sgpr 16", "sgpr 18")), kernel("k_b", BODY_B, 1)], "0"))
    assert rc == 1 and "DIFF k_a" in out
    rc, out = run(tmp_path, base, unit([kernel("k_a", moved.replace("s4", "s6"), 0, desc=DESC_C), kernel("k_b", BODY_B, 1)], "0"))
    assert rc == 1 and "DIFF k_a" in out


def test_a_diff_says_what_a_refactor_is_judged_by(tmp_path):
    # registers renumbered on two lines and two fewer SGPRs: DIFF, with the memory operations, waits and MFMAs in the base's order
    base = unit([kernel("k_a", BODY_C, 0, desc=DESC_C), kernel("k_b", BODY_B, 1)], "0")
    renumbered = BODY_C.replace("s4", "s6")
    rc, out = run(tmp_path, base, unit([kernel("k_a", renumbered, 0, desc=DESC_C.replace("sgpr 16", "sgpr 14")), kernel("k_b", BODY_B, 1)], "0"))
    assert rc == 1 and "identical 1, commuted 0, differing 1" in out[0]
    detail = out[out.index("DIFF k_a") + 1]
    assert detail.startswith("  ordered sequence same (6 -> 6 lines); resources next_free_sgpr 16 -> 14; changed lines 3 of ")
    # a wait with another counter and a larger LDS segment: the sequence differs, both resources are listed, one line changed
    waits = BODY_C.replace("vmcnt(0) lgkmcnt(0)", "vmcnt(1) lgkmcnt(0)")
    desc = DESC_C.replace("group_segment_fixed_size 0", "group_segment_fixed_size 512").replace("vgpr 8", "vgpr 12")
    rc, out = run(tmp_path, base, unit([kernel("k_a", waits, 0, desc=desc), kernel("k_b", BODY_B, 1)], "0"))
    detail = out[out.index("DIFF k_a") + 1]
    assert rc == 1 and detail.startswith("  ordered sequence DIFFERS (6 -> 6 lines); resources group_segment_fixed_size 0 -> 512, "
                                         "next_free_vgpr 8 -> 12; changed lines 3 of ")
    # equal resources are said to be equal; no other class grows a second line
    rc, out = run(tmp_path, base, unit([kernel("k_a", renumbered, 0, desc=DESC_C), kernel("k_b", BODY_B, 1)], "0"))
    assert out[out.index("DIFF k_a") + 1].startswith("  ordered sequence same (6 -> 6 lines); resources same; changed lines 2 of ")
    assert out[out.index("IDENTICAL k_b") + 1] == "DIFF k_a" and len(out) == 4


def test_moved_global_load_is_a_diff_not_rescheduled(tmp_path):
    lines = BODY_C.splitlines(keepends=True)
    moved = "".join([lines[0], lines[1], lines[3], lines[2]] + lines[4:])  # the load behind the LDS read
    rc, out = run(tmp_path, unit([kernel("k_a", BODY_C, 0, desc=DESC_C)], "0"), unit([kernel("k_a", moved, 0, desc=DESC_C)], "0"))
    assert rc == 1 and "DIFF k_a" in out and not [line for line in out if line.startswith("RESCHEDULED")]
    # a wait with another count, the rest in place
    rc, out = run(tmp_path, unit([kernel("k_a", BODY_C, 0, desc=DESC_C)], "0"),
                  unit([kernel("k_a", BODY_C.replace("vmcnt(0) lgkmcnt(0)", "vmcnt(1) lgkmcnt(0)"), 0, desc=DESC_C)], "0"))
    assert rc == 1 and "DIFF k_a" in out


def test_exchanged_counted_waits_are_a_diff(tmp_path):
    # the same lines, the same mnemonics in the same order: only the counters of the two waits changed places
    body = ("\tglobal_load_dwordx4 v[2:5], v1, s[0:1]\n\tglobal_load_dwordx4 v[6:9], v1, s[0:1] offset:16\n\ts_waitcnt vmcnt(1)\n"
            "\tv_mfma_f32_16x16x32_f16 a[0:3], v[2:5], v[2:5], a[0:3]\n\ts_waitcnt vmcnt(0)\n"
            "\tv_mfma_f32_16x16x32_f16 a[0:3], v[6:9], v[6:9], a[0:3]\n")
    swapped = body.replace("vmcnt(1)", "vmcnt(X)").replace("vmcnt(0)", "vmcnt(1)").replace("vmcnt(X)", "vmcnt(0)")
    assert sorted(body.splitlines()) == sorted(swapped.splitlines())
    rc, out = run(tmp_path, unit([kernel("k_a", body, 0, desc=DESC_C)], "0"), unit([kernel("k_a", swapped, 0, desc=DESC_C)], "0"))
    assert rc == 1 and "DIFF k_a" in out and not [line for line in out if line.startswith("RESCHEDULED")]
    # two counters on one line count too
    body2 = body.replace("vmcnt(1)", "vmcnt(1) lgkmcnt(0)").replace("s_waitcnt vmcnt(0)\n", "s_waitcnt vmcnt(0) lgkmcnt(1)\n")
    swapped2 = body2.replace("vmcnt(1) lgkmcnt(0)", "W").replace("vmcnt(0) lgkmcnt(1)", "vmcnt(1) lgkmcnt(0)").replace("W", "vmcnt(0) lgkmcnt(1)")
    assert body2 != swapped2 and sorted(body2.splitlines()) == sorted(swapped2.splitlines())
    rc, out = run(tmp_path, unit([kernel("k_a", body2, 0, desc=DESC_C)], "0"), unit([kernel("k_a", swapped2, 0, desc=DESC_C)], "0"))
    assert rc == 1 and "DIFF k_a" in out


def test_rename_pairs_up(tmp_path):
    base = unit([kernel("k_oldILi1ELb1EE", BODY_A, 0), kernel("k_b", BODY_B, 1)], "0")
    tree = unit([kernel("k_newILi1EE", BODY_A, 0), kernel("k_b", BODY_B, 1)], "1")
    rc, out = run(tmp_path, base, tree)
    assert rc == 1 and "REMOVED k_oldILi1ELb1EE" in out and "ADDED k_newILi1EE" in out
    rc, out = run(tmp_path, base, tree, "k_oldILi1ELb1EE=k_newILi1EE")
    assert rc == 0
    assert "PAIRED k_oldILi1ELb1EE -> k_newILi1EE" in out and "IDENTICAL k_newILi1EE" in out
    assert not [line for line in out if line.startswith(("REMOVED", "ADDED", "DIFF"))]


def test_kernel_only_in_tree_is_added(tmp_path):
    base = unit([kernel("k_a", BODY_A, 0)], "0")
    tree = unit([kernel("k_a", BODY_A, 0), kernel("k_b", BODY_B, 1)], "0")
    rc, out = run(tmp_path, base, tree)
    assert rc == 1 and "IDENTICAL k_a" in out and "ADDED k_b" in out
    rc, out = run(tmp_path, tree, base)  # the other way round: REMOVED alone does not fail
    assert rc == 0 and "REMOVED k_b" in out
