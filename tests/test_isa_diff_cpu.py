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
