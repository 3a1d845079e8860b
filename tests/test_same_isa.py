"""tools/same_isa.py, the gate of a refactoring of the kernel sources, on two small texts in the shape of `make asm`
output: no GPU, no compiler."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "same_isa.py")


def kernel(name, func, body):
    return """\t.protected\t%(n)s
\t.globl\t%(n)s
\t.p2align\t8
\t.type\t%(n)s,@function
%(n)s:
%(b)s\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel %(n)s
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr 3
\t.end_amdhsa_kernel
\t.text
.Lfunc_end%(f)d:
\t.size\t%(n)s, .Lfunc_end%(f)d-%(n)s
""" % {"n": name, "f": func, "b": body}


FIRST = """; %%bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_cmp_gt_u32_e32 vcc, s2, v0
\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB%(f)d_2
; %%bb.1:                                ; %%comment
\tv_mov_b32_e32 v1, 0                   ; %(c)s
\t;;#ASMSTART
\ts_nop 1
\t;;#ASMEND
\tglobal_store_dword v0, v1, s[0:1]
.LBB%(f)d_2:

"""
SECOND = "\ts_load_dword s0, s[4:5], %s\n\ts_waitcnt lgkmcnt(0)\n"


def run(tmp_path, a, b):
    (tmp_path / "a.s").write_text(a)
    (tmp_path / "b.s").write_text(b)
    return subprocess.run([sys.executable, TOOL, str(tmp_path / "a.s"), str(tmp_path / "b.s")], capture_output=True, text=True)


def test_renumbered_labels_and_changed_comments_are_the_same_code(tmp_path):
    a = kernel("_Z5firstPj", 0, FIRST % {"f": 0, "c": "a comment"}) + kernel("_Z6secondPj", 1, SECOND % "0x8")
    b = kernel("_Z6secondPj", 4, SECOND % "0x8") + kernel("_Z5firstPj", 7, FIRST % {"f": 7, "c": "another one, s_nop 9"})
    p = run(tmp_path, a, b)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == 2 and all(l.split()[0] == "SAME" for l in lines), p.stdout
    # the two instruction counts: nine lines that are neither comment nor directive, the label among them
    assert [l.split()[1:] for l in lines] == [["9", "9", "_Z5firstPj"], ["3", "3", "_Z6secondPj"]], p.stdout


def test_one_changed_operand_is_a_difference(tmp_path):
    a = kernel("_Z5firstPj", 0, FIRST % {"f": 0, "c": "c"}) + kernel("_Z6secondPj", 1, SECOND % "0x8")
    b = kernel("_Z5firstPj", 0, FIRST % {"f": 0, "c": "c"}) + kernel("_Z6secondPj", 1, SECOND % "0xc")
    p = run(tmp_path, a, b)
    assert p.returncode == 1, p.stdout + p.stderr
    verdict = {l.split()[-1]: l.split()[0] for l in p.stdout.split("\n")[:-1]}
    assert verdict == {"_Z5firstPj": "SAME", "_Z6secondPj": "DIFF"}, p.stdout


def test_a_missing_kernel_fails(tmp_path):
    both = kernel("_Z5firstPj", 0, FIRST % {"f": 0, "c": "c"}) + kernel("_Z6secondPj", 1, SECOND % "0x8")
    one = kernel("_Z5firstPj", 0, FIRST % {"f": 0, "c": "c"})
    for a, b in ((both, one), (one, both)):
        p = run(tmp_path, a, b)
        assert p.returncode == 1, p.stdout + p.stderr
        assert "MISSING" in p.stdout and "_Z6secondPj" in p.stdout and "SAME" in p.stdout, p.stdout
    assert run(tmp_path, one, one).returncode == 0
    assert run(tmp_path, "", "").returncode == 1       # nothing to compare is not "the same"
