"""CPU: the planner's view rule without a device (tests/cpp/test_view_rule.cpp: for every fp16 conv form and operand, and the broadcast
BinaryOp, whether a channel slice at a given pixel stride and channel offset is taken, against answers spelled out in the program).  The rule
is a header of pure functions (csrc/host/view_rule.h), so the program links nothing."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_view_rule_table(tmp_path):
    exe = str(tmp_path / "test_view_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "simpleinfer_amd", "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "test_view_rule.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "view rule ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
