"""CPU: the activation arena packer (csrc/host/arena_plan.h) as a stand-alone program under AddressSanitizer and UBSan (tests/cpp/test_arena_plan.cpp:
hand-worked layouts and seeded random cases held to the packer's invariants).  A child process: nothing is loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arena_packer_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_arena_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it starts the same under any environment
                           "-I" + os.path.join(ROOT, "simpleinfer_amd", "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "test_arena_plan.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "arena plan ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
