"""CPU: the typed pnnx parameter readers (csrc/host/pnnx/param_read.h) as a stand-alone program under AddressSanitizer and UBSan
(tests/cpp/test_param_read.cpp: every reader on a missing key, type 0, the string "None", int, float, bool, list and a wrong type, with both
rules for "None").  A child process: nothing is loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_param_readers_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_param_read")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it starts the same under any environment
                           "-I" + os.path.join(ROOT, "simpleinfer_amd", "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "test_param_read.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "param read ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
