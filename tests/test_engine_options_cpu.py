"""CPU: the engine's options as a value type (csrc/host/engine_options.h) as a stand-alone program under AddressSanitizer and UBSan
(tests/cpp/test_engine_options.cpp: the defaults, the 34 keys and their rules, one field per key, what a lane or the sliced pipeline's engine
inherits).  A child process: nothing is loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_engine_options_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_engine_options")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it starts the same under any environment
                           "-I" + os.path.join(ROOT, "simpleinfer_amd", "csrc", "host"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_engine_options.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "engine options ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
