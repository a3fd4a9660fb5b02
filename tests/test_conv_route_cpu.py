"""CPU: Conv2d's host-side decisions without a device (tests/cpp/test_conv_route.cpp: for a table of layers and f32_split settings, the kernel
family per storage pair, the weight image that family reads and the Winograd tile, against values spelled out in the program).  A stand-alone
program linked against the two product libraries, as tests/test_gpu_cpp_api.py links test_layers.cpp; it calls nothing that needs a device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv_route_table(native_libs, tmp_path):
    exe = str(tmp_path / "test_conv_route")
    pkg = os.path.join(ROOT, "simpleinfer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-ignored-qualifiers", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "test_conv_route.cpp"),
                           "-L" + pkg, "-lsimpleinfer_amd", "-lsi_hip", "-Wl,-rpath," + pkg, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "conv route ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
