"""CPU: the division by a prepared constant (simpleinfer_amd/csrc/hip/si_magic.h) that the implicit-GEMM, slab, split and Winograd kernels decode
their block and row indices with.  A stand-alone C++ program under AddressSanitizer and UBSan (tests/cpp/test_magic_div.cpp) checks
si_fast_div(n, d, si_magic(d)) == n / d over the header's contract; here also: the header is plain C++, and it is the one place of that scheme."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(ROOT, "simpleinfer_amd", "csrc", "hip")
SANITIZE = ["-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it starts the same under any environment


def _stand_alone(tmp_path, source, include, ok):
    exe = str(tmp_path / os.path.splitext(source)[0])
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined"] + SANITIZE +
                          ["-I" + include, os.path.join(ROOT, "tests", "cpp", source), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ok in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]


def _code(path):
    text = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_quotients_stand_alone_under_sanitizers(tmp_path):
    _stand_alone(tmp_path, "test_magic_div.cpp", HIP_DIR, "magic div ok")


def test_header_is_plain_cpp():
    """nothing of HIP in it but, at most, the guard around the device's multiply-high"""
    code = _code(os.path.join(HIP_DIR, "si_magic.h")).replace("__HIP_DEVICE_COMPILE__", "")
    assert "hip" not in code.lower()
    assert "#include" not in code.replace("#include <cstdint>", "")


def test_the_kernels_share_that_header():
    """every kernel file gets it through si_hip_internal.h; none keeps a multiply-high division or a 2^32 / d constant of its own
    (pixel_shuffle.hip has another scheme -- floor(2^32 / d) + 1, no correction step -- and keeps it)"""
    assert '#include "si_magic.h"' in open(os.path.join(HIP_DIR, "si_hip_internal.h")).read()
    users = []
    for path in sorted(glob.glob(os.path.join(HIP_DIR, "*"))):
        name, code = os.path.basename(path), _code(path)
        if name not in ("si_magic.h", "pixel_shuffle.hip"):
            assert "__umulhi" not in code and "0x100000000ull" not in code, name
        if "si_fast_div(" in code and name != "si_magic.h":
            users.append(name)
            assert "si_magic(" in code, name
    assert users == ["conv_igemm.hip", "conv_igemm_f16.hip", "conv_slab_f16.hip", "conv_split3.hip", "conv_wino23.hip", "conv_wino23_split.hip"]
