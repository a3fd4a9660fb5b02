"""CPU: the host-side plan the reduction files share (simpleinfer_amd/csrc/hip/si_reduce_plan.h: the fold of a mask into levels, the output
pixels under a mask, the lanes-per-row rule, the shared half of the descriptor checks, the kernel-name helper), checked by a stand-alone C++
program under AddressSanitizer and UBSan (tests/cpp/test_reduce_plan.cpp).  Here also: the header is plain C++, and no kernel file keeps a
lane butterfly, a workgroup combine or an axis fold of its own ("Device commons")."""
import os
import re
import subprocess

from test_views_cpu import HIP_DIR, ROOT, SANITIZE, _code, _sources

COMMONS = ("si_hip_internal.h", "si_reduce_dev.h", "si_reduce_plan.h")


def test_reduce_plan_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_reduce_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined"] + SANITIZE +
                          ["-I" + HIP_DIR, os.path.join(ROOT, "tests", "cpp", "test_reduce_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "reduce plan ok" in r.stdout and "448 fold cases" in r.stdout and "runtime error" not in r.stderr, \
        r.stdout[-4000:] + r.stderr[-4000:]


def test_header_is_plain_cpp():
    code = _code(os.path.join(HIP_DIR, "si_reduce_plan.h"))
    assert "hip" not in code.lower() and "__device__" not in code and "__host__" not in code
    assert "#include" not in code.replace("#include <cstdint>", "").replace('#include "si_views.h"', "")
    assert '#include "si_reduce_plan.h"' in open(os.path.join(HIP_DIR, "si_reduce_dev.h")).read()
    assert '#include "si_reduce_dev.h"' in open(os.path.join(HIP_DIR, "si_hip_internal.h")).read()


def test_no_kernel_file_keeps_a_lane_butterfly_of_its_own():
    loop = re.compile(r"for\s*\([^;{}]*;[^;{}]*;[^{}]*\boff\s*>>=\s*1\s*\)")       # for (...; ...; off >>= 1)
    found = []
    for name, code in _sources():
        for m in loop.finditer(code):
            rest = code[m.end():]
            body = rest[:rest.index("}") + 1] if rest.lstrip().startswith("{") else rest[:rest.index(";") + 1]
            if "__shfl_xor(" in body:
                found.append(name)
    assert found == ["si_reduce_dev.h"], found                                        # si_team, once


def test_no_kernel_file_keeps_a_fold_or_a_combine_of_its_own():
    definition = r"\b%s\s*\([^;{}()]*\)\s*\{"        # name(parameters) {
    for name, code in _sources():
        if name in COMMONS:
            continue
        for helper in ("levels_of", r"\w+_team(?:_max|_sum)?", r"\w+_block_(?:max|sum)", r"(?:sm|rd|ln|gn)_block"):
            assert not re.search(definition % helper, code), (name, helper)
        assert not re.search(r"\bstruct\s+Levels\b", code), name
        assert not re.search(r"a\s*!=\s*a\s*\|\|\s*a\s*>\s*b", code), name            # the NaN-keeping maximum: SiMaxNan
    plan = _code(os.path.join(HIP_DIR, "si_reduce_plan.h"))
    assert len(re.findall(definition % "si_fold_levels", plan)) == 1
    dev = _code(os.path.join(HIP_DIR, "si_reduce_dev.h"))
    assert len(re.findall(definition % "si_team", dev)) == 1 and len(re.findall(definition % "si_block", dev)) == 1
    # the axis bits are spelled once on the device side's host half
    for name, code in _sources():
        if name != "si_reduce_plan.h":
            assert not re.search(r"\bkAxis[NHWC]\s*=", code), name
