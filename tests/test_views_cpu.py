"""CPU: the view rules the host side of every kernel file shares (simpleinfer_amd/csrc/hip/si_views.h: alignment, vector width, byte-range overlap,
view extent, the strided-window test), checked by a stand-alone C++ program under AddressSanitizer and UBSan (tests/cpp/test_views.cpp).  Here
also: the header is plain C++, and the kernel files keep no copy of these helpers, of the channel-vector load / store of si_hip_internal.h, or
of a kernel per storage type ("Device commons")."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(ROOT, "simpleinfer_amd", "csrc", "hip")
SANITIZE = ["-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it starts the same under any environment
COMMONS = ("si_hip_internal.h", "si_views.h")


def _code(path):
    text = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def _sources():
    return [(os.path.basename(p), _code(p)) for p in sorted(glob.glob(os.path.join(HIP_DIR, "*"))) if os.path.isfile(p)]


def test_view_rules_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_views")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined"] + SANITIZE +
                          ["-I" + HIP_DIR, os.path.join(ROOT, "tests", "cpp", "test_views.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "views ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]


def test_header_is_plain_cpp():
    code = _code(os.path.join(HIP_DIR, "si_views.h"))
    assert "hip" not in code.lower() and "__device__" not in code and "__host__" not in code
    assert "#include" not in code.replace("#include <cstdint>", "")
    assert '#include "si_views.h"' in open(os.path.join(HIP_DIR, "si_hip_internal.h")).read()


def test_no_kernel_file_keeps_a_vector_load_or_store_of_its_own():
    pattern = re.compile(r"\b(\w+_(?:load|store))\s*\(\s*(?:const\s+)?T\s*\*\s*\w*\s*,\s*(?:const\s+)?float\s*\(\s*&\s*\w*\s*\)\s*\[\s*VW\s*\]")
    commons = _code(os.path.join(HIP_DIR, "si_hip_internal.h"))
    assert sorted(m.group(1) for m in pattern.finditer(commons)) == []       # named si_load_vec / si_store_vec: not *_load / *_store
    assert "void si_load_vec(const T* p, float (&v)[VW])" in commons and "void si_store_vec(T* p, const float (&v)[VW])" in commons
    for name, code in _sources():
        if name not in COMMONS:
            assert pattern.findall(code) == [], name
            assert "si_load_vec(const" not in code and "si_store_vec(T" not in code, name      # ... nor a second definition under the shared name


def test_no_kernel_file_keeps_a_view_helper_of_its_own():
    definition = r"\b%s\s*\([^;{}()]*\)\s*\{"        # name(parameters) {
    for name, code in _sources():
        if name in COMMONS:
            continue
        for helper in ("overlap", "intersects", "aligned16", "Aligned16"):
            assert not re.search(definition % helper, code), (name, helper)
        for m in re.finditer(definition % "views_overlap", code):
            assert name in ("reduce.hip", "activation_param.hip"), name                        # the two wrappers that feed their descriptor ...
            body = code[m.end():code.index("}", m.end())]
            assert "si_strided_windows_overlap(" in body and "uintptr_t" not in body, name     # ... to the shared rule
        for m in re.finditer(r"\bview_extent\s*\(([^;{}()]*)\)\s*\{", code):
            assert m.group(1).count(",") != 4, name                                            # (n, h, w, ld, c): si_view_extent
        assert not re.search(r"uintptr_t>\s*\(\s*[\w.>-]+\s*\)\s*&\s*15\b", code) or name in DEVICE_SIDE_ALIGNMENT, name


# a kernel that asks at run time whether its own destination allows 16-byte stores: device code, which the host helper does not serve
DEVICE_SIDE_ALIGNMENT = ("conv_igemm_f16.hip", "conv_split3.hip", "conv_stem_roll.hip")


def test_every_pointwise_kernel_exists_once():
    assert not os.path.exists(os.path.join(HIP_DIR, "ops_f16.hip"))
    for name, code in _sources():
        assert not re.search(r"\w*_h_kernel\b", code), name
