"""CPU: the C-ABI of include/si_nearest.h without a device (names, the bound table, the structure, every refusal before a launch, the
workspace against the plan restated here) and nearest_plan.h as a stand-alone C++ program under ASan and UBSan (a child process)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import containment as ct
import nearest_reference as nref
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_nearest.h")
BADARG, UNSUPPORTED = -1, -2
ENTRIES = ["si_hip_nearest_f16", "si_hip_nearest_f32", "si_hip_nearest_kernel_name", "si_hip_nearest_workspace_bytes"]


def test_header_bound_table_and_structure(native_libs):
    H, _ = native_libs
    declared = ct.header_functions(HEADER)
    assert sorted(declared) == sorted(H._si_nearest_signatures) == ENTRIES
    others = [getattr(H, k) for k in vars(H) if k.startswith("_si_") and k.endswith("signatures") and k != "_si_nearest_signatures"]
    assert len(others) >= 21 and not any(set(declared) & set(o) for o in others)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    assert all(hasattr(raw, name) for name in declared)
    m = re.search(r"typedef struct SiNearestDesc \{(.*?)\} SiNearestDesc;", open(HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [(n.strip(), C.c_int) for names in re.findall(r"\bint\s+([^;]+);", body) for n in names.split(",")]
    assert fields == list(_native.SiNearestDesc._fields_) and C.sizeof(_native.SiNearestDesc) == 13 * 4


@pytest.mark.parametrize("fn,half", [("si_hip_nearest_f32", 0), ("si_hip_nearest_f16", 1)])
def test_refusals_without_a_device(native_libs, fn, half):
    """every refusal happens before any device call: the pointers are compared, never followed"""
    H, _ = native_libs
    esize = 2 if half else 4
    a, b, i, s, o, w = (C.c_void_p(k << 40) for k in (1, 2, 3, 4, 5, 6))
    desc = hipops.nearest_desc
    call = lambda d, x1=a, x2=b, idx=i, dist=s, rows=o, ws=w, nbytes=1 << 30: getattr(H, fn)(C.byref(d), x1, x2, idx, dist, rows, ws, nbytes, None)
    named = lambda d, x1=a, x2=b, rows=o: H.si_hip_nearest_kernel_name(C.byref(d), x1, x2, rows, half).decode()
    good = lambda **kw: desc((3, 5, 8), (3, 4, 8), **kw)
    assert named(good()) == "nearest_kernel<%s, true, 1>" % ("_Float16" if half else "float")     # (never launched here)
    assert getattr(H, fn)(None, a, b, i, s, o, w, 0, None) == BADARG
    assert call(good(), x1=None) == call(good(), x2=None) == call(good(), idx=None, dist=None, rows=None) == BADARG
    for field in ("b1", "b2", "p", "r", "m"):
        for value in (0, -3):
            bad = good()
            setattr(bad, field, value)
            assert call(bad) == BADARG and named(bad) == "none", (field, value)
    assert call(desc((3, 5, 8), (2, 4, 8))) == BADARG                                                      # batches 3 and 2
    assert call(desc((5, 8), (1, 8), k=2)) == BADARG and named(desc((5, 8), (1, 8), k=1)) != "none"        # k = 2 with one row
    for k in (0, 3, -1):
        assert call(good(k=k)) == BADARG, k
    assert call(good(splits=17)) == call(good(splits=-1)) == BADARG
    assert call(good(x1_ld=7)) == call(good(x2_ld=7)) == call(good(rows_ld=7)) == BADARG
    bad = good()
    bad.x2_sb = 31
    assert call(bad) == BADARG                                                                             # batch items that meet
    # the workspace: needed with more than one split only; null, misaligned or one byte short
    need = H.si_hip_nearest_workspace_bytes(C.byref(good(k=2, splits=3)))
    assert need == 3 * 5 * 2 * 3 * 8
    assert call(good(k=2, splits=3), nbytes=need - 1) == call(good(k=2, splits=3), ws=None) == call(good(k=2, splits=3), ws=C.c_void_p(w.value + 4)) == BADARG
    assert call(good(k=2, splits=3), ws=C.c_void_p(a.value + 8)) == call(good(k=2, splits=3), ws=C.c_void_p(o.value - 8)) == BADARG   # ... or on x1 / rows
    # an output on an operand or on another output
    assert call(good(), rows=a) == call(good(), idx=C.c_void_p(b.value + (3 * 4 * 8 - 1) * esize)) == call(good(), dist=i) == BADARG
    assert named(good(), rows=C.c_void_p(a.value + 8)) == "none"
    # unsupported: R * 64 beyond 31 bits, element offsets beyond 31 bits, and under fp16 rows or views off the 16-byte vector
    assert call(desc((5, 1), (1 << 25, 1))) == UNSUPPORTED and call(desc((2, 1 << 27, 8), (4, 8))) == UNSUPPORTED
    assert call(good(k=5, x1_ld=7)) == BADARG and call(desc((1 << 20, 8), (1 << 25, 8), x1_ld=7)) == BADARG      # SI_E_BADARG is looked for first
    f16_only = [desc((5, 12), (4, 12)), good(x1_ld=12), good(rows_ld=20)]
    for d in f16_only:                                                                                     # (what fp32 accepts is named, never launched)
        assert (named(d) == "none") == bool(half) and (not half or call(d) == UNSUPPORTED)
    assert (named(good(), x1=C.c_void_p(a.value + 8)) == "none") == bool(half) and (not half or call(good(), x1=C.c_void_p(a.value + 8)) == UNSUPPORTED)
    assert hipops.nearest_kernel_name((64, 6), (64, 6), 2) == "nearest_kernel<float, false, 2>"
    assert hipops.nearest_kernel_name((64, 6), (64, 6), half=True) == "none"


def plan_splits(b, p, r, forced=0, cus=256):
    """the choice of include/si_nearest.h restated"""
    panels, tiles = -(-p // 64) * b, -(-r // 64)
    return forced or (1 if panels >= cus else min(16, tiles, cus // panels))


@pytest.mark.parametrize("b,p,r,k,forced", [(1, 8192, 8192, 1, 0), (1, 256, 16384, 2, 0), (3, 70, 200, 2, 0), (1, 5, 65, 1, 0), (1, 5, 65, 1, 16), (2, 1024, 1024, 2, 0),
                                            (1, 64 * 255, 6400, 1, 0), (1, 64 * 256, 6400, 1, 0), (1, 8192, 8192, 1, 2)])
def test_workspace_bytes_against_the_plan(native_libs, b, p, r, k, forced):
    H, _ = native_libs
    splits = plan_splits(b, p, r, forced)
    want = b * p * k * splits * 8 if splits > 1 else 0
    assert H.si_hip_nearest_workspace_bytes(C.byref(hipops.nearest_desc((b, p, 8), (r, 8), k, forced))) == want
    assert H.si_hip_nearest_workspace_bytes(None) == 0 and H.si_hip_nearest_workspace_bytes(C.byref(hipops.nearest_desc((b, p, 8), (r, 8), 3, forced))) == 0


@pytest.mark.parametrize("module", [False, True], ids=["F.embedding", "nn.Embedding"])
def test_lowering_on_the_written_graph(native_libs, tmp_path, module):
    b = mg.build_toy_vq(module=module)
    paths = [str(tmp_path / n) for n in ("a.param", "a.bin", "b.param", "b.bin")]
    b.save(*paths[:2])
    engine.pnnx_save(*paths, expand=True)
    before = [_parse(ln) for ln in b.lines]
    after = [_parse(ln) for ln in open(paths[2]).read().splitlines()[2:]]
    assert [o[0] for o in before][-4:] == ["torch.cdist", "torch.argmin", "nn.Embedding" if module else "F.embedding", "pnnx.Output"]
    assert [o[0] for o in after] == [o[0] for o in before if o[0] not in ("torch.argmin", "F.embedding", "nn.Embedding")]
    (old,), (new,) = [[o for o in ops if o[0] == "torch.cdist"] for ops in (before, after)]
    assert new[1] == old[1] and new[2] == old[2] and new[3] == before[-2][3] == after[-1][2]      # (z, codebook) -> q, which the output reads
    assert new[4] == dict(old[4], nearest_rows="1") and b.shapes[new[3][0]] == (2, 64, 16)
    for name, bad in nref.vq_refusals().items():                                                      # ... and a chain that misses a condition is not written
        bad.save(*paths[:2])
        with pytest.raises(RuntimeError, match="rc=6"):
            engine.pnnx_save(*paths, expand=True)


def test_plan_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_nearest_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleinfer_amd", "csrc", "hip"),
                           os.path.join(ROOT, "tests", "cpp", "test_nearest_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "nearest plan ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
