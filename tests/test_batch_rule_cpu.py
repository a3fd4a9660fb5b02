"""CPU: the per-image rule of the batch-split modes (csrc/host/batch_rule.h) as a stand-alone program under AddressSanitizer and UBSan
(tests/cpp/test_batch_rule.cpp: a table of (type, parameters, operand shapes and batch axes) -> verdict with both verdicts for every layer
class, the coincidence cases, FollowBatchAxis, and FindBatchMixing on hand-built graphs).  The type strings of layer_registry.cpp are handed to
the program: a type the registry serves and the rule has no row for fails here.  A child process: nothing is loaded into this interpreter."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "simpleinfer_amd", "csrc", "host")


def registry_types():
    return re.findall(r'SI_ENTRY\("([^"]+)"', open(os.path.join(HOST, "layer_registry.cpp")).read())


def test_batch_rule_stand_alone_under_sanitizers(tmp_path):
    types = registry_types()
    assert len(types) >= 74 and "nn.Softmax" in types and "models.yolo.Detect" in types, types
    exe = str(tmp_path / "test_batch_rule")
    # (-O0: the table is a few hundred aggregate initialisers, which the instrumented optimiser takes a minute over)
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it starts the same under any environment
                           "-I" + HOST, os.path.join(ROOT, "tests", "cpp", "test_batch_rule.cpp"), "-o", exe])
    r = subprocess.run([exe] + types, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "batch rule ok" in r.stdout and "%d registry types" % len(types) in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    # ... and the check of the registry's types is live: a type string without a row is reported
    r = subprocess.run([exe, "nn.Conv2d", "nn.LayerNorm"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "the batch rule has no row for it" in r.stdout and "[nn.LayerNorm]" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
