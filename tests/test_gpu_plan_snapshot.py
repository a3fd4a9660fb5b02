"""GPU: the engine's plan for every configuration of tests/plan_snapshot.py equals the record tests/golden/plan_snapshot.json -- the launch order,
the fused-away operators, the concat aliases and the arena footprint as LoadModel planned them, and the kernel every step of one forward ran.
Equality of lists, no tolerance.  The schedule tests launch nothing: run them first (-k schedule), so a planner slip shows as a list diff before a
mis-planned launch runs."""
import pytest

import plan_snapshot as ps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def si(gpu):
    import simpleinfer_amd
    return simpleinfer_amd


@pytest.fixture(scope="module")
def record():
    rec = ps.load_record()
    assert sorted(rec) == sorted(ps.IDS), "the record and the configuration list disagree: regenerate it (tests/plan_snapshot.py --write)"
    return rec


@pytest.mark.parametrize("cfg", ps.CONFIGS, ids=ps.IDS)
def test_schedule_matches_snapshot(si, record, cfg):
    got, want = ps.collect_schedule(si, cfg), record[cfg.id]["schedule"]
    for key in ps.SCHEDULE_KEYS:
        assert got[key] == want[key], "%s: %s differs from the record" % (cfg.id, key)


@pytest.mark.parametrize("cfg", ps.CONFIGS, ids=ps.IDS)
def test_kernels_match_snapshot(si, record, cfg):
    assert ps.collect_kernels(si, cfg) == record[cfg.id]["kernels"], cfg.id
