"""GPU: si_hip_yolo_postprocess_f32 (simpleinfer_amd/csrc/hip/postprocess.hip: confidence filter, rank-count sort, two greedy NMS kernels,
compaction) on the adversarial inputs of tests/post_reference.py, against the numpy rule there -- which tests/test_postprocess_cpu.py holds to
the C oracle bit for bit.  Every comparison is EXACT (post_reference.assert_same: NaN in the same places, the same bits everywhere else,
the sign of zero included), into a sentinel-filled `dets` whose rows behind the picks must still hold the sentinel; there is no tolerance.
Besides the case matrix: nc = 1 (the segments path and the agnostic kernel must write the same bytes), max_det around the number of picks,
run-to-run determinism under atomic arrival order, a workspace that holds leftovers, the refusals at ne = 129 and n = 65536, and the image
strides of the resize / letterbox batch entries (the second half of postprocess.hip)."""
import numpy as np
import pytest

import post_reference as pr
from util import assert_exact

pytestmark = pytest.mark.gpu

F = np.float32
SENT = 0x7B                      # dets is pre-filled with this byte (1.3e36 as fp32)
SENT32 = np.uint32(0x7B7B7B7B)
SI_E_UNSUPPORTED = -2            # include/si_hip.h


@pytest.fixture(scope="module")
def hops(gpu):
    from simpleinfer_amd import hipops
    return hipops


def run_raw(hops, case, agnostic, adjusted, max_det=None, workspace=None):
    """one call into a sentinel-filled dets buffer -> (dets as they lie in memory [n][max_det][6], counts)"""
    n, rows, _ = case.pred.shape
    max_det = rows if max_det is None else max_det
    dd = hops.DeviceBuffer(max(n * max_det * 6 * 4, 16))
    dd.fill(SENT)
    _, cnt = hops.yolo_postprocess(case.pred, case.prob_thr, case.nms_thr, agnostic, case.adjust if adjusted else None, max_det=max_det,
                                   workspace=workspace, dets_dev=dd)
    raw = dd.to_numpy((n, max_det, 6)) if max_det else np.zeros((n, 0, 6), F)
    return raw, cnt


def check(raw, cnt, ref, max_det, what):
    """counts report every pick; the first min(count, max_det) rows are the rule's, the rest still hold the sentinel"""
    rdets, rcnt = ref
    assert list(cnt) == list(rcnt), "%s: counts %s, expected %s" % (what, list(cnt), list(rcnt))
    for b, want in enumerate(rdets):
        k = min(int(rcnt[b]), max_det)
        pr.assert_same(raw[b, :k], want[:k], "%s image %d" % (what, b))
        behind = raw[b, k:].view(np.uint32)
        assert (behind == SENT32).all(), "%s image %d: %d words behind the %d stored rows were written" % (what, b, int((behind != SENT32).sum()), k)


# ---- the matrix -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adjusted", [False, True], ids=["raw", "adjust"])
@pytest.mark.parametrize("agnostic", [False, True], ids=["perclass", "agnostic"])
@pytest.mark.parametrize("cid", pr.CASE_IDS)
def test_case_equals_the_rule(hops, cid, agnostic, adjusted):
    c = pr.cases()[cid]
    raw, cnt = run_raw(hops, c, agnostic, adjusted)
    check(raw, cnt, pr.expected(cid, agnostic, adjusted), c.pred.shape[1], cid)


@pytest.mark.parametrize("cid", ["bins_1", "counts_257_nc1"])
def test_one_class_both_paths_write_the_same_bytes(hops, cid):
    c = pr.cases()[cid]
    assert c.pred.shape[2] == 6
    (seg, scnt), (agn, acnt) = run_raw(hops, c, False, True), run_raw(hops, c, True, True)
    assert list(scnt) == list(acnt) and seg.tobytes() == agn.tobytes()
    check(seg, scnt, pr.expected(cid, False, True), c.pred.shape[1], cid)


@pytest.mark.parametrize("agnostic", [False, True], ids=["perclass", "agnostic"])
@pytest.mark.parametrize("delta", ["zero", "one", "picks-1", "picks", "picks+1"])
def test_max_det_around_the_number_of_picks(hops, delta, agnostic):
    """image 0 picks all 129 (more than max_det), image 1 one (fewer), image 2 (random dense) is the one max_det is measured from"""
    c = pr.cases()["counts_129"]
    ref = pr.expected(c.id, agnostic, True)
    picks = int(ref[1][2])
    assert 2 < picks < 129
    max_det = {"zero": 0, "one": 1, "picks-1": picks - 1, "picks": picks, "picks+1": picks + 1}[delta]
    raw, cnt = run_raw(hops, c, agnostic, True, max_det=max_det)
    check(raw, cnt, ref, max_det, "max_det %d" % max_det)


@pytest.mark.parametrize("agnostic", [False, True], ids=["perclass", "agnostic"])
def test_three_runs_the_same_bytes(hops, agnostic):
    """survivors arrive through atomicAdd in whatever order the blocks run; the sort key carries the element index and must cancel that"""
    c = pr.cases()["counts_1025"]
    runs = [run_raw(hops, c, agnostic, True) for _ in range(3)]
    for raw, cnt in runs[1:]:
        assert raw.tobytes() == runs[0][0].tobytes() and cnt.tobytes() == runs[0][1].tobytes()
    check(runs[0][0], runs[0][1], pr.expected(c.id, agnostic, True), c.pred.shape[1], c.id)


@pytest.mark.parametrize("agnostic", [False, True], ids=["perclass", "agnostic"])
def test_workspace_leftovers_do_not_matter(hops, agnostic):
    """only count, bin_count and keep are zeroed per call: a workspace full of 0x7B bytes, and one that a call with more rows has just used,
    must give the bytes of a fresh one"""
    from simpleinfer_amd import _native
    small, large = pr.cases()["counts_129"], pr.cases()["counts_1025"]
    assert large.pred.shape[1] > small.pred.shape[1] and large.pred.shape[0] == small.pred.shape[0]
    fresh, fcnt = run_raw(hops, small, agnostic, True)
    check(fresh, fcnt, pr.expected(small.id, agnostic, True), small.pred.shape[1], small.id)
    ws = hops.DeviceBuffer(_native.hip().si_hip_yolo_postprocess_workspace_bytes(*(int(v) for v in large.pred.shape)))
    ws.fill(SENT)
    dirty, dcnt = run_raw(hops, small, agnostic, True, workspace=ws)
    assert dirty.tobytes() == fresh.tobytes() and list(dcnt) == list(fcnt), "a workspace filled with 0x7B bytes"
    big, bcnt = run_raw(hops, large, agnostic, True, workspace=ws)
    check(big, bcnt, pr.expected(large.id, agnostic, True), large.pred.shape[1], large.id)
    again, acnt = run_raw(hops, small, agnostic, True, workspace=ws)
    assert again.tobytes() == fresh.tobytes() and list(acnt) == list(fcnt), "a workspace a larger call has used"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def _entry_rc(hops, n, rows, ne, agnostic):
    """the entry's return code on zero predictions, with buffers that would serve the call; counts come back as they were left"""
    from simpleinfer_amd import _native
    H = _native.hip()
    pred = hops.DeviceBuffer.from_numpy(np.zeros((n, rows, ne), F))
    wsb = H.si_hip_yolo_postprocess_workspace_bytes(n, rows, ne)
    ws = hops.DeviceBuffer(max(wsb, 16))
    dets = hops.DeviceBuffer(n * 6 * 4)
    cnt = hops.DeviceBuffer.from_numpy(np.full(n, -7, np.int32), out=True)
    rc = H.si_hip_yolo_postprocess_f32(pred.ptr, n, rows, ne, 0.25, 0.45, int(agnostic), None, dets.ptr, cnt.ptr, 1, ws.ptr, wsb, None)
    hops.sync()
    return rc, cnt.to_numpy((n,), np.int32)


@pytest.mark.parametrize("agnostic", [False, True], ids=["perclass", "agnostic"])
def test_refusals_come_before_any_device_work(hops, agnostic):
    rc, cnt = _entry_rc(hops, 1, 130, 129, agnostic)          # 128 rows of 129 floats do not fit the filter's 64 KB stage
    assert rc == SI_E_UNSUPPORTED and (cnt == -7).all()
    rc, cnt = _entry_rc(hops, 65536, 1, 6, agnostic)          # n is a grid's y extent
    assert rc == SI_E_UNSUPPORTED and (cnt == -7).all()
    rc, cnt = _entry_rc(hops, 1, 130, 128, agnostic)          # the last ne that runs (bins_123 holds it to the rule)
    assert rc == 0 and list(cnt) == [0]
    assert pr.cases()["bins_123"].pred.shape[2] == 128 and pr.cases()["bins_123"].pred.shape[1] > 128


# ---- image strides of the resize / letterbox batch entries ------------------------------------------------------------------------------------
def _u8(seed, shape):
    return np.random.Generator(np.random.Philox(seed)).integers(0, 256, shape, dtype=np.uint8)


def test_resize_with_image_strides_on_both_sides(hops):
    imgs = _u8(801, (3, 33, 47, 3))
    per = 20 * 64 * 3
    dense = hops.resize_bilinear_u8c3(imgs, 20, 64)
    with hops.guard_bands(0xFF):          # also holds the source, gaps included, to the bytes that were uploaded
        raw = hops.resize_bilinear_u8c3(imgs, 20, 64, src_stride=33 * 47 * 3 + 37, src_fill=SENT, dst_stride=per + 29, dst_fill=SENT, full=True)
    assert raw.shape == (3, per + 29)
    assert_exact(raw[:, :per].reshape(3, 20, 64, 3), dense, "resize with image strides")
    assert (raw[:, per:] == SENT).all(), "the gap behind each destination image"


@pytest.mark.parametrize("sh,sw,size", [(48, 64, 64), (30, 50, 63)], ids=["vector_path", "per_image_path"])
def test_letterbox_batch_with_a_source_stride(hops, sh, sw, size):
    hr, wr, _, pt, pl = hops.letterbox_geometry(sh, sw, size, size)
    imgs = _u8(802 + size, (3, hr, wr, 3))
    dense = hops.letterbox_batch(imgs, size, size, pt, pl)
    with hops.guard_bands(0xFF):
        got = hops.letterbox_batch(imgs, size, size, pt, pl, src_stride=hr * wr * 3 + 13, src_fill=SENT)
    assert_exact(got, dense, "letterbox batch with a source stride")


def test_resize_letterbox_batch_with_a_source_stride(hops):
    frames = _u8(803, (3, 31, 17, 3))
    dense = hops.resize_letterbox_batch(frames, 63, 63)
    with hops.guard_bands(0xFF):
        got = hops.resize_letterbox_batch(frames, 63, 63, src_stride=31 * 17 * 3 + 11, src_fill=SENT)
    assert_exact(got, dense, "resize + letterbox with a source stride")
