"""GPU: containment of every compute entry of the C-ABI (include/si_hip.h).  The rest of the suite holds the kernels' VALUES to the oracle; this
file holds their ADDRESSES: each case of tests/containment.py runs plain, then twice under hipops.guard_bands -- every device buffer of the call
between two 4096-byte bands and every gap of every strided view filled with one byte pattern (0xFF: NaN; 0x7B: a large finite number that wins
every max) -- and
  (a) all bands of all buffers are intact (inputs, weights, bias, residual, workspace, outputs);
  (b) every byte of an output buffer outside the destination slice still holds the pre-fill;
  (c) the destination slice has the same bits in all three runs, and is finite;
  (d) every input buffer reads back unchanged (the f32_split range-guard word included: it stays 0).
Parity with the oracle is not repeated here.  The bands are part of the test's own allocations: an overrun is observed, never provoked."""
import contextlib

import numpy as np
import pytest

import containment as ct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hops(gpu):
    from simpleinfer_amd import hipops
    return hipops


def _run(hops, case, byte, guarded):
    hops.LAST_KERNEL_NAME.clear()
    del hops.LAST_ENTRIES[:]
    with hops.plan(**case.plan) if case.plan else contextlib.nullcontext():
        if not guarded:
            return case.run(hops, hops.ByteFill(byte)), dict(hops.LAST_KERNEL_NAME), None
        with hops.guard_bands(byte) as g:      # (a) and (d) are checked when the block ends
            outs = case.run(hops, hops.ByteFill(byte))
        return outs, dict(hops.LAST_KERNEL_NAME), g


HEADER_FUNCTIONS = set(ct.header_functions())


def _launched(hops):
    """the compute entries among the calls hipops recorded; a label that is no function of the header is a wrapper's mistake"""
    unknown = sorted(set(hops.LAST_ENTRIES) - HEADER_FUNCTIONS)
    assert not unknown, "hipops recorded calls the header does not declare: %s" % unknown
    return {e for e in hops.LAST_ENTRIES if not ct.is_exempt(e)}


@pytest.mark.parametrize("case", ct.CASES, ids=[c.id for c in ct.CASES])
def test_containment(hops, case):
    plain, plain_kernels, _ = _run(hops, case, 0x00, False)
    assert plain, "a case returns its destinations"
    launched = _launched(hops)
    assert set(case.entries) <= launched, "%s names %s but launched %s" % (case.id, case.entries, sorted(launched))
    if "f16_tile" in case.plan:
        assert plain_kernels["f16_tile_variant"] == case.plan["f16_tile"], "%s: the forced fp16 tile was not taken: %s" % (case.id, plain_kernels)
    for o in plain:
        ct.assert_outside_fill(o.full, o.c_off, o.c, 0x00, "%s, plain run, %s" % (case.id, o.name))
        ct.assert_finite(o.dest, "%s, plain run, %s" % (case.id, o.name))
    for byte in ct.PATTERNS:
        outs, kernels, g = _run(hops, case, byte, True)
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked >= 2, "%s: the guard saw %d buffers" % (what, g.checked)
        assert kernels == plain_kernels, "%s: the guarded call took another kernel: %s vs %s" % (what, kernels, plain_kernels)
        assert _launched(hops) == launched, "%s: the guarded call launched other entries: %s vs %s" % (what, sorted(_launched(hops)), sorted(launched))
        assert [o.name for o in outs] == [o.name for o in plain]
        for o, p in zip(outs, plain):
            ct.assert_outside_fill(o.full, o.c_off, o.c, byte, "%s, %s" % (what, o.name))                      # (b)
            ct.assert_same_bits(o.dest, p.dest, "%s, %s: guarded + pattern-filled vs plain" % (what, o.name))   # (c)
            if o.name.startswith("range_flag"):
                assert not o.full.any(), "%s: the range guard tripped: %s" % (what, o.full)


def test_guarded_buffers_keep_the_alignment_and_the_plain_path_is_untouched(hops):
    """the launchers choose kernels by pointer alignment: a guarded payload starts 256-byte aligned like a plain one, its back band at its last
    byte + 1; outside the context a buffer is the bare allocation it always was"""
    plain = hops.DeviceBuffer(100)
    assert plain.ptr % 256 == 0 and plain._base == plain.ptr and plain._guard is None
    with hops.guard_bands(0x7B, 512) as g:
        b = hops.DeviceBuffer(100)
        assert b.ptr % 256 == 0 and b.ptr - b._base == 512 and b._alloc == 100 + 1024
        raw = hops.DeviceBuffer.view(b._base, b._alloc).to_numpy((b._alloc,), np.uint8)
        assert (raw == 0x7B).all(), "bands and payload start as the pattern"
        v = hops.DeviceBuffer.from_numpy(np.arange(25, dtype=np.float32))
        raw = hops.DeviceBuffer.view(v._base, v._alloc).to_numpy((v._alloc,), np.uint8)
        assert (raw[:512] == 0x7B).all() and (raw[512 + 100:] == 0x7B).all() and np.array_equal(raw[512:612].view(np.float32), np.arange(25, dtype=np.float32))
        assert g.buffers == [b, v]
    assert g.checked == 2 and b.ptr is None and v.ptr is None
    with pytest.raises(AssertionError):
        with hops.guard_bands(0xFF, 1000):
            pass
    assert hops.DeviceBuffer(8)._guard is None


def _copy(hops, src, dst_ptr, pixels, c, in_ld, out_ld):
    from simpleinfer_amd import _native
    rc = _native.hip().si_hip_copy_channels_f32(src.ptr, pixels, c, in_ld, dst_ptr, out_ld, None)
    assert rc == 0, rc
    hops.sync()


# ---- the harness must be shown to see (every access below stays inside the test's own allocations) ----
def test_positive_control_a_kernel_that_writes_four_channels_more_fails_the_outside_check(hops):
    """copy_channels given a slice four channels wider than the one the checker is told about: check (b) names the first pixel and channel; the
    truthful description of the same call passes"""
    x = ct.R(1, (2, 3, 5, 12))
    y = hops.copy_channels(x, out_ld=24, out_c_off=4, out_fill=hops.ByteFill(0x7B), full=True)
    ct.assert_outside_fill(y, 4, 12, 0x7B, "truthful")                      # (iii) negative control
    with pytest.raises(AssertionError) as e:
        ct.assert_outside_fill(y, 4, 8, 0x7B, "told 8 channels, the kernel wrote 12")
    assert "%d elements outside channels [4, 12) of 24" % (2 * 3 * 5 * 4) in str(e.value) and "pixel (0, 0, 0), channel 12" in str(e.value), str(e.value)
    ct.assert_same_bits(y[..., 4:16], x, "the copy itself")


def test_positive_control_a_write_behind_the_declared_payload_fails_the_band_check(hops):
    """a guarded destination whose payload the guard is told is 16 bytes shorter than what the kernel is given: check (a) fails on the back band,
    offsets +0 .. +15; the truthful description of the same call passes"""
    x = ct.R(2, (10, 8))
    for lie in (16, 0):
        def launch():
            with hops.guard_bands(0xFF) as g:
                src = hops.DeviceBuffer.from_numpy(x)
                dst = hops.DeviceBuffer(x.nbytes)
                g.shorten(dst, lie)
                _copy(hops, src, dst.ptr, 10, 8, 8, 8)
                return dst.to_numpy(x.shape)
        if lie:
            with pytest.raises(hops.ContainmentError) as e:
                launch()
            msg = str(e.value)
            assert "back band" in msg and "16 bytes differ" in msg and "offsets +0 .. +15" in msg and "output" in msg and "launch" in msg, msg
        else:
            ct.assert_same_bits(launch(), x, "truthful: passes")              # (iii) negative control


def test_positive_control_front_band_and_written_input(hops):
    """the other two things the guard watches: the bytes in FRONT of a payload (a copy aimed 16 bytes early, still inside the allocation) and an
    input buffer that a kernel wrote"""
    x = ct.R(3, (10, 8))
    with pytest.raises(hops.ContainmentError) as e:
        with hops.guard_bands(0x7B):
            src = hops.DeviceBuffer.from_numpy(x)
            dst = hops.DeviceBuffer(x.nbytes)
            _copy(hops, src, dst.ptr - 16, 10, 8, 8, 8)
    assert "front band" in str(e.value) and "offsets -16 .. -1" in str(e.value), str(e.value)
    with pytest.raises(hops.ContainmentError) as e:
        with hops.guard_bands(0x7B):
            src = hops.DeviceBuffer.from_numpy(x)
            other = hops.DeviceBuffer.from_numpy(np.zeros_like(x))          # uploaded as an INPUT, then used as the destination
            _copy(hops, src, other.ptr, 10, 8, 8, 8)
    assert "input buffer #1" in str(e.value) and "was written" in str(e.value), str(e.value)


# ---- entries that refuse a view say so (SI_E_UNSUPPORTED / SI_E_BADARG), they do not run it some other way ----
def test_views_an_entry_cannot_serve_are_refused(hops):
    x = ct.R(4, (1, 5, 5, 8), -3, -1)
    with pytest.raises(hops.HipError):
        hops.maxpool5_chain3(x, out_ld=19, out_c_off=(3, 3, 3))             # strides that are not multiples of 4 floats (si_hip.h: run three pools)
    with pytest.raises(hops.HipError):
        hops.maxpool5_chain3(x.astype(np.float16), half=True, out_ld=20, out_c_off=(4, 4, 4))   # ... of 8 halves
    with pytest.raises(hops.HipError):
        hops.binary_bcast_f16("mul", ct.R(5, (2, 3, 3, 16), -1, 1, np.float16), ct.R(6, (2, 16), 0, 1, np.float16), out_ld=20, out_c_off=4)
    with pytest.raises(hops.HipError):
        hops.conv2d_f16(ct.R(7, (1, 5, 5, 32), -1, 1, np.float16), ct.R(8, (32, 32, 1, 1)), None, in_ld=36, in_c_off=4)   # channel vectors of 8 halves
    with pytest.raises(hops.HipError):   # the f32_split stem takes dense image rows on 16-byte boundaries: 21 x 3 floats are not
        hops.conv2d_stem_split3(ct.R(11, (1, 19, 21, 3), 0, 1), ct.R(12, (32, 3, 6, 6), -0.3, 0.3), None)
    with pytest.raises(hops.HipError):   # the fused stem pair: image rows of whole 16-byte vectors (iw % 4 == 0)
        hops.conv_stem_s2c32_f16(*ct._stem_ops(1, 38, 50))
    with pytest.raises(hops.HipError):   # Winograd reads 16-byte channel vectors: an input slice that starts 12 bytes into its row
        hops.conv2d_winograd(ct.R(13, (1, 5, 5, 16)), ct.R(14, (32, 16, 3, 3)), None, in_ld=20, in_c_off=3)
    with pytest.raises(AssertionError):
        hops.conv2d(ct.R(9, (1, 2, 2, 8)), ct.R(10, (8, 8, 1, 1)), None, out_ld=12, out_c_off=8)    # a slice that does not fit its row
