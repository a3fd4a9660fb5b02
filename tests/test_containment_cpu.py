"""The containment checkers of tests/containment.py held to hand-corrupted arrays, and the completeness rule: every compute entry of
include/si_hip.h is driven by at least one case of the matrix (no GPU needed)."""
import numpy as np
import pytest

import containment as ct


def _filled(shape, dtype, byte):
    dt = np.dtype(dtype)
    return np.full(int(np.prod(shape)) * dt.itemsize, byte, np.uint8).view(dt).reshape(shape)


def _buffer(dtype, byte, shape=(2, 3, 4, 12), c_off=4, c=5):
    full = _filled(shape, dtype, byte)
    full[..., c_off:c_off + c] = np.arange(np.prod(shape[:-1]) * c).reshape(shape[:-1] + (c,)).astype(dtype)
    return full, c_off, c


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.uint8])
@pytest.mark.parametrize("byte", ct.PATTERNS + (0x00,))
def test_outside_check_passes_clean_buffers(dtype, byte):
    full, off, c = _buffer(dtype, byte)
    ct.assert_outside_fill(full, off, c, byte, "clean")
    ct.assert_outside_fill(_filled((3, 7), dtype, byte), 0, 7, byte, "dense: nothing outside")
    ct.assert_outside_fill(_filled((3, 7), dtype, byte), 7, 0, byte, "empty slice: everything outside")


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.uint8])
@pytest.mark.parametrize("byte", ct.PATTERNS)
@pytest.mark.parametrize("where,pixel,channel", [("left edge", (0, 0, 0), 3), ("right edge", (1, 2, 1), 9), ("last pixel", (1, 2, 3), 11), ("first element", (0, 0, 0), 0)])
def test_outside_check_reports_one_corrupted_byte(dtype, byte, where, pixel, channel):
    """ONE byte off just left of the slice, just right of it, in the last element of the last pixel: reported with its pixel and channel"""
    full, off, c = _buffer(dtype, byte)
    raw = full.view(np.uint8).reshape(full.shape + (full.dtype.itemsize,))
    raw[pixel + (channel, full.dtype.itemsize - 1)] ^= 0x01
    with pytest.raises(AssertionError) as e:
        ct.assert_outside_fill(full, off, c, byte, where)
    msg = str(e.value)
    assert "1 elements outside" in msg and "pixel (%d, %d, %d), channel %d" % (pixel + (channel,)) in msg, msg
    raw[pixel + (channel, full.dtype.itemsize - 1)] ^= 0x01
    ct.assert_outside_fill(full, off, c, byte, "restored")


def test_outside_check_sees_a_written_value_equal_to_nan_only_in_value():
    """a NaN-filled gap: another NaN (other payload bits) is a write; the count covers every element"""
    full, off, c = _buffer(np.float32, 0xFF)
    full[1, :, :, off + c:] = np.float32("nan")     # the canonical quiet NaN 0x7FC00000, not 0xFFFFFFFF
    with pytest.raises(AssertionError) as e:
        ct.assert_outside_fill(full, off, c, 0xFF, "nan")
    assert "%d elements outside" % (3 * 4 * 3) in str(e.value) and "pixel (1, 0, 0), channel 9" in str(e.value), str(e.value)
    zero = _filled((2, 5), np.float16, 0xFF)
    zero[1, 0] = 0
    with pytest.raises(AssertionError, match=r"pixel \(1\), channel 0"):
        ct.assert_outside_fill(zero, 1, 3, 0xFF, "fp16")


def test_inside_the_slice_is_never_looked_at():
    full, off, c = _buffer(np.float16, 0x7B)
    full[..., off:off + c] = np.float16("nan")
    ct.assert_outside_fill(full, off, c, 0x7B, "slice holds anything")


def test_same_bits():
    a = _filled((2, 3, 4), np.float32, 0xFF)
    ct.assert_same_bits(a, a.copy(), "NaN fills compare equal")
    assert not np.array_equal(a, a.copy())           # (what a float comparison would have said)
    b = a.copy()
    b[1, 2, 3] = np.float32("nan")
    with pytest.raises(AssertionError, match=r"1 of 24 elements differ in their bits; first at pixel \(1, 2\), channel 3"):
        ct.assert_same_bits(a, b, "payload")
    z = np.zeros((4, 2), np.float16)
    nz = z.copy()
    nz[3, 1] = -0.0
    with pytest.raises(AssertionError, match=r"pixel \(3\), channel 1"):
        ct.assert_same_bits(z, nz, "-0.0 is not +0.0")
    u = np.arange(12, dtype=np.uint8).reshape(3, 4)
    v = u.copy()
    v[0, 0] = 7
    v[2, 3] = 0
    with pytest.raises(AssertionError, match=r"2 of 12 elements"):
        ct.assert_same_bits(u, v, "u8")
    with pytest.raises(AssertionError):
        ct.assert_same_bits(u, u.astype(np.int8), "dtype")
    with pytest.raises(AssertionError):
        ct.assert_same_bits(u, u.reshape(4, 3), "shape")
    ct.assert_same_bits(np.zeros((0, 6), np.float32), np.zeros((0, 6), np.float32), "empty")


def test_finite():
    ct.assert_finite(np.arange(6, dtype=np.uint8).reshape(2, 3))
    ct.assert_finite(np.ones((2, 3), np.float16))
    x = np.ones((2, 3, 4), np.float32)
    x[1, 0, 2] = np.inf
    with pytest.raises(AssertionError, match=r"pixel \(1, 0\), channel 2"):
        ct.assert_finite(x, "inf")
    with pytest.raises(AssertionError):
        ct.assert_finite(_filled((2, 2), np.float16, 0xFF), "the NaN pattern")
    ct.assert_finite(_filled((2, 2), np.float16, 0x7B), "the large finite pattern")
    assert float(_filled((1,), np.float16, 0x7B)[0]) == 61280.0 and 1.2e36 < float(_filled((1,), np.float32, 0x7B)[0]) < 1.4e36


def test_out_slices_the_destination():
    full, off, c = _buffer(np.float32, 0x7B)
    o = ct.Out("y", full, off, c)
    assert o.dest.shape == (2, 3, 4, 5) and np.array_equal(o.dest, full[..., 4:9])
    assert ct.Out("dense", np.zeros((3, 7))).c == 7


# ---- completeness ----
def test_every_compute_entry_of_the_header_is_driven():
    """Exemptions are by RULE (the runtime group, the host-side queries): a function added to include/si_hip.h that launches work fails here
    until the matrix has a case that names it."""
    fns = ct.header_functions()
    assert len(fns) == len(set(fns)) and all(f.startswith("si_hip_") for f in fns)
    entries = ct.compute_entries()
    driven = set(ct.entries_driven())
    missing = [e for e in entries if e not in driven]
    assert not missing, "compute entries no containment case drives: %s" % missing
    unknown = sorted(driven - set(fns))
    assert not unknown, "cases name functions the header does not declare: %s" % unknown
    exempt_but_named = sorted(e for e in driven if ct.is_exempt(e))
    assert not exempt_but_named, exempt_but_named
    # the header at the time of writing: 135 functions, 57 of them compute entries (a later header has more, never fewer)
    assert len(fns) >= 135 and len(entries) >= 57, (len(fns), len(entries))


def test_exemption_rule():
    for name in ("si_hip_malloc", "si_hip_device_sync", "si_hip_device_by_pci_bus_id", "si_hip_memcpy_d2d", "si_hip_graph_launch", "si_hip_version",
                 "si_hip_error_string", "si_hip_enable_peer_access", "si_hip_ipc_open_mem_handle", "si_hip_host_register", "si_hip_set_device",
                 "si_hip_conv2d_f16_supported", "si_hip_conv2d_wino23_eligible", "si_hip_conv2d_wino43_preferred", "si_hip_conv2d_split3_weight_elems",
                 "si_hip_conv2d_stem_f16_pack_weight_host", "si_hip_conv2d_kernel_name_form", "si_hip_conv2d_f16_tile_variant",
                 "si_hip_yolo_postprocess_workspace_bytes", "si_hip_f32_to_f16_host"):
        assert ct.is_exempt(name), name
    for name in ("si_hip_conv2d_f32", "si_hip_conv2d_yolo_f16_tile", "si_hip_gather_f32", "si_hip_hostile_f32",
                 "si_hip_devicewide_reduce_f32", "si_hip_copy_channels_f32", "si_hip_convert_f16_f32", "si_hip_yolo_postprocess_f32"):
        assert not ct.is_exempt(name), name


def test_header_parser_ignores_comments(tmp_path):
    p = tmp_path / "h.h"
    p.write_text("/* as si_hip_old_f32 (x) */\nint si_hip_new_f32(const float* in);\n// si_hip_gone_f32(\nsize_t si_hip_new_weight_elems(int n);\n"
                 "int si_hip_new_f32 (const float* in, int more);\n")
    assert ct.header_functions(str(p)) == ["si_hip_new_f32", "si_hip_new_weight_elems"]
    assert ct.compute_entries(str(p)) == ["si_hip_new_f32"]


def test_case_ids_are_unique_and_cases_name_entries():
    ids = [c.id for c in ct.CASES]
    assert len(ids) == len(set(ids))
    assert all(c.entries for c in ct.CASES)
