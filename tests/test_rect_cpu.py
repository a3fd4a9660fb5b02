"""CPU: the rectangular conv / pool matrix of tests/rect_reference.py.  The table is sound (every case has its twin, every family occurs, every
output is non-empty), and the CPU oracle -- whose rectangular handling nothing had checked either -- agrees with torch float64 on every case:
`naive` (fp64 accumulation), `chain` (the device implicit GEMM's fma order) and `auto` (the reference's dispatch), in shape and within the bars
the GPU tests use.  The margin this leaves the GPU tests is printed per case."""
import numpy as np
import pytest
import torch

import rect_reference as rr
import util
from simpleinfer_amd import modelgen as mg

CHAIN_FAMILIES = ("igemm_fast", "igemm_padk", "igemm_generic")   # orc_conv2d_chain restates these kernels only (oracle/si_oracle.c)


def test_table_is_sound():
    keys = {rr.key(c): c for c in rr.RECT_CASES}
    assert len(keys) == len(rr.RECT_CASES), "duplicate cases"
    assert len(set(rr.ids_of(rr.RECT_CASES))) == len(rr.RECT_CASES)
    for c in rr.RECT_CASES:
        t = keys.get(rr.key(rr.twin(c)))
        assert t is not None, "no twin of %s" % rr.case_id(c)
        assert t.family == c.family
        assert rr.key(rr.twin(t)) == rr.key(c)
        oh, ow = rr.out_hw(c.shape[1], c.shape[2], c.k, c.s, c.p, c.d)
        assert oh > 0 and ow > 0, rr.case_id(c)
        assert c.shape[3] % c.g == 0 and c.oc % c.g == 0
        # rectangular in at least one of the four pairs (the 64-tap square is the one deliberate exception: the mask's last bit)
        assert c.k[0] != c.k[1] or c.s[0] != c.s[1] or c.p[0] != c.p[1] or c.d[0] != c.d[1] or c.k == (8, 8) or (c.k == (1, 1) and c.shape[1] != c.shape[2])
        assert c.shape[0] * c.shape[1] * c.shape[2] <= 2 * 24 * 30, "keep the images small: %s" % rr.case_id(c)
    assert {c.family for c in rr.RECT_CASES} == set(rr.FAMILIES)
    seeds = [rr.seed_of(c) for c in rr.RECT_CASES]
    assert len(set(seeds)) == len(seeds), "two cases share a seed"
    assert all(abs(a - b) >= 3 for i, a in enumerate(seeds) for b in seeds[:i]), "operand seeds (s, s + 1, s + 2) overlap"
    # what the issue names: 64 taps, 65 taps, both dilation rows, both stems that must not take the rolling-window kernel
    ks = {(c.k, c.s, c.d) for c in rr.RECT_CASES}
    for want in (((8, 8), (1, 1), (1, 1)), ((5, 13), (1, 1), (1, 1)), ((13, 5), (1, 1), (1, 1)), ((3, 3), (1, 1), (2, 1)), ((3, 3), (1, 1), (1, 2)),
                 ((9, 1), (1, 1), (2, 1)), ((6, 6), (2, 1), (1, 1)), ((6, 7), (2, 2), (1, 1)), ((7, 6), (2, 2), (1, 1)),
                 # the 9-element stem row on both sides of its tallest kernel: sh + kh = 7 (5x3 stride 2, 6x3 stride 1) and beyond
                 ((5, 3), (2, 1), (1, 1)), ((6, 3), (1, 2), (1, 1)), ((6, 3), (2, 1), (1, 1)), ((7, 3), (1, 1), (1, 1)), ((7, 3), (2, 2), (1, 1))):
        assert want in ks, want
    for shape, oc, k, s, p in rr.SPLIT3_CASES:
        assert k[0] * k[1] <= 32 and shape[3] in (64, 96)
    assert any(k[0] * k[1] == 32 for _, _, k, _, _ in rr.SPLIT3_CASES)
    assert len({rr.split3_id(c) for c in rr.SPLIT3_CASES}) == len(rr.SPLIT3_CASES)
    for k, s, p, d in rr.POOL_PARAMS:
        assert (rr.swap(k), rr.swap(s), rr.swap(p), rr.swap(d)) in rr.POOL_PARAMS, "pool parameter set without its twin"


@pytest.mark.parametrize("c", rr.RECT_CASES, ids=rr.ids_of(rr.RECT_CASES))
def test_oracle_conv_paths_agree_with_torch_float64(orc, c):
    x, w, b = rr.operands(c)
    ref = rr.conv2d_f64(x, w, b, c.s, c.p, c.d, c.g)
    n, ih, iw, _ = c.shape
    assert ref.shape == (n,) + rr.out_hw(ih, iw, c.k, c.s, c.p, c.d) + (c.oc,)
    line = [rr.case_id(c)]
    for path, bar in (("naive", 1e-6), ("chain", 2e-5), ("auto", 2e-5)):
        if path == "chain" and c.family not in CHAIN_FAMILIES:
            continue
        got = orc.conv2d(x, w, b, c.s, c.p, c.d, c.g, path=path)
        assert got.shape == ref.shape, (path, got.shape, ref.shape)
        e, m = util.rel_err(got, ref), util.mixed_err(got, ref)
        line.append("%s %.2e / %.2e" % (path, e, m))
        # naive accumulates in fp64 and rounds once (2^-24 = 6e-8 of an element): 1e-6 of the tensor's scale; chain and auto are fp32
        # accumulations, held to the bar the GPU kernels are held to, on both metrics
        assert e <= bar and m <= (bar if path == "naive" else util.REL_TOL), (path, e, m)
    print("  ".join(line))


@pytest.mark.parametrize("c", rr.cases_of("grouped"), ids=rr.ids_of(rr.cases_of("grouped")))
def test_merged_groups_as_a_dense_block_diagonal_conv(orc, c):
    """the problem the merged-group path runs (rr.merged_groups_dense) is the grouped convolution, and the oracle's fma chain on it is within the
    GPU bar of torch: the GPU test may hold the merged kernel to that chain bit for bit"""
    x, w, b = rr.operands(c)
    ref = rr.conv2d_f64(x, w, b, c.s, c.p, c.d, c.g)
    dense, g2 = rr.merged_groups_dense(w, c.g)
    assert dense.shape[1] == 32 and g2 * 32 == c.shape[3]
    assert np.array_equal(rr.conv2d_f64(x, dense, b, c.s, c.p, c.d, g2), ref), "zeros add nothing, in float64 either"
    pred = orc.conv2d(x, dense, b, c.s, c.p, c.d, g2, path="chain")
    assert util.rel_err(pred, ref) <= 2e-5 and util.mixed_err(pred, ref) <= util.REL_TOL


@pytest.mark.parametrize("c", rr.SPLIT3_CASES, ids=[rr.split3_id(c) for c in rr.SPLIT3_CASES])
def test_oracle_agrees_with_torch_on_the_split3_cases(orc, c):
    shape, oc, k, s, p = c
    case = rr.Case("split3", shape, oc, k, s, p, (1, 1), 1, "", "")
    x, w, b = rr.operands(case, w_scale=0.2)
    ref = rr.conv2d_f64(x, w, b, s, p)
    got = orc.conv2d(x, w, b, s, p, path="naive")
    assert got.shape == ref.shape and util.rel_err(got, ref) <= 1e-6


@pytest.mark.parametrize("q", rr.POOL_PARAMS, ids=[rr.pool_id(q) for q in rr.POOL_PARAMS])
@pytest.mark.parametrize("ch", [8, 6])
def test_oracle_maxpool_is_bit_exact_against_torch(orc, q, ch):
    k, s, p, d = q
    x = rr.pool_input(ch)
    ref = rr.maxpool2d_f64(x, k, s, p, d)
    assert np.isfinite(ref).all() and (ref < 0).all(), "every window holds at least one real element"
    got = orc.maxpool2d(x, k, s, p, d)
    assert got.shape == ref.shape == (x.shape[0],) + rr.out_hw(x.shape[1], x.shape[2], k, s, p, d) + (ch,)
    util.assert_exact(got.astype(np.float64), ref, rr.pool_id(q))


def test_maxpool_reference_is_torchs_own_padding():
    """where torch accepts the pad itself (pad <= k / 2) the explicit -inf border of maxpool2d_f64 changes nothing"""
    x = rr.pool_input(8)
    t = torch.from_numpy(np.ascontiguousarray(x.astype(np.float64).transpose(0, 3, 1, 2)))
    for k, s, p, d in rr.POOL_PARAMS:
        if 2 * p[0] <= k[0] and 2 * p[1] <= k[1]:
            own = torch.nn.functional.max_pool2d(t, k, stride=s, padding=p, dilation=d).numpy().transpose(0, 2, 3, 1)
            util.assert_exact(rr.maxpool2d_f64(x, k, s, p, d), own, rr.pool_id((k, s, p, d)))


def test_modelgen_maxpool_takes_pairs_and_ints_unchanged():
    b = mg.PnnxBuilder()
    x = b.input((1, 8, 11, 14))
    y = b.maxpool(x, 3, 2, 1)
    assert b.shapes[y] == (1, 8, 6, 7)
    assert "kernel_size=(3,3) padding=(1,1) return_indices=False stride=(2,2)" in b.lines[-1]
    z = b.maxpool(x, (3, 2), (2, 1), (1, 0))
    assert b.shapes[z] == (1, 8, 6, 13)
    assert "kernel_size=(3,2) padding=(1,0) return_indices=False stride=(2,1)" in b.lines[-1]


def test_rect_graph_float32_evaluation_is_within_the_bar(orc, tmp_path):
    """the condition of the engine-level GPU test: on the chosen graph and input the oracle's own fp32 run is within the fp32 graph bar of the
    float64 composition (both metrics), so an fp32 engine can be held to that bar; and every layer of the graph is rectangular"""
    b = rr.build_rect_graph(mg)
    x = mg.synth_input((2, 48, 60, 3))
    ref = rr.eval_rect_graph(b, x)
    assert ref.shape == (2, 3, 13, 10)
    pp, bp = str(tmp_path / "r.pnnx.param"), str(tmp_path / "r.pnnx.bin")
    b.save(pp, bp)
    out = orc.run_graph(pp, bp, {"0": x})
    (got,) = out.values()
    e, m = util.rel_err(got, ref), util.mixed_err(got, ref)
    print("oracle fp32 vs float64 on the rectangular graph: max-based %.3e, element-wise %.3e" % (e, m))
    assert e <= util.REL_TOL / 5 and m <= util.REL_TOL / 5
    convs = [rr._parse(ln)[4] for ln in b.lines if ln.startswith("nn.Conv2d")]
    assert len(convs) == 8
    for prm in convs[:-1]:
        k, s, p = rr._ints(prm["kernel_size"]), rr._ints(prm["stride"]), rr._ints(prm["padding"])
        assert k[0] != k[1] or s[0] != s[1] or p[0] != p[1], prm
