"""GPU: Tensor.permute / reshape / view / torch.transpose / squeeze / unsqueeze -- si_hip_permute_f32 / _f16 (include/si_permute.h) form by
form against numpy, the layout layer and the planner's FuseLayoutChains / AliasViews passes on the toy heads against the torch runner of
tests/layout_reference.py, and torch.cat on rank 2 and rank 3.  Nothing here does arithmetic on a moved value: every comparison is bit for bit
on the integer view."""
import numpy as np
import pytest

import layout_reference as lr
from ct_reference import _parse
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError
from test_layout_cpu import header_int

pytestmark = pytest.mark.gpu

TILE = header_int("SI_PERMUTE_TILE")
DTYPES = {"f32": (np.float32, np.uint32, 4), "f16": (np.float16, np.uint16, 8)}
SENTINEL = 0x7B            # the byte of the gaps: 0x7B7B7B7B / 0x7B7B never occurs in the data below


def ints(dtype):
    return DTYPES["f32" if np.dtype(dtype) == np.float32 else "f16"][1]


def numbered(count, dtype):
    """`count` elements with recognisable bit patterns (a scrambled counter, never the sentinel's word), as dtype"""
    it = ints(dtype)
    size = np.dtype(it).itemsize
    v = (np.arange(count, dtype=np.uint64) * 2654435761 % (2 ** (8 * size) - 1)).astype(it)
    v[v == int.from_bytes(bytes([SENTINEL]) * size, "little")] = 1
    return v.view(dtype)


def same_bits(got, want, what):
    it = ints(got.dtype)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = got.view(it) != want.view(it)
    assert not bad.any(), "%s: %d of %d words differ, first at %r" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def run_forms(src, desc, forms, what, **kw):
    """every eligible form of `forms` under guard bands against the numpy statement, gaps included; returns the kernel names"""
    want = hipops.permute_ref(src, desc, out_fill=hipops.ByteFill(SENTINEL))
    names = []
    for form in forms:
        desc.form = hipops.PERMUTE_FORMS[form]
        if hipops.permute_kernel_name(desc, half=src.dtype == np.float16) == "none":
            continue
        with hipops.guard_bands(0xFF):
            got = hipops.permute(src, desc, out_fill=hipops.ByteFill(SENTINEL), **kw)
        names.append(hipops.LAST_KERNEL_NAME["si_hip_permute"])
        same_bits(got, want, "%s form %s (%s)" % (what, form, names[-1]))
    return names


def gapped(dims_in, gaps, dtype):
    """a source of logical extents dims_in (row-major, the last one contiguous) with `gaps[k]` sentinel elements behind every run of dimension
    k; returns (flat source, the element stride of every dimension)"""
    strides, span = [0] * len(dims_in), 1
    for k in range(len(dims_in) - 1, -1, -1):
        strides[k] = span
        span = span * dims_in[k] + gaps[k]
    src = hipops._full((span,), dtype, hipops.ByteFill(SENTINEL))
    idx = np.zeros(dims_in, np.int64)
    for k, (n, s) in enumerate(zip(dims_in, strides)):
        idx += (np.arange(n, dtype=np.int64) * s).reshape([n if j == k else 1 for j in range(len(dims_in))])
    src[idx.reshape(-1)] = numbered(idx.size, dtype)
    return src, strides


# ---- op level -------------------------------------------------------------------------------------------------------------
EXTENTS = (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_tile_extents(gpu, dt, batch):
    """a transpose [B, C, R] -> [B, R, C] with each tile dimension at 1, 2, tile - 1, tile, tile + 1, 2 tile + 1: the forced tile form, the
    element form and the automatic choice give numpy's bits; the input rows have gaps whose sentinel never shows up, the output pitch
    leaves gaps whose sentinel survives"""
    dtype = DTYPES[dt][0]
    seen = set()
    for r in EXTENTS:
        for c in EXTENTS:
            src, (sb, sc, _) = gapped((batch, c, r), (5, 3, 0), dtype)
            desc = hipops.permute_desc((batch, r, c), (sb, 1, sc), out_ld=c + 3)
            seen.update(run_forms(src, desc, ("tile", "elem", "auto"), "B%d R%d C%d" % (batch, r, c)))
    t = "float" if dt == "f32" else "_Float16"
    assert {"permute_tile<%s>" % t, "permute_elem<%s>" % t} <= seen, seen


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_tile_with_two_batch_dimensions(gpu, dt):
    """the transposed pair in the middle of the nest and at its end, two batch dimensions around it"""
    dtype = DTYPES[dt][0]
    src, (s0, s1, s2, _) = gapped((3, 2, 70, 9), (1, 2, 3, 0), dtype)          # [A, B, C, R]
    for dims, st in (((3, 2, 9, 70), (s0, s1, 1, s2)), ((3, 9, 2, 70), (s0, 1, s1, s2)), ((9, 3, 2, 70), (1, s0, s1, s2)),
                     ((2, 9, 3, 70), (s1, 1, s0, s2))):
        names = run_forms(src, hipops.permute_desc(dims, st, out_ld=72), ("tile", "elem"), "%r" % (dims,))
        assert len(names) == 2 and names[0].startswith("permute_tile<"), names


RUNS = (1, 3, 6, 7, 8, 85, 16, 64)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_rows_run_lengths(gpu, dt):
    """runs of 1, 3, 6, 7, 8, 85 (and 16, 64: the vector form) gathered in permuted order out of a gapped source; the rows form, the element
    form and the automatic choice agree; a base pointer 4 / 2 bytes off 16-byte alignment and an output pitch with gaps take V = 1"""
    dtype, _, vec = DTYPES[dt]
    t = "float" if dt == "f32" else "_Float16"
    for k in RUNS:
        src, (s0, s1, s2, _) = gapped((3, 5, 4, k), (vec, 2 * vec, vec if k % vec == 0 else 1, 0), dtype)
        for out_ld in (k, k + vec, k + 1):
            desc = hipops.permute_desc((4, 3, 5, k), (s2, s0, s1, 1), out_ld=out_ld)
            names = run_forms(src, desc, ("rows", "elem", "auto"), "run %d out_ld %d" % (k, out_ld))
            want_vec = k % vec == 0 and out_ld % vec == 0
            assert names[0] == names[2] == "permute_rows<%s, %d>" % (t, vec if want_vec else 1), (k, out_ld, names)
            assert names[1] == "permute_elem<%s>" % t
        # the same copy from a source / into a destination one element off the 16-byte grid
        desc = hipops.permute_desc((4, 3, 5, k), (s2, s0, s1, 1))
        want = hipops.permute_ref(src, desc)
        for kw in (dict(src_off=1), dict(out_off=1)):
            shifted = np.concatenate([src[:1], src]) if "src_off" in kw else src
            with hipops.guard_bands(0x7B):
                got = hipops.permute(shifted, desc, form="auto", out_fill=hipops.ByteFill(SENTINEL), **kw)
            assert hipops.LAST_KERNEL_NAME["si_hip_permute"] == "permute_rows<%s, 1>" % t
            same_bits(got, want, "run %d %r" % (k, kw))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_special_values_pass_as_bits(gpu, dt):
    """NaN payloads (quiet and signalling), +-0, denormals, +-inf and random words through every form"""
    dtype, it, vec = DTYPES[dt]
    bits = 8 * np.dtype(it).itemsize
    r = np.random.Generator(np.random.Philox(3))
    words = r.integers(0, 2 ** bits, 40 * 72, dtype=np.uint64).astype(it)
    exp = (2 ** (bits - 1)) - (2 ** (23 if bits == 32 else 10))                # all exponent bits
    special = [0, 2 ** (bits - 1), 1, 2 ** (bits - 1) + 1, exp, exp + 2 ** (bits - 1), exp + 1, exp + 2 ** (bits - 1) + 5,
               exp + 2 ** (21 if bits == 32 else 8), exp + 2 ** (22 if bits == 32 else 9) + 3]
    words[:len(special)] = np.array(special, np.uint64).astype(it)
    r.shuffle(words)
    src = words.view(dtype)
    assert np.isnan(src).sum() >= 4 and np.isinf(src).sum() >= 2
    names = run_forms(src, hipops.permute_desc((40, 72), (72, 1)), ("rows", "elem"), "copy")
    names += run_forms(src, hipops.permute_desc((72, 40), (1, 72)), ("tile", "elem"), "transpose")
    names += run_forms(src, hipops.permute_desc((40, 9), (72, 1)), ("rows",), "short runs")
    assert len(set(names)) == 4, names


@pytest.mark.parametrize("form", ["rows_vec", "rows", "elem", "tile"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_grid_stride_passes(gpu, dt, form):
    """every form goes round its capped grid at least three times, the last pass ragged (sizes from the header's caps), and two launches give
    the same bits"""
    dtype, _, vec = DTYPES[dt]
    if form == "tile":
        tiles = 2 * header_int("SI_PERMUTE_TILE_MAX_BLOCKS") + 100
        src = numbered(tiles * 6, dtype)
        desc = hipops.permute_desc((tiles, 2, 3), (6, 1, 2), form="tile")      # one 2 x 3 tile per batch entry
    else:
        items = 2 * header_int("SI_PERMUTE_MAX_BLOCKS") * 256 + 1000
        run = vec * 2 if form == "rows_vec" else 5
        rows = -(-items * (vec if form == "rows_vec" else 1) // run)
        src = numbered(rows * run, dtype)
        desc = hipops.permute_desc((rows // 2, 2, run), (run, (rows // 2) * run, 1), form=form.split("_")[0])
    want = hipops.permute_ref(src, desc)
    got = []
    for _ in range(2):
        with hipops.guard_bands(0xFF):
            got.append(hipops.permute(src, desc))
    name = hipops.LAST_KERNEL_NAME["si_hip_permute"]
    assert name.startswith("permute_%s<" % form.split("_")[0]) and (form != "rows_vec" or name.endswith(", %d>" % vec)), name
    same_bits(got[0], want, "%s %s" % (form, dt))
    same_bits(got[1], got[0], "second launch")


def test_abi_refusals_on_the_device(gpu, native_libs):
    """the refusals of tests/test_layout_cpu.py hold with a device present, and a refused call leaves the device usable"""
    import ctypes as C
    H, _ = native_libs
    for fn in (H.si_hip_permute_f32, H.si_hip_permute_f16):
        assert fn(None, C.c_void_p(256), C.c_void_p(256), None) == -1
        assert fn(C.byref(hipops.permute_desc((3, 16), (7, 3), out_ld=2)), C.c_void_p(256), C.c_void_p(256), None) == -1
        assert fn(C.byref(hipops.permute_desc((2, 4), (2 ** 31, 1))), C.c_void_p(256), C.c_void_p(256), None) == -2
    src = numbered(48, np.float32)
    with hipops.guard_bands(0xFF):
        got = hipops.permute(src, hipops.permute_desc((16, 3), (1, 16)))
    same_bits(got, hipops.permute_ref(src, hipops.permute_desc((16, 3), (1, 16))), "after refusals")


# ---- engine level ---------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def graph_outputs(b):
    return [_parse(ln)[2][0] for ln in b.lines if ln.startswith("pnnx.Output")]


def run_engine(b, tmp_path, x, tag="m", forwards=1, **opts):
    """(engine, {graph output: FILE-order array})"""
    pp, bp = save(b, tmp_path, tag)
    e = Engine(**opts)
    e.load_model(pp, bp)
    e.input(e.input_names()[0], x)
    for _ in range(forwards):
        e.forward()
    return e, {name: np.ascontiguousarray(lr.unstored(e.extract(name))) for name in graph_outputs(b)}


def reference(b, tmp_path, x, half=False, **opts):
    """the graph's outputs with the data movement done by torch on the engine's own arithmetic: a probe engine hands out every arithmetic
    result that movement reads or that is computed from moved data.  fp16 storage: what movement reads is cast to half once -- the probe's
    graph outputs are fp32, the engine under test stores the same accumulators as halves; results computed from moved data are taken as they are.
    Those later taps carry the engine's own movement, so the movement itself is judged first: a second engine whose graph outputs are the
    movement results that arithmetic reads (the fused chains run in it as in the model) against torch's movement of the taps in FRONT of
    the first movement operator, which owe nothing to the code under test."""
    taps = lr.tap_operands(b)
    _, got = run_engine(lr.probe_builder(b, taps), tmp_path, x, tag="probe", **opts)
    moved = lr.read_by_movement(b)
    q = (lambda v: v.astype(np.float16).astype(np.float32)) if half else (lambda v: v)
    got = {k: q(v) if k in moved else v for k, v in got.items()}
    points = lr.moved_checkpoints(b)
    if points:
        entering = {k: got[k] for k in lr.tap_operands(b, entering_only=True)}
        want = lr.eval_graph(b, x, taps=entering, want=points)
        _, have = run_engine(lr.probe_builder(b, points), tmp_path, x, tag="moved", **opts)
        for r in points:
            same_bits(have[r], want[r], "moved operand %s against torch" % r)
    return lr.eval_graph(b, x, taps=got)


TOYS = {
    "ssd_head": lambda n=2: mg.build_toy_ssd_head(batch=n),
    "anchorfree_head": lambda n=2: mg.build_toy_anchorfree_head(batch=n),
    "yolov5_raw_head": lambda n=2: mg.build_toy_yolov5_raw_head(batch=n),
    "view_classifier": lambda n=2: mg.build_toy_view_classifier(batch=n),
    "view_classifier_pool2": lambda n=2: mg.build_toy_view_classifier(batch=n, pool=2),
    "channel_shuffle": lambda n=2: mg.build_toy_channel_shuffle(batch=n),
}


def toy_input(b):
    n, c, h, w = b.shapes["0"]
    return mg.synth_input((n, h, w, c))


def layout_layers(prof):
    return [L for L in prof if L["type"] in lr.LAYOUT_TYPES]


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("which", sorted(TOYS))
def test_toy_eager_and_captured(gpu, tmp_path, which, fp16):
    """every toy against the torch runner, eager and replayed from a captured graph, in fp32 and with fp16 storage (2-byte words: the movement
    of the engine's own half arithmetic, bit for bit, and a result that stays near fp32)"""
    b = TOYS[which]()
    x = toy_input(b)
    want = reference(b, tmp_path, x, half=bool(fp16), fp16=fp16)
    e, got = run_engine(b, tmp_path, x, fp16=fp16)
    (out,) = graph_outputs(b)
    same_bits(got[out], want, "%s fp16=%d" % (which, fp16))
    assert all(L["flops"] == 0.0 for L in layout_layers(e.profile()))
    _, cap = run_engine(b, tmp_path, x, forwards=3, graph=1, fp16=fp16)
    same_bits(cap[out], want, "%s fp16=%d graph=1" % (which, fp16))
    if fp16:
        _, f32 = run_engine(b, tmp_path, x)
        err = np.abs(got[out] - f32[out]).max() / max(np.abs(f32[out]).max(), 1e-30)
        print("%s fp16 vs fp32: max|d| / max|ref| = %.3e" % (which, err))
        assert err < 2e-2      # (the suite's bar for fp16 storage against fp32: a few roundings to 2^-11 through three or four layers)


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("which", sorted(TOYS))
def test_toy_rebatched(gpu, tmp_path, which, fp16):
    """SetOption("batch", 3) on the file traced at batch 2 gives the bits of the file built at batch 3 -- a leading shape= entry follows --, at
    the graph output and at every movement result that arithmetic reads; the file built at 3 is held to the torch runner"""
    b2, b3 = TOYS[which](2), TOYS[which](3)
    x = toy_input(b3)
    _, want = run_engine(b3, tmp_path, x, tag="b3", fp16=fp16)
    _, got = run_engine(b2, tmp_path, x, tag="b2", batch=3, fp16=fp16)
    (out,) = graph_outputs(b3)
    same_bits(got[out], want[out], which + " batch=3")
    same_bits(want[out], reference(b3, tmp_path, x, half=bool(fp16), fp16=fp16), which + " built at 3")
    points = lr.moved_checkpoints(b2)
    if points:
        _, moved3 = run_engine(lr.probe_builder(b3, points), tmp_path, x, tag="m3", fp16=fp16)      # (held to torch inside reference())
        _, moved2 = run_engine(lr.probe_builder(b2, points), tmp_path, x, tag="m2", batch=3, fp16=fp16)
        for r in points:
            same_bits(moved2[r], moved3[r], "%s moved operand %s batch=3" % (which, r))


@pytest.mark.parametrize("which", sorted(TOYS))
def test_plans_agree(gpu, tmp_path, which):
    """the default plan against fuse_layout=0, alias_view=0 and fuse=0: identical bits; the two plans that leave the raw YOLOv5 head's and the
    channel shuffle's rank-5 intermediates in memory are refused at load instead"""
    b = TOYS[which]()
    x = toy_input(b)
    (out,) = graph_outputs(b)
    _, base = run_engine(b, tmp_path, x)
    rank5 = which in ("yolov5_raw_head", "channel_shuffle")
    for opts in (dict(fuse_layout=0), dict(alias_view=0), dict(fuse=0), dict(fuse_layout=0, alias_view=0, arena=0)):
        if rank5 and ("fuse_layout" in opts or "fuse" in opts):
            with pytest.raises(StatusError) as err:
                run_engine(b, tmp_path, x, **opts)
            assert err.value.status == Status.kUnsupport, opts
            continue
        _, got = run_engine(b, tmp_path, x, **opts)
        same_bits(got[out], base[out], "%s %r" % (which, opts))


def test_profiles_show_views_and_forms(gpu, tmp_path):
    def prof(b, **opts):
        e, _ = run_engine(b, tmp_path, toy_input(b), **opts)
        return e, layout_layers(e.profile())

    # the SSD idiom and the 1x1 classifier: every layout step is a view, nothing is launched for it
    for b in (mg.build_toy_ssd_head(), mg.build_toy_view_classifier()):
        for opts in ({}, dict(fp16=1)):
            e, layers = prof(b, **opts)
            views = [ln for ln in b.lines if ln.startswith("Tensor.view")]
            assert len(layers) == len(views) and all(L["type"] == "Tensor.view" and L["kernel"] == "view" for L in layers), layers
            assert len(e.schedule()["alias"]) >= len(views)
            assert sum(ln.startswith("Tensor.permute") for ln in b.lines) == sum(n.startswith("Tensor_permute") for n in e.schedule()["fused"])
        e, layers = prof(b, alias_view=0)          # ... and one permute_rows copy each without the aliases
        assert all(L["kernel"] == "permute_rows<float, 4>" for L in layers), layers
    # view(N, no, -1) with no = 32 on 16 x 16 and 8 x 8 maps: one permute_tile each, and one for the closing permute(0, 2, 1)
    _, layers = prof(mg.build_toy_anchorfree_head())
    assert [(L["type"], L["kernel"]) for L in layers] == [("Tensor.view", "permute_tile<float>")] * 2 + [("Tensor.permute", "permute_tile<float>")]
    _, layers = prof(mg.build_toy_anchorfree_head(), fp16=1)
    assert [L["kernel"] for L in layers[:2]] == ["permute_tile<_Float16>"] * 2
    # the raw YOLOv5 head: each view -> permute -> view chain is ONE launch of runs of `no`
    e, layers = prof(mg.build_toy_yolov5_raw_head())
    assert [(L["type"], L["kernel"]) for L in layers] == [("Tensor.view", "permute_rows<float, 1>")] * 2, layers
    assert len(e.schedule()["fused"]) >= 4
    # the 2 x 2 classifier: a transpose of [4, C] per image, below the tile form's switch
    _, layers = prof(mg.build_toy_view_classifier(pool=2))
    assert [L["kernel"] for L in layers] == ["permute_elem<float>"], layers


@pytest.mark.parametrize("pool,fp16", [(2, 0), (1, 0), (1, 1)])
def test_view_equals_flatten(gpu, tmp_path, pool, fp16):
    """build_toy_view_classifier has the bits of the same model written with torch.flatten: pool=2 moves bytes (fp32: torch.flatten has no
    fp16 kernel for H W > 1), pool=1 is a view on one side and a copy on the other"""
    b, f = mg.build_toy_view_classifier(pool=pool), mg.build_toy_view_classifier(pool=pool, flatten=True)
    x = toy_input(b)
    _, got = run_engine(b, tmp_path, x, tag="v", fp16=fp16)
    _, want = run_engine(f, tmp_path, x, tag="f", fp16=fp16)
    same_bits(got[graph_outputs(b)[0]], want[graph_outputs(f)[0]], "view vs flatten")


def view_of_view():
    """conv -> permute(0,2,3,1) -> view(N,-1,4) read twice: by a sigmoid and by a second view(N,-1,8) with its own sigmoid"""
    b = mg.PnnxBuilder(seed=3)
    x = b.relu(b.conv(b.relu(b.conv(b.input((2, 3, 12, 12)), 16, 3, 1, 1)), 16, 3, 1, 1))   # (two convs: the one movement reads is not the RGB stem)
    v1 = b.view(b.permute(x, (0, 2, 3, 1)), (2, -1, 4))
    v2 = b.view(v1, (2, -1, 8))
    for r in (b.sigmoid(v1), b.sigmoid(v2)):
        b.output(r)
    return b, (v1, v2)


def chunk_of_view():
    """conv -> view(N, C, H W, 1) (the same bytes under another rank-4 shape) -> chunk(2, dim 1), a sigmoid on each half"""
    b = mg.PnnxBuilder(seed=4)
    x = b.relu(b.conv(b.relu(b.conv(b.input((2, 3, 12, 12)), 16, 3, 1, 1)), 16, 3, 1, 1))   # (two convs: the one movement reads is not the RGB stem)
    v = b.view(x, (2, 16, 144, 1))
    halves = b.chunk(v, 2, 1)
    for h in halves:
        b.output(b.sigmoid(h))
    return b, (v,) + tuple(halves)


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("make", [view_of_view, chunk_of_view], ids=["view_of_view", "chunk_of_view"])
def test_views_of_views_share_the_root_buffer(gpu, tmp_path, make, fp16):
    """with the arena on, every view is an alias whose readers keep the ROOT buffer alive: the results are those of the plan without aliases
    and without the arena, and of the graph whose intermediate results are graph outputs"""
    b, views = make()
    x = toy_input(b)
    e, got = run_engine(b, tmp_path, x, fp16=fp16)
    assert set(views) <= set(e.schedule()["alias"]), e.schedule()["alias"]
    assert all(L["kernel"] == "view" for L in e.profile() if L["type"] in lr.LAYOUT_TYPES + ("torch.chunk",))
    _, plain = run_engine(b, tmp_path, x, fp16=fp16, alias_view=0, alias_split=0, arena=0, fuse_layout=0)
    for out in graph_outputs(b):
        same_bits(got[out], plain[out], "%s output %s" % (make.__name__, out))
    taps = lr.tap_operands(b)
    _, probed = run_engine(lr.probe_builder(b, taps), tmp_path, x, tag="probe", fp16=fp16)
    for out in graph_outputs(b):                  # (the graph outputs are arithmetic on moved data: taps themselves)
        same_bits(got[out], probed[out], "%s output %s against the probe" % (make.__name__, out))


def one_chain(shape, chain):
    b = mg.PnnxBuilder(seed=6)
    x = b.input(shape)
    for name, args in chain:
        x = getattr(b, name)(x, *args)
    b.output(x)
    return b


GOOD = [("Tensor.permute", (2, 5, 6, 7), [("permute", ((0, 3, 1, 2),))]),
        ("torch.permute", (2, 5, 6, 7), [("permute", ((0, 2, 3, 1), True))]),
        ("Tensor.reshape", (2, 6, 5, 4), [("reshape", ((2, 3, -1),))]),
        ("torch.transpose", (3, 70, 9), [("transpose", (1, 2))]),
        ("transpose_negative", (2, 5, 6, 7), [("transpose", (-1, -3))]),
        ("squeeze_unsqueeze", (2, 5, 6), [("unsqueeze", (1,)), ("transpose", (2, 3)), ("squeeze", (1,))]),
        ("Tensor.contiguous", (2, 5, 6, 7), [("permute", ((0, 2, 3, 1),)), ("contiguous", ())]),
        ("rank2", (6, 35), [("transpose", (0, 1))])]


@pytest.mark.parametrize("case", GOOD, ids=[c[0] for c in GOOD])
def test_one_chain_graphs(gpu, tmp_path, case):
    """graph input -> layout operators -> graph output (nothing can be aliased: one copy) against numpy on the file-order array"""
    _, shape, chain = case
    b = one_chain(shape, chain)
    x_file = numbered(int(np.prod(shape)), np.float32).reshape(shape)
    want = x_file
    for typ, _, _, _, prm in (_parse(ln) for ln in b.lines[1:-1]):
        want = lr.apply_op(want, *lr.line_op(typ, prm))
    for opts in ({}, dict(fuse_layout=0)):
        e, got = run_engine(b, tmp_path, lr.stored(x_file), **opts)
        same_bits(got[graph_outputs(b)[0]], np.ascontiguousarray(want), "%s %r" % (case[0], opts))
        assert e.schedule()["alias"] == []
        assert len(layout_layers(e.profile())) == (len(chain) if opts else 1)


RANK5 = {
    # the raw YOLOv5 head's chain (na = 3, no = 7) and the channel shuffle (g = 3), as functions of the batch
    "yolov5_view_permute_view": ((21, 5, 6), lambda n: [("view", ((n, 3, 7, 5, 6),)), ("permute", ((0, 1, 3, 4, 2),)), ("view", ((n, -1, 7),))]),
    "shuffle_view_transpose_view": ((24, 5, 6), lambda n: [("view", ((n, 3, 8, 5, 6),)), ("transpose", (1, 2)), ("view", ((n, 24, 5, 6),))]),
    "yolov5_wide": ((96, 9, 8), lambda n: [("view", ((n, 3, 32, 9, 8),)), ("permute", ((0, 1, 3, 4, 2),)), ("view", ((n, -1, 32),))]),
    "shuffle_wide": ((1024, 3, 3), lambda n: [("view", ((n, 32, 32, 3, 3),)), ("transpose", (1, 2)), ("view", ((n, 1024, 3, 3),))]),   # the tile form
}


@pytest.mark.parametrize("batch", [0, 3], ids=["file_batch", "rebatched"])
@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("which", sorted(RANK5))
def test_rank5_chains_against_numpy(gpu, tmp_path, which, fp16, batch):
    """relu -> a chain through rank-5 intermediates -> relu on positive data (the relus only make the chain's operands internal -- halves under
    fp16 storage -- and change no value) against numpy's reshape / transpose of the file-order array: the fused chain itself, with nothing of the
    engine in the expected value; at the file's batch and re-batched from 2 to 3"""
    chw, chain = RANK5[which]
    b = mg.PnnxBuilder(seed=6)
    y = b.relu(b.input((2,) + chw))
    for name, args in chain(2):
        y = getattr(b, name)(y, *args)
    b.output(b.relu(y))
    n = batch or 2
    r = np.random.Generator(np.random.Philox(8))
    x_file = (r.random((n,) + chw, dtype=np.float32) + np.float32(0.5))
    if fp16:
        x_file = x_file.astype(np.float16).astype(np.float32)       # (what the first relu stores)
    want = x_file
    for name, args in chain(n):
        want = lr.apply_op(want, name, args[0] if name != "transpose" else args)
    e, got = run_engine(b, tmp_path, lr.stored(x_file), fp16=fp16, batch=batch)
    same_bits(got[graph_outputs(b)[0]], np.ascontiguousarray(want), "%s fp16=%d batch=%d" % (which, fp16, n))
    layers = layout_layers(e.profile())
    assert len(layers) == 1 and layers[0]["kernel"].startswith("permute_"), layers      # one launch for the whole chain
    _, cap = run_engine(b, tmp_path, lr.stored(x_file), fp16=fp16, batch=batch, graph=1, forwards=3)
    same_bits(cap[graph_outputs(b)[0]], np.ascontiguousarray(want), "%s captured" % which)


def two_input_view():
    b = mg.PnnxBuilder(seed=6)
    x = b.input((2, 4, 3, 3))
    s = b.input((3,))
    out = b._new_operand((2, 4, 9))
    b._emit("Tensor.view", "Tensor_view_0", [x, s], [out])
    b.output(out)
    return b


def cat_dim_out_of_range():
    b = mg.PnnxBuilder(seed=6)
    x, y = b.input((2, 5, 6)), b.input((2, 5, 6))
    out = b._new_operand((2, 5, 12))
    b._emit("torch.cat", "cat_0", [x, y], [out], dict(dim=3))
    b.output(out)
    return b


BAD = {
    "cat_rank3_dim_out_of_range": (cat_dim_out_of_range, {}, Status.kErrorShape),
    "rank5_graph_output": (lambda: one_chain((2, 12, 5, 7), [("view", ((2, 3, 4, 5, 7),))]), {}, Status.kUnsupport),
    "rank5_intermediate_unfused": (lambda: mg.build_toy_yolov5_raw_head(), dict(fuse_layout=0), Status.kUnsupport),
    "non_dividing_reshape": (lambda: one_chain((2, 12, 5, 8), [("view", ((2, 8, -1),))]), {}, Status.kUnsupport),
    "two_input_view": (two_input_view, {}, Status.kUnsupport),
    "folded_batch_rebatched": (lambda: one_chain((2, 4, 3, 3), [("permute", ((0, 2, 3, 1),)), ("view", ((-1, 4),))]), dict(batch=3), Status.kUnsupport),
    "shape_disagrees": (lambda: None, {}, Status.kErrorShape),
}


@pytest.mark.parametrize("which", sorted(BAD))
def test_refused_at_load_and_the_process_goes_on(gpu, tmp_path, which):
    make, opts, status = BAD[which]
    if which == "shape_disagrees":
        b = one_chain((2, 12, 5, 7), [("permute", ((0, 2, 3, 1),)), ("view", ((2, -1, 4),))])
        b.lines = [ln.replace("(2,105,4)f32", "(2,104,4)f32") for ln in b.lines]
    else:
        b = make()
    pp, bp = save(b, tmp_path, "bad")
    e = Engine(**opts)
    with pytest.raises(StatusError) as err:
        e.load_model(pp, bp)
    assert err.value.status == status, (which, err.value.status)
    if which == "folded_batch_rebatched":          # ... at the file's batch it is served
        x = numbered(2 * 4 * 9, np.float32).reshape(2, 3, 3, 4)
        _, got = run_engine(b, tmp_path, x, tag="folded")
        same_bits(got[graph_outputs(b)[0]], x.reshape(18, 4), "folded batch at the file's batch")
    good = mg.build_toy_ssd_head()
    x = toy_input(good)
    pp, bp = save(good, tmp_path, "good")
    e.set_option("batch", 0)
    e.set_option("fuse_layout", 1)
    e.load_model(pp, bp)                           # the same engine object loads and runs a good model
    e.input(e.input_names()[0], x)
    e.forward()
    _, fresh = run_engine(good, tmp_path, x, tag="fresh")
    (out,) = graph_outputs(good)
    same_bits(np.ascontiguousarray(e.extract(out)), fresh[out], "after the refusal")


# ---- torch.cat on rank 2 and rank 3 ---------------------------------------------------------------------------------------
CAT = [((3, 5, 6), (3, 4, 6), 1), ((3, 5, 6), (3, 5, 7), 2), ((3, 5, 6), (2, 5, 6), 0), ((3, 5, 7), (3, 2, 7), -2), ((3, 5, 3), (3, 5, 4), -1),
       ((2, 160, 4), (2, 160, 3), 2), ((4, 10), (4, 7), 1), ((4, 10), (3, 10), 0), ((4, 9), (4, 3), -1), ((5, 7), (2, 7), -2)]


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("case", CAT, ids=["%s_%s_dim%d" % ("x".join(map(str, a)), "x".join(map(str, b)), d) for a, b, d in CAT])
def test_cat_rank2_rank3(gpu, tmp_path, case, fp16):
    """relu(a), relu(b) -> torch.cat on every axis of rank-3 and rank-2 tensors (positive data: the relu only makes the operands internal,
    half under fp16 storage -- odd widths included) against numpy"""
    sa, sb, dim = case
    b = mg.PnnxBuilder(seed=2)
    a_, b_ = b.input(sa), b.input(sb)
    shp = list(sa)
    shp[dim] = sa[dim] + sb[dim]
    out = b._new_operand(shp)
    b._emit("torch.cat", "cat_0", [b.relu(a_), b.relu(b_)], [out], dict(dim=dim))
    b.output(out)
    r = np.random.Generator(np.random.Philox(5))
    xa, xb = (r.random(s, dtype=np.float32) + np.float32(0.5) for s in (sa, sb))
    pp, bp = save(b, tmp_path, "cat")
    e = Engine(fp16=fp16)
    e.load_model(pp, bp)
    e.input(a_, xa)
    e.input(b_, xb)
    e.forward()
    q = (lambda v: v.astype(np.float16).astype(np.float32)) if fp16 else (lambda v: v)
    same_bits(np.ascontiguousarray(e.extract(out)), np.concatenate([q(xa), q(xb)], dim), "cat %r fp16=%d" % (case, fp16))
