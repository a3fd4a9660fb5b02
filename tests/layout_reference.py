"""Restatements for the layout tests (test infrastructure, no product code).

apply_ops: numpy transpose / reshape on the FILE-order (NCHW) array, the yardstick of the layout algebra; stored / unstored convert between
file order and the engine's storage (rank 4: NHWC, every other rank as it is).

expected_gather: for an input whose stored elements are numbered 0, 1, 2, .. the stored output of a chain, flattened -- the element order the
algebra has to reproduce; nest_gather: the same from a (dims, in_stride) loop nest.

random_chain: seeded random chains of layout operators over extents from {1, 2, 3, 4, 6}, intermediates up to rank 5.

eval_graph: a torch runner of a PnnxBuilder graph.  Data movement (the layout operators, torch.cat, torch.flatten) is computed by torch, bit
for bit; every operator that does arithmetic takes its output from `taps` (operand name -> file-order array, e.g. extracted from an engine whose
graph outputs are those operands: probe_builder) or, without taps, from torch in float64.  With taps every value a movement operator produces
is exactly what the engine has to produce from its own arithmetic.  Taps computed FROM moved data carry the engine's own movement, so they only
serve the graph's tail: the movement itself is judged at moved_checkpoints -- the movement results that arithmetic reads -- from the taps that
movement reads (read_by_movement) alone.
"""
import numpy as np

from ct_reference import _ints, _parse

LAYOUT_TYPES = ("Tensor.permute", "torch.permute", "Tensor.reshape", "Tensor.view", "torch.transpose", "torch.squeeze", "torch.unsqueeze",
                "Tensor.contiguous")
ABSENT_TYPES = ("torch.stack", "Tensor.expand", "Tensor.repeat", "torch.einsum")
MOVEMENT_TYPES = LAYOUT_TYPES + ("torch.cat", "torch.flatten", "torch.chunk")
EXTENTS = (1, 2, 3, 4, 6)


def stored(a):
    """file order -> storage order"""
    return np.ascontiguousarray(np.moveaxis(a, -3, -1)) if a.ndim > 3 else np.ascontiguousarray(a)


def unstored(a):
    """storage order -> file order"""
    return np.moveaxis(a, -1, -3) if a.ndim > 3 else a


def apply_op(a, name, args):
    if name == "permute":
        return a.transpose([int(d) for d in args])
    if name in ("reshape", "view"):
        return np.ascontiguousarray(a).reshape([int(s) for s in args])
    if name == "transpose":
        return a.swapaxes(int(args[0]), int(args[1]))
    if name == "squeeze":
        d = int(args[0]) if isinstance(args, (tuple, list)) else int(args)
        return a.squeeze(d) if a.shape[d] == 1 else a
    if name == "unsqueeze":
        d = int(args[0]) if isinstance(args, (tuple, list)) else int(args)
        return np.expand_dims(a, d if d >= 0 else d + a.ndim + 1)
    if name == "contiguous":
        return a
    raise NotImplementedError(name)


def apply_ops(a, ops):
    for name, args in ops:
        a = apply_op(a, name, args)
    return a


def expected_gather(in_shape, ops):
    """(the output's file shape, the stored output flattened) for an input whose STORED elements are 0, 1, 2, .."""
    in_shape = tuple(int(s) for s in in_shape)
    sshape = in_shape if len(in_shape) < 4 else in_shape[:-3] + in_shape[-2:] + in_shape[-3:-2]
    x = unstored(np.arange(int(np.prod(in_shape)), dtype=np.int64).reshape(sshape))
    y = apply_ops(x, ops)
    return tuple(y.shape), stored(y).reshape(-1)


def nest_gather(dims, in_stride):
    idx = np.zeros([int(d) for d in dims] or [1], np.int64)
    for k, (n, s) in enumerate(zip(dims, in_stride)):
        idx += (np.arange(n, dtype=np.int64) * int(s)).reshape([n if j == k else 1 for j in range(len(dims))])
    return idx.reshape(-1)


def _factor(rng, count, rank):
    """a random shape of `rank` dimensions with `count` elements (count's primes are 2 and 3)"""
    shape = [1] * rank
    for p in (2, 3):
        while count % p == 0:
            shape[int(rng.integers(0, rank))] *= p
            count //= p
    assert count == 1
    return shape


def random_chain(rng, rank):
    """(in_shape, ops) with 1 .. 4 operators; the output has rank 1 .. 4, intermediates up to rank 5"""
    shape = [int(rng.choice(EXTENTS)) for _ in range(rank)]
    in_shape, ops = tuple(shape), []
    for _ in range(int(rng.integers(1, 5))):
        r = len(shape)
        kind = int(rng.integers(0, 6))
        if kind == 0 and r > 1:
            p = [int(v) for v in rng.permutation(r)]
            ops.append(("permute", tuple(p)))
            shape = [shape[d] for d in p]
        elif kind == 1 and r > 1:
            a, b = (int(v) for v in rng.choice(r, 2, replace=False))
            if rng.integers(0, 2):
                a -= r
            ops.append(("transpose", (a, b)))
            shape[a], shape[b] = shape[b], shape[a]
        elif kind == 2:
            d = int(rng.integers(-r, r))
            ops.append(("squeeze", (d,)))
            if shape[d] == 1 and r > 1:
                del shape[d % r]
            elif shape[d] == 1:
                ops.pop()
        elif kind == 3 and r < 5:
            d = int(rng.integers(-r - 1, r + 1))
            ops.append(("unsqueeze", (d,)))
            shape.insert(d if d >= 0 else d + r + 1, 1)
        else:
            new = _factor(rng, int(np.prod(shape)), int(rng.integers(1, 6)))
            arg = list(new)
            if rng.integers(0, 2):
                arg[int(rng.integers(0, len(arg)))] = -1
            ops.append(("view" if rng.integers(0, 2) else "reshape", tuple(arg)))
            shape = new
    if len(shape) > 4:
        shape = _factor(rng, int(np.prod(shape)), int(rng.integers(1, 5)))
        ops.append(("reshape", tuple(shape)))
    return in_shape, ops


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def line_op(typ, prm):
    """a builder line of a layout type as (name, args) for apply_op"""
    if typ in ("Tensor.permute", "torch.permute"):
        return "permute", _ints(prm["dims"])
    if typ in ("Tensor.reshape", "Tensor.view"):
        return "reshape", _ints(prm["shape"])
    if typ == "torch.transpose":
        return "transpose", (int(prm["dim0"]), int(prm["dim1"]))
    if typ in ("torch.squeeze", "torch.unsqueeze"):
        return typ.split(".")[1], (int(prm["dim"]),)
    assert typ == "Tensor.contiguous", typ
    return "contiguous", ()


def tap_operands(builder, entering_only=False):
    """the arithmetic operators' outputs that eval_graph(taps=) needs: those a movement operator reads, and those computed from a movement
    operator's output (the backbone in front of the first layout operator stays inside the engine)"""
    lines = [_parse(ln) for ln in builder.lines]
    moved, read_by_movement = set(), set()
    for typ, _, ins, outs, _ in lines:
        if typ in MOVEMENT_TYPES:
            moved.update(outs)
            read_by_movement.update(ins)
        elif set(ins) & moved:
            moved.update(outs)      # (arithmetic on moved data: its result is moved data too)
    taps = [outs[0] for typ, _, ins, outs, _ in lines
            if typ not in MOVEMENT_TYPES and typ not in ("pnnx.Input", "pnnx.Output") and (outs[0] in read_by_movement or outs[0] in moved)]
    # entering_only: the taps that owe nothing to a movement operator (the arithmetic in front of the first one)
    return [r for r in taps if r not in moved] if entering_only else taps


def read_by_movement(builder):
    """the operands a movement operator reads: under fp16 storage these are stored as halves"""
    return {r for typ, _, ins, _, _ in (_parse(ln) for ln in builder.lines) if typ in MOVEMENT_TYPES for r in ins}


def moved_checkpoints(builder):
    """the movement results that arithmetic reads (rank <= 4: they can be graph outputs): the operands at which the movement itself is
    compared with torch, with nothing of the engine's own movement in the expected value"""
    lines = [_parse(ln) for ln in builder.lines]
    made = {o for typ, _, _, outs, _ in lines if typ in MOVEMENT_TYPES for o in outs}
    return [r for r in dict.fromkeys(r for typ, _, ins, _, _ in lines if typ not in MOVEMENT_TYPES and typ != "pnnx.Output" for r in ins)
            if r in made and len(builder.shapes[r]) <= 4]


def probe_builder(builder, operands):
    """a copy of the graph whose graph outputs are `operands` (its own outputs dropped): the engine that loads it hands out its arithmetic"""
    import copy
    b = copy.copy(builder)
    b.lines = [ln for ln in builder.lines if not ln.startswith("pnnx.Output")]
    b.n_ops = len(b.lines)
    b.attrs, b.shapes = dict(builder.attrs), dict(builder.shapes)
    b._counts = dict(builder._counts)
    for r in operands:
        b.output(r)
    return b


def eval_graph(builder, x_nhwc, taps=None, want=None):
    """file-order result of the graph output (want: a list of operands instead -> {operand: file-order array}).  taps: {operand: file-order array} for every arithmetic operator's output (bit-exact mode);
    None: arithmetic in torch float64 (the CPU tests' mode, layout_types only need numpy but torch.cat / conv come from torch)."""
    import torch
    F = torch.nn.functional
    vals, result = {}, None
    for typ, name, ins, outs, prm in (_parse(ln) for ln in builder.lines):
        a = lambda k: torch.from_numpy(np.ascontiguousarray(builder.attrs["%s.%s" % (name, k)], dtype=np.float64))
        if typ == "pnnx.Input":
            x = np.asarray(x_nhwc, np.float32 if taps is not None else np.float64)
            vals[outs[0]] = torch.from_numpy(np.ascontiguousarray(unstored(x))) if taps is None else None
            continue
        if typ == "pnnx.Output":
            result = vals[ins[0]]
            continue
        x = vals[ins[0]]
        if taps is not None and typ in MOVEMENT_TYPES and any(vals[i] is None for i in ins):
            for o in outs:
                vals[o] = None      # (moves something no tap covers: nothing downstream of it is asked for)
            continue
        if typ in LAYOUT_TYPES:
            op, args = line_op(typ, prm)
            if op == "permute":
                y = x.permute(*args)
            elif op == "reshape":
                y = x.reshape(*args)
            elif op == "transpose":
                y = torch.transpose(x, *args)
            elif op == "squeeze":
                y = torch.squeeze(x, args[0])
            elif op == "unsqueeze":
                y = torch.unsqueeze(x, args[0])
            else:
                y = x.contiguous()
        elif typ == "torch.cat":
            y = torch.cat([vals[i] for i in ins], int(prm["dim"]))
        elif typ == "torch.flatten":
            y = torch.flatten(x, 1)
        elif typ == "torch.chunk":
            for o, piece in zip(outs, torch.chunk(x, int(prm["chunks"]), int(prm["dim"]))):
                vals[o] = piece
            continue
        elif taps is not None:
            if outs[0] not in taps:
                vals[outs[0]] = None
                continue
            y = torch.from_numpy(np.ascontiguousarray(taps[outs[0]], dtype=np.float32))
        elif typ == "nn.Conv2d":
            y = F.conv2d(x, a("weight"), a("bias") if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"]),
                         _ints(prm["dilation"]), int(prm["groups"]))
        elif typ == "nn.ReLU":
            y = F.relu(x)
        elif typ == "nn.Sigmoid":
            y = torch.sigmoid(x)
        elif typ == "nn.AdaptiveAvgPool2d":
            y = F.adaptive_avg_pool2d(x, _ints(prm["output_size"]))
        elif typ == "nn.Linear":
            y = F.linear(x, a("weight"), a("bias") if prm["bias"] == "True" else None)
        else:
            raise NotImplementedError(typ)
        assert tuple(y.shape) == tuple(builder.shapes[outs[0]]), (typ, name, tuple(y.shape), builder.shapes[outs[0]])
        vals[outs[0]] = y
    if want is not None:
        return {r: np.ascontiguousarray(vals[r].numpy()) for r in want}
    return np.ascontiguousarray(result.numpy())
