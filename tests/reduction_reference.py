"""What the restatements of the three reduction operators share (softmax_reference, reduce_reference, lpnorm_reference; test
infrastructure, no product code): reading a switch value from a header's enum, the name of a kernel instantiation as a profile shows it, and
the NHWC axis mask (1 n, 2 h, 4 w, 8 c) of torch's dims.  The three modules re-export these under the names their tests import."""
import re

import numpy as np

AXIS_N, AXIS_H, AXIS_W, AXIS_C = 1, 2, 4, 8


def header_enum_of(header):
    """header_enum(name) for one header file: the value of `name = <int>` in it"""
    def header_enum(name):
        return int(re.search(r"\b%s = (\d+)" % name, open(header).read()).group(1))
    return header_enum


def kname_of(operator):
    """kname(form, dtype, vec) for one operator: <operator>_<form>_kernel<T, VW>"""
    def kname(form, dtype, vec):
        base = "%s_%s_kernel" % (operator, form)
        if np.dtype(dtype) == np.float32:
            return base + ("<float, 4>" if vec else "<float, 1>")
        return base + ("<_Float16, 8>" if vec else "<_Float16, 1>")
    return kname


def mask_axes(axes):
    return tuple(a for a in range(4) if (axes >> a) & 1)


def positions(shape, axes):
    return int(np.prod([shape[a] for a in mask_axes(axes)]))


def nhwc_mask(dims, rank):
    """torch's dim (an int or a sequence) on an NCHW (or [N, F]) tensor -> the NHWC bit mask of the descriptor"""
    mask = 0
    for dim in ((dims,) if isinstance(dims, int) else dims):
        dim = dim + rank if dim < 0 else dim
        assert 0 <= dim < rank and rank in (2, 4), (dim, rank)
        axis = (0, 3)[dim] if rank == 2 else (0, 3, 1, 2)[dim]
        assert not mask & (1 << axis), "a repeated dim"
        mask |= 1 << axis
    return mask
