"""The order rule of include/si_nearest.h in numpy: candidates (key, column) compared lexicographically, a NaN key in front of every number
and NaN keys tied -- the first NaN wins, as torch.argmin has it."""
import numpy as np


def topk(keys, k):
    """the columns of the k best keys of every row of keys [.., R] (distances: no key is below 0), best first"""
    keys = np.asarray(keys, np.float64)
    return np.argsort(np.where(np.isnan(keys), -np.inf, keys), axis=-1, kind="stable")[..., :k].astype(np.int32)


def vq_refusals():
    """graphs LoadModel refuses (pnnx/lower_nearest_rows.h): the indices as a graph output, a different table, p = 1"""
    from simpleinfer_amd import modelgen as mg
    cases = {}
    for name in ("i is an output", "another table", "p = 1"):
        b = mg.PnnxBuilder(seed=2)
        z, table = b.input((2, 9, 8)), np.arange(40, dtype=np.float32).reshape(5, 8)
        i = b.argmin(b.cdist(z, b.attribute(table), 1.0 if name == "p = 1" else 2.0))
        b.output(b.embedding(i, table + 1 if name == "another table" else table))
        if name == "i is an output":
            b.output(i)
        cases[name] = b
    return cases


def kname(dtype, vec, k):
    return "nearest_kernel<%s, %s, %d>" % ("_Float16" if np.dtype(dtype) == np.float16 else "float", "true" if vec else "false", k)
