"""What the wrappers of the draw-fed models share (classify.py, tsne.py, random_forest.py; csrc/draw_model.hpp on the library's side)."""
import ctypes as C

import numpy as np

from ._lib import Handle, arr  # (Handle: re-exported for the draw-fed models)

DRAW_STRIDE = 0x9E3779B97F4A7C15  # POLEE_DRAW_STRIDE (csrc/common.hpp)
MASK = (1 << 64) - 1


def draw_seed(seed, i):
    """the seed of the draw with index i of a call under `seed`, as the library forms it"""
    return (int(seed) + DRAW_STRIDE * int(i)) & MASK


def approx_of(vars, ctx):
    """LoadedSamples.variables (its "approx" handle), an RNASeqApproxLikelihood, or the dict of create_tensorflow_variables!"""
    from .core import RNASeqApproxLikelihood
    if isinstance(vars, dict) and isinstance(vars.get("approx"), RNASeqApproxLikelihood):
        return vars["approx"]
    return vars if isinstance(vars, RNASeqApproxLikelihood) else RNASeqApproxLikelihood(vars, ctx=ctx)


def z0_flat(z0, count):
    """the optional N(0,1) noise of a call, flat f32 of exactly `count` values, or None"""
    if z0 is None:
        return None
    z = arr(z0, np.float32).reshape(-1)
    if z.size != count:
        raise ValueError("z0 must hold %d values" % count)
    return z


def make_opts(cls, default_fn, kw):
    """an opts structure with the library's defaults, overridden by keyword; an unknown keyword is a TypeError"""
    o = cls()
    default_fn.restype = None
    default_fn(C.byref(o))
    for name, v in kw.items():
        if name not in dict(cls._fields_):
            raise TypeError("unknown option %r" % name)
        setattr(o, name, v)
    return o
