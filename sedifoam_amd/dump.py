"""The device formatter of `dump custom` (csrc/sf_dump_fmt.h) on host arrays: what every snapshot line is made of."""
import ctypes as C

import numpy as np

from ._lib import lib, check


def format_values(values=(), ints=()):
    """bytes of "%d\\n" for every int of `ints`, then "%g\\n" for every double of `values`, formatted on the GPU
    (sfk_dump_format) -- byte-identical to glibc printf"""
    v = np.ascontiguousarray(values, dtype=np.float64).ravel()
    i = np.ascontiguousarray(ints, dtype=np.int32).ravel()
    cap = 12 * i.size + 14 * v.size + 1
    out = C.create_string_buffer(cap)
    nbytes = C.c_longlong(0)
    check(lib().sfk_dump_format(v.ctypes.data if v.size else None, v.size, i.ctypes.data if i.size else None, i.size,
                                out, cap, C.byref(nbytes)))
    return out.raw[:nbytes.value]


def format_g(values):
    """the "%g" text of every double, as a list of bytes"""
    return format_values(values=values).split(b"\n")[:-1]
