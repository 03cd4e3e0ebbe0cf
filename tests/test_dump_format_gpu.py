"""The device formatter of `dump custom` (csrc/sf_dump_fmt.h through sfk_dump_format) against glibc's own printf, called
through ctypes: "%g" on more than four million doubles and "%d" on ints, zero differing bytes.  (Python's "%" operator
is not the yardstick: it prints "nan" where glibc prints "-nan".)"""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_libc = C.CDLL(ctypes.util.find_library("c"))
_snprintf = _libc.snprintf


def _libc_lines(fmt, values, ctype):
    _snprintf.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, ctype]
    _snprintf.restype = C.c_int
    buf = C.create_string_buffer(64)
    out = []
    for v in values.tolist():
        n = _snprintf(buf, 64, fmt, v)
        out.append(buf.raw[:n])
    return out


def _edge_values(rng):
    f = np.finfo(np.float64)
    bits = lambda u: np.array(u, dtype=np.uint64).view(np.float64)
    vals = [0.0, -0.0, np.inf, -np.inf, f.max, -f.max, f.tiny, -f.tiny, f.smallest_subnormal, -f.smallest_subnormal,
            9.999995, 999999.5, 1234565.0, 1234575.0, 99999.95, 0.5, 1.5, 2.5, 0.0015, 8.21723e-06]
    vals += list(bits([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001,
                       0x000FFFFFFFFFFFFF, 0x8000000000000001]))   # nan, -nan, signalling, largest subnormal
    # the decimal boundaries of the fixed / exponent switch and their neighbours, every decade of the range
    p = 10.0 ** np.arange(-325, 309, dtype=np.float64)
    p = p[np.isfinite(p) & (p > 0)]
    for m in (1.0, 9.999995, 9.9999949999999, 9.99999, 5.0, 1.000005):
        with np.errstate(over="ignore"):
            q = p * m
        vals += list(q) + list(np.nextafter(q, 0)) + list(np.nextafter(q, np.inf))
    # exact binary ties at the sixth digit: (2 D + 1) 2^s with D of six or seven digits, and their neighbours
    D = rng.integers(100000, 10000000, 150000)
    s = rng.integers(-24, 4, D.size)
    t = np.ldexp((2 * D + 1).astype(np.float64), s)
    vals += list(t) + list(np.nextafter(t, 0)) + list(np.nextafter(t, np.inf))
    # carries: values that round up into the next decade
    e = rng.integers(-320, 300, 50000)
    with np.errstate(over="ignore"):
        c = 9.9999950000000 * 10.0 ** e.astype(np.float64)
    vals += list(c[np.isfinite(c)])
    # subnormals
    u = rng.integers(1, 1 << 52, 100000, dtype=np.uint64)
    vals += list(u.view(np.float64))
    v = np.array(vals, dtype=np.float64)
    return np.concatenate([v, -v])


def test_device_g_is_byte_identical_to_glibc():
    from sedifoam_amd import format_values
    rng = np.random.default_rng(20261016)
    random_bits = rng.integers(0, 2 ** 63, 1_500_000, dtype=np.uint64, endpoint=True)
    random_bits ^= rng.integers(0, 2, random_bits.size, dtype=np.uint64) << np.uint64(63)
    log_uniform = 10.0 ** rng.uniform(-12.0, 3.0, 1_500_000) * rng.choice([-1.0, 1.0], 1_500_000)
    values = np.concatenate([random_bits.view(np.float64), log_uniform, _edge_values(rng)])
    assert values.size >= 4_000_000
    got = format_values(values=values)
    want = b"\n".join(_libc_lines(b"%g", values, C.c_double)) + b"\n"
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        bad = [k for k in range(min(len(g), len(w))) if g[k] != w[k]][:10]
        raise AssertionError("differs at %s: %s" % (bad, [(values[k].tobytes().hex(), g[k], w[k]) for k in bad]))


def test_device_d_is_byte_identical_to_glibc():
    from sedifoam_amd import format_values
    rng = np.random.default_rng(7)
    ints = np.concatenate([np.array([0, 1, -1, 9, 10, -10, 2 ** 31 - 1, -2 ** 31, -2 ** 31 + 1], dtype=np.int64),
                           rng.integers(-2 ** 31, 2 ** 31, 200000), 10 ** np.arange(10), -(10 ** np.arange(10))])
    ints = ints.astype(np.int32)
    got = format_values(ints=ints, values=[0.25])
    want = b"\n".join(_libc_lines(b"%d", ints, C.c_int)) + b"\n0.25\n"
    assert got == want


def test_empty_input_formats_to_nothing():
    from sedifoam_amd import format_values, format_g
    assert format_values() == b""
    assert format_g([1e-5, -0.0, 100000.0, 1e6]) == [b"1e-05", b"-0", b"100000", b"1e+06"]
