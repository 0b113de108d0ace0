"""Shared plumbing of the element-wise arithmetic tests (tests/test_math.py on the CPU, tests/test_math_device_gpu.py on the GPU):
the operation list of csrc/probe/ssf_math_ops.h, the three evaluators (the CPU checker's batch entry, the device probe, the probe's
host branches), the input sets and the bit-pattern comparison.  Not a test module."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "supersurfel_fusion_amd", "csrc")
OPS_HEADER = os.path.join(CSRC, "probe", "ssf_math_ops.h")
PROBE_LIB = os.path.join(CSRC, "variants", "mathprobe", "libssf_mathprobe.so")
CHUNK = 1 << 24

# the (scale, limit) pairs the kernels pass to fx64, as exponents of two -- restated from the call sites (ssf_extract.hip,
# ssf_pass_tile.hpp, ssf_track_fuse.hip, ssf_odometry.hip), independent of both libraries
FX64_PAIRS = {"fx64_disp": (30, 52), "fx64_mom": (24, 40), "fx64_icp_r": (44, 62), "fx64_align_pos": (24, 52),
              "fx64_align_d2": (30, 52), "fx64_odo_a": (10, 40), "fx64_odo_b": (24, 40), "fx64_odo_c": (36, 40)}


def parse_ops():
    """{name: (number, in_words, out_words)} from the SSF_MATHOP lines of the shared header"""
    txt = open(OPS_HEADER).read()
    ops = {m[1]: (int(m[0]), int(m[2]), int(m[3])) for m in re.findall(r"SSF_MATHOP\((\d+),\s*(\w+),\s*(\d+),\s*(\d+)\)", txt)}
    assert len(ops) == int(re.search(r"#define SSF_MATHOP_COUNT (\d+)", txt).group(1))
    return ops


OPS = parse_ops()


def load_probe(path=None):
    """the device evaluator; built by csrc/Makefile (target mathprobe, part of all) when it is not there.  SSF_MATHPROBE_LIB names
    another build of the same source instead -- how a deliberately mutated ssf_math.hpp is shown to fail these tests."""
    import torch  # noqa: F401  (the HIP runtime the library links, as binding.load_lab does)
    path = path or os.environ.get("SSF_MATHPROBE_LIB") or PROBE_LIB
    if not os.path.exists(path):
        r = subprocess.run(["make", "-C", CSRC, "mathprobe"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    lib = C.CDLL(path)
    for fn in (lib.ssf_mathprobe_eval, lib.ssf_mathprobe_eval_host):
        fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]; fn.restype = C.c_int
    return lib


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(-1)


def evaluate(fn, name, x):
    """operation `name` on the elements of x (any dtype; viewed as 32-bit words) through fn(op, in, out, n), in chunks of 2^24
    elements -> uint32 array of shape (n, out_words)"""
    op, iw, ow = OPS[name]
    w = _words(x)
    assert w.size % iw == 0, (name, w.size, iw)
    n = w.size // iw
    out = np.empty((n, ow), np.uint32)
    for s in range(0, n, CHUNK):
        e = min(n, s + CHUNK)
        rc = fn(op, w[s * iw:].ctypes.data_as(C.c_void_p), out[s:].ctypes.data_as(C.c_void_p), e - s)
        assert rc == 0, "%s: evaluator returned %d" % (name, rc)
    return out


def _nan_mask(name, out):
    """where an output is a NaN of its type: the one equivalence the comparison allows (any sign, any payload)"""
    if name in F64_OUT:
        v = out.reshape(out.shape[0], -1, 2)
        hi, lo = v[..., 1], v[..., 0]
        nan = ((hi & 0x7FF00000) == 0x7FF00000) & (((hi & 0x000FFFFF) | lo) != 0)
        return np.repeat(nan, 2, axis=-1).reshape(out.shape)
    if name in INT_OUT:
        return np.zeros(out.shape, bool)
    m = ((out & 0x7F800000) == 0x7F800000) & ((out & 0x007FFFFF) != 0)
    if name in FLAG_FIRST:
        m[:, 0] = False
    return m


F64_OUT = {"div3_exact", "div_inrange", "cbrt_spec", "root5_spec"}
INT_OUT = set(FX64_PAIRS) | {"fx32r", "fx32_s20", "fx32_s24", "pixel_round", "div3_u64", "rng_draw", "guard"}
FLAG_FIRST = {"sym_inverse", "plane_solve"}


def differing(name, a, b):
    """indices of the elements whose outputs differ as bit patterns (NaN == NaN whatever sign or payload)"""
    same = (a == b) | (_nan_mask(name, a) & _nan_mask(name, b))
    return np.flatnonzero(~same.all(axis=1))


def hexwords(row):
    return " ".join("%08x" % int(w) for w in row)


def assert_same(name, x, got, want, who=("device", "oracle")):
    """0 differing elements; the message names the operation, the first differing input as a hex pattern and both outputs"""
    bad = differing(name, got, want)
    if bad.size:
        iw = OPS[name][1]
        i = int(bad[0])
        inp = _words(x).reshape(-1, iw)[i]
        raise AssertionError("%s: %d of %d elements differ; first at element %d, input words [%s] (%s): %s [%s], %s [%s]" % (
            name, bad.size, got.shape[0], i, hexwords(inp), describe(name, inp), who[0], hexwords(got[i]), who[1], hexwords(want[i])))
    return got.shape[0]


def describe(name, inp):
    iw = OPS[name][1]
    if name in set(FX64_PAIRS) | {"div3_exact", "div_inrange", "cbrt_spec", "root5_spec"}:
        return ", ".join(float(v).hex() for v in np.asarray(inp, np.uint32).view(np.float64))
    if name in ("div3_u64", "rng_draw", "rng_unit", "rgb8_to_lab", "guard"):
        return "integers"
    return ", ".join(float(v).hex() for v in np.asarray(inp, np.uint32).view(np.float32)[:iw])


# ---- input sets ------------------------------------------------------------------------------------------------------------
def f32_range(lo_exclusive, hi_inclusive):
    """every f32 in (lo, hi] for positive lo < hi, as bit patterns (consecutive patterns are consecutive values)"""
    lo = int(np.float32(lo_exclusive).view(np.uint32)); hi = int(np.float32(hi_inclusive).view(np.uint32))
    return np.arange(lo + 1, hi + 1, dtype=np.uint32)


def _neighbours32(vals):
    b = np.float32(vals).view(np.uint32).astype(np.int64)
    return np.concatenate([b - 1, b, b + 1]).astype(np.uint32)


def f32_binade_set(seed=1):
    """for each of the 256 exponents and both signs the first and last 4096 mantissas and 4096 seeded random ones (this holds
    +-0, the denormals, +-inf and NaNs of both signs with payloads); every k + 0.5 for |k| <= 2^12; the neighbours of +-2^23,
    +-2^31 and +-87.  uint32 bit patterns."""
    rng = np.random.default_rng(seed)
    first = np.arange(4096, dtype=np.uint32); last = np.uint32((1 << 23) - 4096) + first
    parts = []
    for e in range(256):
        m = np.concatenate([first, last, rng.integers(0, 1 << 23, 4096, dtype=np.uint32)])
        for s in (0, 1):
            parts.append(np.uint32((s << 31) | (e << 23)) | m)
    k = np.arange(-4096, 4097, dtype=np.float64)
    parts.append(np.float32(k + 0.5).view(np.uint32))
    parts.append(_neighbours32([8388608.0, -8388608.0, 2147483648.0, -2147483648.0, 87.0, -87.0]))
    parts.append(np.uint32([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 1, 0x80000001, 0x007FFFFF]))
    return np.concatenate(parts)


def f64_binade_set(seed=2):
    """the same set as doubles: each of the 2048 exponents, both signs, first / last / random 4096 mantissas.  uint64 patterns."""
    rng = np.random.default_rng(seed)
    first = np.arange(4096, dtype=np.uint64); last = np.uint64((1 << 52) - 4096) + first
    out = np.empty((2048, 2, 3 * 4096), np.uint64)
    for e in range(2048):
        m = np.concatenate([first, last, rng.integers(0, 1 << 52, 4096, dtype=np.uint64)])
        out[e, 0] = np.uint64(e << 52) | m
        out[e, 1] = np.uint64((1 << 63) | (e << 52)) | m
    return out.reshape(-1)


def _neighbours64(vals):
    b = np.float64(vals).view(np.uint64).astype(np.int64)
    return np.concatenate([b - 1, b, b + 1]).view(np.float64)


def fx64_edges(scale_bits, lim_bits):
    """per (scale, limit) pair: every value whose product with scale is k + 0.5, |k| <= 2^12; the neighbours of +-limit, +-2^50,
    +-2^51, +-2^52 and +-2^62 after scaling; +-0, +-inf, NaN.  Division by a power of two is exact for all of them.  f64."""
    k = np.arange(-4096, 4097, dtype=np.float64) + 0.5
    marks = [2.0 ** lim_bits, 2.0 ** 50, 2.0 ** 51, 2.0 ** 52, 2.0 ** 62]
    t = np.concatenate([k, _neighbours64(marks + [-m for m in marks])])
    v = np.ldexp(t, -scale_bits)
    assert (np.ldexp(v, scale_bits) == t).all()
    return np.concatenate([v, np.float64([0.0, -0.0, np.inf, -np.inf, np.nan])])


def log_uniform_f64(n, seed, lo=1e-30, hi=1e30):
    rng = np.random.default_rng(seed)
    v = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    return np.where(rng.integers(0, 2, n) == 1, -v, v)


def fx_exact(v, scale_bits, lim_bits):
    """round_half_even(v * 2^scale) clamped to +-2^limit in exact integer / rational arithmetic (NaN -> 0): the plain
    high-precision reference of fx64, through neither library"""
    out = np.empty(len(v), np.int64)
    lim = 1 << lim_bits
    for i, x in enumerate(v):
        x = float(x)
        if x != x:
            q = 0
        elif x in (float("inf"), float("-inf")):
            q = lim if x > 0 else -lim
        else:
            q = max(-lim, min(lim, round(Fraction(x) * (1 << scale_bits))))     # round(Fraction): ties to even
        out[i] = q
    return out


def fx_exact_subset(name, seed=5, total=20000):
    """the 20 000 values of the exact-integer check of one pair: all its edge values + seeded picks of the binade and log-uniform sets"""
    sb, lb = FX64_PAIRS[name]
    edges = fx64_edges(sb, lb)
    rng = np.random.default_rng(seed)
    n = total - len(edges)
    e = rng.integers(0, 2048, n // 2).astype(np.uint64); m = rng.integers(0, 1 << 52, n // 2, dtype=np.uint64)
    s = rng.integers(0, 2, n // 2).astype(np.uint64)
    binade = ((s << np.uint64(63)) | (e << np.uint64(52)) | m).view(np.float64)
    return np.concatenate([edges, binade, log_uniform_f64(n - n // 2, seed + 1)])


def div_hard_cases(count, seed):
    """(n, d) pairs of div_inrange's stated ranges whose exact quotient lies as close to the midpoint between two doubles as a
    quotient of doubles can: for an odd 53-bit d, the 54-bit odd m with d m = -+1 (mod 2^54) makes n = (d m +- 1) / 2^54 an integer
    and n / d = (m +- 1 / d) / 2^54 -- 2^-54 of a unit in the last place beside the midpoint m / 2^54.  A quotient assembled from
    a reciprocal that is not the correctly rounded one rounds these to the wrong side; random pairs never come this close.
    Scaled by 2^-53: n in [0.25, 1), d in [0.5, 1), n / d in [0.5, 1)."""
    rng = np.random.default_rng(seed)
    out = np.empty((count, 2), np.float64)
    k = 0
    while k < count:
        for d in rng.integers(1 << 51, 1 << 52, 4096, dtype=np.uint64):
            d = (int(d) << 1) | 1                                        # odd, in [2^52, 2^53)
            inv = pow(d, -1, 1 << 54)
            for m, r in (((1 << 54) - inv, 1), (inv, -1)):               # d m = -1 -> add 1;  d m = +1 -> subtract 1
                if m >> 53 and k < count:
                    n = (d * m + r) >> 54
                    assert (n << 54) == d * m + r and n < (1 << 53)
                    out[k] = (float(n) / 9007199254740992.0, float(d) / 9007199254740992.0); k += 1
    return out
