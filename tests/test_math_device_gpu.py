"""The arithmetic specification ON THE DEVICE, element by element: device == oracle at 0 bits.

csrc/probe/ssf_math_probe.hip (variants/mathprobe/libssf_mathprobe.so, built with the product's flags) runs every helper of
csrc/ssf_math.hpp in one element-wise kernel per operation, so the branches that only the GPU compiles -- fx64's min / max clamp and
magic-number rounding, fx32r's v_cvt_i32_f32, div_inrange's reciprocal + Newton steps, div3_u64's register barrier -- are evaluated on
their own and compared with the CPU checker's plain restatement (oracle/oracle_mathbatch.cpp: llrint, three compares, n / d, b / 3,
x / 3.0), exhaustively over the domains the kernels use and on every binade elsewhere.  Results are compared as bit patterns; the
one equivalence is NaN == NaN whatever sign or payload.  No element is skipped or masked, nothing rests on a tolerance.  A failure
names the operation, the first differing input as a hex pattern and both outputs.  Each test prints how many elements it compared.

Outside a helper's stated domain (test_outside_the_stated_domains): div3_exact, div_inrange and cbrt_spec are only proven for positive
normal operands of moderate exponent.  Their only caller chain is lab_f / srgb_compress / srgb_expand, whose guards (t > 0.008856f,
c > 0.0031308f, c > 0.04045f) hand them positive f32 values widened to double -- exponents within +-150 -- or +inf; those guarded
entry points are compared on EVERY binade of both signs, +-0, denormals, +-inf and NaN (test_f32_helpers_on_every_binade), which is
what keeps hostile model colours (ssf_set_model takes arbitrary floats) inside the contract.
"""
import ctypes as C
import os

import numpy as np
import pytest

import mathops as mo

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WHO = ("device", "oracle")


@pytest.fixture(scope="module")
def dev():
    """the device evaluator: ssf_mathprobe_eval(op, in, out, n) allocates, copies in, launches, copies out, frees"""
    return mo.load_probe().ssf_mathprobe_eval


@pytest.fixture(scope="module")
def probe():
    return mo.load_probe()


@pytest.fixture(scope="module")
def orc(oracle_lib):
    fn = oracle_lib.lib.ssf_oracle_mathbatch
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]; fn.restype = C.c_int
    return fn


@pytest.fixture(scope="module")
def b32():
    return mo.f32_binade_set()


@pytest.fixture(scope="module")
def b64():
    return mo.f64_binade_set()


def check(dev, orc, name, x):
    """device == oracle on every element of x (one array, or an iterable of chunks); returns the number compared"""
    n = 0
    for part in ([x] if isinstance(x, np.ndarray) else x):
        n += mo.assert_same(name, part, mo.evaluate(dev, name, part), mo.evaluate(orc, name, part), WHO)
    print("%s: %d elements compared, 0 differ" % (name, n))
    return n


def chunks(bits, convert=None):
    for s in range(0, len(bits), mo.CHUNK):
        part = bits[s:s + mo.CHUNK]
        yield convert(part) if convert else part


def as_f64(bits32):
    return bits32.view(np.float32).astype(np.float64)


# ---- exhaustive over the domains the kernels use ---------------------------------------------------------------------------------
LAB_DOMAIN = (0.008856, 1.25)         # lab_f's cube-root arm on X / Xn, Y, Z / Zn of colours in [0, 255]
COMPRESS_DOMAIN = (0.0031308, 1.0)    # srgb_compress's power arm
EXPAND_DOMAIN = (0.09, 1.0)           # pow24_spec's argument (c + 0.055) / 1.055 for c in (0.04045, 1]


def pow24_domain():
    return np.concatenate([np.float32([EXPAND_DOMAIN[0]]).view(np.uint32), mo.f32_range(*EXPAND_DOMAIN)])


@pytest.mark.parametrize("name", ["cbrtf_spec", "lab_f"])
def test_every_float_of_the_cube_root_domain(name, dev, orc):
    assert check(dev, orc, name, chunks(mo.f32_range(*LAB_DOMAIN))) > 59_000_000


@pytest.mark.parametrize("name", ["pow_inv24_spec", "srgb_compress"])
def test_every_float_of_the_gamma_compression_domain(name, dev, orc):
    assert check(dev, orc, name, chunks(mo.f32_range(*COMPRESS_DOMAIN))) > 70_000_000


def test_every_float_of_the_gamma_expansion_domain(dev, orc):
    assert check(dev, orc, "pow24_spec", chunks(pow24_domain())) > 29_000_000


def test_gamma_table_is_the_device_function(dev, orc, probe):
    """srgb_expand(c / 255) for c = 0 .. 255: the device, the oracle and the table the host builds for rgb8_to_lab hold the same bits"""
    c = np.float32(np.arange(256, dtype=np.float32) / np.float32(255.0))
    lut = np.zeros(256, np.float32)
    probe.ssf_mathprobe_expand_lut(lut.ctypes.data_as(C.c_void_p))
    check(dev, orc, "srgb_expand", c)
    assert np.array_equal(mo.evaluate(dev, "srgb_expand", c).reshape(-1), lut.view(np.uint32))


def test_all_8bit_colours(dev, orc):
    """rgb_to_lab and rgb8_to_lab (through the host-built table) over all 2^24 colours: both are the oracle's rgbToLab"""
    packed = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([packed & 255, (packed >> 8) & 255, packed >> 16], 1).astype(np.float32)
    assert check(dev, orc, "rgb_to_lab", rgb) == 1 << 24
    assert check(dev, orc, "rgb8_to_lab", packed) == 1 << 24
    assert np.array_equal(mo.evaluate(dev, "rgb8_to_lab", packed[::4099]), mo.evaluate(dev, "rgb_to_lab", rgb[::4099]))


def guard_patches():
    """all 2^8 "ring pixel carries my label" patterns x two alphabets of foreign labels (alike / all different) x two centre labels"""
    ox, oy = (-1, 0, 1, 1, 1, 0, -1, -1), (-1, -1, -1, 0, 1, 1, 1, 0)
    out = []
    for centre in (7, 0):
        for alphabet in range(2):
            for pat in range(256):
                img = np.full(9, centre, np.int32)
                for k in range(8):
                    img[(1 + oy[k]) * 3 + (1 + ox[k])] = centre if (pat >> k) & 1 else (100 + k if alphabet else 3)
                out.append(img)
    return np.stack(out)


def test_guard_truth_table(dev, orc):
    x = guard_patches()
    assert check(dev, orc, "guard", x) == 1024
    want = np.load(os.path.join(GOLDEN, "ref_decision_vectors.npz"))["guard_unchangeable"].astype(np.uint32).reshape(2, 256)
    got = mo.evaluate(dev, "guard", x).reshape(2, 2, 256)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)      # the reference's own text, for both centre labels


# ---- every binade: the f32 -> f32 / i32 helpers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fx32r", "fx32_s20", "fx32_s24", "pixel_round", "exp_neg_spec", "lab_f", "srgb_expand", "srgb_compress",
                                  "rng_unit"])
def test_f32_helpers_on_every_binade(name, dev, orc, b32):
    """256 exponents x both signs x (first 4096, last 4096, 4096 random mantissas), every k + 0.5 for |k| <= 2^12, the neighbours of
    +-2^23, +-2^31, +-87, +-0, denormals, +-inf, NaNs with payloads.  lab_f / srgb_expand / srgb_compress are here on purpose: they
    are what guards the specified roots, and a model colour handed to ssf_set_model can be any float."""
    assert check(dev, orc, name, b32) > 6_000_000


@pytest.mark.parametrize("name", ["cbrtf_spec", "pow24_spec", "pow_inv24_spec"])
def test_specified_roots_on_every_positive_binade(name, dev, orc, b32):
    """outside the exhaustive sweeps: every positive float the guards of lab_f / srgb_expand / srgb_compress can let through --
    denormals to +inf (as doubles all of them are normal numbers of moderate exponent, or +inf)"""
    pos = b32[(b32 > 0) & (b32 <= 0x7F800000)]
    assert check(dev, orc, name, pos) > 3_000_000


def test_rgb_to_lab_of_hostile_colours(dev, orc, b32):
    """a model colour is three arbitrary floats (ssf_set_model): each binade value in one channel, ordinary values in the others"""
    v = b32[::3].view(np.float32)
    n = len(v)
    rgb = np.stack([v, np.full(n, 128.0, np.float32), np.roll(v, 1)], 1)
    rgb[1::3] = rgb[1::3][:, [1, 0, 2]]
    check(dev, orc, "rgb_to_lab", np.ascontiguousarray(rgb))
    lab = np.stack([v, np.roll(v, 7), np.full(n, 10.0, np.float32)], 1)
    lab[1::2] = lab[1::2][:, [2, 0, 1]]
    check(dev, orc, "lab_to_rgb", np.ascontiguousarray(lab))


# ---- fx64, per instantiated (scale, limit) pair ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mo.FX64_PAIRS))
def test_fx64_pair(name, dev, orc, b64):
    sb, lb = mo.FX64_PAIRS[name]
    n = check(dev, orc, name, chunks(b64))
    n += check(dev, orc, name, mo.fx64_edges(sb, lb))
    n += check(dev, orc, name, mo.log_uniform_f64(1 << 22, 40 + sb))
    assert n > 54_000_000
    # the plain high-precision reference, through neither library: exact integer arithmetic in Python
    v = mo.fx_exact_subset(name)
    got = mo.evaluate(dev, name, v).view(np.int64).reshape(-1)
    want = mo.fx_exact(v, sb, lb)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: input %s (bits %016x): device %d, exact %d" % (
        name, float(v[bad[0]]).hex(), int(v[bad[:1]].view(np.uint64)[0]), int(got[bad[0]]), int(want[bad[0]]))
    print("%s: %d elements against exact integer arithmetic, 0 differ" % (name, len(v)))


# ---- f64 helpers ------------------------------------------------------------------------------------------------------------------
def moderate(b64):
    """the doubles of the binade set that are normal and away from the ends of the exponent range (2^-959 .. 2^960), both signs"""
    e = (b64 >> np.uint64(52)) & np.uint64(0x7FF)
    return (e >= 64) & (e <= 1983)


def test_div3_exact_is_the_division(dev, orc, b64):
    """against x / 3.0: every binade from 2^-959 to 2^960, both signs, and 2^22 seeded values of the range the cube root's Newton
    step feeds it (2 y + a / y^2)"""
    check(dev, orc, "div3_exact", b64[moderate(b64)])
    check(dev, orc, "div3_exact", np.random.default_rng(51).uniform(0.016, 3.7, 1 << 22))


def test_div3_u64_is_the_division(dev, orc):
    """against b / 3: 2^22 seeded patterns + the patterns whose low or high word is 0, 1, 2, 3, 2^32 - 1 or 2^32 - 2 (the other word:
    each of those six and 2^16 seeded words)"""
    rng = np.random.default_rng(52)
    edge = np.uint64([0, 1, 2, 3, 0xFFFFFFFF, 0xFFFFFFFE])
    other = np.concatenate([edge, rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)])
    lo_edge = (other[:, None] << np.uint64(32)) | edge[None, :]
    hi_edge = (edge[:, None] << np.uint64(32)) | other[None, :]
    x = np.concatenate([rng.integers(0, 1 << 64, 1 << 22, dtype=np.uint64), lo_edge.reshape(-1), hi_edge.reshape(-1)])
    check(dev, orc, "div3_u64", x)
    got = mo.evaluate(dev, "div3_u64", x).view(np.uint64).reshape(-1)
    assert np.array_equal(got, x // np.uint64(3))                  # and against numpy's integer division, through neither library


def test_div_inrange_is_the_division(dev, orc):
    """against n / d on 2^24 seeded pairs of the stated ranges, [0.008, 1.2] / [0.04, 1.2] -- and on 2^17 pairs of those ranges whose
    quotient lies 2^-54 of a unit in the last place beside a rounding boundary (mathops.div_hard_cases): the reciprocal's
    Newton steps matter only there, seeded pairs are served by a much worse reciprocal"""
    rng = np.random.default_rng(53)
    x = np.stack([rng.uniform(0.008, 1.2, 1 << 24), rng.uniform(0.04, 1.2, 1 << 24)], 1)
    assert check(dev, orc, "div_inrange", x) == 1 << 24
    hard = mo.div_hard_cases(1 << 17, 55)
    assert (hard[:, 0] >= 0.008).all() and (hard[:, 0] <= 1.2).all() and (hard[:, 1] >= 0.04).all() and (hard[:, 1] <= 1.2).all()
    assert check(dev, orc, "div_inrange", hard) == 1 << 17


ROOT_FEEDS = {"cbrt_spec-lab": ("cbrt_spec", lambda: mo.f32_range(*LAB_DOMAIN), as_f64),
              "cbrt_spec-compress": ("cbrt_spec", lambda: mo.f32_range(*COMPRESS_DOMAIN), lambda b: np.sqrt(np.sqrt(as_f64(b)))),
              "root5_spec-expand": ("root5_spec", pow24_domain, as_f64)}


@pytest.mark.parametrize("feed", sorted(ROOT_FEEDS))
def test_roots_on_the_doubles_the_sweeps_feed_them(feed, dev, orc):
    """cbrt_spec on (double)x over lab_f's domain and on sqrt(sqrt((double)x)) over srgb_compress's; root5_spec on (double)x over
    pow24_spec's: the f64 results themselves, before the rounding to f32 could hide a last-bit difference"""
    name, domain, widen = ROOT_FEEDS[feed]
    assert check(dev, orc, name, chunks(domain(), widen)) > 29_000_000


def test_small_helpers(dev, orc):
    """rng_draw, len3 / unit3 on seeded elements (unit3's reciprocal square root is the correctly rounded 1 / sqrt on both sides)"""
    rng = np.random.default_rng(54)
    check(dev, orc, "rng_draw", rng.integers(0, 1 << 32, (1 << 20, 4), dtype=np.uint32))
    v = np.float32(rng.standard_normal((1 << 20, 3)) * np.exp(rng.uniform(-30, 30, (1 << 20, 1))))
    v[:8] = np.float32([[0, 0, 0], [1e-30, 0, 0], [3e38, 3e38, 0], [np.inf, 1, 1], [np.nan, 1, 1], [-0.0, 0, 0], [1e-45, 1e-45, 0], [1, 0, 0]])
    check(dev, orc, "len3", v)
    check(dev, orc, "unit3", v)


# ---- the golden vectors on the device --------------------------------------------------------------------------------------------
def test_reference_math_vectors_on_the_device(dev, orc):
    """the cases of tests/golden/ref_math_vectors.npz (the reference's own headers) through the device evaluator, as a third party
    beside the oracle and the host product of tests/test_math.py: equal to the oracle everywhere, and equal to the reference's
    outputs where the helper is pure + - * / (bit for bit)"""
    g = np.load(os.path.join(GOLDEN, "ref_math_vectors.npz"))
    f = lambda k, w: np.ascontiguousarray(g[k].reshape(-1, w).astype(np.float32))
    cov, vec, rot = f("cov", 6), f("vec", 3), f("rot", 9)
    A, B, v2, qn = f("matA", 9), f("matB", 9), f("vec2", 3), f("quat", 4)
    cases = [("sym_inverse", cov, None), ("sym_square", cov, f("cov_square", 6)), ("sym_mul", np.hstack([cov, vec]), f("cov_times_vec", 3)),
             ("rot_sym", np.hstack([rot, cov]), f("mult_ABAt", 6)), ("m3_mul", np.hstack([A, B]), f("matA_times_matB", 9)),
             ("m3_mulv", np.hstack([A, v2]), f("matA_times_vec", 3)), ("row_mul", np.hstack([v2, A]), f("vec_times_matA", 3)),
             ("rot_to_quat", A, f("rotMatToQuat_of_matA", 4)), ("quat_to_rot_quirk", qn, f("quatToRotMat", 9)),
             ("rgb_to_lab", f("rgb", 3), None), ("lab_to_rgb", f("rgb_to_lab", 3), None), ("lab_to_rgb", f("lab_free", 3), None)]
    for name, x, ref in cases:
        check(dev, orc, name, x)
        if ref is not None:
            mo.assert_same(name, x, mo.evaluate(dev, name, x), ref.view(np.uint32), ("device", "reference headers"))
    got = mo.evaluate(dev, "sym_inverse", cov)
    ok = g["cov_inverse_ok"].astype(np.uint32)
    assert np.array_equal(got[:, 0], ok)
    bad = mo.differing("sym_square", got[ok == 1][:, 1:], f("cov_inverse", 6)[ok == 1].view(np.uint32))        # (six f32 words, like sym_square's)
    assert bad.size == 0, ("sym_inverse against the reference headers", mo.hexwords(cov[ok == 1][bad[0]].view(np.uint32)))


def test_reference_decision_vectors_on_the_device(dev, orc):
    """tests/golden/ref_decision_vectors.npz (the reference's own text of solvePlaneEquations and eigenDecomposition; the guard's
    table is test_guard_truth_table): accept / reject and coefficients, axes and eigenvalue quotients, 0 bits"""
    g = np.load(os.path.join(GOLDEN, "ref_decision_vectors.npz"))
    rows = np.ascontiguousarray(g["plane_rows"].reshape(-1, 12).astype(np.float32))
    ok, th = g["plane_ok"].astype(np.uint32), g["plane_theta"].reshape(-1, 3).astype(np.float32)
    check(dev, orc, "plane_solve", rows)
    got = mo.evaluate(dev, "plane_solve", rows)
    assert np.array_equal(got[:, 0], ok)
    bad = mo.differing("unit3", got[ok == 1][:, 1:], np.ascontiguousarray(th[ok == 1]).view(np.uint32))          # (three f32 words, like unit3's)
    assert bad.size == 0, ("plane_solve against the reference text", mo.hexwords(rows[ok == 1][bad[0]].view(np.uint32)))
    cov = np.ascontiguousarray(g["eig_cov"].reshape(-1, 6).astype(np.float32))
    want = np.hstack([g["eig_vecs"].reshape(-1, 9), g["eig_vals"].reshape(-1, 3)]).astype(np.float32)
    check(dev, orc, "principal_frame", cov)
    mo.assert_same("principal_frame", cov, mo.evaluate(dev, "principal_frame", cov), np.ascontiguousarray(want).view(np.uint32), ("device", "reference text"))


def test_random_matrices_and_plane_rows_on_the_device(dev, orc):
    """the seeded colours, covariances and plane rows of test_math.py::test_kernel_arithmetic_bitwise_oracle_vs_product (same
    generator, same order of draws), on the device"""
    rng = np.random.default_rng(11)
    rgb, lab, cov, rows = [], [], [], []
    for i in range(400):
        rgb.append(rng.uniform(-5, 260, 3)); lab.append(rng.uniform([0, -120, -120], [100, 120, 120]))
        M = rng.standard_normal((3, 3)) * rng.uniform(1e-3, 1.0)
        Cm = M @ M.T + np.eye(3) * 1e-7
        cov.append([Cm[0, 0], Cm[0, 1], Cm[0, 2], Cm[1, 1], Cm[1, 2], Cm[2, 2]]); rows.append(rng.uniform(-50, 50, 12))
    check(dev, orc, "rgb_to_lab", np.float32(rgb)); check(dev, orc, "lab_to_rgb", np.float32(lab))
    check(dev, orc, "sym_inverse", np.float32(cov)); check(dev, orc, "principal_frame", np.float32(cov))
    check(dev, orc, "plane_solve", np.float32(rows))


# ---- outside the stated domains: compared too, reported separately ----------------------------------------------------------------
def outside_cases(b32, b64):
    """div3_exact / div_inrange / cbrt_spec and the bare roots on operands NO CALLER CAN HAND THEM (module docstring): zero,
    negative, denormal, huge, infinite and NaN"""
    special = np.float64([0.0, 5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, 1e-300, 2.0 ** -1000, 0.008, 1.0, 1.2, 3.0,
                          2.0 ** 1000, 1e300, 8.98846567431158e307, 1.7976931348623157e308, np.inf, np.nan])
    special = np.concatenate([special, -special])
    nn, dd = np.meshgrid(special, special, indexing="ij")
    wild = b64[::97].view(np.float64)
    nonpos32 = b32[~((b32 > 0) & (b32 <= 0x7F800000))]
    return [("div3_exact", b64[~moderate(b64)]), ("div_inrange", np.stack([nn.reshape(-1), dd.reshape(-1)], 1)),
            ("div_inrange", np.stack([wild, np.roll(wild, 12289)], 1)), ("cbrt_spec", b64[::5]), ("root5_spec", b64[::5]),
            ("cbrtf_spec", nonpos32), ("pow24_spec", nonpos32), ("pow_inv24_spec", nonpos32)]


def test_outside_the_stated_domains(dev, orc, b32, b64):
    """What the device branches do where their proofs do not reach.  No kernel can hand them these operands -- the guards asserted
    below are the only way in -- so a difference here is no product bug; it is counted, printed and pinned, so that a change of the
    device code that moves these bits is seen."""
    # the callers' guards: at and below the threshold the roots are not called (the linear arm's bits come out), just above they are
    for name, thr in (("lab_f", 0.008856), ("srgb_compress", 0.0031308), ("srgb_expand", 0.04045)):
        t = np.float32(thr).view(np.uint32)
        x = np.uint32([t - 1, t, t + 1, 0, 0x80000000, 0xBF800000, 0xFF800000, 0x7FC00000, 0xFFC00001])
        got = mo.evaluate(dev, name, x).reshape(-1).view(np.float32)
        xf = x.view(np.float32)
        linear = {"lab_f": np.float32(7.787) * xf + np.float32(16.0) / np.float32(116.0), "srgb_compress": np.float32(12.92) * xf,
                  "srgb_expand": xf / np.float32(12.92)}[name]
        not_above = ~(xf > np.float32(thr))
        assert not_above.sum() == 8
        assert np.array_equal(got[not_above].view(np.uint32)[:6], linear[not_above].view(np.uint32)[:6]) and np.isnan(got[not_above][6:]).all()
    report = {}
    for name, x in outside_cases(b32, b64):
        d, o = mo.evaluate(dev, name, x), mo.evaluate(orc, name, x)
        bad = mo.differing(name, d, o)
        report.setdefault(name, [0, 0, None])
        report[name][0] += d.shape[0]; report[name][1] += bad.size
        if bad.size and report[name][2] is None:
            iw = mo.OPS[name][1]
            inp = np.ascontiguousarray(x).view(np.uint32).reshape(-1, iw)[bad[0]]
            report[name][2] = "input [%s] (%s): device [%s], oracle [%s]" % (mo.hexwords(inp), mo.describe(name, inp), mo.hexwords(d[bad[0]]), mo.hexwords(o[bad[0]]))
    for name, (n, nbad, first) in report.items():
        print("outside the domain, %s: %d elements compared, %d differ%s" % (name, n, nbad, "; first " + first if first else ""))
    assert {k: v[1] for k, v in report.items()} == OUTSIDE_DIFFERENCES, report


# the pinned counts of differing elements outside the stated domains (device vs the plain operation), per operation
# (measured on an MI355X.  div3_exact: -0 -> +0 and the two smallest denormals; div_inrange: zero, denormal, huge, infinite operands,
# where the hardware division scales and fixes up; cbrt_spec: denormal and negative operands; cbrtf_spec: every negative float -- NaN
# where the plain sequence overflows to inf)
OUTSIDE_DIFFERENCES = {"div3_exact": 3, "div_inrange": 415, "cbrt_spec": 3774293, "root5_spec": 0, "cbrtf_spec": 3137545, "pow24_spec": 0,
                       "pow_inv24_spec": 0}
