"""Per-element arithmetic: the reference's own math headers as the known answers, and bitwise
oracle-vs-product agreement of the host-evaluated kernel arithmetic (CPU, no GPU needed).

Known answers (fixture G1): tests/golden/ref_math_vectors.npz holds the outputs of the
reference's vector_math.cuh / matrix_math.cuh on seeded inputs (oracle/ref_math_vectors.cpp, compiled in the build
container against the reference's headers where they lie and NVIDIA's CUDA runtime headers from the image).
  * pure +,-,*,/ helpers (inverse, square, Cov3*v, mult_ABAt, Mat33 products, rotMatToQuat, quatToRotMat with its
    wy = q.w*q.z) must agree BIT FOR BIT: same operations in the same order;
  * rgbToLab / labToRgb use libm powf / cbrtf in the reference (CUDA's device versions on the GPU); this build
    replaces them by a specified IEEE sequence so that host and device agree, and is compared to 2e-4 (Lab units /
    8-bit colour units for rgbToLab, 2e-3 of a grey level for labToRgb) -- the tolerance is the transcendental-function
    difference, stated here."""
import ctypes as C

import numpy as np
import pytest


def fptr(a):
    return a.ctypes.data_as(C.c_void_p)


def call3(L, fn, x, nout=3):
    x = np.ascontiguousarray(x, np.float32); o = np.zeros(nout, np.float32)
    getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p]
    getattr(L, fn)(fptr(x), fptr(o))
    return o


import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_math_vectors.npz")
LAB_TOL = 2e-4      # Lab units; observed worst 6.1e-5
RGB_TOL = 2e-3      # 8-bit colour units; observed worst 7.8e-4 (the sRGB curve has slope 12.92 * 255 near black,
                    # which multiplies the one-ulp difference between powf(x, 3.0f) and (x * x) * x)


def call(L, fn, *xs, nout=3):
    xs = [np.ascontiguousarray(x, np.float32) for x in xs]
    o = np.zeros(nout, np.float32)
    getattr(L, fn).argtypes = [C.c_void_p] * (len(xs) + 1)
    rc = getattr(L, fn)(*[fptr(x) for x in xs], fptr(o))
    return o, rc


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("which", ["oracle", "product"])
def test_lab_against_the_reference_headers(which, oracle_lib, product_lib):
    """4096 colours through the reference's rgbToLab and back (vector_math.cuh:543-585) + 1024 free Lab values."""
    L = (oracle_lib if which == "oracle" else product_lib).lib
    g = np.load(GOLD)
    rgb, lab, back = g["rgb"].reshape(-1, 3), g["rgb_to_lab"].reshape(-1, 3), g["lab_to_rgb_of_that"].reshape(-1, 3)
    worst = 0.0
    for i in range(len(rgb)):
        mine = call3(L, "ssf_dbg_rgb_to_lab", rgb[i])
        worst = max(worst, float(np.abs(mine - lab[i]).max()))
        assert np.allclose(mine, lab[i], atol=LAB_TOL), (i, rgb[i], mine, lab[i])
        assert np.allclose(call3(L, "ssf_dbg_lab_to_rgb", lab[i]), back[i], atol=RGB_TOL)
    lf, rf = g["lab_free"].reshape(-1, 3), g["lab_to_rgb_free"].reshape(-1, 3)
    for i in range(len(lf)):
        assert np.allclose(call3(L, "ssf_dbg_lab_to_rgb", lf[i]), rf[i], atol=RGB_TOL), (i, lf[i])
    assert worst < LAB_TOL
    # CIE anchors: white -> L=100, black -> 0
    assert np.allclose(call3(L, "ssf_dbg_rgb_to_lab", [255, 255, 255]), [100, 0, 0], atol=2e-2)
    assert np.allclose(call3(L, "ssf_dbg_rgb_to_lab", [0, 0, 0]), [0, 0, 0], atol=1e-5)


@pytest.mark.parametrize("which", ["oracle", "product"])
def test_matrix_helpers_bit_exact_against_the_reference_headers(which, oracle_lib, product_lib):
    """inverse / square / Cov3*v / mult_ABAt on 1024 SPD + 64 near-singular matrices, Mat33 products, transposed
    products and both quaternion conversions on 1024 rotations: 0 bits of difference to the reference's headers."""
    L = (oracle_lib if which == "oracle" else product_lib).lib
    g = np.load(GOLD)
    cov, inv, ok = g["cov"].reshape(-1, 6), g["cov_inverse"].reshape(-1, 6), g["cov_inverse_ok"]
    sq, vec, cv = g["cov_square"].reshape(-1, 6), g["vec"].reshape(-1, 3), g["cov_times_vec"].reshape(-1, 3)
    rot, aba = g["rot"].reshape(-1, 9), g["mult_ABAt"].reshape(-1, 6)
    assert 100 < ok.sum() < len(ok) - 100            # both sides of the |det| > 1e-9 gate are exercised
    for i in range(len(cov)):
        o, rc = call(L, "ssf_dbg_sym_inverse", cov[i], nout=6)
        assert rc == int(ok[i]), (i, cov[i])
        if rc:
            assert same_bits(o, inv[i]), (i, o, inv[i])
        assert same_bits(call(L, "ssf_dbg_sym_square", cov[i], nout=6)[0], sq[i]), i
        assert same_bits(call(L, "ssf_dbg_sym_mulv", cov[i], vec[i])[0], cv[i]), i
        assert same_bits(call(L, "ssf_dbg_mult_abat", rot[i], cov[i], nout=6)[0], aba[i]), i
    A, B, AB = g["matA"].reshape(-1, 9), g["matB"].reshape(-1, 9), g["matA_times_matB"].reshape(-1, 9)
    v2, Av, vA = g["vec2"].reshape(-1, 3), g["matA_times_vec"].reshape(-1, 3), g["vec_times_matA"].reshape(-1, 3)
    q, qn, q2r = g["rotMatToQuat_of_matA"].reshape(-1, 4), g["quat"].reshape(-1, 4), g["quatToRotMat"].reshape(-1, 9)
    branches = set()
    for i in range(len(A)):
        assert same_bits(call(L, "ssf_dbg_m3_mul", A[i], B[i], nout=9)[0], AB[i]), i
        assert same_bits(call(L, "ssf_dbg_m3_mulv", A[i], v2[i])[0], Av[i]), i
        assert same_bits(call(L, "ssf_dbg_row_mul", v2[i], A[i])[0], vA[i]), i
        assert same_bits(call(L, "ssf_dbg_rot_to_quat", A[i], nout=4)[0], q[i]), (i, A[i])
        assert same_bits(call(L, "ssf_dbg_quat_to_rot", qn[i], nout=9)[0], q2r[i]), i
        tr = A[i][0] + A[i][4] + A[i][8]
        branches.add("tr" if tr > 0 else int(np.argmax(np.abs(q[i][:3]))))
    assert branches == {"tr", 0, 1, 2}, branches     # every branch of rotMatToQuat (matrix_math.cuh:529-618)
    # the reference's quatToRotMat quirk is in the vectors: a proper rotation would have R[0,2] = 2(xz + wy)
    x, y, z, w = qn[:, 0], qn[:, 1], qn[:, 2], qn[:, 3]
    assert np.abs(q2r[:, 2] - 2 * (x * z + w * y)).max() > 1e-2 and np.abs(q2r[:, 2] - 2 * (x * z + w * z)).max() < 1e-5


def test_lab_matches_double_precision_formula(oracle_lib):
    """The specified Newton roots agree with an fp64 evaluation of the same colour formulas."""
    rng = np.random.default_rng(7)
    for c in rng.uniform(0, 255, (200, 3)):
        lab = call3(oracle_lib.lib, "ssf_dbg_rgb_to_lab", c)
        v = np.float32(c).astype(np.float64) / 255.0
        lin = np.where(v > 0.04045, ((v + 0.055) / 1.055) ** 2.4, v / 12.92)
        x = (lin @ [0.4124, 0.3575, 0.1805]) / 0.95047; y = lin @ [0.2126, 0.7152, 0.0722]
        z = (lin @ [0.0193, 0.1192, 0.9505]) / 1.08883
        f = lambda t: np.cbrt(t) if t > 0.008856 else 7.787 * t + 16.0 / 116.0
        ref = [116 * f(y) - 16, 500 * (f(x) - f(y)), 200 * (f(y) - f(z))]
        assert np.allclose(lab, ref, atol=2e-4)


def test_kernel_arithmetic_bitwise_oracle_vs_product(oracle_lib, product_lib):
    rng = np.random.default_rng(11)
    Lo, Lp = oracle_lib.lib, product_lib.lib
    for i in range(400):
        rgb = rng.uniform(-5, 260, 3)
        a, b = call3(Lo, "ssf_dbg_rgb_to_lab", rgb), call3(Lp, "ssf_dbg_rgb_to_lab", rgb)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) or (np.isnan(a).any() and np.isnan(b).any())
        lab = rng.uniform([0, -120, -120], [100, 120, 120])
        a, b = call3(Lo, "ssf_dbg_lab_to_rgb", lab), call3(Lp, "ssf_dbg_lab_to_rgb", lab)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        M = rng.standard_normal((3, 3)) * rng.uniform(1e-3, 1.0)
        Cm = M @ M.T + np.eye(3) * 1e-7
        cov = np.float32([Cm[0, 0], Cm[0, 1], Cm[0, 2], Cm[1, 1], Cm[1, 2], Cm[2, 2]])
        a, b = call3(Lo, "ssf_dbg_sym_inverse", cov, 6), call3(Lp, "ssf_dbg_sym_inverse", cov, 6)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for L, store in ((Lo, []), (Lp, [])):
            pass
        vo, wo, vp, wp = np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(9, np.float32), np.zeros(3, np.float32)
        for L, v, w in ((Lo, vo, wo), (Lp, vp, wp)):
            L.ssf_dbg_principal_frame.argtypes = [C.c_void_p] * 3
            L.ssf_dbg_principal_frame(fptr(cov), fptr(v), fptr(w))
        assert np.array_equal(vo.view(np.uint32), vp.view(np.uint32)) and np.array_equal(wo.view(np.uint32), wp.view(np.uint32))
        rows = np.float32(rng.uniform(-50, 50, 12))
        a, b = call3(Lo, "ssf_dbg_plane_solve", rows), call3(Lp, "ssf_dbg_plane_solve", rows)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_lab_of_8bit_colours_bitwise_oracle_vs_product(oracle_lib, product_lib):
    """rgbToLab for the colours k_render_moments meets -- 8-bit channels: every grey, a 16^3 lattice, 20 000 random ones.
    The product's specified cube root divides by three with a multiply and two fused operations (div3_exact) and takes the
    start value's 64-bit pattern apart in 32-bit pieces (div3_u64); the oracle divides.  Same bits, colour by colour."""
    rng = np.random.default_rng(2024)
    cols = [np.float64([g, g, g]) for g in range(256)]
    lat = np.arange(0, 256, 17, dtype=np.float64)
    cols += [np.float64([r, g, b]) for r in lat for g in lat for b in lat]
    cols += list(rng.integers(0, 256, (20000, 3)).astype(np.float64))
    Lo, Lp = oracle_lib.lib, product_lib.lib
    for c in cols:
        a, b = call3(Lo, "ssf_dbg_rgb_to_lab", c), call3(Lp, "ssf_dbg_rgb_to_lab", c)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (c, a, b)


def test_principal_frame_recovers_known_axes(oracle_lib):
    """eigenDecomposition by repeated squaring: major axis, normal and eigenvalues of a known
    covariance (rows = major, normal x major, normal; supersurfel_fusion_kernels.cu:48-111)."""
    R = np.array([[0.6, 0.8, 0.0], [-0.8, 0.6, 0.0], [0.0, 0.0, 1.0]])   # rows are the axes
    lam = np.array([4e-4, 1e-4, 4e-6])
    Cm = R.T @ np.diag(lam) @ R
    cov = np.float32([Cm[0, 0], Cm[0, 1], Cm[0, 2], Cm[1, 1], Cm[1, 2], Cm[2, 2]])
    v, w = np.zeros(9, np.float32), np.zeros(3, np.float32)
    oracle_lib.lib.ssf_dbg_principal_frame.argtypes = [C.c_void_p] * 3
    oracle_lib.lib.ssf_dbg_principal_frame(fptr(cov), fptr(v), fptr(w))
    v = v.reshape(3, 3)
    assert abs(abs(v[0] @ R[0]) - 1) < 1e-4 and abs(abs(v[2] @ R[2]) - 1) < 1e-4
    assert np.allclose(w, lam, rtol=2e-3)


def test_sym_inverse_threshold(oracle_lib):
    """|det| > 1e-9 gate of inverse(Cov3) (matrix_math.cuh:51): near-singular input is rejected."""
    L = oracle_lib.lib
    L.ssf_dbg_sym_inverse.argtypes = [C.c_void_p, C.c_void_p]
    ok = np.float32([1e-2, 0, 0, 1e-2, 0, 1e-2]); bad = np.float32([1e-4, 0, 0, 1e-4, 0, 1e-4]); o = np.zeros(6, np.float32)
    assert L.ssf_dbg_sym_inverse(fptr(ok), fptr(o)) == 1 and np.allclose(o[[0, 3, 5]], 100.0, rtol=1e-6)
    assert L.ssf_dbg_sym_inverse(fptr(bad), fptr(o)) == 0


# ---- the three DECISION helpers against the reference's own text -------------------------------------------------------------
# tests/golden/ref_decision_vectors.npz = outputs of isUnchangeable (TPS_RGBD_kernels.cuh:178-233), solvePlaneEquations
# (TPS_RGBD_kernels.cu:27-59) and eigenDecomposition (supersurfel_fusion_kernels.cu:48-111), cut out of the reference's files by
# line range at build time and compiled as they stand (oracle/ref_decision_vectors.cpp, oracle/Makefile `decision`).  They gate
# integer results (may a pixel change its label; which RANSAC sample / plane a superpixel gets; which axis is the normal).
# Round 6: TWO generator binaries -- guard_* and plane_* come from one that only DECLARES rsqrtf (no stand-in anywhere in it, the
# recipe checks with nm); eig_* alone comes from the binary that defines rsqrtf := 1 / sqrtf (the one named stand-in).
DECISIONS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_decision_vectors.npz")


@pytest.mark.parametrize("which", ["oracle", "product"])
def test_connectivity_guard_is_the_references_on_every_ring_pattern(which, oracle_lib, product_lib):
    """all 2^8 "neighbour carries my label" patterns x two label alphabets (foreign pixels alike / all different): the guard
    only compares for equality, so this is its whole truth table -- the oracle's ring walk and the product's bit mask +
    population count (csrc/ssf_math.hpp guard_ring / guard_unchangeable, what k_update_pass executes) must both be it"""
    L = (oracle_lib if which == "oracle" else product_lib).lib
    L.ssf_dbg_connectivity_guard.argtypes = [C.c_void_p]
    want = np.load(DECISIONS)["guard_unchangeable"].astype(np.int32).reshape(2, 256)
    ox, oy = (-1, 0, 1, 1, 1, 0, -1, -1), (-1, -1, -1, 0, 1, 1, 1, 0)
    n_bridge = 0
    for alphabet in range(2):
        for pat in range(256):
            img = np.full(9, 7, np.int32)
            for k in range(8):
                img[(1 + oy[k]) * 3 + (1 + ox[k])] = 7 if (pat >> k) & 1 else (100 + k if alphabet else 3)
            got = L.ssf_dbg_connectivity_guard(fptr(img))
            assert got == want[alphabet, pat], (alphabet, pat, got)
            n_bridge += got
    assert (want[0] == want[1]).all() and 0 < n_bridge < 512       # equality only; both outcomes occur (372 bridges of 512)


@pytest.mark.parametrize("which", ["oracle", "product"])
def test_plane_solve_bit_exact_against_the_references_text(which, oracle_lib, product_lib):
    """4096 triples as the extract stage forms them (pixel rows of a RANSAC sample; rows of a superpixel's normal equations) +
    degenerate and non-finite ones: accept / reject and, when accepted, the three plane coefficients bit for bit -- including
    the guard `!isfinite(den) && den < eps` that only ever rejects -inf (kept as the reference wrote it)"""
    L = (oracle_lib if which == "oracle" else product_lib).lib
    g = np.load(DECISIONS)
    rows, ok, th = g["plane_rows"].reshape(-1, 12), g["plane_ok"].astype(np.int32), g["plane_theta"].reshape(-1, 3)
    assert len(rows) == 4160 and 0 < (ok == 0).sum() < 64
    for i in range(len(rows)):
        o, rc = call(L, "ssf_dbg_plane_solve", rows[i])
        assert rc == ok[i], (i, rows[i])
        if rc:
            assert same_bits(o, th[i]), (i, rows[i], o, th[i])
    nonfinite = ~np.isfinite(th).all(axis=1) & (ok == 1)
    assert nonfinite.sum() > 10                      # accepted solves with inf / NaN coefficients exist and are compared too


@pytest.mark.parametrize("which", ["oracle", "product"])
def test_principal_frame_bit_exact_against_the_references_text(which, oracle_lib, product_lib):
    """eigenDecomposition on 1024 SPD matrices at supersurfel scales (thin discs; axis-aligned and round ones for the ties of
    the column choice): the three axes and the three eigenvalue quotients, 0 bits of difference.
    What this does NOT pin: the generator defines the CUDA intrinsic rsqrtf (used by the reference's normalize,
    vector_math.cuh:247-252) as the correctly rounded 1.0f / sqrtf(x) -- this build's specification for oracle and product alike;
    on a CUDA device rsqrtf may differ by <= 2 ulp, i.e. every axis component by a relative 2^-22 (and the eigenvalue quotients
    by as much: they are ratios of expressions linear in the axis).  The column choice, the ten normalised squarings and the
    branch selection of the quotients involve no stand-in."""
    L = (oracle_lib if which == "oracle" else product_lib).lib
    g = np.load(DECISIONS)
    cov, vecs, vals = g["eig_cov"].reshape(-1, 6), g["eig_vecs"].reshape(-1, 9), g["eig_vals"].reshape(-1, 3)
    L.ssf_dbg_principal_frame.argtypes = [C.c_void_p] * 3
    for i in range(len(cov)):
        v, w = np.zeros(9, np.float32), np.zeros(3, np.float32)
        L.ssf_dbg_principal_frame(fptr(np.ascontiguousarray(cov[i])), fptr(v), fptr(w))
        assert same_bits(v, vecs[i]), (i, cov[i], v, vecs[i])
        assert same_bits(w, vals[i]), (i, cov[i], w, vals[i])
    # the vectors mean something: unit axes, rows[1] = rows[2] x rows[0], eigenvalues ordered major >= minor >= normal on the generic cases
    V = vecs.reshape(-1, 3, 3)
    generic = np.arange(len(V)) % 128 > 1
    assert np.abs(np.linalg.norm(V[generic][:, 0], axis=1) - 1).max() < 1e-5 and np.abs(np.linalg.norm(V[generic][:, 2], axis=1) - 1).max() < 1e-5
    assert (vals[generic][:, 0] >= vals[generic][:, 2]).all()


# ---- the element-wise batch evaluators (csrc/probe/ssf_math_ops.h) ----------------------------------------------------------------
# tests/test_math_device_gpu.py runs ssf_math.hpp on the DEVICE, element by element, against the oracle's batch entry
# (oracle/oracle_mathbatch.cpp).  What can be checked without a GPU is checked here: the batch entry is the oracle's per-element
# hooks, its fixed point is exact integer arithmetic, the probe library is built like the product and lists every operation, its
# HOST branches equal the oracle too, and the product library gained nothing.
import mathops as mo


@pytest.fixture(scope="module")
def orc_batch(oracle_lib):
    fn = oracle_lib.lib.ssf_oracle_mathbatch
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]; fn.restype = C.c_int
    return fn


@pytest.fixture(scope="module")
def probe_lib():
    return mo.load_probe()


def _hook_inputs(rng, n):
    """n seeded elements per operation that has an ssf_dbg_* hook: {name: (float32 / int32 array (n, in_words))}"""
    M = rng.standard_normal((n, 3, 3)) * rng.uniform(1e-3, 1.0, (n, 1, 1))
    Cm = M @ M.transpose(0, 2, 1) + np.eye(3) * 1e-7
    cov = np.float32(np.stack([Cm[:, 0, 0], Cm[:, 0, 1], Cm[:, 0, 2], Cm[:, 1, 1], Cm[:, 1, 2], Cm[:, 2, 2]], 1))
    cov[::7] *= np.float32(1e-3)                       # (both sides of sym_inverse's |det| > 1e-9 gate)
    q = rng.standard_normal((n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.float32(np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                             2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1))
    A = np.float32(rng.uniform(-2, 2, (n, 9))); v = np.float32(rng.uniform(-3, 3, (n, 3)))
    labels = rng.integers(0, 3, (n, 9)).astype(np.int32)
    return {
        "rgb_to_lab": np.float32(rng.uniform(-5, 260, (n, 3))), "lab_to_rgb": np.float32(rng.uniform([0, -120, -120], [100, 120, 120], (n, 3))),
        "sym_inverse": cov, "principal_frame": cov, "plane_solve": np.float32(rng.uniform(-50, 50, (n, 12))), "guard": labels,
        "sym_square": cov, "sym_mul": np.hstack([cov, v]), "rot_sym": np.hstack([R, cov]), "m3_mul": np.hstack([R, A]),
        "m3_mulv": np.hstack([A, v]), "row_mul": np.hstack([v, A]), "rot_to_quat": R, "quat_to_rot_quirk": np.float32(q),
    }


def _hook_result(L, name, row):
    """one element through the library's per-element ssf_dbg_* hook, in the batch entry's output layout (uint32 words)"""
    f32 = lambda k: np.zeros(k, np.float32)
    def run(fn, *args):
        getattr(L, fn).argtypes = [C.c_void_p] * len(args); getattr(L, fn).restype = C.c_int
        return getattr(L, fn)(*[fptr(a) for a in args])
    r = np.ascontiguousarray(row)
    if name in ("rgb_to_lab", "lab_to_rgb", "sym_square", "rot_to_quat"):
        o = f32({"sym_square": 6, "rot_to_quat": 4}.get(name, 3)); run("ssf_dbg_" + name, r, o); return o.view(np.uint32)
    if name == "quat_to_rot_quirk":
        o = f32(9); run("ssf_dbg_quat_to_rot", r, o); return o.view(np.uint32)
    if name in ("sym_inverse", "plane_solve"):
        o = f32(6 if name == "sym_inverse" else 3); rc = run("ssf_dbg_" + name, r, o); return np.concatenate([np.uint32([rc]), o.view(np.uint32)])
    if name == "principal_frame":
        v, w = f32(9), f32(3); run("ssf_dbg_principal_frame", r, v, w); return np.concatenate([v, w]).view(np.uint32)
    if name == "guard":
        return np.uint32([run("ssf_dbg_connectivity_guard", r)])
    split, fn, nout = {"sym_mul": (6, "ssf_dbg_sym_mulv", 3), "rot_sym": (9, "ssf_dbg_mult_abat", 6), "m3_mul": (9, "ssf_dbg_m3_mul", 9),
                       "m3_mulv": (9, "ssf_dbg_m3_mulv", 3), "row_mul": (3, "ssf_dbg_row_mul", 3)}[name]
    o = f32(nout); run(fn, np.ascontiguousarray(r[:split]), np.ascontiguousarray(r[split:]), o); return o.view(np.uint32)


def test_oracle_batch_entry_equals_its_per_element_hooks(oracle_lib, orc_batch):
    """2048 seeded elements per operation that include/ssf_testing.h exposes: the batch loop returns what the hook returns, bit for
    bit (no NaN allowance needed: it is the same code in the same library)"""
    ins = _hook_inputs(np.random.default_rng(31), 2048)
    for name, x in ins.items():
        got = mo.evaluate(orc_batch, name, x)
        want = np.stack([_hook_result(oracle_lib.lib, name, row) for row in x])
        assert np.array_equal(got, want), (name, int(np.flatnonzero((got != want).any(axis=1))[0]))
    assert orc_batch(9999, None, None, 0) == -1
    assert oracle_lib.lib.ssf_oracle_mathbatch_num_ops() == len(mo.OPS)


@pytest.mark.parametrize("name", sorted(mo.FX64_PAIRS))
def test_fx_quant_is_exact_integer_rounding(name, orc_batch):
    """the oracle's fx_quant against round_half_even(Fraction(v) * scale) clamped to +-limit in Python integers, on 20 000 values that
    hold every edge of the pair: all k + 0.5 for |k| <= 2^12, the neighbours of +-limit, +-2^50 .. +-2^62 after scaling, +-0, +-inf, NaN"""
    v = mo.fx_exact_subset(name)
    assert len(v) == 20000
    got = mo.evaluate(orc_batch, name, v).view(np.int64).reshape(-1)
    want = mo.fx_exact(v, *mo.FX64_PAIRS[name])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, float(v[bad[0]]).hex(), int(got[bad[0]]), int(want[bad[0]]))


def test_probe_library_is_built_like_the_product_and_lists_every_operation(probe_lib):
    """csrc/Makefile compiles probe/ssf_math_probe.hip with the product's FLAGS, unchanged; the library's table is the shared
    header's list (number, name, element sizes)"""
    import subprocess
    def command(target, touched):
        out = subprocess.run(["make", "-C", mo.CSRC, "-n", "-W", touched, target], stdout=subprocess.PIPE, text=True, check=True).stdout
        line = [l for l in out.splitlines() if "hipcc" in l and touched in l][0].split()
        return [t for t in line if not t.endswith((".hip", ".o", ".so")) and t not in ("-c", "-o", "-shared")]
    assert command("mathprobe", "probe/ssf_math_probe.hip") == command("ssf_testing.o", "ssf_testing.hip")
    assert probe_lib.ssf_mathprobe_num_ops() == len(mo.OPS)
    listed = {}
    for k in range(len(mo.OPS)):
        i, nm, iw, ow = C.c_int(), C.c_char_p(), C.c_int(), C.c_int()
        assert probe_lib.ssf_mathprobe_op_info(k, C.byref(i), C.byref(nm), C.byref(iw), C.byref(ow)) == 0
        listed[nm.value.decode()] = (i.value, iw.value, ow.value)
    assert listed == mo.OPS
    assert sorted(v[0] for v in mo.OPS.values()) == list(range(len(mo.OPS)))
    assert set(mo.FX64_PAIRS) == {n for n in mo.OPS if n.startswith("fx64_")}


def test_probe_host_branches_equal_the_oracle(probe_lib, orc_batch):
    """the probe's operations through the HOST branches of ssf_math.hpp (what the product's ssf_dbg_* hooks evaluate) against the
    oracle's batch entry: every f32 helper on the binade set, fx64 on each pair's edges, the matrix helpers on seeded elements.
    This checks the probe's layouts without a GPU; the device branches are tests/test_math_device_gpu.py's."""
    host = probe_lib.ssf_mathprobe_eval_host
    b32 = mo.f32_binade_set()[::16]
    pos = b32[(b32 >> 31) == 0]
    for name in ("fx32r", "fx32_s20", "fx32_s24", "pixel_round", "exp_neg_spec", "srgb_expand", "srgb_compress", "lab_f", "rng_unit"):
        mo.assert_same(name, b32, mo.evaluate(host, name, b32), mo.evaluate(orc_batch, name, b32), ("product host", "oracle"))
    for name in ("cbrtf_spec", "pow24_spec", "pow_inv24_spec"):
        mo.assert_same(name, pos, mo.evaluate(host, name, pos), mo.evaluate(orc_batch, name, pos), ("product host", "oracle"))
    for name, (sb, lb) in mo.FX64_PAIRS.items():
        v = mo.fx_exact_subset(name)
        mo.assert_same(name, v, mo.evaluate(host, name, v), mo.evaluate(orc_batch, name, v), ("product host", "oracle"))
    rng = np.random.default_rng(32)
    d = rng.uniform(0.008, 1.2, 4096)
    for name, x in (("div3_exact", d), ("cbrt_spec", d), ("root5_spec", d), ("div_inrange", np.stack([d, rng.uniform(0.04, 1.2, 4096)], 1)),
                    ("div3_u64", rng.integers(0, 1 << 63, 4096, dtype=np.uint64)), ("rng_draw", rng.integers(0, 1 << 32, (4096, 4), dtype=np.uint32)),
                    ("rgb8_to_lab", rng.integers(0, 1 << 24, 4096, dtype=np.uint32)), ("len3", np.float32(rng.uniform(-3, 3, (4096, 3)))),
                    ("unit3", np.float32(rng.uniform(-3, 3, (4096, 3))))):
        mo.assert_same(name, x, mo.evaluate(host, name, x), mo.evaluate(orc_batch, name, x), ("product host", "oracle"))
    for name, x in _hook_inputs(np.random.default_rng(33), 1024).items():
        mo.assert_same(name, x, mo.evaluate(host, name, x), mo.evaluate(orc_batch, name, x), ("product host", "oracle"))
    lut = np.zeros(256, np.float32)
    probe_lib.ssf_mathprobe_expand_lut(fptr(lut))
    c = np.float32(np.arange(256, dtype=np.float32) / np.float32(255.0))
    assert np.array_equal(lut.view(np.uint32), mo.evaluate(orc_batch, "srgb_expand", c).reshape(-1))


def test_product_library_exports_what_the_parent_build_exported(product_lib):
    """the arithmetic probe is a library of its own: libssf_hip.so's dynamic symbol table is the list recorded from the build
    before the probe existed (tests/golden/libssf_hip_dynsyms.txt: `nm -D --defined-only | awk '{print $3}' | sort`; a change
    that adds or removes a kernel or an entry point regenerates it) and holds no probe symbol"""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", product_lib.path], stdout=subprocess.PIPE, text=True, check=True).stdout
    have = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3)
    want = open(os.path.join(os.path.dirname(GOLD), "libssf_hip_dynsyms.txt")).read().split()
    assert have == sorted(want), sorted(set(have) ^ set(want))
    assert not [s for s in have if "probe_" in s or "mathprobe" in s]
