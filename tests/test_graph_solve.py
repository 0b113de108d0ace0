"""The numpy restatement of include/ssf_graph_solve.h (tests/graph_solve_ref.py) under test, so that the GPU tests compare against
something proven: its J, J^T and diagonal against finite differences of its own residuals, the identity, a rigid motion, and its
result against an independent Gauss-Newton with a sparse direct solve.  Last, EDGE_CASES: the inputs with which
tests/test_graph_solve_edges_gpu.py drives the device through every inner-loop ending, chunk shape, block boundary and the sort's
third pass; here the restatement alone is shown to reach each of them."""
import functools

import numpy as np
import pytest

import graph_ref as gr
import graph_solve_ref as gs
from supersurfel_fusion_amd import synthetic

f32, f64 = np.float32, np.float64


def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def stamped_rows(n, frames=400, seed=3):
    """rows of the shape of test_graph_gpu.py's stamped_model: seeded room rows, births swept over `frames` stamps by azimuth"""
    m, nvis = synthetic.seed_model_cam0(n, 640, 480, stamp=30, seed=1234 + seed)
    rng = np.random.default_rng(seed)
    pos = np.ascontiguousarray(m["positions"], f32).reshape(n, 3)
    az = np.arctan2(pos[:, 2], pos[:, 0])
    t0 = ((az + np.pi) / (2 * np.pi) * frames + rng.integers(0, max(1, frames // 20), n)).astype(np.int32)
    st = m["stamps"].reshape(n, 2).copy()
    st[:, 0] = t0
    m["stamps"] = st.reshape(m["stamps"].shape)
    return pos, t0, np.asarray(m["confidences"], f32), (m, nvis)


def loop_case(n, stride=50, look=20, n_con=None, deg=3.0, frames=400, seed=3, t_cut=0.7):
    """nodes of a stamped model; the rows born after t_cut * frames are rotated by `deg` about the room's vertical through their
    centroid, the rest is pinned.  n_con random rows (default: two per node) are the constraints, as many others are held out.  `model` is the
    (model, n_visible) pair that Fusion.set_model takes"""
    pos, t0, conf, model = stamped_rows(n, frames, seed)
    rows = gr.sample(pos, t0, conf, stride)
    npos, nt0 = pos[rows].copy(), t0[rows].copy()
    rng = np.random.default_rng(seed + 100)
    n_con = n_con or 2 * len(rows)
    pick = rng.choice(n, 2 * n_con, replace=False)
    con, held = pick[:n_con], pick[n_con:]
    late = t0 >= int(t_cut * frames)
    c = pos[late].mean(axis=0).astype(f64)
    moved = ((pos.astype(f64) - c) @ rot_y(deg).T + c)
    target = np.where(late[:, None], moved, pos.astype(f64)).astype(f32)
    return dict(npos=npos, nt0=nt0, look=look, src=pos[con], t_init=t0[con], dst=target[con], held=pos[held], held_t=t0[held],
                model=model, stride=stride)


# the GPU tests (tests/test_graph_solve_gpu.py) solve these inputs; `test_condition` proves that their last inner loop converges
GPU_CASES = {"n10k": dict(n=10000, stride=50, look=20), "n100k": dict(n=100000, stride=50, look=20)}


# ---- Jacobian -------------------------------------------------------------------------------------------------------------
def test_jacobian_against_finite_differences():
    rng = np.random.default_rng(0)
    m, nc = 9, 7
    npos = rng.uniform(-1, 1, (m, 3)).astype(f32)
    nt0 = np.sort(rng.integers(0, 5, m)).astype(np.int32)
    src = rng.uniform(-1, 1, (nc, 3)).astype(f32)
    P = gs.Problem(npos, nt0, 3, src, rng.integers(0, 5, nc).astype(np.int32), src + f32(0.1), w_rot=1.3, w_reg=7.0, w_con=55.0)
    x = np.zeros((m, 12)); x[:, 0] = x[:, 4] = x[:, 8] = 1.0
    x += rng.uniform(-0.2, 0.2, x.shape)
    flat = lambda r: np.concatenate([a.ravel() for a in r])
    nres, nx, h = len(flat(P.residuals(x))), 12 * m, 1e-6
    Jfd = np.empty((nres, nx))
    for i in range(nx):
        e = np.zeros(nx); e[i] = h
        Jfd[:, i] = (flat(P.residuals(x + e.reshape(m, 12))) - flat(P.residuals(x - e.reshape(m, 12)))) / (2 * h)
    scale = np.abs(Jfd).max()
    # central differences of a quadratic residual are exact up to rounding: 1e-16 / h = 1e-10 relative, a margin of 100
    J = np.stack([flat(P.J(x, np.eye(nx)[i].reshape(m, 12))) for i in range(nx)], 1)
    assert np.abs(J - Jfd).max() <= 1e-8 * scale
    sizes = [6 * m, 12 * m, 3 * nc]
    Jt = np.empty((nx, nres))
    for i in range(nres):
        y = np.zeros(nres); y[i] = 1.0
        parts = np.split(y, np.cumsum(sizes)[:-1])
        Jt[:, i] = P.Jt(x, (parts[0].reshape(m, 6), parts[1].reshape(m, 4, 3), parts[2].reshape(nc, 3))).ravel()
    assert np.abs(Jt - Jfd.T).max() <= 1e-8 * scale
    assert np.abs(P.diag(x).ravel() - (Jfd * Jfd).sum(axis=0)).max() <= 1e-8 * scale * scale
    assert (P.in_off[-1], P.con_off[-1]) == (4 * m, 4 * nc)
    for j in range(m):                                               # edges: four distinct neighbours, never the node itself
        assert j not in P.edges[j] and len(set(P.edges[j])) == 4


# ---- edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("look,dup", [(3, False), (8, False), (20, False), (6, True)])
def test_edges_against_a_naive_search(look, dup):
    """steps 1-4 of the binding and 'the first four that are not j', written node by node with python's own sort"""
    rng = np.random.default_rng(look)
    m = 300
    npos = rng.uniform(-2, 2, (m, 3)).astype(f32)
    if dup:
        npos = npos[rng.integers(0, 12, m)]                          # a dozen positions: ties go to the smaller node index
    nt0 = np.sort(rng.integers(0, 25, m)).astype(np.int32)           # many equal stamps
    got = gs.edges_of(npos, nt0, look)
    for j in range(m):
        c = next((k for k in range(m) if nt0[k] >= nt0[j]), m)
        lo = min(max(c - look, 0), max(0, m - 2 * look))
        cand = []
        for k in range(lo, lo + min(m, 2 * look)):
            d = npos[j] - npos[k]
            d2 = f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])
            cand.append((float(d2), k))
        want = [k for _, k in sorted(cand)[:5] if k != j][:4]
        assert list(got[j]) == want, (j, got[j], want)


# ---- identity ---------------------------------------------------------------------------------------------------------------
def test_pins_only_give_the_identity_exactly_after_no_inner_iteration():
    c = loop_case(10000)
    R, t, res = gs.solve(c["npos"], c["nt0"], c["look"], c["src"], c["t_init"], c["src"])
    assert res["outer"] == 1 and res["inner"] == [0] and res["e_before"] == 0.0 and res["e_after"] == 0.0
    assert (R == np.tile(np.eye(3, dtype=f32).ravel(), (len(R), 1))).all() and (t == 0).all()


# ---- rigid ------------------------------------------------------------------------------------------------------------------
def test_one_rigid_motion_is_reproduced_by_every_node():
    c = loop_case(10000)
    Rm, tm = rot_y(4.0) @ np.array([[1, 0, 0], [0, np.cos(0.05), -np.sin(0.05)], [0, np.sin(0.05), np.cos(0.05)]]), np.array([0.03, -0.02, 0.05])
    dst = (c["src"].astype(f64) @ Rm.T + tm).astype(f32)
    R, t, res = gs.solve(c["npos"], c["nt0"], c["look"], c["src"], c["t_init"], dst)
    g = c["npos"].astype(f64)
    # a node's transform p -> A (p - g) + g + t equals p -> Rm p + tm iff A = Rm and t = Rm g + tm - g
    errA = np.abs(R.astype(f64).reshape(-1, 3, 3) - Rm).max()
    errt = np.abs(t.astype(f64) - (g @ Rm.T + tm - g)).max()
    print("rigid: outer %d inner %s E %.3e -> %.3e, |A - R| %.3e, |t - t*| %.3e" % (res["outer"], res["inner"], res["e_before"],
                                                                                 res["e_after"], errA, errt))
    # the rigid motion has zero energy, so the minimum is exact; what is left is the f32 rounding of dst (2^-24 of a few metres,
    # a constraint residual that the nodes share out) and of the output (2^-24).  Measured: |A - R| 6.9e-7, |t - t*| 5.0e-7, the
    # energy falls from 1.8e3 to 1.1e-10; asserted with a margin of one order of magnitude
    assert errA <= 6.9e-6 and errt <= 5.0e-6
    assert res["e_after"] <= 1.1e-9


# ---- direct solve -------------------------------------------------------------------------------------------------------------
def gap_to_direct(c, **params):
    P = gs.Problem(c["npos"], c["nt0"], c["look"], c["src"], c["t_init"], c["dst"], **params)
    R, t, res = P.solve()
    Rd, td, E = gs.direct_gauss_newton(c["npos"], P.edges, P.w, P.idx4, c["src"], c["dst"], **params)
    w4, idx4 = gr.bind(c["held"], c["held_t"], c["npos"], c["nt0"], c["look"])[:2]
    a = gs.deform_points(c["held"], w4, idx4, c["npos"], R, t)
    b = gs.deform_points(c["held"], w4, idx4, c["npos"], Rd, td)
    moved = np.abs(b - c["held"].astype(f64)).max()
    return res, E, abs(res["e_after"] - E[-1]) / E[-1], np.abs(a - b).max(), moved


# measured on the CPU (profiles/graph_solve.txt): relative energy gap, largest distance between the held-out points (metres)
#   m = 200:  energy 8.1e-16, points 2.4e-8        m = 2000: energy 1.3e-12, points 2.2e-8
# (the points' gap is the f32 rounding of the restatement's output, 2^-24 of A times a node distance; the direct route stays in
# f64).  Asserted: the measured gap times ten, for the platform's libm / BLAS under scipy
@pytest.mark.parametrize("name,e_tol,p_tol", [("n10k", 8.1e-15, 2.4e-7), ("n100k", 1.3e-11, 2.2e-7)])
def test_against_the_direct_gauss_newton(name, e_tol, p_tol):
    c = loop_case(**GPU_CASES[name])
    res, E, e_gap, p_gap, moved = gap_to_direct(c)
    print("%s: m %d, outer %d (direct %d), inner %s, E %.6e -> %.9e (direct %.9e), energy gap %.3e, held-out gap %.3e m of %.3f m"
          % (name, len(c["npos"]), res["outer"], len(E) - 1, res["inner"], res["e_before"], res["e_after"], E[-1], e_gap, p_gap, moved))
    assert moved > 0.05                                              # the held-out points do move
    assert e_gap <= e_tol and p_gap <= p_tol


# ---- condition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_condition_the_last_inner_loop_ends_by_tolerance(name):
    c = loop_case(**GPU_CASES[name])
    res = gs.solve(c["npos"], c["nt0"], c["look"], c["src"], c["t_init"], c["dst"])[2]
    assert res["inner_end"] == gs.END_TOL and max(res["inner"]) < gs.DEFAULTS["max_inner"], res


# ---- edge cases ---------------------------------------------------------------------------------------------------------------
# What tests/test_graph_solve_edges_gpu.py solves on the device: loop_case arguments, solver parameters, the ending that the last
# inner loop must reach, and how the constraints are replaced ("pins": dst = src; "hub": one point a thousand times).  The tests
# below prove on the restatement alone that each entry reaches its ending, iteration pattern and sizes.
LATE = dict(n=300, stride=10, look=4, n_con=20)                      # m = 30
ROOM = dict(n=3000, stride=10, look=6)                               # m = 300
BLOCKS = dict(max_outer=3, max_inner=48)
EDGE_CASES = {
    # rho underflows to zero after about 1500 iterations: a breakdown 50 iterations into a chunk, some 200 frozen launches after it
    "late_breakdown": dict(case=LATE, params=dict(inner_tol=0.0, max_inner=6000, inner_check=300, max_outer=2, damping=0.5),
                           end=gs.END_BREAKDOWN),
    "breakdown_at_0": dict(case=ROOM, params=dict(w_con=1e307, max_outer=2), end=gs.END_BREAKDOWN),      # p.q overflows to +inf
    "pins": dict(case=LATE, params={}, end=gs.END_ZERO, variant="pins"),
    "no_energy": dict(case=ROOM, params=dict(w_rot=0.0, w_reg=0.0, w_con=0.0), end=gs.END_ZERO),
    "check_every_1": dict(case=ROOM, params=dict(inner_check=1, max_outer=2), end=gs.END_TOL),
    "check_beyond_max": dict(case=LATE, params=dict(inner_check=5, max_inner=3, max_outer=64, outer_tol=0.0), end=gs.END_MAX_INNER),
    "hist_cap": dict(case=ROOM, params=dict(inner_check=300, max_inner=600, inner_tol=0.0, max_outer=1), end=gs.END_MAX_INNER),
    # constraints alone: the touched nodes fit them exactly (a few CG iterations, by tolerance), the others have D == 0 and stay
    "no_rot_no_reg": dict(case=LATE, params=dict(w_rot=0.0, w_reg=0.0, max_outer=3, max_inner=64), end=gs.END_TOL),
    "m256": dict(case=dict(n=2560, stride=10, look=6, n_con=257), params=BLOCKS, end=gs.END_MAX_INNER),
    "m257": dict(case=dict(n=2561, stride=10, look=6, n_con=256), params=BLOCKS, end=gs.END_MAX_INNER),
    "nc513": dict(case=dict(n=2561, stride=10, look=6, n_con=513), params=BLOCKS, end=gs.END_MAX_INNER),
    "three_passes": dict(case=dict(n=66000, stride=1, look=6, n_con=300), params=dict(max_outer=2, max_inner=8, inner_check=4),
                         end=gs.END_MAX_INNER),
    "one_hub": dict(case=LATE, params=BLOCKS, end=gs.END_MAX_INNER, variant="hub"),
}
HUB = 1000


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """loop_case of the entry with its variant applied; shared between the tests, so nobody writes into it"""
    e = EDGE_CASES[name]
    c = loop_case(**e["case"])
    if e.get("variant") == "pins":
        c["dst"] = c["src"].copy()
    elif e.get("variant") == "hub":
        c["src"] = np.repeat(c["src"][:1], HUB, axis=0)
        c["t_init"] = np.repeat(c["t_init"][:1], HUB)
        c["dst"] = (c["src"] + np.random.default_rng(77).normal(0.0, 0.01, (HUB, 3)).astype(f32)).astype(f32)
    return c


@functools.lru_cache(maxsize=None)
def edge_solution(name):
    """(Problem, rotations, translations, result) of the restatement for the entry, computed once for every test that needs it"""
    c = edge_case(name)
    P = gs.Problem(c["npos"], c["nt0"], c["look"], c["src"], c["t_init"], c["dst"], **EDGE_CASES[name]["params"])
    return (P,) + P.solve()


def is_identity(R, t):
    return bool((R == np.tile(np.eye(3, dtype=f32).ravel(), (len(R), 1))).all() and (t == 0).all())


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_edge_case_reaches_what_it_is_named_for(name):
    e = EDGE_CASES[name]
    P, R, t, res = edge_solution(name)
    p = P.p
    print(name, "m %d n_con %d" % (P.m, P.nc), {k: res[k] for k in ("outer", "inner", "inner_end", "e_before", "e_after")})
    assert res["inner_end"] == e["end"], res
    assert len(res["inner"]) == res["outer"] <= p["max_outer"]
    in_deg, con_deg = np.diff(P.in_off), np.diff(P.con_off)
    if name == "late_breakdown":
        assert P.m == 30 and res["outer"] == 2
        for it in res["inner"]:                                      # past the history's length, and inside a chunk of host reads
            assert it > 256 and it % 300 not in (0, 256), res
        assert np.isfinite(R).all() and np.isfinite(t).all()
        assert not is_identity(R, t)                                 # delta survived the breakdown
    elif name == "breakdown_at_0":
        assert res["outer"] == 1 and res["inner"] == [0] and is_identity(R, t)
        x = np.zeros((P.m, 12), f64); x[:, 0] = x[:, 4] = x[:, 8] = 1.0
        b = -P.Jt(x, P.residuals(x))
        with np.errstate(all="ignore"):
            z = np.where(P.diag(x) > 0, b / P.diag(x), 0.0)
            assert P.dot(b, z) > 0 and P.dot(z, P.Jt(x, P.J(x, z))) == np.inf          # rho_0 > 0, p.q = +inf
    elif name == "pins":
        assert res["outer"] == 1 and res["inner"] == [0] and res["e_before"] == 0.0 and is_identity(R, t)
    elif name == "no_energy":
        assert res["outer"] == 1 and res["inner"] == [0] and is_identity(R, t)
    elif name == "check_every_1":
        assert res["outer"] == 2 and any(it % 16 for it in res["inner"]), res
    elif name == "check_beyond_max":
        assert res["outer"] == 64 and res["inner"] == [3] * 64
    elif name == "hist_cap":
        assert res["inner"] == [600]
    elif name == "no_rot_no_reg":
        assert (con_deg == 0).any()                                  # nodes that no constraint touches: D == 0 rows, z = 0
        x = np.zeros((P.m, 12), f64); x[:, 0] = x[:, 4] = x[:, 8] = 1.0
        D = P.diag(x)
        assert (D[con_deg == 0] == 0).all() and (D[con_deg > 0] > 0).any()
        assert not is_identity(R, t)
    elif name in ("m256", "m257", "nc513"):
        assert (P.m, P.nc) == {"m256": (256, 257), "m257": (257, 256), "nc513": (257, 513)}[name]
        assert (in_deg == 0).any()                                   # an empty run in the list of edges that point at a node
    elif name == "three_passes":
        assert P.m == 66000 and P.nc == 300
        assert P.edges.max() >= 65536 and P.idx4.max() >= 65536      # keys whose bits 16-19 the third pass sorts
    elif name == "one_hub":
        assert con_deg.max() >= HUB and P.nc == HUB
    else:
        raise AssertionError("no check written for " + name)
