"""The numpy restatement of include/ssf_graph_solve.h (tests/graph_solve_ref.py) under test, so that the GPU tests compare against
something proven: its J, J^T and diagonal against finite differences of its own residuals, the identity, a rigid motion, and its
result against an independent Gauss-Newton with a sparse direct solve."""
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
