"""ssf_graph_solve and its companions (include/ssf_graph_solve.h) on the MI355X against the numpy restatement
(tests/graph_solve_ref.py, proven on the CPU by tests/test_graph_solve.py): edges, transforms and the result record at 0 bits;
run-to-run determinism; graph_apply_solved against graph_apply and the oracle; validity, refusals and no side effects."""
import os
import subprocess

import numpy as np
import pytest

import graph_solve_ref as gs
import test_graph_gpu as tg
import test_graph_solve as cpu
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding, synthetic

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
W, H = tg.W, tg.H
SHORT = dict(max_outer=3, max_inner=48)          # constructed cases: a few steps are enough to compare every kernel's bits


def solve_and_check(f, look, src, t0, dst, what, ref=None, **params):
    """ref: the restatement's (rotations, translations, result) of exactly these inputs, where a test has them already"""
    npos, nt0, _ = f.graph_nodes()
    assert np.array_equal(f.graph_edges(), gs.edges_of(npos, nt0, look)), what + " edges"
    res = f.graph_solve(src, t0, dst, **params)
    R, t = f.graph_transforms()
    Rr, tr, rr = ref if ref is not None else gs.solve(npos, nt0, look, src, t0, dst, **params)
    print(what, res)
    assert (res["outer"], res["inner"], res["inner_end"]) == (rr["outer"], rr["inner"], rr["inner_end"]), (what, res, rr)
    for k in ("e_before", "e_after", "e_rot", "e_reg", "e_con"):
        assert f64(res[k]).tobytes() == f64(rr[k]).tobytes(), (what, k, res[k], rr[k])
    util.assert_same_bits(R, Rr, what + " rotations")
    util.assert_same_bits(t, tr, what + " translations")
    return res, R, t


def model_constraints(f, n_con, seed, shift=0.02):
    """constraints from the model's own finite rows: the later-born half is pushed along a smooth field, the rest pinned"""
    model = f.get_model()
    pos = np.ascontiguousarray(model["positions"], f32).reshape(-1, 3)
    t0 = np.ascontiguousarray(model["stamps"], np.int32).reshape(-1, 2)[:, 0]
    ok = np.flatnonzero(np.isfinite(pos).all(axis=1))
    pick = np.random.default_rng(seed).choice(ok, min(n_con, len(ok)), replace=False)
    src, ts = pos[pick], t0[pick]
    late = ts >= np.median(t0[ok])
    dst = src.copy()
    dst[late] += (f32(shift) * np.stack([np.sin(src[late, 1]), np.cos(src[late, 0]), np.sin(src[late, 2] + src[late, 0])], 1)).astype(f32)
    return src, ts, dst


# ---- 1. bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cpu.GPU_CASES))
def test_solve_of_a_set_model_equals_the_restatement(name, product_lib):
    kw = cpu.GPU_CASES[name]
    c = cpu.loop_case(**kw)
    f = tg.handle(product_lib, 640, 480, nb_supersurfels_max=kw["n"] + 8192)
    f.set_model(c["model"][0], c["model"][1], 500)
    assert f.graph_build(stride=kw["stride"], look=kw["look"]) == len(c["npos"])
    util.assert_same_bits(f.graph_nodes()[0], c["npos"], "nodes")
    res, _, _ = solve_and_check(f, kw["look"], c["src"], c["t_init"], c["dst"], name)
    assert res["inner_end"] == 0 and res["e_after"] < 0.2 * res["e_before"]            # converged by the tolerance rule
    # determinism: the same inputs again, bit for bit
    R0, t0 = f.graph_transforms()
    res1 = f.graph_solve(c["src"], c["t_init"], c["dst"])
    R1, t1 = f.graph_transforms()
    assert res1 == res and R0.tobytes() == R1.tobytes() and t0.tobytes() == t1.tobytes()


def test_solve_after_processed_frames_equals_the_restatement(product_lib):
    f = tg.handle(product_lib)
    tg.run_frames(f, 0, 10)
    f.graph_build(stride=10, look=6)
    src, ts, dst = model_constraints(f, 300, 1)
    solve_and_check(f, 6, src, ts, dst, "frames")


@pytest.mark.parametrize("case", ["m5", "duplicates", "equal_stamps", "one_constraint", "coincident", "damped"])
def test_constructed_cases_equal_the_restatement(case, product_lib):
    f = tg.handle(product_lib, nb_supersurfels_max=20000)
    params = dict(SHORT)
    if case == "m5":
        m, nvis = tg.small_model(1000, 2)
        m["confidences"][:] = 0
        m["confidences"][::100][:9] = 3000
        f.set_model(m, nvis, 100)
        assert f.graph_build(stride=2, look=3) == 5
        look = 3
    elif case == "duplicates":
        m, nvis = tg.small_model(4000, 4, dup=True)
        f.set_model(m, nvis, 100); f.graph_build(stride=10, look=8); look = 8
    elif case == "equal_stamps":
        m, nvis = tg.small_model(5000, 3, t_mode="equal")
        f.set_model(m, nvis, 100); f.graph_build(stride=10, look=6); look = 6
    elif case == "coincident":                                        # every node at one point: every binding is the fallback
        m, nvis = tg.small_model(600, 5, one_point=True)
        f.set_model(m, nvis, 100); f.graph_build(stride=20, look=4); look = 4
    else:
        m, nvis = tg.small_model(9000, 7)
        f.set_model(m, nvis, 100); f.graph_build(stride=17, look=5); look = 5
        if case == "damped":
            params.update(damping=0.5, w_rot=2.0, w_reg=3.0, w_con=50.0, inner_check=5, max_inner=23)
    src, ts, dst = model_constraints(f, 1 if case == "one_constraint" else 200, 11)
    if case == "coincident":
        dst = (src + f32(0.01)).astype(f32)
    solve_and_check(f, look, src, ts, dst, case, **params)


# ---- 2. apply -----------------------------------------------------------------------------------------------------------------
def test_apply_solved_equals_graph_apply_and_the_oracle(product_lib, oracle_lib):
    n = 30000
    m, nvis = tg.stamped_model(n, bad_pos=0)
    a, b, o = [tg.handle(lib, 640, 480, nb_supersurfels_max=n + 8192) for lib in (product_lib, product_lib, oracle_lib)]
    for f in (a, b, o):
        f.set_model(m, nvis, 500)
    k = a.graph_build(stride=50, look=20)
    assert b.graph_build(stride=50, look=20) == k
    src, ts, dst = model_constraints(a, 1500, 2, shift=0.05)
    a.graph_solve(src, ts, dst)
    R, t = a.graph_transforms()
    npos, _, _ = b.graph_nodes()
    w4, idx4 = b.graph_binding()
    a.graph_apply_solved()
    b.graph_apply(R, t)
    o.apply_deformation(npos, R, t, w4, idx4)
    util.compare_state(a, b, maps=False, frame_surfels=False)
    util.compare_state(b, o, maps=False, frame_surfels=False)
    before = np.ascontiguousarray(m["positions"], f32).reshape(-1, 3)
    assert (a.get_model()["positions"].reshape(-1, 3) != before).any(axis=1).mean() > 0.3       # it did move the map


# ---- 3. state -----------------------------------------------------------------------------------------------------------------
def test_validity_and_refusals(product_lib):
    f = tg.handle(product_lib)
    pts, t0 = np.zeros((3, 3), f32), np.zeros(3, np.int32)
    with pytest.raises(binding.SsfError, match="no graph"):
        f.graph_solve(pts, t0, pts)
    tg.run_frames(f, 0, 6)
    f.graph_build(stride=10, look=5)
    with pytest.raises(binding.SsfError, match="no transforms"):
        f.graph_transforms()
    with pytest.raises(binding.SsfError, match="no transforms"):
        f.graph_apply_solved()
    src, ts, dst = model_constraints(f, 100, 3)
    bad = src.copy(); bad[7, 1] = np.nan
    inf = dst.copy(); inf[3, 0] = np.inf
    for args, kw in (((src[:0], ts[:0], dst[:0]), {}), ((bad, ts, dst), {}), ((src, ts, inf), {}), ((src, ts, dst), dict(w_rot=-1.0)),
                     ((src, ts, dst), dict(w_reg=float("nan"))), ((src, ts, dst), dict(w_con=float("inf"))),
                     ((src, ts, dst), dict(damping=-0.1)), ((src, ts, dst), dict(max_outer=0)), ((src, ts, dst), dict(max_inner=0)),
                     ((src, ts, dst), dict(inner_check=0)), ((src, ts, dst), dict(inner_tol=-1e-6)),
                     ((src, ts, dst), dict(inner_tol=float("nan"))), ((src, ts, dst), dict(outer_tol=-1e-6)),
                     ((src, ts, dst), dict(outer_tol=float("inf"))), ((src, ts, dst), dict(max_outer=binding.GRAPH_SOLVE_MAX_OUTER + 1))):
        with pytest.raises(binding.SsfError, match=r"\(-1\)"):       # SSF_ERR_INVALID_ARG
            f.graph_solve(*args, **kw)
    L, p = product_lib.lib, binding.SsfGraphSolveParams()
    assert L.ssf_graph_solve_default_params(None) == -1 and L.ssf_graph_solve_default_params(p) == 0
    ptr = lambda a: a.ctypes.data
    assert L.ssf_graph_solve(None, p, ptr(src), ptr(ts), ptr(dst), len(src), None) == -1
    assert L.ssf_graph_solve(f.h, None, ptr(src), ptr(ts), ptr(dst), len(src), None) == -1
    assert L.ssf_graph_solve(f.h, p, None, ptr(ts), ptr(dst), len(src), None) == -1
    assert L.ssf_graph_solve(f.h, p, ptr(src), None, ptr(dst), len(src), None) == -1
    assert L.ssf_graph_solve(f.h, p, ptr(src), ptr(ts), None, len(src), None) == -1
    assert L.ssf_graph_get_edges(f.h, None, 1 << 20) == -1 and L.ssf_graph_get_transforms(f.h, None, None, 1 << 20) == -1
    assert L.ssf_graph_apply_solved(None) == -1
    big = np.zeros((1 << 20) + 1, f32)                                # more than 2^20 constraints: refused before anything is read
    assert L.ssf_graph_solve(f.h, p, ptr(big), ptr(big), ptr(big), (1 << 20) + 1, None) == -1
    k = f.graph_info()["n_nodes"]
    f.graph_solve(src, ts, dst, **SHORT)                             # (result pointer optional: exercised through the binding with one)
    with pytest.raises(binding.SsfError, match="room for"):
        f.graph_edges(capacity=k - 1)
    with pytest.raises(binding.SsfError, match="room for"):
        f.graph_transforms(capacity=k - 1)

    def all_stale():
        assert not f.graph_info()["valid"]
        for call in (f.graph_edges, f.graph_transforms, f.graph_apply_solved, lambda: f.graph_solve(src, ts, dst)):
            with pytest.raises(binding.SsfError, match="stale"):
                call()
    tg.run_frames(f, 6, 1)                                           # a frame
    all_stale()
    f.graph_build(stride=10, look=5)
    with pytest.raises(binding.SsfError, match="no transforms"):     # solved transforms die with the graph they belong to
        f.graph_transforms()
    f.graph_solve(src, ts, dst, **SHORT)
    f.set_model(f.get_model(), f.counts()["n_visible"], f.counts()["stamp"])
    all_stale()
    f.graph_build(stride=10, look=5); f.graph_solve(src, ts, dst, **SHORT)
    f.graph_apply_solved()                                           # its own apply
    all_stale()
    tg.run_frames(f, 7, 1)                                           # ... and the handle still works
    f.graph_build(stride=10, look=5)
    assert f.graph_solve(src, ts, dst, **SHORT)["outer"] >= 1


def test_refused_with_frames_pending_and_on_a_sharded_handle(product_lib):
    f = tg.handle(product_lib, pipeline_depth=1, extract_batch=2)
    frames = [util.frame(k, W, H) for k in range(4)]
    f.submit_frame(*frames[0]); f.process_submitted()
    f.submit_frame(*frames[1]); f.process_submitted()
    f.graph_build(stride=10, look=5)
    src, ts, dst = model_constraints(f, 50, 4)
    f.graph_solve(src, ts, dst, **SHORT)
    f.submit_frame(*frames[2])
    for call in (lambda: f.graph_solve(src, ts, dst), f.graph_edges, f.graph_transforms, f.graph_apply_solved):
        with pytest.raises(binding.SsfError, match="pending"):
            call()
    f.process_submitted()
    g = tg.handle(product_lib, rank=0, nranks=2, shard_tile=0.25)
    m, nvis = tg.small_model(2000, 9)
    g.set_model(m, nvis, 100)
    for call in (lambda: g.graph_solve(src, ts, dst), g.graph_edges, g.graph_transforms, g.graph_apply_solved):
        with pytest.raises(binding.SsfError, match="sharded"):
            call()


def test_a_build_and_solve_between_frames_changes_nothing_later(product_lib):
    a, b = tg.handle(product_lib), tg.handle(product_lib)
    ra, rb = tg.run_frames(a, 0, 8), tg.run_frames(b, 0, 8)
    a.graph_build(stride=10, look=6)
    src, ts, dst = model_constraints(a, 200, 5)
    a.graph_solve(src, ts, dst, **SHORT)
    a.graph_edges(); a.graph_transforms()
    util.compare_state(a, b)
    ra += tg.run_frames(a, 8, 6); rb += tg.run_frames(b, 8, 6)
    for x, y in zip(ra, rb):
        util.same_result(x, y)
        util.assert_same_bits(x["pose"], y["pose"], "pose")
    util.compare_state(a, b)


def test_kernel_times_are_reported_under_profile(product_lib):
    f = tg.handle(product_lib, profile=1)
    tg.run_frames(f, 0, 4)
    f.graph_build(stride=10, look=5)
    src, ts, dst = model_constraints(f, 100, 6)
    f.graph_solve(src, ts, dst, **SHORT)
    f.graph_apply_solved()
    names = set(f.kernel_times())
    assert {"graph_solve", "graph_rank", "apply_deformation"} <= names, names


# ---- 4. the C++ surface ---------------------------------------------------------------------------------------------------------
def test_graph_solve_smoke_cpp_agrees_with_the_python_mirror(product_lib, tmp_path):
    n = 4
    frames = [util.frame(k, W, H) for k in range(n)]
    raw = tmp_path / "frames.bin"
    with open(raw, "wb") as fh:
        for rgb, depth in frames:
            fh.write(np.ascontiguousarray(rgb, np.uint8).tobytes()); fh.write(np.ascontiguousarray(depth, f32).tobytes())
    exe = tmp_path / "graph_solve_smoke"
    libdir = os.path.dirname(product_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "graph_solve_smoke.cpp"), "-o", str(exe), "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    K = synthetic.intrinsics(W, H)
    r = subprocess.run([str(exe), str(W), str(H), str(n), str(raw)] + [repr(float(K[k])) for k in ("fx", "fy", "cx", "cy")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    f = binding.Fusion(product_lib, product_lib.default_config(nb_supersurfels_max=50000, lambda_pos=10.0, lambda_bound=1000.0,
                                                               lambda_size=1000.0, lambda_disp=1e8,
                                                               **{k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}))
    for rgb, depth in frames:
        f.process_frame(rgb, depth)
    m = f.graph_build(stride=8, look=5)
    gp, gt, _ = f.graph_nodes()
    assert lines[0] == "graph nodes=%d edges %016x" % (m, tg.fnv(f.graph_edges()))
    dst = gp.copy()
    dst[m // 2:, 0] += f32(0.01); dst[m // 2:, 2] -= f32(0.02)
    f.graph_solve(gp, gt, dst, max_outer=3, inner_check=1)           # the smoke's first solve: no result record there
    every_1 = tg.fnv(*f.graph_transforms())
    res = f.graph_solve(gp, gt, dst, max_outer=3)
    inner = (res["inner"] + [0, 0, 0])[:3]
    en = np.array([res[k] for k in ("e_before", "e_after", "e_rot", "e_reg", "e_con")], f64)
    assert lines[1] == "solve outer=%d inner=%d,%d,%d end=%d energy %016x" % ((res["outer"],) + tuple(inner) + (res["inner_end"], tg.fnv(en)))
    R, t = f.graph_transforms()
    assert lines[2] == "transforms %016x" % tg.fnv(R, t)
    f.graph_apply_solved()
    model = f.get_model()
    assert lines[3] == "model %d %016x" % (len(model["confidences"]), tg.fnv(model["positions"]))
    assert lines[4] == "stale_after_apply 1"
    assert lines[5] == "no_record_check_every_1 transforms %016x" % every_1
