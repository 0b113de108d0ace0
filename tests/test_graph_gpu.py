"""ssf_graph_* (include/ssf_graph.h) on the MI355X against the numpy restatement (tests/graph_ref.py): the node table, the binding
of every row and of caller points at 0 bits; graph_apply against apply_deformation (and through it the oracle); a loop closure in
a sequence against today's host route; validity, refusals and no side effects on the frame path."""
import os
import subprocess

import numpy as np
import pytest

import graph_ref as gr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding, synthetic

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 160, 128


def handle(lib, w=W, h=H, **kw):
    return binding.Fusion(lib, util.make_cfg(lib, w, h, **kw))


def stamped_model(n, frames=400, seed=3, dead=0.04, bad_pos=5, t_base=0):
    """seeded room rows in camera 0's frame (visible rows first), births swept over `frames` stamps starting at t_base, a share
    of rows with conf <= 0, a few non-finite positions"""
    m, nvis = synthetic.seed_model_cam0(n, 640, 480, stamp=30, seed=1234 + seed)
    rng = np.random.default_rng(seed)
    pos = m["positions"].reshape(n, 3)
    az = np.arctan2(pos[:, 2], pos[:, 0])
    t0 = ((az + np.pi) / (2 * np.pi) * frames + rng.integers(0, max(1, frames // 20), n)).astype(np.int64) + t_base
    st = m["stamps"].reshape(n, 2).copy()
    st[:, 0] = t0.astype(np.int32)
    m["stamps"] = st.reshape(m["stamps"].shape)
    conf = m["confidences"].copy()
    conf[rng.random(n) < dead] = f32(0)
    conf[rng.random(n) < dead / 4] = f32(-1)
    m["confidences"] = conf
    if bad_pos:
        rows = rng.choice(n, bad_pos, replace=False)
        pos[rows[0::2], 1] = np.nan
        pos[rows[1::2], 0] = np.inf
        m["positions"] = pos.reshape(m["positions"].shape)
    return m, nvis


def check_nodes(f, stride, min_conf=0.0, what=""):
    model = f.get_model()
    npos, nt0, rows = gr.nodes_of(model, stride, min_conf)
    gp, gt, grows = f.graph_nodes()
    assert f.graph_info() == {"n_nodes": len(rows), "n_rows": len(model["confidences"]), "valid": True}, what
    util.assert_same_bits(grows, rows, what + " node rows")
    util.assert_same_bits(gt, nt0, what + " node stamps")
    util.assert_same_bits(gp, npos, what + " node positions")
    return model, (npos, nt0, rows)


def check_binding(f, model, nodes, look, what=""):
    pos = np.ascontiguousarray(model["positions"], f32).reshape(-1, 3)
    t0 = np.ascontiguousarray(model["stamps"], np.int32).reshape(-1, 2)[:, 0]
    w4, idx4, bad, _, _ = gr.bind(pos, t0, nodes[0], nodes[1], look)
    gw, gi = f.graph_binding()
    util.assert_same_bits(gi, idx4, what + " idx4")
    util.assert_same_bits(gw, w4, what + " weights4")
    return bad


def build_and_check(f, stride, look, min_conf=0.0, what=""):
    m = f.graph_build(stride=stride, look=look, min_conf=min_conf)
    model, nodes = check_nodes(f, stride, min_conf, what)
    assert m == len(nodes[2])
    return model, nodes, check_binding(f, model, nodes, look, what)


def run_frames(f, first, count, w=W, h=H):
    return [f.process_frame(*util.frame(k, w, h)) for k in range(first, first + count)]


# ---- 1. nodes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [50000, 200000])
def test_nodes_and_binding_of_a_set_model(n, product_lib):
    f = handle(product_lib, 640, 480, nb_supersurfels_max=n + 8192)
    m, nvis = stamped_model(n)
    f.set_model(m, nvis, 500)
    model, nodes, bad = build_and_check(f, 50, 20, what="n=%d" % n)
    assert len(nodes[2]) > 800 and not np.isfinite(model["positions"]).all() and (model["confidences"] <= 0).sum() > 100
    assert bad.sum() == (~np.isfinite(model["positions"].reshape(-1, 3)).all(axis=1)).sum()      # only the non-finite rows fall back
    build_and_check(f, 50, 20, min_conf=2999.0, what="n=%d min_conf" % n)
    build_and_check(f, 7, 3, what="n=%d stride 7" % n)


def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def test_nodes_and_binding_after_processed_frames(product_lib):
    """44 frames of a camera panning 1.5 degrees per frame (with the true pose as the prior): the rows of the first frames leave
    the view and live in the out-of-view store"""
    w, h = 320, 240
    f = handle(product_lib, w, h, nb_supersurfels_max=40000)
    R0, t0 = synthetic.orbit_pose(0)
    for k in range(44):
        rgb, depth, _ = synthetic.render(R0 @ rot_y(1.5 * k), t0, w, h, noise=True, rng=np.random.default_rng(1000 + k))
        prior = np.concatenate([rot_y(1.5 * k).ravel(), np.zeros(3)]).astype(f32)
        f.process_frame(rgb, depth, prior_pose=prior)
    c = f.counts()
    assert 0 < c["n_visible"] < c["n_model"], c                      # both stores populated, the visible block in front
    model, nodes, bad = build_and_check(f, 20, 8, what="frames")
    assert len(np.unique(nodes[1])) > 5                              # real stamps
    assert (nodes[2] >= c["n_visible"]).any() and (nodes[2] < c["n_visible"]).any()      # nodes from both stores
    build_and_check(f, 50, 20, min_conf=f.cfg.conf_thresh, what="frames conf_thresh")
    build_and_check(f, 3, 3, what="frames stride 3")


# ---- 2. binding over a grid of (stride, look) and constructed cases ------------------------------------------------------------
def small_model(n, seed, t_mode="sweep", dup=False, one_point=False):
    m, nvis = stamped_model(n, frames=60, seed=seed, dead=0.1, bad_pos=3)
    pos = m["positions"].reshape(n, 3)
    st = m["stamps"].reshape(n, 2)
    if t_mode == "equal":
        st[:, 0] = 17
    if dup:                                                          # many rows at a few positions: ties broken by node index
        pos[:] = pos[np.random.default_rng(seed).integers(0, 6, n)]
    if one_point:
        pos[:] = np.array([0.3, -0.2, 1.5], f32)
    m["positions"], m["stamps"] = pos.reshape(m["positions"].shape), st.reshape(m["stamps"].shape)
    return m, nvis


@pytest.mark.parametrize("case", ["clipped", "m5", "equal_stamps", "duplicates", "dmax0", "odd_size", "grid"])
def test_binding_grid(case, product_lib):
    f = handle(product_lib, nb_supersurfels_max=20000)
    if case == "clipped":                                            # m < 2 L
        m, nvis = small_model(3000, 1)
        f.set_model(m, nvis, 100)
        model, nodes, _ = build_and_check(f, 100, 20, what=case)
        assert 5 < len(nodes[2]) < 40
    elif case == "m5":
        m, nvis = small_model(1000, 2, dup=False)
        m["confidences"][:] = 0
        m["confidences"][::100][:9] = 3000                           # 9 eligible rows, stride 2 -> 5 nodes
        f.set_model(m, nvis, 100)
        model, nodes, _ = build_and_check(f, 2, 3, what=case)
        assert len(nodes[2]) == 5
    elif case == "equal_stamps":
        m, nvis = small_model(5000, 3, t_mode="equal")
        f.set_model(m, nvis, 100)
        model, nodes, _ = build_and_check(f, 10, 6, what=case)
        assert (np.diff(nodes[2]) > 0).all()                         # one stamp: node order = row order
    elif case == "duplicates":
        m, nvis = small_model(4000, 4, dup=True)
        f.set_model(m, nvis, 100)
        build_and_check(f, 10, 8, what=case)
    elif case == "dmax0":                                            # every node at one point: the fallback
        m, nvis = small_model(600, 5, one_point=True)
        f.set_model(m, nvis, 100)
        model, nodes, bad = build_and_check(f, 20, 4, what=case)
        assert bad.all()
        w, _ = f.graph_binding()
        assert (w == f32(0.25)).all()
    elif case == "odd_size":                                         # not a multiple of the workgroup size, in either store
        m, nvis = small_model(1234 + 256 * 3 + 77, 6)
        f.set_model(m, min(nvis, 333), 100)
        build_and_check(f, 9, 5, what=case)
    else:
        m, nvis = small_model(9000, 7)
        f.set_model(m, nvis, 100)
        for stride, look in ((1, 3), (3, 20), (50, 4), (200, 3), (17, 40)):
            build_and_check(f, stride, look, what="grid %d %d" % (stride, look))


def test_negative_stamps_just_inside_the_span_and_one_outside(product_lib):
    f = handle(product_lib, nb_supersurfels_max=20000)
    m, nvis = small_model(6000, 8)
    st = m["stamps"].reshape(-1, 2)
    rng = np.random.default_rng(8)
    st[:, 0] = rng.integers(-700000, -700000 + (1 << 20), len(st))
    el = np.flatnonzero(gr.eligible(m["positions"].reshape(-1, 3), m["confidences"]))
    st[el[0], 0], st[el[1], 0] = -700000, -700000 + (1 << 20) - 1    # max - min = 2^20 - 1: the widest span accepted
    m["stamps"] = st.reshape(m["stamps"].shape)
    f.set_model(m, nvis, 100)
    build_and_check(f, 25, 10, what="span 2^20 - 1")
    st[el[1], 0] += 1
    m["stamps"] = st.reshape(m["stamps"].shape)
    f.set_model(m, nvis, 100)
    with pytest.raises(binding.SsfError, match="span"):
        f.graph_build(stride=25, look=10)
    assert not f.graph_info()["valid"]
    st[el[1], 0] -= 1                                                # ... and the handle still works
    m["stamps"] = st.reshape(m["stamps"].shape)
    f.set_model(m, nvis, 100)
    build_and_check(f, 25, 10, what="after the refusal")


# ---- 3. caller points ---------------------------------------------------------------------------------------------------
def test_bind_points(product_lib):
    f = handle(product_lib, 640, 480, nb_supersurfels_max=60000)
    m, nvis = stamped_model(50000, frames=300, t_base=-40)
    f.set_model(m, nvis, 400)
    for stride, look in ((50, 20), (400, 70)):
        f.graph_build(stride=stride, look=look)
        npos, nt0, _ = f.graph_nodes()
        rng = np.random.default_rng(stride)
        n = 10007
        pts = rng.uniform(-4, 4, (n, 3)).astype(f32)
        pts[:500] = npos[rng.integers(0, len(npos), 500)]            # some exactly on nodes
        pts[500] = np.nan
        t0 = rng.integers(int(nt0.min()) - 50, int(nt0.max()) + 50, n).astype(np.int32)
        t0[:10], t0[10:20] = int(nt0.min()) - 1000, int(nt0.max()) + 1000
        w4, idx4 = gr.bind(pts, t0, npos, nt0, look)[:2]
        gw, gi = f.graph_bind_points(pts, t0)
        util.assert_same_bits(gi, idx4, "points idx4")
        util.assert_same_bits(gw, w4, "points weights4")
    with pytest.raises(binding.SsfError, match="stamps"):
        f.graph_bind_points(np.zeros((4, 3), f32), np.zeros(3, np.int32))


# ---- 4. apply ----------------------------------------------------------------------------------------------------------
def node_transforms(m, seed=5, angle=0.02, shift=0.01):
    """smooth per-node rotations / translations, as util.deformation_for makes them"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-angle, angle, (m, 3))
    R = np.stack([(synthetic.rot_y(a[1]) @ synthetic.rot_x(a[0])).reshape(9) for a in ang]).astype(f32)
    return R, rng.uniform(-shift, shift, (m, 3)).astype(f32)


def test_graph_apply_equals_apply_deformation_and_the_oracle(product_lib, oracle_lib):
    n = 30000
    m, nvis = stamped_model(n, bad_pos=0)
    hs = [handle(lib, 640, 480, nb_supersurfels_max=n + 8192) for lib in (product_lib, product_lib, oracle_lib)]
    for f in hs:
        f.set_model(m, nvis, 500)
    a, b, o = hs
    k = a.graph_build(stride=50, look=20)
    assert b.graph_build(stride=50, look=20) == k
    npos, _, _ = b.graph_nodes()
    w4, idx4 = b.graph_binding()
    R, t = node_transforms(k)
    a.graph_apply(R, t)
    b.apply_deformation(npos, R, t, w4, idx4)
    o.apply_deformation(npos, R, t, w4, idx4)
    util.compare_state(a, b, maps=False, frame_surfels=False)
    util.compare_state(b, o, maps=False, frame_surfels=False)
    before = np.ascontiguousarray(m["positions"], f32).reshape(-1, 3)
    assert (a.get_model()["positions"].reshape(-1, 3) != before).any(axis=1).mean() > 0.9       # it did move the map


# ---- 5. in a sequence, against today's host route ------------------------------------------------------------------------
def test_loop_closure_in_a_sequence_against_the_host_route(product_lib):
    a, b = handle(product_lib), handle(product_lib)
    ra, rb = run_frames(a, 0, 12), run_frames(b, 0, 12)
    k = a.graph_build(stride=10, look=6)
    R, t = node_transforms(k, angle=0.004, shift=0.002)
    a.graph_apply(R, t)
    model = b.get_model()                                            # today's route: copy out, bind on the host, upload
    (npos, nt0, rows), (w4, idx4) = gr.bind_model(model, 10, 6)
    assert len(rows) == k
    b.apply_deformation(npos, R, t, w4, idx4)
    util.compare_state(a, b)
    ra += run_frames(a, 12, 6); rb += run_frames(b, 12, 6)
    for x, y in zip(ra, rb):
        util.same_result(x, y)
        util.assert_same_bits(x["pose"], y["pose"], "pose")
    util.compare_state(a, b)


# ---- 6. state ------------------------------------------------------------------------------------------------------------
def test_validity_and_refusals(product_lib):
    f = handle(product_lib)
    with pytest.raises(binding.SsfError, match="empty"):
        f.graph_build()
    with pytest.raises(binding.SsfError, match="no graph"):
        f.graph_binding()
    run_frames(f, 0, 6)
    n = f.counts()["n_model"]
    for kw in (dict(stride=0), dict(look=2), dict(min_conf=float("nan")), dict(min_conf=float("inf"))):
        with pytest.raises(binding.SsfError, match=r"\(-1\)"):       # SSF_ERR_INVALID_ARG
            f.graph_build(**kw)
    k = f.graph_build(stride=10, look=5)
    assert f.graph_info() == {"n_nodes": k, "n_rows": n, "valid": True}
    with pytest.raises(binding.SsfError, match="room for"):          # SSF_ERR_CAPACITY
        f.graph_nodes(capacity=k - 1)
    R, t = node_transforms(k)
    pts, t0 = np.zeros((3, 3), f32), np.zeros(3, np.int32)

    def all_stale():
        assert not f.graph_info()["valid"]
        for call in (f.graph_binding, lambda: f.graph_bind_points(pts, t0), lambda: f.graph_apply(R, t)):
            with pytest.raises(binding.SsfError, match="stale"):
                call()
    run_frames(f, 6, 1)                                              # a frame
    all_stale()
    k = f.graph_build(stride=10, look=5); R, t = node_transforms(k)
    f.set_model(f.get_model(), f.counts()["n_visible"], f.counts()["stamp"])
    all_stale()
    k = f.graph_build(stride=10, look=5); R, t = node_transforms(k)
    f.graph_apply(R, t)                                              # its own apply
    all_stale()
    k = f.graph_build(stride=10, look=5); R, t = node_transforms(k)
    w4, idx4 = f.graph_binding()
    f.apply_deformation(f.graph_nodes()[0], R, t, w4, idx4)
    all_stale()
    # too few nodes: refused, nothing kept, the handle still works
    with pytest.raises(binding.SsfError, match="at least 5"):
        f.graph_build(stride=f.counts()["n_model"], look=5)
    assert f.graph_info() == {"n_nodes": 0, "n_rows": 0, "valid": False}
    run_frames(f, 7, 1)
    assert f.graph_build(stride=10, look=5) >= 5


def test_refused_with_frames_pending_and_on_a_sharded_handle(product_lib):
    f = handle(product_lib, pipeline_depth=1, extract_batch=2)
    frames = [util.frame(k, W, H) for k in range(4)]
    f.submit_frame(*frames[0]); f.process_submitted()
    f.submit_frame(*frames[1]); f.process_submitted()
    k = f.graph_build(stride=10, look=5)
    f.submit_frame(*frames[2])
    for call in (lambda: f.graph_build(stride=10, look=5), f.graph_binding, lambda: f.graph_apply(*node_transforms(k))):
        with pytest.raises(binding.SsfError, match="pending"):
            call()
    f.process_submitted()
    g = handle(product_lib, rank=0, nranks=2, shard_tile=0.25)
    m, nvis = small_model(2000, 9)
    g.set_model(m, nvis, 100)
    with pytest.raises(binding.SsfError, match="sharded"):
        g.graph_build(stride=10, look=5)


# ---- 7. no side effects; run to run ------------------------------------------------------------------------------------------
def test_a_build_between_frames_changes_nothing_later_and_is_reproducible(product_lib):
    a, b = handle(product_lib), handle(product_lib)
    ra, rb = run_frames(a, 0, 8), run_frames(b, 0, 8)
    a.graph_build(stride=10, look=6)
    first = [x.copy() for x in a.graph_nodes() + a.graph_binding()]
    a.graph_build(stride=10, look=6)
    for x, y in zip(first, a.graph_nodes() + a.graph_binding()):
        assert x.tobytes() == y.tobytes()
    util.compare_state(a, b)
    ra += run_frames(a, 8, 6); rb += run_frames(b, 8, 6)
    for x, y in zip(ra, rb):
        util.same_result(x, y)
        util.assert_same_bits(x["pose"], y["pose"], "pose")
    util.compare_state(a, b)


def test_kernel_times_are_reported_under_profile(product_lib):
    f = handle(product_lib, profile=1)
    run_frames(f, 0, 4)
    k = f.graph_build(stride=10, look=5)
    f.graph_apply(*node_transforms(k))
    names = set(f.kernel_times())
    assert {"graph_rank", "graph_sample", "graph_bind", "apply_deformation"} <= names, names


# ---- 8. the C++ surface ------------------------------------------------------------------------------------------------------
def fnv(*arrays):
    h = 1469598103934665603
    for a in arrays:
        for byte in np.ascontiguousarray(a).tobytes():
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_graph_smoke_cpp_agrees_with_the_python_mirror(product_lib, tmp_path):
    n = 4
    frames = [util.frame(k, W, H) for k in range(n)]
    raw = tmp_path / "frames.bin"
    with open(raw, "wb") as fh:
        for rgb, depth in frames:
            fh.write(np.ascontiguousarray(rgb, np.uint8).tobytes()); fh.write(np.ascontiguousarray(depth, f32).tobytes())
    exe = tmp_path / "graph_smoke"
    libdir = os.path.dirname(product_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "graph_smoke.cpp"), "-o", str(exe), "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    K = synthetic.intrinsics(W, H)
    r = subprocess.run([str(exe), str(W), str(H), str(n), str(raw)] + [repr(float(K[k])) for k in ("fx", "fy", "cx", "cy")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    # the same arguments as graph_smoke.cpp's initialize(): reference defaults but for four energy weights
    f = binding.Fusion(product_lib, product_lib.default_config(nb_supersurfels_max=50000, lambda_pos=10.0, lambda_bound=1000.0,
                                                               lambda_size=1000.0, lambda_disp=1e8,
                                                               **{k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}))
    for rgb, depth in frames:
        f.process_frame(rgb, depth)
    m = f.graph_build(stride=8, look=5)
    gp, gt, grows = f.graph_nodes()
    w4, idx4 = f.graph_binding()
    pw, pi = f.graph_bind_points(gp, gt)
    assert lines[0] == "graph nodes=%d rows=%d" % (m, f.counts()["n_model"])
    assert lines[1] == "nodes %016x" % fnv(gp, gt, grows)
    assert lines[2] == "binding %d %016x" % (len(idx4), fnv(w4, idx4))
    assert lines[3] == "points %d %016x" % (len(pi), fnv(pw, pi))
    k = np.arange(m)
    t = np.stack([f32(0.001) * (k % 5).astype(f32), np.zeros(m, f32), f32(-0.002) * (k % 3).astype(f32)], 1).astype(f32)
    f.graph_apply(np.tile(np.eye(3, dtype=f32).reshape(1, 9), (m, 1)), t)
    model = f.get_model()
    assert lines[4] == "model %d %016x" % (len(model["confidences"]), fnv(model["positions"]))
    assert lines[5] == "stale_after_apply 1"
