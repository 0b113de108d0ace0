"""ssf_query_count / ssf_query_rows (include/ssf_query.h) on the MI355X against the numpy restatement (tests/query_ref.py): the
index, every returned field against get_model()[index] and all of stats at 0 bits -- on hand-built models at the block and wave
edges of both stores, boundary-exact rows, a store with holes (before and after its compaction); plus field subsets, capacity,
growth, device outputs, no side effects on the frame path, the refusals, profiling and the C++ surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import query_ref as qr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding, synthetic

pytestmark = pytest.mark.gpu
W, H = 160, 128
ALL_FIELDS = tuple(name for name, _, _ in binding.SURFEL_FIELDS)
CPP = os.path.join(ROOT, "tests", "cpp")


def handle(lib, **kw):
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


def cam_of(f):
    c = f.cfg
    return dict(width=c.width, height=c.height, fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy), (c.range_min, c.range_max)


def same_stats(got, want, what):
    for k in ("n_scanned", "n_selected", "n_selected_visible"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    util.assert_same_bits(got["lo"], want["lo"], what + " lo")
    util.assert_same_bits(got["hi"], want["hi"], what + " hi")


def check(f, what, pose=None, fields=ALL_FIELDS, model=None, **kw):
    """query on the device and in numpy from get_model's rows; returns the device result"""
    model = f.get_model() if model is None else model
    nv = f.counts()["n_visible"]
    cam, zr = cam_of(f)
    q = qr.params(**dict(kw, camera=kw.get("camera") or cam, z_range=kw.get("z_range") or zr))
    idx, stats = qr.select(model, nv, f.get_pose() if pose is None else pose, q)
    got = f.query_model(fields=fields, pose=pose, **kw)
    util.assert_same_bits(got["index"], idx, what + " index")
    same_stats(got["stats"], stats, what)
    same_stats(f.query_count(pose=pose, **kw), stats, what + " (count)")
    assert sorted(got) == sorted(tuple(fields) + ("index", "stats")), what
    for name in fields:
        util.assert_same_bits(got[name], model[name][idx], what + " " + name)
    return got


@pytest.fixture(scope="module")
def fusion(product_lib):
    """one handle for the tests that replace the model through set_model"""
    f = handle(product_lib)
    yield f
    f.close()


# ---- hand-built models ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nv", qr.SIZES)
def test_hand_built_models(n, nv, fusion):
    f = fusion
    cam, zr = cam_of(f)
    for seed in qr.SEEDS:
        m = qr.hand_model(n, seed)
        f.set_model(m, nv, 100)
        model = f.get_model()
        for name in m:
            util.assert_same_bits(model[name], m[name], "set_model / get_model " + name)
        for name, pose, kw in qr.region_queries(cam, zr):
            check(f, "n %d nv %d seed %d %s" % (n, nv, seed, name), pose=pose, model=model, **kw)


def test_selections_of_one_wave_everything_and_nothing(fusion):
    f = fusion
    m = qr.hand_model(1300, 1)
    # rows 576..639 (one wave of the third block of the visible array) and rows 1100..1163 get a stamp nobody else has
    m["stamps"][576:640, 0] = 500
    m["stamps"][1100:1164, 1] = 600
    f.set_model(m, 1024, 100)
    got = check(f, "one wave of the visible array", t_init=(500, 500))
    assert got["index"].tolist() == list(range(576, 640))
    got = check(f, "64 rows of the out-of-view span", t_last=(600, 600))
    assert got["index"].tolist() == list(range(1100, 1164))
    got = check(f, "everything")
    assert got["stats"]["n_selected"] == 1300 and got["stats"]["n_selected_visible"] == 1024
    # nothing: 0 rows, a zero box, and the outputs are not touched
    arrays = {name: np.full((8, k) if k > 1 else (8,), 77, dt) for name, k, dt in binding.SURFEL_FIELDS}
    index = np.full(8, 77, np.int32)
    st = f.query_rows_into(arrays, index, 8, min_conf=1e9)
    assert st["n_selected"] == 0 and st["n_selected_visible"] == 0 and st["n_scanned"] == 1300
    assert not st["lo"].any() and not st["hi"].any()
    assert (index == 77).all() and all((a == 77).all() for a in arrays.values())
    assert check(f, "nothing", min_conf=1e9)["index"].size == 0


def test_boundary_exact_rows(fusion):
    f = fusion
    m, nv, cam, zr, cases = qr.boundary_rows()
    f.set_model(m, nv, 100)
    model = f.get_model()
    util.assert_same_bits(model["positions"], m["positions"], "positions (NaN, inf and -0 survive set_model)")
    for name, kw, want in cases:
        kw = dict(kw, pose=qr.IDENTITY)
        if kw.get("region") == "frustum":
            kw.update(camera=cam, z_range=zr)
        got = check(f, name, model=model, **kw)
        assert got["index"].tolist() == want, (name, got["index"].tolist(), want)
        got = check(f, name + " visible", model=model, visible_only=True, **kw)
        assert got["index"].tolist() == [i for i in want if i < nv], name
    st = f.query_count(pose=qr.IDENTITY, **cases[-1][1])
    util.assert_same_bits(st["lo"], np.array([0.0, 0.0, 0.25], np.float32), "lo with -0 rows")
    util.assert_same_bits(st["hi"], np.array([0.0, 0.0, 1.0], np.float32), "hi with -0 rows")


def test_field_subsets(fusion):
    f = fusion
    m = qr.hand_model(700, 2)
    f.set_model(m, 250, 100)
    kw = dict(region="sphere", radius=2.5, pose=qr.CALLER_POSE)
    full = check(f, "all fields", **kw)
    n = full["stats"]["n_selected"]
    assert 0 < n < 700
    for fields in (("positions",), ("positions", "colors"), ("orientations", "confidences")):
        got = check(f, "fields %s" % (fields,), fields=fields, **kw)
        util.assert_same_bits(got["index"], full["index"], "index with %s" % (fields,))
        # into arrays of every field: the ones not asked for stay as they were
        arrays = {name: np.full((n, k) if k > 1 else (n,), 77, dt) for name, k, dt in binding.SURFEL_FIELDS}
        f.query_rows_into({name: arrays[name] for name in fields}, None, n, **kw)
        for name, a in arrays.items():
            if name in fields:
                util.assert_same_bits(a, full[name], "subset " + name)
            else:
                assert (a == 77).all(), name
    # the index alone
    index = np.zeros(n, np.int32)
    f.query_rows_into({}, index, n, **kw)
    util.assert_same_bits(index, full["index"], "index alone")


def test_capacity(fusion):
    f = fusion
    m = qr.hand_model(700, 0)
    f.set_model(m, 250, 100)
    kw = dict(region="box", half=(2.0, 1.5, 2.5), pose=qr.CALLER_POSE)
    want = check(f, "box", **kw)
    n = want["stats"]["n_selected"]
    assert n > 1
    arrays = {name: np.full((n, k) if k > 1 else (n,), 77, dt) for name, k, dt in binding.SURFEL_FIELDS}
    index = np.full(n, 77, np.int32)
    with pytest.raises(binding.SsfError, match=r"\(-4\)") as e:
        f.query_rows_into(arrays, index, n - 1, **kw)
    same_stats(e.value.stats, want["stats"], "stats of the refused call")
    assert (index == 77).all() and all((a == 77).all() for a in arrays.values())
    st = f.query_rows_into(arrays, index, n, **kw)
    same_stats(st, want["stats"], "capacity == n_selected")
    util.assert_same_bits(index, want["index"], "index")
    for name in arrays:
        util.assert_same_bits(arrays[name], want[name], name)


def test_the_working_buffers_grow(product_lib):
    f = handle(product_lib, nb_supersurfels_max=30000)
    f.set_model(qr.hand_model(257, 0), 256, 100)
    check(f, "small", region="sphere", radius=2.5)
    f.set_model(qr.hand_model(30000, 1), 9000, 100)
    got = check(f, "select-all of 30000 rows")
    assert got["stats"]["n_selected"] == 30000
    check(f, "a region of the large model", region="frustum", pose=qr.CALLER_POSE)
    f.set_model(qr.hand_model(257, 2), 256, 100)
    check(f, "small again", region="box", half=(2.0, 1.5, 2.5))


def test_device_outputs_equal_the_host_outputs(fusion):
    import torch
    f = fusion
    f.set_model(qr.hand_model(1300, 0), 513, 100)
    kw = dict(region="frustum", pose=qr.CALLER_POSE)
    host = check(f, "host", **kw)
    n = host["stats"]["n_selected"]
    assert n > 0
    dev = {name: torch.full((n + 3, k) if k > 1 else (n + 3,), 7, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
           for name, k, dt in binding.SURFEL_FIELDS}
    index = torch.full((n + 3,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = f.query_model_device(dev, index=index, **kw)
    same_stats(st, host["stats"], "device stats")
    util.assert_same_bits(index.cpu().numpy()[:n], host["index"], "device index")
    assert bool((index[n:] == 7).all())
    for name, t in dev.items():
        util.assert_same_bits(t.cpu().numpy()[:n], host[name], "device " + name)
        assert bool((t[n:] == 7).all()), name
    # a subset: the others are not touched
    dev["colors"].fill_(9)
    dev["positions"].fill_(0)
    torch.cuda.synchronize()
    f.query_model_device({"positions": dev["positions"]}, **kw)
    util.assert_same_bits(dev["positions"].cpu().numpy()[:n], host["positions"], "device positions alone")
    assert bool((dev["colors"] == 9).all())


# ---- a store with holes --------------------------------------------------------------------------------------------------
def test_a_store_with_holes_and_its_compaction(product_lib):
    """30 frames of a camera that pans 3 degrees per frame for 15 frames and back (true pose as the prior): rows leave the view and
    come back, which leaves holes in the out-of-view span; compaction (ssf_debug_recentre) changes no result"""
    f = handle(product_lib, nb_supersurfels_max=20000)
    R0, t0 = synthetic.orbit_pose(0)
    recentres = f.debug_recentre_count()
    removed = reentered = 0
    prev_visible = 0
    for k in range(30):
        deg = 3.0 * (k if k < 15 else 29 - k)
        rgb, depth, _ = synthetic.render(R0 @ qr.rot_y(deg), t0, W, H, noise=True, rng=np.random.default_rng(1000 + k))
        r = f.process_frame(rgb, depth, prior_pose=qr.pose_about(qr.rot_y(deg), np.zeros(3)))
        removed += r["n_removed"]
        # more visible rows than the frame can account for by insertion: rows came back from the out-of-view store
        reentered += max(0, r["n_visible"] - prev_visible - r["n_inserted"])
        prev_visible = r["n_visible"]
    cnt = f.counts()
    assert cnt["n_model"] > cnt["n_visible"] > 0, cnt
    # (no getter exposes the out-of-view span: the store has not been compacted, and rows have left it)
    assert f.debug_recentre_count() == recentres
    assert removed > 0 or reentered > 0, (removed, reentered)
    p = f.get_pose()
    R, t = p[:9].reshape(3, 3).astype(np.float64), p[9:].astype(np.float64)
    look_back = qr.pose_about(R @ qr.rot_y(30.0), t)
    queries = [("everything", dict()), ("all", dict(t_last=(0, 27))), ("sphere", dict(region="sphere", radius=2.0)),
               ("box", dict(region="box", half=(1.0, 0.6, 2.0), pose=look_back)), ("frustum", dict(region="frustum")),
               ("frustum look back", dict(region="frustum", pose=look_back)),
               ("frustum visible", dict(region="frustum", visible_only=True))]
    before = {name: check(f, "holes " + name, **kw) for name, kw in queries}
    # (rows of the out-of-view span, holes between them, get their logical indices from the scan of the live counts)
    assert before["everything"]["stats"]["n_selected"] - before["everything"]["stats"]["n_selected_visible"] == cnt["n_model"] - cnt["n_visible"]
    model = f.get_model()
    f.debug_recentre()
    assert f.debug_recentre_count() == recentres + 1
    for name, kw in queries:
        after = check(f, "compacted " + name, **kw)
        util.assert_same_bits(after["index"], before[name]["index"], "compacted index " + name)
        same_stats(after["stats"], before[name]["stats"], "compacted " + name)
        for field in ALL_FIELDS:
            util.assert_same_bits(after[field], before[name][field], "compacted %s %s" % (name, field))
    for name, a in f.get_model().items():
        util.assert_same_bits(a, model[name], "model after compaction " + name)


# ---- no side effects ---------------------------------------------------------------------------------------------------
def test_a_query_changes_no_later_result(product_lib):
    A, B = handle(product_lib), handle(product_lib)
    look_back = qr.pose_about(*synthetic.relative_pose(0))
    for k in range(0, 36, 3):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        A.query_model(min_conf=A.cfg.conf_thresh)
        A.query_model(region="sphere", radius=1.0, fields=("positions",))
        A.query_model(region="box", half=(0.5, 0.5, 3.0), pose=look_back, visible_only=True)
        A.query_model(region="frustum", pose=look_back)
        A.query_count(region="frustum")
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)


# ---- refusals, profiling ---------------------------------------------------------------------------------------------------
def test_the_refusals(product_lib):
    f = handle(product_lib)
    f.process_frame(*util.frame(0, W, H))
    K, _ = cam_of(f)
    nan, inf = float("nan"), float("inf")
    bad = [dict(region=4), dict(region=-1),
           dict(region="sphere", radius=-1.0), dict(region="sphere", radius=nan), dict(region="sphere", radius=inf),
           dict(region="box", half=(1.0, -1.0, 1.0)), dict(region="box", half=(nan, 1.0, 1.0)), dict(region="box", half=(1.0, 1.0, inf)),
           dict(region="frustum", camera=dict(K, width=4097)), dict(region="frustum", camera=dict(K, height=0)),
           dict(region="frustum", camera=dict(K, width=-3)),
           dict(region="frustum", camera=dict(K, fx=0.0)), dict(region="frustum", camera=dict(K, fy=nan)),
           dict(region="frustum", camera=dict(K, fx=inf)),
           dict(region="frustum", z_range=(0.0, 1.0)), dict(region="frustum", z_range=(-1.0, 1.0)),
           dict(region="frustum", z_range=(2.0, 2.0)), dict(region="frustum", z_range=(3.0, 1.0)),
           dict(t_init=(5, 4)), dict(t_last=(1, 0))]
    one = {"positions": np.zeros((1, 3), np.float32)}
    for kw in bad:
        with pytest.raises(binding.SsfError, match=r"ssf_query_count failed \(-1\)"):
            f.query_count(**kw)
        with pytest.raises(binding.SsfError, match=r"ssf_query_rows failed \(-1\)"):
            f.query_rows_into(one, None, 1, **kw)
    L = product_lib.lib
    p, st = binding.SsfQueryParams(), binding.SsfQueryStats()
    assert L.ssf_query_default_params(f.h, binding.C.byref(p)) == 0
    idx = np.zeros(4, np.int32)
    surf = binding.SsfSurfels()
    assert L.ssf_query_default_params(None, binding.C.byref(p)) == -1 and L.ssf_query_default_params(f.h, None) == -1
    assert L.ssf_query_count(None, binding.C.byref(p), binding.C.byref(st)) == -1          # a NULL handle
    assert L.ssf_query_count(f.h, None, binding.C.byref(st)) == -1                         # NULL params
    assert L.ssf_query_count(f.h, binding.C.byref(p), None) == -1                          # NULL stats
    assert L.ssf_query_rows(None, binding.C.byref(p), None, binding._ptr(idx), 4, None) == -1
    assert L.ssf_query_rows(f.h, None, None, binding._ptr(idx), 4, None) == -1
    assert L.ssf_query_rows(f.h, binding.C.byref(p), None, None, 4, binding.C.byref(st)) == -1             # both outputs NULL
    assert L.ssf_query_rows(f.h, binding.C.byref(p), binding.C.byref(surf), None, 4, binding.C.byref(st)) == -1   # ... every array NULL
    assert L.ssf_query_rows(f.h, binding.C.byref(p), None, binding._ptr(idx), -1, binding.C.byref(st)) == -1      # a negative capacity
    # the handle keeps working: a query and a frame after the refusals
    check(f, "after the refusals", region="frustum")
    f.process_frame(*util.frame(1, W, H))
    check(f, "after a frame", region="sphere", radius=1.0)
    d = f.query_default_params()
    assert d["min_conf"] == 0.0 and d["region"] == 0 and d["t_init_min"] == -2 ** 31 and d["t_last_max"] == 2 ** 31 - 1
    assert d["radius"] == 0.0 and d["half"] == [0.0, 0.0, 0.0] and d["width"] == 0 and d["on_device"] == 0 and d["visible_only"] == 0
    # a sharded handle is not queried
    g = handle(product_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.query_count()
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.query_model()
    # a pipelined handle with a frame pending
    q = handle(product_lib, pipeline_depth=2, extract_batch=2)
    q.submit_frame(*util.frame(0, W, H))
    assert q.pending_frames() > 0
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q.query_count()
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q.query_rows_into(one, None, 1)
    q.process_submitted()
    assert q.pending_frames() == 0
    check(q, "pipelined, at rest", region="frustum")


def test_query_kernels_are_timed_under_profile(product_lib):
    f = handle(product_lib, profile=1)
    f.process_frame(*util.frame(0, W, H))
    f.reset_kernel_times()
    assert f.query_model()["stats"]["n_selected"] > 0
    names = f.kernel_times()
    for k in ("query_select", "query_scan", "query_gather"):
        assert k in names and names[k][1] > 0, (k, names)


# ---- the C++ surface -----------------------------------------------------------------------------------------------------
def test_extract_local_point_cloud_in_cpp(product_lib, tmp_path):
    """tests/cpp/query_smoke.cpp on the GPU: the row count and the FNV-1a checksum of the positions of its radius-1.5 m local
    cloud equal those of the Python query of the same map (the program's six frames, reproduced here)"""
    libdir = os.path.dirname(product_lib.path)
    exe = str(tmp_path / "query_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "query_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    got = re.search(r"local_cloud rows=(\d+) fnv=([0-9a-f]{16}) colors=(\d+) normals=(\d+)", r.stdout)
    assert got, r.stdout
    # the same six frames through the binding: initialize(cam, 16, 10, 1000, 1000, 1e8) with the pre-filter off
    # (every argument of SupersurfelFusion::initialize, at its default where the program names none)
    cfg = product_lib.default_config(width=W, height=H, fx=150.0, fy=150.0, cx=79.5, cy=63.5, cell_size=16, lambda_pos=10.0,
                                     lambda_bound=1000.0, lambda_size=1000.0, lambda_disp=1e8, thresh_disp=1e-4, seg_iter=10,
                                     seg_use_ransac=1, nb_samples=16, filter_iter=4, filter_alpha=0.1, filter_beta=1.0,
                                     filter_threshold=0.05, range_min=0.2, range_max=5.0, delta_t=20, conf_thresh=2500.0,
                                     nb_supersurfels_max=50000, icp_iter=10, icp_cov_thresh=0.04, pipeline_depth=0,
                                     extract_batch=1, depth_prefilter=0)
    f = binding.Fusion(product_lib, cfg)
    i = np.arange(W * H)
    for k in range(6):
        x, y = (i % W) + 2 * k, i // W
        rgb = np.stack([x * 255 // (W + 16), y * 255 // H, (x ^ y) & 255], axis=1).astype(np.uint8).reshape(H, W, 3)
        depth = (np.float32(1.0) + np.float32(0.004) * x.astype(np.float32)).astype(np.float32).reshape(H, W)
        f.process_frame(rgb, depth)
    want = check(f, "python local cloud", region="sphere", radius=1.5)
    fnv = 1469598103934665603
    for b in np.ascontiguousarray(want["positions"]).tobytes():
        fnv = ((fnv ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    n = want["stats"]["n_selected"]
    assert n > 0
    assert (int(got.group(1)), got.group(2), int(got.group(3)), int(got.group(4))) == (n, "%016x" % fnv, n, n), r.stdout
