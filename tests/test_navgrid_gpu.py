"""ssf_navgrid_build (include/ssf_navgrid.h) on the MI355X against the numpy restatement (tests/navgrid_ref.py): every output and
every stat at 0 bits -- on hand-built models at the wave and block edges of both stores, grids at the tile edges, boundary-exact
rows with hand-written answers, contention in one cell, a store with holes (before and after its compaction); plus output
subsets, device outputs, growth, no side effects on the frame path, the refusals, profiling and the C++ surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import navgrid_ref as nr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay, synthetic

pytestmark = pytest.mark.gpu
W, H = 160, 128
CPP = os.path.join(ROOT, "tests", "cpp")


def handle(lib, **kw):
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


def same_grid(got, want, what, outputs=nr.OUTPUTS):
    for name in outputs:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name, got[name].shape, got[name].dtype)
        util.assert_same_bits(got[name], want[name], what + " " + name)
    for k in nr.STATS:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"][k], want["stats"][k])


def check(f, what, frame=None, model=None, outputs=nr.OUTPUTS, **kw):
    """the grid on the device and in numpy from get_model's rows; frame: None (the default frame), 'caller' or 12 floats.  Returns the
    device result"""
    model = f.get_model() if model is None else model
    q = nr.params(**kw)
    pose = nr.caller_pose(q) if isinstance(frame, str) else frame
    used = nr.default_pose(f.get_pose(), q) if pose is None else np.asarray(pose, np.float32)
    want = nr.build(model, f.counts()["n_visible"], used, q)
    got = f.nav_grid(outputs=outputs, pose=pose, **kw)
    assert sorted(got) == sorted(tuple(outputs) + ("stats",)), what
    same_grid(got, want, what, outputs)
    util.assert_same_bits(got["stats"]["pose"], used, what + " the frame used")
    assert got["stats"]["list_entries"] >= 0
    return got


@pytest.fixture(scope="module")
def fusion(product_lib):
    """one handle for the tests that replace the model through set_model"""
    f = handle(product_lib)
    yield f
    f.close()


# ---- hand-built models, every grid size -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nv", nr.SIZES)
def test_hand_built_models(n, nv, fusion):
    f = fusion
    for seed in nr.SEEDS:
        m = nr.hand_model(n, seed)
        f.set_model(m, nv, 100)
        model = f.get_model()
        for name in m:
            util.assert_same_bits(model[name], m[name], "set_model / get_model " + name)
        for gw, gh, res in nr.GRIDS:
            # every kind of case on one seed, two of them (one per frame) on the others
            cases = nr.grid_cases(gw, gh, res)
            for name, frame, kw in (cases if seed == 0 else cases[2 * seed:2 * seed + 2] + cases[7 - 2 * seed:8 - 2 * seed]):
                check(f, "n %d nv %d seed %d grid %dx%d %s" % (n, nv, seed, gw, gh, name), frame=frame, model=model, **kw)


def test_boundary_exact_rows(fusion):
    f = fusion
    m, kw, cases = nr.boundary_rows()
    for name, rows, want in cases:
        sub = {k: np.ascontiguousarray(v[rows]) for k, v in m.items()}
        f.set_model(sub, len(rows), 100)
        util.assert_same_bits(f.get_model()["positions"], sub["positions"], "positions (-0 survives set_model)")
        got = check(f, name, frame=nr.BOUNDARY_POSE, model=sub, **kw)
        nr.check_expectations(got, want, kw["width"], kw["height"], name)
    f.set_model(m, 6, 100)
    got = check(f, "all boundary rows", frame=nr.BOUNDARY_POSE, model=m, **kw)
    assert got["state"][0].tolist() == [-1, 100, 100, -1, 0, 0, 0, 0]
    assert got["dist2"][0].tolist() == [1, 0, 0, 1, 1, 2, 1, 2]
    check(f, "the visible boundary rows", frame=nr.BOUNDARY_POSE, model=m, visible_only=True, **kw)


def test_contention_in_one_cell(fusion):
    """1300 rows at one position: every sample of every row lands in the same few cells; the counts are exact"""
    f = fusion
    m = nr.hand_model(1300, 0)
    m["positions"][:] = m["positions"][0]
    m["orientations"][:] = m["orientations"][0]
    m["dims"][:] = m["dims"][0]
    f.set_model(m, 513, 100)
    got = check(f, "1300 rows at one position", frame="caller", model=m, width=33, height=31, res=0.05)
    assert got["stats"]["rows_used"] == 1300 and got["stats"]["samples_in_grid"] == got["stats"]["samples"]
    assert int(got["hits"].sum()) == got["stats"]["samples"] and got["hits"].max() >= 1300
    assert np.array_equal(got["hits"][..., 0] % 1300, np.zeros_like(got["hits"][..., 0]))


def test_an_empty_selection(fusion):
    f = fusion
    f.set_model(nr.hand_model(257, 0), 256, 100)
    for unknown, d in ((False, 49), (True, 0)):
        got = check(f, "nothing selected", frame="caller", width=33, height=31, res=0.05, min_conf=1e9, max_dist_cells=7, unknown_is_obstacle=unknown)
        assert (got["state"] == -1).all() and (got["dist2"] == d).all() and not got["hits"].any()
        assert np.isposinf(got["zmin"]).all() and np.isneginf(got["zmax"]).all()
        assert got["stats"]["rows_used"] == 0 and got["stats"]["samples"] == 0 and got["stats"]["cells_unknown"] == 33 * 31


def test_a_disc_half_outside_the_grid_and_rows_that_are_not_used(fusion):
    f = fusion
    m = nr.hand_model(64, 1)
    q = dict(width=33, height=31, res=0.05, z_min=-1.0, z_max=1.0, floor_max=0.0)
    # rows 0..3: horizontal discs of half-axis 0.16 m centred on the four edges of the 1.65 m x 1.55 m grid (identity frame)
    for k, c in enumerate(((0.0, 0.7, -0.5), (1.65, 0.7, -0.5), (0.8, 0.0, 0.5), (0.8, 1.55, 0.5))):
        m["positions"][k] = c
        m["orientations"][k] = (1, 0, 0, 0, 1, 0, 0, 0, 1)
        m["dims"][k] = (0.0064, 0.0064)
    m["positions"][4:, :2] = np.abs(m["positions"][4:, :2]) % 1.5
    m["positions"][4:, 2] = np.clip(m["positions"][4:, 2], -0.9, 0.9)
    nan, inf = np.nan, np.inf
    for k, (field, value) in enumerate((("positions", (nan, 0.5, 0.0)), ("positions", (0.5, inf, 0.0)), ("positions", (0.5, 0.5, -inf)),
                                        ("dims", (0.0, 0.01)), ("dims", (0.01, -1.0)), ("dims", (nan, 0.01)), ("dims", (0.01, inf)),
                                        ("orientations", (nan, 0, 0, 0, 1, 0, 0, 0, 1)), ("orientations", (1, 0, 0, 0, inf, 0, 0, 0, 1)),
                                        ("orientations", (1, 0, 0, 0, 1, 0, 0, 0, nan)))):
        m[field][10 + k] = value
    f.set_model(m, 40, 100)
    model = f.get_model()
    util.assert_same_bits(model["positions"], m["positions"], "positions (NaN and inf survive set_model)")
    got = check(f, "discs on the grid's edges", frame=nr.IDENTITY, model=model, **q)
    assert got["stats"]["rows_used"] == 64 - 7                       # three positions and four dims are refused; the orientations are not
    alone = {k: np.ascontiguousarray(v[:4]) for k, v in m.items()}
    f.set_model(alone, 4, 100)
    got = check(f, "the four edge discs alone", frame=nr.IDENTITY, model=alone, **q)
    assert 0.3 * got["stats"]["samples"] < got["stats"]["samples_in_grid"] < 0.7 * got["stats"]["samples"], got["stats"]


def test_output_subsets_and_two_calls_in_a_row(fusion):
    f = fusion
    m = nr.hand_model(1300, 2)
    f.set_model(m, 513, 100)
    kw = dict(width=65, height=64, res=0.05, max_dist_cells=9)
    full = check(f, "all outputs", frame="caller", model=m, **kw)
    again = f.nav_grid(pose=nr.caller_pose(nr.params(**kw)), **kw)
    same_grid(again, full, "the second call")
    assert again["stats"]["list_entries"] == full["stats"]["list_entries"]
    for outputs in (("dist2",), ("state",), ("zmin", "zmax"), ("hits", "dist2"), ("zmax",)):
        got = check(f, "outputs %s" % (outputs,), frame="caller", model=m, outputs=outputs, **kw)
        for name in outputs:
            util.assert_same_bits(got[name], full[name], "subset " + name)
    with pytest.raises(binding.SsfError, match="unknown navigation grid outputs"):
        f.nav_grid(outputs=("depth",))


def test_device_outputs_equal_the_host_outputs(fusion):
    import torch
    f = fusion
    m = nr.hand_model(1300, 1)
    f.set_model(m, 513, 100)
    kw = dict(width=65, height=64, res=0.05, unknown_is_obstacle=True, max_dist_cells=5)
    pose = nr.caller_pose(nr.params(**kw))
    host = check(f, "host", frame=pose, model=m, **kw)
    P = 65 * 64
    dev = {name: torch.full((P * (2 if name == "hits" else 1) + 3,), 7, dtype={"uint32": torch.int32}.get(np.dtype(dt).name) or
                            getattr(torch, np.dtype(dt).name), device="cuda") for name, dt, _ in binding.NAVGRID_OUTPUTS}
    torch.cuda.synchronize()
    st = f.nav_grid_device(pose=pose, **dict(kw, **dev))
    for k in nr.STATS + ("list_entries",):
        assert st[k] == host["stats"][k], k
    for name, t in dev.items():
        a = t.cpu().numpy()
        util.assert_same_bits(a[:-3].view(host[name].dtype).reshape(host[name].shape), host[name], "device " + name)
        assert (a[-3:] == 7).all(), name
    # dist2 alone into device memory: the others are not touched
    for t in dev.values():
        t.fill_(9)
    torch.cuda.synchronize()
    f.nav_grid_device(dist2=dev["dist2"], pose=pose, **kw)
    util.assert_same_bits(dev["dist2"].cpu().numpy()[:-3].reshape(64, 65), host["dist2"], "device dist2 alone")
    assert all(bool((dev[name] == 9).all()) for name in ("zmin", "zmax", "hits", "state"))


# ---- a store with holes --------------------------------------------------------------------------------------------------
def test_a_store_with_holes_and_its_compaction(product_lib):
    """30 frames of a camera that pans 3 degrees per frame for 15 frames and back (true pose as the prior): rows leave the view and
    come back, which leaves holes in the out-of-view span; compaction (ssf_debug_recentre) changes no result"""
    f = handle(product_lib, nb_supersurfels_max=20000)
    R0, t0 = synthetic.orbit_pose(0)
    rot_y = lambda deg: nr.rot("y", deg)
    recentres = f.debug_recentre_count()
    removed = reentered = 0
    prev_visible = 0
    for k in range(30):
        deg = 3.0 * (k if k < 15 else 29 - k)
        rgb, depth, _ = synthetic.render(R0 @ rot_y(deg), t0, W, H, noise=True, rng=np.random.default_rng(1000 + k))
        r = f.process_frame(rgb, depth, prior_pose=nr.pose_about(rot_y(deg), np.zeros(3)))
        removed += r["n_removed"]
        reentered += max(0, r["n_visible"] - prev_visible - r["n_inserted"])
        prev_visible = r["n_visible"]
    cnt = f.counts()
    assert cnt["n_model"] > cnt["n_visible"] > 0, cnt
    assert f.debug_recentre_count() == recentres
    assert removed > 0 or reentered > 0, (removed, reentered)
    model = f.get_model()
    lo, hi = model["positions"].min(axis=0), model["positions"].max(axis=0)
    # a frame of the caller's whose bands split the scene's heights in the middle, and the default frame with bands about the scene
    mid = float(0.5 * (lo[1] + hi[1]))
    grids = [("default frame", None, dict(width=96, height=96, res=0.05, z_min=-hi[1] - 0.1, z_max=-lo[1] + 0.1, floor_max=-mid)),
             ("visible", None, dict(width=96, height=96, res=0.05, z_min=-hi[1] - 0.1, z_max=-lo[1] + 0.1, floor_max=-mid, visible_only=True)),
             ("coarse cells", None, dict(width=33, height=31, res=0.15, z_min=-hi[1] - 0.1, z_max=-lo[1] + 0.1, floor_max=-mid, floor_cos=0.0))]
    before = {name: check(f, "holes " + name, frame=frame, model=model, **kw) for name, frame, kw in grids}
    assert before["default frame"]["stats"]["rows_used"] > before["visible"]["stats"]["rows_used"] > 0
    assert before["default frame"]["stats"]["cells_occupied"] > 0 and before["coarse cells"]["stats"]["cells_free"] > 0
    f.debug_recentre()
    assert f.debug_recentre_count() == recentres + 1
    for name, frame, kw in grids:
        after = check(f, "compacted " + name, frame=frame, **kw)
        same_grid(after, before[name], "compacted against holes " + name)
    for name, a in f.get_model().items():
        util.assert_same_bits(a, model[name], "model after compaction " + name)


# ---- growth, no side effects -------------------------------------------------------------------------------------------------
def test_the_working_buffers_grow(product_lib):
    f = handle(product_lib, nb_supersurfels_max=30000)
    f.set_model(nr.hand_model(257, 0), 256, 100)
    check(f, "small model, small grid", frame="caller", width=7, height=5, res=0.2)
    check(f, "small model, larger grid", frame="caller", width=130, height=97, res=0.03)
    f.set_model(nr.hand_model(30000, 1, extent=3.0), 9000, 100)
    got = check(f, "large model", frame="caller", width=130, height=97, res=0.05)
    assert got["stats"]["rows_used"] == 30000
    f.set_model(nr.hand_model(257, 2), 256, 100)
    check(f, "small again", width=33, height=31, res=0.05)
    # more tiles than the workgroups' LDS histograms hold (46 x 46 > 2048): counts and list entries go to the global counters one by one
    got = check(f, "a grid of 2116 tiles", frame="caller", width=1472, height=1472, res=0.0025, max_steps=16, max_dist_cells=2)
    assert got["stats"]["samples_in_grid"] > 0


def test_a_grid_changes_no_later_result(product_lib):
    A, B = handle(product_lib), handle(product_lib)
    for k in range(0, 36, 3):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        A.nav_grid(width=96, height=80)
        A.nav_grid(outputs=("dist2",), z_min=-5.0, z_max=5.0, floor_max=0.0, unknown_is_obstacle=True, visible_only=True)
        A.nav_grid(pose=nr.caller_pose(nr.params(width=33, height=31)), width=33, height=31, min_conf=A.cfg.conf_thresh)
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)


# ---- refusals, profiling ---------------------------------------------------------------------------------------------------
def test_the_refusals(product_lib):
    f = handle(product_lib)
    f.process_frame(*util.frame(0, W, H))
    nan, inf = float("nan"), float("inf")
    small = dict(width=16, height=16)
    bad = [dict(width=0), dict(width=4097), dict(height=0), dict(height=4097), dict(width=-3),
           dict(res=0.0), dict(res=-0.05), dict(res=nan), dict(res=inf),
           dict(splat_scale=-1.0), dict(splat_scale=nan), dict(splat_scale=inf),
           dict(max_steps=0), dict(max_steps=17), dict(max_dist_cells=0), dict(max_dist_cells=1025), dict(min_hits=0), dict(min_hits=-2),
           dict(z_min=1.0, z_max=0.5), dict(z_min=nan), dict(z_max=nan),
           dict(t_init=(5, 4)), dict(t_last=(1, 0)), dict(floor_cos=-0.1), dict(floor_cos=1.5), dict(floor_cos=nan)]
    for kw in bad:
        with pytest.raises(binding.SsfError, match=r"ssf_navgrid_build failed \(-1\)"):
            f.nav_grid(**dict(small, **kw))
    with pytest.raises(binding.SsfError, match=r"ssf_navgrid_build failed \(-1\)"):
        f.nav_grid(outputs=(), **small)                                # every output NULL
    L = product_lib.lib
    p, st, out = binding.SsfNavGridParams(), binding.SsfNavGridStats(), binding.SsfNavGridOut()
    byref = binding.C.byref
    assert L.ssf_navgrid_default_params(f.h, byref(p)) == 0
    assert L.ssf_navgrid_default_params(None, byref(p)) == -1 and L.ssf_navgrid_default_params(f.h, None) == -1
    state = np.zeros((512, 512), np.int8)
    out.state = state.ctypes.data
    assert L.ssf_navgrid_build(None, byref(p), byref(out), byref(st)) == -1        # a NULL handle
    assert L.ssf_navgrid_build(f.h, None, byref(out), byref(st)) == -1             # NULL params
    assert L.ssf_navgrid_build(f.h, byref(p), None, byref(st)) == -1               # no outputs at all
    assert L.ssf_navgrid_build(f.h, byref(p), byref(binding.SsfNavGridOut()), byref(st)) == -1
    assert L.ssf_navgrid_build(f.h, byref(p), byref(out), None) == 0               # stats are optional
    pose = np.zeros(12, np.float32)
    assert L.ssf_navgrid_default_pose(f.h, byref(p), None) == -1 and L.ssf_navgrid_default_pose(None, byref(p), binding._ptr(pose)) == -1
    # splat_scale 0 means the default
    util.assert_same_bits(f.nav_grid(splat_scale=0.0, **small)["hits"], f.nav_grid(splat_scale=2.0, **small)["hits"], "splat_scale 0")
    # the handle keeps working: a grid and a frame after the refusals
    check(f, "after the refusals", width=96, height=80)
    f.process_frame(*util.frame(1, W, H))
    check(f, "after a frame", width=96, height=80, z_min=-5.0, z_max=5.0, floor_max=0.0)
    d = f.nav_grid_default_params()
    assert (d["width"], d["height"], d["max_steps"], d["min_hits"], d["max_dist_cells"]) == (512, 512, 8, 1, 40)
    assert (d["res"], d["z_min"], d["z_max"], d["floor_max"], d["floor_cos"], d["splat_scale"]) == \
           tuple(np.float32(v) for v in (0.05, -1.5, 0.5, -0.8, 0.8, 2.0))
    assert d["min_conf"] == 0.0 and d["t_init_min"] == -2 ** 31 and d["t_last_max"] == 2 ** 31 - 1
    assert d["visible_only"] == 0 and d["unknown_is_obstacle"] == 0 and d["on_device"] == 0
    util.assert_same_bits(f.nav_grid_default_pose(width=96, height=80), nr.default_pose(f.get_pose(), nr.params(width=96, height=80)),
                          "ssf_navgrid_default_pose")
    # a sharded handle has no grid
    g = handle(product_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_grid(**small)
    # a pipelined handle with a frame pending
    q = handle(product_lib, pipeline_depth=2, extract_batch=2)
    q.submit_frame(*util.frame(0, W, H))
    assert q.pending_frames() > 0
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q.nav_grid(**small)
    q.process_submitted()
    assert q.pending_frames() == 0
    check(q, "pipelined, at rest", width=96, height=80)


def test_navgrid_kernels_are_timed_under_profile(product_lib):
    f = handle(product_lib, profile=1)
    f.process_frame(*util.frame(0, W, H))
    f.reset_kernel_times()
    assert f.nav_grid(width=96, height=80, z_min=-5.0, z_max=5.0, floor_max=0.0)["stats"]["samples_in_grid"] > 0
    names = f.kernel_times()
    for k in ("navgrid_prep", "navgrid_fill", "navgrid_tile", "navgrid_cells", "navgrid_columns", "navgrid_rows"):
        assert k in names and names[k][1] > 0, (k, names)


# ---- replay.py's files -----------------------------------------------------------------------------------------------------
def test_replay_writes_the_grid_in_map_servers_convention(product_lib, tmp_path):
    f = handle(product_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    replay.replay(f, frames, nav_grid_dir=str(tmp_path), nav_grid_every=2, nav_grid_res=0.1)
    assert sorted(os.listdir(str(tmp_path))) == ["000000.pgm", "000000.yaml", "000000_dist2.npy", "000002.pgm", "000002.yaml", "000002_dist2.npy"]
    want = f.nav_grid(outputs=("state", "dist2"), res=0.1)            # the map after the last frame = what frame 2's files show
    raw = open(str(tmp_path / "000002.pgm"), "rb").read()
    assert raw.startswith(b"P5\n512 512\n255\n")
    img = np.frombuffer(raw[len(b"P5\n512 512\n255\n"):], np.uint8).reshape(512, 512)[::-1]
    assert np.array_equal(img == 0, want["state"] == 100) and np.array_equal(img == 254, want["state"] == 0)
    assert np.array_equal(img == 205, want["state"] == -1)
    util.assert_same_bits(np.load(str(tmp_path / "000002_dist2.npy")), want["dist2"], "dist2.npy")
    yaml = open(str(tmp_path / "000002.yaml")).read()
    t = want["stats"]["pose"][9:]
    assert "image: 000002.pgm\n" in yaml and "resolution: 0.1\n" in yaml and "negate: 0\n" in yaml
    assert "origin: [%.9g, %.9g, 0.0]\n" % (t[0], t[2]) in yaml, yaml


# ---- the C++ surface -----------------------------------------------------------------------------------------------------
def test_build_nav_grid_in_cpp(product_lib, tmp_path):
    """tests/cpp/navgrid_smoke.cpp on the GPU: the counts and the FNV-1a checksums of its grid's state, dist2 and hits equal those
    of the Python call on the same map (the program's six frames, reproduced here)"""
    libdir = os.path.dirname(product_lib.path)
    exe = str(tmp_path / "navgrid_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "navgrid_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    got = re.search(r"navgrid 64x64 rows=(\d+) samples=(\d+) in_grid=(\d+) free=(\d+) occupied=(\d+) unknown=(\d+) state=([0-9a-f]{16}) "
                    r"dist2=([0-9a-f]{16}) hits=([0-9a-f]{16})", r.stdout)
    assert got, r.stdout
    assert "occupancy 64x64 res=0.050 origin=(-1.60 -1.60 0.00)" in r.stdout and "data=4096" in r.stdout, r.stdout
    assert "dist2_alone 1536 state=0 zmin=0" in r.stdout, r.stdout
    # the same six frames through the binding: initialize(cam, 16, 10, 1000, 1000, 1e8) with the pre-filter off
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
    frame = np.array([0, 1, 0, 1, 0, 0, 0, 0, -1, -1.6, -1.6, 0], np.float32)
    want = check(f, "python grid", frame=frame, width=64, height=64, res=0.05, z_min=-2.0, floor_max=-1.3, z_max=0.0, max_dist_cells=12)
    s = want["stats"]
    assert s["cells_free"] > 0 and s["cells_occupied"] > 0 and s["cells_unknown"] > 0, s

    def fnv(a):
        h = 1469598103934665603
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return "%016x" % h
    assert tuple(int(v) for v in got.groups()[:6]) == (s["rows_used"], s["samples"], s["samples_in_grid"], s["cells_free"], s["cells_occupied"],
                                                       s["cells_unknown"]), r.stdout
    assert got.groups()[6:] == (fnv(want["state"]), fnv(want["dist2"]), fnv(want["hits"])), r.stdout
