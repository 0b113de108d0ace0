"""ssf_navgrid_carve (include/ssf_navcarve.h) on the MI355X against the numpy restatement (tests/navcarve_ref.py): every output and
every stat at 0 bits (list_entries is informative) -- hand-built models at the wave and block edges of both stores, ray counts and
sample counts at the wave edges, grids at the tile edges, the wall scene, boundary cases with hand-written answers, contention, a
store with holes; plus no views, parameter variants, output subsets, device outputs, chunking, index reuse, no side effects on the
frame path, the refusals, growth, profiling, replay's files and the C++ surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import navcarve_ref as nc
import navgrid_ref as nr
import raycast_ref as rr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay, synthetic

pytestmark = pytest.mark.gpu
W, H = 160, 128
CPP = os.path.join(ROOT, "tests", "cpp")
RANGE = dict(t_min=0.05, t_max=8.0)


def handle(lib, **kw):
    """a handle of a test's own, which the test closes when it is done with it"""
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


def cfg_camera(f):
    return dict(fx=f.cfg.fx, fy=f.cfg.fy, cx=f.cfg.cx, cy=f.cfg.cy, width=f.cfg.width, height=f.cfg.height)


def same(got, want, what, outputs=nc.OUTPUTS):
    for name in outputs:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name, got[name].shape, got[name].dtype)
        util.assert_same_bits(got[name], want[name], what + " " + name)
    for k in nc.GRID_STATS + nc.RAY_STATS:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"][k], want["stats"][k])


def check(f, what, views, carve, frame=None, model=None, outputs=nc.OUTPUTS, **kw):
    """the carved grid on the device and in numpy from get_model's rows; frame: None (the default frame), 'caller' or 12 floats.
    Returns the device result"""
    model = f.get_model() if model is None else model
    q = nr.params(**kw)
    pose = nr.caller_pose(q) if isinstance(frame, str) else frame
    used = nr.default_pose(f.get_pose(), q) if pose is None else np.asarray(pose, np.float32)
    want = nc.carve(model, f.counts()["n_visible"], used, q, views, nc.params(cfg_camera=cfg_camera(f), **carve))
    got = f.nav_grid_carve(views, outputs=outputs, carve=carve, pose=pose, **kw)
    assert sorted(got) == sorted(tuple(outputs) + ("stats",)), what
    same(got, want, what, outputs)
    util.assert_same_bits(got["stats"]["pose"], used, what + " the frame used")
    assert got["stats"]["list_entries"] >= 0 and got["stats"]["ray_entries"] >= f.debug_navcarve_last()["atomics"] >= 0
    return got


def scene_views(n, seed=0):
    """n camera poses inside hand_model's box, about a metre above its floor, looking around and slightly down"""
    rng = np.random.default_rng(40 + seed)
    return np.stack([nr.pose_about(nr.rot("y", rng.uniform(0, 360)) @ nr.rot("x", rng.uniform(-25, 10)),
                                   (rng.uniform(-0.6, 0.6), rng.uniform(-0.1, 0.3), rng.uniform(-0.6, 0.6))) for _ in range(n)])


def lattice_camera(cw, ch, stride):
    return dict(fx=0.9 * max(cw, ch, 8), fy=0.9 * max(cw, ch, 8), cx=0.5 * (cw - 1), cy=0.5 * (ch - 1), cam_width=cw, cam_height=ch, stride=stride)


@pytest.fixture(scope="module")
def carve_lib():
    """libssf_hip_navcarve.so: the product's objects plus the carve's entry points (no fallback: a missing .so is an error)"""
    return binding.load_navcarve()


@pytest.fixture(scope="module")
def fusion(carve_lib):
    """one handle for the tests that replace the model through set_model"""
    f = handle(carve_lib)
    yield f
    f.close()


# ---- wave, block and tile edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nv", nr.SIZES)
def test_hand_built_models_ray_counts_and_grids(n, nv, fusion):
    f = fusion
    m = nr.hand_model(n, 0)
    f.set_model(m, nv, 100)
    model = f.get_model()
    total = []
    for k, (cw, ch, stride, n_views) in enumerate(nc.RAY_LATTICES):
        gw, gh, frame = ((33, 31, None), (65, 64, "caller"))[k % 2]
        carve = dict(lattice_camera(cw, ch, stride), carve_misses=k % 3 == 0, **RANGE)
        got = check(f, "n %d nv %d lattice %s grid %dx%d" % (n, nv, (cw, ch, stride, n_views), gw, gh), scene_views(n_views, k), carve,
                    frame=frame, model=model, width=gw, height=gh, res=0.05)
        total.append(got["stats"]["rays"])
    assert total == [1, 63, 64, 65, 257, 1025]


@pytest.mark.parametrize("t_max,count", nc.SAMPLE_COUNTS)
def test_sample_counts_at_the_wave_edges(t_max, count, fusion):
    """a ray that misses and carves to t_max along a row of a 65 x 64 grid of 0.25 m cells: M + 1 = 1, 63, 64, 65, 129 samples"""
    f = fusion
    m, _, _ = nc.boundary_cases()
    f.set_model(m, 1, 100)
    view = nc.view_at(-nc.ALONG_X @ np.diag([1, -1, 1]), (16.125, 2.125, 0.5)).reshape(1, 12)           # y = 2.125: past the disc's rim, row 8
    carve = dict(nc.BOUNDARY_CAMERA, t_min=0.03125, t_max=t_max, carve_misses=True)
    kw = dict(nc.BOUNDARY_GRID, width=65, height=64)
    got = check(f, "t_max %g" % t_max, view, carve, frame=nr.IDENTITY, model=m, **kw)
    s = got["stats"]
    assert (s["rays"], s["rays_hit"], s["rays_carving"], s["ray_samples"]) == (1, 0, 1, count)
    # x = 16.125 - m / 8: gx = 64.5, 64, 63.5, 63, ...: two samples per cell from cell 64 down
    assert s["ray_entries"] == (count + 1) // 2 and (got["seen"][8, 65 - s["ray_entries"]:] == 1).all() and got["seen"].sum() == s["ray_entries"]


# ---- the fixed scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("carve_misses", [False, True])
def test_the_wall_scene(carve_misses, fusion):
    f = fusion
    m, n, pose, gkw, views, ckw = nc.wall_scene()
    f.set_model(m, n, 100)
    got = check(f, "wall scene", views, dict(ckw, carve_misses=carve_misses), frame=pose, model=m, **gkw)
    plain = f.nav_grid(pose=pose, **gkw)
    nc.check_wall(dict(got, uncarved=plain["state"]), carve_misses, "wall scene on the device")
    assert ((plain["state"] == 100) == (got["state"] == 100)).all()
    assert got["stats"]["cells_carved"] == int(((plain["state"] < 0) & (got["state"] == 0)).sum())


def test_boundary_cases_with_hand_written_answers(fusion):
    f = fusion
    m, gkw, cases = nc.boundary_cases()
    f.set_model(m, 1, 100)
    for name, views, carve, want in cases:
        got = check(f, name, views, carve, frame=nr.IDENTITY, model=m, **gkw)
        nc.check_expectations(got, want, gkw["width"], gkw["height"], name)


def test_contention_1025_identical_rays(fusion):
    f = fusion
    m, gkw, cases = nc.boundary_cases()
    f.set_model(m, 1, 100)
    name, view, carve, want = cases[0]
    got = check(f, "1025 identical rays", np.repeat(view, 1025, axis=0), carve, frame=nr.IDENTITY, model=m, **gkw)
    nc.check_expectations(dict(got, stats={}), dict(seen={k: 1025 for k in want["seen"]}), gkw["width"], gkw["height"], "1025 x " + name)
    assert got["stats"]["rays"] == got["stats"]["rays_hit"] == got["stats"]["rays_carving"] == 1025
    assert got["stats"]["ray_entries"] == 1025 * want["ray_entries"] and got["stats"]["cells_seen"] == want["cells_seen"]
    # consecutive rays share every cell: a wave merges what it adds to one address before the atomic
    assert f.debug_navcarve_last()["atomics"] < got["stats"]["ray_entries"]


# ---- no views, parameter variants --------------------------------------------------------------------------------------------
def test_no_views_is_the_uncarved_grid(fusion):
    f = fusion
    m = nr.hand_model(1300, 1)
    f.set_model(m, 513, 100)
    kw = dict(width=65, height=64, res=0.05, max_dist_cells=9)
    pose = nr.caller_pose(nr.params(**kw))
    plain = f.nav_grid(pose=pose, **kw)
    for views in (None, np.zeros((0, 12), np.float32)):
        got = f.nav_grid_carve(views, carve=RANGE, pose=pose, **kw)
        for name in nr.OUTPUTS:
            util.assert_same_bits(got[name], plain[name], "no views " + name)
        for k in nr.STATS + ("list_entries",):
            assert got["stats"][k] == plain["stats"][k], k
        util.assert_same_bits(got["stats"]["pose"], plain["stats"]["pose"], "pose")
        assert not got["seen"].any() and all(got["stats"][k] == 0 for k in nc.RAY_STATS)
    check(f, "no views against the restatement", np.zeros((0, 12), np.float32), RANGE, frame=pose, model=m, **kw)


@pytest.mark.parametrize("variant", [dict(min_seen=2), dict(hit_margin_cells=0.0), dict(hit_margin_cells=2.5), dict(ray_min_conf=nr.MIN_CONF),
                                     dict(ray_splat_scale=1.5, carve_misses=True), dict()])
def test_parameter_variants(variant, fusion):
    f = fusion
    m = nr.hand_model(1300, 2)
    f.set_model(m, 513, 100)
    carve = dict(stride=16, **RANGE) if not variant else dict(lattice_camera(64, 48, 4), **dict(RANGE, **variant))      # {}: the handle's camera
    got = check(f, "variant %s" % (variant,), scene_views(2, 7), carve, frame="caller", model=m, width=65, height=64, res=0.05, unknown_is_obstacle=True)
    assert got["stats"]["rays_hit"] > 0 and got["stats"]["ray_entries"] > 0


# ---- output handling ---------------------------------------------------------------------------------------------------------
def test_output_subsets_and_two_calls_in_a_row(fusion):
    f = fusion
    m = nr.hand_model(1300, 2)
    f.set_model(m, 513, 100)
    kw = dict(width=65, height=64, res=0.05, max_dist_cells=9)
    views, carve = scene_views(2, 3), dict(lattice_camera(64, 48, 4), **RANGE)
    full = check(f, "all outputs", views, carve, frame="caller", model=m, **kw)
    again = f.nav_grid_carve(views, carve=carve, pose=nr.caller_pose(nr.params(**kw)), **kw)
    same(again, full, "the second call")
    for outputs in (("seen",), ("dist2",), ("state", "seen"), ("zmin", "hits")):
        got = f.nav_grid_carve(views, outputs=outputs, carve=carve, pose=nr.caller_pose(nr.params(**kw)), **kw)
        assert sorted(got) == sorted(outputs + ("stats",))
        for name in outputs:
            util.assert_same_bits(got[name], full[name], "subset %s: %s" % (outputs, name))
        for k in nc.GRID_STATS + nc.RAY_STATS:
            assert got["stats"][k] == full["stats"][k], (outputs, k)
    with pytest.raises(binding.SsfError, match="unknown carved grid outputs"):
        f.nav_grid_carve(views, outputs=("depth",))


def test_device_outputs_with_guard_words(fusion):
    import torch
    f = fusion
    m = nr.hand_model(1300, 1)
    f.set_model(m, 513, 100)
    kw = dict(width=65, height=64, res=0.05, unknown_is_obstacle=True, max_dist_cells=5)
    pose = nr.caller_pose(nr.params(**kw))
    views, carve = scene_views(2, 5), dict(lattice_camera(64, 48, 4), **RANGE)
    host = check(f, "host", views, carve, frame=pose, model=m, **kw)
    P = 65 * 64
    dev = {name: torch.full((P * (2 if name == "hits" else 1) + 3,), 7, dtype={"uint32": torch.int32}.get(np.dtype(dt).name) or
                            getattr(torch, np.dtype(dt).name), device="cuda") for name, dt, _ in binding.NAVCARVE_OUTPUTS}
    torch.cuda.synchronize()
    st = f.nav_grid_carve_device(views, carve=carve, pose=pose, **dict(kw, **dev))
    for k in nc.GRID_STATS + nc.RAY_STATS + ("list_entries",):
        assert st[k] == host["stats"][k], k
    for name, t in dev.items():
        a = t.cpu().numpy()
        util.assert_same_bits(a[:-3].view(host[name].dtype).reshape(host[name].shape), host[name], "device " + name)
        assert (a[-3:] == 7).all(), name
    for t in dev.values():
        t.fill_(9)
    torch.cuda.synchronize()
    f.nav_grid_carve_device(views, seen=dev["seen"], carve=carve, pose=pose, **kw)
    util.assert_same_bits(dev["seen"].cpu().numpy()[:-3].view(np.uint32).reshape(64, 65), host["seen"], "device seen alone")
    assert all(bool((dev[name] == 9).all()) for name in nr.OUTPUTS) and bool((dev["seen"][-3:] == 9).all())


def test_chunks_give_the_same_result(fusion):
    f = fusion
    m = nr.hand_model(1300, 0)
    f.set_model(m, 513, 100)
    kw = dict(width=65, height=64, res=0.05)
    views, carve = scene_views(5, 9), dict(lattice_camera(41, 5, 1), carve_misses=True, **RANGE)
    whole = check(f, "one chunk", views, carve, frame="caller", model=m, **kw)
    assert f.debug_navcarve_last()["chunks"] == 1
    try:
        for chunk, n in ((205, 5), (100, 11), (1024, 2)):               # a view per chunk; chunks that cut views; a last chunk of one ray
            f.debug_navcarve_set_chunk_rays(chunk)
            got = f.nav_grid_carve(views, carve=carve, pose=nr.caller_pose(nr.params(**kw)), **kw)
            same(got, whole, "chunks of %d rays" % chunk)
            assert f.debug_navcarve_last()["chunks"] == n
        for bad in (-1, (1 << 24) + 1):
            with pytest.raises(binding.SsfError, match=r"ssf_debug_navcarve_set_chunk_rays failed \(-1\)"):
                f.debug_navcarve_set_chunk_rays(bad)
        f.debug_navcarve_set_chunk_rays(1 << 24)
    finally:
        f.debug_navcarve_set_chunk_rays(0)


# ---- a store with holes --------------------------------------------------------------------------------------------------
def test_a_store_with_holes_and_its_compaction(carve_lib):
    """the panning camera of tests/test_navgrid_gpu.py leaves holes in the out-of-view span; the views are the tracked poses"""
    f = handle(carve_lib, nb_supersurfels_max=20000)
    R0, t0 = synthetic.orbit_pose(0)
    rot_y = lambda deg: nr.rot("y", deg)
    poses = []
    for k in range(30):
        deg = 3.0 * (k if k < 15 else 29 - k)
        rgb, depth, _ = synthetic.render(R0 @ rot_y(deg), t0, W, H, noise=True, rng=np.random.default_rng(1000 + k))
        poses.append(f.process_frame(rgb, depth, prior_pose=nr.pose_about(rot_y(deg), np.zeros(3)))["pose"])
    cnt = f.counts()
    assert cnt["n_model"] > cnt["n_visible"] > 0, cnt
    model = f.get_model()
    lo, hi = model["positions"].min(axis=0), model["positions"].max(axis=0)
    mid = float(0.5 * (lo[1] + hi[1]))
    kw = dict(width=96, height=96, res=0.05, z_min=-hi[1] - 0.1, z_max=-lo[1] + 0.1, floor_max=-mid)
    views = replay.thin_views(poses, 5)
    assert len(views) == 5
    carve = dict(stride=8)                                              # the handle's camera and range
    before = check(f, "holes", views, carve, model=model, **kw)
    assert before["stats"]["rays"] == 5 * 20 * 16 and before["stats"]["rays_hit"] > 0 and before["stats"]["ray_entries"] > 0
    f.debug_recentre()
    after = check(f, "compacted", views, carve, **kw)
    same(after, before, "compacted against holes")
    f.close()


# ---- index reuse, no side effects --------------------------------------------------------------------------------------------
def test_the_raycast_index_is_shared(fusion):
    f = fusion
    m = rr.hand_model(513, 0)
    f.set_model(m, 257, 100)
    views, carve = scene_views(2, 1), dict(lattice_camera(64, 48, 4), **RANGE)
    kw = dict(width=33, height=31, res=0.05)
    first = f.nav_grid_carve(views, carve=carve, **kw)
    rays = rr.scene_rays(m, 65, 0)
    assert f.raycast(rays, pose=rr.scene_pose(0), **RANGE)["stats"]["index_rebuilt"] == 0            # built by the carve
    f.set_model(m, 257, 100)                                            # a new model generation
    assert f.raycast(rays, pose=rr.scene_pose(0), **RANGE)["stats"]["index_rebuilt"] == 1
    same(f.nav_grid_carve(views, carve=carve, **kw), first, "on the ray cast's index")
    assert f.raycast(rays, pose=rr.scene_pose(0), **RANGE)["stats"]["index_rebuilt"] == 0


def test_a_carve_changes_no_later_result(carve_lib):
    A, B = handle(carve_lib), handle(carve_lib)
    poses = []
    for k in range(0, 36, 3):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        poses.append(ra["pose"])
        got = A.nav_grid_carve(poses, width=96, height=80)
        assert got["stats"]["rays"] == len(poses) * 20 * 16
        A.nav_grid_carve(poses[-2:], outputs=("dist2", "seen"), carve=dict(stride=4, carve_misses=True), z_min=-5.0, z_max=5.0, floor_max=0.0,
                         unknown_is_obstacle=True)
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)
    B.close()
    A.close()


# ---- refusals, growth, profiling -----------------------------------------------------------------------------------------------
def test_the_refusals(carve_lib):
    f = handle(carve_lib)
    f.process_frame(*util.frame(0, W, H))
    nan, inf = float("nan"), float("inf")
    small = dict(width=16, height=16)
    views = f.get_pose().reshape(1, 12)
    refused = pytest.raises(binding.SsfError, match=r"ssf_navgrid_carve failed \(-1\)")
    for kw in (dict(width=0), dict(height=4097), dict(res=0.0), dict(res=nan), dict(splat_scale=-1.0), dict(max_steps=0), dict(max_dist_cells=1025),
               dict(min_hits=0), dict(z_min=1.0, z_max=0.5), dict(t_init=(5, 4)), dict(floor_cos=1.5)):                    # the grid's part
        with refused:
            f.nav_grid_carve(views, **dict(small, **kw))
    cam = dict(fx=150.0, fy=150.0, cx=79.5, cy=63.5, cam_width=160, cam_height=128)
    bad = [dict(stride=0), dict(stride=65), dict(cam, stride=64, cam_height=63), dict(cam, fx=0.0), dict(cam, fy=-1.0), dict(cam, fx=nan),
           dict(cam, fy=inf), dict(cam, cx=nan), dict(cam, cy=inf), dict(cam, cam_width=8193), dict(cam, cam_height=0), dict(cam, cam_height=8193),
           dict(cam, cam_width=-1), dict(hit_margin_cells=-0.5), dict(hit_margin_cells=nan), dict(hit_margin_cells=inf), dict(min_seen=0),
           dict(t_min=0.0, t_max=1.0), dict(t_min=2.0, t_max=1.0), dict(t_min=nan, t_max=1.0), dict(t_min=0.1, t_max=inf),          # the ray cast's part
           dict(ray_min_conf=nan), dict(ray_splat_scale=1e-4), dict(ray_splat_scale=2048.0), dict(ray_splat_scale=nan)]
    for carve in bad:
        for v in (views, None):                                        # refused with and without views
            with refused:
                f.nav_grid_carve(v, carve=carve, **small)
    with refused:
        f.nav_grid_carve(views, carve=dict(t_min=0.1, t_max=1700.0), res=0.05, **small)          # t_max / step = 68000 > 65535
    f.nav_grid_carve(views, carve=dict(t_min=0.1, t_max=1600.0), res=0.05, **small)
    with refused:
        f.nav_grid_carve(views, outputs=(), **small)                   # every output NULL
    with refused:
        f.nav_grid_carve(np.tile(views, (4097, 1)), **small)
    with refused:                                                      # 4096 views x 8192 x 8192 pixels
        f.nav_grid_carve(np.tile(views, (4096, 1)), carve=dict(cam, cam_width=8192, cam_height=8192, stride=1), **small)
    L = carve_lib.lib
    byref = binding.C.byref
    p, c, st, out = binding.SsfNavGridParams(), binding.SsfNavCarveParams(), binding.SsfNavCarveStats(), binding.SsfNavCarveOut()
    assert L.ssf_navgrid_default_params(f.h, byref(p)) == 0 and L.ssf_navcarve_default_params(f.h, byref(c)) == 0
    assert L.ssf_navcarve_default_params(None, byref(c)) == -1 and L.ssf_navcarve_default_params(f.h, None) == -1
    seen = np.zeros((512, 512), np.uint32)
    out.seen = seen.ctypes.data
    assert L.ssf_navgrid_carve(None, byref(p), byref(c), byref(out), byref(st)) == -1
    assert L.ssf_navgrid_carve(f.h, None, byref(c), byref(out), byref(st)) == -1
    assert L.ssf_navgrid_carve(f.h, byref(p), None, byref(out), byref(st)) == -1
    assert L.ssf_navgrid_carve(f.h, byref(p), byref(c), None, byref(st)) == -1
    assert L.ssf_navgrid_carve(f.h, byref(p), byref(c), byref(binding.SsfNavCarveOut()), byref(st)) == -1
    c.n_views = 1                                                      # views NULL with n_views > 0
    assert L.ssf_navgrid_carve(f.h, byref(p), byref(c), byref(out), byref(st)) == -1
    c.n_views = 0
    assert L.ssf_navgrid_carve(f.h, byref(p), byref(c), byref(out), None) == 0        # seen alone; stats are optional
    d = f.nav_grid_carve_default_params()
    assert (d["n_views"], d["cam_width"], d["cam_height"], d["stride"], d["carve_misses"], d["min_seen"]) == (0, 0, 0, 8, 0, 1)
    assert (d["fx"], d["t_min"], d["t_max"], d["ray_min_conf"], d["ray_splat_scale"], d["hit_margin_cells"]) == (0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    # the handle keeps working: a carve and a frame after the refusals
    check(f, "after the refusals", views, dict(), width=96, height=80)
    f.process_frame(*util.frame(1, W, H))
    check(f, "after a frame", views, dict(carve_misses=True), width=96, height=80, z_min=-5.0, z_max=5.0, floor_max=0.0)
    g = handle(carve_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_grid_carve(views, **small)
    q = handle(carve_lib, pipeline_depth=2, extract_batch=2)
    q.submit_frame(*util.frame(0, W, H))
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q.nav_grid_carve(views, **small)
    q.process_submitted()
    check(q, "pipelined, at rest", views, dict(), width=96, height=80)
    q.close()
    g.close()
    f.close()


def test_the_working_buffers_grow(carve_lib):
    f = handle(carve_lib, nb_supersurfels_max=30000)
    f.set_model(nr.hand_model(257, 0), 256, 100)
    check(f, "few rays, small grid", scene_views(1), dict(lattice_camera(8, 8, 8), **RANGE), frame="caller", width=7, height=5, res=0.2)
    check(f, "more rays, larger grid", scene_views(3), dict(lattice_camera(41, 5, 1), **RANGE), frame="caller", width=130, height=97, res=0.03)
    f.set_model(nr.hand_model(30000, 1, extent=3.0), 9000, 100)
    f.debug_navcarve_set_chunk_rays(64)
    got = f.nav_grid_carve(scene_views(3), carve=dict(lattice_camera(41, 5, 1), **RANGE), width=130, height=97, res=0.05)
    f.debug_navcarve_set_chunk_rays(0)
    same(f.nav_grid_carve(scene_views(3), carve=dict(lattice_camera(41, 5, 1), **RANGE), width=130, height=97, res=0.05), got, "large model")
    assert got["stats"]["rows_used"] == 30000 and got["stats"]["rays_hit"] > 0
    f.set_model(nr.hand_model(257, 2), 256, 100)
    check(f, "small again", scene_views(2), dict(stride=16, **RANGE), width=33, height=31, res=0.05)
    f.close()


def test_the_kernels_are_timed_under_profile(carve_lib):
    f = handle(carve_lib, profile=1)
    f.process_frame(*util.frame(0, W, H))
    f.reset_kernel_times()
    got = f.nav_grid_carve(f.get_pose().reshape(1, 12), width=96, height=80, z_min=-5.0, z_max=5.0, floor_max=0.0)
    assert got["stats"]["rays_hit"] > 0
    names = f.kernel_times()
    for k in ("navgrid_prep", "navgrid_fill", "navgrid_tile", "navgrid_cells", "navgrid_columns", "navgrid_rows", "navcarve_rays", "navcarve_march",
              "raycast_prep", "raycast_march"):
        assert k in names and names[k][1] > 0, (k, names)
    f.close()


# ---- replay.py's files -----------------------------------------------------------------------------------------------------
def test_replay_writes_the_carved_grid(carve_lib, tmp_path):
    f = handle(carve_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    _, results = replay.replay(f, frames, nav_grid_dir=str(tmp_path), nav_grid_every=2, nav_grid_res=0.1, nav_grid_carve=True, nav_grid_carve_stride=4)
    assert sorted(os.listdir(str(tmp_path))) == ["000000.pgm", "000000.yaml", "000000_dist2.npy", "000000_seen.npy",
                                                 "000002.pgm", "000002.yaml", "000002_dist2.npy", "000002_seen.npy"]
    want = f.nav_grid_carve([r["pose"] for r in results], outputs=("state", "dist2", "seen"), carve=dict(stride=4), res=0.1)
    raw = open(str(tmp_path / "000002.pgm"), "rb").read()
    img = np.frombuffer(raw[len(b"P5\n512 512\n255\n"):], np.uint8).reshape(512, 512)[::-1]
    assert np.array_equal(img == 0, want["state"] == 100) and np.array_equal(img == 254, want["state"] == 0)
    util.assert_same_bits(np.load(str(tmp_path / "000002_dist2.npy")), want["dist2"], "dist2.npy")
    util.assert_same_bits(np.load(str(tmp_path / "000002_seen.npy")), want["seen"], "seen.npy")
    assert want["stats"]["rays"] == 3 * 40 * 32 and want["seen"].any()
    with pytest.raises(ValueError, match="nav_grid_carve needs nav_grid_dir"):
        replay.replay(f, [], nav_grid_carve=True)
    f.close()


# ---- the C++ surface -----------------------------------------------------------------------------------------------------
def test_build_a_carved_nav_grid_in_cpp(carve_lib, tmp_path):
    """tests/cpp/navcarve_smoke.cpp on the GPU: its counts and FNV-1a checksums equal those of the Python call on the same map (the
    program's six frames, reproduced here as in tests/test_navgrid_gpu.py)"""
    libdir = os.path.dirname(carve_lib.path)
    exe = str(tmp_path / "navcarve_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "navcarve_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip_navcarve", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    names = ("rays", "hit", "invalid", "carving", "samples", "entries", "seen", "carved", "free", "occupied", "unknown")
    got = re.search(r"navcarve 64x64 " + " ".join(nm + r"=(\d+)" for nm in names) + r" state=([0-9a-f]{16}) dist2=([0-9a-f]{16}) seen=([0-9a-f]{16})", r.stdout)
    assert got and "no_views same=1" in r.stdout, r.stdout
    cfg = carve_lib.default_config(width=W, height=H, fx=150.0, fy=150.0, cx=79.5, cy=63.5, cell_size=16, lambda_pos=10.0,
                                     lambda_bound=1000.0, lambda_size=1000.0, lambda_disp=1e8, thresh_disp=1e-4, seg_iter=10,
                                     seg_use_ransac=1, nb_samples=16, filter_iter=4, filter_alpha=0.1, filter_beta=1.0,
                                     filter_threshold=0.05, range_min=0.2, range_max=5.0, delta_t=20, conf_thresh=2500.0,
                                     nb_supersurfels_max=50000, icp_iter=10, icp_cov_thresh=0.04, pipeline_depth=0,
                                     extract_batch=1, depth_prefilter=0)
    f = binding.Fusion(carve_lib, cfg)
    i = np.arange(W * H)
    poses = []
    for k in range(6):
        x, y = (i % W) + 2 * k, i // W
        rgb = np.stack([x * 255 // (W + 16), y * 255 // H, (x ^ y) & 255], axis=1).astype(np.uint8).reshape(H, W, 3)
        depth = (np.float32(1.0) + np.float32(0.004) * x.astype(np.float32)).astype(np.float32).reshape(H, W)
        poses.append(f.process_frame(rgb, depth)["pose"])
    frame = np.array([0, 1, 0, 1, 0, 0, 0, 0, -1, -1.6, -1.6, 0], np.float32)
    want = check(f, "python carve", poses, dict(stride=4, hit_margin_cells=2.0), frame=frame, width=64, height=64, res=0.05, z_min=-2.0,
                 floor_max=-1.3, z_max=0.0, max_dist_cells=12)
    s = want["stats"]
    assert s["rays_hit"] > 0 and s["ray_entries"] > 0, s

    def fnv(a):
        h = 1469598103934665603
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return "%016x" % h
    keys = ("rays", "rays_hit", "rays_invalid", "rays_carving", "ray_samples", "ray_entries", "cells_seen", "cells_carved", "cells_free",
            "cells_occupied", "cells_unknown")
    assert tuple(int(v) for v in got.groups()[:11]) == tuple(s[k] for k in keys), r.stdout
    assert got.groups()[11:] == (fnv(want["state"]), fnv(want["dist2"]), fnv(want["seen"])), r.stdout
    f.close()
