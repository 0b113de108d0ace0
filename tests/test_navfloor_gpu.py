"""ssf_navfloor_fit (include/ssf_navfloor.h) on the MI355X against the numpy restatement (tests/navfloor_ref.py): every integer,
histogram and float of the result with == -- on hand-built models at the wave and block edges of both stores, the rooms, the
compaction's rank and cursor edges, contention in one bin, boundary-exact rows, a store with holes (before and after its compaction),
growth, every parameter off its default, a permuted model, a caller's origin and up; plus no side effects on the frame path, the
refusals by their texts, profiling, the grid in the fitted frame and the C++ surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import navfloor_ref as fr
import navgrid_ref as nr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding, synthetic
from test_navfloor import PARAMETER_ROWS, POSE_ROWS

pytestmark = pytest.mark.gpu
W, H = 160, 128
CPP = os.path.join(ROOT, "tests", "cpp")
f32 = np.float32


@pytest.fixture(scope="module")
def floor_lib(product_lib):
    return binding.load_floor()


def handle(lib, **kw):
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


@pytest.fixture(scope="module")
def fusion(floor_lib):
    """one handle for the tests that replace the model through set_model"""
    f = handle(floor_lib, nb_supersurfels_max=30000)
    yield f
    f.close()


@pytest.fixture(scope="module")
def rooms():
    """the scenes of tests/test_navfloor.py, made once: name -> (model, planted, fit keywords)"""
    out = {}
    for name, room_kw, kw, _ in fr.SCENES + (fr.STEEP,):
        m, planted = fr.room(**room_kw)
        out[name] = (m, planted, kw)
    return out


def check(f, what, model=None, **kw):
    """the fit on the device and in numpy from get_model's rows; returns (device result, restatement)"""
    model = f.get_model() if model is None else model
    want = fr.fit(model, f.counts()["n_visible"], f.get_pose()[9:], fr.params(**kw))
    got = f.nav_floor(**kw)
    fr.same_fit(got, want, what)
    assert got["status_name"] == binding.NAVFLOOR_STATUS[want["status"]]
    g = got["grid"]
    util.assert_same_bits(g["pose"], want["pose"], what + " grid pose")
    assert (f32(g["z_min"]), f32(g["floor_max"]), f32(g["z_max"]), g["width"], g["height"], f32(g["res"])) == \
           (want["z_min"], want["floor_max"], want["z_max"], want["width"], want["height"], want["res"]), what
    return got, want


# ---- hand-built models at the wave and block edges of both stores ---------------------------------------------------------------
@pytest.mark.parametrize("n,nv", nr.SIZES)
def test_hand_built_models(n, nv, fusion):
    f = fusion
    m = nr.hand_model(n, 0)
    f.set_model(m, nv, 100)
    for visible_only in (False, True):
        got, _ = check(f, "n %d nv %d visible_only %d" % (n, nv, visible_only), model=m, visible_only=visible_only)
        assert got["rows_used"] == (nv if visible_only else n)
        check(f, "n %d nv %d visible_only %d, gated" % (n, nv, visible_only), model=m, visible_only=visible_only, min_conf=nr.MIN_CONF, t_init=(10, 90),
              t_last=(20, 100), min_rows=3, tilt_cos=0.5)


# ---- the rooms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in fr.SCENES + (fr.STEEP,)])
def test_the_rooms(name, fusion, rooms):
    f = fusion
    m, planted, kw = rooms[name]
    f.set_model(m, len(m["confidences"]) // 2, 100)
    got, want = check(f, name, model=m, **kw)
    assert got["status"] == fr.OK and got["rounds"] == 3 and got["inliers"][2] > 100, (name, got["status_name"])


# ---- the compaction's rank and cursor edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_block", [0, 1, 255, 256, 257])
def test_candidates_per_workgroup(per_block, fusion):
    """1300 rows, visible rows 513 (three blocks of visible slots, then the out-of-view blocks): the first `per_block` rows of every 256
    are floor candidates (257: all of the first block and one of the second, and so on), the others walls"""
    f = fusion
    m = nr.hand_model(1300, 1)
    k = np.arange(1300)
    cand = (k % 256 < per_block) if per_block <= 256 else (k % 512 < 257)
    rng = np.random.default_rng(per_block)
    m["orientations"][:, 6:9] = np.where(cand[:, None], np.array([[0.0, -1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]])).astype(f32)
    m["positions"][cand, 1] = (1.0 + rng.normal(0, 0.004, int(cand.sum()))).astype(f32)
    f.set_model(m, 513, 100)
    got, _ = check(f, "%d candidates per block" % per_block, model=m, min_rows=3)
    assert got["candidates"] == int(cand.sum()) and got["rows_used"] == 1300
    assert got["status"] == (fr.OK if per_block else fr.NO_FLOOR)


# ---- contention: one bin of both histograms, one sum; the flat level floor -----------------------------------------------------
def test_contention_in_one_bin_and_the_level_floor(fusion):
    f = fusion
    m = fr.flat_floor(2000)
    f.set_model(m, 700, 100)
    got, want = check(f, "2000 rows of one normal and one height", model=m)
    assert got["status"] == fr.OK and got["inliers"] == [2000] * 3 + [0] * 5 and int(got["dir_hist"][15, 15]) == 2000
    assert int(got["height_hist"].max()) == 2000 and want["alpha_beta"] == [(0.0, 0.0)] * 3
    util.assert_same_bits(got["pose"][:9], nr.FLOOR_R, "the level floor's rotation is the default frame's")
    util.assert_same_bits(got["normal"], np.array([0, -1, 0], f32), "the level floor's normal")


# ---- boundary rows, exact in f32 ---------------------------------------------------------------------------------------------
def boundary_model():
    """rows whose values sit exactly on a boundary of the rule (tilt_cos 0.5, u = (0, -1, 0), origin 0, height_res 0.25: every operation
    exact)"""
    below = float(np.nextafter(f32(512.0), f32(0.0)))
    nan, inf = float("nan"), float("inf")
    s3 = 0.8660254
    rows = [
        # |s| == tilt_cos on both signs: candidates (>=); one ulp less: not
        ((0.0, 1.0, 0.0), (s3, -0.5, 0.0), (4e-3, 4e-3)), ((0.0, 1.0, 0.0), (s3, 0.5, 0.0), (4e-3, 4e-3)),
        ((0.0, 1.0, 0.0), (s3, -0.49999997, 0.0), (4e-3, 4e-3)),
        # |p.k| at 512: no candidate; just below: one (its height is out of the histogram's range or in it, see below)
        ((512.0, 1.0, 0.0), (0.0, -1.0, 0.0), (4e-3, 4e-3)), ((below, 1.0, 0.0), (0.0, -1.0, 0.0), (4e-3, 4e-3)),
        ((0.0, 1.0, -512.0), (0.0, -1.0, 0.0), (4e-3, 4e-3)), ((0.0, 1.0, -below), (0.0, -1.0, 0.0), (4e-3, 4e-3)),
        # heights with height_res 0.25: hgt = -y; the first bin is t = -1024 (y = 256), the last t = 1023 (y = -255.75); just outside both
        ((0.0, 256.0, 0.0), (0.0, -1.0, 0.0), (4e-3, 4e-3)), ((0.0, 256.25, 0.0), (0.0, -1.0, 0.0), (4e-3, 4e-3)),
        ((0.0, -255.75, 0.0), (0.0, -1.0, 0.0), (4e-3, 4e-3)), ((0.0, -256.0, 0.0), (0.0, -1.0, 0.0), (4e-3, 4e-3)),
        # not used: a NaN normal, an infinite one, a non-finite position, dims 0
        ((0.0, 1.0, 0.0), (0.0, nan, 0.0), (4e-3, 4e-3)), ((0.0, 1.0, 0.0), (0.0, -inf, 0.0), (4e-3, 4e-3)),
        ((0.0, inf, 0.0), (0.0, -1.0, 0.0), (4e-3, 4e-3)), ((nan, 1.0, 0.0), (0.0, -1.0, 0.0), (4e-3, 4e-3)),
        ((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 4e-3)),
    ]
    n = len(rows)
    m = dict(positions=np.array([r[0] for r in rows]), colors=np.zeros((n, 3)), stamps=np.tile([40, 60], (n, 1)),
             orientations=np.array([(1, 0, 0, 0, 0, 1) + r[1] for r in rows]), shapes=np.zeros((n, 6)), dims=np.array([r[2] for r in rows]),
             confidences=np.full(n, 3.0))
    return {name: np.ascontiguousarray(m[name], dt) for name, _, dt in nr.FIELDS}


def test_boundary_exact_rows(fusion):
    f = fusion
    m = boundary_model()
    f.set_model(m, 6, 100)
    util.assert_same_bits(f.get_model()["orientations"], m["orientations"], "orientations (NaN and inf survive set_model)")
    kw = dict(tilt_cos=0.5, height_res=0.25, origin=(0.0, 0.0, 0.0), min_rows=3)
    got, want = check(f, "boundary rows", model=m, **kw)
    assert got["rows_used"] == 11 and got["candidates"] == 8
    # with tilt_cos 0.5 the two rows at 60 degrees vote far from the six level ones; align_cos 0.95 keeps them out of the heights
    assert got["direction_rows"] == 6 and got["aligned"] == 6 and got["height_out_of_range"] == 2
    util.assert_same_bits(got["normal"], np.array([0, -1, 0], f32), "n0 of exactly level rows")
    hh = got["height_hist"]
    assert hh[0] == 1 and hh[2047] == 1 and hh[1020] == 2 and int(hh.sum()) == 4
    # each row alone agrees as well (the NaN normal, the position at 512)
    for k in range(len(m["confidences"])):
        sub = {name: np.ascontiguousarray(v[k:k + 1]) for name, v in m.items()}
        f.set_model(sub, 1, 100)
        check(f, "boundary row %d alone" % k, model=sub, **kw)


# ---- a store with holes --------------------------------------------------------------------------------------------------
def test_a_store_with_holes_and_its_compaction(floor_lib):
    """30 frames of a camera that pans 3 degrees per frame for 15 frames and back (true pose as the prior): rows leave the view and
    come back, which leaves holes in the out-of-view span; compaction (ssf_debug_recentre) changes no result"""
    f = handle(floor_lib, nb_supersurfels_max=20000)
    R0, t0 = synthetic.orbit_pose(0)
    rot_y = lambda deg: nr.rot("y", deg)
    recentres = f.debug_recentre_count()
    for k in range(30):
        deg = 3.0 * (k if k < 15 else 29 - k)
        rgb, depth, _ = synthetic.render(R0 @ rot_y(deg), t0, W, H, noise=True, rng=np.random.default_rng(1000 + k))
        f.process_frame(rgb, depth, prior_pose=nr.pose_about(rot_y(deg), np.zeros(3)))
    cnt = f.counts()
    assert cnt["n_model"] > cnt["n_visible"] > 0, cnt
    assert f.debug_recentre_count() == recentres
    model = f.get_model()
    cases = [("any plane", dict(tilt_cos=0.3, min_rows=3, align_cos=0.9)), ("visible", dict(tilt_cos=0.3, min_rows=3, align_cos=0.9, visible_only=True)),
             ("towards the camera", dict(up=(0.0, 0.0, -1.0), tilt_cos=0.5, min_rows=3, height_res=0.05))]
    before = {name: check(f, "holes " + name, model=model, **kw)[0] for name, kw in cases}
    assert before["any plane"]["rows_used"] > before["visible"]["rows_used"] > 0
    assert max(b["candidates"] for b in before.values()) > 0
    f.debug_recentre()
    assert f.debug_recentre_count() == recentres + 1
    for name, kw in cases:
        after, _ = check(f, "compacted " + name, **kw)
        fr.same_fit(after, dict(before[name], sums=np.asarray(before[name]["sums"])), "compacted against holes " + name)


# ---- growth, permutation, the caller's origin and up ----------------------------------------------------------------------------
def test_the_working_buffers_grow_and_shrink(floor_lib):
    f = handle(floor_lib, nb_supersurfels_max=30000)
    f.set_model(nr.hand_model(257, 0), 256, 100)
    check(f, "small model", min_rows=3)
    big = nr.hand_model(30000, 1, extent=3.0)
    f.set_model(big, 9000, 100)
    got, _ = check(f, "large model", model=big)
    assert got["rows_used"] == 30000 and got["status"] == fr.OK
    f.set_model(nr.hand_model(257, 2), 256, 100)
    check(f, "small again", min_rows=3)


def test_a_permuted_model_gives_the_same_bits(fusion, rooms):
    f = fusion
    m, planted, kw = rooms["tilt 25 15"]
    n = len(m["confidences"])
    f.set_model(m, n // 2, 100)
    first = f.nav_floor()
    perm = np.random.default_rng(5).permutation(n)
    f.set_model({k: np.ascontiguousarray(v[perm]) for k, v in m.items()}, n, 100)
    again = f.nav_floor()
    fr.same_fit(again, dict(first, sums=np.asarray(first["sums"])), "permuted")
    twice = f.nav_floor()
    fr.same_fit(twice, dict(again, sums=np.asarray(again["sums"])), "the same model twice (the records' order differs from run to run)")


@pytest.mark.parametrize("name,kw", PARAMETER_ROWS + tuple(("tilt 25 15", kw) for kw in POSE_ROWS))
def test_each_parameter_off_its_default(name, kw, fusion, rooms):
    f = fusion
    m, planted, base = rooms[name]
    f.set_model(m, len(m["confidences"]) // 2, 100)
    check(f, "%s %s" % (name, kw), model=m, **dict(base, **kw))


def test_a_callers_origin_and_up(fusion, rooms):
    f = fusion
    m, planted, kw = rooms["tilt 12 -7"]
    f.set_model(m, len(m["confidences"]) // 2, 100)
    base, _ = check(f, "default origin", model=m)
    for origin in ((0.0, 0.0, 0.0), (40.0, -3.0, 25.0), (511.0, 0.0, 0.0)):
        got, _ = check(f, "origin %s" % (origin,), model=m, origin=origin)
        util.assert_same_bits(got["origin"], np.array(origin, f32), "origin")
    # far from the rows nothing is a candidate
    got, _ = check(f, "origin out of reach", model=m, origin=(600.0, 0.0, 0.0))
    assert got["status"] == fr.NO_FLOOR and got["candidates"] == 0 and got["rows_used"] == base["rows_used"]
    for up in ((0.0, -3.0, 0.0), tuple(planted["normal"]), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (-0.5, -0.5, 0.7)):
        check(f, "up %s" % (up,), model=m, up=up, min_rows=8)
    flipped = f.nav_floor(up=(0.0, 1.0, 0.0))                             # the hint points down: the same plane, seen from below
    assert flipped["status"] == fr.OK and float(np.dot(flipped["normal"], base["normal"])) < -0.999


# ---- no side effects, refusals, profiling ------------------------------------------------------------------------------------
def test_a_fit_changes_no_later_result(floor_lib):
    A, B = handle(floor_lib), handle(floor_lib)
    for k in range(0, 36, 3):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        A.nav_floor(up=(0.0, 0.0, -1.0), tilt_cos=0.3, min_rows=3)
        A.nav_floor(visible_only=True, min_conf=A.cfg.conf_thresh, refine_iters=8)
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)


def test_the_refusals(floor_lib):
    f = handle(floor_lib)
    f.process_frame(*util.frame(0, W, H))
    nan, inf = float("nan"), float("inf")
    positive = lambda nm: [(dict([(nm, v)]), "%s must be finite and > 0" % nm) for v in (0.0, -1.0, nan, inf)]
    bad = [(dict(up=(0.0, 0.0, 0.0)), "up must be finite and not zero"), (dict(up=(nan, 1.0, 0.0)), "up must be finite and not zero"),
           (dict(up=(0.0, inf, 0.0)), "up must be finite and not zero"), (dict(origin=(0.0, nan, 0.0)), "origin must be finite"),
           (dict(tilt_cos=0.0), r"tilt_cos must be in \(0, 1\)"), (dict(tilt_cos=1.0), r"tilt_cos must be in \(0, 1\)"),
           (dict(tilt_cos=nan), r"tilt_cos must be in \(0, 1\)"), (dict(align_cos=0.0), r"align_cos must be in \(0, 1\]"),
           (dict(align_cos=1.5), r"align_cos must be in \(0, 1\]"), (dict(align_cos=nan), r"align_cos must be in \(0, 1\]"),
           (dict(refine_iters=-1), r"refine_iters must be 0\.\.8"), (dict(refine_iters=9), r"refine_iters must be 0\.\.8"),
           (dict(min_rows=2), "min_rows must be >= 3"), (dict(floor_share256=0), r"floor_share256 must be 1\.\.256"),
           (dict(floor_share256=257), r"floor_share256 must be 1\.\.256"), (dict(width=0), "the grid's size must be"), (dict(width=4097), "the grid's size must be"),
           (dict(height=0), "the grid's size must be"), (dict(height=4097), "the grid's size must be"), (dict(t_init=(5, 4)), "a stamp range has min > max"),
           (dict(t_last=(1, 0)), "a stamp range has min > max")]
    for nm in ("height_res", "inlier_dist", "first_dist", "res", "below", "step", "body_height"):
        bad += positive(nm)
    for kw, text in bad:
        with pytest.raises(binding.SsfError, match=r"ssf_navfloor_fit failed \(-1\): ssf_navfloor_fit: " + text):
            f.nav_floor(**kw)
    f.nav_floor(align_cos=1.0)                                            # the closed end
    L = floor_lib.lib
    p, res, out = binding.SsfNavFloorParams(), binding.SsfNavFloorFitResult(), binding.SsfNavFloorOut()
    byref = binding.C.byref
    assert L.ssf_navfloor_default_params(f.h, byref(p)) == 0
    assert L.ssf_navfloor_default_params(None, byref(p)) == -1 and L.ssf_navfloor_default_params(f.h, None) == -1
    assert L.ssf_navfloor_fit(None, byref(p), byref(out), byref(res)) == -1
    assert L.ssf_navfloor_fit(f.h, None, byref(out), byref(res)) == -1 and L.ssf_last_error(f.h).decode() == "ssf_navfloor_fit: params is NULL"
    assert L.ssf_navfloor_fit(f.h, byref(p), byref(out), None) == -1 and L.ssf_last_error(f.h).decode() == "ssf_navfloor_fit: the result is NULL"
    assert L.ssf_navfloor_fit(f.h, byref(p), None, byref(res)) == 0       # the histograms are optional
    assert L.ssf_navfloor_fit(f.h, byref(p), byref(out), byref(res)) == 0
    d = f.nav_floor_default_params()
    want = fr.params()
    for nm in ("tilt_cos", "align_cos", "height_res", "first_dist", "inlier_dist", "min_conf", "res", "below", "step", "body_height"):
        assert d[nm] == f32(want[nm]), nm
    for nm in ("min_rows", "floor_share256", "refine_iters", "visible_only", "width", "height"):
        assert d[nm] == int(want[nm]), nm
    assert d["up"] == (0.0, -1.0, 0.0) and d["t_init_min"] == -2 ** 31 and d["t_last_max"] == 2 ** 31 - 1
    # the handle keeps working: a fit and a frame after the refusals
    check(f, "after the refusals", up=(0.0, 0.0, -1.0), tilt_cos=0.3, min_rows=3)
    f.process_frame(*util.frame(1, W, H))
    check(f, "after a frame", up=(0.0, 0.0, -1.0), tilt_cos=0.3, min_rows=3)
    # a sharded handle has no fit
    g = handle(floor_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\): ssf_navfloor_fit: a sharded handle"):
        g.nav_floor()
    # a pipelined handle with a frame pending
    q = handle(floor_lib, pipeline_depth=2, extract_batch=2)
    q.submit_frame(*util.frame(0, W, H))
    assert q.pending_frames() > 0
    with pytest.raises(binding.SsfError, match=r"\(-5\): frames are pending"):
        q.nav_floor()
    q.process_submitted()
    assert q.pending_frames() == 0
    check(q, "pipelined, at rest", up=(0.0, 0.0, -1.0), tilt_cos=0.3, min_rows=3)


def test_navfloor_kernels_are_timed_under_profile(floor_lib, rooms):
    f = handle(floor_lib, profile=1)
    m, planted, kw = rooms["tilt 12 -7"]
    f.set_model(m, len(m["confidences"]) // 2, 100)
    f.reset_kernel_times()
    assert f.nav_floor()["status"] == fr.OK
    names = f.kernel_times()
    for k in ("navfloor_prep", "navfloor_direction", "navfloor_height", "navfloor_refine"):
        assert k in names and names[k][1] > 0, (k, names)


# ---- the grid in the fitted frame ------------------------------------------------------------------------------------------------
def test_the_grid_in_the_fitted_frame(fusion, rooms):
    f = fusion
    m, planted, kw = rooms["tilt 25 15"]
    nv = len(m["confidences"]) // 2
    f.set_model(m, nv, 100)
    size = dict(width=160, height=160, res=0.05)
    both = f.nav_floor_grid(outputs=("state", "hits"), floor=dict(min_rows=40), max_dist_cells=5, **size)
    fit = both["floor"]
    want_fit = fr.fit(m, nv, f.get_pose()[9:], fr.params(min_rows=40, **size))
    fr.same_fit(fit, want_fit, "nav_floor_grid's fit")
    direct = f.nav_grid(outputs=("state", "hits"), max_dist_cells=5, **fit["grid"])
    q = nr.params(max_dist_cells=5, z_min=fit["grid"]["z_min"], z_max=fit["grid"]["z_max"], floor_max=fit["grid"]["floor_max"], **size)
    want = nr.build(m, nv, want_fit["pose"], q)
    for got in (both["grid"], direct):
        for name in ("state", "hits"):
            util.assert_same_bits(got[name], want[name], "the grid in the fitted frame: " + name)
        for k in nr.STATS:
            assert got["stats"][k] == want["stats"][k], k
        util.assert_same_bits(got["stats"]["pose"], want_fit["pose"], "the frame used")
    # the default frame takes the tilted floor for obstacles and noise: fewer free cells, in numpy and on the device
    dq = nr.params(max_dist_cells=5, **size)
    default = nr.build(m, nv, nr.default_pose(f.get_pose(), dq), dq)
    on_device = f.nav_grid(outputs=("state",), max_dist_cells=5, **size)
    assert on_device["stats"]["cells_free"] == default["stats"]["cells_free"]
    assert want["stats"]["cells_free"] > default["stats"]["cells_free"], (want["stats"]["cells_free"], default["stats"]["cells_free"])
    with pytest.raises(binding.SsfError, match="nav_floor_grid takes pose"):
        f.nav_floor_grid(pose=np.zeros(12, f32))


# ---- replay.py's files -----------------------------------------------------------------------------------------------------
def test_replay_builds_every_grid_in_the_fitted_frame(floor_lib, tmp_path):
    import json
    from supersurfel_fusion_amd import replay
    f = handle(floor_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    up = (0.0, 0.0, -1.0)
    replay.replay(f, frames, nav_grid_dir=str(tmp_path), nav_grid_every=2, nav_grid_res=0.1, nav_fit_floor=dict(up=up))
    assert sorted(os.listdir(str(tmp_path))) == ["000000.pgm", "000000.yaml", "000000_dist2.npy", "000000_floor.json", "000002.pgm", "000002.yaml",
                                                 "000002_dist2.npy", "000002_floor.json"]
    fit, want = check(f, "the map after the last frame", up=up, res=0.1)      # = what frame 2's files show
    side = json.load(open(str(tmp_path / "000002_floor.json")))
    for k in ("status", "rounds", "rows_used", "candidates", "direction_rows", "aligned", "height_out_of_range", "height_rows", "height_bin", "inliers"):
        assert side[k] == want[k], k
    assert side["status_name"] == fit["status_name"] and side["dir_bin"] == list(want["dir_bin"])
    assert [f32(v) for v in side["normal"]] == list(want["normal"]) and f32(side["d"]) == want["d"] and f32(side["camera_height"]) == want["camera_height"]
    grid = f.nav_grid(outputs=("state", "dist2"), **fit["grid"])
    util.assert_same_bits(np.load(str(tmp_path / "000002_dist2.npy")), grid["dist2"], "dist2.npy")
    assert "grid_to_map: [%s]\n" % ", ".join("%.9g" % v for v in want["pose"]) in open(str(tmp_path / "000002.yaml")).read()


# ---- the C++ surface -----------------------------------------------------------------------------------------------------
def test_fit_floor_in_cpp(floor_lib, tmp_path):
    """tests/cpp/navfloor_smoke.cpp on the GPU: its counts and FNV-1a checksums equal those of the Python calls on the same map (the
    program's six frames, reproduced here)"""
    libdir = os.path.dirname(floor_lib.path)
    exe = str(tmp_path / "navfloor_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "navfloor_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip_floor", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    got = re.search(r"navfloor status=(\d+) rounds=(\d+) rows=(\d+) candidates=(\d+) direction=(\d+) aligned=(\d+) out=(\d+) height_rows=(\d+) "
                    r"bin=\((\d+) (\d+) (\d+)\) inliers=\((\d+) (\d+) (\d+)\) sums=([0-9a-f]{16}) plane=([0-9a-f]{16}) pose=([0-9a-f]{16}) "
                    r"dir_hist=([0-9a-f]{16}) height_hist=([0-9a-f]{16})", r.stdout)
    grid = re.search(r"floorgrid 64x48 rows=(\d+) in_grid=(\d+) free=(\d+) occupied=(\d+) unknown=(\d+) state=([0-9a-f]{16}) dist2=([0-9a-f]{16})", r.stdout)
    assert got and grid and "apply ok" in r.stdout, r.stdout
    cfg = floor_lib.default_config(width=W, height=H, fx=150.0, fy=150.0, cx=79.5, cy=63.5, cell_size=16, lambda_pos=10.0,
                                   lambda_bound=1000.0, lambda_size=1000.0, lambda_disp=1e8, thresh_disp=1e-4, seg_iter=10,
                                   seg_use_ransac=1, nb_samples=16, filter_iter=4, filter_alpha=0.1, filter_beta=1.0,
                                   filter_threshold=0.05, range_min=0.2, range_max=5.0, delta_t=20, conf_thresh=2500.0,
                                   nb_supersurfels_max=50000, icp_iter=10, icp_cov_thresh=0.04, pipeline_depth=0,
                                   extract_batch=1, depth_prefilter=0)
    f = binding.Fusion(floor_lib, cfg)
    i = np.arange(W * H)
    for k in range(6):
        x, y = (i % W) + 2 * k, i // W
        rgb = np.stack([x * 255 // (W + 16), y * 255 // H, (x ^ y) & 255], axis=1).astype(np.uint8).reshape(H, W, 3)
        depth = (np.float32(1.0) + np.float32(0.004) * x.astype(np.float32)).astype(np.float32).reshape(H, W)
        f.process_frame(rgb, depth)
    kw = dict(up=(0.0, 0.0, -1.0), min_rows=8, width=64, height=48, res=0.05, below=0.3, step=0.1, body_height=1.0)
    fit, _ = check(f, "python fit", **kw)
    assert fit["status"] == fr.OK and fit["rounds"] == 3
    both = f.nav_floor_grid(outputs=("state", "dist2"), floor={k: v for k, v in kw.items() if k not in ("width", "height", "res")}, max_dist_cells=12,
                            width=64, height=48, res=0.05)

    def fnv(a):
        h = 1469598103934665603
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return "%016x" % h
    assert tuple(int(v) for v in got.groups()[:14]) == (fit["status"], fit["rounds"], fit["rows_used"], fit["candidates"], fit["direction_rows"], fit["aligned"],
                                                        fit["height_out_of_range"], fit["height_rows"], fit["dir_bin"][0], fit["dir_bin"][1], fit["height_bin"],
                                                        fit["inliers"][0], fit["inliers"][1], fit["inliers"][2]), r.stdout
    plane = np.concatenate([fit["normal"], np.array([fit["d"]], f32)])
    assert got.groups()[14:] == (fnv(fit["sums"]), fnv(plane), fnv(fit["pose"]), fnv(fit["dir_hist"]), fnv(fit["height_hist"])), r.stdout
    s = both["grid"]["stats"]
    assert tuple(int(v) for v in grid.groups()[:5]) == (s["rows_used"], s["samples_in_grid"], s["cells_free"], s["cells_occupied"], s["cells_unknown"]), r.stdout
    assert grid.groups()[5:] == (fnv(both["grid"]["state"]), fnv(both["grid"]["dist2"])), r.stdout
    assert s["cells_free"] > 0
