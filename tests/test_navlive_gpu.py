"""The live obstacle layer (include/ssf_navlive.h) on the GPU: every array and every exact stat of ssf_navlive_overlay equals the
numpy restatement (tests/navlive_ref.py) with ==, on the scenes that tests/test_navlive.py guards against being vacuous, on the
smallest images and grids at which the kernels take another path, with every parameter off its default in turn, with masks off the
full tile, with rays that end on both sides of a round of 64 samples, on boundary cases with hand-written answers, through device
pointers, through nav_live_plan, replay.py and the C++ wrapper."""
import os
import re
import subprocess

import numpy as np
import pytest

import navgrid_ref as nr
import navlive_ref as lr
import navpath_ref as wr
import navplan_ref as pr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
W, H = 160, 128
CPP = os.path.join(ROOT, "tests", "cpp")


def handle(lib, depth_format="f32", depth_scale=1.0, **kw):
    """a handle of a test's own, which the test closes when it is done with it"""
    f = binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))
    if depth_format != "f32":
        f.set_input_format(depth=depth_format, depth_scale=depth_scale)
    return f


@pytest.fixture(scope="module")
def live_lib():
    """libssf_hip_live.so: drive's objects plus the overlay's entry points (no fallback: a missing .so is an error)"""
    return binding.load_live()


@pytest.fixture(scope="module")
def fusion(live_lib):
    f = handle(live_lib)
    yield f
    f.close()


@pytest.fixture(scope="module")
def fusion_u16(live_lib):
    f = handle(live_lib, "u16", 0.001)
    yield f
    f.close()


def same(got, want, what, outputs=lr.OUTPUTS):
    for name in outputs:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name, got[name].shape, got[name].dtype)
        diff = got[name] != want[name]
        assert not diff.any(), (what, name, int(diff.sum()), np.argwhere(diff)[:5].tolist(), got[name][diff][:5].tolist(), want[name][diff][:5].tolist())
    for k in lr.STATS:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"], want["stats"])


def call_kw(kw):
    """the keywords of Fusion.nav_live from a restatement's: width and height come from state"""
    return {k: v for k, v in kw.items() if k not in ("width", "height")}


def check(f, what, depth, state_in, grid_pose, cam_pose, kw, mask=None, fmt="f32", scale=1.0, want=None):
    """the overlay on the device (host arrays) and in the restatement; returns both"""
    if want is None:
        want = lr.overlay(depth, mask, state_in, grid_pose, cam_pose, lr.params(**kw), fmt, scale)
    got = f.nav_live(depth, state_in, mask=mask, grid_pose=grid_pose, cam_pose=cam_pose, **call_kw(kw))
    same(got, want, what)
    assert (got["stats"]["pose"] == np.asarray(grid_pose, np.float32)).all(), what
    return got, want


# ---- the scenes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,fmt,stride", lr.GPU_CASES, ids=["%s-%s-stride%d" % c for c in lr.GPU_CASES])
def test_the_scenes(scene, fmt, stride, fusion, fusion_u16):
    i = lr.case_inputs(scene, fmt, stride)
    f = fusion_u16 if fmt == "u16" else fusion
    got, want = check(f, scene, i["depth"], i["state_in"], i["grid_pose"], i["cam_pose"], i["kw"], fmt=fmt, scale=i["depth_scale"],
                      want=lr.case_reference(scene, fmt, stride))
    s = got["stats"]
    assert s["cells_stamped"] > 0 and s["cells_opened"] > 0 and int(got["live_hits"].max()) >= 64
    # the merges: fewer atomics than points and entries, never none
    assert 0 < s["atomics"] < s["points_in_band"] + s["ray_entries"]


# image (width, height, stride, depth format): partial waves, partial pixel tiles, one row, several tiles both ways, one lattice pixel
IMAGES = ((1, 1, 1, "f32"), (13, 5, 1, "u16"), (64, 4, 4, "f32"), (257, 3, 1, "u16"), (160, 128, 8, "f32"), (100, 70, 64, "u16"))
# grid (width, height, res) and the map position of its corner: the grid's own tile edges; the camera is inside each
GRIDS = ((1, 1, 0.5, (0.6, 0.3)), (33, 31, 0.05, (0.0, 0.0)), (65, 64, 0.05, (-0.7, -0.9)))


@pytest.mark.parametrize("w,h,stride,fmt", IMAGES, ids=["%dx%d-stride%d-%s" % c for c in IMAGES])
def test_image_and_grid_shapes(w, h, stride, fmt, fusion, fusion_u16):
    f = fusion_u16 if fmt == "u16" else fusion
    d = lr.noise_depth(w, h, 7 * w + h, lo=0.1, hi=1.6)
    _, scale, image = dict((x[0], x) for x in lr.scene_formats(d))[fmt]
    cam_pose = lr.room_pose(yaw=8.0, roll=2.0, at=(0.8, 0.1, 0.35))
    points = 0
    for gw, gh, res, (tx, tz) in GRIDS:
        kw = dict(fx=150.0 * w / 160.0 + 20.0, fy=150.0 * w / 160.0 + 20.0, cx=0.5 * (w - 1), cy=0.5 * (h - 1), cam_width=w, cam_height=h, t_min=0.2,
                  t_max=5.0, width=gw, height=gh, res=res, max_dist_cells=5, stride=stride, min_hits=1 if w * h < 100 else 3)
        state_in = lr.state_pattern(gw, gh, gw + w)
        got, _ = check(f, "%dx%d on %dx%d" % (w, h, gw, gh), image, state_in, lr.grid_pose_at(tx, tz), cam_pose, kw, fmt=fmt, scale=scale)
        points += got["stats"]["points_in_band"]
    assert points > 0 or w * h == 1


@pytest.mark.parametrize("stride", [1, 4, 8, 64])
def test_the_strides_on_one_scene(stride, fusion):
    i = lr.case_inputs("room yaw pitch roll", "f32", stride)
    got, want = check(fusion, "stride %d" % stride, i["depth"], i["state_in"], i["grid_pose"], i["cam_pose"], i["kw"])
    assert got["stats"]["rays"] <= (W // stride) * (H // stride) and got["stats"]["rays_carving"] > 0


# ---- the parameter space: one entry off its default at a time (tests/test_navlive.py guards that each row changes its arrays) -----
@pytest.mark.parametrize("fmt", lr.PARAM_FORMATS)
@pytest.mark.parametrize("row", [None] + list(range(len(lr.PARAM_ROWS))), ids=("base",) + lr.PARAM_IDS)
def test_the_parameter_space(row, fmt, fusion, fusion_u16):
    i = lr.param_inputs(fmt, {} if row is None else lr.PARAM_ROWS[row][0])
    check(fusion_u16 if fmt == "u16" else fusion, "base" if row is None else lr.PARAM_IDS[row], i["depth"], i["state_in"], i["grid_pose"], i["cam_pose"],
          i["kw"], fmt=fmt, scale=i["depth_scale"], want=lr.param_reference(fmt, row))


# ---- masks off the full tile, in both formats and behind device pointers ----------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "u16"])
def test_the_mask_on_partial_pixel_tiles(fmt, fusion, fusion_u16):
    """37 x 29 at stride 3: the threads of a partial tile that lie outside the image read no mask"""
    i = lr.small_inputs(fmt)
    f = fusion_u16 if fmt == "u16" else fusion
    for mode in (1, 2):
        got, _ = check(f, "37x29 mask_mode %d" % mode, i["depth"], i["state_in"], i["grid_pose"], i["cam_pose"], dict(i["kw"], mask_mode=mode),
                       mask=i["mask"], fmt=fmt, scale=i["depth_scale"])
        assert 0 < got["stats"]["pixels_stamping"] < got["stats"]["pixels_valid"] and got["stats"]["cells_stamped"] > 0


def test_a_device_mask_inside_guard_bytes(fusion_u16):
    """depth, mask and grid behind device pointers, mask_mode 2: the 37 x 29 mask starts at an odd address between sentinel bytes"""
    import torch
    dev = torch.device("cuda")
    i = lr.small_inputs("u16")
    kw = dict(i["kw"], mask_mode=2)
    want = lr.overlay(i["depth"], i["mask"], i["state_in"], i["grid_pose"], i["cam_pose"], lr.params(**kw), "u16", i["depth_scale"])
    gw, gh, G = kw["width"], kw["height"], 67
    guarded = np.full(2 * G + i["mask"].size, 0xA5, np.uint8)
    guarded[G:-G] = i["mask"].ravel()
    d_mask = torch.from_numpy(guarded).to(dev)
    d_depth, d_in = torch.from_numpy(i["depth"].view(np.int16)).to(dev), torch.from_numpy(i["state_in"]).to(dev)
    out = dict(live_hits=torch.zeros((gh, gw), dtype=torch.int32, device=dev), live_seen=torch.zeros((gh, gw), dtype=torch.int32, device=dev),
               state_out=torch.zeros((gh, gw), dtype=torch.int8, device=dev), dist2=torch.zeros((gh, gw), dtype=torch.int32, device=dev))
    stats = fusion_u16.nav_live_device(d_depth, d_in, gw, gh, mask=d_mask.data_ptr() + G, grid_pose=i["grid_pose"], cam_pose=i["cam_pose"],
                                       **dict(out, **call_kw(kw)))
    got = dict(live_hits=out["live_hits"].cpu().numpy().view(np.uint32), live_seen=out["live_seen"].cpu().numpy().view(np.uint32),
               state=out["state_out"].cpu().numpy(), dist2=out["dist2"].cpu().numpy(), stats=stats)
    same(got, want, "device mask")
    assert (d_mask.cpu().numpy() == guarded).all() and (d_in.cpu().numpy() == i["state_in"]).all()
    assert 0 < stats["pixels_stamping"] < stats["pixels_valid"]


# ---- rays longer than a round of 64 samples, sixteen to a wave ---------------------------------------------------------------------
@pytest.mark.parametrize("shift", lr.EDGE_SHIFTS)
@pytest.mark.parametrize("tilt", lr.EDGE_TILTS)
def test_rays_that_end_on_both_sides_of_a_round_of_64_samples(tilt, shift, fusion):
    """64 x 2 pixels at stride 1: eight waves of sixteen rays of 49 .. 80 and 113 .. 144 samples (tests/test_navlive.py recomputes them);
    shifted, a round ends in the middle of a wave"""
    i = lr.edge_inputs(tilt, shift)
    got, _ = check(fusion, "round edges, tilt %g, shift %d" % (tilt, shift), i["depth"], i["state_in"], i["grid_pose"], i["cam_pose"], i["kw"])
    assert (got["stats"]["rays_carving"], got["stats"]["ray_samples"]) == (126, 12167 if shift == 0 else 12671)


# ---- specific cases ------------------------------------------------------------------------------------------------------------
def test_every_point_in_one_cell(fusion):
    """the contention case: a constant depth and a lens so long that the whole image lands in one cell"""
    kw = dict(lr.CAMERA, fx=1e6, fy=1e6, width=33, height=31, res=0.05, max_dist_cells=6, stride=4)
    d = np.full((H, W), 1.0, np.float32)
    state_in = np.full((31, 33), -1, np.int8)
    got, _ = check(fusion, "one cell", d, state_in, lr.grid_pose_at(), lr.room_pose(at=(0.825, 0.0, 0.225)), kw)      # the middle of cell (16, 24)
    hits = np.zeros((31, 33), np.uint32)
    hits[24, 16] = W * H
    assert (got["live_hits"] == hits).all() and got["stats"]["cells_stamped"] == 1
    assert got["stats"]["atomics"] < W * H // 8                            # runs of 16 vertically adjacent pixels went out as one addition each


def test_the_camera_inside_the_band_with_every_ray_valid(fusion):
    kw = dict(lr.CAMERA, width=33, height=31, res=0.05, max_dist_cells=6, stride=4)
    d = np.full((H, W), 1.0, np.float32)
    got, _ = check(fusion, "wall", d, np.full((31, 33), -1, np.int8), lr.grid_pose_at(), lr.room_pose(at=(0.8, 0.0, 0.225)), kw)
    n = (W // 4) * (H // 4)
    assert got["live_seen"][4, 16] == n == got["stats"]["rays"] == got["stats"]["rays_carving"]
    occ = got["state"] == 100
    assert occ[24].sum() >= 20 and not occ[:24].any() and not occ[25:].any() and not (got["live_seen"][25:] > 0).any()


def test_the_boundary_cases(fusion):
    for name, d, at, kw, want in lr.boundary_cases():
        kw = dict(lr.BOUNDARY, **kw)
        got, _ = check(fusion, name, np.full((1, 1), d, np.float32), np.full((4, 8), -1, np.int8), nr.IDENTITY, lr.boundary_pose(*at), kw)
        lr.check_expectations(got, want, 8, 4, name)


def test_a_camera_outside_the_grid_and_a_pose_that_is_not_finite(fusion):
    i = lr.case_inputs("room straight", "f32", 4)
    far = lr.room_pose(at=(40.0, 0.0, -30.0))
    got, _ = check(fusion, "outside", i["depth"], i["state_in"], i["grid_pose"], far, i["kw"])
    s = got["stats"]
    assert s["points_in_band"] == 0 == s["ray_entries"] and s["rays_carving"] > 0 and s["cells_stamped"] == 0 == s["cells_opened"]
    for k, bad in ((0, np.nan), (4, np.inf), (9, np.nan), (11, -np.inf)):
        pose = i["cam_pose"].copy()
        pose[k] = bad
        got, _ = check(fusion, "pose[%d] = %s" % (k, bad), i["depth"], i["state_in"], i["grid_pose"], pose, i["kw"])
        s = got["stats"]
        assert s["pixels_valid"] > 0 and s["rays"] > 0 and s["cells_stamped"] == 0 == s["cells_opened"] and s["ray_entries"] == 0
        assert (s["points_in_band"] == 0 and s["rays_carving"] == 0) or k == 0      # a NaN in R's first row leaves the other two coordinates finite
    got, _ = check(fusion, "after the poses", i["depth"], i["state_in"], i["grid_pose"], i["cam_pose"], i["kw"])
    assert got["stats"]["cells_stamped"] > 0


def test_the_mask_modes(fusion):
    i = lr.case_inputs("room rolled", "f32", 8)
    mask = lr.modes_mask()                                               # 40 % random, a solid band, values other than 1
    seen = []
    for mode in (0, 1, 2):
        got, _ = check(fusion, "mask_mode %d" % mode, i["depth"], i["state_in"], i["grid_pose"], i["cam_pose"], dict(i["kw"], mask_mode=mode), mask=mask)
        seen.append(got)
    assert (seen[0]["live_hits"] == seen[1]["live_hits"] + seen[2]["live_hits"]).all() and (seen[1]["live_seen"] == seen[0]["live_seen"]).all()
    assert seen[1]["stats"]["pixels_stamping"] + seen[2]["stats"]["pixels_stamping"] == seen[0]["stats"]["pixels_valid"]


def test_the_identity_and_the_fixed_point(fusion):
    i = lr.case_inputs("noise", "f32", 4)
    want_state = np.where(i["state_in"] == 100, 100, np.where(i["state_in"] == 0, 0, -1)).astype(np.int8)
    for unknown in (0, 1):
        got, _ = check(fusion, "no valid pixel", np.zeros((H, W), np.float32), i["state_in"], i["grid_pose"], i["cam_pose"],
                       dict(i["kw"], unknown_is_obstacle=unknown))
        assert (got["state"] == want_state).all() and not got["live_hits"].any() and not got["live_seen"].any()
        assert (got["dist2"] == nr.clearance(want_state, i["kw"]["max_dist_cells"], bool(unknown))).all()
    first, _ = check(fusion, "first", i["depth"], i["state_in"], i["grid_pose"], i["cam_pose"], i["kw"])
    again, _ = check(fusion, "fed back", i["depth"], first["state"], i["grid_pose"], i["cam_pose"], i["kw"])
    assert (again["state"] == first["state"]).all() and again["stats"]["cells_stamped"] == 0 == again["stats"]["cells_opened"]


def test_the_default_frame_and_camera_are_the_handles(live_lib):
    """grid_pose None = nav_grid_default_pose now, cam_pose None = the tracked pose, cam_width 0 = cfg's camera, t = cfg's range"""
    f = handle(live_lib)
    rgb, depth = util.frame(0, W, H)
    f.process_frame(rgb, depth)
    K = util.synthetic.intrinsics(W, H)
    kw = dict(width=65, height=64, res=0.1, max_dist_cells=7, stride=8)
    c = lr.params(cfg_camera=K, **kw)
    grid_pose = nr.default_pose(f.get_pose(), c)
    state_in = np.full((64, 65), -1, np.int8)
    want = lr.overlay(depth, None, state_in, grid_pose, f.get_pose(), c)
    got = f.nav_live(depth, state_in, **call_kw(kw))
    same(got, want, "defaults")
    assert (got["stats"]["pose"] == grid_pose).all() and (f.nav_grid_default_pose(width=65, height=64, res=0.1) == grid_pose).all()
    assert got["stats"]["points_in_band"] > 0 and got["stats"]["ray_entries"] > 0
    f.close()


# ---- through the binding ----------------------------------------------------------------------------------------------------------
def test_device_pointers_aliasing_and_outputs_that_are_not_asked_for(fusion, fusion_u16):
    import torch
    dev = torch.device("cuda")
    for fmt, f in (("f32", fusion), ("u16", fusion_u16)):
        i = lr.case_inputs("room yaw pitch roll", fmt, 4)
        want = lr.case_reference("room yaw pitch roll", fmt, 4)
        gw, gh = i["kw"]["width"], i["kw"]["height"]
        P = gw * gh
        kw = dict(call_kw(i["kw"]), grid_pose=i["grid_pose"], cam_pose=i["cam_pose"])
        image = i["depth"].view(np.int16) if fmt == "u16" else i["depth"]
        d_depth, d_in = torch.from_numpy(np.ascontiguousarray(image)).to(dev), torch.from_numpy(i["state_in"]).to(dev)
        # one buffer of int32 words: [guard | live_hits | guard | live_seen | guard | dist2 | guard | state | guard], sentinel-filled
        G, SENT = 64, -0x0A0B0C0D
        off = dict(live_hits=G, live_seen=2 * G + P, dist2=3 * G + 2 * P, state=4 * G + 3 * P)
        words = 5 * G + 3 * P + (P + 3) // 4

        def run(asked, state_out=None):
            buf = torch.full((words,), SENT, dtype=torch.int32, device=dev)
            ptr = {nm: buf.data_ptr() + 4 * o for nm, o in off.items()}
            out = {("state_out" if nm == "state" else nm): ptr[nm] for nm in asked}
            if state_out is not None:
                out["state_out"] = state_out
            stats = f.nav_live_device(d_depth, d_in.clone() if state_out is None else d_in, gw, gh, **dict(out, **kw))
            raw = buf.cpu().numpy().view(np.uint8)
            untouched = np.ones(len(raw), bool)
            got = dict(stats=stats)
            for nm in asked:
                nbytes = P * want[nm].dtype.itemsize
                got[nm] = raw[4 * off[nm]:4 * off[nm] + nbytes].view(want[nm].dtype).reshape(gh, gw).copy()
                untouched[4 * off[nm]:4 * off[nm] + nbytes] = False
            sentinel = np.full(words, SENT, np.int32).view(np.uint8)
            wrong = np.flatnonzero(untouched & (raw != sentinel))
            assert not len(wrong), (fmt, asked, "bytes outside the asked outputs were written", wrong[:8].tolist())
            return got
        same(run(lr.OUTPUTS), want, fmt + ": device pointers")
        same(run(("dist2",)), want, fmt + ": dist2 alone", outputs=("dist2",))
        same(run(("live_hits", "state")), want, fmt + ": hits and state", outputs=("live_hits", "state"))
        same(run(("live_seen",)), want, fmt + ": seen alone", outputs=("live_seen",))
        # the update in place
        before = d_in.clone()
        got = run(("dist2",), state_out=d_in)
        assert (d_in.cpu().numpy() == want["state"]).all() and (got["dist2"] == want["dist2"]).all()
        d_in.copy_(before)
        # host frame, device grid
        t = torch.zeros((gh, gw), dtype=torch.int32, device=dev)
        f.nav_live_device(i["depth"], d_in, gw, gh, dist2=t, frame_on_device=False, **kw)
        assert (t.cpu().numpy() == want["dist2"]).all()


def test_overlay_plan_and_waypoints_without_the_grid_leaving_the_device(fusion):
    """nav_live_plan against the three restatements chained on the host; the wall that only the frame knows turns the path"""
    kw = dict(lr.CAMERA, width=33, height=31, res=0.05, max_dist_cells=6, stride=4)
    cam_pose, grid_pose = lr.room_pose(at=(0.8, 0.0, 0.2)), lr.grid_pose_at()
    depth = lr.room_depth(cam_pose)
    state_in = np.zeros((31, 33), np.int8)                               # the map knows a free floor and nothing of wall and box
    state_in[:, :2] = -1
    lv = lr.overlay(depth, None, state_in, grid_pose, cam_pose, lr.params(**kw))
    goals, starts = [(16, 29)], [(16, 4), (2, 2), (40, 1)]
    plan = dict(min_dist2=1, max_path=300)
    wq = dict(keep_clearance=1, clearance_cap=4, lookahead=64)
    got = fusion.nav_live_plan(depth, state_in, goals, starts, waypoints=True, live=dict(call_kw(kw), grid_pose=grid_pose, cam_pose=cam_pose), plan=plan,
                               waypoint_params=wq)
    assert (got["live"]["state"] == lv["state"]).all() and (got["live"]["dist2"] == lv["dist2"]).all()
    assert {k: got["live"]["stats"][k] for k in lr.STATS} == lv["stats"] and lv["stats"]["cells_stamped"] > 10
    pl = pr.plan(lv["state"], lv["dist2"], goals, starts, **plan)
    for k in ("start_cost", "start_status", "path_len"):
        assert (got["plan"][k] == pl[k]).all(), k
    assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got["plan"]["path"], pl["path"]))
    assert {k: got["plan"]["stats"][k] for k in pr.STATS} == {k: pl["stats"][k] for k in pr.STATS}
    wp = wr.waypoints(lv["state"], lv["dist2"], pl["path"], min_dist2=1, max_waypoints=300, **wq)
    for k in ("n_waypoints", "status", "path_min"):
        assert (got["waypoints"][k] == wp[k]).all(), k
    assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got["waypoints"]["waypoints"], wp["waypoints"]))
    assert {k: got["waypoints"]["stats"][k] for k in wr.STATS} == wp["stats"]
    # the path from the camera's cell goes round the wall: on the static grid it is the straight column of 26 cells
    static = pr.plan(state_in, nr.clearance(state_in, 6, False), goals, starts[:1], **plan)
    assert pl["start_status"][0] == 0 and len(pl["path"][0]) > len(static["path"][0]) == 26
    assert all(lv["state"][y, x] == 0 for x, y in pl["path"][0]) and any(lv["state"][y, x] == 100 for x, y in static["path"][0])
    without = fusion.nav_live_plan(depth, state_in, goals, starts, live=dict(call_kw(kw), grid_pose=grid_pose, cam_pose=cam_pose), plan=plan)
    assert "waypoints" not in without and all((a == b).all() for a, b in zip(without["plan"]["path"], pl["path"]))


def test_a_call_between_two_frames_changes_no_later_result(live_lib):
    A, B = handle(live_lib), handle(live_lib)
    state_in = np.full((64, 65), -1, np.int8)
    for k in (0, 3, 6):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        lv = A.nav_live(depth, state_in, res=0.1, stride=8)
        A.nav_live_plan(depth, lv["state"], [(30, 30)], [(32, 32)], waypoints=True, live=dict(res=0.1), plan=dict(allow_unknown=1, max_path=100))
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)
    B.close()
    A.close()


def test_the_refusals(live_lib):
    import torch
    f = handle(live_lib)
    i = lr.case_inputs("room straight", "f32", 4)
    base = dict(call_kw(i["kw"]), grid_pose=i["grid_pose"], cam_pose=i["cam_pose"])
    depth, state_in = i["depth"], i["state_in"]
    refused = pytest.raises(binding.SsfError, match=r"ssf_navlive_overlay failed \(-1\)")
    nan, inf = float("nan"), float("inf")
    for kw in (dict(res=0.0), dict(res=nan), dict(res=inf), dict(res=-0.05), dict(max_dist_cells=0), dict(max_dist_cells=1025), dict(min_hits=0),
               dict(floor_max=nan), dict(z_max=nan), dict(cam_width=8193), dict(cam_height=0), dict(cam_height=8193), dict(fx=0.0), dict(fy=-1.0),
               dict(fx=nan), dict(fy=inf), dict(cx=inf), dict(cy=nan), dict(stride=0), dict(stride=65), dict(hit_margin_cells=-0.5),
               dict(hit_margin_cells=nan), dict(hit_margin_cells=inf), dict(min_seen=0), dict(t_min=0.0, t_max=3.0), dict(t_min=-1.0, t_max=3.0),
               dict(t_min=2.0, t_max=2.0), dict(t_min=3.0, t_max=2.0), dict(t_min=nan, t_max=2.0), dict(t_min=0.2, t_max=inf), dict(mask_mode=3),
               dict(mask_mode=-1), dict(mask_mode=1), dict(mask_mode=2), dict(t_min=0.2, t_max=2000.0)):
        with refused:
            image = np.zeros((kw.get("cam_height", H), kw.get("cam_width", W)), np.float32) if "cam_width" in kw or "cam_height" in kw else depth
            f.nav_live(image, state_in, **dict(base, **kw))
    with refused:                                                        # the stride leaves no lattice
        f.nav_live(np.ones((5, 13), np.float32), state_in, **dict(base, cam_width=13, cam_height=5, stride=8))
    with refused:
        f.nav_live(depth, state_in, outputs=(), **base)                   # every output NULL
    with refused:
        f.nav_live(depth, np.zeros((1, 4097), np.int8), **base)
    # just inside the corner bound: (t_max * l) / step <= 65535
    c = lr.params(**dict(i["kw"], t_max=1300.0))
    assert lr.corner_bound(c) <= 65535 < lr.corner_bound(dict(c, t_max=1400.0))
    f.nav_live(depth, state_in, **dict(base, t_max=1300.0))
    with refused:
        f.nav_live(depth, state_in, **dict(base, t_max=1400.0))
    # device pointers: alignment for the format, and overlaps
    dev = torch.device("cuda")
    gw, gh = i["kw"]["width"], i["kw"]["height"]
    P = gw * gh
    d_depth = torch.zeros(W * H + 8, dtype=torch.float32, device=dev)
    d_in = torch.from_numpy(state_in).to(dev)
    buf = torch.zeros(4 * P + 64, dtype=torch.int32, device=dev)
    a = buf.data_ptr()
    with refused:
        f.nav_live_device(d_depth.data_ptr() + 2, d_in, gw, gh, dist2=a, **base)
    f.nav_live_device(d_depth.data_ptr() + 4, d_in, gw, gh, dist2=a, **base)
    g = handle(live_lib, "u16", 0.001)
    with refused:
        g.nav_live_device(d_depth.data_ptr() + 1, d_in, gw, gh, dist2=a, **base)
    g.nav_live_device(d_depth.data_ptr() + 2, d_in, gw, gh, dist2=a, **base)
    g.close()
    for out in (dict(live_hits=a, live_seen=a), dict(live_hits=a, dist2=a + 4 * P - 4), dict(dist2=a, state_out=a + 4), dict(state_out=d_in.data_ptr() + 1),
                dict(live_seen=d_in.data_ptr()), dict(dist2=d_depth.data_ptr() + 4 * W * H - 4), dict(dist2=d_depth.data_ptr())):
        with refused:
            f.nav_live_device(d_depth, d_in, gw, gh, **dict(out, **base))
    f.nav_live_device(d_depth, d_in, gw, gh, state_out=d_in, **base)      # the one overlap that is the update in place
    # the mask is one of the arrays only when it is read: an output on its first byte alone, on its last alone, and beside it
    mbuf = torch.zeros(2 * P + W * H, dtype=torch.uint8, device=dev)
    m = mbuf.data_ptr() + P
    for ptr in (m - P + 1, m + W * H - 1, m):
        with refused:
            f.nav_live_device(d_depth, d_in, gw, gh, mask=m, state_out=ptr, **dict(base, mask_mode=2))
        assert live_lib.lib.ssf_last_error(f.h).decode() == "ssf_navlive_overlay: arrays overlap (only state == state_in may)"
    with refused:
        f.nav_live_device(d_depth, d_in, gw, gh, mask=m, dist2=m + W * H - 4, **dict(base, mask_mode=1))
    assert not mbuf.any()                                                # refused before any kernel
    for ptr in (m - P, m + W * H):
        f.nav_live_device(d_depth, d_in, gw, gh, mask=m, state_out=ptr, **dict(base, mask_mode=2))
    for ptr in (m - P + 1, m + W * H - 1, m):
        f.nav_live_device(d_depth, d_in, gw, gh, mask=m, state_out=ptr, **dict(base, mask_mode=0))
    # the C entry points themselves
    L, byref, vp = live_lib.lib, binding.C.byref, binding.C.c_void_p
    p, st = binding.SsfNavLiveParams(), binding.SsfNavLiveStats()
    assert L.ssf_navlive_default_params(f.h, byref(p)) == 0
    assert L.ssf_navlive_default_params(None, byref(p)) == -1 and L.ssf_navlive_default_params(f.h, None) == -1
    assert f.nav_live_default_params() == dict(width=512, height=512, res=np.float32(0.05), floor_max=np.float32(-0.8), z_max=0.5, max_dist_cells=40,
                                               unknown_is_obstacle=0, fx=0.0, fy=0.0, cx=0.0, cy=0.0, cam_width=0, cam_height=0, t_min=0.0, t_max=0.0,
                                               mask_mode=0, min_hits=4, stride=4, hit_margin_cells=1.0, min_seen=1, open_unknown=1, on_device=0,
                                               frame_on_device=0)
    p.width, p.height = 8, 4
    dd, s8, o8 = np.ones((H, W), np.float32), np.zeros((4, 8), np.int8), np.zeros((4, 8), np.int8)
    out = binding.SsfNavLiveOut()
    out.state = o8.ctypes.data
    d, s = dd.ctypes.data_as(vp), s8.ctypes.data_as(vp)
    assert L.ssf_navlive_overlay(f.h, byref(p), d, None, s, byref(out), None) == 0          # stats are optional
    assert L.ssf_navlive_overlay(None, byref(p), d, None, s, byref(out), byref(st)) == -1
    assert L.ssf_navlive_overlay(f.h, None, d, None, s, byref(out), byref(st)) == -1
    assert L.ssf_navlive_overlay(f.h, byref(p), None, None, s, byref(out), byref(st)) == -1
    assert L.ssf_navlive_overlay(f.h, byref(p), d, None, None, byref(out), byref(st)) == -1
    assert L.ssf_navlive_overlay(f.h, byref(p), d, None, s, None, byref(st)) == -1
    assert L.ssf_navlive_overlay(f.h, byref(p), d, None, s, byref(binding.SsfNavLiveOut()), byref(st)) == -1
    for field, bad in (("width", 0), ("width", 4097), ("height", -3), ("height", 4097)):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert L.ssf_navlive_overlay(f.h, byref(p), d, None, s, byref(out), byref(st)) == -1, (field, bad)
        setattr(p, field, keep)
    # the handle keeps working: a call and a frame after the refusals
    check(f, "after the refusals", depth, state_in, i["grid_pose"], i["cam_pose"], i["kw"], want=lr.case_reference("room straight", "f32", 4))
    f.process_frame(*util.frame(0, W, H))
    check(f, "after a frame", depth, state_in, i["grid_pose"], i["cam_pose"], i["kw"], want=lr.case_reference("room straight", "f32", 4))
    g = handle(live_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_live(depth, state_in, **base)
    q = handle(live_lib, pipeline_depth=2, extract_batch=2)
    q.submit_frame(*util.frame(0, W, H))
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q.nav_live(depth, state_in, **base)
    q.process_submitted()
    check(q, "pipelined, at rest", depth, state_in, i["grid_pose"], i["cam_pose"], i["kw"], want=lr.case_reference("room straight", "f32", 4))
    q.close()
    g.close()
    f.close()


def test_the_refusal_texts(live_lib):
    """Every refusal of ssf_navlive_overlay by its exact ssf_last_error text (as the entry point's source had them before the refusals
    it shares with ssf_navmem_update moved into one place), on the 8 x 4 grid and the handle-size image of test_the_refusals: a row
    violates one parameter; the last four violate two, one on each side of the overlay's own checks (the NaN test of the band between
    the grid and the camera, min_seen between the margin and the range), which pins the order.  All are refused before any kernel."""
    f = handle(live_lib)
    L, byref, vp = live_lib.lib, binding.C.byref, binding.C.c_void_p
    dd, s8, o8 = np.ones((H, W), np.float32), np.zeros((4, 8), np.int8), np.zeros((4, 8), np.int32)
    nan = float("nan")
    cam = dict(cam_width=W, cam_height=H, fx=100.0, fy=100.0, cx=80.0, cy=64.0)
    rows = [(dict(depth=None), "depth is NULL"), (dict(state_in=None), "state_in is NULL"), (dict(state=None), "every output is NULL"),
            (dict(width=0), "the grid's size must be 1..4096 x 1..4096"), (dict(res=0.0), "res must be finite and > 0"),
            (dict(max_dist_cells=0), "max_dist_cells must be 1..1024"), (dict(min_hits=0), "min_hits must be >= 1"),
            (dict(floor_max=nan), "floor_max or z_max is a NaN"),
            (dict(cam, cam_width=8193), "cam_width and cam_height must be 1..8192"),
            (dict(cam, fx=-1.0), "fx and fy must be finite and > 0, cx and cy finite"), (dict(stride=0), "stride must be 1..64"),
            (dict(cam, cam_width=13, cam_height=5, stride=8), "the stride leaves no pixel lattice"),
            (dict(hit_margin_cells=-0.5), "hit_margin_cells must be finite and >= 0"), (dict(min_seen=0), "min_seen must be >= 1"),
            (dict(t_min=3.0, t_max=2.0), "the range needs 0 < t_min < t_max, both finite"), (dict(mask_mode=3), "mask_mode must be 0..2"),
            (dict(mask_mode=1), "mask is NULL with mask_mode != 0"),
            (dict(frame_on_device=1, depth=dd.ctypes.data + 2), "the device depth pointer is not aligned for the input format"),
            (dict(t_min=0.2, t_max=2000.0), "(t_max * l) / (res / 2) must be <= 65535 at the image's corners"),
            (dict(dist2=o8.ctypes.data), "arrays overlap (only state == state_in may)"),
            (dict(min_hits=0, floor_max=nan), "min_hits must be >= 1"), (dict(floor_max=nan, stride=0), "floor_max or z_max is a NaN"),
            (dict(hit_margin_cells=-0.5, min_seen=0), "hit_margin_cells must be finite and >= 0"),
            (dict(min_seen=0, t_min=3.0, t_max=2.0), "min_seen must be >= 1")]
    for bad, text in rows:
        p, out = binding.SsfNavLiveParams(), binding.SsfNavLiveOut()
        assert L.ssf_navlive_default_params(f.h, byref(p)) == 0
        p.width, p.height = 8, 4
        arg = dict(depth=dd.ctypes.data, state_in=s8.ctypes.data, state=o8.ctypes.data, dist2=None)
        for k, v in bad.items():
            if k in arg:
                arg[k] = v
            else:
                setattr(p, k, v)
        out.state, out.dist2 = arg["state"], arg["dist2"]
        rc = L.ssf_navlive_overlay(f.h, byref(p), vp(arg["depth"]), None, vp(arg["state_in"]), byref(out), None)
        got = L.ssf_last_error(f.h).decode()
        print(bad, rc, got)
        assert rc == -1 and got == "ssf_navlive_overlay: " + text, (bad, rc, got)
    f.close()


def test_the_kernels_are_timed_under_profile(live_lib):
    f = handle(live_lib, profile=1)
    f.reset_kernel_times()
    i = lr.case_inputs("room straight", "f32", 4)
    check(f, "profiled", i["depth"], i["state_in"], i["grid_pose"], i["cam_pose"], i["kw"], want=lr.case_reference("room straight", "f32", 4))
    names = f.kernel_times()
    for k in ("navlive_stamp", "navlive_march", "navlive_cells", "navgrid_columns", "navgrid_rows"):
        assert k in names and names[k][1] > 0, (k, names)
    f.reset_kernel_times()
    f.nav_live(i["depth"], i["state_in"], outputs=("live_hits", "state"), open_unknown=0, grid_pose=i["grid_pose"], cam_pose=i["cam_pose"], **call_kw(i["kw"]))
    names = f.kernel_times()
    assert "navlive_stamp" in names and "navlive_march" not in names and "navgrid_rows" not in names       # nothing asked for the march or the clearance
    f.close()


# ---- replay.py's files -----------------------------------------------------------------------------------------------------
def test_replay_writes_the_live_layer_next_to_the_grid(live_lib, tmp_path, capsys):
    from supersurfel_fusion_amd import replay
    f = handle(live_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    replay.replay(f, frames, nav_grid_dir=str(tmp_path), nav_grid_every=2, nav_grid_res=0.1, nav_live=dict(min_hits=2, stride=8))
    per_grid = [".pgm", ".yaml", "_dist2.npy", "_live_dist2.npy", "_live_state.npy"]
    assert sorted(os.listdir(str(tmp_path))) == sorted("%06d%s" % (k, s) for k in (0, 2) for s in per_grid)
    grid = f.nav_grid(outputs=("state", "dist2"), res=0.1)
    lv = f.nav_live(frames[2][2], grid["state"], grid_pose=grid["stats"]["pose"], res=0.1, min_hits=2, stride=8)
    assert (np.load(str(tmp_path / "000002_live_state.npy")) == lv["state"]).all() and (np.load(str(tmp_path / "000002_live_dist2.npy")) == lv["dist2"]).all()
    assert (np.load(str(tmp_path / "000002_dist2.npy")) == grid["dist2"]).all() and lv["stats"]["points_in_band"] > 0
    logged = [l for l in capsys.readouterr().out.splitlines() if l.startswith("nav-live ")]
    assert len(logged) == 2 and "cells_stamped=%d " % lv["stats"]["cells_stamped"] in logged[1] and "points_in_band=%d" % lv["stats"]["points_in_band"] in logged[1]
    with pytest.raises(ValueError, match="nav_live needs nav_grid_dir"):
        replay.replay(f, [], nav_live=dict())
    f.close()


# ---- the C++ surface -----------------------------------------------------------------------------------------------------
def test_overlay_in_cpp(live_lib, fusion, fusion_u16, tmp_path):
    """tests/cpp/navlive_smoke.cpp on the GPU: its counts and FNV-1a checksums equal those of the Python calls on the same arrays"""
    libdir = os.path.dirname(live_lib.path)
    exe = str(tmp_path / "navlive_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "navlive_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip_live", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "grid ok=1" in r.stdout, r.stdout
    names = ("valid", "stamping", "points", "rays", "entries", "stamped", "opened")
    line = lambda tag: re.search(tag + " " + " ".join(nm + r"=(\d+)" for nm in names) + r" state=([0-9a-f]{16}) dist2=([0-9a-f]{16}) hits=([0-9a-f]{16}) "
                                 r"seen=([0-9a-f]{16})", r.stdout)
    p = np.arange(W * H, dtype=np.uint64)
    k = ((p * 2654435761 & 0xFFFFFFFF) >> 12) % 1024
    depth = np.where(p % 97 == 0, 0.0, 0.5 + k.astype(np.float32) * np.float32(0.0009765625)).astype(np.float32).reshape(H, W)
    counts = np.where(p % 97 == 0, 0, 500 + k).astype(np.uint16).reshape(H, W)
    mask = np.where(p % 3 == 0, 255, 0).astype(np.uint8).reshape(H, W)
    c = np.arange(48 * 40, dtype=np.uint64)
    u = ((c * 2654435761 & 0xFFFFFFFF) >> 16) % 100
    state_in = np.where(u < 5, 100, np.where(u < 75, -1, 0)).astype(np.int8).reshape(40, 48)
    grid_pose = np.array([1, 0, 0, 0, 0, -1, 0, 1, 0, -1.2, 0, -0.2], np.float32)
    kw = dict(lr.CAMERA, grid_pose=grid_pose, cam_pose=nr.IDENTITY, res=0.05, max_dist_cells=8)
    for tag, f, image, extra in (("navlive", fusion, depth, {}), ("masked", fusion, depth, dict(mask=mask, mask_mode=2)), ("u16", fusion_u16, counts, {})):
        got, told = f.nav_live(image, state_in, **dict(kw, **extra)), line(tag)
        assert told, (tag, r.stdout)
        s = got["stats"]
        counts_py = (s["pixels_valid"], s["pixels_stamping"], s["points_in_band"], s["rays"], s["ray_entries"], s["cells_stamped"], s["cells_opened"])
        assert tuple(int(v) for v in told.groups()[:7]) == counts_py, (tag, told.groups(), counts_py)
        sums = tuple(pr.fnv1a(got[nm].tobytes()) for nm in ("state", "dist2", "live_hits", "live_seen"))
        assert tuple(int(v, 16) for v in told.groups()[7:]) == sums, (tag, told.groups()[7:], sums)
        assert s["cells_stamped"] > 0 and s["points_in_band"] > 1000
