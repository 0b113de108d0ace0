"""The live layer with memory (include/ssf_navmem.h) on the GPU: every array and every exact stat of ssf_navmem_update equals the numpy
restatement (tests/navmem_ref.py) with ==, on the scenes that tests/test_navmem.py guards against being vacuous, with zero and random
layers, on the smallest images and grids at which the kernels take another path, with every parameter off its default in turn, under the
three mask modes, with rays that end on both sides of a round of 64 samples, on boundary cases with hand-written answers, through
device pointers and in place, against the device's own ssf_navlive_overlay, and through nav_memory_plan and nav_memory_dyn_steer."""
import numpy as np
import pytest

import navcarve_ref as ncr
import navgrid_ref as nr
import navlive_ref as lr
import navmem_ref as mr
import navpath_ref as wr
import navplan_ref as pr
import util
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
W, H = 160, 128


def handle(lib, depth_format="f32", depth_scale=1.0, **kw):
    """a handle of a test's own, which the test closes when it is done with it"""
    f = binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))
    if depth_format != "f32":
        f.set_input_format(depth=depth_format, depth_scale=depth_scale)
    return f


@pytest.fixture(scope="module")
def mem_lib():
    """libssf_hip_mem.so: dyn's objects plus the memory's entry points (no fallback: a missing .so is an error)"""
    return binding.load_mem()


@pytest.fixture(scope="module")
def fusion(mem_lib):
    f = handle(mem_lib)
    yield f
    f.close()


@pytest.fixture(scope="module")
def fusion_u16(mem_lib):
    f = handle(mem_lib, "u16", 0.001)
    yield f
    f.close()


def same(got, want, what, outputs=mr.OUTPUTS, stats=mr.STATS):
    for name in outputs:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name, got[name].shape, got[name].dtype)
        diff = got[name] != want[name]
        assert not diff.any(), (what, name, int(diff.sum()), np.argwhere(diff)[:5].tolist(), got[name][diff][:5].tolist(), want[name][diff][:5].tolist())
    for k in stats:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"], want["stats"])


def call_kw(kw):
    """the keywords of Fusion.nav_memory from a restatement's: width and height come from state, the tick from the memory"""
    return {k: v for k, v in kw.items() if k not in ("width", "height", "tick")}


def host_memory(layer, w, h, tick):
    """a LiveMemory of host arrays holding a copy of `layer` (None: zero) whose next tick is `tick`"""
    mem = binding.LiveMemory(w, h)
    if layer is not None:
        for a, nm in zip(mem.arrays(), mr.LAYER):
            a[...] = layer[nm]
    mem.tick = tick - 1
    return mem


def check(f, what, depth, state_in, layer, grid_pose, cam_pose, kw, mask=None, fmt="f32", scale=1.0, want=None):
    """the update on the device (host arrays, a host LiveMemory updated in place) and in the restatement; returns both"""
    c = mr.params(**kw)
    if want is None:
        want = mr.update(depth, mask, state_in, layer, grid_pose, cam_pose, c, fmt, scale)
    mem = host_memory(layer, c["width"], c["height"], c["tick"])
    got = f.nav_memory(depth, state_in, memory=mem, mask=mask, grid_pose=grid_pose, cam_pose=cam_pose, **call_kw(kw))
    same(got, want, what)
    assert mem.tick == c["tick"] and all(got[nm] is a for nm, a in zip(mr.LAYER, mem.arrays())), what
    assert (got["stats"]["pose"] == np.asarray(grid_pose, np.float32)).all(), what
    return got, want


# ---- the scenes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", ["zero", "random"])
@pytest.mark.parametrize("scene,fmt,stride,slices", mr.GPU_CASES, ids=["%s-%s-stride%d-slices%d" % c for c in mr.GPU_CASES])
def test_the_scenes(scene, fmt, stride, slices, layer, fusion, fusion_u16):
    i, ev = mr.case_evidence(scene, fmt, stride)
    f = fusion_u16 if fmt == "u16" else fusion
    kw = dict(i["kw"], slices=slices, tick=mr.GPU_TICK, **mr.GPU_AGES)
    c = mr.params(**kw)
    lay = None if layer == "zero" else mr.random_layer(c["width"], c["height"], c["width"] + stride, mr.GPU_TICK, slices=slices, **mr.GPU_AGES)
    got, want = check(f, scene, i["depth"], i["state_in"], lay, i["grid_pose"], i["cam_pose"], kw, fmt=fmt, scale=i["depth_scale"],
                      want=mr.update_from(ev, i["state_in"], lay, c))
    s = got["stats"]
    assert s["cells_marked"] > 0 and s["cells_opened"] > 0 and int(got["live_hits"].max()) >= 64
    if layer == "random":
        assert s["cells_expired"] > 0 and s["cells_remembered"] > 0 and s["bits_cleared"] > 0
    # the merges: fewer atomics than two per point and one per sample, never none
    assert 0 < s["atomics"] < 2 * s["points_in_band"] + s["ray_samples"]


# grid (width, height, res) and the map position of its corner; the camera is inside each
GRIDS = ((1, 1, 0.5, (0.6, 0.3)), (31, 33, 0.05, (0.0, 0.0)), (64, 65, 0.05, (-0.7, -0.9)))


@pytest.mark.parametrize("fmt", ["f32", "u16"])
def test_image_and_grid_shapes(fmt, fusion, fusion_u16):
    """37 x 29 at stride 3: partial 16 x 16 tiles both ways, 12 x 9 = 108 rays = six waves of 16 and a partial seventh"""
    f = fusion_u16 if fmt == "u16" else fusion
    w, h, stride = 37, 29, 3
    d = lr.noise_depth(w, h, 7 * w + h, lo=0.1, hi=1.6)
    _, scale, image = dict((x[0], x) for x in lr.scene_formats(d))[fmt]
    cam_pose = lr.room_pose(yaw=8.0, roll=2.0, at=(0.8, 0.1, 0.35))
    points = 0
    for gw, gh, res, (tx, tz) in GRIDS:
        kw = dict(fx=60.0, fy=60.0, cx=0.5 * (w - 1), cy=0.5 * (h - 1), cam_width=w, cam_height=h, t_min=0.2, t_max=5.0, width=gw, height=gh, res=res,
                  max_dist_cells=5, stride=stride, min_hits=3, slices=7, tick=9, max_mark_age=3, max_seen_age=2)
        lay = mr.random_layer(gw, gh, gw, 9, 3, 2, slices=7)
        got, _ = check(f, "%dx%d on %dx%d" % (w, h, gw, gh), image, lr.state_pattern(gw, gh, gw + w), lay, lr.grid_pose_at(tx, tz), cam_pose, kw,
                       fmt=fmt, scale=scale)
        points += got["stats"]["points_in_band"]
        assert got["stats"]["rays"] > 64                                  # (of the 108 lattice pixels, the valid ones)
    assert points > 0


# ---- the parameter space: one entry off its default at a time (tests/test_navmem.py guards that each row changes its arrays) ------
@pytest.mark.parametrize("fmt", lr.PARAM_FORMATS)
@pytest.mark.parametrize("row", [None] + list(range(len(mr.PARAM_ROWS))), ids=("base",) + mr.PARAM_IDS)
def test_the_parameter_space(row, fmt, fusion, fusion_u16):
    i = mr.param_inputs(fmt, {} if row is None else mr.PARAM_ROWS[row][1])
    got, _ = check(fusion_u16 if fmt == "u16" else fusion, "base" if row is None else mr.PARAM_IDS[row], i["depth"], i["state_in"], i["layer"], i["grid_pose"],
                   i["cam_pose"], i["kw"], fmt=fmt, scale=i["depth_scale"], want=mr.param_reference(fmt, row))
    assert got["stats"]["cells_opened"] > 0 or not i["c"]["open_unknown"]


# ---- the mask: the three modes against the restatement, off the full tile, behind device pointers --------------------------------
@pytest.mark.parametrize("fmt", ["f32", "u16"])
def test_the_mask_modes(fmt, fusion, fusion_u16):
    i = mr.masked_inputs(fmt)
    f = fusion_u16 if fmt == "u16" else fusion
    seen = []
    for mode in (0, 1, 2):
        got, _ = check(f, "mask_mode %d" % mode, i["depth"], i["state_in"], i["layer"], i["grid_pose"], i["cam_pose"], dict(i["kw"], mask_mode=mode),
                       mask=i["mask"], fmt=fmt, scale=i["depth_scale"])
        seen.append(got)                                                 # (each check has a memory of its own)
    assert (seen[0]["live_hits"] == seen[1]["live_hits"] + seen[2]["live_hits"]).all()
    for got in seen[1:]:                                                 # the rays do not consult the mask
        assert (got["seen_bits"] == seen[0]["seen_bits"]).all() and (got["seen_tick"] == seen[0]["seen_tick"]).all()
        assert all(got["stats"][k] == seen[0]["stats"][k] for k in ("pixels_valid", "rays", "rays_carving", "ray_samples"))
    assert seen[1]["stats"]["pixels_stamping"] + seen[2]["stats"]["pixels_stamping"] == seen[0]["stats"]["pixels_valid"]


@pytest.mark.parametrize("fmt", ["f32", "u16"])
def test_the_mask_on_partial_pixel_tiles(fmt, fusion, fusion_u16):
    """37 x 29 at stride 3: the threads of a partial tile that lie outside the image read no mask"""
    i = mr.small_inputs(fmt)
    f = fusion_u16 if fmt == "u16" else fusion
    for mode in (1, 2):
        got, _ = check(f, "37x29 mask_mode %d" % mode, i["depth"], i["state_in"], i["layer"], i["grid_pose"], i["cam_pose"], dict(i["kw"], mask_mode=mode),
                       mask=i["mask"], fmt=fmt, scale=i["depth_scale"])
        assert 0 < got["stats"]["pixels_stamping"] < got["stats"]["pixels_valid"] and got["stats"]["cells_newly_marked"] > 0


def test_a_device_mask_inside_guard_bytes(fusion):
    """depth, mask, grid and layer behind device pointers, mask_mode 2: the 37 x 29 mask starts at an odd address between sentinel bytes"""
    import torch
    dev = torch.device("cuda")
    i = mr.small_inputs("f32")
    kw = dict(i["kw"], mask_mode=2)
    c = mr.params(**kw)
    want = mr.update(i["depth"], i["mask"], i["state_in"], i["layer"], i["grid_pose"], i["cam_pose"], c)
    gw, gh, G = c["width"], c["height"], 67
    guarded = np.full(2 * G + i["mask"].size, 0xA5, np.uint8)
    guarded[G:-G] = i["mask"].ravel()
    d_mask = torch.from_numpy(guarded).to(dev)
    d_depth, d_in = torch.from_numpy(i["depth"]).to(dev), torch.from_numpy(i["state_in"]).to(dev)
    d_lay = [torch.from_numpy(i["layer"][nm].view(np.int32)).to(dev) for nm in mr.LAYER]
    out = {nm: torch.zeros((gh, gw), dtype=torch.int8 if nm == "state" else torch.int32, device=dev) for nm in mr.OUTPUTS}
    stats = fusion.nav_memory_device(d_depth, d_in, gw, gh, mask=d_mask.data_ptr() + G, layer_in=d_lay, grid_pose=i["grid_pose"], cam_pose=i["cam_pose"],
                                     **dict({("state_out" if nm == "state" else nm): t for nm, t in out.items()}, **call_kw(kw)), tick=c["tick"])
    got = {nm: t.cpu().numpy().view(want[nm].dtype) for nm, t in out.items()}
    same(dict(got, stats=stats), want, "device mask")
    assert (d_mask.cpu().numpy() == guarded).all() and (d_in.cpu().numpy() == i["state_in"]).all()
    assert all((t.cpu().numpy().view(np.uint32) == i["layer"][nm]).all() for t, nm in zip(d_lay, mr.LAYER))
    assert 0 < stats["pixels_stamping"] < stats["pixels_valid"]


# ---- rays at the ends of a round of 64 samples, sixteen to a wave -----------------------------------------------------------------
@pytest.mark.parametrize("shift", lr.EDGE_SHIFTS)
@pytest.mark.parametrize("tilt", lr.EDGE_TILTS)
def test_rays_that_end_on_both_sides_of_a_round_of_64_samples(tilt, shift, fusion):
    """64 x 2 pixels at stride 1: eight waves of sixteen rays of 49 .. 80 and 113 .. 144 samples (tests/test_navmem.py recomputes them):
    the pending pair merges across the rays of a wave while the carry crosses the rounds of each; tilted, a continued cell brings a new
    bit in most cells, level it brings none.  Shifted, a round ends in the middle of a wave: its pending pair lives across rays of one
    round and of two"""
    i = mr.edge_inputs(tilt, shift)
    got, _ = check(fusion, "round edges, tilt %g, shift %d" % (tilt, shift), i["depth"], i["state_in"], None, i["grid_pose"], i["cam_pose"], i["kw"])
    assert (got["stats"]["rays_carving"], got["stats"]["ray_samples"]) == (126, 12167 if shift == 0 else 12671)
    words = len(np.unique(got["seen_bits"]))
    assert words > 12 if tilt else words == 3


def test_the_boundary_cases(fusion):
    for name, d, at, kw, want in mr.boundary_cases():
        kw = dict(lr.BOUNDARY, **kw)
        got, _ = check(fusion, name, np.full((1, 1), d, np.float32), np.full((4, 8), -1, np.int8), None, nr.IDENTITY, lr.boundary_pose(*at), kw)
        mr.check_expectations(got, want, 8, 4, name)


# ---- contention ----------------------------------------------------------------------------------------------------------------
def test_every_point_in_one_cell(fusion):
    """a constant depth and a lens so long that the whole image lands in one cell and one slice: one run is a whole column"""
    kw = dict(lr.CAMERA, fx=1e6, fy=1e6, width=33, height=31, res=0.05, max_dist_cells=6, stride=4)
    d = np.full((H, W), 1.0, np.float32)
    got, _ = check(fusion, "one cell", d, np.full((31, 33), -1, np.int8), None, lr.grid_pose_at(), lr.room_pose(at=(0.825, 0.0, 0.225)), kw)
    hits = np.zeros((31, 33), np.uint32)
    hits[24, 16] = W * H
    assert (got["live_hits"] == hits).all() and got["stats"]["cells_marked"] == 1 and bin(int(got["marks"][24, 16])).count("1") == 1
    assert got["stats"]["atomics"] < W * H // 4                            # runs of 16 vertically adjacent pixels: two atomics each, and the march's


def test_a_rolled_camera_merges_less_and_counts_the_same(fusion):
    """the wall seen upright and rolled by 90 degrees: pixel columns no longer fall into one cell, the stamp issues more atomics"""
    kw = dict(lr.CAMERA, width=33, height=31, res=0.05, max_dist_cells=6, stride=4)
    d = np.full((H, W), 1.0, np.float32)
    state_in = np.full((31, 33), -1, np.int8)
    up, _ = check(fusion, "upright", d, state_in, None, lr.grid_pose_at(), lr.room_pose(at=(0.8, 0.0, 0.225)), kw)
    rolled, _ = check(fusion, "rolled", d, state_in, None, lr.grid_pose_at(), lr.room_pose(roll=90.0, at=(0.8, 0.0, 0.225)), kw)
    assert up["stats"]["points_in_band"] > 1000 and rolled["stats"]["points_in_band"] > 1000
    assert rolled["stats"]["atomics"] > up["stats"]["atomics"]


def test_rays_longer_than_a_round_of_64_samples(fusion):
    """one pixel, a ray of 159 samples that climbs through the slices (three rounds, the carry crosses them), and the walker's room"""
    kw = dict(lr.BOUNDARY, width=128, height=4, res=0.05, t_max=4.0, slices=32)
    for tilt in (5.0, -5.0):                                             # along map +x, rising or falling by 0.35 m over its 4 m
        cam_pose = nr.pose_about(ncr.ALONG_X @ nr.rot("x", tilt), (0.0125, 0.125, 0.5))
        got, _ = check(fusion, "long ray", np.full((1, 1), 4.0, np.float32), np.full((4, 128), -1, np.int8), None, nr.IDENTITY, cam_pose, kw)
        assert got["stats"]["ray_samples"] > 128 and (got["seen_bits"] != 0).sum() > 64 and len(np.unique(got["seen_bits"])) > 8
    check(fusion, "empty room", mr.walker_depth(None), np.full((64, 65), -1, np.int8), None, mr.WALKER_GRID, mr.WALKER_CAM, mr.WALKER_KW)


# ---- the walker and the low box, the layer fed back in place on the device ------------------------------------------------------
def device_sequence(f, frames, poses, grid_pose, kw):
    """the frames through nav_memory_device with a LiveMemory(device=True), and through the restatement: every frame compared"""
    import torch
    dev = torch.device("cuda")
    c = mr.params(**kw)
    gw, gh = c["width"], c["height"]
    static = np.full((gh, gw), -1, np.int8)
    d_static = torch.from_numpy(static).to(dev)
    mem = binding.LiveMemory(gw, gh, device=True)
    d_state = torch.empty((gh, gw), dtype=torch.int8, device=dev)
    d_dist2 = torch.empty((gh, gw), dtype=torch.int32, device=dev)
    extra = {nm: torch.empty((gh, gw), dtype=torch.int32, device=dev) for nm in ("live_hits", "hit_bits", "seen_bits")}
    layer, out = None, []
    for k, (d, pose) in enumerate(zip(frames, poses)):
        want = mr.update(d, None, static, layer, grid_pose, pose, dict(c, tick=k + 1))
        stats = f.nav_memory_device(torch.from_numpy(d).to(dev), d_static, gw, gh, memory=mem, state_out=d_state, dist2=d_dist2, grid_pose=grid_pose,
                                    cam_pose=pose, **dict(extra, **call_kw(kw)))
        got = dict(mem.numpy(), state=d_state.cpu().numpy(), dist2=d_dist2.cpu().numpy(), stats=stats,
                   **{nm: a.cpu().numpy().view(np.uint32) for nm, a in extra.items()})
        same(got, want, "frame %d" % k)
        assert mem.tick == k + 1 and (d_static.cpu().numpy() == static).all()
        layer = {nm: want[nm] for nm in mr.LAYER}
        out.append(got)
    return out


def test_the_walker_on_the_device(fusion):
    out = device_sequence(fusion, [mr.walker_depth(k) for k in range(mr.WALKER_FRAMES)], [mr.WALKER_CAM] * mr.WALKER_FRAMES, mr.WALKER_GRID, mr.WALKER_KW)
    first, last = out[0], out[-1]
    trail = (first["marks"] != 0) & (last["live_hits"] == 0) & (last["seen_bits"] != 0)
    assert trail.sum() >= 4 and not last["marks"][trail].any()            # where the walker stood first is clear again
    assert all(g["stats"]["cells_cleared"] > 0 for g in out[1:])


def test_the_low_box_on_the_device(fusion):
    for slices, kept in ((16, True), (1, False)):
        a, b = device_sequence(fusion, [mr.lowbox_depth(0), mr.lowbox_depth(1)], mr.LOWBOX_POSES, mr.LOWBOX_GRID, dict(mr.LOWBOX_KW, slices=slices))
        crossed = (a["marks"] != 0) & (np.arange(64)[:, None] < mr.LOWBOX_ROWS) & (b["seen_bits"] != 0)
        assert crossed.sum() >= 10 and (b["marks"][crossed] != 0).all() == kept and (b["marks"][crossed] != 0).any() == kept


# ---- identity (a): the device's own stateless overlay ------------------------------------------------------------------------------
@pytest.mark.parametrize("slices", [1, 16, 32])
def test_a_zero_layer_without_ages_is_the_devices_own_overlay(slices, fusion):
    i = lr.case_inputs("room yaw pitch roll", "f32", 4)
    kw = dict(call_kw(i["kw"]), grid_pose=i["grid_pose"], cam_pose=i["cam_pose"])
    live = fusion.nav_live(i["depth"], i["state_in"], min_seen=1, **kw)
    got = fusion.nav_memory(i["depth"], i["state_in"], slices=slices, **kw)
    for nm in ("state", "dist2", "live_hits"):
        assert (got[nm] == live[nm]).all(), nm
    assert ((got["seen_bits"] != 0) == (live["live_seen"] >= 1)).all() and live["stats"]["cells_stamped"] > 0
    for nm in ("pixels_valid", "pixels_stamping", "points_in_band", "rays", "rays_carving", "ray_samples", "cells_opened", "cells_free", "cells_occupied"):
        assert got["stats"][nm] == live["stats"][nm], nm


def test_without_a_valid_pixel_the_layer_is_a_fixed_point(fusion):
    i = lr.case_inputs("noise", "f32", 4)
    kw = dict(i["kw"], tick=77)
    layer = mr.random_layer(33, 31, 1, 77, 40, 25)
    got, _ = check(fusion, "no valid pixel", np.zeros((H, W), np.float32), i["state_in"], layer, i["grid_pose"], i["cam_pose"], kw)
    for nm in mr.LAYER:
        assert (got[nm] == layer[nm]).all(), nm


# ---- the handle's defaults and cameras that see nothing ----------------------------------------------------------------------------
def test_the_default_frame_and_camera_are_the_handles(mem_lib):
    """grid_pose None = nav_grid_default_pose now, cam_pose None = the tracked pose, cam_width 0 = cfg's camera, t = cfg's range"""
    f = handle(mem_lib)
    rgb, depth = util.frame(0, W, H)
    f.process_frame(rgb, depth)
    K = util.synthetic.intrinsics(W, H)
    kw = dict(width=65, height=64, res=0.1, max_dist_cells=7, stride=8, slices=9, tick=mr.GPU_TICK, **mr.GPU_AGES)
    c = mr.params(cfg_camera=K, **kw)
    grid_pose = nr.default_pose(f.get_pose(), c)
    state_in = np.full((64, 65), -1, np.int8)
    layer = mr.random_layer(65, 64, 5, mr.GPU_TICK, slices=9, **mr.GPU_AGES)
    want = mr.update(depth, None, state_in, layer, grid_pose, f.get_pose(), c)
    mem = host_memory(layer, 65, 64, mr.GPU_TICK)
    got = f.nav_memory(depth, state_in, memory=mem, **call_kw(kw))
    same(got, want, "defaults")
    assert (got["stats"]["pose"] == grid_pose).all() and (f.nav_grid_default_pose(width=65, height=64, res=0.1) == grid_pose).all()
    assert got["stats"]["points_in_band"] > 0 and got["stats"]["ray_samples"] > 0 and got["stats"]["bits_cleared"] > 0 and mem.tick == mr.GPU_TICK
    f.close()


def test_a_camera_outside_the_grid_and_a_pose_that_is_not_finite(fusion):
    """no point and no sample reaches the grid: only ageing changes the layer"""
    i, _ = mr.case_evidence("room straight", "f32", 4)
    kw = dict(i["kw"], slices=5, tick=mr.GPU_TICK, **mr.GPU_AGES)
    c = mr.params(**kw)
    layer = mr.random_layer(c["width"], c["height"], 3, mr.GPU_TICK, slices=5, **mr.GPU_AGES)
    zero = np.zeros((c["height"], c["width"]), np.uint32)
    aged = mr.cells_rule(zero, zero, zero, i["state_in"], layer, c)

    def only_ageing(got, what):
        assert not got["live_hits"].any() and not got["hit_bits"].any() and not got["seen_bits"].any(), what
        assert all((got[nm] == aged[nm]).all() for nm in mr.LAYER + ("state",)), what
        s = got["stats"]
        assert all(s[k] == n for k, n in aged["stats"].items()), (what, s, aged["stats"])
        assert s["cells_expired"] > 0 and s["cells_cleared"] == 0 == s["bits_cleared"] == s["cells_newly_marked"] and s["pixels_valid"] > 0 and s["rays"] > 0, what
    got, _ = check(fusion, "outside", i["depth"], i["state_in"], layer, i["grid_pose"], lr.room_pose(at=(40.0, 0.0, -30.0)), kw)
    only_ageing(got, "outside")
    assert got["stats"]["points_in_band"] == 0 and got["stats"]["rays_carving"] > 0 and got["stats"]["ray_samples"] > 0
    for k, bad in ((0, np.nan), (4, np.inf), (9, np.nan), (11, -np.inf)):
        pose = i["cam_pose"].copy()
        pose[k] = bad
        got, _ = check(fusion, "pose[%d] = %s" % (k, bad), i["depth"], i["state_in"], layer, i["grid_pose"], pose, kw)
        only_ageing(got, "pose[%d] = %s" % (k, bad))
        assert got["stats"]["rays_carving"] == 0 == got["stats"]["ray_samples"] == got["stats"]["points_in_band"] or k == 0
    got, _ = check(fusion, "after the poses", i["depth"], i["state_in"], layer, i["grid_pose"], i["cam_pose"], kw)
    assert got["stats"]["cells_newly_marked"] > 0 and got["stats"]["bits_cleared"] > 0


# ---- pointers and outputs --------------------------------------------------------------------------------------------------------
def random_case(slices=5):
    i, ev = mr.case_evidence("room yaw pitch roll", "u16", 4)
    kw = dict(i["kw"], slices=slices, tick=mr.GPU_TICK, **mr.GPU_AGES)
    c = mr.params(**kw)
    lay = mr.random_layer(c["width"], c["height"], 3, mr.GPU_TICK, slices=slices, **mr.GPU_AGES)
    return i, kw, c, lay, mr.update_from(ev, i["state_in"], lay, c)


def test_device_pointers_in_place_and_out_of_place(fusion_u16):
    import torch
    dev = torch.device("cuda")
    f = fusion_u16
    i, kw, c, lay, want = random_case()
    gw, gh = c["width"], c["height"]
    ckw = dict(call_kw(kw), grid_pose=i["grid_pose"], cam_pose=i["cam_pose"], tick=mr.GPU_TICK)
    d_depth = torch.from_numpy(i["depth"].view(np.int16)).to(dev)
    d_in = torch.from_numpy(i["state_in"]).to(dev)
    up = lambda a: torch.from_numpy(a.view(np.int32)).to(dev)
    names = {"state": "state_out"}
    torch_dt = {np.dtype(np.uint32): torch.int32, np.dtype(np.int32): torch.int32, np.dtype(np.int8): torch.int8}

    def run(asked, in_place=False, layer=lay):
        d_lay = None if layer is None else [up(layer[nm]) for nm in mr.LAYER]
        o = {nm: torch.full((gh, gw), 0x5A if nm == "state" else 0x5A5A5A5A, dtype=torch_dt[want[nm].dtype], device=dev) for nm in mr.OUTPUTS}
        if in_place:
            o.update(zip(mr.LAYER, d_lay))
            o["state"] = d_in.clone()
        st = f.nav_memory_device(d_depth, o["state"] if in_place else d_in, gw, gh, layer_in=d_lay, **dict({names.get(nm, nm): o[nm] for nm in asked}, **ckw))
        got = {nm: o[nm].cpu().numpy().view(want[nm].dtype) for nm in mr.OUTPUTS}
        for nm in mr.OUTPUTS:
            if nm not in asked and not (in_place and nm in mr.LAYER + ("state",)):
                assert (o[nm].cpu().numpy() == (0x5A if nm == "state" else 0x5A5A5A5A)).all(), (asked, nm, "written though not asked for")
        if not in_place and layer is not None:
            assert all((t.cpu().numpy().view(np.uint32) == layer[nm]).all() for t, nm in zip(d_lay, mr.LAYER)), "the input layer was written"
        got["stats"] = st
        return got
    same(run(mr.OUTPUTS), want, "device pointers, out of place")
    same(run(mr.OUTPUTS, in_place=True), want, "device pointers, in place")
    for left_out in mr.OUTPUTS:                                          # each output NULL in turn
        asked = tuple(nm for nm in mr.OUTPUTS if nm != left_out)
        same(run(asked), want, "without " + left_out, outputs=asked)
    same(run(("dist2",)), want, "dist2 alone", outputs=("dist2",))
    same(run(("marks",), in_place=True), want, "marks alone, in place", outputs=("marks",))
    # a NULL layer and a layer of three NULL arrays are the zero layer
    zero = mr.update_from(mr.case_evidence("room yaw pitch roll", "u16", 4)[1], i["state_in"], None, c)
    same(run(mr.OUTPUTS, layer=None), zero, "layer_in NULL")
    st = f.nav_memory_device(d_depth, d_in, gw, gh, layer_in=[None, None, None], state_out=d_in.clone(), **ckw)
    assert {k: st[k] for k in mr.STATS} == zero["stats"]
    # host frame, device grid; host arrays out of place
    t = torch.zeros((gh, gw), dtype=torch.int32, device=dev)
    f.nav_memory_device(i["depth"], d_in, gw, gh, layer_in=[up(lay[nm]) for nm in mr.LAYER], dist2=t, frame_on_device=False, **ckw)
    assert (t.cpu().numpy() == want["dist2"]).all()
    p, keep = f._navmem_params(False, False, width=gw, height=gh, **ckw)
    out = {nm: np.zeros((gh, gw), want[nm].dtype) for nm in mr.OUTPUTS}
    before = {nm: lay[nm].copy() for nm in mr.LAYER}
    st = f._navmem_update(p, binding._ptr(i["depth"]), None, binding._ptr(i["state_in"]), [binding._ptr(lay[nm]) for nm in mr.LAYER],
                          {nm: binding._ptr(a) for nm, a in out.items()})
    same(dict(out, stats=st), want, "host arrays, out of place")
    assert all((lay[nm] == before[nm]).all() for nm in mr.LAYER)


# ---- the staging of host arrays: twelve in one buffer ----------------------------------------------------------------------------
_STAGING = {}


def staging_case(gw, gh):
    """dict(depth, state_in, layer, grid_pose, cam_pose, kw, want): test_image_and_grid_shapes' noise frame of 37 x 29 pixels over a
    grid of gw x gh cells that holds the camera, with a random layer and both ages; the restatement's answer, computed once and shared"""
    if (gw, gh) not in _STAGING:
        w, h = 37, 29
        res, corner = (0.05, (0.0, 0.0)) if gw >= 31 else (0.25, (0.0, 0.0)) if gw >= 8 else (0.5, (0.6, 0.3))
        kw = dict(fx=60.0, fy=60.0, cx=0.5 * (w - 1), cy=0.5 * (h - 1), cam_width=w, cam_height=h, t_min=0.2, t_max=5.0, width=gw, height=gh, res=res,
                  max_dist_cells=5, stride=3, min_hits=3, slices=7, tick=9, max_mark_age=3, max_seen_age=2)
        c = dict(depth=lr.noise_depth(w, h, 7 * w + h, lo=0.1, hi=1.6), state_in=lr.state_pattern(gw, gh, gw + w), layer=mr.random_layer(gw, gh, gw, 9, 3, 2, slices=7),
                 grid_pose=lr.grid_pose_at(*corner), cam_pose=lr.room_pose(yaw=8.0, roll=2.0, at=(0.8, 0.1, 0.35)), kw=kw)
        c["want"] = mr.update(c["depth"], None, c["state_in"], c["layer"], c["grid_pose"], c["cam_pose"], mr.params(**kw))
        _STAGING[gw, gh] = c
    return _STAGING[gw, gh]


def memory_host(f, c, names, in_place=False):
    """ssf_navmem_update with host arrays, the outputs `names` alone, each between guard bytes and filled with them; in_place: the
    layer's outputs are its inputs and state is state_in, whatever `names` says of them.  Returns (name -> array, stats)"""
    gw, gh = c["kw"]["width"], c["kw"]["height"]
    out = {nm: util.guarded((gh, gw), dt) for nm, dt in binding.NAVMEM_OUTPUTS if nm in names or (in_place and nm in mr.LAYER + ("state",))}
    ins = {nm: c["layer"][nm].copy() for nm in mr.LAYER}
    ins["state"] = c["state_in"].copy()
    if in_place:
        for nm in ins:
            out[nm][0][...] = ins[nm]
        ins = {nm: out[nm][0] for nm in ins}
    p, keep = f._navmem_params(False, False, width=gw, height=gh, grid_pose=c["grid_pose"], cam_pose=c["cam_pose"], tick=c["kw"]["tick"], **call_kw(c["kw"]))
    stats = f._navmem_update(p, binding._ptr(c["depth"]), None, binding._ptr(ins["state"]), [binding._ptr(ins[nm]) for nm in mr.LAYER],
                             {nm: binding._ptr(a) for nm, (a, _) in out.items()})
    assert all(intact() for _, intact in out.values()), names
    assert in_place or ((ins["state"] == c["state_in"]).all() and all((ins[nm] == c["layer"][nm]).all() for nm in mr.LAYER)), "an input was written"
    return {nm: a for nm, (a, _) in out.items()}, stats


@pytest.mark.parametrize("gw,gh", [(37, 19), (1, 1)])
def test_host_arrays_whose_items_all_start_at_rounded_offsets(gw, gh, fusion):
    """703 cells and one cell, a frame of 37 x 29 pixels: neither P nor 4 P nor 4 times the pixels is a multiple of 256, so each of the
    twelve arrays behind the first sits at a rounded offset of the one staging buffer.  Host arrays, device pointers and the
    restatement agree"""
    import torch
    c = staging_case(gw, gh)
    host, hs = memory_host(fusion, c, mr.OUTPUTS)
    same(dict(host, stats=hs), c["want"], "host %d x %d" % (gw, gh))
    t = {nm: torch.full((gh, gw), 0x5A, dtype=torch.int8 if dt is np.int8 else torch.int32, device="cuda") for nm, dt in binding.NAVMEM_OUTPUTS}
    up = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda")
    ds = fusion.nav_memory_device(up(c["depth"]), up(c["state_in"]), gw, gh, layer_in=[up(c["layer"][nm]) for nm in mr.LAYER], grid_pose=c["grid_pose"],
                                  cam_pose=c["cam_pose"], tick=c["kw"]["tick"], **dict({("state_out" if nm == "state" else nm): a for nm, a in t.items()}, **call_kw(c["kw"])))
    assert all(host[nm].tobytes() == t[nm].cpu().numpy().tobytes() for nm in mr.OUTPUTS) and {k: hs[k] for k in mr.STATS} == {k: ds[k] for k in mr.STATS}
    s = c["want"]["stats"]
    assert s["rays"] > 64 and (gw == 1 or (s["points_in_band"] > 0 and s["cells_remembered"] > 0 and s["cells_expired"] > 0))


@pytest.mark.parametrize("name", mr.OUTPUTS)
def test_one_host_output_alone_between_guard_bytes(name, fusion):
    """37 x 19, host arrays: each of the eight outputs on its own, all others NULL, equals the same array of the call that asks for
    all of them, and the 256 bytes on either side of the caller's array are untouched"""
    c = staging_case(37, 19)
    if "every" not in c:
        c["every"] = memory_host(fusion, c, mr.OUTPUTS)
    every, stats = c["every"]
    same(dict(every, stats=stats), c["want"], "every output")
    alone, st = memory_host(fusion, c, (name,))
    assert alone[name].tobytes() == every[name].tobytes() and {k: st[k] for k in mr.STATS} == {k: stats[k] for k in mr.STATS}, name


def test_host_arrays_updated_in_place(fusion):
    """37 x 19, host arrays: the layer's three outputs are its inputs and state is state_in.  Each pair is two items of the staging
    buffer, so the update reads what the caller had and the caller gets what a call out of place gives"""
    c = staging_case(37, 19)
    got, stats = memory_host(fusion, c, mr.OUTPUTS, in_place=True)
    same(dict(got, stats=stats), c["want"], "in place")
    few, stats = memory_host(fusion, c, ("dist2",), in_place=True)        # the other five NULL
    same(dict(few, stats=stats), c["want"], "in place, dist2", outputs=mr.LAYER + ("state", "dist2"))
    assert (c["want"]["state"] != c["state_in"]).any() and any((c["want"][nm] != c["layer"][nm]).any() for nm in mr.LAYER)


def test_the_staging_buffer_grows_and_is_used_again(mem_lib):
    """one handle: 8 x 8, 37 x 19, 8 x 8 again.  Each call gives what a handle that has made no other call gives"""
    f = handle(mem_lib)
    for gw, gh in ((8, 8), (37, 19), (8, 8)):
        c = staging_case(gw, gh)
        fresh = handle(mem_lib)
        (got, gs), (want, ws) = memory_host(f, c, mr.OUTPUTS), memory_host(fresh, c, mr.OUTPUTS)
        fresh.close()
        assert all(got[nm].tobytes() == want[nm].tobytes() for nm in mr.OUTPUTS) and {k: gs[k] for k in mr.STATS} == {k: ws[k] for k in mr.STATS}, (gw, gh)
        same(dict(got, stats=gs), c["want"], (gw, gh))
    f.close()


def test_a_call_between_two_frames_changes_no_later_result(mem_lib):
    import torch
    A, B = handle(mem_lib), handle(mem_lib)
    state_in = np.full((64, 65), -1, np.int8)
    mem, dmem = binding.LiveMemory(65, 64), binding.LiveMemory(65, 64, device=True)
    for k in (0, 3, 6):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        A.nav_memory(depth, state_in, memory=mem, res=0.1, stride=8, max_mark_age=1)
        A.nav_memory_plan(depth, state_in, dmem, [(30, 30)], [(32, 32)], waypoints=True, live=dict(res=0.1), plan=dict(allow_unknown=1, max_path=100))
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)
    assert mem.tick == 3 == dmem.tick and mem.marks.any() and dmem.numpy()["marks"].any()
    mem.clear(); dmem.clear()
    assert mem.tick == 0 == dmem.tick and not mem.marks.any() and not any(a.any() for a in dmem.numpy().values())
    B.close()
    A.close()


def test_the_refusals(mem_lib):
    import torch
    f = handle(mem_lib)
    i, ev = mr.case_evidence("room straight", "f32", 4)
    base = dict(call_kw(i["kw"]), grid_pose=i["grid_pose"], cam_pose=i["cam_pose"])
    depth, state_in = i["depth"], i["state_in"]
    want = mr.update_from(ev, state_in, None, mr.params(**i["kw"]))
    refused = pytest.raises(binding.SsfError, match=r"ssf_navmem_update failed \(-1\)")
    nan, inf = float("nan"), float("inf")
    for kw in (dict(res=0.0), dict(res=nan), dict(res=inf), dict(res=-0.05), dict(max_dist_cells=0), dict(max_dist_cells=1025), dict(min_hits=0),
               dict(floor_max=nan), dict(z_max=nan), dict(cam_width=8193), dict(cam_height=0), dict(cam_height=8193), dict(fx=0.0), dict(fy=-1.0),
               dict(fx=nan), dict(fy=inf), dict(cx=inf), dict(cy=nan), dict(stride=0), dict(stride=65), dict(hit_margin_cells=-0.5),
               dict(hit_margin_cells=nan), dict(hit_margin_cells=inf), dict(t_min=0.0, t_max=3.0), dict(t_min=-1.0, t_max=3.0),
               dict(t_min=2.0, t_max=2.0), dict(t_min=3.0, t_max=2.0), dict(t_min=nan, t_max=2.0), dict(t_min=0.2, t_max=inf), dict(mask_mode=3),
               dict(mask_mode=-1), dict(mask_mode=1), dict(mask_mode=2), dict(t_min=0.2, t_max=2000.0),
               # the memory's own
               dict(tick=0), dict(slices=0), dict(slices=33), dict(slices=-1), dict(floor_max=inf), dict(floor_max=-inf), dict(z_max=inf),
               dict(z_max=-0.8), dict(z_max=-0.9), dict(floor_max=-3e38, z_max=3e38), dict(floor_max=0.0, z_max=1e-45, slices=32)):
        with refused:
            image = np.zeros((kw.get("cam_height", H), kw.get("cam_width", W)), np.float32) if "cam_width" in kw or "cam_height" in kw else depth
            f.nav_memory(image, state_in, **dict(base, **kw))
    with refused:                                                        # the stride leaves no lattice
        f.nav_memory(np.ones((5, 13), np.float32), state_in, **dict(base, cam_width=13, cam_height=5, stride=8))
    with refused:
        f.nav_memory(depth, state_in, outputs=(), **base)                 # every output NULL
    with refused:
        f.nav_memory(depth, np.zeros((1, 4097), np.int8), **base)
    with pytest.raises(binding.SsfError, match="unknown memory parameter 'min_seen'"):
        f.nav_memory(depth, state_in, min_seen=2, **base)
    f.nav_memory(depth, state_in, **dict(base, tick=0xFFFFFFFF, max_mark_age=0xFFFFFFFF))
    # device pointers: alignment for the format, and overlaps
    dev = torch.device("cuda")
    gw, gh = i["kw"]["width"], i["kw"]["height"]
    P = gw * gh
    d_depth = torch.zeros(W * H + 8, dtype=torch.float32, device=dev)
    d_in = torch.from_numpy(state_in).to(dev)
    buf = torch.zeros(8 * P + 64, dtype=torch.int32, device=dev)
    a = buf.data_ptr()
    with refused:
        f.nav_memory_device(d_depth.data_ptr() + 2, d_in, gw, gh, dist2=a, **base)
    f.nav_memory_device(d_depth.data_ptr() + 4, d_in, gw, gh, dist2=a, **base)
    lay = [a + 4 * P * k for k in range(3)]
    for out in (dict(marks=a, mark_tick=a), dict(live_hits=a, dist2=a + 4 * P - 4), dict(dist2=a, state_out=a + 4), dict(state_out=d_in.data_ptr() + 1),
                dict(seen_bits=d_in.data_ptr()), dict(dist2=d_depth.data_ptr() + 4 * W * H - 4), dict(hit_bits=d_depth.data_ptr()),
                # the layer: an output on ANOTHER input of the layer, or shifted against its own
                dict(layer_in=lay, marks=lay[1]), dict(layer_in=lay, mark_tick=lay[0]), dict(layer_in=lay, seen_tick=lay[2] + 4),
                dict(layer_in=lay, dist2=lay[0]), dict(layer_in=lay, live_hits=lay[2] + 4 * P - 4)):
        with refused:
            f.nav_memory_device(d_depth, d_in, gw, gh, **dict(out, **base))
    f.nav_memory_device(d_depth, d_in, gw, gh, layer_in=lay, marks=lay[0], mark_tick=lay[1], seen_tick=lay[2], state_out=d_in, **base)      # in place
    # the mask is one of the arrays only when it is read: an output on its first byte alone, on its last alone, and beside it
    mbuf = torch.zeros(2 * P + W * H, dtype=torch.uint8, device=dev)
    m = mbuf.data_ptr() + P
    for ptr in (m - P + 1, m + W * H - 1, m):
        with refused:
            f.nav_memory_device(d_depth, d_in, gw, gh, mask=m, state_out=ptr, **dict(base, mask_mode=2))
        assert mem_lib.lib.ssf_last_error(f.h).decode() == ("ssf_navmem_update: arrays overlap (only an output of the layer on its own input, and "
                                                            "state == state_in, may)")
    with refused:
        f.nav_memory_device(d_depth, d_in, gw, gh, mask=m, seen_bits=m + W * H - 4, **dict(base, mask_mode=1))
    assert not mbuf.any()                                                # refused before any kernel
    for ptr in (m - P, m + W * H):
        f.nav_memory_device(d_depth, d_in, gw, gh, mask=m, state_out=ptr, **dict(base, mask_mode=2))
    for ptr in (m - P + 1, m + W * H - 1, m):
        f.nav_memory_device(d_depth, d_in, gw, gh, mask=m, state_out=ptr, **dict(base, mask_mode=0))
    with pytest.raises(binding.SsfError, match="LiveMemory"):
        f.nav_memory_device(d_depth, d_in, gw, gh, memory=binding.LiveMemory(gw, gh), dist2=a, **base)
    with pytest.raises(binding.SsfError, match="LiveMemory"):
        f.nav_memory(depth, state_in, memory=binding.LiveMemory(gw + 1, gh), **base)
    # the C entry points themselves
    L, byref, vp = mem_lib.lib, binding.C.byref, binding.C.c_void_p
    p, st = binding.SsfNavMemParams(), binding.SsfNavMemStats()
    assert L.ssf_navmem_default_params(f.h, byref(p)) == 0
    assert L.ssf_navmem_default_params(None, byref(p)) == -1 and L.ssf_navmem_default_params(f.h, None) == -1
    live = f.nav_live_default_params()
    assert f.nav_memory_default_params() == dict({k: v for k, v in live.items() if k != "min_seen"}, slices=16, tick=1, max_mark_age=0, max_seen_age=0)
    p.width, p.height = 8, 4
    dd, s8, o8 = np.ones((H, W), np.float32), np.zeros((4, 8), np.int8), np.zeros((4, 8), np.int8)
    out = binding.SsfNavMemOut()
    out.state = o8.ctypes.data
    d, s = dd.ctypes.data_as(vp), s8.ctypes.data_as(vp)
    assert L.ssf_navmem_update(f.h, byref(p), d, None, s, None, byref(out), None) == 0          # the layer and the stats are optional
    assert L.ssf_navmem_update(None, byref(p), d, None, s, None, byref(out), byref(st)) == -1
    assert L.ssf_navmem_update(f.h, None, d, None, s, None, byref(out), byref(st)) == -1
    assert L.ssf_navmem_update(f.h, byref(p), None, None, s, None, byref(out), byref(st)) == -1
    assert L.ssf_navmem_update(f.h, byref(p), d, None, None, None, byref(out), byref(st)) == -1
    assert L.ssf_navmem_update(f.h, byref(p), d, None, s, None, None, byref(st)) == -1
    assert L.ssf_navmem_update(f.h, byref(p), d, None, s, None, byref(binding.SsfNavMemOut()), byref(st)) == -1
    for field, bad in (("width", 0), ("width", 4097), ("height", -3), ("height", 4097), ("tick", 0), ("slices", 33)):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert L.ssf_navmem_update(f.h, byref(p), d, None, s, None, byref(out), byref(st)) == -1, (field, bad)
        setattr(p, field, keep)
    # the handle keeps working: a call and a frame after the refusals
    check(f, "after the refusals", depth, state_in, None, i["grid_pose"], i["cam_pose"], i["kw"], want=want)
    f.process_frame(*util.frame(0, W, H))
    check(f, "after a frame", depth, state_in, None, i["grid_pose"], i["cam_pose"], i["kw"], want=want)
    g = handle(mem_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_memory(depth, state_in, **base)
    q = handle(mem_lib, pipeline_depth=2, extract_batch=2)
    q.submit_frame(*util.frame(0, W, H))
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q.nav_memory(depth, state_in, **base)
    q.process_submitted()
    check(q, "pipelined, at rest", depth, state_in, None, i["grid_pose"], i["cam_pose"], i["kw"], want=want)
    q.close()
    g.close()
    f.close()


def test_the_refusal_texts(mem_lib):
    """Every refusal of ssf_navmem_update by its exact ssf_last_error text (as the entry point's source had them before the refusals it
    shares with ssf_navlive_overlay moved into one place), on the 8 x 4 grid and the handle-size image of test_the_refusals: a row
    violates one parameter; the last two violate two, one on each side of the memory's own checks (the tick, the slices and the finite
    band, between the grid and the camera), which pins the order.  All are refused before any kernel."""
    f = handle(mem_lib)
    L, byref, vp = mem_lib.lib, binding.C.byref, binding.C.c_void_p
    dd, s8, o8 = np.ones((H, W), np.float32), np.zeros((4, 8), np.int8), np.zeros((4, 8), np.int32)
    inf = float("inf")
    cam = dict(cam_width=W, cam_height=H, fx=100.0, fy=100.0, cx=80.0, cy=64.0)
    rows = [(dict(depth=None), "depth is NULL"), (dict(state_in=None), "state_in is NULL"), (dict(state=None), "every output is NULL"),
            (dict(width=0), "the grid's size must be 1..4096 x 1..4096"), (dict(res=0.0), "res must be finite and > 0"),
            (dict(max_dist_cells=0), "max_dist_cells must be 1..1024"), (dict(min_hits=0), "min_hits must be >= 1"),
            (dict(tick=0), "tick must be >= 1"), (dict(slices=33), "slices must be 1..32"),
            (dict(floor_max=inf), "floor_max and z_max must be finite"), (dict(z_max=-0.9), "z_max must be > floor_max"),
            (dict(floor_max=0.0, z_max=1e-45, slices=32), "(z_max - floor_max) / slices must be finite and > 0"),
            (dict(cam, cam_width=8193), "cam_width and cam_height must be 1..8192"),
            (dict(cam, fx=-1.0), "fx and fy must be finite and > 0, cx and cy finite"), (dict(stride=0), "stride must be 1..64"),
            (dict(cam, cam_width=13, cam_height=5, stride=8), "the stride leaves no pixel lattice"),
            (dict(hit_margin_cells=-0.5), "hit_margin_cells must be finite and >= 0"),
            (dict(t_min=3.0, t_max=2.0), "the range needs 0 < t_min < t_max, both finite"), (dict(mask_mode=3), "mask_mode must be 0..2"),
            (dict(mask_mode=1), "mask is NULL with mask_mode != 0"),
            (dict(frame_on_device=1, depth=dd.ctypes.data + 2), "the device depth pointer is not aligned for the input format"),
            (dict(t_min=0.2, t_max=2000.0), "(t_max * l) / (res / 2) must be <= 65535 at the image's corners"),
            (dict(dist2=o8.ctypes.data), "arrays overlap (only an output of the layer on its own input, and state == state_in, may)"),
            (dict(min_hits=0, tick=0), "min_hits must be >= 1"), (dict(slices=0, stride=0), "slices must be 1..32")]
    for bad, text in rows:
        p, out = binding.SsfNavMemParams(), binding.SsfNavMemOut()
        assert L.ssf_navmem_default_params(f.h, byref(p)) == 0
        p.width, p.height = 8, 4
        arg = dict(depth=dd.ctypes.data, state_in=s8.ctypes.data, state=o8.ctypes.data, dist2=None)
        for k, v in bad.items():
            if k in arg:
                arg[k] = v
            else:
                setattr(p, k, v)
        out.state, out.dist2 = arg["state"], arg["dist2"]
        rc = L.ssf_navmem_update(f.h, byref(p), vp(arg["depth"]), None, vp(arg["state_in"]), None, byref(out), None)
        got = L.ssf_last_error(f.h).decode()
        print(bad, rc, got)
        assert rc == -1 and got == "ssf_navmem_update: " + text, (bad, rc, got)
    f.close()


def test_the_kernels_are_timed_under_profile(mem_lib):
    f = handle(mem_lib, profile=1)
    f.reset_kernel_times()
    i, ev = mr.case_evidence("room straight", "f32", 4)
    check(f, "profiled", i["depth"], i["state_in"], None, i["grid_pose"], i["cam_pose"], i["kw"], want=mr.update_from(ev, i["state_in"], None, mr.params(**i["kw"])))
    names = f.kernel_times()
    for k in ("navmem_stamp", "navmem_march", "navmem_cells", "navgrid_columns", "navgrid_rows"):
        assert k in names and names[k][1] > 0, (k, names)
    assert not [k for k in names if k.startswith("navlive_")]
    f.reset_kernel_times()
    f.nav_memory(i["depth"], i["state_in"], outputs=("marks", "state"), grid_pose=i["grid_pose"], cam_pose=i["cam_pose"], **call_kw(i["kw"]))
    names = f.kernel_times()
    assert "navmem_march" in names and "navgrid_rows" not in names       # nothing asked for the clearance
    f.close()


# ---- the chains ------------------------------------------------------------------------------------------------------------------
def test_update_plan_and_waypoints_without_the_grid_leaving_the_device(fusion):
    """nav_memory_plan over two frames of the walker against the restatements chained on the host: the plan goes round the walker where it
    stands, and through where it stood"""
    kw = mr.WALKER_KW
    c = mr.params(**kw)
    static = np.zeros((64, 65), np.int8)                                 # the map knows a free floor and nothing of wall and walker
    static[:, :2] = -1
    mem = binding.LiveMemory(65, 64, device=True)
    goals, starts = [(31, 42)], [(31, 10), (12, 12)]
    plan, wq = dict(min_dist2=1, max_path=400), dict(keep_clearance=1, clearance_cap=4, lookahead=64)
    layer, paths = None, []
    for k, frame in enumerate((2, 5)):
        d = mr.walker_depth(frame)
        lv = mr.update(d, None, static, layer, mr.WALKER_GRID, mr.WALKER_CAM, dict(c, tick=k + 1))
        layer = {nm: lv[nm] for nm in mr.LAYER}
        got = fusion.nav_memory_plan(d, static, mem, goals, starts, waypoints=True, live=dict(call_kw(kw), grid_pose=mr.WALKER_GRID, cam_pose=mr.WALKER_CAM),
                                     plan=plan, waypoint_params=wq)
        assert (got["live"]["state"] == lv["state"]).all() and (got["live"]["dist2"] == lv["dist2"]).all()
        assert {nm: got["live"]["stats"][nm] for nm in mr.STATS} == lv["stats"] and mem.tick == k + 1
        assert all((a == layer[nm]).all() for nm, a in mem.numpy().items())
        pl = pr.plan(lv["state"], lv["dist2"], goals, starts, **plan)
        for nm in ("start_cost", "start_status", "path_len"):
            assert (got["plan"][nm] == pl[nm]).all(), nm
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got["plan"]["path"], pl["path"]))
        wp = wr.waypoints(lv["state"], lv["dist2"], pl["path"], min_dist2=1, max_waypoints=400, **wq)
        for nm in ("n_waypoints", "status", "path_min"):
            assert (got["waypoints"][nm] == wp[nm]).all(), nm
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got["waypoints"]["waypoints"], wp["waypoints"]))
        paths.append(lv)
    assert paths[0]["stats"]["cells_marked"] > 0 and paths[1]["stats"]["cells_cleared"] > 0
    stood = (paths[0]["marks"] != 0) & (paths[1]["live_hits"] == 0) & (paths[1]["seen_bits"] != 0)
    assert stood.sum() >= 4 and (paths[1]["state"][stood] == 0).all()
    with pytest.raises(binding.SsfError, match="LiveMemory\\(device=True\\)"):
        fusion.nav_memory_plan(mr.walker_depth(2), static, binding.LiveMemory(65, 64), goals, starts)


def test_nav_memory_dyn_steer_is_the_chain_of_its_calls(mem_lib):
    """motion mask, update without the movers' stamps, blobs, tracker, plan, rollouts in one call, against the same calls made one by one
    with host arrays on a second handle with the same map"""
    A, B = handle(mem_lib), handle(mem_lib)
    for k in (0, 3):
        rgb, depth = util.frame(k, W, H)
        A.process_frame(rgb, depth)
        B.process_frame(rgb, depth)
    rgb, depth = util.frame(6, W, H)
    near = depth.copy()
    near[30:100, 50:110] = np.minimum(near[30:100, 50:110], np.float32(0.6))                          # something stands in front of the map
    grid = A.nav_grid(outputs=("state", "dist2"), res=0.1)
    pose, state = grid["stats"]["pose"], grid["state"]
    gh, gw = state.shape
    poses = binding.Fusion.nav_steer_units([(gw * 0.05, gh * 0.05, 0.0)], 0.1)
    goals = [(gw // 2 + 5, gh // 2)]
    ta, tb = binding.MoverTracker(inflate=200), binding.MoverTracker(inflate=200)
    ma, mb = binding.LiveMemory(gw, gh, device=True), binding.LiveMemory(gw, gh)
    steer_kw = dict(n_steps=12, mover_weight=3)
    mkw = dict(grid_pose=pose, res=0.1, min_hits=2, stride=8, slices=8, max_mark_age=1)
    for step, img in enumerate((near, depth, near)):
        got = A.nav_memory_dyn_steer(img, state, ma, goals, poses, ta, steps_since=2, live=mkw, blobs=dict(min_points=8), plan=dict(min_dist2=1),
                                     steer=steer_kw)
        mm = B.motion_mask(img, outputs=("mask", "label"))
        assert got["motion"]["stats"] == mm["stats"]
        lv = B.nav_memory(img, state, memory=mb, mask=mm["mask"], mask_mode=2, **mkw)
        assert {k: got["live"]["stats"][k] for k in mr.STATS} == {k: lv["stats"][k] for k in mr.STATS}          # (atomics: informative only)
        assert ma.tick == mb.tick == step + 1 and all((a == b).all() for a, b in zip(ma.numpy().values(), mb.arrays()))
        table = B.nav_dyn_blobs(img, mm["mask"], mm["label"], grid_pose=pose, res=0.1, width=gw, height=gh, min_points=8)
        assert (got["blobs"]["blobs"] == table["blobs"]).all() and got["blobs"]["stats"] == table["stats"]
        movers = tb.update(table["blobs"], 2)
        assert (got["movers"] == movers).all()
        cost = B.nav_plan(lv["state"], lv["dist2"], goals, None, outputs=("cost",), min_dist2=1)["cost"]
        want = B.nav_dyn_steer(lv["state"], lv["dist2"], poses, movers=movers, cost=cost, min_dist2=1, **steer_kw)
        for nm in binding.NAVSTEER_POSE_OUTPUTS + ("best_min_gap",):
            if nm == "best_traj":
                assert all((x == y).all() for x, y in zip(got["steer"][nm], want[nm]))
            else:
                assert (got["steer"][nm] == want[nm]).all(), (step, nm)
        assert got["steer"]["stats"] == want["stats"]
    assert mb.marks.any() or mb.seen_tick.any()
    B.close()
    A.close()


# ---- replay.py's files -----------------------------------------------------------------------------------------------------
def test_replay_writes_the_layer_next_to_the_grid(mem_lib, tmp_path, capsys):
    import os
    import re
    from supersurfel_fusion_amd import replay
    f = handle(mem_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    replay.replay(f, frames, nav_grid_dir=str(tmp_path), nav_grid_every=2, nav_grid_res=0.1, nav_live=dict(min_hits=2, stride=8, memory=dict(forget=5, slices=8)))
    per_grid = [".pgm", ".yaml", "_dist2.npy", "_live_dist2.npy", "_live_state.npy", "_live_marks.npy", "_live_mark_tick.npy", "_live_seen_tick.npy"]
    assert sorted(os.listdir(str(tmp_path))) == sorted("%06d%s" % (k, s) for k in (0, 2) for s in per_grid)
    logged = [l for l in capsys.readouterr().out.splitlines() if l.startswith("nav-memory ")]
    assert len(logged) == 2 and "tick=1 fresh=1 " in logged[0] and "tick=3 " in logged[1]
    fresh = int(re.search(r"fresh=(\d)", logged[1]).group(1))
    load = lambda k, nm: np.load(str(tmp_path / ("%06d_live_%s.npy" % (k, nm))))
    grid = f.nav_grid(outputs=("state", "dist2"), res=0.1)
    mem = binding.LiveMemory(grid["state"].shape[1], grid["state"].shape[0])
    if not fresh:                                                        # the grid's frame stayed: the layer of frame 0 went in
        for a, nm in zip(mem.arrays(), mr.LAYER):
            a[...] = load(0, nm)
    lv = f.nav_memory(frames[2][2], grid["state"], memory=mem, tick=3, grid_pose=grid["stats"]["pose"], res=0.1, min_hits=2, stride=8, slices=8,
                      max_mark_age=5, max_seen_age=5)
    for nm in mr.LAYER + ("state", "dist2"):
        assert (load(2, nm) == lv[nm]).all(), nm
    assert lv["stats"]["points_in_band"] > 0 and "cells_marked=%d " % lv["stats"]["cells_marked"] in logged[1]
    assert (load(0, "mark_tick").max(), load(2, "mark_tick").max()) == (1, 3)
    f.close()


# ---- the C++ surface -----------------------------------------------------------------------------------------------------
def test_the_memory_in_cpp(mem_lib, fusion, fusion_u16, tmp_path):
    """tests/cpp/navmem_smoke.cpp on the GPU: its counts and FNV-1a checksums equal those of the Python calls on the same arrays"""
    import os
    import re
    import subprocess
    from conftest import ROOT
    cpp = os.path.join(ROOT, "tests", "cpp")
    libdir = os.path.dirname(mem_lib.path)
    exe = str(tmp_path / "navmem_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", cpp, os.path.join(cpp, "navmem_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip_mem", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "grid ok=1" in r.stdout, r.stdout
    names = ("tick", "valid", "points", "samples", "marked", "cleared", "expired", "remembered", "opened")
    sums = ("state", "dist2", "hits", "marks", "mark_tick", "seen_tick", "seen_bits")
    line = lambda tag: re.search(tag + " " + " ".join(nm + r"=(\d+)" for nm in names) + " " + " ".join(nm + "=([0-9a-f]{16})" for nm in sums), r.stdout)
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
    mem, five = binding.LiveMemory(48, 40), binding.LiveMemory(48, 40)
    calls = (("navmem", fusion, depth, mem, 1, {}), ("masked", fusion, depth, mem, 4, dict(mask=mask, mask_mode=2, min_hits=30, max_mark_age=2, max_seen_age=2)),
             ("u16", fusion_u16, counts, five, 7, dict(slices=5)))
    for tag, f, image, memory, tick, extra in calls:
        got, told = f.nav_memory(image, state_in, memory=memory, tick=tick, **dict(kw, **extra)), line(tag)
        assert told, (tag, r.stdout)
        s = got["stats"]
        counts_py = (tick, s["pixels_valid"], s["points_in_band"], s["ray_samples"], s["cells_marked"], s["cells_cleared"], s["cells_expired"],
                     s["cells_remembered"], s["cells_opened"])
        assert tuple(int(v) for v in told.groups()[:9]) == counts_py, (tag, told.groups(), counts_py)
        want = tuple(pr.fnv1a(got[nm].tobytes()) for nm in ("state", "dist2", "live_hits", "marks", "mark_tick", "seen_tick", "seen_bits"))
        assert tuple(int(v, 16) for v in told.groups()[9:]) == want, (tag, told.groups()[9:], want)
        assert s["cells_marked"] > 0 and s["points_in_band"] > 1000
    assert s["cells_marked"] > 0
