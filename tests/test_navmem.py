"""The live layer with memory (include/ssf_navmem.h) without a GPU, on the restatement (tests/navmem_ref.py): the walker whose trail the
fed-back overlay keeps and the memory clears, the low box that only the slices save, decay and the tick's wrap-around, the same-frame and
bucket edges by hand, the boundary cases, the two identities against navlive_ref.overlay, and guards that the scenes of the GPU file
show what they are there to show."""
import numpy as np
import pytest

import navgrid_ref as nr
import navlive_ref as lr
import navmem_ref as mr

u32 = lambda *v: np.array(v, np.uint32)


def rule(hits, hit_bits, seen_bits, state_in=-1, marks=0, mark_tick=0, seen_tick=0, **kw):
    """cells_rule on one cell: (marks, mark_tick, seen_tick, state, stats)"""
    c = dict(dict(mr.MEM_DEFAULTS, min_hits=4, open_unknown=True), **kw)
    got = mr.cells_rule(u32(hits), u32(hit_bits), u32(seen_bits), np.array([state_in], np.int8),
                        dict(marks=u32(marks), mark_tick=u32(mark_tick), seen_tick=u32(seen_tick)), c)
    return int(got["marks"][0]), int(got["mark_tick"][0]), int(got["seen_tick"][0]), int(got["state"][0]), got["stats"]


# ---- the walker ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk():
    """the crossing through the memory (static state_in every frame) and through navlive_ref.overlay fed its own state"""
    c = mr.params(**mr.WALKER_KW)
    static = np.full((c["height"], c["width"]), -1, np.int8)
    layer, fed, frames = None, static, []
    for k in range(mr.WALKER_FRAMES):
        d = mr.walker_depth(k)
        g = mr.update(d, None, static, layer, mr.WALKER_GRID, mr.WALKER_CAM, dict(c, tick=k + 1))
        layer = {nm: g[nm] for nm in mr.LAYER}
        fed = lr.overlay(d, None, fed, mr.WALKER_GRID, mr.WALKER_CAM, lr.params(**mr.WALKER_KW))["state"]
        frames.append(g)
    return dict(c=c, frames=frames, fed=fed)


def test_the_walker_leaves_a_wall_in_the_fed_back_overlay_and_none_in_the_memory(walk):
    c, frames, last = walk["c"], walk["frames"], walk["frames"][-1]
    assert mr.WALKER_FRAMES >= 5 and (c["cam_width"], c["cam_height"], c["width"], c["height"]) == (160, 128, 65, 64)
    hb = [np.where(g["live_hits"] >= c["min_hits"], g["hit_bits"], 0) for g in frames]
    stamped = np.zeros_like(hb[0])
    for b in hb[:-1]:
        stamped |= b
    earlier = (stamped != 0) & (hb[-1] == 0)                             # footprints of the frames before the last, not stamped by it
    assert earlier.sum() >= 20
    assert (walk["fed"][earlier] == 100).all()                           # the one-way state: every earlier footprint is still a wall
    through = earlier & ((stamped & ~last["seen_bits"]) == 0)            # ... whose marked slices the final frame sees through
    assert through.sum() >= 10
    assert not last["marks"][through].any() and (last["state"][through] != 100).all()
    under = hb[-1] != 0                                                  # the walker's final position (and the wall behind the room)
    assert under.sum() >= 4 and (last["marks"][under] != 0).all() and (last["state"][under] == 100).all()
    assert all(g["stats"]["cells_cleared"] > 0 and g["stats"]["bits_cleared"] > g["stats"]["cells_cleared"] for g in frames[1:])
    assert last["stats"]["cells_remembered"] == 0 or (last["marks"][earlier] != 0).any()


# ---- the low box -----------------------------------------------------------------------------------------------------------------
def lowbox(slices):
    c = mr.params(**dict(mr.LOWBOX_KW, slices=slices))
    static = np.full((c["height"], c["width"]), -1, np.int8)
    a = mr.update(mr.lowbox_depth(0), None, static, None, mr.LOWBOX_GRID, mr.LOWBOX_POSES[0], dict(c, tick=1))
    b = mr.update(mr.lowbox_depth(1), None, static, {nm: a[nm] for nm in mr.LAYER}, mr.LOWBOX_GRID, mr.LOWBOX_POSES[1], dict(c, tick=2))
    return c, a, b


def test_the_low_box_survives_rays_that_pass_over_it_only_with_slices():
    c, a, b = lowbox(16)
    box = (a["marks"] != 0) & (np.arange(c["height"])[:, None] < mr.LOWBOX_ROWS)
    assert box.sum() >= 10 and not (b["live_hits"][box] > 0).any()       # stamped at first, out of view when the camera looks up
    crossed = box & (b["seen_bits"] != 0)
    assert crossed.sum() >= 10
    rays = int(np.bitwise_or.reduce(b["seen_bits"][crossed]))
    assert int(a["marks"][box].max()) < (rays & -rays)                   # the lowest slice any ray crosses lies above every mark
    assert (b["marks"][crossed] == a["marks"][crossed]).all() and (b["state"][crossed] == 100).all()
    assert b["stats"]["cells_remembered"] >= crossed.sum() and b["stats"]["cells_cleared"] == 0
    c1, a1, b1 = lowbox(1)
    assert ((a1["marks"] != 0) == (a["marks"] != 0)).all() and ((b1["seen_bits"] != 0) == (b["seen_bits"] != 0)).all()
    assert not b1["marks"][crossed].any() and (b1["state"][crossed] == 0).all() and b1["stats"]["cells_cleared"] >= crossed.sum()


# ---- decay -----------------------------------------------------------------------------------------------------------------------
def test_a_mark_out_of_view_survives_at_its_age_and_expires_one_tick_later():
    m, mt, _, state, s = rule(0, 0, 0, marks=0b101, mark_tick=10, tick=17, max_mark_age=7)
    assert (m, mt, state) == (0b101, 10, 100) and s["cells_expired"] == 0 and s["cells_remembered"] == 1
    m, mt, _, state, s = rule(0, 0, 0, marks=0b101, mark_tick=10, tick=18, max_mark_age=7)
    assert (m, mt, state) == (0, 0, -1) and s["cells_expired"] == 1 and s["cells_cleared"] == 0 and s["cells_marked"] == 0
    assert rule(0, 0, 0, marks=1, mark_tick=10, tick=4000000000, max_mark_age=0)[:2] == (1, 10)          # 0: never
    # a hit in the frame refreshes the tick, however old the cell was
    assert rule(4, 2, 0, marks=1, mark_tick=1, tick=100, max_mark_age=7)[:2] == (3, 100)


def test_seen_tick_decays_the_same_way():
    assert rule(0, 0, 0, seen_tick=10, tick=15, max_seen_age=5)[2:4] == (10, 0)
    assert rule(0, 0, 0, seen_tick=10, tick=16, max_seen_age=5)[2:4] == (0, -1)
    assert rule(0, 0, 0, seen_tick=10, tick=4000000000, max_seen_age=0)[2:4] == (10, 0)
    assert rule(0, 0, 1, seen_tick=1, tick=16, max_seen_age=5)[2:4] == (16, 0)
    assert rule(0, 0, 1, seen_tick=1, tick=16, max_seen_age=5, open_unknown=False)[2:4] == (16, -1)
    assert rule(0, 0, 0, state_in=0, seen_tick=10, tick=16, max_seen_age=5)[2:4] == (0, 0)


def test_the_tick_wraps_around():
    """mark_tick_in = 0xFFFFFFFE and tick = 3: five ticks have passed"""
    assert rule(0, 0, 0, marks=1, mark_tick=0xFFFFFFFE, tick=3, max_mark_age=5)[:2] == (1, 0xFFFFFFFE)
    assert rule(0, 0, 0, marks=1, mark_tick=0xFFFFFFFE, tick=3, max_mark_age=4)[:2] == (0, 0)
    assert rule(0, 0, 0, seen_tick=0xFFFFFFFE, tick=3, max_seen_age=5)[2] == 0xFFFFFFFE
    assert rule(0, 0, 0, seen_tick=0xFFFFFFFE, tick=3, max_seen_age=4)[2] == 0


# ---- same-frame and bucket edges ---------------------------------------------------------------------------------------------------
def test_hit_wins_over_seen_and_min_hits_gates_all_bits():
    m, mt, st, state, s = rule(4, 0b0110, 0b1111, marks=0b1001, mark_tick=3, tick=9)
    assert (m, mt, st, state) == (0b0110, 9, 9, 100) and s["bits_cleared"] == 2 and s["cells_cleared"] == 0 and s["cells_remembered"] == 0
    # three points of four: none of the cell's bits count, and the rays clear it
    m, mt, st, state, s = rule(3, 0b0110, 0b1111, marks=0b1001, mark_tick=3, tick=9)
    assert (m, mt, st, state) == (0, 0, 9, 0) and s["bits_cleared"] == 2 and s["cells_cleared"] == 1 and s["cells_opened"] == 1
    m, mt, st, state, s = rule(3, 0b0110, 0, tick=9)
    assert (m, mt, st, state) == (0, 0, 0, -1) and s["cells_marked"] == 0
    # what the map knows stays: an occupied cell is never opened, a foreign value is unknown
    assert rule(0, 0, 1, state_in=100, tick=2)[3] == 100 and rule(0, 0, 0, state_in=7, tick=2)[3] == -1
    assert rule(4, 1, 0, state_in=0, tick=2)[3] == 100 and rule(4, 1, 0, state_in=0, tick=2)[4]["cells_newly_marked"] == 1


def test_the_slice_of_a_height():
    c = dict(floor_max=-0.8, z_max=0.5, slices=16)
    z = np.array([0.5, np.nextafter(np.float32(-0.8), np.float32(0)), -0.3, 0.0], np.float32)
    assert mr.slice_bits(z, c).tolist() == [1 << 15, 1, 1 << 6, 1 << 9]
    assert mr.slice_bits(z, dict(c, slices=1)).tolist() == [1, 1, 1, 1]
    assert mr.slice_bits(z[:1], dict(c, slices=32)).tolist() == [1 << 31]
    assert mr.slice_bits(np.float32([1.0, 0.25, 2.0 ** -20]), dict(floor_max=0.0, z_max=1.0, slices=4)).tolist() == [8, 2, 1]
    for bad in (dict(floor_max=np.nan), dict(z_max=np.inf), dict(z_max=-0.8), dict(z_max=-0.9), dict(floor_max=-3e38, z_max=3e38),
                dict(floor_max=0.0, z_max=1e-45, slices=32)):
        assert mr.refused_slices(dict(c, **bad)), bad
    assert not mr.refused_slices(c)


def test_the_boundary_cases():
    for name, d, at, kw, want in mr.boundary_cases():
        c = mr.params(**dict(lr.BOUNDARY, **kw))
        got = mr.update(np.full((1, 1), d, np.float32), None, np.full((4, 8), -1, np.int8), None, nr.IDENTITY, lr.boundary_pose(*at), c)
        mr.check_expectations(got, want, 8, 4, name)
        assert (got["marks"] == got["hit_bits"]).all() and ((got["seen_tick"] != 0) == (got["seen_bits"] != 0)).all()
    assert {kw["slices"] for _, _, _, kw, _ in mr.boundary_cases()} == {1, 4, 32}


# ---- the identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,fmt,stride,slices", mr.GPU_CASES[::2], ids=["%s-%s-stride%d-slices%d" % c for c in mr.GPU_CASES[::2]])
def test_a_zero_layer_without_ages_is_the_stateless_overlay(scene, fmt, stride, slices):
    i, ev = mr.case_evidence(scene, fmt, stride)
    want = lr.case_reference(scene, fmt, stride)
    got = mr.update_from(ev, i["state_in"], None, mr.params(slices=slices, **i["kw"]))
    for nm in ("state", "dist2", "live_hits"):
        assert (got[nm] == want[nm]).all(), nm
    assert ((got["seen_bits"] != 0) == (want["live_seen"] >= 1)).all()
    for nm in ("pixels_valid", "pixels_stamping", "points_in_band", "rays", "rays_carving", "ray_samples", "cells_opened", "cells_free", "cells_occupied"):
        assert got["stats"][nm] == want["stats"][nm], nm
    assert got["stats"]["cells_newly_marked"] == got["stats"]["cells_marked"] > 0 and got["stats"]["cells_opened"] > 0


def test_without_a_valid_pixel_the_layer_is_a_fixed_point():
    i, _ = mr.case_evidence("noise", "f32", 4)
    c = mr.params(tick=77, **i["kw"])
    layer = mr.random_layer(c["width"], c["height"], 1, 77, 40, 25)
    layer["seen_tick"][...] = 0
    got = mr.update(np.zeros((128, 160), np.float32), None, i["state_in"], layer, i["grid_pose"], i["cam_pose"], c)
    for nm in mr.LAYER:
        assert (got[nm] == layer[nm]).all(), nm
    static = np.where(i["state_in"] == 100, 100, np.where(i["state_in"] == 0, 0, -1))
    assert (got["state"] == np.where(layer["marks"] != 0, 100, static)).all() and (layer["marks"] != 0).sum() > 100


# ---- the GPU file's scenes are not vacuous --------------------------------------------------------------------------------------
def test_the_random_layers_of_the_gpu_cases_exercise_every_branch():
    seen = dict.fromkeys(("cells_cleared", "cells_expired", "bits_cleared", "cells_remembered", "cells_newly_marked", "cells_opened"), 0)
    for scene, fmt, stride, slices in mr.GPU_CASES:
        i, ev = mr.case_evidence(scene, fmt, stride)
        c = mr.params(slices=slices, tick=mr.GPU_TICK, **dict(i["kw"], **mr.GPU_AGES))
        layer = mr.random_layer(c["width"], c["height"], i["c"]["width"] + stride, mr.GPU_TICK, slices=slices, **mr.GPU_AGES)
        age = (mr.GPU_TICK - layer["mark_tick"].astype(np.int64))[layer["marks"] != 0]
        assert (age > 40).any() and (age <= 40).any() and abs((layer["marks"] != 0).mean() - 0.2) < 0.05
        got = mr.update_from(ev, i["state_in"], layer, c)
        for k in seen:
            seen[k] += got["stats"][k]
        assert got["stats"]["cells_expired"] > 0 and got["stats"]["cells_remembered"] > 0
        assert int(got["hit_bits"].max()) < (1 << slices) and (slices == 1 or len(np.unique(got["seen_bits"])) > 2)
    assert all(v > 0 for v in seen.values()), seen


# ---- the guards of the parameter space, the masks and the round-edge rays of the GPU file ------------------------------------------
@pytest.mark.parametrize("fmt", lr.PARAM_FORMATS)
@pytest.mark.parametrize("row", range(len(mr.PARAM_ROWS)), ids=mr.PARAM_IDS)
def test_every_row_of_the_parameter_space_changes_its_arrays(row, fmt):
    base, got = mr.param_reference(fmt, None), mr.param_reference(fmt, row)
    arrays = mr.PARAM_ROWS[row][2]
    differ = [bool((got[a] != base[a]).any()) for a in arrays]
    print(mr.PARAM_IDS[row], fmt, {a: int((got[a] != base[a]).sum()) for a in arrays})
    if (mr.PARAM_IDS[row], fmt) in mr.PARAM_UNCHANGED:
        assert not any(differ), (mr.PARAM_IDS[row], fmt, "is listed as a row that changes nothing")
    else:
        assert all(differ), (mr.PARAM_IDS[row], fmt, "repeats the base case", arrays, differ)


def test_the_parameter_space_is_the_overlays_without_min_seen():
    over = [r[1] for r in mr.PARAM_ROWS]
    assert over == [{k: v for k, v in r[0].items() if k != "min_seen"} for r in lr.PARAM_ROWS if set(r[0]) != {"min_seen"}]
    assert len(over) == len(lr.PARAM_ROWS) - 2 == len(mr.PARAM_IDS) and dict(min_hits=64, stride=7) in over and not any("min_seen" in o for o in over)
    changed = lambda k, fmt: all((mr.param_reference(fmt, k)[a] != mr.param_reference(fmt, None)[a]).any() for a in mr.PARAM_ROWS[k][2])
    for name, fmt in mr.PARAM_UNCHANGED:                                 # another row of the same parameter changes its array in that format
        o = over[mr.PARAM_IDS.index(name)]
        others = [k for k, x in enumerate(over) if set(x) == set(o) and (mr.PARAM_IDS[k], fmt) not in mr.PARAM_UNCHANGED]
        assert others and all(changed(k, fmt) for k in others), (name, fmt)
    # the base case is random_case()'s kind: five slices, both ages on, a random layer with marks that expire and marks that stay
    i = mr.param_inputs("f32", {})
    assert (i["c"]["slices"], i["c"]["tick"], i["c"]["max_mark_age"], i["c"]["max_seen_age"]) == (5, mr.GPU_TICK, 40, 25)
    base = mr.param_reference("f32", None)["stats"]
    assert base["cells_expired"] > 0 and base["cells_remembered"] > 0 and base["cells_cleared"] > 0 and base["cells_opened"] > 0
    # open_unknown = 0: no cell is opened, in cells whose seen_tick is not 0 -- the branch rule.open_unknown && st != 0
    closed = mr.param_reference("f32", mr.PARAM_IDS.index("open_unknown=0"))
    assert closed["stats"]["cells_opened"] == 0 and ((closed["seen_tick"] != 0) & (closed["state"] == -1)).sum() > 100
    assert closed["stats"]["cells_remembered"] == base["cells_remembered"]
    # margin 0: rays clear bits in the cells their own pixels mark (hit wins over seen: m = (m_in & ~sb) | hb)
    zero = mr.param_reference("f32", mr.PARAM_IDS.index("hit_margin_cells=0.0"))
    hb = np.where(zero["live_hits"] >= 4, zero["hit_bits"], 0)
    assert ((hb & zero["seen_bits"]) != 0).sum() > 0 and ((zero["marks"] & hb) == hb).all()


@pytest.mark.parametrize("fmt", ["f32", "u16"])
def test_the_mask_modes_on_the_large_image(fmt):
    i = mr.masked_inputs(fmt)
    run = lambda mode: mr.update(i["depth"], i["mask"], i["state_in"], i["layer"], i["grid_pose"], i["cam_pose"], dict(i["c"], mask_mode=mode), fmt,
                                 i["depth_scale"])
    got = [run(m) for m in (0, 1, 2)]
    assert (got[0]["live_hits"] == got[1]["live_hits"] + got[2]["live_hits"]).all() and (got[0]["hit_bits"] == got[1]["hit_bits"] | got[2]["hit_bits"]).all()
    assert got[1]["stats"]["pixels_stamping"] + got[2]["stats"]["pixels_stamping"] == got[0]["stats"]["pixels_valid"]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert (got[a]["live_hits"] != got[b]["live_hits"]).any() and (got[a]["seen_bits"] == got[b]["seen_bits"]).all()
        assert (got[a]["seen_tick"] == got[b]["seen_tick"]).all()
    assert (got[1]["marks"] != got[2]["marks"]).any() and (got[1]["hit_bits"] != got[2]["hit_bits"]).any()
    assert all(0 < g["stats"]["pixels_stamping"] < got[0]["stats"]["pixels_valid"] and g["stats"]["cells_newly_marked"] > 0 for g in got[1:])


@pytest.mark.parametrize("fmt", ["f32", "u16"])
def test_the_mask_of_the_small_image_splits_its_pixels(fmt):
    i = mr.small_inputs(fmt)
    assert (i["depth"].shape, i["mask"].shape, i["state_in"].shape) == ((29, 37), (29, 37), (33, 31))
    run = lambda mode: mr.update(i["depth"], i["mask"], i["state_in"], i["layer"], i["grid_pose"], i["cam_pose"],
                                 mr.params(**dict(i["kw"], mask_mode=mode)), fmt, i["depth_scale"])
    only, rest = run(1), run(2)
    for got in (only, rest):
        s = got["stats"]
        print(fmt, s)
        assert 0 < s["pixels_stamping"] < s["pixels_valid"] and s["cells_newly_marked"] > 0 and s["rays"] > 64
    assert (only["stats"]["pixels_stamping"], rest["stats"]["pixels_stamping"], rest["stats"]["pixels_valid"]) == ((413, 421, 834) if fmt == "f32" else (414, 421, 835))
    assert (only["marks"] != rest["marks"]).any() and (only["seen_bits"] == rest["seen_bits"]).all()


@pytest.mark.parametrize("tilt", lr.EDGE_TILTS)
def test_the_round_edge_rays_end_on_both_sides_of_a_round(tilt):
    i = mr.edge_inputs(tilt)
    c = mr.params(**i["kw"])
    run = lambda d, i: mr.update(d, None, i["state_in"], None, i["grid_pose"], i["cam_pose"], c)
    got = run(i["depth"], i)
    s = got["stats"]
    assert (s["pixels_valid"], s["rays"], s["rays_carving"], s["ray_samples"], c["slices"]) == (126, 126, 126, 12167, 32)
    n = lr.edge_ray_counts(tilt, lambda d, i: run(d, i)["stats"])
    assert n.sum() == s["ray_samples"] and [(v, u) for v, u in np.argwhere(n == 0)] == list(lr.EDGE_INVALID)
    assert set(n[0]) - {0} == set(range(49, 81)) and set(n[1]) - {0} == set(range(113, 145))
    for count in lr.EDGE_COUNTS:
        assert (n == count).any(), count
    # a tilted ray climbs or falls through the slices: a cell that continues over a round's end brings a new bit in most cells; the
    # level camera's rays stay in one slice (and the two image rows in two), so a continued cell brings none
    words = len(np.unique(got["seen_bits"]))
    print(tilt, words)
    assert (17 <= words <= 18) if tilt else words == 3
    assert s["cells_marked"] > 30 and s["cells_opened"] > 100


def test_a_camera_that_sees_nothing_only_ages_the_layer():
    """the GPU file's camera outside the grid and its poses that are not finite, on the restatement: no hit, no seen bit, and a layer with
    marks on both sides of the age"""
    i, _ = mr.case_evidence("room straight", "f32", 4)
    c = mr.params(**dict(i["kw"], slices=5, tick=mr.GPU_TICK, **mr.GPU_AGES))
    layer = mr.random_layer(c["width"], c["height"], 3, mr.GPU_TICK, slices=5, **mr.GPU_AGES)
    zero = np.zeros((c["height"], c["width"]), np.uint32)
    aged = mr.cells_rule(zero, zero, zero, i["state_in"], layer, c)
    assert aged["stats"]["cells_expired"] > 0 and aged["stats"]["cells_marked"] > 0 and (aged["seen_tick"] != layer["seen_tick"]).any()
    poses = [lr.room_pose(at=(40.0, 0.0, -30.0))]
    for k, bad in ((0, np.nan), (4, np.inf), (9, np.nan), (11, -np.inf)):
        poses.append(i["cam_pose"].copy())
        poses[-1][k] = bad
    for pose in poses:
        got = mr.update(i["depth"], None, i["state_in"], layer, i["grid_pose"], pose, c)
        assert not got["live_hits"].any() and not got["hit_bits"].any() and not got["seen_bits"].any()
        assert all((got[nm] == aged[nm]).all() for nm in mr.LAYER + ("state",)) and all(got["stats"][k] == n for k, n in aged["stats"].items())
    assert got["stats"]["rays"] > 0 and mr.update(i["depth"], None, i["state_in"], layer, i["grid_pose"], poses[0], c)["stats"]["ray_samples"] > 0


@pytest.mark.parametrize("tilt", lr.EDGE_TILTS)
def test_the_shifted_round_edge_rays_end_a_round_inside_a_wave(tilt):
    i = mr.edge_inputs(tilt, 8)
    c = mr.params(**i["kw"])
    run = lambda d, i: mr.update(d, None, i["state_in"], None, i["grid_pose"], i["cam_pose"], c)
    got = run(i["depth"], i)
    n = lr.edge_ray_counts(tilt, lambda d, i: run(d, i)["stats"], 8)
    assert (got["stats"]["rays_carving"], got["stats"]["ray_samples"], c["slices"]) == (126, n.sum(), 32)
    waves = [set(n.ravel()[k:k + 16]) for k in range(0, 128, 16)]
    assert {64, 65} <= waves[1] and {128, 129} <= waves[5]
    words = len(np.unique(got["seen_bits"]))
    assert words > 12 if tilt else words == 3
