"""An oriented footprint on the navigation grid (include/ssf_navfoot.h) on the GPU: every array and every stat of ssf_navfoot_layers and
ssf_navfoot_rollouts equals the numpy restatement (tests/navfoot_ref.py) with ==, at the smallest grids at which the kernels can go
wrong (one cell, one row, sizes that are no multiple of the 32-cell tile, obstacles at a tile's corner, the largest reach), through
device pointers fed by the overlay and the plan, through nav_live_foot_steer, and with the disc's call beside it."""
import numpy as np
import pytest

import navdyn_ref as dr
import navfoot_ref as fr
import navlive_ref as lr
import navplan_ref as pr
import navsteer_ref as sr
import util
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
W, H = 160, 128
SMALL = (1536, 512, 512, 512, 0)                                         # a body of 3 x 2 cells: survives on a cluttered grid
QUARTER_FOOT = (6144, 1024, 2048, 3072, 0)                               # 8 x 6 cells: turns in the open, not beside a wall


def handle(lib, **kw):
    """a handle of a test's own, which the test closes when it is done with it"""
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


@pytest.fixture(scope="module")
def foot_lib():
    """libssf_hip_foot.so: steer's objects plus the footprint's entry points (no fallback: a missing .so is an error)"""
    return binding.load_foot()


@pytest.fixture(scope="module")
def fusion(foot_lib):
    f = handle(foot_lib)
    yield f
    f.close()


def foot_kw(foot, B, allow=0):
    return dict(zip(("front", "back", "left", "right", "pad"), foot), n_headings=B, allow_unknown=allow)


def call_kw(c):
    return {k: v for k, v in c.items() if k not in ("width", "height", "n_poses")}


# ---- the layers --------------------------------------------------------------------------------------------------------------------
def grid(h, w, obstacles):
    state = np.zeros((h, w), np.int8)
    if obstacles == "one":
        state[h // 2, w // 2] = 100
    elif obstacles == "tile start":                                       # the first cell of a tile, two tiles in
        state[64, 64] = 100
    elif obstacles == "tile corner":
        state[31, 31] = state[32, 32] = 100
    elif obstacles == "random":
        rng = np.random.default_rng(h * 1000 + w)
        state[rng.random((h, w)) < 0.02] = 100
        state[rng.random((h, w)) < 0.01] = -1
    elif obstacles == "foreign":
        state = pr.foreign_grid(h, w, 7000 + 10 * h + w)[0]
    else:
        assert obstacles == "none"
    return state


# (name, h, w, footprint, B, obstacles, allow_unknown)
LAYER_CASES = (
    ("1x1 point", 1, 1, fr.POINT, 1, "none", 0),
    ("1x1 asym", 1, 1, fr.ASYM, 4, "none", 0),
    ("1x70 line", 1, 70, fr.LINE, 32, "none", 0),
    ("1x70 point random", 1, 70, fr.POINT, 32, "random", 1),
    ("37x53 asym one", 37, 53, fr.ASYM, 32, "one", 0),
    ("37x53 line random", 37, 53, fr.LINE, 4, "random", 0),
    ("37x53 point one", 37, 53, fr.POINT, 2, "one", 0),
    ("64x64 asym tile corner", 64, 64, fr.ASYM, 8, "tile corner", 0),
    ("64x64 line tile corner", 64, 64, fr.LINE, 32, "tile corner", 0),
    ("64x64 line none", 64, 64, fr.LINE, 16, "none", 0),
    ("97x33 asym random", 97, 33, fr.ASYM, 32, "random", 1),
    ("97x33 small random", 97, 33, SMALL, 16, "random", 0),
    ("97x33 corner1 none", 97, 33, fr.CORNERS[1], 2, "none", 0),
    ("20x20 largest reach", 20, 20, fr.CORNERS[0], 32, "none", 0),
    ("130x130 largest reach tile start", 130, 130, fr.CORNERS[0], 8, "tile start", 0),
    ("130x130 corner2 tile start", 130, 130, fr.CORNERS[2], 4, "tile start", 0),
    ("130x130 corner3 tile start", 130, 130, fr.CORNERS[3], 4, "tile start", 0),
    ("45x70 foreign", 45, 70, SMALL, 16, "foreign", 0),
    ("45x70 foreign unknown", 45, 70, SMALL, 16, "foreign", 1),
    ("64x65 foreign point", 64, 65, fr.POINT, 32, "foreign", 1),
)


def layer_case(name):
    _, h, w, foot, B, obstacles, allow = [c for c in LAYER_CASES if c[0] == name][0]
    state = grid(h, w, obstacles)
    return state, foot, B, allow, fr.cached(("layers", name), lambda: fr.layers(state, allow, foot, B))


@pytest.mark.parametrize("name", [c[0] for c in LAYER_CASES])
def test_the_layers(name, fusion):
    state, foot, B, allow, want = layer_case(name)
    got = fusion.nav_foot(state, outputs=("free_mask", "n_free"), **foot_kw(foot, B, allow))
    for nm in ("free_mask", "n_free"):
        assert got[nm].dtype == want[nm].dtype and got[nm].shape == want[nm].shape
        diff = got[nm] != want[nm]
        assert not diff.any(), (name, nm, int(diff.sum()), np.argwhere(diff)[:5].tolist(), got[nm][diff][:5].tolist(), want[nm][diff][:5].tolist())
    assert got["stats"] == want["stats"], (name, got["stats"], want["stats"])
    assert B == 32 or (got["free_mask"] >> np.uint32(B) == 0).all()                       # bits >= B are 0
    s = got["stats"]
    if name == "20x20 largest reach":
        assert s["reach"] == 39 and s["cells_none"] == 400 and s["cells_clear"] == 400          # sqrt(2) * 28 = 39.6: the bound of the ranges
    if name == "130x130 largest reach tile start":
        assert s["reach"] == 39 and s["cells_some"] > 0 and s["cells_all"] == 0          # no cell holds the square and its diagonal
    if "foreign" in name or "random" in name or "tile corner" in name or "tile start" in name or name.endswith("one"):
        assert s["cells_some"] > 0 or foot == fr.POINT, s
    if foot == fr.POINT:
        assert (got["free_mask"] == np.where(fr.clear_cells(state, allow), np.uint32((1 << B) - 1), 0)).all()


def test_one_output_alone_guard_bytes_and_two_calls_giving_the_same_bytes(fusion):
    """device buffers inside sentinels: an output that is not asked for is not written, nothing lands outside the one that is, and a
    second call writes the same bytes"""
    import torch
    dev = torch.device("cuda")
    state, foot, B, allow, want = layer_case("37x53 asym one")
    h, w = state.shape
    P, G, SENT = h * w, 256, 0x5A
    d_state = torch.from_numpy(state).to(dev)
    assert P % 4 == 1                                                     # (an odd count: the guards do not start word-aligned)
    for asked in (("free_mask",), ("n_free",), ("free_mask", "n_free")):
        buf = torch.full((2 * G + 4 * P + G + P + 3,), SENT, dtype=torch.uint8, device=dev)
        off_mask, off_n = G, G + 4 * P + G
        stats = fusion.nav_foot_device(d_state, w, h, free_mask=buf.data_ptr() + off_mask if "free_mask" in asked else None,
                                       n_free=buf.data_ptr() + off_n if "n_free" in asked else None, **foot_kw(foot, B, allow))
        raw = buf.cpu().numpy()
        keep = np.ones(len(raw), bool)
        if "free_mask" in asked:
            assert (raw[off_mask:off_mask + 4 * P].view(np.uint32).reshape(h, w) == want["free_mask"]).all()
            keep[off_mask:off_mask + 4 * P] = False
        if "n_free" in asked:
            assert (raw[off_n:off_n + P].reshape(h, w) == want["n_free"]).all()
            keep[off_n:off_n + P] = False
        assert (raw[keep] == SENT).all(), asked
        assert stats == want["stats"]
    again = fusion.nav_foot(state, outputs=("free_mask", "n_free"), **foot_kw(foot, B, allow))
    assert again["free_mask"].tobytes() == want["free_mask"].tobytes() and again["n_free"].tobytes() == want["n_free"].tobytes()


# ---- the rollouts ------------------------------------------------------------------------------------------------------------------
def same(got, want, what, outputs=sr.OUTPUTS):
    n = len(want["best"])
    for name in outputs:
        if name == "best_traj":                                          # a list, cut at best_len
            assert len(got[name]) == n, (what, name)
            for q in range(n):
                w = want[name][q, :want["best_len"][q]]
                assert got[name][q].shape == w.shape and got[name][q].dtype == w.dtype and (got[name][q] == w).all(), (what, name, q)
            continue
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name, got[name].shape, got[name].dtype)
        diff = got[name] != want[name]
        assert not diff.any(), (what, name, int(diff.sum()), np.argwhere(diff)[:5].tolist(), got[name][diff][:5].tolist(), want[name][diff][:5].tolist())
    for k in sr.STATS + sr.INFORMATIVE:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"], want["stats"])


def foot_check(f, what, mask, B, i, c, want=None):
    cost = i["cost"] if c["cost_weight"] else None
    targets = i["targets"] if c["target_weight"] else None
    if want is None:
        want = fr.rollouts(mask, B, i["dist2"], cost, i["poses"], targets, c)
    got = f.nav_foot_steer(mask, i["dist2"], i["poses"], B, cost=cost, targets=targets, outputs=sr.OUTPUTS, **call_kw(c))
    same(got, want, what)
    return got, want


def test_the_corridor(fusion):
    """the demonstration: an 11 x 5-cell robot in a 7-cell corridor drives along it and cannot turn on the spot; the disc of the
    circumscribed radius does not fit"""
    i = fr.corridor_scene()
    c, B = i["c"], i["B"]
    lay = fusion.nav_foot(i["state"], **foot_kw(i["foot"], B))
    want_lay = fr.cached("corridor layers", lambda: fr.layers(i["state"], 0, i["foot"], B))
    assert (lay["free_mask"] == want_lay["free_mask"]).all() and lay["stats"] == want_lay["stats"]
    want = fr.cached("corridor rollouts", lambda: fr.rollouts(want_lay["free_mask"], B, i["dist2"], i["cost"], i["poses"], None, c))
    got, _ = foot_check(fusion, "corridor", lay["free_mask"], B, i, c, want=want)
    v, w, _ = sr.lattice(c)
    assert (got["pose_status"] == 0).all() and (got["best_cmd"][:, 0] == v.max()).all() and (got["best_cmd"][:, 1] == 0).all()
    assert all((t[:, 1] >> 10 == 18).all() and t[-1, 0] - t[0, 0] == 16 * 512 for t in got["best_traj"])
    spin = (v == 0) & (w != 0)
    assert set(np.unique(got["cand_free"][:, spin]).tolist()) == {0, 1}
    disc = fusion.nav_steer(i["state"], i["dist2"], i["poses"], cost=i["cost"], **dict(call_kw(c), min_dist2=37))
    assert set(disc["pose_status"].tolist()) <= {2, 3} and (disc["best"] == -1).all()
    # a start across the corridor, where the body does not fit (along it, it does: bins 0 and 16)
    across = np.array([sr.centre(40, 18, 16384)], np.int32)
    m = int(lay["free_mask"][18, 40])
    assert m == (1 | 1 << 16) and not m >> fr.bin_of(16384, B) & 1
    got = fusion.nav_foot_steer(lay["free_mask"], i["dist2"], across, B, cost=i["cost"], **call_kw(c))
    assert got["pose_status"].tolist() == [2] and got["stats"]["poses_blocked"] == 1 and got["stats"]["windows_global"] == 0


def test_a_start_cell_whose_mask_lacks_only_the_start_bin(fusion):
    """an open floor with one obstacle four cells ahead of a thin body (4 cells forward, half a cell to each side): the cell's mask lacks
    bin 0 of 32 and nothing else, so status 2 is the answer at the headings of bin 0 only, and not at those of bins 1 and 31"""
    B, foot = 32, (4096, 0, 512, 512, 0)
    state = np.zeros((24, 24), np.int8)
    state[12, 16] = 100
    lay = fusion.nav_foot(state, **foot_kw(foot, B))
    assert int(lay["free_mask"][12, 12]) == 0xFFFFFFFE
    c = sr.params(width=24, height=24, n_poses=7, n_steps=6)
    dist2 = sr.clearance(state)
    cost = sr.field(state, dist2, (3, 3), c)
    # bin 0 holds the headings -1024 .. 1023; 1024 is the first of bin 1 and 65536 - 1025 the last of bin 31
    headings = (0, 1023, 65536 - 1024, 1024, 2048, 65536 - 1025, 65536 - 2048)
    assert [fr.bin_of(h, B) for h in headings] == [0, 0, 0, 1, 1, 31, 31]
    poses = np.array([sr.centre(12, 12, h) for h in headings], np.int32)
    i = dict(dist2=dist2, cost=cost, poses=poses, targets=None)
    got, want = foot_check(fusion, "the start bin alone", lay["free_mask"], B, i, c)
    assert got["pose_status"][:3].tolist() == [2, 2, 2] and (got["pose_status"][3:] != 2).all() and (got["best"][:3] == -1).all()
    assert got["stats"]["poses_blocked"] == 3 and got["stats"]["poses_ok"] >= 1


@pytest.mark.parametrize("scene", ["room 65x64 reverse", "room K257 T256"])
def test_the_point_footprint_with_one_bin_gives_the_discs_bytes(scene, fusion):
    """ssf_navsteer_rollouts and ssf_navfoot_rollouts over the point's mask through the same handle: byte for byte the same outputs"""
    i = sr.scene(scene)
    c = i["c"]
    mask = fusion.nav_foot(i["state"], **foot_kw(fr.POINT, 1, c["allow_unknown"]))["free_mask"]
    cost = i["cost"] if c["cost_weight"] else None
    targets = i["targets"] if c["target_weight"] else None
    a = fusion.nav_steer(i["state"], i["dist2"], i["poses"], cost=cost, targets=targets, outputs=sr.OUTPUTS, **call_kw(c))
    b = fusion.nav_foot_steer(mask, i["dist2"], i["poses"], 1, cost=cost, targets=targets, outputs=sr.OUTPUTS, **call_kw(c))
    for nm in sr.OUTPUTS:
        if nm == "best_traj":
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[nm], b[nm])), nm
        else:
            assert a[nm].tobytes() == b[nm].tobytes(), nm
    assert {k: a["stats"][k] for k in sr.STATS} == {k: b["stats"][k] for k in sr.STATS}
    want = sr.case_reference(scene)
    for nm in sr.OUTPUTS:
        if nm != "best_traj":
            assert (b[nm] == want[nm]).all(), nm
    assert b["stats"]["windows_staged"] == 0 and b["stats"]["windows_global"] == a["stats"]["windows_staged"] + a["stats"]["windows_global"]


def room_scene(B, foot, n_poses, seed, **kw):
    """navsteer_ref's room with the footprint's layers (restated) over it"""
    Wd, Hd = 65, 64
    state = sr.room(Wd, Hd, seed)
    c = sr.params(width=Wd, height=Hd, n_poses=n_poses, **kw)
    dist2 = sr.clearance(state)
    cost = sr.field(state, dist2, (Wd - 10, Hd // 2), c)
    S = sr.SUB
    poses = [sr.centre(48, 20, 0), sr.centre(48, 20, 1), sr.centre(48, 20, 65535), sr.centre(5, 30, 0),            # the open floor; beside the wall
             (-5, 700, 0), (Wd * S, 100, 9), (40 * S, 50 * S + 1023, 32768), (40 * S + 1023, 50 * S, 49152 + 65536), sr.centre(3, 3, 1234),
             sr.centre(Wd // 3 + 1, Hd // 3 + 1, 0)]
    rng = np.random.default_rng(300 + seed)
    while len(poses) < n_poses:
        poses.append((int(rng.integers(0, Wd * S)), int(rng.integers(0, Hd * S)), int(rng.integers(-sr.TURN, 2 * sr.TURN))))
    poses = np.array(poses[:n_poses], np.int32)
    targets = np.stack([rng.integers(0, Wd * S, n_poses), rng.integers(0, Hd * S, n_poses)], axis=1).astype(np.int32)
    lay = fr.layers(state, c["allow_unknown"], foot, B)
    return dict(state=state, dist2=dist2, cost=cost, poses=poses, targets=targets, c=c, mask=lay["free_mask"])


def test_quarter_turn_sweeps(fusion):
    """w = +-16384 from headings 0, 1 and 65535 (and others): every step asks for nine or ten bins of 32, wrapping below bin 0"""
    for B in (32, 4):
        i = fr.cached(("quarter", B), lambda: room_scene(B, QUARTER_FOOT, 12, 31, n_v=3, n_w=3, v_min=0, v_step=256, w_min=-16384,
                                                          w_step=16384, n_steps=6, min_free_steps=1, turn_weight=1))
        got, want = foot_check(fusion, "quarter turns B=%d" % B, i["mask"], B, i, i["c"])
        spin = got["cand_free"][:3, 0]                                    # v = 0, w = -16384 on the open floor
        assert (got["pose_status"][:3] == 0).all() and want["stats"]["collided"] > 0 and want["stats"]["admissible"] > 0
        assert (spin == 6).all() and (got["cand_free"][3, (0, 2, 6, 8)] < 6).all()      # the body turns in the open, and not beside the wall


def test_two_chunks_and_one_lane_and_300_poses(fusion):
    """K = 257: two chunks and one lane; 300 poses: two workgroups of the pick; poses outside the grid and on cell boundaries among them"""
    i = fr.cached("K257", lambda: room_scene(16, SMALL, 300, 32, n_v=1, n_w=257, v_min=700, v_step=0, w_min=-2048, w_step=16, n_steps=8,
                                             target_weight=2, turn_weight=1))
    got, want = foot_check(fusion, "K257 x 300", i["mask"], 16, i, i["c"])
    s = got["stats"]
    assert s["candidates"] == 300 * 257 and s["poses_ok"] > 100 and s["poses_blocked"] > 10 and s["collided"] > 0 and (got["best"] > 0).any()
    assert s["windows_global"] == 2 * (s["poses_ok"] + s["poses_stuck"])
    assert got["pose_status"][4] == 1 and got["pose_status"][5] == 1 and got["pose_status"][6] == 0 and got["pose_status"][7] == 0


# ---- the staging of host arrays ----------------------------------------------------------------------------------------------------
FILL = util.GUARD_WORD


def layers_host(f, s, names):
    """ssf_navfoot_layers on staging_scene's floor with host arrays, the outputs `names` alone between guard bytes: (name -> array, stats)"""
    h, w = s["state"].shape
    out = {nm: util.guarded((h, w), np.uint32 if nm == "free_mask" else np.uint8) for nm in names}
    ptr = lambda nm: binding._ptr(out[nm][0]) if nm in out else None
    stats = f._navfoot_layers(f._navfoot_params(False, w, h, foot_kw(s["foot"], s["B"])), binding._ptr(s["state"]), ptr("free_mask"), ptr("n_free"))
    assert all(intact() for _, intact in out.values()), names
    return {nm: a for nm, (a, _) in out.items()}, stats


@pytest.mark.parametrize("w,h", [(37, 19), (1, 1)])
def test_host_arrays_whose_items_all_start_at_rounded_offsets(w, h, fusion):
    """703 cells and one cell: neither P nor 4 P is a multiple of 256, so every array behind the first sits at a rounded offset of the
    staging buffer.  Host arrays, device pointers and the restatement agree, for the layers and for the rollouts over them"""
    import torch
    s = dr.staging_scene(w, h, 5)
    want = s["layers"]
    got, stats = layers_host(fusion, s, ("free_mask", "n_free"))
    d_mask, d_n = torch.zeros((h, w), dtype=torch.int32, device="cuda"), torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    dev_stats = fusion.nav_foot_device(torch.from_numpy(s["state"]).to("cuda"), w, h, free_mask=d_mask, n_free=d_n, **foot_kw(s["foot"], s["B"]))
    for nm, d in (("free_mask", d_mask.cpu().numpy().view(np.uint32)), ("n_free", d_n.cpu().numpy())):
        assert got[nm].dtype == want[nm].dtype and (got[nm] == want[nm]).all() and (d == want[nm]).all(), (w, h, nm)
    assert stats == dev_stats == want["stats"] and (w == 1 or want["stats"]["cells_some"] > 0)
    want = dr.staging_reference(w, h, 5, "foot")
    host, hs = util.rollouts_host(fusion, "foot", s, sr.OUTPUTS)
    dev, ds = util.rollouts_device(fusion, "foot", s, sr.OUTPUTS)
    util.rollouts_same(host, want, "host %d x %d" % (w, h), FILL)
    util.rollouts_same(dev, want, "device %d x %d" % (w, h), FILL)
    assert all(host[nm].tobytes() == dev[nm].tobytes() for nm in sr.OUTPUTS)
    assert {k: hs[k] for k in sr.STATS} == {k: ds[k] for k in sr.STATS} == {k: want["stats"][k] for k in sr.STATS}
    assert w == 1 or ((want["pose_status"] == 0).sum() >= 3 and want["stats"]["collided"] > 0 and (want["pose_status"] == 1).any())


@pytest.mark.parametrize("name", ("free_mask", "n_free") + sr.OUTPUTS)
def test_one_host_output_alone_between_guard_bytes(name, fusion):
    """37 x 19, host arrays: every output of the layers and of the rollouts on its own, all others NULL, equals the same array of the
    call that asks for all of them, and the 256 bytes on either side of the caller's array are untouched"""
    s = dr.staging_scene(37, 19, 5)
    if name in ("free_mask", "n_free"):
        alone, st = layers_host(fusion, s, (name,))
        assert (alone[name] == s["layers"][name]).all() and st == s["layers"]["stats"]
        return
    every, stats = dr.cached(("staging host", "foot"), lambda: util.rollouts_host(fusion, "foot", s, sr.OUTPUTS))
    util.rollouts_same(every, dr.staging_reference(37, 19, 5, "foot"), "every output", FILL)
    alone, st = util.rollouts_host(fusion, "foot", s, (name,))
    assert alone[name].tobytes() == every[name].tobytes() and {k: st[k] for k in sr.STATS} == {k: stats[k] for k in sr.STATS}, name


def test_the_staging_buffers_grow_and_are_used_again(foot_lib):
    """one handle: 8 x 8 with one pose, 37 x 19 with five, 8 x 8 with one again, the layers and the rollouts.  Each call gives what a
    handle that has made no other call gives"""
    f = handle(foot_lib)
    for w, h, n in ((8, 8, 1), (37, 19, 5), (8, 8, 1)):
        s = dr.staging_scene(w, h, n)
        fresh = handle(foot_lib)
        (lay, ls), (want, ws) = layers_host(f, s, ("free_mask", "n_free")), layers_host(fresh, s, ("free_mask", "n_free"))
        assert all(lay[nm].tobytes() == want[nm].tobytes() == s["layers"][nm].tobytes() for nm in lay) and ls == ws == s["layers"]["stats"], (w, h, n)
        (got, gs), (want, ws) = util.rollouts_host(f, "foot", s, sr.OUTPUTS), util.rollouts_host(fresh, "foot", s, sr.OUTPUTS)
        fresh.close()
        assert all(got[nm].tobytes() == want[nm].tobytes() for nm in sr.OUTPUTS) and {k: gs[k] for k in sr.STATS} == {k: ws[k] for k in sr.STATS}, (w, h, n)
        util.rollouts_same(got, dr.staging_reference(w, h, n, "foot"), (w, h, n), FILL)
    f.close()


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
def overlay_scene():
    """a depth frame over a free floor (tests/navlive_ref.py's room): what the overlay, the plan and the layers make of it is steered on"""
    kw = dict(lr.CAMERA, width=33, height=31, res=0.05, max_dist_cells=6, stride=4)
    cam_pose, grid_pose = lr.room_pose(at=(0.8, 0.0, 0.2)), lr.grid_pose_at()
    depth = lr.room_depth(cam_pose)
    state_in = np.zeros((31, 33), np.int8)
    state_in[:, :2] = -1
    S = sr.SUB
    poses = np.array([sr.centre(16, 4, 16384), sr.centre(2, 2, 0), (40 * S, S, 0), sr.centre(16, 4, 0), sr.centre(20, 8, 20000), sr.centre(10, 27, 50000)], np.int32)
    foot = dict(front=1536, back=512, left=512, right=512, n_headings=16, pad=0)
    return dict(kw=kw, cam_pose=cam_pose, grid_pose=grid_pose, depth=depth, state_in=state_in, goals=[(16, 29)], plan=dict(min_dist2=1), poses=poses,
                steer=dict(n_steps=20, clearance_cap=36, brake_div=64), foot=foot)


def live_kw(o):
    return dict({k: v for k, v in o["kw"].items() if k not in ("width", "height")}, grid_pose=o["grid_pose"], cam_pose=o["cam_pose"])


def chained_restatements(o):
    def make():
        lv = lr.overlay(o["depth"], None, o["state_in"], o["grid_pose"], o["cam_pose"], lr.params(**o["kw"]))
        pl = pr.plan(lv["state"], lv["dist2"], o["goals"], None, **o["plan"])
        ft = o["foot"]
        lay = fr.layers(lv["state"], 0, (ft["front"], ft["back"], ft["left"], ft["right"], ft["pad"]), ft["n_headings"])
        c = sr.params(width=33, height=31, n_poses=len(o["poses"]), min_dist2=o["plan"]["min_dist2"], **o["steer"])
        return lv, pl, lay, fr.rollouts(lay["free_mask"], ft["n_headings"], lv["dist2"], pl["cost"], o["poses"], None, c), c
    return fr.cached("chain", make)


def test_device_pointers_fed_from_the_overlay_the_plan_and_the_layers(fusion):
    import torch
    dev = torch.device("cuda")
    o = overlay_scene()
    lv, pl, lay, want, c = chained_restatements(o)
    gw, gh, n, K, T = 33, 31, len(o["poses"]), c["n_v"] * c["n_w"], c["n_steps"]
    d_depth, d_state = torch.from_numpy(o["depth"]).to(dev), torch.from_numpy(o["state_in"]).to(dev)
    d_dist2, d_cost, d_mask = (torch.empty((gh, gw), dtype=torch.int32, device=dev) for _ in range(3))
    fusion.nav_live_device(d_depth, d_state, gw, gh, state_out=d_state, dist2=d_dist2, **live_kw(o))
    fusion.nav_plan_device(d_state, d_dist2, gw, gh, o["goals"], None, cost=d_cost, **o["plan"])
    foot_stats = fusion.nav_foot_device(d_state, gw, gh, free_mask=d_mask, **o["foot"])
    assert (d_mask.cpu().numpy().view(np.uint32) == lay["free_mask"]).all() and foot_stats == lay["stats"] and lay["stats"]["cells_some"] > 0
    d_poses = torch.from_numpy(o["poses"]).to(dev)
    outs = {nm: torch.zeros(binding.Fusion._navsteer_shape(kind, tail, n, K, T), dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
            for nm, dt, kind, tail in binding.NAVSTEER_OUTPUTS}
    stats = fusion.nav_foot_steer_device(d_mask, d_dist2, gw, gh, d_poses, n, o["foot"]["n_headings"], cost=d_cost, min_dist2=o["plan"]["min_dist2"],
                                         **dict(outs, **o["steer"]))
    got = {nm: a.cpu().numpy().view(dt) if dt is np.uint32 else a.cpu().numpy() for (nm, dt, _, _), a in zip(binding.NAVSTEER_OUTPUTS, outs.values())}
    got["best_traj"] = [got["best_traj"][q, :got["best_len"][q]] for q in range(n)]
    got["stats"] = stats
    same(got, want, "device pointers")
    assert want["stats"]["poses_ok"] >= 3 and want["stats"]["poses_blocked"] >= 1 and want["stats"]["collided"] > 0
    # the footprint matters on this scene: the disc's rollouts differ
    disc = sr.rollouts(lv["state"], lv["dist2"], pl["cost"], o["poses"], None, c)
    assert (disc["cand_free"] != want["cand_free"]).any()


def test_overlay_plan_layers_and_rollouts_with_only_the_command_leaving_the_device(fusion):
    o = overlay_scene()
    lv, pl, lay, want, c = chained_restatements(o)
    got = fusion.nav_live_foot_steer(o["depth"], o["state_in"], o["goals"], o["poses"], o["foot"], live=live_kw(o), plan=o["plan"], steer=o["steer"],
                                     keep_mask=True)
    assert {k: got["live"]["stats"][k] for k in lr.STATS} == lv["stats"] and lv["stats"]["cells_stamped"] > 10
    assert {k: got["plan"]["stats"][k] for k in pr.STATS} == {k: pl["stats"][k] for k in pr.STATS}
    assert got["foot"]["stats"] == lay["stats"] and (got["foot"]["free_mask"] == lay["free_mask"]).all()
    same(got["steer"], want, "nav_live_foot_steer", outputs=binding.NAVSTEER_POSE_OUTPUTS)
    assert (got["steer"]["best_cmd"] == want["best_cmd"]).all() and (want["best"] > 0).any()


# ---- conventions -------------------------------------------------------------------------------------------------------------------
def test_a_call_between_two_frames_changes_no_later_result(foot_lib):
    A, B = handle(foot_lib), handle(foot_lib)
    state, foot, bins, allow, want = layer_case("37x53 asym one")
    i = fr.corridor_scene()
    for k in (0, 3, 6):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        got = A.nav_foot(state, outputs=("free_mask", "n_free"), **foot_kw(foot, bins, allow))
        assert (got["free_mask"] == want["free_mask"]).all() and got["stats"] == want["stats"]
        lay = A.nav_foot(i["state"], **foot_kw(i["foot"], i["B"]))
        foot_check(A, "between frames", lay["free_mask"], i["B"], i, i["c"], want=fr.cached(
            "corridor rollouts", lambda: fr.rollouts(lay["free_mask"], i["B"], i["dist2"], i["cost"], i["poses"], None, i["c"])))
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)
    B.close()
    A.close()


def test_the_refusals(foot_lib):
    f = handle(foot_lib)
    state, foot, B, allow, want = layer_case("37x53 asym one")
    base = foot_kw(foot, B, allow)
    refused = pytest.raises(binding.SsfError, match=r"ssf_navfoot_layers failed \(-1\)")
    for kw in (dict(front=-1), dict(back=24577), dict(left=-1), dict(right=1 << 20), dict(pad=-1), dict(pad=4097), dict(n_headings=0), dict(n_headings=3),
               dict(n_headings=64), dict(allow_unknown=2), dict(allow_unknown=-1)):
        with refused:
            f.nav_foot(state, **dict(base, **kw))
    with refused:
        f.nav_foot(state, outputs=(), **base)                            # every output NULL
    with refused:
        f.nav_foot(np.zeros((1, 4097), np.int8), **base)
    f.nav_foot(np.zeros((2, 4096), np.int8), **dict(base, front=24576, back=24576, left=24576, right=24576, pad=4096, n_headings=32))     # the limits themselves
    L, byref, vp = foot_lib.lib, binding.C.byref, binding.C.c_void_p
    p, st, out = binding.SsfNavFootParams(), binding.SsfNavFootStats(), binding.SsfNavFootOut()
    assert L.ssf_navfoot_default_params(f.h, byref(p)) == 0 and L.ssf_navfoot_default_params(None, byref(p)) == -1
    assert L.ssf_navfoot_default_params(f.h, None) == -1
    assert f.nav_foot_default_params() == dict(width=512, height=512, allow_unknown=0, n_headings=16, front=0, back=0, left=0, right=0, pad=0, on_device=0)
    p.width, p.height = 8, 4
    s8, m8 = np.zeros((4, 8), np.int8), np.zeros((4, 8), np.uint32)
    out.free_mask = m8.ctypes.data
    assert L.ssf_navfoot_layers(f.h, byref(p), s8.ctypes.data_as(vp), byref(out), None) == 0 and (m8 == 0xFFFF).all()        # stats are optional
    assert L.ssf_navfoot_layers(None, byref(p), s8.ctypes.data_as(vp), byref(out), byref(st)) == -1
    assert L.ssf_navfoot_layers(f.h, None, s8.ctypes.data_as(vp), byref(out), byref(st)) == -1
    assert L.ssf_navfoot_layers(f.h, byref(p), None, byref(out), byref(st)) == -1
    assert L.ssf_navfoot_layers(f.h, byref(p), s8.ctypes.data_as(vp), None, byref(st)) == -1
    assert L.ssf_navfoot_layers(f.h, byref(p), s8.ctypes.data_as(vp), byref(binding.SsfNavFootOut()), byref(st)) == -1
    for field, bad in (("width", 0), ("width", 4097), ("height", -3), ("height", 4097)):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert L.ssf_navfoot_layers(f.h, byref(p), s8.ctypes.data_as(vp), byref(out), byref(st)) == -1, (field, bad)
        setattr(p, field, keep)
    # the rollouts: the heading count, the mask, and the disc's refusals through the shared call
    i = fr.corridor_scene()
    c = i["c"]
    mask = f.nav_foot(i["state"], **foot_kw(i["foot"], i["B"]))["free_mask"]
    rolled = pytest.raises(binding.SsfError, match=r"ssf_navfoot_rollouts failed \(-1\)")
    for bins in (0, 3, 64, -1):
        with rolled:
            f.nav_foot_steer(mask, i["dist2"], i["poses"], bins, cost=i["cost"], **call_kw(c))
    for kw in (dict(min_dist2=-1), dict(allow_unknown=2), dict(n_v=0), dict(w_min=-16385, n_w=1), dict(n_steps=257), dict(cost_weight=1001), dict(walk=2),
               dict(cost_weight=0, target_weight=0, clear_weight=0, speed_weight=0, turn_weight=0)):
        with rolled:
            f.nav_foot_steer(mask, i["dist2"], i["poses"], i["B"], cost=i["cost"], **dict(call_kw(c), **kw))
    with rolled:                                                         # cost NULL with cost_weight > 0
        f.nav_foot_steer(mask, i["dist2"], i["poses"], i["B"], **call_kw(c))
    with rolled:
        f.nav_foot_steer(mask, i["dist2"], i["poses"], i["B"], cost=i["cost"], outputs=(), **call_kw(c))
    q, sp, so, ss = binding.SsfNavSteerParams(), binding.SsfNavSteerOut(), binding.SsfNavSteerStats(), np.zeros(3, np.int32)
    assert L.ssf_navsteer_default_params(f.h, byref(q)) == 0
    q.width, q.height, q.n_poses, q.cost_weight = 96, 40, 3, 0
    sp.best = ss.ctypes.data
    m, d, ps = mask.ctypes.data_as(vp), i["dist2"].ctypes.data_as(vp), i["poses"].ctypes.data_as(vp)
    assert L.ssf_navfoot_rollouts(f.h, byref(q), 32, m, d, None, ps, None, byref(sp), None) == 0 and (ss >= 0).all()
    assert L.ssf_navfoot_rollouts(f.h, byref(q), 32, None, d, None, ps, None, byref(sp), byref(so)) == -1
    assert L.ssf_navfoot_rollouts(f.h, byref(q), 32, m, None, None, ps, None, byref(sp), byref(so)) == -1
    assert L.ssf_navfoot_rollouts(f.h, byref(q), 32, m, d, None, None, None, byref(sp), byref(so)) == -1
    assert L.ssf_navfoot_rollouts(f.h, byref(q), 32, m, d, None, ps, None, None, byref(so)) == -1
    assert L.ssf_navfoot_rollouts(None, byref(q), 32, m, d, None, ps, None, byref(sp), byref(so)) == -1
    assert L.ssf_navfoot_rollouts(f.h, None, 32, m, d, None, ps, None, byref(sp), byref(so)) == -1
    # the handle keeps working: a call and a frame after the refusals
    got = f.nav_foot(state, outputs=("free_mask", "n_free"), **base)
    assert (got["free_mask"] == want["free_mask"]).all() and got["stats"] == want["stats"]
    f.process_frame(*util.frame(0, W, H))
    got = f.nav_foot(state, outputs=("free_mask",), **base)
    assert (got["free_mask"] == want["free_mask"]).all()
    g = handle(foot_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_foot(state, **base)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_foot_steer(mask, i["dist2"], i["poses"], i["B"], cost=i["cost"], **call_kw(c))
    q2 = handle(foot_lib, pipeline_depth=2, extract_batch=2)
    q2.submit_frame(*util.frame(0, W, H))
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q2.nav_foot(state, **base)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q2.nav_foot_steer(mask, i["dist2"], i["poses"], i["B"], cost=i["cost"], **call_kw(c))
    q2.process_submitted()
    got = q2.nav_foot(state, outputs=("free_mask",), **base)
    assert (got["free_mask"] == want["free_mask"]).all()
    q2.close()
    g.close()
    f.close()


def test_the_kernels_are_timed_under_profile(foot_lib):
    f = handle(foot_lib, profile=1)
    f.reset_kernel_times()
    i = fr.corridor_scene()
    lay = f.nav_foot(i["state"], **foot_kw(i["foot"], i["B"]))
    f.nav_foot_steer(lay["free_mask"], i["dist2"], i["poses"], i["B"], cost=i["cost"], **call_kw(i["c"]))
    names = f.kernel_times()
    for k in ("navfoot_layers", "navfoot_pack", "navfoot_roll", "navfoot_pick"):
        assert k in names and names[k][1] > 0, (k, names)
    f.close()


# ---- replay.py's files and the C++ surface ---------------------------------------------------------------------------------------------
def test_replay_writes_the_mask_and_logs_the_command(foot_lib, tmp_path, capsys):
    import os
    import re
    from supersurfel_fusion_amd import replay
    f = handle(foot_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    plan = dict(goals=[(12.0, 12.5)], frontier=True, radius=0.12)
    body = (0.25, 0.15, 0.1, 0.1)
    replay.replay(f, frames, nav_grid_dir=str(tmp_path), nav_grid_every=2, nav_grid_res=0.1, nav_plan=plan, nav_live=dict(min_hits=2, stride=8),
                  nav_steer=dict(horizon=16, speed=0.4, footprint=body, headings=8))
    assert all(os.path.exists(str(tmp_path / ("%06d%s" % (k, s)))) for k in (0, 2) for s in ("_foot_mask.npy", "_steer_traj.npy", "_cost.npy", "_live_state.npy"))
    pose = np.array([float(v) for v in re.search(r"grid_to_map: \[(.*)\]", open(str(tmp_path / "000002.yaml")).read()).group(1).split(",")], np.float32)
    state, dist2 = np.load(str(tmp_path / "000002_live_state.npy")), np.load(str(tmp_path / "000002_live_dist2.npy"))
    cost = np.load(str(tmp_path / "000002_cost.npy"))
    units = binding.Fusion.nav_foot_units(*body, 0.1)
    foot = (units["front"], units["back"], units["left"], units["right"], fr.pad_for(units["front"], units["back"], units["left"], units["right"], 8))
    lay = fr.layers(state, 0, foot, 8)
    mask = np.load(str(tmp_path / "000002_foot_mask.npy"))
    assert mask.dtype == np.uint32 and (mask == lay["free_mask"]).all()
    start = replay.steer_pose(pose, 0.1, f.get_pose())
    c = sr.params(width=state.shape[1], height=state.shape[0], n_poses=1, min_dist2=4, n_steps=16, **replay.steer_lattice(0.4, 0.1))
    want = fr.rollouts(mask, 8, dist2, cost, start, None, c)
    traj = np.load(str(tmp_path / "000002_steer_traj.npy"))
    assert traj.dtype == np.int32 and traj.shape == (want["best_len"][0], 3) and (traj == want["best_traj"][0, :want["best_len"][0]]).all()
    out = capsys.readouterr().out.splitlines()
    logged = [l for l in out if l.startswith("nav-steer ")]
    assert len(logged) == 2 and logged[1].startswith("nav-steer 000002: status=%d best=%d v=%d w=%d " % (
        want["pose_status"][0], want["best"][0], want["best_cmd"][0, 0], want["best_cmd"][0, 1])), logged
    assert all("%s=%d" % (k, want["stats"][k]) in logged[1] for k in sr.STATS)
    layers = [l for l in out if l.startswith("nav-foot ")]
    assert len(layers) == 2 and layers[1] == "nav-foot 000002: headings=8 " + " ".join("%s=%d" % (k, lay["stats"][k]) for k in fr.STATS), layers
    f.close()


def test_the_command_line_loads_the_library_of_the_footprint(tmp_path, capsys):
    """replay.main() with --nav-steer-footprint, end to end: it picks the library that exports the footprint's entry points itself"""
    import os
    from conftest import ROOT
    from supersurfel_fusion_amd import replay
    replay.main(["--npz", os.path.join(ROOT, "tests", "golden", "tum_fr1_xyz_8frames.npz"), "--out", str(tmp_path / "estimated.txt"),
                 "--nav-grid-dir", str(tmp_path), "--nav-grid-every", "4", "--nav-plan-frontier", "--nav-steer", "--nav-steer-horizon", "8",
                 "--nav-steer-footprint", "0.15", "0.1", "0.1", "0.1", "--nav-steer-headings", "8"])
    out = capsys.readouterr().out.splitlines()
    for k in (0, 4):
        mask, pgm_dist2 = np.load(str(tmp_path / ("%06d_foot_mask.npy" % k))), np.load(str(tmp_path / ("%06d_dist2.npy" % k)))
        assert mask.dtype == np.uint32 and mask.shape == pgm_dist2.shape and (mask >> np.uint32(8) == 0).all()
        assert os.path.exists(str(tmp_path / ("%06d_steer_traj.npy" % k)))
        assert len([l for l in out if l.startswith("nav-foot %06d: headings=8 cells_clear=" % k)]) == 1, out
        assert len([l for l in out if l.startswith("nav-steer %06d: status=" % k)]) == 1, out


def test_the_footprint_in_cpp(foot_lib, fusion, tmp_path):
    """tests/cpp/navfoot_smoke.cpp on the GPU: its counts and FNV-1a checksums equal those of the Python calls on the same arrays"""
    import os
    import re
    import subprocess
    from conftest import ROOT
    cpp = os.path.join(ROOT, "tests", "cpp")
    libdir = os.path.dirname(foot_lib.path)
    exe = str(tmp_path / "navfoot_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", cpp, os.path.join(cpp, "navfoot_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip_foot", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "messages ok=1" in r.stdout, r.stdout
    p = np.arange(70 * 45, dtype=np.uint64)
    h = ((p * 2654435761) & 0xFFFFFFFF) >> 16
    state = np.where(h % 100 < 3, 100, np.where(h % 100 < 5, -1, 0)).astype(np.int8).reshape(45, 70)
    dist2 = np.where(state.ravel() == 0, 1 + (h >> 7) % 40, 0).astype(np.int32).reshape(45, 70)
    cost = fusion.nav_plan(state, dist2, goals=[(60, 30)], outputs=("cost",))["cost"]
    poses = np.array([((5 + 11 * k) * 1024 + 300, (4 + 7 * k) * 1024 + 700, 9000 * k) for k in range(6)], np.int32)
    foot = (2048, 1024, 1024, 1024, 0)
    lay = fusion.nav_foot(state, outputs=("free_mask", "n_free"), **foot_kw(foot, 16))
    want_lay = fr.layers(state, 0, foot, 16)
    assert (lay["free_mask"] == want_lay["free_mask"]).all() and lay["stats"] == want_lay["stats"] and lay["stats"]["cells_some"] > 0
    told = re.search("navfoot " + " ".join(nm + r"=(\d+)" for nm in ("clear", "all", "some", "none", "reach", "cells")) + " mask=([0-9a-f]{16}) n_free=([0-9a-f]{16})", r.stdout)
    assert told, r.stdout
    assert tuple(int(v) for v in told.groups()[:6]) == tuple(lay["stats"][k] for k in fr.STATS)
    assert (int(told.group(7), 16), int(told.group(8), 16)) == (pr.fnv1a(lay["free_mask"].tobytes()), pr.fnv1a(lay["n_free"].tobytes()))
    c = sr.params(width=70, height=45, n_poses=6, n_steps=24)
    got = fusion.nav_foot_steer(lay["free_mask"], dist2, poses, 16, cost=cost, outputs=sr.OUTPUTS, n_steps=24)
    same(got, fr.rollouts(lay["free_mask"], 16, dist2, cost, poses, None, c), "the smoke program's arrays")
    counts = ("ok", "blocked", "stuck", "admissible", "collided", "steps")
    sums = ("best", "v", "w", "score", "traj", "cand_score", "cand_end")
    told = re.search("footsteer " + " ".join(nm + r"=(\d+)" for nm in counts) + " " + " ".join(nm + "=([0-9a-f]{16})" for nm in sums), r.stdout)
    assert told, r.stdout
    s = got["stats"]
    assert tuple(int(v) for v in told.groups()[:6]) == (s["poses_ok"], s["poses_blocked"], s["poses_stuck"], s["admissible"], s["collided"], s["steps_taken"])
    flat = np.concatenate(got["best_traj"]) if len(got["best_traj"]) else np.zeros((0, 3), np.int32)
    py_sums = tuple(pr.fnv1a(a.tobytes()) for a in (got["best"], np.ascontiguousarray(got["best_cmd"][:, 0]), np.ascontiguousarray(got["best_cmd"][:, 1]),
                                                      got["best_score"], flat, got["cand_score"], got["cand_end"]))
    assert tuple(int(v, 16) for v in told.groups()[6:]) == py_sums
    assert s["poses_ok"] >= 2 and s["collided"] > 0


def test_the_kept_table_follows_the_footprint(fusion):
    """the footprint's table stays on the device while the body is the same: one body twice, another, a change of pad alone, a change of
    the heading count alone, and the first again, each equal to the restatement"""
    state = grid(37, 53, "one")
    for name, foot, B in (("a", fr.ASYM, 32), ("a again", fr.ASYM, 32), ("line", fr.LINE, 32), ("pad", fr.ASYM[:4] + (0,), 32), ("bins", fr.ASYM[:4] + (0,), 8),
                          ("a at last", fr.ASYM, 32)):
        want = fr.cached(("kept", foot, B), lambda: fr.layers(state, 0, foot, B))
        got = fusion.nav_foot(state, outputs=("free_mask", "n_free"), **foot_kw(foot, B))
        assert (got["free_mask"] == want["free_mask"]).all() and (got["n_free"] == want["n_free"]).all() and got["stats"] == want["stats"], name
    with pytest.raises(binding.SsfError):                                # a refusal in between leaves the kept table as it was
        fusion.nav_foot(state, **dict(foot_kw(fr.ASYM, 32), pad=4097))
    got = fusion.nav_foot(state, **foot_kw(fr.ASYM, 32))
    assert (got["free_mask"] == fr.cached(("kept", fr.ASYM, 32), None)["free_mask"]).all()
