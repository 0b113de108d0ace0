"""Plan over (x, y, heading) (include/ssf_navpose.h) on the GPU: every array and every exact stat of ssf_navpose_field equals the
restatement (tests/navpose_ref.py) with ==, at the smallest grids at which the kernels can go wrong (one cell, one row, sizes that are
no multiple of the 16-cell tile, obstacles at a tile's corner, a corridor that needs more rounds than one host batch), through device
pointers fed by the overlay and the layers and read by the rollouts, through nav_live_pose_steer, and on the T-junction with the
disc's plan beside it."""
import numpy as np
import pytest

import navfoot_ref as fr
import navlive_ref as lr
import navplan_ref as pr
import navpose_ref as qr
import navsteer_ref as sr
import util
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
W, H = 160, 128
T = qr.TILE
SMALL = (1536, 512, 512, 512, 0)                                         # a body of 3 x 2 cells: survives on a cluttered grid
FOOT = dict(point=fr.POINT, line=fr.LINE, asym=fr.ASYM, small=SMALL)
ARRAYS = ("cost", "cell_cost", "cell_bin", "start_cost", "start_status", "path_len")


def handle(lib, **kw):
    """a handle of a test's own, which the test closes when it is done with it"""
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


@pytest.fixture(scope="module")
def pose_lib():
    """libssf_hip_pose.so: foot's objects plus the pose plan's entry points (no fallback: a missing .so is an error)"""
    return binding.load_pose()


@pytest.fixture(scope="module")
def fusion(pose_lib):
    f = handle(pose_lib)
    yield f
    f.close()


def same(got, want, what):
    for nm in ARRAYS:
        assert got[nm].dtype == want[nm].dtype and got[nm].shape == want[nm].shape, (what, nm, got[nm].dtype, got[nm].shape, want[nm].shape)
        diff = got[nm] != want[nm]
        assert not diff.any(), (what, nm, int(diff.sum()), np.argwhere(diff)[:5].tolist(), got[nm][diff][:5].tolist(), want[nm][diff][:5].tolist())
    assert len(got["path"]) == len(want["path"])
    for i, (a, b) in enumerate(zip(got["path"], want["path"])):
        assert a.shape == b.shape and (a == b).all(), (what, "path", i, a[:4].tolist(), b[:4].tolist())
    assert {k: got["stats"][k] for k in qr.STATS} == want["stats"], (what, got["stats"], want["stats"])


# ---- the table of cases ------------------------------------------------------------------------------------------------------------
def grid(h, w, obstacles, seed):
    """(state, dist2): dist2 at random in 0..40 (the call reads both as given)"""
    rng = np.random.default_rng(seed)
    state = np.zeros((h, w), np.int8)
    if obstacles == "random":                                             # obstacles and unknown cells
        u = rng.random((h, w))
        state = np.where(u < 0.12, 100, np.where(u < 0.2, -1, 0)).astype(np.int8)
    elif obstacles == "few":
        state[rng.random((h, w)) < 0.012] = 100
        state[rng.random((h, w)) < 0.01] = -1
    elif obstacles == "corner":
        state = qr.corner_grid(seed)[0]
    else:
        assert obstacles == "none"
    return state, rng.integers(0, 41, (h, w)).astype(np.int32)


# (name, h, w, footprint, B, obstacles, allow_unknown, the rule's parameters)
CASES = (
    ("1x1 point B1", 1, 1, "point", 1, "none", 0, dict()),
    ("1x1 asym B4", 1, 1, "asym", 4, "none", 0, dict()),
    ("1x1 point B32", 1, 1, "point", 32, "none", 0, dict(turn_cost=1000)),
    ("1x70 point B8 tol0", 1, 70, "point", 8, "few", 0, dict(move_tol=0)),
    ("1x70 line B32", 1, 70, "line", 32, "none", 0, dict(turn_cost=1)),
    ("1x70 point B2 no reverse", 1, 70, "point", 2, "none", 0, dict(allow_reverse=0)),
    ("37x53 point B1 tol256", 37, 53, "point", 1, "random", 0, dict(move_tol=256, reverse_cost=0)),
    ("37x53 point B1 no reverse", 37, 53, "point", 1, "random", 1, dict(allow_reverse=0)),
    ("37x53 small B2", 37, 53, "small", 2, "few", 0, dict()),
    ("37x53 small B4 tol0", 37, 53, "small", 4, "few", 1, dict(move_tol=0, turn_cost=1)),
    ("37x53 line B8 penalty", 37, 53, "line", 8, "few", 0, dict(soft_dist2=30, near_penalty=40)),
    ("37x53 asym B16", 37, 53, "asym", 16, "few", 0, dict(reverse_cost=1000)),
    ("37x53 small B32 no reverse", 37, 53, "small", 32, "random", 1, dict(allow_reverse=0, turn_cost=1)),
    ("37x53 point B16 turn1000", 37, 53, "point", 16, "random", 0, dict(turn_cost=1000, min_dist2=3)),
    ("corner point B4 tol256", 2 * T, 2 * T, "point", 4, "corner", 0, dict(move_tol=256)),
    ("corner small B8", 2 * T, 2 * T, "small", 8, "corner", 0, dict()),
    ("corner small B32 penalty", 2 * T, 2 * T, "small", 32, "corner", 0, dict(soft_dist2=25, near_penalty=1000, reverse_cost=3)),
    ("corner line B16 tol256", 2 * T, 2 * T, "line", 16, "corner", 0, dict(move_tol=256, reverse_cost=0, turn_cost=1)),
    ("97x33 point B8", 97, 33, "point", 8, "random", 1, dict(min_dist2=2)),
    ("97x33 small B1", 97, 33, "small", 1, "random", 0, dict()),
    ("97x33 small B16 penalty", 97, 33, "small", 16, "random", 1, dict(soft_dist2=40, near_penalty=17, move_tol=64)),
    ("97x33 small B32 tol256", 97, 33, "small", 32, "random", 1, dict(move_tol=256, turn_cost=1000)),
    ("97x33 line B4 no reverse", 97, 33, "line", 4, "few", 0, dict(allow_reverse=0, move_tol=0)),
    ("97x33 asym B32", 97, 33, "asym", 32, "few", 1, dict(turn_cost=1)),
    ("97x33 point B2 tol0", 97, 33, "point", 2, "random", 1, dict(move_tol=0, turn_cost=1000, reverse_cost=0)),
)


def case(name):
    """dict(mask, dist2, goals, starts, kw, want): the inputs and the restatement's answer, computed once and shared"""
    def make():
        i = [c[0] for c in CASES].index(name)
        _, h, w, foot, B, obstacles, allow, rule = CASES[i]
        state, dist2 = grid(h, w, obstacles, 100 + i)
        mask = fr.layers(state, allow, FOOT[foot], B)["free_mask"] if foot != "point" else qr.point_mask(state, allow, B)
        kw = dict(rule, n_headings=B, max_path=4096)
        trav, _ = qr.prep(mask, dist2, qr.params(**kw))
        rng = np.random.default_rng(500 + i)
        at = np.argwhere(trav)                                            # (b, y, x) of every traversable state
        goals = []
        if len(at):
            b, y, x = at[rng.integers(len(at))]
            goals.append((x, y, -1))                                      # every bin of a cell
            b, y, x = at[rng.integers(len(at))]
            goals.append((x, y, b))                                       # a named bin
        shut = np.argwhere(~trav)
        if len(shut):
            b, y, x = shut[rng.integers(len(shut))]
            goals.append((x, y, b))                                       # blocked: that bin does not fit there
        none = np.argwhere(~trav.any(axis=0))
        if len(none):
            goals.append((none[0][1], none[0][0], -1))                    # blocked: no bin fits there
        goals += [(-1, 0, 0), (w, 0, -1), (0, h, 0), (0, 0, B), (0, 0, -2)]        # outside, and a bad bin
        starts = np.stack([rng.integers(-600, w * 1024 + 600, 8), rng.integers(-600, h * 1024 + 600, 8), rng.integers(-70000, 140000, 8)], axis=1)
        if len(at):                                                       # two more that stand on traversable states
            for j in rng.integers(len(at), size=2):
                b, y, x = at[j]
                starts = np.vstack([starts, [x * 1024 + 100, y * 1024 + 1000, b * (65536 // B)]])
        goals, starts = np.array(goals, np.int32), starts.astype(np.int32)
        return dict(mask=mask, dist2=dist2, goals=goals, starts=starts, kw=kw, want=qr.plan(mask, dist2, goals, starts, **kw))
    return qr.cached(("case", name), make)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_the_field_the_projection_and_the_paths(name, fusion):
    c = case(name)
    want = c["want"]
    got = fusion.nav_pose_plan(c["mask"], c["dist2"], c["goals"], c["starts"], **c["kw"])
    same(got, want, name)
    s = want["stats"]
    assert s["goals_outside"] == 5 and s["goals_used"] + s["goals_blocked"] == len(c["goals"]) - 5
    if not name.startswith("1x1 asym"):                                   # (a body on a single cell fits nowhere: both goals are blocked)
        assert s["goals_used"] >= 1 and s["states_reached"] >= 1
    if "x1 " not in name:
        assert s["states_reached"] > 10 and (s["goals_blocked"] >= 1 or s["states_traversable"] == c["want"]["trav"].size), s
    assert got["stats"]["rounds"] >= (1 if s["goals_used"] else 0) and got["stats"]["tile_visits"] >= got["stats"]["rounds"]


def narrow_last_tile(h, w, B):
    """dict(mask, dist2, goals, starts, kw, want): a free grid with a handful of fixed obstacle cells, the goal in the last column --
    which is one cell wide at 17 and 33 columns -- and the start in the opposite corner; every move allowed, so B = 1 reaches it"""
    def make():
        state = np.zeros((h, w), np.int8)
        for x, y in ((5, 3), (9, 9), (15, 8), (16, 2), (2, 15), (20, 7), (31, 12), (32, 3)):
            if x < w and y < h: state[y, x] = 100
        dist2 = ((7 * np.arange(w)[None, :] + 3 * np.arange(h)[:, None]) % 41).astype(np.int32)
        mask = qr.point_mask(state, 0, B)
        kw = dict(n_headings=B, move_tol=256, max_path=4096)
        goals, starts = np.array([(w - 1, h - 1, -1)], np.int32), np.array([(512, 512, 0)], np.int32)
        return dict(mask=mask, dist2=dist2, goals=goals, starts=starts, kw=kw, want=qr.plan(mask, dist2, goals, starts, **kw))
    return qr.cached(("narrow last tile", h, w, B), make)


@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("h,w", [(1, 1), (17, 17), (16, 33)])
def test_a_last_tile_column_or_row_one_cell_wide(h, w, B, fusion):
    """the smallest grids at which the seers of a tile's edge cells and the flags of its neighbours can go wrong: the goal's tile is
    one cell wide (17 x 17: and one cell high), so every round's news crosses a tile boundary at once"""
    c = narrow_last_tile(h, w, B)
    want = c["want"]
    assert want["stats"]["goals_used"] == 1 and want["start_status"][0] == qr.STATUS_REACHED        # (no all-INF field passes)
    assert want["path_len"][0] >= max(h, w) and want["stats"]["cells_reached"] == int(want["trav"].any(axis=0).sum())
    same(fusion.nav_pose_plan(c["mask"], c["dist2"], c["goals"], c["starts"], **c["kw"]), want, (h, w, B))


def test_a_serpentine_that_needs_more_rounds_than_one_batch(fusion):
    """one-cell corridors that cross the boundary between two tile columns once per lane: every crossing costs a round, so the field
    settles only in the host's second batch of rounds or later"""
    state, dist2 = qr.serpentine(2 * T + 3, 2 * T + 1)
    mask = qr.point_mask(state, 0, 1)
    kw = dict(n_headings=1, move_tol=256, reverse_cost=0, max_path=4096)
    goals, starts = [(0, 0, -1)], [(2 * T * 1024 + 512, (2 * T + 2) * 1024 + 512, 0)]
    want = qr.cached("serpentine", lambda: qr.plan(mask, dist2, goals, starts, **kw))
    got = fusion.nav_pose_plan(mask, dist2, goals, starts, **kw)
    same(got, want, "serpentine")
    assert got["stats"]["rounds"] > binding.NAVPOSE_ROUND_BATCH == qr.ROUND_BATCH, got["stats"]
    assert want["stats"]["states_reached"] == want["stats"]["states_traversable"] and want["start_status"][0] == 0
    assert want["path_len"][0] > (T + 1) * (2 * T + 1)                      # the path walks every lane


# ---- starts ------------------------------------------------------------------------------------------------------------------------
def starts_scene():
    """a room of 37 x 53 cells cut in two by a wall; the small body at 8 bins; one goal with a named bin on the left"""
    state = np.zeros((37, 53), np.int8)
    state[:, 30] = 100
    dist2 = np.full((37, 53), 50, np.int32)
    mask = fr.layers(state, 0, SMALL, 8)["free_mask"]
    c = sr.centre
    starts = np.array([c(5, 30, 0), c(60, 3, 0), c(-1, 3, 0), c(30, 10, 0), c(29, 10, 0), c(45, 20, 8192), c(10, 8, 3 * 8192), c(10, 8, 65536 + 5 * 8192 + 4095),
                       c(20, 8, 8192 - 4096), c(20, 8, 8192 - 4097)], np.int32)
    return mask, dist2, np.array([(10, 8, 1)], np.int32), starts


def test_the_five_statuses_and_the_paths_lengths(fusion):
    mask, dist2, goals, starts = starts_scene()
    kw = dict(n_headings=8)
    full = qr.cached("starts", lambda: qr.plan(mask, dist2, goals, starts, max_path=4096, **kw))
    st = full["start_status"].tolist()
    assert st == [0, 1, 1, 2, 2, 3, 0, 0, 0, 0], st                      # (29, 10) at bin 0: the body's front stands in the wall
    L = int(full["path_len"][0])
    assert L > 20 and len(set(full["path_len"][[0, 6, 7]].tolist())) == 3
    # a path that is rotations only: the start stands in the goal's cell, two and four bins off
    for i, n in ((6, 3), (7, 5)):
        p = full["path"][i]
        assert len(p) == n and (p[:, :2] == (10, 8)).all() and p[-1, 2] == 1 and full["start_cost"][i] == 5 * (n - 1)
    assert full["path"][0][-1].tolist() == [10, 8, 1] and full["path"][8][0, 2] == 1 and full["path"][9][0, 2] == 0      # the bin's edge
    for mp in (4096, L, L - 1, 1, 0):
        want = qr.cached(("starts", mp), lambda: qr.plan(mask, dist2, goals, starts, max_path=mp, **kw))
        got = fusion.nav_pose_plan(mask, dist2, goals, starts, max_path=mp, **kw)
        same(got, want, "max_path %d" % mp)
        if 0 < mp < L:
            assert want["start_status"][0] == 4 and want["path_len"][0] == mp
        if mp == L:
            assert want["start_status"][0] == 0 and want["path_len"][0] == L and (want["start_status"] == 4).sum() == 0
        if mp == 0:
            assert (want["path_len"] == 0).all() and want["start_status"].tolist() == st
    # the paths alone, and the status alone
    got = fusion.nav_pose_plan(mask, dist2, goals, starts, outputs=("path",), max_path=L, **kw)
    assert sorted(got) == ["path", "stats"] and all((a == b).all() for a, b in zip(got["path"], full["path"]))
    got = fusion.nav_pose_plan(mask, dist2, goals, starts, outputs=("start_status",), max_path=L, **kw)
    assert sorted(got) == ["start_status", "stats"] and got["start_status"].tolist() == st


# ---- the staging of a host grid --------------------------------------------------------------------------------------------------------
FILL = util.GUARD_WORD


def staging_case(h, w):
    """dict(mask, dist2, goals, starts, kw, want): a floor with a few obstacles, the small body at 8 bins (on one cell: the point), two
    goals and five starts; the restatement's answer, computed once and shared"""
    def make():
        state, dist2 = grid(h, w, "few", 700 + h + w)
        state[h // 2, w // 2] = 0
        mask = fr.layers(state, 0, SMALL, 8)["free_mask"] if min(h, w) >= 8 else qr.point_mask(state, 0, 8)
        kw = dict(n_headings=8, soft_dist2=30, near_penalty=40, max_path=256)
        rng = np.random.default_rng(h * w)
        goals = np.array([(w // 2, h // 2, -1), (w - 1, 0, 2), (w, 0, 0)], np.int32)
        starts = np.stack([rng.integers(0, w * 1024, 5), rng.integers(0, h * 1024, 5), rng.integers(-70000, 140000, 5)], axis=1).astype(np.int32)
        return dict(mask=mask, dist2=dist2, goals=goals, starts=starts, kw=kw, want=qr.plan(mask, dist2, goals, starts, **kw))
    return qr.cached(("staging", h, w), make)


def pose_host(f, c, names):
    """ssf_navpose_field with host arrays, the outputs `names` alone, each between guard bytes and filled with them: (name -> array, stats)"""
    (h, w), n, mp, B = c["mask"].shape, len(c["starts"]), c["kw"]["max_path"], c["kw"]["n_headings"]
    shapes = dict(cost=((B, h, w), np.uint32), cell_cost=((h, w), np.uint32), cell_bin=((h, w), np.uint8), start_cost=((n,), np.uint32),
                  start_status=((n,), np.int32), path_len=((n,), np.int32), path=((n, mp, 3), np.int32))
    out = {nm: util.guarded(*shapes[nm]) for nm in names}
    p, keep = f._navpose_params(False, w, h, c["goals"], c["starts"], c["kw"])
    stats = f._navpose_field(p, binding._ptr(c["mask"]), binding._ptr(c["dist2"]), {nm: binding._ptr(a) for nm, (a, _) in out.items()})
    assert all(intact() for _, intact in out.values()), names
    return {nm: a for nm, (a, _) in out.items()}, stats


def pose_same(got, want, what):
    """every array of got equals the restatement's; a path up to its length, and past it it holds the fill"""
    for nm, a in got.items():
        if nm != "path":
            assert a.dtype == want[nm].dtype and a.shape == want[nm].shape and (a == want[nm]).all(), (what, nm)
            continue
        for i, states in enumerate(want["path"]):
            assert (a[i, :len(states)] == states).all() and (a[i, len(states):] == FILL).all(), (what, nm, i)


@pytest.mark.parametrize("h,w", [(19, 37), (1, 1)])
def test_a_host_grid_whose_arrays_start_at_rounded_offsets(h, w, fusion):
    """703 cells and one cell: 4 P is no multiple of 256, so dist2 sits at a rounded offset of the staging buffer.  Host arrays,
    device pointers and the restatement agree"""
    import torch
    c = staging_case(h, w)
    host, hs = pose_host(fusion, c, binding.NAVPOSE_OUTPUT_NAMES)
    pose_same(host, c["want"], "host %d x %d" % (h, w))
    t = {nm: torch.full(a.shape, util.GUARD_FILL, dtype=torch.uint8, device="cuda") if a.dtype == np.uint8 else torch.full(a.shape, FILL, dtype=torch.int32, device="cuda")
         for nm, a in host.items()}
    ds = fusion.nav_pose_plan_device(torch.from_numpy(c["mask"].view(np.int32)).to("cuda"), torch.from_numpy(c["dist2"]).to("cuda"), w, h, c["goals"], c["starts"],
                                     **dict(t, **c["kw"]))
    assert all(host[nm].tobytes() == t[nm].cpu().numpy().tobytes() for nm in host)
    assert {k: hs[k] for k in qr.STATS} == {k: ds[k] for k in qr.STATS} == c["want"]["stats"]
    assert h == 1 or (c["want"]["stats"]["states_reached"] > 1000 and (c["want"]["path_len"] > 1).any() and c["want"]["stats"]["goals_outside"] == 1)


@pytest.mark.parametrize("name", binding.NAVPOSE_OUTPUT_NAMES)
def test_one_host_output_alone_between_guard_bytes(name, fusion):
    """19 x 37, host arrays: every output on its own, all others NULL, equals the same array of the call that asks for all seven, and
    the 256 bytes on either side of the caller's array are untouched"""
    c = staging_case(19, 37)
    every, stats = qr.cached("staging every", lambda: pose_host(fusion, c, binding.NAVPOSE_OUTPUT_NAMES))
    pose_same(every, c["want"], "every output")
    alone, st = pose_host(fusion, c, (name,))
    assert alone[name].tobytes() == every[name].tobytes() and {k: st[k] for k in qr.STATS} == {k: stats[k] for k in qr.STATS}, name


def test_the_staging_buffer_grows_and_is_used_again(pose_lib):
    """one handle: 8 x 8, 19 x 37, 8 x 8 again.  Each call gives what a handle that has made no other call gives"""
    f = handle(pose_lib)
    for h, w in ((8, 8), (19, 37), (8, 8)):
        c = staging_case(h, w)
        fresh = handle(pose_lib)
        (got, gs), (want, ws) = pose_host(f, c, binding.NAVPOSE_OUTPUT_NAMES), pose_host(fresh, c, binding.NAVPOSE_OUTPUT_NAMES)
        fresh.close()
        assert all(got[nm].tobytes() == want[nm].tobytes() for nm in got) and {k: gs[k] for k in qr.STATS} == {k: ws[k] for k in qr.STATS}, (h, w)
        pose_same(got, c["want"], (h, w))
    f.close()


# ---- device pointers -------------------------------------------------------------------------------------------------------------------
def overlay_scene():
    """a depth frame over a free floor (tests/navlive_ref.py's room): what the overlay, the layers and the pose plan make of it is steered on"""
    kw = dict(lr.CAMERA, width=33, height=31, res=0.05, max_dist_cells=6, stride=4)
    cam_pose, grid_pose = lr.room_pose(at=(0.8, 0.0, 0.2)), lr.grid_pose_at()
    depth = lr.room_depth(cam_pose)
    state_in = np.zeros((31, 33), np.int8)
    state_in[:, :2] = -1
    S = sr.SUB
    poses = np.array([sr.centre(16, 4, 16384), sr.centre(2, 2, 0), (40 * S, S, 0), sr.centre(16, 4, 0), sr.centre(20, 8, 20000), sr.centre(10, 27, 50000)], np.int32)
    foot = dict(front=1536, back=512, left=512, right=512, n_headings=16, pad=0)
    return dict(kw=kw, cam_pose=cam_pose, grid_pose=grid_pose, depth=depth, state_in=state_in, goals=[(16, 29, -1), (3, 3, 4)], pose=dict(min_dist2=1, turn_cost=3),
                poses=poses, steer=dict(n_steps=20, clearance_cap=36, brake_div=64), foot=foot)


def live_kw(o):
    return dict({k: v for k, v in o["kw"].items() if k not in ("width", "height")}, grid_pose=o["grid_pose"], cam_pose=o["cam_pose"])


def chained_restatements(o):
    def make():
        lv = lr.overlay(o["depth"], None, o["state_in"], o["grid_pose"], o["cam_pose"], lr.params(**o["kw"]))
        ft = o["foot"]
        lay = fr.layers(lv["state"], 0, (ft["front"], ft["back"], ft["left"], ft["right"], ft["pad"]), ft["n_headings"])
        pl = qr.plan(lay["free_mask"], lv["dist2"], o["goals"], o["poses"], n_headings=ft["n_headings"], max_path=64, **o["pose"])
        c = sr.params(width=33, height=31, n_poses=len(o["poses"]), min_dist2=o["pose"]["min_dist2"], **o["steer"])
        return lv, lay, pl, fr.rollouts(lay["free_mask"], ft["n_headings"], lv["dist2"], pl["cell_cost"], o["poses"], None, c), c
    return qr.cached("chain", make)


def same_steer(got, want, what, outputs):
    for nm in outputs:
        if nm == "best_traj":
            for q in range(len(want["best_len"])):
                assert (np.asarray(got[nm][q]) == want[nm][q, :want["best_len"][q]]).all(), (what, nm, q)
        else:
            assert (np.asarray(got[nm]) == want[nm]).all(), (what, nm, np.asarray(got[nm]).tolist(), want[nm].tolist())


def test_device_pointers_from_the_layers_into_the_plan_and_from_the_plan_into_the_rollouts(fusion):
    import torch
    dev = torch.device("cuda")
    o = overlay_scene()
    lv, lay, pl, want, c = chained_restatements(o)
    gw, gh, n, B, mp = 33, 31, len(o["poses"]), o["foot"]["n_headings"], 64
    d_depth, d_state = torch.from_numpy(o["depth"]).to(dev), torch.from_numpy(o["state_in"]).to(dev)
    d_dist2, d_cell, d_mask = (torch.empty((gh, gw), dtype=torch.int32, device=dev) for _ in range(3))
    fusion.nav_live_device(d_depth, d_state, gw, gh, state_out=d_state, dist2=d_dist2, **live_kw(o))
    foot_stats = fusion.nav_foot_device(d_state, gw, gh, free_mask=d_mask, **o["foot"])
    assert (d_mask.cpu().numpy().view(np.uint32) == lay["free_mask"]).all() and foot_stats == lay["stats"] and lay["stats"]["cells_some"] > 0
    d_field = torch.full((B, gh, gw), 7, dtype=torch.int32, device=dev)
    d_bin = torch.full((gh, gw), 7, dtype=torch.uint8, device=dev)
    d_sc, d_ss, d_pl = (torch.full((n,), 7, dtype=torch.int32, device=dev) for _ in range(3))
    d_path = torch.full((n, mp, 3), -7, dtype=torch.int32, device=dev)
    stats = fusion.nav_pose_plan_device(d_mask, d_dist2, gw, gh, o["goals"], o["poses"], cost=d_field, cell_cost=d_cell, cell_bin=d_bin, start_cost=d_sc,
                                        start_status=d_ss, path_len=d_pl, path=d_path, n_headings=B, max_path=mp, **o["pose"])
    path = d_path.cpu().numpy()
    got = dict(cost=d_field.cpu().numpy().view(np.uint32), cell_cost=d_cell.cpu().numpy().view(np.uint32), cell_bin=d_bin.cpu().numpy(),
               start_cost=d_sc.cpu().numpy().view(np.uint32), start_status=d_ss.cpu().numpy(), path_len=d_pl.cpu().numpy(), stats=stats)
    got["path"] = [path[i, :got["path_len"][i]] for i in range(n)]
    same(got, pl, "device pointers")
    assert all((path[i, got["path_len"][i]:] == -7).all() for i in range(n))             # entries past path_len are not written
    assert (pl["start_status"] == 0).sum() >= 3 and pl["stats"]["goals_used"] == 2 and (pl["cell_bin"] != 255).sum() > 100
    # the projection alone, into the caller's array: the library's own field
    d_cell2 = torch.full((gh, gw), 7, dtype=torch.int32, device=dev)
    fusion.nav_pose_plan_device(d_mask, d_dist2, gw, gh, o["goals"], None, cell_cost=d_cell2, n_headings=B, **o["pose"])
    assert (d_cell2.cpu().numpy().view(np.uint32) == pl["cell_cost"]).all()
    # the rollouts read cell_cost where it lies
    d_poses = torch.from_numpy(o["poses"]).to(dev)
    K, Tn = c["n_v"] * c["n_w"], c["n_steps"]
    outs = {nm: torch.zeros(binding.Fusion._navsteer_shape(kind, tail, n, K, Tn), dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
            for nm, dt, kind, tail in binding.NAVSTEER_OUTPUTS}
    fusion.nav_foot_steer_device(d_mask, d_dist2, gw, gh, d_poses, n, B, cost=d_cell, min_dist2=o["pose"]["min_dist2"], **dict(outs, **o["steer"]))
    gs = {nm: a.cpu().numpy().view(dt) if dt is np.uint32 else a.cpu().numpy() for (nm, dt, _, _), a in zip(binding.NAVSTEER_OUTPUTS, outs.values())}
    gs["best_traj"] = [gs["best_traj"][q, :gs["best_len"][q]] for q in range(n)]
    same_steer(gs, want, "device pointers", sr.OUTPUTS)
    assert want["stats"]["poses_ok"] >= 3


def test_overlay_layers_pose_plan_and_rollouts_with_only_the_command_leaving_the_device(fusion):
    o = overlay_scene()
    lv, lay, pl, want, c = chained_restatements(o)
    got = fusion.nav_live_pose_steer(o["depth"], o["state_in"], o["goals"], o["poses"], o["foot"], live=live_kw(o), pose=o["pose"], steer=o["steer"],
                                     keep_mask=True, keep_cost=True)
    assert {k: got["live"]["stats"][k] for k in lr.STATS} == lv["stats"] and lv["stats"]["cells_stamped"] > 10
    assert got["foot"]["stats"] == lay["stats"] and (got["foot"]["free_mask"] == lay["free_mask"]).all()
    assert {k: got["pose"]["stats"][k] for k in qr.STATS} == pl["stats"] and (got["pose"]["cell_cost"] == pl["cell_cost"]).all()
    same_steer(got["steer"], want, "nav_live_pose_steer", binding.NAVSTEER_POSE_OUTPUTS)
    assert (want["best"] > 0).any()


# ---- the scene the call is there for ---------------------------------------------------------------------------------------------------
TJ_STEER = dict(n_steps=16, n_v=5, n_w=9, v_min=0, v_step=128, w_min=-4096, w_step=1024)


@pytest.mark.parametrize("B", [32, 8])
def test_the_t_junction(B, fusion):
    for detour in (False, True):
        s = qr.tjunction_scene(detour)
        kw = dict(qr.TJ_KW, n_headings=B, max_path=4096)
        lay = fusion.nav_foot(s["state"], **dict(zip(("front", "back", "left", "right", "pad"), s["foot"]), n_headings=B))
        want_lay = qr.cached(("tj layers", detour, B), lambda: fr.layers(s["state"], 0, s["foot"], B))
        assert (lay["free_mask"] == want_lay["free_mask"]).all()
        want = qr.cached(("tj", detour, B), lambda: qr.plan(lay["free_mask"], s["dist2"], s["goals"], s["start"], **kw))
        got = fusion.nav_pose_plan(lay["free_mask"], s["dist2"], s["goals"], s["start"], **kw)
        same(got, want, "t-junction %s" % detour)
        disc = fusion.nav_plan(s["state"], s["dist2"], [s["goal_cell"]], [s["start_cell"]], min_dist2=qr.TJ_DISC_MIN_DIST2, max_path=4096)
        want_disc = qr.cached(("tj disc", detour), lambda: pr.plan(s["state"], s["dist2"], [s["goal_cell"]], [s["start_cell"]], min_dist2=qr.TJ_DISC_MIN_DIST2,
                                                                   max_path=4096))
        assert (disc["cost"] == want_disc["cost"]).all() and disc["start_status"][0] == 0
        on_bend = ((disc["path"][0][:, 0] >= 33) & (disc["path"][0][:, 1] <= 14)).any()
        assert on_bend                                                   # the disc turns where the corridors meet, with or without the detour
        sx, sy = s["start_cell"]
        if not detour:
            assert got["start_status"][0] == 3 and (got["cost"][:, sy, sx] == qr.INF).all() and got["cell_bin"][sy, sx] == 255
            assert (got["cost"][:, :, :33] == qr.INF).all() and got["stats"]["states_reached"] > 0          # all reached states lie in the vertical corridor
            continue
        assert got["start_status"][0] == 0 and int(got["start_cost"][0]) > int(disc["start_cost"][0])
        p = got["path"][0]
        junction = (p[:, 0] >= 40) & (p[:, 0] < 48) & (p[:, 1] >= 8) & (p[:, 1] < 15)
        lengthwise = np.minimum(np.minimum(p[:, 2], B - p[:, 2]), np.abs(p[:, 2] - B // 2)) <= 1
        assert junction.any() and lengthwise[junction].all(), p[junction & ~lengthwise].tolist()
        assert (p[:, 1] > 36).any() and p[-1, :2].tolist() == list(s["goal_cell"])                # through the room, into the corridor from below
        # the rollouts on cell_cost: the winner drives along the corridor
        c = sr.params(width=70, height=64, n_poses=1, **TJ_STEER)
        steer = fusion.nav_foot_steer(lay["free_mask"], s["dist2"], s["start"], B, cost=got["cell_cost"], **TJ_STEER)
        want_steer = qr.cached(("tj steer", B), lambda: fr.rollouts(lay["free_mask"], B, s["dist2"], want["cell_cost"], s["start"], None, c))
        same_steer(steer, want_steer, "t-junction rollouts", binding.NAVSTEER_POSE_OUTPUTS)
        assert steer["pose_status"][0] == 0 and steer["best_cmd"][0, 0] > 0 and steer["best_cmd"][0, 1] == 0
        end = steer["best_traj"][0][-1]
        assert end[0] >> 10 > sx + 1 and end[1] >> 10 == sy and steer["best_len"][0] == TJ_STEER["n_steps"] + 1


# ---- conventions -------------------------------------------------------------------------------------------------------------------
def test_a_call_between_two_frames_changes_no_later_result(pose_lib):
    A, B = handle(pose_lib), handle(pose_lib)
    c = case("37x53 small B4 tol0")
    for k in (0, 3, 6):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        same(A.nav_pose_plan(c["mask"], c["dist2"], c["goals"], c["starts"], **c["kw"]), c["want"], "between frames")
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)
    B.close()
    A.close()


def test_the_refusals_leave_the_handle_working(pose_lib):
    f = handle(pose_lib)
    c = case("37x53 small B4 tol0")
    mask, dist2, goals, starts, base, want = c["mask"], c["dist2"], c["goals"], c["starts"], c["kw"], c["want"]
    valid = lambda: same(f.nav_pose_plan(mask, dist2, goals, starts, **base), want, "after a refusal")
    valid()
    refused = pytest.raises(binding.SsfError, match=r"ssf_navpose_field failed \(-1\)")
    for kw in (dict(n_headings=0), dict(n_headings=3), dict(n_headings=64), dict(n_headings=-4), dict(min_dist2=-1), dict(soft_dist2=-1),
               dict(soft_dist2=1024 * 1024 + 1), dict(near_penalty=-1), dict(near_penalty=1001), dict(move_tol=-1), dict(move_tol=257), dict(allow_reverse=2),
               dict(allow_reverse=-1), dict(reverse_cost=-1), dict(reverse_cost=1001), dict(turn_cost=0), dict(turn_cost=1001), dict(max_path=-1),
               dict(max_path=(1 << 20) + 1)):
        with refused:
            f.nav_pose_plan(mask, dist2, goals, starts, **dict(base, **kw))
        valid()
    with refused:
        f.nav_pose_plan(mask, dist2, goals, starts, outputs=(), **base)                  # every output NULL
    valid()
    with refused:
        f.nav_pose_plan(mask, dist2, None, starts, **base)                               # n_goals 0
    with refused:
        f.nav_pose_plan(mask, dist2, np.zeros((65537, 3), np.int32), starts, **base)
    with refused:
        f.nav_pose_plan(mask, dist2, goals, np.zeros((4097, 3), np.int32), **base)
    valid()
    with refused:
        f.nav_pose_plan(np.zeros((1, 4097), np.uint32), np.zeros((1, 4097), np.int32), goals, **dict(base, n_headings=1))
    with refused:                                                        # 2^26 states + one row
        f.nav_pose_plan(np.zeros((2049, 1024), np.uint32), np.zeros((2049, 1024), np.int32), goals, outputs=("cell_cost",), **dict(base, n_headings=32))
    with refused:                                                        # 1024 * 2^22 >= 2^32 - 1: a cost could wrap
        f.nav_pose_plan(np.zeros((2048, 2048), np.uint32), np.zeros((2048, 2048), np.int32), goals, outputs=("cell_cost",),
                        **dict(base, n_headings=1, near_penalty=1000, soft_dist2=4, reverse_cost=10))
    with refused:                                                        # the turn alone: 1000 * 2^23 >= 2^32 - 1
        f.nav_pose_plan(np.zeros((2048, 2048), np.uint32), np.zeros((2048, 2048), np.int32), goals, outputs=("cell_cost",),
                        **dict(base, n_headings=2, turn_cost=1000))
    valid()
    L, byref, vp = pose_lib.lib, binding.C.byref, binding.C.c_void_p
    p, st, out = binding.SsfNavPoseParams(), binding.SsfNavPoseStats(), binding.SsfNavPoseOut()
    assert L.ssf_navpose_default_params(f.h, byref(p)) == 0 and L.ssf_navpose_default_params(None, byref(p)) == -1
    assert L.ssf_navpose_default_params(f.h, None) == -1
    assert f.nav_pose_default_params() == dict(width=512, height=512, n_headings=16, min_dist2=0, soft_dist2=0, near_penalty=0, move_tol=64, allow_reverse=1,
                                               reverse_cost=10, turn_cost=5, n_goals=0, n_starts=0, max_path=0, on_device=0)
    m8, d8, c8, g8 = np.full((4, 8), 0xFFFF, np.uint32), np.ones((4, 8), np.int32), np.zeros((4, 8), np.uint32), np.array([[7, 3, -1]], np.int32)
    p.width, p.height, p.goals, p.n_goals = 8, 4, g8.ctypes.data, 1
    out.cell_cost = c8.ctypes.data
    m, d = m8.ctypes.data_as(vp), d8.ctypes.data_as(vp)
    assert L.ssf_navpose_field(f.h, byref(p), m, d, byref(out), None) == 0 and c8[3, 7] == 0 and c8[3, 0] == 70        # stats are optional
    assert L.ssf_navpose_field(None, byref(p), m, d, byref(out), byref(st)) == -1
    assert L.ssf_navpose_field(f.h, None, m, d, byref(out), byref(st)) == -1
    assert L.ssf_navpose_field(f.h, byref(p), None, d, byref(out), byref(st)) == -1
    assert L.ssf_navpose_field(f.h, byref(p), m, None, byref(out), byref(st)) == -1
    assert L.ssf_navpose_field(f.h, byref(p), m, d, None, byref(st)) == -1
    assert L.ssf_navpose_field(f.h, byref(p), m, d, byref(binding.SsfNavPoseOut()), byref(st)) == -1
    for field, bad in (("width", 0), ("width", 4097), ("height", -3), ("height", 4097), ("goals", None), ("n_goals", 0), ("n_starts", 1), ("n_starts", -1)):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert L.ssf_navpose_field(f.h, byref(p), m, d, byref(out), byref(st)) == -1, (field, bad)
        setattr(p, field, keep)
    assert L.ssf_navpose_field(f.h, byref(p), m, d, byref(out), byref(st)) == 0 and st.states_reached == 16 * 32
    valid()
    # the handle keeps working: a frame and a call after the refusals
    f.process_frame(*util.frame(0, W, H))
    valid()
    g = handle(pose_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_pose_plan(mask, dist2, goals, starts, **base)
    q2 = handle(pose_lib, pipeline_depth=2, extract_batch=2)
    q2.submit_frame(*util.frame(0, W, H))
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q2.nav_pose_plan(mask, dist2, goals, starts, **base)
    q2.process_submitted()
    same(q2.nav_pose_plan(mask, dist2, goals, starts, **base), want, "after the pipeline drained")
    q2.close()
    g.close()
    f.close()


def test_the_kernels_are_timed_under_profile(pose_lib):
    f = handle(pose_lib, profile=1)
    f.reset_kernel_times()
    c = case("37x53 small B4 tol0")
    f.nav_pose_plan(c["mask"], c["dist2"], c["goals"], c["starts"], **c["kw"])
    names = f.kernel_times()
    for k in ("navpose_init", "navpose_goals", "navpose_relax", "navpose_stats", "navpose_trace"):
        assert k in names and names[k][1] > 0, (k, names)
    f.close()


# ---- replay.py's files and the C++ surface ---------------------------------------------------------------------------------------------
def test_replay_writes_the_pose_plan_and_steers_on_it(pose_lib, tmp_path, capsys):
    import os
    import re
    from supersurfel_fusion_amd import replay
    f = handle(pose_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    plan = dict(goals=[(12.0, 12.5)], frontier=False, radius=0.12)
    body = (0.25, 0.15, 0.1, 0.1)
    replay.replay(f, frames, nav_grid_dir=str(tmp_path), nav_grid_every=2, nav_grid_res=0.1, nav_plan=plan, nav_live=dict(min_hits=2, stride=8),
                  nav_steer=dict(horizon=16, speed=0.4, footprint=body, headings=8, poses=dict(turn_cost=7)))
    k = "000002"
    assert all(os.path.exists(str(tmp_path / (k + s))) for s in ("_foot_mask.npy", "_pose_cost.npy", "_pose_bin.npy", "_pose_path.npy", "_steer_traj.npy"))
    pose = np.array([float(v) for v in re.search(r"grid_to_map: \[(.*)\]", open(str(tmp_path / (k + ".yaml"))).read()).group(1).split(",")], np.float32)
    dist2, mask = np.load(str(tmp_path / (k + "_live_dist2.npy"))), np.load(str(tmp_path / (k + "_foot_mask.npy")))
    start = replay.steer_pose(pose, 0.1, f.get_pose())
    _, goals = replay.plan_cells(pose, 0.1, f.get_pose()[9:12], plan["goals"])
    want = qr.plan(mask, dist2, [(int(goals[0][0]), int(goals[0][1]), -1)], start, n_headings=8, min_dist2=4, turn_cost=7, max_path=16 * sum(mask.shape))
    cell_cost = np.load(str(tmp_path / (k + "_pose_cost.npy")))
    assert cell_cost.dtype == np.uint32 and (cell_cost == want["cell_cost"]).all() and (np.load(str(tmp_path / (k + "_pose_bin.npy"))) == want["cell_bin"]).all()
    path = np.load(str(tmp_path / (k + "_pose_path.npy")))
    assert path.dtype == np.int32 and path.shape == want["path"][0].shape and (path == want["path"][0]).all()
    c = sr.params(width=mask.shape[1], height=mask.shape[0], n_poses=1, min_dist2=4, n_steps=16, **replay.steer_lattice(0.4, 0.1))
    steer = fr.rollouts(mask, 8, dist2, want["cell_cost"], start, None, c)
    traj = np.load(str(tmp_path / (k + "_steer_traj.npy")))
    assert traj.shape == (steer["best_len"][0], 3) and (traj == steer["best_traj"][0, :steer["best_len"][0]]).all()
    out = capsys.readouterr().out.splitlines()
    logged = [l for l in out if l.startswith("nav-pose ")]
    assert len(logged) == 2 and logged[1].startswith("nav-pose %s: headings=8 status=%d cost=%d path=%d " % (k, want["start_status"][0], want["start_cost"][0],
                                                                                                        len(want["path"][0]))), logged
    assert all("%s=%d" % (nm, want["stats"][nm]) in logged[1] for nm in qr.STATS)
    f.close()


def test_the_pose_plan_in_cpp(pose_lib, fusion, tmp_path):
    """tests/cpp/navpose_smoke.cpp on the GPU: its counts and FNV-1a checksums equal those of the Python calls on the same arrays"""
    import os
    import re
    import subprocess
    from conftest import ROOT
    cpp = os.path.join(ROOT, "tests", "cpp")
    libdir = os.path.dirname(pose_lib.path)
    exe = str(tmp_path / "navpose_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", cpp, os.path.join(cpp, "navpose_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip_pose", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "messages ok=1" in r.stdout, r.stdout
    p = np.arange(70 * 45, dtype=np.uint64)
    h = ((p * 2654435761) & 0xFFFFFFFF) >> 16
    state = np.where(h % 100 < 3, 100, np.where(h % 100 < 5, -1, 0)).astype(np.int8).reshape(45, 70)
    dist2 = np.where(state.ravel() == 0, 1 + (h >> 7) % 40, 0).astype(np.int32).reshape(45, 70)
    poses = np.array([((5 + 11 * k) * 1024 + 300, (4 + 7 * k) * 1024 + 700, 9000 * k) for k in range(6)], np.int32)
    mask = fusion.nav_foot(state, front=2048, back=1024, left=1024, right=1024, pad=0, n_headings=16)["free_mask"]
    kw = dict(n_headings=16, max_path=512, soft_dist2=20, near_penalty=8)
    goals = [(60, 30, -1), (5, 40, 4)]
    got = fusion.nav_pose_plan(mask, dist2, goals, poses, **kw)
    same(got, qr.plan(mask, dist2, goals, poses, **kw), "the smoke program's arrays")
    counts = ("traversable", "reached", "cells", "used", "blocked", "outside", "max")
    sums = ("cost", "cell_cost", "cell_bin", "start_cost", "status", "paths")
    told = re.search("navpose " + " ".join(nm + r"=(\d+)" for nm in counts) + " " + " ".join(nm + "=([0-9a-f]{16})" for nm in sums), r.stdout)
    assert told, r.stdout
    assert tuple(int(v) for v in told.groups()[:7]) == tuple(got["stats"][nm] for nm in qr.STATS)
    flat = np.concatenate(got["path"]) if len(got["path"]) else np.zeros((0, 3), np.int32)
    py_sums = tuple(pr.fnv1a(np.ascontiguousarray(a).tobytes()) for a in (got["cost"], got["cell_cost"], got["cell_bin"], got["start_cost"], got["start_status"], flat))
    assert tuple(int(v, 16) for v in told.groups()[7:]) == py_sums
    assert got["stats"]["goals_used"] >= 1 and (got["start_status"] == 0).any() and len(flat) > 10
    steer = fusion.nav_foot_steer(mask, dist2, poses, 16, cost=got["cell_cost"], n_steps=24)
    told = re.search(r"posesteer ok=(\d+) best=([0-9a-f]{16})", r.stdout)
    assert told and int(told.group(1)) == steer["stats"]["poses_ok"] and int(told.group(2), 16) == pr.fnv1a(steer["best"].tobytes()), r.stdout
