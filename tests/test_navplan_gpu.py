"""ssf_navplan_field (include/ssf_navplan.h) on the MI355X against the restatement (tests/navplan_ref.py): every cell of every
output and every exact stat with == -- grids at the tile edges, doors on tile edges and corners, serpentines inside one tile and
across many rounds (whatever the round batch), a grid 128 tiles wide, unknown cells, states outside {0, -1, 100}, clearance, frontier goals, goal and start
bookkeeping, truncation and the tie-break; plus device arrays, the plan of a carved map without the grid leaving the device, no side
effects on the frame path, the refusals, profiling, replay's files and the C++ surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import navcarve_ref as nc
import navplan_ref as pr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
W, H = 160, 128
CPP = os.path.join(ROOT, "tests", "cpp")
INF = pr.INF
ARRAYS = ("cost", "frontier", "start_cost", "start_status", "path_len")


def handle(lib, **kw):
    """a handle of a test's own, which the test closes when it is done with it"""
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


@pytest.fixture(scope="module")
def nav_lib():
    """libssf_hip_nav.so: the product's objects plus the carve's and the plan's entry points (no fallback: a missing .so is an error)"""
    return binding.load_nav()


@pytest.fixture(scope="module")
def fusion(nav_lib):
    f = handle(nav_lib)
    yield f
    f.close()


def same(got, want, what, outputs=binding.NAVPLAN_OUTPUT_NAMES):
    for name in outputs:
        if name == "path":
            assert len(got["path"]) == len(want["path"]), what
            for i, (a, b) in enumerate(zip(got["path"], want["path"])):
                assert a.dtype == np.int32 and a.shape == b.shape and (a == b).all(), (what, "path", i, a.shape, b.shape)
        else:
            assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name, got[name].shape, got[name].dtype)
            assert (got[name] == want[name]).all(), "%s %s: %d of %d differ" % (what, name, int((got[name] != want[name]).sum()), want[name].size)
    for k in pr.STATS:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"][k], want["stats"][k])


def check(f, what, state, dist2, goals=None, starts=None, **kw):
    """the plan on the device and in the restatement; returns both"""
    want = pr.plan(state, dist2, goals, starts, **kw)
    got = f.nav_plan(state, dist2, goals, starts, **kw)
    assert sorted(got) == sorted(binding.NAVPLAN_OUTPUT_NAMES + ("stats",)), what
    same(got, want, what)
    last = f.debug_navplan_last()
    assert (got["stats"]["rounds"], got["stats"]["tile_visits"]) == (last["rounds"], last["tile_visits"]) and last["rounds"] <= last["tile_visits"]
    return got, want


def some_starts(h, w, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1).astype(np.int32)


# ---- grids at the tile edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 97), (33, 31), (45, 70), (64, 64), (160, 160)])
def test_random_grids_with_penalties(h, w, fusion):
    state, dist2 = pr.random_grid(h, w, 100 + h + w)
    layouts = [[(0, 0)], [(w // 2, h // 2)], [(w - 1, h - 1), (0, h - 1), (w // 2, 0), (min(w - 1, 40), min(h - 1, 33))]]
    for gx, gy in layouts[2] + layouts[1] + layouts[0]:
        state[gy, gx] = 0                                                # the goals stand on free cells: every layout plans something
    starts = some_starts(h, w, 6, h * w)
    for i, goals in enumerate(layouts):
        kw = (dict(), dict(soft_dist2=30, near_penalty=40), dict(soft_dist2=25, near_penalty=1000, min_dist2=0))[i]
        got, want = check(fusion, "%d x %d goals %s" % (h, w, goals), state, dist2, goals, starts, max_path=h * w, **kw)
        assert got["stats"]["goals_used"] == len(goals) and got["stats"]["cells_reached"] >= 1
        assert got["stats"]["rounds"] >= 1 and (h * w < 2000 or got["stats"]["cells_reached"] > h * w // 3)


@pytest.mark.parametrize("h,w", pr.FOREIGN_SIZES)
@pytest.mark.parametrize("allow", [0, 1])
def test_grids_with_states_outside_0_minus_1_100_and_dist2_outside_the_cap(h, w, allow, fusion):
    """tests/navplan_ref.py's foreign grid (states 1, 50, 99, 101, 127, -2, -128; dist2 negative, INT32_MIN, above the cap, INT32_MAX):
    only 0 is free, only -1 is unknown and a frontier's neighbour, a negative dist2 is below min_dist2 = 0 and counts as 0 in the penalty"""
    f = pr.foreign_case(h, w, allow)
    want = f["plan"]
    got = fusion.nav_plan(f["state"], f["dist2"], f["goals"], f["starts"], **f["kw"])
    same(got, want, "foreign %d x %d unknown %d, goals" % (h, w, allow))
    assert got["stats"]["cells_reached"] > h * w // 3 and max(got["path_len"]) > 10
    got = fusion.nav_plan(f["state"], f["dist2"], None, f["starts"], goals_from_frontier=1, min_dist2=2, **f["kw"])
    same(got, f["frontier_plan"], "foreign %d x %d unknown %d, frontier" % (h, w, allow))
    assert got["stats"]["frontier_goals"] > 100
    check(fusion, "foreign, no penalty, both", f["state"], f["dist2"], f["goals"], f["starts"], allow_unknown=allow, goals_from_frontier=1, max_path=50)


DOORS = [dict(wall_x=32, door=31), dict(wall_x=32, door=32), dict(wall_x=31, door=31), dict(wall_x=31, door=0), dict(wall_y=32, door=31),
         dict(wall_y=32, door=32), dict(wall_y=31, door=32), dict(wall_y=31, door=63), dict(wall_x=33, door=17)]


@pytest.mark.parametrize("door", DOORS, ids=["-".join("%s%d" % kv for kv in sorted(d.items())) for d in DOORS])
def test_a_door_on_a_tile_edge_or_corner(door, fusion):
    """one free cell in a wall: every way through ends with two axial moves, because a diagonal into or out of the door cuts the
    wall's corner.  With a second free cell beside the door the diagonal across the tile corner is open"""
    state, dist2 = pr.wall_with_door(64, 64, **door)
    starts = [(0, 0), (63, 63), (31, 31), (32, 32), (0, 63), (63, 0)]
    got, want = check(fusion, "door %s" % door, state, dist2, [(2, 60)], starts, max_path=400)
    on_wall = [state[y, x] == 100 for x, y in starts]
    assert got["stats"]["cells_reached"] == 64 * 64 - 63 and got["start_status"].tolist() == [2 if w else 0 for w in on_wall] and sum(on_wall) <= 2
    wide = state.copy()
    if "wall_x" in door:
        wide[min(door["door"] + 1, 63), door["wall_x"]] = 0
        wide[max(door["door"] - 1, 0), door["wall_x"]] = 0
    else:
        wide[door["wall_y"], min(door["door"] + 1, 63)] = 0
        wide[door["wall_y"], max(door["door"] - 1, 0)] = 0
    got2, _ = check(fusion, "wide door %s" % door, wide, dist2, [(2, 60)], starts, max_path=400)
    assert (got2["cost"] <= got["cost"]).all() and (got2["cost"] < got["cost"]).any()


def test_a_diagonal_across_a_tile_corner(fusion):
    state, dist2 = pr.open_grid(64, 64)
    got, _ = check(fusion, "open 64 x 64", state, dist2, [(63, 63)], [(0, 0), (0, 63)], max_path=200)
    assert got["path"][0].tolist() == [[i, i] for i in range(64)] and got["start_cost"].tolist() == [63 * 14, 630]
    state[31, 32] = 100                                                  # beside the corner: (31, 31) -> (32, 32) would cut it
    got, _ = check(fusion, "a block at the tile corner", state, dist2, [(63, 63)], [(0, 0)], max_path=200)
    cells = got["path"][0].tolist()
    assert got["start_cost"][0] == 62 * 14 + 20 and not ([31, 31] in cells and [32, 32] in cells) and [32, 31] not in cells


# ---- many sweeps, many rounds ------------------------------------------------------------------------------------------------
def test_a_serpentine_inside_one_tile(fusion):
    state, dist2 = pr.serpentine(32)
    got, want = check(fusion, "serpentine 32", state, dist2, [(0, 0)], [(31, 30), (0, 30)], max_path=1024)
    assert got["stats"]["rounds"] == 1 and got["stats"]["tile_visits"] == 1 and got["stats"]["max_cost"] > 32 * 16 * 10 - 400
    assert got["stats"]["cells_reached"] == got["stats"]["cells_traversable"] == 16 * 32 + 16


@pytest.fixture(scope="module")
def serpentine160():
    state, dist2 = pr.serpentine(160)
    starts = [(159, 158), (0, 158), (80, 80), (3, 1)]
    return state, dist2, starts, pr.plan(state, dist2, [(0, 0)], starts, max_path=1 << 15)


@pytest.mark.parametrize("batch", [1, 3, 16, 0])
def test_the_serpentine_of_many_rounds_whatever_the_round_batch(batch, fusion, serpentine160):
    state, dist2, starts, want = serpentine160
    fusion.debug_navplan_set_round_batch(batch)
    try:
        got = fusion.nav_plan(state, dist2, [(0, 0)], starts, max_path=1 << 15)
    finally:
        fusion.debug_navplan_set_round_batch(0)
    same(got, want, "serpentine 160, batch %d" % batch)
    assert got["stats"]["rounds"] > 16 and got["stats"]["tile_visits"] >= got["stats"]["rounds"], got["stats"]
    assert want["stats"]["cells_reached"] == 80 * 160 + 80 and want["stats"]["max_cost"] > 80 * 159 * 10 and want["path_len"][0] > 12000


def test_a_grid_128_tiles_wide(fusion):
    state, dist2 = pr.random_grid(2, 4096, 9, obstacles=0.0)
    state[0, 100::200] = 100                                             # one row blocked here and there: the way weaves
    state[1, 200::200] = 100
    dist2[:] = np.arange(2 * 4096).reshape(2, 4096) % 23
    got, _ = check(fusion, "4096 x 2", state, dist2, [(4095, 0)], [(0, 1), (2048, 0)], soft_dist2=20, near_penalty=7, max_path=5000)
    assert got["stats"]["cells_reached"] == 2 * 4096 - 40 and got["path_len"][0] >= 4096 and got["stats"]["rounds"] >= 128


# ---- who may go where ----------------------------------------------------------------------------------------------------
def test_unknown_cells_and_the_clearance_that_cuts_the_only_door(fusion):
    state, dist2 = pr.wall_with_door(40, 70, wall_x=32, door=20)
    state[:, 40:44] = -1                                                 # a band of unknown cells behind the wall
    dist2[20, 32] = 3                                                    # the door is narrow
    starts = [(0, 0), (69, 39), (41, 5)]
    off, _ = check(fusion, "unknown blocks", state, dist2, [(2, 2)], starts, max_path=300)
    on, _ = check(fusion, "unknown allowed", state, dist2, [(2, 2)], starts, allow_unknown=1, max_path=300)
    assert off["start_status"].tolist() == [0, 3, 2] and on["start_status"].tolist() == [0, 0, 0]
    assert off["stats"]["frontier_cells"] == 2 * 40 and on["stats"]["cells_traversable"] == off["stats"]["cells_traversable"] + 4 * 40
    fits, _ = check(fusion, "the robot fits the door", state, dist2, [(2, 2)], starts, allow_unknown=1, min_dist2=3, max_path=300)
    cut, _ = check(fusion, "the robot does not fit", state, dist2, [(2, 2)], starts, allow_unknown=1, min_dist2=4, max_path=300)
    assert fits["start_status"].tolist() == [0, 0, 0] and cut["start_status"].tolist() == [0, 3, 3]
    assert cut["stats"]["cells_reached"] == 32 * 40 and (cut["cost"][:, 32:] == INF).all()


def test_frontier_goals(fusion):
    state, dist2 = pr.random_grid(45, 70, 21, obstacles=0.2, unknown=0.2)
    starts = some_starts(45, 70, 8, 5)
    alone, want = check(fusion, "frontier alone", state, dist2, None, starts, goals_from_frontier=1, max_path=300)
    s = alone["stats"]
    assert s["frontier_goals"] == s["frontier_cells"] > 100 and s["goals_used"] == 0 and (alone["cost"][alone["frontier"] == 1] == 0).all()
    both, _ = check(fusion, "frontier and goals", state, dist2, [(0, 0), (69, 44), (200, 3)], starts, goals_from_frontier=1, min_dist2=9,
                    soft_dist2=36, near_penalty=15, max_path=300)
    assert 0 < both["stats"]["frontier_goals"] < both["stats"]["frontier_cells"] and both["stats"]["goals_outside"] == 1
    only = fusion.nav_plan(state, dist2, outputs=("frontier",), goals_from_frontier=1)         # the frontier alone is a valid request
    assert sorted(only) == ["frontier", "stats"] and (only["frontier"] == want["frontier"]).all() and only["frontier"].dtype == np.uint8
    none, _ = check(fusion, "no unknown cell, no frontier", *pr.open_grid(5, 5), goals=None, starts=[(1, 1)], goals_from_frontier=1)
    assert none["stats"]["frontier_cells"] == 0 and none["start_status"].tolist() == [3] and none["stats"]["rounds"] == 0


def test_goals_outside_blocked_and_twice(fusion):
    state, dist2 = pr.random_grid(33, 31, 2)
    state[4, 4] = state[30, 20] = 0
    state[10, 10] = 100
    goals = [(4, 4), (4, 4), (31, 0), (0, 33), (-1, 5), (5, -1), (10, 10), (20, 30), (1 << 30, 1 << 30), (-(1 << 31), 0)]
    got, _ = check(fusion, "goal bookkeeping", state, dist2, goals, some_starts(33, 31, 4, 1), max_path=100)
    s = got["stats"]
    assert (s["goals_used"], s["goals_blocked"], s["goals_outside"]) == (3, 1, 6) and got["cost"][4, 4] == 0 and got["cost"][30, 20] == 0


def test_no_reachable_goal(fusion):
    state, dist2 = pr.random_grid(45, 70, 4)
    state[20, 20] = 100
    starts = some_starts(45, 70, 5, 2)
    starts = starts[state[starts[:, 1], starts[:, 0]] == 0]
    got, _ = check(fusion, "every goal refused", state, dist2, [(20, 20), (70, 0)], starts, max_path=50)
    assert (got["cost"] == INF).all() and (got["start_status"] == 3).all() and (got["start_cost"] == INF).all() and (got["path_len"] == 0).all()
    assert (got["stats"]["rounds"], got["stats"]["tile_visits"], got["stats"]["cells_reached"], got["stats"]["max_cost"]) == (0, 0, 0, 0)
    state, dist2 = pr.open_grid(45, 70)
    state[9:12, 39:42] = 100
    state[10, 40] = 0                                                    # the goal is walled in
    got, _ = check(fusion, "a goal walled in", state, dist2, [(40, 10)], [(0, 0), (40, 10), (40, 9)], max_path=50)
    assert got["start_status"].tolist() == [3, 0, 2] and got["stats"]["cells_reached"] == 1 and got["path"][1].tolist() == [[40, 10]]
    assert got["stats"]["rounds"] == 1 and got["stats"]["tile_visits"] == 1       # no round of work after the first


# ---- starts ----------------------------------------------------------------------------------------------------------------
def test_one_start_of_each_status_and_truncation(fusion):
    state, dist2 = pr.open_grid(40, 70)
    state[:, 50] = 100                                                   # nothing behind column 50 reaches the goal
    starts = [(10, 10), (70, 3), (3, -1), (50, 7), (60, 7), (0, 39), (5, 5)]
    got, _ = check(fusion, "statuses", state, dist2, [(5, 5)], starts, max_path=30)
    assert got["start_status"].tolist() == [0, 1, 1, 2, 3, 4, 0] and got["path_len"].tolist() == [6, 0, 0, 0, 0, 30, 1]
    exact, _ = check(fusion, "a path of exactly max_path cells", state, dist2, [(5, 5)], [(0, 39)], max_path=35)
    one_less, _ = check(fusion, "one cell too long", state, dist2, [(5, 5)], [(0, 39)], max_path=34)
    assert (exact["start_status"][0], exact["path_len"][0], one_less["start_status"][0], one_less["path_len"][0]) == (0, 35, 4, 34)
    assert (one_less["path"][0] == exact["path"][0][:34]).all()
    no_path, _ = check(fusion, "max_path 0", state, dist2, [(5, 5)], starts)
    assert no_path["start_status"].tolist() == [0, 1, 1, 2, 3, 0, 0] and not no_path["path_len"].any()
    # entries past path_len are not written
    p, keep = fusion._navplan_params(False, 70, 40, [(5, 5)], starts, dict(max_path=30))
    path = np.full((len(starts), 30, 2), -7, np.int32)
    lens = np.zeros(len(starts), np.int32)
    st8, d2 = np.ascontiguousarray(state), np.ascontiguousarray(dist2)
    fusion._navplan_field(p, st8.ctypes.data_as(binding.C.c_void_p), d2.ctypes.data_as(binding.C.c_void_p),
                          dict(path=path.ctypes.data_as(binding.C.c_void_p), path_len=lens.ctypes.data_as(binding.C.c_void_p)))
    assert lens.tolist() == [6, 0, 0, 0, 0, 30, 1]
    for i, n in enumerate(lens):
        assert (path[i, :n] == got["path"][i]).all() and (path[i, n:] == -7).all()


def test_the_tie_break_against_the_hand_written_path(fusion):
    got, _ = check(fusion, "open 8 x 8", *pr.open_grid(8, 8), goals=[(5, 2)], starts=[(0, 0), (7, 7)], max_path=64)
    assert got["path"][0].tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [4, 1], [5, 2]] and got["start_cost"].tolist() == [58, 2 * 14 + 3 * 10]
    assert got["path"][1].tolist() == [[7, 7], [7, 6], [7, 5], [7, 4], [6, 3], [5, 2]]      # k = 3 (0, -1) before k = 6 (-1, -1)


# ---- device arrays, the carved map ------------------------------------------------------------------------------------------
def test_device_tensors_give_the_same_bits(fusion):
    import torch
    state, dist2 = pr.random_grid(70, 97, 8, unknown=0.1)
    goals, starts = [(3, 3), (90, 60)], some_starts(70, 97, 7, 3)
    kw = dict(soft_dist2=30, near_penalty=40, min_dist2=1, goals_from_frontier=1, max_path=150)
    host, want = check(fusion, "host arrays", state, dist2, goals, starts, **kw)
    dev = torch.device("cuda")
    n = len(starts)
    t = dict(cost=torch.zeros((70, 97), dtype=torch.int32, device=dev), frontier=torch.zeros((70, 97), dtype=torch.uint8, device=dev),
             start_cost=torch.zeros(n, dtype=torch.int32, device=dev), start_status=torch.zeros(n, dtype=torch.int32, device=dev),
             path_len=torch.zeros(n, dtype=torch.int32, device=dev), path=torch.full((n, 150, 2), -7, dtype=torch.int32, device=dev))
    stats = fusion.nav_plan_device(torch.from_numpy(state).to(dev), torch.from_numpy(dist2).to(dev), 97, 70, goals, starts, **dict(t, **kw))
    got = {k: v.cpu().numpy() for k, v in t.items()}
    for k in ARRAYS:
        a = got[k].view(np.uint32) if k in ("cost", "start_cost") else got[k]
        assert (a == host[k]).all(), k
    for i, ln in enumerate(got["path_len"]):
        assert (got["path"][i, :ln] == host["path"][i]).all() and (got["path"][i, ln:] == -7).all()
    assert {k: stats[k] for k in pr.STATS} == {k: host["stats"][k] for k in pr.STATS}
    # addresses instead of tensors, and fewer outputs
    t2, s_dev, d_dev = torch.zeros((70, 97), dtype=torch.int32, device=dev), torch.from_numpy(state).to(dev), torch.from_numpy(dist2).to(dev)
    fusion.nav_plan_device(s_dev.data_ptr(), d_dev, 97, 70, goals, cost=t2.data_ptr(), **kw)       # (the tensors outlive the call)
    assert (t2.cpu().numpy().view(np.uint32) == host["cost"]).all()


# ---- the staging of a host grid -----------------------------------------------------------------------------------------------
FILL = util.GUARD_WORD
_STAGING = {}


def staging_case(h, w):
    """dict(state, dist2, goals, starts, kw, want): a random grid with unknown cells, goals in two corners, five
    starts; the restatement's answer, computed once and shared"""
    if (h, w) not in _STAGING:
        state, dist2 = pr.random_grid(h, w, 900 + h + w, obstacles=0.15, unknown=0.1)
        state[0, 0] = state[h - 1, w - 1] = 0
        goals, starts = [(0, 0), (w - 1, h - 1)], some_starts(h, w, 5, 7 * h + w)
        kw = dict(soft_dist2=30, near_penalty=40, max_path=h * w)
        _STAGING[h, w] = dict(state=state, dist2=dist2, goals=goals, starts=starts, kw=kw, want=pr.plan(state, dist2, goals, starts, **kw))
    return _STAGING[h, w]


def plan_host(f, c, names):
    """ssf_navplan_field with host arrays, the outputs `names` alone, each between guard bytes and filled with them: (name -> array, stats)"""
    (h, w), n, mp = c["state"].shape, len(c["starts"]), c["kw"]["max_path"]
    shapes = dict(cost=((h, w), np.uint32), frontier=((h, w), np.uint8), start_cost=((n,), np.uint32), start_status=((n,), np.int32),
                  path_len=((n,), np.int32), path=((n, mp, 2), np.int32))
    out = {nm: util.guarded(*shapes[nm]) for nm in names}
    p, keep = f._navplan_params(False, w, h, c["goals"], c["starts"], c["kw"])
    stats = f._navplan_field(p, binding._ptr(c["state"]), binding._ptr(c["dist2"]), {nm: binding._ptr(a) for nm, (a, _) in out.items()})
    assert all(intact() for _, intact in out.values()), names
    return {nm: a for nm, (a, _) in out.items()}, stats


def plan_same(got, want, what):
    """every array of got equals the restatement's; a path up to its length, and past it it holds the fill"""
    for nm, a in got.items():
        if nm != "path":
            assert a.dtype == want[nm].dtype and (a == want[nm]).all(), (what, nm)
            continue
        for i, cells in enumerate(want["path"]):
            assert (a[i, :len(cells)] == cells).all() and (a[i, len(cells):] == FILL).all(), (what, nm, i)


@pytest.mark.parametrize("h,w", [(19, 37), (1, 1)])
def test_a_host_grid_whose_arrays_start_at_rounded_offsets(h, w, fusion):
    """703 cells and one cell: neither P nor 4 P is a multiple of 256, so dist2 sits at a rounded offset of the staging buffer.  Host
    arrays, device pointers and the restatement agree"""
    import torch
    c = staging_case(h, w)
    host, hs = plan_host(fusion, c, binding.NAVPLAN_OUTPUT_NAMES)
    plan_same(host, c["want"], "host %d x %d" % (h, w))
    t = {nm: torch.full(a.shape, util.GUARD_FILL, dtype=torch.uint8, device="cuda") if a.dtype == np.uint8 else torch.full(a.shape, FILL, dtype=torch.int32, device="cuda")
         for nm, a in host.items()}
    ds = fusion.nav_plan_device(torch.from_numpy(c["state"]).to("cuda"), torch.from_numpy(c["dist2"]).to("cuda"), w, h, c["goals"], c["starts"], **dict(t, **c["kw"]))
    assert all(host[nm].tobytes() == t[nm].cpu().numpy().tobytes() for nm in host)
    assert {k: hs[k] for k in pr.STATS} == {k: ds[k] for k in pr.STATS} == {k: c["want"]["stats"][k] for k in pr.STATS}
    assert h == 1 or (c["want"]["stats"]["cells_reached"] > 100 and c["want"]["stats"]["frontier_cells"] > 0 and (c["want"]["path_len"] > 10).any())


@pytest.mark.parametrize("name", binding.NAVPLAN_OUTPUT_NAMES)
def test_one_host_output_alone_between_guard_bytes(name, fusion):
    """19 x 37, host arrays: every output on its own, all others NULL, equals the same array of the call that asks for all six, and
    the 256 bytes on either side of the caller's array are untouched"""
    c = staging_case(19, 37)
    if "every" not in c:
        c["every"] = plan_host(fusion, c, binding.NAVPLAN_OUTPUT_NAMES)
    every, stats = c["every"]
    plan_same(every, c["want"], "every output")
    alone, st = plan_host(fusion, c, (name,))
    assert alone[name].tobytes() == every[name].tobytes() and {k: st[k] for k in pr.STATS} == {k: stats[k] for k in pr.STATS}, name


def test_the_staging_buffer_grows_and_is_used_again(nav_lib):
    """one handle: 8 x 8, 19 x 37, 8 x 8 again.  Each call gives what a handle that has made no other call gives"""
    f = handle(nav_lib)
    for h, w in ((8, 8), (19, 37), (8, 8)):
        c = staging_case(h, w)
        fresh = handle(nav_lib)
        (got, gs), (want, ws) = plan_host(f, c, binding.NAVPLAN_OUTPUT_NAMES), plan_host(fresh, c, binding.NAVPLAN_OUTPUT_NAMES)
        fresh.close()
        assert all(got[nm].tobytes() == want[nm].tobytes() for nm in got) and {k: gs[k] for k in pr.STATS} == {k: ws[k] for k in pr.STATS}, (h, w)
        plan_same(got, c["want"], (h, w))
    f.close()


def test_plan_from_the_carved_map_without_the_grid_leaving_the_device(fusion):
    f = fusion
    m, n, pose, gkw, views, ckw = nc.wall_scene()
    f.set_model(m, n, 100)
    grid = dict(pose=pose, **gkw)
    base = f.nav_grid_carve(views, outputs=("state", "dist2"), carve=ckw, **grid)
    free = np.argwhere(base["state"] == 0)
    assert len(free) > 100
    goals = [tuple(free[0][::-1])]
    starts = [tuple(free[-1][::-1]), tuple(free[len(free) // 2][::-1]), (0, 0)]
    for plan in (dict(max_path=120), dict(goals_from_frontier=1, min_dist2=1, soft_dist2=9, near_penalty=30, max_path=120)):
        want, _ = check(f, "the carved wall scene %s" % sorted(plan), base["state"], base["dist2"], goals, starts, **plan)
        got = f.nav_plan_from_map(views, goals, starts, grid=grid, carve=ckw, plan=plan)
        same(got, want, "nav_plan_from_map")
        assert got["grid_stats"]["cells_carved"] > 0 and got["grid_stats"]["cells_free"] == int((base["state"] == 0).sum())
    assert want["stats"]["frontier_goals"] > 0 and want["stats"]["cells_reached"] > 100


# ---- no side effects, refusals, profiling -------------------------------------------------------------------------------------
def test_a_plan_changes_no_later_result(nav_lib):
    A, B = handle(nav_lib), handle(nav_lib)
    state, dist2 = pr.random_grid(45, 70, 6, unknown=0.1)
    for k in (0, 3, 6):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        A.nav_plan(state, dist2, [(3, 3)], [(60, 40)], goals_from_frontier=1, max_path=100)
        grid = A.nav_grid(outputs=("state", "dist2"), width=96, height=80)
        A.nav_plan(grid["state"], grid["dist2"], starts=[(48, 40)], goals_from_frontier=1, allow_unknown=1, max_path=200)
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)
    B.close()
    A.close()


def test_the_refusals(nav_lib):
    f = handle(nav_lib)
    state, dist2 = pr.open_grid(6, 9)
    refused = pytest.raises(binding.SsfError, match=r"ssf_navplan_field failed \(-1\)")
    for kw in (dict(min_dist2=-1), dict(soft_dist2=-1), dict(soft_dist2=1024 * 1024 + 1), dict(near_penalty=-1), dict(near_penalty=1001),
               dict(max_path=-1), dict(max_path=(1 << 20) + 1)):
        with refused:
            f.nav_plan(state, dist2, [(1, 1)], [(2, 2)], **kw)
    with refused:
        f.nav_plan(state, dist2, None, [(2, 2)])                        # no goals and no frontier goals
    with refused:
        f.nav_plan(state, dist2, [(1, 1)], outputs=())                  # every output NULL
    with refused:
        f.nav_plan(state, dist2, np.zeros((65537, 2), np.int32))
    with refused:
        f.nav_plan(state, dist2, [(1, 1)], np.zeros((4097, 2), np.int32))
    with refused:
        f.nav_plan(np.zeros((0, 5), np.int8), np.zeros((0, 5), np.int32), [(1, 1)])
    with refused:
        f.nav_plan(np.zeros((1, 4097), np.int8), np.zeros((1, 4097), np.int32), [(1, 1)])
    big = np.zeros((4096, 4096), np.int8), np.full((4096, 4096), 9, np.int32)
    with refused:                                                      # (14 + 242) * 2^24 = 2^32 >= 2^32 - 1: a cost could wrap
        f.nav_plan(big[0], big[1], [(1, 1)], outputs=("start_cost",), soft_dist2=4, near_penalty=242)
    L, byref, vp = nav_lib.lib, binding.C.byref, binding.C.c_void_p
    p, st, out = binding.SsfNavPlanParams(), binding.SsfNavPlanStats(), binding.SsfNavPlanOut()
    assert L.ssf_navplan_default_params(f.h, byref(p)) == 0
    assert L.ssf_navplan_default_params(None, byref(p)) == -1 and L.ssf_navplan_default_params(f.h, None) == -1
    d = f.nav_plan_default_params()
    assert d == dict(width=512, height=512, min_dist2=0, soft_dist2=0, near_penalty=0, allow_unknown=0, n_goals=0, goals_from_frontier=0,
                     n_starts=0, max_path=0, on_device=0)
    s8, d2 = np.ascontiguousarray(state), np.ascontiguousarray(dist2)
    cost = np.zeros((6, 9), np.uint32)
    goals = np.array([[1, 1]], np.int32)
    p.width, p.height, p.goals, p.n_goals = 9, 6, goals.ctypes.data, 1
    out.cost = cost.ctypes.data
    a, b = s8.ctypes.data_as(vp), d2.ctypes.data_as(vp)
    assert L.ssf_navplan_field(f.h, byref(p), a, b, byref(out), None) == 0 and cost[1, 1] == 0 and cost[5, 8] == 4 * 14 + 3 * 10      # stats are optional
    assert L.ssf_navplan_field(None, byref(p), a, b, byref(out), byref(st)) == -1
    assert L.ssf_navplan_field(f.h, None, a, b, byref(out), byref(st)) == -1
    assert L.ssf_navplan_field(f.h, byref(p), None, b, byref(out), byref(st)) == -1
    assert L.ssf_navplan_field(f.h, byref(p), a, None, byref(out), byref(st)) == -1
    assert L.ssf_navplan_field(f.h, byref(p), a, b, None, byref(st)) == -1
    assert L.ssf_navplan_field(f.h, byref(p), a, b, byref(binding.SsfNavPlanOut()), byref(st)) == -1
    for field, bad in (("n_goals", -1), ("n_starts", -1), ("n_starts", 1), ("width", 0), ("height", -3), ("width", 4097)):
        keep = getattr(p, field)
        setattr(p, field, bad)                                           # a negative count; a NULL list with a positive count; the size
        assert L.ssf_navplan_field(f.h, byref(p), a, b, byref(out), byref(st)) == -1, (field, bad)
        setattr(p, field, keep)
    p.goals = None                                                     # goals NULL with n_goals > 0
    assert L.ssf_navplan_field(f.h, byref(p), a, b, byref(out), byref(st)) == -1
    assert L.ssf_debug_navplan_set_round_batch(f.h, -1) == -1 and L.ssf_debug_navplan_set_round_batch(f.h, 1025) == -1
    assert L.ssf_debug_navplan_set_round_batch(None, 1) == -1 and L.ssf_debug_navplan_last(None, None, None) == -1
    # the largest grid that is not refused for its size plans (the bound is sharp: 255 * 2^24 < 2^32 - 1)
    got = f.nav_plan(big[0], big[1], [(4095, 4095)], [(4090, 4090)], outputs=("start_cost", "start_status"), soft_dist2=10, near_penalty=241)
    assert got["start_cost"].tolist() == [5 * (14 + 24)] and got["stats"]["cells_reached"] == 4096 * 4096
    # the handle keeps working: a plan and a frame after the refusals
    check(f, "after the refusals", *pr.random_grid(33, 31, 1), goals=[(1, 1), (30, 30)], starts=[(5, 5)], max_path=80)
    f.process_frame(*util.frame(0, W, H))
    check(f, "after a frame", *pr.random_grid(33, 31, 2), goals=[(1, 1), (30, 30)], starts=[(5, 5)], max_path=80)
    g = handle(nav_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_plan(state, dist2, [(1, 1)])
    q = handle(nav_lib, pipeline_depth=2, extract_batch=2)
    q.submit_frame(*util.frame(0, W, H))
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q.nav_plan(state, dist2, [(1, 1)])
    q.process_submitted()
    check(q, "pipelined, at rest", state, dist2, [(1, 1)], [(8, 5)], max_path=20)
    q.close()
    g.close()
    f.close()


def test_the_kernels_are_timed_under_profile(nav_lib):
    f = handle(nav_lib, profile=1)
    f.reset_kernel_times()
    state, dist2 = pr.serpentine(70)
    got, _ = check(f, "profiled", state, dist2, [(0, 0), (3, 0)], [(69, 68)], max_path=4000)
    names = f.kernel_times()
    for k in ("navplan_init", "navplan_goals", "navplan_relax", "navplan_stats", "navplan_trace"):
        assert k in names and names[k][1] > 0, (k, names)
    assert names["navplan_relax"][1] >= got["stats"]["rounds"] > 3
    f.close()


# ---- replay.py's files -----------------------------------------------------------------------------------------------------
def test_replay_writes_the_plan_next_to_the_grid(nav_lib, tmp_path):
    import json
    from supersurfel_fusion_amd import replay
    f = handle(nav_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    plan = dict(goals=[(12.0, 12.5), (-3.0, 1.0)], frontier=True, radius=0.12)
    _, results = replay.replay(f, frames, nav_grid_dir=str(tmp_path), nav_grid_every=2, nav_grid_res=0.1, nav_grid_carve=True, nav_grid_carve_stride=4,
                               nav_plan=plan)
    per_grid = [".pgm", ".yaml", "_cost.npy", "_dist2.npy", "_path.npy", "_plan.json", "_seen.npy"]
    assert sorted(os.listdir(str(tmp_path))) == sorted("%06d%s" % (k, s) for k in (0, 2) for s in per_grid)
    grid = f.nav_grid_carve([r["pose"] for r in results], outputs=("state", "dist2"), carve=dict(stride=4), res=0.1)
    start, goals = replay.plan_cells(grid["stats"]["pose"], 0.1, f.get_pose()[9:12], plan["goals"])
    assert np.abs(start - 256).max() <= 1 and goals.tolist() == [[120, 125], [-30, 10]]      # the default grid is centred on the camera
    want = pr.plan(grid["state"], grid["dist2"], goals, start, goals_from_frontier=1, min_dist2=4, max_path=4 * 1024)
    assert (np.load(str(tmp_path / "000002_cost.npy")) == want["cost"]).all() and (np.load(str(tmp_path / "000002_path.npy")) == want["path"][0]).all()
    told = json.load(open(str(tmp_path / "000002_plan.json")))
    assert {k: told[k] for k in pr.STATS} == want["stats"] and told["goals_outside"] == 1 and told["frontier_goals"] > 0
    assert (told["start"], told["start_status"], told["start_cost"], told["min_dist2"]) == (start[0].tolist(), int(want["start_status"][0]),
                                                                                         int(want["start_cost"][0]), 4)
    with pytest.raises(ValueError, match="nav_plan needs nav_grid_dir"):
        replay.replay(f, [], nav_plan=plan)
    f.close()


# ---- the C++ surface -----------------------------------------------------------------------------------------------------
def test_plan_on_a_grid_in_cpp(nav_lib, fusion, tmp_path):
    """tests/cpp/navplan_smoke.cpp on the GPU: its counts and FNV-1a checksums equal those of the Python call on the same arrays"""
    libdir = os.path.dirname(nav_lib.path)
    exe = str(tmp_path / "navplan_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "navplan_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip_nav", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    names = ("trav", "reached", "frontier", "fgoals", "used", "blocked", "outside", "max", "cells")
    got = re.search(r"navplan 70x45 " + " ".join(nm + r"=(\d+)" for nm in names) +
                    r" cost=([0-9a-f]{16}) frontier=([0-9a-f]{16}) status=([0-9a-f]{16}) paths=([0-9a-f]{16})", r.stdout)
    assert got and re.search(r"path start=\d+ poses=\d+ ok=1", r.stdout), r.stdout
    state, dist2 = pr.hashed_grid()
    goals, starts = [(3, 3), (66, 40), (70, 2), (35, 22)], [(0, 0), (69, 44), (20, 30), (-1, 4), (50, 10)]
    want, _ = check(fusion, "python plan", state, dist2, goals, starts, min_dist2=2, soft_dist2=30, near_penalty=25, goals_from_frontier=1, max_path=64)
    s = want["stats"]
    assert s["cells_reached"] > 500 and s["frontier_goals"] > 0 and sum(want["path_len"]) > 0, s
    counts = (s["cells_traversable"], s["cells_reached"], s["frontier_cells"], s["frontier_goals"], s["goals_used"], s["goals_blocked"],
              s["goals_outside"], s["max_cost"], int(sum(want["path_len"])))
    assert tuple(int(v) for v in got.groups()[:9]) == counts, (got.groups(), counts)
    hp = 1469598103934665603
    for path in want["path"]:
        hp = pr.fnv1a(np.ascontiguousarray(path).tobytes(), hp)
    sums = (pr.fnv1a(want["cost"].tobytes()), pr.fnv1a(want["frontier"].tobytes()), pr.fnv1a(want["start_status"].tobytes()), hp)
    assert tuple(int(v, 16) for v in got.groups()[9:]) == sums, (got.groups(), sums)
