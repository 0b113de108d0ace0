"""ssf_navfrontier_regions (include/ssf_navfrontier.h) on the MI355X against the restatement (tests/navfrontier_ref.py): the map, every
record of the table, the order and every exact stat with == -- grids at the tile edges, pairs of members across tile edges and
corners under both connectivities, a spiral through every tile, a checkerboard past max_regions, the filters and the
representative's tie-break, the gain at R = 1, 7 and 128 (clipped, shadowed, with shared cells); plus device arrays, nav_explore end
to end, no side effects on the frame path, the refusals, profiling, replay's files and the C++ surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import navfrontier_ref as fr
import navplan_ref as pr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
W, H = 160, 128
CPP = os.path.join(ROOT, "tests", "cpp")
INF = fr.INF


def handle(lib, **kw):
    """a handle of a test's own, which the test closes when it is done with it"""
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


@pytest.fixture(scope="module")
def explore_lib():
    """libssf_hip_explore.so: nav's objects plus the regions' entry points (no fallback: a missing .so is an error)"""
    return binding.load_explore()


@pytest.fixture(scope="module")
def fusion(explore_lib):
    f = handle(explore_lib)
    yield f
    f.close()


def same(got, want, what):
    assert got["region"].dtype == np.int32 and got["region"].shape == want["region"].shape, what
    assert (got["region"] == want["region"]).all(), "%s region: %d of %d differ" % (what, int((got["region"] != want["region"]).sum()), want["region"].size)
    same_table(got, want, what)


def same_table(got, want, what):
    table = fr.as_records(want["regions"], binding.NAVFRONTIER_REGION_DTYPE)
    assert got["regions"].dtype == table.dtype and got["regions"].shape == table.shape, (what, got["regions"].shape, table.shape)
    for nm in fr.FIELDS:
        assert (got["regions"][nm] == table[nm]).all(), (what, nm, got["regions"][nm][:8], table[nm][:8])
    assert got["order"].dtype == np.int32 and got["order"].shape == want["order"].shape and (got["order"] == want["order"]).all(), what
    for k in fr.STATS:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"][k], want["stats"][k])


def check(f, what, state, dist2=None, cost=None, **kw):
    """the regions on the device and in the restatement; returns both"""
    want = fr.frontiers(state, dist2, cost, **kw)
    got = f.nav_frontiers(state, dist2, cost, **kw)
    assert sorted(got) == ["order", "region", "regions", "stats"], what
    same(got, want, what)
    return got, want


# ---- grids at the tile edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 70), (70, 1), (33, 33), (45, 70)])
def test_random_grids(h, w, fusion):
    state, dist2 = fr.random_grid(h, w, 100 + h + w)
    cost = fr.random_cost(h, w, 7 + h)
    if h * w == 1:
        for s in (0, -1, 100):
            got, _ = check(fusion, "1 x 1 state %d" % s, np.full((1, 1), s, np.int8), dist2, cost)
            assert got["stats"]["frontier_cells"] == 0 and got["region"].tolist() == [[-1]] and len(got["regions"]) == 0
        return
    for conn in (8, 4):
        plain, want = check(fusion, "%d x %d connectivity %d" % (h, w, conn), state, dist2, cost, connectivity=conn)
        assert want["stats"]["regions_found"] >= 2 and want["stats"]["frontier_cells"] >= 4
        got, want = check(fusion, "%d x %d connectivity %d filtered" % (h, w, conn), state, dist2, cost, connectivity=conn, min_cells=2, reachable_only=1,
                          gain_radius=3, gain_weight=5, size_weight=2)
        if min(h, w) > 1:                                                # a case whose reference has nothing to label or to drop shows nothing
            assert want["stats"]["regions_kept"] >= 2 and want["stats"]["regions_small"] + want["stats"]["regions_unreached"] >= 1, want["stats"]
            assert (want["region"] == -2).any() and (want["region"] >= 0).any()
        assert got["stats"]["merge_pairs"] >= 0
    no_cost, _ = check(fusion, "%d x %d without cost and dist2" % (h, w), state)
    assert (no_cost["regions"]["rep_cost"] == INF).all() and no_cost["stats"]["frontier_cells"] == plain["stats"]["frontier_cells"]


@pytest.mark.parametrize("h,w", pr.FOREIGN_SIZES)
@pytest.mark.parametrize("allow", [0, 1])
def test_grids_with_states_outside_0_minus_1_100(h, w, allow, fusion):
    """tests/navplan_ref.py's foreign grid with the field planned on it: a member is a cell of state 0 beside one of state -1 (-2 and
    -128 make none), a negative dist2 is below min_dist2 = 0, a gain ray stops at 100 alone and counts -1 alone"""
    f = pr.foreign_case(h, w, allow)
    state, dist2, cost = f["state"], f["dist2"], f["plan"]["cost"]
    for conn in (8, 4):
        what = "foreign %d x %d unknown %d connectivity %d" % (h, w, allow, conn)
        check(fusion, what, state, dist2, cost, connectivity=conn, gain_radius=2)
        got, want = check(fusion, what + " filtered", state, dist2, cost, connectivity=conn, min_cells=2, reachable_only=1, gain_radius=4, gain_weight=5,
                          size_weight=2, traversable_only=1)
        assert want["stats"]["regions_kept"] >= 5 and want["stats"]["regions_small"] + want["stats"]["regions_unreached"] >= 2
        assert int(got["regions"]["gain"].max()) > 3


def two_members(a, b, size=64):
    """walls everywhere but two free cells a and b, each with an unknown cell on its far side: the only members"""
    state = np.full((size, size), 100, np.int8)
    (ax, ay), (bx, by) = a, b
    s = 1 if bx >= ax else -1
    state[ay, ax] = state[by, bx] = 0
    state[ay, ax - s] = state[by, bx + s] = -1
    return state


PAIRS = [((31, 31), (32, 32)), ((32, 31), (31, 32)), ((31, 30), (32, 31)), ((31, 33), (32, 32)), ((30, 31), (31, 32)), ((33, 31), (32, 32)),
         ((31, 9), (32, 10)), ((31, 10), (32, 9)), ((9, 31), (10, 32)), ((10, 31), (9, 32)), ((31, 0), (32, 1)), ((61, 31), (62, 32))]


@pytest.mark.parametrize("a,b", PAIRS, ids=["%d.%d-%d.%d" % (a + b) for a, b in PAIRS])
def test_two_members_across_a_tile_corner_or_edge(a, b, fusion):
    """diagonal neighbours in different tiles: one region with connectivity 8, two with 4"""
    state = two_members(a, b)
    assert fr.members(state, None, fr.params()).sum() == 2
    eight, _ = check(fusion, "pair %s %s connectivity 8" % (a, b), state)
    four, _ = check(fusion, "pair %s %s connectivity 4" % (a, b), state, connectivity=4)
    pa, pb = a[1] * 64 + a[0], b[1] * 64 + b[0]
    assert eight["regions"]["label"].tolist() == [min(pa, pb)] and eight["regions"]["cells"].tolist() == [2]
    assert eight["region"][a[1], a[0]] == 0 and eight["region"][b[1], b[0]] == 0
    assert four["regions"]["label"].tolist() == sorted([pa, pb]) and four["regions"]["cells"].tolist() == [1, 1]


@pytest.mark.parametrize("a,b", [((31, 5), (32, 5)), ((5, 31), (5, 32)), ((31, 31), (32, 31)), ((32, 31), (32, 32))])
def test_two_axial_members_across_a_tile_edge(a, b, fusion):
    state = np.full((64, 64), 100, np.int8)
    state[a[1], a[0]] = state[b[1], b[0]] = 0
    if a[1] == b[1]:
        state[a[1] - 1, a[0]] = state[b[1] + 1, b[0]] = -1
    else:
        state[a[1], a[0] - 1] = state[b[1], b[0] + 1] = -1
    for conn in (4, 8):
        got, _ = check(fusion, "axial pair %s %s" % (a, b), state, connectivity=conn)
        assert got["regions"]["cells"].tolist() == [2] and got["stats"]["merge_pairs"] >= 1


def test_a_spiral_through_every_tile(fusion):
    state, cells = fr.spiral()
    got, want = check(fusion, "spiral", state)
    assert want["stats"]["regions_found"] == 1 and got["regions"]["label"].tolist() == [0] and got["regions"]["cells"][0] > 3000
    assert (got["regions"]["x0"][0], got["regions"]["y0"][0], got["regions"]["x1"][0], got["regions"]["y1"][0]) == (0, 0, 96, 63)
    check(fusion, "spiral connectivity 4", state, connectivity=4)
    flipped = np.ascontiguousarray(state[::-1, ::-1])                    # the smallest index no longer where the corridor starts
    check(fusion, "spiral flipped", flipped)
    cost = np.full(state.shape, INF, np.uint32)
    far, near = cells[len(cells) // 2], cells[-5]
    cost[far[1], far[0]] = cost[near[1], near[0]] = 77                   # two members of one region, tiles apart, tie on cost
    tie, _ = check(fusion, "spiral with a tie", state, None, cost)
    p = min(far[1] * 97 + far[0], near[1] * 97 + near[0])
    assert (tie["regions"]["rep_x"][0], tie["regions"]["rep_y"][0], tie["regions"]["rep_cost"][0]) == (p % 97, p // 97, 77)


def test_a_checkerboard_past_max_regions(fusion):
    cb = fr.checkerboard()
    one, _ = check(fusion, "checkerboard connectivity 8", cb)
    assert one["stats"]["regions_found"] == 1 and one["regions"]["cells"].tolist() == [2048]
    many, _ = check(fusion, "checkerboard connectivity 4", cb, connectivity=4, max_regions=100)
    s = many["stats"]
    assert (s["regions_found"], s["regions_kept"], s["regions_written"], s["largest_cells"]) == (2048, 2048, 100, 1)
    assert (many["region"] == -2).sum() == 1948 and (many["region"] >= 0).sum() == 100 and len(many["regions"]) == 100 and len(many["order"]) == 100
    assert many["regions"]["label"].tolist() == sorted(many["regions"]["label"].tolist()) and many["regions"]["label"][99] == 2 * 99 + 1 * (99 // 32 % 2)
    # records and entries past regions_written are not written
    p = fusion._navfrontier_params(False, 64, 64, dict(connectivity=8, max_regions=7))
    regions, order = np.zeros(7, binding.NAVFRONTIER_REGION_DTYPE), np.full(7, -7, np.int32)
    regions["label"] = -7
    out = binding.SsfNavFrontierOut(None, regions.ctypes.data, order.ctypes.data)
    st = binding.SsfNavFrontierStats()
    vp = binding.C.c_void_p
    assert explore_call(fusion, p, cb.ctypes.data_as(vp), None, None, out, st) == 0 and st.regions_written == 1
    assert regions["label"].tolist() == [0] + [-7] * 6 and order.tolist() == [0] + [-7] * 6


def explore_call(f, p, state, dist2, cost, out, st):
    return f.L.lib.ssf_navfrontier_regions(f.h, binding.C.byref(p), state, dist2, cost, binding.C.byref(out), binding.C.byref(st) if st is not None else None)


# ---- the filters and the representative --------------------------------------------------------------------------------------
def strips():
    """(state, dist2, cost): a strip of members across a tile border with two members that tie on cost, a strip that nothing
    reaches, and a one-cell region that is reached"""
    state = np.full((40, 70), 100, np.int8)
    dist2 = np.full((40, 70), 9, np.int32)
    cost = np.full((40, 70), INF, np.uint32)
    state[5, 28:37] = 0
    state[4, 28:37] = -1
    cost[5, 30] = cost[5, 34] = 9
    cost[5, 33] = 12
    state[20, 3:6] = 0
    state[21, 3:6] = -1
    state[30, 50] = 0
    state[30, 51] = -1
    cost[30, 50] = 4
    cost[30, 51] = 1                                                     # an unknown cell's cost is nobody's
    dist2[5, 28:31] = 3
    return state, dist2, cost


def test_the_filters_and_the_representatives_tie_break(fusion):
    state, dist2, cost = strips()
    got, _ = check(fusion, "strips", state, dist2, cost)
    assert got["regions"]["cells"].tolist() == [9, 3, 1] and got["regions"]["rep_cost"].tolist() == [9, INF, 4]
    assert (got["regions"]["rep_x"].tolist(), got["regions"]["rep_y"].tolist()) == ([30, 3, 50], [5, 20, 30])       # the tie: the smaller p; nothing reached: the label
    assert got["order"].tolist() == [2, 0, 1]
    kept, _ = check(fusion, "strips reachable", state, dist2, cost, reachable_only=1)
    assert kept["regions"]["label"].tolist() == [5 * 70 + 28, 30 * 70 + 50] and kept["stats"]["regions_unreached"] == 1 and (kept["region"][20, 3:6] == -2).all()
    big, _ = check(fusion, "strips min_cells 2", state, dist2, cost, min_cells=2, reachable_only=1)
    assert big["regions"]["cells"].tolist() == [9] and (big["stats"]["regions_small"], big["stats"]["regions_unreached"]) == (1, 1)
    three, _ = check(fusion, "strips min_cells 3 without cost", state, dist2, None, min_cells=3)
    assert three["regions"]["cells"].tolist() == [9, 3] and (three["regions"]["rep_cost"] == INF).all()
    none, _ = check(fusion, "strips min_cells 10", state, dist2, cost, min_cells=10)
    assert len(none["regions"]) == 0 and len(none["order"]) == 0 and none["stats"]["regions_small"] == 3 and (none["region"] > -1).sum() == 0
    trav, _ = check(fusion, "strips traversable", state, dist2, cost, traversable_only=1, min_dist2=4)
    assert trav["regions"]["cells"].tolist() == [6, 3, 1] and trav["regions"]["rep_cost"].tolist() == [9, INF, 4] and trav["regions"]["rep_x"][0] == 34
    by_size, _ = check(fusion, "strips by size", state, dist2, cost, size_weight=1 << 20, cost_weight=0)
    assert by_size["order"].tolist() == [0, 2, 1]


@pytest.mark.parametrize("seed", [11, 12])
def test_traversable_only_on_a_random_grid(seed, fusion):
    state, dist2 = fr.random_grid(70, 45, seed)
    cost = fr.random_cost(70, 45, seed)
    _, want = check(fusion, "traversable seed %d" % seed, state, dist2, cost, traversable_only=1, min_dist2=4, min_cells=2, reachable_only=1)
    _, every = check(fusion, "every member seed %d" % seed, state, dist2, cost, min_cells=2, reachable_only=1)
    assert 0 < want["stats"]["frontier_cells"] < every["stats"]["frontier_cells"]
    assert want["stats"]["regions_kept"] >= 2 and want["stats"]["regions_small"] + want["stats"]["regions_unreached"] >= 1


# ---- the gain -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 7, 128])
def test_the_gain_on_a_random_grid(R, fusion):
    state, dist2 = fr.random_grid(140, 150, 21, obstacles=0.004, unknown=0.06)
    got, want = check(fusion, "gain R %d" % R, state, dist2, None, gain_radius=R, min_cells=4, max_regions=5, gain_weight=3)
    assert want["stats"]["regions_written"] == 5 and want["stats"]["regions_small"] >= 1 and want["stats"]["gain_rays"] == 40 * R
    assert all(g > 0 for g in got["regions"]["gain"]) and (R < 128 or min(got["regions"]["gain"]) > 500)
    r = want["regions"][0]
    distinct, visits = fr.gain_by_ray_lists(state, r["rep_x"], r["rep_y"], R)
    assert distinct == r["gain"] and (R == 1 or visits > distinct)       # many rays share their first cells


def test_the_gain_in_a_corner_behind_a_wall_and_by_weight(fusion):
    state = np.full((45, 70), -1, np.int8)
    state[0, 0] = state[44, 69] = state[20, 33] = 0                      # two corners and a cell beside a tile border
    state[:, 34] = 100                                                   # a wall beside the middle cell shadows the right half of its window
    state[30, 34] = -1                                                   # ... but for one hole, which longer rays pass
    for R in (1, 7, 40, 128):
        got, want = check(fusion, "corners R %d" % R, state, gain_radius=R, gain_weight=1, cost_weight=0)
        assert got["regions"]["label"].tolist() == [0, 20 * 70 + 33, 44 * 70 + 69]
        if R == 7:
            assert got["regions"]["gain"].tolist() == [8 * 8 - 1, 15 * 15 - 1 - 7 * 15, 8 * 8 - 1]
            assert got["order"].tolist() == [1, 0, 2]                    # the largest gain first; a tie goes to the smaller label
        if R == 128:
            assert min(got["regions"]["gain"]) > 1000 and got["order"].tolist() == [2, 0, 1]


# ---- device arrays ---------------------------------------------------------------------------------------------------------------
def test_device_tensors_give_the_same_bits(fusion):
    import torch
    state, dist2 = fr.random_grid(70, 97, 8)
    cost = fr.random_cost(70, 97, 9)
    kw = dict(min_cells=2, reachable_only=1, traversable_only=1, min_dist2=2, gain_radius=9, gain_weight=2, max_regions=40)
    host, want = check(fusion, "host arrays", state, dist2, cost, **kw)
    assert want["stats"]["regions_kept"] > 40 and want["stats"]["regions_small"] >= 1
    dev = torch.device("cuda")
    s_dev, d_dev, c_dev = torch.from_numpy(state).to(dev), torch.from_numpy(dist2).to(dev), torch.from_numpy(cost.view(np.int32)).to(dev)
    region = torch.full((70, 97), -7, dtype=torch.int32, device=dev)
    got = fusion.nav_frontiers_device(s_dev, 97, 70, d_dev, c_dev, region, **kw)
    assert (region.cpu().numpy() == host["region"]).all()
    assert got["regions"].tobytes() == host["regions"].tobytes() and (got["order"] == host["order"]).all()
    assert {k: got["stats"][k] for k in fr.STATS} == {k: host["stats"][k] for k in fr.STATS}
    # addresses instead of tensors, and no map
    less = fusion.nav_frontiers_device(s_dev.data_ptr(), 97, 70, d_dev.data_ptr(), c_dev.data_ptr(), None, **kw)      # (the tensors outlive the call)
    assert less["regions"].tobytes() == host["regions"].tobytes() and (less["order"] == host["order"]).all()
    assert (s_dev.cpu().numpy() == state).all() and (c_dev.cpu().numpy().view(np.uint32) == cost).all()      # the inputs are read only


# ---- the staging of host arrays ------------------------------------------------------------------------------------------------
FILL = util.GUARD_WORD
OUTPUTS = ("region", "regions", "order")
_STAGING = {}


def staging_case(h, w):
    """dict(state, dist2, cost, kw, want): a random grid and cost field under every filter, with a gain; the restatement's answer,
    computed once and shared"""
    if (h, w) not in _STAGING:
        state, dist2 = fr.random_grid(h, w, 300 + h + w)
        cost = fr.random_cost(h, w, 11 + h)
        kw = dict(min_cells=2, reachable_only=1, traversable_only=1, min_dist2=2, gain_radius=3, gain_weight=2, max_regions=64)
        _STAGING[h, w] = dict(state=state, dist2=dist2, cost=cost, kw=kw, want=fr.frontiers(state, dist2, cost, **kw))
    return _STAGING[h, w]


def frontiers_host(f, c, names):
    """ssf_navfrontier_regions with host arrays, the outputs `names` alone, each between guard bytes and filled with them: (name ->
    array, stats)"""
    C = binding.C
    (h, w), n = c["state"].shape, c["kw"]["max_regions"]
    shapes = dict(region=((h, w), np.int32), regions=((n,), binding.NAVFRONTIER_REGION_DTYPE), order=((n,), np.int32))
    out = {nm: util.guarded(*shapes[nm]) for nm in names}
    p, st = f._navfrontier_params(False, w, h, c["kw"]), binding.SsfNavFrontierStats()
    o = binding.SsfNavFrontierOut(*[binding._ptr(out[nm][0]) if nm in out else None for nm in OUTPUTS])
    f._ck(f.L.lib.ssf_navfrontier_regions(f.h, C.byref(p), binding._ptr(c["state"]), binding._ptr(c["dist2"]), binding._ptr(c["cost"]), C.byref(o), C.byref(st)),
          "ssf_navfrontier_regions")
    assert all(intact() for _, intact in out.values()), names
    return {nm: a for nm, (a, _) in out.items()}, st.as_dict()


def frontiers_same(got, stats, want, what):
    """every array of got equals the restatement's; the table and the order up to regions_written, and past it they hold the fill"""
    k = want["stats"]["regions_written"]
    cut = {nm: (a if nm == "region" else a[:k]) for nm, a in got.items()}
    if "region" in cut:
        assert (cut["region"] == want["region"]).all(), what
    if "regions" in cut:
        table = fr.as_records(want["regions"], binding.NAVFRONTIER_REGION_DTYPE)
        assert len(table) == k and all((cut["regions"][nm] == table[nm]).all() for nm in fr.FIELDS), what
        assert (got["regions"][k:].view(np.uint8) == util.GUARD_FILL).all(), what
    if "order" in cut:
        assert (cut["order"] == want["order"]).all() and (got["order"][k:] == FILL).all(), what
    assert {nm: stats[nm] for nm in fr.STATS} == {nm: want["stats"][nm] for nm in fr.STATS}, what


@pytest.mark.parametrize("h,w", [(19, 37), (1, 1)])
def test_host_arrays_whose_items_all_start_at_rounded_offsets(h, w, fusion):
    """703 cells and one cell: neither P nor 4 P is a multiple of 256, so dist2 and cost sit at rounded offsets of the staging buffer.
    Host arrays, device pointers and the restatement agree"""
    import torch
    c = staging_case(h, w)
    host, hs = frontiers_host(fusion, c, OUTPUTS)
    frontiers_same(host, hs, c["want"], "host %d x %d" % (h, w))
    region = torch.full((h, w), -7, dtype=torch.int32, device="cuda")
    dev = fusion.nav_frontiers_device(torch.from_numpy(c["state"]).to("cuda"), w, h, torch.from_numpy(c["dist2"]).to("cuda"),
                                      torch.from_numpy(c["cost"].view(np.int32)).to("cuda"), region, **c["kw"])
    k = hs["regions_written"]
    assert (region.cpu().numpy() == host["region"]).all() and dev["regions"].tobytes() == host["regions"][:k].tobytes() and (dev["order"] == host["order"][:k]).all()
    assert {nm: dev["stats"][nm] for nm in fr.STATS} == {nm: hs[nm] for nm in fr.STATS}
    assert h == 1 or (k >= 2 and c["want"]["stats"]["regions_small"] + c["want"]["stats"]["regions_unreached"] >= 1 and (c["want"]["region"] >= 0).any())


@pytest.mark.parametrize("name", OUTPUTS)
def test_one_host_output_alone_between_guard_bytes(name, fusion):
    """19 x 37, host arrays: every output on its own, all others NULL, equals the same array of the call that asks for all three, and
    the 256 bytes on either side of the caller's array are untouched"""
    c = staging_case(19, 37)
    if "every" not in c:
        c["every"] = frontiers_host(fusion, c, OUTPUTS)
    every, stats = c["every"]
    frontiers_same(every, stats, c["want"], "every output")
    alone, st = frontiers_host(fusion, c, (name,))
    assert alone[name].tobytes() == every[name].tobytes() and {k: st[k] for k in fr.STATS} == {k: stats[k] for k in fr.STATS}, name


def test_the_staging_buffer_grows_and_is_used_again(explore_lib):
    """one handle: 8 x 8, 19 x 37, 8 x 8 again.  Each call gives what a handle that has made no other call gives"""
    f = handle(explore_lib)
    for h, w in ((8, 8), (19, 37), (8, 8)):
        c = staging_case(h, w)
        fresh = handle(explore_lib)
        (got, gs), (want, ws) = frontiers_host(f, c, OUTPUTS), frontiers_host(fresh, c, OUTPUTS)
        fresh.close()
        assert all(got[nm].tobytes() == want[nm].tobytes() for nm in got) and {k: gs[k] for k in fr.STATS} == {k: ws[k] for k in fr.STATS}, (h, w)
        frontiers_same(got, gs, c["want"], (h, w))
    f.close()


# ---- where to go next ----------------------------------------------------------------------------------------------------------------
def test_nav_explore_equals_the_three_reference_calls_chained(fusion):
    state, dist2, robot = fr.room()
    assert state.shape == (45, 70)
    plan = dict(soft_dist2=16, near_penalty=20)
    frontier = dict(min_cells=2, gain_radius=6)
    got = fusion.nav_explore(state, dist2, robot, plan=plan, frontier=frontier)
    field = pr.plan(state, dist2, [robot], None, **plan)
    want = fr.frontiers(state, dist2, field["cost"], reachable_only=1, **frontier)
    same(got, want, "nav_explore")
    assert want["stats"]["regions_kept"] >= 2 and want["stats"]["regions_small"] >= 1 and want["stats"]["regions_unreached"] >= 1, want["stats"]
    c = int(want["order"][0])
    goal = (want["regions"][c]["rep_x"], want["regions"][c]["rep_y"])
    drive = pr.plan(state, dist2, [goal], [robot], max_path=45 * 70, **plan)
    assert got["chosen"] == c and got["goal"] == goal and got["status"] == 0 == drive["start_status"][0]
    assert got["cost"] == drive["start_cost"][0] and (got["path"] == drive["path"][0]).all() and got["path"][-1].tolist() == list(goal)
    # the field's cost is from the cell to the robot: the drive out pays the goal's penalty and not the robot's
    pen = field["pen"]
    assert got["cost"] == want["regions"][c]["rep_cost"] + int(pen[goal[1], goal[0]]) - int(pen[robot[1], robot[0]])
    assert int(pen[goal[1], goal[0]]) != int(pen[robot[1], robot[0]])
    assert {k: got["field_stats"][k] for k in pr.STATS} == field["stats"] and {k: got["path_stats"][k] for k in pr.STATS} == drive["stats"]
    # a robot that is walled in reaches no region
    walled = state.copy()
    walled[8:13, 13] = walled[8:13, 17] = walled[8, 13:18] = walled[12, 13:18] = 100
    nothing = fusion.nav_explore(walled, dist2, robot, plan=plan, frontier=frontier)
    assert nothing["chosen"] == -1 and nothing["goal"] is None and len(nothing["path"]) == 0 and len(nothing["regions"]) == 0
    assert nothing["stats"]["regions_unreached"] >= 2


# ---- no side effects, refusals, profiling -------------------------------------------------------------------------------------
def test_the_regions_change_no_later_result(explore_lib):
    A, B = handle(explore_lib), handle(explore_lib)
    state, dist2 = fr.random_grid(45, 70, 6)
    cost = fr.random_cost(45, 70, 6)
    for k in (0, 3, 6):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        A.nav_frontiers(state, dist2, cost, gain_radius=12, min_cells=2)
        grid = A.nav_grid(outputs=("state", "dist2"), width=96, height=80)
        A.nav_explore(grid["state"], grid["dist2"], (48, 40), plan=dict(allow_unknown=1), frontier=dict(gain_radius=5))
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)
    B.close()
    A.close()


def test_the_refusals(explore_lib):
    f = handle(explore_lib)
    state, dist2 = fr.random_grid(6, 9, 1)
    cost = fr.random_cost(6, 9, 1)
    refused = pytest.raises(binding.SsfError, match=r"ssf_navfrontier_regions failed \(-1\)")
    for kw in (dict(connectivity=6), dict(connectivity=0), dict(min_dist2=-1), dict(min_cells=0), dict(max_regions=0), dict(max_regions=65537),
               dict(gain_radius=-1), dict(gain_radius=129), dict(cost_weight=-1), dict(gain_weight=(1 << 20) + 1), dict(size_weight=-1)):
        with refused:
            f.nav_frontiers(state, dist2, cost, **kw)
    with refused:
        f.nav_frontiers(state, None, cost, traversable_only=1)         # traversable_only without dist2
    with refused:
        f.nav_frontiers(state, dist2, None, reachable_only=1)          # reachable_only without cost
    with refused:
        f.nav_frontiers(np.zeros((0, 5), np.int8))
    with refused:
        f.nav_frontiers(np.zeros((1, 4097), np.int8))
    L, byref, vp = explore_lib.lib, binding.C.byref, binding.C.c_void_p
    p, st = binding.SsfNavFrontierParams(), binding.SsfNavFrontierStats()
    assert L.ssf_navfrontier_default_params(f.h, byref(p)) == 0
    assert L.ssf_navfrontier_default_params(None, byref(p)) == -1 and L.ssf_navfrontier_default_params(f.h, None) == -1
    assert f.nav_frontiers_default_params() == dict(width=512, height=512, connectivity=8, traversable_only=0, min_dist2=0, min_cells=1,
                                                    reachable_only=0, max_regions=4096, gain_radius=0, cost_weight=1, gain_weight=0, size_weight=0,
                                                    on_device=0)
    s8 = np.ascontiguousarray(state)
    region = np.zeros((6, 9), np.int32)
    p.width, p.height = 9, 6
    out = binding.SsfNavFrontierOut(region.ctypes.data, None, None)
    a = s8.ctypes.data_as(vp)
    assert L.ssf_navfrontier_regions(f.h, byref(p), a, None, None, byref(out), None) == 0       # stats, dist2 and cost are optional
    assert (region == fr.frontiers(state)["region"]).all()
    assert L.ssf_navfrontier_regions(None, byref(p), a, None, None, byref(out), byref(st)) == -1
    assert L.ssf_navfrontier_regions(f.h, None, a, None, None, byref(out), byref(st)) == -1
    assert L.ssf_navfrontier_regions(f.h, byref(p), None, None, None, byref(out), byref(st)) == -1
    assert L.ssf_navfrontier_regions(f.h, byref(p), a, None, None, None, byref(st)) == -1
    assert L.ssf_navfrontier_regions(f.h, byref(p), a, None, None, byref(binding.SsfNavFrontierOut()), byref(st)) == -1
    for field, bad in (("width", 0), ("height", -3), ("width", 4097), ("height", 4097)):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert L.ssf_navfrontier_regions(f.h, byref(p), a, None, None, byref(out), byref(st)) == -1, (field, bad)
        setattr(p, field, keep)
    # the handle keeps working: the regions and a frame after the refusals
    check(f, "after the refusals", *fr.random_grid(33, 31, 1), cost=fr.random_cost(33, 31, 1), min_cells=2)
    f.process_frame(*util.frame(0, W, H))
    check(f, "after a frame", *fr.random_grid(33, 31, 2), cost=fr.random_cost(33, 31, 2), gain_radius=4)
    g = handle(explore_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_frontiers(state)
    q = handle(explore_lib, pipeline_depth=2, extract_batch=2)
    q.submit_frame(*util.frame(0, W, H))
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q.nav_frontiers(state)
    q.process_submitted()
    check(q, "pipelined, at rest", state, dist2, cost)
    q.close()
    g.close()
    f.close()


def test_the_largest_grid_and_a_grid_that_shrinks(explore_lib):
    """4096 x 4096: cell indices up to 2^24 - 1 in the labels; then a small grid on the same handle's buffers"""
    f = handle(explore_lib)
    state = np.full((4096, 4096), 100, np.int8)
    state[4095, 4000:4096] = 0
    state[4094, 4000:4096] = -1
    state[0, 0] = 0
    state[1, 0] = -1
    state[2000:2100, 2047:2049] = 0                                      # two columns of members on either side of a tile border
    state[2000:2100, 2046] = state[2000:2100, 2049] = -1
    got, _ = check(f, "4096 x 4096", state, gain_radius=2)
    assert got["regions"]["label"].tolist() == [0, 2000 * 4096 + 2047, 4095 * 4096 + 4000] and got["regions"]["cells"].tolist() == [1, 200, 96]
    assert got["regions"]["sum_x"].tolist() == [0, 100 * (2047 + 2048), sum(range(4000, 4096))] and got["regions"]["sum_y"][2] == 96 * 4095
    assert (got["region"] >= 0).sum() == 297 and got["region"][4095, 4095] == 2 and got["stats"]["merge_pairs"] >= 100
    check(f, "a small grid afterwards", *fr.random_grid(33, 31, 3))
    f.close()


def test_the_kernels_are_timed_under_profile(explore_lib):
    f = handle(explore_lib, profile=1)
    f.reset_kernel_times()
    state, dist2 = fr.random_grid(70, 97, 4)
    check(f, "profiled", state, dist2, fr.random_cost(70, 97, 4), gain_radius=5)
    names = f.kernel_times()
    for k in ("navfrontier_label", "navfrontier_merge", "navfrontier_flatten", "navfrontier_sums", "navfrontier_table", "navfrontier_map", "navfrontier_gain"):
        assert k in names and names[k][1] > 0, (k, names)
    f.close()


# ---- replay.py's files -----------------------------------------------------------------------------------------------------
def test_replay_writes_the_regions_next_to_the_grid(explore_lib, tmp_path):
    import json
    from supersurfel_fusion_amd import replay
    f = handle(explore_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    _, results = replay.replay(f, frames, nav_grid_dir=str(tmp_path), nav_grid_every=2, nav_grid_res=0.1, nav_grid_carve=True, nav_grid_carve_stride=4,
                               nav_frontiers=dict(min_cells=2, gain_radius=10))
    per_grid = [".pgm", ".yaml", "_dist2.npy", "_frontier_regions.npy", "_frontiers.json", "_seen.npy"]
    assert sorted(os.listdir(str(tmp_path))) == sorted("%06d%s" % (k, s) for k in (0, 2) for s in per_grid)
    grid = f.nav_grid_carve([r["pose"] for r in results], outputs=("state", "dist2"), carve=dict(stride=4), res=0.1)
    start, _ = replay.plan_cells(grid["stats"]["pose"], 0.1, f.get_pose()[9:12], [])
    field = pr.plan(grid["state"], grid["dist2"], start)
    want = fr.frontiers(grid["state"], grid["dist2"], field["cost"], min_cells=2, gain_radius=10)
    assert want["stats"]["regions_kept"] >= 1 and want["stats"]["frontier_cells"] > 0
    assert (np.load(str(tmp_path / "000002_frontier_regions.npy")) == want["region"]).all()
    told = json.load(open(str(tmp_path / "000002_frontiers.json")))
    assert told["regions"] == [{nm: int(r[nm]) for nm in fr.FIELDS} for r in want["regions"]] and told["order"] == want["order"].tolist()
    assert {k: told["stats"][k] for k in fr.STATS} == want["stats"] and told["start"] == start[0].tolist()
    with pytest.raises(ValueError, match="nav_frontiers needs nav_grid_dir"):
        replay.replay(f, [], nav_frontiers=dict())
    f.close()


# ---- the C++ surface -----------------------------------------------------------------------------------------------------
def test_the_regions_in_cpp(explore_lib, fusion, tmp_path):
    """tests/cpp/navfrontier_smoke.cpp on the GPU: its counts and FNV-1a checksums equal those of the Python calls on the same arrays"""
    libdir = os.path.dirname(explore_lib.path)
    exe = str(tmp_path / "navfrontier_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "navfrontier_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip_explore", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    names = ("cells", "found", "small", "unreached", "kept", "written", "largest", "rays")
    got = re.search(r"navfrontier 70x45 " + " ".join(nm + r"=(\d+)" for nm in names) + r" region=([0-9a-f]{16}) table=([0-9a-f]{16}) order=([0-9a-f]{16})",
                    r.stdout)
    assert got and re.search(r"goal ok=1", r.stdout), r.stdout
    state, dist2 = pr.hashed_grid()
    kw = dict(min_cells=2, gain_radius=5, max_regions=64)
    py, want = check(fusion, "python regions", state, dist2, None, **kw)
    s = want["stats"]
    assert s["regions_kept"] >= 2 and s["regions_small"] >= 1, s
    counts = (s["frontier_cells"], s["regions_found"], s["regions_small"], s["regions_unreached"], s["regions_kept"], s["regions_written"],
              s["largest_cells"], s["gain_rays"])
    assert tuple(int(v) for v in got.groups()[:8]) == counts, (got.groups(), counts)
    sums = (pr.fnv1a(py["region"].tobytes()), pr.fnv1a(py["regions"].tobytes()), pr.fnv1a(py["order"].tobytes()))
    assert tuple(int(v, 16) for v in got.groups()[8:]) == sums, (got.groups(), sums)
    ex = re.search(r"explore robot=(\d+),(\d+) chosen=(\d+) label=(\d+) goal=(\d+),(\d+) rep_cost=(\d+) drive=(\d+) status=(\d+) cells=(\d+) "
                   r"table=([0-9a-f]{16}) path=([0-9a-f]{16})", r.stdout)
    assert ex, r.stdout
    robot = (int(ex.group(1)), int(ex.group(2)))
    assert state[robot[1], robot[0]] == 0
    e = fusion.nav_explore(state, dist2, robot, plan=dict(soft_dist2=30, near_penalty=25), frontier=kw)
    c = e["chosen"]
    told = tuple(int(v) for v in ex.groups()[2:10])
    assert told == (c, e["regions"]["label"][c], e["goal"][0], e["goal"][1], e["regions"]["rep_cost"][c], e["cost"], e["status"], len(e["path"]))
    assert (int(ex.group(11), 16), int(ex.group(12), 16)) == (pr.fnv1a(e["regions"].tobytes()), pr.fnv1a(np.ascontiguousarray(e["path"]).tobytes()))
