"""ssf_navpath_waypoints (include/ssf_navpath.h) on the MI355X against the restatement (tests/navpath_ref.py): every waypoint, count,
status, minimum and exact stat with == -- paths planned on random grids under every rule, corridors and staircases at the edges of
the LDS window and of the 256-candidate chunks, the hand-written cases, a pillar placed across and inside a chunk, many paths with
bad ones among them, truncation, untouched entries; plus device arrays, plan and refine without leaving the device, no side effects
on the frame path, the refusals, profiling, replay's files and the C++ surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import navpath_ref as wr
import navplan_ref as pr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
W, H = 160, 128
CPP = os.path.join(ROOT, "tests", "cpp")
ARRAYS = ("n_waypoints", "status", "path_min")
F, X = 0, 100


def handle(lib, **kw):
    """a handle of a test's own, which the test closes when it is done with it"""
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


@pytest.fixture(scope="module")
def drive_lib():
    """libssf_hip_drive.so: explore's objects plus the waypoints' entry points (no fallback: a missing .so is an error)"""
    return binding.load_drive()


@pytest.fixture(scope="module")
def fusion(drive_lib):
    f = handle(drive_lib)
    yield f
    f.close()


def same(got, want, what):
    for name in ARRAYS:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name, got[name].shape, got[name].dtype)
        assert (got[name] == want[name]).all(), (what, name, got[name].tolist()[:20], want[name].tolist()[:20])
    assert len(got["waypoints"]) == len(want["waypoints"]), what
    for i, (a, b) in enumerate(zip(got["waypoints"], want["waypoints"])):
        assert a.dtype == np.int32 and a.shape == b.shape and (a == b).all(), (what, "path", i, a.tolist()[:8], b.tolist()[:8])
    for k in wr.STATS:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"], want["stats"])


def check(f, what, state, dist2, path, path_len=None, **kw):
    """the waypoints on the device and in the restatement; returns both"""
    want = wr.waypoints(state, dist2, path, path_len, **kw)
    got = f.nav_waypoints(state, dist2, path, path_len, **kw)
    assert sorted(got) == sorted(binding.NAVPATH_OUTPUT_NAMES + ("stats",)), what
    same(got, want, what)
    assert got["stats"]["segments_tested"] >= got["stats"]["waypoints"] - got["stats"]["paths_ok"]
    return got, want


def some_starts(h, w, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1).astype(np.int32)


# ---- paths planned on random grids ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 97), (33, 31), (45, 70), (64, 64), (160, 160)])
def test_planned_paths_under_every_rule(h, w, fusion):
    state, dist2 = pr.random_grid(h, w, 300 + h + w, obstacles=0.15, unknown=0.1)
    goal = (w // 2, h // 2)
    state[goal[1], goal[0]], dist2[goal[1], goal[0]] = 0, 5
    starts = np.concatenate([some_starts(h, w, 7, h * w), [goal]]).astype(np.int32)
    for allow in (0, 1):
        plan = fusion.nav_plan(state, dist2, [goal], starts, outputs=("path", "path_len"), max_path=h * w, allow_unknown=allow)
        paths = plan["path"]
        assert len(paths[-1]) == 1 and (h * w < 1000 or max(len(p) for p in paths) > 10)
        got, _ = check(fusion, "%d x %d defaults, unknown %d" % (h, w, allow), state, dist2, paths, allow_unknown=allow)
        assert got["stats"]["forced_steps"] == 0 and got["stats"]["paths_ok"] == 8 and (got["status"] == 0).all()
        if allow:                                                        # a path through unknown cells is refused where they are not allowed
            strict = wr.waypoints(state, dist2, paths)
            assert h * w < 3000 or (strict["status"] == 2).any()
            same(fusion.nav_waypoints(state, dist2, paths), strict, "unknown cells refused")
        # more clearance than the paths have: forced steps, in the restatement first
        # (every path ends on the goal, whose clearance is 5: the last segment is never visible, so the last step is forced; a cell
        # of less clearance in the middle of a path may be passed by and forces nothing)
        low = min([int(dist2[c[1], c[0]]) for p in paths if len(p) > 1 for c in p] or [0])
        for los in sorted({low + 1, 6}):
            want = wr.waypoints(state, dist2, paths, allow_unknown=allow, los_dist2=los)
            long = sum(len(p) > 1 for p in paths)
            assert los < 6 or (want["stats"]["forced_steps"] >= long and (long > 0 or h * w < 1000))
            same(fusion.nav_waypoints(state, dist2, paths, allow_unknown=allow, los_dist2=los), want, "los_dist2 %d, above the paths' clearance" % los)
        check(fusion, "keep_clearance", state, dist2, paths, allow_unknown=allow, keep_clearance=1, clearance_cap=12)
        check(fusion, "keep_clearance, a window of 9", state, dist2, paths, allow_unknown=allow, keep_clearance=1, clearance_cap=1024 * 1024, los_dist2=2,
              lookahead=9)


@pytest.mark.parametrize("h,w", pr.FOREIGN_SIZES)
@pytest.mark.parametrize("allow", [0, 1])
def test_paths_planned_on_grids_with_states_outside_0_minus_1_100_and_dist2_outside_the_cap(h, w, allow, fusion):
    """tests/navplan_ref.py's foreign grid and the paths planned on it: a cell of any state but 0 (and -1 when allowed) or of negative
    dist2 hides what lies behind it; d is max(dist2, 0), whatever its size"""
    f = pr.foreign_case(h, w, allow)
    state, dist2 = f["state"], f["dist2"]
    plan = fusion.nav_plan(state, dist2, f["goals"], f["starts"], outputs=("path", "path_len"), **f["kw"])
    paths = plan["path"]
    assert len(paths) == len(f["plan"]["path"]) and all((a == b).all() for a, b in zip(paths, f["plan"]["path"])) and sum(len(p) > 10 for p in paths) >= 2
    what = "foreign %d x %d unknown %d" % (h, w, allow)
    got, _ = check(fusion, what + " defaults", state, dist2, paths, allow_unknown=allow)
    assert (got["status"] == 0).all() and got["stats"]["forced_steps"] == 0
    check(fusion, what + " keep_clearance, los", state, dist2, paths, allow_unknown=allow, keep_clearance=1, clearance_cap=12, los_dist2=2)
    check(fusion, what + " the largest cap, a window of 9", state, dist2, paths, allow_unknown=allow, keep_clearance=1, clearance_cap=1024 * 1024, lookahead=9)
    got, _ = check(fusion, what + " los above the paths' clearance", state, dist2, paths, allow_unknown=allow, los_dist2=41)
    assert got["stats"]["forced_steps"] > 0
    if allow:                                                            # the same paths where unknown cells are not allowed
        strict, _ = check(fusion, what + " unknown refused", state, dist2, paths)
        assert (strict["status"] == 2).any()


# ---- the edges of the window and of the chunks ---------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 258, 513, 4097)
LOOKAHEADS = (1, 2, 255, 256, 257, 4096)


@pytest.fixture(scope="module")
def corridors():
    """the corridor paths of every length as one call's paths, on one grid, with the restatement's answers per lookahead"""
    state, dist2, full = wr.corridor(4097, seed=4)
    paths = [full[:n] for n in LENGTHS]
    return state, dist2, paths, {la: wr.waypoints(state, dist2, paths, lookahead=la, keep_clearance=1, clearance_cap=30) for la in LOOKAHEADS}


@pytest.mark.parametrize("lookahead", LOOKAHEADS)
def test_corridors_at_the_window_and_chunk_edges(lookahead, fusion, corridors):
    state, dist2, paths, wants = corridors
    want = wants[lookahead]
    got = fusion.nav_waypoints(state, dist2, paths, lookahead=lookahead, keep_clearance=1, clearance_cap=30)
    same(got, want, "corridors, lookahead %d" % lookahead)
    assert got["n_waypoints"].tolist() == [1 + (n - 1 + lookahead - 1) // lookahead for n in LENGTHS]      # every candidate of a straight run is seen
    assert got["stats"]["cells_in"] == sum(LENGTHS) and got["stats"]["forced_steps"] == 0


@pytest.mark.parametrize("n", [2, 65, 257, 258, 513])
def test_staircases_that_keep_their_clearance(n, fusion):
    """what a segment crosses is not on the path, so the running minimum of the window decides, candidate by candidate"""
    state, dist2, cells = wr.staircase(n, n)
    counts = set()
    for la in (2, 255, 256, 257, 4096):
        got, _ = check(fusion, "staircase %d, lookahead %d" % (n, la), state, dist2, [cells], lookahead=la, keep_clearance=1, clearance_cap=25)
        counts.add(int(got["n_waypoints"][0]))
        check(fusion, "staircase %d, lookahead %d, los" % (n, la), state, dist2, [cells], lookahead=la, los_dist2=12)
    assert n < 100 or (len(counts) > 1 and max(counts) > 5)


# ---- hand-written answers ----------------------------------------------------------------------------------------------------
def test_the_hand_written_cases(fusion):
    state, dist2 = wr.open_grid(6, 9, 7)
    got, _ = check(fusion, "a straight run", state, dist2, [np.array([(x, 2) for x in range(9)])])
    assert got["waypoints"][0].tolist() == [[0, 2, 0, 7], [8, 2, 8, 7]] and got["path_min"].tolist() == [7]
    stairs = np.array([(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2), (6, 3), (7, 3), (8, 4)])
    got, _ = check(fusion, "a staircase", state, dist2, [stairs])
    assert got["waypoints"][0].tolist() == [[0, 0, 0, 7], [8, 4, 8, 7]]
    state = np.array([[F, F, F, F, F], [F, F, F, F, F], [X, X, X, F, F], [F, F, F, F, F], [F, F, F, F, F]], np.int8)
    cells = np.array([(0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (4, 2), (4, 3), (3, 4), (2, 4), (1, 4), (0, 4)])
    got, _ = check(fusion, "an L", state, np.full((5, 5), 2, np.int32), [cells])
    assert got["waypoints"][0].tolist() == [[0, 0, 0, 2], [4, 2, 5, 2], [0, 4, 10, 2]]
    state = np.array([[F, X, F], [X, F, F], [F, F, F]], np.int8)
    got, _ = check(fusion, "a shared corner", state, np.array([[5, 0, 5], [0, 5, 5], [5, 5, 5]], np.int32), [np.array([(0, 0), (1, 1), (2, 2)])])
    assert got["waypoints"][0].tolist() == [[0, 0, 0, 5], [1, 1, 1 | wr.FORCED, 0], [2, 2, 2, 5]] and got["stats"]["forced_steps"] == 1
    state, dist2, cells, win = wr.pillar()
    got, _ = check(fusion, "a pillar", state, dist2, [cells], los_dist2=1)
    assert got["waypoints"][0].tolist() == [[0, 2, 0, 1], [5, 0, 7, 1]]


@pytest.mark.parametrize("tail,where", [(10, "inside the first chunk"), (255, "the last lane of the first chunk"), (256, "the first lane of the second chunk"),
                                        (300, "inside the second chunk"), (511, "the last lane of the second chunk")])
def test_a_pillar_across_and_inside_a_chunk(tail, where, fusion):
    """the winner is `tail` candidates from the far end of the window and its nearer neighbours are hidden: with 255 and 511 they
    fall into the chunk after the winner's, otherwise into the same one"""
    state, dist2, cells, win = wr.pillar(hidden=20, Y=12, tail=tail)
    trav, d = wr.prep(state, dist2, wr.params())
    assert wr.visible(trav, d, cells[0], cells[win], 1) and not wr.visible(trav, d, cells[0], cells[win - 1], 1) and len(cells) - 1 - win == tail
    got, _ = check(fusion, "pillar, winner %s" % where, state, dist2, [cells], los_dist2=1, lookahead=4096)
    wp = got["waypoints"][0]
    assert wp[1].tolist() == [cells[win][0], cells[win][1], win, 1] and got["stats"]["forced_steps"] == tail and len(wp) == 2 + tail
    assert (wp[2:, 2] == (np.arange(win + 1, len(cells)) | wr.FORCED)).all() and (wp[2:, 3] == 0).all() and got["path_min"].tolist() == [0]
    check(fusion, "pillar, a window that ends on the winner", state, dist2, [cells], los_dist2=1, lookahead=win)
    check(fusion, "pillar, a window that ends before the winner", state, dist2, [cells], los_dist2=1, lookahead=win - 1)


# ---- many paths, bad ones among them ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_paths", [1, 3, 4, 5, 257])
def test_many_paths_with_bad_ones_among_them(n_paths, fusion):
    state, dist2 = pr.random_grid(45, 70, 17, obstacles=0.1)
    state[10, :] = 0
    row = np.stack([np.arange(70), np.full(70, 10)], 1).astype(np.int32)
    rng = np.random.default_rng(n_paths)
    paths, lens, kinds = [], [], []
    for i in range(n_paths):
        kind = i % 5 if n_paths > 1 else 0
        a = int(rng.integers(0, 30))
        c = row[a:a + int(rng.integers(2, 40))].copy()
        n = len(c)
        if kind == 1:
            n = 71 if i % 2 else -1                                      # longer than max_path; negative
        elif kind == 2:
            c[len(c) // 2] = ((70, 10), (-1, 10), (5, 45))[i % 3]        # outside the grid
        elif kind == 3:
            c[-1, 0] += 1                                                # a jump of two cells
        elif kind == 4 and i % 2:
            c = c[:0]; n = 0                                             # an empty path is no error
        paths.append(c); lens.append(n); kinds.append(kind)
    path, _ = wr.pack_paths(paths, max_path=70)
    lens = np.array(lens, np.int32)
    got, _ = check(fusion, "%d paths" % n_paths, state, dist2, path, lens, lookahead=16)
    want_status = [{0: 0, 1: 1, 2: 2, 3: 3, 4: 0}[k] for k in kinds]
    assert got["status"].tolist() == want_status and ((got["n_waypoints"] > 0) == ((np.array(want_status) == 0) & (lens > 0))).all()
    assert (got["path_min"][got["n_waypoints"] == 0] == -1).all() and got["stats"]["paths_bad"] == sum(s != 0 for s in want_status)


def test_truncation_and_entries_that_are_not_written(fusion):
    state, dist2 = wr.open_grid(4, 7, 1)
    stairs = np.array([(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2), (6, 3)], np.int32)
    full, _ = check(fusion, "all four", state, dist2, [stairs, stairs[:1], stairs[:0]], lookahead=2)
    assert full["n_waypoints"].tolist() == [4, 1, 0] and full["status"].tolist() == [0, 0, 0]
    for mw, status in ((1, 4), (2, 4), (3, 4), (4, 0)):
        got, _ = check(fusion, "max_waypoints %d" % mw, state, dist2, [stairs, stairs[:1], stairs[:0]], lookahead=2, max_waypoints=mw)
        assert got["status"].tolist() == [status, 0, 0] and (got["waypoints"][0] == full["waypoints"][0][:mw]).all()
        assert got["stats"]["paths_truncated"] == (status == 4) and got["stats"]["paths_ok"] == 3
    # entries past n_waypoints keep what the caller wrote
    path, lens = wr.pack_paths([stairs, stairs[:1], stairs[:0], stairs[::-1]])
    lens[3] = 9
    p = fusion._navpath_params(False, 7, 4, 4, path.shape[1], dict(lookahead=2, max_waypoints=5))
    wp = np.full((4, 5, 4), -7, np.int32)
    n = np.full(4, -7, np.int32)
    vp = binding.C.c_void_p
    st8, d2 = np.ascontiguousarray(state), np.ascontiguousarray(dist2)
    fusion._navpath_waypoints(p, st8.ctypes.data_as(vp), d2.ctypes.data_as(vp), path.ctypes.data_as(vp), lens.ctypes.data_as(vp),
                              dict(waypoints=wp.ctypes.data_as(vp), n_waypoints=n.ctypes.data_as(vp)))
    assert n.tolist() == [4, 1, 0, 0]
    for i, k in enumerate(n):
        assert (wp[i, k:] == -7).all() and (wp[i, :k] == full["waypoints"][i]).all() if i < 3 else (wp[i] == -7).all()
    only = fusion.nav_waypoints(state, dist2, [stairs], outputs=("path_min",), lookahead=2)           # one output alone is a valid request
    assert sorted(only) == ["path_min", "stats"] and only["path_min"].tolist() == [1] and only["stats"]["waypoints"] == 4


# ---- device arrays, plan and refine on the device ----------------------------------------------------------------------------
def test_device_tensors_give_the_same_bits(fusion):
    import torch
    state, dist2 = pr.random_grid(70, 97, 8, obstacles=0.12, unknown=0.1)
    state[35, 48] = 0
    starts = some_starts(70, 97, 9, 3)
    plan = fusion.nav_plan(state, dist2, [(48, 35)], starts, outputs=("path", "path_len"), max_path=300, allow_unknown=1)
    path, lens = wr.pack_paths(plan["path"], max_path=300)
    assert (lens == plan["path_len"]).all() and lens.max() > 20
    kw = dict(allow_unknown=1, keep_clearance=1, clearance_cap=10, los_dist2=1, lookahead=50, max_waypoints=40)
    host, _ = check(fusion, "host arrays", state, dist2, path, lens, **kw)
    dev = torch.device("cuda")
    n = len(lens)
    t = dict(n_waypoints=torch.zeros(n, dtype=torch.int32, device=dev), status=torch.zeros(n, dtype=torch.int32, device=dev),
             path_min=torch.zeros(n, dtype=torch.int32, device=dev), waypoints=torch.full((n, 40, 4), -7, dtype=torch.int32, device=dev))
    d_state, d_dist2, d_path, d_len = (torch.from_numpy(a).to(dev) for a in (state, dist2, path, lens))
    stats = fusion.nav_waypoints_device(d_state, d_dist2, 97, 70, d_path, d_len, n, 300, **dict(t, **kw))
    got = {k: v.cpu().numpy() for k, v in t.items()}
    for k in ARRAYS:
        assert (got[k] == host[k]).all(), k
    for i, c in enumerate(got["n_waypoints"]):
        assert (got["waypoints"][i, :c] == host["waypoints"][i]).all() and (got["waypoints"][i, c:] == -7).all()
    assert {k: stats[k] for k in wr.STATS} == {k: host["stats"][k] for k in wr.STATS}
    # addresses instead of tensors, and fewer outputs
    t2 = torch.zeros(n, dtype=torch.int32, device=dev)
    fusion.nav_waypoints_device(d_state.data_ptr(), d_dist2, 97, 70, d_path.data_ptr(), d_len, n, 300, path_min=t2.data_ptr(), **kw)
    assert (t2.cpu().numpy() == host["path_min"]).all()


# ---- the staging of the host grid and the lengths -----------------------------------------------------------------------------
FILL = util.GUARD_WORD
_STAGING = {}


def staging_case(h, w):
    """dict(state, dist2, path, lens, kw, want): five paths of the plan's restatement on a random grid, one with a length of 0 and one
    with a length past max_path among them, refined with a kept clearance; the restatement's answer, computed once and shared"""
    if (h, w) not in _STAGING:
        state, dist2 = pr.random_grid(h, w, 600 + h + w, obstacles=0.12, unknown=0.05)
        goal = (w // 2, h // 2)
        state[goal[1], goal[0]] = 0
        plan = pr.plan(state, dist2, [goal], some_starts(h, w, 5, 3 * h + w), max_path=h * w, allow_unknown=1)
        path, lens = wr.pack_paths(plan["path"] + [plan["path"][0][:0], plan["path"][0]])
        lens[-1] = path.shape[1] + 1
        kw = dict(allow_unknown=1, keep_clearance=1, clearance_cap=10, los_dist2=1, lookahead=50, max_waypoints=max(1, path.shape[1] // 2))
        _STAGING[h, w] = dict(state=state, dist2=dist2, path=path, lens=lens, kw=kw, want=wr.waypoints(state, dist2, path, lens, **kw))
    return _STAGING[h, w]


def waypoints_host(f, c, names):
    """ssf_navpath_waypoints with host arrays, the outputs `names` alone, each between guard bytes and filled with them: (name ->
    array, stats)"""
    (h, w), (n, mp, _), mw = c["state"].shape, c["path"].shape, c["kw"]["max_waypoints"]
    shapes = dict(n_waypoints=(n,), status=(n,), waypoints=(n, mw, 4), path_min=(n,))
    out = {nm: util.guarded(shapes[nm], np.int32) for nm in names}
    stats = f._navpath_waypoints(f._navpath_params(False, w, h, n, mp, c["kw"]), binding._ptr(c["state"]), binding._ptr(c["dist2"]), binding._ptr(c["path"]),
                                 binding._ptr(c["lens"]), {nm: binding._ptr(a) for nm, (a, _) in out.items()})
    assert all(intact() for _, intact in out.values()), names
    return {nm: a for nm, (a, _) in out.items()}, stats


def waypoints_same(got, want, what):
    """every array of got equals the restatement's; a path's waypoints up to their count, and past it they hold the fill"""
    for nm, a in got.items():
        if nm != "waypoints":
            assert (a == want[nm]).all(), (what, nm, a.tolist(), want[nm].tolist())
            continue
        for i, wp in enumerate(want["waypoints"]):
            assert (a[i, :len(wp)] == wp).all() and (a[i, len(wp):] == FILL).all(), (what, nm, i)


@pytest.mark.parametrize("h,w", [(19, 37), (1, 1)])
def test_host_arrays_whose_items_all_start_at_rounded_offsets(h, w, fusion):
    """703 cells and one cell: neither P nor 4 P is a multiple of 256, so dist2 and the lengths sit at rounded offsets of the staging
    buffer.  Host arrays, device pointers and the restatement agree"""
    import torch
    c = staging_case(h, w)
    host, hs = waypoints_host(fusion, c, binding.NAVPATH_OUTPUT_NAMES)
    waypoints_same(host, c["want"], "host %d x %d" % (h, w))
    t = {nm: torch.full(a.shape, FILL, dtype=torch.int32, device="cuda") for nm, a in host.items()}
    d = [torch.from_numpy(c[k]).to("cuda") for k in ("state", "dist2", "path", "lens")]
    ds = fusion.nav_waypoints_device(d[0], d[1], w, h, d[2], d[3], len(c["lens"]), c["path"].shape[1], **dict(t, **c["kw"]))
    assert all(host[nm].tobytes() == t[nm].cpu().numpy().tobytes() for nm in host)
    assert {k: hs[k] for k in wr.STATS} == {k: ds[k] for k in wr.STATS} == {k: c["want"]["stats"][k] for k in wr.STATS}
    s = c["want"]["stats"]
    assert s["paths_bad"] == 1 and (h == 1 or (s["paths_ok"] == 6 and s["waypoints"] > 12 and s["cells_in"] > 40))


@pytest.mark.parametrize("name", binding.NAVPATH_OUTPUT_NAMES)
def test_one_host_output_alone_between_guard_bytes(name, fusion):
    """19 x 37, host arrays: every output on its own, all others NULL, equals the same array of the call that asks for all four, and
    the 256 bytes on either side of the caller's array are untouched"""
    c = staging_case(19, 37)
    if "every" not in c:
        c["every"] = waypoints_host(fusion, c, binding.NAVPATH_OUTPUT_NAMES)
    every, stats = c["every"]
    waypoints_same(every, c["want"], "every output")
    alone, st = waypoints_host(fusion, c, (name,))
    assert alone[name].tobytes() == every[name].tobytes() and {k: st[k] for k in wr.STATS} == {k: stats[k] for k in wr.STATS}, name


def test_the_staging_buffer_grows_and_is_used_again(drive_lib):
    """one handle: 8 x 8, 19 x 37, 8 x 8 again.  Each call gives what a handle that has made no other call gives"""
    f = handle(drive_lib)
    for h, w in ((8, 8), (19, 37), (8, 8)):
        c = staging_case(h, w)
        fresh = handle(drive_lib)
        (got, gs), (want, ws) = waypoints_host(f, c, binding.NAVPATH_OUTPUT_NAMES), waypoints_host(fresh, c, binding.NAVPATH_OUTPUT_NAMES)
        fresh.close()
        assert all(got[nm].tobytes() == want[nm].tobytes() for nm in got) and {k: gs[k] for k in wr.STATS} == {k: ws[k] for k in wr.STATS}, (h, w)
        waypoints_same(got, c["want"], (h, w))
    f.close()


def test_plan_and_refine_without_leaving_the_device(fusion):
    state, dist2 = pr.random_grid(64, 64, 23, obstacles=0.15)
    state[5, 5] = 0
    starts = np.concatenate([some_starts(64, 64, 6, 9), [(-1, 3)]]).astype(np.int32)
    plan = dict(min_dist2=1, soft_dist2=20, near_penalty=10, max_path=500)
    wq = dict(keep_clearance=1, clearance_cap=9, lookahead=64)
    got = fusion.nav_plan_waypoints(state, dist2, [(5, 5)], starts, plan=plan, waypoints=wq)
    host = fusion.nav_plan(state, dist2, [(5, 5)], starts, outputs=("start_cost", "start_status", "path_len", "path"), **plan)
    for k in ("start_cost", "start_status", "path_len"):
        assert (got["plan"][k] == host[k]).all() and got["plan"][k].dtype == host[k].dtype, k
    assert all((a == b).all() and a.shape == b.shape for a, b in zip(got["plan"]["path"], host["path"])) and host["start_status"][-1] == 1
    assert {k: got["plan"]["stats"][k] for k in pr.STATS} == {k: host["stats"][k] for k in pr.STATS}
    path, lens = wr.pack_paths(host["path"], max_path=500)
    ref, want = check(fusion, "plan to the host, then nav_waypoints", state, dist2, path, lens, min_dist2=1, max_waypoints=500, **wq)
    same(got["waypoints"], want, "nav_plan_waypoints")
    assert got["waypoints"]["stats"]["waypoints"] > 12 and got["waypoints"]["n_waypoints"][-1] == 0


# ---- no side effects, refusals, profiling -------------------------------------------------------------------------------------
def test_a_call_between_two_frames_changes_no_later_result(drive_lib):
    A, B = handle(drive_lib), handle(drive_lib)
    state, dist2, cells = wr.staircase(65, 2)
    for k in (0, 3, 6):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        A.nav_waypoints(state, dist2, [cells], keep_clearance=1, clearance_cap=20)
        A.nav_plan_waypoints(state, dist2, [tuple(cells[-1])], [tuple(cells[0])], waypoints=dict(los_dist2=3))
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)
    B.close()
    A.close()


def test_the_refusals(drive_lib):
    f = handle(drive_lib)
    state, dist2 = wr.open_grid(6, 9)
    cells = [np.array([(0, 0), (1, 1), (2, 2)], np.int32)]
    refused = pytest.raises(binding.SsfError, match=r"ssf_navpath_waypoints failed \(-1\)")
    for kw in (dict(min_dist2=-1), dict(los_dist2=-1), dict(keep_clearance=2), dict(keep_clearance=-1), dict(clearance_cap=-1),
               dict(clearance_cap=1024 * 1024 + 1), dict(lookahead=0), dict(lookahead=4097), dict(max_waypoints=0), dict(max_waypoints=(1 << 20) + 1)):
        with refused:
            f.nav_waypoints(state, dist2, cells, **kw)
    with refused:
        f.nav_waypoints(state, dist2, cells, outputs=())                  # every output NULL
    with refused:
        f.nav_waypoints(state, dist2, np.zeros((0, 3, 2), np.int32), np.zeros(0, np.int32))       # no path
    with refused:
        f.nav_waypoints(state, dist2, np.zeros((4097, 1, 2), np.int32), np.ones(4097, np.int32))
    with refused:
        f.nav_waypoints(np.zeros((1, 4097), np.int8), np.zeros((1, 4097), np.int32), cells)
    L, byref, vp = drive_lib.lib, binding.C.byref, binding.C.c_void_p
    p, st, out = binding.SsfNavPathParams(), binding.SsfNavPathStats(), binding.SsfNavPathOut()
    assert L.ssf_navpath_default_params(f.h, byref(p)) == 0
    assert L.ssf_navpath_default_params(None, byref(p)) == -1 and L.ssf_navpath_default_params(f.h, None) == -1
    assert f.nav_waypoints_default_params() == dict(width=512, height=512, min_dist2=0, allow_unknown=0, los_dist2=0, keep_clearance=0, clearance_cap=0,
                                                    lookahead=256, n_paths=0, max_path=0, max_waypoints=0, on_device=0)
    s8, d2 = np.ascontiguousarray(state), np.ascontiguousarray(dist2)
    path, lens = wr.pack_paths(cells)
    count = np.zeros(1, np.int32)
    p.width, p.height, p.n_paths, p.max_path, p.max_waypoints = 9, 6, 1, 3, 3
    out.n_waypoints = count.ctypes.data
    a, b, c, d = (x.ctypes.data_as(vp) for x in (s8, d2, path, lens))
    assert L.ssf_navpath_waypoints(f.h, byref(p), a, b, c, d, byref(out), None) == 0 and count[0] == 2      # stats are optional
    assert L.ssf_navpath_waypoints(None, byref(p), a, b, c, d, byref(out), byref(st)) == -1
    assert L.ssf_navpath_waypoints(f.h, None, a, b, c, d, byref(out), byref(st)) == -1
    assert L.ssf_navpath_waypoints(f.h, byref(p), None, b, c, d, byref(out), byref(st)) == -1
    assert L.ssf_navpath_waypoints(f.h, byref(p), a, None, c, d, byref(out), byref(st)) == -1
    assert L.ssf_navpath_waypoints(f.h, byref(p), a, b, None, d, byref(out), byref(st)) == -1
    assert L.ssf_navpath_waypoints(f.h, byref(p), a, b, c, None, byref(out), byref(st)) == -1
    assert L.ssf_navpath_waypoints(f.h, byref(p), a, b, c, d, None, byref(st)) == -1
    assert L.ssf_navpath_waypoints(f.h, byref(p), a, b, c, d, byref(binding.SsfNavPathOut()), byref(st)) == -1
    for field, bad in (("n_paths", 0), ("n_paths", -1), ("max_path", 0), ("max_path", (1 << 20) + 1), ("width", 0), ("height", -3), ("width", 4097)):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert L.ssf_navpath_waypoints(f.h, byref(p), a, b, c, d, byref(out), byref(st)) == -1, (field, bad)
        setattr(p, field, keep)
    # the handle keeps working: a call and a frame after the refusals
    check(f, "after the refusals", state, dist2, cells)
    f.process_frame(*util.frame(0, W, H))
    check(f, "after a frame", *wr.staircase(65, 1)[:2], [wr.staircase(65, 1)[2]], los_dist2=9)
    g = handle(drive_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_waypoints(state, dist2, cells)
    q = handle(drive_lib, pipeline_depth=2, extract_batch=2)
    q.submit_frame(*util.frame(0, W, H))
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q.nav_waypoints(state, dist2, cells)
    q.process_submitted()
    check(q, "pipelined, at rest", state, dist2, cells)
    q.close()
    g.close()
    f.close()


def test_the_kernels_are_timed_under_profile(drive_lib):
    f = handle(drive_lib, profile=1)
    f.reset_kernel_times()
    state, dist2, cells = wr.staircase(65, 5)
    check(f, "profiled", state, dist2, [cells], keep_clearance=1, clearance_cap=20)
    names = f.kernel_times()
    for k in ("navpath_pack", "navpath_check", "navpath_pull"):
        assert k in names and names[k][1] > 0, (k, names)
    f.close()


# ---- replay.py's files -----------------------------------------------------------------------------------------------------
def test_replay_writes_the_waypoints_next_to_the_plan(drive_lib, tmp_path):
    import json
    from supersurfel_fusion_amd import replay
    f = handle(drive_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    plan = dict(goals=[(12.0, 12.5)], frontier=True, radius=0.12)
    _, results = replay.replay(f, frames, nav_grid_dir=str(tmp_path), nav_grid_every=2, nav_grid_res=0.1, nav_grid_carve=True, nav_grid_carve_stride=4,
                               nav_plan=plan, nav_waypoints=dict(lookahead=32, los_radius=0.25))
    per_grid = [".pgm", ".yaml", "_cost.npy", "_dist2.npy", "_path.npy", "_plan.json", "_seen.npy", "_waypoints.json", "_waypoints.npy"]
    assert sorted(os.listdir(str(tmp_path))) == sorted("%06d%s" % (k, s) for k in (0, 2) for s in per_grid)
    grid = f.nav_grid_carve([r["pose"] for r in results], outputs=("state", "dist2"), carve=dict(stride=4), res=0.1)
    cells = np.load(str(tmp_path / "000002_path.npy"))
    kw = dict(min_dist2=4, los_dist2=9, keep_clearance=1, clearance_cap=9, lookahead=32)
    want = wr.waypoints(grid["state"], grid["dist2"], [cells], **kw)
    wp = np.load(str(tmp_path / "000002_waypoints.npy"))
    assert wp.dtype == np.int32 and wp.shape == want["waypoints"][0].shape and (wp == want["waypoints"][0]).all()
    told = json.load(open(str(tmp_path / "000002_waypoints.json")))
    assert {k: told[k] for k in wr.STATS} == want["stats"] and {k: told[k] for k in kw} == kw
    assert (told["status"], told["path_min"]) == (int(want["status"][0]), int(want["path_min"][0]))
    with pytest.raises(ValueError, match="nav_waypoints needs nav_plan"):
        replay.replay(f, [], nav_grid_dir=str(tmp_path), nav_waypoints=dict())
    f.close()


# ---- the C++ surface -----------------------------------------------------------------------------------------------------
def test_refine_paths_in_cpp(drive_lib, fusion, tmp_path):
    """tests/cpp/navpath_smoke.cpp on the GPU: its counts and FNV-1a checksums equal those of the Python calls on the same arrays"""
    libdir = os.path.dirname(drive_lib.path)
    exe = str(tmp_path / "navpath_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "navpath_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip_drive", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    names = ("ok", "bad", "truncated", "waypoints", "forced", "cells")
    got = re.search(r"navpath " + " ".join(nm + r"=(\d+)" for nm in names) + r" status=([0-9a-f]{16}) min=([0-9a-f]{16}) points=([0-9a-f]{16})", r.stdout)
    assert got and re.search(r"path start=\d+ poses=\d+ ok=1", r.stdout), r.stdout
    state, dist2 = pr.hashed_grid()
    goals, starts = [(3, 3), (66, 40), (70, 2), (35, 22)], [(0, 0), (69, 44), (20, 30), (-1, 4), (50, 10)]
    plan = fusion.nav_plan(state, dist2, goals, starts, outputs=("path",), min_dist2=1, allow_unknown=1, max_path=200)
    want, _ = check(fusion, "python waypoints", state, dist2, plan["path"], min_dist2=1, allow_unknown=1, keep_clearance=1, clearance_cap=9, lookahead=40)
    s = want["stats"]
    assert s["waypoints"] > 10 and s["paths_ok"] == 5 and s["forced_steps"] > 0
    counts = (s["paths_ok"], s["paths_bad"], s["paths_truncated"], s["waypoints"], s["forced_steps"], s["cells_in"])
    assert tuple(int(v) for v in got.groups()[:6]) == counts, (got.groups(), counts)
    hp = 1469598103934665603
    for wp in want["waypoints"]:
        hp = pr.fnv1a(np.ascontiguousarray(wp).tobytes(), hp)
    sums = (pr.fnv1a(want["status"].tobytes()), pr.fnv1a(want["path_min"].tobytes()), hp)
    assert tuple(int(v, 16) for v in got.groups()[6:]) == sums, (got.groups(), sums)
