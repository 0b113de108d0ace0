"""The plan on the navigation grid (include/ssf_navplan.h) without a GPU: who exports the entry points, the header on its own, the
struct layouts of the binding, the C++ surface, replay.py's options, and the restatement the GPU tests compare against
(tests/navplan_ref.py): hand-written answers, a second formulation (whole-grid Bellman-Ford sweeps) and a third (the device's tile
rounds, run one tile after the other in shuffled order)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import navplan_ref as pr
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
INF = pr.INF


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


# ---- static checks -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nav_lib(product_lib):
    return binding.load_nav()


def test_the_nav_library_exports_the_plan_the_carve_and_all_of_the_product(nav_lib, product_lib, oracle_lib):
    """libssf_hip_nav.so = the product's objects + ssf_navcarve.hip + ssf_navplan.hip; the other libraries' tables stay what they
    were (tests/test_math.py and tests/test_navcarve.py pin them) and hold no name of the plan"""
    have, product, carve = exported(nav_lib.path), exported(product_lib.path), exported(binding.NAVCARVE_LIB)
    hip_ids = lambda names: {nm for nm in names if nm.startswith("__hip_cuid_")}         # one per translation unit, named by content
    assert set(binding.NAVPLAN_SYMBOLS) <= have and set(binding.NAVCARVE_SYMBOLS) <= have and set(binding.ABI_SYMBOLS) <= have
    assert nav_lib.has_navplan and nav_lib.has_navcarve and nav_lib.has_navgrid and nav_lib.has_raycast and nav_lib.backend == "hip-gfx950"
    assert product - hip_ids(product) <= have and carve - hip_ids(carve) <= have
    extra = have - carve - hip_ids(have)
    assert extra - set(binding.NAVPLAN_SYMBOLS) == {nm for nm in extra if "k_navplan_" in nm}, sorted(extra)
    for other in (product, carve, exported(oracle_lib.path)):
        assert not [nm for nm in other if "navplan" in nm]
    carve_lib = binding.load_navcarve()
    assert not product_lib.has_navplan and not carve_lib.has_navplan and not oracle_lib.has_navplan
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    for call, symbol in ((lambda: f.nav_plan(None, None), "ssf_navplan_field"), (lambda: f.nav_plan_device(None, None, 1, 1), "ssf_navplan_field"),
                         (lambda: f.nav_plan_from_map(None), "ssf_navplan_field"), (f.nav_plan_default_params, "ssf_navplan_default_params"),
                         (lambda: f.debug_navplan_set_round_batch(1), "ssf_debug_navplan_set_round_batch"),
                         (f.debug_navplan_last, "ssf_debug_navplan_last")):
        with pytest.raises(binding.SsfError, match=symbol):
            call()


def test_the_plan_symbols_stay_out_of_ssf_h():
    for nm in binding.NAVPLAN_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        for hdr in ("ssf.h", "ssf_testing.h", "ssf_navgrid.h", "ssf_navcarve.h"):
            assert nm not in open(os.path.join(INCLUDE, hdr)).read(), (nm, hdr)
        assert (nm + "(" in open(os.path.join(INCLUDE, "ssf_navplan.h")).read()) != nm.startswith("ssf_debug_")      # the hooks: a header of their own
        assert (nm + "(" in open(os.path.join(INCLUDE, "ssf_navplan_testing.h")).read()) == nm.startswith("ssf_debug_")
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_navplan.h"\n'
                   '#include "ssf_navplan_testing.h"\n'
                   "int f(ssf_handle* h, const int8_t* state, const int32_t* dist2, const int32_t* goals, uint32_t* cost) {\n"
                   "    ssf_navplan_params p; ssf_navplan_stats s; ssf_navplan_out o; int64_t rounds, visits;\n"
                   "    if (ssf_navplan_default_params(h, &p) != SSF_OK || ssf_debug_navplan_set_round_batch(h, 4) != SSF_OK) return -1;\n"
                   "    p.width = 64; p.height = 48; p.goals = goals; p.n_goals = 2; p.min_dist2 = 4;\n"
                   "    o.cost = cost; o.frontier = 0; o.start_cost = 0; o.start_status = 0; o.path_len = 0; o.path = 0;\n"
                   "    if (ssf_navplan_field(h, &p, state, dist2, &o, &s) != SSF_OK || cost[0] == SSF_NAVPLAN_UNREACHED) return -2;\n"
                   "    return ssf_debug_navplan_last(h, &rounds, &visits) + (int)s.cells_reached + (int)rounds; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    classes = (("ssf_navplan_params", binding.SsfNavPlanParams), ("ssf_navplan_out", binding.SsfNavPlanOut),
               ("ssf_navplan_stats", binding.SsfNavPlanStats))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_navplan.h"', "int main(void) {"]
    for st, cls in classes:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for nm, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, nm, st, nm))
    lines += ["    return 0; }"]
    src = tmp_path / "off.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "off")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict(l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    for st, cls in classes:
        assert int(got[st]) == C.sizeof(cls), st
        for nm, _ in cls._fields_:
            assert int(got["%s.%s" % (st, nm)]) == getattr(cls, nm).offset, (st, nm)
    assert tuple(nm for nm, _ in binding.SsfNavPlanStats._fields_) == pr.STATS + ("rounds", "tile_visits")
    assert binding.NAVPLAN_UNREACHED == INF


def test_ssf_hpp_plan_members_compile_and_link_against_the_nav_library(nav_lib, tmp_path):
    libdir = os.path.dirname(nav_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "navplan_smoke.cpp"),
           "-o", str(tmp_path / "navplan_smoke"), "-L", libdir, "-lssf_hip_nav", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_replay_options_parse():
    a = replay.parse_args(["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-plan-goal", "1.5", "-2", "--nav-plan-goal", "0", "3",
                           "--nav-plan-radius", "0.12"])
    assert replay.nav_plan_of(a) == dict(goals=[(1.5, -2.0), (0.0, 3.0)], frontier=False, radius=0.12)
    b = replay.parse_args(["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-plan-frontier"])
    assert replay.nav_plan_of(b) == dict(goals=[], frontier=True, radius=0.0)
    assert replay.nav_plan_of(replay.parse_args(["--npz", "frames.npz", "--nav-grid-dir", "grids"])) is None
    for bad in (["--nav-plan-frontier"], ["--nav-plan-goal", "1", "2"], ["--nav-grid-dir", "grids", "--nav-plan-radius", "0.2"],
                ["--nav-grid-dir", "grids", "--nav-plan-frontier", "--nav-plan-radius", "-1"]):
        with pytest.raises(SystemExit):
            replay.parse_args(["--npz", "frames.npz"] + bad)
    # the camera's cell and the goals' cells: the default grid frame (x = map x, y = map z), cells of 0.05 m
    pose = np.array([1, 0, 0, 0, 0, -1, 0, 1, 0, -1, 0, -2], np.float32)
    start, goals = replay.plan_cells(pose, 0.05, (0.3, 0.1, 0.0), [(1.0, 2.0), (-0.01, 0.0)])
    assert start.tolist() == [[26, 40]] and goals.tolist() == [[20, 40], [-1, 0]]


def test_the_restatements_defaults_are_the_headers():
    hdr = open(os.path.join(INCLUDE, "ssf_navplan.h")).read()
    for text in ("min_dist2 0, soft_dist2 0, near_penalty 0, allow_unknown 0", "goals_from_frontier 0", "max_path 0, on_device 0",
                 "dist2 is capped at the grid's max_dist_cells^2", "no corner cutting", "ties to the smallest k"):
        assert text in hdr, text
    assert pr.DEFAULTS == dict(min_dist2=0, soft_dist2=0, near_penalty=0, allow_unknown=0, goals_from_frontier=0, max_path=0)
    assert pr.DIRS == ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1)) and pr.WEIGHT == (10,) * 4 + (14,) * 4


# ---- hand-written answers ------------------------------------------------------------------------------------------------------
def test_no_diagonal_across_a_blocked_corner():
    state, dist2 = pr.open_grid(3, 3)
    state[1, 1] = 100
    got = pr.plan(state, dist2, [(1, 0)], [(0, 1), (2, 1), (1, 2), (1, 1)], max_path=9)
    want = np.array([[10, 0, 10], [20, INF, 20], [30, 40, 30]], np.uint32)       # (0, 1) -> (1, 0) goes round the corner: 10 + 10
    assert np.array_equal(got["cost"], want)
    assert got["start_status"].tolist() == [0, 0, 0, 2] and got["start_cost"].tolist() == [20, 20, 40, INF]
    assert got["path"][0].tolist() == [[0, 1], [0, 0], [1, 0]] and got["path"][1].tolist() == [[2, 1], [2, 0], [1, 0]]
    assert got["path"][2].tolist() == [[1, 2], [2, 2], [2, 1], [2, 0], [1, 0]]      # k = 0 (+1, 0) before k = 2 (-1, 0)
    state[1, 1] = 0
    open3 = pr.plan(state, dist2, [(1, 0)])
    assert np.array_equal(open3["cost"], np.array([[10, 0, 10], [14, 10, 14], [24, 20, 24]], np.uint32))
    s = got["stats"]
    assert (s["cells_traversable"], s["cells_reached"], s["max_cost"], s["goals_used"]) == (8, 8, 40, 1)


def test_a_corridor_of_one_row():
    state, dist2 = pr.open_grid(1, 9)
    got = pr.plan(state, dist2, [(6, 0)], [(0, 0), (8, 0)], max_path=5)
    assert got["cost"].tolist() == [[60, 50, 40, 30, 20, 10, 0, 10, 20]]
    assert got["start_status"].tolist() == [4, 0] and got["path_len"].tolist() == [5, 3]
    assert got["path"][0].tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [4, 0]] and got["path"][1].tolist() == [[8, 0], [7, 0], [6, 0]]
    state[0, 3] = 100
    cut = pr.plan(state, dist2, [(6, 0)], [(0, 0)], max_path=5)
    assert cut["cost"].tolist() == [[INF, INF, INF, INF, 20, 10, 0, 10, 20]] and cut["start_status"].tolist() == [3] and cut["path_len"].tolist() == [0]


def test_the_penalty_formula():
    soft, near = 30, 25
    state = np.zeros((1, 5), np.int8)
    dist2 = np.array([[0, soft - 1, soft, soft + 7, 1]], np.int32)
    _, pen, _ = pr.prep(state, dist2, pr.params(soft_dist2=soft, near_penalty=near))
    assert pen.tolist() == [[25, 25 * 1 // 30, 0, 0, 25 * 29 // 30]] == [[25, 0, 0, 0, 24]]
    _, none, _ = pr.prep(state, dist2, pr.params(soft_dist2=0, near_penalty=near))
    assert not none.any()
    got = pr.plan(state, dist2, [(2, 0)], soft_dist2=soft, near_penalty=near)
    assert got["cost"].tolist() == [[20, 10, 0, 10, 20]]                 # entering q costs w + pen[q], and no cell on these ways has one
    back = pr.plan(state, dist2, [(4, 0)], soft_dist2=soft, near_penalty=near)
    assert back["cost"].tolist() == [[64, 54, 44, 34, 0]]                # the last move enters the goal (4, 0), whose penalty is 24
    assert pr.plan(state, dist2, [(0, 0)], soft_dist2=soft, near_penalty=near)["cost"].tolist() == [[0, 35, 45, 55, 65]]
    trav, _, _ = pr.prep(state, dist2, pr.params(min_dist2=1))
    assert trav.tolist() == [[False, True, True, True, True]]


def test_the_penalty_is_paid_on_entering_a_cell():
    state = np.zeros((1, 3), np.int8)
    dist2 = np.array([[9, 0, 9]], np.int32)
    got = pr.plan(state, dist2, [(0, 0)], soft_dist2=4, near_penalty=8)
    assert got["cost"].tolist() == [[0, 10, 28]]                         # (1, 0) -> goal: 10 + 0; (2, 0) -> (1, 0): 10 + 8, then 10


def test_the_frontier_at_the_grids_edge():
    state = np.array([[0, 0, -1], [0, 100, 0], [-1, 0, 0]], np.int8)
    dist2 = np.full((3, 3), 9, np.int32)
    _, _, fr = pr.prep(state, dist2, pr.params())
    assert fr.tolist() == [[0, 1, 0], [1, 0, 1], [0, 1, 0]]              # 4-neighbours only, none across the edge, an obstacle is none
    got = pr.plan(state, dist2, None, goals_from_frontier=1)
    assert got["stats"]["frontier_cells"] == got["stats"]["frontier_goals"] == 4 and got["cost"][0, 0] == 10 and got["cost"][2, 2] == 10
    blocked = pr.plan(state, np.where(np.arange(9).reshape(3, 3) == 1, 0, 9).astype(np.int32), None, goals_from_frontier=1, min_dist2=1)
    assert blocked["stats"]["frontier_cells"] == 4 and blocked["stats"]["frontier_goals"] == 3 and blocked["cost"][0, 1] == INF
    alone = np.zeros((1, 1), np.int8)
    assert pr.prep(alone, np.zeros((1, 1), np.int32), pr.params())[2].tolist() == [[0]]


def test_goals_are_counted_per_entry():
    state, dist2 = pr.open_grid(4, 6)
    state[2, 2] = 100
    state[0, 5] = -1
    got = pr.plan(state, dist2, [(1, 1), (1, 1), (6, 0), (0, 4), (-1, 2), (2, 2), (5, 0), (5, 3)])
    s = got["stats"]
    assert (s["goals_used"], s["goals_blocked"], s["goals_outside"], s["frontier_goals"]) == (3, 2, 3, 0)
    assert got["cost"][1, 1] == 0 and got["cost"][3, 5] == 0 and got["cost"][0, 5] == INF


def test_the_tie_break_on_an_open_grid():
    state, dist2 = pr.open_grid(8, 8)
    got = pr.plan(state, dist2, [(5, 2)], [(0, 0)], max_path=64)
    assert got["start_cost"].tolist() == [58]
    assert got["path"][0].tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [4, 1], [5, 2]]       # k = 0 wins every tie against k = 4


# ---- the other formulations ----------------------------------------------------------------------------------------------
SCENES = [("random 45 x 70 with penalties", lambda: pr.random_grid(45, 70, 3), [(3, 3), (60, 40), (35, 20)], dict(soft_dist2=30, near_penalty=40, min_dist2=2)),
          ("random 33 x 31 with unknown", lambda: pr.random_grid(33, 31, 5, unknown=0.15), [(0, 0)], dict(allow_unknown=1, goals_from_frontier=1)),
          ("serpentine 40", lambda: pr.serpentine(40), [(0, 0)], dict()),
          ("door on a tile corner", lambda: pr.wall_with_door(64, 64, wall_x=32, door=31), [(2, 60)], dict())]


@pytest.mark.parametrize("name,make,goals,kw", SCENES, ids=[s[0] for s in SCENES])
def test_dijkstra_agrees_with_bellman_ford_sweeps_and_with_tile_rounds(name, make, goals, kw):
    state, dist2 = make()
    q = pr.params(**kw)
    trav, pen, frontier = pr.prep(state, dist2, q)
    goal, _ = pr.goal_cells(trav, frontier, goals, q)
    want = pr.field(trav, pen, goal)
    assert (want != INF).sum() > 20 and goal.any(), name
    swept, sweeps = pr.field_by_sweeps(trav, pen, goal)
    assert np.array_equal(swept, want) and sweeps > 5, name
    rng = np.random.default_rng(11)
    shuffled = lambda r, tiles: [tiles[i] for i in rng.permutation(len(tiles))]
    for order, stale in ((None, False), (shuffled, False), (shuffled, True), (lambda r, tiles: tiles[::-1], True)):
        got, rounds, visits = pr.field_by_tile_rounds(trav, pen, goal, order, stale)
        assert np.array_equal(got, want), (name, stale)
        assert 1 <= rounds <= visits and rounds <= trav.size + 1, (name, rounds, visits)
    # every path runs down the field to a goal, one admissible move at a time (trace asserts the minimum = the cost at every step)
    ys, xs = np.nonzero(want != INF)
    for i in range(0, len(xs), max(1, len(xs) // 25)):
        status, c, path = pr.trace(want, trav, pen, (xs[i], ys[i]), trav.size)
        assert status == 0 and c == want[ys[i], xs[i]] and goal[path[-1][1], path[-1][0]]


def test_a_goal_on_a_tile_edge_wakes_the_neighbour_tile():
    """the goal's own tile lowers nothing on that edge, so whoever sets the goal flags the tiles that see it"""
    state, dist2 = pr.open_grid(40, 70)
    q = pr.params()
    trav, pen, frontier = pr.prep(state, dist2, q)
    for cell in ((31, 5), (32, 5), (31, 31), (32, 32), (63, 39)):
        goal, _ = pr.goal_cells(trav, frontier, [cell], q)
        got, rounds, _ = pr.field_by_tile_rounds(trav, pen, goal, stale=True)
        assert np.array_equal(got, pr.field(trav, pen, goal)), cell


# ---- grids with values outside {0, -1, 100} and dist2 outside 0 .. the cap (the GPU files' foreign cases) -------------------------------
def test_what_the_plan_does_with_an_odd_state_or_a_negative_dist2_by_hand():
    """only 0 is free and only -1 is unknown, whatever allow_unknown; a negative dist2 is below min_dist2 = 0 and pays the full penalty"""
    for allow in (0, 1):
        for odd in pr.ODD_STATES:
            state, dist2 = pr.open_grid(1, 5)
            state[0, 2] = odd                                            # a corridor of one row with the odd cell in the way
            got = pr.plan(state, dist2, [(4, 0)], [(0, 0), (2, 0), (3, 0)], allow_unknown=allow, max_path=9)
            assert got["start_status"].tolist() == [3, 2, 0] and got["stats"]["cells_reached"] == 2 and got["stats"]["frontier_cells"] == 0, (odd, allow)
        state, dist2 = pr.open_grid(1, 5)
        dist2[0, 2] = -1
        assert pr.plan(state, dist2, [(4, 0)], [(0, 0)], allow_unknown=allow)["start_status"].tolist() == [3]
    state, dist2 = pr.open_grid(1, 3)
    dist2[0, 1] = (1 << 31) - 1                                          # far above soft_dist2: no penalty
    assert pr.plan(state, dist2, [(2, 0)], [(0, 0)], soft_dist2=30, near_penalty=40)["start_cost"].tolist() == [20]
    state[0, 1], dist2[0, 1] = -1, -(1 << 31)                            # unknown and allowed, but its dist2 is negative
    assert pr.plan(state, dist2, [(2, 0)], [(0, 0)], allow_unknown=1)["start_status"].tolist() == [3]
    assert pr.prep(state, dist2, pr.params(soft_dist2=30, near_penalty=40))[1][0, 1] == 40


@pytest.mark.parametrize("h,w", pr.FOREIGN_SIZES)
@pytest.mark.parametrize("allow", [0, 1])
def test_the_foreign_grids_odd_values_decide_the_plan(h, w, allow):
    f = pr.foreign_case(h, w, allow)
    state, dist2, got = f["state"], f["dist2"], f["plan"]
    assert set(np.unique(state).tolist()) == set(pr.ODD_STATES) | {0, -1, 100} and set(pr.ODD_DIST2) <= set(np.unique(dist2).tolist())
    assert (w + 31) // 32 == 3 and (h + 31) // 32 == 2
    s = got["stats"]
    assert s["cells_reached"] > h * w // 3 and (got["start_status"] == 0).sum() >= 2 and max(got["path_len"]) > 10 and s["frontier_cells"] > 100
    assert f["frontier_plan"]["stats"]["frontier_goals"] > 100 and (f["frontier_plan"]["start_status"] == 0).any()
    reached = np.pad(got["cost"] != pr.INF, 1, constant_values=False)
    beside = reached[1:-1, 2:] | reached[1:-1, :-2] | reached[2:, 1:-1] | reached[:-2, 1:-1]          # a reached 4-neighbour
    for odd in pr.ODD_STATES:                                            # every odd state stands in the field's way somewhere
        assert ((state == odd) & beside & (got["cost"] == pr.INF)).any(), odd
    assert ((state == 0) & (dist2 < 0) & beside & ~got["trav"]).any()    # a free cell of negative dist2 does
    # taken for plain values, the same grid plans otherwise: a shorter path where a cell of state 50 stood
    plain_state, plain_dist2 = pr.plain_grid(state, dist2)
    fifty = np.where(state == 50, 0, state).astype(np.int8)
    other = pr.plan(fifty, dist2, f["goals"], f["starts"], **f["kw"])
    ok = (got["start_status"] == 0) & (other["start_status"] == 0)
    assert (other["start_cost"][ok] < got["start_cost"][ok]).any() or (other["start_status"] == 0).sum() > (got["start_status"] == 0).sum()
    assert (pr.plan(plain_state, dist2, f["goals"], **f["kw"])["cost"] != got["cost"]).any()
    assert (pr.plan(state, plain_dist2, f["goals"], **f["kw"])["cost"] != got["cost"]).any()
    # a cell of state -2 or -128 beside a free cell makes no frontier; taken for unknown it would
    minus = np.where((state == -2) | (state == -128), -1, state).astype(np.int8)
    more = pr.prep(minus, dist2, pr.params(**f["kw"]))[2]
    assert (more >= got["frontier"]).all() and int(more.sum()) > int(got["frontier"].sum())
