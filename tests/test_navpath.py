"""The waypoints of the plan's paths (include/ssf_navpath.h) without a GPU: who exports the entry points, the header on its own, the
struct layouts of the binding, the C++ surface, replay.py's options, and the restatement the GPU tests compare against
(tests/navpath_ref.py): hand-written answers on grids of a dozen cells, a second formulation of the segment walk in exact fractions,
and properties of the waypoints on random grids."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import navpath_ref as wr
import navplan_ref as pr
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
U, F, X = -1, 0, 100


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


# ---- static checks -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drive_lib(product_lib):
    return binding.load_drive()


def test_the_drive_library_exports_the_waypoints_and_all_of_the_explore_library(drive_lib, product_lib, oracle_lib):
    """libssf_hip_drive.so = libssf_hip_explore.so's objects + ssf_navpath.hip; the four older tables hold no name of the waypoints"""
    have, explore = exported(drive_lib.path), exported(binding.EXPLORE_LIB)
    hip_ids = lambda names: {nm for nm in names if nm.startswith("__hip_cuid_")}         # one per translation unit, named by content
    for names in (binding.NAVPATH_SYMBOLS, binding.NAVFRONTIER_SYMBOLS, binding.NAVPLAN_SYMBOLS, binding.NAVCARVE_SYMBOLS, binding.ABI_SYMBOLS):
        assert set(names) <= have
    assert drive_lib.has_navpath and drive_lib.has_navfrontier and drive_lib.has_navplan and drive_lib.has_navcarve and drive_lib.has_navgrid
    assert drive_lib.has_raycast and drive_lib.backend == "hip-gfx950"
    assert explore - hip_ids(explore) <= have
    extra = have - explore - hip_ids(have)
    assert set(binding.NAVPATH_SYMBOLS) <= extra
    assert extra - set(binding.NAVPATH_SYMBOLS) == {nm for nm in extra if "k_navpath_" in nm}, sorted(extra)
    kernels = extra - set(binding.NAVPATH_SYMBOLS)
    assert all(any(k in nm for nm in kernels) for k in ("k_navpath_pack", "k_navpath_check", "k_navpath_pull"))
    for other in (exported(product_lib.path), exported(binding.NAVCARVE_LIB), exported(binding.NAV_LIB), explore, exported(oracle_lib.path)):
        assert not [nm for nm in other if "navpath" in nm]
    assert not product_lib.has_navpath and not binding.load_navcarve().has_navpath and not binding.load_nav().has_navpath
    assert not binding.load_explore().has_navpath and not oracle_lib.has_navpath


def test_an_oracle_backed_fusion_names_the_missing_symbol(oracle_lib):
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    state, dist2 = np.zeros((3, 3), np.int8), np.zeros((3, 3), np.int32)
    for call, symbol in ((lambda: f.nav_waypoints(state, dist2, [[(0, 0)]]), "ssf_navpath_waypoints"),
                         (lambda: f.nav_waypoints_device(None, None, 1, 1, None, None, 1, 1), "ssf_navpath_waypoints"),
                         (f.nav_waypoints_default_params, "ssf_navpath_default_params")):
        with pytest.raises(binding.SsfError, match=symbol):
            call()
    with pytest.raises(binding.SsfError, match="ssf_navplan_field|ssf_navpath_waypoints"):
        f.nav_plan_waypoints(state, dist2, [(1, 1)], [(0, 0)])


@pytest.mark.parametrize("load", ["load_product", "load_nav", "load_explore"])
def test_an_older_library_names_the_waypoints_symbol(load, product_lib):
    """the product, nav and explore libraries refine no path: the calls say which symbol is missing before anything runs"""
    lib = getattr(binding, load)()
    assert not lib.has_navpath
    f = binding.Fusion.__new__(binding.Fusion)                            # (no handle: the check comes before any call)
    f.L = lib
    state, dist2 = np.zeros((3, 3), np.int8), np.zeros((3, 3), np.int32)
    with pytest.raises(binding.SsfError, match="ssf_navpath_waypoints"):
        f.nav_waypoints(state, dist2, [[(0, 0)]])
    with pytest.raises(binding.SsfError, match="ssf_navpath_default_params"):
        f.nav_waypoints_default_params()
    with pytest.raises(binding.SsfError, match="ssf_navpath_waypoints" if lib.has_navplan else "ssf_navplan_field"):
        f.nav_plan_waypoints(state, dist2, [(1, 1)], [(0, 0)])


def test_the_waypoints_symbols_stay_out_of_the_other_headers():
    for nm in binding.NAVPATH_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        for hdr in ("ssf.h", "ssf_testing.h", "ssf_navgrid.h", "ssf_navcarve.h", "ssf_navplan.h", "ssf_navplan_testing.h", "ssf_navfrontier.h"):
            assert nm not in open(os.path.join(INCLUDE, hdr)).read(), (nm, hdr)
        assert nm + "(" in open(os.path.join(INCLUDE, "ssf_navpath.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_navpath.h"\n'
                   "int f(ssf_handle* h, const int8_t* state, const int32_t* dist2, const int32_t* path, const int32_t* len, int32_t* wp, int32_t* n) {\n"
                   "    ssf_navpath_params p; ssf_navpath_stats s; ssf_navpath_out o;\n"
                   "    if (ssf_navpath_default_params(h, &p) != SSF_OK) return -1;\n"
                   "    p.width = 64; p.height = 48; p.n_paths = 2; p.max_path = 100; p.max_waypoints = 10; p.los_dist2 = 4; p.keep_clearance = 1;\n"
                   "    o.n_waypoints = n; o.status = 0; o.waypoints = wp; o.path_min = 0;\n"
                   "    if (ssf_navpath_waypoints(h, &p, state, dist2, path, len, &o, &s) != SSF_OK) return -2;\n"
                   "    return (wp[2] & SSF_NAVPATH_FORCED) + (wp[2] & SSF_NAVPATH_INDEX_MASK) + (int)s.forced_steps + n[0]; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    classes = (("ssf_navpath_params", binding.SsfNavPathParams), ("ssf_navpath_out", binding.SsfNavPathOut), ("ssf_navpath_stats", binding.SsfNavPathStats))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_navpath.h"', "int main(void) {"]
    for st, cls in classes:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for nm, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, nm, st, nm))
    lines += ['    printf("forced %d\\n", SSF_NAVPATH_FORCED);', '    printf("mask %d\\n", SSF_NAVPATH_INDEX_MASK);', "    return 0; }"]
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
    assert int(got["forced"]) == binding.NAVPATH_FORCED == wr.FORCED == 1 << 30 and int(got["mask"]) == wr.INDEX_MASK
    assert tuple(nm for nm, _ in binding.SsfNavPathStats._fields_) == wr.STATS + ("segments_tested",)
    assert tuple(nm for nm, _ in binding.SsfNavPathParams._fields_)[2:8] == tuple(wr.DEFAULTS)
    assert tuple(nm for nm, _ in binding.SsfNavPathOut._fields_) == binding.NAVPATH_OUTPUT_NAMES


def test_ssf_hpp_waypoint_members_compile_and_link_against_the_drive_library(drive_lib, tmp_path):
    libdir = os.path.dirname(drive_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "navpath_smoke.cpp"),
           "-o", str(tmp_path / "navpath_smoke"), "-L", libdir, "-lssf_hip_drive", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_replay_options_parse():
    base = ["--npz", "frames.npz", "--nav-grid-dir", "grids"]
    a = replay.parse_args(base + ["--nav-plan-goal", "1.5", "-2", "--nav-plan-waypoints", "--nav-plan-lookahead", "64", "--nav-plan-los-radius", "0.3"])
    assert replay.nav_waypoints_of(a) == dict(lookahead=64, los_radius=0.3) and replay.nav_plan_of(a) == dict(goals=[(1.5, -2.0)], frontier=False, radius=0.0)
    b = replay.parse_args(base + ["--nav-plan-frontier", "--nav-plan-waypoints"])
    assert replay.nav_waypoints_of(b) == dict(lookahead=256, los_radius=0.0)
    assert replay.nav_waypoints_of(replay.parse_args(base + ["--nav-plan-frontier"])) is None
    for bad in (["--nav-plan-waypoints"], ["--nav-plan-frontier", "--nav-plan-lookahead", "3"], ["--nav-plan-frontier", "--nav-plan-los-radius", "0.1"],
                ["--nav-plan-frontier", "--nav-plan-waypoints", "--nav-plan-lookahead", "0"],
                ["--nav-plan-frontier", "--nav-plan-waypoints", "--nav-plan-lookahead", "4097"],
                ["--nav-plan-frontier", "--nav-plan-waypoints", "--nav-plan-los-radius", "-0.5"]):
        with pytest.raises(SystemExit):
            replay.parse_args(base + bad)
    with pytest.raises(SystemExit):                                      # without a grid directory there is no plan either
        replay.parse_args(["--npz", "frames.npz", "--nav-plan-frontier", "--nav-plan-waypoints"])
    with pytest.raises(ValueError, match="nav_waypoints needs nav_plan"):
        replay.replay(None, [], nav_grid_dir="grids", nav_waypoints=dict(lookahead=8))


def test_the_restatements_defaults_are_the_headers():
    hdr = open(os.path.join(INCLUDE, "ssf_navpath.h")).read()
    for text in ("min_dist2 0, allow_unknown 0, los_dist2 0, keep_clearance 0, clearance_cap 0, lookahead 256", "design choices, not tuned values",
                 "bit 30 (SSF_NAVPATH_FORCED) set on a forced step", "e += 2 dx - 2 dy; n -= 2", "max(base, min(clearance_cap, min over a <= i <= j of d(p_i)))"):
        assert text in hdr, text
    assert wr.DEFAULTS == dict(min_dist2=0, allow_unknown=0, los_dist2=0, keep_clearance=0, clearance_cap=0, lookahead=256)


# ---- hand-written answers ------------------------------------------------------------------------------------------------------
def points(state, dist2, cells, **kw):
    got = wr.waypoints(np.array(state, np.int8), np.array(dist2, np.int32), [np.array(cells, np.int32)], **kw)
    return got["waypoints"][0].tolist(), int(got["status"][0]), got


def test_a_straight_run_and_a_staircase_in_an_empty_grid_give_two_waypoints():
    state, dist2 = wr.open_grid(6, 9, 7)
    wp, status, got = points(state, dist2, [(x, 2) for x in range(9)])
    assert wp == [[0, 2, 0, 7], [8, 2, 8, 7]] and status == 0 and got["path_min"].tolist() == [7]
    assert got["stats"] == dict(paths_ok=1, paths_bad=0, paths_truncated=0, waypoints=2, forced_steps=0, cells_in=9)
    stairs = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2), (6, 3), (7, 3), (8, 4)]
    assert points(state, dist2, stairs)[0] == [[0, 0, 0, 7], [8, 4, 8, 7]]
    assert points(state, dist2, stairs, lookahead=3)[0] == [[0, 0, 0, 7], [3, 1, 3, 7], [6, 3, 6, 7], [8, 4, 8, 7]]
    assert points(state, dist2, [(4, 4)])[0] == [[4, 4, 0, 7]] and points(state, dist2, [])[0] == []
    assert points(state, dist2, [])[2]["path_min"].tolist() == [-1]


def test_an_l_around_one_wall_corner_gives_three():
    state = [[F, F, F, F, F],
             [F, F, F, F, F],
             [X, X, X, F, F],
             [F, F, F, F, F],
             [F, F, F, F, F]]
    dist2 = np.full((5, 5), 2, np.int32)
    cells = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (4, 2), (4, 3), (3, 4), (2, 4), (1, 4), (0, 4)]
    wp, status, _ = points(state, dist2, cells)
    # by hand: (0, 0) -> (4, 2) visits (1, 0), (1, 1), (2, 1), (3, 1), (3, 2): past the wall's end; (0, 0) -> (4, 3) visits (1, 0), (1, 1),
    # (2, 1), (2, 2): the wall.  From (4, 2) the walk to (0, 4) mirrors the first
    assert wp == [[0, 0, 0, 2], [4, 2, 5, 2], [0, 4, 10, 2]] and status == 0
    assert wr.walk(0, 0, 4, 2) == [(0, 0), (1, 0), (1, 1), (2, 1), (3, 1), (3, 2), (4, 2)] and (2, 2) in wr.walk(0, 0, 4, 3)


def test_two_diagonal_obstacles_that_share_a_corner_block_the_segment_through_it():
    state = [[F, X, F],
             [X, F, F],
             [F, F, F]]
    dist2 = np.ones((3, 3), np.int32)
    trav, d = wr.prep(np.array(state, np.int8), dist2, wr.params())
    assert wr.walk(0, 0, 1, 1) == [(0, 0), (1, 0), (0, 1), (1, 1)] and not wr.visible(trav, d, (0, 0), (1, 1), 0)
    assert wr.walk(0, 0, 2, 2) == [(0, 0), (1, 0), (0, 1), (1, 1), (2, 1), (1, 2), (2, 2)] and not wr.visible(trav, d, (0, 0), (2, 2), 0)
    # a path that cuts the corner is a valid input; its step is forced, and seg_min is over the four cells of the walk
    wp, status, got = points(state, [[5, 0, 5], [0, 5, 5], [5, 5, 5]], [(0, 0), (1, 1), (2, 2)])
    assert wp == [[0, 0, 0, 5], [1, 1, 1 | wr.FORCED, 0], [2, 2, 2, 5]] and status == 0 and got["stats"]["forced_steps"] == 1
    assert got["path_min"].tolist() == [0]
    one = [[F, X, F], [F, F, F], [F, F, F]]                               # one obstacle at the corner blocks it as well
    assert points(one, np.ones((3, 3), np.int32), [(0, 0), (1, 1)])[0][1][2] == 1 | wr.FORCED


def test_a_pillar_hides_the_nearer_candidates_and_the_farther_one_wins():
    state, dist2, cells, win = wr.pillar()
    assert cells.tolist() == [[0, 2], [1, 2], [2, 1], [3, 1], [4, 2], [5, 2], [5, 1], [5, 0]] and win == 7 and state[2, 3] == X
    trav, d = wr.prep(state, dist2, wr.params())
    seen = [wr.visible(trav, d, cells[0], c, 1) for c in cells]
    assert seen == [True, True, True, True, False, False, False, True]     # (4, 2), (5, 2), (5, 1) lie behind the pillar; (5, 0) is seen past it
    got = wr.waypoints(state, dist2, [cells], los_dist2=1)
    assert got["waypoints"][0].tolist() == [[0, 2, 0, 1], [5, 0, 7, 1]]
    first = wr.waypoints(state, dist2, [cells], los_dist2=1, lookahead=6)  # (5, 0) out of the window: the last cell seen is (3, 1)
    assert first["waypoints"][0].tolist() == [[0, 2, 0, 1], [3, 1, 3, 1], [5, 0, 7, 1]]


def test_clearance_thresholds_and_forced_steps():
    state = np.zeros((3, 7), np.int8)
    dist2 = np.array([[9, 9, 9, 9, 9, 9, 9], [9, 9, 9, 2, 9, 9, 9], [9, 9, 9, 9, 9, 9, 9]], np.int32)
    up = [(0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 1), (6, 1)]          # the path avoids the narrow cell (3, 1)
    assert points(state, dist2, up)[0] == [[0, 1, 0, 9], [6, 1, 6, 2]]      # nothing asks for clearance: straight through it
    assert points(state, dist2, up, los_dist2=3)[0] == [[0, 1, 0, 9], [3, 0, 3, 9], [6, 1, 6, 9]]
    assert points(state, dist2, up, keep_clearance=1, clearance_cap=9)[0] == [[0, 1, 0, 9], [3, 0, 3, 9], [6, 1, 6, 9]]
    assert points(state, dist2, up, keep_clearance=1, clearance_cap=2)[0] == [[0, 1, 0, 9], [6, 1, 6, 2]]     # the cap: 2 is enough
    through = [(x, 1) for x in range(7)]                                    # this path enters it: it keeps its own clearance, 2
    assert points(state, dist2, through, keep_clearance=1, clearance_cap=9)[0] == [[0, 1, 0, 9], [6, 1, 6, 2]]
    wp, _, got = points(state, dist2, through, los_dist2=3)                 # more than the path has: forced steps in and out of the cell
    assert wp == [[0, 1, 0, 9], [2, 1, 2, 9], [3, 1, 3 | wr.FORCED, 2], [4, 1, 4 | wr.FORCED, 2], [6, 1, 6, 9]] and got["stats"]["forced_steps"] == 2
    assert points(state, dist2, through, min_dist2=3)[1] == 2               # not traversable for this robot: the path is refused


def test_the_statuses_and_truncation():
    state = np.array([[F, F, F, U], [F, X, F, F]], np.int8)
    dist2 = np.array([[3, 3, 3, 3], [3, 0, 3, 3]], np.int32)
    path, lens = wr.pack_paths([[(0, 0), (1, 0), (2, 0)], [(0, 0), (1, 1)], [(0, 0), (2, 0)], [(0, 0), (0, 0)], [(2, 0), (3, 0)], [(0, 0), (4, 0)], [], [(0, 1)]])
    lens[7] = 4                                                          # longer than max_path = 3
    got = wr.waypoints(state, dist2, path, lens)
    assert got["status"].tolist() == [0, 2, 3, 3, 2, 2, 0, 1] and got["n_waypoints"].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
    assert got["stats"] == dict(paths_ok=2, paths_bad=6, paths_truncated=0, waypoints=2, forced_steps=0, cells_in=3)
    lens[7] = -1
    assert wr.waypoints(state, dist2, path, lens, allow_unknown=1)["status"].tolist() == [0, 2, 3, 3, 0, 2, 0, 1]
    jump_then_wall = wr.pack_paths([[(0, 0), (2, 0), (1, 1)]])           # status 3 and 2 both apply: the smaller wins
    assert wr.waypoints(state, dist2, *jump_then_wall)["status"].tolist() == [2]
    stairs = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2), (6, 3)]
    state, dist2 = wr.open_grid(4, 7, 1)
    full = wr.waypoints(state, dist2, [np.array(stairs)], lookahead=2)
    assert full["n_waypoints"].tolist() == [4] and full["status"].tolist() == [0]
    for mw, status in ((1, 4), (2, 4), (3, 4), (4, 0), (5, 0)):
        cut = wr.waypoints(state, dist2, [np.array(stairs)], lookahead=2, max_waypoints=mw)
        assert cut["status"].tolist() == [status] and (cut["waypoints"][0] == full["waypoints"][0][:mw]).all(), mw
        assert cut["stats"]["paths_truncated"] == (status == 4) and cut["stats"]["waypoints"] == min(mw, 4) and cut["stats"]["paths_ok"] == 1


# ---- the second formulation of the walk ------------------------------------------------------------------------------------------
def test_the_walk_against_exact_fractions():
    corners = 0
    for dx in range(-12, 13):
        for dy in range(-12, 13):
            cells = wr.walk(0, 0, dx, dy)
            assert cells[0] == (0, 0) and cells[-1] == (dx, dy) and len(set(cells)) == len(cells), (dx, dy)
            assert set(cells) == wr.walk_by_fractions(dx, dy), (dx, dy)
            assert all(min(0, dx) <= x <= max(0, dx) and min(0, dy) <= y <= max(0, dy) for x, y in cells)
            corners += len(cells) > abs(dx) + abs(dy) + 1
    assert corners > 100                                                 # many segments pass through a lattice corner
    assert set(wr.walk(5, -3, 9, 4)) == {(x + 5, y - 3) for x, y in wr.walk_by_fractions(4, 7)}
    assert set(wr.walk(9, 4, 5, -3)) == set(wr.walk(5, -3, 9, 4))


def test_long_walks_stay_in_the_bounding_box_and_end_at_the_far_cell():
    rng = np.random.default_rng(5)
    for dx, dy in [(4095, 4095), (4095, 1), (1, 4095), (-4095, 4094), (4095, -1365), (0, 4095), (-4095, 0)] + rng.integers(-4095, 4096, (40, 2)).tolist():
        cells = wr.walk(7, 9, 7 + dx, 9 + dy)
        assert cells[-1] == (7 + dx, 9 + dy) and len(cells) <= abs(dx) + abs(dy) + 1 + min(abs(dx), abs(dy))
        xs, ys = [c[0] for c in cells], [c[1] for c in cells]
        assert min(xs) == min(7, 7 + dx) and max(xs) == max(7, 7 + dx) and min(ys) == min(9, 9 + dy) and max(ys) == max(9, 9 + dy)


# ---- properties on random grids ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned():
    """paths planned by the plan's restatement on a random grid, shared by the property tests"""
    state, dist2 = pr.random_grid(45, 70, 11, obstacles=0.2, unknown=0.1)
    rng = np.random.default_rng(3)
    starts = np.stack([rng.integers(0, 70, 12), rng.integers(0, 45, 12)], 1)
    state[22, 35] = 0
    plan = pr.plan(state, dist2, [(35, 22)], starts, max_path=400)
    paths = [p for p in plan["path"] if len(p) > 1]
    assert len(paths) >= 6 and max(len(p) for p in paths) > 30
    return state, dist2, paths


KWS = [dict(), dict(lookahead=5), dict(los_dist2=6), dict(keep_clearance=1, clearance_cap=12), dict(keep_clearance=1, clearance_cap=40, los_dist2=2, lookahead=17)]


@pytest.mark.parametrize("kw", KWS, ids=["-".join("%s%d" % kv for kv in sorted(k.items())) or "defaults" for k in KWS])
def test_the_waypoints_are_an_increasing_subsequence_whose_unforced_segments_are_visible(kw, planned):
    state, dist2, paths = planned
    q = wr.params(**kw)
    got = wr.waypoints(state, dist2, paths, **kw)
    same = wr.waypoints(state, dist2, paths, every_candidate=True, **kw)     # step 5 as it is written: every candidate walked to its end
    trav, d = wr.prep(state, dist2, q)
    base = max(q["min_dist2"], q["los_dist2"])
    forced = 0
    for cells, wp, wp2, status in zip(paths, got["waypoints"], same["waypoints"], got["status"]):
        assert status == 0 and (wp == wp2).all()
        idx = wp[:, 2] & wr.INDEX_MASK
        assert idx[0] == 0 and idx[-1] == len(cells) - 1 and (np.diff(idx) > 0).all() and (np.diff(idx) <= q["lookahead"]).all()
        assert (wp[:, :2] == cells[idx]).all() and wp[0, 3] == d[cells[0][1]][cells[0][0]]
        for a, b, word, seg_min in zip(idx[:-1], idx[1:], wp[1:, 2], wp[1:, 3]):
            run = min(d[y][x] for x, y in cells[a:b + 1])
            thr = max(base, min(q["clearance_cap"], run)) if q["keep_clearance"] else base
            vis, m = wr.segment(trav, d, cells[a], cells[b], thr)
            assert m == seg_min and vis == (not word & wr.FORCED)
            assert vis or b == a + 1                                     # only a single step is ever forced
            forced += not vis
            if vis and q["keep_clearance"]:
                assert seg_min >= min(q["clearance_cap"], run)           # the shortcut keeps the clearance of the piece it replaces
    assert forced == got["stats"]["forced_steps"] and (forced > 0) == (q["los_dist2"] > 0)
    assert got["stats"]["waypoints"] == sum(len(w) for w in got["waypoints"]) < got["stats"]["cells_in"] == sum(len(p) for p in paths)


# ---- grids with values outside {0, -1, 100} and dist2 outside 0 .. the cap (the GPU file's foreign cases) ------------------------------
def test_what_the_waypoints_do_with_an_odd_state_or_dist2_by_hand():
    """a path over a cell of an odd state, or of negative dist2, is status 2 whether unknown cells are allowed or not; such a cell beside
    the path hides what lies behind it; d is max(dist2, 0), uncapped: INT32_MAX stays INT32_MAX"""
    row = np.array([(x, 0) for x in range(5)], np.int32)
    for allow in (0, 1):
        for odd in pr.ODD_STATES:
            state, dist2 = wr.open_grid(2, 5, 7)
            state[0, 2] = odd
            got = wr.waypoints(state, dist2, [row, row[:2]], allow_unknown=allow)
            assert got["status"].tolist() == [2, 0] and got["n_waypoints"].tolist() == [0, 2] and got["path_min"].tolist() == [-1, 7], (odd, allow)
            round_it = np.array([(0, 0), (1, 1), (2, 1), (3, 1), (4, 0)], np.int32)      # the straight line back crosses the odd cell
            got = wr.waypoints(state, dist2, [round_it], allow_unknown=allow)
            assert got["status"].tolist() == [0] and got["n_waypoints"][0] > 2 and got["stats"]["forced_steps"] == 0
        state, dist2 = wr.open_grid(2, 5, 7)
        dist2[0, 2] = -3
        assert wr.waypoints(state, dist2, [row], allow_unknown=allow)["status"].tolist() == [2]
    state, dist2 = wr.open_grid(1, 5, (1 << 31) - 1)
    got = wr.waypoints(state, dist2, [row], keep_clearance=1, clearance_cap=1 << 20)
    assert got["waypoints"][0].tolist() == [[0, 0, 0, (1 << 31) - 1], [4, 0, 4, (1 << 31) - 1]] and got["path_min"].tolist() == [(1 << 31) - 1]


@pytest.mark.parametrize("h,w", pr.FOREIGN_SIZES)
@pytest.mark.parametrize("allow", [0, 1])
def test_the_foreign_grids_odd_values_decide_the_waypoints(h, w, allow):
    f = pr.foreign_case(h, w, allow)
    state, dist2, paths = f["state"], f["dist2"], f["plan"]["path"]
    assert sum(len(p) > 10 for p in paths) >= 2
    kw = dict(allow_unknown=allow, keep_clearance=1, clearance_cap=12, los_dist2=2)
    got = wr.waypoints(state, dist2, paths, **kw)
    assert (got["status"] == 0).all() and got["stats"]["waypoints"] > 2 * len(paths)
    plain_state, plain_dist2 = pr.plain_grid(state, dist2)
    fewer = wr.waypoints(plain_state, dist2, paths, **kw)                 # with the odd cells free, more is seen: fewer waypoints
    assert fewer["stats"]["waypoints"] < got["stats"]["waypoints"]
    other = wr.waypoints(state, np.where(dist2 < 0, 40, dist2), paths, **kw)        # likewise the cells of negative dist2
    assert other["stats"]["waypoints"] < got["stats"]["waypoints"]
