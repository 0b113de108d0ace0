"""The frontier regions of the navigation grid (include/ssf_navfrontier.h) without a GPU: who exports the entry points, the header on
its own, the struct layouts of the binding, the C++ surface, replay.py's options, and the restatement the GPU tests compare against
(tests/navfrontier_ref.py): hand-written answers on grids of a dozen cells and a second formulation (a union-find over cell pairs
for the regions, one list per ray with len(set(...)) for the gain)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import navfrontier_ref as fr
import navplan_ref as pr
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
INF = fr.INF


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


# ---- static checks -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def explore_lib(product_lib):
    return binding.load_explore()


def test_the_explore_library_exports_the_regions_and_all_of_the_nav_library(explore_lib, product_lib, oracle_lib):
    """libssf_hip_explore.so = libssf_hip_nav.so's objects + ssf_navfrontier.hip; the three older tables hold no name of the regions"""
    have, nav = exported(explore_lib.path), exported(binding.NAV_LIB)
    hip_ids = lambda names: {nm for nm in names if nm.startswith("__hip_cuid_")}         # one per translation unit, named by content
    for names in (binding.NAVFRONTIER_SYMBOLS, binding.NAVPLAN_SYMBOLS, binding.NAVCARVE_SYMBOLS, binding.ABI_SYMBOLS):
        assert set(names) <= have
    assert explore_lib.has_navfrontier and explore_lib.has_navplan and explore_lib.has_navcarve and explore_lib.has_navgrid
    assert explore_lib.has_raycast and explore_lib.backend == "hip-gfx950"
    assert nav - hip_ids(nav) <= have
    extra = have - nav - hip_ids(have)
    assert set(binding.NAVFRONTIER_SYMBOLS) <= extra
    assert extra - set(binding.NAVFRONTIER_SYMBOLS) == {nm for nm in extra if "k_navfrontier_" in nm}, sorted(extra)
    assert len(extra - set(binding.NAVFRONTIER_SYMBOLS)) >= 8
    for other in (exported(product_lib.path), exported(binding.NAVCARVE_LIB), nav, exported(oracle_lib.path)):
        assert not [nm for nm in other if "navfrontier" in nm]
    assert not product_lib.has_navfrontier and not binding.load_navcarve().has_navfrontier and not binding.load_nav().has_navfrontier
    assert not oracle_lib.has_navfrontier


def test_an_oracle_backed_fusion_names_the_missing_symbol(oracle_lib):
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    state = np.zeros((3, 3), np.int8)
    for call, symbol in ((lambda: f.nav_frontiers(state), "ssf_navfrontier_regions"), (lambda: f.nav_frontiers_device(None, 1, 1), "ssf_navfrontier_regions"),
                         (f.nav_frontiers_default_params, "ssf_navfrontier_default_params")):
        with pytest.raises(binding.SsfError, match=symbol):
            call()
    with pytest.raises(binding.SsfError, match="ssf_navplan_field|ssf_navfrontier_regions"):
        f.nav_explore(state, np.zeros((3, 3), np.int32), (1, 1))


def test_a_nav_backed_fusion_names_the_regions_symbol_in_nav_explore(product_lib):
    """the nav library plans but groups no frontier: nav_explore says which symbol is missing before it plans"""
    nav = binding.load_nav()
    assert nav.has_navplan and not nav.has_navfrontier
    f = binding.Fusion.__new__(binding.Fusion)                            # (no handle: the check comes before any call)
    f.L = nav
    with pytest.raises(binding.SsfError, match="ssf_navfrontier_regions"):
        f.nav_explore(np.zeros((3, 3), np.int8), np.zeros((3, 3), np.int32), (1, 1))


def test_the_regions_symbols_stay_out_of_the_other_headers():
    for nm in binding.NAVFRONTIER_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        for hdr in ("ssf.h", "ssf_testing.h", "ssf_navgrid.h", "ssf_navcarve.h", "ssf_navplan.h", "ssf_navplan_testing.h"):
            assert nm not in open(os.path.join(INCLUDE, hdr)).read(), (nm, hdr)
        assert nm + "(" in open(os.path.join(INCLUDE, "ssf_navfrontier.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_navfrontier.h"\n'
                   "int f(ssf_handle* h, const int8_t* state, const uint32_t* cost, int32_t* region, ssf_navfrontier_region* table, int32_t* order) {\n"
                   "    ssf_navfrontier_params p; ssf_navfrontier_stats s; ssf_navfrontier_out o;\n"
                   "    if (ssf_navfrontier_default_params(h, &p) != SSF_OK) return -1;\n"
                   "    p.width = 64; p.height = 48; p.min_cells = 3; p.gain_radius = 8; p.reachable_only = 1;\n"
                   "    o.region = region; o.regions = table; o.order = order;\n"
                   "    if (ssf_navfrontier_regions(h, &p, state, 0, cost, &o, &s) != SSF_OK || table[0].rep_cost == SSF_NAVFRONTIER_UNREACHED) return -2;\n"
                   "    return (region[0] == SSF_NAVFRONTIER_NO_MEMBER) + (region[1] == SSF_NAVFRONTIER_DROPPED) + (int)s.regions_written + table[order[0]].gain; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    classes = (("ssf_navfrontier_params", binding.SsfNavFrontierParams), ("ssf_navfrontier_out", binding.SsfNavFrontierOut),
               ("ssf_navfrontier_stats", binding.SsfNavFrontierStats), ("ssf_navfrontier_region", binding.SsfNavFrontierRegion))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_navfrontier.h"', "int main(void) {"]
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
    # the numpy record is the same record
    dt = binding.NAVFRONTIER_REGION_DTYPE
    assert dt.itemsize == C.sizeof(binding.SsfNavFrontierRegion) == 56 and dt.names == fr.FIELDS
    for nm, _ in binding.SsfNavFrontierRegion._fields_:
        assert dt.fields[nm][1] == getattr(binding.SsfNavFrontierRegion, nm).offset, nm
    assert tuple(nm for nm, _ in binding.SsfNavFrontierStats._fields_) == fr.STATS + ("merge_pairs",)
    assert tuple(nm for nm, _ in binding.SsfNavFrontierParams._fields_)[2:-1] == tuple(fr.DEFAULTS)


def test_ssf_hpp_frontier_members_compile_and_link_against_the_explore_library(explore_lib, tmp_path):
    libdir = os.path.dirname(explore_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "navfrontier_smoke.cpp"),
           "-o", str(tmp_path / "navfrontier_smoke"), "-L", libdir, "-lssf_hip_explore", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_replay_options_parse():
    a = replay.parse_args(["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-frontiers", "--nav-frontier-min-cells", "5",
                           "--nav-frontier-gain-radius", "24"])
    assert replay.nav_frontiers_of(a) == dict(min_cells=5, gain_radius=24)
    b = replay.parse_args(["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-frontiers"])
    assert replay.nav_frontiers_of(b) == dict(min_cells=1, gain_radius=0)
    assert replay.nav_frontiers_of(replay.parse_args(["--npz", "frames.npz", "--nav-grid-dir", "grids"])) is None
    for bad in (["--nav-frontiers"], ["--nav-grid-dir", "grids", "--nav-frontier-min-cells", "3"],
                ["--nav-grid-dir", "grids", "--nav-frontier-gain-radius", "3"], ["--nav-grid-dir", "grids", "--nav-frontiers", "--nav-frontier-min-cells", "0"],
                ["--nav-grid-dir", "grids", "--nav-frontiers", "--nav-frontier-gain-radius", "129"]):
        with pytest.raises(SystemExit):
            replay.parse_args(["--npz", "frames.npz"] + bad)


def test_the_restatements_defaults_are_the_headers():
    hdr = open(os.path.join(INCLUDE, "ssf_navfrontier.h")).read()
    for text in ("connectivity 8, min_cells 1, max_regions 4096, gain_radius 0, cost_weight 1, gain_weight 0, size_weight 0",
                 "max(|dx|, |dy|) == R", "(2 |dx| s + R) / (2 R)", "ties go to the smaller label", "the smallest p among its cells"):
        assert text in hdr, text
    assert fr.DEFAULTS == dict(connectivity=8, traversable_only=0, min_dist2=0, min_cells=1, reachable_only=0, max_regions=4096, gain_radius=0,
                               cost_weight=1, gain_weight=0, size_weight=0)


# ---- hand-written answers ------------------------------------------------------------------------------------------------------
U, F, X = -1, 0, 100


def test_members_and_regions_on_a_dozen_cells():
    state = np.array([[F, U, F, F],
                      [F, F, X, U],
                      [U, F, F, F]], np.int8)
    q = fr.params()
    assert fr.members(state, None, q).astype(int).tolist() == [[1, 0, 1, 1], [1, 1, 0, 0], [0, 1, 0, 1]]       # 4-neighbours only; (2, 2) has none
    got = fr.frontiers(state)                                            # eight neighbours: (1, 1) touches (2, 0) across the corner
    assert got["region"].tolist() == [[0, -1, 0, 0], [0, 0, -1, -1], [-1, 0, -1, 1]]       # (3, 2) touches no member: (2, 1) is a wall, (2, 2) no member
    r0, r1 = got["regions"]
    assert (r0["label"], r0["cells"], r0["sum_x"], r0["sum_y"], r0["x0"], r0["y0"], r0["x1"], r0["y1"]) == (0, 6, 7, 4, 0, 0, 3, 2)
    assert (r1["label"], r1["cells"], r1["sum_x"], r1["sum_y"], r1["x0"], r1["y0"], r1["x1"], r1["y1"]) == (11, 1, 3, 2, 3, 2, 3, 2)
    assert all(r["rep_cost"] == INF and (r["rep_x"], r["rep_y"]) == (r["label"] % 4, r["label"] // 4) and r["gain"] == 0 for r in got["regions"])
    assert got["order"].tolist() == [0, 1]                               # nothing reached: the labels decide
    assert got["stats"] == dict(frontier_cells=7, regions_found=2, regions_small=0, regions_unreached=0, regions_kept=2, regions_written=2,
                                largest_cells=6, gain_rays=0)
    four = fr.frontiers(state, connectivity=4)                           # four neighbours: (2, 0)-(3, 0) stand alone
    assert four["region"].tolist() == [[0, -1, 1, 1], [0, 0, -1, -1], [-1, 0, -1, 2]]
    r0, r1, r2 = four["regions"]
    assert (r0["label"], r0["cells"], r0["sum_x"], r0["sum_y"], r0["x0"], r0["y0"], r0["x1"], r0["y1"]) == (0, 4, 2, 4, 0, 0, 1, 2)
    assert (r1["label"], r1["cells"], r1["sum_x"], r1["sum_y"]) == (2, 2, 5, 0) and (r2["label"], r2["cells"]) == (11, 1)
    state[1, 1] = X
    assert fr.frontiers(state, connectivity=4)["region"].tolist() == [[0, -1, 1, 1], [0, -1, -1, -1], [-1, 2, -1, 3]]
    assert fr.frontiers(state, connectivity=8)["region"].tolist() == [[0, -1, 1, 1], [0, -1, -1, -1], [-1, 0, -1, 2]]


def test_filters_the_representative_and_the_order():
    state = np.array([[F, F, U, F, X, F],
                      [U, X, X, F, X, U]], np.int8)
    #                 members: (0,0) (1,0) | (3,0) | (5,0)
    cost = np.array([[7, 7, INF, INF, INF, 3],
                     [INF, INF, INF, 5, INF, INF]], np.uint32)
    got = fr.frontiers(state, None, cost)
    assert got["region"].tolist() == [[0, 0, -1, 1, -1, 2], [-1, -1, -1, -1, -1, -1]]
    reps = [(r["rep_x"], r["rep_y"], r["rep_cost"]) for r in got["regions"]]
    assert reps == [(0, 0, 7), (3, 0, INF), (5, 0, 3)]                   # a tie on cost goes to the smaller p; (3, 1) is no member
    assert got["order"].tolist() == [2, 0, 1]                            # the unreached region last
    assert fr.frontiers(state, None, cost, size_weight=4)["order"].tolist() == [0, 2, 1]         # keys 7 - 8 = 3 - 4: the smaller label
    assert fr.frontiers(state, None, cost, size_weight=3)["order"].tolist() == [2, 0, 1]         # keys 7 - 6 = 1 and 3 - 3 = 0
    kept = fr.frontiers(state, None, cost, reachable_only=1, min_cells=1)
    assert kept["region"].tolist()[0] == [0, 0, -1, -2, -1, 1] and kept["stats"]["regions_unreached"] == 1 and kept["stats"]["regions_kept"] == 2
    big = fr.frontiers(state, None, cost, min_cells=2, reachable_only=1)
    assert big["region"].tolist()[0] == [0, 0, -1, -2, -1, -2] and (big["stats"]["regions_small"], big["stats"]["regions_unreached"]) == (2, 0)
    one = fr.frontiers(state, None, cost, max_regions=1)
    assert one["region"].tolist()[0] == [0, 0, -1, -2, -1, -2] and (one["stats"]["regions_kept"], one["stats"]["regions_written"]) == (3, 1)
    dist2 = np.array([[4, 3, 0, 9, 0, 4], [0, 0, 0, 9, 0, 0]], np.int32)
    trav = fr.frontiers(state, dist2, cost, traversable_only=1, min_dist2=4)
    assert trav["region"].tolist()[0] == [0, -1, -1, 1, -1, 2] and trav["stats"]["frontier_cells"] == 3


def test_the_gain_on_a_small_window():
    state = np.full((5, 5), U, np.int8)
    state[2, 2] = F
    assert fr.rim(1) == [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)] and len(fr.rim(2)) == 16 and len(fr.rim(128)) == 1024
    assert fr.gain(state, 2, 2, 1) == 8 and fr.gain(state, 2, 2, 2) == 24 and fr.gain(state, 2, 2, 0) == 0
    # the ray to (2, 1): step 1 is ((2 * 2 * 1 + 2) // 4, (2 * 1 * 1 + 2) // 4) = (1, 1), step 2 is (2, 1)
    assert fr.ray_cells(state, 2, 2, 2, 1, 2) == [(3, 3), (4, 3)] and fr.ray_cells(state, 2, 2, -2, 0, 2) == [(1, 2), (0, 2)]
    assert fr.gain(state, 0, 0, 2) == 7                                  # a corner: the window is clipped to 3 x 3, less the origin and the free (2, 2)
    wall = state.copy()
    wall[:, 3] = X                                                       # a wall shadows the right-hand side: columns 3 and 4 are never visited
    assert fr.gain(wall, 2, 2, 2) == 24 - 10
    free = state.copy()
    free[1, :] = F                                                       # free cells do not count and do not stop a ray
    assert fr.gain(free, 2, 2, 2) == 24 - 5
    distinct, visits = fr.gain_by_ray_lists(state, 2, 2, 2)
    assert (distinct, visits) == (24, 32)                                # 16 rays of two cells; the eight inner cells are shared
    got = fr.frontiers(np.array([[U, F, U]], np.int8), gain_radius=3, gain_weight=2)
    assert got["regions"][0]["gain"] == 2 and got["stats"]["gain_rays"] == 24


# ---- the second formulation ------------------------------------------------------------------------------------------------------
SCENES = [("random 45 x 70", lambda: fr.random_grid(45, 70, 3)), ("random 33 x 33 dense", lambda: fr.random_grid(33, 33, 5, obstacles=0.05, unknown=0.45)),
          ("random 70 x 45 sparse", lambda: fr.random_grid(70, 45, 7, obstacles=0.3, unknown=0.05)), ("spiral", lambda: (fr.spiral()[0], None)),
          ("checkerboard", lambda: (fr.checkerboard(), None)), ("room", lambda: fr.room()[:2])]


@pytest.mark.parametrize("name,make", SCENES, ids=[s[0] for s in SCENES])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_bfs_agrees_with_a_union_find_over_cell_pairs(name, make, connectivity):
    state, dist2 = make()
    q = fr.params(connectivity=connectivity)
    member = fr.members(state, dist2, q)
    label = fr.regions_by_union_find(member, connectivity)
    got = fr.frontiers(state, dist2, connectivity=connectivity, max_regions=65536)
    assert member.sum() > 20 and ((label >= 0) == member).all() and ((got["region"] >= 0) == member).all(), name
    table_label = np.array([r["label"] for r in got["regions"]], np.int64)
    assert (np.diff(table_label) > 0).all() and (table_label[got["region"][member]] == label[member]).all(), name
    for r in got["regions"]:
        ys, xs = np.nonzero(label == r["label"])
        assert (r["cells"], r["sum_x"], r["sum_y"], r["x0"], r["x1"], r["y0"], r["y1"]) == (len(xs), xs.sum(), ys.sum(), xs.min(), xs.max(), ys.min(), ys.max())
        assert label[r["label"] // state.shape[1], r["label"] % state.shape[1]] == r["label"] == (ys * state.shape[1] + xs).min()


def test_the_scenes_say_what_the_gpu_tests_need():
    s, cells = fr.spiral()
    one = fr.frontiers(s)
    assert s.shape == (64, 97) and one["stats"]["regions_found"] == 1 and one["regions"][0]["label"] == 0 and one["stats"]["frontier_cells"] > 3000
    tiles = {(x // 32, y // 32) for x, y in cells}
    assert len(tiles) == 8 and fr.frontiers(s, connectivity=4)["stats"]["regions_found"] > 1       # every tile; the corners hold it only diagonally
    cb = fr.checkerboard()
    assert fr.frontiers(cb)["stats"]["regions_found"] == 1
    many = fr.frontiers(cb, connectivity=4, max_regions=100)
    assert (many["stats"]["regions_found"], many["stats"]["regions_kept"], many["stats"]["regions_written"]) == (2048, 2048, 100)
    assert (many["region"] == -2).sum() == 1948 and many["region"].max() == 99


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_distinct_cells_against_one_list_per_ray(seed):
    state, _ = fr.random_grid(40, 40, seed, obstacles=0.04, unknown=0.5)
    rng = np.random.default_rng(seed)
    shared = 0
    for R in (1, 2, 7, 19, 40):
        for ox, oy in [(0, 0), (39, 39), (39, 0)] + [tuple(rng.integers(0, 40, 2)) for _ in range(3)]:
            distinct, visits = fr.gain_by_ray_lists(state, int(ox), int(oy), R)
            assert distinct == fr.gain(state, int(ox), int(oy), R) <= visits
            shared += visits > distinct
    assert shared > 10                                                   # many rays share their first cells


# ---- grids with values outside {0, -1, 100} (tests/navplan_ref.py's foreign grid, the GPU file's foreign cases) -------------------------
def test_what_the_regions_do_with_an_odd_state_by_hand():
    """a member is a cell of state 0 beside a cell of state -1: no other negative state makes one, and no other state is one; a gain ray
    stops at 100 alone and counts -1 alone"""
    for odd in pr.ODD_STATES:
        state = np.array([[0, odd, 0, -1, odd]], np.int8)
        got = fr.frontiers(state)
        assert got["region"].tolist() == [[-1, -1, 0, -1, -1]] and got["stats"]["frontier_cells"] == 1, odd
        # from (2, 0) with R = 2: the ray to the right passes -1 and the odd cell; the ray to the left passes the odd cell and a free one
        assert fr.ray_cells(state, 2, 0, 2, 0, 2) == [(3, 0), (4, 0)] and fr.ray_cells(state, 2, 0, -2, 0, 2) == [(1, 0), (0, 0)] and fr.gain(state, 2, 0, 2) == 1
    state = np.array([[0, 100, -1, 0, -1, 100, -1]], np.int8)
    assert fr.gain(state, 3, 0, 3) == 2 and fr.ray_cells(state, 3, 0, 3, 0, 3) == [(4, 0)]
    state, dist2 = np.array([[0, -1, 0]], np.int8), np.array([[-5, 3, (1 << 31) - 1]], np.int32)       # a negative dist2 is below min_dist2 = 0
    assert fr.frontiers(state, dist2, traversable_only=1)["region"].tolist() == [[-1, -1, 0]]
    assert fr.frontiers(state, dist2)["stats"]["frontier_cells"] == 2


@pytest.mark.parametrize("h,w", pr.FOREIGN_SIZES)
def test_the_foreign_grids_odd_values_decide_the_regions(h, w):
    f = pr.foreign_case(h, w, 0)
    state, dist2, cost = f["state"], f["dist2"], f["plan"]["cost"]
    kw = dict(min_cells=2, reachable_only=1, gain_radius=4, gain_weight=5, size_weight=2, traversable_only=1)
    got = fr.frontiers(state, dist2, cost, **kw)
    s = got["stats"]
    assert s["regions_kept"] >= 5 and s["regions_small"] >= 1 and s["regions_unreached"] >= 1 and max(r["gain"] for r in got["regions"]) > 3
    # a free cell whose only negative 4-neighbours are -2 or -128 is no member
    def beside(mask):
        m = np.pad(mask, 1, constant_values=False)
        return m[1:-1, 2:] | m[1:-1, :-2] | m[2:, 1:-1] | m[:-2, 1:-1]
    lone = (state == 0) & beside((state == -2) | (state == -128)) & ~beside(state == -1)
    assert lone.sum() > 10 and (got["region"][lone] == -1).all()
    assert ((state == 0) & (dist2 < 0) & beside(state == -1)).any() and (got["region"][(state == 0) & (dist2 < 0)] == -1).all()
    # the rays pass cells of odd states: with those cells occupied the gains are smaller
    walls = np.where(np.isin(state, (0, -1)), state, 100).astype(np.int8)
    reps = [(r["rep_x"], r["rep_y"]) for r in got["regions"]]
    assert sum(fr.gain(walls, x, y, 4) for x, y in reps) < sum(fr.gain(state, x, y, 4) for x, y in reps)
    # ... and cells of state -2 and -128, which are not counted
    minus = np.where(state < -1, -1, state).astype(np.int8)
    assert sum(fr.gain(minus, x, y, 4) for x, y in reps) > sum(r["gain"] for r in got["regions"])
