"""Plan over (x, y, heading) (include/ssf_navpose.h) without a GPU: the move table (ssf_navpose_moves is host only) against the
restatement (tests/navpose_ref.py) and its symmetries, the restatement's three formulations against each other (Dijkstra, whole-grid
sweeps, the device's tile rounds in any order and with stale rims), the tie to the disc's plan, guards that the T-junction shows what
it is there to show, who exports the entry points, the header on its own, the struct layouts of the binding, the refusals that need
no device, replay's options and the C++ surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import navfoot_ref as fr
import navplan_ref as pr
import navpose_ref as qr
from conftest import ROOT
from supersurfel_fusion_amd import binding

INCLUDE = os.path.join(ROOT, "include")
OLDER = ("NAVCARVE_LIB", "NAV_LIB", "EXPLORE_LIB", "DRIVE_LIB", "LIVE_LIB", "STEER_LIB", "FOOT_LIB")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


@pytest.fixture(scope="module")
def pose_lib(product_lib):
    return binding.load_pose()


# ---- the move table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", qr.HEADINGS)
def test_the_move_table_equals_the_restatement(B, pose_lib):
    for tol in (0, 63, 64, 65, 128, 256):
        for rev in (0, 1):
            got, want = binding.navpose_moves(B, tol, rev, pose_lib), qr.moves(B, tol, rev)
            assert got.dtype == np.int8 and got.shape == (B, 8) and (got == want).all(), (B, tol, rev, got.tolist(), want.tolist())
            assert rev or not (got == 2).any()


def test_the_move_table_by_hand(pose_lib):
    m = lambda *a: binding.navpose_moves(*a, library=pose_lib).tolist()
    assert m(1, 64, 0) == [[1, 0, 0, 0, 0, 0, 0, 0]]                      # one bin, heading +x: exactly one move
    assert m(1, 64, 1) == [[1, 0, 2, 0, 0, 0, 0, 0]]
    assert m(4, 0, 1) == [[1, 0, 2, 0, 0, 0, 0, 0], [0, 1, 0, 2, 0, 0, 0, 0], [2, 0, 1, 0, 0, 0, 0, 0], [0, 2, 0, 1, 0, 0, 0, 0]]
    assert m(8, 0, 0)[1] == [0, 0, 0, 0, 1, 0, 0, 0] and m(8, 0, 0)[7] == [0, 0, 0, 0, 0, 0, 0, 1]
    t = m(16, 64, 0)
    assert t[1] == [1, 0, 0, 0, 1, 0, 0, 0]                               # 22.5 degrees: 64 units from both +x and the diagonal: both on a tie
    assert m(16, 63, 0)[1] == [0] * 8 and m(32, 64, 0)[1] == [1, 0, 0, 0, 0, 0, 0, 0] and m(32, 64, 0)[3] == [0, 0, 0, 0, 1, 0, 0, 0]
    assert m(2, 256, 0) == [[1, 1, 0, 1, 1, 0, 0, 1], [0, 1, 1, 1, 0, 1, 1, 0]]      # a half plane each, the boundary included
    assert (np.array(m(8, 256, 1)) != 0).all()                            # holonomic: every move at every bin


@pytest.mark.parametrize("B", [4, 8, 16, 32])
def test_the_move_table_has_the_quarter_turn_symmetry(B, pose_lib):
    """a quarter turn of the heading (B / 4 bins) turns every move by a quarter turn: (+1,0) -> (0,+1) -> (-1,0) -> (0,-1) and the
    diagonals likewise: k -> (k + 1) % 4 within each group of four"""
    turned = [1, 2, 3, 0, 5, 6, 7, 4]
    for tol in (0, 64, 100, 256):
        for rev in (0, 1):
            t = binding.navpose_moves(B, tol, rev, pose_lib)
            for b in range(B):
                for k in range(8):
                    assert t[(b + B // 4) % B, turned[k]] == t[b, k], (B, tol, rev, b, k)
            half = np.roll(t, B // 2, axis=0)                             # a half turn swaps forward and reverse where both are allowed
            if rev and tol < 256:
                assert ((t == 1) == (half == 2)).all() and ((t == 0) == (half == 0)).all()


# ---- the restatement against itself ----------------------------------------------------------------------------------------------------
def random_case(seed, B=8, h=37, w=45, foot=fr.LINE, **kw):
    state, dist2 = pr.random_grid(h, w, seed, obstacles=0.03, unknown=0.02)
    mask = fr.layers(state, 0, foot, B)["free_mask"]
    q = qr.params(n_headings=B, **kw)
    trav, pen = qr.prep(mask, dist2, q)
    at = np.argwhere(trav)
    rng = np.random.default_rng(seed)
    goals = [(at[i][2], at[i][1], -1 if j else at[i][0]) for j, i in enumerate(rng.integers(len(at), size=2))]
    goal, n = qr.goal_states(trav, goals)
    assert n["goals_used"] == 2
    return trav, pen, goal, q


@pytest.mark.parametrize("seed,kw", [(1, dict()), (2, dict(soft_dist2=20, near_penalty=9, turn_cost=1)), (3, dict(allow_reverse=0, move_tol=0)),
                                     (4, dict(move_tol=256, reverse_cost=0, turn_cost=1000))])
def test_the_tile_rounds_in_any_order_and_with_stale_rims_give_dijkstras_field(seed, kw):
    """the kernel's rounds emulated on the CPU: 16 x 16-cell tiles with all layers, one after another, in shuffled order, and with every
    rim read as stale as a round allows: Dijkstra's field each time, and the whole-grid sweeps' as well"""
    trav, pen, goal, q = random_case(seed, **kw)
    want = qr.field(trav, pen, goal, q)
    assert (want != qr.INF).sum() > trav.sum() // 2 and (want[trav] == qr.INF).sum() >= 0
    assert (qr.field_by_sweeps(trav, pen, goal, q) == want).all()
    got, rounds, visits = qr.field_by_tile_rounds(trav, pen, goal, q)
    assert (got == want).all() and rounds >= 2 and visits >= 9              # 3 x 3 tiles
    rng = np.random.default_rng(seed)
    shuffled = lambda r, tiles: [tiles[i] for i in rng.permutation(len(tiles))]
    assert (qr.field_by_tile_rounds(trav, pen, goal, q, order=shuffled)[0] == want).all()
    got, stale_rounds, _ = qr.field_by_tile_rounds(trav, pen, goal, q, order=lambda r, tiles: tiles[::-1], stale=True)
    assert (got == want).all() and stale_rounds >= rounds
    assert (want[~trav] == qr.INF).all() and (want[goal] == 0).all()


def test_the_point_footprint_with_one_bin_and_every_move_is_the_discs_plan():
    """a point footprint (mask all ones where clear), move_tol 256, reverse allowed at no cost: with B = 1 the field is navplan_ref's for
    the same min_dist2, soft_dist2 and near_penalty, and so are the paths"""
    for seed, allow, kw in ((11, 0, dict(min_dist2=3)), (12, 1, dict(min_dist2=0, soft_dist2=25, near_penalty=30))):
        state, dist2 = pr.random_grid(33, 47, seed, obstacles=0.2, unknown=0.1)
        goals, starts = [(5, 5), (40, 30), (20, 16)], [(1, 1), (46, 32), (23, 2), (10, 30)]
        state[5, 5] = state[30, 40] = 0
        dist2[5, 5] = dist2[30, 40] = 9
        disc = pr.plan(state, dist2, goals, starts, allow_unknown=allow, max_path=4096, **kw)
        pose = qr.plan(qr.point_mask(state, allow, 1), dist2, [g + (-1,) for g in goals], [(x * 1024 + 7, y * 1024 + 1000, 12345) for x, y in starts],
                       n_headings=1, move_tol=256, allow_reverse=1, reverse_cost=0, max_path=4096, **kw)
        assert (pose["cost"][0] == disc["cost"]).all() and (pose["cell_cost"] == disc["cost"]).all() and (disc["cost"] != pr.INF).sum() > 500
        assert (pose["cell_bin"] == np.where(disc["cost"] == pr.INF, 255, 0)).all()
        assert (pose["start_status"] == disc["start_status"]).all() and (pose["start_cost"] == disc["start_cost"]).all()
        for a, b in zip(pose["path"], disc["path"]):
            assert (a[:, :2] == b).all() and (a[:, 2] == 0).all()
        assert pose["stats"]["states_reached"] == disc["stats"]["cells_reached"] == pose["stats"]["cells_reached"]
        # with more bins the holonomic point pays nothing for its heading either: the projection is still the disc's field
        more = qr.plan(qr.point_mask(state, allow, 4), dist2, [g + (-1,) for g in goals], None, n_headings=4, move_tol=256, allow_reverse=1, reverse_cost=0, **kw)
        assert (more["cell_cost"] == disc["cost"]).all()


def test_the_projection_and_the_start_state_by_hand():
    cost = np.full((4, 1, 3), qr.INF, np.uint32)
    cost[2, 0, 0], cost[1, 0, 0], cost[3, 0, 1], cost[0, 0, 1] = 7, 7, 5, 9
    cc, cb = qr.project(cost)
    assert cc.tolist() == [[7, 5, qr.INF]] and cb.tolist() == [[1, 3, 255]]          # the smallest bin that attains the minimum; 255 where none does
    assert qr.start_state((1024 * 3 + 1023, -1, 65536 + 8191), 4) == (3, -1, 0) and qr.start_state((0, 2048, 8192), 4) == (0, 2, 1)
    assert qr.start_state((5, 5, -1), 32) == (0, 0, 0) and qr.start_state((5, 5, 65535 - 1024), 32) == (0, 0, 31) and qr.start_state((5, 5, 40000), 1) == (0, 0, 0)


# ---- the scene the call is there for ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [32, 16, 8])
def test_the_t_junction_shows_what_the_disc_cannot(B):
    sx, sy = qr.TJ_START_CELL
    costs = {}
    for detour in (False, True):
        s = qr.tjunction_scene(detour)
        assert s["state"].shape == (64, 70) and s["state"][sy, sx] == 0 and s["state"][s["goal_cell"][1], s["goal_cell"][0]] == 0
        disc = pr.plan(s["state"], s["dist2"], [s["goal_cell"]], [s["start_cell"]], min_dist2=qr.TJ_DISC_MIN_DIST2, max_path=4096)
        assert disc["start_status"][0] == 0                               # the disc by the inscribed radius drives through the bend
        lay = fr.layers(s["state"], 0, s["foot"], B)
        assert (lay["free_mask"][sy, sx] & 1) and (lay["free_mask"][s["goal_cell"][1], s["goal_cell"][0]] >> (B // 4)) & 1        # lengthwise in either corridor
        pose = qr.plan(lay["free_mask"], s["dist2"], s["goals"], s["start"], n_headings=B, max_path=4096, **qr.TJ_KW)
        costs[detour] = (int(disc["start_cost"][0]), int(pose["start_cost"][0]))
        if not detour:
            assert pose["start_status"][0] == qr.STATUS_NO_GOAL and (pose["cost"][:, sy, sx] == qr.INF).all()      # no state of the start cell is reached
            assert pose["stats"]["states_reached"] > 0 and (pose["cost"][:, :, :33] == qr.INF).all()              # what is reached lies in the vertical corridor
        else:
            assert pose["start_status"][0] == qr.STATUS_REACHED and qr.INF > costs[True][1] > costs[True][0]
            p = pose["path"][0]
            junction = (p[:, 0] >= 40) & (p[:, 0] < 48) & (p[:, 1] >= 8) & (p[:, 1] < 15)
            lengthwise = np.minimum(np.minimum(p[:, 2], B - p[:, 2]), np.abs(p[:, 2] - B // 2)) <= 1
            assert junction.any() and lengthwise[junction].all()
    assert costs[False][0] == costs[True][0]                              # the detour is no shortcut for the disc: it still turns in the junction


# ---- who exports what ------------------------------------------------------------------------------------------------------------------
def test_the_pose_library_exports_the_pose_plan_and_all_of_the_foot_library(pose_lib, product_lib, oracle_lib):
    """libssf_hip_pose.so = libssf_hip_foot.so's objects + ssf_navpose.hip; the eight older tables and the oracle hold no name of it"""
    have, foot = exported(pose_lib.path), exported(binding.FOOT_LIB)
    hip_ids = lambda names: {nm for nm in names if nm.startswith("__hip_cuid_")}         # one per translation unit, named by content
    for names in (binding.NAVPOSE_SYMBOLS, binding.NAVFOOT_SYMBOLS, binding.NAVSTEER_SYMBOLS, binding.NAVLIVE_SYMBOLS, binding.NAVPATH_SYMBOLS,
                  binding.NAVFRONTIER_SYMBOLS, binding.NAVPLAN_SYMBOLS, binding.NAVCARVE_SYMBOLS, binding.ABI_SYMBOLS):
        assert set(names) <= have
    assert pose_lib.has_navpose and pose_lib.has_navfoot and pose_lib.has_navsteer and pose_lib.has_navplan and pose_lib.backend == "hip-gfx950"
    assert foot - hip_ids(foot) <= have
    extra = have - foot - hip_ids(have)
    assert set(binding.NAVPOSE_SYMBOLS) <= extra and len(binding.NAVPOSE_SYMBOLS) == 3
    kernels = extra - set(binding.NAVPOSE_SYMBOLS)
    assert kernels == {nm for nm in extra if "k_navpose_" in nm}, sorted(extra)
    assert all(any(k in nm for nm in kernels) for k in ("k_navpose_init", "k_navpose_goals", "k_navpose_relax", "k_navpose_stats", "k_navpose_trace"))
    for other in [exported(product_lib.path), exported(oracle_lib.path)] + [exported(getattr(binding, nm)) for nm in OLDER]:
        assert not [nm for nm in other if "navpose" in nm]
    for load in ("load_navcarve", "load_nav", "load_explore", "load_drive", "load_live", "load_steer", "load_foot"):
        assert not getattr(binding, load)().has_navpose
    assert not product_lib.has_navpose and not oracle_lib.has_navpose


def test_the_foot_library_exports_what_it_exported():
    have, steer = exported(binding.FOOT_LIB), exported(binding.STEER_LIB)
    extra = {nm for nm in have - steer if not nm.startswith("__hip_cuid_")}
    assert extra == set(binding.NAVFOOT_SYMBOLS) | {nm for nm in extra if "k_navfoot_" in nm}, sorted(extra)


def test_an_older_library_names_the_missing_symbol(product_lib):
    lib = binding.load_foot()
    assert not lib.has_navpose
    f = binding.Fusion.__new__(binding.Fusion)                            # (no handle: the check comes before any call)
    f.L = lib
    mask, dist2, poses = np.ones((3, 3), np.uint32), np.ones((3, 3), np.int32), np.zeros((1, 3), np.int32)
    with pytest.raises(binding.SsfError, match="ssf_navpose_field.*binding.load_pose"):
        f.nav_pose_plan(mask, dist2, [(1, 1, -1)], n_headings=1)
    with pytest.raises(binding.SsfError, match="ssf_navpose_field.*binding.load_pose"):
        f.nav_pose_plan_device(0, 0, 3, 3, [(1, 1, -1)], n_headings=1)
    with pytest.raises(binding.SsfError, match="ssf_navpose_default_params"):
        f.nav_pose_default_params()
    with pytest.raises(binding.SsfError, match="ssf_navpose_moves.*binding.load_pose"):
        binding.navpose_moves(8, 64, 1, lib)
    f.L = binding.load_live()                                             # (the overlay's library: the chain stops at the footprint, by name)
    with pytest.raises(binding.SsfError, match="ssf_navfoot_rollouts.*binding.load_foot"):
        f.nav_live_pose_steer(np.ones((48, 64), np.float32), np.zeros((3, 3), np.int8), [(1, 1, -1)], poses, dict(front=1024))
    f.L = lib
    with pytest.raises(binding.SsfError, match="ssf_navpose_field.*binding.load_pose"):
        f.nav_live_pose_steer(np.ones((48, 64), np.float32), np.zeros((3, 3), np.int8), [(1, 1, -1)], poses, dict(front=1024))


def test_the_pose_plans_symbols_stay_out_of_the_other_headers():
    for nm in binding.NAVPOSE_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        for hdr in ("ssf.h", "ssf_testing.h", "ssf_navgrid.h", "ssf_navplan.h", "ssf_navlive.h", "ssf_navsteer.h", "ssf_navfoot.h"):
            assert nm not in open(os.path.join(INCLUDE, hdr)).read(), (nm, hdr)
        assert nm + "(" in open(os.path.join(INCLUDE, "ssf_navpose.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_navpose.h"\n'
                   "int f(ssf_handle* h, const uint32_t* mask, const int32_t* dist2, const int32_t* goals, uint32_t* cell_cost) {\n"
                   "    ssf_navpose_params p; ssf_navpose_stats s; ssf_navpose_out o; int8_t moves[SSF_NAVFOOT_MAX_HEADINGS * 8];\n"
                   "    if (ssf_navpose_moves(8, 64, 1, moves) != SSF_OK || moves[0] != 1) return -1;\n"
                   "    if (ssf_navpose_default_params(h, &p) != SSF_OK || p.width * p.height * p.n_headings > SSF_NAVPOSE_MAX_STATES) return -2;\n"
                   "    p.goals = goals; p.n_goals = 1;\n"
                   "    o.cost = 0; o.cell_cost = cell_cost; o.cell_bin = 0; o.start_cost = 0; o.start_status = 0; o.path_len = 0; o.path = 0;\n"
                   "    if (ssf_navpose_field(h, &p, mask, dist2, &o, &s) != SSF_OK) return -3;\n"
                   "    return (int)(s.states_reached + s.rounds) + (cell_cost[0] == SSF_NAVPOSE_UNREACHED) + SSF_NAVPOSE_NO_BIN + SSF_NAVPOSE_TILE + SSF_NAVPOSE_ROUND_BATCH; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    classes = (("ssf_navpose_params", binding.SsfNavPoseParams), ("ssf_navpose_out", binding.SsfNavPoseOut),
               ("ssf_navpose_stats", binding.SsfNavPoseStats))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_navpose.h"', "int main(void) {"]
    for st, cls in classes:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for nm, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, nm, st, nm))
    lines += ['    printf("consts %u %d %d %d %d\\n", SSF_NAVPOSE_UNREACHED, SSF_NAVPOSE_NO_BIN, SSF_NAVPOSE_TILE, SSF_NAVPOSE_ROUND_BATCH, SSF_NAVPOSE_MAX_STATES);',
              "    return 0; }"]
    src = tmp_path / "off.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "off")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    rows = [l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()]
    got = {r[0]: r[1] for r in rows if r[0] != "consts"}
    for st, cls in classes:
        assert int(got[st]) == C.sizeof(cls), st
        for nm, _ in cls._fields_:
            assert int(got["%s.%s" % (st, nm)]) == getattr(cls, nm).offset, (st, nm)
    consts = tuple(int(v) for v in [r for r in rows if r[0] == "consts"][0][1:])
    assert consts == (binding.NAVPOSE_UNREACHED, binding.NAVPOSE_NO_BIN, binding.NAVPOSE_TILE, binding.NAVPOSE_ROUND_BATCH, binding.NAVPOSE_MAX_STATES)
    assert consts[:4] == (qr.INF, qr.NO_BIN, qr.TILE, qr.ROUND_BATCH)
    assert tuple(nm for nm, _ in binding.SsfNavPoseStats._fields_)[:len(qr.STATS)] == qr.STATS
    assert tuple(nm for nm, _ in binding.SsfNavPoseOut._fields_) == binding.NAVPOSE_OUTPUT_NAMES


def test_the_refusals_that_need_no_device(pose_lib):
    L = pose_lib.lib
    out = np.full(32 * 8 + 1, 77, np.int8)
    call = lambda *a: L.ssf_navpose_moves(*a, out.ctypes.data_as(C.c_void_p))
    assert call(1, 0, 0) == 0 and call(32, 256, 1) == 0 and out[-1] == 77
    for bad in ((0, 64, 1), (3, 64, 1), (64, 64, 1), (-2, 64, 1), (8, -1, 1), (8, 257, 1), (8, 64, 2), (8, 64, -1)):
        assert call(*bad) != 0, bad
    assert L.ssf_navpose_moves(8, 64, 1, None) != 0
    for bad in ((3, 64, 1), (8, 300, 1), (8, 64, 5)):
        with pytest.raises(binding.SsfError, match="ssf_navpose_moves refused"):
            binding.navpose_moves(*bad, library=pose_lib)
    assert L.ssf_navpose_default_params(None, None) != 0
    assert L.ssf_navpose_field(None, None, None, None, None, None) != 0
    p = binding.SsfNavPoseParams()
    assert L.ssf_navpose_field(None, C.byref(p), None, None, None, None) != 0
    f = binding.Fusion.__new__(binding.Fusion)                            # (no handle: the binding's own checks come before any call)
    f.L = pose_lib
    with pytest.raises(binding.SsfError, match="unknown pose plan outputs"):
        f.nav_pose_plan(np.ones((3, 3), np.uint32), np.ones((3, 3), np.int32), [(1, 1, -1)], outputs=("frontier",))
    with pytest.raises(binding.SsfError, match="one shape"):
        f.nav_pose_plan(np.ones((3, 3), np.uint32), np.ones((3, 4), np.int32), [(1, 1, -1)])


# ---- replay.py's options and the C++ surface ---------------------------------------------------------------------------------------------
def test_the_replay_options_parse_and_pick_the_library(pose_lib):
    from supersurfel_fusion_amd import replay
    base = ["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-plan-goal", "1.0", "2.0"]
    foot = base + ["--nav-steer", "--nav-steer-footprint", "0.3", "0.3", "0.2", "0.2"]
    a = replay.parse_args(foot + ["--nav-plan-poses"])
    assert replay.nav_steer_of(a) == dict(horizon=32, speed=0.5, footprint=(0.3, 0.3, 0.2, 0.2), headings=16, poses=dict(turn_cost=5))
    a = replay.parse_args(foot + ["--nav-plan-poses", "--nav-plan-turn-cost", "40", "--nav-steer-headings", "8"])
    assert replay.nav_steer_of(a) == dict(horizon=32, speed=0.5, footprint=(0.3, 0.3, 0.2, 0.2), headings=8, poses=dict(turn_cost=40))
    assert replay.nav_steer_of(replay.parse_args(foot)) == dict(horizon=32, speed=0.5, footprint=(0.3, 0.3, 0.2, 0.2), headings=16)      # without it: as before
    for bad in (base + ["--nav-steer", "--nav-plan-poses"], base + ["--nav-plan-poses"], foot + ["--nav-plan-turn-cost", "5"],
                foot + ["--nav-plan-poses", "--nav-plan-turn-cost", "0"], foot + ["--nav-plan-poses", "--nav-plan-turn-cost", "1001"]):
        with pytest.raises(SystemExit):
            replay.parse_args(bad)
    assert replay.library_of(replay.parse_args(foot + ["--nav-plan-poses"])) == "load_pose"
    assert replay.library_of(replay.parse_args(foot)) == "load_foot" and replay.library_of(replay.parse_args(base + ["--nav-steer"])) == "load_steer"
    lib = getattr(binding, replay.library_of(replay.parse_args(foot + ["--nav-plan-poses"])))()
    assert lib.has_navpose and lib.path == pose_lib.path


def test_ssf_hpp_pose_members_compile_and_link_against_the_pose_library(pose_lib, tmp_path):
    libdir = os.path.dirname(pose_lib.path)
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "navpose_smoke")
    # the host-only part runs under the address and undefined-behaviour sanitizers: a stand-alone program, nothing loaded into Python
    cmd = ["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", INCLUDE,
           "-I", cpp, os.path.join(cpp, "navpose_smoke.cpp"), "-o", exe, "-L", libdir, "-lssf_hip_pose", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe, "--sizes"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "moves refused=1" in r.stdout, r.stdout
    assert "sizes params=%d out=%d stats=%d" % (C.sizeof(binding.SsfNavPoseParams), C.sizeof(binding.SsfNavPoseOut), C.sizeof(binding.SsfNavPoseStats)) in r.stdout, r.stdout
    for B in qr.HEADINGS:
        for tol in (0, 64, 256):
            for rev in (0, 1):
                assert "moves B=%d tol=%d rev=%d rc=0 sum=%016x" % (B, tol, rev, pr.fnv1a(qr.moves(B, tol, rev).tobytes())) in r.stdout, (B, tol, rev, r.stdout)
    # a program that steers with the footprint alone still links against the foot library: the pose plan's members leave no reference behind
    exe2 = str(tmp_path / "navfoot_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", INCLUDE, "-I", cpp, os.path.join(cpp, "navfoot_smoke.cpp"), "-o", exe2, "-L", libdir,
                        "-lssf_hip_foot", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
