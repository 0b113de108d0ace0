"""Velocity commands on the navigation grid (include/ssf_navsteer.h) without a GPU: who exports the entry points, the header on its
own, the struct layouts of the binding, the direction table, the host helpers, the C++ surface, replay.py's options, and the
restatement the GPU tests compare against (tests/navsteer_ref.py): hand cases with written-out answers, and guards that no
scene of the GPU file is vacuous."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import navplan_ref as pr
import navsteer_ref as sr
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


# ---- static checks -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def steer_lib(product_lib):
    return binding.load_steer()


def test_the_steer_library_exports_the_rollouts_and_all_of_the_live_library(steer_lib, product_lib, oracle_lib):
    """libssf_hip_steer.so = libssf_hip_live.so's objects + ssf_navsteer.hip; the six older tables and the oracle hold no name of it"""
    have, live = exported(steer_lib.path), exported(binding.LIVE_LIB)
    hip_ids = lambda names: {nm for nm in names if nm.startswith("__hip_cuid_")}         # one per translation unit, named by content
    for names in (binding.NAVSTEER_SYMBOLS, binding.NAVLIVE_SYMBOLS, binding.NAVPATH_SYMBOLS, binding.NAVFRONTIER_SYMBOLS, binding.NAVPLAN_SYMBOLS,
                  binding.NAVCARVE_SYMBOLS, binding.ABI_SYMBOLS):
        assert set(names) <= have
    assert steer_lib.has_navsteer and steer_lib.has_navlive and steer_lib.has_navpath and steer_lib.has_navfrontier and steer_lib.has_navplan
    assert steer_lib.has_navcarve and steer_lib.has_navgrid and steer_lib.backend == "hip-gfx950"
    assert live - hip_ids(live) <= have
    extra = have - live - hip_ids(have)
    assert set(binding.NAVSTEER_SYMBOLS) <= extra and len(binding.NAVSTEER_SYMBOLS) == 3
    kernels = extra - set(binding.NAVSTEER_SYMBOLS)
    assert kernels == {nm for nm in extra if "k_navsteer_" in nm}, sorted(extra)
    assert all(any(k in nm for nm in kernels) for k in ("k_navsteer_pack", "k_navsteer_roll", "k_navsteer_pick"))
    for other in (exported(product_lib.path), exported(binding.NAVCARVE_LIB), exported(binding.NAV_LIB), exported(binding.EXPLORE_LIB),
                  exported(binding.DRIVE_LIB), live, exported(oracle_lib.path)):
        assert not [nm for nm in other if "navsteer" in nm]
    for load in ("load_navcarve", "load_nav", "load_explore", "load_drive", "load_live"):
        assert not getattr(binding, load)().has_navsteer
    assert not product_lib.has_navsteer and not oracle_lib.has_navsteer


def test_an_oracle_backed_fusion_names_the_missing_symbol(oracle_lib):
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    state, dist2, poses, depth = np.zeros((3, 3), np.int8), np.ones((3, 3), np.int32), np.zeros((1, 3), np.int32), np.ones((48, 64), np.float32)
    for call, symbol in ((lambda: f.nav_steer(state, dist2, poses, cost_weight=0), "ssf_navsteer_rollouts"),
                         (lambda: f.nav_steer_device(None, None, 3, 3, None, 1), "ssf_navsteer_rollouts"),
                         (f.nav_steer_default_params, "ssf_navsteer_default_params")):
        with pytest.raises(binding.SsfError, match=symbol + ".*binding.load_steer"):
            call()
    with pytest.raises(binding.SsfError, match="binding.load_"):         # (the overlay is missing there too, and is asked for first)
        f.nav_live_steer(depth, state, [(1, 1)], poses)
    with pytest.raises(binding.SsfError, match="ssf_navsteer_direction_table.*binding.load_steer"):
        binding.navsteer_direction_table(oracle_lib)


@pytest.mark.parametrize("load", ["load_product", "load_nav", "load_live"])
def test_an_older_library_names_the_rollouts_symbol(load, product_lib):
    """the older libraries steer nothing: the calls say which symbol is missing before anything runs"""
    lib = getattr(binding, load)()
    assert not lib.has_navsteer
    f = binding.Fusion.__new__(binding.Fusion)                            # (no handle: the check comes before any call)
    f.L = lib
    state, dist2, poses = np.zeros((3, 3), np.int8), np.ones((3, 3), np.int32), np.zeros((1, 3), np.int32)
    with pytest.raises(binding.SsfError, match="ssf_navsteer_rollouts.*binding.load_steer"):
        f.nav_steer(state, dist2, poses, cost_weight=0)
    with pytest.raises(binding.SsfError, match="ssf_navsteer_default_params"):
        f.nav_steer_default_params()
    with pytest.raises(binding.SsfError, match="ssf_navsteer_direction_table"):
        binding.navsteer_direction_table(lib)
    if load == "load_live":                                              # everything but the rollouts is there: they are what is named
        with pytest.raises(binding.SsfError, match="ssf_navsteer_rollouts.*binding.load_steer"):
            f.nav_live_steer(np.ones((48, 64), np.float32), state, [(1, 1)], poses)


def test_the_rollout_symbols_stay_out_of_the_other_headers():
    for nm in binding.NAVSTEER_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        for hdr in ("ssf.h", "ssf_testing.h", "ssf_navgrid.h", "ssf_navcarve.h", "ssf_navplan.h", "ssf_navfrontier.h", "ssf_navpath.h", "ssf_navlive.h"):
            assert nm not in open(os.path.join(INCLUDE, hdr)).read(), (nm, hdr)
        assert nm + "(" in open(os.path.join(INCLUDE, "ssf_navsteer.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_navsteer.h"\n'
                   "int f(ssf_handle* h, const int8_t* state, const int32_t* dist2, const uint32_t* cost, const int32_t* poses, int32_t* cmd) {\n"
                   "    ssf_navsteer_params p; ssf_navsteer_stats s; ssf_navsteer_out o; int32_t c[SSF_NAVSTEER_DIRECTIONS];\n"
                   "    if (ssf_navsteer_default_params(h, &p) != SSF_OK || ssf_navsteer_direction_table(c, 0) != SSF_OK) return -1;\n"
                   "    p.n_poses = 1; p.n_steps = 16; p.turn_weight = 1;\n"
                   "    o.best = 0; o.best_cmd = cmd; o.best_score = 0; o.n_admissible = 0; o.pose_status = 0; o.best_len = 0; o.best_traj = 0;\n"
                   "    o.cand_free = 0; o.cand_min_d = 0; o.cand_end = 0; o.cand_end_cost = 0; o.cand_score = 0;\n"
                   "    if (ssf_navsteer_rollouts(h, &p, state, dist2, cost, poses, 0, &o, &s) != SSF_OK) return -2;\n"
                   "    return (int)(s.poses_ok + s.admissible + s.windows_staged) + c[0] / SSF_NAVSTEER_SUBUNITS + (cost[0] == SSF_NAVSTEER_NO_COST)\n"
                   "           + SSF_NAVSTEER_TURN; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    classes = (("ssf_navsteer_params", binding.SsfNavSteerParams), ("ssf_navsteer_out", binding.SsfNavSteerOut),
               ("ssf_navsteer_stats", binding.SsfNavSteerStats))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_navsteer.h"', "int main(void) {"]
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
    assert tuple(nm for nm, _ in binding.SsfNavSteerStats._fields_) == sr.STATS + sr.INFORMATIVE
    assert tuple(nm for nm, _ in binding.SsfNavSteerOut._fields_) == binding.NAVSTEER_OUTPUT_NAMES == sr.OUTPUTS
    assert {nm: np.dtype(dt) for nm, dt, _, _ in binding.NAVSTEER_OUTPUTS} == {nm: np.dtype(dt) for nm, dt in sr.DTYPES.items()}
    assert [nm for nm, _ in binding.SsfNavSteerParams._fields_ if nm != "on_device"] == list(sr.DEFAULTS)
    assert (binding.NAVSTEER_SUBUNITS, binding.NAVSTEER_TURN, binding.NAVSTEER_NO_COST) == (sr.SUB, sr.TURN, sr.NO_COST)


def test_the_restatements_defaults_and_staging_limit_are_the_sources():
    hdr = open(os.path.join(INCLUDE, "ssf_navsteer.h")).read()
    for text in ("design choices, not tuned values", "n_v 9, n_w 33, n_steps 32, v_min 0, v_step 64, w_min -2048, w_step 128, min_free_steps 2, brake_div 128, clearance_cap 64",
                 "cost_weight 1, clear_weight 1, speed_weight 1", "k  = ((2 h + w + 64) >> 7) & 1023", "no-corner-cutting rule",
                 "smallest (score, c)", "C[k] = floor(16384 * cos(2 pi k / 1024) + 0.5)"):
        assert text in hdr, text
    d = sr.DEFAULTS
    assert (d["width"], d["height"], d["n_v"], d["n_w"], d["n_steps"], d["v_min"], d["v_step"], d["w_min"], d["w_step"]) == (512, 512, 9, 33, 32, 0, 64, -2048, 128)
    assert (d["min_free_steps"], d["brake_div"], d["clearance_cap"], d["cost_weight"], d["clear_weight"], d["speed_weight"]) == (2, 128, 64, 1, 1, 1)
    assert all(d[k] == 0 for k in ("min_dist2", "allow_unknown", "target_weight", "turn_weight", "walk", "n_poses"))
    src = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "ssf_navsteer.hip")).read()
    assert "NS_LDS_CELLS = %d," % sr.LDS_CELLS in src and "NS_LDS_FREE = NS_CU_LDS / 8, NS_CUS = 256" in src


# ---- the direction table and the host helpers --------------------------------------------------------------------------------
def test_the_direction_table_is_the_formula_and_has_the_quarter_turn_symmetry(steer_lib):
    c, s = binding.navsteer_direction_table(steer_lib)
    k = np.arange(1024)
    assert c.dtype == np.int32 and s.dtype == np.int32 and c.shape == s.shape == (1024,)
    assert (c == np.floor(16384 * np.cos(2 * np.pi * k / 1024) + 0.5)).all() and (s == np.floor(16384 * np.sin(2 * np.pi * k / 1024) + 0.5)).all()
    rc, rs = sr.direction_table()
    assert (c == rc).all() and (s == rs).all()
    # a quarter turn on: (C, S) -> (-S, C); the mirror: C even, S odd
    assert (c[(k + 256) % 1024] == -s).all() and (s[(k + 256) % 1024] == c).all()
    assert (c[(1024 - k) % 1024] == c).all() and (s[(1024 - k) % 1024] == -s).all()
    assert (c[0], s[0], c[256], s[256], c[512], s[512], c[768], s[768]) == (16384, 0, 0, 16384, -16384, 0, 0, -16384)
    assert (c[128], s[128], c[1], s[1], c[1008], s[1008]) == (11585, 11585, 16384, 101, 16305, -1606)
    # no entry near a rounding boundary: the fractional part of 16384 cos + 0.5 stays away from 0 and 1
    frac = np.concatenate([16384 * np.cos(2 * np.pi * k / 1024) + 0.5, 16384 * np.sin(2 * np.pi * k / 1024) + 0.5])
    frac = frac - np.floor(frac)
    exact = np.isin(np.concatenate([k, k]) % 256, (0,)) | (np.abs(frac - 0.5) < 1e-9)       # the axes are exact integers
    assert np.minimum(frac, 1 - frac)[~exact].min() > 3.9e-4
    # only the two pointers that are given are written
    only = np.full(1024, 7, np.int32)
    assert steer_lib.lib.ssf_navsteer_direction_table(None, only.ctypes.data_as(C.c_void_p)) == 0 and (only == s).all()
    assert steer_lib.lib.ssf_navsteer_direction_table(None, None) == 0


def test_the_window_helper():
    win = binding.Fusion.nav_steer_window
    # 0.3 m/s now, +-0.5 m/s^2 over 0.1 s: 0.25 .. 0.35 m/s; at 0.05 m cells one m/s is 2048 units per step: 512 .. 716
    got = win(0.3, 0.0, (0.0, 0.5), (-1.0, 1.0), (0.5, 2.0), 0.1, 0.05, 9, 33)
    assert got == dict(n_v=9, n_w=33, v_min=512, v_step=25, w_min=-208, w_step=13)
    v = got["v_min"] + np.arange(9) * got["v_step"]
    w = got["w_min"] + np.arange(33) * got["w_step"]
    assert v[-1] <= 0.35 * 2048 + 1e-9 and v[0] >= 0.25 * 2048 - 1e-9 and abs(w).max() <= 0.2 * 0.1 * 65536 / (2 * np.pi)
    # the limits cut the window; the call's own caps cut it too
    assert win(0.48, 0.0, (0.0, 0.5), (-1.0, 1.0), (0.5, 2.0), 0.1, 0.05, 3, 1) == dict(n_v=3, n_w=1, v_min=881, v_step=71, w_min=-208, w_step=0)
    fast = win(2.0, 0.0, (-5.0, 5.0), (-50.0, 50.0), (100.0, 1000.0), 0.1, 0.05, 5, 5)
    assert fast == dict(n_v=5, n_w=5, v_min=-1024, v_step=512, w_min=-16384, w_step=8192)
    # narrower than its count, and narrower than one unit
    assert win(0.0, 0.0, (0.0, 0.5), (-1.0, 1.0), (0.01, 0.0), 0.1, 0.05, 9, 33) == dict(n_v=3, n_w=1, v_min=0, v_step=1, w_min=0, w_step=0)
    assert win(0.1001, 0.3, (0.0, 0.5), (-1.0, 1.0), (0.0, 0.0), 0.1, 0.05, 9, 33) == dict(n_v=1, n_w=1, v_min=205, v_step=0, w_min=313, w_step=0)
    # the current speed outside the limits: the nearest limit
    assert win(0.9, 0.0, (0.0, 0.5), (-1.0, 1.0), (0.5, 2.0), 0.1, 0.05, 9, 1)["v_min"] == 1024 and win(0.9, 0.0, (0.0, 0.5), (-1.0, 1.0), (0.5, 2.0), 0.1, 0.05, 9, 1)["n_v"] == 1
    for bad in (dict(dt=0.0), dict(res=0.0), dict(n_v=0), dict(n_w=0)):
        kw = dict(dict(dt=0.1, res=0.05, n_v=9, n_w=33), **bad)
        with pytest.raises(binding.SsfError):
            win(0.3, 0.0, (0.0, 0.5), (-1.0, 1.0), (0.5, 2.0), **kw)
    # whatever comes out is a lattice the call accepts
    for got in (fast, win(-0.2, 3.0, (-0.3, 0.5), (-4.0, 4.0), (1.0, 8.0), 0.05, 0.1, 256, 1024)):
        v = got["v_min"] + np.arange(got["n_v"]) * got["v_step"]
        w = got["w_min"] + np.arange(got["n_w"]) * got["w_step"]
        assert abs(v).max() <= 1024 and abs(w).max() <= 16384 and 1 <= got["n_v"] <= 256 and 1 <= got["n_w"] <= 1024


def test_the_units_helper():
    u = binding.Fusion.nav_steer_units
    assert u((0.0, 0.0, 0.0), 0.05).tolist() == [[0, 0, 0]]
    assert u((0.025, 0.125, np.pi / 2), 0.05).tolist() == [[512, 2560, 16384]]          # the centre of cell (0, 2), facing +iy
    assert u([(-0.01, 0.05, -np.pi / 2), (1.0, 2.0, np.pi)], 0.25).tolist() == [[-41, 204, 49152], [4096, 8192, 32768]]
    assert u((0.0, 0.0, 2 * np.pi - 1e-9), 0.05)[0, 2] == 0 and u((0.0, 0.0, -1e-9), 0.05)[0, 2] == 0      # a whole turn wraps to 0
    assert u((1.0, 2.0, -0.1), 0.05).dtype == np.int32 and u((1.0, 2.0, -0.1), 0.05)[0, 2] == sr.units(1.0, 2.0, -0.1, 0.05)[2] == 64493
    with pytest.raises(binding.SsfError):
        u((0.0, 0.0), 0.05)
    with pytest.raises(binding.SsfError):
        u((0.0, 0.0, 0.0), 0.0)


# ---- hand cases of the restatement ---------------------------------------------------------------------------------------------
def corridor():
    """5 x 12: row 2 free in columns 1 .. 10, everything else occupied; dist2 4 on the free cells"""
    s = np.full((5, 12), 100, np.int8)
    s[2, 1:11] = 0
    return s, np.where(s == 0, 4, 0).astype(np.int32)


def run(poses, grid=None, cost=None, targets=None, **kw):
    state, dist2 = corridor() if grid is None else grid
    c = sr.params(width=state.shape[1], height=state.shape[0], n_poses=len(poses), **dict(dict(cost_weight=0 if cost is None else 1), **kw))
    return sr.rollouts(state, dist2, cost, np.array(poses, np.int32), targets, c)


ONE = dict(n_v=1, n_w=1, v_step=0, w_step=0)                           # a lattice of one candidate: v_min, w_min


def test_a_straight_run_down_a_corridor():
    """heading 0: C = 16384, so a step is exactly v; from the centre of cell 1 (x = 1536) ten steps of 512 end at 6656, in cell 6"""
    got = run([sr.centre(1, 2)], v_min=512, w_min=0, n_steps=10, **ONE)
    assert got["cand_free"].tolist() == [[10]] and got["cand_end"].tolist() == [[[6656, 2560, 0]]] and got["cand_min_d"].tolist() == [[4]]
    assert got["best"].tolist() == [0] and got["best_cmd"].tolist() == [[512, 0]] and got["best_len"].tolist() == [11] and got["pose_status"].tolist() == [0]
    assert got["best_score"].tolist() == [60] == got["cand_score"].ravel().tolist()          # clear 64 - 4, speed 512 - 512
    assert got["best_traj"][0, :, 0].tolist() == list(range(1536, 6657, 512)) and (got["best_traj"][0, :, 1] == 2560).all()
    assert got["cand_end_cost"].tolist() == [[sr.NO_COST]]               # no cost weight: not read
    assert got["stats"] == dict(poses_ok=1, poses_blocked=0, poses_stuck=0, candidates=1, admissible=1, collided=0, steps_taken=10, windows_staged=1,
                                windows_global=0)
    # twenty steps: the 19th would enter cell 11 (x = 11264), a wall; the rollout ends in cell 10 after 18
    got = run([sr.centre(1, 2)], v_min=512, w_min=0, n_steps=20, **ONE)
    assert got["cand_free"].tolist() == [[18]] and got["cand_end"].tolist() == [[[10752, 2560, 0]]] and got["stats"]["collided"] == 1
    assert got["best_len"].tolist() == [19] and got["best_score"].tolist() == [60]      # it collided later than need = 2 + 4: scored where it stopped
    # backwards: heading 0, v = -512, from cell 10: x = 1024 after 19 steps is still cell 1 (the cell is a floor), the 20th enters cell 0
    got = run([sr.centre(10, 2)], v_min=-512, w_min=0, n_steps=20, **ONE)
    assert got["cand_free"].tolist() == [[19]] and got["cand_end"].tolist() == [[[1024, 2560, 0]]]


def test_a_pure_rotation():
    got = run([sr.centre(5, 2, 65000)], v_min=0, w_min=1000, n_steps=5, **ONE)
    assert got["cand_free"].tolist() == [[5]] and got["cand_end"].tolist() == [[[5632, 2560, 4464]]]      # (65000 + 5000) - 65536
    assert got["best_traj"][0, :, 2].tolist() == [65000, 464, 1464, 2464, 3464, 4464] and got["best_score"].tolist() == [60]
    assert got["stats"]["collided"] == 0 and got["stats"]["steps_taken"] == 5


def test_a_diagonal_step_between_two_obstacles_that_share_a_corner_is_blocked():
    """heading 8192 = 45 degrees: k = 128, C = S = 11585, a step of 1024 moves (724, 724): from the centre of (1, 1) into (2, 2)"""
    free = (np.zeros((4, 4), np.int8), np.full((4, 4), 3, np.int32))
    kw = dict(v_min=1024, w_min=0, n_steps=2, min_free_steps=0, brake_div=0, **ONE)
    got = run([sr.centre(1, 1, 8192)], grid=free, **kw)
    assert got["cand_free"].tolist() == [[2]] and got["cand_end"].tolist() == [[[2984, 2984, 8192]]]
    for blocked in ([(2, 1), (1, 2)], [(2, 1)], [(1, 2)]):
        s = free[0].copy()
        for ix, iy in blocked:
            s[iy, ix] = 100
        got = run([sr.centre(1, 1, 8192)], grid=(s, free[1]), **kw)
        assert got["cand_free"].tolist() == [[0]] and got["cand_end"].tolist() == [[[1536, 1536, 8192]]], blocked
        assert got["best"].tolist() == [0] and got["best_len"].tolist() == [1]           # need = 0: admissible where it stands
    s = free[0].copy()
    s[2, 2] = 100                                                        # the cell itself
    assert run([sr.centre(1, 1, 8192)], grid=(s, free[1]), **kw)["cand_free"].tolist() == [[0]]


def test_a_start_on_a_blocked_cell_and_outside_the_grid():
    got = run([sr.centre(0, 2, 77), (-1, 2560, 0), (12 * 1024, 2560, 0), (5632, 5 * 1024, 65536 + 5)], n_v=2, n_w=2, n_steps=3)
    assert got["pose_status"].tolist() == [2, 1, 1, 1] and (got["cand_free"] == 0).all() and (got["cand_min_d"] == -1).all()
    assert (got["cand_score"] == -1).all() and (got["best"] == -1).all() and (got["best_cmd"] == 0).all() and (got["best_score"] == -1).all()
    assert (got["best_len"] == 0).all() and (got["n_admissible"] == 0).all() and (got["cand_end_cost"] == sr.NO_COST).all()
    assert got["cand_end"][0].tolist() == [[512, 2560, 77]] * 4 and got["cand_end"][3].tolist() == [[5632, 5120, 5]] * 4
    assert got["stats"] == dict(poses_ok=0, poses_blocked=4, poses_stuck=0, candidates=16, admissible=0, collided=16, steps_taken=0, windows_staged=0,
                                windows_global=0)
    # min_dist2 above the corridor's clearance: nothing is traversable
    assert run([sr.centre(5, 2)], min_dist2=5, n_steps=3)["pose_status"].tolist() == [2]
    # unknown cells: traversable only when allowed
    s, d = corridor()
    s[2, 5] = -1
    d[2, 5] = 4
    assert run([sr.centre(5, 2)], grid=(s, d), n_steps=3)["pose_status"].tolist() == [2]
    assert run([sr.centre(5, 2)], grid=(s, d), n_steps=3, allow_unknown=1)["pose_status"].tolist() == [0]


def test_a_collision_at_exactly_need_and_one_step_earlier():
    """v = 512 with brake_div 128 and min_free_steps 2: need = 2 + 4 = 6.  The wall cell 11 begins at x = 11264: from 7680 the seventh
    step hits it (6 free: admissible); from 8192 the sixth does (5 free: not)"""
    got = run([(7680, 2560, 0), (8192, 2560, 0)], v_min=512, w_min=0, n_steps=20, **ONE)
    assert got["cand_free"].ravel().tolist() == [6, 5] and got["cand_score"].ravel().tolist() == [60, -1]
    assert got["pose_status"].tolist() == [0, 3] and got["n_admissible"].tolist() == [1, 0] and got["best_len"].tolist() == [7, 0]
    assert got["stats"]["poses_stuck"] == 1 and got["stats"]["collided"] == 2
    # need is capped at n_steps: with 5 steps both run free to the end and both are admissible
    got = run([(7680, 2560, 0), (8192, 2560, 0)], v_min=512, w_min=0, n_steps=5, **ONE)
    assert got["cand_free"].ravel().tolist() == [5, 5] and got["pose_status"].tolist() == [0, 0]
    # no braking term: need = 2
    assert run([(8192, 2560, 0)], v_min=512, w_min=0, n_steps=20, brake_div=0, **ONE)["pose_status"].tolist() == [0]


def test_a_negative_midpoint_sum():
    """h = 0, w = -2048: 2 h + w + 64 = -1984, >> 7 is the floor -16 (not -15), & 1023 = 1008: the midpoint heading -1024 units.
    C[1008] = 16305, S[1008] = -1606: (1024 * 16305 + 8192) >> 14 = 1019, (1024 * -1606 + 8192) >> 14 = -100 (a floor again)"""
    got = run([sr.centre(5, 2, 0)], v_min=1024, w_min=-2048, n_steps=1, **ONE)
    assert got["cand_free"].tolist() == [[1]] and got["cand_end"].tolist() == [[[5632 + 1019, 2560 - 100, 65536 - 2048]]]


def test_the_heading_wraps_at_65535():
    """h = 65535, w = 1: 2 h + w + 64 = 131135, >> 7 = 1024, & 1023 = 0: along +ix; then h = 0, then 1"""
    got = run([sr.centre(5, 2, 65535)], v_min=1024, w_min=1, n_steps=2, **ONE)
    assert got["best_traj"][0].tolist() == [[5632, 2560, 65535], [6656, 2560, 0], [7680, 2560, 1]]
    # a heading beyond one turn is taken & 0xFFFF on the way in
    assert run([sr.centre(5, 2, 65536 + 65535)], v_min=1024, w_min=1, n_steps=2, **ONE)["best_traj"][0].tolist() == got["best_traj"][0].tolist()
    assert run([sr.centre(5, 2, -1)], v_min=1024, w_min=1, n_steps=2, **ONE)["best_traj"][0].tolist() == got["best_traj"][0].tolist()


def test_a_tie_on_the_score_goes_to_the_smaller_index():
    kw = dict(n_v=1, v_min=0, v_step=0, n_steps=3, clear_weight=0, speed_weight=0, turn_weight=1)
    got = run([sr.centre(5, 2)], n_w=4, w_min=-300, w_step=200, **kw)    # w = -300, -100, 100, 300
    assert got["cand_score"].tolist() == [[300, 100, 100, 300]] and got["best"].tolist() == [1] and got["best_cmd"].tolist() == [[0, -100]]
    assert sr.tied_poses(got) == [0]
    got = run([sr.centre(5, 2)], n_w=3, w_min=-200, w_step=100, **kw)    # w = -200, -100, 0: no tie
    assert got["cand_score"].tolist() == [[200, 100, 0]] and got["best"].tolist() == [2] and sr.tied_poses(got) == []


def test_the_score_terms():
    """cost at the end cell, the target term in the field's unit, and an unreached end"""
    s, d = corridor()
    cost = np.full((5, 12), sr.NO_COST, np.uint32)
    cost[2, 1:10] = 10 * (9 - np.arange(1, 10))                           # the goal is cell 9; cell 10 is free but the field did not reach it
    targets = np.array([[9 * 1024 + 512, 3 * 1024 + 512]], np.int32)
    kw = dict(n_v=3, n_w=1, v_min=0, v_step=512, w_min=0, w_step=0, n_steps=4, cost_weight=2, target_weight=3)
    got = run([sr.centre(5, 2)], grid=(s, d), cost=cost, targets=targets, **kw)
    # v = 0 stays in cell 5 (cost 40), v = 512 ends at x = 7680 (cell 7, cost 20), v = 1024 at 9728 (cell 9, cost 0)
    assert got["cand_end_cost"].tolist() == [[40, 20, 0]] and got["cand_end"][0, :, 0].tolist() == [5632, 7680, 9728]
    # target (9728, 3584): dx = 4096, 2048, 0; dy = 1024: (10 max + 4 min) >> 10 = 44, 24, 10
    assert got["cand_score"].tolist() == [[2 * 40 + 3 * 44 + 60 + 1024, 2 * 20 + 3 * 24 + 60 + 512, 0 + 3 * 10 + 60 + 0]] and got["best"].tolist() == [2]
    got = run([sr.centre(6, 2)], grid=(s, d), cost=cost, targets=targets, **kw)
    assert got["cand_end_cost"].tolist() == [[30, 10, sr.NO_COST]] and got["cand_score"][0, 2] == -1 and got["best"].tolist() == [1]      # cell 10: unreached


# ---- the guard against vacuous GPU tests -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", sr.GUARDED)
def test_no_guarded_scene_of_the_gpu_file_is_vacuous(scene):
    i, got = sr.scene(scene), sr.case_reference(scene)
    s, c = got["stats"], i["c"]
    assert s["collided"] > 0 and 0 < s["admissible"] < s["candidates"], s
    assert (got["pose_status"] == 3).any() and (got["pose_status"] == 2).any() and (got["pose_status"] == 1).any() and (got["pose_status"] == 0).any()
    assert (got["best"] > 0).any()                                        # a winner that is not candidate 0
    assert sr.tied_poses(got)                                             # two candidates share the minimum score
    assert (got["cand_free"] == c["n_steps"]).any() and ((got["cand_free"] > 0) & (got["cand_free"] < c["n_steps"])).any()
    assert ((got["cand_score"] == -1) & (got["cand_free"] > 0)).any()     # inadmissible although it moved
    assert (got["cand_end_cost"] == sr.NO_COST).any() and (got["cand_end_cost"] != sr.NO_COST).any()
    assert (i["poses"][:, 0] & 1023 == 0).any() and (i["poses"][:, 0] & 1023 == 1023).any() and (i["poses"][:, 2] > 65535).any()


def test_what_a_launch_stages():
    """the restatement's copy of the library's choice: small windows always, large ones while the launch is resident at once"""
    c = sr.params(n_poses=4096)                                           # R = 17: 1225 cells, 9 KiB with the table
    assert sr.stage_cells(c) == sr.LDS_CELLS and sr.stage_cells(dict(c, walk=1)) == 0
    slow = sr.params(n_v=16, n_w=16, v_min=0, v_step=13, w_min=-480, w_step=64, n_steps=256)      # R = 50: 10201 cells, 44 KiB: three workgroups a CU
    assert sr.reach(slow) == 50 and sr.stage_cells(dict(slow, n_poses=16)) == sr.LDS_CELLS == sr.stage_cells(dict(slow, n_poses=768))
    assert sr.stage_cells(dict(slow, n_poses=769)) == 4056 == sr.stage_cells(dict(slow, n_poses=4096))


def test_the_shapes_of_the_gpu_file_are_the_ones_asked_for():
    ks = {sr.scene(nm)["c"]["n_v"] * sr.scene(nm)["c"]["n_w"] for nm in sr.GPU_CASES}
    assert {1, 63, 64, 65, 256, 257} <= ks
    assert {1, 2, 256} <= {sr.SCENES[nm][2].get("n_steps", 32) for nm in sr.GPU_CASES}
    assert {1, 3, 257} <= {sr.SCENES[nm][2]["n_poses"] for nm in sr.GPU_CASES}
    assert {(1, 1), (33, 31), (65, 64)} <= {sr.SCENES[nm][:2] for nm in sr.GPU_CASES}
    assert any(sr.SCENES[nm][2].get("v_min", 0) < 0 for nm in sr.GPU_CASES)                   # reverse candidates
    assert any(sr.SCENES[nm][2].get("n_v") == 1 and sr.SCENES[nm][2].get("v_step") == 0 for nm in sr.GPU_CASES)
    big = sr.big_scene()
    assert big["c"]["n_steps"] == 256 and sr.lattice(big["c"])[2] == 1024 and 120 * 120 > sr.LDS_CELLS >= 119 * 120


# ---- replay.py and the C++ surface ---------------------------------------------------------------------------------------------
def test_the_replay_options_parse():
    base = ["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-plan-goal", "1.0", "2.0"]
    assert replay.nav_steer_of(replay.parse_args(base + ["--nav-steer"])) == dict(horizon=32, speed=0.5)
    a = replay.parse_args(base + ["--nav-steer", "--nav-steer-horizon", "64", "--nav-steer-speed", "0.25", "--nav-live"])
    assert replay.nav_steer_of(a) == dict(horizon=64, speed=0.25) and a.nav_live
    assert replay.nav_steer_of(replay.parse_args(base)) is None
    frontier = ["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-plan-frontier", "--nav-steer"]
    assert replay.nav_steer_of(replay.parse_args(frontier)) == dict(horizon=32, speed=0.5)
    for bad in (["--nav-steer-horizon", "8"], ["--nav-steer-speed", "0.3"], ["--nav-steer", "--nav-steer-horizon", "0"], ["--nav-steer", "--nav-steer-horizon", "257"],
                ["--nav-steer", "--nav-steer-speed", "0"], ["--nav-steer", "--nav-steer-speed", "-1"]):
        with pytest.raises(SystemExit):
            replay.parse_args(base + bad)
    with pytest.raises(SystemExit):                                      # without a plan there is no field to steer down
        replay.parse_args(["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-steer"])
    with pytest.raises(ValueError, match="nav_steer needs nav_plan"):
        replay.replay(None, [], nav_grid_dir="grids", nav_steer=dict(horizon=32, speed=0.5))
    assert replay.steer_lattice(0.5, 0.05) == dict(n_v=9, v_min=0, v_step=128) and replay.steer_lattice(5.0, 0.05) == dict(n_v=9, v_min=0, v_step=128)
    assert replay.steer_lattice(0.001, 0.05) == dict(n_v=1, v_min=2, v_step=0)
    # the camera at map (1, 0, 2) looking along map z, the grid frame y = map z with its corner at (-1.2, 0, -0.2)
    grid = np.array([1, 0, 0, 0, 0, -1, 0, 1, 0, -1.2, 0, -0.2], np.float32)
    cam = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 1.0, 0.0, 2.0], np.float32)
    assert replay.steer_pose(grid, 0.05, cam).tolist() == [[int(np.floor((1.0 + np.float32(1.2)) / 0.05 * 1024)), int(np.floor((2.0 + np.float32(0.2)) / 0.05 * 1024)), 16384]]


def test_ssf_hpp_steering_members_compile_and_link_against_the_steer_library(steer_lib, tmp_path):
    libdir = os.path.dirname(steer_lib.path)
    exe = str(tmp_path / "navsteer_smoke")
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "navsteer_smoke.cpp"),
           "-o", exe, "-L", libdir, "-lssf_hip_steer", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    # the two host helpers run before the program needs a device: they agree with the binding's
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120).stdout
    win = binding.Fusion.nav_steer_window(0.3, 0.0, (0.0, 0.5), (-1.0, 1.0), (0.5, 2.0), 0.1, float(np.float32(0.05)), 9, 33)
    assert "window " + " ".join("%s=%d" % (k, win[k]) for k in ("n_v", "n_w", "v_min", "v_step", "w_min", "w_step")) in out, out
    x, y, h = binding.Fusion.nav_steer_units((1.0, 2.0, -0.1), float(np.float32(0.05)))[0]
    assert "units x=%d y=%d heading=%d" % (x, y, h) in out, out


# ---- the guards of the scenes beyond the room: the mixed launch, the largest lattice, the widest scores, foreign grids -------------
def window_cells(i, q):
    c, R = i["c"], sr.reach(i["c"])
    cx, cy = int(i["poses"][q, 0]) >> 10, int(i["poses"][q, 1]) >> 10
    return (min(cx + R, c["width"] - 1) - max(cx - R, 0) + 1) * (min(cy + R, c["height"] - 1) - max(cy - R, 0) + 1)


def test_the_mixed_scene_stages_some_windows_and_walks_others():
    i, got = sr.scene_reference("mixed", sr.mixed_scene)
    c, s = i["c"], got["stats"]
    assert len(i["poses"]) == 1281 and c["n_v"] * c["n_w"] == 16 and sr.reach(c) == 39
    assert sr.stage_cells(c) == 4056 and sr.stage_cells(dict(c, n_poses=1280)) == sr.LDS_CELLS == 14336
    assert (window_cells(i, sr.MIXED_EDGE_STAGED), window_cells(i, sr.MIXED_EDGE_WALKED)) == (78 * 52, 78 * 53) == (4056, 4134)
    assert window_cells(i, sr.MIXED_CORNER) == 41 * 41 and window_cells(i, sr.MIXED_CENTRAL) == 78 * 79
    assert (got["pose_status"][:4 + sr.MIXED_LIVE] == 0).sum() >= 200 and (got["pose_status"][:4] == 0).all()
    assert s["windows_staged"] >= 100 and s["windows_global"] >= 100 and s["windows_staged"] + s["windows_global"] == s["poses_ok"] + s["poses_stuck"]
    assert s["collided"] > 0 and 0 < s["admissible"] < s["candidates"] and (got["best"] > 0).any()
    assert int(got["cand_free"][sr.MIXED_CENTRAL].max()) == 38 and int(got["cand_free"][sr.MIXED_EDGE_WALKED].max()) == 38      # arcs that cross the window
    assert (got["pose_status"][4 + sr.MIXED_LIVE:] == 1).any() and (got["pose_status"][4 + sr.MIXED_LIVE:] == 2).any()
    # one pose fewer: the same poses, every window staged
    j = sr.mixed_scene(1280)
    assert (j["poses"] == i["poses"][:1280]).all() and got["pose_status"][1280] in (1, 2)         # (the pose dropped was not live)


def test_the_largest_lattice_has_its_last_candidate_among_the_minima():
    i, got = sr.scene_reference(("lattice", False), lambda: sr.lattice_scene(False))
    assert i["c"]["n_v"] * i["c"]["n_w"] == 65536 and got["cand_score"].shape == (2, 65536)
    assert i["state"][15, 0] == 100 and not i["state"][15, 1:4].any() and not i["state"][15, 22:27].any()      # the wall behind, the floor ahead
    assert got["best"][0] == 65535 and got["best_score"][0] == 0 and 256 < got["best"][1] < 65535 and got["best_score"][1] > 0 and not sr.tied_poses(got)
    assert (got["cand_score"][0, :65535] > 0).all() and got["stats"]["collided"] > 0 and got["cand_score"][1, 65535] == -1
    i, got = sr.scene_reference(("lattice", True), lambda: sr.lattice_scene(True))
    assert got["best"].tolist() == [0, 65280] and sr.tied_poses(got) == [0, 1] and (got["cand_score"][:, 65535] == got["best_score"]).all()
    assert int((got["cand_score"][0] == 0).sum()) == 512 and int((got["cand_score"][1] == 0).sum()) == 256 and (got["cand_score"][1, :256] == -1).all()
    assert 0 < got["n_admissible"][1] < 65536 == got["n_admissible"][0]


def test_the_widest_scores_pass_2_to_the_41_and_stay_below_2_to_the_44():
    i, got = sr.scene_reference("wide", sr.wide_scene)
    c = i["c"]
    assert all(c[k] == 1000 for k in ("cost_weight", "target_weight", "clear_weight", "speed_weight", "turn_weight")) and c["clearance_cap"] == 1 << 20
    top = int(got["cand_score"].max())
    assert 1 << 41 < top < 1 << 44 and top == int(got["cand_score"].astype(object).max())
    assert (got["pose_status"] == 0).sum() >= 5 and int(got["best_score"].max()) > 1 << 41
    reached = got["cand_end_cost"][got["cand_score"] >= 0]
    assert int(reached.max()) == 0xFFFFFFFE and (got["cand_end_cost"][got["pose_status"] == 0] == sr.NO_COST).any()
    assert (i["cost"] == sr.NO_COST).any() and int(i["cost"].min()) >= 0xFFFF0000
    assert ((got["cand_min_d"] == 0) & (got["cand_score"] >= 0)).any()                       # dist2 0 along an admissible arc: the whole cap counts
    t = i["targets"].astype(np.int64)
    assert {(sr.I32_MIN, sr.I32_MAX), (sr.I32_MAX, sr.I32_MIN)} <= {tuple(r) for r in t.tolist()}
    # the target term alone passes 32 bits: 1000 * ((10 * 2^31 + 4 * 2^31) >> 10) is about 2^34.8
    far = np.abs(got["cand_end"][0, 0, :2].astype(np.int64) - t[0])
    assert 1000 * ((10 * int(far.max()) + 4 * int(far.min())) >> 10) > 1 << 34
    # the extreme poses: outside, their ends are the poses with the heading masked, and the live poses are as without them
    at = [q for q in range(len(i["poses"])) if tuple(i["poses"][q]) in sr.EXTREME_POSES]
    assert at == [2, 5, len(i["poses"]) - 1] and (got["pose_status"][at] == 1).all()
    assert got["cand_end"][at, 0].tolist() == [[sr.I32_MIN, 0, 0], [sr.I32_MAX, sr.I32_MAX, 65535], [0, sr.I32_MIN, 0]]
    _, alone = sr.scene_reference("wide, live only", lambda: sr.wide_scene(False))
    live = [q for q in range(len(i["poses"])) if q not in at]
    # (the targets go round by pose index, so only what does not read them is compared here; the GPU test gives each pose its target)
    for nm in ("pose_status", "n_admissible", "cand_free", "cand_min_d", "cand_end", "cand_end_cost"):
        assert (got[nm][live] == alone[nm]).all(), nm


@pytest.mark.parametrize("h,w", pr.FOREIGN_SIZES)
@pytest.mark.parametrize("allow", [0, 1])
def test_the_rollouts_on_a_foreign_grid_meet_its_odd_values(h, w, allow):
    """cells of a state outside {0, -1, 100} and of negative dist2 stop arcs; dist2 above the cap counts as the cap"""
    i, got = sr.scene_reference(("foreign", h, w, allow), lambda: sr.foreign_scene(h, w, allow))
    c, s = i["c"], got["stats"]
    assert s["poses_ok"] >= 8 and s["collided"] > 0 and 0 < s["admissible"] < s["candidates"] and got["pose_status"][-2:].tolist() == [2, 1]
    assert (got["cand_min_d"] == c["clearance_cap"]).any() and int(i["dist2"].max()) == sr.I32_MAX and int(i["dist2"].min()) == sr.I32_MIN
    cost = i["cost"]
    run = lambda state, dist2: sr.rollouts(state, dist2, cost, i["poses"], None, dict(c, cost_weight=0))["cand_free"]
    free = got["cand_free"]
    plain_state, plain_dist2 = pr.plain_grid(i["state"], i["dist2"])
    assert (run(plain_state, i["dist2"]) > free).any()                    # an odd state ended an arc
    assert (run(i["state"], np.where(i["dist2"] < 0, 1, i["dist2"])) > free).any()          # a negative dist2 did
    # hand cases: state 50 and -2 are walls whether unknown cells are allowed or not; a negative dist2 is below min_dist2 = 0
    for odd in (1, 50, 99, 101, 127, -2, -128):
        s3, d3 = np.zeros((3, 6), np.int8), np.full((3, 6), 5, np.int32)
        s3[:, 3] = odd
        r = run_hand(s3, d3, allow)
        assert r["cand_free"].tolist() == [[1]] and r["cand_end"][0, 0, 0] >> 10 == 2, odd
    s3, d3 = np.zeros((3, 6), np.int8), np.full((3, 6), 5, np.int32)
    d3[:, 3] = -1
    assert run_hand(s3, d3, allow)["cand_free"].tolist() == [[1]]
    d3[:, 3] = sr.I32_MAX                                                # above the cap: the cap
    r = run_hand(s3, d3, allow)
    assert r["cand_free"].tolist() == [[4]] and r["cand_min_d"].tolist() == [[5]]
    d3[:] = sr.I32_MAX
    assert run_hand(s3, d3, allow)["cand_min_d"].tolist() == [[20]]


def run_hand(state, dist2, allow):
    """one candidate straight along row 1 from cell 1 of a 3 x 6 grid, four steps of one cell"""
    c = sr.params(width=6, height=3, n_poses=1, n_v=1, n_w=1, v_min=1024, v_step=0, w_min=0, w_step=0, n_steps=4, min_free_steps=0, brake_div=0,
                  cost_weight=0, allow_unknown=allow, clearance_cap=20)
    return sr.rollouts(state, dist2, None, np.array([sr.centre(1, 1)], np.int32), None, c)
