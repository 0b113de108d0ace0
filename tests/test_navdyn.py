"""Steering among movers (include/ssf_navdyn.h) without a GPU: the rule by hand on the restatement (tests/navdyn_ref.py), the restatement
without movers against the disc's and the footprint's, the tracker in Python against ssf.hpp's and the restatement's, the blobs'
restatement by hand, who exports the entry points, the header on its own, the struct layouts of the binding, the refusals that need no
device, replay.py's options, and guards that the scenes of the GPU file show what they are there to show: among them the touching
discs by hand, and for six wrong rules (navdyn_ref.WRONG_RULES) a scene of the GPU file whose reference each of them changes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import navdyn_ref as dr
import navfoot_ref as fr
import navlive_ref as lr
import navsteer_ref as sr
from conftest import ROOT
from supersurfel_fusion_amd import binding

INCLUDE = os.path.join(ROOT, "include")
OLDER = ("NAVCARVE_LIB", "NAV_LIB", "EXPLORE_LIB", "DRIVE_LIB", "LIVE_LIB", "STEER_LIB", "FOOT_LIB", "POSE_LIB")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


@pytest.fixture(scope="module")
def dyn_lib(product_lib):
    return binding.load_dyn()


# ---- who exports what ----------------------------------------------------------------------------------------------------------
def test_the_dyn_library_exports_its_own_symbols_and_all_of_the_pose_library(dyn_lib, product_lib, oracle_lib):
    """libssf_hip_dyn.so = libssf_hip_pose.so's objects + ssf_navdyn.hip; the older tables and the oracle hold no name of it"""
    have, pose = exported(dyn_lib.path), exported(binding.POSE_LIB)
    hip_ids = lambda names: {nm for nm in names if nm.startswith("__hip_cuid_")}         # one per translation unit, named by content
    for names in (binding.NAVDYN_SYMBOLS, binding.NAVPOSE_SYMBOLS, binding.NAVFOOT_SYMBOLS, binding.NAVSTEER_SYMBOLS, binding.NAVLIVE_SYMBOLS,
                  binding.NAVPATH_SYMBOLS, binding.NAVFRONTIER_SYMBOLS, binding.NAVPLAN_SYMBOLS, binding.NAVCARVE_SYMBOLS, binding.ABI_SYMBOLS):
        assert set(names) <= have
    assert dyn_lib.has_navdyn and dyn_lib.has_navpose and dyn_lib.has_navfoot and dyn_lib.has_navsteer and dyn_lib.has_navlive
    assert dyn_lib.backend == "hip-gfx950"
    assert pose - hip_ids(pose) <= have
    extra = have - pose - hip_ids(have)
    assert set(binding.NAVDYN_SYMBOLS) <= extra and len(binding.NAVDYN_SYMBOLS) == 5
    kernels = extra - set(binding.NAVDYN_SYMBOLS)
    assert kernels == {nm for nm in extra if "k_navdyn_" in nm}, sorted(extra)
    for k in ("k_navdyn_pack", "k_navdyn_roll", "k_navdyn_pick", "k_navdyn_foot_pack", "k_navdyn_foot_roll", "k_navdyn_foot_pick", "k_navdyn_blob_seen",
              "k_navdyn_blob_slots", "k_navdyn_blob_sum"):
        assert any(k in nm for nm in kernels), k
    for other in [exported(product_lib.path), exported(oracle_lib.path)] + [exported(getattr(binding, nm)) for nm in OLDER]:
        assert not [nm for nm in other if "navdyn" in nm]
    for load in ("load_navcarve", "load_nav", "load_explore", "load_drive", "load_live", "load_steer", "load_foot", "load_pose"):
        assert not getattr(binding, load)().has_navdyn
    assert not product_lib.has_navdyn and not oracle_lib.has_navdyn


def test_the_pose_library_exports_what_it_exported():
    """the cell tests, the roll frames and the live layer's camera moved into headers that ssf_navdyn.hip shares: the libraries before
    it gain no symbol by that"""
    have, foot = exported(binding.POSE_LIB), exported(binding.FOOT_LIB)
    extra = {nm for nm in have - foot if not nm.startswith("__hip_cuid_")}
    assert extra == set(binding.NAVPOSE_SYMBOLS) | {nm for nm in extra if "k_navpose_" in nm}, sorted(extra)
    steer, live, drive = exported(binding.STEER_LIB), exported(binding.LIVE_LIB), exported(binding.DRIVE_LIB)
    more = {nm for nm in foot - steer if not nm.startswith("__hip_cuid_")}
    assert more == set(binding.NAVFOOT_SYMBOLS) | {nm for nm in more if "k_navfoot_" in nm}, sorted(more)
    more = {nm for nm in steer - live if not nm.startswith("__hip_cuid_")}
    assert more == set(binding.NAVSTEER_SYMBOLS) | {nm for nm in more if "k_navsteer_" in nm}, sorted(more)
    assert len({nm for nm in more if "k_navsteer_" in nm and "__device_stub__" not in nm}) == 3          # pack, roll, pick: no template instance
    more = {nm for nm in live - drive if not nm.startswith("__hip_cuid_")}
    assert more == set(binding.NAVLIVE_SYMBOLS) | {nm for nm in more if "k_navlive_" in nm}, sorted(more)


def test_an_older_library_names_the_missing_symbol(product_lib):
    lib = binding.load_pose()
    assert not lib.has_navdyn
    f = binding.Fusion.__new__(binding.Fusion)                            # (no handle: the check comes before any call)
    f.L = lib
    state, dist2, poses = np.zeros((3, 3), np.int8), np.ones((3, 3), np.int32), np.zeros((1, 3), np.int32)
    with pytest.raises(binding.SsfError, match="ssf_navdyn_rollouts.*binding.load_dyn"):
        f.nav_dyn_steer(state, dist2, poses, cost_weight=0)
    with pytest.raises(binding.SsfError, match="ssf_navdyn_foot_rollouts.*binding.load_dyn"):
        f.nav_dyn_foot_steer(np.ones((3, 3), np.uint32), dist2, poses, 1, cost_weight=0)
    with pytest.raises(binding.SsfError, match="ssf_navdyn_rollouts.*binding.load_dyn"):
        f.nav_dyn_steer_device(0, 0, 3, 3, 0, 1)
    with pytest.raises(binding.SsfError, match="ssf_navdyn_blobs.*binding.load_dyn"):
        f.nav_dyn_blobs(np.ones((3, 3), np.float32), np.ones((3, 3), np.uint8), np.zeros((3, 3), np.int32))
    with pytest.raises(binding.SsfError, match="ssf_navdyn_blobs.*binding.load_dyn"):
        f.nav_dyn_blobs_device(0, 0, 0)
    with pytest.raises(binding.SsfError, match="ssf_navdyn_default_params"):
        f.nav_dyn_default_params()
    with pytest.raises(binding.SsfError, match="ssf_navdyn_rollouts.*binding.load_dyn"):
        f.nav_live_dyn_steer(np.ones((48, 64), np.float32), state, [(1, 1)], poses, binding.MoverTracker())


def test_the_symbols_stay_out_of_the_other_headers():
    for nm in binding.NAVDYN_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        for hdr in ("ssf.h", "ssf_testing.h", "ssf_navgrid.h", "ssf_navplan.h", "ssf_navlive.h", "ssf_navsteer.h", "ssf_navfoot.h", "ssf_navpose.h"):
            assert nm not in open(os.path.join(INCLUDE, hdr)).read(), (nm, hdr)
        assert nm + "(" in open(os.path.join(INCLUDE, "ssf_navdyn.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_navdyn.h"\n'
                   "int f(ssf_handle* h, const int8_t* state, const uint32_t* mask, const int32_t* dist2, const int32_t* poses, int32_t* cmd,\n"
                   "      const void* depth, const uint8_t* moving, const int32_t* label) {\n"
                   "    ssf_navsteer_params q; ssf_navsteer_out r; ssf_navsteer_stats t; ssf_navdyn_params d; ssf_navdyn_out o; ssf_navdyn_stats u;\n"
                   "    ssf_navdyn_blob_params b; ssf_navdyn_blob_stats bs;\n"
                   "    int32_t movers[SSF_NAVDYN_MAX_MOVERS * SSF_NAVDYN_MOVER_WORDS] = {0}; int32_t gap[1]; int32_t blobs[SSF_NAVDYN_MAX_BLOBS * SSF_NAVDYN_BLOB_WORDS];\n"
                   "    if (ssf_navsteer_default_params(h, &q) != SSF_OK || ssf_navdyn_default_params(h, &d) != SSF_OK) return -1;\n"
                   "    q.n_poses = 1; q.cost_weight = 0; d.n_movers = 1;\n"
                   "    r.best = 0; r.best_cmd = cmd; r.best_score = 0; r.n_admissible = 0; r.pose_status = 0; r.best_len = 0; r.best_traj = 0;\n"
                   "    r.cand_free = 0; r.cand_min_d = 0; r.cand_end = 0; r.cand_end_cost = 0; r.cand_score = 0;\n"
                   "    o.cand_hit = 0; o.cand_min_gap = 0; o.best_min_gap = gap;\n"
                   "    if (ssf_navdyn_rollouts(h, &q, &d, state, dist2, 0, poses, 0, movers, &r, &o, &t, &u) != SSF_OK) return -2;\n"
                   "    if (ssf_navdyn_foot_rollouts(h, &q, &d, 16, mask, dist2, 0, poses, 0, movers, &r, &o, &t, &u) != SSF_OK) return -3;\n"
                   "    if (ssf_navdyn_default_blob_params(h, &b) != SSF_OK) return -4;\n"
                   "    if (ssf_navdyn_blobs(h, &b, depth, moving, label, blobs, &bs) != SSF_OK) return -5;\n"
                   "    return (int)(t.poses_ok + u.hit_movers + bs.blobs_written) + gap[0]; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    classes = (("ssf_navdyn_params", binding.SsfNavDynParams), ("ssf_navdyn_out", binding.SsfNavDynOut), ("ssf_navdyn_stats", binding.SsfNavDynStats),
               ("ssf_navdyn_blob_params", binding.SsfNavDynBlobParams), ("ssf_navdyn_blob_stats", binding.SsfNavDynBlobStats))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_navdyn.h"', "int main(void) {"]
    for st, cls in classes:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for nm, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, nm, st, nm))
    lines += ['    printf("consts %d %d %d %d\\n", SSF_NAVDYN_MAX_MOVERS, SSF_NAVDYN_MOVER_WORDS, SSF_NAVDYN_MAX_BLOBS, SSF_NAVDYN_BLOB_WORDS);', "    return 0; }"]
    src = tmp_path / "off.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "off")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    rows = [l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()]
    got = {r[0]: r[1] for r in rows if r[0] != "consts"}
    for st, cls in classes:
        assert int(got[st]) == C.sizeof(cls), st
        for nm, _ in cls._fields_:
            assert int(got["%s.%s" % (st, nm)]) == getattr(cls, nm).offset, (st, nm)
    consts = tuple(int(v) for v in [r for r in rows if r[0] == "consts"][0][1:])
    assert consts == (binding.NAVDYN_MAX_MOVERS, binding.NAVDYN_MOVER_WORDS, binding.NAVDYN_MAX_BLOBS, binding.NAVDYN_BLOB_WORDS)
    assert consts == (dr.MAX_MOVERS, dr.MOVER_WORDS, dr.MAX_BLOBS, dr.BLOB_WORDS)
    assert (binding.NAVDYN_MAX_XY, binding.NAVDYN_MAX_V, binding.NAVDYN_MAX_R, binding.NAVDYN_MAX_GROW) == (dr.MAX_XY, dr.MAX_V, dr.MAX_R, dr.MAX_GROW)
    assert binding.NAVDYN_OUTPUT_NAMES == dr.DYN_OUTPUTS and tuple(nm for nm, _ in binding.SsfNavDynBlobStats._fields_) == dr.BLOB_STATS
    assert tuple(nm for nm, _ in binding.SsfNavSteerStats._fields_)[:7] + tuple(nm for nm, _ in binding.SsfNavDynStats._fields_) == dr.STATS


def test_the_refusals_that_need_no_device(dyn_lib):
    L = dyn_lib.lib
    assert L.ssf_navdyn_default_params(None, None) != 0 and L.ssf_navdyn_default_blob_params(None, None) != 0
    assert L.ssf_navdyn_rollouts(None, None, None, None, None, None, None, None, None, None, None, None, None) != 0
    assert L.ssf_navdyn_foot_rollouts(None, None, None, 16, None, None, None, None, None, None, None, None, None, None) != 0
    assert L.ssf_navdyn_blobs(None, None, None, None, None, None, None) != 0
    t = binding.MoverTracker()
    with pytest.raises(binding.SsfError):
        t.update(np.zeros((1, 8), np.int32), 0)
    with pytest.raises(binding.SsfError):
        t.update(np.zeros((65, 8), np.int32), 1)
    assert t.update(np.zeros((0, 8), np.int32)).shape == (0, 6)


# ---- the rule by hand ------------------------------------------------------------------------------------------------------------------
def hand(r, **kw):
    s = dr.hand_scene(r)
    c = dict(s["c"], **kw)
    return dr.rollouts(s["state"], s["dist2"], None, s["poses"], None, s["movers"], c), c


def test_the_hand_case_of_the_issue():
    """an open grid, the pose at the centre of cell (10, 10) heading 0, v in {0, 512}, w = 0, need = 2 + 512 / 128 = 6; the mover
    (14848, 12800, 0, -256, r, 0) comes down the column the fast candidate reaches at step 7"""
    # by hand: the fast candidate is at x = 10752 + 512 s, y = 10752; the mover at (14848, 12800 - 256 s)
    for s, d2 in ((6, 1310720), (7, 327680)):
        assert (10752 + 512 * s - 14848) ** 2 + (10752 - (12800 - 256 * s)) ** 2 == d2
    assert 327680 < 600 ** 2 == 360000 <= 1310720 < 1200 ** 2
    got, c = hand(600)
    assert got["cand_free"].tolist() == [[12, 6]] and got["cand_hit"].tolist() == [[-1, 0]]
    assert got["cand_min_gap"][0, 1] == 544 == int(np.floor(np.sqrt(1310720))) - 600 and c["mover_cap"] >= 544
    assert got["cand_score"][0, 1] >= 0 and got["n_admissible"].tolist() == [2]                     # need = 6: still admissible
    assert got["best"].tolist() == [1] and got["best_min_gap"].tolist() == [544] and got["best_len"].tolist() == [7]
    assert got["stats"]["hit_movers"] == 1 and got["stats"]["collided"] == 1
    # the score's sixth term: 1 * ((10 * (4096 - 544)) >> 10) = 34 with every other term 0 for the fast candidate
    assert got["cand_score"][0, 1] == (10 * (4096 - 544)) >> 10 == 34
    # a cap below the gap: the gap is the cap, the term 0
    low, _ = hand(600, mover_cap=500)
    assert low["cand_min_gap"].tolist() == [[500, 500]] and low["cand_score"][0, 1] == 0
    got, _ = hand(1200)
    assert got["cand_free"].tolist() == [[12, 5]] and got["cand_hit"].tolist() == [[-1, 0]]         # hit at step 6
    assert got["cand_score"][0, 1] == -1 and got["best"].tolist() == [0] and got["best_cmd"].tolist() == [[0, 0]]      # the standing candidate wins
    # the standing candidate's gap: the mover passes it at its nearest at step 8, (14848 - 10752, 0): 4096 - 1200
    assert got["cand_min_gap"][0, 0] == 4096 - 1200 and got["best_min_gap"].tolist() == [2896]


def test_the_start_is_not_tested_and_the_first_step_is():
    """a mover on top of the robot refuses nothing by itself: the standing candidate (which re-tests its own place at step 1) is hit,
    a candidate that leaves the disc within its first step is not"""
    s = dr.hand_scene(300)
    movers = np.array([(10752, 10752, 0, 0, 300, 0)], np.int32)
    got = dr.rollouts(s["state"], s["dist2"], None, s["poses"], None, movers, s["c"])
    assert got["pose_status"].tolist() == [0] and got["cand_free"].tolist() == [[0, 12]] and got["cand_hit"].tolist() == [[0, -1]]
    assert got["cand_min_gap"].tolist() == [[4096, 512 - 300]] and got["best"].tolist() == [1]
    assert got["cand_min_gap"][0, 0] == s["c"]["mover_cap"]                                         # no committed step: the cap


def test_without_movers_the_restatement_is_the_discs_and_the_footprints():
    for scene in ("room 65x64 reverse", "K65"):
        i = sr.scene(scene)
        c = i["c"]
        cost, targets = (i["cost"] if c["cost_weight"] else None), (i["targets"] if c["target_weight"] else None)
        got = dr.rollouts(i["state"], i["dist2"], cost, i["poses"], targets, None, dict(c, mover_cap=4096, mover_weight=0))
        want = sr.case_reference(scene)
        for nm in sr.OUTPUTS:
            assert got[nm].dtype == want[nm].dtype and (got[nm] == want[nm]).all(), (scene, nm)
        assert {k: got["stats"][k] for k in sr.STATS + sr.INFORMATIVE} == {k: want["stats"][k] for k in sr.STATS + sr.INFORMATIVE}
        assert (got["cand_hit"] == -1).all() and got["stats"]["hit_movers"] == 0
        assert ((got["cand_min_gap"] == 4096) | ((got["cand_min_gap"] == -1) & (got["cand_min_d"] == -1))).all()
    i = fr.corridor_scene()
    lay = fr.cached("corridor layers", lambda: fr.layers(i["state"], 0, i["foot"], i["B"]))
    want = fr.cached("corridor rollouts", lambda: fr.rollouts(lay["free_mask"], i["B"], i["dist2"], i["cost"], i["poses"], None, i["c"]))
    got = dr.rollouts(lay["free_mask"], i["dist2"], i["cost"], i["poses"], None, None, dict(i["c"], mover_cap=0, mover_weight=0), i["B"])
    for nm in sr.OUTPUTS:
        assert (got[nm] == want[nm]).all(), nm
    assert {k: got["stats"][k] for k in sr.STATS + sr.INFORMATIVE} == {k: want["stats"][k] for k in sr.STATS + sr.INFORMATIVE}


@pytest.mark.parametrize("name", dr.GUARDED)
def test_the_random_lists_show_a_hit_an_admissible_candidate_and_a_gap(name):
    want, c = dr.scene_reference(name), dr.scene_inputs(name)["c"]
    assert dr.not_vacuous(want, c) == (True, True, True), name


def test_the_special_lists_show_what_they_are_there_to_show():
    want = dr.scene_reference("r 0 never hits")
    assert (want["cand_hit"] == -1).all() and (want["cand_min_gap"] < dr.scene_inputs("r 0 never hits")["c"]["mover_cap"]).any()
    want = dr.scene_reference("two movers one step")
    assert set(np.unique(want["cand_hit"]).tolist()) == {-1, 1}                                     # never 2: the smaller index wins
    alone = dr.scene_inputs("two movers one step")
    only2 = dr.rollouts(alone["state"], alone["dist2"], alone["cost"], alone["poses"], None, alone["movers"][[0, 2]], alone["c"])
    assert (only2["cand_hit"] == 1).any()                                                           # without mover 1, mover 2 does hit
    want = dr.scene_reference("mover on the start")
    assert (want["pose_status"] == 0).all() and (want["cand_hit"][0] == 0).any() and (want["cand_free"][0] > 0).any()
    want = dr.scene_reference("int64 path")
    assert set(np.unique(want["cand_hit"]).tolist()) >= {-1, 4, 5} and want["stats"]["admissible"] > 0
    want = dr.scene_reference("grow 4096")
    assert (want["cand_hit"] == 0).all() and (want["cand_free"] > 0).all()                           # the disc grows over every rollout
    want = dr.scene_reference("cap 0")
    assert ((want["cand_min_gap"] == 0) | (want["cand_min_gap"] == -1)).all() and (want["cand_hit"] >= 0).any()
    want = dr.scene_reference("1x1")
    assert (want["cand_min_gap"] == 0).all() and want["stats"]["poses_ok"] == 1


def test_the_footprint_scenes_stand_at_the_edges_they_name():
    """B = 1 and 32, 256 steps, 64 movers, one cell, and more poses than a pick workgroup holds with winners on both sides of it"""
    got = {name: dr.scene_inputs(name) for name in dr.FOOT_CASES}
    assert {s["B"] for s in got.values()} >= {1, 4, 8, 16, 32} and got["foot 37x53"]["foot"] == dr.FOOT and got["foot 37x53"]["B"] == 16
    assert got["foot T256"]["c"]["n_steps"] == 256 and len(got["foot B32 K512 64 movers"]["movers"]) == dr.MAX_MOVERS
    assert got["foot 1x1 B4"]["free_mask"].shape == (1, 1) and got["foot 1x1 B4"]["free_mask"][0, 0] == 15
    want = dr.scene_reference("foot 1x1 B4")
    assert want["stats"]["poses_ok"] == 1 and (want["cand_min_gap"] == 0).all()
    want = dr.scene_reference("foot T256")
    assert want["cand_free"].max() > 64                                   # a rollout that is still running long after the others ended
    for name in ("foot 300 poses K257", "300 poses K64"):
        want = dr.scene_reference(name)
        ok = np.flatnonzero(want["pose_status"] == 0)
        assert len(want["best"]) >= 300 and (ok < 256).any() and (ok >= 256).any(), name
        assert len(np.unique(want["best_min_gap"][ok[ok < 256]])) > 2 and len(np.unique(want["best_min_gap"][ok[ok >= 256]])) > 2, name
        assert (want["best_len"][ok[ok >= 256]] > 1).any(), name             # a winner past the first workgroup whose replay takes steps
    assert dr.scene_reference("foot 300 poses K257")["stats"]["poses_ok"] > 256


def test_the_mixed_scene_stages_some_windows_and_walks_the_others():
    s, want = dr.scene_inputs("mixed walks"), dr.scene_reference("mixed walks")
    assert sr.stage_cells(s["c"]) == 4056 and len(s["poses"]) == 1281 and len(s["movers"]) >= 8
    assert want["stats"]["windows_staged"] > 0 and want["stats"]["windows_global"] > 0
    assert dr.not_vacuous(want, s["c"]) == (True, True, True)
    for q in (sr.MIXED_EDGE_STAGED, sr.MIXED_EDGE_WALKED, sr.MIXED_CORNER, sr.MIXED_CENTRAL):
        assert want["pose_status"][q] == 0, q


# ---- touching discs: the strict comparisons, by hand ---------------------------------------------------------------------------------
def fast(want):
    """(cand_free, cand_hit, cand_min_gap) of a hand-made scene's fast candidate (v = 512)"""
    return tuple(int(want[nm][0, 1]) for nm in ("cand_free", "cand_hit", "cand_min_gap"))


def test_a_touching_disc_does_not_hit_and_its_gap_is_zero():
    """D2 == R_s^2 is free (step A.2 asks D2 >= R_s^2) with gap isqrt(D2) - R_s = 0; the step after it lies inside.  The fast candidate is at
    (x0 + 512 s, y0) at step s, (x0, y0) = (10752, 10752); need = 2 + 512 / 128 = 6 of 12 steps"""
    x0 = y0 = dr.X0
    assert x0 == 10752
    # static: the disc of radius 1000 at x0 + 4072: |dx| = 4072 - 512 s: 1000 at s = 6, 488 at s = 7
    assert 4072 - 512 * 6 == 1000 and 4072 - 512 * 7 == 488 < 1000
    want = dr.scene_reference("touch static")
    assert fast(want) == (6, 0, 0) and want["cand_min_gap"][0, 0] == 4072 - 1000 == 3072 and want["cand_hit"][0, 0] == -1
    assert want["cand_score"][0, 1] == (10 * 4096) >> 10 == 40 and want["best"].tolist() == [1] and want["best_min_gap"].tolist() == [0]
    # growing: R_s = 100 s at x0 + 3060: |dx| = 3060 - 512 s: 500 = R_5 at s = 5; 12 < R_6 = 600 at s = 6
    assert 3060 - 512 * 5 == 500 and abs(3060 - 512 * 6) == 12 < 600 and 3060 - 512 * 4 == 1012 > 400
    want = dr.scene_reference("touch growing")
    assert fast(want) == (5, 0, 0) and want["cand_min_gap"][0, 0] == 3060 - 100 * 12
    # off the axis: (dx, dy) = (2136 - 512 s, 800): (600, 800) at s = 3, 600^2 + 800^2 = 1000^2; (88, 800) at s = 4
    assert (2136 - 512 * 3, 600 ** 2 + 800 ** 2) == (600, 1000 ** 2) and 88 ** 2 + 800 ** 2 < 1000 ** 2 < 1112 ** 2 + 800 ** 2
    want = dr.scene_reference("touch pythagorean")
    assert fast(want) == (3, 0, 0)
    # a quarter turn: the static case along +y
    want = dr.scene_reference("touch quarter turn")
    assert fast(want) == (6, 0, 0) and want["cand_min_gap"][0, 0] == 3072
    assert want["cand_end"][0, 1].tolist() == [x0, y0 + 512 * 6, 16384]
    # a mover that walks: X_s = x0 + 3772 - 256 s, the robot at x0 + 512 s: |dx| = 3772 - 768 s: 1468 at s = 3, 700 = R at s = 4, 68 at s = 5.
    # The standing candidate sees |dx| = 3772 - 256 s: 700 at s = 12, the last step: all 12 steps free, gap 0
    assert 3772 - 768 * 4 == 700 and abs(3772 - 768 * 5) == 68 < 700 and 3772 - 256 * 12 == 700
    want = dr.scene_reference("touch moving")
    assert fast(want) == (4, 0, 0)
    assert (int(want["cand_free"][0, 0]), int(want["cand_hit"][0, 0]), int(want["cand_min_gap"][0, 0])) == (12, -1, 0)
    assert want["best"].tolist() == [0] and want["best_min_gap"].tolist() == [0] and want["stats"]["hit_movers"] == 1


def test_the_static_test_comes_first_and_a_refused_steps_gaps_do_not_count():
    # the wall cell (13, 10) begins at x = 13312 = x0 + 512 * 5; the disc of radius 800 at its centre 13824: |dx| = 1024 at s = 4 (free,
    # gap 224), 512 at s = 5: inside the disc AND in the wall: the rollout ended on the static test, cand_hit is -1
    assert 13 * 1024 == dr.X0 + 512 * 5 and 13824 - (dr.X0 + 512 * 4) == 1024 and 13824 - (dr.X0 + 512 * 5) == 512 < 800
    s, want = dr.scene_inputs("wall inside a disc"), dr.scene_reference("wall inside a disc")
    assert s["state"][10, 13] == 100 and fast(want) == (4, -1, 224) and want["stats"]["hit_movers"] == 0
    assert want["stats"]["collided"] == 1
    # mover 1 (radius 1000 at x0 + 3972) refuses step 6 (|dx| = 900) after a gap of 1412 - 1000 at step 5; mover 0 (radius 1000 at
    # (x0 + 3072, y0 + 1300)) is at distance 1300 at the refused step 6 and at isqrt(512^2 + 1300^2) = 1397 at step 5: the gap is 397
    assert 3972 - 512 * 6 == 900 < 1000 < 3972 - 512 * 5 == 1412 and 1397 ** 2 <= 512 ** 2 + 1300 ** 2 < 1398 ** 2
    want = dr.scene_reference("gap of a refused step")
    assert fast(want) == (5, 1, 397)


# ---- what the scenes are sensitive to ------------------------------------------------------------------------------------------------
# the references of the scenes from before the wrong rules were added to the restatement: sha256 of every output's bytes and the stats
DIGESTS = {"1x1": "4ee5cbb739ffbe73", "1x70 K297 one mover": "99b4d213c8b99c39", "37x53 K512 64 movers 70 poses": "512d41a123120328",
           "64x65 K297 T256": "743fdddea12f54c6", "97x33 K512 T1": "4eaad3ea30eeb66e", "r 0 never hits": "24d8157c34df22ca",
           "two movers one step": "4f51a47ad069b854", "mover on the start": "c9cac9b9eb542161", "int64 path": "d68e283b4552c9ac",
           "grow 4096": "e1f79390230f6d1b", "cap 0": "772544cf20db27d9", "foot 37x53": "9dc1b33bfbc4c1f0"}
# wrong rule -> (a scene of the GPU suite, an output of its reference that the rule changes)
SENSITIVE = {"hit_le": ("touch static", "cand_free"), "movers_first": ("wall inside a disc", "cand_hit"), "last_hit": ("two movers one step", "cand_hit"),
             "gap_uncommitted": ("gap of a refused step", "cand_min_gap"), "zero_based": ("touch moving", "cand_min_gap"),
             "start_tested": ("mover on the start", "cand_free")}


def test_the_default_rule_computes_what_it_computed():
    import hashlib
    import json
    for name, told in DIGESTS.items():
        want = dr.scene_reference(name)
        h = hashlib.sha256()
        for nm in dr.OUTPUTS:
            h.update(np.ascontiguousarray(want[nm]).tobytes())
        h.update(json.dumps(want["stats"], sort_keys=True).encode())
        assert h.hexdigest()[:16] == told, name


@pytest.mark.parametrize("rule", dr.WRONG_RULES)
def test_every_wrong_rule_changes_an_output_of_a_scene_the_gpu_suite_runs(rule):
    """a condition on the scenes: a kernel that followed the wrong rule would differ from the reference on the named scene's output"""
    assert set(SENSITIVE) == set(dr.WRONG_RULES)
    name, output = SENSITIVE[rule]
    assert name in dr.DISC_CASES + dr.FOOT_CASES + dr.HAND_CASES
    right, wrong = dr.scene_reference(name), dr.scene_reference(name, _wrong=rule)
    assert (right[output] != wrong[output]).any(), (rule, name, output)
    if rule == "hit_le":                                                  # every touching scene tells <= from <
        for name in dr.HAND_CASES[:5]:
            assert (dr.scene_reference(name)["cand_free"] != dr.scene_reference(name, _wrong=rule)["cand_free"]).any(), name
    if rule == "movers_first":
        assert wrong["cand_hit"][0, 1] == 0 and right["cand_hit"][0, 1] == -1 and (right["cand_free"] == wrong["cand_free"]).all()
    if rule == "gap_uncommitted":
        assert wrong["cand_min_gap"][0, 1] == 1300 - 1000


# ---- the tracker -------------------------------------------------------------------------------------------------------------------------
def test_the_tracker_by_hand():
    out = dr.tracker_case(0)
    assert out[0].tolist() == [[10000, 20000, 0, 0, 1000, 128]]                                      # nothing before it: unmatched
    assert out[1].tolist() == [[10301, 19499, 150, -251, 950, 16]]                                   # floor(301 / 2), floor(-501 / 2)
    assert out[2].tolist() == [[20000, 19499, 0, 0, 950, 128]]                                       # 9699 away, the gate is 2048
    out = dr.tracker_case(1)
    assert out[1].tolist() == [[300, 0, 100, 0, 10, 5], [300, 1, -100, 0, 10, 5], [5000, 5000, 0, 0, 10, 50]]
    out = dr.tracker_case(2)
    assert out[1].tolist() == [[1 << 23, -(1 << 23), 4096, -4096, 1 << 20, 4096]]


def test_the_python_tracker_is_the_restatements():
    for k, (cfg, updates) in enumerate(dr.TRACKER_CASES):
        t = binding.MoverTracker(*cfg)
        for (steps, rows), want in zip(updates, dr.tracker_case(k)):
            got = t.update(np.array(rows, np.int32), steps)
            assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (k, got, want)
            assert dr.movers_ok(got)
    rng = np.random.default_rng(3)
    a, b = binding.MoverTracker(3000, 200, 7, 90), dr.Tracker(3000, 200, 7, 90)
    for step in range(6):
        n = int(rng.integers(0, 9))
        table = np.zeros((n, 8), np.int32)
        table[:, 0], table[:, 1] = rng.permutation(100)[:n], rng.integers(1, 500, n)
        table[:, 2:4], table[:, 4] = rng.integers(0, 20000, (n, 2)), rng.integers(0, 2000, n)
        steps = int(rng.integers(1, 5))
        assert (a.update(table, steps) == b.update(table, steps)).all(), step


def test_the_cpp_tracker_is_the_python_tracker(dyn_lib, tmp_path):
    """tests/cpp/navdyn_smoke.cpp --tracker: ssf.hpp's MoverTracker on the shared case list, no device"""
    libdir = os.path.dirname(dyn_lib.path)
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "navdyn_smoke")
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", cpp, os.path.join(cpp, "navdyn_smoke.cpp"),
           "-o", exe, "-L", libdir, "-lssf_hip_dyn", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe, "--tracker"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "sizes params=%d out=%d stats=%d blob_params=%d blob_stats=%d mover=24 blob=32" % (
        C.sizeof(binding.SsfNavDynParams), C.sizeof(binding.SsfNavDynOut), C.sizeof(binding.SsfNavDynStats), C.sizeof(binding.SsfNavDynBlobParams),
        C.sizeof(binding.SsfNavDynBlobStats)) in r.stdout, r.stdout
    told = {(int(m.group(1)), int(m.group(2))): [[int(v) for v in row.split()] for row in re.findall(r"\(([-\d ]+)\)", m.group(3))]
            for m in re.finditer(r"case (\d+) update (\d+):(.*)", r.stdout)}
    n = 0
    for k in range(len(dr.TRACKER_CASES)):
        for u, want in enumerate(dr.tracker_case(k)):
            assert told[(k, u)] == want.tolist(), (k, u, told[(k, u)], want.tolist())
            n += 1
    assert n == len(told) == 7
    # a program that steers with the footprint alone still links against the foot library: the new members leave no reference behind
    exe2 = str(tmp_path / "navfoot_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", INCLUDE, "-I", cpp, os.path.join(cpp, "navfoot_smoke.cpp"), "-o", exe2, "-L", libdir,
                        "-lssf_hip_foot", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


# ---- the blobs' restatement ------------------------------------------------------------------------------------------------------------
def test_the_restated_back_projection_is_the_live_layers():
    for name, s in lr.scenes().items():
        c = lr.params(**s["kw"])
        gx, gy, ok = dr.grid_points(s["depth"], s["cam_pose"], s["grid_pose"], c)
        cell = lr.point_cells(s["depth"], s["cam_pose"], s["grid_pose"], c)
        with np.errstate(invalid="ignore"):
            mine = np.where(ok, np.where(ok, gy, 0).astype(np.int64) * int(c["width"]) + np.where(ok, gx, 0).astype(np.int64), -1)
        assert (mine == cell).all() and ok.any(), name


def test_the_blobs_by_hand():
    """one pixel looking along map +x from navlive_ref's boundary camera: grid = map frame, res 0.25, 8 x 4 cells, band (0, 1]"""
    c = lr.params(**lr.BOUNDARY)
    grid_pose = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    one = lambda a, dt: np.array([[a]], dt)
    # depth 1.125 from (0.25, 0.625, 0.5): the point (1.375, 0.625, 0.5) is at gx = 5.5, gy = 2.5: bx = 5632, by = 2560
    got = dr.blobs(one(1.125, np.float32), one(1, np.uint8), one(0, np.int32), grid_pose, lr.boundary_pose(0.25, 0.625, 0.5), c, min_points=1)
    assert got["blobs"].tolist() == [[0, 1, 5632, 2560, 0, 0, 0, 0]]
    assert got["stats"] == dict(pixels_member=1, pixels_valid=1, points_in_band=1, labels_seen=1, blobs_kept=1, blobs_written=1)
    for kw, stats in ((dict(mask=0), (0, 0, 0)), (dict(label=-1), (0, 0, 0)), (dict(label=1), (0, 0, 0)), (dict(depth=8.0), (1, 0, 0)),
                      (dict(z=1.5), (1, 1, 0)), (dict(x0=1.0), (1, 1, 0))):
        got = dr.blobs(one(kw.get("depth", 1.125), np.float32), one(kw.get("mask", 1), np.uint8), one(kw.get("label", 0), np.int32), grid_pose,
                       lr.boundary_pose(kw.get("x0", 0.25), 0.625, kw.get("z", 0.5)), c, min_points=1)
        assert (got["stats"]["pixels_member"], got["stats"]["pixels_valid"], got["stats"]["points_in_band"]) == stats, kw
        assert len(got["blobs"]) == 0 and got["stats"]["labels_seen"] == 0
    assert dr.ceil_sqrt(0) == 0 and dr.ceil_sqrt(25) == 5 and dr.ceil_sqrt(26) == 6 and dr.ceil_sqrt(3 ** 2 + 4 ** 2) == 5


@pytest.mark.parametrize("cam", dr.BLOB_CAMERAS)
def test_the_blob_scenes_show_what_they_are_there_to_show(cam):
    cw, ch = cam
    s, _, _, none = dr.blob_reference(cw, ch, "none", "f32")
    assert none["stats"] == dict.fromkeys(dr.BLOB_STATS, 0) and len(none["blobs"]) == 0
    _, _, _, many = dr.blob_reference(cw, ch, "many", "f32")
    if cw * ch > 5:
        assert many["stats"]["blobs_kept"] > many["stats"]["blobs_written"] == 5 and (many["blobs"][:, 1] == 1).all()
        assert (np.diff(many["blobs"][:, 0]) > 0).all()                                             # equal n: ordered by label
    if cw >= 17:
        s, _, _, cols = dr.blob_reference(cw, ch, "columns", "f32")
        st = cols["stats"]
        assert st["pixels_member"] > st["pixels_valid"] > st["points_in_band"] > 0                  # invalid depths; points outside the band or the grid
        assert st["labels_seen"] > st["blobs_kept"] >= 2                                             # a label below min_points
        n = cols["blobs"][:, 1]
        assert (np.diff(n) <= 0).all() and (cols["blobs"][:, 5] > 0).all() and (cols["blobs"][:, 6] > 0).all()      # an extent along both axes
        assert (cols["blobs"][:, 4] ** 2 >= cols["blobs"][:, 5] ** 2 + cols["blobs"][:, 6] ** 2).all()
        first = s["label"][ch // 2] == cols["blobs"][np.argmin(cols["blobs"][:, 0]), 0]              # the stripe of the smallest label starts at
        assert first[0] and (cw < 160 or first[:20].all())                                          # column 0: 20 wide at 160, across a 16-pixel tile border


def test_the_blocks_share_labels_between_tiles_and_all_are_reported():
    """the "blocks" kind: several labels of several pixels each in a tile, most of them in two tiles or four, and every one written"""
    for cw, ch in dr.BLOCK_CAMERAS:
        assert cw % 16 and ch % 16
        s, _, _, want = dr.blob_reference(cw, ch, "blocks", "f32")
        st, n = want["stats"], want["blobs"][:, 1]
        assert 20 <= st["labels_seen"] <= 64 and st["blobs_written"] == st["labels_seen"] == st["blobs_kept"], (cw, ch, st)
        assert n.min() >= 1 and n.max() == 15 and len(set(n.tolist())) >= 4, n
        assert st["pixels_member"] == cw * ch - 3                          # the three labels that are no pixel index
        odd = s["label"][(s["label"] < 0) | (s["label"] >= cw * ch)]
        assert sorted(odd.tolist()) == [-(1 << 31), cw * ch, (1 << 31) - 1] and (s["mask"] != 0).all()
    s, _, _, want = dr.blob_reference(40, 24, "blocks", "f32")
    shared, crowded = dr.blob_tiles(s)
    assert shared >= 10 and crowded >= 4, (shared, crowded)
    # one of the three pixels would contribute if its label were a pixel index: the member test decides it
    as_member = np.where((s["label"] < 0) | (s["label"] >= 40 * 24), 0, s["label"]).astype(np.int32)
    more = dr.blobs(s["depth"], s["mask"], as_member, s["grid_pose"], s["cam_pose"], s["c"], 1, 64)
    assert more["stats"]["points_in_band"] > want["stats"]["points_in_band"]


# ---- replay.py's options -------------------------------------------------------------------------------------------------------------------
def test_the_replay_options_parse():
    from supersurfel_fusion_amd import replay
    base = ["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-plan-goal", "1.0", "2.0"]
    a = replay.parse_args(base + ["--nav-steer", "--nav-live", "--nav-steer-movers"])
    assert replay.nav_steer_of(a) == dict(horizon=32, speed=0.5, movers=dict(inflate=0.3, gate=1.0)) and replay.library_of(a) == "load_dyn"
    a = replay.parse_args(base + ["--nav-steer", "--nav-live", "--nav-steer-movers", "--nav-steer-mover-inflate", "0.25", "--nav-steer-mover-gate", "0.5",
                                  "--nav-steer-footprint", "0.3", "0.3", "0.2", "0.2"])
    assert replay.nav_steer_of(a) == dict(horizon=32, speed=0.5, footprint=(0.3, 0.3, 0.2, 0.2), headings=16, movers=dict(inflate=0.25, gate=0.5))
    assert replay.library_of(a) == "load_dyn"
    t = replay.mover_tracker_of(dict(inflate=0.25, gate=0.5), 0.05)
    assert (t["tracker"].gate, t["tracker"].inflate, t["last"]) == (10240, 5120, None)
    assert replay.nav_steer_of(replay.parse_args(base + ["--nav-steer", "--nav-live"])) == dict(horizon=32, speed=0.5)        # without it: as before
    assert replay.library_of(replay.parse_args(base + ["--nav-steer", "--nav-live"])) == "load_steer"
    for bad in (["--nav-steer-movers"], ["--nav-steer", "--nav-steer-movers"], ["--nav-live", "--nav-steer-movers"],
                ["--nav-steer", "--nav-live", "--nav-steer-mover-inflate", "0.3"], ["--nav-steer", "--nav-live", "--nav-steer-mover-gate", "1"],
                ["--nav-steer", "--nav-live", "--nav-steer-movers", "--nav-steer-mover-inflate", "-0.1"],
                ["--nav-steer", "--nav-live", "--nav-steer-movers", "--nav-steer-mover-gate", "0"]):
        with pytest.raises(SystemExit):
            replay.parse_args(base + bad)
