"""Velocity commands on the navigation grid (include/ssf_navsteer.h) on the GPU: every array and every exact stat of
ssf_navsteer_rollouts equals the numpy restatement (tests/navsteer_ref.py) with ==, on the scenes that tests/test_navsteer.py guards
against being vacuous, at the smallest grids, lattices and horizons at which the kernels take another path, with the window staged on
chip and not and both in one launch, at the largest lattice, the widest scores and poses at the ends of int32, on grids of
states outside {0, -1, 100}, through device pointers fed by the overlay and the plan, through nav_live_steer, replay.py and the C++ wrapper."""
import os
import re
import subprocess

import numpy as np
import pytest

import navdyn_ref as dr
import navlive_ref as lr
import navplan_ref as pr
import navsteer_ref as sr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
W, H = 160, 128
CPP = os.path.join(ROOT, "tests", "cpp")


def handle(lib, **kw):
    """a handle of a test's own, which the test closes when it is done with it"""
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


@pytest.fixture(scope="module")
def steer_lib():
    """libssf_hip_steer.so: live's objects plus the rollouts' entry points (no fallback: a missing .so is an error)"""
    return binding.load_steer()


@pytest.fixture(scope="module")
def fusion(steer_lib):
    f = handle(steer_lib)
    yield f
    f.close()


def call_kw(c):
    """the keywords of Fusion.nav_steer from a restatement's: the grid's size comes from state, n_poses from poses"""
    return {k: v for k, v in c.items() if k not in ("width", "height", "n_poses")}


def same(got, want, what, outputs=sr.OUTPUTS):
    n = len(want["best"])
    for name in outputs:
        if name == "best_traj":                                          # a list, cut at best_len
            assert len(got[name]) == n, (what, name)
            for q in range(n):
                w = want[name][q, :want["best_len"][q]]
                assert got[name][q].shape == w.shape and got[name][q].dtype == w.dtype and (got[name][q] == w).all(), (what, name, q, got[name][q][:4].tolist(), w[:4].tolist())
            continue
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name, got[name].shape, got[name].dtype)
        diff = got[name] != want[name]
        assert not diff.any(), (what, name, int(diff.sum()), np.argwhere(diff)[:5].tolist(), got[name][diff][:5].tolist(), want[name][diff][:5].tolist())
    for k in sr.STATS:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"], want["stats"])


def check(f, what, i, want=None, **over):
    """the rollouts on the device (host arrays) and in the restatement; returns both"""
    c = dict(i["c"], **over)
    cost = i["cost"] if c["cost_weight"] else None
    targets = i["targets"] if c["target_weight"] else None
    if want is None:
        want = sr.rollouts(i["state"], i["dist2"], cost, i["poses"], targets, c)
    got = f.nav_steer(i["state"], i["dist2"], i["poses"], cost=cost, targets=targets, outputs=sr.OUTPUTS, **call_kw(c))
    same(got, want, what)
    return got, want


# ---- the scenes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", sr.GPU_CASES)
def test_the_scenes(scene, fusion):
    i = sr.scene(scene)
    got, want = check(fusion, scene, i, want=sr.case_reference(scene))
    s = got["stats"]
    assert s["candidates"] == len(i["poses"]) * i["c"]["n_v"] * i["c"]["n_w"]
    assert s["windows_staged"] == want["stats"]["windows_staged"] > 0 and s["windows_global"] == 0       # every window of these grids fits
    if scene in sr.GUARDED:
        assert s["collided"] > 0 and 0 < s["admissible"] < s["candidates"] and s["poses_stuck"] > 0 and s["poses_blocked"] > 0
        assert (got["best"] > 0).any() and sr.tied_poses(got)


def test_the_walk_through_the_grid_itself_gives_the_same_bytes(fusion):
    """walk = 1: no window is staged; every output and exact stat is what the staged walk gave"""
    for scene in ("room 65x64 reverse", "room K257 T256"):
        i = sr.scene(scene)
        got, _ = check(fusion, scene + " walk=1", i, want=sr.case_reference(scene), walk=1)
        assert got["stats"]["windows_staged"] == 0 and got["stats"]["windows_global"] == sr.case_reference(scene)["stats"]["windows_staged"]


def test_a_window_too_large_to_stage_is_walked_in_the_grid(fusion):
    """120 x 120 cells at T = 256 and |v| = 1024: the clipped window is the whole grid, 14400 cells > the 14336 the kernel stages"""
    i = sr.big_scene()
    assert i["c"]["width"] * i["c"]["height"] > sr.LDS_CELLS and sr.reach(i["c"]) > 120
    got, want = check(fusion, "big", i)
    s = got["stats"]
    assert s["windows_global"] == 3 and s["windows_staged"] == 0 and s["collided"] > 0 and s["admissible"] > 0
    assert int(got["cand_free"].max()) > 60                              # arcs that cross half the grid
    # one row fewer: 119 x 120 = 14280 cells fit, and the same poses are staged
    j = dict(i, state=i["state"][1:], dist2=sr.clearance(i["state"][1:]), c=dict(i["c"], height=119))
    got, _ = check(fusion, "just small enough", j)
    assert got["stats"]["windows_staged"] == 3 and got["stats"]["windows_global"] == 0


def same_bytes(a, b, what):
    for nm in sr.OUTPUTS:
        if nm == "best_traj":
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[nm], b[nm])), (what, nm)
        else:
            assert a[nm].tobytes() == b[nm].tobytes(), (what, nm)
    assert {k: a["stats"][k] for k in sr.STATS} == {k: b["stats"][k] for k in sr.STATS}, what


def test_a_launch_that_stages_some_windows_and_walks_the_others(fusion):
    """1281 workgroups whose largest window would take 28904 B of LDS: the launch stages the windows of up to 4056 cells and walks
    the others in the grid, in one launch with the dynamic LDS sized for the smaller bound; with 1280 it stages them all"""
    i, want = sr.scene_reference("mixed", sr.mixed_scene)
    assert sr.stage_cells(i["c"]) == 4056 and len(i["poses"]) == 1281
    got, _ = check(fusion, "mixed", i, want=want)
    s = got["stats"]
    print("mixed launch: windows_staged=%d windows_global=%d" % (s["windows_staged"], s["windows_global"]))
    assert s["windows_staged"] == want["stats"]["windows_staged"] > 0 and s["windows_global"] == want["stats"]["windows_global"] > 0
    walked, _ = check(fusion, "mixed walk=1", i, want=want, walk=1)
    assert walked["stats"]["windows_staged"] == 0 and walked["stats"]["windows_global"] == s["windows_staged"] + s["windows_global"]
    same_bytes(got, walked, "mixed against walk=1")
    for q in (sr.MIXED_EDGE_STAGED, sr.MIXED_EDGE_WALKED, sr.MIXED_CORNER, sr.MIXED_CENTRAL):       # the poses on either side of the rule
        assert got["pose_status"][q] == 0 and (got["cand_free"][q] == walked["cand_free"][q]).all() and (got["cand_free"][q] == want["cand_free"][q]).all(), q
    # one pose fewer: the launch is resident at once and every window is staged; the poses it shares give the same results
    j = sr.mixed_scene(1280)
    fewer = fusion.nav_steer(j["state"], j["dist2"], j["poses"], outputs=sr.OUTPUTS, **call_kw(j["c"]))
    assert fewer["stats"]["windows_global"] == 0 and fewer["stats"]["windows_staged"] == s["windows_staged"] + s["windows_global"]
    for nm in sr.OUTPUTS:
        if nm == "best_traj":
            assert all(x.tobytes() == y.tobytes() for x, y in zip(fewer[nm], got[nm][:1280])), nm
        else:
            assert (fewer[nm] == want[nm][:1280]).all(), nm


@pytest.mark.parametrize("tie", [False, True], ids=["last candidate alone", "ties with the last candidate"])
def test_the_largest_lattice(tie, fusion):
    """K = 65536: c = 65535 fills the low 16 bits of the key; it wins alone, or ties and loses to the smallest index"""
    i, want = sr.scene_reference(("lattice", tie), lambda: sr.lattice_scene(tie))
    got, _ = check(fusion, "K = 65536, tie %d" % tie, i, want=want)
    K = got["cand_score"].shape[1]
    print("largest lattice: K == %d best=%s" % (K, got["best"].tolist()))
    assert K == 65536 and got["stats"]["candidates"] == 2 * 65536
    if tie:
        assert got["best"].tolist() == [0, 65280] and (got["cand_score"][:, 65535] == got["best_score"]).all() and sr.tied_poses(got) == [0, 1]
    else:
        assert got["best"][0] == 65535 and got["best_score"][0] == 0 and 0 < got["n_admissible"][1] < 65536


def test_the_widest_scores_and_poses_at_the_ends_of_int32(fusion):
    """every weight 1000, costs up to 0xFFFFFFFE, targets at the corners of the int32 square: scores above 2^41; poses at INT32_MIN /
    INT32_MAX are outside the grid, read nothing and leave the live poses' results as they are without them"""
    i, want = sr.scene_reference("wide", sr.wide_scene)
    got, _ = check(fusion, "wide", i, want=want)
    assert 1 << 41 < int(got["cand_score"].max()) < 1 << 44 and int(got["best_score"].max()) > 1 << 41
    at = [q for q in range(len(i["poses"])) if tuple(i["poses"][q]) in sr.EXTREME_POSES]
    live = [q for q in range(len(i["poses"])) if q not in at]
    assert len(at) == 3 and (got["pose_status"][at] == 1).all() and (got["cand_score"][at] == -1).all() and (got["best"][at] == -1).all()
    assert got["cand_end"][at, 0].tolist() == [[sr.I32_MIN, 0, 0], [sr.I32_MAX, sr.I32_MAX, 65535], [0, sr.I32_MIN, 0]]
    alone = fusion.nav_steer(i["state"], i["dist2"], i["poses"][live], cost=i["cost"], targets=i["targets"][live], outputs=sr.OUTPUTS, **call_kw(i["c"]))
    for nm in sr.OUTPUTS:
        if nm == "best_traj":
            assert all(alone[nm][k].tobytes() == got[nm][q].tobytes() for k, q in enumerate(live)), nm
        else:
            assert alone[nm].tobytes() == np.ascontiguousarray(got[nm][live]).tobytes(), nm


@pytest.mark.parametrize("h,w", pr.FOREIGN_SIZES)
@pytest.mark.parametrize("allow", [0, 1])
def test_a_grid_with_states_outside_0_minus_1_100_and_dist2_outside_the_cap(h, w, allow, fusion):
    """tests/navplan_ref.py's foreign grid, steered down the field planned on it: only 0 (and -1 when allowed) is traversable, a negative
    dist2 is below min_dist2 = 0, dist2 above the cap counts as the cap"""
    i, want = sr.scene_reference(("foreign", h, w, allow), lambda: sr.foreign_scene(h, w, allow))
    got, _ = check(fusion, "foreign %d x %d unknown %d" % (h, w, allow), i, want=want)
    assert got["stats"]["windows_global"] == 0 and got["stats"]["collided"] > 0 and (got["cand_min_d"] == i["c"]["clearance_cap"]).any()
    check(fusion, "foreign, walk=1", i, want=want, walk=1)
    field = fusion.nav_plan(i["state"], i["dist2"], pr.foreign_case(h, w, allow)["goals"], outputs=("cost",), **pr.foreign_case(h, w, allow)["kw"])
    assert (field["cost"] == i["cost"]).all()                             # the field steered on is the one the device plans


def test_poses_on_cell_boundaries_in_corners_and_on_edges(fusion):
    """an open 33 x 31 floor without walls: arcs leave the grid on every side; x & 1023 and y & 1023 in {0, 1023}"""
    c = sr.params(width=33, height=31, n_v=5, n_w=13, v_min=-512, v_step=256, w_min=-1536, w_step=256, n_steps=40, cost_weight=0, turn_weight=1)
    state = np.zeros((31, 33), np.int8)
    S = sr.SUB
    poses = np.array([(0, 0, 0), (0, 0, 24576), (33 * S - 1, 31 * S - 1, 8192), (33 * S - 1, 0, 32768), (0, 31 * S - 1, 49152), (16 * S, 0, 49152),
                      (16 * S + 1023, 30 * S + 1023, 16384), (0, 15 * S, 32768), (33 * S - 1, 15 * S + 1023, 0), (5 * S, 5 * S, 65535), (5 * S + 1023, 5 * S + 1023, 1)],
                     np.int32)
    i = dict(state=state, dist2=sr.clearance(state), cost=None, poses=poses, targets=None, c=dict(c, n_poses=len(poses)))
    got, _ = check(fusion, "open floor", i)
    assert got["stats"]["collided"] > 0 and (got["pose_status"] == 0).all() and (got["cand_free"].min(axis=1) < 40).all()


def test_outputs_that_are_not_asked_for_and_two_calls_giving_the_same_bytes(fusion):
    i = sr.scene("room 65x64 reverse")
    want = sr.case_reference("room 65x64 reverse")
    c = i["c"]
    for asked in (("best_cmd",), ("cand_score", "best_traj"), ("pose_status", "cand_end"), ("cand_end_cost",), ("n_admissible", "best_len", "cand_free", "cand_min_d")):
        got = fusion.nav_steer(i["state"], i["dist2"], i["poses"], cost=i["cost"], outputs=asked, **call_kw(c))
        assert set(got) == set(asked) | {"stats"}
        same(got, want, asked, outputs=asked)
    a = fusion.nav_steer(i["state"], i["dist2"], i["poses"], cost=i["cost"], outputs=sr.OUTPUTS, **call_kw(c))
    b = fusion.nav_steer(i["state"], i["dist2"], i["poses"], cost=i["cost"], outputs=sr.OUTPUTS, **call_kw(c))
    for nm in sr.OUTPUTS:
        if nm == "best_traj":
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[nm], b[nm]))
        else:
            assert a[nm].tobytes() == b[nm].tobytes(), nm
    assert {k: a["stats"][k] for k in sr.STATS} == {k: b["stats"][k] for k in sr.STATS}


def test_entries_of_best_traj_past_best_len_are_not_written(steer_lib, fusion):
    """the C call with host arrays: a sentinel-filled best_traj keeps its sentinels past best_len"""
    i = sr.scene("room 9x33")
    want = sr.case_reference("room 9x33")
    c = i["c"]
    n, T = len(i["poses"]), c["n_steps"]
    p = fusion._navsteer_params(False, c["width"], c["height"], n, call_kw(c))
    SENT = -0x0A0B0C0D
    traj, blen = np.full((n, T + 1, 3), SENT, np.int32), np.zeros(n, np.int32)
    ptr = binding._ptr
    fusion._navsteer_rollouts(p, ptr(i["state"]), ptr(i["dist2"]), ptr(i["cost"]), ptr(i["poses"]), None, dict(best_traj=ptr(traj), best_len=ptr(blen)))
    assert (blen == want["best_len"]).all() and (blen < T + 1).any() and (blen == 0).any()
    for q in range(n):
        assert (traj[q, :blen[q]] == want["best_traj"][q, :blen[q]]).all() and (traj[q, blen[q]:] == SENT).all(), q


# ---- the staging of host arrays ----------------------------------------------------------------------------------------------------
same_arrays, FILL = util.rollouts_same, util.GUARD_WORD


@pytest.mark.parametrize("w,h", [(37, 19), (1, 1)])
def test_host_arrays_whose_items_all_start_at_rounded_offsets(w, h, fusion):
    """703 cells and one cell: neither P nor 4 P is a multiple of 256, so every array behind the first sits at a rounded offset of the
    staging buffer.  Host arrays, device pointers and the restatement agree on every output and exact stat"""
    s, want = dr.staging_scene(w, h, 5), dr.staging_reference(w, h, 5, "disc")
    host, hs = util.rollouts_host(fusion, "disc", s, sr.OUTPUTS)
    dev, ds = util.rollouts_device(fusion, "disc", s, sr.OUTPUTS)
    same_arrays(host, want, "host %d x %d" % (w, h), FILL)
    same_arrays(dev, want, "device %d x %d" % (w, h), FILL)
    assert all(host[nm].tobytes() == dev[nm].tobytes() for nm in sr.OUTPUTS)
    assert {k: hs[k] for k in sr.STATS} == {k: ds[k] for k in sr.STATS} == {k: want["stats"][k] for k in sr.STATS}
    assert w == 1 or ((want["pose_status"] == 0).sum() >= 3 and want["stats"]["collided"] > 0 and (want["pose_status"] == 1).any())


@pytest.mark.parametrize("name", sr.OUTPUTS)
def test_one_host_output_alone_between_guard_bytes(name, fusion):
    """37 x 19, host arrays: every output on its own, all others NULL, equals the same array of the call that asks for all twelve,
    and the 256 bytes on either side of the caller's array are untouched"""
    s = dr.staging_scene(37, 19, 5)
    every, stats = dr.cached(("staging host", "disc"), lambda: util.rollouts_host(fusion, "disc", s, sr.OUTPUTS))
    same_arrays(every, dr.staging_reference(37, 19, 5, "disc"), "every output", FILL)
    alone, st = util.rollouts_host(fusion, "disc", s, (name,))
    assert alone[name].tobytes() == every[name].tobytes() and {k: st[k] for k in sr.STATS} == {k: stats[k] for k in sr.STATS}, name


def test_best_traj_goes_in_as_well_as_out(fusion):
    """host arrays: best_traj is staged in both directions, so the entries past best_len, which the kernel does not write, come back
    as the caller's 0x5A5A5A5A and not as what the staging buffer held.  The first pose's winner stops at the wall after two steps"""
    s, want = dr.staging_scene(37, 19, 5), dr.staging_reference(37, 19, 5, "disc")
    T1 = s["c"]["n_steps"] + 1
    assert want["pose_status"][0] == 0 and 1 < want["best_len"][0] < T1 and (want["best_len"] == T1).any() and (want["best_len"] == 0).any()
    util.rollouts_host(fusion, "disc", s, ("cand_end",))                # (the place of best_len and best_traj then holds other bytes)
    got, _ = util.rollouts_host(fusion, "disc", s, ("best_traj", "best_len"))
    assert (got["best_len"] == want["best_len"]).all()
    same_arrays(got, want, "best_traj", FILL)
    assert sum(int((got["best_traj"][q, n:] == FILL).sum()) for q, n in enumerate(want["best_len"])) == 3 * int((T1 - want["best_len"]).sum()) > 0


def test_the_staging_buffer_grows_and_is_used_again(steer_lib):
    """one handle: 8 x 8 with one pose, 37 x 19 with five, 8 x 8 with one again.  Each call gives what a handle that has made no
    other call gives"""
    f = handle(steer_lib)
    for w, h, n in ((8, 8, 1), (37, 19, 5), (8, 8, 1)):
        s = dr.staging_scene(w, h, n)
        got, gs = util.rollouts_host(f, "disc", s, sr.OUTPUTS)
        fresh = handle(steer_lib)
        want, ws = util.rollouts_host(fresh, "disc", s, sr.OUTPUTS)
        fresh.close()
        assert all(got[nm].tobytes() == want[nm].tobytes() for nm in sr.OUTPUTS) and {k: gs[k] for k in sr.STATS} == {k: ws[k] for k in sr.STATS}, (w, h, n)
        same_arrays(got, dr.staging_reference(w, h, n, "disc"), (w, h, n), FILL)
    f.close()


# ---- through the binding ----------------------------------------------------------------------------------------------------------
def overlay_scene():
    """a depth frame over a free floor (tests/navlive_ref.py's room): what the overlay and the plan make of it is steered on"""
    kw = dict(lr.CAMERA, width=33, height=31, res=0.05, max_dist_cells=6, stride=4)
    cam_pose, grid_pose = lr.room_pose(at=(0.8, 0.0, 0.2)), lr.grid_pose_at()
    depth = lr.room_depth(cam_pose)
    state_in = np.zeros((31, 33), np.int8)
    state_in[:, :2] = -1
    S = sr.SUB
    poses = np.array([sr.centre(16, 4, 16384), sr.centre(2, 2, 0), (40 * S, S, 0), sr.centre(16, 4, 0), sr.centre(20, 8, 20000), sr.centre(10, 27, 50000)], np.int32)
    return dict(kw=kw, cam_pose=cam_pose, grid_pose=grid_pose, depth=depth, state_in=state_in, goals=[(16, 29)], plan=dict(min_dist2=1), poses=poses,
                steer=dict(n_steps=20, clearance_cap=36, brake_div=64))


def live_kw(o):
    return dict({k: v for k, v in o["kw"].items() if k not in ("width", "height")}, grid_pose=o["grid_pose"], cam_pose=o["cam_pose"])


def chained_restatements(o):
    lv = lr.overlay(o["depth"], None, o["state_in"], o["grid_pose"], o["cam_pose"], lr.params(**o["kw"]))
    pl = pr.plan(lv["state"], lv["dist2"], o["goals"], None, **o["plan"])
    c = sr.params(width=33, height=31, n_poses=len(o["poses"]), min_dist2=o["plan"]["min_dist2"], **o["steer"])
    return lv, pl, sr.rollouts(lv["state"], lv["dist2"], pl["cost"], o["poses"], None, c), c


def test_device_pointers_fed_from_the_overlay_and_the_plan(fusion):
    """nav_live_device -> nav_plan_device -> nav_steer_device: state, dist2 and cost are read where the calls before wrote them; the
    outputs land in one sentinel-filled buffer and no byte outside them changes"""
    import torch
    dev = torch.device("cuda")
    o = overlay_scene()
    lv, pl, want, c = chained_restatements(o)
    gw, gh, n, K, T = 33, 31, len(o["poses"]), c["n_v"] * c["n_w"], c["n_steps"]
    d_depth, d_state = torch.from_numpy(o["depth"]).to(dev), torch.from_numpy(o["state_in"]).to(dev)
    d_dist2, d_cost = torch.empty((gh, gw), dtype=torch.int32, device=dev), torch.empty((gh, gw), dtype=torch.int32, device=dev)
    fusion.nav_live_device(d_depth, d_state, gw, gh, state_out=d_state, dist2=d_dist2, **live_kw(o))
    fusion.nav_plan_device(d_state, d_dist2, gw, gh, o["goals"], None, cost=d_cost, **o["plan"])
    assert (d_cost.cpu().numpy().view(np.uint32) == pl["cost"]).all()
    d_poses = torch.from_numpy(o["poses"]).to(dev)
    G, SENT = 64, -0x0A0B0C0D
    shapes = {nm: binding.Fusion._navsteer_shape(kind, tail, n, K, T) for nm, _, kind, tail in binding.NAVSTEER_OUTPUTS}
    dtypes = {nm: dt for nm, dt, _, _ in binding.NAVSTEER_OUTPUTS}
    words = {nm: int(np.prod(shapes[nm])) * np.dtype(dtypes[nm]).itemsize // 4 for nm in shapes}

    def run(asked):
        off, at = {}, G + (G & 1)
        for nm in asked:
            off[nm] = at
            at += words[nm] + G + ((words[nm] + G) & 1)                   # (64-bit outputs stay 8-byte aligned)
        buf = torch.full((at,), SENT, dtype=torch.int32, device=dev)
        assert buf.data_ptr() % 8 == 0
        stats = fusion.nav_steer_device(d_state, d_dist2, gw, gh, d_poses, n, cost=d_cost, min_dist2=o["plan"]["min_dist2"],
                                        **dict({nm: buf.data_ptr() + 4 * off[nm] for nm in asked}, **o["steer"]))
        raw = buf.cpu().numpy()
        got, untouched = dict(stats=stats), np.ones(at, bool)
        for nm in asked:
            got[nm] = raw[off[nm]:off[nm] + words[nm]].view(dtypes[nm]).reshape(shapes[nm]).copy()
            untouched[off[nm]:off[nm] + words[nm]] = False
        assert (raw[untouched] == SENT).all(), (asked, "words outside the asked outputs were written")
        if "best_traj" in got:
            full = got["best_traj"]
            for q in range(n):
                assert (full[q, want["best_len"][q]:] == SENT).all(), q
            got["best_traj"] = [full[q, :want["best_len"][q]] for q in range(n)]
        return got
    same(run(sr.OUTPUTS), want, "device pointers")
    same(run(("best_cmd",)), want, "the command alone", outputs=("best_cmd",))
    same(run(("cand_score", "best_score")), want, "the scores", outputs=("cand_score", "best_score"))
    assert want["stats"]["poses_ok"] >= 3 and want["stats"]["poses_blocked"] >= 1 and want["stats"]["collided"] > 0


def test_overlay_plan_and_steer_with_only_the_command_leaving_the_device(fusion):
    """nav_live_steer against the three restatements chained on the host"""
    o = overlay_scene()
    lv, pl, want, c = chained_restatements(o)
    got = fusion.nav_live_steer(o["depth"], o["state_in"], o["goals"], o["poses"], live=live_kw(o), plan=o["plan"], steer=o["steer"])
    assert {k: got["live"]["stats"][k] for k in lr.STATS} == lv["stats"] and lv["stats"]["cells_stamped"] > 10
    assert {k: got["plan"]["stats"][k] for k in pr.STATS} == {k: pl["stats"][k] for k in pr.STATS}
    same(got["steer"], want, "nav_live_steer", outputs=binding.NAVSTEER_POSE_OUTPUTS)
    assert want["stats"]["poses_ok"] >= 3 and want["stats"]["collided"] > 0 and (want["best"] > 0).any()


def test_a_call_between_two_frames_changes_no_later_result(steer_lib):
    A, B = handle(steer_lib), handle(steer_lib)
    i = sr.scene("K64")
    for k in (0, 3, 6):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        check(A, "between frames", i, want=sr.case_reference("K64"))
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)
    B.close()
    A.close()


def test_the_refusals(steer_lib):
    f = handle(steer_lib)
    i = sr.scene("K64")
    c = i["c"]
    base = call_kw(c)
    refused = pytest.raises(binding.SsfError, match=r"ssf_navsteer_rollouts failed \(-1\)")
    run = lambda **kw: f.nav_steer(i["state"], i["dist2"], i["poses"], cost=i["cost"], targets=i["targets"], **dict(base, **kw))
    for kw in (dict(min_dist2=-1), dict(allow_unknown=2), dict(clearance_cap=-1), dict(clearance_cap=1024 * 1024 + 1), dict(n_v=0), dict(n_v=257),
               dict(n_w=0), dict(n_w=1025), dict(n_v=256, n_w=257, v_step=0), dict(v_min=1025, n_v=1), dict(v_min=-1025, n_v=1), dict(v_min=0, v_step=400, n_v=4),
               dict(v_min=0, v_step=-400, n_v=4), dict(w_min=16385, n_w=1), dict(w_min=-16385, n_w=1), dict(w_min=0, w_step=2000, n_w=10), dict(n_steps=0),
               dict(n_steps=257), dict(min_free_steps=-1), dict(min_free_steps=257), dict(brake_div=-1), dict(brake_div=1025), dict(cost_weight=-1),
               dict(cost_weight=1001), dict(target_weight=1001), dict(clear_weight=-1), dict(speed_weight=1001), dict(turn_weight=-1),
               dict(cost_weight=0, target_weight=0, clear_weight=0, speed_weight=0, turn_weight=0), dict(walk=2), dict(walk=-1)):
        with refused:
            run(**kw)
    with refused:                                                        # cost NULL with cost_weight > 0
        f.nav_steer(i["state"], i["dist2"], i["poses"], **base)
    with refused:                                                        # targets NULL with target_weight > 0
        f.nav_steer(i["state"], i["dist2"], i["poses"], cost=i["cost"], **dict(base, target_weight=1))
    with refused:
        f.nav_steer(i["state"], i["dist2"], i["poses"], cost=i["cost"], outputs=(), **base)         # every output NULL
    with refused:
        f.nav_steer(i["state"], i["dist2"], np.zeros((0, 3), np.int32), cost=i["cost"], **base)      # n_poses 0
    with refused:
        f.nav_steer(i["state"], i["dist2"], np.zeros((4097, 3), np.int32), cost=i["cost"], **base)
    with refused:                                                        # n_poses * K > 1 << 24
        f.nav_steer(i["state"], i["dist2"], np.zeros((4096, 3), np.int32), cost=i["cost"], **dict(base, n_v=8, n_w=513, v_step=0, w_step=0))
    with refused:
        f.nav_steer(np.zeros((1, 4097), np.int8), np.zeros((1, 4097), np.int32), i["poses"], **dict(base, cost_weight=0))
    # the limits themselves are accepted
    run(v_min=-1024, v_step=2048, n_v=2, w_min=-16384, w_step=32768, n_w=2, n_steps=256, min_free_steps=256, brake_div=1024, clearance_cap=1024 * 1024)
    # the C entry points themselves
    L, byref, vp = steer_lib.lib, binding.C.byref, binding.C.c_void_p
    p, st = binding.SsfNavSteerParams(), binding.SsfNavSteerStats()
    assert L.ssf_navsteer_default_params(f.h, byref(p)) == 0
    assert L.ssf_navsteer_default_params(None, byref(p)) == -1 and L.ssf_navsteer_default_params(f.h, None) == -1
    assert f.nav_steer_default_params() == dict(sr.DEFAULTS, on_device=0)
    p.width, p.height, p.n_poses, p.cost_weight = 8, 4, 1, 0
    s8, d8, ps, best = np.zeros((4, 8), np.int8), np.full((4, 8), 9, np.int32), np.array([sr.centre(1, 1)], np.int32), np.zeros(1, np.int32)
    out = binding.SsfNavSteerOut()
    out.best = best.ctypes.data
    s, d, q = s8.ctypes.data_as(vp), d8.ctypes.data_as(vp), ps.ctypes.data_as(vp)
    assert L.ssf_navsteer_rollouts(f.h, byref(p), s, d, None, q, None, byref(out), None) == 0 and best[0] > 0          # stats are optional
    assert L.ssf_navsteer_rollouts(None, byref(p), s, d, None, q, None, byref(out), byref(st)) == -1
    assert L.ssf_navsteer_rollouts(f.h, None, s, d, None, q, None, byref(out), byref(st)) == -1
    assert L.ssf_navsteer_rollouts(f.h, byref(p), None, d, None, q, None, byref(out), byref(st)) == -1
    assert L.ssf_navsteer_rollouts(f.h, byref(p), s, None, None, q, None, byref(out), byref(st)) == -1
    assert L.ssf_navsteer_rollouts(f.h, byref(p), s, d, None, None, None, byref(out), byref(st)) == -1
    assert L.ssf_navsteer_rollouts(f.h, byref(p), s, d, None, q, None, None, byref(st)) == -1
    assert L.ssf_navsteer_rollouts(f.h, byref(p), s, d, None, q, None, byref(binding.SsfNavSteerOut()), byref(st)) == -1
    for field, bad in (("width", 0), ("width", 4097), ("height", -3), ("height", 4097)):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert L.ssf_navsteer_rollouts(f.h, byref(p), s, d, None, q, None, byref(out), byref(st)) == -1, (field, bad)
        setattr(p, field, keep)
    # the handle keeps working: a call and a frame after the refusals
    check(f, "after the refusals", i, want=sr.case_reference("K64"))
    f.process_frame(*util.frame(0, W, H))
    check(f, "after a frame", i, want=sr.case_reference("K64"))
    g = handle(steer_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_steer(i["state"], i["dist2"], i["poses"], cost=i["cost"], **base)
    q2 = handle(steer_lib, pipeline_depth=2, extract_batch=2)
    q2.submit_frame(*util.frame(0, W, H))
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q2.nav_steer(i["state"], i["dist2"], i["poses"], cost=i["cost"], **base)
    q2.process_submitted()
    check(q2, "pipelined, at rest", i, want=sr.case_reference("K64"))
    q2.close()
    g.close()
    f.close()


def test_the_kernels_are_timed_under_profile(steer_lib):
    f = handle(steer_lib, profile=1)
    f.reset_kernel_times()
    check(f, "profiled", sr.scene("K64"), want=sr.case_reference("K64"))
    names = f.kernel_times()
    for k in ("navsteer_pack", "navsteer_roll", "navsteer_pick"):
        assert k in names and names[k][1] > 0, (k, names)
    f.close()


# ---- replay.py's files -----------------------------------------------------------------------------------------------------
def test_replay_logs_the_command_and_writes_its_arc_next_to_the_plan(steer_lib, tmp_path, capsys):
    from supersurfel_fusion_amd import replay
    f = handle(steer_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    plan = dict(goals=[(12.0, 12.5)], frontier=True, radius=0.12)
    replay.replay(f, frames, nav_grid_dir=str(tmp_path), nav_grid_every=2, nav_grid_res=0.1, nav_grid_carve=True, nav_grid_carve_stride=4, nav_plan=plan,
                  nav_live=dict(min_hits=2, stride=8), nav_steer=dict(horizon=16, speed=0.4))
    per_grid = [".pgm", ".yaml", "_cost.npy", "_dist2.npy", "_live_dist2.npy", "_live_state.npy", "_path.npy", "_plan.json", "_seen.npy", "_steer_traj.npy"]
    assert sorted(os.listdir(str(tmp_path))) == sorted("%06d%s" % (k, s) for k in (0, 2) for s in per_grid)
    # the same call again on the files of the last grid: the live layer, the plan's field, the camera's pose in the grid
    pose = np.array([float(v) for v in re.search(r"grid_to_map: \[(.*)\]", open(str(tmp_path / "000002.yaml")).read()).group(1).split(",")], np.float32)
    state, dist2 = np.load(str(tmp_path / "000002_live_state.npy")), np.load(str(tmp_path / "000002_live_dist2.npy"))
    cost = np.load(str(tmp_path / "000002_cost.npy"))
    start = replay.steer_pose(pose, 0.1, f.get_pose())
    c = sr.params(width=state.shape[1], height=state.shape[0], n_poses=1, min_dist2=4, n_steps=16, **replay.steer_lattice(0.4, 0.1))
    assert (c["n_v"], c["v_step"]) == (9, 51)
    want = sr.rollouts(state, dist2, cost, start, None, c)
    traj = np.load(str(tmp_path / "000002_steer_traj.npy"))
    assert traj.dtype == np.int32 and traj.shape == (want["best_len"][0], 3) and (traj == want["best_traj"][0, :want["best_len"][0]]).all()
    logged = [l for l in capsys.readouterr().out.splitlines() if l.startswith("nav-steer ")]
    assert len(logged) == 2 and logged[1].startswith("nav-steer 000002: status=%d best=%d v=%d w=%d " % (
        want["pose_status"][0], want["best"][0], want["best_cmd"][0, 0], want["best_cmd"][0, 1])), logged
    assert "score=%d n_admissible=%d best_len=%d " % (want["best_score"][0], want["n_admissible"][0], want["best_len"][0]) in logged[1]
    assert all("%s=%d" % (k, want["stats"][k]) in logged[1] for k in sr.STATS)
    with pytest.raises(ValueError, match="nav_steer needs nav_plan"):
        replay.replay(f, [], nav_grid_dir=str(tmp_path), nav_steer=dict())
    f.close()


# ---- the C++ surface -----------------------------------------------------------------------------------------------------
def test_steering_in_cpp(steer_lib, fusion, tmp_path):
    """tests/cpp/navsteer_smoke.cpp on the GPU: its counts and FNV-1a checksums equal those of the Python calls on the same arrays"""
    libdir = os.path.dirname(steer_lib.path)
    exe = str(tmp_path / "navsteer_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "navsteer_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip_steer", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "messages ok=1" in r.stdout, r.stdout
    counts = ("ok", "blocked", "stuck", "admissible", "collided", "steps")
    sums = ("best", "v", "w", "score", "traj", "cand_score", "cand_end")
    told = re.search("navsteer " + " ".join(nm + r"=(\d+)" for nm in counts) + " " + " ".join(nm + "=([0-9a-f]{16})" for nm in sums), r.stdout)
    assert told, r.stdout
    p = np.arange(70 * 45, dtype=np.uint64)
    h = ((p * 2654435761) & 0xFFFFFFFF) >> 16
    state = np.where(h % 100 < 6, 100, np.where(h % 100 < 10, -1, 0)).astype(np.int8).reshape(45, 70)
    dist2 = np.where(state.ravel() == 0, 1 + (h >> 7) % 40, 0).astype(np.int32).reshape(45, 70)
    cost = fusion.nav_plan(state, dist2, goals=[(60, 30)], outputs=("cost",))["cost"]
    poses = np.array([((5 + 11 * k) * 1024 + 300, (4 + 7 * k) * 1024 + 700, 9000 * k) for k in range(6)], np.int32)
    got = fusion.nav_steer(state, dist2, poses, cost=cost, outputs=sr.OUTPUTS, n_steps=24)
    same(got, sr.rollouts(state, dist2, cost, poses, None, sr.params(width=70, height=45, n_poses=6, n_steps=24)), "the smoke program's arrays")
    s = got["stats"]
    py_counts = (s["poses_ok"], s["poses_blocked"], s["poses_stuck"], s["admissible"], s["collided"], s["steps_taken"])
    assert tuple(int(v) for v in told.groups()[:6]) == py_counts, (told.groups(), py_counts)
    flat = np.concatenate(got["best_traj"]) if len(got["best_traj"]) else np.zeros((0, 3), np.int32)
    py_sums = tuple(pr.fnv1a(a.tobytes()) for a in (got["best"], np.ascontiguousarray(got["best_cmd"][:, 0]), np.ascontiguousarray(got["best_cmd"][:, 1]),
                                                      got["best_score"], flat, got["cand_score"], got["cand_end"]))
    assert tuple(int(v, 16) for v in told.groups()[6:]) == py_sums, (told.groups()[6:], py_sums)
    assert s["poses_ok"] >= 2 and s["collided"] > 0
    twist = re.search(r"twist pose=(\d+) v=(-?\d+) w=(-?\d+) linear.x=(\S+) angular.z=(\S+) poses=(\d+)", r.stdout)
    q = int(twist.group(1))
    assert q == int(np.flatnonzero(got["best"] >= 0)[0]) and (int(twist.group(2)), int(twist.group(3))) == tuple(got["best_cmd"][q]) and int(twist.group(6)) == got["best_len"][q]
    assert abs(float(twist.group(4)) - got["best_cmd"][q, 0] * float(np.float32(0.05)) / (1024.0 * float(np.float32(0.1)))) < 1e-8
