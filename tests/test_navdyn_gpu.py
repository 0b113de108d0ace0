"""Steering among movers (include/ssf_navdyn.h) on the GPU: every array and every exact stat of ssf_navdyn_rollouts,
ssf_navdyn_foot_rollouts and ssf_navdyn_blobs equals the restatement (tests/navdyn_ref.py) with ==, at the smallest shapes at which
the kernels can go wrong (one cell, one row, grids that are no multiple of anything, K = 297 and 512, 1 and 256 steps, 1 and 70
poses, 0 / 1 / 64 movers, the largest operands; cameras of 1 x 1, 17 x 13 and 160 x 128), through device pointers from the motion
detector and the overlay to the command, and with the older calls beside them through the same handle.
The edges: the footprint at B = 1, 4 and 32, at 256 steps, with 64 movers, on one cell and through device pointers; 300 poses (two
pick workgroups) for the disc and the footprint; one launch that stages some windows and walks the others; discs that touch
(D2 == R_s^2: free, gap 0), a wall inside a disc (the static test answers), a refused step's gaps; blocks of labels that share tiles
(cameras of 40 x 24 and 35 x 19), a large frame after a small one on one handle; a device mover list outside the header's bounds."""
import os
import re
import subprocess

import numpy as np
import pytest

import navdyn_ref as dr
import navfoot_ref as fr
import navlive_ref as lr
import navplan_ref as pr
import navsteer_ref as sr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
W, H = 160, 128


def handle(lib, **kw):
    """a handle of a test's own, which the test closes when it is done with it"""
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


@pytest.fixture(scope="module")
def dyn_lib():
    """libssf_hip_dyn.so: pose's objects plus the movers' entry points (no fallback: a missing .so is an error)"""
    return binding.load_dyn()


@pytest.fixture(scope="module")
def fusion(dyn_lib):
    f = handle(dyn_lib)
    yield f
    f.close()


def call_kw(c):
    return {k: v for k, v in c.items() if k not in ("width", "height", "n_poses")}


def same(got, want, what, outputs=dr.OUTPUTS, stats=dr.STATS + sr.INFORMATIVE):
    n = len(want["best"])
    for name in outputs:
        if name == "best_traj":                                          # a list, cut at best_len
            assert len(got[name]) == n, (what, name)
            for q in range(n):
                w = want[name][q, :want["best_len"][q]]
                assert got[name][q].shape == w.shape and got[name][q].dtype == w.dtype and (got[name][q] == w).all(), (what, name, q)
            continue
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name, got[name].shape, got[name].dtype)
        diff = got[name] != want[name]
        assert not diff.any(), (what, name, int(diff.sum()), np.argwhere(diff)[:5].tolist(), got[name][diff][:5].tolist(), want[name][diff][:5].tolist())
    for k in stats:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"], want["stats"])


def steer(f, name, **more):
    s = dr.scene_inputs(name)
    c = s["c"]
    cost, targets = (s["cost"] if c["cost_weight"] else None), (s["targets"] if c["target_weight"] else None)
    if name in dr.FOOT_CASES:
        return f.nav_dyn_foot_steer(s["free_mask"], s["dist2"], s["poses"], s["B"], movers=s["movers"], cost=cost, targets=targets, outputs=dr.OUTPUTS,
                                    **dict(call_kw(c), **more))
    return f.nav_dyn_steer(s["state"], s["dist2"], s["poses"], movers=s["movers"], cost=cost, targets=targets, outputs=dr.OUTPUTS, **dict(call_kw(c), **more))


# ---- the rollouts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dr.DISC_CASES + dr.FOOT_CASES + dr.HAND_CASES)
def test_the_rollouts_with_movers(name, fusion):
    want, c = dr.scene_reference(name), dr.scene_inputs(name)["c"]
    if name in dr.GUARDED:                                               # (on the restatement alone: the case is not vacuous)
        assert dr.not_vacuous(want, c) == (True, True, True), name
    if c["n_poses"] > 256:                                               # winners on both sides of the first pick workgroup, of several gaps
        ok = np.flatnonzero(want["pose_status"] == 0)
        assert (ok < 256).any() and (ok >= 256).any() and len(np.unique(want["best_min_gap"][ok[ok >= 256]])) > 2, name
    same(steer(fusion, name), want, name)
    if name in ("37x53 K512 64 movers 70 poses", "64x65 K297 T256", "300 poses K64", "touch static"):     # the grid walked in place of the staged window: the same outputs
        same(steer(fusion, name, walk=1), want, name + " walk", stats=dr.STATS)


def test_without_movers_the_older_calls_give_the_same_bytes(fusion):
    """n_movers == 0 and mover_weight == 0: every output and stat that nav_steer / nav_foot_steer also produce equals theirs, through the
    same handle"""
    for scene in ("room 65x64 reverse", "room K257 T256"):
        i = sr.scene(scene)
        c = i["c"]
        cost, targets = (i["cost"] if c["cost_weight"] else None), (i["targets"] if c["target_weight"] else None)
        a = fusion.nav_steer(i["state"], i["dist2"], i["poses"], cost=cost, targets=targets, outputs=sr.OUTPUTS, **call_kw(c))
        b = fusion.nav_dyn_steer(i["state"], i["dist2"], i["poses"], cost=cost, targets=targets, outputs=dr.OUTPUTS, mover_weight=0, **call_kw(c))
        for nm in sr.OUTPUTS:
            if nm == "best_traj":
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a[nm], b[nm])), nm
            else:
                assert a[nm].tobytes() == b[nm].tobytes(), (scene, nm)
        assert a["stats"] == {k: b["stats"][k] for k in a["stats"]} and b["stats"]["hit_movers"] == 0          # the informative ones as well
        assert (b["cand_hit"] == -1).all() and (a["stats"]["collided"] > 0)
        same(a, sr.case_reference(scene), scene, outputs=sr.OUTPUTS, stats=sr.STATS)
    i = fr.corridor_scene()
    c, B = i["c"], i["B"]
    lay = fusion.nav_foot(i["state"], n_headings=B, **dict(zip(("front", "back", "left", "right", "pad"), i["foot"])))
    a = fusion.nav_foot_steer(lay["free_mask"], i["dist2"], i["poses"], B, cost=i["cost"], outputs=sr.OUTPUTS, **call_kw(c))
    b = fusion.nav_dyn_foot_steer(lay["free_mask"], i["dist2"], i["poses"], B, cost=i["cost"], outputs=dr.OUTPUTS, mover_weight=0, mover_cap=0, **call_kw(c))
    for nm in sr.OUTPUTS:
        if nm == "best_traj":
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[nm], b[nm])), nm
        else:
            assert a[nm].tobytes() == b[nm].tobytes(), nm
    assert a["stats"] == {k: b["stats"][k] for k in a["stats"]} and (a["best"] >= 0).all()


def test_one_output_alone_guard_bytes_and_two_calls_giving_the_same_bytes(fusion):
    """device buffers inside sentinels: an output that is not asked for is not written, nothing lands outside the one that is, and a
    second call writes the same bytes"""
    import torch
    dev = torch.device("cuda")
    name = "37x53 K512 64 movers 70 poses"
    s, want = dr.scene_inputs(name), dr.scene_reference(name)
    c = s["c"]
    gw, gh, n, K = c["width"], c["height"], c["n_poses"], c["n_v"] * c["n_w"]
    d = {k: torch.from_numpy(s[k].view(np.int32) if s[k].dtype == np.uint32 else s[k]).to(dev) for k in ("state", "dist2", "cost", "poses", "targets", "movers")}
    G, SENT = 256, 0x5A
    for nm, words in (("cand_hit", n * K), ("cand_min_gap", n * K), ("best_min_gap", n), ("cand_free", n * K)):
        raws = []
        for _ in range(2):
            buf = torch.full((2 * G + 4 * words + 3,), SENT, dtype=torch.uint8, device=dev)
            st = fusion.nav_dyn_steer_device(d["state"], d["dist2"], gw, gh, d["poses"], n, movers=d["movers"], n_movers=len(s["movers"]), cost=d["cost"],
                                             targets=d["targets"], **dict(call_kw(c), **{nm: buf.data_ptr() + G}))
            raws.append(buf.cpu().numpy())
            assert {k: st[k] for k in dr.STATS} == {k: want["stats"][k] for k in dr.STATS}
        raw = raws[0]
        assert (raw[G:G + 4 * words].view(np.int32).reshape(want[nm].shape) == want[nm]).all(), nm
        assert (raw[:G] == SENT).all() and (raw[G + 4 * words:] == SENT).all(), nm
        assert raws[0].tobytes() == raws[1].tobytes(), nm


def on_device(s, keys, dev):
    import torch
    return {k: torch.from_numpy(s[k].view(np.int32) if s[k].dtype == np.uint32 else s[k]).to(dev) for k in keys}


def test_one_footprint_output_alone_guard_bytes_and_two_calls_giving_the_same_bytes(fusion):
    """the footprint's rollouts through device pointers (nav_dyn_steer_device with n_headings), B = 32, 64 movers: the twin of the
    test above"""
    import torch
    dev = torch.device("cuda")
    name = "foot B32 K512 64 movers"
    s, want = dr.scene_inputs(name), dr.scene_reference(name)
    c = s["c"]
    gw, gh, n, K = c["width"], c["height"], c["n_poses"], c["n_v"] * c["n_w"]
    assert s["B"] == 32 and c["cost_weight"] > 0 and c["target_weight"] > 0
    d = on_device(s, ("free_mask", "dist2", "cost", "poses", "targets", "movers"), dev)
    G, SENT = 256, 0x5A
    for nm, words in (("cand_hit", n * K), ("cand_min_gap", n * K), ("best_min_gap", n)):
        raws = []
        for _ in range(2):
            buf = torch.full((2 * G + 4 * words + 3,), SENT, dtype=torch.uint8, device=dev)
            st = fusion.nav_dyn_steer_device(d["free_mask"], d["dist2"], gw, gh, d["poses"], n, movers=d["movers"], n_movers=len(s["movers"]),
                                             n_headings=s["B"], cost=d["cost"], targets=d["targets"], **dict(call_kw(c), **{nm: buf.data_ptr() + G}))
            raws.append(buf.cpu().numpy())
            assert {k: st[k] for k in dr.STATS + sr.INFORMATIVE} == {k: want["stats"][k] for k in dr.STATS + sr.INFORMATIVE}
        raw = raws[0]
        assert (raw[G:G + 4 * words].view(np.int32).reshape(want[nm].shape) == want[nm]).all(), nm
        assert (raw[:G] == SENT).all() and (raw[G + 4 * words:] == SENT).all(), nm
        assert raws[0].tobytes() == raws[1].tobytes(), nm


# ---- the staging of host arrays: the 21 arrays of a call with movers ----------------------------------------------------------------
FILL = util.GUARD_WORD
KINDS = ("dyn", "dyn foot")


@pytest.mark.parametrize("w,h", [(37, 19), (1, 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_host_arrays_whose_items_all_start_at_rounded_offsets(kind, w, h, fusion):
    """703 cells and one cell: neither P nor 4 P is a multiple of 256, so every array behind the first sits at a rounded offset of the
    staging buffer.  Host arrays, device pointers and the restatement agree on every output and exact stat"""
    s, want = dr.staging_scene(w, h, 5), dr.staging_reference(w, h, 5, kind)
    host, hs = util.rollouts_host(fusion, kind, s, dr.OUTPUTS)
    dev, ds = util.rollouts_device(fusion, kind, s, dr.OUTPUTS)
    util.rollouts_same(host, want, "host %d x %d" % (w, h), FILL)
    util.rollouts_same(dev, want, "device %d x %d" % (w, h), FILL)
    assert all(host[nm].tobytes() == dev[nm].tobytes() for nm in dr.OUTPUTS)
    assert {k: hs[k] for k in dr.STATS} == {k: ds[k] for k in dr.STATS} == {k: want["stats"][k] for k in dr.STATS}
    assert want["stats"]["hit_movers"] > 0 and (w == 1 or ((want["pose_status"] == 0).sum() >= 3 and want["stats"]["collided"] > 0))


@pytest.mark.parametrize("name", dr.OUTPUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_one_host_output_alone_between_guard_bytes(kind, name, fusion):
    """37 x 19, host arrays: each of the 15 outputs on its own, all others NULL, equals the same array of the call that asks for all
    of them, and the 256 bytes on either side of the caller's array are untouched"""
    s = dr.staging_scene(37, 19, 5)
    every, stats = dr.cached(("staging host", kind), lambda: util.rollouts_host(fusion, kind, s, dr.OUTPUTS))
    util.rollouts_same(every, dr.staging_reference(37, 19, 5, kind), "every output", FILL)
    alone, st = util.rollouts_host(fusion, kind, s, (name,))
    assert alone[name].tobytes() == every[name].tobytes() and {k: st[k] for k in dr.STATS} == {k: stats[k] for k in dr.STATS}, name


def test_best_traj_goes_in_as_well_as_out(fusion):
    """host arrays: best_traj is staged in both directions, so the entries past best_len, which the kernel does not write, come back
    as the caller's 0x5A5A5A5A and not as what the staging buffer held.  The first pose's winner stops at the wall after two steps"""
    s, want = dr.staging_scene(37, 19, 5), dr.staging_reference(37, 19, 5, "dyn")
    T1 = s["c"]["n_steps"] + 1
    assert want["pose_status"][0] == 0 and 1 < want["best_len"][0] < T1 and (want["best_len"] == T1).any() and (want["best_len"] == 0).any()
    util.rollouts_host(fusion, "dyn", s, ("cand_end",))                 # (the place of best_len and best_traj then holds other bytes)
    got, _ = util.rollouts_host(fusion, "dyn", s, ("best_traj", "best_len"))
    assert (got["best_len"] == want["best_len"]).all()
    util.rollouts_same(got, want, "best_traj", FILL)
    assert sum(int((got["best_traj"][q, n:] == FILL).sum()) for q, n in enumerate(want["best_len"])) == 3 * int((T1 - want["best_len"]).sum()) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_the_staging_buffer_grows_and_is_used_again(kind, dyn_lib):
    """one handle: 8 x 8 with one pose, 37 x 19 with five, 8 x 8 with one again.  Each call gives what a handle that has made no
    other call gives"""
    f = handle(dyn_lib)
    for w, h, n in ((8, 8, 1), (37, 19, 5), (8, 8, 1)):
        s = dr.staging_scene(w, h, n)
        got, gs = util.rollouts_host(f, kind, s, dr.OUTPUTS)
        fresh = handle(dyn_lib)
        want, ws = util.rollouts_host(fresh, kind, s, dr.OUTPUTS)
        fresh.close()
        assert all(got[nm].tobytes() == want[nm].tobytes() for nm in dr.OUTPUTS) and {k: gs[k] for k in dr.STATS} == {k: ws[k] for k in dr.STATS}, (w, h, n)
        util.rollouts_same(got, dr.staging_reference(w, h, n, kind), (w, h, n), FILL)
    f.close()


def test_a_launch_with_movers_that_stages_some_windows_and_walks_the_others(fusion):
    """navsteer_ref.mixed_scene among ten movers: 1281 workgroups, of which one launch stages the windows of up to 4056 cells in LDS and
    walks the others in the grid; both kinds test their steps against the list in LDS"""
    name = "mixed walks"
    s, want = dr.scene_inputs(name), dr.scene_reference(name)
    assert want["stats"]["windows_staged"] > 0 and want["stats"]["windows_global"] > 0 and len(s["movers"]) >= 8     # (on the restatement alone)
    assert want["stats"]["hit_movers"] > 0
    got = steer(fusion, name)
    same(got, want, name)
    assert got["stats"]["windows_staged"] == want["stats"]["windows_staged"] and got["stats"]["windows_global"] == want["stats"]["windows_global"]
    walked = steer(fusion, name, walk=1)
    same(walked, want, name + " walk", stats=dr.STATS)
    assert walked["stats"]["windows_staged"] == 0
    assert walked["stats"]["windows_global"] == want["stats"]["windows_staged"] + want["stats"]["windows_global"]


def test_a_device_mover_list_outside_the_bounds_touches_nothing_else(dyn_lib):
    """a device list is not read by the host (ssf_navdyn.h: "change what is computed, never what is touched"): entries at INT32_MIN,
    INT32_MAX and 1 << 30 in every field, every output inside sentinels.  Only what the header promises is asserted: no gap, no score"""
    import torch
    dev = torch.device("cuda")
    f = handle(dyn_lib)
    name = "37x53 K512 64 movers 70 poses"
    s = dr.scene_inputs(name)
    c = s["c"]
    gw, gh, n, K, T = c["width"], c["height"], c["n_poses"], c["n_v"] * c["n_w"], c["n_steps"]
    bad = s["movers"].copy()
    odd = (sr.I32_MIN, sr.I32_MAX, 1 << 30)
    for k, val in enumerate(odd):
        for field in range(6):
            bad[6 * k + field, field] = val                               # one field out of range, the others as they were
        bad[18 + k] = val                                                 # all six
    bad[21] = (sr.I32_MIN, sr.I32_MAX, sr.I32_MAX, sr.I32_MIN, 1 << 30, sr.I32_MAX)
    assert len(bad) == dr.MAX_MOVERS and not dr.movers_ok(bad) and dr.movers_ok(bad[22:])
    d = on_device(dict(s, movers=bad), ("state", "dist2", "cost", "poses", "targets", "movers"), dev)
    known = binding.NAVSTEER_OUTPUTS + binding.NAVDYN_OUTPUTS
    G, SENT = 256, 0x5A
    bufs, ptrs = {}, {}
    for nm, dt, kind, tail in known:
        nbytes = int(np.prod(binding.Fusion._navsteer_shape(kind, tail, n, K, T))) * np.dtype(dt).itemsize
        bufs[nm] = (torch.full((2 * G + nbytes,), SENT, dtype=torch.uint8, device=dev), nbytes)
        ptrs[nm] = bufs[nm][0].data_ptr() + G
    st = f.nav_dyn_steer_device(d["state"], d["dist2"], gw, gh, d["poses"], n, movers=d["movers"], n_movers=len(bad), cost=d["cost"], targets=d["targets"],
                                **dict(call_kw(c), **ptrs))              # the call returns
    got = {}
    for nm, dt, kind, tail in known:
        raw, nbytes = bufs[nm][0].cpu().numpy(), bufs[nm][1]
        assert (raw[:G] == SENT).all() and (raw[G + nbytes:] == SENT).all(), nm
        got[nm] = raw[G:G + nbytes].view(dt)
    assert ((got["cand_free"] >= 0) & (got["cand_free"] <= T)).all()
    assert ((got["cand_hit"] >= -1) & (got["cand_hit"] < len(bad))).all()
    assert st["hit_movers"] == int((got["cand_hit"] >= 0).sum()) and st["collided"] == int((got["cand_free"] < T).sum())
    same(steer(f, name), dr.scene_reference(name), "after the list out of bounds")
    f.close()


# ---- the blobs -------------------------------------------------------------------------------------------------------------------------
def blob_kw(s):
    c = s["c"]
    return dict(s["cam"], grid_pose=s["grid_pose"], cam_pose=s["cam_pose"], width=c["width"], height=c["height"], res=c["res"], floor_max=c["floor_max"],
                z_max=c["z_max"], min_points=s["min_points"], max_blobs=s["max_blobs"])


def same_blobs(got, want, what):
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert got["blobs"].dtype == np.int32 and got["blobs"].shape == want["blobs"].shape and (got["blobs"] == want["blobs"]).all(), (
        what, got["blobs"][:4].tolist(), want["blobs"][:4].tolist())


# every kind at every camera of BLOB_CAMERAS (cam0 .. cam2), and the "blocks" at theirs (cam3, cam4)
BLOB_CASES = [(k, cam, kind) for kind in dr.BLOB_KINDS for k, cam in enumerate(dr.BLOB_CAMERAS)] + \
             [(len(dr.BLOB_CAMERAS) + k, cam, "blocks") for k, cam in enumerate(dr.BLOCK_CAMERAS)]


@pytest.mark.parametrize("cam,kind,fmt", [pytest.param(cam, kind, fmt, id="cam%d-%s-%s" % (k, kind, fmt)) for fmt in ("f32", "u16") for k, cam, kind in BLOB_CASES])
def test_the_blobs(cam, kind, fmt, dyn_lib):
    s, img, scale, want = dr.blob_reference(cam[0], cam[1], kind, fmt)
    if kind == "blocks":                                                 # (on the restatement alone: every label is written)
        assert 20 <= want["stats"]["labels_seen"] == want["stats"]["blobs_written"] <= 64
    f = handle(dyn_lib)
    if fmt == "u16":
        f.set_input_format("rgb8", "u16", scale)
    for direct in (0, 1):
        same_blobs(f.nav_dyn_blobs(img, s["mask"], s["label"], direct=direct, **blob_kw(s)), want, (cam, kind, fmt, direct))
    f.close()


def test_the_blobs_after_a_smaller_frame_on_the_same_handle(dyn_lib):
    """160 x 128, then 17 x 13, then 160 x 128 again with other labels, on one handle: the working buffers (the per-pixel points, the
    slots, the records) are those of the first call, and a smaller frame leaves most of them as the larger one left them"""
    f = handle(dyn_lib)
    for direct in (0, 1):
        for cam, kind in (((160, 128), "blocks"), ((17, 13), "blocks"), ((160, 128), "columns"), ((17, 13), "many"), ((160, 128), "many")):
            s, img, scale, want = dr.blob_reference(cam[0], cam[1], kind, "f32")
            same_blobs(f.nav_dyn_blobs(img, s["mask"], s["label"], direct=direct, **blob_kw(s)), want, (cam, kind, direct))
    s, _, _, want = dr.blob_reference(160, 128, "blocks", "f32")
    assert want["stats"]["labels_seen"] > 64 == want["stats"]["blobs_written"] and (want["blobs"][:, 1] == 15).all()
    f.close()


def test_the_blobs_on_device_images_inside_guard_bytes_twice(fusion):
    import torch
    dev = torch.device("cuda")
    s, img, scale, want = dr.blob_reference(160, 128, "columns", "f32")
    d_depth, d_mask, d_label = (torch.from_numpy(a).to(dev) for a in (img, s["mask"], s["label"]))
    k = want["stats"]["blobs_written"]
    G, SENT = 256, 0x5A
    raws = []
    for _ in range(2):
        buf = torch.full((2 * G + 32 * dr.MAX_BLOBS,), SENT, dtype=torch.uint8, device=dev)
        got = fusion.nav_dyn_blobs_device(d_depth, d_mask, d_label, blobs=buf.data_ptr() + G, **blob_kw(s))
        assert got["blobs"] is None and got["stats"] == want["stats"]
        raws.append(buf.cpu().numpy())
    raw = raws[0]
    assert 0 < k < dr.MAX_BLOBS and (raw[G:G + 32 * k].view(np.int32).reshape(k, 8) == want["blobs"]).all()
    assert (raw[:G] == SENT).all() and (raw[G + 32 * k:] == SENT).all()                              # rows past the count are not written
    assert raws[0].tobytes() == raws[1].tobytes()
    host = fusion.nav_dyn_blobs_device(d_depth, d_mask, d_label, **blob_kw(s))
    assert (host["blobs"] == want["blobs"]).all()


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
def chain_scene():
    """a depth frame over a free floor (tests/navlive_ref.py's room) with the box in it labelled as moving"""
    kw = dict(lr.CAMERA, width=33, height=31, res=0.05, max_dist_cells=6, stride=4)
    cam_pose, grid_pose = lr.room_pose(at=(0.8, 0.0, 0.2)), lr.grid_pose_at()
    depth = lr.room_depth(cam_pose)
    state_in = np.zeros((31, 33), np.int8)
    mask = np.zeros((128, 160), np.uint8)
    mask[40:100, 60:110] = 1
    label = np.where(mask != 0, 40 * 160 + 60, -1).astype(np.int32)
    poses = np.array([sr.centre(16, 4, 16384), sr.centre(2, 2, 0), sr.centre(20, 8, 20000)], np.int32)
    return dict(kw=kw, cam_pose=cam_pose, grid_pose=grid_pose, depth=depth, state_in=state_in, mask=mask, label=label, goals=[(16, 29)], plan=dict(min_dist2=1),
                poses=poses, steer=dict(n_steps=20, clearance_cap=36, brake_div=64, mover_cap=3000, mover_weight=4))


def chain_reference(o):
    def make():
        c_live = lr.params(mask_mode=2, **o["kw"])
        lv = lr.overlay(o["depth"], o["mask"], o["state_in"], o["grid_pose"], o["cam_pose"], c_live)
        tables = [dr.blobs(o["depth"] + np.float32(0.02 * k), o["mask"], o["label"], o["grid_pose"], o["cam_pose"], c_live, 16, 64) for k in (1, 0)]
        t = dr.Tracker(2048, 300, 16, 128)
        t.update(tables[0]["blobs"], 1)
        movers = t.update(tables[1]["blobs"], 2)
        pl = pr.plan(lv["state"], lv["dist2"], o["goals"], None, **o["plan"])
        c = dr.params(width=33, height=31, n_poses=len(o["poses"]), min_dist2=o["plan"]["min_dist2"], **o["steer"])
        return lv, tables, movers, pl, dr.rollouts(lv["state"], lv["dist2"], pl["cost"], o["poses"], None, movers, c), c
    return dr.cached("chain", make)


def test_device_pointers_from_the_mask_and_the_overlay_to_the_command(fusion):
    """the mask and the labels on the device, the overlay without the movers (mask_mode 2), their blobs, the tracker, the plan and the
    rollouts: only the blob table and the command leave the device"""
    import torch
    dev = torch.device("cuda")
    o = chain_scene()
    lv, tables, movers, pl, want, c = chain_reference(o)
    assert len(movers) >= 1 and (movers[:, 2:4] != 0).any() and want["stats"]["hit_movers"] > 0 and (want["best"] >= 0).any()
    gw, gh, n, K, T = 33, 31, len(o["poses"]), c["n_v"] * c["n_w"], c["n_steps"]
    live = dict({k: v for k, v in o["kw"].items() if k not in ("width", "height")}, grid_pose=o["grid_pose"], cam_pose=o["cam_pose"])
    d_mask, d_label, d_state = (torch.from_numpy(o[k]).to(dev) for k in ("mask", "label", "state_in"))
    d_dist2, d_cost = (torch.empty((gh, gw), dtype=torch.int32, device=dev) for _ in range(2))
    tracker = binding.MoverTracker(2048, 300, 16, 128)
    bkw = {k: live[k] for k in ("grid_pose", "cam_pose", "res", "fx", "fy", "cx", "cy", "cam_width", "cam_height", "t_min", "t_max")}
    for k, steps in ((1, 1), (0, 2)):                                    # the object seen twice, two steps apart
        d_depth = torch.from_numpy(o["depth"] + np.float32(0.02 * k)).to(dev)
        table = fusion.nav_dyn_blobs_device(d_depth, d_mask, d_label, width=gw, height=gh, **bkw)
        assert (table["blobs"] == tables[1 - k]["blobs"]).all() and table["stats"] == tables[1 - k]["stats"]
        got_movers = tracker.update(table["blobs"], steps)
    assert (got_movers == movers).all()
    live_stats = fusion.nav_live_device(d_depth, d_state, gw, gh, mask=d_mask, state_out=d_state, dist2=d_dist2, mask_mode=2, **live)
    assert {k: live_stats[k] for k in lr.STATS} == lv["stats"]
    fusion.nav_plan_device(d_state, d_dist2, gw, gh, o["goals"], None, cost=d_cost, **o["plan"])
    d_poses, d_movers = torch.from_numpy(o["poses"]).to(dev), torch.from_numpy(got_movers).to(dev)
    known = binding.NAVSTEER_OUTPUTS + binding.NAVDYN_OUTPUTS
    outs = {nm: torch.zeros(binding.Fusion._navsteer_shape(kind, tail, n, K, T), dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
            for nm, dt, kind, tail in known}
    stats = fusion.nav_dyn_steer_device(d_state, d_dist2, gw, gh, d_poses, n, movers=d_movers, n_movers=len(got_movers), cost=d_cost,
                                        min_dist2=o["plan"]["min_dist2"], **dict(outs, **o["steer"]))
    got = {nm: a.cpu().numpy().view(dt) if dt is np.uint32 else a.cpu().numpy() for (nm, dt, _, _), a in zip(known, outs.values())}
    got["best_traj"] = [got["best_traj"][q, :got["best_len"][q]] for q in range(n)]
    got["stats"] = stats
    same(got, want, "device pointers")
    # the movers matter on this scene: without them the rollouts differ
    still = dr.rollouts(lv["state"], lv["dist2"], pl["cost"], o["poses"], None, None, c)
    assert (still["cand_free"] != want["cand_free"]).any()


def test_nav_live_dyn_steer_is_the_chain_of_its_calls(dyn_lib):
    """motion mask, overlay without the movers, blobs, tracker, plan, rollouts in one call, against the same calls made one by one with
    host arrays on a second handle with the same map"""
    A, B = handle(dyn_lib), handle(dyn_lib)
    for k in (0, 3):
        rgb, depth = util.frame(k, W, H)
        A.process_frame(rgb, depth)
        B.process_frame(rgb, depth)
    rgb, depth = util.frame(6, W, H)
    near = depth.copy()
    near[30:100, 50:110] = np.minimum(near[30:100, 50:110], np.float32(0.6))                          # something stands in front of the map
    grid = A.nav_grid(outputs=("state", "dist2"), res=0.1)
    pose, state = grid["stats"]["pose"], grid["state"]
    poses = binding.Fusion.nav_steer_units([(state.shape[1] * 0.05, state.shape[0] * 0.05, 0.0)], 0.1)
    goals = [(state.shape[1] // 2 + 5, state.shape[0] // 2)]
    ta, tb = binding.MoverTracker(inflate=200), binding.MoverTracker(inflate=200)
    steer_kw = dict(n_steps=12, mover_weight=3)
    for step, img in enumerate((near, near)):
        got = A.nav_live_dyn_steer(img, state, goals, poses, ta, steps_since=2, live=dict(grid_pose=pose, res=0.1, min_hits=2, stride=8),
                                   blobs=dict(min_points=8), plan=dict(min_dist2=1), steer=steer_kw)
        mm = B.motion_mask(img, outputs=("mask", "label"))
        assert got["motion"]["stats"] == mm["stats"]
        lv = B.nav_live(img, state, mask=mm["mask"], outputs=("state", "dist2"), grid_pose=pose, res=0.1, min_hits=2, stride=8, mask_mode=2)
        tb_table = B.nav_dyn_blobs(img, mm["mask"], mm["label"], grid_pose=pose, res=0.1, width=state.shape[1], height=state.shape[0], min_points=8)
        assert (got["blobs"]["blobs"] == tb_table["blobs"]).all() and got["blobs"]["stats"] == tb_table["stats"]
        movers = tb.update(tb_table["blobs"], 2)
        assert (got["movers"] == movers).all()
        cost = B.nav_plan(lv["state"], lv["dist2"], goals, None, outputs=("cost",), min_dist2=1)["cost"]
        want = B.nav_dyn_steer(lv["state"], lv["dist2"], poses, movers=movers, cost=cost, min_dist2=1, **steer_kw)
        for nm in binding.NAVSTEER_POSE_OUTPUTS + ("best_min_gap",):
            if nm == "best_traj":
                assert all((x == y).all() for x, y in zip(got["steer"][nm], want[nm]))
            else:
                assert (got["steer"][nm] == want[nm]).all(), (step, nm)
        assert got["steer"]["stats"] == want["stats"]
    assert mm["stats"]["pixels_masked"] > 0 and len(movers) >= 1, (mm["stats"], tb_table["stats"])
    B.close()
    A.close()


# ---- conventions -------------------------------------------------------------------------------------------------------------------
def test_a_call_between_two_frames_changes_no_later_result(dyn_lib):
    A, B = handle(dyn_lib), handle(dyn_lib)
    s, img, scale, want_blobs = dr.blob_reference(160, 128, "columns", "f32")
    for k in (0, 3, 6):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        same(steer(A, "two movers one step"), dr.scene_reference("two movers one step"), "between frames")
        same(steer(A, "foot 37x53"), dr.scene_reference("foot 37x53"), "between frames, footprint")
        got = A.nav_dyn_blobs(img, s["mask"], s["label"], **blob_kw(s))
        assert (got["blobs"] == want_blobs["blobs"]).all() and got["stats"] == want_blobs["stats"]
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)
    B.close()
    A.close()


def test_the_refusals_leave_the_handle_working(dyn_lib):
    f = handle(dyn_lib)
    name = "two movers one step"
    s = dr.scene_inputs(name)
    c = s["c"]
    rolled = pytest.raises(binding.SsfError, match=r"ssf_navdyn_rollouts failed \(-1\)")
    base = dict(cost=s["cost"], **call_kw(c))
    ok = s["movers"][:1]
    for bad in ((1 << 24) + 1, 0, 0, 0, 10, 0), (0, -(1 << 24) - 1, 0, 0, 10, 0), (0, 0, 4097, 0, 10, 0), (0, 0, 0, -4097, 10, 0), (0, 0, 0, 0, -1, 0), \
               (0, 0, 0, 0, (1 << 20) + 1, 0), (0, 0, 0, 0, 10, -1), (0, 0, 0, 0, 10, 4097):
        with rolled:
            f.nav_dyn_steer(s["state"], s["dist2"], s["poses"], movers=np.array([ok[0], bad], np.int32), **base)
    f.nav_dyn_steer(s["state"], s["dist2"], s["poses"], movers=np.array([(1 << 24, -(1 << 24), 4096, -4096, 1 << 20, 4096)], np.int32), **base)       # the limits themselves
    for kw in (dict(mover_cap=-1), dict(mover_cap=65537), dict(mover_weight=-1), dict(mover_weight=1001), dict(n_steps=257), dict(walk=2),
               dict(cost_weight=0, target_weight=0, clear_weight=0, speed_weight=0, turn_weight=0, mover_weight=0)):
        with rolled:
            f.nav_dyn_steer(s["state"], s["dist2"], s["poses"], movers=ok, **dict(base, **kw))
    with rolled:
        f.nav_dyn_steer(s["state"], s["dist2"], s["poses"], movers=np.zeros((65, 6), np.int32), **base)
    with rolled:
        f.nav_dyn_steer(s["state"], s["dist2"], s["poses"], movers=ok, outputs=(), **base)                # every output NULL, over both structs
    # the mover weight alone is a weight; one dyn output alone is an output
    got = f.nav_dyn_steer(s["state"], s["dist2"], s["poses"], movers=s["movers"], outputs=("cand_hit",),
                          **dict(call_kw(c), cost_weight=0, clear_weight=0, speed_weight=0, mover_weight=1))
    assert (got["cand_hit"] == dr.scene_reference(name)["cand_hit"]).all()
    L, byref, vp = dyn_lib.lib, binding.C.byref, binding.C.c_void_p
    q, dp, so, do, st, ds = (binding.SsfNavSteerParams(), binding.SsfNavDynParams(), binding.SsfNavSteerOut(), binding.SsfNavDynOut(), binding.SsfNavSteerStats(),
                             binding.SsfNavDynStats())
    assert L.ssf_navsteer_default_params(f.h, byref(q)) == 0 and L.ssf_navdyn_default_params(f.h, byref(dp)) == 0
    assert f.nav_dyn_default_params()["steer"] == dict(n_movers=0, mover_cap=4096, mover_weight=1)
    assert f.nav_dyn_default_params()["blobs"]["min_points"] == 16 and f.nav_dyn_default_params()["blobs"]["max_blobs"] == 64
    q.width, q.height, q.n_poses, q.cost_weight = c["width"], c["height"], 1, 0
    gap = np.zeros(1, np.int32)
    do.best_min_gap = gap.ctypes.data
    a = lambda x: x.ctypes.data_as(vp)
    mv = np.ascontiguousarray(ok)
    assert L.ssf_navdyn_rollouts(f.h, byref(q), byref(dp), a(s["state"]), a(s["dist2"]), None, a(s["poses"]), None, None, None, byref(do), None, None) == 0      # out NULL, stats NULL
    dp.n_movers = 1
    assert L.ssf_navdyn_rollouts(f.h, byref(q), byref(dp), a(s["state"]), a(s["dist2"]), None, a(s["poses"]), None, None, None, byref(do), None, None) == -1     # movers NULL with n_movers 1
    assert L.ssf_navdyn_rollouts(f.h, byref(q), byref(dp), a(s["state"]), a(s["dist2"]), None, a(s["poses"]), None, a(mv), None, byref(do), byref(st), byref(ds)) == 0
    dp.n_movers = 0
    assert L.ssf_navdyn_rollouts(f.h, byref(q), byref(dp), a(s["state"]), a(s["dist2"]), None, a(s["poses"]), None, a(mv), None, byref(do), None, None) == -1     # movers given with n_movers 0
    assert L.ssf_navdyn_rollouts(f.h, byref(q), None, a(s["state"]), a(s["dist2"]), None, a(s["poses"]), None, None, byref(so), byref(do), None, None) == -1
    assert L.ssf_navdyn_rollouts(f.h, byref(q), byref(dp), a(s["state"]), a(s["dist2"]), None, a(s["poses"]), None, None, byref(so), None, None, None) == -1
    assert L.ssf_navdyn_foot_rollouts(f.h, byref(q), byref(dp), 3, a(s["dist2"]), a(s["dist2"]), None, a(s["poses"]), None, None, None, byref(do), None, None) == -1
    # the blobs
    b, img, scale, want = dr.blob_reference(17, 13, "columns", "f32")
    blobbed = pytest.raises(binding.SsfError, match=r"ssf_navdyn_blobs failed \(-1\)")
    for kw in (dict(min_points=0), dict(max_blobs=0), dict(max_blobs=65), dict(direct=2), dict(res=0.0), dict(width=0), dict(height=4097), dict(fx=0.0),
               dict(t_min=2.0, t_max=1.0), dict(floor_max=float("nan"))):
        with blobbed:
            f.nav_dyn_blobs(img, b["mask"], b["label"], **dict(blob_kw(b), **kw))
    # the handle keeps working: the calls and a frame after the refusals
    same(steer(f, name), dr.scene_reference(name), "after the refusals")
    got = f.nav_dyn_blobs(img, b["mask"], b["label"], **blob_kw(b))
    assert (got["blobs"] == want["blobs"]).all() and got["stats"] == want["stats"]
    f.process_frame(*util.frame(0, W, H))
    same(steer(f, name), dr.scene_reference(name), "after a frame")
    g = handle(dyn_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        steer(g, name)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.nav_dyn_blobs(img, b["mask"], b["label"], **blob_kw(b))
    g.close()
    f.close()


def test_the_kernels_are_timed_under_profile(dyn_lib):
    f = handle(dyn_lib, profile=1)
    f.reset_kernel_times()
    steer(f, "two movers one step")
    steer(f, "foot 37x53")
    s, img, scale, want = dr.blob_reference(17, 13, "columns", "f32")
    f.nav_dyn_blobs(img, s["mask"], s["label"], **blob_kw(s))
    names = f.kernel_times()
    for k in ("navdyn_pack", "navdyn_roll", "navdyn_pick", "navdyn_blob_seen", "navdyn_blob_slots", "navdyn_blob_sum"):
        assert k in names and names[k][1] > 0, (k, names)
    assert "navsteer_roll" not in names and "navfoot_roll" not in names
    f.close()


# ---- replay.py's files and the C++ surface ---------------------------------------------------------------------------------------------
def test_replay_writes_the_commands_on_the_walking_frames(tmp_path, capsys):
    """replay.main() with --nav-steer-movers on the committed fr3_walking frames, end to end: it loads the library that exports the
    movers' entry points itself, and writes the blob table, the movers and the command of every grid"""
    from supersurfel_fusion_amd import replay
    replay.main(["--npz", os.path.join(ROOT, "tests", "golden", "tum_fr3_walking_4frames.npz"), "--out", str(tmp_path / "estimated.txt"),
                 "--nav-grid-dir", str(tmp_path), "--nav-grid-every", "2", "--nav-plan-frontier", "--nav-live", "--nav-steer", "--nav-steer-horizon", "8",
                 "--nav-steer-movers", "--nav-steer-mover-inflate", "0.2", "--nav-steer-mover-gate", "0.8"])
    out = capsys.readouterr().out.splitlines()
    for k in (0, 2):
        blobs, movers = np.load(str(tmp_path / ("%06d_blobs.npy" % k))), np.load(str(tmp_path / ("%06d_movers.npy" % k)))
        assert blobs.dtype == np.int32 and blobs.ndim == 2 and blobs.shape[1] == 8 and movers.shape == (len(blobs), 6) and dr.movers_ok(movers)
        assert os.path.exists(str(tmp_path / ("%06d_steer_traj.npy" % k))) and os.path.exists(str(tmp_path / ("%06d_live_state.npy" % k)))
        line = [l for l in out if l.startswith("nav-movers %06d: movers=%d " % (k, len(movers)))]
        assert len(line) == 1 and "blobs_written=%d" % len(blobs) in line[0], out
        steer_line = [l for l in out if l.startswith("nav-steer %06d: status=" % k)]
        assert len(steer_line) == 1 and "hit_movers=" in steer_line[0], out


def test_the_movers_in_cpp(dyn_lib, fusion, tmp_path):
    """tests/cpp/navdyn_smoke.cpp on the GPU: its counts and FNV-1a checksums equal those of the Python calls on the same arrays"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    libdir = os.path.dirname(dyn_lib.path)
    exe = str(tmp_path / "navdyn_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", cpp, os.path.join(cpp, "navdyn_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip_dyn", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "messages ok=1" in r.stdout, r.stdout
    p = np.arange(70 * 45, dtype=np.uint64)
    h = ((p * 2654435761) & 0xFFFFFFFF) >> 16
    state = np.where(h % 100 < 3, 100, np.where(h % 100 < 5, -1, 0)).astype(np.int8).reshape(45, 70)
    dist2 = np.where(state.ravel() == 0, 1 + (h >> 7) % 40, 0).astype(np.int32).reshape(45, 70)
    cost = fusion.nav_plan(state, dist2, goals=[(60, 30)], outputs=("cost",))["cost"]
    poses = np.array([((5 + 11 * k) * 1024 + 300, (4 + 7 * k) * 1024 + 700, 9000 * k) for k in range(6)], np.int32)
    t = binding.MoverTracker(4096, 400, 16, 128)
    t.update(np.array([(3, 50, 20 * 1024, 14 * 1024, 600, 400, 400, 0), (8, 30, 44 * 1024, 30 * 1024, 500, 300, 400, 0)], np.int32), 1)
    movers = t.update(np.array([(3, 52, 20 * 1024 - 600, 14 * 1024 - 300, 600, 400, 400, 0), (9, 31, 44 * 1024 - 500, 30 * 1024 + 400, 500, 300, 400, 0)], np.int32), 2)
    told = re.search(r"case 9 update 0:(.*)", r.stdout)
    assert [[int(v) for v in row.split()] for row in re.findall(r"\(([-\d ]+)\)", told.group(1))] == movers.tolist()
    kw = dict(n_steps=24, mover_cap=3000, mover_weight=5)
    got = fusion.nav_dyn_steer(state, dist2, poses, movers=movers, cost=cost, outputs=dr.OUTPUTS, **kw)
    c = dr.params(width=70, height=45, n_poses=6, **kw)
    same(got, dr.rollouts(state, dist2, cost, poses, None, movers, c), "the smoke program's arrays")
    fnv = lambda a: pr.fnv1a(np.ascontiguousarray(a).tobytes())
    flat = np.concatenate(got["best_traj"]) if len(got["best_traj"]) else np.zeros((0, 3), np.int32)
    s = got["stats"]
    told = re.search("dynsteer " + " ".join(nm + r"=(\d+)" for nm in ("ok", "admissible", "collided", "steps", "hit")) + " " +
                     " ".join(nm + "=([0-9a-f]{16})" for nm in ("best", "score", "traj", "cand_score", "min_gap", "cand_hit", "cand_min_gap")), r.stdout)
    assert told, r.stdout
    assert tuple(int(v) for v in told.groups()[:5]) == (s["poses_ok"], s["admissible"], s["collided"], s["steps_taken"], s["hit_movers"])
    assert tuple(int(v, 16) for v in told.groups()[5:]) == tuple(fnv(a) for a in (got["best"], got["best_score"], flat, got["cand_score"], got["best_min_gap"],
                                                                                   got["cand_hit"], got["cand_min_gap"]))
    assert s["hit_movers"] > 0 and s["poses_ok"] >= 2
    lay = fusion.nav_foot(state, front=2048, back=1024, left=1024, right=1024, pad=0, n_headings=16)
    gf = fusion.nav_dyn_foot_steer(lay["free_mask"], dist2, poses, 16, movers=movers, cost=cost, outputs=dr.OUTPUTS, **kw)
    told = re.search(r"dynfoot ok=(\d+) admissible=(\d+) hit=(\d+) " + " ".join(nm + "=([0-9a-f]{16})" for nm in ("best", "score", "min_gap", "cand_hit")), r.stdout)
    assert told, r.stdout
    assert tuple(int(v) for v in told.groups()[:3]) == (gf["stats"]["poses_ok"], gf["stats"]["admissible"], gf["stats"]["hit_movers"])
    assert tuple(int(v, 16) for v in told.groups()[3:]) == tuple(fnv(a) for a in (gf["best"], gf["best_score"], gf["best_min_gap"], gf["cand_hit"]))
    # the blobs of the program's wall: depth 1 m everywhere, the left half labelled 7 and the right half 80, through the default frames
    depth, mask = np.ones((H, W), np.float32), np.ones((H, W), np.uint8)
    label = np.where(np.arange(W)[None, :] < 80, 7, 80).astype(np.int32) * np.ones((H, 1), np.int32)
    rt = np.array([1, 0, 0, 0, 0, -1, 0, 1, 0, -1.2, 0, -0.2], np.float32)
    gb = fusion.nav_dyn_blobs(depth, mask, label, grid_pose=rt, width=70, height=45, res=0.05, floor_max=-10.0, z_max=10.0, fx=150.0, fy=150.0, cx=79.5,
                              cy=63.5, cam_width=W, cam_height=H)                                    # (the program's camera)
    told = re.search(r"blobs member=(\d+) band=(\d+) labels=(\d+) kept=(\d+) written=(\d+) rows=([0-9a-f]{16})", r.stdout)
    assert told, r.stdout
    st = gb["stats"]
    assert tuple(int(v) for v in told.groups()[:5]) == (st["pixels_member"], st["points_in_band"], st["labels_seen"], st["blobs_kept"], st["blobs_written"])
    assert int(told.group(6), 16) == fnv(gb["blobs"]) and st["blobs_written"] == 2
