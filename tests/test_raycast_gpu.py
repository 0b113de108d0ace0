"""ssf_raycast (include/ssf_raycast.h) on the MI355X against the numpy restatement (tests/raycast_ref.py, a brute force without any
index): every output and every exact stat at 0 bits -- on hand-built models at the wave and block edges of both stores, ray counts
at the wave edges, the edges of the index (crowded buckets, rows over many cells, oversize rows, colliding cells) and of the walk
(axis-parallel rays, rays in cell faces and through cell corners, far hits), boundary-exact rows with hand-written answers, a store
with holes (before and after its compaction), a real map; plus the index's residency, output subsets, device memory, growth, no
side effects on the frame path, the refusals, profiling and the C++ surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import raycast_ref as rr
import navgrid_ref as nr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay, synthetic

pytestmark = pytest.mark.gpu
W, H = 160, 128
CPP = os.path.join(ROOT, "tests", "cpp")
GOLD = os.path.join(ROOT, "tests", "golden")
INFORMATIVE = ("index_entries", "cells_visited", "candidates_tested", "index_rebuilt")


def handle(lib, **kw):
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


def same_cast(got, want, what, outputs=rr.OUTPUTS):
    for name in outputs:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name, got[name].shape, got[name].dtype)
        util.assert_same_bits(got[name], want[name], what + " " + name)
    for k in rr.STATS:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"][k], want["stats"][k])


def check(f, what, rays, pose=None, model=None, outputs=rr.OUTPUTS, **kw):
    """the cast on the device and in numpy from get_model's rows; pose None = the handle's.  Returns the device result"""
    model = f.get_model() if model is None else model
    q = rr.params(range_min=f.cfg.range_min, range_max=f.cfg.range_max, **kw)
    used = f.get_pose() if pose is None else np.asarray(pose, np.float32)
    want = rr.cast(model, f.counts()["n_visible"], rays, used, q)
    got = f.raycast(rays, outputs=outputs, pose=pose, **kw)
    assert sorted(got) == sorted(tuple(outputs) + ("stats",)), what
    same_cast(got, want, what, outputs)
    assert all(got["stats"][k] >= 0 for k in INFORMATIVE)
    return got


@pytest.fixture(scope="module")
def fusion(product_lib):
    """one handle for the tests that replace the model through set_model"""
    f = handle(product_lib)
    yield f
    f.close()


# ---- hand-built models, every ray count ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nv", rr.SIZES)
def test_hand_built_models(n, nv, fusion):
    f = fusion
    for seed in (0, 1, 2):
        m = rr.hand_model(n, seed)
        f.set_model(m, nv, 100)
        model = f.get_model()
        for name in m:
            util.assert_same_bits(model[name], m[name], "set_model / get_model " + name)
        pose = rr.scene_pose(seed)
        for k in (rr.RAY_COUNTS if seed == 0 else rr.RAY_COUNTS[-1:]):
            rays = rr.scene_rays(m, k, seed)
            got = check(f, "n %d nv %d seed %d rays %d" % (n, nv, seed, k), rays, pose=pose, model=model, **rr.scene_kw(seed))
            assert got["stats"]["rays"] == k
        rays = rr.scene_rays(m, 257, seed)
        check(f, "n %d visible rows" % n, rays, pose=pose, model=model, visible_only=True, **rr.scene_kw(seed))
        if n >= 257:
            assert got["stats"]["rays_hit"] > 0 and got["stats"]["rows_oversize"] > 0 and got["stats"]["index_entries"] > 0


def test_boundary_exact_rows(fusion):
    f = fusion
    m, cases = rr.boundary_cases()
    for name, rows, rays, kw, want in cases:
        sub = {k: np.ascontiguousarray(v[rows]) for k, v in m.items()}
        f.set_model(sub, len(rows), 100)
        for cell, oversize in ((0.0, len(rows)), (1.0, 0)):              # through the oversize list, and through the grid
            got = check(f, name, rays, pose=rr.BOUNDARY_POSE, model=sub, cell=cell, **kw)
            rr.check_expectations(got, want, "%s cell %g" % (name, cell))
            assert got["stats"]["rows_oversize"] == oversize and (got["stats"]["index_entries"] > 0) == (oversize == 0)


# ---- the index's edges -------------------------------------------------------------------------------------------------------
def test_index_edges(fusion):
    f = fusion
    m = rr.hand_model(1300, 0)
    m["positions"] += np.float32(2.2)                                   # the box 0.4 .. 4 m: all in the positive octant of the lattice
    f.set_model(m, 513, 100)
    rays, pose = rr.scene_rays(m, 257, 0), rr.scene_pose(0)
    rays[:, :3] += (np.full(3, 2.2) @ pose[:9].reshape(3, 3).astype(np.float64)).astype(np.float32)     # (the sensors move with the box)
    kw = rr.scene_kw(0)
    per_cell = lambda st: (st["candidates_tested"] - 257 * st["rows_oversize"]) / max(st["cells_visited"], 1)
    # 8 m cells: the whole box in ONE cell (a large disc may reach into a neighbour): over a thousand rows in the bucket of every visit
    got = check(f, "crowded buckets", rays, pose=pose, model=m, cell=8.0, **kw)["stats"]
    assert got["rows_oversize"] < 20 and got["cells_visited"] > 0 and got["index_entries"] >= got["rows_indexed"] - got["rows_oversize"]
    assert per_cell(got) > 256, got
    # 2 m cells: eight cells hold the box: between one and four rounds of a wave per visit
    got64 = check(f, "more than 64 per bucket", rays, pose=pose, model=m, cell=2.0, **kw)["stats"]
    assert 64 < per_cell(got64) < per_cell(got), got64
    # 6 cm cells: a row is spread over many cells (up to the 64 of the rule), the larger half of the rows is oversize
    got = check(f, "rows over many cells", rays, pose=pose, model=m, cell=0.0625, **kw)["stats"]
    in_grid = got["rows_indexed"] - got["rows_oversize"]
    assert in_grid > 200 and got["rows_oversize"] > 200 and got["index_entries"] > 16 * in_grid, got
    # 4 mm cells: nearly every row is oversize
    got = check(f, "oversize rows", rays, pose=pose, model=m, cell=0.00390625, **kw)["stats"]
    assert got["rows_oversize"] > 0.9 * got["rows_indexed"], got
    # 16 buckets: nearly every cell collides; the same answer from more candidates
    wide = check(f, "default table", rays, pose=pose, model=m, **kw)["stats"]
    got = check(f, "hash_bits at its minimum", rays, pose=pose, model=m, hash_bits=4, **kw)["stats"]
    assert got["index_entries"] == wide["index_entries"] and got["candidates_tested"] > 4 * wide["candidates_tested"], (got, wide)
    assert got["index_rebuilt"] == 1
    got = check(f, "hash_bits at its maximum", rays, pose=pose, model=m, hash_bits=24, **kw)["stats"]
    assert got["candidates_tested"] <= wide["candidates_tested"]


def test_contention_in_one_place(fusion):
    """1300 rows at one position: one bucket's list holds them all; the winner is the smallest index that takes part"""
    f = fusion
    m = rr.hand_model(1300, 0)
    for name in ("positions", "orientations", "dims"):
        m[name][:] = m[name][0]
    f.set_model(m, 513, 100)
    c, n = m["positions"][0].astype(np.float64), m["orientations"][0, 6:9].astype(np.float64)
    o = c + 1.5 * n + np.array([0.01, 0.0, -0.01])
    rays = np.tile(np.concatenate([o, -n]).astype(np.float32), (65, 1))
    rays[1::2, :3] += np.float32(0.3)                                   # every other ray passes beside the discs
    got = check(f, "1300 rows at one position", rays, pose=rr.IDENTITY, model=m, t_min=0.1, t_max=10.0)
    assert (got["index"][0::2] == 0).all() and (got["index"][1::2] == -1).all() and got["stats"]["candidates_tested"] >= 33 * 1300
    above = 1.75 * nr.MIN_CONF                                          # (row 0 has 1.5 MIN_CONF)
    got = check(f, "... above a confidence", rays, pose=rr.IDENTITY, model=m, t_min=0.1, t_max=10.0, min_conf=above)
    first = int(np.flatnonzero(m["confidences"] > np.float32(above))[0])
    assert first > 0 and (got["index"][0::2] == first).all() and got["stats"]["index_rebuilt"] == 0


# ---- the walk's edges -------------------------------------------------------------------------------------------------------
def walk_rays():
    """rays in the map frame (identity pose) for a model inside |x|, |z| < 1.8, -0.8 < y < 1.8 and its far rows at x = 1e5"""
    rays = []
    for axis in range(3):                                               # axis-parallel, both signs, from inside and from outside the box
        for sign in (1.0, -1.0):
            for o in ((0.1, 0.3, -0.2), (0.25, 0.5, -0.75)):            # the second: on multiples of the cell, the ray lies in two cell faces
                d = [0.0, 0.0, 0.0]
                d[axis] = sign
                rays.append(list(o) + d)
                far = list(o)
                far[axis] = -6.0 * sign
                rays.append(far + d)                                    # starts outside, points in
                rays.append(far + [-x for x in d])                      # starts outside, points away
    for a, b in (((-1.0, -0.5, -1.5), (1.0, 0.5, 1.5)), ((-2.0, -1.0, 2.0), (2.0, 1.75, -2.0)), ((0.0, 0.0, 0.0), (0.125, 0.125, 0.125)),
                 ((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0)), ((0.5, 1.0, -1.0), (-0.5, 1.0, 1.0))):     # lattice point to lattice point: through cell corners
        rays.append(list(a) + [q - p for p, q in zip(a, b)])                                       # (non-unit directions)
    rays.append([3.0, 0.5, -0.25, 1.0, 0.0, 0.0])                      # from beside the box to a far row: tt about 1e5
    rays.append([3.0, 0.5, -0.25, 1000.0, 0.0, 0.0])                   # ... with a long direction: tt about 100
    rays.append([rr.FAR - 3.0, 0.5, -0.25, 1.0, 0.0, 0.0])             # from out there
    rays.append([rr.FAR + 50.0, 0.55, -0.2, -1.0, 0.0, 0.0])           # from behind the far rows, back through them into the map
    rays.append([0.0, 40.0, 0.0, 0.0, -1.0, 0.0])                      # from 40 m above, down into the map
    rays.append([0.0, 40.0, 0.0, 0.0, -0.015625, 0.0])                 # ... slowly
    return np.array(rays, np.float32)


def test_walk_edges(fusion):
    f = fusion
    m = rr.hand_model(1300, 2)
    f.set_model(m, 513, 100)
    rays = walk_rays()
    rng = np.random.default_rng(9)
    more = rr.scene_rays(m, 200, 2)
    pose = rr.scene_pose(2).astype(np.float64)
    more = np.concatenate([more[:, :3] @ pose[:9].reshape(3, 3).T + pose[9:], more[:, 3:] @ pose[:9].reshape(3, 3).T], axis=1).astype(np.float32)
    more[:, :3] = np.round(more[:, :3] * 8) / 8                         # origins on lattice points of the default cell
    rays = np.concatenate([rays, more, more * np.float32(1.0) + rng.normal(0, 1e-3, more.shape).astype(np.float32)])
    for what, kw in (("default cell", dict()), ("1 m cells", dict(cell=1.0)), ("8 m cells: the far rows are in the grid", dict(cell=8.0)),
                     ("6 cm cells", dict(cell=0.0625))):
        got = check(f, "walk edges, " + what, rays, pose=rr.IDENTITY, model=m, t_min=0.03125, t_max=1.0e6, **kw)
        far = np.isin(got["index"], np.arange(17, 1300, 100))
        assert far[-len(more) * 2 - 6] and got["t"][-len(more) * 2 - 6] > 9.0e4, what          # the ray from beside the box: not cut short
        assert far[-len(more) * 2 - 5] and far[-len(more) * 2 - 4] and far[-len(more) * 2 - 3], what
        assert got["stats"]["rays_hit"] > 100 and got["stats"]["cells_visited"] > 0
    s8 = f.raycast(rays, pose=rr.IDENTITY, t_min=0.03125, t_max=1.0e6, cell=8.0)["stats"]
    assert s8["rows_oversize"] < 20 and s8["index_rebuilt"] == 1           # (the far rows are entered in the grid at 8 m)
    # a range that ends inside the map, and one that starts behind most of it
    check(f, "short range", rays, pose=rr.IDENTITY, model=m, t_min=0.03125, t_max=0.75)
    check(f, "late range", rays, pose=rr.IDENTITY, model=m, t_min=2.5, t_max=3.0)


# ---- the index stays while the model does --------------------------------------------------------------------------------
def test_the_index_is_kept_until_the_model_or_its_parameters_change(product_lib):
    f = handle(product_lib)
    m = rr.hand_model(1300, 1)
    f.set_model(m, 513, 100)
    rays, pose, kw = rr.scene_rays(m, 257, 1), rr.scene_pose(1), dict(rr.SCENE_RANGE)
    first = check(f, "first call", rays, pose=pose, model=m, **kw)
    assert first["stats"]["index_rebuilt"] == 1
    for what, more in (("again", dict()), ("visible_only", dict(visible_only=True)), ("min_conf", dict(min_conf=nr.MIN_CONF)),
                       ("another range", dict(t_min=0.5, t_max=2.0)), ("another pose", dict())):
        got = check(f, what, rays, pose=rr.IDENTITY if what == "another pose" else pose, model=m, **dict(kw, **more))
        assert got["stats"]["index_rebuilt"] == 0, what
        if what in ("visible_only", "min_conf"):
            assert not np.array_equal(got["index"], first["index"]), what
    for what, more in (("another cell", dict(cell=0.25)), ("another splat_scale", dict(splat_scale=2.0)), ("hash_bits", dict(hash_bits=12))):
        got = check(f, what, rays, pose=pose, model=m, **dict(kw, **more))
        assert got["stats"]["index_rebuilt"] == 1, what
        assert check(f, what + " again", rays, pose=pose, model=m, **dict(kw, **more))["stats"]["index_rebuilt"] == 0
    assert check(f, "back to the defaults", rays, pose=pose, model=m, **kw)["stats"]["index_rebuilt"] == 1
    # set_model
    m2 = rr.hand_model(1300, 2)
    f.set_model(m2, 600, 100)
    got = check(f, "after set_model", rays, pose=pose, model=m2, **kw)
    assert got["stats"]["index_rebuilt"] == 1 and not np.array_equal(got["index"], first["index"])
    # apply_deformation
    npos, nrot, ntr, w4, i4 = util.deformation_for(m2, 16, angle=0.05, shift=0.02)
    f.apply_deformation(npos, nrot, ntr, w4, i4)
    moved = f.get_model()
    assert not np.array_equal(moved["positions"], m2["positions"])
    got = check(f, "after apply_deformation", rays, pose=pose, model=moved, **kw)
    assert got["stats"]["index_rebuilt"] == 1
    assert check(f, "... again", rays, pose=pose, model=moved, **kw)["stats"]["index_rebuilt"] == 0


def test_a_processed_frame_rebuilds_the_index(product_lib):
    f = handle(product_lib)
    fan = replay.laser_scan_rays(257)
    f.process_frame(*util.frame(0, W, H))
    assert check(f, "after frame 0", fan)["stats"]["index_rebuilt"] == 1
    assert check(f, "again", fan)["stats"]["index_rebuilt"] == 0
    f.process_frame(*util.frame(1, W, H))
    got = check(f, "after frame 1", fan)
    assert got["stats"]["index_rebuilt"] == 1 and got["stats"]["rays_hit"] > 0


def test_raycast_kernels_are_timed_under_profile(product_lib):
    f = handle(product_lib, profile=1)
    f.process_frame(*util.frame(0, W, H))
    fan = replay.laser_scan_rays(64)
    f.reset_kernel_times()
    assert f.raycast(fan)["stats"]["index_rebuilt"] == 1
    one = f.kernel_times()
    for k in ("raycast_prep", "raycast_scan", "raycast_fill", "raycast_march"):
        assert k in one and one[k][1] > 0, (k, one)
    assert f.raycast(fan)["stats"]["index_rebuilt"] == 0
    two = f.kernel_times()
    assert two["raycast_march"][1] == one["raycast_march"][1] + 1
    for k in ("raycast_prep", "raycast_scan", "raycast_fill"):
        assert two[k][1] == one[k][1], (k, one, two)


# ---- outputs ----------------------------------------------------------------------------------------------------------------
def test_output_subsets(fusion):
    f = fusion
    m = rr.hand_model(1300, 2)
    f.set_model(m, 513, 100)
    rays, pose, kw = rr.scene_rays(m, 257, 2), rr.scene_pose(2), rr.scene_kw(2)
    full = check(f, "all outputs", rays, pose=pose, model=m, **kw)
    for outputs in (("t",), ("index",), ("point", "normal"), ("color",), ("t", "color"), ("normal",)):
        got = check(f, "outputs %s" % (outputs,), rays, pose=pose, model=m, outputs=outputs, **kw)
        for name in outputs:
            util.assert_same_bits(got[name], full[name], "subset " + name)
    with pytest.raises(binding.SsfError, match="unknown ray cast outputs"):
        f.raycast(rays, outputs=("depth",))


def test_device_rays_and_outputs_equal_the_host_call(fusion):
    import torch
    f = fusion
    m = rr.hand_model(1300, 1)
    f.set_model(m, 513, 100)
    rays, pose, kw = rr.scene_rays(m, 1025, 1), rr.scene_pose(1), rr.scene_kw(1)
    host = check(f, "host", rays, pose=pose, model=m, **kw)
    n = len(rays)
    d_rays = torch.from_numpy(rays).cuda()
    dev = {name: torch.full((n * (3 if tail else 1) + 3,), 7, dtype=torch.int32 if dt is np.int32 else torch.float32, device="cuda")
           for name, dt, tail in binding.RAYCAST_OUTPUTS}
    torch.cuda.synchronize()
    st = f.raycast_device(d_rays, n, pose=pose, **dict(kw, **dev))
    for k in rr.STATS:
        assert st[k] == host["stats"][k], k
    for name, t in dev.items():
        a = t.cpu().numpy()
        util.assert_same_bits(a[:-3].reshape(host[name].shape), host[name], "device " + name)
        assert (a[-3:] == 7).all(), name
    for t in dev.values():
        t.fill_(9)
    torch.cuda.synchronize()
    f.raycast_device(d_rays, n, index=dev["index"], pose=pose, **kw)
    util.assert_same_bits(dev["index"].cpu().numpy()[:-3], host["index"], "device index alone")
    assert all(bool((dev[name] == 9).all()) for name in ("t", "point", "normal", "color"))


def test_the_working_buffers_grow(product_lib):
    f = handle(product_lib, nb_supersurfels_max=30000)
    m = rr.hand_model(257, 0)
    f.set_model(m, 256, 100)
    check(f, "small model, one ray", rr.scene_rays(m, 1, 0), pose=rr.scene_pose(0), model=m, **rr.scene_kw(0))
    check(f, "small model, many rays", rr.scene_rays(m, 5000, 0), pose=rr.scene_pose(0), model=m, **rr.scene_kw(0))
    big = rr.hand_model(30000, 1)
    f.set_model(big, 9000, 100)
    got = check(f, "large model", rr.scene_rays(big, 257, 1), pose=rr.scene_pose(1), model=big, **rr.scene_kw(1))
    assert got["stats"]["rows_indexed"] == 30000 and got["stats"]["index_entries"] > 30000
    check(f, "large model, a fine table", rr.scene_rays(big, 65, 1), pose=rr.scene_pose(1), model=big, cell=0.0625, hash_bits=20, **rr.scene_kw(1))
    f.set_model(m, 256, 100)
    check(f, "small again", rr.scene_rays(m, 64, 0), pose=rr.scene_pose(0), model=m, **rr.scene_kw(0))


def test_more_out_of_view_blocks_than_one_round_of_the_scan(product_lib):
    """270 000 rows, 256 of them visible: 1054 out-of-view blocks, so the one-workgroup scan of their live counts (1024 a round) takes
    a second round, and the logical index of a row of the last blocks comes from the second round's offsets.  The rows are 250 copies
    of a hand-built model of 1080, each copy 4 m further along z; eight rays come down the normals of rows of the last copy.  Then
    513 rows on the same handle: offsets beyond the new block count are stale and must not be read."""
    n, tile, nv = 270000, 1080, 256
    base = rr.hand_model(tile, 3)
    m = {name: np.ascontiguousarray(np.tile(a, (n // tile,) + (1,) * (a.ndim - 1))) for name, a in base.items()}
    m["positions"][:, 2] += np.repeat(np.arange(n // tile, dtype=np.float32) * np.float32(4.0), tile)
    f = handle(product_lib, nb_supersurfels_max=n)
    f.set_model(m, nv, 100)
    first_of_round_two = nv + 1024 * 256
    targets = [k for k in range(n - 1, n - 400, -1) if abs(m["positions"][k, 0]) < 1e3][:8]
    assert len(targets) == 8 and min(targets) >= first_of_round_two
    c, nrm = m["positions"][targets].astype(np.float64), m["orientations"][targets, 6:9].astype(np.float64)
    rays = np.concatenate([c + 0.4 * nrm, -nrm], axis=1).astype(np.float32)
    got = check(f, "270 000 rows", rays, pose=rr.IDENTITY, model=m, t_min=0.05, t_max=8.0)
    assert got["stats"]["rays_hit"] == 8 and got["stats"]["rows_indexed"] == n and (got["index"] >= first_of_round_two).all(), got["index"]
    m2 = rr.hand_model(513, 0)
    f.set_model(m2, 257, 100)
    check(f, "513 rows after 270 000", rr.scene_rays(m2, 257, 0), pose=rr.scene_pose(0), model=m2, **rr.scene_kw(0))
    f.close()


# ---- a store with holes; a real map --------------------------------------------------------------------------------------------
def test_a_store_with_holes_and_its_compaction(product_lib):
    """30 frames of a camera that pans 3 degrees per frame for 15 frames and back (true pose as the prior): rows leave the view and
    come back, which leaves holes in the out-of-view span; compaction (ssf_debug_recentre) moves rows to other slots, so the index is
    rebuilt, and changes no result"""
    f = handle(product_lib, nb_supersurfels_max=20000)
    R0, t0 = synthetic.orbit_pose(0)
    rot_y = lambda deg: nr.rot("y", deg)
    recentres = f.debug_recentre_count()
    for k in range(30):
        deg = 3.0 * (k if k < 15 else 29 - k)
        rgb, depth, _ = synthetic.render(R0 @ rot_y(deg), t0, W, H, noise=True, rng=np.random.default_rng(1000 + k))
        f.process_frame(rgb, depth, prior_pose=nr.pose_about(rot_y(deg), np.zeros(3)))
    cnt = f.counts()
    assert cnt["n_model"] > cnt["n_visible"] > 0, cnt
    assert f.debug_recentre_count() == recentres
    model = f.get_model()
    fan = replay.laser_scan_rays(257)
    u, v = np.meshgrid(np.arange(0, W, 8), np.arange(0, H, 8))
    bundle = np.zeros((u.size, 6), np.float32)
    bundle[:, 3], bundle[:, 4], bundle[:, 5] = (u.ravel() - f.cfg.cx) / f.cfg.fx, (v.ravel() - f.cfg.cy) / f.cfg.fy, 1.0
    look_back = nr.pose_about(rot_y(40.0), np.zeros(3))                  # towards what left the view
    cases = [("fan", fan, None, dict(t_max=20.0, t_min=0.1)), ("bundle", bundle, None, dict()), ("bundle, visible", bundle, None, dict(visible_only=True)),
             ("look back", bundle, look_back, dict(t_max=20.0, t_min=0.1)), ("look back, visible", bundle, look_back, dict(t_max=20.0, t_min=0.1, visible_only=True))]
    before = {name: check(f, "holes " + name, rays, pose=pose, model=model, **kw) for name, rays, pose, kw in cases}
    assert before["bundle"]["stats"]["rays_hit"] > 100 and before["look back"]["stats"]["rays_hit"] > before["look back, visible"]["stats"]["rays_hit"]
    assert (before["look back"]["index"] >= cnt["n_visible"]).any(), "no out-of-view row is hit"
    assert before["look back, visible"]["stats"]["index_rebuilt"] == 0
    f.debug_recentre()
    assert f.debug_recentre_count() == recentres + 1
    for j, (name, rays, pose, kw) in enumerate(cases):
        after = check(f, "compacted " + name, rays, pose=pose, **kw)
        same_cast(after, before[name], "compacted against holes " + name)
        assert after["stats"]["index_rebuilt"] == (1 if j == 0 else 0), name
    for name, a in f.get_model().items():
        util.assert_same_bits(a, model[name], "model after compaction " + name)


def test_a_map_built_from_tum_fr1_xyz(product_lib):
    cfg = dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000)
    f = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    replay.replay(f, replay.frames_from_npz(os.path.join(GOLD, "tum_fr1_xyz_8frames.npz")))
    model = f.get_model()
    got = check(f, "fr1_xyz, a 360-beam fan", replay.laser_scan_rays(360), model=model)
    assert 10 < got["stats"]["rays_hit"] < 360
    u, v = np.meshgrid(np.arange(64) * 10.0 + 5.0, np.arange(48) * 10.0 + 5.0)
    bundle = np.zeros((64 * 48, 6), np.float32)
    bundle[:, 3], bundle[:, 4], bundle[:, 5] = (u.ravel() - f.cfg.cx) / f.cfg.fx, (v.ravel() - f.cfg.cy) / f.cfg.fy, 1.0
    for kw in (dict(), dict(visible_only=True), dict(min_conf=f.cfg.conf_thresh)):
        got = check(f, "fr1_xyz, a 64 x 48 pinhole bundle %s" % sorted(kw), bundle, model=model, **kw)
    assert check(f, "fr1_xyz, every row", bundle, model=model)["stats"]["rays_hit"] > 64 * 48 // 2


# ---- no side effects ----------------------------------------------------------------------------------------------------------
def test_ray_casts_change_no_later_result(product_lib):
    A, B = handle(product_lib), handle(product_lib)
    fan = replay.laser_scan_rays(257)
    for k in range(0, 24, 3):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth)
        A.raycast(fan)
        A.raycast(fan, outputs=("index", "color"), visible_only=True, cell=0.5, t_min=0.1, t_max=30.0)
        A.raycast(fan[:7], pose=rr.IDENTITY, min_conf=A.cfg.conf_thresh, hash_bits=6)
        util.same_result(ra, B.process_frame(rgb, depth))
    util.compare_state(A, B)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_the_refusals(product_lib):
    f = handle(product_lib)
    f.process_frame(*util.frame(0, W, H))
    fan = replay.laser_scan_rays(16)
    nan, inf = float("nan"), float("inf")
    bad = [dict(t_min=-1.0, t_max=2.0), dict(t_min=0.0, t_max=2.0), dict(t_min=2.0, t_max=2.0), dict(t_min=2.0, t_max=1.0), dict(t_min=nan, t_max=2.0),
           dict(t_min=1.0, t_max=nan), dict(t_min=1.0, t_max=inf), dict(splat_scale=-1.0), dict(splat_scale=nan), dict(splat_scale=inf),
           dict(splat_scale=2.0 ** -11), dict(splat_scale=2048.0), dict(cell=-0.1), dict(cell=nan), dict(cell=inf), dict(cell=2.0 ** -11),
           dict(cell=2048.0), dict(hash_bits=3), dict(hash_bits=25), dict(hash_bits=-1), dict(min_conf=nan)]
    for kw in bad:
        with pytest.raises(binding.SsfError, match=r"ssf_raycast failed \(-1\)"):
            f.raycast(fan, **kw)
    with pytest.raises(binding.SsfError, match=r"ssf_raycast failed \(-1\)"):
        f.raycast(fan, outputs=())                                     # every output NULL
    L = product_lib.lib
    p, st = binding.SsfRaycastParams(), binding.SsfRaycastStats()
    byref = binding.C.byref
    assert L.ssf_raycast_default_params(f.h, byref(p)) == 0
    assert L.ssf_raycast_default_params(None, byref(p)) == -1 and L.ssf_raycast_default_params(f.h, None) == -1
    t = np.zeros(16, np.float32)
    tp, rp = binding._ptr(t), binding._ptr(fan)
    assert L.ssf_raycast(None, byref(p), rp, 16, tp, None, None, None, None, byref(st)) == -1       # a NULL handle
    assert L.ssf_raycast(f.h, None, rp, 16, tp, None, None, None, None, byref(st)) == -1            # NULL params
    assert L.ssf_raycast(f.h, byref(p), None, 16, tp, None, None, None, None, byref(st)) == -1      # NULL rays with n > 0
    assert L.ssf_raycast(f.h, byref(p), rp, -1, tp, None, None, None, None, byref(st)) == -1        # n < 0
    assert L.ssf_raycast(f.h, byref(p), rp, 16, None, None, None, None, None, byref(st)) == -1      # every output NULL
    assert L.ssf_raycast(f.h, byref(p), rp, 16, tp, None, None, None, None, None) == 0              # stats are optional
    assert L.ssf_raycast(f.h, byref(p), None, 0, tp, None, None, None, None, byref(st)) == 0        # n == 0: stats only
    assert st.rays == 0 and st.rays_hit == 0 and st.rows_indexed > 0 and st.index_rebuilt == 0
    d = f.raycast_default_params()
    assert d == dict(t_min=0.0, t_max=0.0, min_conf=0.0, splat_scale=0.0, visible_only=0, on_device=0, cell=0.0, hash_bits=0)
    # splat_scale 0 and cell 0 mean the defaults
    util.assert_same_bits(f.raycast(fan, splat_scale=0.0)["t"], f.raycast(fan, splat_scale=3.0)["t"], "splat_scale 0")
    assert f.raycast(fan, cell=0.125, splat_scale=3.0)["stats"]["index_entries"] == f.raycast(fan)["stats"]["index_entries"]
    # the handle keeps working: a cast and a frame after the refusals
    check(f, "after the refusals", fan)
    f.process_frame(*util.frame(1, W, H))
    check(f, "after a frame", fan, t_min=0.1, t_max=30.0)
    # a sharded handle casts no rays
    g = handle(product_lib, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.raycast(fan)
    # a pipelined handle with a frame pending
    q = handle(product_lib, pipeline_depth=2, extract_batch=2)
    q.submit_frame(*util.frame(0, W, H))
    assert q.pending_frames() > 0
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        q.raycast(fan)
    q.process_submitted()
    assert q.pending_frames() == 0
    check(q, "pipelined, at rest", fan)


# ---- replay.py's files, the C++ surface ------------------------------------------------------------------------------------------
def test_replay_writes_the_scans(product_lib, tmp_path):
    f = handle(product_lib)
    frames = [("%d.000000" % k,) + tuple(util.frame(k, W, H)) for k in (0, 3, 6)]
    replay.replay(f, frames, laser_scan_dir=str(tmp_path), laser_scan_every=2, laser_scan_beams=90)
    assert sorted(os.listdir(str(tmp_path))) == ["000000.npy", "000002.npy"]
    want = f.raycast(replay.laser_scan_rays(90), outputs=("t",))["t"]   # the map after the last frame = what frame 2's file shows
    got = np.load(str(tmp_path / "000002.npy"))
    assert got.dtype == np.float32 and got.shape == (90,)
    assert np.array_equal(np.isposinf(got), want == 0) and (want > 0).any() and (want == 0).any()
    util.assert_same_bits(got[want > 0], want[want > 0], "ranges")


def test_cast_rays_in_cpp(product_lib, tmp_path):
    """tests/cpp/raycast_smoke.cpp on the GPU: the counts and the FNV-1a checksums of castRays' outputs equal those of the Python call
    on the same map (the program's six frames, reproduced here); laserScan fills the message double, +inf on the misses"""
    libdir = os.path.dirname(product_lib.path)
    exe = str(tmp_path / "raycast_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "raycast_smoke.cpp"),
                        "-o", exe, "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    got = re.search(r"raycast rays=(\d+) hit=(\d+) invalid=(\d+) rows=(\d+) oversize=(\d+) t=([0-9a-f]{16}) index=([0-9a-f]{16}) "
                    r"point=([0-9a-f]{16}) normal=([0-9a-f]{16}) color=([0-9a-f]{16})", r.stdout)
    assert got, r.stdout
    scan = re.search(r"scan beams=9 hit=(\d+) inf=(\d+) inc=0\.785398 min=0\.25 max=4\.00 forward=(\d+\.\d+) intensities=0", r.stdout)
    assert scan and int(scan.group(1)) + int(scan.group(2)) == 9 and int(scan.group(2)) >= 1, r.stdout
    # the same six frames through the binding: initialize(cam, 16, 10, 1000, 1000, 1e8) with the pre-filter off
    cfg = product_lib.default_config(width=W, height=H, fx=150.0, fy=150.0, cx=79.5, cy=63.5, cell_size=16, lambda_pos=10.0,
                                     lambda_bound=1000.0, lambda_size=1000.0, lambda_disp=1e8, thresh_disp=1e-4, seg_iter=10,
                                     seg_use_ransac=1, nb_samples=16, filter_iter=4, filter_alpha=0.1, filter_beta=1.0,
                                     filter_threshold=0.05, range_min=0.2, range_max=5.0, delta_t=20, conf_thresh=2500.0,
                                     nb_supersurfels_max=50000, icp_iter=10, icp_cov_thresh=0.04, pipeline_depth=0,
                                     extract_batch=1, depth_prefilter=0)
    f = binding.Fusion(product_lib, cfg)
    i = np.arange(W * H)
    for k in range(6):
        x, y = (i % W) + 2 * k, i // W
        rgb = np.stack([x * 255 // (W + 16), y * 255 // H, (x ^ y) & 255], axis=1).astype(np.uint8).reshape(H, W, 3)
        depth = (np.float32(1.0) + np.float32(0.004) * x.astype(np.float32)).astype(np.float32).reshape(H, W)
        f.process_frame(rgb, depth)
    u, v = np.meshgrid(np.arange(5, W, 10), np.arange(4, H, 10))
    rays = np.zeros((u.size, 6), np.float32)
    rays[:, 3] = (u.ravel().astype(np.float32) - np.float32(79.5)) / np.float32(150.0)
    rays[:, 4] = (v.ravel().astype(np.float32) - np.float32(63.5)) / np.float32(150.0)
    rays[:, 5] = 1.0
    want = check(f, "python cast", rays, t_min=0.25, t_max=4.0)
    s = want["stats"]
    assert 0 < s["rays_hit"] <= s["rays"] == 16 * 13

    def fnv(a):
        h = 1469598103934665603
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return "%016x" % h
    assert tuple(int(x) for x in got.groups()[:5]) == (s["rays"], s["rays_hit"], s["rays_invalid"], s["rows_indexed"], s["rows_oversize"]), r.stdout
    assert got.groups()[5:] == tuple(fnv(want[k]) for k in rr.OUTPUTS), r.stdout
