"""The numpy restatement of ssf_navmem_update (include/ssf_navmem.h): every step one IEEE f32 operation in the header's order on
np.float32 arrays.  The depth, the validity, the lattice, the ray's extent and the clearance are navlive_ref's, navcarve_ref's and
navgrid_ref's (the header takes them from ssf_navlive.h word for word); what is restated here is the height z beside the cell of a
point and of a sample, the slice of z, and the layer's rule.  update() is what the GPU tests compare against with ==.

The evidence of a frame -- per stamping obstacle point and per accepted sample its (cell, z) -- does not depend on `slices`, the layer
or the tick: evidence() computes it once, and update() takes it, so that the tests vary those for one march.

Also here: the scenes that tests/test_navmem.py and tests/test_navmem_gpu.py share -- the room of navlive_ref with a movable "walker"
box, the low box under a camera pitched up, random layers, and boundary cases of small dyadic rationals."""
import numpy as np

import navcarve_ref as ncr
import navgrid_ref as nr
import navlive_ref as lr
import raycast_ref as rr

f32 = np.float32
LAYER = ("marks", "mark_tick", "seen_tick")
OUTPUTS = LAYER + ("live_hits", "hit_bits", "seen_bits", "state", "dist2")
STATS = ("pixels_valid", "pixels_stamping", "points_in_band", "rays", "rays_carving", "ray_samples", "cells_marked", "cells_newly_marked",
         "cells_cleared", "cells_expired", "bits_cleared", "cells_remembered", "cells_opened", "cells_free", "cells_occupied", "cells_unknown")
MEM_DEFAULTS = dict(slices=16, tick=1, max_mark_age=0, max_seen_age=0)
U32 = 0xFFFFFFFF


def params(**kw):
    """an update as update() takes it: navlive_ref.params (min_seen has no part in it) and the four fields of the memory"""
    mem = {k: kw.pop(k) for k in list(kw) if k in MEM_DEFAULTS}
    assert "min_seen" not in kw and "march" not in kw
    c = lr.params(**kw)
    c.update(MEM_DEFAULTS, **mem)
    assert 1 <= int(c["slices"]) <= 32 and 1 <= int(c["tick"]) <= U32
    return c


def refused_slices(c):
    """what step 2 refuses, in f32"""
    lo, hi = f32(c["floor_max"]), f32(c["z_max"])
    with np.errstate(all="ignore"):
        h = (hi - lo) / f32(int(c["slices"]))
    return bool(not np.isfinite(lo) or not np.isfinite(hi) or not hi > lo or not np.isfinite(h) or not h > 0)


def grid_cell_z(S, grid_pose, c):
    """ssf_navgrid.h steps 1 and 4 on map-frame points S (three f32 arrays): (cell or -1, z)"""
    gp = np.asarray(grid_pose, f32).ravel()
    R, t = gp[:9].reshape(3, 3), gp[9:]
    res, W = f32(c["res"]), int(c["width"])
    with np.errstate(all="ignore"):
        dd = [S[k] - t[k] for k in range(3)]
        C = [(R[0, j] * dd[0] + R[1, j] * dd[1]) + R[2, j] * dd[2] for j in range(3)]
        gx, gy, z = C[0] / res, C[1] / res, C[2]
        assert gx.dtype == np.float32 and z.dtype == np.float32
        ok = (gx >= 0) & (gx < f32(W)) & (gy >= 0) & (gy < f32(c["height"])) & (z > f32(c["floor_max"])) & (z <= f32(c["z_max"]))
        cell = np.where(ok, np.where(ok, gy, 0).astype(np.int64) * W + np.where(ok, gx, 0).astype(np.int64), -1)
    return cell, z


def slice_bits(z, c):
    """step 2: the u32 bit of the slice of each band height z"""
    n = int(c["slices"])
    lo = f32(c["floor_max"])
    h = (f32(c["z_max"]) - lo) / f32(n)
    q = (np.asarray(z, f32) - lo) / h
    assert q.dtype == np.float32
    k = np.minimum(n - 1, np.floor(q).astype(np.int64))
    assert (k >= 0).all()
    return (np.uint64(1) << k.astype(np.uint64)).astype(np.uint32)


def evidence(depth, mask, grid_pose, cam_pose, c, depth_format="f32", depth_scale=1.0):
    """dict(pt_cell, pt_z: the stamping obstacle points; sm_cell, sm_z: the accepted samples of all rays; the pixel and ray stats)"""
    d = lr.metres(depth, depth_format, depth_scale).reshape(int(c["cam_height"]), int(c["cam_width"]))
    valid = lr.valid_pixels(d, c)
    mode = int(c["mask_mode"])
    stamping = valid if mode == 0 else valid & ((np.asarray(mask).reshape(d.shape) != 0) == (mode == 1))
    # the point of every pixel (ssf_navlive.h step 2)
    H, W = d.shape
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cp = np.asarray(cam_pose, f32).ravel()
    Rc, tc = cp[:9].reshape(3, 3), cp[9:]
    with np.errstate(all="ignore"):
        x, y = (u.astype(f32) - f32(c["cx"])) / f32(c["fx"]), (v.astype(f32) - f32(c["cy"])) / f32(c["fy"])
        px, py = x * d, y * d
        M3 = [((Rc[i, 0] * px + Rc[i, 1] * py) + Rc[i, 2] * d) + tc[i] for i in range(3)]
    cell, z = grid_cell_z(M3, grid_pose, c)
    assert np.array_equal(cell, lr.point_cells(d, cam_pose, grid_pose, c))          # the same cell as the stateless overlay's
    pt = stamping & (cell >= 0)
    # the rays (ssf_navlive.h step 4), all of them at once: sample m of ray r in row r, column m
    s = int(c["stride"])
    nu, nv = ncr.lattice(c)
    cam = ncr.camera_rays(c)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="xy")
    ru, rv = (i * s + s // 2).ravel(), (j * s + s // 2).ravel()
    dl, has_ray = d[rv, ru], valid[rv, ru]
    x, y = (ru.astype(f32) - f32(c["cx"])) / f32(c["fx"]), (rv.astype(f32) - f32(c["cy"])) / f32(c["fy"])
    l = np.sqrt((x * x + y * y) + f32(1.0))
    O, D, rvalid = rr.transform(cam, cam_pose)
    with np.errstate(all="ignore"):
        rvalid = rvalid & np.isfinite(np.stack(O + D)).all(axis=0)
        tt = (dl * l).astype(f32)
    M = np.where(has_ray, ncr.extent(tt, has_ray & rvalid, rvalid, c, dict(c, carve_misses=False)), -1)
    sm_cell, sm_z = [np.zeros(0, np.int64)], [np.zeros(0, f32)]
    step = f32(c["res"]) * f32(0.5)
    rays = np.flatnonzero(M >= 0)
    for lo in range(0, len(rays), 2048):
        r = rays[lo:lo + 2048]
        m = np.arange(int(M[r].max()) + 1)
        with np.errstate(all="ignore"):
            tm = (m.astype(f32) * step)[None, :]
            S = [O[k][r].astype(f32)[:, None] + tm * D[k][r].astype(f32)[:, None] for k in range(3)]
        assert S[0].dtype == np.float32
        cc, zz = grid_cell_z(S, grid_pose, c)
        keep = (m[None, :] <= M[r][:, None]) & (cc >= 0)
        sm_cell.append(cc[keep]); sm_z.append(zz[keep])
    return dict(pt_cell=cell[pt], pt_z=z[pt], sm_cell=np.concatenate(sm_cell), sm_z=np.concatenate(sm_z),
                stats=dict(pixels_valid=int(valid.sum()), pixels_stamping=int(stamping.sum()), points_in_band=int(pt.sum()), rays=int(has_ray.sum()),
                           rays_carving=int((M >= 0).sum()), ray_samples=int((M[M >= 0] + 1).sum())))


def frame_bits(ev, c):
    """step 3: (live_hits, hit_bits, seen_bits), each height x width u32"""
    W, H = int(c["width"]), int(c["height"])
    hits = np.bincount(ev["pt_cell"], minlength=W * H).astype(np.uint32)
    hit_bits, seen_bits = np.zeros(W * H, np.uint32), np.zeros(W * H, np.uint32)
    np.bitwise_or.at(hit_bits, ev["pt_cell"], slice_bits(ev["pt_z"], c))
    np.bitwise_or.at(seen_bits, ev["sm_cell"], slice_bits(ev["sm_z"], c))
    return hits.reshape(H, W), hit_bits.reshape(H, W), seen_bits.reshape(H, W)


def zero_layer(W, H):
    return {nm: np.zeros((H, W), np.uint32) for nm in LAYER}


def cells_rule(hits, hit_bits, seen_bits, state_in, layer_in, c):
    """steps 4 and 5 and the cell stats on arrays of one shape: dict(marks, mark_tick, seen_tick, state, stats)"""
    u = lambda a: np.asarray(a, np.uint32).astype(np.uint64)
    tick, amax, smax = int(c["tick"]), int(c["max_mark_age"]), int(c["max_seen_age"])
    m_in, mt_in, st_in = u(layer_in["marks"]), u(layer_in["mark_tick"]), u(layer_in["seen_tick"])
    sb = u(seen_bits)
    hb = np.where(np.asarray(hits, np.uint32) >= int(c["min_hits"]), u(hit_bits), np.uint64(0))
    m = (m_in & (~sb & np.uint64(U32))) | hb
    mt = np.where(hb != 0, np.uint64(tick), mt_in)
    cleared = (m_in != 0) & (m == 0)
    bits = m_in & sb & (~hb & np.uint64(U32))
    age = (np.uint64(tick) - mt) & np.uint64(U32)                       # modulo 2^32
    expired = (m != 0) & (amax > 0) & (age > np.uint64(amax))
    m = np.where(expired, np.uint64(0), m)
    mt = np.where(m == 0, np.uint64(0), mt)
    st = np.where(sb != 0, np.uint64(tick), st_in)
    sage = (np.uint64(tick) - st) & np.uint64(U32)
    st = np.where((st != 0) & (smax > 0) & (sage > np.uint64(smax)), np.uint64(0), st)
    state_in = np.asarray(state_in, np.int8)
    occ = (state_in == 100) | (m != 0)
    free = ~occ & ((state_in == 0) | (bool(c["open_unknown"]) & (st != 0)))
    state = np.where(occ, 100, np.where(free, 0, -1)).astype(np.int8)
    popcount = lambda a: sum(((a >> np.uint64(k)) & np.uint64(1)).astype(np.int64) for k in range(32))
    stats = dict(cells_marked=int((m != 0).sum()), cells_newly_marked=int(((m != 0) & (m_in == 0)).sum()), cells_cleared=int(cleared.sum()),
                 cells_expired=int(expired.sum()), bits_cleared=int(popcount(bits).sum()),
                 cells_remembered=int(((state == 100) & (state_in != 100) & (hb == 0)).sum()),
                 cells_opened=int(((state_in != 100) & (state_in != 0) & (state == 0)).sum()), cells_free=int((state == 0).sum()),
                 cells_occupied=int((state == 100).sum()), cells_unknown=int((state < 0).sum()))
    return dict(marks=m.astype(np.uint32), mark_tick=mt.astype(np.uint32), seen_tick=st.astype(np.uint32), state=state, stats=stats)


def update_from(ev, state_in, layer_in, c):
    """dict(the eight outputs, stats) of a frame's evidence on state_in (height x width i8) and layer_in (dict of three, or None)"""
    W, H = int(c["width"]), int(c["height"])
    hits, hit_bits, seen_bits = frame_bits(ev, c)
    got = cells_rule(hits, hit_bits, seen_bits, np.asarray(state_in, np.int8).reshape(H, W), layer_in or zero_layer(W, H), c)
    got["stats"] = dict(ev["stats"], **got["stats"])
    got.update(live_hits=hits, hit_bits=hit_bits, seen_bits=seen_bits,
               dist2=nr.clearance(got["state"], int(c["max_dist_cells"]), bool(c["unknown_is_obstacle"])))
    return got


def update(depth, mask, state_in, layer_in, grid_pose, cam_pose, c, depth_format="f32", depth_scale=1.0):
    return update_from(evidence(depth, mask, grid_pose, cam_pose, c, depth_format, depth_scale), state_in, layer_in, c)


# ---- the shared scenes ------------------------------------------------------------------------------------------------------
def boxes_depth(pose, boxes, cam=lr.CAMERA):
    """navlive_ref.room_depth with any boxes ((x0, x1), (y0, y1), (z0, z1)) in the place of its one: floor, wall and boxes intersected
    analytically in f64 with the pixel's ray, the nearest taken, cast to f32 (0 where nothing is hit)"""
    W, H = cam["cam_width"], cam["cam_height"]
    p = np.asarray(pose, np.float64).ravel()
    R, c = p[:9].reshape(3, 3), p[9:]
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ray = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones((H, W))], axis=-1) @ R.T
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        for axis, level in ((1, lr.FLOOR_Y), (2, lr.WALL_Z)):
            t = (level - c[axis]) / ray[..., axis]
            best = np.where((t > 0) & (t < best), t, best)
        for box in boxes:
            lo = np.stack([(box[k][0] - c[k]) / ray[..., k] for k in range(3)])
            hi = np.stack([(box[k][1] - c[k]) / ray[..., k] for k in range(3)])
            t0, t1 = np.minimum(lo, hi).max(axis=0), np.maximum(lo, hi).min(axis=0)
            best = np.where((t0 <= t1) & (t0 > 0) & (t0 < best), t0, best)
    return np.where(np.isfinite(best), best, 0.0).astype(f32)


# The walker: a box 0.2 m wide, 0.15 m deep and 1.3 m tall crosses the room 1.4 m in front of the camera, a quarter metre a frame, so
# that no two footprints share a cell.  The grid's corner is moved so that camera, walker and wall are inside it.
WALKER_FRAMES = 6
WALKER_CAM = lr.room_pose(at=(0.8, 0.0, -0.6))
WALKER_GRID = lr.grid_pose_at(-0.8, -1.0)
WALKER_KW = dict(lr.CAMERA, width=65, height=64, res=0.05, max_dist_cells=6, stride=4)


def walker_box(k):
    x0 = 0.1 + 0.25 * k
    return ((x0, x0 + 0.2), (-0.3, lr.FLOOR_Y), (0.82, 0.97))


def walker_depth(k):
    """frame k of the crossing; k None: the empty room"""
    return boxes_depth(WALKER_CAM, [] if k is None else [walker_box(k)])


# The low box: a box whose top is half a metre below the camera, 1.6 m in front of it (the walker's camera and grid), seen from the level
# camera, then the camera pitched up by 25 degrees: its lowest ray rises, so every ray crosses the box's cells above the camera's height,
# in higher slices than the box's.  Rows of the grid below LOWBOX_ROWS hold the box, the wall lies behind them.
LOW_BOX = ((0.7, 0.95), (0.5, lr.FLOOR_Y), (1.0, 1.15))
LOWBOX_ROWS = 44
LOWBOX_KW = dict(lr.CAMERA, width=65, height=64, res=0.05, max_dist_cells=6, stride=2, min_hits=2)
LOWBOX_GRID = lr.grid_pose_at(-0.8, -1.0)
LOWBOX_POSES = (lr.room_pose(at=(0.8, 0.0, -0.6)), lr.room_pose(pitch=25.0, at=(0.8, 0.0, -0.6)))


def lowbox_depth(k):
    return boxes_depth(LOWBOX_POSES[k], [LOW_BOX])


def random_layer(W, H, seed, tick, max_mark_age, max_seen_age, slices=32):
    """a layer with marks in a fifth of the cells (bits below `slices`) and ticks on both sides of the two ages as seen from `tick`"""
    rng = np.random.default_rng(7000 + seed)
    marked = rng.random((H, W)) < 0.2
    full = (1 << slices) - 1
    marks = np.where(marked, np.maximum(rng.integers(0, 1 << 32, (H, W), dtype=np.uint64) & np.uint64(full), 1), 0).astype(np.uint32)
    back = lambda age: ((tick - rng.integers(0, 2 * max(age, 2) + 1, (H, W))) & U32).astype(np.uint32)
    mark_tick = np.where(marked, np.maximum(back(max_mark_age), 1), 0).astype(np.uint32)
    seen_tick = np.where(rng.random((H, W)) < 0.5, np.maximum(back(max_seen_age), 1), 0).astype(np.uint32)
    return dict(marks=marks, mark_tick=mark_tick, seen_tick=seen_tick)


# ---- boundary cases with hand-written answers -----------------------------------------------------------------------------------
# navlive_ref.BOUNDARY's one-pixel camera along map +x from (x0, y0, z0), grid = map frame, res 0.25, 8 x 4 cells, band (0, 1]: the point
# lies at (x0 + d, y0, z0) and the ray runs at the height z0, so with 4 slices of 0.25 the slice is ceil(z0 / 0.25) - 1 bar the edges.
def boundary_cases():
    """[(name, depth, (x0, y0, z0), keywords, expectations)]: 'hit_bits' / 'seen_bits' map (ix, iy) to the word (every other cell 0)"""
    row = lambda iy, xs, word: {(ix, iy): word for ix in xs}
    return [
        # the point at x = 1.5 (cell 6), its ray over cells 0 .. 5 (navlive_ref's first case), all at z = 0.5: q = 2.0, slice 2 of 4
        ("4 slices, z = 0.5", 1.375, (0.125, 0.5, 0.5), dict(slices=4), dict(hit_bits={(6, 2): 4}, seen_bits=row(2, range(6), 4))),
        ("1 slice", 1.375, (0.125, 0.5, 0.5), dict(slices=1), dict(hit_bits={(6, 2): 1}, seen_bits=row(2, range(6), 1))),
        ("32 slices, z = 0.5", 1.375, (0.125, 0.5, 0.5), dict(slices=32), dict(hit_bits={(6, 2): 1 << 16}, seen_bits=row(2, range(6), 1 << 16))),
        ("z == z_max is the top slice", 1.375, (0.125, 0.5, 1.0), dict(slices=4), dict(hit_bits={(6, 2): 8}, seen_bits=row(2, range(6), 8))),
        ("z == z_max, 32 slices", 1.375, (0.125, 0.5, 1.0), dict(slices=32), dict(hit_bits={(6, 2): 1 << 31}, seen_bits=row(2, range(6), 1 << 31))),
        ("z just above floor_max is slice 0", 1.375, (0.125, 0.5, 2.0 ** -20), dict(slices=32), dict(hit_bits={(6, 2): 1}, seen_bits=row(2, range(6), 1))),
        ("z == floor_max is out of the band", 1.375, (0.125, 0.5, 0.0), dict(slices=4), dict(hit_bits={}, seen_bits={})),
        ("a slice's lower edge belongs to it", 1.375, (0.125, 0.5, 0.25), dict(slices=4), dict(hit_bits={(6, 2): 2}, seen_bits=row(2, range(6), 2))),
        ("just under a slice's edge", 1.375, (0.125, 0.5, 0.25 - 2.0 ** -20), dict(slices=4), dict(hit_bits={(6, 2): 1}, seen_bits=row(2, range(6), 1))),
    ]


def check_expectations(got, want, W, H, what):
    for key, words in want.items():
        a = np.zeros((H, W), np.uint32)
        for (ix, iy), n in words.items():
            a[iy, ix] = n
        assert np.array_equal(got[key], a), (what, key, got[key].tolist())


# ---- the parametrised scenes of tests/test_navmem_gpu.py -------------------------------------------------------------------------
# navlive_ref.GPU_CASES' scenes, each with a slice count; both ages on, so that the random layer's ticks fall on both sides of them
GPU_SLICES = (16, 1, 5, 32, 16, 5, 32, 1)
GPU_CASES = tuple(case + (n,) for case, n in zip(lr.GPU_CASES, GPU_SLICES))
GPU_TICK, GPU_AGES = 1000, dict(max_mark_age=40, max_seen_age=25)
_EV = {}


def case_evidence(scene, fmt, stride):
    """(navlive_ref.case_inputs, evidence()) of a scene, computed once and shared (the callers leave it unchanged)"""
    key = (scene, fmt, stride)
    if key not in _EV:
        i = lr.case_inputs(*key)
        c = params(**i["kw"])
        _EV[key] = (i, evidence(i["depth"], None, i["grid_pose"], i["cam_pose"], c, fmt, i["depth_scale"]))
    return _EV[key]


# ---- the parameter space, the masks and the round-edge rays (navlive_ref's inputs with the memory's fields) ------------------------------
PARAM_SLICES, PARAM_LAYER_SEED = 5, 3
PARAM_ROWS = tuple((k, {nm: v for nm, v in over.items() if nm != "min_seen"}, arrays)
                   for k, (over, _, arrays) in enumerate(lr.PARAM_ROWS) if arrays is not None)          # (row of lr.PARAM_ROWS, overrides, arrays)
PARAM_IDS = tuple(lr.PARAM_IDS[k].replace("-min_seen=9", "") for k, _, _ in PARAM_ROWS)
# navlive_ref.PARAM_UNCHANGED's rows, and one more: a fifth of the random layer's cells are marked, so no cell lies further than the
# default's 6 cells from an obstacle and a larger max_dist_cells caps nothing (max_dist_cells = 1 does)
PARAM_UNCHANGED = lr.PARAM_UNCHANGED | {("max_dist_cells=40", "f32"), ("max_dist_cells=40", "u16")}


def param_inputs(fmt, over):
    """navlive_ref.param_inputs with the memory's fields and a random layer: dict(..., kw, c, layer)"""
    i = lr.param_inputs(fmt, over)
    kw = dict(i["kw"], slices=PARAM_SLICES, tick=GPU_TICK, **GPU_AGES)
    c = params(**kw)
    return dict(i, kw=kw, c=c, layer=random_layer(c["width"], c["height"], PARAM_LAYER_SEED, GPU_TICK, slices=PARAM_SLICES, **GPU_AGES))


_WANT = {}


def param_reference(fmt, row):
    """update() of row `row` of PARAM_ROWS (None: the base case), computed once and shared (the callers leave it unchanged)"""
    key = ("param", fmt, row)
    if key not in _WANT:
        i = param_inputs(fmt, {} if row is None else PARAM_ROWS[row][1])
        _WANT[key] = update(i["depth"], None, i["state_in"], i["layer"], i["grid_pose"], i["cam_pose"], i["c"], fmt, i["depth_scale"])
    return _WANT[key]


def masked_inputs(fmt):
    """the parameter space's base case at stride 8 with navlive_ref.modes_mask: the mask modes on the 160 x 128 image"""
    i = lr.case_inputs(lr.PARAM_SCENE, fmt, 8)
    kw = dict(i["kw"], slices=PARAM_SLICES, tick=GPU_TICK, **GPU_AGES)
    c = params(**kw)
    return dict(i, kw=kw, c=c, mask=lr.modes_mask(), layer=random_layer(c["width"], c["height"], PARAM_LAYER_SEED, GPU_TICK, slices=PARAM_SLICES, **GPU_AGES))


SMALL_MEM = dict(slices=7, tick=9, max_mark_age=3, max_seen_age=2)


def small_inputs(fmt):
    """navlive_ref.small_inputs with the memory's fields and a random layer"""
    i = lr.small_inputs(fmt)
    gw, gh, _ = lr.SMALL_GRID
    return dict(i, kw=dict(i["kw"], **SMALL_MEM), layer=random_layer(gw, gh, gw, 9, 3, 2, slices=7))


EDGE_SLICES = 32


def edge_inputs(tilt, shift=0):
    """navlive_ref.edge_inputs with 32 slices"""
    i = lr.edge_inputs(tilt, shift)
    return dict(i, kw=dict(i["kw"], slices=EDGE_SLICES))
