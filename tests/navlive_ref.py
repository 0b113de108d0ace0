"""The numpy restatement of ssf_navlive_overlay (include/ssf_navlive.h): steps 1 to 8, every step one IEEE f32 operation in the
header's order on np.float32 scalars and arrays (no einsum, no dot).  The lattice, the extent, the samples of a ray and its entries
are navcarve_ref's (the header takes them from ssf_navcarve.h word for word), the ray goes to the map frame through
raycast_ref.transform, the clearance and the default frame are navgrid_ref's.  overlay() is what the GPU tests compare against
with ==.

Also here: the scenes that tests/test_navlive.py and tests/test_navlive_gpu.py share -- a room (floor, wall and box, intersected
analytically in f64 and cast to f32), a noise image sprinkled with invalid depths, and boundary cases of small dyadic rationals."""
import numpy as np

import navcarve_ref as ncr
import navgrid_ref as nr
import raycast_ref as rr

f32 = np.float32
OUTPUTS = ("live_hits", "live_seen", "state", "dist2")
STATS = ("pixels_valid", "pixels_stamping", "points_in_band", "rays", "rays_carving", "ray_samples", "ray_entries", "cells_stamped",
         "cells_opened", "cells_free", "cells_occupied", "cells_unknown")
# range_min / range_max and the camera stand for the handle's cfg (t_min = t_max = 0; cam_width = 0): util.make_cfg's handles have
# the library's 0.2 / 5.0 and synthetic.intrinsics(160, 128).  The rest are ssf_navlive_default_params'.
DEFAULTS = dict(width=512, height=512, res=0.05, floor_max=-0.8, z_max=0.5, max_dist_cells=40, unknown_is_obstacle=False,
                fx=0.0, fy=0.0, cx=0.0, cy=0.0, cam_width=0, cam_height=0, t_min=0.0, t_max=0.0, mask_mode=0, min_hits=4, stride=4,
                hit_margin_cells=1.0, min_seen=1, open_unknown=True, range_min=0.2, range_max=5.0, cfg_camera=None, march=True)


def params(**kw):
    """an overlay as overlay() takes it: the fields of ssf_navlive_params (without the poses and the memory flags) with the defaults
    resolved.  cfg_camera: dict(fx, fy, cx, cy, width, height) of the handle, used when cam_width == 0.  march False: the caller
    asks for no live_seen, so with open_unknown 0 step 4 is skipped."""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    c = dict(DEFAULTS, **kw)
    if c["cam_width"] == 0:
        K = c["cfg_camera"]
        assert K is not None, "cam_width == 0 needs the handle's camera"
        c.update(fx=K["fx"], fy=K["fy"], cx=K["cx"], cy=K["cy"], cam_width=K["width"], cam_height=K["height"])
    if c["t_min"] == 0 and c["t_max"] == 0:
        c["t_min"], c["t_max"] = c["range_min"], c["range_max"]
    return c


def metres(depth, depth_format="f32", depth_scale=1.0):
    """step 1: the depth image in metres as the handle's input format reads it"""
    if depth_format == "u16":
        return (np.ascontiguousarray(depth, np.uint16).astype(np.float64) * np.float64(depth_scale)).astype(f32)
    return np.ascontiguousarray(depth, f32)


def valid_pixels(d, c):
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d >= f32(c["t_min"])) & (d <= f32(c["t_max"]))


def point_cells(d, cam_pose, grid_pose, c):
    """step 2 for every pixel of d (H x W f32): the cell iy * W + ix whose obstacle band holds the pixel's point, else -1"""
    H, W = d.shape
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cp, gp = np.asarray(cam_pose, f32).ravel(), np.asarray(grid_pose, f32).ravel()
    Rc, tc, R, t = cp[:9].reshape(3, 3), cp[9:], gp[:9].reshape(3, 3), gp[9:]
    res = f32(c["res"])
    with np.errstate(all="ignore"):
        x, y = (u.astype(f32) - f32(c["cx"])) / f32(c["fx"]), (v.astype(f32) - f32(c["cy"])) / f32(c["fy"])
        px, py = x * d, y * d
        M = [((Rc[i, 0] * px + Rc[i, 1] * py) + Rc[i, 2] * d) + tc[i] for i in range(3)]
        dd = [M[k] - t[k] for k in range(3)]
        C = [(R[0, j] * dd[0] + R[1, j] * dd[1]) + R[2, j] * dd[2] for j in range(3)]
        gx, gy, z = C[0] / res, C[1] / res, C[2]
        assert gx.dtype == np.float32 and z.dtype == np.float32
        ok = (gx >= 0) & (gx < f32(c["width"])) & (gy >= 0) & (gy < f32(c["height"])) & (z > f32(c["floor_max"])) & (z <= f32(c["z_max"]))
        return np.where(ok, np.where(ok, gy, 0).astype(np.int64) * int(c["width"]) + np.where(ok, gx, 0).astype(np.int64), -1)


def corner_bound(c):
    """the refusal of the corners: max over the four corner pixels of (t_max * l) / step, in f32"""
    W, H = int(c["cam_width"]), int(c["cam_height"])
    step = f32(c["res"]) * f32(0.5)
    worst = f32(0)
    for u in (0, W - 1):
        for v in (0, H - 1):
            x, y = (f32(u) - f32(c["cx"])) / f32(c["fx"]), (f32(v) - f32(c["cy"])) / f32(c["fy"])
            l = np.sqrt((x * x + y * y) + f32(1.0))
            worst = max(worst, (f32(c["t_max"]) * l) / step)
    return worst


def overlay(depth, mask, state_in, grid_pose, cam_pose, c, depth_format="f32", depth_scale=1.0):
    """dict(live_hits, live_seen, state, dist2, stats) of the depth image (H x W in the given format) and mask (H x W u8 or None)
    stamped onto state_in (height x width i8) with the overlay c (params())"""
    W, H = int(c["width"]), int(c["height"])
    d = metres(depth, depth_format, depth_scale).reshape(int(c["cam_height"]), int(c["cam_width"]))
    state_in = np.asarray(state_in, np.int8).reshape(H, W)
    valid = valid_pixels(d, c)
    mode = int(c["mask_mode"])
    stamping = valid if mode == 0 else valid & ((np.asarray(mask).reshape(d.shape) != 0) == (mode == 1))
    cell = point_cells(d, cam_pose, grid_pose, c)
    hits = np.bincount(cell[stamping & (cell >= 0)], minlength=W * H).astype(np.uint32)
    seen = np.zeros(W * H, np.uint32)
    st = dict(rays=0, rays_carving=0, ray_samples=0)
    if c["march"] or c["open_unknown"]:
        s = int(c["stride"])
        nu, nv = ncr.lattice(c)
        cam = ncr.camera_rays(c)                                   # ray j * nu + i, direction (x / l, y / l, 1 / l)
        i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="xy")
        u, v = (i * s + s // 2).ravel(), (j * s + s // 2).ravel()
        dl, has_ray = d[v, u], valid[v, u]
        x, y = (u.astype(f32) - f32(c["cx"])) / f32(c["fx"]), (v.astype(f32) - f32(c["cy"])) / f32(c["fy"])
        l = np.sqrt((x * x + y * y) + f32(1.0))
        O, D, rvalid = rr.transform(cam, cam_pose)
        with np.errstate(all="ignore"):
            rvalid = rvalid & np.isfinite(np.stack(O + D)).all(axis=0)
            tt = (dl * l).astype(f32)
        M = np.where(has_ray, ncr.extent(tt, has_ray & rvalid, rvalid, c, dict(c, carve_misses=False)), -1)
        st.update(rays=int(has_ray.sum()), rays_carving=int((M >= 0).sum()), ray_samples=int((M[M >= 0] + 1).sum()))
        for r in np.flatnonzero(M >= 0):
            cells = ncr.sample_cells([O[k][r] for k in range(3)], [D[k][r] for k in range(3)], int(M[r]), grid_pose, c)
            np.add.at(seen, cells[ncr.entries(cells)], 1)
    hits, seen = hits.reshape(H, W), seen.reshape(H, W)
    occ = (state_in == 100) | (hits >= int(c["min_hits"]))
    free = ~occ & ((state_in == 0) | (bool(c["open_unknown"]) & (seen >= int(c["min_seen"]))))
    state = np.where(occ, 100, np.where(free, 0, -1)).astype(np.int8)
    stats = dict(st, pixels_valid=int(valid.sum()), pixels_stamping=int(stamping.sum()), points_in_band=int(hits.sum(dtype=np.int64)),
                 ray_entries=int(seen.sum(dtype=np.int64)), cells_stamped=int(((state_in != 100) & (state == 100)).sum()),
                 cells_opened=int(((state_in != 100) & (state_in != 0) & (state == 0)).sum()), cells_free=int((state == 0).sum()),
                 cells_occupied=int((state == 100).sum()), cells_unknown=int((state < 0).sum()))
    return dict(live_hits=hits, live_seen=seen, state=state, dist2=nr.clearance(state, int(c["max_dist_cells"]), bool(c["unknown_is_obstacle"])),
                stats=stats)


# ---- the shared scenes ------------------------------------------------------------------------------------------------------
CAMERA = dict(fx=150.0, fy=150.0, cx=79.5, cy=63.5, cam_width=160, cam_height=128, t_min=0.2, t_max=5.0)
FLOOR_Y, WALL_Z = 1.0, 1.3                                          # map frame of the room: y down, the floor 1 m below its origin
BOX = ((0.9, 1.15), (0.3, 1.0), (0.6, 0.8))                          # x, y, z extents of the box standing on the floor


def room_pose(yaw=0.0, pitch=0.0, roll=0.0, at=(0.8, 0.0, 0.2)):
    """camera-to-map, 12 floats: yaw about map y, then a little pitch (about x) and roll (about z), degrees"""
    R = nr.rot("y", yaw) @ nr.rot("x", pitch) @ nr.rot("z", roll)
    return nr.pose_about(R, at)


def room_depth(pose, cam=CAMERA):
    """the depth image (H x W f32 metres, 0 where nothing is hit) of the room from `pose`: the floor plane y = FLOOR_Y, the wall
    z = WALL_Z and the box, each intersected analytically in f64 with the pixel's ray (x, y, 1) * d, the nearest taken"""
    W, H = cam["cam_width"], cam["cam_height"]
    p = np.asarray(pose, np.float64).ravel()
    R, c = p[:9].reshape(3, 3), p[9:]
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ray = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones((H, W))], axis=-1) @ R.T
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        for axis, level in ((1, FLOOR_Y), (2, WALL_Z)):
            t = (level - c[axis]) / ray[..., axis]
            best = np.where((t > 0) & (t < best), t, best)
        lo = np.stack([(BOX[k][0] - c[k]) / ray[..., k] for k in range(3)])
        hi = np.stack([(BOX[k][1] - c[k]) / ray[..., k] for k in range(3)])
        t0, t1 = np.minimum(lo, hi).max(axis=0), np.maximum(lo, hi).min(axis=0)
        best = np.where((t0 <= t1) & (t0 > 0) & (t0 < best), t0, best)
    return np.where(np.isfinite(best), best, 0.0).astype(f32)


def noise_depth(W, H, seed, lo=0.1, hi=6.0):
    """uniform depths in [lo, hi) (some out of a 0.2 .. 5 range) with NaN, +inf, -inf, 0 and negative values sprinkled in"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(lo, hi, (H, W)).astype(f32)
    bad = np.array([np.nan, np.inf, -np.inf, 0.0, -1.5], f32)
    k = rng.random((H, W)) < 0.15
    d[k] = bad[rng.integers(0, len(bad), int(k.sum()))]
    d.ravel()[0] = np.nan if W * H > 1 else d.ravel()[0]
    return d


def state_pattern(W, H, seed):
    """a state_in with every kind of value: mostly unknown, some free, a few occupied, a few foreign ones (7, -5, 99)"""
    rng = np.random.default_rng(1000 + seed)
    return rng.choice(np.array([-1, 0, 100, 7, -5, 99], np.int8), size=(H, W), p=[0.7, 0.2, 0.04, 0.02, 0.02, 0.02]).astype(np.int8)


def grid_pose_at(tx=0.0, tz=0.0):
    """the default rotation (grid y = map z, grid z = -map y) with the grid's corner at map (tx, 0, tz)"""
    return np.concatenate([nr.FLOOR_R, np.array([tx, 0.0, tz], f32)]).astype(f32)


# the parametrised scenes of the GPU file: name -> (depth f32, depth format, scale, cam pose, grid pose, overlay keywords, seed).
# tests/test_navlive.py checks on the restatement that none of them is vacuous.
def scenes():
    out = {}
    for name, (yaw, pitch, roll), grid in (("room straight", (0, 0, 0), (33, 31, 0.05)), ("room yaw pitch roll", (12, -4, 3), (65, 64, 0.05)),
                                           ("room rolled", (-15, 5, 20), (33, 31, 0.05))):
        pose = room_pose(yaw, pitch, roll)
        d = room_depth(pose)
        d[:3, :5] = np.array([np.nan, 0.0, np.inf, -1.0, 7.5], f32)  # invalid pixels of every kind
        out[name] = dict(depth=d, cam_pose=pose, grid_pose=grid_pose_at(), seed=len(out),
                         kw=dict(CAMERA, width=grid[0], height=grid[1], res=grid[2], max_dist_cells=6))
    # noise: a long lens, so that the points crowd into a few cells; the camera looks along map z from inside the grid
    d = noise_depth(160, 128, 5, lo=0.1, hi=1.6)
    out["noise"] = dict(depth=d, cam_pose=room_pose(at=(0.8, 0.3, 0.05)), grid_pose=grid_pose_at(), seed=len(out),
                        kw=dict(CAMERA, fx=900.0, fy=900.0, width=33, height=31, res=0.05, max_dist_cells=6, floor_max=-0.5))
    return out


def scene_formats(depth):
    """the two input formats of a scene's depth: ('f32', 1.0, image) and ('u16', 1 / 1000, image in millimetres; invalid -> 0)"""
    with np.errstate(invalid="ignore"):
        mm = np.where(np.isfinite(depth) & (depth > 0), np.minimum(np.rint(depth.astype(np.float64) * 1000.0), 65535), 0).astype(np.uint16)
    return (("f32", 1.0, depth), ("u16", 0.001, mm))


# ---- boundary cases with hand-written answers -----------------------------------------------------------------------------------
# One pixel (u = v = 0, cx = cy = 0: x = y = 0, l = 1), the camera looking along map +x (ncr.ALONG_X), grid = map frame, res 0.25,
# 8 x 4 cells, band (0, 1]: every value a small dyadic rational, every f32 operation exact.  A depth d from (x0, y0, z0) puts the
# point at (x0 + d, y0, z0).
BOUNDARY = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, cam_width=1, cam_height=1, stride=1, t_min=0.125, t_max=4.0, width=8, height=4,
                res=0.25, floor_max=0.0, z_max=1.0, max_dist_cells=3, min_hits=1)


def boundary_cases():
    """[(name, depth, (x0, y0, z0), overlay keywords, expectations)]; expectations: 'hits' / 'seen' map (ix, iy) to the count (every
    other cell 0), the rest are stats"""
    row = lambda iy, xs: {(ix, iy): 1 for ix in xs}
    return [
        # the point at x = 1.5 (gx = 6); tt = 1.375, margin 0.25: M = 9, samples x = 0.125 .. 1.25: cells 0 .. 5 of row 2
        ("a point and its ray", 1.375, (0.125, 0.5, 0.5), {}, dict(hits={(6, 2): 1}, seen=row(2, range(6)), pixels_valid=1, rays=1, rays_carving=1,
                                                                  ray_samples=10, ray_entries=6, points_in_band=1)),
        ("C.z == floor_max", 1.375, (0.125, 0.5, 0.0), {}, dict(hits={}, seen={}, pixels_valid=1, points_in_band=0, ray_entries=0)),
        ("C.z == z_max", 1.375, (0.125, 0.5, 1.0), {}, dict(hits={(6, 2): 1}, seen=row(2, range(6)), points_in_band=1)),
        # the point at x = 0 exactly: gx = 0 is in the grid
        ("gx == 0", 0.5, (-0.5, 0.5, 0.5), {}, dict(hits={(0, 2): 1}, seen={}, points_in_band=1, ray_entries=0)),
        # the point at x = 2 = width * res: gx == width is out
        ("gx == width", 1.0, (1.0, 0.5, 0.5), {}, dict(hits={}, points_in_band=0, pixels_valid=1)),
        ("d == t_min", 0.125, (0.125, 0.5, 0.5), {}, dict(hits={(1, 2): 1}, seen={}, pixels_valid=1, rays=1, rays_carving=0)),
        ("d == t_max", 4.0, (-2.5, 0.5, 0.5), {}, dict(hits={(6, 2): 1}, pixels_valid=1, rays=1, rays_carving=1, ray_samples=31)),
        ("d just past t_max", float(np.nextafter(f32(4.0), f32(5.0))), (-2.5, 0.5, 0.5), {}, dict(hits={}, seen={}, pixels_valid=0, rays=0)),
        # the camera outside the grid: samples enter at x = 0
        ("the camera outside the grid", 1.875, (-0.375, 0.375, 0.5), {}, dict(hits={(6, 1): 1}, seen=row(1, range(6)), ray_samples=14, ray_entries=6)),
    ]


def boundary_pose(x0, y0, z0):
    return nr.pose_about(ncr.ALONG_X, (x0, y0, z0))


def check_expectations(got, want, W, H, what):
    for key in ("hits", "seen"):
        if key in want:
            a = np.zeros((H, W), np.uint32)
            for (ix, iy), n in want[key].items():
                a[iy, ix] = n
            assert np.array_equal(got["live_" + key], a), (what, key, got["live_" + key].tolist())
    for key, n in want.items():
        if key not in ("hits", "seen"):
            assert got["stats"][key] == n, (what, key, got["stats"][key], n)


# ---- the parametrised scenes of tests/test_navlive_gpu.py -------------------------------------------------------------------------
# (scene, depth format, stride); tests/test_navlive.py checks on the restatement that none of them is vacuous: cells stamped, cells
# opened, invalid pixels, and a cell with at least 64 points (contention inside a wave)
GPU_CASES = (("room straight", "f32", 4), ("room straight", "u16", 1), ("room yaw pitch roll", "f32", 8), ("room yaw pitch roll", "u16", 4),
             ("room rolled", "f32", 1), ("room rolled", "u16", 8), ("noise", "f32", 4), ("noise", "u16", 1))


def case_inputs(scene, fmt, stride):
    """dict(depth (in the format), depth_scale, state_in, cam_pose, grid_pose, kw (the overlay's keywords), c (params()))"""
    sc = scenes()[scene]
    _, scale, image = dict((f[0], f) for f in scene_formats(sc["depth"]))[fmt]
    kw = dict(sc["kw"], stride=stride)
    return dict(depth=image, depth_scale=scale, state_in=state_pattern(kw["width"], kw["height"], sc["seed"]), cam_pose=sc["cam_pose"],
                grid_pose=sc["grid_pose"], kw=kw, c=params(**kw))


_WANT = {}


def case_reference(scene, fmt, stride):
    """overlay() of a case, computed once and shared (the callers leave it unchanged)"""
    key = (scene, fmt, stride)
    if key not in _WANT:
        i = case_inputs(*key)
        _WANT[key] = overlay(i["depth"], None, i["state_in"], i["grid_pose"], i["cam_pose"], i["c"], fmt, i["depth_scale"])
    return _WANT[key]


# ---- the parameter space of tests/test_navlive_gpu.py and tests/test_navmem_gpu.py ------------------------------------------------
# One scene, one entry overridden at a time (and two combined rows): (overrides, the outputs the row must change against the base case
# on the overlay, the same on the memory).  min_seen is the overlay's alone: a row of min_seen only has no memory side (None), a
# combined row drops it there.  tests/test_navlive.py and tests/test_navmem.py check on the restatements that every row changes
# its arrays, so that no row repeats the base case.
PARAM_SCENE, PARAM_STRIDE, PARAM_FORMATS = "room rolled", 4, ("f32", "u16")
_SEEN, _STATE, _DIST2, _HITS = ("live_seen",), ("state",), ("dist2",), ("live_hits",)
PARAM_ROWS = tuple((dict(hit_margin_cells=m), _SEEN, ("seen_bits",)) for m in (0.0, 0.37, 2.5, 40.0)) + (
    (dict(min_seen=2), _STATE, None), (dict(min_seen=9), _STATE, None),
    (dict(open_unknown=0), _STATE, _STATE), (dict(unknown_is_obstacle=1), _DIST2, _DIST2),
    (dict(min_hits=1), _STATE, _STATE), (dict(min_hits=64), _STATE, _STATE),
    (dict(t_min=0.9, t_max=1.4), _HITS, _HITS), (dict(t_min=1.05, t_max=1.25), _HITS, _HITS), (dict(floor_max=-0.3, z_max=0.1), _HITS, _HITS),
    (dict(max_dist_cells=1), _DIST2, _DIST2), (dict(max_dist_cells=40), _DIST2, _DIST2),
    (dict(stride=3), _SEEN, ("seen_bits",)), (dict(stride=7), _SEEN, ("seen_bits",)), (dict(stride=64), _SEEN, ("seen_bits",)),
    (dict(open_unknown=0, unknown_is_obstacle=1, hit_margin_cells=0.0), ("state", "dist2", "live_seen"), ("state", "dist2", "seen_bits")),
    (dict(min_hits=64, min_seen=9, stride=7), ("state", "live_seen"), ("state", "seen_bits")))
PARAM_IDS = tuple("-".join("%s=%s" % kv for kv in row[0].items()) for row in PARAM_ROWS)
# The rows that do NOT change their array on this scene, by (id, format): the guard checks that they are exactly these, and that
# another row of the same parameter changes it in that format.  Every valid depth of the scene lies in 0.99 .. 1.36 m, so the range
# 0.9 .. 1.4 cuts nothing off: the range 1.05 .. 1.25, inside the scene's depths, cuts pixels off at both ends.  min_hits = 1 changes
# the state of one cell in f32 and of none with the depths rounded to millimetres (min_hits = 64 changes two in both).
PARAM_UNCHANGED = frozenset({("t_min=0.9-t_max=1.4", "f32"), ("t_min=0.9-t_max=1.4", "u16"), ("min_hits=1", "u16")})


def param_inputs(fmt, over):
    """case_inputs of the parameter space's scene with the keywords `over` in the place of the base case's"""
    i = case_inputs(PARAM_SCENE, fmt, PARAM_STRIDE)
    kw = dict(i["kw"], **over)
    return dict(i, kw=kw, c=params(**kw))


def param_reference(fmt, row):
    """overlay() of row `row` of PARAM_ROWS (None: the base case), computed once and shared (the callers leave it unchanged)"""
    key = ("param", fmt, row)
    if key not in _WANT:
        i = param_inputs(fmt, {} if row is None else PARAM_ROWS[row][0])
        _WANT[key] = overlay(i["depth"], None, i["state_in"], i["grid_pose"], i["cam_pose"], i["c"], fmt, i["depth_scale"])
    return _WANT[key]


# ---- masks --------------------------------------------------------------------------------------------------------------------
def modes_mask(W=160, H=128):
    """the mask of the mask-mode tests: 40 % random, a solid band, values other than 1"""
    mask = (np.random.default_rng(4).random((H, W)) < 0.4).astype(np.uint8) * 3
    mask[:, 60:100] = 1
    return mask


# 37 x 29 at stride 3 on a 31 x 33 grid: partial 16 x 16 pixel tiles both ways (the mask must not be read outside the image), 12 x 9
# lattice pixels with a remainder both ways, a mask of half the pixels with the value 200
SMALL_W, SMALL_H, SMALL_STRIDE = 37, 29, 3
SMALL_GRID = (31, 33, 0.05)
SMALL_KW = dict(fx=60.0, fy=60.0, cx=0.5 * (SMALL_W - 1), cy=0.5 * (SMALL_H - 1), cam_width=SMALL_W, cam_height=SMALL_H, t_min=0.2, t_max=5.0,
                width=SMALL_GRID[0], height=SMALL_GRID[1], res=SMALL_GRID[2], max_dist_cells=5, stride=SMALL_STRIDE, min_hits=3)


def small_inputs(fmt):
    """dict(depth (in the format), depth_scale, mask, state_in, cam_pose, grid_pose, kw) of the small image"""
    gw, gh, _ = SMALL_GRID
    d = noise_depth(SMALL_W, SMALL_H, 7 * SMALL_W + SMALL_H, lo=0.1, hi=1.6)
    _, scale, image = dict((x[0], x) for x in scene_formats(d))[fmt]
    mask = (np.random.default_rng(1).random((SMALL_H, SMALL_W)) < 0.5).astype(np.uint8) * 200
    return dict(depth=image, depth_scale=scale, mask=mask, state_in=state_pattern(gw, gh, gw + SMALL_W), grid_pose=grid_pose_at(0.0, 0.0),
                cam_pose=room_pose(yaw=8.0, roll=2.0, at=(0.8, 0.1, 0.35)), kw=dict(SMALL_KW))


# ---- rays at the round edges ----------------------------------------------------------------------------------------------------
# A 64 x 2 image at stride 1 along map +x over a 160 x 8 grid: 128 lattice pixels = eight waves of sixteen rays.  The depths rise by a
# quarter cell a pixel, so that the rays of row 0 have 49 .. 80 samples and those of row 1 113 .. 144: the rounds of 64 samples end
# inside both rows (64 | 65, 128 | 129).  Two pixels are invalid.  A tilted camera climbs or falls through the slices of the memory.
EDGE_KW = dict(BOUNDARY, width=160, height=8, res=0.05, t_max=4.5, cam_width=64, cam_height=2, fx=2000.0, fy=2000.0, cx=31.5, cy=0.5)
EDGE_TILTS = (5.0, -5.0, 0.0)
EDGE_INVALID = ((0, 7), (1, 40))                                     # (v, u): a NaN and a 0
EDGE_COUNTS = (64, 65, 128, 129)                                     # the sample counts on both sides of a round's end
# With the depths as above a round ends between pixels 31 and 32 of a row, which is between two waves: every wave's rays have one
# number of rounds.  Eight pixels further along the ramp the round ends in the middle of a wave, whose pending pair then lives
# across rays of one round and of two (of two and of three).
EDGE_SHIFTS = (0, 8)


def edge_inputs(tilt, shift=0):
    """dict(depth, state_in, grid_pose, cam_pose, kw) of the round-edge image, its ramp begun `shift` pixels later, seen by the
    camera tilted by `tilt` degrees"""
    u = np.arange(64, dtype=np.float64) + shift
    d = np.stack([1.25 + 0.0125 * u, 2.85 + 0.0125 * u]).astype(f32)
    d[EDGE_INVALID[0]] = np.nan
    d[EDGE_INVALID[1]] = 0.0
    return dict(depth=d, state_in=np.full((8, 160), -1, np.int8), grid_pose=nr.IDENTITY,
                cam_pose=nr.pose_about(ncr.ALONG_X @ nr.rot("x", tilt), (0.0125, 0.2, 0.5)), kw=dict(EDGE_KW))


def edge_ray_counts(tilt, run, shift=0):
    """the sample count of each lattice pixel's ray (2 x 64, 0: no carving ray), each from a call of its own with every other pixel
    invalid; run(depth, inputs) -> the stats of a restatement"""
    i = edge_inputs(tilt, shift)
    n = np.zeros((2, 64), np.int64)
    for v in range(2):
        for u in range(64):
            d = np.zeros((2, 64), f32)
            d[v, u] = i["depth"][v, u]
            n[v, u] = run(d, i)["ray_samples"]
    return n
