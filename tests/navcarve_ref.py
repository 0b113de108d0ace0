"""The numpy restatement of ssf_navgrid_carve (include/ssf_navcarve.h): steps 1 to 8, every step one IEEE f32 operation in the
header's order on np.float32 scalars and arrays (no einsum, no dot).  The uncarved grid is navgrid_ref.build, the rays go to the map
frame through raycast_ref.transform and get their hits from raycast_ref.cast (the brute force without an index).  carve() is what the
GPU tests compare against at 0 bits.

samples_f64() is an independent formulation of steps 2, 4 and 5 in f64 with matrix products, compared outside a guard band by
tests/test_navcarve.py.

Also here: the scenes and cases that tests/test_navcarve.py and tests/test_navcarve_gpu.py share -- the wall scene, and boundary
cases built from small dyadic rationals with the expected `seen` written out by hand."""
import numpy as np

import navgrid_ref as nr
import raycast_ref as rr

f32 = np.float32
OUTPUTS = nr.OUTPUTS + ("seen",)
GRID_STATS = nr.STATS
RAY_STATS = ("rays", "rays_hit", "rays_invalid", "rays_carving", "ray_samples", "ray_entries", "cells_seen", "cells_carved")
# range_min / range_max and the camera stand for the handle's cfg (t_min = t_max = 0; cam_width = 0): util.make_cfg's handles have
# the library's 0.2 / 5.0 and synthetic.intrinsics(160, 128)
DEFAULTS = dict(fx=0.0, fy=0.0, cx=0.0, cy=0.0, cam_width=0, cam_height=0, stride=8, t_min=0.0, t_max=0.0, ray_min_conf=0.0,
                ray_splat_scale=0.0, hit_margin_cells=1.0, carve_misses=False, min_seen=1, range_min=0.2, range_max=5.0, cfg_camera=None)
GUARD = 1e-4


def params(**kw):
    """a carve as carve() takes it: the keys of Fusion.nav_grid_carve's `carve` with the defaults resolved.  cfg_camera: dict(fx, fy,
    cx, cy, width, height) of the handle, used when cam_width == 0"""
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


def lattice(c):
    """(nu, nv) of step 2"""
    return int(c["cam_width"]) // int(c["stride"]), int(c["cam_height"]) // int(c["stride"])


def camera_rays(c):
    """step 2 in the camera frame: nu * nv x 6 (origin 0, direction d), ray j * nu + i"""
    nu, nv = lattice(c)
    s = int(c["stride"])
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="xy")
    u, v = (i * s + s // 2).ravel().astype(f32), (j * s + s // 2).ravel().astype(f32)
    x, y = (u - f32(c["cx"])) / f32(c["fx"]), (v - f32(c["cy"])) / f32(c["fy"])
    l = np.sqrt((x * x + y * y) + f32(1.0))
    assert l.dtype == np.float32
    zero = np.zeros_like(x)
    return np.stack([zero, zero, zero, x / l, y / l, f32(1.0) / l], axis=1).astype(f32)


def map_rays(views, c):
    """step 2: n_views * nv * nu x 6 (O, D) in the map frame"""
    views = np.asarray(views, f32).reshape(-1, 12)
    cam = camera_rays(c)
    out = np.zeros((len(views) * len(cam), 6), f32)
    for k, pose in enumerate(views):
        O, D, _ = rr.transform(cam, pose)
        out[k * len(cam):(k + 1) * len(cam)] = np.stack(O + D, axis=1)
    return out


def extent(t, hit, valid, q, c):
    """step 4: M per ray (-1: the ray carves nothing)"""
    res = f32(q["res"])
    step, margin = res * f32(0.5), f32(c["hit_margin_cells"]) * res
    with np.errstate(all="ignore"):
        t_end = np.where(hit, t - margin, np.where(valid & bool(c["carve_misses"]), f32(c["t_max"]), f32(-1.0))).astype(f32)
        M = np.where(t_end >= 0, np.floor(t_end / step), -1)
    return M.astype(np.int64)


def sample_cells(O, D, M, pose, q):
    """steps 5: the cell iy * W + ix of samples 0 .. M of ONE ray (O, D: three f32 each) where the sample is accepted, else -1"""
    pose = np.asarray(pose, f32).ravel()
    R, t = pose[:9].reshape(3, 3), pose[9:]
    res = f32(q["res"])
    step = res * f32(0.5)
    W, H = int(q["width"]), int(q["height"])
    with np.errstate(all="ignore"):
        tm = np.arange(M + 1).astype(f32) * step
        d = [(f32(O[k]) + tm * f32(D[k])) - t[k] for k in range(3)]
        C = [(R[0, j] * d[0] + R[1, j] * d[1]) + R[2, j] * d[2] for j in range(3)]
        gx, gy, z = C[0] / res, C[1] / res, C[2]
        assert gx.dtype == np.float32 and z.dtype == np.float32
        ok = (gx >= 0) & (gx < f32(W)) & (gy >= 0) & (gy < f32(H)) & (z > f32(q["floor_max"])) & (z <= f32(q["z_max"]))
        cell = np.where(ok, np.where(ok, gy, 0).astype(np.int64) * W + np.where(ok, gx, 0).astype(np.int64), -1)
    return cell


def entries(cell):
    """step 6: which samples of a ray are entries"""
    prev = np.concatenate([[-1], cell[:-1]])
    return (cell >= 0) & (cell != prev)


def carve(model, n_visible, pose, q, views, c):
    """dict(zmin, zmax, hits, state, dist2, seen, stats) of the grid q in frame `pose` carved by the views (n x 12) with the carve c
    (params()).  stats: navgrid_ref's (the cell counts of the carved state) and RAY_STATS.  Also 'uncarved': the state of step 1."""
    base = nr.build(model, n_visible, pose, q)
    W, H = int(q["width"]), int(q["height"])
    seen = np.zeros(W * H, np.uint32)
    views = np.asarray(views, f32).reshape(-1, 12)
    st = dict(rays=0, rays_hit=0, rays_invalid=0, rays_carving=0, ray_samples=0)
    if len(views):
        rays = map_rays(views, c)
        rq = rr.params(t_min=c["t_min"], t_max=c["t_max"], min_conf=c["ray_min_conf"], splat_scale=c["ray_splat_scale"])
        got = rr.cast(model, n_visible, rays, nr.IDENTITY, rq)
        hit = got["index"] >= 0
        valid = rr.transform(rays, nr.IDENTITY)[2]
        M = extent(got["t"], hit, valid, q, c)
        st.update(rays=len(rays), rays_hit=int(hit.sum()), rays_invalid=int((~valid).sum()), rays_carving=int((M >= 0).sum()),
                  ray_samples=int((M[M >= 0] + 1).sum()))
        for r in np.flatnonzero(M >= 0):
            cell = sample_cells(rays[r, :3], rays[r, 3:], int(M[r]), pose, q)
            np.add.at(seen, cell[entries(cell)], 1)
    seen = seen.reshape(H, W)
    through = seen >= int(c["min_seen"])
    state = np.where((base["state"] < 0) & through, 0, base["state"]).astype(np.int8)
    stats = dict(base["stats"], cells_free=int((state == 0).sum()), cells_occupied=int((state == 100).sum()),
                 cells_unknown=int((state < 0).sum()), ray_entries=int(seen.sum(dtype=np.int64)), cells_seen=int(through.sum()),
                 cells_carved=int(((base["state"] < 0) & (state == 0)).sum()), **st)
    return dict(zmin=base["zmin"], zmax=base["zmax"], hits=base["hits"], state=state, seen=seen, uncarved=base["state"],
                dist2=nr.clearance(state, int(q["max_dist_cells"]), bool(q["unknown_is_obstacle"])), stats=stats)


def samples_f64(views, c, t, hit, valid, pose, q):
    """Steps 2, 4 and 5 in f64 with matrix products, given the hits of step 3 (t, hit, valid per ray).  Returns dict(M, M_uncertain,
    cells): per ray M and whether t_end / step is within GUARD of an integer (or t_end of 0); cells[r] = (cell per sample, uncertain
    per sample) for the samples 0 .. M[r]: a sample is uncertain within GUARD cells of a cell edge or the grid's border, or within
    GUARD metres of floor_max or z_max."""
    views = np.asarray(views, f32).reshape(-1, 12).astype(np.float64)
    nu, nv = lattice(c)
    s = int(c["stride"])
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="xy")
    fx, fy, cx, cy = (np.float64(f32(c[k])) for k in ("fx", "fy", "cx", "cy"))
    d = np.stack([((i * s + s // 2).ravel() - cx) / fx, ((j * s + s // 2).ravel() - cy) / fy, np.ones(nu * nv)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pose = np.asarray(pose, f32).ravel().astype(np.float64)
    R, tg = pose[:9].reshape(3, 3), pose[9:]
    res = np.float64(f32(q["res"]))
    step, margin = 0.5 * res, np.float64(f32(c["hit_margin_cells"])) * res
    W, H = int(q["width"]), int(q["height"])
    fmax, zmax = np.float64(f32(q["floor_max"])), np.float64(f32(q["z_max"]))
    Ms, Munc, cells = [], [], []
    for k, view in enumerate(views):
        Rv, tv = view[:9].reshape(3, 3), view[9:]
        D = d @ Rv.T
        for p in range(nu * nv):
            r = k * nu * nv + p
            t_end = np.float64(t[r]) - margin if hit[r] else (np.float64(f32(c["t_max"])) if valid[r] and c["carve_misses"] else -1.0)
            ratio = t_end / step
            M = int(np.floor(ratio)) if t_end >= 0 else -1
            Ms.append(M)
            Munc.append(bool((hit[r] or (valid[r] and c["carve_misses"])) and (abs(ratio - np.rint(ratio)) < GUARD)))
            if M < 0:
                cells.append((np.zeros(0, np.int64), np.zeros(0, bool)))
                continue
            S = tv[None, :] + (np.arange(M + 1) * step)[:, None] * D[p][None, :]
            C = (S - tg) @ R
            gx, gy, z = C[:, 0] / res, C[:, 1] / res, C[:, 2]
            ok = (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H) & (z > fmax) & (z <= zmax)
            unc = (np.abs(gx - np.rint(gx)) < GUARD) | (np.abs(gy - np.rint(gy)) < GUARD) | (np.abs(z - fmax) < GUARD) | (np.abs(z - zmax) < GUARD)
            cell = np.where(ok, np.floor(np.where(ok, gy, 0)).astype(np.int64) * W + np.floor(np.where(ok, gx, 0)).astype(np.int64), -1)
            cells.append((cell, unc))
    return dict(M=np.array(Ms, np.int64), M_uncertain=np.array(Munc, bool), cells=cells)


# ---- the shared scenes ------------------------------------------------------------------------------------------------------
def _rows(pos, ori, dims, conf, seed):
    n = len(pos)
    rng = np.random.default_rng(seed)
    m = dict(positions=np.asarray(pos, np.float64).reshape(n, 3), colors=rng.uniform(0, 255, (n, 3)), stamps=np.tile([50, 60], (n, 1)),
             orientations=np.asarray(ori, np.float64).reshape(n, 9), shapes=rng.uniform(-1e-3, 1e-3, (n, 6)),
             dims=np.asarray(dims, np.float64).reshape(n, 2), confidences=np.full(n, float(conf)))
    return {name: np.ascontiguousarray(m[name], dt) for name, _, dt in nr.FIELDS}


def view_at(R, t):
    return nr.pose_about(R, t)


WALL_CAMERA = dict(fx=150.0, fy=150.0, cx=79.5, cy=63.5, cam_width=160, cam_height=128, stride=8, t_min=0.05, t_max=8.0)
WALL_GRID = dict(width=33, height=31, res=0.05)
WALL_ROW_IY = 24                                                   # map z = 1.2 is grid y = 1.2: cell row 24


def wall_scene():
    """(model, n_visible, grid pose, grid keywords, views, carve keywords): a floor strip 1 m below the camera (map y = 1.0, x = 0.8 ..
    1.6, z = 0.0 .. 1.5) and a wall across the view at map z = 1.2 (x = 0.4 .. 1.2, y = -0.1 .. 1.0), rows every 0.1 m, one view with
    the identity rotation at (0.8, 0, 0.2) looking along map z.  The grid frame is the default rotation with t = 0.  The floor
    between the camera and x < 0.8 is NOT in the map: the cells there are unknown in the uncarved grid and seen through."""
    pos, ori = [], []
    for ix in range(9):
        for iz in range(16):
            pos.append((0.8 + 0.1 * ix, 1.0, 0.1 * iz))
            ori.append((1, 0, 0, 0, 0, 1, 0, 1, 0))
    for ix in range(9):
        for iy in range(12):
            pos.append((0.4 + 0.1 * ix, -0.1 + 0.1 * iy, 1.2))
            ori.append((1, 0, 0, 0, 1, 0, 0, 0, 1))
    n = len(pos)
    m = _rows(pos, ori, np.full((n, 2), 0.0025), 10.0, 3)
    pose = np.concatenate([nr.FLOOR_R, np.zeros(3, f32)]).astype(f32)
    views = view_at(np.eye(3), (0.8, 0.0, 0.2)).reshape(1, 12)
    return m, n, pose, dict(WALL_GRID), views, dict(WALL_CAMERA)


def check_wall(got, carve_misses, what):
    """the structural conditions of the wall scene on a result (carve()'s or the device's)"""
    s = got["stats"]
    assert s["rays_hit"] > 0 and s["rays"] - s["rays_hit"] > 0, (what, s)
    assert s["cells_carved"] > 0, (what, s)
    occupied = got["state"] == 100
    assert occupied.any(), what
    if "uncarved" in got:
        assert np.array_equal(occupied, got["uncarved"] == 100), what + ": an occupied cell changed its state"
    assert np.array_equal(occupied, got["hits"][..., 1] >= 1), what
    if not carve_misses:
        assert not (got["seen"][occupied] > 0).any(), what + ": seen on an occupied cell"
        assert not (got["seen"][WALL_ROW_IY + 1:] > 0).any(), what + ": seen beyond the wall"


# ---- boundary cases with hand-written answers -----------------------------------------------------------------------------------
ALONG_X = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64)      # a view whose optical axis (camera z) is map +x
BOUNDARY_GRID = dict(width=8, height=4, res=0.25, z_min=-1.0, z_max=1.0, floor_max=0.0, floor_cos=0.5, max_dist_cells=3)
# one pixel: u = v = 0, x = y = 0, l = 1, d = (0, 0, 1) exactly
BOUNDARY_CAMERA = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, cam_width=1, cam_height=1, stride=1, t_min=0.125, t_max=4.0, ray_splat_scale=2.0)


def boundary_cases():
    """Grid = map frame (nr.IDENTITY), res 0.25 (step 0.125), 8 x 4 cells, the band (0, 1].  One row: a disc in the plane x = 1.5
    about (1.5, 0.5, 0.5) with dims 2^-4 (half-axes 0.5 at s = 2), normal along x.  A one-pixel camera looking along map +x from
    (x0, y0, z0): D = (1, 0, 0), tt = 1.5 - x0, sample m at x = x0 + m / 8: every value a small dyadic rational, every f32
    operation exact.  Returns (model, grid keywords, [(name, views, carve keywords, expectations)]); expectations: 'seen' maps
    (ix, iy) to the count (every other cell 0), the rest are stats."""
    m = _rows([(1.5, 0.5, 0.5)], [(0, 1, 0, 0, 0, 1, 1, 0, 0)], [(2.0 ** -4, 2.0 ** -4)], 9.0, 5)
    view = lambda x0, y0, z0: view_at(ALONG_X, (x0, y0, z0)).reshape(1, 12)
    cam = BOUNDARY_CAMERA
    row = lambda iy, xs: {(ix, iy): 1 for ix in xs}
    nan_view = view(0.125, 0.5, 0.5)
    nan_view[0, 4] = np.nan
    cases = [
        # y0 = 0.5: gy = 2 exactly, the edge belongs to row 2.  tt = 1.375, margin 0.25: t_end = 1.125 = 9 steps exactly: M = 9, the last
        # sample at x = 1.25 (gx = 5) counts.  x = 0.125 .. 1.25: gx = 0.5, 1, 1.5, .. 5: cells 0 1 1 2 2 3 3 4 4 5
        ("a ray along a cell edge, t_end a multiple of step", view(0.125, 0.5, 0.5), cam,
         dict(seen=row(2, range(6)), rays=1, rays_hit=1, rays_invalid=0, rays_carving=1, ray_samples=10, ray_entries=6, cells_seen=6)),
        # z0 = 0 = floor_max: z > floor_max fails for every sample (the ray still hits the disc's rim at b = -0.5)
        ("z == floor_max", view(0.125, 0.5, 0.0), cam, dict(seen={}, rays_hit=1, rays_carving=1, ray_samples=10, ray_entries=0, cells_seen=0)),
        # z0 = 1 = z_max: accepted
        ("z == z_max", view(0.125, 0.5, 1.0), cam, dict(seen=row(2, range(6)), rays_hit=1, rays_carving=1, ray_samples=10, ray_entries=6)),
        # no margin: t_end = tt = 1.375 = 11 steps: M = 11, the samples reach x = 1.5 (gx = 6) in the disc's own plane
        ("hit_margin_cells 0", view(0.125, 0.5, 0.5), dict(cam, hit_margin_cells=0.0),
         dict(seen=row(2, range(7)), rays_carving=1, ray_samples=12, ray_entries=7)),
        # margin 1.5 > tt: t_end = -0.125 < 0: M = -1
        ("tt < margin", view(0.125, 0.5, 0.5), dict(cam, hit_margin_cells=6.0),
         dict(seen={}, rays_hit=1, rays_carving=0, ray_samples=0, ray_entries=0, cells_carved=0)),
        # from x0 = -0.375: tt = 1.875, t_end = 1.625 = 13 steps; samples 0..2 at x = -0.375, -0.25, -0.125 are outside (gx < 0), sample
        # 3 at x = 0 is the first inside: an entry although m != 0.  x = 0 .. 1.25: cells 0 0 1 1 2 2 3 3 4 4 5; y0 = 0.375: row 1
        ("a view outside the grid", view(-0.375, 0.375, 0.5), cam,
         dict(seen=row(1, range(6)), rays_hit=1, rays_carving=1, ray_samples=14, ray_entries=6)),
        ("a NaN in the pose", nan_view, dict(cam, carve_misses=True),
         dict(seen={}, rays=1, rays_hit=0, rays_invalid=1, rays_carving=0, ray_samples=0, ray_entries=0)),
        # looking along -x from x0 = 0.625 the ray hits nothing and is valid: with carve_misses it carves t_max = 4 (M = 32) and leaves
        # the grid after x = 0 (sample 5): x = 0.625 .. 0: gx = 2.5 2 1.5 1 0.5 0: cells 2 2 1 1 0 0; without carve_misses nothing
        ("a miss with carve_misses", view_at(-ALONG_X @ np.diag([1, -1, 1]), (0.625, 0.5, 0.5)).reshape(1, 12), dict(cam, carve_misses=True),
         dict(seen=row(2, range(3)), rays_hit=0, rays_invalid=0, rays_carving=1, ray_samples=33, ray_entries=3)),
        ("a miss without carve_misses", view_at(-ALONG_X @ np.diag([1, -1, 1]), (0.625, 0.5, 0.5)).reshape(1, 12), cam,
         dict(seen={}, rays_hit=0, rays_invalid=0, rays_carving=0, ray_samples=0, ray_entries=0)),
    ]
    return m, dict(BOUNDARY_GRID), cases


def check_expectations(got, want, W, H, what):
    seen = np.zeros((H, W), np.uint32)
    for (ix, iy), v in want["seen"].items():
        seen[iy, ix] = v
    assert np.array_equal(got["seen"], seen), (what, got["seen"].tolist())
    for key, v in want.items():
        if key != "seen":
            assert got["stats"][key] == v, (what, key, got["stats"][key], v)


# ---- the device tests' lattices and sample counts --------------------------------------------------------------------------------
# (cam_width, cam_height, stride, n_views) -> 1, 63, 64, 65, 257 and 1025 rays in total
RAY_LATTICES = ((8, 8, 8, 1), (72, 56, 8, 1), (64, 32, 8, 2), (13, 5, 1, 1), (257, 1, 1, 1), (41, 5, 1, 5))
# M + 1 of a ray that carves to t_max: t_max / (res / 2) + 1 with res = 0.25: 1, 63, 64, 65, 129 samples
SAMPLE_COUNTS = ((0.0625, 1), (7.75, 63), (7.875, 64), (8.0, 65), (16.0, 129))
