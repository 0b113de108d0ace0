"""The numpy restatement of ssf_navgrid_build (include/ssf_navgrid.h): every step one IEEE f32 operation in the header's order, on
np.float32 scalars and arrays (no einsum, no dot), the clearance by the same two separable integer passes.  build() is what the
GPU tests compare against at 0 bits.

Two independent formulations check build() itself (tests/test_navgrid.py): samples_f64(), the sampling and banding in f64 with
matrix products, compared sample by sample outside a guard band (GUARD_CELLS of a cell edge, GUARD_M of a band limit), and
clearance_brute(), the minimum over all obstacle cells written as such.

Also here: the hand-built models, grids and boundary rows that tests/test_navgrid.py and tests/test_navgrid_gpu.py share."""
import numpy as np

f32 = np.float32
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)
# the frame of boundary_rows(): the identity with R02 = R12 = -0, so that C.z = (R02 d.x + R12 d.y) + R22 d.z keeps a -0 height
BOUNDARY_POSE = np.array([1, 0, -0.0, 0, 1, -0.0, 0, 0, 1, 0, 0, 0], f32)
FLOOR_R = np.array([1, 0, 0, 0, 0, -1, 0, 1, 0], f32)          # grid x = map x, grid y = map z, grid z = -map y
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
GUARD_CELLS, GUARD_M = 1e-4, 1e-4
FIELDS = (("positions", 3, np.float32), ("colors", 3, np.float32), ("stamps", 2, np.int32), ("orientations", 9, np.float32),
          ("shapes", 6, np.float32), ("dims", 2, np.float32), ("confidences", 1, np.float32))
OUTPUTS = ("zmin", "zmax", "hits", "state", "dist2")
STATS = ("rows_used", "samples", "samples_in_grid", "cells_free", "cells_occupied", "cells_unknown")
DEFAULTS = dict(width=512, height=512, res=0.05, z_min=-1.5, z_max=0.5, floor_max=-0.8, floor_cos=0.8, min_conf=0.0,
                t_init=(I32_MIN, I32_MAX), t_last=(I32_MIN, I32_MAX), visible_only=False, splat_scale=2.0, max_steps=8, min_hits=1,
                max_dist_cells=40, unknown_is_obstacle=False)


def params(**kw):
    """a grid as build() takes it: the keywords of Fusion.nav_grid (without pose and outputs) with the defaults written out"""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    q = dict(DEFAULTS, **kw)
    q["t_init"] = (I32_MIN, I32_MAX) if q["t_init"] is None else tuple(q["t_init"])
    q["t_last"] = (I32_MIN, I32_MAX) if q["t_last"] is None else tuple(q["t_last"])
    return q


def default_pose(camera_pose, q):
    """what pose NULL means: floor-aligned, centred on the camera position, snapped to the cell size"""
    p = np.asarray(camera_pose, f32).ravel()[9:]
    res = f32(q["res"])
    tx = (np.floor(p[0] / res) - f32(q["width"] // 2)) * res
    tz = (np.floor(p[2] / res) - f32(q["height"] // 2)) * res
    return np.concatenate([FLOOR_R, np.array([tx, 0, tz], f32)]).astype(f32)


def used_rows(model, n_visible, q):
    """step 2: the indices of the rows that are used"""
    pos = np.ascontiguousarray(model["positions"], f32).reshape(-1, 3)
    conf = np.ascontiguousarray(model["confidences"], f32).reshape(-1)
    stamps = np.ascontiguousarray(model["stamps"], np.int32).reshape(-1, 2)
    dims = np.ascontiguousarray(model["dims"], f32).reshape(-1, 2)
    n = len(conf)
    ok = np.arange(n) < (int(n_visible) if q["visible_only"] else n)
    ok &= np.isfinite(pos).all(axis=1)
    ok &= conf > f32(q["min_conf"])
    ok &= (stamps[:, 0] >= q["t_init"][0]) & (stamps[:, 0] <= q["t_init"][1])
    ok &= (stamps[:, 1] >= q["t_last"][0]) & (stamps[:, 1] <= q["t_last"][1])
    with np.errstate(invalid="ignore"):
        ok &= (dims[:, 0] > 0) & (dims[:, 1] > 0) & np.isfinite(dims).all(axis=1)
    return np.flatnonzero(ok)


def lattice(n1, n2):
    """step 3: the (i, j) of the samples that exist, i major"""
    i, j = np.meshgrid(np.arange(-n1, n1 + 1), np.arange(-n2, n2 + 1), indexing="ij")
    keep = i * i * n2 * n2 + j * j * n1 * n1 <= n1 * n1 * n2 * n2
    return i[keep], j[keep]


def _steps(h, step, max_steps):
    with np.errstate(all="ignore"):
        qn = np.ceil(h / step)
        return np.where(qn >= f32(max_steps), max_steps, np.where(qn >= f32(1), qn, 1)).astype(np.int64)


def samples(model, n_visible, pose, q, chunk=1 << 20):
    """Steps 1 to 5 in f32.  Yields, per group of rows with the same lattice and per chunk, a dict of flat arrays, one entry per
    sample that exists: row (logical index), i, j, gx, gy, z, in_grid, accepted (steps 4 and 5), obstacle, floor."""
    pose = np.asarray(pose, f32).ravel()
    R, t = pose[:9].reshape(3, 3), pose[9:]
    rows = used_rows(model, n_visible, q)
    pos = np.ascontiguousarray(model["positions"], f32).reshape(-1, 3)[rows]
    ori = np.ascontiguousarray(model["orientations"], f32).reshape(-1, 9)[rows]
    dims = np.ascontiguousarray(model["dims"], f32).reshape(-1, 2)[rows]
    res, s = f32(q["res"]), f32(q["splat_scale"] if q["splat_scale"] != 0 else 2.0)
    step = res * f32(0.5)
    zmin, zmax, fmax, fcos = f32(q["z_min"]), f32(q["z_max"]), f32(q["floor_max"]), f32(q["floor_cos"])
    fW, fH = f32(q["width"]), f32(q["height"])
    with np.errstate(all="ignore"):
        d = [pos[:, k] - t[k] for k in range(3)]

        def rt(v):        # R^T v: (R0j v.x + R1j v.y) + R2j v.z
            return [(R[0, j] * v[0] + R[1, j] * v[1]) + R[2, j] * v[2] for j in range(3)]
        C = rt(d)
        E1 = rt([ori[:, 0], ori[:, 1], ori[:, 2]])
        E2 = rt([ori[:, 3], ori[:, 4], ori[:, 5]])
        Nz = rt([ori[:, 6], ori[:, 7], ori[:, 8]])[2]
        h1, h2 = s * np.sqrt(dims[:, 0]), s * np.sqrt(dims[:, 1])
        assert h1.dtype == np.float32 and C[0].dtype == np.float32
    n1, n2 = _steps(h1, step, q["max_steps"]), _steps(h2, step, q["max_steps"])
    key = n1 * 64 + n2
    for k in np.unique(key):
        m1, m2 = int(k) // 64, int(k) % 64
        li, lj = lattice(m1, m2)
        grp = np.flatnonzero(key == k)
        per = max(1, chunk // len(li))
        with np.errstate(all="ignore"):
            ra = (li.astype(f32) / f32(m1))[None, :]
            rb = (lj.astype(f32) / f32(m2))[None, :]
            for g0 in range(0, len(grp), per):
                g = grp[g0:g0 + per]
                a, b = ra * h1[g, None], rb * h2[g, None]
                S = [(C[c][g, None] + a * E1[c][g, None]) + b * E2[c][g, None] for c in range(3)]
                gx, gy, z = S[0] / res, S[1] / res, S[2]
                assert gx.dtype == np.float32 and z.dtype == np.float32
                in_grid = (gx >= 0) & (gx < fW) & (gy >= 0) & (gy < fH)
                acc = in_grid & (z >= zmin) & (z <= zmax)
                obst = acc & (z > fmax)
                floor = acc & (z <= fmax) & (np.abs(Nz[g, None]) >= fcos)
                shape = gx.shape
                yield dict(row=np.broadcast_to(rows[g, None], shape).ravel(), i=np.broadcast_to(li[None, :], shape).ravel(),
                           j=np.broadcast_to(lj[None, :], shape).ravel(), gx=gx.ravel(), gy=gy.ravel(), z=z.ravel(),
                           in_grid=in_grid.ravel(), accepted=acc.ravel(), obstacle=obst.ravel(), floor=floor.ravel())


def all_samples(model, n_visible, pose, q):
    """samples() as one dict, sorted by (row, i, j)"""
    parts = list(samples(model, n_visible, pose, q))
    if not parts:
        return None
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    order = np.lexsort((out["j"], out["i"], out["row"]))
    return {k: v[order] for k, v in out.items()}


def states(hits, min_hits):
    """step 7"""
    return np.where(hits[..., 1] >= min_hits, 100, np.where(hits[..., 0] >= min_hits, 0, -1)).astype(np.int8)


def clearance(state, R, unknown_is_obstacle):
    """step 8 by the two separable passes: per column the distance along y to the nearest obstacle cell capped at R + 1 (a sweep
    up, a sweep down), then per row the minimum over |dx| <= R of g^2 + dx^2, capped at R^2.  Integers."""
    H, W = state.shape
    obst = (state == 100) | ((state < 0) if unknown_is_obstacle else False)
    g = np.empty((H, W), np.int64)
    d = np.full(W, R + 1, np.int64)
    for y in range(H):
        d = np.where(obst[y], 0, np.minimum(d + 1, R + 1))
        g[y] = d
    d = np.full(W, R + 1, np.int64)
    for y in range(H - 1, -1, -1):
        d = np.where(obst[y], 0, np.minimum(d + 1, R + 1))
        g[y] = np.minimum(g[y], d)
    g2 = g * g
    best = np.full((H, W), R * R, np.int64)
    for dx in range(-min(R, W - 1), min(R, W - 1) + 1):
        lo, hi = max(0, -dx), min(W, W - dx)                        # cells x with 0 <= x + dx < W
        best[:, lo:hi] = np.minimum(best[:, lo:hi], g2[:, lo + dx:hi + dx] + dx * dx)
    return best.astype(np.int32)


def clearance_brute(state, R, unknown_is_obstacle):
    """step 8 as written: the minimum over ALL obstacle cells, capped"""
    H, W = state.shape
    obst = (state == 100) | ((state < 0) if unknown_is_obstacle else False)
    oy, ox = np.nonzero(obst)
    out = np.full((H, W), R * R, np.int64)
    for y in range(H):
        for x in range(W):
            if len(ox):
                out[y, x] = min(R * R, int(((ox - x) ** 2 + (oy - y) ** 2).min()))
    return out.astype(np.int32)


def build(model, n_visible, pose, q):
    """dict(zmin, zmax, hits, state, dist2, stats) of the grid q in frame `pose` (12 floats; default_pose() for the default)"""
    W, H = int(q["width"]), int(q["height"])
    zlo, zhi = np.full(W * H, np.inf, f32), np.full(W * H, -np.inf, f32)
    hits = np.zeros((W * H, 2), np.uint32)
    n_samples = n_acc = 0
    for p in samples(model, n_visible, pose, q):
        n_samples += len(p["z"])
        a = p["accepted"]
        n_acc += int(a.sum())
        cell = p["gy"][a].astype(np.int64) * W + p["gx"][a].astype(np.int64)     # (int)gx: truncation of a non-negative float
        z = p["z"][a] + f32(0.0)                                                 # -0 counts as +0
        np.minimum.at(zlo, cell, z)
        np.maximum.at(zhi, cell, z)
        np.add.at(hits[:, 0], cell[p["floor"][a]], 1)
        np.add.at(hits[:, 1], cell[p["obstacle"][a]], 1)
    hits = hits.reshape(H, W, 2)
    state = states(hits, int(q["min_hits"]))
    stats = dict(rows_used=len(used_rows(model, n_visible, q)), samples=n_samples, samples_in_grid=n_acc,
                 cells_free=int((state == 0).sum()), cells_occupied=int((state == 100).sum()), cells_unknown=int((state < 0).sum()))
    return dict(zmin=zlo.reshape(H, W), zmax=zhi.reshape(H, W), hits=hits, state=state,
                dist2=clearance(state, int(q["max_dist_cells"]), bool(q["unknown_is_obstacle"])), stats=stats)


def samples_f64(model, n_visible, pose, q):
    """The sampling and banding in f64 with matrix products.  Returns a dict as all_samples() (sorted by (row, i, j)) with gx, gy, z in
    f64 plus `uncertain`: the sample is within GUARD_CELLS of a cell edge or the grid's border, within GUARD_M of a band limit it is
    compared against, its row's |N.z| within GUARD_M of floor_cos where that matters, or its row's h / step within GUARD_CELLS of an
    integer (the lattice itself could differ).  Rows whose lattice size differs from the f32 one are reported in `bad_rows`."""
    pose = np.asarray(pose, f32).ravel().astype(np.float64)
    R, t = pose[:9].reshape(3, 3), pose[9:]
    rows = used_rows(model, n_visible, q)
    pos = np.asarray(model["positions"], f32).reshape(-1, 3)[rows].astype(np.float64)
    ori = np.asarray(model["orientations"], f32).reshape(-1, 3, 3)[rows].astype(np.float64)
    dims = np.asarray(model["dims"], f32).reshape(-1, 2)[rows].astype(np.float64)
    res = np.float64(f32(q["res"]))
    s = np.float64(f32(q["splat_scale"] if q["splat_scale"] != 0 else 2.0))
    zmin, zmax, fmax, fcos = (np.float64(f32(q[k])) for k in ("z_min", "z_max", "floor_max", "floor_cos"))
    W, H, ms = int(q["width"]), int(q["height"]), int(q["max_steps"])
    C = (pos - t) @ R
    E = ori @ R                                                   # rows e1, e2, n in the grid frame
    h = s * np.sqrt(dims)
    qn = h / (0.5 * res)
    n = np.clip(np.ceil(qn), 1, ms).astype(np.int64)
    row_unc = ((np.abs(qn - np.rint(qn)) < GUARD_CELLS) & (qn < ms + 1)).any(axis=1)
    out = {k: [] for k in ("row", "i", "j", "gx", "gy", "z", "in_grid", "accepted", "obstacle", "floor", "uncertain")}
    for r in range(len(rows)):
        li, lj = lattice(int(n[r, 0]), int(n[r, 1]))
        a, b = li / n[r, 0] * h[r, 0], lj / n[r, 1] * h[r, 1]
        S = C[r][None, :] + a[:, None] * E[r, 0][None, :] + b[:, None] * E[r, 1][None, :]
        gx, gy, z = S[:, 0] / res, S[:, 1] / res, S[:, 2]
        in_grid = (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H)
        acc = in_grid & (z >= zmin) & (z <= zmax)
        nz = abs(E[r, 2, 2])
        obst = acc & (z > fmax)
        floor = acc & (z <= fmax) & (nz >= fcos)
        unc = (np.abs(gx - np.rint(gx)) < GUARD_CELLS) | (np.abs(gy - np.rint(gy)) < GUARD_CELLS)
        unc |= (np.abs(z - zmin) < GUARD_M) | (np.abs(z - zmax) < GUARD_M) | (np.abs(z - fmax) < GUARD_M)
        unc |= (z <= fmax + GUARD_M) & (abs(nz - fcos) < GUARD_M)
        unc |= bool(row_unc[r])
        for k, v in (("row", np.full(len(li), rows[r])), ("i", li), ("j", lj), ("gx", gx), ("gy", gy), ("z", z), ("in_grid", in_grid),
                     ("accepted", acc), ("obstacle", obst), ("floor", floor), ("uncertain", unc)):
            out[k].append(v)
    out = {k: np.concatenate(v) if v else np.zeros(0) for k, v in out.items()}
    order = np.lexsort((out["j"], out["i"], out["row"]))
    return {k: v[order] for k, v in out.items()}


# ---- the hand-built models, grids and poses of the tests ----------------------------------------------------------------
SIZES = ((1, 1), (255, 0), (257, 256), (1300, 513))              # (n, n_visible): wave and block edges of both stores
SEEDS = (0, 1, 2)
GRIDS = ((1, 1, 0.5), (7, 5, 0.2), (32, 32, 0.05), (33, 31, 0.05), (65, 64, 0.05))      # (width, height, res): one tile, tile edges, partial tiles
MIN_CONF = 2.0


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def pose_about(R, t):
    return np.concatenate([np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64)]).astype(f32)


def caller_pose(q):
    """a grid frame of the caller's: the floor frame turned 30 degrees about the vertical, with the model's middle near the grid's"""
    R = FLOOR_R.reshape(3, 3).astype(np.float64) @ rot("z", 30.0)
    half = 0.5 * np.array([q["width"] * q["res"], q["height"] * q["res"], 0.0])
    return pose_about(R, np.array([0.07, 0.11, -0.05]) - R @ half)


def hand_model(n, seed, extent=1.8):
    """n rows: positions uniform in a box about the origin (map frame: y down, heights -0.8..1.8 m below the origin), a third of
    the discs near-horizontal, a third near-vertical, a third at random attitudes; half-axes of 2 to 20 cm; confidences uniform
    about MIN_CONF; stamps spread over 0..100.  Row 0 is fixed: a horizontal disc at the origin, 1 m below it, that every grid of
    the tests contains."""
    rng = np.random.default_rng(104729 * seed + n)
    pos = np.stack([rng.uniform(-extent, extent, n), rng.uniform(-0.8, 1.8, n), rng.uniform(-extent, extent, n)], axis=1)
    pos[0::3, 1] = 1.0 + rng.normal(0, 0.03, len(pos[0::3]))       # the near-horizontal third: a floor 1 m below the origin
    ori = np.empty((n, 3, 3))
    for k in range(n):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if k % 3 == 0:      # near-horizontal: normal close to map y
            Q = rot("x", rng.normal(0, 8)) @ rot("z", rng.normal(0, 8)) @ np.array([[1.0, 0, 0], [0, 0, 1], [0, -1, 0]]) @ rot("z", rng.uniform(0, 360))
            Q = Q.T
        elif k % 3 == 1:    # near-vertical: normal horizontal
            Q = (rot("y", rng.uniform(0, 360)) @ rot("z", rng.normal(0, 5))).T
        ori[k] = Q
    m = dict(positions=pos, colors=rng.uniform(0.0, 255.0, (n, 3)), orientations=ori.reshape(n, 9),
             shapes=rng.uniform(-1e-3, 1e-3, (n, 6)), dims=rng.uniform(1e-4, 1e-2, (n, 2)), confidences=rng.uniform(0.0, 2.0 * MIN_CONF, n))
    t0 = rng.integers(0, 101, n)
    m["stamps"] = np.stack([t0, t0 + (rng.integers(0, 101, n) * (100 - t0)) // 100], axis=1)
    m = {name: np.ascontiguousarray(m[name], dt) for name, _, dt in FIELDS}
    m["positions"][0] = (0.01, 1.0, 0.02)
    m["orientations"][0] = (1, 0, 0, 0, 0, 1, 0, -1, 0)
    m["dims"][0] = (4e-3, 9e-3)
    m["confidences"][0] = 1.5 * MIN_CONF
    m["stamps"][0] = (40, 60)
    return m


def grid_cases(width, height, res):
    """[(name, 'caller' or None, keywords)]: the default rule, a stricter gate with both stamp ranges, visible rows with the unknown
    cells as obstacles, and coarse lattices with a higher hit count -- each in the caller's frame and in the default one"""
    base = dict(width=width, height=height, res=res)
    kinds = [("plain", dict()),
             ("gated", dict(min_conf=MIN_CONF, t_init=(10, 90), t_last=(20, 100), max_dist_cells=3)),
             ("visible", dict(visible_only=True, unknown_is_obstacle=True, max_dist_cells=7, floor_cos=0.95)),
             ("coarse", dict(max_steps=2, min_hits=2, splat_scale=3.0, z_min=-1.2, z_max=0.1, floor_max=-0.9, max_dist_cells=1))]
    return [("%s %s" % (name, frame or "default"), frame, dict(base, **kw)) for name, kw in kinds for frame in ("caller", None)]


def boundary_rows():
    """Rows whose samples sit EXACTLY on a boundary of the rule, in the frame BOUNDARY_POSE (grid = map), with the answers written by
    hand.  res = 0.25, an 8 x 4 grid, s = 2, bands z_min -1, floor_max 0, z_max 1, floor_cos 0.5, max_steps 8: every value is a
    small dyadic rational, so every f32 operation of the rule is exact.  A disc with dims 2^-8 has half-axis 2 / 16 = 0.125 = step:
    n = 1, five samples (the centre and +-0.125 along each axis).  Returns (model, keywords, [(name, rows, expectations)]) where
    expectations maps 'hits' to {(ix, iy): (floor, obstacle)}, 'zmin' / 'zmax' to {(ix, iy): value} and the stats by name; every
    case is evaluated on its rows ALONE."""
    X, Y, Zp = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    d = 2.0 ** -8
    rows = [
        # 0: centre (0.625, 0.375): the sample at x - 0.125 = 0.5 has gx = 2 exactly: cell 2, not 1; y - 0.125 = 0.25: gy = 1: cell 1;
        #    y + 0.125 = 0.5: gy = 2: cell 2.  z = -0.5: floor
        ((0.625, 0.375, -0.5), X, Y, Zp, (d, d)),
        # 1: centre (1.875, 0.625): the sample at x + 0.125 = 2.0 has gx = 8 = W: outside.  The other four are in (7, 2), y - 0.125 = 0.5
        #    and y + 0.125 = 0.75: gy = 2 and 3
        ((1.875, 0.625, -0.5), X, Y, Zp, (d, d)),
        # 2: z == floor_max = 0: floor samples (z <= floor_max)
        ((1.125, 0.125, 0.0), X, Y, Zp, (d, d)),
        # 3: z == z_min = -1: accepted        4: z == z_max = 1: accepted, an obstacle       5: z just below z_min: ignored
        ((0.125, 0.875, -1.0), X, Y, Zp, (d, d)),
        ((0.375, 0.875, 1.0), X, Y, Zp, (d, d)),
        ((0.625, 0.875, -1.0000001), X, Y, Zp, (d, d)),
        # 6: |N.z| == floor_cos = 0.5: floor samples      7: |N.z| one ulp below: heights only
        ((1.125, 0.875, -0.5), X, Y, (0, 0, -0.5), (d, d)),
        ((1.375, 0.875, -0.5), X, Y, (0, 0, 0.49999997), (d, d)),
        # 8: a wall: e1 = x, e2 = z with dims.y = 2^-4: h2 = 0.5, n2 = 4, b = j / 8; centre (0.375, 0.125, 0.25).  The lattice is
        #    i = 0: j = -4..4, i = +-1: j = 0.  Samples: x = 0.375: z = -0.25 .. 0.75 (9 samples: 3 with z <= 0, 6 above); x = 0.25 and
        #    0.5 at z = 0.25.  All at gy = 0.5: a line of cells, (1, 0) for x = 0.25 and 0.375, (2, 0) for x = 0.5
        ((0.375, 0.125, 0.25), X, Zp, Y, (d, 2.0 ** -4)),
        # 9: clipped by max_steps = 8: dims.x = 4: h1 = 4, q = 32 -> n1 = 8, a = i / 2; centre (0.0625, 0.375): x = 0.0625 + i / 2 for
        #    i = 0..3 are in the grid (gx = 0.25, 2.25, 4.25, 6.25), i = 4 gives 2.0625: gx = 8.25: outside; negative i: outside.  j: +-1
        #    only at i = 0.  Cells 0, 2, 4, 6 of row 1: holes between them
        ((0.0625, 0.375, 0.5), X, Y, Zp, (4.0, d)),
        # 10: -0 heights: C.z = -0 and E1.z = E2.z = -0 (BOUNDARY_POSE): a * E1.z is -0 for i >= 0 and +0 for i < 0, so the samples
        #     with i >= 0 and j >= 0 have z = -0 + -0 + -0 = -0, the others +0
        ((1.625, 0.125, -0.0), (1, 0, -0.0), (0, 1, -0.0), Zp, (d, d)),
    ]
    n = len(rows)
    rng = np.random.default_rng(11)
    m = dict(positions=np.array([r[0] for r in rows]), colors=rng.uniform(0, 255, (n, 3)), stamps=np.tile([50, 60], (n, 1)),
             orientations=np.array([r[1] + r[2] + r[3] for r in rows]), shapes=rng.uniform(-1e-3, 1e-3, (n, 6)),
             dims=np.array([r[4] for r in rows]), confidences=np.full(n, 9.0))
    m = {name: np.ascontiguousarray(m[name], dt) for name, _, dt in FIELDS}
    kw = dict(width=8, height=4, res=0.25, z_min=-1.0, z_max=1.0, floor_max=0.0, floor_cos=0.5, max_steps=8, max_dist_cells=3)
    cases = [
        ("a sample on a cell edge", [0], dict(hits={(2, 1): (3, 0), (3, 1): (1, 0), (2, 2): (1, 0)}, samples=5, samples_in_grid=5,
                                              zmin={(2, 1): -0.5}, zmax={(2, 2): -0.5})),
        ("a sample at gx == W", [1], dict(hits={(7, 2): (3, 0), (7, 3): (1, 0)}, samples=5, samples_in_grid=4)),
        # x - 0.125 = 1.0: gx = 4; x + 0.125: gx = 5; y - 0.125 = 0: gy = 0; y + 0.125 = 0.25: gy = 1
        ("z == floor_max", [2], dict(hits={(4, 0): (3, 0), (5, 0): (1, 0), (4, 1): (1, 0)}, samples_in_grid=5, zmax={(4, 0): 0.0})),
        # rows 3 to 7 sit at y = 0.875: the sample at y + 0.125 = 1.0 has gy = 4 = H: outside
        ("z == z_min", [3], dict(hits={(0, 3): (3, 0), (1, 3): (1, 0)}, samples_in_grid=4, zmin={(0, 3): -1.0})),
        ("z == z_max", [4], dict(hits={(1, 3): (0, 3), (2, 3): (0, 1)}, samples_in_grid=4, zmax={(1, 3): 1.0})),
        ("z below z_min", [5], dict(hits={}, samples=5, samples_in_grid=0)),
        ("|N.z| == floor_cos", [6], dict(hits={(4, 3): (3, 0), (5, 3): (1, 0)}, samples_in_grid=4)),
        ("|N.z| below floor_cos", [7], dict(hits={}, samples_in_grid=4, zmin={(5, 3): -0.5, (6, 3): -0.5}, zmax={(5, 3): -0.5})),
        # the wall's normal is horizontal (N.z = 0 < floor_cos): its three samples with z <= 0 are no floor samples
        ("a wall", [8], dict(hits={(1, 0): (0, 7), (2, 0): (0, 1)}, samples=11, samples_in_grid=11,
                             zmin={(1, 0): -0.25, (2, 0): 0.25}, zmax={(1, 0): 0.75, (2, 0): 0.25})),
        # at i = 0 the samples j = +-1 are at y = 0.25 and 0.5: gy = 1 and 2
        ("n clipped by max_steps", [9], dict(hits={(0, 1): (0, 2), (0, 2): (0, 1), (2, 1): (0, 1), (4, 1): (0, 1), (6, 1): (0, 1)},
                                             samples=19, samples_in_grid=6)),
        # x = 1.5, 1.625, 1.75: gx = 6, 6.5, 7; y = 0, 0.125, 0.25: gy = 0, 0.5, 1
        ("-0 heights", [10], dict(hits={(6, 0): (3, 0), (7, 0): (1, 0), (6, 1): (1, 0)}, samples_in_grid=5,
                                  zmin={(6, 0): 0.0, (7, 0): 0.0, (6, 1): 0.0}, zmax={(6, 0): 0.0, (7, 0): 0.0, (6, 1): 0.0})),
    ]
    return m, kw, cases


def check_expectations(got, want, W, H, what):
    """a grid (build()'s or the device's dict) against one case of boundary_rows()"""
    hits = np.zeros((H, W, 2), np.uint32)
    for (ix, iy), v in want.get("hits", {}).items():
        hits[iy, ix] = v
    assert np.array_equal(got["hits"], hits), (what, np.argwhere(got["hits"] != hits).tolist(), got["hits"][got["hits"].any(axis=2)].tolist())
    for key in ("zmin", "zmax"):
        for (ix, iy), v in want.get(key, {}).items():
            assert got[key][iy, ix].view(np.uint32) == f32(v).view(np.uint32), (what, key, ix, iy, got[key][iy, ix], v)
    for key in ("samples", "samples_in_grid"):
        if key in want:
            assert got["stats"][key] == want[key], (what, key, got["stats"][key], want[key])
