"""The numpy restatement of ssf_raycast (include/ssf_raycast.h): every step one IEEE f32 operation in the header's order, on
np.float32 arrays (no einsum, no dot), as a brute force over rays x rows WITHOUT any index.  cast() is what the GPU tests compare
against at 0 bits; oversize() restates the header's oversize rule (rows_oversize is exact).

cast_f64() is an independent formulation in f64 with matrix products that also reports, per ray, whether one of its margins is
within GUARD (relative) -- tests/test_raycast.py compares the two outside those rays.

Also here: the hand-built scenes and the boundary-exact rows that tests/test_raycast.py and tests/test_raycast_gpu.py share."""
import numpy as np

import navgrid_ref as nr

f32 = np.float32
FIELDS = nr.FIELDS
IDENTITY = nr.IDENTITY
OUTPUTS = ("t", "index", "point", "normal", "color")
STATS = ("rays", "rays_hit", "rays_invalid", "rows_indexed", "rows_oversize")
# range_min / range_max stand for cfg.range_min / cfg.range_max (t_min = t_max = 0): util.make_cfg's handles have the library's 0.2 / 5.0
DEFAULTS = dict(t_min=0.0, t_max=0.0, min_conf=0.0, splat_scale=0.0, visible_only=False, cell=0.0, hash_bits=0, range_min=0.2, range_max=5.0)
DEFAULT_SPLAT, DEFAULT_CELL = 3.0, 0.125
GUARD = 1e-4
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def params(**kw):
    """a call as cast() takes it: the keywords of Fusion.raycast (without rays, pose and outputs) with the defaults resolved"""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    q = dict(DEFAULTS, **kw)
    if q["t_min"] == 0 and q["t_max"] == 0:
        q["t_min"], q["t_max"] = q["range_min"], q["range_max"]
    q["splat_scale"] = q["splat_scale"] if q["splat_scale"] != 0 else DEFAULT_SPLAT
    q["cell"] = q["cell"] if q["cell"] != 0 else DEFAULT_CELL
    return q


def _model(model):
    g = lambda name, k: np.ascontiguousarray(model[name], f32).reshape(-1, k)
    return g("positions", 3), g("orientations", 9), g("dims", 2), g("confidences", 1)[:, 0], g("colors", 3)


def indexed_rows(model):
    """the position and dims part of step 5 (rows_indexed counts these)"""
    pos, _, dims, _, _ = _model(model)
    with np.errstate(invalid="ignore"):
        return np.isfinite(pos).all(axis=1) & (dims[:, 0] > 0) & (dims[:, 1] > 0) & np.isfinite(dims).all(axis=1)


def used_rows(model, n_visible, q):
    """step 5: the rows that take part"""
    _, _, _, conf, _ = _model(model)
    ok = indexed_rows(model) & (conf > f32(q["min_conf"]))
    if q["visible_only"]:
        ok &= np.arange(len(conf)) < int(n_visible)
    return np.flatnonzero(ok)


def oversize(model, q):
    """the header's oversize rule, a to d, in f32: a boolean per row (meaningful for indexed_rows() only)"""
    pos, ori, dims, _, _ = _model(model)
    s, cell = f32(q["splat_scale"]), f32(q["cell"])
    T = f32(2.0 ** -7)
    e1, e2, n = ori[:, 0:3], ori[:, 3:6], ori[:, 6:9]
    dot = lambda u, v: (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
    with np.errstate(all="ignore"):
        over = (dims[:, 0] < f32(2.0 ** -40)) | (dims[:, 1] < f32(2.0 ** -40))
        ortho = (np.abs(dot(e1, e1) - f32(1)) <= T) & (np.abs(dot(e2, e2) - f32(1)) <= T) & (np.abs(dot(n, n) - f32(1)) <= T) & \
                (np.abs(dot(e1, e2)) <= T) & (np.abs(dot(e1, n)) <= T) & (np.abs(dot(e2, n)) <= T)
        over |= ~ortho
        h1, h2 = s * np.sqrt(dims[:, 0]), s * np.sqrt(dims[:, 1])
        hs = h1 + h2
        cells = np.ones(len(pos), np.float64)
        for j in range(3):
            E = ((np.abs(e1[:, j]) * h1 + np.abs(e2[:, j]) * h2) * f32(1.0625) + hs * f32(0.03125)) + \
                (np.abs(pos[:, j]) * f32(2.0 ** -20) + cell * f32(2.0 ** -10))
            glo, ghi = (pos[:, j] - E) / cell, (pos[:, j] + E) / cell
            assert glo.dtype == np.float32
            inside = (glo >= f32(-32000)) & (ghi <= f32(32000))
            over |= ~inside
            cells *= np.where(inside, np.floor(ghi).astype(np.float64) - np.floor(glo).astype(np.float64) + 1, 1)
        over |= cells > 64
    return over


def transform(rays, pose):
    """step 1: (O, D) as lists of three f32 arrays, and the valid rays"""
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 6)
    pose = np.asarray(pose, f32).ravel()
    R, t0 = pose[:9].reshape(3, 3), pose[9:]
    o, d = rays[:, 0:3], rays[:, 3:6]
    with np.errstate(all="ignore"):
        O = [((R[i, 0] * o[:, 0] + R[i, 1] * o[:, 1]) + R[i, 2] * o[:, 2]) + t0[i] for i in range(3)]
        D = [(R[i, 0] * d[:, 0] + R[i, 1] * d[:, 1]) + R[i, 2] * d[:, 2] for i in range(3)]
    valid = np.isfinite(rays).all(axis=1) & ~((D[0] == 0) & (D[1] == 0) & (D[2] == 0))
    assert O[0].dtype == np.float32 and D[0].dtype == np.float32
    return O, D, valid


def cast(model, n_visible, rays, pose, q, chunk=512, detail=False):
    """dict(t, index, point, normal, color, stats) of the rays (n x 6) in frame `pose` (12 floats) against the model.  detail: also
    'candidates' (accepted rows per ray)"""
    pos, ori, dims, conf, col = _model(model)
    rows = used_rows(model, n_visible, q)
    O, D, valid = transform(rays, pose)
    n = len(valid)
    tmin, tmax, s = f32(q["t_min"]), f32(q["t_max"]), f32(q["splat_scale"])
    k = s * s
    c, e1, e2, nn, dm = pos[rows], ori[rows, 0:3], ori[rows, 3:6], ori[rows, 6:9], dims[rows]
    rhs = ((k * dm[:, 0]) * dm[:, 1])[None, :]
    key = np.full(n, NO_KEY, np.uint64)
    ncand = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for r0 in range(0, n, chunk):
            sl = slice(r0, min(n, r0 + chunk))
            Ox, Oy, Oz = (O[i][sl, None] for i in range(3))
            Dx, Dy, Dz = (D[i][sl, None] for i in range(3))
            den = (nn[None, :, 0] * Dx + nn[None, :, 1] * Dy) + nn[None, :, 2] * Dz
            wx, wy, wz = c[None, :, 0] - Ox, c[None, :, 1] - Oy, c[None, :, 2] - Oz
            num = (nn[None, :, 0] * wx + nn[None, :, 1] * wy) + nn[None, :, 2] * wz
            tt = num / den
            assert tt.dtype == np.float32
            cand = (den != 0) & np.isfinite(tt) & (tt >= tmin) & (tt <= tmax)
            Px, Py, Pz = Ox + tt * Dx, Oy + tt * Dy, Oz + tt * Dz
            Vx, Vy, Vz = Px - c[None, :, 0], Py - c[None, :, 1], Pz - c[None, :, 2]
            a = (Vx * e1[None, :, 0] + Vy * e1[None, :, 1]) + Vz * e1[None, :, 2]
            b = (Vx * e2[None, :, 0] + Vy * e2[None, :, 1]) + Vz * e2[None, :, 2]
            inside = (a * a) * dm[None, :, 1] + (b * b) * dm[None, :, 0] <= rhs
            ok = cand & inside & valid[sl, None]
            kk = (tt.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows[None, :].astype(np.uint64)
            kk = np.where(ok, kk, NO_KEY)
            if len(rows):
                key[sl] = kk.min(axis=1)
            ncand[sl] = ok.sum(axis=1)
    hit = key != NO_KEY
    idx = np.where(hit, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    t = np.where(hit, (key >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(f32)
    w = np.where(hit, idx, 0)
    with np.errstate(all="ignore"):
        point = np.stack([np.where(hit, O[i] + t * D[i], f32(0)) for i in range(3)], axis=1).astype(f32)
        nw = ori[w, 6:9] if len(ori) else np.zeros((n, 3), f32)
        den = (nw[:, 0] * D[0] + nw[:, 1] * D[1]) + nw[:, 2] * D[2]
        normal = np.where(hit[:, None], np.where((den > 0)[:, None], -nw, nw), f32(0)).astype(f32)
    color = np.where(hit[:, None], col[w] if len(col) else np.zeros((n, 3), f32), f32(0)).astype(f32)
    ind = indexed_rows(model)
    stats = dict(rays=n, rays_hit=int(hit.sum()), rays_invalid=int((~valid).sum()), rows_indexed=int(ind.sum()),
                 rows_oversize=int((oversize(model, q) & ind).sum()))
    out = dict(t=t, index=idx.astype(np.int32), point=point, normal=normal, color=color, stats=stats)
    if detail:
        out["candidates"] = ncand
    return out


def cast_f64(model, n_visible, rays, pose, q):
    """The rule in f64 with matrix products.  Returns dict(t, index, uncertain, face): `uncertain` marks the rays one of whose f64
    margins is within GUARD (relative): the inside test's slack or tt against the range ends for a row that could decide the ray, or
    the gap between the best and the second tt.  face: +1 when the winner is hit on its n side (den < 0), -1 from behind, 0 a miss; cos: |cos| of the angle between D and the winner's normal."""
    pos, ori, dims, conf, _ = _model(model)
    rows = used_rows(model, n_visible, q)
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 6).astype(np.float64)
    pose = np.asarray(pose, f32).ravel().astype(np.float64)
    R, t0 = pose[:9].reshape(3, 3), pose[9:]
    with np.errstate(all="ignore"):
        O, D = rays[:, :3] @ R.T + t0, rays[:, 3:] @ R.T
        valid = np.isfinite(rays).all(axis=1) & (D != 0).any(axis=1)
        c, E, dm = pos[rows].astype(np.float64), ori[rows].astype(np.float64).reshape(-1, 3, 3), dims[rows].astype(np.float64)
        tmin, tmax, s = (np.float64(f32(q[k])) for k in ("t_min", "t_max", "splat_scale"))
        den = D @ E[:, 2].T
        num = ((c[None] - O[:, None]) * E[None, :, 2]).sum(axis=2)
        tt = num / den
        P = O[:, None] + tt[..., None] * D[:, None]
        V = P - c[None]
        a, b = (V * E[None, :, 0]).sum(axis=2), (V * E[None, :, 1]).sum(axis=2)
        lhs, rhs = a * a * dm[None, :, 1] + b * b * dm[None, :, 0], (s * s * dm[:, 0] * dm[:, 1])[None]
        fin = (den != 0) & np.isfinite(tt) & valid[:, None]
        loose = fin & (tt >= tmin * (1 - GUARD)) & (tt <= tmax * (1 + GUARD)) & (lhs <= rhs * (1 + GUARD))
        sure = fin & (tt >= tmin * (1 + GUARD)) & (tt <= tmax * (1 - GUARD)) & (lhs <= rhs * (1 - GUARD))
        acc = fin & (tt >= tmin) & (tt <= tmax) & (lhs <= rhs)
    n = len(rays)
    big = np.where(acc, tt, np.inf)
    if len(rows):
        j = big.argmin(axis=1)
        best = big[np.arange(n), j]
        second = np.partition(big, 1, axis=1)[:, 1] if len(rows) > 1 else np.full(n, np.inf)
        amb = (loose & ~sure & (tt <= (best * (1 + GUARD))[:, None])).any(axis=1)
        with np.errstate(invalid="ignore"):
            amb |= np.isfinite(second) & (second - best <= GUARD * best)
    else:
        j, best, amb = np.zeros(n, np.int64), np.full(n, np.inf), np.zeros(n, bool)
    hit = np.isfinite(best)
    face = np.where(hit, np.where(den[np.arange(n), j] < 0, 1, -1), 0) if len(rows) else np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        cos = np.abs(den[np.arange(n), j]) / (np.linalg.norm(D, axis=1) * np.linalg.norm(E[j, 2], axis=1)) if len(rows) else np.ones(n)
    return dict(t=np.where(hit, best, 0.0), index=np.where(hit, rows[j] if len(rows) else 0, -1), uncertain=amb, face=face, cos=cos)


# ---- the hand-built scenes of the tests -----------------------------------------------------------------------------------
SIZES = ((1, 1), (63, 63), (64, 0), (65, 64), (255, 0), (256, 256), (257, 256), (513, 257), (1300, 513))     # (n, n_visible)
RAY_COUNTS = (0, 1, 63, 64, 65, 257, 1025)
SCENE_RANGE = dict(t_min=0.05, t_max=8.0)
AIM = 1.4
FAR = 1.0e5                                       # beyond the coordinate bound of the default cell (32000 * 0.125 m)


def hand_model(n, seed):
    """navgrid_ref.hand_model's rows (a box of 3.6 m; dims quartered: discs of 1.5 to 15 cm at s = 3) changed so that a cast meets every
    case: every fortieth row is a copy of the row before it (coincident discs: exact ties in tt), rows 7, 107, ... are 0.6 to 1.2 m across
    (oversize by their box), rows 17, 117, ... sit FAR away (oversize by the coordinate bound), rows 27, 127, ... have a sheared
    e1 (oversize: not orthonormal)."""
    m = nr.hand_model(n, seed)
    rng = np.random.default_rng(7919 * seed + n)
    m["dims"] *= f32(0.25)
    for k in range(39, n, 40):
        for name in ("positions", "orientations", "dims"):
            m[name][k] = m[name][k - 1]
    for k in range(7, n, 100):
        m["dims"][k] = rng.uniform(0.01, 0.04, 2)
    for k in range(17, n, 100):
        m["positions"][k] = (FAR + 0.01 * k, 0.5, -0.25)
        m["orientations"][k] = (0, 1, 0, 0, 0, 1, 1, 0, 0)                 # faces -x / +x
        m["dims"][k] = (0.01, 0.01)
    for k in range(27, n, 100):
        m["orientations"][k, 0:3] += m["orientations"][k, 3:6] * f32(0.25)
    return m


def scene_rays(model, nr_rays, seed):
    """nr_rays x 6 in the ray frame scene_pose(seed), described here in the map frame: from four sensor positions inside the box (each ray's origin jittered), three eighths of them aimed at a point on or near
    a row's disc (up to AIM half-axes from its centre: in and out), three eighths random unit directions, an eighth non-unit, and an
    eighth along the +x axis towards the FAR rows"""
    rng = np.random.default_rng(31337 * seed + nr_rays + len(model["confidences"]))
    pos, ori, dims, _, _ = _model(model)
    n = len(pos)
    sensors = np.array([[0.0, 0.3, 0.0], [1.1, -0.2, -0.9], [-1.3, 0.9, 1.2], [0.2, 1.5, 0.4]])
    o = sensors[rng.integers(0, 4, nr_rays)] + rng.normal(0, 0.05, (nr_rays, 3))
    d = rng.normal(size=(nr_rays, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kind = rng.integers(0, 8, nr_rays)
    near = np.flatnonzero(np.abs(pos[:, 0]) < 1e3) if n else np.zeros(0, np.int64)
    for r in range(nr_rays):
        if kind[r] < 3 and len(near):
            k = near[rng.integers(0, len(near))]
            u, v = rng.uniform(-AIM, AIM, 2) * 3.0 * np.sqrt(dims[k].astype(np.float64))
            target = pos[k] + u * ori[k, 0:3] + v * ori[k, 3:6]
            d[r] = target - o[r]
            d[r] /= np.linalg.norm(d[r])
        elif kind[r] == 6:
            d[r] *= rng.uniform(0.25, 4.0)
        elif kind[r] == 7:
            o[r] = (FAR - 3.0, 0.5 + rng.uniform(-0.15, 0.15), -0.25 + rng.uniform(-0.15, 0.15))   # (well inside the rim: f32 has 8 mm there)
            d[r] = (1.0, 0.0, 0.0)
    # (o, d) are in the map frame: into the ray frame of scene_pose(seed)
    pose = scene_pose(seed).astype(np.float64)
    R, t0 = pose[:9].reshape(3, 3), pose[9:]
    return np.concatenate([(o - t0) @ R, d @ R], axis=1).astype(f32)


def scene_pose(seed):
    """a ray frame of the caller's: turned about two axes, shifted"""
    return nr.pose_about(nr.rot("y", 25.0 + 10 * seed) @ nr.rot("x", -15.0), np.array([0.05, -0.1, 0.07]))


def scene_kw(seed):
    """the far rows need a range that reaches them from the rays that start 3 m in front of them"""
    return dict(SCENE_RANGE, min_conf=(nr.MIN_CONF if seed == 1 else 0.0))


# ---- boundary-exact rows --------------------------------------------------------------------------------------------------
def _up(x):
    return np.nextafter(f32(x), f32(np.inf))


def _down(x):
    return np.nextafter(f32(x), f32(-np.inf))


# the frame of boundary_cases(): the identity with t0 = -0, so that O keeps the -0 components of o (0 * -0 = -0, -0 + -0 = -0)
BOUNDARY_POSE = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, -0.0, -0.0, -0.0], f32)


def boundary_cases():
    """Rows and rays built from powers of two, with the answers written by hand: s = 2 and dims = 2^-4 give half-axes 0.5, k = 4,
    (k dims.x) dims.y = 2^-6, so a point is inside iff a a + b b <= 0.25, every operation exact.  Row 0: centre (0, 0, 2), e1 = x,
    e2 = y, n = +z; row 1 its copy.  Returns (model, [(name, rows, rays, keywords, expectations)]): expectations maps an output
    to its values and 'stats' to the exact counts; every case is evaluated on its rows ALONE in the frame BOUNDARY_POSE."""
    d = 2.0 ** -4
    geo = [((0, 0, 2), (1, 0, 0, 0, 1, 0, 0, 0, 1), (d, d)), ((0, 0, 2), (1, 0, 0, 0, 1, 0, 0, 0, 1), (d, d))]
    n = len(geo)
    rng = np.random.default_rng(5)
    m = dict(positions=np.array([g[0] for g in geo]), colors=rng.uniform(0, 255, (n, 3)), stamps=np.tile([50, 60], (n, 1)),
             orientations=np.array([g[1] for g in geo]), shapes=rng.uniform(-1e-3, 1e-3, (n, 6)), dims=np.array([g[2] for g in geo]),
             confidences=np.full(n, 9.0))
    m = {name: np.ascontiguousarray(m[name], dt) for name, _, dt in FIELDS}
    up = [0, 0, 0, 0, 0, 1]                        # from the origin along +z: den = 1, num = 2, tt = 2, hits row 0's back (-n faces it)
    kw = dict(splat_scale=2.0, t_min=1.0, t_max=4.0)
    nan, inf = np.nan, np.inf
    cases = [
        ("tt == t_min", [0], [up], dict(kw, t_min=2.0), dict(t=[2.0], index=[0], point=[[0, 0, 2]])),
        ("tt one ulp below t_min", [0], [up], dict(kw, t_min=_up(2.0)), dict(t=[0.0], index=[-1], point=[[0, 0, 0]], normal=[[0, 0, 0]])),
        ("tt == t_max", [0], [up], dict(kw, t_max=2.0), dict(t=[2.0], index=[0])),
        ("tt one ulp above t_max", [0], [up], dict(kw, t_max=_down(2.0)), dict(t=[0.0], index=[-1])),
        # a = 0.5: a a = 0.25 = the rim (inside); a = 0.5 + 2^-24: a a rounds to 0.25 + 2^-24 > 0.25 (outside)
        ("on the rim and one ulp beyond", [0], [[0.5, 0, 0, 0, 0, 1], [_up(0.5), 0, 0, 0, 0, 1], [0, -0.5, 0, 0, 0, 1], [0, _down(-0.5), 0, 0, 0, 1]],
         kw, dict(t=[2.0, 0.0, 2.0, 0.0], index=[0, -1, 0, -1], point=[[0.5, 0, 2], [0, 0, 0], [0, -0.5, 2], [0, 0, 0]])),
        # a ray in the disc's plane: den = 0 and num = 0
        ("den == 0", [0], [[-2, 0, 2, 1, 0, 0], [-2, 0, 2.5, 1, 0, 0]], kw, dict(t=[0.0, 0.0], index=[-1, -1])),
        ("two coincident discs", [0, 1], [up], kw, dict(t=[2.0], index=[0], stats=dict(rays_hit=1, rows_indexed=2))),
        # from the front (the origin side is -n: den = 1 > 0, the normal flips to -n, with -0 components) and from behind (z = 4 looking down)
        ("both faces", [0], [up, [0, 0, 4, 0, 0, -1]], kw, dict(t=[2.0, 2.0], index=[0, 0], normal=[[-0.0, -0.0, -1.0], [0, 0, 1]],
                                                                 point=[[0, 0, 2], [0, 0, 2]])),
        # -0 in o and d: D = (-0, -0, -1) keeps its signs (1 * -0 + 0 * -0 = -0, + 0 * -1 = -0), O.x = ((-0 + -0) + 0 * 4) + -0 = +0;
        # den = -1, num = -2, tt = 2; P.x = +0 + 2 * -0 = +0
        ("-0 components", [0], [[-0.0, -0.0, 4, -0.0, -0.0, -1]], kw, dict(t=[2.0], index=[0], point=[[0.0, 0.0, 2]], normal=[[0, 0, 1]])),
        ("invalid rays", [0], [[nan, 0, 0, 0, 0, 1], [0, inf, 0, 0, 0, 1], [0, 0, 0, 0, nan, 1], [0, 0, 0, -inf, 0, 1], [0, 0, 0, 0, 0, 0],
                               [0, 0, 0, -0.0, 0, -0.0], up], kw,
         dict(t=[0, 0, 0, 0, 0, 0, 2.0], index=[-1, -1, -1, -1, -1, -1, 0], stats=dict(rays=7, rays_hit=1, rays_invalid=6))),
        # a non-unit direction: tt is a multiple of D (D = 4 z: tt = 0.5, below t_min = 1; D = z / 2: tt = 4 = t_max)
        ("a non-unit direction", [0], [[0, 0, 0, 0, 0, 4], [0, 0, 0, 0, 0, 0.5], [0, 0, 0, 0, 0, 2]], kw,
         dict(t=[0.0, 4.0, 1.0], index=[-1, 0, 0], point=[[0, 0, 0], [0, 0, 2], [0, 0, 2]])),
    ]
    return m, [(name, rows, np.array(rays, f32).reshape(-1, 6), k, want) for name, rows, rays, k, want in cases]


def check_expectations(got, want, what):
    """a result (cast()'s or the device's dict) against one case of boundary_cases(), bit for bit"""
    for key in OUTPUTS:
        if key in want:
            exp = np.array(want[key], got[key].dtype).reshape(got[key].shape)
            a, b = np.ascontiguousarray(got[key]), exp
            same = a.view(np.uint32) == b.view(np.uint32) if a.dtype == np.float32 else a == b
            assert bool(np.all(same)), (what, key, got[key].tolist(), exp.tolist())
    for key, v in want.get("stats", {}).items():
        assert got["stats"][key] == v, (what, key, got["stats"][key], v)
