"""The numpy restatement of ssf_query_count / ssf_query_rows (include/ssf_query.h): every step one IEEE f32 operation in the
header's order, on np.float32 scalars and arrays (no einsum, no dot).  select() is what the GPU tests compare against at 0 bits.

select_f64() is a second, independent formulation used only to check select() itself: the same rule in f64, with a guard band.
A row whose f64 margin to any boundary it is compared against is below GUARD (relative to the magnitude of the terms that
made the compared quantity) is "uncertain" and left out of that comparison: f32 rounding (a few units of 6e-8 of those terms) may
legitimately put it on either side.  The boundary-exact rows are tested on their own against hand-written expectations.

Also here: the hand-built models and queries that tests/test_query.py and tests/test_query_gpu.py share."""
import numpy as np

f32 = np.float32
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)
REGIONS = ("all", "sphere", "box", "frustum")
GUARD = 1e-5
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
FIELDS = (("positions", 3, np.float32), ("colors", 3, np.float32), ("stamps", 2, np.int32), ("orientations", 9, np.float32),
          ("shapes", 6, np.float32), ("dims", 2, np.float32), ("confidences", 1, np.float32))


def params(min_conf=0.0, t_init=None, t_last=None, visible_only=False, region="all", radius=0.0, half=(0.0, 0.0, 0.0),
           camera=None, z_range=None):
    """a query as select() takes it: the keywords of Fusion.query_model with the defaults written out (camera and z_range must be
    given for a frustum: the restatement knows no handle)"""
    return dict(min_conf=min_conf, t_init=(I32_MIN, I32_MAX) if t_init is None else tuple(t_init),
                t_last=(I32_MIN, I32_MAX) if t_last is None else tuple(t_last), visible_only=bool(visible_only), region=region,
                radius=radius, half=tuple(half), camera=camera, z_range=z_range)


def _rows_and_gates(model, n_visible, q):
    """the part of the rule that involves no arithmetic: live rows, finite positions, confidence, stamps"""
    pos = np.ascontiguousarray(model["positions"], f32).reshape(-1, 3)
    conf = np.ascontiguousarray(model["confidences"], f32).reshape(-1)
    stamps = np.ascontiguousarray(model["stamps"], np.int32).reshape(-1, 2)
    n = len(conf)
    scanned = int(n_visible) if q["visible_only"] else n
    ok = np.arange(n) < scanned
    ok &= np.isfinite(pos).all(axis=1)
    ok &= conf > f32(q["min_conf"])
    ok &= (stamps[:, 0] >= q["t_init"][0]) & (stamps[:, 0] <= q["t_init"][1])
    ok &= (stamps[:, 1] >= q["t_last"][0]) & (stamps[:, 1] <= q["t_last"][1])
    return pos, ok, scanned


def region_mask(pos, pose, q):
    """steps 2 and 3 of the header in f32, for every row"""
    n = len(pos)
    if q["region"] == "all":
        return np.ones(n, bool)
    pose = np.asarray(pose, f32).ravel()
    R, t = pose[:9].reshape(3, 3), pose[9:]
    with np.errstate(all="ignore"):
        dx, dy, dz = pos[:, 0] - t[0], pos[:, 1] - t[1], pos[:, 2] - t[2]
        if q["region"] == "sphere":
            r2 = (dx * dx + dy * dy) + dz * dz
            return r2 <= f32(q["radius"]) * f32(q["radius"])
        Cx = (R[0, 0] * dx + R[1, 0] * dy) + R[2, 0] * dz
        Cy = (R[0, 1] * dx + R[1, 1] * dy) + R[2, 1] * dz
        Cz = (R[0, 2] * dx + R[1, 2] * dy) + R[2, 2] * dz
        assert Cx.dtype == np.float32 and Cz.dtype == np.float32
        if q["region"] == "box":
            h = [f32(v) for v in q["half"]]
            return (np.abs(Cx) <= h[0]) & (np.abs(Cy) <= h[1]) & (np.abs(Cz) <= h[2])
        assert q["region"] == "frustum", q["region"]
        K = q["camera"]
        fx, fy, cx, cy = f32(K["fx"]), f32(K["fy"]), f32(K["cx"]), f32(K["cy"])
        ulim, vlim = f32(K["width"]) - f32(0.5), f32(K["height"]) - f32(0.5)
        zmin, zmax = f32(q["z_range"][0]), f32(q["z_range"][1])
        inz = (Cz >= zmin) & (Cz <= zmax)
        u = (fx * Cx) / Cz + cx
        v = (fy * Cy) / Cz + cy
        assert u.dtype == np.float32
        return inz & (u >= f32(-0.5)) & (u < ulim) & (v >= f32(-0.5)) & (v < vlim)


def select(model, n_visible, pose, q):
    """(index int32: the selected rows' logical indices in ascending order, stats as Fusion.query_count returns them)"""
    pos, ok, scanned = _rows_and_gates(model, n_visible, q)
    ok = ok & region_mask(pos, pose, q)
    index = np.flatnonzero(ok).astype(np.int32)
    lo, hi = np.zeros(3, f32), np.zeros(3, f32)
    if len(index):
        p = pos[index] + f32(0.0)                    # -0 counts as +0
        lo, hi = p.min(axis=0), p.max(axis=0)
    return index, dict(n_scanned=scanned, n_selected=len(index), n_selected_visible=int((index < n_visible).sum()), lo=lo, hi=hi)


def select_f64(model, n_visible, pose, q):
    """(selected: bool per row, uncertain: bool per row) -- the rule in f64 with the guard band of this module's docstring"""
    pos, ok, _ = _rows_and_gates(model, n_visible, q)
    n = len(pos)
    uncertain = np.zeros(n, bool)
    if q["region"] == "all":
        return ok, uncertain
    P = np.where(np.isfinite(pos), pos, 0).astype(np.float64)
    pose = np.asarray(pose, f32).ravel().astype(np.float64)
    R, t = pose[:9].reshape(3, 3), pose[9:]
    d = P - t

    def cmp_le(a, b, scale):
        """a <= b, and whether the margin is inside the guard band"""
        return a <= b, np.abs(a - b) < GUARD * np.maximum(scale, np.abs(b))

    if q["region"] == "sphere":
        r2 = (d * d).sum(axis=1)
        inside, unc = cmp_le(r2, np.float64(f32(q["radius"])) ** 2, r2)
        return ok & inside, ok & unc
    C = d @ R                                        # C_j = sum_i R_ij d_i
    S = np.abs(d) @ np.abs(R)                        # the magnitude of the terms of each sum
    if q["region"] == "box":
        inside = np.ones(n, bool)
        for j in range(3):
            a, u_ = cmp_le(np.abs(C[:, j]), np.float64(f32(q["half"][j])), S[:, j])
            inside &= a
            uncertain |= u_
        return ok & inside, ok & uncertain
    K = q["camera"]
    fx, fy, cx, cy = (np.float64(f32(K[k])) for k in ("fx", "fy", "cx", "cy"))
    zmin, zmax = (np.float64(f32(v)) for v in q["z_range"])
    z = C[:, 2]
    a0, u0 = cmp_le(zmin, z, S[:, 2])
    a1, u1 = cmp_le(z, zmax, S[:, 2])
    inside = a0 & a1
    uncertain = u0 | u1
    zs = np.where(inside, z, 1.0)
    for f, c, j, lim in ((fx, cx, 0, K["width"]), (fy, cy, 1, K["height"])):
        w = f * C[:, j] / zs + c
        scale = np.abs(f) * S[:, j] / zs + np.abs(f * C[:, j] / zs) * S[:, 2] / zs + np.abs(c) + 0.5
        a, ua = cmp_le(-0.5, w, scale)
        b, ub = cmp_le(w, lim - 0.5, scale)          # (the rule is w < lim - 0.5: equality is inside the band anyway)
        uncertain |= inside & (ua | ub)
        inside = inside & a & b & (w < lim - 0.5)
    return ok & inside, ok & uncertain


# ---- the hand-built models and queries of the tests --------------------------------------------------------------------
SIZES = ((1, 1), (255, 0), (256, 256), (257, 256), (700, 250), (1300, 513))      # (n, n_visible): block and wave edges of both stores
SEEDS = (0, 1, 2)
MIN_CONF = 10.0


def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def pose_about(R, t):
    return np.concatenate([np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64)]).astype(f32)


CALLER_POSE = pose_about(rot_y(30.0), (0.3, -0.2, 0.4))          # rotated 30 degrees about y, shifted


def hand_model(n, seed):
    """n rows: positions uniform in a 6 m cube about the camera (the origin), confidences uniform about MIN_CONF, stamps spread
    over 0..100, everything else arbitrary (it is only copied).  Row 0 is fixed: 0.6 m in front of CALLER_POSE's origin and 1 m in
    front of the identity pose's, with a confidence below MIN_CONF -- so that even the one-row model is selected by some of
    region_queries() and rejected by others."""
    rng = np.random.default_rng(7919 * seed + n)
    m = dict(positions=rng.uniform(-3.0, 3.0, (n, 3)), colors=rng.uniform(0.0, 255.0, (n, 3)),
             orientations=rng.normal(size=(n, 9)), shapes=rng.uniform(-1e-3, 1e-3, (n, 6)), dims=rng.uniform(1e-4, 1e-2, (n, 2)),
             confidences=rng.uniform(0.0, 2.0 * MIN_CONF, n))
    t0 = rng.integers(0, 101, n)
    m["stamps"] = np.stack([t0, t0 + (rng.integers(0, 101, n) * (100 - t0)) // 100], axis=1)
    m = {name: np.ascontiguousarray(m[name], dt) for name, _, dt in FIELDS}
    m["positions"][0] = (0.3, -0.2, 1.0)
    m["confidences"][0] = 0.5 * MIN_CONF
    m["stamps"][0] = (40, 60)
    return m


def region_queries(camera, z_range):
    """[(name, pose or None, keywords of Fusion.query_model)]: each of the four regions with and without visible_only, with
    CALLER_POSE and with the handle's pose (None)"""
    base = dict(all=dict(region="all", min_conf=MIN_CONF, t_last=(20, 80)),
                sphere=dict(region="sphere", radius=2.5),
                box=dict(region="box", half=(2.0, 1.5, 2.5), t_init=(10, 90)),
                frustum=dict(region="frustum", camera=camera, z_range=z_range))
    out = []
    for name in REGIONS:
        for vis in (False, True):
            for pose in (CALLER_POSE, None):
                out.append(("%s%s%s" % (name, " visible" if vis else "", " caller-pose" if pose is not None else ""), pose,
                            dict(base[name], visible_only=vis)))
    return out


def boundary_rows():
    """Rows that sit EXACTLY on a boundary of the rule at the identity pose, with the answer written by hand.  Returns (model,
    n_visible, camera, z_range, [(name, keywords, expected logical indices)]).  Camera 21 x 17, fx = fy = 8, cx = 10, cy = 8, z in 0.25..4: all
    values are small dyadic rationals, so every f32 operation of the rule is exact."""
    cam = dict(width=21, height=17, fx=8.0, fy=8.0, cx=10.0, cy=8.0)
    zr = (0.25, 4.0)
    nan = np.nan
    pos = [(1.5, 2.0, 0.0),        # 0: r2 = 6.25 = 2.5^2 exactly: inside the sphere of radius 2.5
           (1.5, 2.0, 0.125),      # 1: r2 = 6.265625: outside
           (1.25, 0.0, 0.5),       # 2: |C.x| = half[0] = 1.25: inside the box (u = 30: outside the frustum)
           (-1.25, 0.5, -0.5),     # 3: |C.x| = half[0] on the other side, |C.y| = half[1]: inside
           (1.2500001, 0.0, 0.5),  # 4: one ulp past half[0]: outside
           (-1.3125, 0.0, 1.0),    # 5: u = 8 * -1.3125 / 1 + 10 = -0.5: inside the frustum (u >= -0.5)
           (1.3125, 0.0, 1.0),     # 6: u = 20.5 = W - 0.5: outside (u < W - 0.5)
           (0.0, -1.0625, 1.0),    # 7: v = -0.5: inside
           (0.0, 1.0625, 1.0),     # 8: v = 16.5 = H - 0.5: outside
           (0.0, 0.0, 0.25),       # 9: z = z_min: inside
           (0.0, 0.0, 4.0),        # 10: z = z_max: inside
           (0.0, 0.0, 4.5),        # 11: z beyond z_max: outside; its stamps are outside both stamp queries
           (nan, 0.0, 1.0),        # 12: a NaN position: never selected
           (0.0, np.inf, 1.0),     # 13: an infinite position: never selected
           (-0.0, -0.0, 1.0),      # 14: -0 coordinates: lo / hi report +0
           (0.0, 0.0, 1.0)]        # 15: conf == min_conf (below): not selected where min_conf = 7
    n = len(pos)
    conf = np.full(n, 9.0)
    conf[15] = 7.0
    stamps = np.tile([50, 60], (n, 1))
    stamps[9] = (10, 60)           # t_init == the lower bound of the stamp query
    stamps[10] = (50, 90)          # t_last == the upper bound
    stamps[11] = (9, 91)           # one outside each
    rng = np.random.default_rng(5)
    m = dict(positions=np.array(pos), colors=rng.uniform(0, 255, (n, 3)), stamps=stamps, orientations=rng.normal(size=(n, 9)),
             shapes=rng.uniform(-1e-3, 1e-3, (n, 6)), dims=rng.uniform(1e-4, 1e-2, (n, 2)), confidences=conf)
    m = {name: np.ascontiguousarray(m[name], dt) for name, _, dt in FIELDS}
    finite = [i for i in range(n) if i not in (12, 13)]
    cases = [
        ("sphere r2 == radius^2", dict(region="sphere", radius=2.5), [i for i in finite if i != 1 and i not in (10, 11)]),
        ("box |C.x| == half[0]", dict(region="box", half=(1.25, 0.5, 0.5)), [2, 3, 9]),
        ("frustum u, v, z on the bounds", dict(region="frustum", camera=cam, z_range=zr), [5, 7, 9, 10, 14, 15]),
        ("conf == min_conf", dict(min_conf=7.0), [i for i in finite if i != 15]),
        ("conf just above min_conf", dict(min_conf=6.9999995), finite),
        ("t_init == its lower bound", dict(t_init=(10, 50)), [i for i in finite if i != 11]),
        ("t_init above its lower bound", dict(t_init=(11, 50)), [i for i in finite if i not in (9, 11)]),
        ("t_last == its upper bound", dict(t_last=(60, 90)), [i for i in finite if i != 11]),
        ("t_last below its upper bound", dict(t_last=(60, 89)), [i for i in finite if i not in (10, 11)]),
        ("NaN and infinite positions", dict(), finite),
        ("-0 in lo / hi", dict(region="sphere", radius=1.0, min_conf=8.0), [9, 14]),
    ]
    return m, 9, cam, zr, cases
