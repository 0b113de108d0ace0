"""The render of include/ssf_render.h in numpy f32, one IEEE operation per step in the header's order, so that it reproduces
ssf_render_model bit for bit.

Two forms share the per-(row, pixel) evaluation and differ only in which pairs they evaluate:
  * brute force: every row against every pixel (small images only);
  * fragments: every row against the pixels of its own conservative box (float64, wider than the library's), for large maps.
The result depends on the minimum key per pixel only, so both forms must agree exactly; the tests check that they do."""
import numpy as np

f32 = np.float32
OUTPUTS = ("depth", "index", "rgb8", "color", "normal")
STATS = ("fragments", "pixels_filled", "rows_shown")


def _to_camera(R, v):
    """R^T v per row with component j = (R0j v.x + R1j v.y) + R2j v.z, all f32"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([(R[0, j] * x + R[1, j] * y) + R[2, j] * z for j in range(3)], 1)


class Scene:
    """the camera-frame records of the rows that are drawn (rule 5), in logical order"""

    def __init__(self, model, n_visible, pose12, camera, z_range, min_conf=0.0, s=3.0, visible_only=False):
        pose = np.asarray(pose12, f32).ravel()
        R, t = pose[:9].reshape(3, 3), pose[9:12]
        self.W, self.H = int(camera["width"]), int(camera["height"])
        self.fx, self.fy, self.cx, self.cy = (f32(camera[k]) for k in ("fx", "fy", "cx", "cy"))
        self.zmin, self.zmax = f32(z_range[0]), f32(z_range[1])
        s = f32(3.0) if f32(s) == 0 else f32(s)
        self.s, k = s, f32(s) * f32(s)
        n = len(model["confidences"]) if not visible_only else int(n_visible)
        conf = np.asarray(model["confidences"], f32)[:n]
        dims = np.asarray(model["dims"], f32).reshape(-1, 2)[:n]
        with np.errstate(all="ignore"):
            keep = (conf > f32(min_conf)) & (dims[:, 0] > 0) & (dims[:, 1] > 0) & np.isfinite(dims[:, 0]) & np.isfinite(dims[:, 1])
            self.logical = np.nonzero(keep)[0].astype(np.int64)
            pos = np.asarray(model["positions"], f32).reshape(-1, 3)[:n][keep]
            ori = np.asarray(model["orientations"], f32).reshape(-1, 3, 3)[:n][keep]
            self.C = _to_camera(R, pos - t)
            self.E1, self.E2, self.N = _to_camera(R, ori[:, 0]), _to_camera(R, ori[:, 1]), _to_camera(R, ori[:, 2])
            self.dx, self.dy = dims[keep, 0], dims[keep, 1]
            N, C = self.N, self.C
            self.num = (N[:, 0] * C[:, 0] + N[:, 1] * C[:, 1]) + N[:, 2] * C[:, 2]
            self.rhs = (k * self.dx) * self.dy
            self.qx = (np.arange(self.W).astype(f32) - self.cx) / self.fx
            self.qy = (np.arange(self.H).astype(f32) - self.cy) / self.fy
        self.colors = np.asarray(model["colors"], f32).reshape(-1, 3)

    def evaluate(self, r, u, v):
        """rows r (indices into the drawn rows), pixels (u, v): (passes steps 3-5, z)"""
        with np.errstate(all="ignore"):
            qx, qy = self.qx[u], self.qy[v]
            N = self.N[r]
            den = (N[:, 0] * qx + N[:, 1] * qy) + N[:, 2]
            z = self.num[r] / den
            ok = (den != 0) & np.isfinite(z) & (z >= self.zmin) & (z <= self.zmax)
            C = self.C[r]
            Dx, Dy, Dz = z * qx - C[:, 0], z * qy - C[:, 1], z - C[:, 2]
            E1, E2 = self.E1[r], self.E2[r]
            a = (Dx * E1[:, 0] + Dy * E1[:, 1]) + Dz * E1[:, 2]
            b = (Dx * E2[:, 0] + Dy * E2[:, 1]) + Dz * E2[:, 2]
            ok &= (a * a) * self.dy[r] + (b * b) * self.dx[r] <= self.rhs[r]
        return ok, z

    def boxes(self):
        """(u0, u1, v0, v1) per drawn row, inclusive; u0 > u1 = nothing.  float64, conservative: a candidate's hit point lies in
        the disc's plane and ellipse up to f32 rounding, and z_min <= z <= z_max; the whole image when an input is not finite."""
        n, W, H = len(self.logical), self.W, self.H
        u0, u1 = np.zeros(n, np.int64), np.full(n, W - 1, np.int64)
        v0, v1 = np.zeros(n, np.int64), np.full(n, H - 1, np.int64)
        with np.errstate(all="ignore"):
            C, E1, E2 = self.C.astype(np.float64), self.E1.astype(np.float64), self.E2.astype(np.float64)
            s = float(self.s)
            hx, hy = s * np.sqrt(self.dx.astype(np.float64)), s * np.sqrt(self.dy.astype(np.float64))
            fin = np.isfinite(C).all(1) & np.isfinite(E1).all(1) & np.isfinite(E2).all(1) & np.isfinite(hx) & np.isfinite(hy)
            slack = 1e-4 * (np.abs(C).sum(1) + hx + hy) + 1e-5
            ext = np.sqrt((E1 * hx[:, None]) ** 2 + (E2 * hy[:, None]) ** 2) * 1.01 + slack[:, None]
            z0 = np.maximum(C[:, 2] - ext[:, 2], float(self.zmin))
            z1 = np.minimum(C[:, 2] + ext[:, 2], float(self.zmax))
            empty = fin & ~(z0 <= z1)
            lo, hi = C - ext, C + ext
            sx = np.stack([lo[:, 0] / z0, lo[:, 0] / z1, hi[:, 0] / z0, hi[:, 0] / z1], 1)
            sy = np.stack([lo[:, 1] / z0, lo[:, 1] / z1, hi[:, 1] / z0, hi[:, 1] / z1], 1)
            us = float(self.fx) * sx + float(self.cx)
            vs = float(self.fy) * sy + float(self.cy)
            ulo, uhi = np.floor(us.min(1)) - 3, np.ceil(us.max(1)) + 3
            vlo, vhi = np.floor(vs.min(1)) - 3, np.ceil(vs.max(1)) + 3
            boxed = fin & ~empty
            off = boxed & ((uhi < 0) | (ulo > W - 1) | (vhi < 0) | (vlo > H - 1))
            on = boxed & ~off
            u0[on] = np.clip(ulo[on], 0, W - 1).astype(np.int64); u1[on] = np.clip(uhi[on], 0, W - 1).astype(np.int64)
            v0[on] = np.clip(vlo[on], 0, H - 1).astype(np.int64); v1[on] = np.clip(vhi[on], 0, H - 1).astype(np.int64)
            u0[empty | off] = 1; u1[empty | off] = 0
        return u0, u1, v0, v1


def _pairs_brute(sc, chunk=1 << 22):
    P, n = sc.W * sc.H, len(sc.logical)
    per = max(1, chunk // max(P, 1))
    for r0 in range(0, n, per):
        rows = np.arange(r0, min(n, r0 + per))
        r = np.repeat(rows, P)
        pix = np.tile(np.arange(P), len(rows))
        yield r, pix % sc.W, pix // sc.W


def _pairs_fragments(sc, chunk=1 << 24):
    u0, u1, v0, v1 = sc.boxes()
    wu, hv = np.maximum(u1 - u0 + 1, 0), np.maximum(v1 - v0 + 1, 0)
    cnt = wu * hv
    n, r0 = len(cnt), 0
    while r0 < n:
        csum = np.cumsum(cnt[r0:])
        r1 = r0 + max(1, int(np.searchsorted(csum, chunk, side="right")))
        rows = np.arange(r0, min(r1, n))
        c = cnt[rows]
        r = np.repeat(rows, c)
        start = np.repeat(np.cumsum(c) - c, c)
        local = np.arange(len(r)) - start
        yield r, u0[r] + local % wu[r], v0[r] + local // wu[r]
        r0 = r1


def render(model, n_visible, pose12, camera, z_range, min_conf=0.0, s=3.0, visible_only=False, form="fragments"):
    """dict of the five images and the three stats of ssf_render_model; form 'brute' or 'fragments'"""
    sc = Scene(model, n_visible, pose12, camera, z_range, min_conf, s, visible_only)
    W, H = sc.W, sc.H
    P = W * H
    EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = np.full(P, EMPTY, np.uint64)
    frags = 0
    for r, u, v in (_pairs_brute(sc) if form == "brute" else _pairs_fragments(sc)):
        ok, z = sc.evaluate(r, u, v)
        frags += int(ok.sum())
        if ok.any():
            key = (z[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | sc.logical[r[ok]].astype(np.uint64)
            np.minimum.at(best, (v[ok] * W + u[ok]).astype(np.int64), key)
    filled = best != EMPTY
    depth = np.zeros(P, f32)
    index = np.full(P, -1, np.int32)
    color = np.zeros((P, 3), f32)
    normal = np.zeros((P, 3), f32)
    if filled.any():
        kb = best[filled]
        depth[filled] = (kb >> np.uint64(32)).astype(np.uint32).view(f32)
        lg = (kb & np.uint64(0xFFFFFFFF)).astype(np.int64)
        index[filled] = lg.astype(np.int32)
        color[filled] = sc.colors[lg]
        pix = np.nonzero(filled)[0]
        pos = np.searchsorted(sc.logical, lg)
        N = sc.N[pos]
        den = (N[:, 0] * sc.qx[pix % W] + N[:, 1] * sc.qy[pix // W]) + N[:, 2]
        normal[filled] = np.where((den > 0)[:, None], -N, N)
    with np.errstate(all="ignore"):
        rgb8 = np.fmin(f32(255), np.fmax(f32(0), np.rint(color))).astype(np.uint8)
    return dict(depth=depth.reshape(H, W), index=index.reshape(H, W), rgb8=rgb8.reshape(H, W, 3), color=color.reshape(H, W, 3),
                normal=normal.reshape(H, W, 3),
                stats=dict(fragments=frags, pixels_filled=int(filled.sum()),
                           rows_shown=int(len(np.unique(index[filled]))) if filled.any() else 0))


def assert_same_render(got, ref, what=""):
    """all five images bit for bit and the three stats"""
    for nm in OUTPUTS:
        a, b = np.ascontiguousarray(got[nm]), np.ascontiguousarray(ref[nm])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, nm, a.shape, a.dtype, b.shape, b.dtype)
        ua, ub = a.view(np.uint8).reshape(a.shape[0], a.shape[1], -1), b.view(np.uint8).reshape(b.shape[0], b.shape[1], -1)
        bad = np.nonzero((ua != ub).any(2))
        assert len(bad[0]) == 0, "%s %s: %d pixels differ, first at (v, u) = (%d, %d): %r vs %r" % (
            what, nm, len(bad[0]), bad[0][0], bad[1][0], a[bad[0][0], bad[1][0]], b[bad[0][0], bad[1][0]])
    for k in STATS:
        assert got["stats"][k] == ref["stats"][k], (what, k, got["stats"][k], ref["stats"][k])


def disc_rows(centres, e1, e2, dims, conf=10.0, colors=None):
    """a model (get_model's dict) of discs: centre, in-plane axes e1 / e2 (normal = e1 x e2), dims = (dx, dy) per row"""
    c = np.asarray(centres, f32).reshape(-1, 3)
    n = len(c)
    e1 = np.broadcast_to(np.asarray(e1, np.float64), (n, 3))
    e2 = np.broadcast_to(np.asarray(e2, np.float64), (n, 3))
    nrm = np.cross(e1, e2)
    ori = np.stack([e1, e2, nrm], 1).astype(f32).reshape(n, 9)
    dims = np.broadcast_to(np.asarray(dims, f32), (n, 2)).copy()
    conf = np.broadcast_to(np.asarray(conf, f32), (n,)).copy()
    col = (np.asarray(colors, f32).reshape(n, 3) if colors is not None
           else (np.arange(3 * n).reshape(n, 3) * 37 % 256).astype(f32))
    shapes = np.zeros((n, 6), f32)
    shapes[:, 0], shapes[:, 3], shapes[:, 5] = dims[:, 0], dims[:, 1], 1e-6
    return dict(positions=c, colors=col, stamps=np.zeros((n, 2), np.int32), orientations=ori, shapes=shapes, dims=dims,
                confidences=conf)


IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)


def adversarial_model(rng, n, W, H, fx, with_huge=True):
    """seeded discs in front of a camera at the identity: random orientations and sizes, grazing discs (normal nearly
    perpendicular to the ray), discs straddling the camera plane, discs larger than the image, duplicates at equal depth,
    rows below the confidence threshold, zero / negative / NaN dims"""
    z = rng.uniform(0.3, 4.0, n)
    x = rng.uniform(-0.6, 0.6, n) * z
    y = rng.uniform(-0.5, 0.5, n) * z
    c = np.stack([x, y, z], 1)
    a = rng.normal(size=(n, 3)); a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = rng.normal(size=(n, 3)); b -= (b * a).sum(1, keepdims=True) * a; b /= np.linalg.norm(b, axis=1, keepdims=True)
    dims = rng.uniform(1e-5, 4e-3, (n, 2))
    k = n // 8
    # grazing: the normal almost perpendicular to the ray through the centre
    ray = c[:k] / np.linalg.norm(c[:k], axis=1, keepdims=True)
    a[:k] = ray
    b[:k] = np.cross(ray, rng.normal(size=(k, 3))); b[:k] /= np.linalg.norm(b[:k], axis=1, keepdims=True)
    a[:k] = np.cross(b[:k], ray + 1e-3 * rng.normal(size=(k, 3))); a[:k] /= np.linalg.norm(a[:k], axis=1, keepdims=True)
    # straddling the camera plane z = 0 (and the near plane)
    c[k:2 * k, 2] = rng.uniform(-0.2, 0.3, k)
    dims[k:2 * k] = rng.uniform(0.01, 0.05, (k, 2))
    if with_huge:
        dims[2 * k:2 * k + 3] = 4.0                  # half-axes of 6 m: larger than the image
    # duplicates of some rows (equal depth: the smaller index wins)
    c[3 * k:3 * k + 5] = c[3 * k + 5:3 * k + 10]; a[3 * k:3 * k + 5] = a[3 * k + 5:3 * k + 10]; b[3 * k:3 * k + 5] = b[3 * k + 5:3 * k + 10]
    dims[3 * k:3 * k + 5] = dims[3 * k + 5:3 * k + 10]
    conf = rng.uniform(0.5, 20.0, n)
    conf[4 * k:4 * k + 4] = 1.0
    dims[5 * k] = (0.0, 1e-3); dims[5 * k + 1] = (-1e-3, 1e-3); dims[5 * k + 2] = (np.nan, 1e-3); dims[5 * k + 3] = (1e-3, np.inf)
    m = disc_rows(c, a, b, dims, conf, colors=rng.uniform(-20, 280, (n, 3)))
    m["colors"][0] = (2.5, 3.5, 254.5)
    return m
