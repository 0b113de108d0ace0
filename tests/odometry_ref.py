"""numpy restatement of include/ssf_odometry.h: intensity, pyramid, gradients, the linearisation with exact integer sums, the
coarse-to-fine loop.  Every f32 step is one numpy f32 operation in the header's order, so the device's outputs are compared at 0
bits.  The two host steps of an iteration -- the LDLT solve and the Gauss-Newton increment -- are the checker library's
ssf_dbg_ldlt_solve6 / ssf_dbg_gn_increment (pinned against the reference's Eigen by tests/test_solvers.py), so nothing here depends
on numpy's sin / cos.

The sums are taken with numpy int64; no sum can overflow (the header's argument; test_odometry.py evaluates it), so they equal
Python-int sums -- record() with exact=True takes them as Python ints."""
import ctypes as C

import numpy as np

f32, f64 = np.float32, np.float64
MAX_LEVELS, MIN_W, MIN_H, RECORD = 6, 8, 8, 29
S_A, S_B, S_C, CLAMP_BITS = 10, 24, 36, 40
CLAMP = 1 << CLAMP_BITS
REASONS = ("converged", "max_iterations", "too_few_pixels", "degenerate", "motion_gate")
RANGE = (f32(0.2), f32(5.0))              # ssf_default_config's range_min / range_max


def default_params():
    return dict(levels=4, iters=[4, 6, 8, 10, 10, 10], r_max=f32(0.5), huber=f32(0.2), min_pixel_share=f32(0.05), tol_rot=f32(1e-4),
                tol_trans=f32(1e-4), max_translation=f32(0.3), max_rotation=f32(0.35))


def params(**kw):
    p = default_params()
    for k, v in kw.items():
        assert k in p, k
        p[k] = v if k in ("levels", "iters") else f32(v)
    p["iters"] = (list(p["iters"]) + [0] * MAX_LEVELS)[:MAX_LEVELS]
    return p


def convert_depth(depth, scale):
    """uint16 counts -> (float)((double)v * scale); f32 metres pass"""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        return (depth.astype(f64) * f64(scale)).astype(f32)
    assert depth.dtype == f32
    return depth


def intensity(rgb, order="rgb"):
    """H x W x 3|4 uint8 -> Y = (77 R + 150 G + 29 B) >> 8 as f32 * 2^-8"""
    c = np.asarray(rgb).astype(np.int64)
    r, g, b = (c[..., 0], c[..., 1], c[..., 2]) if order.startswith("rgb") else (c[..., 2], c[..., 1], c[..., 0])
    return ((77 * r + 150 * g + 29 * b) >> 8).astype(f32) * f32(0.00390625)


def valid_depth(d, rng=RANGE):
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d >= rng[0]) & (d <= rng[1])


def level_sizes(W, H):
    out = []
    w, h = W, H
    for l in range(MAX_LEVELS):
        if l > 0 and not (w >= MIN_W and h >= MIN_H):
            break
        out.append((w, h))
        w, h = w // 2, h // 2
    return out


def level_intrinsics(K, n):
    """K = (fx, fy, cx, cy) -> one f32 4-tuple per level"""
    fx, fy, cx, cy = (f32(v) for v in K)
    out = [(fx, fy, cx, cy)]
    for _ in range(1, n):
        fx, fy = fx / f32(2), fy / f32(2)
        cx, cy = (cx + f32(0.5)) / f32(2) - f32(0.5), (cy + f32(0.5)) / f32(2) - f32(0.5)
        out.append((fx, fy, cx, cy))
    return out


def gradients(I):
    H, W = I.shape
    xs, ys = np.arange(W), np.arange(H)
    gx = f32(0.5) * (I[:, np.minimum(xs + 1, W - 1)] - I[:, np.maximum(xs - 1, 0)])
    gy = f32(0.5) * (I[np.minimum(ys + 1, H - 1), :] - I[np.maximum(ys - 1, 0), :])
    return gx.astype(f32), gy.astype(f32)


def _min_valid(a, b):
    return np.where(a == 0, b, np.where(b == 0, a, np.minimum(a, b)))


def reduce_level(I, D):
    """level l -> level l + 1: floor(W / 2) x floor(H / 2); I = 0.25f * ((a + b) + (c + d)), D = the smallest non-zero depth of the block"""
    h, w = I.shape[0] // 2, I.shape[1] // 2
    a, b, c, e = I[0:2 * h:2, 0:2 * w:2], I[0:2 * h:2, 1:2 * w:2], I[1:2 * h:2, 0:2 * w:2], I[1:2 * h:2, 1:2 * w:2]
    In = (f32(0.25) * ((a + b) + (c + e))).astype(f32)
    Dn = _min_valid(_min_valid(D[0:2 * h:2, 0:2 * w:2], D[0:2 * h:2, 1:2 * w:2]),
                    _min_valid(D[1:2 * h:2, 0:2 * w:2], D[1:2 * h:2, 1:2 * w:2])).astype(f32)
    return In, Dn


def level0(rgb, depth, order="rgb", depth_scale=1.0, mask=None, rng=RANGE):
    I = intensity(rgb, order)
    d = convert_depth(depth, depth_scale)
    ok = valid_depth(d, rng)
    if mask is not None:
        ok &= np.asarray(mask) == 0
    return I, np.where(ok, d, f32(0)).astype(f32)


def pyramid(rgb, depth, K, order="rgb", depth_scale=1.0, mask=None, rng=RANGE):
    """list of levels: dict(I, D, gx, gy, K, W, H)"""
    I, D = level0(rgb, depth, order, depth_scale, mask, rng)
    H, W = I.shape
    sizes = level_sizes(W, H)
    Ks = level_intrinsics(K, len(sizes))
    out = []
    for l, (w, h) in enumerate(sizes):
        if l > 0:
            I, D = reduce_level(I, D)
        gx, gy = gradients(I)
        out.append(dict(I=I, D=D, gx=gx, gy=gy, K=Ks[l], W=w, H=h))
    return out


def _dot3(a, X):
    return (a[0] * X[0] + a[1] * X[1]) + a[2] * X[2]


def _bilinear(a, i00, W, ax, ay):
    a = a.ravel()
    p00, p10, p01, p11 = a[i00], a[i00 + 1], a[i00 + W], a[i00 + W + 1]
    top, bot = p00 + ax * (p10 - p00), p01 + ax * (p11 - p01)
    return top + ay * (bot - top)


def quantise(v, S):
    """rint((double)v * 2^S) clamped to +-2^40, NaN -> 0, as int64"""
    t = v.astype(f64) * f64(1 << S)
    nan = np.isnan(t)
    t = np.clip(np.where(nan, 0.0, t), -float(CLAMP), float(CLAMP))
    return np.rint(t).astype(np.int64)


def terms(ref, cur, T12, p, rng=RANGE):
    """the 28 quantised term arrays (one entry per pixel that passed step 8) of a level: (int64 28 x n, n, the raw f32 J, r, w)"""
    T = np.asarray(T12, f32)
    R, t = T[:9].reshape(3, 3), T[9:]
    fx, fy, cx, cy = ref["K"]
    W, H = ref["W"], ref["H"]
    ys, xs = np.nonzero(ref["D"] != 0)
    d = ref["D"][ys, xs]
    with np.errstate(all="ignore"):
        X = (((xs.astype(f32) - cx) / fx) * d, ((ys.astype(f32) - cy) / fy) * d, d)
        Y = [_dot3(R[i], X) + t[i] for i in range(3)]
        keep = (Y[2] >= rng[0]) & (Y[2] <= rng[1])
        iz = f32(1) / Y[2]
        u, v = ((fx * Y[0]) * iz) + cx, ((fy * Y[1]) * iz) + cy
        keep &= (u >= 0) & (v >= 0) & (u < f32(W - 1)) & (v < f32(H - 1))
    sel = np.nonzero(keep)[0]
    xs, ys, Y, iz, u, v = xs[sel], ys[sel], [a[sel] for a in Y], iz[sel], u[sel], v[sel]
    x0, y0 = u.astype(np.int64), v.astype(np.int64)
    ax, ay = u - x0.astype(f32), v - y0.astype(f32)
    i00 = y0 * W + x0
    r = _bilinear(cur["I"], i00, W, ax, ay) - ref["I"][ys, xs]
    ar = np.abs(r)
    keep = ar <= p["r_max"]
    with np.errstate(all="ignore"):
        w = np.where(ar <= p["huber"], f32(1), p["huber"] / ar).astype(f32)
    a = _bilinear(cur["gx"], i00, W, ax, ay) * fx
    b = _bilinear(cur["gy"], i00, W, ax, ay) * fy
    g = [a * iz, b * iz, -((((a * Y[0]) + (b * Y[1])) * iz) * iz)]
    c = [Y[1] * g[2] - Y[2] * g[1], Y[2] * g[0] - Y[0] * g[2], Y[0] * g[1] - Y[1] * g[0]]
    J = [q[keep].astype(f32) for q in c + g]
    r, w = r[keep].astype(f32), w[keep]
    q = []
    for i in range(6):
        wj = w * J[i]
        for j in range(i, 6):
            q.append(quantise(wj * J[j], S_A))
    for i in range(6):
        q.append(quantise((w * J[i]) * r, S_B))
    q.append(quantise((w * r) * r, S_C))
    return np.array(q, np.int64).reshape(28, -1), int(keep.sum()), J, r, w


def record(ref, cur, T12, p, rng=RANGE, exact=False):
    """the 29 int64 words"""
    q, n, _, _, _ = terms(ref, cur, T12, p, rng)
    if exact:
        sums = [sum(int(x) for x in row) for row in q]
        assert all(abs(s) < (1 << 63) for s in sums)
    else:
        sums = q.sum(axis=1, dtype=np.int64).tolist()
    return np.array(sums + [n], np.int64)


def _dptr(a):
    return a.ctypes.data_as(C.c_void_p)


def solvers(oracle):
    """(ldlt_solve6, gn_increment) of the checker library (binding.Library)"""
    L = oracle.lib
    L.ssf_dbg_ldlt_solve6.argtypes = [C.c_void_p] * 3
    L.ssf_dbg_gn_increment.argtypes = [C.c_void_p] * 2

    def ldlt(A, b):
        A, b, x = np.ascontiguousarray(A, f64), np.ascontiguousarray(b, f64), np.zeros(6, f64)
        L.ssf_dbg_ldlt_solve6(_dptr(A), _dptr(b), _dptr(x))
        return x

    def gn(X):
        X, tf = np.ascontiguousarray(X, f64), np.zeros(16, f64)
        L.ssf_dbg_gn_increment(_dptr(X), _dptr(tf))
        return tf.reshape(4, 4)
    return ldlt, gn


def mat4_lmul(a, b):
    """a * b with the operation order of ssf_solvers.hpp's mat4_lmul"""
    r = np.zeros((4, 4), f64)
    for i in range(4):
        for j in range(4):
            r[i, j] = ((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) + a[i, 3] * b[3, j]
    return r


def invert(T):
    out = np.zeros((4, 4), f64)
    for i in range(3):
        for j in range(3):
            out[i, j] = T[j, i]
        out[i, 3] = -(((T[0, i] * T[0, 3]) + (T[1, i] * T[1, 3])) + (T[2, i] * T[2, 3]))
    out[3, 3] = 1.0
    return out


def from12(p):
    T = np.eye(4, dtype=f64)
    p = np.asarray(p, f32)
    T[:3, :3] = p[:9].reshape(3, 3).astype(f64)
    T[:3, 3] = p[9:].astype(f64)
    return T


def to12(T):
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]).astype(f32)


def estimate(ref_pyr, cur_pyr, p, oracle, init12=None, rng=RANGE):
    """the LOOP: (rel 12 x f32, result dict as binding.SsfOdometryResult.as_dict)"""
    ldlt, gn = solvers(oracle)
    L = min(p["levels"], len(ref_pyr))
    res = dict(valid=0, reason=None, levels=L, iters=[0] * MAX_LEVELS, pixels=0, mean_sq_residual=0.0)
    T = invert(from12(init12)) if init12 is not None else np.eye(4, dtype=f64)
    failed = converged = False
    for l in range(L - 1, -1, -1):
        if failed:
            break
        ref, cur = ref_pyr[l], cur_pyr[l]
        min_pixels = max(1, int(p["min_pixel_share"] * f32(ref["W"] * ref["H"])))
        converged = False
        for _ in range(p["iters"][l]):
            rec = record(ref, cur, to12(T), p, rng)
            res["iters"][l] += 1
            n = int(rec[28])
            res["pixels"] = n
            res["mean_sq_residual"] = float((f64(rec[27]) / f64(1 << S_C)) / f64(n)) if n > 0 else 0.0
            if n < min_pixels:
                res["reason"], failed = "too_few_pixels", True
                break
            A, k = np.zeros((6, 6), f64), 0
            for i in range(6):
                for j in range(i, 6):
                    A[i, j] = A[j, i] = f64(rec[k]) / f64(1 << S_A)
                    k += 1
            b = np.array([-(f64(rec[21 + i]) / f64(1 << S_B)) for i in range(6)], f64)
            delta = ldlt(A, b)
            if not np.isfinite(delta).all():
                res["reason"], failed = "degenerate", True
                break
            T = mat4_lmul(gn(delta), T)
            nr = np.sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2])
            nt = np.sqrt((delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5])
            if nr < f64(p["tol_rot"]) and nt < f64(p["tol_trans"]):
                converged = True
                break
    inv = invert(T)
    rel = to12(inv)
    if not failed:
        res["reason"] = "converged" if converged else "max_iterations"
        nt = np.sqrt((inv[0, 3] * inv[0, 3] + inv[1, 3] * inv[1, 3]) + inv[2, 3] * inv[2, 3])
        chord = np.sqrt(max(0.0, 3.0 - ((inv[0, 0] + inv[1, 1]) + inv[2, 2])))
        if nt > f64(p["max_translation"]) or chord > f64(p["max_rotation"]) or nt != nt or chord != chord:
            res["reason"] = "motion_gate"
        else:
            res["valid"] = 1
    return rel, res


def compose(pose_ref12, rel12):
    """prior = pose_ref o rel in f32: m3_mul (row_mul order) and m3_mulv (dot3 order) + t"""
    a, r = np.asarray(pose_ref12, f32), np.asarray(rel12, f32)
    A, B = a[:9].reshape(3, 3), r[:9].reshape(3, 3)
    R = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            R[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
    t = np.array([((A[i, 0] * r[9] + A[i, 1] * r[10]) + A[i, 2] * r[11]) + a[9 + i] for i in range(3)], f32)
    return np.concatenate([R.reshape(9), t]).astype(f32)


# ---- what the tests measure: the error of an estimate against a true relative motion ------------------------------------------
def true_rel(pose_ref, pose_cur):
    """(R, t) current camera -> reference camera from two camera-to-map poses (R, t) in f64"""
    Rr, tr = (np.asarray(a, f64) for a in pose_ref)
    Rc, tc = (np.asarray(a, f64) for a in pose_cur)
    return Rr.T @ Rc, Rr.T @ (tc - tr)


def errors(rel12, true):
    """(translation error in metres, rotation error in radians) of rel against true = (R, t)"""
    R, t = np.asarray(rel12[:9], f64).reshape(3, 3), np.asarray(rel12[9:], f64)
    dR = R.T @ true[0]
    skew = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    ang = float(np.arctan2(0.5 * np.linalg.norm(skew), (np.trace(dR) - 1.0) / 2.0))
    return float(np.linalg.norm(t - true[1])), ang


IDENTITY12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)


def quat_to_R(q):
    q = np.asarray(q, f64) / np.linalg.norm(np.asarray(q, f64))        # (a trajectory file rounds to four digits)
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], f64)
