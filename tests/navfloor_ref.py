"""The numpy restatement of ssf_navfloor_fit (include/ssf_navfloor.h): the device steps one IEEE f32 operation each in the header's
order on np.float32 arrays (no einsum, no dot), the sums and the centring in Python ints, the host steps on Python floats (f64) in the
header's order.  fit() is what the GPU tests compare against with ==, and what tests/test_navfloor.py checks against an independent
f64 least-squares plane.

Also here: the scenes that tests/test_navfloor.py and tests/test_navfloor_gpu.py share."""
import math

import numpy as np

import navgrid_ref as nr

f32 = np.float32
OK, NO_FLOOR, DEGENERATE = 0, 1, 2
DIR_BINS, HEIGHT_BINS, MAX_ROUNDS = 31, 2048, 8
I32_MIN, I32_MAX = nr.I32_MIN, nr.I32_MAX
DEFAULTS = dict(up=(0.0, -1.0, 0.0), origin=None, tilt_cos=0.8, align_cos=0.95, height_res=0.02, min_rows=32, floor_share256=64,
                refine_iters=3, first_dist=0.15, inlier_dist=0.05, min_conf=0.0, t_init=(I32_MIN, I32_MAX), t_last=(I32_MIN, I32_MAX),
                visible_only=False, width=512, height=512, res=0.05, below=0.5, step=0.2, body_height=1.5)
COUNTS = ("rows_used", "candidates", "direction_rows", "aligned", "height_out_of_range", "height_rows")
INTEGERS = ("status", "rounds") + COUNTS + ("dir_bin", "height_bin", "inliers", "sums")      # what test_navfloor.py's parameter guard looks at
FLOATS = ("normal", "d", "origin", "camera_height", "rms", "pose", "z_min", "floor_max", "z_max", "res")


def params(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    q = dict(DEFAULTS, **kw)
    q["t_init"] = (I32_MIN, I32_MAX) if q["t_init"] is None else tuple(q["t_init"])
    q["t_last"] = (I32_MIN, I32_MAX) if q["t_last"] is None else tuple(q["t_last"])
    return q


# ---- the host steps: f64 in the header's order (csrc/ssf_navfloor_solve.hpp) ---------------------------------------------------
def dot3(v, w):
    return (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]


def _d(v):
    return [float(x) for x in v]


def _f(v):
    return np.array([f32(x) for x in v], f32)


def unit_up(up):
    U = _d(np.asarray(up, f32))
    L = math.sqrt(dot3(U, U))
    return _f([U[k] / L for k in range(3)])


def frame(n, v):
    """frame(n, v) of step 0: (x, y) as f32 vectors, or None"""
    N, V = _d(n), _d(v)
    t = dot3(V, N)
    Wv = [V[k] - t * N[k] for k in range(3)]
    L = math.sqrt(dot3(Wv, Wv))
    if not L > 0.0:
        return None
    X = [Wv[k] / L for k in range(3)]
    Y = [N[1] * X[2] - N[2] * X[1], N[2] * X[0] - N[0] * X[2], N[0] * X[1] - N[1] * X[0]]
    return _f(X), _f(Y)


def hint_frame(u):
    e = 0
    for k in (1, 2):
        if abs(u[k]) < abs(u[e]):
            e = k
    ax = np.zeros(3, f32)
    ax[e] = 1
    return frame(u, ax)


def vote_scale(tilt_cos):
    tc = f32(tilt_cos)
    return f32(15.0) / np.sqrt(f32(1.0) - tc * tc)


def direction_winner(hist):
    """(ia, ib, window sum) of a 31 x 31 histogram (index ib * 31 + ia), or None when it is empty"""
    h = np.asarray(hist, np.uint64).reshape(DIR_BINS, DIR_BINS)
    pad = np.zeros((DIR_BINS + 2, DIR_BINS + 2), np.uint64)
    pad[1:-1, 1:-1] = h
    win = sum(pad[1 + dy:1 + dy + DIR_BINS, 1 + dx:1 + dx + DIR_BINS] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    if not win.any():
        return None
    at = int(np.argmax(win.ravel()))                                  # the first of the largest: the smallest ib * 31 + ia
    return at % DIR_BINS, at // DIR_BINS, int(win.ravel()[at])


def direction_normal(S):
    D = [float(int(s)) for s in S]
    L = math.sqrt(dot3(D, D))
    if not L > 0.0:
        return None
    return _f([D[k] / L for k in range(3)])


def height_windows(hist):
    h = np.asarray(hist, np.uint64)
    w = h.copy()
    w[1:] += h[:-1]
    w[:-1] += h[1:]
    return w


def height_winner(hist, min_rows, floor_share256):
    """(j*, W(j*)) or None"""
    w = [int(v) for v in height_windows(hist)]
    wmax = max(w)
    j0 = next((j for j in range(HEIGHT_BINS) if w[j] >= min_rows and w[j] * 256 >= floor_share256 * wmax), None)
    if j0 is None:
        return None
    js = j0
    for j in range(j0 + 1, min(j0 + 4, HEIGHT_BINS - 1) + 1):
        if w[j] > w[js]:
            js = j
    return js, w[js]


def height_of_bin(j, height_res):
    return (f32(j - 1024) + f32(0.5)) * f32(height_res)


def refine_round(s, min_rows, n, a, b, d):
    """(status, n_new, d_new, rms, (alpha, beta)) of one round's ten words"""
    s = [int(v) for v in s]
    N, Sx, Sy, Sz = s[:4]
    if N < min_rows:
        return NO_FLOOR, None, None, None, None
    Cxx, Cxy, Cyy = float(N * s[4] - Sx * Sx), float(N * s[5] - Sx * Sy), float(N * s[6] - Sy * Sy)
    Cxz, Cyz, Czz = float(N * s[7] - Sx * Sz), float(N * s[8] - Sy * Sz), float(N * s[9] - Sz * Sz)
    det = Cxx * Cyy - Cxy * Cxy
    if not det > 0.0:
        return DEGENERATE, None, None, None, None
    alpha = (Cxz * Cyy - Cyz * Cxy) / det
    beta = (Cyz * Cxx - Cxz * Cxy) / det
    gamma = ((float(Sz) - alpha * float(Sx)) - beta * float(Sy)) / float(N)
    nd, ad, bd = _d(n), _d(a), _d(b)
    V = [(nd[k] - alpha * ad[k]) - beta * bd[k] for k in range(3)]
    L = math.sqrt(dot3(V, V))
    if not L > 0.0 or not math.isfinite(L):
        return DEGENERATE, None, None, None, None
    n_new = _f([V[k] / L for k in range(3)])
    d_new = f32((float(d) + gamma * 0.0009765625) / L)
    r = (Czz - alpha * Cxz) - beta * Cyz
    if not r > 0.0:
        r = 0.0
    rms = f32(math.sqrt(r / (float(N) * float(N))) * 0.0009765625)
    return OK, n_new, d_new, rms, (alpha, beta)


def camera_height(pc, normal, d):
    return f32(dot3(_d(pc), _d(normal)) - float(d))


def grid_pose(normal, d, o, pc, a, b, width, height, res):
    fr = frame(normal, a) or frame(normal, b)
    x, y = fr
    res = f32(res)
    gx, gy = dot3(pc, x), dot3(pc, y)
    sx = (np.floor(gx / res) - f32(width // 2)) * res
    sy = (np.floor(gy / res) - f32(height // 2)) * res
    assert sx.dtype == np.float32
    pose = np.zeros(12, f32)
    for i in range(3):
        pose[3 * i], pose[3 * i + 1], pose[3 * i + 2] = x[i] + f32(0.0), y[i] + f32(0.0), normal[i] + f32(0.0)
        pose[9 + i] = f32(((float(o[i]) + float(sx) * float(x[i])) + float(sy) * float(y[i])) + float(d) * float(normal[i]))
    return pose


# ---- the device steps: f32, one operation each ---------------------------------------------------------------------------------
def _dotv(v, w):
    """dot of the n x 3 f32 array v with the f32 vector w, three-term form"""
    return (v[:, 0] * w[0] + v[:, 1] * w[1]) + v[:, 2] * w[2]


def _dir_bin(v, scale):
    with np.errstate(all="ignore"):
        t = np.floor(v * scale + f32(0.5))
    out = np.where(~(t > f32(-15.0)), 0, np.where(t >= f32(15.0), 30, 0)).astype(np.int64)
    mid = (t > f32(-15.0)) & ~(t >= f32(15.0))
    out[mid] = t[mid].astype(np.int64) + 15
    return out


def _quant(v, scale):
    return np.rint(v.astype(np.float64) * scale).astype(np.int64)


def fit(model, n_visible, camera, q):
    """The result of ssf_navfloor_fit as Fusion.nav_floor returns it (without 'grid'), plus 'dir_hist', 'height_hist', 'alpha_beta'
    (per round run) and 'inlier_rows' (the logical indices of the inliers of the last round that ran).  camera: the handle's camera
    position (3 floats)."""
    cam = np.asarray(camera, f32).ravel()[-3:]
    u = unit_up(q["up"])
    a, b = hint_frame(u)
    o = cam.copy() if q["origin"] is None else np.asarray(q["origin"], f32)
    pc = cam - o
    gate = dict(min_conf=q["min_conf"], t_init=q["t_init"], t_last=q["t_last"], visible_only=q["visible_only"])
    rows = nr.used_rows(model, n_visible, gate)
    nrm = np.ascontiguousarray(model["orientations"], f32).reshape(-1, 9)[rows][:, 6:9]
    with np.errstate(invalid="ignore"):
        ok = (np.abs(nrm) <= f32(2.0)).all(axis=1)
    rows, nrm = rows[ok], nrm[ok]
    pos = np.ascontiguousarray(model["positions"], f32).reshape(-1, 3)[rows]
    tc, ac, hres = f32(q["tilt_cos"]), f32(q["align_cos"]), f32(q["height_res"])
    with np.errstate(all="ignore"):
        p = pos - o[None, :]
        s = _dotv(nrm, u)
        cand = (np.abs(s) >= tc) & (np.abs(p) < f32(512.0)).all(axis=1)
    assert p.dtype == np.float32 and s.dtype == np.float32
    crow, p, s, nrm = rows[cand], p[cand], s[cand], nrm[cand]
    m = np.where((s < 0)[:, None], -nrm, nrm)
    scale = vote_scale(tc)
    ia, ib = _dir_bin(_dotv(m, a), scale), _dir_bin(_dotv(m, b), scale)
    dir_hist = np.bincount(ib * DIR_BINS + ia, minlength=DIR_BINS * DIR_BINS).astype(np.uint32)
    out = dict(status=NO_FLOOR, rounds=0, rows_used=len(rows), candidates=len(crow), direction_rows=0, aligned=0, height_out_of_range=0, height_rows=0,
               dir_bin=(0, 0), height_bin=0, inliers=[0] * MAX_ROUNDS, rms=np.zeros(MAX_ROUNDS, f32), sums=np.zeros((MAX_ROUNDS, 10), np.int64),
               origin=o, z_min=-f32(q["below"]), floor_max=f32(q["step"]), z_max=f32(q["body_height"]), width=int(q["width"]), height=int(q["height"]),
               res=f32(q["res"]), dir_hist=dir_hist.reshape(DIR_BINS, DIR_BINS), height_hist=np.zeros(HEIGHT_BINS, np.uint32), alpha_beta=[],
               inlier_rows=np.zeros(0, np.int64))
    normal, d = u, f32(0.0)

    def stages():
        nonlocal normal, d
        win = direction_winner(dir_hist) if len(crow) else None
        if win is None:
            return
        ia0, ib0, _ = win
        out["dir_bin"] = (ia0, ib0)
        inw = (np.abs(ia - ia0) <= 1) & (np.abs(ib - ib0) <= 1)
        out["direction_rows"] = int(inw.sum())
        S = [int(_quant(m[inw, k], 1048576.0).sum()) for k in range(3)]
        n0 = direction_normal(S)
        if n0 is None:
            return
        normal = n0
        aligned = _dotv(m, n0) >= ac
        with np.errstate(all="ignore"):
            t = np.floor(_dotv(p[aligned], n0) / hres)
        inr = (t >= f32(-1024.0)) & (t < f32(1024.0))
        out["aligned"], out["height_out_of_range"] = int(aligned.sum()), int((~inr).sum())
        hh = np.bincount(t[inr].astype(np.int64) + 1024, minlength=HEIGHT_BINS).astype(np.uint32)
        out["height_hist"] = hh
        hw = height_winner(hh, int(q["min_rows"]), int(q["floor_share256"]))
        if hw is None:
            return
        out["height_bin"], out["height_rows"] = hw
        d = height_of_bin(hw[0], hres)
        out["status"] = OK
        for k in range(int(q["refine_iters"])):
            fr = frame(normal, a)
            if fr is None:
                out["status"] = DEGENERATE
                return
            ak, bk = fr
            dist = f32(q["first_dist"] if k == 0 else q["inlier_dist"])
            z = _dotv(p, normal) - d
            inl = (_dotv(m, normal) >= ac) & (np.abs(z) <= dist)
            x, y, z = _quant(_dotv(p[inl], ak), 1024.0), _quant(_dotv(p[inl], bk), 1024.0), _quant(z[inl], 1024.0)
            words = [int(inl.sum())] + [int(v.sum()) for v in (x, y, z, x * x, x * y, y * y, x * z, y * z, z * z)]
            out["sums"][k] = words
            out["inliers"][k] = words[0]
            out["inlier_rows"] = crow[inl]
            status, n_new, d_new, rms, ab = refine_round(words, int(q["min_rows"]), normal, ak, bk, d)
            out["status"] = status
            if status != OK:
                return
            normal, d = n_new, d_new
            out["rms"][k], out["rounds"] = rms, k + 1
            out["alpha_beta"].append(ab)

    stages()
    out["normal"], out["d"] = normal, f32(d)
    out["camera_height"] = camera_height(pc, normal, d)
    out["pose"] = grid_pose(normal, d, o, pc, a, b, q["width"], q["height"], q["res"])
    return out


def same_fit(got, want, what):
    """every integer, histogram and float of a result (the device's or the C++ program's) against fit()'s, with =="""
    for k in ("status", "rounds", "height_bin", "width", "height") + COUNTS:
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
    assert tuple(got["dir_bin"]) == tuple(want["dir_bin"]), (what, got["dir_bin"], want["dir_bin"])
    assert [int(v) for v in got["inliers"]] == [int(v) for v in want["inliers"]], (what, got["inliers"], want["inliers"])
    assert np.array_equal(np.asarray(got["sums"], np.int64), want["sums"]), (what, "sums", np.argwhere(np.asarray(got["sums"]) != want["sums"]).tolist())
    for k in ("dir_hist", "height_hist"):
        if k in got:
            assert np.array_equal(np.asarray(got[k], np.uint32).ravel(), want[k].ravel()), (what, k)
    for k in FLOATS:
        g, w = np.asarray(got[k], f32).ravel(), np.asarray(want[k], f32).ravel()
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, k, g, w)


# ---- the scenes ----------------------------------------------------------------------------------------------------------------
def tilt_matrix(tilt):
    """the level frame turned as a whole: by tilt[0] degrees about map x, then tilt[1] about map z"""
    return nr.rot("z", tilt[1]) @ nr.rot("x", tilt[0])


def _basis(n, rng):
    """per normal an orthonormal pair (e1, e2) turned at random about it"""
    ref = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    e1 = np.cross(n, ref)
    e1 /= np.linalg.norm(e1, axis=1)[:, None]
    e2 = np.cross(n, e1)
    ang = rng.uniform(0, 2 * np.pi, len(n))[:, None]
    return np.cos(ang) * e1 + np.sin(ang) * e2, -np.sin(ang) * e1 + np.cos(ang) * e2


def room(tilt=(0.0, 0.0), nf=3000, nt=2500, nl=0, nw=1500, nr_=1000, seed=0, flat=False, wall=(3.0, -1.5, 1.0)):
    """A room in a level frame (map y down), turned as a whole by `tilt` about the origin: a floor of nf rows over 6 x 6 m at y = +1 m,
    a table top of nt rows 0.75 m above it, a wall of nw rows (wall: its half width and its span in y), nr_ rows with random normals, nl rows 0.4 m below the floor; normals
    signed at random, normal noise sigma 0.03, height noise 5 mm (flat: neither).  Returns (model, planted) with planted = dict(normal,
    d): the floor's plane normal . c = d with the normal pointing up (against map y before the tilt)."""
    rng = np.random.default_rng(7919 * seed + 13)
    sig_n, sig_h = (0.0, 0.0) if flat else (0.03, 0.005)
    down = np.array([0.0, 1.0, 0.0])

    def horizontal(n, y, half, centre=(0.0, 0.0)):
        pos = np.stack([rng.uniform(-half, half, n) + centre[0], y + rng.normal(0, 1, n) * sig_h, rng.uniform(-half, half, n) + centre[1]], axis=1)
        return pos, np.tile(down, (n, 1))
    parts = [horizontal(nf, 1.0, 3.0), horizontal(nt, 0.25, 0.6, (1.0, 0.5)), horizontal(nl, 1.4, 0.8, (-1.5, -1.0))]
    wall = np.stack([rng.uniform(-wall[0], wall[0], nw), rng.uniform(wall[1], wall[2], nw), 3.0 + rng.normal(0, 1, nw) * sig_h], axis=1)
    wall_pos = wall
    parts.append((wall_pos, np.tile(np.array([0.0, 0.0, 1.0]), (nw, 1))))
    rn = rng.normal(size=(nr_, 3))
    parts.append((np.stack([rng.uniform(-3, 3, nr_), rng.uniform(-1.5, 1.0, nr_), rng.uniform(-3, 3, nr_)], axis=1), rn / np.linalg.norm(rn, axis=1)[:, None]))
    pos = np.concatenate([q[0] for q in parts])
    nrm = np.concatenate([q[1] for q in parts])
    n = len(pos)
    nrm = nrm + rng.normal(0, 1, (n, 3)) * sig_n
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm *= 1.0 if flat else rng.choice([-1.0, 1.0], n)[:, None]
    T = tilt_matrix(tilt)
    pos, nrm = pos @ T.T, nrm @ T.T
    e1, e2 = _basis(nrm, rng)
    order = rng.permutation(n)
    m = dict(positions=pos, colors=rng.uniform(0.0, 255.0, (n, 3)), stamps=np.tile([40, 60], (n, 1)), orientations=np.concatenate([e1, e2, nrm], axis=1),
             shapes=rng.uniform(-1e-3, 1e-3, (n, 6)), dims=rng.uniform(1e-4, 1e-2, (n, 2)), confidences=rng.uniform(1.0, 4.0, n))
    m = {name: np.ascontiguousarray(m[name][order], dt) for name, _, dt in nr.FIELDS}
    up = T @ -down
    return m, dict(normal=up, d=-1.0)


# (name, room keywords, fit keywords, which plane wins: the planted d of it in the level frame, or None for "not the floor")
FLOOR_D, TABLE_D, LOW_D = -1.0, -0.25, -1.4
SCENES = (
    ("tilt 12 -7", dict(tilt=(12.0, -7.0)), dict(), FLOOR_D),
    ("tilt 25 15", dict(tilt=(25.0, 15.0)), dict(), FLOOR_D),
    ("level", dict(tilt=(0.0, 0.0)), dict(), FLOOR_D),
    ("low rows too few", dict(tilt=(20.0, 10.0), nf=800, nl=150), dict(), FLOOR_D),
    ("the table wins", dict(nf=400, nt=2500, nl=60), dict(floor_share256=64), TABLE_D),
    ("a smaller share finds the floor", dict(nf=400, nt=2500, nl=60), dict(floor_share256=26), FLOOR_D),
    ("the low rows win", dict(nf=400, nt=2500, nl=300), dict(floor_share256=26), LOW_D),
)
# past tilt_cos the floor is no candidate, and the wall is one only by the rows whose noisy normals lean towards the hint (40 degrees from
# it, against acos 0.8 = 36.9): a compact, dense wall collects enough of them in one height window
STEEP = ("tilted 50 degrees", dict(tilt=(50.0, 0.0), nw=4000, wall=(0.8, -0.2, 0.8)), dict(), None)
CAMERA = np.array([0.1, -0.05, 0.2], f32)                              # the camera position the CPU tests give the scenes


def flat_floor(n=2000):
    """n rows of one normal (0, -1, 0) and one height (y = 1), on a lattice of exact f32 positions: the contention case and the level floor"""
    k = np.arange(n)
    pos = np.stack([(k % 50) * 0.125 - 3.0, np.ones(n), (k // 50) * 0.125 - 2.0], axis=1)
    m = dict(positions=pos, colors=np.zeros((n, 3)), stamps=np.tile([40, 60], (n, 1)), orientations=np.tile([1, 0, 0, 0, 0, 1, 0, -1, 0], (n, 1)),
             shapes=np.zeros((n, 6)), dims=np.full((n, 2), 4e-3), confidences=np.full(n, 3.0))
    return {name: np.ascontiguousarray(m[name], dt) for name, _, dt in nr.FIELDS}


def lstsq_plane(model, rows):
    """an independent f64 least-squares plane through the positions of `rows`: (unit normal, offset) with normal . c = offset, by
    np.linalg.lstsq in the frame of the rows' principal axes"""
    c = np.asarray(model["positions"], np.float64).reshape(-1, 3)[rows]
    mean = c.mean(axis=0)
    _, _, vt = np.linalg.svd(c - mean, full_matrices=False)
    local = (c - mean) @ vt.T                                         # the third axis is roughly the normal
    A = np.stack([local[:, 0], local[:, 1], np.ones(len(c))], axis=1)
    (al, be, ga), *_ = np.linalg.lstsq(A, local[:, 2], rcond=None)
    n = vt[2] - al * vt[0] - be * vt[1]
    L = np.linalg.norm(n)
    n = n / L
    return n, float(n @ mean + ga / L)
