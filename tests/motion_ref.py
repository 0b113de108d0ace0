"""numpy restatement of include/ssf_motion.h, steps 1-7: every step one float32 operation in the header's order, so the device
outputs are compared at 0 bits.  Two independent forms of the labelling: a union-find over the link arrays (form="uf", the one the
GPU tests use) and a breadth-first flood fill that evaluates the link rule pixel by pixel (form="bfs", the check of the first at
small shapes).  Also the generators of the adversarial images both test files use.  The model depth of ssf_motion_mask comes from
tests/render_ref.py (model_depth)."""
from collections import deque

import numpy as np

import render_ref as rr

f32 = np.float32
INVALID, STATIC, SEED, UNKNOWN = 0, 1, 2, 3
STAT_KEYS = ("n_seed", "n_unknown", "n_components", "n_dynamic_components", "pixels_masked")
RANGE = (0.2, 5.0)                      # the default configuration's range_min / range_max


def default_params(W, H):
    """ssf_motion_default_params (the fields the rule reads)"""
    return dict(front_abs=0.05, front_quad=0.01, link_abs=0.02, link_rel=0.01, min_seeds=max(1, (W * H) // 1024), unknown_per_seed=2)


def convert_depth(depth, depth_scale=None):
    """the depth in metres as the kernels load it (ssf_input.h)"""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        return (depth.astype(np.float64) * float(depth_scale)).astype(f32)
    assert depth.dtype == f32
    return depth


def classify(d, m, z_range, front_abs, front_quad):
    """steps 1 and 2"""
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(d) & (d >= f32(z_range[0])) & (d <= f32(z_range[1]))
        tau = f32(front_abs) + f32(front_quad) * (d * d)
        seed = valid & (m > 0) & ((m - d) > tau)
    unknown = valid & ~seed & (m == 0)
    cls = np.full(d.shape, STATIC, np.uint8)
    cls[~valid] = INVALID
    cls[seed] = SEED
    cls[unknown] = UNKNOWN
    return cls


def _linked(dp, dq, link_abs, link_rel):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(dp - dq) <= f32(link_abs) + f32(link_rel) * np.minimum(dp, dq)


def _labels_uf(d, member, link_abs, link_rel):
    """union-find over the link arrays; the root of a set is kept at its smallest index"""
    H, W = d.shape
    idx = np.arange(H * W).reshape(H, W)
    lh = member[:, 1:] & member[:, :-1] & _linked(d[:, 1:], d[:, :-1], link_abs, link_rel)
    lv = member[1:, :] & member[:-1, :] & _linked(d[1:, :], d[:-1, :], link_abs, link_rel)
    pairs = np.concatenate([np.stack([idx[:, 1:][lh], idx[:, :-1][lh]], 1), np.stack([idx[1:, :][lv], idx[:-1, :][lv]], 1)])
    parent = list(range(H * W))

    def find(i):
        r = i
        while parent[r] != r:
            r = parent[r]
        while parent[i] != r:
            parent[i], i = r, parent[i]
        return r

    for a, b in pairs.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = np.full(H * W, -1, np.int32)
    for i in np.flatnonzero(member.ravel()).tolist():
        label[i] = find(i)
    return label.reshape(H, W)


def _labels_bfs(d, member, link_abs, link_rel):
    """flood fill in row-major order (so a component is first met at its smallest index), the link rule on scalars"""
    H, W = d.shape
    la, lr = f32(link_abs), f32(link_rel)
    label = np.full((H, W), -1, np.int32)
    mem = member.tolist()
    for y0 in range(H):
        for x0 in range(W):
            if not mem[y0][x0] or label[y0, x0] >= 0:
                continue
            lab = y0 * W + x0
            label[y0, x0] = lab
            todo = deque([(y0, x0)])
            while todo:
                y, x = todo.popleft()
                dp = d[y, x]
                for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if 0 <= yy < H and 0 <= xx < W and mem[yy][xx] and label[yy, xx] < 0:
                        dq = d[yy, xx]
                        if f32(abs(f32(dp - dq))) <= f32(la + f32(lr * min(dp, dq))):
                            label[yy, xx] = lab
                            todo.append((yy, xx))
    return label


def segment(depth, model, z_range=RANGE, front_abs=0.05, front_quad=0.01, link_abs=0.02, link_rel=0.01, min_seeds=1, unknown_per_seed=2,
            depth_scale=None, form="uf"):
    """steps 1-7 on two images: dict(mask, label, cls, stats)"""
    d = convert_depth(depth, depth_scale)
    m = np.asarray(model, f32)
    assert d.shape == m.shape
    cls = classify(d, m, z_range, front_abs, front_quad)
    member = (cls == SEED) | (cls == UNKNOWN)
    label = (_labels_uf if form == "uf" else _labels_bfs)(d, member, link_abs, link_rel)
    P = d.size
    lab = label.ravel()
    ns = np.bincount(lab[(cls == SEED).ravel()], minlength=P).astype(np.int64)
    nu = np.bincount(lab[(cls == UNKNOWN).ravel()], minlength=P).astype(np.int64)
    dyn = (ns >= int(min_seeds)) & (nu <= int(unknown_per_seed) * ns)           # (per label; only roots have counts)
    roots = np.flatnonzero(lab == np.arange(P))
    mask = np.zeros(P, np.uint8)
    mask[member.ravel()] = dyn[lab[member.ravel()]]
    stats = dict(n_seed=int((cls == SEED).sum()), n_unknown=int((cls == UNKNOWN).sum()), n_components=int(len(roots)),
                 n_dynamic_components=int(dyn[roots].sum()), pixels_masked=int(mask.sum()))
    return dict(mask=mask.reshape(d.shape), label=label, cls=cls, stats=stats)


def model_depth(model, n_visible, pose12, camera, z_range=RANGE, min_conf=0.0, splat_scale=3.0):
    """m of ssf_motion_mask: render_ref's depth image with visible_only = 0"""
    return rr.render(model, n_visible, pose12, camera, z_range, min_conf, splat_scale, False, "fragments")["depth"]


def assert_same(got, ref, what=""):
    for k in ("mask", "label", "cls"):
        if k in got:
            assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape)
            bad = got[k] != ref[k]
            assert not bad.any(), "%s: %s differs at %d pixels (first %s)" % (what, k, int(bad.sum()), np.argwhere(bad)[0])
    assert got["stats"] == ref["stats"], (what, got["stats"], ref["stats"])


# ---- adversarial images ------------------------------------------------------------------------------------------------
# A pattern image: members at depth 1 m (all neighbouring members link), seeds with the map 1 m behind them, unknowns with no map;
# everything else agrees with the map at 2 m (STATIC).
def from_pattern(member, seed=None):
    member = np.asarray(member, bool)
    seed = member if seed is None else (np.asarray(seed, bool) & member)
    depth = np.where(member, f32(1), f32(2)).astype(f32)
    model = np.full(member.shape, 2, f32)
    model[member & ~seed] = 0
    return depth, model


def serpentine(W, H):
    """a one-pixel corridor over the whole image: one component whose only path is about W * H / 2 long"""
    m = np.zeros((H, W), bool)
    m[0::2, :] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    return m


def spiral(W, H, off, pitch=4):
    m = np.zeros((H, W), bool)
    top, left, bottom, right = off, off, H - 1 - off, W - 1 - off
    x0 = left
    while top <= bottom and x0 <= right:
        m[top, x0:right + 1] = True
        if bottom <= top:
            break
        m[top:bottom + 1, right] = True
        if right - pitch < left:
            break
        m[bottom, left:right + 1] = True
        if bottom - pitch < top + pitch:
            break
        m[top + pitch:bottom + 1, left] = True
        x0 = left
        top, left, bottom, right = top + pitch, left + pitch, bottom - pitch, right - pitch
    return m


def spirals(W, H):
    """two interleaved square spirals, one pixel wide, one pixel apart"""
    return spiral(W, H, 0), spiral(W, H, 2)


def comb(W, H):
    m = np.zeros((H, W), bool)
    m[0, :] = True
    m[:, 0::2] = True
    return m


def checkerboard(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    return (xx + yy) % 2 == 0


def diagonal_blobs(W, H):
    """4 x 4 blobs that touch only diagonally across the tile corners at (32, 32) and (32, 64): four components"""
    m = np.zeros((H, W), bool)
    m[28:32, 28:32] = True
    m[32:36, 32:36] = True
    m[28:32, 64:68] = True
    m[32:36, 60:64] = True
    return m


def cross(W, H):
    """both diagonals as staircases: one component that crosses tile borders in both directions many times"""
    m = np.zeros((H, W), bool)
    prev = 0
    for x in range(W):
        y = x * (H - 1) // (W - 1)
        m[min(prev, y):max(prev, y) + 1, x] = True
        prev = y
    return m | m[:, ::-1]


def ulp_up(v):
    return np.nextafter(f32(v), f32(np.inf))


def cases(W, H, seed=0):
    """(name, depth, model, params) of every hand-built image; params are overrides of default_params(W, H)"""
    rng = np.random.default_rng(seed)
    out = []

    def add(name, member, seed_px=None, **params):
        d, m = from_pattern(member, seed_px)
        out.append((name, d, m, params))

    add("serpentine", serpentine(W, H))
    sa, sb = spirals(W, H)
    add("spirals", sa | sb, sa)                                    # one spiral of seeds, one of unknowns
    add("comb", comb(W, H))
    add("checkerboard", checkerboard(W, H), min_seeds=1)
    add("full", np.ones((H, W), bool))
    add("full_unknown", np.ones((H, W), bool), np.zeros((H, W), bool))
    add("diagonal_blobs", diagonal_blobs(W, H), min_seeds=1)
    add("cross", cross(W, H))
    # random members, random seeds among them
    mem = rng.random((H, W)) < 0.62
    add("random", mem, rng.random((H, W)) < 0.3, min_seeds=3)

    # link threshold: with link_abs = 2^-6, link_rel = 2^-7 and the nearer depth 1 the threshold is 0.0234375, and 1.0234375 - 1 is
    # exactly that: linked; one ulp above is not.  Columns 0 | 1 and 3 | 4 of every row; column 2 and 5.. are static.
    d = np.full((H, W), 2, f32)
    m = np.full((H, W), 2, f32)
    d[:, 0] = 1; d[:, 1] = f32(1.0234375); d[:, 3] = 1; d[:, 4] = ulp_up(1.0234375)
    m[:, [0, 1, 3, 4]] = 0
    d[1::2, :] = 2; m[1::2, :] = 2                                 # (every second row static: the pairs stay pairs)
    out.append(("link_threshold", d, m, dict(link_abs=2.0 ** -6, link_rel=2.0 ** -7, min_seeds=1)))

    # a ramp whose steps hover within a few ulps of the default threshold at every depth
    d = np.empty((H, W), f32)
    for y in range(H):
        v = f32(0.5 + 0.01 * y)
        for x in range(W):
            d[y, x] = v
            step = f32(0.02) + f32(0.01) * v
            v = f32(v + step)
            for _ in range(int(rng.integers(0, 4))):
                v = np.nextafter(v, f32(np.inf) if rng.random() < 0.5 else f32(0))
            if v > 4.5:
                v = f32(0.5 + 0.001 * x)
    d[1::2, :] = 0                                                 # (holes: only the links along a row decide)
    out.append(("link_noise", d, np.zeros((H, W), f32), dict(min_seeds=1)))

    # tau: front_abs = 2^-4, front_quad = 2^-6, d = 1: tau = 0.078125; m - d == tau is no seed, one ulp above is
    d = np.full((H, W), 1, f32)
    m = np.full((H, W), 1, f32)
    m[0::2, 0::2] = f32(1.078125)
    m[0::2, 1::4] = ulp_up(1.078125)
    out.append(("tau_threshold", d, m, dict(front_abs=2.0 ** -4, front_quad=2.0 ** -6, min_seeds=1)))

    # invalid depths inside a region of unknowns and seeds
    d = np.full((H, W), 1, f32)
    m = np.zeros((H, W), f32)
    m[:, : W // 2] = 2
    bad = np.array([np.nan, np.inf, -np.inf, 0.0, -1.0, 0.19999, 5.0001, 1e30, np.nextafter(f32(0.2), f32(0)), np.nextafter(f32(5), f32(9))], f32)
    pick = rng.random((H, W)) < 0.2
    d[pick] = bad[rng.integers(0, len(bad), int(pick.sum()))]
    d[0, 0] = f32(0.2); d[0, 1] = f32(5.0)                         # the ends of the range are valid
    out.append(("invalid_depths", d, m, dict(link_abs=10.0)))

    # min_seeds = 12: a blob of 12 seeds is dynamic, a blob of 11 is not
    mem = np.zeros((H, W), bool)
    mem[2:5, 2:6] = True
    mem[10:13, 30:34] = True; mem[10, 30] = False
    add("min_seeds", mem, min_seeds=12)
    # unknown_per_seed = 3, 5 seeds: 15 unknowns are dynamic, 16 are not (the blobs straddle the tile border at x = 32)
    mem = np.zeros((H, W), bool)
    sd = np.zeros((H, W), bool)
    mem[20, 22:42] = True; sd[20, 22:27] = True                    # 5 + 15
    mem[40, 22:43] = True; sd[40, 38:43] = True                    # 5 + 16
    add("unknown_per_seed", mem, sd, min_seeds=1, unknown_per_seed=3)
    return out


# the tile grids cases()' shapes do not have: one row of tiles (only vertical borders), one column (only horizontal ones), a single
# tile (no merge launch), and a last tile one cell wide
TILE_SHAPES = [(70, 24), (24, 70), (24, 24), (33, 33)]


def tile_cases(W, H, seed=0):
    """(name, depth, model, params) of the patterns that stress the labelling, every component counted (min_seeds = 1)"""
    rng = np.random.default_rng(seed)
    sa, sb = spirals(W, H)
    mem = rng.random((H, W)) < 0.62
    patterns = [("serpentine", serpentine(W, H), None), ("comb", comb(W, H), None), ("cross", cross(W, H), None),
                ("checkerboard", checkerboard(W, H), None), ("full", np.ones((H, W), bool), None), ("spirals", sa | sb, sa),
                ("random", mem, rng.random((H, W)) < 0.3)]
    return [(name,) + from_pattern(member, seed_px) + (dict(min_seeds=1),) for name, member, seed_px in patterns]


# ---- the end-to-end scene: the synthetic room with a box pasted in front of it -----------------------------------------
def box_rect(W, H):
    """(y0, y1, x0, x1) of the pasted box"""
    return H // 4, H // 4 + H // 3, W // 3, W // 3 + W // 4


def box_scene(k, W, H):
    """frame k of the synthetic orbit (util.frame's) with a flat box pasted half a metre in front of the nearest surface behind
    it: (rgb, depth, the scene's noise-free depth without the box, rect).  The depth step at the box's edge is >= 0.5 m, far
    above the link threshold (at most 0.07 m inside the range), so the box is cut off from everything around it."""
    from supersurfel_fusion_amd import synthetic
    R, t = synthetic.orbit_pose(k)
    rgb, depth, _ = synthetic.render(R, t, W, H, noise=True, rng=np.random.default_rng(1000 + k))
    clean = synthetic.render(R, t, W, H, noise=False)[1]
    y0, y1, x0, x1 = box_rect(W, H)
    rgb, depth = rgb.copy(), depth.copy()
    depth[y0:y1, x0:x1] = f32(clean[y0:y1, x0:x1].min() - 0.5)
    rgb[y0:y1, x0:x1] = (200, 40, 40)
    return rgb, depth, clean, (y0, y1, x0, x1)
