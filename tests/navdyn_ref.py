"""A restatement of include/ssf_navdyn.h.  It shares no code with the library.

Part A, the rollouts with movers: the loop of tests/navsteer_ref.py / tests/navfoot_ref.py (their lattice, direction table, traversable
rule, sweep of heading bins and parameter names) with the mover test after the static test, the gap, the sixth score term and the
three new outputs.  The candidates of a pose are vectorised in int64 (the header proves D2 < 2^53); the floor square root is
math.isqrt on Python ints.
Part B, the blobs: the back-projection of tests/navlive_ref.py (point_cells, restated here because the position in the cell is
needed, and checked against it), then Python ints per label.
Part C, the tracker: Python ints.

Also here: the scenes tests/test_navdyn.py and tests/test_navdyn_gpu.py share."""
import math

import numpy as np

import navfoot_ref as fr
import navlive_ref as lr
import navsteer_ref as sr

f32 = np.float32
SUB, TURN, NO_COST = sr.SUB, sr.TURN, sr.NO_COST
_C, _S = sr.direction_table()
MAX_MOVERS, MOVER_WORDS, MAX_BLOBS, BLOB_WORDS = 64, 6, 64, 8
MAX_XY, MAX_V, MAX_R, MAX_GROW, MAX_CAP = 1 << 24, 4096, 1 << 20, 4096, 65536
DYN_OUTPUTS = ("cand_hit", "cand_min_gap", "best_min_gap")
OUTPUTS = sr.OUTPUTS + DYN_OUTPUTS
DTYPES = dict(sr.DTYPES, cand_hit=np.int32, cand_min_gap=np.int32, best_min_gap=np.int32)
STATS = sr.STATS + ("hit_movers",)                                     # the exact ones
DYN_DEFAULTS = dict(mover_cap=4096, mover_weight=1)


def params(**kw):
    """navsteer_ref.params with mover_cap and mover_weight"""
    dyn = {k: kw.pop(k) for k in list(kw) if k in DYN_DEFAULTS}
    return dict(sr.params(**kw), **dict(DYN_DEFAULTS, **dyn))


def movers_ok(movers):
    """the header's bounds on a host list"""
    m = np.asarray(movers, np.int64).reshape(-1, MOVER_WORDS)
    return bool(len(m) <= MAX_MOVERS and (np.abs(m[:, :2]) <= MAX_XY).all() and (np.abs(m[:, 2:4]) <= MAX_V).all() and (m[:, 4] >= 0).all()
                and (m[:, 4] <= MAX_R).all() and (m[:, 5] >= 0).all() and (m[:, 5] <= MAX_GROW).all())


WRONG_RULES = ("hit_le", "movers_first", "last_hit", "gap_uncommitted", "zero_based", "start_tested")


def rollouts(grid, dist2, cost, poses, targets, movers, c, B=None, _wrong=None):
    """every output of ssf_navdyn_rollouts (B None: grid is state) or ssf_navdyn_foot_rollouts (B: the heading bins; grid is free_mask)
    in the ABI's dtypes (best_traj entries past best_len are 0 here and unwritten there) and 'stats'.  c: params().
    _wrong (tests/test_navdyn.py only): one of WRONG_RULES, a rule the header does NOT state, swapped in for the one it does, to show
    on the CPU which scenes would tell the two apart"""
    assert _wrong is None or _wrong in WRONG_RULES, _wrong
    grid = np.asarray(grid)
    H, W = grid.shape
    dist2 = np.asarray(dist2).astype(np.int64)
    d = np.minimum(np.maximum(dist2, 0), c["clearance_cap"])
    if B is None:
        trav, _ = sr.traversable(grid, dist2, c)
    else:
        mask, roomy = grid.astype(np.int64), dist2 >= c["min_dist2"]
        shift, half = fr.bins(B)
    movers = np.asarray(movers if movers is not None else [], np.int64).reshape(-1, MOVER_WORDS)
    assert movers_ok(movers)
    poses = np.asarray(poses, np.int64).reshape(-1, 3)
    n, T, cap = len(poses), c["n_steps"], c["mover_cap"]
    v, w, vmax = sr.lattice(c)
    K = len(v)
    av, aw = np.abs(v), np.abs(w)
    if c["cost_weight"] > 0:
        cost = np.asarray(cost).astype(np.int64)
    if c["target_weight"] > 0:
        targets = np.asarray(targets, np.int64).reshape(-1, 2)
    need_steps = np.minimum(T, c["min_free_steps"] + ((av + c["brake_div"] - 1) // c["brake_div"] if c["brake_div"] > 0 else 0))

    def ok(ix, iy, need):              # traversable (under need); outside the grid: not
        inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        cy, cx = np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)
        if B is None:
            return inside & trav[cy, cx]
        return inside & ((mask[cy, cx] & need) == need) & roomy[cy, cx]

    def sweep(h):                      # the footprint's need of every candidate's step from its heading h
        if B is None:
            return None
        a = h + half
        lo, hi = np.minimum(a, a + w) >> shift, np.maximum(a, a + w) >> shift
        need = np.zeros(K, np.int64)
        for k in range(int((hi - lo).max()) + 1):
            need |= np.where(lo + k <= hi, np.int64(1) << ((lo + k) & (B - 1)), 0)
        return need

    out = dict(best=np.full(n, -1), best_cmd=np.zeros((n, 2)), best_score=np.full(n, -1), n_admissible=np.zeros(n), pose_status=np.zeros(n),
               best_len=np.zeros(n), best_traj=np.zeros((n, T + 1, 3)), cand_free=np.zeros((n, K)), cand_min_d=np.full((n, K), -1),
               cand_end=np.zeros((n, K, 3)), cand_end_cost=np.full((n, K), NO_COST), cand_score=np.full((n, K), -1),
               cand_hit=np.full((n, K), -1), cand_min_gap=np.full((n, K), -1), best_min_gap=np.full(n, -1))
    out = {nm: a.astype(np.int64) for nm, a in out.items()}
    staged = glob = 0
    R, stage = sr.reach(c), (sr.stage_cells(dict(c, n_poses=n)) if B is None else 0)
    for q in range(n):
        px, py, ph = int(poses[q, 0]), int(poses[q, 1]), int(poses[q, 2]) & 0xFFFF
        cx, cy = px >> 10, py >> 10
        out["cand_end"][q] = (px, py, ph)
        if not (0 <= cx < W and 0 <= cy < H):
            out["pose_status"][q] = 1
            continue
        if not ok(np.int64(cx), np.int64(cy), None if B is None else np.int64(1) << fr.bin_of(ph, B)):
            out["pose_status"][q] = 2
            continue
        chunks = -(-K // 256)
        window = (min(cx + R, W - 1) - max(cx - R, 0) + 1) * (min(cy + R, H - 1) - max(cy - R, 0) + 1)
        if window <= stage:
            staged += chunks
        else:
            glob += chunks
        x, y, h = np.full(K, px), np.full(K, py), np.full(K, ph)
        free, min_d, alive = np.zeros(K, np.int64), np.full(K, d[cy, cx]), np.ones(K, bool)
        hit, gap = np.full(K, -1, np.int64), np.full(K, cap, np.int64)
        traj = np.zeros((K, T + 1, 3), np.int64)
        traj[:, 0] = (px, py, ph)
        if _wrong == "start_tested":                                    # (wrong: the start is tested like a step, against R_0)
            for m in range(len(movers) - 1, -1, -1):
                mx, my, _, _, mr, _ = (int(e) for e in movers[m])
                if (px - mx) ** 2 + (py - my) ** 2 < mr * mr:
                    hit[:], alive[:] = m, False
        for s in range(1, T + 1):                                       # s: the step being attempted, 1-based
            k = ((2 * h + w + 64) >> 7) & 1023
            nx, ny = x + ((v * _C[k] + 8192) >> 14), y + ((v * _S[k] + 8192) >> 14)
            ox, oy, ncx, ncy = x >> 10, y >> 10, nx >> 10, ny >> 10
            need = sweep(h)
            step = ok(ncx, ncy, need)
            diag = (ncx != ox) & (ncy != oy)
            step &= ~diag | (ok(ncx, oy, need) & ok(ox, ncy, need))
            step &= alive
            # the movers, after the static test: the smallest m with D2 < R_s^2 ends the rollout
            g = gap.copy()
            at = s - 1 if _wrong == "zero_based" else s                  # (wrong: the movers of the step before)
            for m in range(len(movers) - 1, -1, -1):                    # (downwards, so that the smallest hitting m is written last)
                mx, my, mvx, mvy, mr, mg = (int(e) for e in movers[m])
                X, Y, Rs = mx + at * mvx, my + at * mvy, mr + at * mg
                D2 = (nx - X) ** 2 + (ny - Y) ** 2
                assert int(D2.max()) < 1 << 53 and Rs * Rs < 1 << 43
                inside = step & (D2 < Rs * Rs)
                if _wrong == "hit_le":                                  # (wrong: a touching disc hits)
                    inside = step & (D2 <= Rs * Rs)
                if _wrong == "movers_first":                            # (wrong: a step the static test refuses is still charged to a mover)
                    inside = alive & (D2 < Rs * Rs)
                if _wrong == "last_hit":                                # (wrong: downwards, the first one written stays: the largest m)
                    inside &= hit < 0
                hit = np.where(inside, m, hit)
                for i in np.flatnonzero(step & ~inside & (D2 < (g + Rs) ** 2)):
                    g[i] = math.isqrt(int(D2[i])) - Rs
            if _wrong == "gap_uncommitted":                             # (wrong: the gaps of a step that a mover refuses count as well)
                gap = np.where(step, g, gap)
            step &= hit < 0
            alive &= step
            if not alive.any():
                break
            gap = np.where(alive, g, gap)                               # (a committed step's gaps count)
            x, y, h = np.where(alive, nx, x), np.where(alive, ny, y), np.where(alive, (h + w) & 0xFFFF, h)
            free += alive
            dn = d[np.clip(y >> 10, 0, H - 1), np.clip(x >> 10, 0, W - 1)]
            min_d = np.where(alive, np.minimum(min_d, dn), min_d)
            traj[alive, s] = np.stack([x, y, h], axis=1)[alive]
        assert (gap >= 0).all() and (gap <= cap).all()
        ec = cost[y >> 10, x >> 10] if c["cost_weight"] > 0 else np.full(K, NO_COST)
        adm = free >= need_steps
        if c["cost_weight"] > 0:
            adm &= ec != NO_COST
        score = c["clear_weight"] * (c["clearance_cap"] - min_d) + c["speed_weight"] * (vmax - av) + c["turn_weight"] * aw
        score = score + c["mover_weight"] * ((10 * (cap - gap)) >> 10)
        if c["cost_weight"] > 0:
            score = score + c["cost_weight"] * ec
        if c["target_weight"] > 0:
            dx, dy = np.abs(x - targets[q, 0]), np.abs(y - targets[q, 1])
            score = score + c["target_weight"] * ((10 * np.maximum(dx, dy) + 4 * np.minimum(dx, dy)) >> 10)
        score = np.where(adm, score, -1)
        out["cand_free"][q], out["cand_min_d"][q], out["cand_end_cost"][q], out["cand_score"][q] = free, min_d, ec, score
        out["cand_end"][q] = np.stack([x, y, h], axis=1)
        out["cand_hit"][q], out["cand_min_gap"][q] = hit, gap
        out["n_admissible"][q] = adm.sum()
        if not adm.any():
            out["pose_status"][q] = 3
            continue
        cands = np.flatnonzero(adm)
        b = int(cands[np.lexsort((cands, score[cands]))[0]])              # the smallest (score, c)
        out["best"][q], out["best_cmd"][q], out["best_score"][q] = b, (v[b], w[b]), score[b]
        out["best_len"][q] = free[b] + 1
        out["best_traj"][q, :free[b] + 1] = traj[b, :free[b] + 1]
        out["best_min_gap"][q] = gap[b]
    st = out["pose_status"]
    stats = dict(poses_ok=int((st == 0).sum()), poses_blocked=int(((st == 1) | (st == 2)).sum()), poses_stuck=int((st == 3).sum()),
                 candidates=n * K, admissible=int(out["n_admissible"].sum()), collided=int((out["cand_free"] < T).sum()),
                 steps_taken=int(out["cand_free"].sum()), windows_staged=staged, windows_global=glob, hit_movers=int((out["cand_hit"] >= 0).sum()))
    res = {nm: out[nm].astype(DTYPES[nm]) for nm in OUTPUTS}
    res["stats"] = stats
    return res


# ---- part B: the blobs -----------------------------------------------------------------------------------------------------------------
BLOB_STATS = ("pixels_member", "pixels_valid", "points_in_band", "labels_seen", "blobs_kept", "blobs_written")
BLOB_DEFAULTS = dict(min_points=16, max_blobs=64)


def grid_points(d, cam_pose, grid_pose, c):
    """ssf_navlive.h step 2 for every pixel of d (H x W f32), as navlive_ref.point_cells words it: (gx, gy, ok) with ok = in the grid
    and in the band"""
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
    return gx, gy, ok


def ceil_sqrt(a):
    r = math.isqrt(a)
    return r if r * r == a else r + 1


def blobs(depth, mask, label, grid_pose, cam_pose, c, min_points=16, max_blobs=64, depth_format="f32", depth_scale=1.0):
    """dict(blobs: k x 8 int32, stats) of ssf_navdyn_blobs.  c: navlive_ref.params (grid, band, camera, range)"""
    ch, cw = int(c["cam_height"]), int(c["cam_width"])
    d = lr.metres(depth, depth_format, depth_scale).reshape(ch, cw)
    mask, label = np.asarray(mask).reshape(ch, cw), np.asarray(label).astype(np.int64).reshape(ch, cw)
    member = (mask != 0) & (label >= 0) & (label < cw * ch)
    valid = member & lr.valid_pixels(d, c)
    gx, gy, ok = grid_points(d, cam_pose, grid_pose, c)
    contrib = valid & ok
    with np.errstate(all="ignore"):
        bx, by = (gx * f32(1024.0)), (gy * f32(1024.0))
    acc = {}
    for vv, uu in np.argwhere(contrib):
        x, y = int(bx[vv, uu]), int(by[vv, uu])
        assert 0 <= x < int(c["width"]) * 1024 and 0 <= y < int(c["height"]) * 1024
        a = acc.setdefault(int(label[vv, uu]), [0, 0, 0, x, x, y, y])
        a[0] += 1; a[1] += x; a[2] += y
        a[3], a[4], a[5], a[6] = min(a[3], x), max(a[4], x), min(a[5], y), max(a[6], y)
    kept = sorted((-a[0], L) for L, a in acc.items() if a[0] >= min_points)
    rows = []
    for _, L in kept[:max_blobs]:
        n, sx, sy, x0, x1, y0, y1 = acc[L]
        cx, cy = sx // n, sy // n
        ex, ey = max(cx - x0, x1 - cx), max(cy - y0, y1 - cy)
        rows.append((L, n, cx, cy, ceil_sqrt(ex * ex + ey * ey), ex, ey, 0))
    stats = dict(pixels_member=int(member.sum()), pixels_valid=int(valid.sum()), points_in_band=int(contrib.sum()), labels_seen=len(acc),
                 blobs_kept=len(kept), blobs_written=len(rows))
    return dict(blobs=np.array(rows, np.int32).reshape(-1, BLOB_WORDS), stats=stats)


# ---- part C: the tracker ---------------------------------------------------------------------------------------------------------------
class Tracker:
    def __init__(self, gate=2048, inflate=0, grow=16, grow_unmatched=128):
        self.gate, self.inflate, self.grow, self.grow_unmatched, self.prev = gate, inflate, grow, grow_unmatched, []

    def update(self, table, steps_since=1):
        table = [[int(e) for e in row] for row in np.asarray(table, np.int64).reshape(-1, BLOB_WORDS)]
        clamp = lambda val, lo, hi: max(lo, min(hi, val))
        taken, out = set(), []
        for row in table:
            cx, cy, r = row[2], row[3], row[4]
            cands = sorted(((cx - p[2]) ** 2 + (cy - p[3]) ** 2, j) for j, p in enumerate(self.prev) if j not in taken)
            cands = [e for e in cands if e[0] <= self.gate ** 2]
            if cands:
                j = cands[0][1]
                taken.add(j)
                vx, vy, grow = (cx - self.prev[j][2]) // steps_since, (cy - self.prev[j][3]) // steps_since, self.grow
            else:
                vx, vy, grow = 0, 0, self.grow_unmatched
            out.append((clamp(cx, -MAX_XY, MAX_XY), clamp(cy, -MAX_XY, MAX_XY), clamp(vx, -MAX_V, MAX_V), clamp(vy, -MAX_V, MAX_V),
                        clamp(r + self.inflate, 0, MAX_R), clamp(grow, 0, MAX_GROW)))
        self.prev = table
        return np.array(out, np.int32).reshape(-1, MOVER_WORDS)


# the case list the Python tracker and ssf.hpp's share (tests/cpp/navdyn_smoke.cpp holds the same numbers): (gate, inflate, grow,
# grow_unmatched), then (steps_since, table rows as (label, n, cx, cy, r, ex, ey, 0)) per update
TRACKER_CASES = (
    ((2048, 300, 16, 128), ((1, ((5, 40, 10000, 20000, 700, 500, 500, 0),)),
                            (2, ((9, 44, 10301, 19499, 650, 400, 500, 0),)),                          # matched: floor of 301 / 2 and -501 / 2
                            (1, ((9, 44, 20000, 19499, 650, 400, 500, 0),)))),                        # outside the gate: unmatched
    ((1000, 0, 5, 50), ((1, ((1, 9, 0, 0, 10, 1, 1, 0), (2, 8, 600, 0, 10, 1, 1, 0))),
                        (3, ((7, 9, 300, 0, 10, 1, 1, 0), (8, 9, 300, 1, 10, 1, 1, 0), (9, 9, 5000, 5000, 10, 1, 1, 0))))),   # a tie: index 0 wins, then 1
    ((1 << 25, 1 << 20, 4096, 4096), ((1, ((1, 1, -(1 << 23), 1 << 23, 1 << 20, 0, 0, 0),)),
                                      (1, ((1, 1, 1 << 23, -(1 << 23), 1 << 20, 0, 0, 0),)))),        # matched across the whole square: every clamp
)


def tracker_case(k):
    """the mover lists of TRACKER_CASES[k], one per update"""
    cfg, updates = TRACKER_CASES[k]
    t = Tracker(*cfg)
    return [t.update(np.array(rows, np.int64), steps) for steps, rows in updates]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def hand_scene(r):
    """the issue's hand case: an open 21 x 21 grid, the pose at the centre of cell (10, 10) heading 0, v in {0, 512}, w = 0, one
    mover coming down the column the fast candidate reaches"""
    W = H = 21
    state = np.zeros((H, W), np.int8)
    dist2 = np.full((H, W), 64, np.int32)
    c = params(width=W, height=H, n_poses=1, n_v=2, n_w=1, v_min=0, v_step=512, w_min=0, w_step=0, n_steps=12, min_free_steps=2, brake_div=128,
               cost_weight=0)
    return dict(state=state, dist2=dist2, cost=None, poses=np.array([sr.centre(10, 10, 0)], np.int32), targets=None,
                movers=np.array([(14848, 12800, 0, -256, r, 0)], np.int32), c=c)


X0 = Y0 = 10 * SUB + 512                                                # hand_scene's pose
# name -> (heading, movers, wall cells (ix, iy)) on hand_scene: the fast candidate advances exactly 512 a step along a heading that is
# a multiple of a quarter turn, so D2 == R_s^2 can be met.  tests/test_navdyn.py states what each must give, by hand
HAND_SCENES = {
    "touch static": (0, [(X0 + 512 * 6 + 1000, Y0, 0, 0, 1000, 0)], ()),
    "touch growing": (0, [(X0 + 2560 + 500, Y0, 0, 0, 0, 100)], ()),
    "touch pythagorean": (0, [(X0 + 512 * 3 + 600, Y0 + 800, 0, 0, 1000, 0)], ()),
    "touch quarter turn": (16384, [(X0, Y0 + 512 * 6 + 1000, 0, 0, 1000, 0)], ()),
    # the mover walks towards the robot at 256 a step: the two close at 768 a step and touch at step 4; it touches the standing
    # candidate at step 12, the last
    "touch moving": (0, [(X0 + 768 * 4 + 700, Y0, -256, 0, 700, 0)], ()),
    # the cell (13, 10) is a wall and lies inside the disc; the fast candidate's step 5 enters both: the static test answers
    "wall inside a disc": (0, [(13 * SUB + 512, Y0, 0, 0, 800, 0)], ((13, 10),)),
    # mover 1 refuses step 6; at that refused step mover 0 is nearer than it is at any committed step
    "gap of a refused step": (0, [(X0 + 512 * 6, Y0 + 1300, 0, 0, 1000, 0), (X0 + 512 * 6 + 900, Y0, 0, 0, 1000, 0)], ()),
}
HAND_CASES = tuple(HAND_SCENES)


def hand_made(name):
    heading, movers, walls = HAND_SCENES[name]
    s = hand_scene(0)
    for ix, iy in walls:
        s["state"][iy, ix] = 100
    s["poses"] = np.array([sr.centre(10, 10, heading)], np.int32)
    return _with(s, movers)


def random_movers(W, H, m, seed, r_max=1500):
    """m movers inside and around a W x H grid, walking at up to half a cell a step"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(-2 * SUB, (W + 2) * SUB, m), rng.integers(-2 * SUB, (H + 2) * SUB, m), rng.integers(-512, 513, m),
                     rng.integers(-512, 513, m), rng.integers(0, r_max, m), rng.integers(0, 64, m)], axis=1).astype(np.int32)


# name -> (steering scene of navsteer_ref, keywords that override its lattice, mover list maker, dyn keywords).
# Grids 1 x 1, 1 x 70, 37 x 53, 64 x 65, 97 x 33; K = 297 and 512; n_steps 1 and 256; n_poses 1, 70 and 300.  A footprint's scene
# carries its own (foot, B): B = 1, 4, 8, 16, 32
K297 = dict(n_v=9, n_w=33)                                              # the default lattice: 297 candidates
K512 = dict(n_v=8, n_w=64, v_min=-128, v_step=128, w_min=-2016, w_step=64)


def _grid_scene(W, H, n_poses, seed, **kw):
    """a room of navsteer_ref with n_poses poses: its hand-placed ones first, then random ones"""
    c = params(width=W, height=H, n_poses=n_poses, **kw)
    state = sr.room(W, H, seed)
    if W < 8 or H < 8:
        state = np.zeros((H, W), np.int8)
    dist2 = sr.clearance(state)
    goal = (W - 10, H // 2) if W >= 16 and H >= 8 else (W - 1, H - 1)
    cost = sr.field(state, dist2, goal, c)
    rng = np.random.default_rng(500 + seed)
    poses = [sr.centre(W // 2, H // 2 + (2 if H >= 8 else 0), 65535), sr.centre(W // 2, H // 2, 16384)]
    if W >= 8 and H >= 8:
        poses += [sr.centre(3, 3, 1234), sr.centre(W // 3 + 1, H // 3 + 1, 0), (-5, 700, 0), sr.centre(1, 1, 8192)]
    while len(poses) < n_poses:
        poses.append((int(rng.integers(0, W * SUB)), int(rng.integers(0, H * SUB)), int(rng.integers(-TURN, 2 * TURN))))
    poses = np.array(poses[:n_poses], np.int32)
    targets = np.stack([rng.integers(0, W * SUB, n_poses), rng.integers(0, H * SUB, n_poses)], axis=1).astype(np.int32)
    return dict(state=state, dist2=dist2, cost=cost, poses=poses, targets=targets, c=c)


def _with(scene, movers):
    assert movers_ok(movers)
    return dict(scene, movers=np.asarray(movers, np.int32).reshape(-1, MOVER_WORDS))


def _centre_of(scene, q=0):
    return int(scene["poses"][q, 0]), int(scene["poses"][q, 1])


def make_scene(name):
    if name == "1x1":
        s = _grid_scene(1, 1, 1, 1, n_steps=4, n_v=3, n_w=3, v_min=-300, v_step=300, w_min=-100, w_step=100, min_free_steps=0, brake_div=0,
                        cost_weight=0, mover_cap=0)
        return _with(s, [(512, 900, 0, -64, 100, 1)])
    if name == "1x70 K297 one mover":
        s = _grid_scene(70, 1, 1, 2, n_steps=32, **K297)
        x, y = _centre_of(s)
        return _with(s, [(x + 9 * SUB, y, -256, 0, 700, 8)])
    if name == "37x53 K512 64 movers 70 poses":
        return _with(_grid_scene(37, 53, 70, 3, n_steps=24, target_weight=1, mover_weight=7, mover_cap=3000, **K512), random_movers(37, 53, 64, 11))
    if name == "64x65 K297 T256":
        return _with(_grid_scene(64, 65, 3, 4, n_steps=256, min_free_steps=4, mover_cap=65536, **dict(K297, v_step=16)),
                     random_movers(64, 65, 12, 12, r_max=2500))
    if name == "97x33 K512 T1":
        s = _grid_scene(97, 33, 70, 5, n_steps=1, min_free_steps=1, brake_div=0, **K512)
        return _with(s, random_movers(97, 33, 16, 13, r_max=2500))
    if name == "r 0 never hits":
        s = _grid_scene(37, 53, 2, 6, n_steps=24, **K297)
        x, y = _centre_of(s)
        return _with(s, [(x + 3 * SUB, y, -64, 0, 0, 0), (x, y + 2 * SUB, 0, -128, 0, 0)])
    if name == "two movers one step":
        s = _grid_scene(37, 53, 1, 7, n_steps=24, **K297)
        x, y = _centre_of(s)
        # movers 1 and 2 are the same disc, so they hit at the same steps; mover 0 is far away: the smaller index of the two wins
        return _with(s, [(50 * SUB, 70 * SUB, 0, 0, 100, 0), (x + 6 * SUB, y, -128, 0, 1000, 0), (x + 6 * SUB, y, -128, 0, 1000, 0)])
    if name == "mover on the start":
        s = _grid_scene(37, 53, 2, 8, n_steps=24, **K297)
        x, y = _centre_of(s)
        return _with(s, [(x, y, 0, 0, 300, 0)])
    if name == "int64 path":
        s = _grid_scene(37, 53, 2, 9, n_steps=256, mover_cap=65536, **dict(K297, v_step=24))
        e = 1 << 24
        x, y = _centre_of(s)
        # four at the corners of the allowed square, at full speed and radius (they never arrive: the large operands only); a disc of
        # radius 2^20 whose edge stands three cells from the pose; a small one that arrives at 4096 a step around step 40
        return _with(s, [(e, e, -4096, -4096, 1 << 20, 0), (-e, -e, 4096, 4096, 1 << 20, 0), (e, -e, -4096, 4096, 1 << 20, 0),
                         (-e, e, 4096, -4096, 1 << 20, 4096), (x + (1 << 20) + 3000, y, 0, 0, 1 << 20, 0),
                         (x + 40 * 4096 + 5000, y + 300, -4096, 0, 500, 0)])
    if name == "grow 4096":
        s = _grid_scene(64, 65, 2, 10, n_steps=32, mover_cap=65536, mover_weight=1000, **K297)
        x, y = _centre_of(s)
        return _with(s, [(x + 40 * SUB, y + 30 * SUB, 0, 0, 0, 4096)])
    if name == "cap 0":
        return _with(_grid_scene(37, 53, 4, 11, n_steps=24, mover_cap=0, mover_weight=1000, **K297), random_movers(37, 53, 8, 14))
    if name == "300 poses K64":
        # more poses than one pick workgroup holds: the second one's lanes replay their winners against the list in global memory
        return _with(_grid_scene(37, 53, 300, 13, n_steps=12, n_v=4, n_w=16, v_min=128, v_step=128, w_min=-1920, w_step=256, mover_weight=5),
                     random_movers(37, 53, 12, 16))
    if name == "mixed walks":
        return mixed_scene()
    if name in HAND_SCENES:
        return hand_made(name)
    # the footprint's: (footprint, B) with the scene
    if name == "foot 37x53":
        s = _with(_grid_scene(37, 53, 8, 12, n_steps=24, mover_weight=3, **dict(K297, w_min=-8192, w_step=512)), random_movers(37, 53, 16, 15))
        return dict(s, foot=FOOT, B=16)
    if name == "foot B1 point":
        s = _with(_grid_scene(37, 53, 8, 14, n_steps=24, mover_weight=3, **dict(K297, w_min=-8192, w_step=512)), random_movers(37, 53, 16, 17))
        return dict(s, foot=fr.POINT, B=1)
    if name == "foot B32 K512 64 movers":
        s = _with(_grid_scene(37, 53, 8, 15, n_steps=24, target_weight=1, mover_weight=7, mover_cap=3000, **K512), random_movers(37, 53, 64, 18))
        return dict(s, foot=BODY, B=32)
    if name == "foot 300 poses K257":
        s = _with(_grid_scene(64, 65, 300, 16, n_steps=8, n_v=1, n_w=257, v_min=700, v_step=0, w_min=-2048, w_step=16), random_movers(64, 65, 12, 19))
        return dict(s, foot=BODY, B=16)
    if name == "foot T256":
        s = _grid_scene(64, 65, 3, 17, n_steps=256, min_free_steps=4, mover_cap=65536, **dict(K297, v_step=16))
        return dict(_with(s, random_movers(64, 65, 12, 20, r_max=2500)), foot=BODY, B=8)
    if name == "foot 1x1 B4":
        return dict(make_scene("1x1"), foot=fr.POINT, B=4)
    raise KeyError(name)


def mixed_scene():
    """navsteer_ref.mixed_scene (1281 workgroups, of which the launch stages the windows of up to 4056 cells and walks the others) among
    ten movers, with 60 of its live poses: the others stand outside the grid, where they end at once but still count as workgroups"""
    s = sr.mixed_scene()
    live = 4 + 60
    poses = s["poses"].copy()
    poses[live:4 + sr.MIXED_LIVE] = [((-3 - k) * SUB, 5 * SUB, k) for k in range(4 + sr.MIXED_LIVE - live)]
    c = dict(s["c"], **DYN_DEFAULTS)
    return _with(dict(s, poses=poses, c=c), random_movers(78, 120, 10, 21, r_max=2500))


def staging_scene(W, H, n_poses):
    """the scene of the tests of a call's host arrays, for the four rollouts: a lattice of 21 candidates over 10 steps among three
    movers on a W x H floor, with a cost, targets and the small body (on one cell: the point) at 8 bins.  From 8 x 8 cells on the floor is walled in, with a
    pillar in the middle and one unknown cell; the first pose then faces the wall from two cells away, so that its winner stops
    before the horizon, and the first mover stands in the way of the second pose"""
    def make():
        c = params(width=W, height=H, n_poses=n_poses, n_steps=10, n_v=3, n_w=7, v_min=0, v_step=384, w_min=-3072, w_step=1024, min_free_steps=1,
                   brake_div=0, target_weight=1, mover_weight=3)
        state = np.zeros((H, W), np.int8)
        room = W >= 8 and H >= 8
        if room:
            state[0, :] = state[-1, :] = state[:, 0] = state[:, -1] = 100
            state[H // 2 - 1:H // 2 + 1, W // 2:W // 2 + 2] = 100
            state[H - 2, 1] = -1
        dist2 = sr.clearance(state)
        cost = sr.field(state, dist2, (W - 3, 2) if room else (0, 0), c)
        rng = np.random.default_rng(40 + W + H)
        poses = [sr.centre(2, H // 2, 32768), sr.centre(W // 4, H // 4 + 1, 0), sr.centre(W - 3, H - 3, 16384 + 65536), (-5, 700, 0)] if room else \
                [sr.centre(0, 0, 0), (1023, 0, 16384), (0, 1023, 65535), (-1, 0, 0)]
        while len(poses) < n_poses:
            poses.append((int(rng.integers(0, W * SUB)), int(rng.integers(0, H * SUB)), int(rng.integers(-TURN, 2 * TURN))))
        poses = np.array(poses[:n_poses], np.int32)
        targets = np.stack([rng.integers(0, W * SUB, n_poses), rng.integers(0, H * SUB, n_poses)], axis=1).astype(np.int32)
        x, y, _ = sr.centre(W // 4, H // 4 + 1) if room else (512, 900, 0)
        movers = np.vstack([[(x + (3 * SUB if room else 0), y, -128 if room else 0, -64, 600, 8)], random_movers(W, H, 2, 41)])
        foot = BODY if room else fr.POINT                               # (the body does not fit on a floor of one cell)
        s = dict(_with(dict(state=state, dist2=dist2, cost=cost, poses=poses, targets=targets, c=c), movers), foot=foot, B=8)
        s["layers"] = fr.layers(state, 0, foot, 8)                       # (what ssf_navfoot_layers makes of the floor: tests/test_navfoot_gpu.py)
        s["free_mask"] = s["layers"]["free_mask"]
        return s
    return cached(("staging", W, H, n_poses), make)


def staging_reference(W, H, n_poses, kind):
    """the restatement's answer to staging_scene: kind 'disc' (navsteer_ref), 'foot' (navfoot_ref), 'dyn' or 'dyn foot' (this file)"""
    def make():
        s = staging_scene(W, H, n_poses)
        if kind == "disc":
            return sr.rollouts(s["state"], s["dist2"], s["cost"], s["poses"], s["targets"], steer_params(s["c"]))
        if kind == "foot":
            return fr.rollouts(s["free_mask"], s["B"], s["dist2"], s["cost"], s["poses"], s["targets"], steer_params(s["c"]))
        return rollouts(s["free_mask"] if kind == "dyn foot" else s["state"], s["dist2"], s["cost"], s["poses"], s["targets"], s["movers"], s["c"],
                        s["B"] if kind == "dyn foot" else None)
    return cached(("staging want", W, H, n_poses, kind), make)


def steer_params(c):
    """c without the movers' two parameters: what the calls of ssf_navsteer.h and ssf_navfoot.h take"""
    return {k: v for k, v in c.items() if k not in DYN_DEFAULTS}


FOOT = (2048, 1536, 1024, 1024, 0)                                       # the footprint of "foot 37x53", with B = 16
BODY = (1536, 512, 512, 512, 0)                                          # a smaller body, for the scenes that set B themselves
DISC_CASES = ("1x1", "1x70 K297 one mover", "37x53 K512 64 movers 70 poses", "64x65 K297 T256", "97x33 K512 T1", "r 0 never hits",
              "two movers one step", "mover on the start", "int64 path", "grow 4096", "cap 0", "300 poses K64")
FOOT_CASES = ("foot 37x53", "foot B1 point", "foot B32 K512 64 movers", "foot 300 poses K257", "foot T256", "foot 1x1 B4")
# the random lists: the reference alone must show a hit, an admissible candidate and a gap strictly between 0 and the cap
GUARDED = ("37x53 K512 64 movers 70 poses", "64x65 K297 T256", "97x33 K512 T1", "foot 37x53", "300 poses K64", "foot B1 point",
           "foot B32 K512 64 movers", "foot 300 poses K257", "foot T256")
_WANT = {}


def cached(key, make):
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


def scene_inputs(name):
    def make():
        s = make_scene(name)
        if name in FOOT_CASES:
            s["free_mask"] = fr.layers(s["state"], s["c"]["allow_unknown"], s["foot"], s["B"])["free_mask"]
        return s
    return cached(("in", name), make)


def scene_reference(name, _wrong=None):
    """rollouts() of a scene, computed once and shared (the callers leave it unchanged)"""
    def make():
        s = scene_inputs(name)
        c = s["c"]
        foot = name in FOOT_CASES
        return rollouts(s["free_mask"] if foot else s["state"], s["dist2"], s["cost"] if c["cost_weight"] else None, s["poses"],
                        s["targets"] if c["target_weight"] else None, s["movers"], c, s["B"] if foot else None, _wrong=_wrong)
    return cached(("want", name) if _wrong is None else ("want", name, _wrong), make)


def not_vacuous(want, c):
    """the three facts of a guarded case: a hit, an admissible candidate, a gap strictly between 0 and the cap"""
    gap = want["cand_min_gap"]
    return bool((want["cand_hit"] >= 0).any()), bool((want["cand_score"] >= 0).any()), bool(((gap > 0) & (gap < c["mover_cap"])).any())


# ---- blob scenes ------------------------------------------------------------------------------------------------------------------------
def blob_camera(cw, ch):
    """a pinhole for a cw x ch image with the room's field of view"""
    return dict(fx=150.0 * cw / 160.0, fy=150.0 * ch / 128.0, cx=(cw - 1) / 2.0, cy=(ch - 1) / 2.0, cam_width=cw, cam_height=ch, t_min=0.2, t_max=5.0)


def blob_scene(cw, ch, kind):
    """dict(depth f32, mask, label, cam_pose, grid_pose, c, min_points, max_blobs) for a cw x ch camera at navlive_ref's room pose.
    The depth and the label image are hand-made per kind"""
    cam = blob_camera(cw, ch)
    pose = lr.room_pose(0, 0, 0)
    # a surface that recedes from 0.9 m at the image's left edge to 1.3 m at its right: a blob has an extent along both axes of the grid
    d = np.tile((0.9 + 0.4 * np.arange(cw) / cw).astype(f32), (ch, 1))
    # a grid narrower than the surface and a band that cuts it: points outside the grid and outside the band
    c = lr.params(width=20, height=31, res=0.05, floor_max=-0.3, z_max=0.1, **cam)
    label = np.full((ch, cw), -1, np.int32)
    mask = np.zeros((ch, cw), np.uint8)
    kw = dict(min_points=1, max_blobs=64)
    if kind == "none":
        pass
    elif kind == "one pixel":
        label[ch // 2, cw // 2] = ch // 2 * cw + cw // 2
        mask[ch // 2, cw // 2] = 1
    elif kind == "columns":
        # vertical stripes, each its own label (the stripe's first pixel), two of equal width side by side, one thin one below
        # min_points, one across a 16 x 16 tile border, members with invalid depth and members outside the band or the grid
        edges = [0, cw // 8, cw // 4, cw // 4 + 1, cw // 4 + cw // 8 + 1, cw // 2 + 3, cw - cw // 5, cw]
        for a, b in zip(edges[:-1], edges[1:]):
            label[:, a:b] = a
            mask[:, a:b] = 1
        mask[:, edges[1]:edges[1] + 1] = 0                               # a gap: pixels with a label and no mask
        label[0, :] = -1                                                 # masked pixels without a label
        if ch > 4:
            d[1, :] = np.nan
            d[2, ::2] = 0.0
        kw = dict(min_points=ch, max_blobs=64)                             # (more than a stripe of one column can hold)
    elif kind == "many":
        # every pixel its own label: more kept labels than max_blobs, all of n = 1: the order is by label alone
        label[:] = np.arange(cw * ch, dtype=np.int32).reshape(ch, cw)[::-1, ::-1]
        mask[:] = 1
        kw = dict(min_points=1, max_blobs=5)
    elif kind == "blocks":
        # blocks of 5 x 3 pixels, each labelled with its first pixel: a tile's 16 columns are no multiple of 5 and its 16 rows none of 3,
        # so a tile holds many labels of several pixels each and most labels lie in two tiles or in four.  A grid wide enough for the whole
        # surface; the band still cuts it.  Three pixels carry labels that are no pixel index (step B.1: not members)
        v, u = np.mgrid[0:ch, 0:cw]
        label[:] = (v // 3 * 3) * cw + u // 5 * 5
        mask[:] = 1
        c = lr.params(width=64, height=31, res=0.05, floor_max=-0.3, z_max=0.1, **cam)
        for k, odd in enumerate((cw * ch, np.iinfo(np.int32).max, np.iinfo(np.int32).min)):
            label[(ch // 2 + k) % ch, (cw // 2 + 3 * k) % cw] = odd
        kw = dict(min_points=1, max_blobs=64)
    else:
        raise KeyError(kind)
    return dict(depth=d, mask=mask, label=label, cam_pose=pose, grid_pose=lr.grid_pose_at(), c=c, cam=cam, **kw)


def blob_tiles(s):
    """of a blob scene, on the restatement's own pixels: (labels with contributing pixels in two or more 16 x 16 tiles, tiles that hold
    eight or more labels)"""
    c = s["c"]
    ch, cw = s["label"].shape
    d = s["depth"]
    member = (s["mask"] != 0) & (s["label"] >= 0) & (s["label"].astype(np.int64) < cw * ch)
    contrib = member & lr.valid_pixels(d, c) & grid_points(d, s["cam_pose"], s["grid_pose"], c)[2]
    tiles_of, labels_in = {}, {}
    for v, u in np.argwhere(contrib):
        L, t = int(s["label"][v, u]), (int(v) // 16, int(u) // 16)
        tiles_of.setdefault(L, set()).add(t)
        labels_in.setdefault(t, set()).add(L)
    return sum(len(t) >= 2 for t in tiles_of.values()), sum(len(l) >= 8 for l in labels_in.values())


BLOB_CAMERAS = ((1, 1), (17, 13), (160, 128))
BLOB_KINDS = ("none", "one pixel", "columns", "many")
BLOCK_CAMERAS = ((40, 24), (35, 19))                                     # the "blocks" kind's: neither side a multiple of 16


def blob_reference(cw, ch, kind, fmt):
    def make():
        s = blob_scene(cw, ch, kind)
        name, scale, img = [f for f in lr.scene_formats(s["depth"]) if f[0] == fmt][0]
        return s, img, scale, blobs(img, s["mask"], s["label"], s["grid_pose"], s["cam_pose"], s["c"], s["min_points"], s["max_blobs"], fmt, scale)
    return cached(("blob", cw, ch, kind, fmt), make)
