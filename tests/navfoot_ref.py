"""A restatement of include/ssf_navfoot.h in numpy integers: the footprint's cells by the header's inequalities, the heading layers
as a dilation by shifted copies (one per covered cell), and the rollouts restated from the header, vectorised over the candidates of
a pose.  It shares no code with the library.  The lattice, the direction table and the parameter names are tests/navsteer_ref.py's,
as the header takes them from ssf_navsteer.h."""
import numpy as np

import navsteer_ref as sr

MAX_REACH, ROWS, MAX_SIDE, MAX_PAD = 40, 81, 24576, 4096
HEADINGS = (1, 2, 4, 8, 16, 32)
STATS = ("cells_clear", "cells_all", "cells_some", "cells_none", "reach", "kernel_cells")
SUB, TURN, NO_COST = sr.SUB, sr.TURN, sr.NO_COST
_C, _S = sr.direction_table()

# the footprints of the issue: (front, back, left, right, pad)
POINT = (0, 0, 0, 0, 0)
LINE = (9216, 0, 0, 0, 0)
ASYM = (6144, 1024, 2048, 3072, 724)
CORNERS = ((24576, 24576, 24576, 24576, 4096), (24576, 0, 24576, 0, 4096), (0, 24576, 0, 24576, 4096), (24576, 0, 0, 24576, 4096))
FOOTPRINTS = dict(point=POINT, line=LINE, asym=ASYM, corner0=CORNERS[0], corner1=CORNERS[1], corner2=CORNERS[2], corner3=CORNERS[3])


def bins(B):
    """(shift, half) of B heading bins"""
    assert B in HEADINGS, B
    shift = 16 - (B.bit_length() - 1)
    return shift, 1 << (shift - 1)


def bin_of(h, B):
    shift, half = bins(B)
    return ((h + half) >> shift) & (B - 1)


def covered(foot, B, span=MAX_REACH):
    """bool B x (2 span + 1) x (2 span + 1), [b, dy + span, dx + span]: the header's inequalities in Python integers (int64 suffices)"""
    front, back, left, right, pad = (int(v) for v in foot)
    dy, dx = np.mgrid[-span:span + 1, -span:span + 1].astype(np.int64)
    out = np.zeros((B, 2 * span + 1, 2 * span + 1), bool)
    for b in range(B):
        k = b * (1024 // B)
        C, S = int(_C[k]), int(_S[k])
        u, v = 1024 * (dx * C + dy * S), 1024 * (dy * C - dx * S)
        out[b] = (-(back + pad) * 16384 <= u) & (u <= (front + pad) * 16384) & (-(right + pad) * 16384 <= v) & (v <= (left + pad) * 16384)
    return out


def spans(foot, B):
    """(spans int16 B x 81 x 2, reach, kernel_cells, one_interval): what ssf_navfoot_spans returns, and whether every row is one interval"""
    cov = covered(foot, B, MAX_REACH + 1)
    edge = cov.copy()
    edge[:, 1:-1, 1:-1] = False
    assert not edge.any(), "the footprint reaches farther than 40 cells"
    cov = cov[:, 1:-1, 1:-1]
    out = np.zeros((B, ROWS, 2), np.int16)
    out[..., 0] = 1
    one, reach = True, 0
    for b in range(B):
        for r in range(ROWS):
            at = np.flatnonzero(cov[b, r])
            if len(at):
                lo, hi = int(at[0]) - MAX_REACH, int(at[-1]) - MAX_REACH
                out[b, r] = (lo, hi)
                one &= len(at) == hi - lo + 1
                reach = max(reach, abs(r - MAX_REACH), abs(lo), abs(hi))
    return out, reach, int(cov.sum()), bool(one)


def clear_cells(state, allow_unknown):
    state = np.asarray(state).astype(np.int64)
    return (state == 0) | ((state == -1) if allow_unknown else False)


def layers(state, allow_unknown, foot, B):
    """dict(free_mask uint32, n_free uint8, stats): step 2, a dilation by shifted copies: bit b of a cell survives iff the clear map
    shifted by every covered offset of bin b is clear there; outside the grid nothing is clear"""
    clear = clear_cells(state, allow_unknown)
    H, W = clear.shape
    cov = covered(foot, B)
    _, reach, cells, _ = spans(foot, B)
    R = MAX_REACH
    pad = np.zeros((H + 2 * R, W + 2 * R), bool)
    pad[R:R + H, R:R + W] = clear
    mask = np.zeros((H, W), np.uint32)
    for b in range(B):
        ok = np.ones((H, W), bool)
        for r, c in np.argwhere(cov[b]):
            ok &= pad[r:r + H, c:c + W]                                # the cell at offset (dx, dy) = (c - R, r - R)
            if not ok.any():
                break
        mask |= ok.astype(np.uint32) << np.uint32(b)
    n_free = np.zeros((H, W), np.uint8)
    for b in range(B):
        n_free += ((mask >> np.uint32(b)) & 1).astype(np.uint8)
    full = np.uint32((1 << B) - 1)
    stats = dict(cells_clear=int(clear.sum()), cells_all=int((mask == full).sum()), cells_some=int(((mask != 0) & (mask != full)).sum()),
                 cells_none=int((mask == 0).sum()), reach=reach, kernel_cells=cells)
    return dict(free_mask=mask, n_free=n_free, stats=stats)


def sweep_mask(h, w, B):
    """the bins a step from heading h (0..65535) with turn w sweeps, as a bit mask: the header's loop, literally"""
    shift, half = bins(B)
    a = h + half
    lo, hi = min(a, a + w) >> shift, max(a, a + w) >> shift
    need = 0
    for u in range(lo, hi + 1):
        need |= 1 << (u & (B - 1))
    return need


def rollouts(free_mask, B, dist2, cost, poses, targets, c):
    """every output of ssf_navfoot_rollouts (navsteer_ref.OUTPUTS, in the ABI's dtypes; best_traj entries past best_len are 0 here and
    unwritten there) and 'stats'.  cost / targets may be None with their weight 0.  c: navsteer_ref.params"""
    mask = np.asarray(free_mask).astype(np.int64)
    dist2 = np.asarray(dist2).astype(np.int64)
    H, W = mask.shape
    d = np.minimum(np.maximum(dist2, 0), c["clearance_cap"])
    roomy = dist2 >= c["min_dist2"]
    poses = np.asarray(poses, np.int64).reshape(-1, 3)
    n, T = len(poses), c["n_steps"]
    v, w, vmax = sr.lattice(c)
    K = len(v)
    av, aw = np.abs(v), np.abs(w)
    if c["cost_weight"] > 0:
        cost = np.asarray(cost).astype(np.int64)
    if c["target_weight"] > 0:
        targets = np.asarray(targets, np.int64).reshape(-1, 2)
    need_steps = np.minimum(T, c["min_free_steps"] + ((av + c["brake_div"] - 1) // c["brake_div"] if c["brake_div"] > 0 else 0))
    shift, half = bins(B)

    def ok(ix, iy, need):              # traversable under need; outside the grid: not
        inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        cy, cx = np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)
        return inside & ((mask[cy, cx] & need) == need) & roomy[cy, cx]

    def sweep(h):                      # the need of every candidate's step from its heading h
        a = h + half
        lo, hi = np.minimum(a, a + w) >> shift, np.maximum(a, a + w) >> shift
        need = np.zeros(K, np.int64)
        for k in range(int((hi - lo).max()) + 1):
            need |= np.where(lo + k <= hi, np.int64(1) << ((lo + k) & (B - 1)), 0)
        return need

    out = dict(best=np.full(n, -1), best_cmd=np.zeros((n, 2)), best_score=np.full(n, -1), n_admissible=np.zeros(n), pose_status=np.zeros(n),
               best_len=np.zeros(n), best_traj=np.zeros((n, T + 1, 3)), cand_free=np.zeros((n, K)), cand_min_d=np.full((n, K), -1),
               cand_end=np.zeros((n, K, 3)), cand_end_cost=np.full((n, K), NO_COST), cand_score=np.full((n, K), -1))
    out = {nm: a.astype(np.int64) for nm, a in out.items()}
    glob = 0
    for q in range(n):
        px, py, ph = int(poses[q, 0]), int(poses[q, 1]), int(poses[q, 2]) & 0xFFFF
        cx, cy = px >> 10, py >> 10
        out["cand_end"][q] = (px, py, ph)
        if not (0 <= cx < W and 0 <= cy < H):
            out["pose_status"][q] = 1
            continue
        if not ok(np.int64(cx), np.int64(cy), np.int64(1) << bin_of(ph, B)):
            out["pose_status"][q] = 2
            continue
        glob += -(-K // 256)
        x, y, h = np.full(K, px), np.full(K, py), np.full(K, ph)
        free, min_d, alive = np.zeros(K, np.int64), np.full(K, d[cy, cx]), np.ones(K, bool)
        traj = np.zeros((K, T + 1, 3), np.int64)
        traj[:, 0] = (px, py, ph)
        for s in range(T):
            k = ((2 * h + w + 64) >> 7) & 1023
            nx, ny = x + ((v * _C[k] + 8192) >> 14), y + ((v * _S[k] + 8192) >> 14)
            ox, oy, ncx, ncy = x >> 10, y >> 10, nx >> 10, ny >> 10
            need = sweep(h)
            step = ok(ncx, ncy, need)
            diag = (ncx != ox) & (ncy != oy)
            step &= ~diag | (ok(ncx, oy, need) & ok(ox, ncy, need))
            alive &= step
            if not alive.any():
                break
            x, y, h = np.where(alive, nx, x), np.where(alive, ny, y), np.where(alive, (h + w) & 0xFFFF, h)
            free += alive
            dn = d[np.clip(y >> 10, 0, H - 1), np.clip(x >> 10, 0, W - 1)]
            min_d = np.where(alive, np.minimum(min_d, dn), min_d)
            traj[alive, s + 1] = np.stack([x, y, h], axis=1)[alive]
        ec = cost[y >> 10, x >> 10] if c["cost_weight"] > 0 else np.full(K, NO_COST)
        adm = free >= need_steps
        if c["cost_weight"] > 0:
            adm &= ec != NO_COST
        score = c["clear_weight"] * (c["clearance_cap"] - min_d) + c["speed_weight"] * (vmax - av) + c["turn_weight"] * aw
        if c["cost_weight"] > 0:
            score = score + c["cost_weight"] * ec
        if c["target_weight"] > 0:
            dx, dy = np.abs(x - targets[q, 0]), np.abs(y - targets[q, 1])
            score = score + c["target_weight"] * ((10 * np.maximum(dx, dy) + 4 * np.minimum(dx, dy)) >> 10)
        score = np.where(adm, score, -1)
        out["cand_free"][q], out["cand_min_d"][q], out["cand_end_cost"][q], out["cand_score"][q] = free, min_d, ec, score
        out["cand_end"][q] = np.stack([x, y, h], axis=1)
        out["n_admissible"][q] = adm.sum()
        if not adm.any():
            out["pose_status"][q] = 3
            continue
        cands = np.flatnonzero(adm)
        b = int(cands[np.lexsort((cands, score[cands]))[0]])              # the smallest (score, c)
        out["best"][q], out["best_cmd"][q], out["best_score"][q] = b, (v[b], w[b]), score[b]
        out["best_len"][q] = free[b] + 1
        out["best_traj"][q, :free[b] + 1] = traj[b, :free[b] + 1]
    st = out["pose_status"]
    stats = dict(poses_ok=int((st == 0).sum()), poses_blocked=int(((st == 1) | (st == 2)).sum()), poses_stuck=int((st == 3).sum()),
                 candidates=n * K, admissible=int(out["n_admissible"].sum()), collided=int((out["cand_free"] < T).sum()),
                 steps_taken=int(out["cand_free"].sum()), windows_staged=0, windows_global=glob)
    res = {nm: out[nm].astype(sr.DTYPES[nm]) for nm in sr.OUTPUTS}
    res["stats"] = stats
    return res


# ---- the host helpers of the wrappers, restated -------------------------------------------------------------------------------------
def pad_for(front, back, left, right, B):
    """the pad that makes the layers conservative (the header's step 1): ceil(2 * 724.1 + rho * pi / B)"""
    rho = float(np.hypot(max(front, back), max(left, right)))
    return int(np.ceil(2 * 724.1 + rho * np.pi / B))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
CORRIDOR_FOOT = (5632, 5632, 2560, 2560, 0)                              # an 11 x 5-cell robot: 5.5 cells ahead and behind, 2.5 to either side
CORRIDOR_B = 32


def corridor_scene():
    """a corridor 7 cells wide along x in a 40 x 96 grid (rows 16..22 free), closed at both ends; an 11 x 5-cell robot one row off its
    middle, heading along it: two clear rows to one side of the body's five, so it fits at bin 0 only (at bin 1, 11.25 degrees, the
    body spans seven rows).  The disc by the circumscribed radius (6.04 cells: dist2 >= 37) does not fit anywhere in it."""
    H, W = 40, 96
    state = np.full((H, W), 100, np.int8)
    state[16:23, 2:94] = 0
    yy, xx = np.mgrid[0:H, 0:W]
    near = np.minimum(np.minimum(yy - 15, 23 - yy), np.minimum(xx - 1, 94 - xx))         # the walls are whole lines: the nearest is axial
    dist2 = np.where(state == 0, np.minimum(near * near, 64), 0).astype(np.int32)
    cost = sr.field(state, dist2, (88, 19), sr.params(width=W, height=H))
    poses = np.array([sr.centre(20, 18, 0), sr.centre(40, 18, 65535), sr.centre(60, 18, 300)], np.int32)
    c = sr.params(width=W, height=H, n_poses=len(poses), n_steps=16, n_v=5, n_w=9, v_min=0, v_step=128, w_min=-4096, w_step=1024)
    return dict(state=state, dist2=dist2, cost=cost, poses=poses, targets=None, c=c, foot=CORRIDOR_FOOT, B=CORRIDOR_B)


_WANT = {}


def cached(key, make):
    """make() computed once under `key` and shared (the callers leave it unchanged)"""
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]
