"""The restatement of include/ssf_navpose.h that the GPU tests compare against, bit for bit: numpy for the per-state rules (steps 1
to 3), the move table (step 5), a heapq Dijkstra from the goals over (b, iy, ix) for the field (step 7), the projection (step 8) and
the trace (step 9).  Two more formulations check it on the CPU (tests/test_navpose.py): whole-grid Jacobi sweeps, and a sequential
simulation of the device's tile rounds (16 x 16-cell tiles with a one-cell rim and all layers, flags for the tiles that see a
lowered cell) in any tile order.  It shares no code with the library.  Also the shared scenes, tjunction_scene among them."""
import heapq

import numpy as np

import navfoot_ref as fr
import navplan_ref as pr

INF = 0xFFFFFFFF
NO_BIN = 255
TILE = 16
ROUND_BATCH = 16
DIRS, WEIGHT = pr.DIRS, pr.WEIGHT
ANGLE = (0, 256, 512, 768, 128, 384, 640, 896)                          # the direction index of move k
HEADINGS = fr.HEADINGS
DEFAULTS = dict(n_headings=16, min_dist2=0, soft_dist2=0, near_penalty=0, move_tol=64, allow_reverse=1, reverse_cost=10, turn_cost=5, max_path=0)
STATS = ("states_traversable", "states_reached", "cells_reached", "goals_used", "goals_blocked", "goals_outside", "max_cost")
STATUS_REACHED, STATUS_OUTSIDE, STATUS_BLOCKED, STATUS_NO_GOAL, STATUS_TRUNCATED = 0, 1, 2, 3, 4


def params(**kw):
    bad = [k for k in kw if k not in DEFAULTS]
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def triples(a):
    """n x 3 int32"""
    return np.zeros((0, 3), np.int32) if a is None or len(a) == 0 else np.asarray(a, np.int32).reshape(-1, 3)


def circ(a, b):
    return min((a - b) & 1023, (b - a) & 1023)


def moves(B, move_tol, allow_reverse):
    """B x 8 int8: 0 = not a move of the bin, 1 = forward, 2 = reverse (steps 3 and 5)"""
    assert B in HEADINGS, B
    out = np.zeros((B, 8), np.int8)
    for b in range(B):
        kb = b * (1024 // B)
        for k in range(8):
            if circ(kb, ANGLE[k]) <= move_tol:
                out[b, k] = 1
            elif allow_reverse and circ(kb + 512, ANGLE[k]) <= move_tol:
                out[b, k] = 2
    return out


# ---- steps 1, 2 -------------------------------------------------------------------------------------------------------------------
def prep(free_mask, dist2, q):
    """(trav bool B x H x W, pen int64 H x W)"""
    mask, dist2 = np.asarray(free_mask).astype(np.int64), np.asarray(dist2, np.int32).astype(np.int64)
    B = q["n_headings"]
    roomy = dist2 >= q["min_dist2"]
    trav = np.stack([(((mask >> b) & 1) != 0) & roomy for b in range(B)])
    soft = int(q["soft_dist2"])
    pen = (int(q["near_penalty"]) * (soft - np.clip(dist2, 0, soft))) // soft if soft > 0 else np.zeros_like(dist2)
    return trav, pen


def goal_states(trav, goals):
    """(goal mask B x H x W, the counts of step 6)"""
    B, H, W = trav.shape
    mask = np.zeros((B, H, W), bool)
    n = dict(goals_used=0, goals_blocked=0, goals_outside=0)
    for x, y, b in triples(goals):
        if not (0 <= x < W and 0 <= y < H and -1 <= b < B):
            n["goals_outside"] += 1
            continue
        sel = trav[:, y, x].copy()
        if b >= 0:
            sel[np.arange(B) != b] = False
        if not sel.any():
            n["goals_blocked"] += 1
        else:
            n["goals_used"] += 1
            mask[:, y, x] |= sel
    return mask, n


# ---- step 7: Dijkstra from the goals over the reversed transitions ---------------------------------------------------------------------
def field(trav, pen, goal, q):
    B, H, W = trav.shape
    mv = moves(B, q["move_tol"], q["allow_reverse"]).tolist()
    rev, turn = int(q["reverse_cost"]), int(q["turn_cost"])
    T = trav.tolist()
    Pn = np.asarray(pen).tolist()
    cost = [[[INF] * W for _ in range(H)] for _ in range(B)]
    heap = []
    for b, y, x in zip(*np.nonzero(goal)):
        cost[b][y][x] = 0
        heap.append((0, int(b), int(y), int(x)))
    heapq.heapify(heap)
    while heap:
        c, b, y, x = heapq.heappop(heap)
        if c != cost[b][y][x]:
            continue
        Tb, Cb = T[b], cost[b]
        step = Pn[y][x]
        for k, (dx, dy) in enumerate(DIRS):                              # the move (p, b) -> (q, b) = (x, y, b) along k: p = q - d
            code = mv[b][k]
            if not code:
                continue
            px, py = x - dx, y - dy
            if not (0 <= px < W and 0 <= py < H) or not Tb[py][px]:
                continue
            if k >= 4 and not (Tb[py][px + dx] and Tb[py + dy][px]):     # the two axial cells at the corner, at bin b
                continue
            v = c + WEIGHT[k] + step + (rev if code == 2 else 0)
            if v < Cb[py][px]:
                Cb[py][px] = v
                heapq.heappush(heap, (v, b, py, px))
        if B > 1:
            for nb in {(b + 1) & (B - 1), (b - 1) & (B - 1)}:            # the rotation (p, nb) -> (p, b)
                if T[nb][y][x] and c + turn < cost[nb][y][x]:
                    cost[nb][y][x] = c + turn
                    heapq.heappush(heap, (c + turn, nb, y, x))
    return np.array(cost, np.uint32).reshape(B, H, W)


def project(cost):
    """(cell_cost uint32 H x W, cell_bin uint8 H x W): step 8"""
    cell_cost = cost.min(axis=0)
    cell_bin = np.where(cell_cost == INF, NO_BIN, np.argmin(cost, axis=0)).astype(np.uint8)      # (argmin: the first, so the smallest b)
    return cell_cost.astype(np.uint32), cell_bin


# ---- step 9 ----------------------------------------------------------------------------------------------------------------------
def start_state(start, B):
    x, y, h = (int(v) for v in start)
    return x >> 10, y >> 10, fr.bin_of(h & 0xFFFF, B)


def transition_value(cost, trav, pen, mv, q, x, y, b, t):
    """(c + cost[t], the state t) of transition number t from (x, y, b), or None when it is not admissible or leads nowhere"""
    B, H, W = trav.shape
    if t < 8:
        code = int(mv[b, t])
        dx, dy = DIRS[t]
        qx, qy = x + dx, y + dy
        if not code or not (0 <= qx < W and 0 <= qy < H) or not trav[b, qy, qx]:
            return None
        if t >= 4 and not (trav[b, y, qx] and trav[b, qy, x]):
            return None
        if int(cost[b, qy, qx]) == INF:
            return None
        return WEIGHT[t] + int(pen[qy, qx]) + (q["reverse_cost"] if code == 2 else 0) + int(cost[b, qy, qx]), (qx, qy, b)
    nb = ((b + 1) if t == 8 else (b - 1)) & (B - 1)
    if nb == b or not trav[nb, y, x] or int(cost[nb, y, x]) == INF:
        return None
    return q["turn_cost"] + int(cost[nb, y, x]), (x, y, nb)


def trace(cost, trav, pen, start, q):
    """(status, cost, path (len, 3) int32)"""
    B, H, W = trav.shape
    mv = moves(B, q["move_tol"], q["allow_reverse"])
    x, y, b = start_state(start, B)
    none = np.zeros((0, 3), np.int32)
    if not (0 <= x < W and 0 <= y < H):
        return STATUS_OUTSIDE, INF, none
    if not trav[b, y, x]:
        return STATUS_BLOCKED, INF, none
    c0 = int(cost[b, y, x])
    if c0 == INF:
        return STATUS_NO_GOAL, INF, none
    if q["max_path"] <= 0:
        return STATUS_REACHED, c0, none
    path = []
    while True:
        if len(path) == q["max_path"]:
            return STATUS_TRUNCATED, c0, np.array(path, np.int32).reshape(-1, 3)
        path.append((x, y, b))
        c = int(cost[b, y, x])
        if c == 0:
            return STATUS_REACHED, c0, np.array(path, np.int32).reshape(-1, 3)
        vals = [(r[0], t, r[1]) for t in range(10) for r in [transition_value(cost, trav, pen, mv, q, x, y, b, t)] if r is not None]
        v, _, (x, y, b) = min(vals)
        assert v == c, (x, y, b, v, c)                                  # step 7: the minimum equals cost[s]


def plan(free_mask, dist2, goals, starts=None, **kw):
    """every output and exact stat of ssf_navpose_field: cost, cell_cost, cell_bin, start_cost, start_status, path_len, path (a list),
    stats; and trav, pen"""
    q = params(**kw)
    trav, pen = prep(free_mask, dist2, q)
    goal, n = goal_states(trav, goals)
    cost = field(trav, pen, goal, q)
    reached = cost != INF
    cell_cost, cell_bin = project(cost)
    out = dict(cost=cost, cell_cost=cell_cost, cell_bin=cell_bin, trav=trav, pen=pen)
    res = [trace(cost, trav, pen, s, q) for s in triples(starts)]
    out["start_status"] = np.array([r[0] for r in res], np.int32)
    out["start_cost"] = np.array([r[1] for r in res], np.uint32)
    out["path"] = [r[2] for r in res]
    out["path_len"] = np.array([len(r[2]) for r in res], np.int32)
    out["stats"] = dict(n, states_traversable=int(trav.sum()), states_reached=int(reached.sum()), cells_reached=int(reached.any(axis=0).sum()),
                        max_cost=int(cost[reached].max()) if reached.any() else 0)
    return out


# ---- the second formulation: Jacobi sweeps over an array of states ---------------------------------------------------------------------
def sweep(cost, trav, pen, mv, rev, turn):
    """one Jacobi sweep of cost[s] = min(cost[s], min over transitions s -> t of c + cost[t]) over int64 B x H x W (INF = not reached)"""
    B, H, W = cost.shape
    C = np.pad(cost, ((0, 0), (1, 1), (1, 1)), constant_values=INF)
    T = np.pad(trav, ((0, 0), (1, 1), (1, 1)), constant_values=False)
    Pn = np.pad(pen, 1, constant_values=0)
    best = cost.copy()
    for b in range(B):
        for k, (dx, dy) in enumerate(DIRS):
            code = int(mv[b, k])
            if not code:
                continue
            cq, tq, pq = C[b, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W], T[b, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W], Pn[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            ok = tq & (cq != INF)
            if k >= 4:
                ok = ok & T[b, 1:1 + H, 1 + dx:1 + dx + W] & T[b, 1 + dy:1 + dy + H, 1:1 + W]
            best[b] = np.minimum(best[b], np.where(ok, cq + WEIGHT[k] + pq + (rev if code == 2 else 0), INF))
        if B > 1:
            for nb in ((b + 1) & (B - 1), (b - 1) & (B - 1)):
                best[b] = np.minimum(best[b], np.where(cost[nb] != INF, cost[nb] + turn, INF))
    return np.where(trav, best, cost)


def field_by_sweeps(trav, pen, goal, q):
    mv = moves(trav.shape[0], q["move_tol"], q["allow_reverse"])
    cost = np.where(goal, 0, INF).astype(np.int64)
    pen = np.asarray(pen, np.int64)
    while True:
        new = sweep(cost, trav, pen, mv, q["reverse_cost"], q["turn_cost"])
        if np.array_equal(new, cost):
            return cost.astype(np.uint32)
        cost = new


# ---- the third: the device's tile rounds, one tile after the other in the order `order` gives ---------------------------------------
def seers(lx, ly):
    """the tile offsets (sx, sy) != (0, 0) whose 18 x 18 window holds cell (lx, ly) of a tile"""
    sx = -1 if lx == 0 else (1 if lx == TILE - 1 else 0)
    sy = -1 if ly == 0 else (1 if ly == TILE - 1 else 0)
    return ([(sx, 0)] if sx else []) + ([(0, sy)] if sy else []) + ([(sx, sy)] if sx and sy else [])


def field_by_tile_rounds(trav, pen, goal, q, order=None, stale=False):
    """(cost, rounds, tile visits).  order(round, tiles) -> the tiles in the order they are worked on (None: ascending).  A tile
    reads its window from the field as it stands when its turn comes or, with stale, as it stood when the round began: the two
    ends of what a workgroup may see of its neighbours' stores of the same round."""
    B, H, W = trav.shape
    mv = moves(B, q["move_tol"], q["allow_reverse"])
    rev, turn = q["reverse_cost"], q["turn_cost"]
    ntx, nty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    cost = np.where(goal, 0, INF).astype(np.int64)
    C = np.pad(cost, ((0, 0), (1, 1), (1, 1)), constant_values=INF)
    T = np.pad(trav, ((0, 0), (1, 1), (1, 1)), constant_values=False)
    Pn = np.pad(np.asarray(pen, np.int64), 1, constant_values=0)

    def flag(into, tx, ty, lx, ly, own):
        for sx, sy in ([(0, 0)] if own else []) + seers(lx, ly):
            if 0 <= tx + sx < ntx and 0 <= ty + sy < nty:
                into.add((tx + sx, ty + sy))
    cur = set()
    for _, y, x in zip(*np.nonzero(goal)):
        flag(cur, x // TILE, y // TILE, x % TILE, y % TILE, True)
    rounds = visits = 0
    while cur:
        nxt = set()
        tiles = sorted(cur)
        seen = C.copy() if stale else C
        for tx, ty in (order(rounds, tiles) if order else tiles):
            x0, y0 = tx * TILE, ty * TILE                               # (the window's corner in the padded arrays)
            x1, y1 = min(x0 + TILE + 2, W + 2), min(y0 + TILE + 2, H + 2)
            wc, wt, wp = seen[:, y0:y1, x0:x1].copy(), T[:, y0:y1, x0:x1], Pn[y0:y1, x0:x1]
            inner = np.zeros(wt.shape, bool)
            inner[:, 1:-1, 1:-1] = True                                 # the rim is read, never written
            old = wc.copy()
            while True:
                new = np.where(inner, sweep(wc, wt, wp, mv, rev, turn), wc)
                if np.array_equal(new, wc):
                    break
                wc = new
            for b, wy, wx in np.argwhere(wc < old):
                C[b, y0 + wy, x0 + wx] = wc[b, wy, wx]
                flag(nxt, tx, ty, wx - 1, wy - 1, False)
            visits += 1
        rounds += 1
        cur = nxt
    return C[:, 1:-1, 1:-1].astype(np.uint32), rounds, visits


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def point_mask(state, allow_unknown, B):
    """the layers of the point footprint: every bin where the cell is clear"""
    return np.where(fr.clear_cells(state, allow_unknown), (1 << B) - 1, 0).astype(np.uint32)


def clearance2(state, cap=64):
    """squared distance in cells from every free cell to the nearest cell that is not free (0 on those), capped: a plain minimum over
    the grid's cells, as the grid calls define dist2 inside the map"""
    state = np.asarray(state)
    H, W = state.shape
    oy, ox = np.nonzero(state != 0)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.full((H, W), cap, np.int64)
    for i in range(0, len(oy), 512):
        d = (yy[..., None] - oy[i:i + 512]) ** 2 + (xx[..., None] - ox[i:i + 512]) ** 2
        out = np.minimum(out, d.min(axis=-1))
    return np.where(state == 0, out, 0).astype(np.int32)


TJ_FOOT = fr.CORRIDOR_FOOT                                               # 11 x 5 cells, pad 0
TJ_START_CELL, TJ_GOAL_CELL = (10, 11), (36, 29)                        # (ix, iy)
TJ_DISC_MIN_DIST2 = 7
TJ_KW = dict(move_tol=64, allow_reverse=1, reverse_cost=10, turn_cost=5)


def tjunction_scene(detour):
    """64 x 70 cells, everything occupied but a horizontal corridor state[8:15, 2:40] and a vertical one state[8:36, 33:40], both 7
    cells wide, which meet in a bend at the top right: the 11 x 5-cell body drives along either and cannot turn in the bend.  With
    `detour` the horizontal corridor runs on to column 65 (the bend becomes a T-junction), a wide passage state[1:62, 48:66] leads down
    and a room state[36:62, 20:66] lies below the vertical corridor: the body reaches it from below.  dict(state, dist2, start (a pose
    in the start cell's centre, heading 0), goals (the goal cell, any heading), goal_cell, start_cell, foot)"""
    H, W = 64, 70
    state = np.full((H, W), 100, np.int8)
    state[8:15, 2:40] = 0
    state[8:36, 33:40] = 0
    if detour:
        state[8:15, 2:66] = 0
        state[1:62, 48:66] = 0
        state[36:62, 20:66] = 0
    sx, sy = TJ_START_CELL
    gx, gy = TJ_GOAL_CELL
    return dict(state=state, dist2=clearance2(state), start=np.array([[sx * 1024 + 512, sy * 1024 + 512, 0]], np.int32),
                goals=np.array([[gx, gy, -1]], np.int32), goal_cell=TJ_GOAL_CELL, start_cell=TJ_START_CELL, foot=TJ_FOOT)


def serpentine(h, w):
    """walls on every second row, open at alternating ends: one corridor a cell wide from (0, 0), which crosses every tile column
    boundary once per lane.  Returns (state, dist2)"""
    state, dist2 = pr.open_grid(h, w)
    for i, y in enumerate(range(1, h, 2)):
        state[y, :] = 100
        state[y, w - 1 if i % 2 == 0 else 0] = 0
    return state, dist2


def corner_grid(seed=5):
    """2 TILE x 2 TILE cells with obstacles on both sides of the corner the four tiles share, and a few at random"""
    n = 2 * TILE
    rng = np.random.default_rng(seed)
    state = np.where(rng.random((n, n)) < 0.08, 100, 0).astype(np.int8)
    state[TILE - 3:TILE + 3, TILE - 3:TILE + 3] = 0
    state[TILE - 1, TILE - 2], state[TILE, TILE + 1] = 100, 100          # either side of the corner, so that diagonals across it are cut
    return state, rng.integers(0, 41, (n, n)).astype(np.int32)


_WANT = {}


def cached(key, make):
    """make() computed once under `key` and shared (the callers leave it unchanged)"""
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]
