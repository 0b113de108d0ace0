"""The restatement of include/ssf_navplan.h that the GPU tests compare against, bit for bit: numpy for the per-cell rules (steps 1,
2, 4), a heapq Dijkstra from the goals for the field (step 6) and the path trace (step 7).  Two more formulations check it on the
CPU (tests/test_navplan.py): whole-grid Bellman-Ford sweeps to the fixed point, and a sequential simulation of the device's tile
rounds (32 x 32 tiles with a one-cell rim, flags for the tiles that see a lowered cell) in any tile order.  Also the shared scenes."""
import heapq

import numpy as np

INF = 0xFFFFFFFF
TILE = 32
DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))          # (dx, dy), k = 0..7
WEIGHT = (10, 10, 10, 10, 14, 14, 14, 14)
DEFAULTS = dict(min_dist2=0, soft_dist2=0, near_penalty=0, allow_unknown=0, goals_from_frontier=0, max_path=0)
STATS = ("cells_traversable", "cells_reached", "frontier_cells", "frontier_goals", "goals_used", "goals_blocked", "goals_outside", "max_cost")
STATUS_REACHED, STATUS_OUTSIDE, STATUS_BLOCKED, STATUS_NO_GOAL, STATUS_TRUNCATED = 0, 1, 2, 3, 4


def params(**kw):
    bad = [k for k in kw if k not in DEFAULTS]
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def cells(a):
    """n x 2 int32 (ix, iy)"""
    return np.zeros((0, 2), np.int32) if a is None or len(a) == 0 else np.asarray(a, np.int32).reshape(-1, 2)


# ---- steps 1, 2, 4 -------------------------------------------------------------------------------------------------------
def prep(state, dist2, q):
    """(trav bool, pen int64, frontier uint8), each H x W"""
    state, dist2 = np.asarray(state, np.int8), np.asarray(dist2, np.int32).astype(np.int64)
    trav = ((state == 0) | ((state == -1) if q["allow_unknown"] else False)) & (dist2 >= q["min_dist2"])
    soft = int(q["soft_dist2"])
    pen = (int(q["near_penalty"]) * (soft - np.clip(dist2, 0, soft))) // soft if soft > 0 else np.zeros_like(dist2)
    unknown = np.pad(state == -1, 1, constant_values=False)
    near = unknown[1:-1, 2:] | unknown[1:-1, :-2] | unknown[2:, 1:-1] | unknown[:-2, 1:-1]
    return trav, pen, ((state == 0) & near).astype(np.uint8)


def goal_cells(trav, frontier, goals, q):
    """(goal mask H x W, the counts of step 5)"""
    H, W = trav.shape
    mask = np.zeros((H, W), bool)
    n = dict(goals_used=0, goals_blocked=0, goals_outside=0, frontier_goals=0)
    for x, y in cells(goals):
        if not (0 <= x < W and 0 <= y < H):
            n["goals_outside"] += 1
        elif not trav[y, x]:
            n["goals_blocked"] += 1
        else:
            n["goals_used"] += 1
            mask[y, x] = True
    if q["goals_from_frontier"]:
        fg = (frontier != 0) & trav
        n["frontier_goals"] = int(fg.sum())
        mask |= fg
    return mask, n


# ---- step 6: Dijkstra from the goals over the reversed moves ---------------------------------------------------------------------
def field(trav, pen, goal):
    H, W = trav.shape
    T = [[bool(v) for v in row] for row in trav]
    Pn = [[int(v) for v in row] for row in pen]
    cost = [[INF] * W for _ in range(H)]
    heap = []
    for y, x in zip(*np.nonzero(goal)):
        cost[y][x] = 0
        heap.append((0, int(x), int(y)))
    heapq.heapify(heap)
    while heap:
        c, x, y = heapq.heappop(heap)
        if c != cost[y][x]:
            continue
        step = Pn[y][x]
        for k, (dx, dy) in enumerate(DIRS):                              # the move p -> q = (x, y) along direction k: p = q - d
            px, py = x - dx, y - dy
            if not (0 <= px < W and 0 <= py < H) or not T[py][px]:
                continue
            if k >= 4 and not (T[py][px + dx] and T[py + dy][px]):      # the two axial cells that share the corner
                continue
            v = c + WEIGHT[k] + step
            if v < cost[py][px]:
                cost[py][px] = v
                heapq.heappush(heap, (v, px, py))
    return np.array(cost, np.uint32).reshape(H, W)


def move_value(cost, trav, pen, x, y, k):
    """w(k) + pen[q] + cost[q] of the move from (x, y) along k, or None when it is not admissible or q is not reached"""
    H, W = trav.shape
    dx, dy = DIRS[k]
    qx, qy = x + dx, y + dy
    if not (0 <= qx < W and 0 <= qy < H) or not trav[qy, qx]:
        return None
    if k >= 4 and not (trav[y, qx] and trav[qy, x]):
        return None
    if int(cost[qy, qx]) == INF:
        return None
    return WEIGHT[k] + int(pen[qy, qx]) + int(cost[qy, qx])


# ---- step 7 ----------------------------------------------------------------------------------------------------------------------
def trace(cost, trav, pen, start, max_path):
    """(status, cost, path (len, 2) int32)"""
    H, W = trav.shape
    x, y = int(start[0]), int(start[1])
    none = np.zeros((0, 2), np.int32)
    if not (0 <= x < W and 0 <= y < H):
        return STATUS_OUTSIDE, INF, none
    if not trav[y, x]:
        return STATUS_BLOCKED, INF, none
    c0 = int(cost[y, x])
    if c0 == INF:
        return STATUS_NO_GOAL, INF, none
    if max_path <= 0:
        return STATUS_REACHED, c0, none
    path = []
    while True:
        if len(path) == max_path:
            return STATUS_TRUNCATED, c0, np.array(path, np.int32).reshape(-1, 2)
        path.append((x, y))
        c = int(cost[y, x])
        if c == 0:
            return STATUS_REACHED, c0, np.array(path, np.int32).reshape(-1, 2)
        vals = [(v, k) for k in range(8) for v in [move_value(cost, trav, pen, x, y, k)] if v is not None]
        v, k = min(vals)
        assert v == c, (x, y, v, c)                                     # step 6: the minimum equals cost[p]
        x, y = x + DIRS[k][0], y + DIRS[k][1]


def plan(state, dist2, goals=None, starts=None, **kw):
    """every output and exact stat of ssf_navplan_field: cost, frontier, start_cost, start_status, path_len, path (a list), stats"""
    q = params(**kw)
    trav, pen, frontier = prep(state, dist2, q)
    goal, n = goal_cells(trav, frontier, goals, q)
    cost = field(trav, pen, goal)
    reached = cost != INF
    out = dict(cost=cost, frontier=frontier, trav=trav, pen=pen)
    res = [trace(cost, trav, pen, s, q["max_path"]) for s in cells(starts)]
    out["start_status"] = np.array([r[0] for r in res], np.int32)
    out["start_cost"] = np.array([r[1] for r in res], np.uint32)
    out["path"] = [r[2] for r in res]
    out["path_len"] = np.array([len(r[2]) for r in res], np.int32)
    out["stats"] = dict(n, cells_traversable=int(trav.sum()), cells_reached=int(reached.sum()), frontier_cells=int(frontier.sum()),
                        max_cost=int(cost[reached].max()) if reached.any() else 0)
    return out


# ---- the second formulation: Bellman-Ford sweeps over the whole grid -------------------------------------------------------------
def sweep(cost, trav, pen):
    """one Jacobi sweep of cost[p] = min(cost[p], min_k w(k) + pen[q_k] + cost[q_k]) over an array (int64, INF = not reached)"""
    H, W = cost.shape
    C, T, Pn = np.pad(cost, 1, constant_values=INF), np.pad(trav, 1, constant_values=False), np.pad(pen, 1, constant_values=0)
    best = cost.copy()
    for k, (dx, dy) in enumerate(DIRS):
        cq, tq, pq = C[1 + dy:1 + dy + H, 1 + dx:1 + dx + W], T[1 + dy:1 + dy + H, 1 + dx:1 + dx + W], Pn[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        ok = tq & (cq != INF)
        if k >= 4:
            ok = ok & T[1:1 + H, 1 + dx:1 + dx + W] & T[1 + dy:1 + dy + H, 1:1 + W]
        best = np.minimum(best, np.where(ok, cq + WEIGHT[k] + pq, INF))
    return np.where(trav, best, cost)


def field_by_sweeps(trav, pen, goal):
    cost = np.where(goal, 0, INF).astype(np.int64)
    pen = np.asarray(pen, np.int64)
    n = 0
    while True:
        new = sweep(cost, trav, pen)
        n += 1
        if np.array_equal(new, cost):
            return cost.astype(np.uint32), n
        cost = new


# ---- the third: the device's tile rounds, one tile after the other in the order `order` gives -----------------------------------
def seers(lx, ly):
    """the tile offsets (sx, sy) != (0, 0) whose 34 x 34 window holds cell (lx, ly) of a tile"""
    sx = -1 if lx == 0 else (1 if lx == TILE - 1 else 0)
    sy = -1 if ly == 0 else (1 if ly == TILE - 1 else 0)
    return ([(sx, 0)] if sx else []) + ([(0, sy)] if sy else []) + ([(sx, sy)] if sx and sy else [])


def field_by_tile_rounds(trav, pen, goal, order=None, stale=False):
    """(cost, rounds, tile visits).  order(round, tiles) -> the tiles in the order they are worked on (None: ascending).  A tile
    reads its window from the field as it stands when its turn comes or, with stale, as it stood when the round began: the two
    ends of what a workgroup may see of its neighbours' stores of the same round."""
    H, W = trav.shape
    ntx, nty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    cost = np.where(goal, 0, INF).astype(np.int64)
    pen = np.asarray(pen, np.int64)
    C, T, Pn = np.pad(cost, 1, constant_values=INF), np.pad(trav, 1, constant_values=False), np.pad(pen, 1, constant_values=0)

    def flag(into, tx, ty, lx, ly, own):
        for sx, sy in ([(0, 0)] if own else []) + seers(lx, ly):
            if 0 <= tx + sx < ntx and 0 <= ty + sy < nty:
                into.add((tx + sx, ty + sy))
    cur = set()
    for y, x in zip(*np.nonzero(goal)):
        flag(cur, x // TILE, y // TILE, x % TILE, y % TILE, True)
    rounds = visits = 0
    while cur:
        nxt = set()
        tiles = sorted(cur)
        seen = C.copy() if stale else C
        for tx, ty in (order(rounds, tiles) if order else tiles):
            x0, y0 = tx * TILE, ty * TILE                               # (the window's corner in the padded arrays)
            x1, y1 = min(x0 + TILE + 2, W + 2), min(y0 + TILE + 2, H + 2)
            wc, wt, wp = seen[y0:y1, x0:x1].copy(), T[y0:y1, x0:x1], Pn[y0:y1, x0:x1]
            inner = np.zeros(wt.shape, bool)
            inner[1:-1, 1:-1] = True                                    # the rim is read, never written
            old = wc.copy()
            while True:
                new = np.where(inner, sweep(wc, wt, wp), wc)
                if np.array_equal(new, wc):
                    break
                wc = new
            low = np.argwhere(wc < old)
            for wy, wx in low:
                C[y0 + wy, x0 + wx] = wc[wy, wx]
                flag(nxt, tx, ty, wx - 1, wy - 1, False)
            visits += 1
        rounds += 1
        cur = nxt
    return C[1:-1, 1:-1].astype(np.uint32), rounds, visits


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def random_grid(h, w, seed, obstacles=0.25, unknown=0.0, max_dist2=40):
    """(state, dist2): obstacles and unknown cells at random, dist2 at random (the plan reads both as given)"""
    rng = np.random.default_rng(seed)
    u = rng.random((h, w))
    state = np.where(u < obstacles, 100, np.where(u < obstacles + unknown, -1, 0)).astype(np.int8)
    return state, rng.integers(0, max_dist2 + 1, (h, w)).astype(np.int32)


def open_grid(h, w, dist2=100):
    return np.zeros((h, w), np.int8), np.full((h, w), dist2, np.int32)


def serpentine(n, lane=1):
    """n x n: walls on every (lane + 1)-th row, open at alternating ends: one long corridor from (0, 0).  Returns (state, dist2)"""
    state, dist2 = open_grid(n, n)
    for i, y in enumerate(range(lane, n, lane + 1)):
        state[y, :] = 100
        state[y, n - 1 if i % 2 == 0 else 0] = 0
    return state, dist2


def wall_with_door(h, w, wall_x=None, wall_y=None, door=0):
    """a wall along column wall_x (or row wall_y) with one free cell at `door`"""
    state, dist2 = open_grid(h, w)
    if wall_x is not None:
        state[:, wall_x] = 100
        state[door, wall_x] = 0
    else:
        state[wall_y, :] = 100
        state[wall_y, door] = 0
    return state, dist2


def hashed_grid(w=70, h=45):
    """the grid of tests/cpp/navplan_smoke.cpp"""
    p = np.arange(w * h, dtype=np.uint64)
    u = ((p * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)
    v = ((p * np.uint64(40503) + np.uint64(977)) & np.uint64(0xFFFFFFFF)) >> np.uint64(5)
    state = np.where(u % 100 < 20, 100, np.where(u % 100 < 32, -1, 0)).astype(np.int8).reshape(h, w)
    return state, (v % 37).astype(np.int32).reshape(h, w)


def fnv1a(data, h=1469598103934665603):
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- grids as a caller may hand them over: states outside {0, -1, 100}, dist2 outside 0 .. the cap ---------------------------------------
ODD_STATES = (1, 50, 99, 101, 127, -2, -128)                            # nav_msgs/OccupancyGrid allows 1..99; the rest is what an int8 can hold
ODD_DIST2 = (-1, -7, -(1 << 31), 0, 41, 1 << 20, (1 << 20) + 1, (1 << 31) - 1)
FOREIGN_SIZES = ((45, 70), (64, 65))                                     # (h, w); 65 cells wide: three tile columns, two tile rows


def foreign_grid(h, w, seed):
    """(state, dist2): about two thirds plain free cells, a tenth unknown, a twelfth occupied and a seventh drawn from ODD_STATES; dist2
    in 1..40 but for a sixth of the cells, which draw from ODD_DIST2.  Every call states what it does with such values (the headers'
    step 1): only 0 is free, only -1 is unknown, only 100 stops a gain ray, and a negative dist2 is below every min_dist2."""
    rng = np.random.default_rng(seed)
    u = rng.random((h, w))
    odd = np.array(ODD_STATES, np.int64)[rng.integers(0, len(ODD_STATES), (h, w))]
    state = np.where(u < 0.68, 0, np.where(u < 0.78, -1, np.where(u < 0.86, 100, odd))).astype(np.int8)
    dist2 = rng.integers(1, 41, (h, w)).astype(np.int64)
    pick = np.array(ODD_DIST2, np.int64)[rng.integers(0, len(ODD_DIST2), (h, w))]
    return state, np.where(rng.random((h, w)) < 0.16, pick, dist2).astype(np.int32)


def plain_grid(state, dist2):
    """foreign_grid's arrays with every odd value replaced by the plain one a careless reader would take it for: an odd state is free,
    a dist2 outside 0..40 is 40.  The CPU guards plan on both: where the answers differ, an odd value decided an outcome."""
    return (np.where(np.isin(state, (0, -1, 100)), state, 0).astype(np.int8),
            np.where((dist2 < 0) | (dist2 > 40), 40, dist2).astype(np.int32))


_FOREIGN = {}


def foreign_case(h, w, allow_unknown):
    """the inputs of the foreign-grid cases of the four GPU files and the plan's restatement on them, computed once and shared (the
    callers leave it unchanged): dict(state, dist2, goals, starts, kw, plan, frontier_plan)"""
    key = (h, w, allow_unknown)
    if key not in _FOREIGN:
        state, dist2 = foreign_grid(h, w, 7000 + 10 * h + w)
        rng = np.random.default_rng(h * w + allow_unknown)
        goals = [(w // 2, h // 2), (3, h - 4), (w - 3, 2)]
        for gx, gy in goals:                                             # the goals stand on plain free cells: every case plans something
            state[gy, gx], dist2[gy, gx] = 0, 9
        starts = np.stack([rng.integers(0, w, 10), rng.integers(0, h, 10)], axis=1).astype(np.int32)
        kw = dict(allow_unknown=allow_unknown, soft_dist2=30, near_penalty=40, max_path=h * w)
        _FOREIGN[key] = dict(state=state, dist2=dist2, goals=goals, starts=starts, kw=kw, plan=plan(state, dist2, goals, starts, **kw),
                             frontier_plan=plan(state, dist2, None, starts, goals_from_frontier=1, min_dist2=2, **kw))
    return _FOREIGN[key]
