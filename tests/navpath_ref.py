"""The waypoints of include/ssf_navpath.h restated in numpy and plain Python, written from the header: steps 1 to 7, every output and
every exact stat.  The GPU tests compare the device with this, with ==.  Not a tuned string-puller: the candidates of every
window are walked cell by cell in plain Python."""
from fractions import Fraction

import numpy as np

FORCED = 1 << 30
INDEX_MASK = FORCED - 1
DEFAULTS = dict(min_dist2=0, allow_unknown=0, los_dist2=0, keep_clearance=0, clearance_cap=0, lookahead=256)
STATS = ("paths_ok", "paths_bad", "paths_truncated", "waypoints", "forced_steps", "cells_in")
STATUS_OK, STATUS_LENGTH, STATUS_CELL, STATUS_JUMP, STATUS_TRUNCATED = 0, 1, 2, 3, 4


def params(**kw):
    bad = [k for k in kw if k not in DEFAULTS]
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def prep(state, dist2, q):
    """step 1: (trav: H x W list of lists of bool, d: H x W list of lists of int)"""
    state, dist2 = np.asarray(state, np.int8), np.asarray(dist2, np.int32).astype(np.int64)
    trav = ((state == 0) | ((state == -1) if q["allow_unknown"] else False)) & (dist2 >= q["min_dist2"])
    return trav.tolist(), np.maximum(dist2, 0).tolist()


def walk_cells(ax, ay, bx, by):
    """step 3: the cells visited from (ax, ay) to (bx, by), one after the other (a generator: who stops early walks no further)"""
    ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
    dx, dy = abs(bx - ax), abs(by - ay)
    sx, sy = (bx > ax) - (bx < ax), (by > ay) - (by < ay)
    x, y, e, n = ax, ay, dx - dy, dx + dy
    yield (x, y)
    while n > 0:
        if e > 0:
            x += sx; e -= 2 * dy; n -= 1
        elif e < 0:
            y += sy; e += 2 * dx; n -= 1
        else:
            yield (x + sx, y)
            yield (x, y + sy)
            x += sx; y += sy; e += 2 * dx - 2 * dy; n -= 2
        yield (x, y)


def walk(ax, ay, bx, by):
    """step 3: the list of the cells visited from (ax, ay) to (bx, by), in order"""
    return list(walk_cells(ax, ay, bx, by))


def walk_by_fractions(dx, dy):
    """the second formulation, from (0, 0) to (dx, dy): the set of cells whose open unit square (centred on the cell) the segment
    between the two centres meets, plus both axial cells at every lattice corner (a point with both coordinates at k + 1/2) that the
    segment passes through"""
    cells = set()
    half = Fraction(1, 2)
    x0, x1, y0, y1 = min(0, dx), max(0, dx), min(0, dy), max(0, dy)
    for cx in range(x0, x1 + 1):
        for cy in range(y0, y1 + 1):
            # the segment is (t dx, t dy), 0 <= t <= 1; per axis |t d - c| < 1/2 is an open interval (lo, hi) of t (every t when
            # d == 0 and c == 0, none when d == 0 and c != 0); the square is met iff the intervals and [0, 1] share a point
            lo, hi, ok = Fraction(-1), Fraction(2), True
            for d, c in ((dx, cx), (dy, cy)):
                if d == 0:
                    ok = ok and c == 0
                    continue
                a, b = sorted(((c - half) / d, (c + half) / d))
                lo, hi = max(lo, a), min(hi, b)
            if ok and lo < hi and lo < 1 and hi > 0:
                cells.add((cx, cy))
    if dx != 0 and dy != 0:
        sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
        for kx in range(abs(dx)):                                      # the corner between columns kx and kx + 1 (in steps of sx)
            t = (kx + half) / abs(dx)
            yy = t * abs(dy) - half                                    # = ky when the segment passes the corner (kx + 1/2, ky + 1/2)
            if yy.denominator == 1 and 0 <= yy < abs(dy):
                ky = int(yy)
                cells.add(((kx + 1) * sx, ky * sy))
                cells.add((kx * sx, (ky + 1) * sy))
    return cells


def check(trav, cells, L, max_path):
    """step 2: the status of a path (0, 1, 2 or 3)"""
    H, W = len(trav), len(trav[0])
    if L < 0 or L > max_path:
        return STATUS_LENGTH
    status = STATUS_OK
    for k in range(L):
        x, y = int(cells[k][0]), int(cells[k][1])
        if not (0 <= x < W and 0 <= y < H) or not trav[y][x]:
            return STATUS_CELL
        if k > 0 and max(abs(x - int(cells[k - 1][0])), abs(y - int(cells[k - 1][1]))) != 1:
            status = STATUS_JUMP
    return status


def segment(trav, d, a, b, thr):
    """(visible, seg_min) of the walk from cell a to cell b under the threshold thr (step 4)"""
    vis, m = True, None
    for x, y in walk(a[0], a[1], b[0], b[1]):
        m = d[y][x] if m is None else min(m, d[y][x])
        vis = vis and trav[y][x] and d[y][x] >= thr
    return vis, m


def visible(trav, d, a, b, thr):
    """segment's first answer alone, leaving the walk at the first cell that fails"""
    for x, y in walk_cells(a[0], a[1], b[0], b[1]):
        if not trav[y][x] or d[y][x] < thr:
            return False
    return True


def pull(trav, d, cells, q, max_waypoints, every_candidate=False):
    """steps 4 to 6 for one checked path: (status 0 or 4, waypoints (n, 4), forced steps among them).  The largest visible j is
    found from the far end of the window, stopping at the first hit; every_candidate walks all of them to their ends instead, as
    step 5 is written (the tests compare the two)."""
    L = len(cells)
    P = [(int(c[0]), int(c[1])) for c in cells]
    base = max(q["min_dist2"], q["los_dist2"])
    if L == 0:
        return STATUS_OK, np.zeros((0, 4), np.int32), 0
    out, a, forced, status = [(P[0][0], P[0][1], 0, d[P[0][1]][P[0][0]])], 0, 0, STATUS_OK
    while a < L - 1:
        if len(out) == max_waypoints:
            status = STATUS_TRUNCATED
            break
        far = min(L - 1, a + q["lookahead"])
        thr = dict.fromkeys(range(a + 1, far + 1), base)
        if q["keep_clearance"]:
            run = d[P[a][1]][P[a][0]]
            for j in range(a + 1, far + 1):
                run = min(run, d[P[j][1]][P[j][0]])
                thr[j] = max(base, min(q["clearance_cap"], run))
        if every_candidate:
            J = max([a + 1] + [j for j in range(a + 1, far + 1) if segment(trav, d, P[a], P[j], thr[j])[0]])
        else:
            J = next((j for j in range(far, a, -1) if visible(trav, d, P[a], P[j], thr[j])), a + 1)
        vis, m = segment(trav, d, P[a], P[J], thr[J])
        forced += not vis
        out.append((P[J][0], P[J][1], J | (0 if vis else FORCED), m))
        a = J
    return status, np.array(out, np.int32).reshape(-1, 4), forced


def waypoints(state, dist2, path, path_len=None, max_waypoints=None, every_candidate=False, **kw):
    """every output and exact stat of ssf_navpath_waypoints.  path: n x max_path x 2 (or a list of (len, 2) arrays, then path_len may be
    None and max_path is the longest).  Returns n_waypoints, status, waypoints (a list of (n, 4) int32 arrays), path_min, stats."""
    q = params(**kw)
    trav, d = prep(state, dist2, q)
    if path_len is None:
        path_len = [len(c) for c in path]
        max_path = max(1, max(path_len))
    else:
        max_path = np.asarray(path).shape[1]
    if max_waypoints is None:
        max_waypoints = max_path
    n = len(path_len)
    out = dict(n_waypoints=np.zeros(n, np.int32), status=np.zeros(n, np.int32), waypoints=[], path_min=np.full(n, -1, np.int32))
    stats = dict.fromkeys(STATS, 0)
    for i in range(n):
        L = int(path_len[i])
        s = check(trav, path[i], L, max_path)
        wp = np.zeros((0, 4), np.int32)
        if s == STATUS_OK:
            s, wp, forced = pull(trav, d, path[i][:L], q, max_waypoints, every_candidate)
            stats["paths_ok"] += 1
            stats["paths_truncated"] += s == STATUS_TRUNCATED
            stats["waypoints"] += len(wp)
            stats["forced_steps"] += forced
            stats["cells_in"] += L
        else:
            stats["paths_bad"] += 1
        out["status"][i], out["n_waypoints"][i] = s, len(wp)
        out["waypoints"].append(wp)
        if len(wp):
            out["path_min"][i] = wp[:, 3].min()
    out["stats"] = {k: int(v) for k, v in stats.items()}
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def open_grid(h, w, dist2=100):
    return np.zeros((h, w), np.int8), np.full((h, w), dist2, np.int32)


def corridor(n, seed=None):
    """a 3-row open grid of min(n, 4096) columns and the straight path along row 1 from (0, 1); the 4097th cell, for which a grid has
    no column, is (4095, 2).  dist2 is 100, or with a seed: random in 1..40, falling along row 1.  Returns (state, dist2, path (n, 2))"""
    assert 1 <= n <= 4097
    w = min(n, 4096)
    state, dist2 = open_grid(3, w)
    if seed is not None:
        rng = np.random.default_rng(seed)
        dist2[:] = rng.integers(1, 41, (3, w))
        dist2[1] = np.sort(dist2[1])[::-1]
    path = np.stack([np.arange(w, dtype=np.int32), np.ones(w, np.int32)], 1)
    if n > w:
        path = np.concatenate([path, [[w - 1, 2]]]).astype(np.int32)
    return state, dist2, path


def staircase(n, seed, run=3):
    """an open grid with dist2 at random in 1..40 and a path of n cells from (0, 0) that goes `run` cells along x, then one
    diagonal cell up, and so on: the segments between its cells cross cells that are not on it.  Returns (state, dist2, path)"""
    cells, x, y = [], 0, 0
    for k in range(n):
        cells.append((x, y))
        x, y = x + 1, y + (k % (run + 1) == run)
    w, h = cells[-1][0] + 1, cells[-1][1] + 1
    rng = np.random.default_rng(seed)
    dist2 = rng.integers(1, 41, (h, w)).astype(np.int32)
    for x, y in cells:
        dist2[y, x] = rng.integers(15, 41)                               # the path keeps some clearance; what lies beside it may not
    return np.zeros((h, w), np.int8), dist2, np.array(cells, np.int32)


def pillar(hidden=2, down=None, tail=0, Y=2):
    """The path runs along row Y from (0, Y), steps round the pillar at (3, Y) through row Y - 1, runs on along row Y for `hidden`
    cells, which the pillar hides from (0, Y), then goes straight down for `down` cells -- the first of them are still hidden, the
    later ones are seen past the pillar -- and at last runs along x for `tail` cells of dist2 0, which los_dist2 = 1 hides although
    the path may use them.  down None: the fewest cells such that the last one is seen from (0, Y) under los_dist2 = 1, so that the
    winner's nearer neighbour is hidden.  Every other cell has dist2 1.  Returns (state, dist2, path, the winner's index)"""
    def make(q):
        cells = [(0, Y), (1, Y), (2, Y - 1), (3, Y - 1)] + [(4 + i, Y) for i in range(hidden)]
        X = cells[-1][0]
        cells += [(X, Y - 1 - t) for t in range(q)]
        win = len(cells) - 1
        cells += [(X + 1 + i, Y - q) for i in range(tail)]
        w = cells[-1][0] + 1
        state, dist2 = np.zeros((Y + 1, max(w, X + 1)), np.int8), np.ones((Y + 1, max(w, X + 1)), np.int32)
        state[Y, 3], dist2[Y, 3] = 100, 0
        for x, y in cells[win + 1:]:
            dist2[y, x] = 0
        return state, dist2, np.array(cells, np.int32), win
    if down is not None:
        return make(down)
    for q in range(1, Y + 1):
        state, dist2, cells, win = make(q)
        trav, d = prep(state, dist2, params())
        if visible(trav, d, cells[0], cells[win], 1):
            return state, dist2, cells, win
    raise AssertionError("no cell of the way down is seen: raise Y")


def pack_paths(paths, max_path=None):
    """(path n x max_path x 2 int32, path_len n int32) from a list of (len, 2) arrays"""
    lens = np.array([len(c) for c in paths], np.int32)
    mp = max(1, int(lens.max()) if len(lens) else 1) if max_path is None else max_path
    out = np.zeros((len(paths), mp, 2), np.int32)
    for i, c in enumerate(paths):
        out[i, :len(c)] = np.asarray(c, np.int32).reshape(-1, 2)
    return out, lens
