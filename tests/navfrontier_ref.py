"""The restatement of include/ssf_navfrontier.h that the GPU tests compare against, bit for bit: numpy for the members (step 1), a
plain BFS for the regions (step 2), Python loops for the per-region figures (step 3), Python sets for the gain (step 6) and sorted()
for the order (step 7).  It is a statement of the rule, not a tuned labeller.  A second formulation checks it on the CPU
(tests/test_navfrontier.py): a union-find over the pairs of neighbouring members for the regions, and one list per ray with
len(set(...)) over all of them for the gain.  Also the shared scenes."""
from collections import deque

import numpy as np

INF = 0xFFFFFFFF
TILE = 32
NEIGHBOURS = {4: ((1, 0), (0, 1), (-1, 0), (0, -1)),
              8: ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))}
DEFAULTS = dict(connectivity=8, traversable_only=0, min_dist2=0, min_cells=1, reachable_only=0, max_regions=4096, gain_radius=0,
                cost_weight=1, gain_weight=0, size_weight=0)
STATS = ("frontier_cells", "regions_found", "regions_small", "regions_unreached", "regions_kept", "regions_written", "largest_cells",
         "gain_rays")
FIELDS = ("sum_x", "sum_y", "label", "cells", "x0", "y0", "x1", "y1", "rep_x", "rep_y", "rep_cost", "gain")


def params(**kw):
    bad = [k for k in kw if k not in DEFAULTS]
    assert not bad, bad
    return dict(DEFAULTS, **kw)


# ---- step 1 ------------------------------------------------------------------------------------------------------------------------
def members(state, dist2, q):
    """H x W bool"""
    state = np.asarray(state, np.int8)
    unknown = np.pad(state == -1, 1, constant_values=False)
    near = unknown[1:-1, 2:] | unknown[1:-1, :-2] | unknown[2:, 1:-1] | unknown[:-2, 1:-1]
    m = (state == 0) & near
    if q["traversable_only"]:
        m &= np.asarray(dist2, np.int64) >= q["min_dist2"]
    return m


# ---- step 2: a BFS from every member not yet seen, in ascending p: the first cell of a region is its label ----------------------------
def regions_by_bfs(member, connectivity):
    """the regions as lists of (x, y), in ascending label"""
    H, W = member.shape
    seen = np.zeros((H, W), bool)
    out = []
    for y, x in zip(*np.nonzero(member)):
        if seen[y, x]:
            continue
        seen[y, x] = True
        cells, todo = [], deque([(int(x), int(y))])
        while todo:
            cx, cy = todo.popleft()
            cells.append((cx, cy))
            for dx, dy in NEIGHBOURS[connectivity]:
                nx, ny = cx + dx, cy + dy
                if 0 <= nx < W and 0 <= ny < H and member[ny, nx] and not seen[ny, nx]:
                    seen[ny, nx] = True
                    todo.append((nx, ny))
        out.append(cells)
    return out


# ---- step 3 ------------------------------------------------------------------------------------------------------------------------
def describe(cells, W, cost):
    """one region's record, gain 0"""
    xs, ys = [c[0] for c in cells], [c[1] for c in cells]
    label = min(y * W + x for x, y in cells)
    reached = sorted((int(cost[y, x]), y * W + x) for x, y in cells if int(cost[y, x]) != INF) if cost is not None else []
    rep_cost, rep = reached[0] if reached else (INF, label)
    return dict(sum_x=sum(xs), sum_y=sum(ys), label=label, cells=len(cells), x0=min(xs), y0=min(ys), x1=max(xs), y1=max(ys), rep_x=rep % W,
                rep_y=rep // W, rep_cost=rep_cost, gain=0)


# ---- step 6 ------------------------------------------------------------------------------------------------------------------------
def ray_cells(state, ox, oy, dx, dy, R):
    """the cells a ray visits before it ends, in order"""
    H, W = state.shape
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    out = []
    for s in range(1, R + 1):
        x, y = ox + sx * ((2 * abs(dx) * s + R) // (2 * R)), oy + sy * ((2 * abs(dy) * s + R) // (2 * R))
        if not (0 <= x < W and 0 <= y < H) or state[y, x] == 100:
            break
        out.append((x, y))
    return out


def rim(R):
    """the 8 R ray ends: every (dx, dy) with max(|dx|, |dy|) == R"""
    return [(dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if max(abs(dx), abs(dy)) == R]


def gain(state, ox, oy, R):
    if R <= 0:
        return 0
    seen = set()
    for dx, dy in rim(R):
        for x, y in ray_cells(state, ox, oy, dx, dy, R):
            if state[y, x] == -1:
                seen.add((x, y))
    return len(seen)


# ---- step 7 ------------------------------------------------------------------------------------------------------------------------
def order_of(table, q):
    def rank(i):
        r = table[i]
        key = r["rep_cost"] * q["cost_weight"] - r["gain"] * q["gain_weight"] - r["cells"] * q["size_weight"]
        return (r["rep_cost"] == INF, key, r["label"])
    return np.array(sorted(range(len(table)), key=rank), np.int32)


def frontiers(state, dist2=None, cost=None, **kw):
    """every output and exact stat of ssf_navfrontier_regions: region (H x W int32), regions (a list of dicts), order, stats"""
    q = params(**kw)
    state = np.asarray(state, np.int8)
    H, W = state.shape
    assert q["connectivity"] in (4, 8) and (dist2 is not None or not q["traversable_only"]) and (cost is not None or not q["reachable_only"])
    member = members(state, dist2, q)
    found = regions_by_bfs(member, q["connectivity"])
    recs = [describe(cells, W, cost) for cells in found]
    small = [r["cells"] < q["min_cells"] for r in recs]
    unreached = [not s and bool(q["reachable_only"]) and r["rep_cost"] == INF for r, s in zip(recs, small)]
    kept = [i for i in range(len(recs)) if not small[i] and not unreached[i]]
    table_of = {i: t for t, i in enumerate(kept[:q["max_regions"]])}
    region = np.full((H, W), -1, np.int32)
    for i, cells in enumerate(found):
        for x, y in cells:
            region[y, x] = table_of.get(i, -2)
    table = [recs[i] for i in kept[:q["max_regions"]]]
    for r in table:
        r["gain"] = gain(state, r["rep_x"], r["rep_y"], q["gain_radius"])
    stats = dict(frontier_cells=int(member.sum()), regions_found=len(recs), regions_small=sum(small), regions_unreached=sum(unreached),
                 regions_kept=len(kept), regions_written=len(table), largest_cells=max([r["cells"] for r in recs], default=0),
                 gain_rays=8 * q["gain_radius"] * len(table))
    return dict(region=region, regions=table, order=order_of(table, q), stats=stats)


def as_records(table, dtype):
    """the list of dicts as a numpy record array of `dtype` (binding.NAVFRONTIER_REGION_DTYPE)"""
    a = np.zeros(len(table), dtype)
    for i, r in enumerate(table):
        for nm in FIELDS:
            a[nm][i] = r[nm]
    return a


# ---- the second formulation --------------------------------------------------------------------------------------------------------
def regions_by_union_find(member, connectivity):
    """label per cell (H x W int64, -1 no member): a union-find over every pair of neighbouring members, in no special order"""
    H, W = member.shape
    parent = {int(y) * W + int(x): int(y) * W + int(x) for y, x in zip(*np.nonzero(member))}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for p in sorted(parent, reverse=True):
        x, y = p % W, p // W
        for dx, dy in NEIGHBOURS[connectivity]:
            nx, ny = x + dx, y + dy
            if 0 <= nx < W and 0 <= ny < H and member[ny, nx]:
                a, b = find(p), find(ny * W + nx)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    out = np.full((H, W), -1, np.int64)
    for p in parent:
        out[p // W, p % W] = find(p)
    return out


def gain_by_ray_lists(state, ox, oy, R):
    """(distinct unknown cells, visits of unknown cells): one list per ray, then len(set(...)) over all of them"""
    lists = [[c for c in ray_cells(state, ox, oy, dx, dy, R) if state[c[1], c[0]] == -1] for dx, dy in rim(R)] if R > 0 else []
    every = [c for l in lists for c in l]
    return len(set(every)), len(every)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def random_grid(h, w, seed, obstacles=0.15, unknown=0.2, max_dist2=12):
    """(state, dist2): obstacles and unknown cells at random, dist2 at random (the call reads both as given)"""
    rng = np.random.default_rng(seed)
    u = rng.random((h, w))
    state = np.where(u < obstacles, 100, np.where(u < obstacles + unknown, -1, 0)).astype(np.int8)
    return state, rng.integers(0, max_dist2 + 1, (h, w)).astype(np.int32)


def random_cost(h, w, seed, unreached=0.3, top=50):
    """a cost field at random with many ties and many unreached cells"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, top, (h, w)).astype(np.uint32)
    c[rng.random((h, w)) < unreached] = INF
    return c


def spiral(w=97, h=64):
    """a one-cell corridor of free cells that spirals inwards from (0, 0) through unknown space, every other cell unknown: each
    corridor cell is a member, and they are one region whose smallest index is cell 0.  Returns (state, the corridor's cells)"""
    state = np.full((h, w), -1, np.int8)
    x0, y0, x1, y1 = 0, 0, w - 1, h - 1
    x, y, cells = 0, 0, []

    def go(tx, ty):
        nonlocal x, y
        while (x, y) != (tx, ty):
            cells.append((x, y))
            x += (tx > x) - (tx < x)
            y += (ty > y) - (ty < y)
    while x1 - x0 >= 2 and y1 - y0 >= 2:
        go(x1, y0); go(x1, y1); go(x0, y1); go(x0, y0 + 2)
        x0, y0, x1, y1 = x0 + 2, y0 + 2, x1 - 2, y1 - 2
        go(x0, y0)
    cells.append((x, y))
    for cx, cy in cells:
        state[cy, cx] = 0
    return state, cells


def checkerboard(n=64):
    """0 / -1 alternating, (0, 0) free"""
    yy, xx = np.mgrid[0:n, 0:n]
    return np.where((xx + yy) % 2 == 0, 0, -1).astype(np.int8)


def room(w=70, h=45):
    """a walled room with two inner walls, a door in each, unknown space behind windows in the outer wall, unknown patches inside and
    a sealed closet whose frontier nobody reaches:
    (state, dist2 = the squared distance to the nearest obstacle cell capped at 25, a robot cell)"""
    state = np.zeros((h, w), np.int8)
    state[0, :] = state[-1, :] = 100
    state[:, 0] = state[:, -1] = 100
    state[:, 30] = 100
    state[20, 30] = 0
    state[25, 30:] = 100
    state[25, 50] = 0
    state[0, 5:12] = -1                      # windows: unknown cells in the outer wall
    state[10:14, -1] = -1
    state[-1, 40:41] = -1                    # a one-cell speck
    state[30:36, 5:9] = -1                   # an unknown patch in the first room
    state[31:35, 6:8] = 100                  # ... with an obstacle inside it
    state[35:40, 55:60] = -1                 # and one in the third
    state[37:43, 20:26] = 100                # a sealed closet: free cells around an unknown core, walls all round
    state[38:42, 21:25] = 0
    state[39:41, 22:24] = -1
    oy, ox = np.nonzero(state == 100)
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = np.full((h, w), 25, np.int64)
    for x, y in zip(ox, oy):
        np.minimum(d2, (xx - x) ** 2 + (yy - y) ** 2, out=d2)
    return state, d2.astype(np.int32), (15, 10)
