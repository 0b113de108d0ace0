"""A restatement of include/ssf_navsteer.h in numpy integers: the rule of the velocity commands, step by step as the header words it,
vectorised over the candidates of a pose and looping over poses and steps.  It shares no code with the library.  Every array is
int64 here; the comparison casts to the ABI's types."""
import numpy as np

OUTPUTS = ("best", "best_cmd", "best_score", "n_admissible", "pose_status", "best_len", "best_traj",
           "cand_free", "cand_min_d", "cand_end", "cand_end_cost", "cand_score")
DTYPES = dict(best=np.int32, best_cmd=np.int32, best_score=np.int64, n_admissible=np.int32, pose_status=np.int32, best_len=np.int32,
              best_traj=np.int32, cand_free=np.int32, cand_min_d=np.int32, cand_end=np.int32, cand_end_cost=np.uint32, cand_score=np.int64)
STATS = ("poses_ok", "poses_blocked", "poses_stuck", "candidates", "admissible", "collided", "steps_taken")      # the exact ones
INFORMATIVE = ("windows_staged", "windows_global")
NO_COST = 0xFFFFFFFF
SUB = 1024                            # sub-units per cell
TURN = 65536                          # heading units per turn
LDS_CELLS = 14336                     # the largest window the library stages (informative stats only: no output depends on it)

DEFAULTS = dict(width=512, height=512, min_dist2=0, allow_unknown=0, clearance_cap=64, n_poses=0, n_v=9, n_w=33, v_min=0, v_step=64,
                w_min=-2048, w_step=128, n_steps=32, min_free_steps=2, brake_div=128, cost_weight=1, target_weight=0, clear_weight=1,
                speed_weight=1, turn_weight=0, walk=0)


def params(**kw):
    bad = [k for k in kw if k not in DEFAULTS]
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def direction_table():
    """step 1: (C, S), int64 arrays of 1024"""
    k = np.arange(1024, dtype=np.float64)
    a = 2.0 * np.pi * k / 1024.0
    return np.floor(16384.0 * np.cos(a) + 0.5).astype(np.int64), np.floor(16384.0 * np.sin(a) + 0.5).astype(np.int64)


_C, _S = direction_table()


def lattice(c):
    """step 2: (v, w) of every candidate, and v_abs_max"""
    i, j = np.divmod(np.arange(c["n_v"] * c["n_w"], dtype=np.int64), c["n_w"])
    v, w = c["v_min"] + i * c["v_step"], c["w_min"] + j * c["w_step"]
    return v, w, int(np.abs(v).max())


def traversable(state, dist2, c):
    """step 3: (trav, d)"""
    state, dist2 = np.asarray(state).astype(np.int64), np.asarray(dist2).astype(np.int64)
    trav = ((state == 0) | ((state == -1) if c["allow_unknown"] else False)) & (dist2 >= c["min_dist2"])
    return trav, np.minimum(np.maximum(dist2, 0), c["clearance_cap"])


def reach(c):
    return -(-c["n_steps"] * lattice(c)[2] // SUB) + 1


def stage_cells(c):
    """the largest window that a call stages on chip (csrc/ssf_navsteer.hip's measured choice; informative stats only): every window
    that fits while a workgroup's LDS leaves a CU its eight workgroups or the whole launch is resident at once, else the small ones"""
    if c["walk"]:
        return 0
    side = 2 * reach(c) + 1
    lds = 4 * min(min(side, c["width"]) * min(side, c["height"]), LDS_CELLS) + 4096 + 160
    wgs = -(-c["n_v"] * c["n_w"] // 256) * c["n_poses"]
    return LDS_CELLS if lds <= 20480 or wgs <= 256 * (163840 // lds) else (20480 - 4256) // 4


def rollouts(state, dist2, cost, poses, targets, c):
    """every output of ssf_navsteer_rollouts (OUTPUTS, in the ABI's dtypes; best_traj entries past best_len are 0 here and unwritten
    there) and 'stats'.  cost / targets may be None with their weight 0."""
    H, W = np.asarray(state).shape
    trav, d = traversable(state, dist2, c)
    poses = np.asarray(poses, np.int64).reshape(-1, 3)
    n, T = len(poses), c["n_steps"]
    v, w, vmax = lattice(c)
    K = len(v)
    av, aw = np.abs(v), np.abs(w)
    if c["cost_weight"] > 0:
        cost = np.asarray(cost).astype(np.int64)
    if c["target_weight"] > 0:
        targets = np.asarray(targets, np.int64).reshape(-1, 2)
    need = np.minimum(T, c["min_free_steps"] + ((av + c["brake_div"] - 1) // c["brake_div"] if c["brake_div"] > 0 else 0))

    def ok(ix, iy):                   # traversable, outside the grid: not
        inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        return inside & trav[np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)]

    out = dict(best=np.full(n, -1), best_cmd=np.zeros((n, 2)), best_score=np.full(n, -1), n_admissible=np.zeros(n), pose_status=np.zeros(n),
               best_len=np.zeros(n), best_traj=np.zeros((n, T + 1, 3)), cand_free=np.zeros((n, K)), cand_min_d=np.full((n, K), -1),
               cand_end=np.zeros((n, K, 3)), cand_end_cost=np.full((n, K), NO_COST), cand_score=np.full((n, K), -1))
    out = {nm: a.astype(np.int64) for nm, a in out.items()}
    staged = glob = 0
    R, stage = reach(c), stage_cells(dict(c, n_poses=n))
    for q in range(n):
        px, py, ph = int(poses[q, 0]), int(poses[q, 1]), int(poses[q, 2]) & 0xFFFF
        cx, cy = px >> 10, py >> 10
        out["cand_end"][q] = (px, py, ph)
        if not (0 <= cx < W and 0 <= cy < H):
            out["pose_status"][q] = 1
            continue
        if not trav[cy, cx]:
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
        traj = np.zeros((K, T + 1, 3), np.int64)
        traj[:, 0] = (px, py, ph)
        for s in range(T):
            k = ((2 * h + w + 64) >> 7) & 1023
            nx, ny = x + ((v * _C[k] + 8192) >> 14), y + ((v * _S[k] + 8192) >> 14)
            ox, oy, ncx, ncy = x >> 10, y >> 10, nx >> 10, ny >> 10
            step = ok(ncx, ncy)
            diag = (ncx != ox) & (ncy != oy)
            step &= ~diag | (ok(ncx, oy) & ok(ox, ncy))
            alive &= step
            if not alive.any():
                break
            x, y, h = np.where(alive, nx, x), np.where(alive, ny, y), np.where(alive, (h + w) & 0xFFFF, h)
            free += alive
            dn = d[np.clip(y >> 10, 0, H - 1), np.clip(x >> 10, 0, W - 1)]
            min_d = np.where(alive, np.minimum(min_d, dn), min_d)
            traj[alive, s + 1] = np.stack([x, y, h], axis=1)[alive]
        ec = cost[y >> 10, x >> 10] if c["cost_weight"] > 0 else np.full(K, NO_COST)
        adm = free >= need
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
                 steps_taken=int(out["cand_free"].sum()), windows_staged=staged, windows_global=glob)
    res = {nm: out[nm].astype(DTYPES[nm]) for nm in OUTPUTS}
    res["stats"] = stats
    return res


def tied_poses(got):
    """the poses with two admissible candidates sharing the minimum score"""
    return [q for q in range(len(got["best"])) if got["best"][q] >= 0 and int((got["cand_score"][q] == got["best_score"][q]).sum()) >= 2]


# ---- the host helpers of the wrappers, restated -------------------------------------------------------------------------------------
def units(x_m, y_m, yaw, res):
    """a metric grid-frame pose in units: (x, y, heading)"""
    return (int(np.floor(x_m / res * SUB)), int(np.floor(y_m / res * SUB)), int(np.rint(yaw / (2.0 * np.pi) * TURN)) & 0xFFFF)


def centre(ix, iy, heading=0):
    return (ix * SUB + 512, iy * SUB + 512, heading)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def clearance(state, cap_cells=8):
    """dist2 of a state: the squared distance in cells to the nearest cell that is not free, capped at cap_cells^2 (brute force: the
    scenes are small); what the grid calls write, near enough for a scene (the tests take it as an input, not as a claim)"""
    H, W = state.shape
    oy, ox = np.nonzero(state != 0)
    out = np.full((H, W), cap_cells * cap_cells, np.int64)
    if len(ox):
        yy, xx = np.mgrid[0:H, 0:W]
        d2 = ((yy[..., None] - oy) ** 2 + (xx[..., None] - ox) ** 2).min(axis=2)
        out = np.minimum(out, d2)
    return out.astype(np.int32)


def field(state, dist2, goal, c):
    """a cost-to-goal field in the plan's unit (10 straight, 14 diagonal, no corner cutting), by plain relaxation: an input of the
    scenes, stated here so that this file needs no other"""
    import heapq
    trav, _ = traversable(state, dist2, c)
    H, W = trav.shape
    cost = np.full((H, W), NO_COST, np.int64)
    gx, gy = goal
    if not trav[gy, gx]:
        return cost.astype(np.uint32)
    cost[gy, gx] = 0
    heap = [(0, gx, gy)]
    while heap:
        cc, x, y = heapq.heappop(heap)
        if cc != cost[y, x]:
            continue
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                nx, ny = x + dx, y + dy
                if (dx or dy) and 0 <= nx < W and 0 <= ny < H and trav[ny, nx]:
                    if dx and dy and not (trav[y, nx] and trav[ny, x]):
                        continue
                    nc = cc + (14 if dx and dy else 10)
                    if nc < cost[ny, nx]:
                        cost[ny, nx] = nc
                        heapq.heappush(heap, (nc, nx, ny))
    return cost.astype(np.uint32)


def room(W, H, seed):
    """a walled room with two pillars, a pocket nobody can leave, and a sealed chamber the field does not reach: state int8"""
    s = np.zeros((H, W), np.int8)
    if W < 8 or H < 8:
        return s
    s[0, :] = s[-1, :] = 100
    s[:, 0] = s[:, -1] = 100
    s[H // 3:H // 3 + 3, W // 3:W // 3 + 3] = 100
    s[2 * H // 3 - 2:2 * H // 3, W // 2:W // 2 + 4] = 100
    s[2:5, 2:5] = 100                                                   # a pocket: one free cell with walls all round
    s[3, 3] = 0
    s[H - 7:H - 1, W - 7] = 100                                          # a chamber in the far corner, sealed: free inside, unreached
    s[H - 7, W - 7:W - 1] = 100
    rng = np.random.default_rng(seed)
    s[rng.integers(1, H - 1, 3), rng.integers(1, W - 1, 3)] = -1          # a few unknown cells
    return s


def scene(name):
    """dict(state, dist2, cost, poses, targets, c): the inputs of a GPU case"""
    W, H, kw, seed = SCENES[name]
    c = params(width=W, height=H, **kw)
    state = room(W, H, seed)
    dist2 = clearance(state)
    goal = (W - 10, H // 2) if W >= 8 and H >= 8 else (0, 0)
    cost = field(state, dist2, goal, c)
    rng = np.random.default_rng(100 + seed)
    poses = []
    if W >= 8 and H >= 8:
        poses += [centre(W // 2, H // 2 + 2, 65535),                     # open floor, the heading about to wrap
                  centre(3, 3, 1234),                                    # the pocket: status 3
                  centre(W // 3 + 1, H // 3 + 1, 0),                     # inside a pillar: status 2
                  (-5, 700, 0), (W * SUB, 100, 9),                        # outside: status 1
                  centre(1, 1, 8192),                                    # a corner of the free space, heading into the diagonal
                  (1 * SUB, (H // 2) * SUB + 1023, 32768),                # on cell boundaries: x & 1023 == 0, y & 1023 == 1023, facing the wall
                  ((W // 2) * SUB + 1023, 1 * SUB, 49152 + 65536),        # x & 1023 == 1023, y & 1023 == 0, a heading beyond one turn
                  centre(W - 4, H - 4, 40000),                           # inside the sealed chamber: every end cost unreached
                  centre(W // 2, H // 2 + 2, 0)]
    else:
        poses += [centre(0, 0, 0), (1023, 0, 16384), (0, 1023, 65535), (-1, 0, 0)]
    n = c["n_poses"]
    while len(poses) < n:
        poses.append((int(rng.integers(0, W * SUB)), int(rng.integers(0, H * SUB)), int(rng.integers(-TURN, 2 * TURN))))
    poses = np.array(poses[:n], np.int32)
    targets = np.stack([rng.integers(0, W * SUB, n), rng.integers(0, H * SUB, n)], axis=1).astype(np.int32)
    return dict(state=state, dist2=dist2, cost=cost, poses=poses, targets=targets, c=c)


# name -> (width, height, keywords, seed).  K = 1, 63, 64, 65, 256, 257; T = 1, 2, 256; n_poses = 1, 3, 257; reverse candidates;
# n_v == 1 with v_step 0; cost NULL; targets only.  tests/test_navsteer.py checks on the restatement that the scenes marked in
# GUARDED are not vacuous.
SCENES = {
    "room 9x33": (33, 31, dict(n_poses=12, n_steps=24), 1),
    "room 65x64 reverse": (65, 64, dict(n_poses=12, n_v=9, n_w=33, v_min=-256, v_step=96, n_steps=24, brake_div=64), 2),
    "room K257 T256": (65, 64, dict(n_poses=12, n_v=1, n_w=257, v_min=1024, v_step=0, w_min=-1024, w_step=8, n_steps=256, min_free_steps=4), 3),
    "room 257 poses": (33, 31, dict(n_poses=257, n_v=4, n_w=16, v_min=128, v_step=128, w_min=-1920, w_step=256, n_steps=12, target_weight=2, turn_weight=1), 4),
    "K1 T1": (33, 31, dict(n_poses=1, n_v=1, n_w=1, v_min=512, v_step=0, w_min=0, w_step=0, n_steps=1, min_free_steps=1), 5),
    "K63 T2": (33, 31, dict(n_poses=3, n_v=3, n_w=21, v_min=100, v_step=300, w_min=-2000, w_step=200, n_steps=2), 6),
    "K64": (33, 31, dict(n_poses=12, n_v=4, n_w=16, v_min=0, v_step=200, w_min=-1600, w_step=200, n_steps=20), 7),
    "K65": (65, 64, dict(n_poses=12, n_v=5, n_w=13, v_min=-200, v_step=200, w_min=-1200, w_step=200, n_steps=20), 8),
    "K256": (33, 31, dict(n_poses=12, n_v=16, n_w=16, v_min=0, v_step=60, w_min=-1500, w_step=200, n_steps=16), 9),
    "no cost": (33, 31, dict(n_poses=12, cost_weight=0, n_steps=16), 10),
    "targets only": (65, 64, dict(n_poses=12, cost_weight=0, clear_weight=0, speed_weight=0, target_weight=1000, n_steps=16), 11),
    "1x1": (1, 1, dict(n_poses=4, n_v=3, n_w=3, v_min=-600, v_step=600, w_min=-100, w_step=100, n_steps=4, min_free_steps=0, brake_div=0, cost_weight=0), 12),
    "unknown allowed": (33, 31, dict(n_poses=12, allow_unknown=1, min_dist2=1, clearance_cap=1024 * 1024, n_steps=16), 13),
}
GPU_CASES = tuple(SCENES)
GUARDED = ("room 9x33", "room 65x64 reverse", "room K257 T256", "K64", "K65", "K256")

_WANT = {}


def case_reference(name):
    """rollouts() of a scene, computed once and shared (the callers leave it unchanged)"""
    if name not in _WANT:
        i = scene(name)
        c = i["c"]
        _WANT[name] = rollouts(i["state"], i["dist2"], i["cost"] if c["cost_weight"] else None, i["poses"],
                               i["targets"] if c["target_weight"] else None, c)
    return _WANT[name]


def big_scene():
    """120 x 120 free cells inside a wall, T = 256 at |v| = 1024: the clipped window of a pose in the middle is the whole grid, 14400
    cells, more than the library stages; a pose in a corner reaches the same cells from there"""
    W = H = 120
    c = params(width=W, height=H, n_poses=3, n_v=2, n_w=40, v_min=-1024, v_step=2048, w_min=-400, w_step=20, n_steps=256, cost_weight=0,
               turn_weight=1)
    state = np.zeros((H, W), np.int8)
    state[0, :] = state[-1, :] = 100
    state[:, 0] = state[:, -1] = 100
    state[40:80, 60] = 100
    poses = np.array([centre(30, 60, 0), centre(1, 1, 8192), centre(90, 30, 30000)], np.int32)
    return dict(state=state, dist2=clearance(state), cost=None, poses=poses, targets=None, c=c)


I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
MIXED_EDGE_STAGED, MIXED_EDGE_WALKED, MIXED_CORNER, MIXED_CENTRAL = 0, 1, 2, 3            # mixed_scene's hand-placed poses
MIXED_LIVE = 400


def mixed_scene(n_poses=1281):
    """78 x 120 inside a wall with one bar across it, T = 38 at |v| = 1024: R = 39, the clipped bound is 78 x 79 = 6162 cells and a
    workgroup's LDS 28904 B, more than leaves a CU its eight workgroups, so from 1281 workgroups on (K = 16: one per pose) the launch
    stages only the windows of up to 4056 cells and walks the others.  centre(38, 12) has a 78 x 52 = 4056-cell window, centre(38, 13)
    one of 78 x 53 = 4134; then a corner, the middle (the whole width, 79 rows), MIXED_LIVE poses at random in the grid, and the rest
    outside the grid or in the wall: they end at once but count as workgroups.  n_poses = 1280 drops one of those."""
    W, H = 78, 120
    c = params(width=W, height=H, n_poses=n_poses, n_v=2, n_w=8, v_min=-1024, v_step=2048, w_min=-1792, w_step=512, n_steps=38, cost_weight=0,
               turn_weight=1)
    state = np.zeros((H, W), np.int8)
    state[0, :] = state[-1, :] = 100
    state[:, 0] = state[:, -1] = 100
    state[70, 15:60] = 100
    rng = np.random.default_rng(78120)
    poses = [centre(38, 12, 16384), centre(38, 13, 16384), centre(1, 1, 8192), centre(38, 60, 49152)]
    poses += [(int(rng.integers(SUB, (W - 1) * SUB)), int(rng.integers(SUB, (H - 1) * SUB)), int(rng.integers(0, TURN))) for _ in range(MIXED_LIVE)]
    k = 0
    while len(poses) < 1281:
        poses.append(((-3 - k) * SUB, 5 * SUB, k) if k % 2 else centre(k % W, 0, k))           # outside / in the top wall
        k += 1
    return dict(state=state, dist2=clearance(state), cost=None, poses=np.array(poses[:n_poses], np.int32), targets=None, c=c)


def lattice_scene(tie):
    """K = 65536 on the 33 x 31 room, two steps, two poses: open floor, and a wall one cell behind the robot.
    tie False: the score is (v_abs_max - |v|) + |w| with the fastest row and the straightest column last: c = 65535 alone has score 0
    on the open floor; the other pose faces the wall, where the fast rows collide.
    tie True: the score is v_abs_max - |v| with v = -1020 .. 1020: rows 0 and 255 tie wherever both are admissible, so on the open
    floor c = 0 wins a tie of 512 that spans the first and the last chunk; with the wall behind, row 0 collides, and c = 65280 wins
    the tie of the last row, c = 65535 among it."""
    W, H = 33, 31
    kw = dict(n_v=256, n_w=256, v_min=-1020, v_step=8, w_min=-512, w_step=4, turn_weight=0) if tie else \
         dict(n_v=256, n_w=256, v_min=0, v_step=4, w_min=-16320, w_step=64, turn_weight=1)
    c = params(width=W, height=H, n_poses=2, n_steps=2, cost_weight=0, clear_weight=0, speed_weight=1, **kw)
    state = room(W, H, 21)
    poses = np.array([centre(24, 15, 0), centre(1, 15, 0 if tie else 32768)], np.int32)                 # (without the tie it faces the wall)
    return dict(state=state, dist2=clearance(state), cost=None, poses=poses, targets=None, c=c)


EXTREME_POSES = ((I32_MIN, 0, 0), (I32_MAX, I32_MAX, -1), (0, I32_MIN, 65536))


def wide_scene(extremes=True):
    """the widest scores the call allows, on the 33 x 31 room: every weight 1000, clearance_cap 1024 * 1024, a cost field set by hand
    (0xFFFF0000 .. 0xFFFFFFFE, a sixth of the cells unreached), targets at the corners of the int32 square, dist2 0 on a tenth of the
    cells; with extremes, EXTREME_POSES stand among the live poses (at 2, 5 and the end)."""
    W, H = 33, 31
    rng = np.random.default_rng(44)
    state = room(W, H, 22)
    dist2 = clearance(state)
    dist2[rng.random((H, W)) < 0.1] = 0
    cost = rng.integers(0xFFFF0000, 0xFFFFFFFF, (H, W)).astype(np.uint32)
    cost[rng.random((H, W)) < 0.05] = 0xFFFFFFFE
    cost[rng.random((H, W)) < 0.16] = NO_COST
    live = [centre(16, 17, 65535), centre(1, 1, 8192), centre(24, 15, 32768), centre(8, 25, 50000), centre(28, 5, 20000), centre(16, 6, 0),
            centre(3, 3, 0)]
    live += [(int(rng.integers(SUB, (W - 1) * SUB)), int(rng.integers(SUB, (H - 1) * SUB)), int(rng.integers(-TURN, 2 * TURN))) for _ in range(5)]
    poses = live[:2] + [EXTREME_POSES[0]] + live[2:4] + [EXTREME_POSES[1]] + live[4:] + [EXTREME_POSES[2]] if extremes else live
    corners = [(I32_MIN, I32_MAX), (I32_MAX, I32_MIN), (I32_MIN + 1, I32_MAX - 1), (I32_MAX - 3, I32_MIN + 2), (I32_MIN, I32_MIN), (I32_MAX, I32_MAX)]
    targets = np.array([corners[q % len(corners)] for q in range(len(poses))], np.int32)
    c = params(width=W, height=H, n_poses=len(poses), n_v=4, n_w=16, v_min=-256, v_step=256, w_min=-16384, w_step=2048, n_steps=12,
               clearance_cap=1024 * 1024, cost_weight=1000, target_weight=1000, clear_weight=1000, speed_weight=1000, turn_weight=1000)
    return dict(state=state, dist2=dist2, cost=cost, poses=np.array(poses, np.int32), targets=targets, c=c)


def foreign_scene(h, w, allow_unknown):
    """rollouts down the cost field planned on navplan_ref.foreign_grid (states outside {0, -1, 100}, dist2 negative and above the
    cap): the plan's own restatement supplies the field"""
    import navplan_ref as pr
    f = pr.foreign_case(h, w, allow_unknown)
    state, dist2 = f["state"], f["dist2"]
    rng = np.random.default_rng(h + w + allow_unknown)
    trav, _ = traversable(state, dist2, dict(allow_unknown=allow_unknown, min_dist2=0, clearance_cap=20))
    iy, ix = np.nonzero(trav)
    at = rng.choice(len(ix), 10, replace=False)
    poses = [(int(ix[k]) * SUB + int(rng.integers(0, SUB)), int(iy[k]) * SUB + int(rng.integers(0, SUB)), int(rng.integers(0, TURN))) for k in at]
    odd = np.argwhere(~np.isin(state, (0, -1, 100)))
    poses += [centre(int(odd[0][1]), int(odd[0][0])), (w * SUB, 0, 0)]         # on a cell of an odd state: status 2; outside: status 1
    c = params(width=w, height=h, n_poses=len(poses), allow_unknown=allow_unknown, clearance_cap=20, n_steps=16, v_step=96, brake_div=256)
    return dict(state=state, dist2=dist2, cost=f["plan"]["cost"], poses=np.array(poses, np.int32), targets=None, c=c)


def scene_reference(key, make):
    """rollouts() of make(), computed once under `key` and shared (the callers leave it unchanged): (inputs, outputs)"""
    if key not in _WANT:
        i = make()
        c = i["c"]
        _WANT[key] = (i, rollouts(i["state"], i["dist2"], i["cost"] if c["cost_weight"] else None, i["poses"],
                                  i["targets"] if c["target_weight"] else None, c))
    return _WANT[key]
