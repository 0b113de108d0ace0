"""ssf_navplan_field (include/ssf_navplan.h) on three 512 x 512 grids: the carved grid of the 1 M-row synthetic map of the other
probes (tools/navcarve_probe.py: 64 views along the orbit, stride 8; planned with allow_unknown, the frontier and the camera's cell
as goals), an open grid with one goal in a corner, and a serpentine of one-cell corridors (the worst case for rounds: the field
advances about one tile per round along a corridor 131 000 cells long).

Reports, with warm-ups and --reps repetitions (medians):
  * per kernel (hipEvent brackets of ssf_get_kernel_times under profile = 1, at the default round batch), rounds and tile visits;
  * the wall clock of the whole call with device arrays (profile off) for round batches K = 1, 4, 16, 64 (the hook of
    include/ssf_navplan_testing.h): the table the default K is chosen from;
  * the host path a caller had before: the device-to-host copy of state and dist2 plus the reference Dijkstra of
    tests/navplan_ref.py (numpy prep + a Python heapq loop: a statement of the rule, not a tuned planner -- the figure says what THAT
    route costs, not what a C++ Dijkstra would), with the device's field compared bit for bit.
Prints a table and JSON lines; --out also writes them to a file.  No threshold is asserted: the table is the record.

    python tools/navplan_probe.py [--rows 1000000] [--reps 10] [--skip-map] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from supersurfel_fusion_amd import binding, synthetic  # noqa: E402
import navgrid_ref as nr  # noqa: E402
import navplan_ref as pr  # noqa: E402

WARM = 3
KERNELS = ("navplan_init", "navplan_goals", "navplan_relax", "navplan_stats", "navplan_trace")
BATCHES = (1, 4, 16, 64)
N = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-map", action="store_true", help="the two synthetic grids only")
    ap.add_argument("--out", default=None, help="also append the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_nav()
    W, H = 640, 480
    K = synthetic.intrinsics(W, H)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    rows = 4096 if a.skip_map else a.rows
    f = binding.Fusion(lib, lib.default_config(**cam, nb_supersurfels_max=rows + 4096))
    dev = torch.device("cuda")
    scenes = []
    if not a.skip_map:
        model, nvis = synthetic.seed_model_cam0(rows, W, H, stamp=30)
        f.set_model(model, nvis, 30)
        y = model["positions"][:, 1]
        bands = dict(z_min=float(-y.max() - 0.1), z_max=float(-y.min() + 0.1), floor_max=float(-np.median(y)))
        views = np.stack([nr.pose_about(*synthetic.relative_pose(k)) for k in range(64)])
        state, dist2 = torch.zeros((N, N), dtype=torch.int8, device=dev), torch.zeros((N, N), dtype=torch.int32, device=dev)
        gs = f.nav_grid_carve_device(views, state=state, dist2=dist2, carve=dict(stride=8), width=N, height=N, res=0.05, **bands)
        say("[map] synthetic %d rows; carved grid 512x512@0.05: %d free, %d occupied, %d unknown" %
            (rows, gs["cells_free"], gs["cells_occupied"], gs["cells_unknown"]))
        scenes.append(("carved map", state, dist2, [(N // 2, N // 2)], dict(allow_unknown=1, goals_from_frontier=1, min_dist2=4, soft_dist2=100,
                                                                              near_penalty=50)))
    op = pr.open_grid(N, N)
    scenes.append(("open grid", torch.from_numpy(op[0]).to(dev), torch.from_numpy(op[1]).to(dev), [(0, 0)], dict()))
    sp = pr.serpentine(N)
    scenes.append(("serpentine", torch.from_numpy(sp[0]).to(dev), torch.from_numpy(sp[1]).to(dev), [(0, 0)], dict()))
    starts = np.stack([np.linspace(5, N - 6, 16).astype(np.int32), np.linspace(N - 6, 4, 16).astype(np.int32)], axis=1)
    cost = torch.zeros((N, N), dtype=torch.int32, device=dev)
    outs = dict(cost=cost, frontier=torch.zeros((N, N), dtype=torch.uint8, device=dev), start_cost=torch.zeros(16, dtype=torch.int32, device=dev),
                start_status=torch.zeros(16, dtype=torch.int32, device=dev), path_len=torch.zeros(16, dtype=torch.int32, device=dev),
                path=torch.zeros((16, 4096, 2), dtype=torch.int32, device=dev))
    say("512 x 512 cells = 256 tiles; 16 starts, max_path 4096; %d calls per figure after %d warm-ups; times in ms" % (a.reps, WARM))
    for name, state, dist2, goals, kw in scenes:
        call = lambda: f.nav_plan_device(state, dist2, N, N, goals, starts, max_path=4096, **dict(outs, **kw))
        f.set_profile(1)
        per = []
        for k in range(WARM + a.reps):
            f.reset_kernel_times()
            st = call()
            kt = f.kernel_times()
            if k >= WARM:
                per.append([kt.get(nm, (0.0, 0))[0] for nm in KERNELS])
        f.set_profile(0)
        kern = dict(zip(KERNELS, np.median(np.array(per), axis=0).tolist()))
        say("[%s] %d traversable, %d reached, %d frontier goals, max cost %d; rounds %d, tile visits %d (%.1f per round)" %
            (name, st["cells_traversable"], st["cells_reached"], st["frontier_goals"], st["max_cost"], st["rounds"], st["tile_visits"],
             st["tile_visits"] / max(1, st["rounds"])))
        say("[%s] kernels: %s | summed %.4f (relax: %.4f per round)" % (name, "  ".join("%s %.4f" % (k[8:], v) for k, v in kern.items()), sum(kern.values()),
                                                                       kern["navplan_relax"] / max(1, st["rounds"])))
        table = {}
        for batch in BATCHES:
            f.debug_navplan_set_round_batch(batch)
            wall = []
            for k in range(WARM + a.reps):
                t0 = time.perf_counter()
                call()
                if k >= WARM:
                    wall.append(time.perf_counter() - t0)
            table[batch] = 1e3 * float(np.median(wall))
        f.debug_navplan_set_round_batch(0)
        say("[%s] wall of the whole call by round batch: %s" % (name, "  ".join("K=%d %.3f" % kv for kv in table.items())))
        # the host path: both arrays to the host, then the reference
        t0 = time.perf_counter()
        hs, hd = state.cpu().numpy(), dist2.cpu().numpy()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        want = pr.plan(hs, hd, goals, None, **kw)
        t_ref = time.perf_counter() - t0
        equal = bool(np.array_equal(cost.cpu().numpy().view(np.uint32), want["cost"]))
        say("[%s] the host path: copy of state and dist2 %.3f ms + the reference Dijkstra (numpy + Python heapq) %.1f ms; cost equal bit for bit: %s" %
            (name, 1e3 * t_copy, 1e3 * t_ref, equal))
        say(json.dumps(dict(scene=name, stats=st, kernel_ms={k: round(v, 4) for k, v in kern.items()}, wall_ms_by_batch={str(k): round(v, 3) for k, v in table.items()},
                            host_copy_ms=round(1e3 * t_copy, 3), host_reference_ms=round(1e3 * t_ref, 1), cost_equal=equal)))
    f.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
