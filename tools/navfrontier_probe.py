"""ssf_navfrontier_regions (include/ssf_navfrontier.h) on the 512 x 512 carved grid of the 1 M-row synthetic map of the other probes
(tools/navcarve_probe.py: 64 views along the orbit, stride 8) and, because that grid's frontier is short (the orbit carves a small
free patch), on a 512 x 512 grid of random cells (0.4 % obstacles, 6 % unknown: thousands of regions; max_regions 256 there, so that
the reference's Python rays end).  The cost field is ssf_navplan_field's with the free cell nearest the grid's centre as the only goal
(the robot) and allow_unknown, so the regions are ranked as nav_explore ranks them.

Reports, with warm-ups and --reps repetitions (medians), for gain_radius R = 0 and R = 64:
  * per kernel (hipEvent brackets of ssf_get_kernel_times under profile = 1);
  * the wall clock of the whole call with device arrays (profile off);
  * the host path a caller had before: the device-to-host copy of state, dist2 and cost plus tests/navfrontier_ref.py (numpy for the
    members, a Python BFS, Python sets for the gain: a statement of the rule, not a tuned labeller -- the figure says what THAT
    route costs, not what a C++ labeller would), with the device's map, table and order compared bit for bit;
  * the wall clock of nav_plan (the carved-map scene of tools/navplan_probe.py) through this library and, with --other-lib, through
    another build of libssf_hip_nav.so (the parent commit's), to show that the plan costs what it cost.
Prints a table and JSON lines; --out also writes them to a file.  No threshold is asserted: the table is the record.

    python tools/navfrontier_probe.py [--rows 1000000] [--reps 10] [--other-lib PATH] [--out FILE]"""
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
import navfrontier_ref as fr  # noqa: E402
import navgrid_ref as nr  # noqa: E402

WARM = 3
KERNELS = ("navfrontier_label", "navfrontier_merge", "navfrontier_flatten", "navfrontier_sums", "navfrontier_table", "navfrontier_map",
           "navfrontier_gain")
RADII = (0, 64)
N = 512
PLAN = dict(allow_unknown=1, goals_from_frontier=1, min_dist2=4, soft_dist2=100, near_penalty=50)       # tools/navplan_probe.py's carved-map scene


def carved_grid(f, rows, torch, dev):
    W, H = 640, 480
    model, nvis = synthetic.seed_model_cam0(rows, W, H, stamp=30)
    f.set_model(model, nvis, 30)
    y = model["positions"][:, 1]
    bands = dict(z_min=float(-y.max() - 0.1), z_max=float(-y.min() + 0.1), floor_max=float(-np.median(y)))
    views = np.stack([nr.pose_about(*synthetic.relative_pose(k)) for k in range(64)])
    state, dist2 = torch.zeros((N, N), dtype=torch.int8, device=dev), torch.zeros((N, N), dtype=torch.int32, device=dev)
    gs = f.nav_grid_carve_device(views, state=state, dist2=dist2, carve=dict(stride=8), width=N, height=N, res=0.05, **bands)
    return state, dist2, gs


def plan_wall(f, state, dist2, torch, dev, reps):
    """the median wall clock in ms of tools/navplan_probe.py's call on the carved map"""
    starts = np.stack([np.linspace(5, N - 6, 16).astype(np.int32), np.linspace(N - 6, 4, 16).astype(np.int32)], axis=1)
    outs = dict(cost=torch.zeros((N, N), dtype=torch.int32, device=dev), frontier=torch.zeros((N, N), dtype=torch.uint8, device=dev),
                start_cost=torch.zeros(16, dtype=torch.int32, device=dev), start_status=torch.zeros(16, dtype=torch.int32, device=dev),
                path_len=torch.zeros(16, dtype=torch.int32, device=dev), path=torch.zeros((16, 4096, 2), dtype=torch.int32, device=dev))
    wall = []
    for k in range(WARM + reps):
        t0 = time.perf_counter()
        st = f.nav_plan_device(state, dist2, N, N, [(N // 2, N // 2)], starts, max_path=4096, **dict(outs, **PLAN))
        if k >= WARM:
            wall.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(wall)), st["rounds"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--other-lib", default=None, help="another build of libssf_hip_nav.so: nav_plan is timed through it as well")
    ap.add_argument("--out", default=None, help="also append the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_explore()
    K = synthetic.intrinsics(640, 480)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    f = binding.Fusion(lib, lib.default_config(**cam, nb_supersurfels_max=a.rows + 4096))
    dev = torch.device("cuda")
    state, dist2, gs = carved_grid(f, a.rows, torch, dev)
    say("[map] synthetic %d rows; carved grid 512x512@0.05: %d free, %d occupied, %d unknown" %
        (a.rows, gs["cells_free"], gs["cells_occupied"], gs["cells_unknown"]))
    rs, rd = fr.random_grid(N, N, 21, obstacles=0.004, unknown=0.06)
    scenes = [("carved map", state, dist2, 4096), ("random cells", torch.from_numpy(rs).to(dev), torch.from_numpy(rd).to(dev), 256)]
    cost, region = torch.zeros((N, N), dtype=torch.int32, device=dev), torch.zeros((N, N), dtype=torch.int32, device=dev)
    say("512 x 512 cells = 256 tiles; min_cells 3, reachable_only; %d calls per figure after %d warm-ups; times in ms" % (a.reps, WARM))
    for name, st8, d2, max_regions in scenes:
        fy, fx = np.nonzero(st8.cpu().numpy() == 0)
        near = int(np.argmin((fx - N // 2) ** 2 + (fy - N // 2) ** 2))
        robot = (int(fx[near]), int(fy[near]))
        ps = f.nav_plan_device(st8, d2, N, N, [robot], cost=cost, allow_unknown=1)
        say("[%s] the field from the free cell nearest the centre, %s, allow_unknown: %d traversable, %d reached, %d rounds; max_regions %d" %
            (name, robot, ps["cells_traversable"], ps["cells_reached"], ps["rounds"], max_regions))
        for R in RADII:
            kw = dict(min_cells=3, reachable_only=1, gain_radius=R, gain_weight=1 if R else 0, max_regions=max_regions)
            call = lambda: f.nav_frontiers_device(st8, N, N, d2, cost, region, **kw)
            f.set_profile(1)
            per = []
            for k in range(WARM + a.reps):
                f.reset_kernel_times()
                got = call()
                kt = f.kernel_times()
                if k >= WARM:
                    per.append([kt.get(nm, (0.0, 0))[0] for nm in KERNELS])
            f.set_profile(0)
            kern = dict(zip(KERNELS, np.median(np.array(per), axis=0).tolist()))
            wall = []
            for k in range(WARM + a.reps):
                t0 = time.perf_counter()
                got = call()
                if k >= WARM:
                    wall.append(time.perf_counter() - t0)
            wall_ms = 1e3 * float(np.median(wall))
            st = got["stats"]
            tag = "%s, R = %d" % (name, R)
            say("[%s] %d frontier cells, %d regions found, %d small, %d unreached, %d kept, %d written, largest %d cells, %d rays, %d merge pairs" %
                (tag, st["frontier_cells"], st["regions_found"], st["regions_small"], st["regions_unreached"], st["regions_kept"], st["regions_written"],
                 st["largest_cells"], st["gain_rays"], st["merge_pairs"]))
            say("[%s] kernels: %s | summed %.4f; wall of the whole call %.3f" %
                (tag, "  ".join("%s %.4f" % (k[12:], v) for k, v in kern.items()), sum(kern.values()), wall_ms))
            # the host path: the three arrays to the host, then the reference
            t0 = time.perf_counter()
            hs, hd, hc = st8.cpu().numpy(), d2.cpu().numpy(), cost.cpu().numpy().view(np.uint32)
            t_copy = time.perf_counter() - t0
            t0 = time.perf_counter()
            want = fr.frontiers(hs, hd, hc, **kw)
            t_ref = time.perf_counter() - t0
            equal = bool(np.array_equal(region.cpu().numpy(), want["region"]) and np.array_equal(got["order"], want["order"]) and
                         got["regions"].tobytes() == fr.as_records(want["regions"], binding.NAVFRONTIER_REGION_DTYPE).tobytes())
            say("[%s] the host path: copy of state, dist2 and cost %.3f ms + the reference (numpy + Python BFS and sets) %.1f ms; map, table and "
                "order equal bit for bit: %s" % (tag, 1e3 * t_copy, 1e3 * t_ref, equal))
            say(json.dumps(dict(scene=name, gain_radius=R, stats=st, kernel_ms={k: round(v, 4) for k, v in kern.items()}, wall_ms=round(wall_ms, 3),
                                host_copy_ms=round(1e3 * t_copy, 3), host_reference_ms=round(1e3 * t_ref, 1), equal=equal)))
    hs, hd = state.cpu().numpy(), dist2.cpu().numpy()
    here, rounds = plan_wall(f, state, dist2, torch, dev, a.reps)
    say("[nav_plan] the carved-map scene of tools/navplan_probe.py through this library: wall %.3f ms (%d rounds)" % (here, rounds))
    rec = dict(nav_plan_wall_ms=round(here, 3), rounds=rounds)
    f.close()
    if a.other_lib:
        other = binding.Library(a.other_lib)
        g = binding.Fusion(other, other.default_config(**cam, nb_supersurfels_max=a.rows + 4096))
        s2, d2, _ = carved_grid(g, a.rows, torch, dev)
        same = bool(np.array_equal(s2.cpu().numpy(), hs) and np.array_equal(d2.cpu().numpy(), hd))
        there, rounds2 = plan_wall(g, s2, d2, torch, dev, a.reps)
        say("[nav_plan] the same through %s: wall %.3f ms (%d rounds); the same grid: %s" % (os.path.relpath(a.other_lib, ROOT), there, rounds2, same))
        rec.update(other_nav_plan_wall_ms=round(there, 3), other_rounds=rounds2, same_grid=same)
        g.close()
    say(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
