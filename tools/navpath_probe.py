"""ssf_navpath_waypoints (include/ssf_navpath.h) on 512 x 512 device arrays: the carved grid of the 1 M-row synthetic map of the other
probes (tools/navcarve_probe.py: 64 views along the orbit, stride 8; planned with allow_unknown, as tools/navplan_probe.py does) and
an open grid with scattered pillars, with 16 and 4096 starts each.  The paths are ssf_navplan_field's to the free cell nearest the
grid's centre and stay on the device.

Reports, with warm-ups and --reps repetitions (medians):
  * per kernel (hipEvent brackets of ssf_get_kernel_times under profile = 1) and the wall clock of the whole call (profile off);
  * the share of lane slots of the candidate chunks that held no candidate or were not needed: 1 - segments_tested / (256 x chunks),
    the chunks counted on the host from the waypoints (the chunk of a step's winner, counted from the far end of its window).  This is
    what one wave per path instead of one workgroup could win back on short paths;
  * the host path a caller had before: the device-to-host copy of state, dist2, the paths and their lengths plus
    tests/navpath_ref.py (plain Python: a statement of the rule, not a tuned string-puller -- the figure says what THAT route costs,
    not what a C++ string-puller would), at 16 starts (and at 4096 with --host-all), with the device's outputs compared bit for bit;
  * the wall clock of nav_plan (the carved-map scene of tools/navplan_probe.py) through this library and, with --other-lib, through
    another build of libssf_hip_explore.so (the parent commit's), to show that the plan costs what it cost.
Prints a table and JSON lines; --out also writes them to a file.  No threshold is asserted: the table is the record.

    python tools/navpath_probe.py [--rows 1000000] [--reps 10] [--other-lib PATH] [--host-all] [--out FILE]"""
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
import navpath_ref as wr  # noqa: E402

WARM = 3
KERNELS = ("navpath_pack", "navpath_check", "navpath_pull")
N = 512
MAX_PATH, MAX_WP = 2048, 256
PLAN = dict(allow_unknown=1, goals_from_frontier=1, min_dist2=4, soft_dist2=100, near_penalty=50)       # tools/navplan_probe.py's carved-map scene
RULES = (("defaults", dict()), ("keep_clearance, cap 36, lookahead 4096", dict(keep_clearance=1, clearance_cap=36, lookahead=4096)))


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


def pillar_grid():
    """an open 512 x 512 grid with a 3 x 3 pillar every 37 x 41 cells and the exact squared clearance to them, capped at 400"""
    state = np.zeros((N, N), np.int8)
    for y in range(20, N, 41):
        for x in range(15 + (y % 3) * 9, N, 37):
            state[y:y + 3, x:x + 3] = 100
    oy, ox = np.nonzero(state == 100)
    yy, xx = np.mgrid[0:N, 0:N]
    d2 = np.full((N, N), 400, np.int64)
    for y, x in zip(oy.tolist(), ox.tolist()):
        np.minimum(d2, (yy - y) ** 2 + (xx - x) ** 2, out=d2)
    return state, d2.astype(np.int32)


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


def chunks_of(wp, n_wp, lens, lookahead):
    """the 256-candidate chunks the pull kernel tested, from its waypoints: per step from path index a to J the window holds
    n = min(L - 1 - a, lookahead) candidates; the winner lies in chunk (n - 1 - (J - a - 1)) // 256 from the far end, a forced step
    went through all of them"""
    total = 0
    for i in range(len(lens)):
        idx = wp[i, :n_wp[i], 2]
        for a, word in zip((idx[:-1] & wr.INDEX_MASK).tolist(), idx[1:].tolist()):
            n = min(int(lens[i]) - 1 - a, lookahead)
            J = word & wr.INDEX_MASK
            total += (n + 255) // 256 if word & wr.FORCED else (n - 1 - (J - a - 1)) // 256 + 1
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--other-lib", default=None, help="another build of libssf_hip_explore.so: nav_plan is timed through it as well")
    ap.add_argument("--host-all", action="store_true", help="run the Python reference at 4096 starts as well (minutes)")
    ap.add_argument("--out", default=None, help="also append the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_drive()
    K = synthetic.intrinsics(640, 480)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    f = binding.Fusion(lib, lib.default_config(**cam, nb_supersurfels_max=a.rows + 4096))
    dev = torch.device("cuda")
    state, dist2, gs = carved_grid(f, a.rows, torch, dev)
    say("[map] synthetic %d rows; carved grid 512x512@0.05: %d free, %d occupied, %d unknown" %
        (a.rows, gs["cells_free"], gs["cells_occupied"], gs["cells_unknown"]))
    ps, pd = pillar_grid()
    scenes = [("carved map", state, dist2, dict(allow_unknown=1, min_dist2=4, soft_dist2=100, near_penalty=50)),
              ("open grid with pillars", torch.from_numpy(ps).to(dev), torch.from_numpy(pd).to(dev), dict(min_dist2=4, soft_dist2=100, near_penalty=50))]
    say("512 x 512 cells; max_path %d, max_waypoints %d; %d calls per figure after %d warm-ups; times in ms" % (MAX_PATH, MAX_WP, a.reps, WARM))
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    for name, st8, d2, plan in scenes:
        hs, hd = st8.cpu().numpy(), d2.cpu().numpy()
        ok = (hs == 0) | ((hs == -1) if plan.get("allow_unknown") else False)
        ok &= hd >= plan["min_dist2"]
        fy, fx = np.nonzero(ok)
        near = int(np.argmin((fx - N // 2) ** 2 + (fy - N // 2) ** 2))
        goal = (int(fx[near]), int(fy[near]))
        rng = np.random.default_rng(7)
        for ns in (16, 4096):
            pick = rng.choice(len(fx), ns, replace=False)
            starts = np.stack([fx[pick], fy[pick]], 1).astype(np.int32)
            path, path_len = i32(ns, MAX_PATH, 2), i32(ns)
            pst = f.nav_plan_device(st8, d2, N, N, [goal], starts, path=path, path_len=path_len, start_status=i32(ns), max_path=MAX_PATH, **plan)
            lens = path_len.cpu().numpy()
            say("[%s, %d starts] planned to %s in %d rounds: %d paths of more than one cell, %d cells, longest %d" %
                (name, ns, goal, pst["rounds"], int((lens > 1).sum()), int(lens.sum()), int(lens.max())))
            for rule_name, rule in RULES:
                kw = dict(min_dist2=plan["min_dist2"], allow_unknown=plan.get("allow_unknown", 0), max_waypoints=MAX_WP, **rule)
                o = dict(n_waypoints=i32(ns), status=i32(ns), waypoints=i32(ns, MAX_WP, 4), path_min=i32(ns))
                call = lambda: f.nav_waypoints_device(st8, d2, N, N, path, path_len, ns, MAX_PATH, **dict(o, **kw))
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
                h = {nm: t.cpu().numpy() for nm, t in o.items()}
                chunks = chunks_of(h["waypoints"], h["n_waypoints"], lens, kw.get("lookahead", 256))
                idle = 1.0 - got["segments_tested"] / (256.0 * chunks) if chunks else 0.0
                tag = "%s, %d starts, %s" % (name, ns, rule_name)
                say("[%s] %d ok, %d bad, %d truncated, %d waypoints of %d cells, %d forced; %d walks in %d chunks: %.1f %% of the lane slots idle" %
                    (tag, got["paths_ok"], got["paths_bad"], got["paths_truncated"], got["waypoints"], got["cells_in"], got["forced_steps"],
                     got["segments_tested"], chunks, 100.0 * idle))
                say("[%s] kernels: %s | summed %.4f; wall of the whole call %.3f" %
                    (tag, "  ".join("%s %.4f" % (k[8:], v) for k, v in kern.items()), sum(kern.values()), wall_ms))
                rec = dict(scene=name, starts=ns, rule=rule_name, stats=got, chunks=chunks, idle_share=round(idle, 4),
                           kernel_ms={k: round(v, 4) for k, v in kern.items()}, wall_ms=round(wall_ms, 3))
                if ns == 16 or a.host_all:
                    # the host path: the arrays and the paths to the host, then the reference
                    t0 = time.perf_counter()
                    cs, cd, cp, cl = st8.cpu().numpy(), d2.cpu().numpy(), path.cpu().numpy(), path_len.cpu().numpy()
                    t_copy = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    want = wr.waypoints(cs, cd, cp, cl, **kw)
                    t_ref = time.perf_counter() - t0
                    equal = bool(np.array_equal(h["n_waypoints"], want["n_waypoints"]) and np.array_equal(h["status"], want["status"]) and
                                 np.array_equal(h["path_min"], want["path_min"]) and
                                 all(np.array_equal(h["waypoints"][i, :h["n_waypoints"][i]], want["waypoints"][i]) for i in range(ns)) and
                                 all(got[k] == want["stats"][k] for k in wr.STATS))
                    say("[%s] the host path: copy of state, dist2, paths and lengths %.3f ms + the reference (plain Python) %.1f ms; every output "
                        "equal bit for bit: %s" % (tag, 1e3 * t_copy, 1e3 * t_ref, equal))
                    rec.update(host_copy_ms=round(1e3 * t_copy, 3), host_reference_ms=round(1e3 * t_ref, 1), equal=equal)
                say(json.dumps(rec))
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
        again, _ = plan_wall(g, s2, d2, torch, dev, a.reps)
        say("[nav_plan] the same through %s: wall %.3f ms (%d rounds), and %.3f ms when timed again; the same grid: %s" %
            (os.path.relpath(a.other_lib, ROOT), there, rounds2, again, same))
        rec.update(other_nav_plan_wall_ms=round(there, 3), other_again_ms=round(again, 3), other_rounds=rounds2, same_grid=same)
        g.close()
    say(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
