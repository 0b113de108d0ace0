"""ssf_navpose_field (include/ssf_navpose.h) at the size a robot has: 512 x 512 cells, device arrays in and out, a 12 x 8-cell body with
nav_foot_pad's pad (at 8 bins the helper asks for 4348 sub-units, above the call's 4096: 4096 there), at 8, 16 and 32 heading bins, on
  * the carved grid of the 1 M-row synthetic map of the other probes (tools/navplan_probe.py: 64 views along the orbit, stride 8;
    unknown cells count as clear), the goal the camera's cell at any heading;
  * tools/navsteer_probe.py's hall: an open floor with hashed pillars and a few unknown patches;
and, as the known worst case for rounds, the serpentine of one-cell corridors with the point footprint at one bin.

Reports, after 5 warm-ups, medians of --reps calls with the smallest and largest as the spread:
  * the whole call (a host clock around the synchronous call, profile off) and its kernels (hipEvent brackets of
    ssf_get_kernel_times under profile = 1), with rounds and tile visits;
  * the disc's nav_plan on the same grid and goal, through the same library;
  * the host route a caller had before, at --host-bins bins only (the restatement is a Python heapq loop over up to 8 M states): mask
    and dist2 copied out plus tests/navpose_ref.py, a statement of the rule and not a tuned planner; the device's field is compared
    with it with ==;
  * with --other-lib (the parent commit's libssf_hip_foot.so), nav_plan, nav_foot and nav_foot_steer on the hall through this
    library, the other, and this one again, in one process: they cost what they cost.
Prints a table and JSON lines; --out also writes them to a file.  No threshold is asserted: the table is the record.

    python tools/navpose_probe.py [--rows 1000000] [--reps 20] [--host-bins 8] [--skip-map] [--other-lib PATH] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from supersurfel_fusion_amd import binding, synthetic  # noqa: E402
import navgrid_ref as nr  # noqa: E402
import navplan_ref as pr  # noqa: E402
import navpose_ref as qr  # noqa: E402
import navsteer_probe as sp  # noqa: E402

WARM, N = 5, sp.N
KERNELS = ("navpose_init", "navpose_goals", "navpose_relax", "navpose_stats", "navpose_trace")
BODY = dict(front=6144, back=6144, left=4096, right=4096)                # 12 x 8 cells
BINS = (8, 16, 32)


def timed(f, call, kernels, reps):
    """(wall ms list, per-kernel ms array, the last result)"""
    f.set_profile(1)
    per = []
    for k in range(WARM + reps):
        f.reset_kernel_times()
        got = call()
        kt = f.kernel_times()
        if k >= WARM:
            per.append([kt.get(nm, (0.0, 0))[0] for nm in kernels])
    f.set_profile(0)
    wall = []
    for k in range(WARM + reps):
        t0 = time.perf_counter()
        got = call()
        if k >= WARM:
            wall.append(1e3 * (time.perf_counter() - t0))
    return wall, np.array(per), got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-bins", type=int, default=8, help="the bin count at which the host route is timed and compared (0: skip it)")
    ap.add_argument("--skip-map", action="store_true", help="the hall and the serpentine only")
    ap.add_argument("--other-lib", default=None, help="another build of libssf_hip_foot.so: nav_plan, nav_foot and nav_foot_steer are timed through it as well")
    ap.add_argument("--out", default=None, help="also append the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_pose()
    K = synthetic.intrinsics(sp.W, sp.H)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    rows = 4096 if a.skip_map else a.rows
    f = binding.Fusion(lib, lib.default_config(**cam, nb_supersurfels_max=rows + 4096))
    dev = torch.device("cuda")
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    scenes = []
    if not a.skip_map:
        model, nvis = synthetic.seed_model_cam0(rows, sp.W, sp.H, stamp=30)
        f.set_model(model, nvis, 30)
        y = model["positions"][:, 1]
        bands = dict(z_min=float(-y.max() - 0.1), z_max=float(-y.min() + 0.1), floor_max=float(-np.median(y)))
        views = np.stack([nr.pose_about(*synthetic.relative_pose(k)) for k in range(64)])
        state, dist2 = torch.zeros((N, N), dtype=torch.int8, device=dev), i32(N, N)
        gs = f.nav_grid_carve_device(views, state=state, dist2=dist2, carve=dict(stride=8), width=N, height=N, res=0.05, **bands)
        say("[carved map] synthetic %d rows; carved grid 512x512@0.05: %d free, %d occupied, %d unknown" %
            (rows, gs["cells_free"], gs["cells_occupied"], gs["cells_unknown"]))
        scenes.append(("carved map", state, dist2, (N // 2, N // 2), 1))
    state, dist2 = sp.grid_on_device(f, torch, dev)
    scenes.append(("hall with pillars", state, dist2, sp.GOAL, 0))
    say("512 x 512 cells = 1024 tiles of 16 x 16; a 12 x 8-cell body; 16 starts, max_path 4096; %d calls per figure after %d warm-ups; times in ms: "
        "median (smallest .. largest)" % (a.reps, WARM))
    rng = np.random.default_rng(5)
    starts = np.stack([rng.integers(0, N * 1024, 16), rng.integers(0, N * 1024, 16), rng.integers(0, 65536, 16)], axis=1).astype(np.int32)
    mask, cell_cost, cell_bin = i32(N, N), i32(N, N), torch.zeros((N, N), dtype=torch.uint8, device=dev)
    outs = dict(cell_cost=cell_cost, cell_bin=cell_bin, start_cost=i32(16), start_status=i32(16), path_len=i32(16), path=i32(16, 4096, 3))
    for name, state, dist2, goal, allow in scenes:
        # the goal of all four plans: the cell nearest the scene's nominal goal at which the body fits at every one of 8 bins under the widest pad
        f.nav_foot_device(state, N, N, free_mask=mask, n_headings=8, allow_unknown=allow, pad=binding.NAVFOOT_MAX_PAD, **BODY)
        fits = np.argwhere(mask.cpu().numpy() == 0xFF)
        gy, gx = fits[np.argmin((fits[:, 0] - goal[1]) ** 2 + (fits[:, 1] - goal[0]) ** 2)]
        goal, pgoal = (int(gx), int(gy)), (int(gx), int(gy), -1)
        disc_cost = i32(N, N)
        wall = []
        for k in range(WARM + a.reps):
            t0 = time.perf_counter()
            ds = f.nav_plan_device(state, dist2, N, N, [goal], None, cost=disc_cost, allow_unknown=allow)
            if k >= WARM:
                wall.append(1e3 * (time.perf_counter() - t0))
        say("[%s] the disc's nav_plan (min_dist2 0): wall %s | %d cells reached in %d rounds, %d tile visits" %
            (name, sp.spread(wall), ds["cells_reached"], ds["rounds"], ds["tile_visits"]))
        say(json.dumps(dict(scene=name, disc_wall_ms=[round(float(x), 4) for x in (np.median(wall), np.min(wall), np.max(wall))], disc_stats=ds)))
        for B in BINS:
            pad = min(binding.Fusion.nav_foot_pad(n_headings=B, **BODY), binding.NAVFOOT_MAX_PAD)      # (8 bins ask for 4348: the call's largest pad there)
            fs = f.nav_foot_device(state, N, N, free_mask=mask, n_headings=B, allow_unknown=allow, pad=pad, **BODY)
            field = i32(B, N, N)
            call = lambda: f.nav_pose_plan_device(mask, dist2, N, N, [pgoal], starts, cost=field, n_headings=B, max_path=4096, **outs)
            wall, per, st = timed(f, call, KERNELS, a.reps)
            kern = np.median(per, axis=0)
            say("[%s, %d bins, pad %d] goal cell (%d, %d); %d cells hold the body at some bin; %d traversable states, %d reached in %d cells, max cost %d; rounds %d, "
                "tile visits %d (%.1f per round)" % (name, B, pad, pgoal[0], pgoal[1], fs["cells_all"] + fs["cells_some"], st["states_traversable"], st["states_reached"],
                                                     st["cells_reached"], st["max_cost"], st["rounds"], st["tile_visits"], st["tile_visits"] / max(1, st["rounds"])))
            say("[%s, %d bins] wall %s | kernels: %s | summed %.4f (relax: %.4f per round)" %
                (name, B, sp.spread(wall), "  ".join("%s %.4f" % (k[8:], v) for k, v in zip(KERNELS, kern)), float(kern.sum()),
                 float(kern[2]) / max(1, st["rounds"])))
            rec = dict(scene=name, bins=B, pad=pad, goal=pgoal[:2], stats=st, wall_ms=[round(float(x), 4) for x in (np.median(wall), np.min(wall), np.max(wall))],
                       kernel_ms={k: round(float(v), 4) for k, v in zip(KERNELS, kern)})
            if B == a.host_bins:
                t0 = time.perf_counter()
                hm, hd = mask.cpu().numpy().view(np.uint32), dist2.cpu().numpy()
                t_out = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                want = qr.plan(hm, hd, [pgoal], starts, n_headings=B, max_path=4096)
                t_ref = 1e3 * (time.perf_counter() - t0)
                equal = bool(np.array_equal(field.cpu().numpy().view(np.uint32), want["cost"]) and
                             np.array_equal(cell_cost.cpu().numpy().view(np.uint32), want["cell_cost"]) and np.array_equal(cell_bin.cpu().numpy(), want["cell_bin"]) and
                             np.array_equal(outs["start_status"].cpu().numpy(), want["start_status"]) and all(st[k] == want["stats"][k] for k in qr.STATS))
                say("[%s, %d bins] the host route: mask and dist2 out %.3f ms + the restatement (numpy + Python heapq) %.0f ms; field, projection, "
                    "statuses and stats equal with ==: %s" % (name, B, t_out, t_ref, equal))
                rec.update(host_out_ms=round(t_out, 3), host_reference_ms=round(t_ref, 1), equal=equal)
            say(json.dumps(rec))

    # ---- the worst case for rounds -----------------------------------------------------------------------------------------------
    s_state, s_dist2 = pr.serpentine(N)
    s_mask = torch.from_numpy(qr.point_mask(s_state, 0, 1).view(np.int32)).to(dev)
    d_dist2 = torch.from_numpy(s_dist2).to(dev)
    field = i32(1, N, N)
    kw = dict(n_headings=1, move_tol=256, reverse_cost=0)
    wall, per, st = timed(f, lambda: f.nav_pose_plan_device(s_mask, d_dist2, N, N, [(0, 0, -1)], None, cost=field, **kw), KERNELS, a.reps)
    kern = np.median(per, axis=0)
    say("[serpentine, 1 bin, point] %d states reached, max cost %d; rounds %d, tile visits %d | wall %s | relax %.4f (%.4f per round)" %
        (st["states_reached"], st["max_cost"], st["rounds"], st["tile_visits"], sp.spread(wall), float(kern[2]), float(kern[2]) / max(1, st["rounds"])))
    d_state = torch.from_numpy(s_state).to(dev)
    disc_cost = i32(N, N)
    dwall = []
    for k in range(WARM + a.reps):
        t0 = time.perf_counter()
        ds = f.nav_plan_device(d_state, d_dist2, N, N, [(0, 0)], None, cost=disc_cost)
        if k >= WARM:
            dwall.append(1e3 * (time.perf_counter() - t0))
    equal = bool(np.array_equal(field.cpu().numpy()[0], disc_cost.cpu().numpy()))
    say("[serpentine] the disc's nav_plan: wall %s, rounds %d, tile visits %d; the two fields are equal: %s" % (sp.spread(dwall), ds["rounds"], ds["tile_visits"], equal))
    say(json.dumps(dict(scene="serpentine", stats=st, wall_ms=[round(float(x), 4) for x in (np.median(wall), np.min(wall), np.max(wall))],
                        kernel_ms={k: round(float(v), 4) for k, v in zip(KERNELS, kern)},
                        disc_wall_ms=[round(float(x), 4) for x in (np.median(dwall), np.min(dwall), np.max(dwall))], disc_rounds=ds["rounds"], equal=equal)))
    f.close()

    # ---- the older calls against another build ---------------------------------------------------------------------------------------
    def older(g, tag):
        s2, d2 = sp.grid_on_device(g, torch, dev)
        pw, r2, c2 = sp.plan_wall(g, s2, d2, torch, dev, a.reps)
        m2 = i32(N, N)
        pad = binding.Fusion.nav_foot_pad(n_headings=32, **BODY)
        fw, _, fs = timed(g, lambda: g.nav_foot_device(s2, N, N, free_mask=m2, n_headings=32, pad=pad, **BODY), ("navfoot_layers",), a.reps)
        hm, hd = m2.cpu().numpy().view(np.uint32), d2.cpu().numpy()
        fits = np.argwhere((hm != 0) & (hd >= sp.PLAN["min_dist2"]))
        pick = fits[np.random.default_rng(3).permutation(len(fits))[:16]]
        bits = hm[pick[:, 0], pick[:, 1]]
        poses = np.stack([pick[:, 1] * 1024 + 512, pick[:, 0] * 1024 + 512, np.array([int(b & -b).bit_length() - 1 for b in bits.tolist()]) * 2048], axis=1).astype(np.int32)
        d_poses = torch.from_numpy(poses).to(dev)
        o = dict(best=i32(16), best_cmd=i32(16, 2), best_score=torch.zeros(16, dtype=torch.int64, device=dev), n_admissible=i32(16), pose_status=i32(16),
                 best_len=i32(16), best_traj=i32(16, 33, 3))
        sw, _, ss = timed(g, lambda: g.nav_foot_steer_device(m2, d2, N, N, d_poses, 16, 32, cost=c2, min_dist2=sp.PLAN["min_dist2"], **o),
                          ("navfoot_roll",), a.reps)
        say("[%s] nav_plan wall %s (%d rounds) | nav_foot (32 bins) wall %s | nav_foot_steer (16 poses) wall %s" % (tag, sp.spread(pw), r2, sp.spread(fw), sp.spread(sw)))
        return dict(plan_ms=[round(float(x), 4) for x in (np.median(pw), np.min(pw), np.max(pw))], foot_ms=[round(float(x), 4) for x in (np.median(fw), np.min(fw), np.max(fw))],
                    steer_ms=[round(float(x), 4) for x in (np.median(sw), np.min(sw), np.max(sw))], cost_sum=int(c2.to(torch.int64).sum().item()),
                    mask_sum=int(m2.to(torch.int64).sum().item()), best_sum=int(o["best"].sum().item()), score_sum=int(o["best_score"].sum().item()))

    if a.other_lib:
        rec = {}
        for tag, path in (("this library", None), ("the other library", a.other_lib), ("this library again", None)):
            L = lib if path is None else binding.Library(path)
            g = binding.Fusion(L, L.default_config(**cam))
            rec[tag] = older(g, tag)
            g.close()
        same = all(rec["this library"][k] == rec["the other library"][k] for k in ("cost_sum", "mask_sum", "best_sum", "score_sum"))
        say("[other] %s; the field, the mask, the winners and their scores are the same through both: %s" % (os.path.relpath(a.other_lib, ROOT), same))
        rec["same_results"] = bool(same)
        say(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
