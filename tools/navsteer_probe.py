"""ssf_navsteer_rollouts (include/ssf_navsteer.h) at the size a robot has: a 512 x 512 grid (a walled hall with pillars drawn from a
hash, its clearance from ssf_navlive_overlay's identity on an empty frame, its cost-to-goal field from ssf_navplan_field), device
arrays in and out, per-pose outputs only (the command, its score and status, the winner's arc).

Reports, with warm-ups and --reps repetitions (medians, and the smallest and largest of the repetitions as the spread):
  * the whole call (a host clock around the synchronous call, profile off) and each kernel (hipEvent brackets of ssf_get_kernel_times
    under profile = 1) at 1, 16 and 4096 poses, with the default lattice (9 x 33 candidates, 32 steps) and with 64 x 64 candidates
    over 64 steps (a window of 131 x 131 cells, more than is ever staged), and with 16 x 16 slow candidates over 256 steps (a window
    of 101 x 101 cells, staged while the launch is resident at once);
  * the same inputs with walk = 1: every rollout reads the packed grid in global memory instead of the window staged in LDS (where
    the library's own choice is the global walk the two rows are the same measurement twice);
  * the host route a caller had before, as a statement of the rule and not a tuned implementation: state, dist2 and cost copied out,
    tests/navsteer_ref.py (numpy over the candidates, Python loops over poses and steps); the device's outputs are compared with it
    with == (at 4096 poses only on the default lattice);
  * nav_plan on the same grid through this library and, with --other-lib, through another build of libssf_hip_live.so (the parent
    commit's), to show that the plan costs what it cost.
Prints a table and JSON lines; --out also writes them to a file.  No threshold is asserted: the table is the record.

    python tools/navsteer_probe.py [--reps 20] [--other-lib PATH] [--out FILE]"""
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
import navsteer_ref as sr  # noqa: E402

WARM = 5
KERNELS = ("navsteer_pack", "navsteer_roll", "navsteer_pick")
N = 512
W, H = 160, 128
GOAL = (N - 40, N // 2)
PLAN = dict(min_dist2=4, soft_dist2=36, near_penalty=20)
LATTICES = (("default 9 x 33, T = 32", dict()),
            ("64 x 64, T = 64", dict(n_v=64, n_w=64, v_min=0, v_step=16, w_min=-2016, w_step=64, n_steps=64)),
            ("16 x 16, T = 256, |v| <= 195", dict(n_v=16, n_w=16, v_min=0, v_step=13, w_min=-480, w_step=64, n_steps=256)))
POSES = (1, 16, 4096)


def hall():
    """512 x 512: a wall all round, pillars of 6 x 6 cells on a hashed third of a 32-cell lattice, a few unknown patches"""
    s = np.zeros((N, N), np.int8)
    s[0, :] = s[-1, :] = 100
    s[:, 0] = s[:, -1] = 100
    for j in range(1, N // 32):
        for i in range(1, N // 32):
            h = ((j * 16 + i) * 2654435761 & 0xFFFFFFFF) >> 16
            if h % 3 == 0:
                y, x = 32 * j + h % 11, 32 * i + (h >> 4) % 11
                s[y:y + 6, x:x + 6] = 100
            elif h % 17 == 0:
                s[32 * j:32 * j + 9, 32 * i:32 * i + 9] = -1
    return s


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def plan_wall(f, state, dist2, torch, dev, reps):
    cost = torch.zeros((N, N), dtype=torch.int32, device=dev)
    wall = []
    for k in range(WARM + reps):
        t0 = time.perf_counter()
        st = f.nav_plan_device(state, dist2, N, N, [GOAL], None, cost=cost, **PLAN)
        if k >= WARM:
            wall.append(1e3 * (time.perf_counter() - t0))
    return wall, st["rounds"], cost


def grid_on_device(f, torch, dev):
    """(state, dist2): the hall, and its clearance as ssf_navlive_overlay's identity gives it (no valid pixel: dist2 of state_in)"""
    state = torch.from_numpy(hall()).to(dev)
    dist2 = torch.zeros((N, N), dtype=torch.int32, device=dev)
    f.nav_live_device(torch.zeros((H, W), dtype=torch.float32, device=dev), state, N, N, dist2=dist2, open_unknown=0)
    return state, dist2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--other-lib", default=None, help="another build of libssf_hip_live.so: nav_plan is timed through it as well")
    ap.add_argument("--out", default=None, help="also append the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_steer()
    K = synthetic.intrinsics(W, H)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    f = binding.Fusion(lib, lib.default_config(**cam))
    dev = torch.device("cuda")
    state, dist2 = grid_on_device(f, torch, dev)
    here, rounds, cost = plan_wall(f, state, dist2, torch, dev, a.reps)
    h_state, h_dist2, h_cost = state.cpu().numpy(), dist2.cpu().numpy(), cost.cpu().numpy().view(np.uint32)
    say("[grid] %d x %d: %d free, %d occupied, %d unknown cells; the field reaches %d cells from %s in %d rounds" %
        (N, N, int((h_state == 0).sum()), int((h_state == 100).sum()), int((h_state == -1).sum()), int((h_cost != sr.NO_COST).sum()), GOAL, rounds))
    say("%d calls per figure after %d warm-ups; times in ms: median (smallest .. largest)" % (a.reps, WARM))
    rng = np.random.default_rng(3)
    free = np.argwhere((h_state == 0) & (h_dist2 >= PLAN["min_dist2"]))
    pick = free[rng.permutation(len(free))[:max(POSES)]]
    all_poses = np.stack([pick[:, 1] * 1024 + rng.integers(0, 1024, len(pick)), pick[:, 0] * 1024 + rng.integers(0, 1024, len(pick)),
                          rng.integers(0, 65536, len(pick))], axis=1).astype(np.int32)
    for lname, lat in LATTICES:
        c0 = sr.params(width=N, height=N, min_dist2=PLAN["min_dist2"], **lat)
        T, Kc = c0["n_steps"], c0["n_v"] * c0["n_w"]
        for n in POSES:
            poses = np.ascontiguousarray(all_poses[:n])
            d_poses = torch.from_numpy(poses).to(dev)
            i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
            o = dict(best=i32(n), best_cmd=i32(n, 2), best_score=torch.zeros(n, dtype=torch.int64, device=dev), n_admissible=i32(n), pose_status=i32(n),
                     best_len=i32(n), best_traj=i32(n, T + 1, 3))
            rec = dict(lattice=lname, candidates=Kc, n_steps=T, n_poses=n)
            for walk in (0, 1):
                call = lambda: f.nav_steer_device(state, dist2, N, N, d_poses, n, cost=cost, min_dist2=PLAN["min_dist2"], walk=walk, **dict(o, **lat))
                f.set_profile(1)
                per = []
                for k in range(WARM + a.reps):
                    f.reset_kernel_times()
                    got = call()
                    kt = f.kernel_times()
                    if k >= WARM:
                        per.append([kt.get(nm, (0.0, 0))[0] for nm in KERNELS])
                f.set_profile(0)
                per = np.array(per)
                wall = []
                for k in range(WARM + a.reps):
                    t0 = time.perf_counter()
                    got = call()
                    if k >= WARM:
                        wall.append(1e3 * (time.perf_counter() - t0))
                tag = "[%s, %d poses, %s]" % (lname, n, "walk 1: the grid in global memory" if walk else "walk 0: the window in LDS")
                say("%s wall %s | %s | summed %.4f | windows staged %d, global %d" %
                    (tag, spread(wall), "  ".join("%s %s" % (k, spread(per[:, i])) for i, k in enumerate(KERNELS)), float(np.median(per, axis=0).sum()),
                     got["windows_staged"], got["windows_global"]))
                rec["walk%d" % walk] = dict(wall_ms=[round(float(x), 4) for x in (np.median(wall), np.min(wall), np.max(wall))],
                                            kernel_ms={k: round(float(np.median(per[:, i])), 4) for i, k in enumerate(KERNELS)},
                                            windows_staged=got["windows_staged"], windows_global=got["windows_global"])
                if walk == 0:
                    first = {nm: t.cpu().numpy() for nm, t in o.items()}
                    rec["stats"] = {k: got[k] for k in sr.STATS}
                else:
                    rec["walks_equal"] = bool(all(np.array_equal(first[nm], t.cpu().numpy()) for nm, t in o.items() if nm != "best_traj"))
            say("[%s, %d poses] %s; the two walks give the same bytes: %s" % (lname, n, " ".join("%s=%d" % kv for kv in rec["stats"].items()), rec["walks_equal"]))
            if n < max(POSES) or not lat:
                # the host route: the three arrays out, the restatement
                t0 = time.perf_counter()
                hs, hd, hc = state.cpu().numpy(), dist2.cpu().numpy(), cost.cpu().numpy().view(np.uint32)
                t_out = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                want = sr.rollouts(hs, hd, hc, poses, None, dict(c0, n_poses=n))
                t_ref = 1e3 * (time.perf_counter() - t0)
                equal = all(np.array_equal(first[nm].astype(sr.DTYPES[nm]), want[nm]) for nm in o if nm != "best_traj")
                equal = bool(equal and all(np.array_equal(first["best_traj"][q, :want["best_len"][q]], want["best_traj"][q, :want["best_len"][q]]) for q in range(n))
                             and all(rec["stats"][k] == want["stats"][k] for k in sr.STATS))
                say("[%s, %d poses] the host route: copies out %.3f ms + the restatement (numpy) %.0f ms; every output equal with ==: %s" %
                    (lname, n, t_out, t_ref, equal))
                rec.update(host_out_ms=round(t_out, 3), host_reference_ms=round(t_ref, 1), equal=equal)
            say(json.dumps(rec))
    here2, _, _ = plan_wall(f, state, dist2, torch, dev, a.reps)
    say("[nav_plan] this grid through this library: wall %s ms (%d rounds), and %s when timed again" % (spread(here), rounds, spread(here2)))
    rec = dict(nav_plan_wall_ms=round(float(np.median(here)), 3), again_ms=round(float(np.median(here2)), 3), rounds=rounds)
    f.close()
    if a.other_lib:
        other = binding.Library(a.other_lib)
        g = binding.Fusion(other, other.default_config(**cam))
        s2, d2 = grid_on_device(g, torch, dev)
        there, rounds2, cost2 = plan_wall(g, s2, d2, torch, dev, a.reps)
        again, _, _ = plan_wall(g, s2, d2, torch, dev, a.reps)
        same = bool(np.array_equal(d2.cpu().numpy(), h_dist2) and np.array_equal(cost2.cpu().numpy().view(np.uint32), h_cost))
        say("[nav_plan] the same through %s: wall %s ms (%d rounds), and %s when timed again; the same grid and field: %s" %
            (os.path.relpath(a.other_lib, ROOT), spread(there), rounds2, spread(again), same))
        rec.update(other_nav_plan_wall_ms=round(float(np.median(there)), 3), other_again_ms=round(float(np.median(again)), 3), other_rounds=rounds2, same_field=same)
        g.close()
        f2 = binding.Fusion(lib, lib.default_config(**cam))
        s3, d3 = grid_on_device(f2, torch, dev)
        third, _, _ = plan_wall(f2, s3, d3, torch, dev, a.reps)
        say("[nav_plan] through this library again, after the other: wall %s ms" % spread(third))
        rec.update(nav_plan_third_ms=round(float(np.median(third)), 3))
        f2.close()
    say(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
