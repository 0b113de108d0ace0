"""ssf_navfoot_layers and ssf_navfoot_rollouts (include/ssf_navfoot.h) at the size a robot has: tools/navsteer_probe.py's 512 x 512 hall
(walls, hashed pillars, unknown patches; clearance from ssf_navlive_overlay's identity, cost-to-goal field from ssf_navplan_field),
device arrays in and out, per-pose outputs only.

Reports, after 5 warm-ups, medians of --reps calls with the smallest and largest as the spread:
  * the layers alone: a 12 x 8-cell body with nav_foot_pad's pad at 32 headings, and the largest body the call takes (28 cells to
    every side with the pad, reach 39) at 32 headings: the whole call (a host clock around the synchronous call, profile off) and
    the kernel (hipEvent brackets of ssf_get_kernel_times under profile = 1);
  * the rollouts over the 12 x 8 body's mask at 1, 16 and 4096 poses on the default lattice (9 x 33 candidates, 32 steps), per kernel,
    beside nav_steer on the same grid, field and poses through the same library;
  * the host route a caller had before, as a statement of the rule and not a tuned implementation: state copied out and
    tests/navfoot_ref.py's dilation (numpy), then mask, dist2 and cost copied out and its rollouts (at 1 and 16 poses); the device's
    outputs are compared with it with ==;
  * with --other-lib (the parent commit's libssf_hip_steer.so), nav_steer and nav_plan on the same inputs through this library, the
    other, and this one again, in one process: the disc's rollouts and the plan cost what they cost.
Prints a table and JSON lines; --out also writes them to a file.  No threshold is asserted: the table is the record.

    python tools/navfoot_probe.py [--reps 20] [--other-lib PATH] [--out FILE]"""
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
import navfoot_ref as fr  # noqa: E402
import navsteer_ref as sr  # noqa: E402
import navsteer_probe as sp  # noqa: E402

WARM, N, PLAN, POSES = sp.WARM, sp.N, sp.PLAN, sp.POSES
FOOT_KERNELS = ("navfoot_pack", "navfoot_roll", "navfoot_pick")
BODY = dict(front=6144, back=6144, left=4096, right=4096)                # 12 x 8 cells
BINS = 32
LARGEST = dict(front=24576, back=24576, left=24576, right=24576, pad=4096)


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--other-lib", default=None, help="another build of libssf_hip_steer.so: nav_steer and nav_plan are timed through it as well")
    ap.add_argument("--out", default=None, help="also append the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_foot()
    K = synthetic.intrinsics(sp.W, sp.H)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    f = binding.Fusion(lib, lib.default_config(**cam))
    dev = torch.device("cuda")
    state, dist2 = sp.grid_on_device(f, torch, dev)
    plan_here, rounds, cost = sp.plan_wall(f, state, dist2, torch, dev, a.reps)
    h_state, h_dist2, h_cost = state.cpu().numpy(), dist2.cpu().numpy(), cost.cpu().numpy().view(np.uint32)
    say("[grid] %d x %d: %d free, %d occupied, %d unknown cells; the field reaches %d cells in %d rounds" %
        (N, N, int((h_state == 0).sum()), int((h_state == 100).sum()), int((h_state == -1).sum()), int((h_cost != sr.NO_COST).sum()), rounds))
    say("%d calls per figure after %d warm-ups; times in ms: median (smallest .. largest)" % (a.reps, WARM))

    # ---- the layers -------------------------------------------------------------------------------------------------------------
    mask = torch.zeros((N, N), dtype=torch.int32, device=dev)
    pad = binding.Fusion.nav_foot_pad(n_headings=BINS, **BODY)
    for name, kw in (("12 x 8 cells, pad %d" % pad, dict(BODY, pad=pad)), ("the largest: 28 cells to every side", LARGEST)):
        wall, per, got = timed(f, lambda: f.nav_foot_device(state, N, N, free_mask=mask, n_headings=BINS, **kw), ("navfoot_layers",), a.reps)
        say("[layers, %s, %d headings] wall %s | navfoot_layers %s | %s" % (name, BINS, sp.spread(wall), sp.spread(per[:, 0]),
                                                                             " ".join("%s=%d" % kv for kv in got.items())))
        rec = dict(layers=name, headings=BINS, wall_ms=[round(float(x), 4) for x in (np.median(wall), np.min(wall), np.max(wall))],
                   kernel_ms=round(float(np.median(per[:, 0])), 4), stats=got)
        if kw is not LARGEST:
            t0 = time.perf_counter()
            hs = state.cpu().numpy()
            t_out = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            want = fr.layers(hs, 0, (kw["front"], kw["back"], kw["left"], kw["right"], kw["pad"]), BINS)
            t_ref = 1e3 * (time.perf_counter() - t0)
            equal = bool(np.array_equal(mask.cpu().numpy().view(np.uint32), want["free_mask"]) and got == want["stats"])
            say("[layers, %s] the host route: state out %.3f ms + the restatement's dilation (numpy) %.0f ms; mask and stats equal with ==: %s" %
                (name, t_out, t_ref, equal))
            rec.update(host_out_ms=round(t_out, 3), host_reference_ms=round(t_ref, 1), equal=equal)
        say(json.dumps(rec))
    f.nav_foot_device(state, N, N, free_mask=mask, n_headings=BINS, **dict(BODY, pad=pad))
    h_mask = mask.cpu().numpy().view(np.uint32)

    # ---- the rollouts beside the disc's ------------------------------------------------------------------------------------------
    rng = np.random.default_rng(3)
    fits = np.argwhere((h_mask != 0) & (h_dist2 >= PLAN["min_dist2"]))
    pick = fits[rng.permutation(len(fits))[:max(POSES)]]
    bits = h_mask[pick[:, 0], pick[:, 1]]
    first_bin = np.array([int(b & -b).bit_length() - 1 for b in bits.tolist()])                    # a heading at which the body fits there
    all_poses = np.stack([pick[:, 1] * 1024 + rng.integers(0, 1024, len(pick)), pick[:, 0] * 1024 + rng.integers(0, 1024, len(pick)),
                          first_bin * (65536 // BINS)], axis=1).astype(np.int32)
    c0 = sr.params(width=N, height=N, min_dist2=PLAN["min_dist2"])
    T = c0["n_steps"]
    for n in POSES:
        poses = np.ascontiguousarray(all_poses[:n])
        d_poses = torch.from_numpy(poses).to(dev)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        o = dict(best=i32(n), best_cmd=i32(n, 2), best_score=torch.zeros(n, dtype=torch.int64, device=dev), n_admissible=i32(n), pose_status=i32(n),
                 best_len=i32(n), best_traj=i32(n, T + 1, 3))
        wall, per, got = timed(f, lambda: f.nav_foot_steer_device(mask, dist2, N, N, d_poses, n, BINS, cost=cost, min_dist2=PLAN["min_dist2"], **o),
                               FOOT_KERNELS, a.reps)
        first = {nm: t.cpu().numpy() for nm, t in o.items()}
        say("[footprint rollouts, %d poses] wall %s | %s | summed %.4f | %s" %
            (n, sp.spread(wall), "  ".join("%s %s" % (k, sp.spread(per[:, i])) for i, k in enumerate(FOOT_KERNELS)), float(np.median(per, axis=0).sum()),
             " ".join("%s=%d" % (k, got[k]) for k in sr.STATS)))
        rec = dict(n_poses=n, foot=dict(wall_ms=[round(float(x), 4) for x in (np.median(wall), np.min(wall), np.max(wall))],
                                        kernel_ms={k: round(float(np.median(per[:, i])), 4) for i, k in enumerate(FOOT_KERNELS)},
                                        stats={k: got[k] for k in sr.STATS}))
        wall, per, disc = timed(f, lambda: f.nav_steer_device(state, dist2, N, N, d_poses, n, cost=cost, min_dist2=PLAN["min_dist2"], **o), sp.KERNELS, a.reps)
        say("[disc rollouts, %d poses, the same grid, field and poses] wall %s | %s | summed %.4f | %s" %
            (n, sp.spread(wall), "  ".join("%s %s" % (k, sp.spread(per[:, i])) for i, k in enumerate(sp.KERNELS)), float(np.median(per, axis=0).sum()),
             " ".join("%s=%d" % (k, disc[k]) for k in sr.STATS)))
        rec["disc"] = dict(wall_ms=[round(float(x), 4) for x in (np.median(wall), np.min(wall), np.max(wall))],
                           kernel_ms={k: round(float(np.median(per[:, i])), 4) for i, k in enumerate(sp.KERNELS)}, stats={k: disc[k] for k in sr.STATS})
        if n < max(POSES):
            t0 = time.perf_counter()
            hm, hd, hc = mask.cpu().numpy().view(np.uint32), dist2.cpu().numpy(), cost.cpu().numpy().view(np.uint32)
            t_out = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            want = fr.rollouts(hm, BINS, hd, hc, poses, None, dict(c0, n_poses=n))
            t_ref = 1e3 * (time.perf_counter() - t0)
            equal = all(np.array_equal(first[nm].astype(sr.DTYPES[nm]), want[nm]) for nm in o if nm != "best_traj")
            equal = bool(equal and all(np.array_equal(first["best_traj"][q, :want["best_len"][q]], want["best_traj"][q, :want["best_len"][q]]) for q in range(n))
                         and all(got[k] == want["stats"][k] for k in sr.STATS))
            say("[footprint rollouts, %d poses] the host route: copies out %.3f ms + the restatement (numpy) %.0f ms; every output equal with ==: %s" %
                (n, t_out, t_ref, equal))
            rec.update(host_out_ms=round(t_out, 3), host_reference_ms=round(t_ref, 1), equal=equal)
        say(json.dumps(rec))

    # ---- the disc's rollouts and the plan against another build ---------------------------------------------------------------------
    def disc_and_plan(g, tag):
        s2, d2 = sp.grid_on_device(g, torch, dev)
        pw, r2, c2 = sp.plan_wall(g, s2, d2, torch, dev, a.reps)
        out = dict(plan_ms=round(float(np.median(pw)), 4), rounds=r2)
        say("[%s] nav_plan wall %s (%d rounds)" % (tag, sp.spread(pw), r2))
        for n in POSES:
            d_poses = torch.from_numpy(np.ascontiguousarray(all_poses[:n])).to(dev)
            i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
            o = dict(best=i32(n), best_cmd=i32(n, 2), best_score=torch.zeros(n, dtype=torch.int64, device=dev), n_admissible=i32(n), pose_status=i32(n),
                     best_len=i32(n), best_traj=i32(n, T + 1, 3))
            wall, per, st = timed(g, lambda: g.nav_steer_device(s2, d2, N, N, d_poses, n, cost=c2, min_dist2=PLAN["min_dist2"], **o), sp.KERNELS, a.reps)
            say("[%s] nav_steer, %d poses: wall %s | %s | summed %.4f" %
                (tag, n, sp.spread(wall), "  ".join("%s %s" % (k, sp.spread(per[:, i])) for i, k in enumerate(sp.KERNELS)), float(np.median(per, axis=0).sum())))
            out["steer_%d" % n] = dict(wall_ms=[round(float(x), 4) for x in (np.median(wall), np.min(wall), np.max(wall))],
                                       kernel_ms={k: round(float(np.median(per[:, i])), 4) for i, k in enumerate(sp.KERNELS)},
                                       sum=int(o["best"].sum().item()), score=int(o["best_score"].sum().item()))
        return out

    f.close()
    if a.other_lib:
        rec = {}
        for tag, path in (("this library", None), ("the other library", a.other_lib), ("this library again", None)):
            L = lib if path is None else binding.Library(path)
            g = binding.Fusion(L, L.default_config(**cam))
            rec[tag] = disc_and_plan(g, tag)
            g.close()
        same = all(rec["this library"]["steer_%d" % n][k] == rec["the other library"]["steer_%d" % n][k] for n in POSES for k in ("sum", "score"))
        say("[other] %s; the winners and their scores are the same through both: %s" % (os.path.relpath(a.other_lib, ROOT), same))
        rec["same_winners"] = bool(same)
        say(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
