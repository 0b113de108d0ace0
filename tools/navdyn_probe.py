"""ssf_navdyn_rollouts, ssf_navdyn_foot_rollouts and ssf_navdyn_blobs (include/ssf_navdyn.h) at the size a robot has:
tools/navsteer_probe.py's 512 x 512 hall (walls, hashed pillars, unknown patches; clearance from ssf_navlive_overlay's identity,
cost-to-goal field from ssf_navplan_field), device arrays in and out, per-pose outputs only.

Reports, after 5 warm-ups, medians of --reps calls with the smallest and largest as the spread:
  * the rollouts at 1, 16 and 4096 poses on the default lattice (9 x 33 candidates, 32 steps) with 0, 1, 16 and 64 movers walking about
    the hall, the whole call (a host clock around the synchronous call, profile off) and per kernel (ssf_get_kernel_times under
    profile = 1), beside nav_steer and nav_foot_steer on the same grid, field and poses through the same library;
  * the blobs of a 640 x 480 frame with a person-sized mask (a third of the width, most of the height, two labels), with the tile
    merge in LDS and without it, and the host route a caller had before: label, mask and depth copied out and tests/navdyn_ref.py's
    blobs (numpy and Python ints: a statement of the rule, not a tuned implementation); the tables are compared with ==;
  * with --other-lib (the parent commit's libssf_hip_pose.so), nav_steer, nav_foot_steer and nav_plan on the same inputs through this
    library, the other, this one again and the other again, in one process: the older calls cost what they cost.  The two runs of the
    other library give its own run-to-run spread.
Prints a table and JSON lines; --out also writes them to a file.  No threshold is asserted: the table is the record.

    python tools/navdyn_probe.py [--reps 20] [--other-lib PATH] [--out FILE]"""
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
import navdyn_ref as dr  # noqa: E402
import navlive_ref as lr  # noqa: E402
import navsteer_ref as sr  # noqa: E402
import navsteer_probe as sp  # noqa: E402
from navfoot_probe import BINS, BODY, FOOT_KERNELS, timed  # noqa: E402

N, PLAN, POSES = sp.N, sp.PLAN, sp.POSES
DYN_KERNELS = ("navdyn_pack", "navdyn_roll", "navdyn_pick")
BLOB_KERNELS = ("navdyn_blob_seen", "navdyn_blob_slots", "navdyn_blob_sum")
MOVERS = (0, 1, 16, 64)


def med3(x):
    return [round(float(v), 4) for v in (np.median(x), np.min(x), np.max(x))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--other-lib", default=None, help="another build of libssf_hip_pose.so: nav_steer, nav_foot_steer and nav_plan are timed through it as well")
    ap.add_argument("--out", default=None, help="also append the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_dyn()
    K = synthetic.intrinsics(sp.W, sp.H)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    f = binding.Fusion(lib, lib.default_config(**cam))
    dev = torch.device("cuda")
    state, dist2 = sp.grid_on_device(f, torch, dev)
    _, rounds, cost = sp.plan_wall(f, state, dist2, torch, dev, a.reps)
    h_state, h_dist2, h_cost = state.cpu().numpy(), dist2.cpu().numpy(), cost.cpu().numpy().view(np.uint32)
    say("[grid] %d x %d: %d free cells; the field reaches %d cells in %d rounds" % (N, N, int((h_state == 0).sum()), int((h_cost != sr.NO_COST).sum()), rounds))
    say("%d calls per figure after %d warm-ups; times in ms: median (smallest .. largest)" % (a.reps, sp.WARM))
    mask = torch.zeros((N, N), dtype=torch.int32, device=dev)
    pad = binding.Fusion.nav_foot_pad(n_headings=BINS, **BODY)
    f.nav_foot_device(state, N, N, free_mask=mask, n_headings=BINS, **dict(BODY, pad=pad))
    h_mask = mask.cpu().numpy().view(np.uint32)
    rng = np.random.default_rng(3)
    fits = np.argwhere((h_mask != 0) & (h_dist2 >= PLAN["min_dist2"]))
    pick = fits[rng.permutation(len(fits))[:max(POSES)]]
    bits = h_mask[pick[:, 0], pick[:, 1]]
    first_bin = np.array([int(b & -b).bit_length() - 1 for b in bits.tolist()])
    all_poses = np.stack([pick[:, 1] * 1024 + rng.integers(0, 1024, len(pick)), pick[:, 0] * 1024 + rng.integers(0, 1024, len(pick)),
                          first_bin * (65536 // BINS)], axis=1).astype(np.int32)
    # the movers walk about the first poses, so that they are met: half a cell a step at the most, people-sized discs plus the robot's radius
    near = all_poses[rng.integers(0, 16, max(MOVERS))]
    all_movers = np.stack([near[:, 0] + rng.integers(-12 * 1024, 12 * 1024, len(near)), near[:, 1] + rng.integers(-12 * 1024, 12 * 1024, len(near)),
                           rng.integers(-512, 513, len(near)), rng.integers(-512, 513, len(near)), rng.integers(6000, 12000, len(near)),
                           rng.integers(0, 64, len(near))], axis=1).astype(np.int32)
    c0 = dr.params(width=N, height=N, min_dist2=PLAN["min_dist2"])
    T = c0["n_steps"]

    def outputs(n):
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        return dict(best=i32(n), best_cmd=i32(n, 2), best_score=torch.zeros(n, dtype=torch.int64, device=dev), n_admissible=i32(n), pose_status=i32(n),
                    best_len=i32(n), best_traj=i32(n, T + 1, 3))

    # ---- the rollouts among movers beside the older calls ----------------------------------------------------------------------------
    for n in POSES:
        poses = np.ascontiguousarray(all_poses[:n])
        d_poses = torch.from_numpy(poses).to(dev)
        o = outputs(n)
        rec = dict(n_poses=n)
        for nm, call, kernels in (("nav_steer", lambda: f.nav_steer_device(state, dist2, N, N, d_poses, n, cost=cost, min_dist2=PLAN["min_dist2"], **o), sp.KERNELS),
                                  ("nav_foot_steer", lambda: f.nav_foot_steer_device(mask, dist2, N, N, d_poses, n, BINS, cost=cost, min_dist2=PLAN["min_dist2"], **o),
                                   FOOT_KERNELS)):
            wall, per, st = timed(f, call, kernels, a.reps)
            say("[%s, %d poses] wall %s | %s | summed %.4f" % (nm, n, sp.spread(wall), "  ".join("%s %s" % (k, sp.spread(per[:, i])) for i, k in enumerate(kernels)),
                                                             float(np.median(per, axis=0).sum())))
            rec[nm] = dict(wall_ms=med3(wall), kernel_ms={k: round(float(np.median(per[:, i])), 4) for i, k in enumerate(kernels)})
        gap = torch.zeros(n, dtype=torch.int32, device=dev)
        for m in MOVERS:
            movers = np.ascontiguousarray(all_movers[:m])
            d_movers = torch.from_numpy(movers).to(dev) if m else None
            for nm, grid, bins in (("disc", state, None), ("footprint", mask, BINS)):
                wall, per, st = timed(f, lambda: f.nav_dyn_steer_device(grid, dist2, N, N, d_poses, n, movers=d_movers, n_movers=m, n_headings=bins, cost=cost,
                                                                       min_dist2=PLAN["min_dist2"], best_min_gap=gap, **o), DYN_KERNELS, a.reps)
                say("[among %d movers, %s, %d poses] wall %s | %s | summed %.4f | hit_movers=%d collided=%d admissible=%d" %
                    (m, nm, n, sp.spread(wall), "  ".join("%s %s" % (k, sp.spread(per[:, i])) for i, k in enumerate(DYN_KERNELS)),
                     float(np.median(per, axis=0).sum()), st["hit_movers"], st["collided"], st["admissible"]))
                rec["%s_%d" % (nm, m)] = dict(wall_ms=med3(wall), kernel_ms={k: round(float(np.median(per[:, i])), 4) for i, k in enumerate(DYN_KERNELS)},
                                               hit_movers=st["hit_movers"])
                if n == 16 and m == 16:                                  # the device's answer against the restatement, once per body
                    first = {k: t.cpu().numpy() for k, t in dict(o, best_min_gap=gap).items()}
                    want = dr.rollouts(h_mask if bins else h_state, h_dist2, h_cost, poses, None, movers, dict(c0, n_poses=n), bins)
                    equal = all(np.array_equal(first[k].astype(dr.DTYPES[k]), want[k]) for k in first if k != "best_traj")
                    equal = bool(equal and all(st[k] == want["stats"][k] for k in dr.STATS))
                    say("[among 16 movers, %s, 16 poses] every per-pose output and exact stat equals the restatement with ==: %s" % (nm, equal))
                    rec["%s_equal" % nm] = equal
        say(json.dumps(rec))

    # ---- the blobs of a 640 x 480 frame -------------------------------------------------------------------------------------------
    cw, ch = 640, 480
    bcam = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, cam_width=cw, cam_height=ch, t_min=0.2, t_max=5.0)
    depth = np.full((ch, cw), 3.0, np.float32)
    depth[40:460, 220:430] = (1.5 + 0.2 * np.arange(210) / 210).astype(np.float32)[None, :]           # a person-sized thing 1.5 m ahead
    bmask = np.zeros((ch, cw), np.uint8)
    bmask[40:460, 220:430] = 1
    label = np.where(bmask != 0, np.where(np.arange(cw)[None, :] < 330, 40 * cw + 220, 40 * cw + 330), -1).astype(np.int32)
    gpose, cpose = lr.grid_pose_at(-2.0, 0.0), lr.room_pose(at=(0.0, 0.0, 0.2))
    kw = dict(bcam, grid_pose=gpose, cam_pose=cpose, width=N, height=N, res=0.05)
    d_depth, d_bmask, d_label = (torch.from_numpy(x).to(dev) for x in (depth, bmask, label))
    rec = dict(frame=[cw, ch])
    for direct in (0, 1):
        wall, per, got = timed(f, lambda: f.nav_dyn_blobs_device(d_depth, d_bmask, d_label, direct=direct, **kw), BLOB_KERNELS, a.reps)
        say("[blobs, %d x %d, direct=%d (%s)] wall %s | %s | summed %.4f | %s" %
            (cw, ch, direct, "every pixel adds to the table itself" if direct else "a tile is merged in LDS first", sp.spread(wall),
             "  ".join("%s %s" % (k, sp.spread(per[:, i])) for i, k in enumerate(BLOB_KERNELS)), float(np.median(per, axis=0).sum()),
             " ".join("%s=%d" % kv for kv in got["stats"].items())))
        rec["direct_%d" % direct] = dict(wall_ms=med3(wall), kernel_ms={k: round(float(np.median(per[:, i])), 4) for i, k in enumerate(BLOB_KERNELS)},
                                       stats=got["stats"])
    t0 = time.perf_counter()
    hd, hm, hl = d_depth.cpu().numpy(), d_bmask.cpu().numpy(), d_label.cpu().numpy()
    t_out = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = dr.blobs(hd, hm, hl, gpose, cpose, lr.params(width=N, height=N, res=0.05, **bcam), 16, 64)
    t_ref = 1e3 * (time.perf_counter() - t0)
    equal = bool(np.array_equal(got["blobs"], want["blobs"]) and got["stats"] == want["stats"])
    say("[blobs] the host route: label, mask and depth out %.3f ms + the restatement %.0f ms; table and stats equal with ==: %s" % (t_out, t_ref, equal))
    rec.update(host_out_ms=round(t_out, 3), host_reference_ms=round(t_ref, 1), equal=equal)
    say(json.dumps(rec))
    f.close()

    # ---- the older calls against another build ------------------------------------------------------------------------------------
    def older(g, tag):
        s2, d2 = sp.grid_on_device(g, torch, dev)
        pw, r2, c2 = sp.plan_wall(g, s2, d2, torch, dev, a.reps)
        out = dict(plan_ms=med3(pw), rounds=r2)
        say("[%s] nav_plan wall %s (%d rounds)" % (tag, sp.spread(pw), r2))
        m2 = torch.zeros((N, N), dtype=torch.int32, device=dev)
        g.nav_foot_device(s2, N, N, free_mask=m2, n_headings=BINS, **dict(BODY, pad=pad))
        for n in POSES:
            d_poses = torch.from_numpy(np.ascontiguousarray(all_poses[:n])).to(dev)
            o = outputs(n)
            for nm, call, kernels in (("steer", lambda: g.nav_steer_device(s2, d2, N, N, d_poses, n, cost=c2, min_dist2=PLAN["min_dist2"], **o), sp.KERNELS),
                                      ("foot", lambda: g.nav_foot_steer_device(m2, d2, N, N, d_poses, n, BINS, cost=c2, min_dist2=PLAN["min_dist2"], **o), FOOT_KERNELS)):
                wall, per, st = timed(g, call, kernels, a.reps)
                say("[%s] nav_%s, %d poses: wall %s | %s | summed %.4f" %
                    (tag, "steer" if nm == "steer" else "foot_steer", n, sp.spread(wall), "  ".join("%s %s" % (k, sp.spread(per[:, i])) for i, k in enumerate(kernels)),
                     float(np.median(per, axis=0).sum())))
                out["%s_%d" % (nm, n)] = dict(wall_ms=med3(wall), kernel_sum_ms=round(float(np.median(per, axis=0).sum()), 4),
                                              sum=int(o["best"].sum().item()), score=int(o["best_score"].sum().item()))
        return out

    if a.other_lib:
        rec = {}
        for tag, path in (("this library", None), ("the other library", a.other_lib), ("this library again", None), ("the other library again", a.other_lib)):
            L = lib if path is None else binding.Library(path)
            g = binding.Fusion(L, L.default_config(**cam))
            rec[tag] = older(g, tag)
            g.close()
        same = all(rec["this library"]["%s_%d" % (nm, n)][k] == rec["the other library"]["%s_%d" % (nm, n)][k] for n in POSES for nm in ("steer", "foot")
                   for k in ("sum", "score"))
        say("[other] %s; the winners and their scores are the same through both: %s" % (os.path.basename(a.other_lib), same))
        rec["same_winners"] = bool(same)
        say(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
