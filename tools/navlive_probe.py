"""ssf_navlive_overlay (include/ssf_navlive.h) on the workload a robot has: the 640 x 480 depth frame of the synthetic stream stamped
onto the carved 512 x 512 grid of the ~1 M-row synthetic map of the other probes (tools/navcarve_probe.py: 64 views along the orbit,
stride 8), device arrays in and out.  A second frame is a wall across the whole image at 0.6 m: every pixel column lands in one
cell, the worst contention on live_hits, and every ray ends after a few cells.  A third puts a person-sized block at 0.9 m into the
stream frame and stamps it onto an all-unknown grid, where the frame stamps and opens many cells (the synthetic map's rows fill the
room, so on its own grid the frame changes almost nothing; the cost does not depend on that).

Reports, with warm-ups and --reps repetitions (medians, and the smallest and largest of the repetitions as the spread):
  * the whole call (a host clock around the synchronous call, profile off) and each kernel (hipEvent brackets of ssf_get_kernel_times
    under profile = 1), on both frames, at the default parameters (stride 4, min_hits 4);
  * points per atomic in the stamp and entries per atomic in the march (the stamp's atomics from a call that skips the march);
  * the host route a caller had before, as a statement of the rule and not a tuned implementation: the depth image and the state copied
    out, tests/navlive_ref.py, state and dist2 copied back; the device's outputs are compared with it with ==;
  * nav_grid_carve through the same library: the only way to refresh the grid without this call (it asks the map, not the sensor);
  * nav_plan (the carved-map scene of tools/navplan_probe.py) through this library and, with --other-lib, through another build of
    libssf_hip_drive.so (the parent commit's), to show that the plan costs what it cost.
Prints a table and JSON lines; --out also writes them to a file.  No threshold is asserted: the table is the record.

    python tools/navlive_probe.py [--rows 1000000] [--reps 20] [--other-lib PATH] [--out FILE]"""
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
import navlive_ref as lr  # noqa: E402

WARM = 5
KERNELS = ("navlive_stamp", "navlive_march", "navlive_cells", "navgrid_columns", "navgrid_rows")
N = 512
W, H = 640, 480
FRAME = 10
PLAN = dict(allow_unknown=1, goals_from_frontier=1, min_dist2=4, soft_dist2=100, near_penalty=50)       # tools/navplan_probe.py's carved-map scene


def carved_grid(f, rows, torch, dev, time_it=0):
    model, nvis = synthetic.seed_model_cam0(rows, W, H, stamp=30)
    f.set_model(model, nvis, 30)
    y = model["positions"][:, 1]
    bands = dict(z_min=float(-y.max() - 0.1), z_max=float(-y.min() + 0.1), floor_max=float(-np.median(y)))
    views = np.stack([nr.pose_about(*synthetic.relative_pose(k)) for k in range(64)])
    state, dist2 = torch.zeros((N, N), dtype=torch.int8, device=dev), torch.zeros((N, N), dtype=torch.int32, device=dev)
    wall = []
    for k in range(1 + time_it):
        t0 = time.perf_counter()
        gs = f.nav_grid_carve_device(views, state=state, dist2=dist2, carve=dict(stride=8), width=N, height=N, res=0.05, **bands)
        wall.append(1e3 * (time.perf_counter() - t0))
    return state, dist2, gs, bands, wall[1:]


def plan_wall(f, state, dist2, torch, dev, reps):
    """the wall clocks in ms of tools/navplan_probe.py's call on the carved map"""
    starts = np.stack([np.linspace(5, N - 6, 16).astype(np.int32), np.linspace(N - 6, 4, 16).astype(np.int32)], axis=1)
    outs = dict(cost=torch.zeros((N, N), dtype=torch.int32, device=dev), frontier=torch.zeros((N, N), dtype=torch.uint8, device=dev),
                start_cost=torch.zeros(16, dtype=torch.int32, device=dev), start_status=torch.zeros(16, dtype=torch.int32, device=dev),
                path_len=torch.zeros(16, dtype=torch.int32, device=dev), path=torch.zeros((16, 4096, 2), dtype=torch.int32, device=dev))
    wall = []
    for k in range(WARM + reps):
        t0 = time.perf_counter()
        st = f.nav_plan_device(state, dist2, N, N, [(N // 2, N // 2)], starts, max_path=4096, **dict(outs, **PLAN))
        if k >= WARM:
            wall.append(1e3 * (time.perf_counter() - t0))
    return wall, st["rounds"]


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--other-lib", default=None, help="another build of libssf_hip_drive.so: nav_plan is timed through it as well")
    ap.add_argument("--out", default=None, help="also append the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_live()
    K = synthetic.intrinsics(W, H)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    f = binding.Fusion(lib, lib.default_config(**cam, nb_supersurfels_max=a.rows + 4096))
    dev = torch.device("cuda")
    state, dist2, gs, bands, carve_ms = carved_grid(f, a.rows, torch, dev, time_it=5)
    grid_pose = gs["pose"]
    say("[map] synthetic %d rows; carved grid 512x512@0.05: %d free, %d occupied, %d unknown" %
        (a.rows, gs["cells_free"], gs["cells_occupied"], gs["cells_unknown"]))
    say("[nav_grid_carve] 64 views, stride 8, through this library: wall %s ms over 5 calls" % spread(carve_ms))
    say("%d x %d depth frame, %d x %d cells; %d calls per figure after %d warm-ups; times in ms: median (smallest .. largest)" % (W, H, N, N, a.reps, WARM))
    cam_pose = nr.pose_about(*synthetic.relative_pose(FRAME))
    _, stream, _ = synthetic.render(*synthetic.orbit_pose(FRAME), W, H, noise=True, rng=np.random.default_rng(FRAME))
    person = np.ascontiguousarray(stream, np.float32).copy()
    person[60:, 260:380] = np.minimum(person[60:, 260:380], np.float32(0.9))       # somebody 0.9 m in front of the camera, 120 pixels wide
    carved = state
    unknown = torch.full((N, N), -1, dtype=torch.int8, device=dev)
    frames = (("stream frame %d" % FRAME, np.ascontiguousarray(stream, np.float32), carved), ("wall at 0.6 m", np.full((H, W), 0.6, np.float32), carved),
              ("stream frame with a person at 0.9 m, onto an all-unknown grid", person, unknown))
    kw = dict(grid_pose=grid_pose, cam_pose=cam_pose, res=0.05, floor_max=bands["floor_max"], z_max=bands["z_max"])
    o = dict(live_hits=torch.zeros((N, N), dtype=torch.int32, device=dev), live_seen=torch.zeros((N, N), dtype=torch.int32, device=dev),
             state_out=torch.zeros((N, N), dtype=torch.int8, device=dev), dist2=torch.zeros((N, N), dtype=torch.int32, device=dev))
    for name, depth, state in frames:
        d_depth = torch.from_numpy(depth).to(dev)
        call = lambda: f.nav_live_device(d_depth, state, N, N, **dict(o, **kw))
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
        stamp_only = f.nav_live_device(d_depth, state, N, N, live_hits=o["live_hits"], open_unknown=0, **kw)
        a_stamp, a_march = stamp_only["atomics"], got["atomics"] - stamp_only["atomics"]
        say("[%s] %d valid pixels, %d points in the band, %d rays, %d samples, %d entries; %d cells stamped, %d opened" %
            (name, got["pixels_valid"], got["points_in_band"], got["rays"], got["ray_samples"], got["ray_entries"], got["cells_stamped"], got["cells_opened"]))
        say("[%s] the whole call: wall %s" % (name, spread(wall)))
        say("[%s] kernels: %s | summed %.4f" % (name, "  ".join("%s %s" % (k, spread(per[:, i])) for i, k in enumerate(KERNELS)),
                                               float(np.median(per, axis=0).sum())))
        say("[%s] stamp: %d atomics, %.1f points per atomic; march: %d atomics, %.2f entries per atomic" %
            (name, a_stamp, got["points_in_band"] / max(a_stamp, 1), a_march, got["ray_entries"] / max(a_march, 1)))
        # the host route: the frame and the state out, the restatement, state and dist2 back
        t0 = time.perf_counter()
        h_depth, h_state = d_depth.cpu().numpy(), state.cpu().numpy()
        t_out = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        c = lr.params(cfg_camera=K, width=N, height=N, res=0.05, floor_max=bands["floor_max"], z_max=bands["z_max"])
        want = lr.overlay(h_depth, None, h_state, grid_pose, cam_pose, c)
        t_ref = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        back = [torch.from_numpy(want[nm]).to(dev) for nm in ("state", "dist2")]
        torch.cuda.synchronize()
        t_back = 1e3 * (time.perf_counter() - t0)
        h = dict(live_hits=o["live_hits"].cpu().numpy().view(np.uint32), live_seen=o["live_seen"].cpu().numpy().view(np.uint32),
                 state=o["state_out"].cpu().numpy(), dist2=o["dist2"].cpu().numpy())
        equal = bool(all(np.array_equal(h[nm], want[nm]) for nm in lr.OUTPUTS) and all(got[k] == want["stats"][k] for k in lr.STATS))
        del back
        say("[%s] the host route: copies out %.3f ms + the restatement (numpy) %.0f ms + copies back %.3f ms; every output equal with ==: %s" %
            (name, t_out, t_ref, t_back, equal))
        say(json.dumps(dict(frame=name, stats={k: v for k, v in got.items() if k != "pose"}, wall_ms=[round(float(x), 4) for x in
                            (np.median(wall), np.min(wall), np.max(wall))], kernel_ms={k: round(float(np.median(per[:, i])), 4) for i, k in enumerate(KERNELS)},
                            stamp_atomics=a_stamp, march_atomics=a_march, host_out_ms=round(t_out, 3), host_reference_ms=round(t_ref, 1),
                            host_back_ms=round(t_back, 3), equal=equal)))
    state = carved
    hs, hd = state.cpu().numpy(), dist2.cpu().numpy()
    here, rounds = plan_wall(f, state, dist2, torch, dev, a.reps)
    here2, _ = plan_wall(f, state, dist2, torch, dev, a.reps)
    say("[nav_plan] the carved-map scene of tools/navplan_probe.py through this library: wall %s ms (%d rounds), and %s when timed again" %
        (spread(here), rounds, spread(here2)))
    rec = dict(nav_plan_wall_ms=round(float(np.median(here)), 3), again_ms=round(float(np.median(here2)), 3), rounds=rounds)
    f.close()
    if a.other_lib:
        other = binding.Library(a.other_lib)
        g = binding.Fusion(other, other.default_config(**cam, nb_supersurfels_max=a.rows + 4096))
        s2, d2, _, _, other_carve = carved_grid(g, a.rows, torch, dev, time_it=5)
        same = bool(np.array_equal(s2.cpu().numpy(), hs) and np.array_equal(d2.cpu().numpy(), hd))
        there, rounds2 = plan_wall(g, s2, d2, torch, dev, a.reps)
        again, _ = plan_wall(g, s2, d2, torch, dev, a.reps)
        say("[nav_plan] the same through %s: wall %s ms (%d rounds), and %s when timed again; the same grid: %s" %
            (os.path.relpath(a.other_lib, ROOT), spread(there), rounds2, spread(again), same))
        say("[nav_grid_carve] through that library: wall %s ms over 5 calls" % spread(other_carve))
        rec.update(other_nav_plan_wall_ms=round(float(np.median(there)), 3), other_again_ms=round(float(np.median(again)), 3), other_rounds=rounds2,
                   same_grid=same, other_carve_ms=round(float(np.median(other_carve)), 3), carve_ms=round(float(np.median(carve_ms)), 3))
        g.close()
        # ... and through this library once more, after the other: the order of the two is not what differs
        f2 = binding.Fusion(lib, lib.default_config(**cam, nb_supersurfels_max=a.rows + 4096))
        s3, d3, _, _, carve_again = carved_grid(f2, a.rows, torch, dev, time_it=5)
        plan_again, _ = plan_wall(f2, s3, d3, torch, dev, a.reps)
        say("[nav_grid_carve] through this library again, after the other: wall %s ms over 5 calls; nav_plan %s ms" % (spread(carve_again), spread(plan_again)))
        rec.update(carve_again_ms=round(float(np.median(carve_again)), 3), nav_plan_third_ms=round(float(np.median(plan_again)), 3))
        f2.close()
    say(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
