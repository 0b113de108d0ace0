"""ssf_navmem_update (include/ssf_navmem.h) on the workload a robot has, next to ssf_navlive_overlay in the same process: the setup of
tools/navlive_probe.py (the 640 x 480 depth frame of the synthetic stream, and a wall across the whole image at 0.6 m, onto the carved
512 x 512 grid of the ~1 M-row synthetic map), device arrays in and out, the layer updated in place, the defaults (16 slices).

Reports, with warm-ups and --reps repetitions (medians, and the smallest and largest of the repetitions as the spread):
  * the whole call (a host clock around the synchronous call, profile off) and each kernel (ssf_get_kernel_times under profile = 1) of
    ssf_navlive_overlay and of ssf_navmem_update, the ratio to the overlay, and points and samples per atomic;
  * the host route, as a statement of the rule and not a tuned implementation: arrays out, tests/navmem_ref.py, arrays back; the
    device's outputs are compared with it with ==;
  * the older calls through this library and, with --other-lib, through another build of libssf_hip_dyn.so (the parent commit's):
    nav_live and nav_plan, alternating this / other / this / other in one process.
Prints a table and JSON lines; --out also writes them to a file.  No threshold is asserted: the table is the record.

    python tools/navmem_probe.py [--rows 1000000] [--reps 20] [--other-lib PATH] [--out FILE]"""
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
import navmem_ref as mr  # noqa: E402
import navlive_probe as lp  # noqa: E402

WARM, N, W, H, FRAME = lp.WARM, lp.N, lp.W, lp.H, lp.FRAME
LIVE_KERNELS = lp.KERNELS
MEM_KERNELS = ("navmem_stamp", "navmem_march", "navmem_cells", "navgrid_columns", "navgrid_rows")
spread = lp.spread


def timed(f, call, kernels, reps):
    """(wall clocks in ms with profile off, per-kernel ms under profile = 1 as reps x kernels, the last call's result)"""
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


def older_calls(f, frame, state, dist2, kw, torch, dev, reps):
    """the wall clocks in ms of nav_live (the stream frame onto the carved grid) and of nav_plan (tools/navplan_probe.py's scene)"""
    o = dict(live_hits=torch.zeros((N, N), dtype=torch.int32, device=dev), live_seen=torch.zeros((N, N), dtype=torch.int32, device=dev),
             state_out=torch.zeros((N, N), dtype=torch.int8, device=dev), dist2=torch.zeros((N, N), dtype=torch.int32, device=dev))
    live = []
    for k in range(WARM + reps):
        t0 = time.perf_counter()
        f.nav_live_device(frame, state, N, N, **dict(o, **kw))
        if k >= WARM:
            live.append(1e3 * (time.perf_counter() - t0))
    plan, _ = lp.plan_wall(f, state, dist2, torch, dev, reps)
    return live, plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--other-lib", default=None, help="another build of libssf_hip_dyn.so: nav_live and nav_plan are timed through it as well")
    ap.add_argument("--out", default=None, help="also append the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_mem()
    K = synthetic.intrinsics(W, H)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    f = binding.Fusion(lib, lib.default_config(**cam, nb_supersurfels_max=a.rows + 4096))
    dev = torch.device("cuda")
    state, dist2, gs, bands, _ = lp.carved_grid(f, a.rows, torch, dev)
    grid_pose = gs["pose"]
    say("[map] synthetic %d rows; carved grid 512x512@0.05: %d free, %d occupied, %d unknown" %
        (a.rows, gs["cells_free"], gs["cells_occupied"], gs["cells_unknown"]))
    say("%d x %d depth frame, %d x %d cells, 16 slices; %d calls per figure after %d warm-ups; times in ms: median (smallest .. largest)" % (W, H, N, N, a.reps, WARM))
    cam_pose = nr.pose_about(*synthetic.relative_pose(FRAME))
    _, stream, _ = synthetic.render(*synthetic.orbit_pose(FRAME), W, H, noise=True, rng=np.random.default_rng(FRAME))
    stream = np.ascontiguousarray(stream, np.float32)
    frames = (("stream frame %d" % FRAME, stream), ("wall at 0.6 m", np.full((H, W), 0.6, np.float32)))
    kw = dict(grid_pose=grid_pose, cam_pose=cam_pose, res=0.05, floor_max=bands["floor_max"], z_max=bands["z_max"])
    i32 = lambda: torch.zeros((N, N), dtype=torch.int32, device=dev)
    lo = dict(live_hits=i32(), live_seen=i32(), state_out=torch.zeros((N, N), dtype=torch.int8, device=dev), dist2=i32())
    mo = dict(live_hits=i32(), hit_bits=i32(), seen_bits=i32(), state_out=torch.zeros((N, N), dtype=torch.int8, device=dev), dist2=i32())
    for name, depth in frames:
        d_depth = torch.from_numpy(depth).to(dev)
        lw, lper, lgot = timed(f, lambda: f.nav_live_device(d_depth, state, N, N, **dict(lo, **kw)), LIVE_KERNELS, a.reps)
        say("[%s] %d valid pixels, %d points in the band, %d rays, %d samples" % (name, lgot["pixels_valid"], lgot["points_in_band"], lgot["rays"], lgot["ray_samples"]))
        say("[%s] nav_live: wall %s | kernels: %s | summed %.4f" % (name, spread(lw), "  ".join("%s %s" % (k, spread(lper[:, i])) for i, k in enumerate(LIVE_KERNELS)),
                                                                  float(np.median(lper, axis=0).sum())))
        rec = dict(frame=name, live_wall_ms=round(float(np.median(lw)), 4), live_kernel_ms={k: round(float(np.median(lper[:, i])), 4) for i, k in enumerate(LIVE_KERNELS)},
                   live_atomics=lgot["atomics"])
        mem = binding.LiveMemory(N, N, device=True)
        mw, mper, mgot = timed(f, lambda: f.nav_memory_device(d_depth, state, N, N, memory=mem, **dict(mo, **kw)), MEM_KERNELS, a.reps)
        say("[%s] nav_memory: wall %s (%.2f x nav_live) | kernels: %s | summed %.4f" %
            (name, spread(mw), float(np.median(mw)) / float(np.median(lw)), "  ".join("%s %s" % (k, spread(mper[:, i])) for i, k in enumerate(MEM_KERNELS)),
             float(np.median(mper, axis=0).sum())))
        say("[%s] nav_memory: %d atomics, %.1f points and samples per atomic (nav_live: %d atomics); %d cells marked, %d remembered" %
            (name, mgot["atomics"], (mgot["points_in_band"] + mgot["ray_samples"]) / max(mgot["atomics"], 1), lgot["atomics"], mgot["cells_marked"],
             mgot["cells_remembered"]))
        rec["mem"] = dict(wall_ms=[round(float(x), 4) for x in (np.median(mw), np.min(mw), np.max(mw))],
                          kernel_ms={k: round(float(np.median(mper[:, i])), 4) for i, k in enumerate(MEM_KERNELS)}, atomics=mgot["atomics"])
        # the host route on a zero layer at tick 1: arrays out, the restatement, arrays back
        mem = binding.LiveMemory(N, N, device=True)
        got = f.nav_memory_device(d_depth, state, N, N, memory=mem, **dict(mo, **kw))
        t0 = time.perf_counter()
        h_depth, h_state = d_depth.cpu().numpy(), state.cpu().numpy()
        t_out = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        c = mr.params(cfg_camera=K, width=N, height=N, res=0.05, floor_max=bands["floor_max"], z_max=bands["z_max"])
        want = mr.update(h_depth, None, h_state, None, grid_pose, cam_pose, c)
        t_ref = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        back = [torch.from_numpy(want[nm].view(np.int32) if want[nm].dtype == np.uint32 else want[nm]).to(dev) for nm in mr.LAYER + ("state", "dist2")]
        torch.cuda.synchronize()
        t_back = 1e3 * (time.perf_counter() - t0)
        del back
        h = dict(mem.numpy(), state=mo["state_out"].cpu().numpy(), dist2=mo["dist2"].cpu().numpy(),
                 **{nm: mo[nm].cpu().numpy().view(np.uint32) for nm in ("live_hits", "hit_bits", "seen_bits")})
        equal = bool(all(np.array_equal(h[nm], want[nm]) for nm in mr.OUTPUTS) and all(got[k] == want["stats"][k] for k in mr.STATS))
        say("[%s] the host route (a statement of the rule, not a tuned implementation): copies out %.3f ms + the restatement (numpy) %.0f ms + copies back "
            "%.3f ms; every output equal with ==: %s" % (name, t_out, t_ref, t_back, equal))
        rec.update(host_out_ms=round(t_out, 3), host_reference_ms=round(t_ref, 1), host_back_ms=round(t_back, 3), equal=equal)
        say(json.dumps(rec))
    # the older calls: this library and the other in turn
    d_stream = torch.from_numpy(stream).to(dev)
    rec = {}
    if a.other_lib:
        other = binding.Library(a.other_lib)
        g = binding.Fusion(other, other.default_config(**cam, nb_supersurfels_max=a.rows + 4096))
        s2, d2, gs2, _, _ = lp.carved_grid(g, a.rows, torch, dev)
        same = bool(np.array_equal(s2.cpu().numpy(), state.cpu().numpy()) and np.array_equal(d2.cpu().numpy(), dist2.cpu().numpy()))
        say("[older calls] the other library is %s; the same carved grid: %s" % (os.path.relpath(a.other_lib, ROOT), same))
        for turn in range(2):
            for who, h_, s_, d_ in (("this", f, state, dist2), ("other", g, s2, d2)):
                live, plan = older_calls(h_, d_stream, s_, d_, kw, torch, dev, a.reps)
                say("[older calls] turn %d, %s library: nav_live wall %s ms; nav_plan wall %s ms" % (turn + 1, who, spread(live), spread(plan)))
                rec["%s_%d" % (who, turn + 1)] = dict(nav_live_ms=round(float(np.median(live)), 4), nav_plan_ms=round(float(np.median(plan)), 3))
        g.close()
    else:
        live, plan = older_calls(f, d_stream, state, dist2, kw, torch, dev, a.reps)
        say("[older calls] this library: nav_live wall %s ms; nav_plan wall %s ms" % (spread(live), spread(plan)))
        rec["this_1"] = dict(nav_live_ms=round(float(np.median(live)), 4), nav_plan_ms=round(float(np.median(plan)), 3))
    f.close()
    say(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
