"""ssf_navfloor_fit (include/ssf_navfloor.h) on the maps a robot has: the ~1 M-row synthetic map of bench.py (ssf_set_model with the
bench's visible split, as tools/navgrid_probe.py) and the map of the 8 committed TUM fr1_xyz frames.

Reports, with warm-ups and --reps repetitions (medians, and the smallest and largest of the repetitions as the spread):
  * the whole call (a host clock around the synchronous call, profile off) and each kernel (ssf_get_kernel_times under profile = 1), and
    what of the wall time is not kernel time: the 3 + refine_iters waits for the stream with their small copies, and the host steps;
  * the same call with refine_iters = 0 (three waits), which prices a round;
  * the host route it replaces, as a statement of the rule and not a tuned implementation: get_model plus tests/navfloor_ref.py; the
    device's result is compared with it with ==;
  * the older calls through this library and, with --other-lib, through another build of libssf_hip_mem.so (the parent commit's):
    nav_grid and nav_plan on the carved 512 x 512 grid of the synthetic map, alternating this / other / this / other in one process.
Prints a table and JSON lines; --out also writes them to a file.  No threshold is asserted: the table is the record.

    python tools/navfloor_probe.py [--rows 1000000] [--reps 20] [--other-lib PATH] [--out FILE]"""
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
from supersurfel_fusion_amd import binding, replay, synthetic  # noqa: E402
import navfloor_ref as fr  # noqa: E402
import navlive_probe as lp  # noqa: E402

WARM, N, W, H = lp.WARM, lp.N, lp.W, lp.H
KERNELS = ("navfloor_prep", "navfloor_direction", "navfloor_height", "navfloor_refine")
spread = lp.spread


def timed(f, call, reps):
    """(wall clocks in ms with profile off, per-kernel ms under profile = 1 as reps x kernels, the last call's result)"""
    f.set_profile(1)
    per = []
    for k in range(WARM + reps):
        f.reset_kernel_times()
        got = call()
        kt = f.kernel_times()
        if k >= WARM:
            per.append([kt.get(nm, (0.0, 0))[0] for nm in KERNELS])
    f.set_profile(0)
    wall = []
    for k in range(WARM + reps):
        t0 = time.perf_counter()
        got = call()
        if k >= WARM:
            wall.append(1e3 * (time.perf_counter() - t0))
    return wall, np.array(per), got


def older_calls(f, state, dist2, bands, torch, dev, reps):
    """the wall clocks in ms of nav_grid (512 x 512 at 0.05 m, device outputs) and of nav_plan (tools/navplan_probe.py's scene)"""
    s2, d2 = torch.zeros((N, N), dtype=torch.int8, device=dev), torch.zeros((N, N), dtype=torch.int32, device=dev)
    grid = []
    for k in range(WARM + reps):
        t0 = time.perf_counter()
        f.nav_grid_device(state=s2, dist2=d2, width=N, height=N, res=0.05, **bands)
        if k >= WARM:
            grid.append(1e3 * (time.perf_counter() - t0))
    plan, _ = lp.plan_wall(f, state, dist2, torch, dev, reps)
    return grid, plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--other-lib", default=None, help="another build of libssf_hip_mem.so: nav_grid and nav_plan are timed through it as well")
    ap.add_argument("--out", default=None, help="also append the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_floor()
    K = synthetic.intrinsics(W, H)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    dev = torch.device("cuda")
    f = binding.Fusion(lib, lib.default_config(**cam, nb_supersurfels_max=a.rows + 4096))
    state, dist2, gs, bands, _ = lp.carved_grid(f, a.rows, torch, dev)
    g = binding.Fusion(lib, lib.default_config(**dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000)))
    replay.replay(g, replay.frames_from_npz(os.path.join(ROOT, "tests", "golden", "tum_fr1_xyz_8frames.npz")))
    say("%d calls per figure after %d warm-ups; times in ms: median (smallest .. largest)" % (a.reps, WARM))
    for label, h, kw in (("synthetic %d rows" % a.rows, f, dict()), ("fr1_xyz 8 frames", g, dict())):
        cnt = h.counts()
        t0 = time.perf_counter()
        model = h.get_model()
        t_copy = 1e3 * (time.perf_counter() - t0)
        say("[%s] %d rows, %d visible; get_model %.2f ms (%.1f MB)" % (label, cnt["n_model"], cnt["n_visible"], t_copy, 104e-6 * cnt["n_model"]))
        rec = dict(map=label, rows=cnt["n_model"], get_model_ms=round(t_copy, 3))
        for iters in (3, 0):
            call = lambda: h.nav_floor(histograms=False, refine_iters=iters, **kw)
            wall, per, got = timed(h, call, a.reps)
            ksum = float(np.median(per, axis=0).sum())
            w = float(np.median(wall))
            say("[%s] refine_iters %d: status %s, %d candidates of %d rows, inliers %s, camera_height %.3f m, rms %s mm" %
                (label, iters, got["status_name"], got["candidates"], got["rows_used"], got["inliers"][:max(got["rounds"], 1)], float(got["camera_height"]),
                 ["%.2f" % (1e3 * float(v)) for v in got["rms"][:got["rounds"]]]))
            say("[%s] refine_iters %d: wall %s | kernels: %s | summed %.4f | not kernel time (%d waits, their copies, the host steps): %.4f = %.0f %% of the wall" %
                (label, iters, spread(wall), "  ".join("%s %s" % (k, spread(per[:, i])) for i, k in enumerate(KERNELS)), ksum, 3 + got["rounds"], w - ksum,
                 100.0 * (w - ksum) / w))
            rec["iters_%d" % iters] = dict(wall_ms=[round(float(x), 4) for x in (np.median(wall), np.min(wall), np.max(wall))],
                                           kernel_ms={k: round(float(np.median(per[:, i])), 4) for i, k in enumerate(KERNELS)}, status=got["status_name"],
                                           candidates=got["candidates"], not_kernel_ms=round(w - ksum, 4))
        # the host route: the copy above, then the restatement
        t0 = time.perf_counter()
        want = fr.fit(model, cnt["n_visible"], h.get_pose()[9:], fr.params(**kw))
        t_ref = 1e3 * (time.perf_counter() - t0)
        got = h.nav_floor(**kw)
        try:
            fr.same_fit(got, want, label)
            equal = True
        except AssertionError as e:
            equal = False
            say("[%s] DIFFERS: %s" % (label, str(e)[:300]))
        say("[%s] the host route (a statement of the rule, not a tuned implementation): get_model %.2f ms + the restatement (numpy) %.0f ms; every integer and "
            "float equal with ==: %s" % (label, t_copy, t_ref, equal))
        rec.update(host_reference_ms=round(t_ref, 1), equal=equal)
        say(json.dumps(rec))
    g.close()
    # the older calls: this library and the other in turn
    rec = {}
    if a.other_lib:
        other = binding.Library(a.other_lib)
        o = binding.Fusion(other, other.default_config(**cam, nb_supersurfels_max=a.rows + 4096))
        s2, d2, gs2, _, _ = lp.carved_grid(o, a.rows, torch, dev)
        same = bool(np.array_equal(s2.cpu().numpy(), state.cpu().numpy()) and np.array_equal(d2.cpu().numpy(), dist2.cpu().numpy()))
        say("[older calls] the other library is %s; the same carved grid: %s" % (os.path.relpath(a.other_lib, ROOT), same))
        for turn in range(2):
            for who, h_, s_, d_ in (("this", f, state, dist2), ("other", o, s2, d2)):
                grid, plan = older_calls(h_, s_, d_, bands, torch, dev, a.reps)
                say("[older calls] turn %d, %s library: nav_grid wall %s ms; nav_plan wall %s ms" % (turn + 1, who, spread(grid), spread(plan)))
                rec["%s_%d" % (who, turn + 1)] = dict(nav_grid_ms=round(float(np.median(grid)), 4), nav_plan_ms=round(float(np.median(plan)), 3))
        o.close()
    else:
        grid, plan = older_calls(f, state, dist2, bands, torch, dev, a.reps)
        say("[older calls] this library: nav_grid wall %s ms; nav_plan wall %s ms" % (spread(grid), spread(plan)))
        rec["this_1"] = dict(nav_grid_ms=round(float(np.median(grid)), 4), nav_plan_ms=round(float(np.median(plan)), 3))
    f.close()
    say(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
