"""Dense RGB-D odometry (include/ssf_odometry.h): what it costs on the MI355X and how close it gets on a CPU.

    python tools/odometry_probe.py --accuracy [--out profiles/odometry.txt]      # no GPU: the numpy restatement (tests/odometry_ref.py)
    python tools/odometry_probe.py [--reps 20] [--out FILE]                      # one MI355X

--accuracy runs the restatement with the default parameters on the pairs the CPU tests use -- synthetic.render at orbit_pose(k) ->
orbit_pose(k + 1), k = 0 .. 11, 160 x 128, without and with noise; the seven consecutive pairs of the eight committed fr1_xyz
frames against tests/golden/fr1_xyz_gt.txt -- and prints, per pair, the translation and rotation error of the estimate next to the
identity's.  tests/test_odometry.py asserts twice these errors.  With --sequence DIR (a TUM directory with associations_with_gt.txt,
e.g. fr3_walking_halfsphere) the same figures are printed for its first --pairs consecutive pairs.

Without --accuracy, at 640 x 480 on the committed fr1_xyz frames with the defaults: us per pyramid build (odo_pyramid: every launch
of one frame's pyramid in one bracket), us per k_odo_linearise per level (ssf_odometry_linearise repeated, profile = 1 brackets),
iterations taken, ms per ssf_odometry_track (wall clock, host frames), next to the frame it precedes: process_frame without a
prior and with the odometry prior, in the same run.  Warm-up, then the median of --reps runs with the spread (min .. max).  No
time is gated.  For a kernel trace run it under rocprofv3 --kernel-trace --stats; for counters, a run of its own."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import odometry_ref as orf  # noqa: E402
from supersurfel_fusion_amd import binding, replay, synthetic  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
TUM = os.path.join(GOLD, "tum_fr1_xyz_8frames.npz")
ORACLE_LIB = os.path.join(ROOT, "oracle", "_build", "libssf_oracle.so")
FR1_K = (525.0, 525.0, 319.5, 239.5)
SYNTH_SHAPE = (160, 128)


def synthetic_pair(k, noise, W=SYNTH_SHAPE[0], H=SYNTH_SHAPE[1]):
    """(reference pyramid, current pyramid, true rel) of orbit_pose(k) -> orbit_pose(k + 1)"""
    K = synthetic.intrinsics(W, H)
    pyr = []
    for j in (k, k + 1):
        R, t = synthetic.orbit_pose(j)
        rgb, depth, _ = synthetic.render(R, t, W, H, noise=noise, rng=np.random.default_rng(1000 + j))
        pyr.append(orf.pyramid(rgb, depth, (K["fx"], K["fy"], K["cx"], K["cy"])))
    return pyr[0], pyr[1], orf.true_rel(synthetic.orbit_pose(k), synthetic.orbit_pose(k + 1))


def fr1_pairs():
    """[(reference pyramid, current pyramid, true rel)] of the seven consecutive pairs of the committed fr1_xyz frames"""
    frames = list(replay.frames_from_npz(TUM))
    stamps, xyz, quat = replay.read_trajectory(os.path.join(GOLD, "fr1_xyz_gt.txt"))
    assert [f[0] for f in frames] == list(stamps[:len(frames)])
    pyr = [orf.pyramid(rgb, depth, FR1_K) for _, rgb, depth in frames]
    poses = [(orf.quat_to_R(quat[i]), np.asarray(xyz[i], np.float64)) for i in range(len(frames))]
    return [(pyr[i], pyr[i + 1], orf.true_rel(poses[i], poses[i + 1])) for i in range(len(frames) - 1)]


def measure(pair, oracle, p=None):
    ref, cur, true = pair
    rel, res = orf.estimate(ref, cur, p or orf.params(), oracle)
    return dict(result=res, err=orf.errors(rel, true), identity=orf.errors(orf.IDENTITY12, true))


def accuracy_line(name, m):
    return "  %-22s valid %d %-14s iters %-14s t %.5f m (identity %.5f)  angle %.5f rad (identity %.5f)  closer: t %s angle %s" % (
        name, m["result"]["valid"], m["result"]["reason"], m["result"]["iters"][:m["result"]["levels"]], m["err"][0], m["identity"][0],
        m["err"][1], m["identity"][1], m["err"][0] < m["identity"][0], m["err"][1] < m["identity"][1])


def sequence_pairs(seq_dir, n):
    ent = replay.read_associations(os.path.join(seq_dir, "associations_with_gt.txt"), max_frames=n + 1)
    frames = list(replay.frames_from_dataset(seq_dir, max_frames=n + 1))
    pyr = [orf.pyramid(rgb, depth, FR1_K) for _, rgb, depth in frames]
    poses = [(orf.quat_to_R(e["gt"][1]), np.asarray(e["gt"][0], np.float64)) for e in ent]
    return [(pyr[i], pyr[i + 1], orf.true_rel(poses[i], poses[i + 1])) for i in range(len(frames) - 1)]


def accuracy(a):
    oracle = binding.Library(ORACLE_LIB)
    lines = ["# tools/odometry_probe.py --accuracy: the numpy restatement (tests/odometry_ref.py) with the default parameters, on a CPU.",
             "# error of rel against the true relative motion: translation |t - t_true| and the angle of R^T R_true; 'identity' = the same",
             "# for rel = identity, i.e. what tracking from the previous pose starts from.  Deterministic.",
             "synthetic.render at orbit_pose(k) -> orbit_pose(k + 1), %d x %d" % SYNTH_SHAPE]
    for noise in (False, True):
        for k in range(12):
            lines.append(accuracy_line("k = %d%s" % (k, ", noise" if noise else ""), measure(synthetic_pair(k, noise), oracle)))
    lines.append("tum_fr1_xyz_8frames against fr1_xyz_gt.txt, 640 x 480")
    for i, pair in enumerate(fr1_pairs()):
        lines.append(accuracy_line("frames %d -> %d" % (i, i + 1), measure(pair, oracle)))
    if a.sequence:
        lines.append("%s, first %d pairs" % (os.path.basename(os.path.normpath(a.sequence)), a.pairs))
        for i, pair in enumerate(sequence_pairs(a.sequence, a.pairs)):
            lines.append(accuracy_line("frames %d -> %d" % (i, i + 1), measure(pair, oracle)))
    return lines


def spread(us):
    return "%.1f (min %.1f .. max %.1f, %d runs)" % (float(np.median(us)), min(us), max(us), len(us))


def wall(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e6 * (time.perf_counter() - t0))
    return t


def kernel_runs(f, fn, reps, name, warm=3):
    """us per launch bracket of `name`, one figure per run of fn"""
    f.set_profile(1)
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        f.reset_kernel_times()
        fn()
        kt = f.kernel_times()
        out.append(1e3 * kt[name][0] / max(kt[name][1], 1))
    f.set_profile(0)
    return out


def timings(a):
    lib = binding.load_product()
    frames = list(replay.frames_from_npz(TUM))
    cfg = dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000)
    f = binding.Fusion(lib, lib.default_config(**cfg))
    (_, rgb0, d0), (_, rgb1, d1) = frames[0], frames[1]
    lines = ["# tools/odometry_probe.py --reps %d, one MI355X, one session, %d x %d, the committed fr1_xyz frames, default parameters." % (a.reps, f.W, f.H),
             "# Kernel times: profile = 1 event brackets (each bracket carries a few us of its own).  median (min .. max).  No time is gated."]
    lines.append("odo_pyramid (one frame's pyramid, every launch in one bracket), us: " + spread(kernel_runs(f, lambda: f.odometry_set_reference(rgb0, d0), a.reps, "odo_pyramid")))
    rel, res = f.odometry_estimate(rgb1, d1)
    lines.append("ssf_odometry_estimate frames 0 -> 1: %s" % res)
    T = orf.to12(orf.invert(orf.from12(rel)))                      # reference camera -> current camera, where the loop ended
    for l in range(res["levels"]):
        lv = f.odometry_pyramid(0, l)["I"].shape
        lines.append("k_odo_linearise level %d (%d x %d), us: %s" % (l, lv[1], lv[0], spread(kernel_runs(f, lambda: f.odometry_linearise(l, T), a.reps, "odo_linearise"))))

    def track():
        f.odometry_set_reference(rgb0, d0)
        return f.odometry_track(rgb1, d1)
    t_ref = wall(lambda: f.odometry_set_reference(rgb0, d0), a.reps)
    t_both = wall(track, a.reps)
    lines.append("ssf_odometry_set_reference (host frame), us wall clock: " + spread(t_ref))
    lines.append("ssf_odometry_set_reference + ssf_odometry_track (host frames), us wall clock: " + spread(t_both))
    lines.append("ssf_odometry_track alone = the difference of the medians: %.3f ms" % (1e-3 * (np.median(t_both) - np.median(t_ref))))
    f.close()
    # the frame the track precedes: frame 3 on the map of frames 0-2, fresh handles; without a prior and with the odometry prior
    for mode in ("process_frame, no prior", "process_frame(odometry=True): track + the frame with its prior"):
        t, iters = [], []
        for _ in range(max(3, a.reps // 4) + 1):
            g = binding.Fusion(lib, lib.default_config(**cfg))
            kw = dict(odometry=True) if "odometry" in mode else {}
            for _, rgb, depth in frames[:3]:
                g.process_frame(rgb, depth, **kw)
            t0 = time.perf_counter()
            r = g.process_frame(frames[3][1], frames[3][2], **kw)
            t.append(1e6 * (time.perf_counter() - t0))
            iters.append(r["icp_iters"])
            g.close()
        lines.append("%s, us wall clock: %s ; icp_iters %s" % (mode, spread(t[1:]), iters[1:]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accuracy", action="store_true", help="the CPU accuracy figures of the restatement (no GPU)")
    ap.add_argument("--sequence", default=None, metavar="DIR", help="with --accuracy: a TUM sequence directory to add")
    ap.add_argument("--pairs", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the lines to this file")
    a = ap.parse_args()
    text = "\n".join(accuracy(a) if a.accuracy else timings(a)) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
