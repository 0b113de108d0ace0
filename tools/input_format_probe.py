"""Raw sensor frames against converted ones (include/ssf_input.h), host frames through ssf_process_sequence.

Three forms of the same 720 host frames (the 8 real fr1_xyz frames, cycled back and forth), pipeline depth 2 x 8 frames per
launch, depth pre-filter off and on:
  1  float32 metres + RGB8 host frames, converted before the timed region (what the library took until now)
  2  the caller converts every frame on the host inside the timed region (BGR -> RGB, u16 -> float metres; the reference
     node's cvtColor + convertTo), then form 1
  3  BGR8 + uint16 host frames handed over as they are (set_input_format("bgr8", "u16", 0.0002))
A fresh handle per run (warm-up sequence first); forms alternate, `--reps` rounds.  Prints frames/s and the upload workers'
counters (ssf_upload_stats) per run and a JSON line per run.

    python tools/input_format_probe.py [--frames 720] [--reps 2] [--forms 1,2,3] [--prefilter 0,1]

For kernel times run it under rocprofv3 --kernel-trace --stats with --forms 1,3: the instantiations of k_ingest /
k_bilateral_r7 name the formats they read (k_ingest<colour, depth>, k_bilateral_r7<waves, depth>)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from supersurfel_fusion_amd import binding, replay  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
SCALE = 0.0002
WARMUP = 24


def upload_stats(lib, f):
    st = (C.c_double * 6)()
    lib.lib.ssf_upload_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.lib.ssf_upload_stats(f.h, st)
    return list(st)


def run(lib, form, prefilter, order, rgb, d16, f32, bgr):
    cfg = dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=100000, pipeline_depth=2, extract_batch=8, depth_prefilter=prefilter)
    f = binding.Fusion(lib, lib.default_config(**cfg))
    if form == 3:
        f.set_input_format("bgr8", "u16", SCALE)
        frames = [(bgr[k], d16[k]) for k in order]
    elif form == 1:
        frames = [(rgb[k], f32[k]) for k in order]
    else:
        frames = [(bgr[k], d16[k]) for k in order]
    warm, timed = frames[:WARMUP], frames[WARMUP:]
    if form == 2:
        warm = [(np.ascontiguousarray(c[..., ::-1]), replay.convert_depth(d, SCALE)) for c, d in warm]
    rp, dp, keep = f.host_sequence([c for c, _ in warm], [d for _, d in warm])
    f.process_sequence(rp, dp, on_device=False)
    s0 = upload_stats(lib, f)
    t0 = time.perf_counter()
    if form == 2:                                 # the node's per-frame conversion, then the float RGB sequence
        timed = [(np.ascontiguousarray(c[..., ::-1]), replay.convert_depth(d, SCALE)) for c, d in timed]
        t_conv = time.perf_counter() - t0
    else:
        t_conv = 0.0
    rp, dp, keep = f.host_sequence([c for c, _ in timed], [d for _, d in timed])
    res = f.process_sequence(rp, dp, on_device=False)
    dt = time.perf_counter() - t0
    s1 = upload_stats(lib, f)
    n = len(timed)
    nfr = max(s1[1] - s0[1], 1.0)
    out = dict(form=form, prefilter=prefilter, frames=n, frames_per_sec=round(n / dt, 1), us_per_frame=round(1e6 * dt / n, 2),
               host_conversion_us_per_frame=round(1e6 * t_conv / n, 2),
               bytes_per_frame=int(keep[0][0].nbytes + keep[0][1].nbytes),
               upload_workers=int(s1[0]), uploaded_frames=int(s1[1] - s0[1]),
               upload_us_per_frame=dict(ring_wait=round((s1[2] - s0[2]) / nfr, 1), staging_memcpy=round((s1[3] - s0[3]) / nfr, 1),
                                        enqueue=round((s1[4] - s0[4]) / nfr, 1), caller_wait=round((s1[5] - s0[5]) / n, 1)),
               last_n_model=res[-1]["n_model"])
    f.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=720)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--forms", default="1,2,3")
    ap.add_argument("--prefilter", default="0,1")
    a = ap.parse_args()
    lib = binding.load_product()
    z = list(replay.frames_from_npz(os.path.join(GOLD, "tum_fr1_xyz_8frames.npz"), SCALE, raw=True))
    rgb = [np.ascontiguousarray(c) for _, c, _ in z]
    d16 = [np.ascontiguousarray(d) for _, _, d in z]
    f32 = [replay.convert_depth(d, SCALE) for d in d16]
    bgr = [np.ascontiguousarray(c[..., ::-1]) for c in rgb]
    m = len(z)
    period = 2 * m - 2
    order = [(i % period) if (i % period) < m else period - (i % period) for i in range(WARMUP + a.frames)]
    forms = [int(x) for x in a.forms.split(",")]
    results = []
    for rep in range(a.reps):
        for pf in [int(x) for x in a.prefilter.split(",")]:
            for form in forms:
                r = run(lib, form, pf, order, rgb, d16, f32, bgr)
                r["rep"] = rep
                results.append(r)
                u = r["upload_us_per_frame"]
                print("rep %d prefilter %d form %d: %8.1f frames/s  %7.2f us/frame (host conversion %6.2f)  %7d B/frame  upload per frame: "
                      "staging memcpy %6.1f us, enqueue %5.1f us, ring wait %6.1f us, caller wait %5.1f us" %
                      (rep, pf, form, r["frames_per_sec"], r["us_per_frame"], r["host_conversion_us_per_frame"], r["bytes_per_frame"],
                       u["staging_memcpy"], u["enqueue"], u["ring_wait"], u["caller_wait"]), flush=True)
                print("JSON " + json.dumps(r), flush=True)
    for pf in [int(x) for x in a.prefilter.split(",")]:
        for form in forms:
            v = [r["frames_per_sec"] for r in results if r["prefilter"] == pf and r["form"] == form]
            print("prefilter %d form %d: frames/s %s  mean %.1f" % (pf, form, " ".join("%.1f" % x for x in v), sum(v) / len(v)))


if __name__ == "__main__":
    main()
