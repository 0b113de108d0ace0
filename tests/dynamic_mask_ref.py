"""The pixel-mask vote of include/ssf_dynamic.h in numpy, and the checker driven by it.

The checker library takes no pixel mask, and needs none: extraction depends on earlier frames only through the frame counter
(the RANSAC epoch), so a handle E that only extracts (stage_extract) sees every frame's final label map exactly as a handle T that
processes the same frames does.  The vote of E's label map and the pixel mask is then T's S-byte dynamic_mask (ssf.h)."""
import numpy as np

from supersurfel_fusion_amd import binding


def vote(label, pixel_mask, S):
    """S bytes, 1 = dynamic: masked > 0 and 2 * masked >= total, over the pixels of each label (integer counts)"""
    lab = np.asarray(label).ravel()
    hit = np.asarray(pixel_mask).ravel() != 0
    total = np.bincount(lab, minlength=S)[:S].astype(np.int64)
    masked = np.bincount(lab[hit], minlength=S)[:S].astype(np.int64)
    return ((masked > 0) & (2 * masked >= total)).astype(np.uint8)


def checker_run(lib, cfg, frames, masks):
    """frames [(rgb, depth)], masks [H x W or None]: returns (T, [result dicts], [vote or None]) -- T processed every frame with
    the vote of E's label map as its dynamic_mask"""
    E, T = binding.Fusion(lib, cfg), binding.Fusion(lib, cfg)
    results, votes = [], []
    for (rgb, depth), m in zip(frames, masks):
        E.stage_extract(rgb, depth)
        v = None if m is None else vote(E.index_map(), m, E.S)
        results.append(T.process_frame(rgb, depth, dynamic_mask=v))
        votes.append(v)
    return T, results, votes
