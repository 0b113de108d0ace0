"""Per-pixel dynamic-object masks (include/ssf_dynamic.h), voted onto the frame's superpixels by k_render_moments<., true> and
k_finalize_surfels<true>.  The checker takes no pixel mask; it is driven the way the header defines the vote (dynamic_mask_ref):
handle E only extracts and yields the final label map, the numpy vote of that map and the pixel mask becomes the S-byte
dynamic_mask of ssf.h for handle T.  The product must equal T bit for bit -- results, maps, frame supersurfels, model rows -- and
its own vote (dynamic_superpixels) must equal the numpy vote of its own index map."""
import os

import numpy as np
import pytest

import util
from dynamic_mask_ref import checker_run, vote
from supersurfel_fusion_amd import binding, replay

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ERR_INVALID_ARG, ERR_STATE = -1, -5


def rect_mask(W, H, x0, y0, x1, y1):
    m = np.zeros((H, W), np.uint8)
    m[int(y0 * H):int(y1 * H), int(x0 * W):int(x1 * W)] = 255
    return m


def disc_mask(W, H, cx, cy, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((xx - cx * W) ** 2 + (yy - cy * H) ** 2) <= (r * W) ** 2).astype(np.uint8)


def random_mask(W, H, seed, p=0.3):
    return (np.random.default_rng(seed).random((H, W)) < p).astype(np.uint8) * np.uint8(7)


def masks_for(W, H, n):
    """a rectangle, a disc, random pixels, no mask, in turn"""
    kinds = [lambda k: rect_mask(W, H, 0.2, 0.1, 0.6, 0.7), lambda k: disc_mask(W, H, 0.6, 0.5, 0.2),
             lambda k: random_mask(W, H, k), lambda k: None]
    return [kinds[k % 4](k) for k in range(n)]


def to_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def check_vote(f, pixel_mask):
    """the product's vote equals the numpy vote of its own index map (all 0 without a mask)"""
    got, n = f.dynamic_superpixels()
    want = np.zeros(f.S, np.uint8) if pixel_mask is None else vote(f.index_map(), pixel_mask, f.S)
    util.assert_same_bits(got, want, "dynamic superpixels")
    assert n == int(want.sum())
    return got


@pytest.mark.parametrize("W,H", [(320, 240), (640, 480)])
def test_one_frame_in_flight_against_the_checker(W, H, oracle_lib, product_lib):
    n = 4 if W == 320 else 2
    frames = [util.frame(k, W, H, noise=True) for k in range(n)]
    masks = masks_for(W, H, n)
    kw = dict(nb_supersurfels_max=40000)
    T, want, votes = checker_run(oracle_lib, util.make_cfg(oracle_lib, W, H, **kw), frames, masks)
    fx = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H, **kw))
    for (rgb, depth), m, v in zip(frames, masks, votes):
        util.same_result(fx.process_frame(rgb, depth, pixel_mask=m), want.pop(0))
        got = check_vote(fx, m)
        if v is not None:
            util.assert_same_bits(got, v, "vote against the checker's label map")
    util.compare_state(T, fx)


@pytest.mark.parametrize("on_device", [False, True])
def test_pipelined_batches_mix_masked_and_unmasked_frames(on_device, oracle_lib, product_lib):
    """depth 2 x 8 frames per launch, 20 frames: batch 1 mixes masked and unmasked frames, batch 2 has no mask at all"""
    W, H, nf = 320, 240, 20
    frames = [util.frame(k, W, H, noise=True) for k in range(nf)]
    masks = masks_for(W, H, 8) + [None] * 8 + masks_for(W, H, 4)
    T, want, _ = checker_run(oracle_lib, util.make_cfg(oracle_lib, W, H), frames, masks)
    fx = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H, pipeline_depth=2, extract_batch=8))
    inputs = frames
    if on_device:
        inputs = [(to_device(c), to_device(d)) for c, d in frames]
        dmasks = [None if m is None else to_device(m) for m in masks]
    got, nsub = [], 0
    for k in range(nf):
        while nsub < nf and fx.can_submit():
            c, d = inputs[nsub]
            if on_device:
                fx.submit_frame(c.data_ptr(), d.data_ptr(), on_device=True,
                                pixel_mask=None if dmasks[nsub] is None else dmasks[nsub].data_ptr())
            else:
                fx.submit_frame(c, d, pixel_mask=masks[nsub])
            nsub += 1
        got.append(fx.process_submitted().as_dict())
        check_vote(fx, masks[k])
    for a, b in zip(want, got):
        util.same_result(a, b)
    util.compare_state(T, fx)


@pytest.mark.parametrize("on_device", [False, True])
def test_sequence_with_masks(on_device, oracle_lib, product_lib):
    """ssf_process_sequence_pixmask: host frames through the upload ring, or device frames; some entries NULL"""
    W, H, n = 320, 240, 24
    frames = [util.frame(k, W, H, noise=True) for k in range(n)]
    masks = masks_for(W, H, n)
    T, want, _ = checker_run(oracle_lib, util.make_cfg(oracle_lib, W, H), frames, masks)
    fx = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H, pipeline_depth=2, extract_batch=8))
    if on_device:
        dev = [(to_device(c), to_device(d)) for c, d in frames]
        dm = [None if m is None else to_device(m) for m in masks]
        got = fx.process_sequence([c.data_ptr() for c, _ in dev], [d.data_ptr() for _, d in dev], on_device=True,
                                  mask_ptrs=[None if m is None else m.data_ptr() for m in dm])
    else:
        rp, dp, keep = fx.host_sequence([f[0] for f in frames], [f[1] for f in frames])
        mp, keep_m = fx.host_masks(masks)
        got = fx.process_sequence(rp, dp, on_device=False, mask_ptrs=mp)
    assert len(got) == n
    for a, b in zip(want, got):
        util.same_result(a, b)
    check_vote(fx, masks[-1])
    util.compare_state(T, fx)


def test_stage_extract_with_a_mask(oracle_lib, product_lib):
    W, H = 320, 240
    rgb, depth = util.frame(3, W, H, noise=True)
    m = disc_mask(W, H, 0.4, 0.5, 0.25)
    fo = binding.Fusion(oracle_lib, util.make_cfg(oracle_lib, W, H))
    fo.stage_extract(rgb, depth)
    v = vote(fo.index_map(), m, fo.S)
    fo2 = binding.Fusion(oracle_lib, util.make_cfg(oracle_lib, W, H))
    fo2.stage_extract(rgb, depth, dynamic_mask=v)
    fx = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    fx.stage_extract(rgb, depth, pixel_mask=m)
    util.assert_same_bits(check_vote(fx, m), v, "vote")
    assert v.sum() > 0
    util.compare_state(fo2, fx)
    c, d, dmask = to_device(rgb), to_device(depth), to_device(m)
    fx.stage_extract(c.data_ptr(), d.data_ptr(), on_device=True, pixel_mask=dmask.data_ptr())
    fo2.stage_extract(rgb, depth, dynamic_mask=vote(fo2.index_map(), m, fo2.S))
    check_vote(fx, m)
    util.compare_state(fo2, fx)


def test_raw_frames_with_a_mask(oracle_lib, product_lib):
    """BGR8 + u16 frames and a pixel mask in the same call"""
    W, H, n, scale = 320, 240, 3, 0.0002
    frames, raw = [], []
    for k in range(n):
        rgb, depth = util.frame(k, W, H, noise=True)
        d16 = np.clip(np.rint(np.asarray(depth, np.float64) / scale), 0, 65535).astype(np.uint16)
        frames.append((rgb, replay.convert_depth(d16, scale)))
        raw.append((np.ascontiguousarray(rgb[..., ::-1]), d16))
    masks = [rect_mask(W, H, 0.3, 0.2, 0.7, 0.6)] * n
    T, want, _ = checker_run(oracle_lib, util.make_cfg(oracle_lib, W, H), frames, masks)
    fx = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    fx.set_input_format("bgr8", "u16", scale)
    for (c, d), m, w in zip(raw, masks, want):
        util.same_result(fx.process_frame(c, d, pixel_mask=m), w)
        check_vote(fx, m)
    util.compare_state(T, fx)


def test_fr3_walking_with_a_box_mask(oracle_lib, product_lib):
    """the committed fr3_walking frames with a fixed box over the middle of the image (where the walkers are)"""
    path = os.path.join(GOLD, "tum_fr3_walking_4frames.npz")
    frames = [(c, d) for _, c, d in replay.frames_from_npz(path)]
    H, W = frames[0][1].shape
    masks = [rect_mask(W, H, 0.35, 0.1, 0.75, 0.95)] * len(frames)
    cfg = dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000, **replay.FR3_INTRINSICS)
    T, want, votes = checker_run(oracle_lib, oracle_lib.default_config(**cfg), frames, masks)
    fx = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    for (c, d), m, w, v in zip(frames, masks, want, votes):
        util.same_result(fx.process_frame(c, d, pixel_mask=m), w)
        util.assert_same_bits(check_vote(fx, m), v, "vote")
        assert v.sum() > 0
    util.compare_state(T, fx)


def test_an_all_zero_mask_is_no_mask(product_lib):
    W, H, n = 320, 240, 4
    fa = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    fb = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    zero = np.zeros((H, W), np.uint8)
    for k in range(n):
        rgb, depth = util.frame(k, W, H, noise=True)
        util.same_result(fa.process_frame(rgb, depth), fb.process_frame(rgb, depth, pixel_mask=zero))
        assert fb.dynamic_superpixels()[1] == 0
    util.compare_state(fa, fb)


def test_an_all_ones_mask(oracle_lib, product_lib):
    """first frame: no valid supersurfel enters the model (the reference copies the whole first frame into the model,
    supersurfel_fusion.cu:477-483, so its rows are there, every one with confidence -1, and the next frame removes them).
    A later frame: ICP is invalid and no model row is updated or inserted; the classification and reorder of the model still
    run (as the checker's)"""
    W, H = 320, 240
    ones = np.ones((H, W), np.uint8)
    frames = [util.frame(k, W, H, noise=True) for k in range(4)]
    T0, want0, _ = checker_run(oracle_lib, util.make_cfg(oracle_lib, W, H), frames[:2], [ones, None])
    fx = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    r = fx.process_frame(*frames[0], pixel_mask=ones)
    util.same_result(r, want0[0])
    assert r["n_inserted"] == 0 and not (fx.get_model()["confidences"] > 0).any()
    assert fx.dynamic_superpixels()[1] == int((np.bincount(fx.index_map().ravel(), minlength=fx.S) > 0).sum())
    r = fx.process_frame(*frames[1])
    util.same_result(r, want0[1])
    assert r["n_removed"] == want0[0]["n_model"]
    util.compare_state(T0, fx)
    masks = [None, None, ones, None]
    T, want, _ = checker_run(oracle_lib, util.make_cfg(oracle_lib, W, H), frames, masks)
    fy = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    got = [fy.process_frame(c, d, pixel_mask=m) for (c, d), m in zip(frames, masks)]
    for a, b in zip(want, got):
        util.same_result(a, b)
    assert got[2]["icp_valid"] == 0 and got[2]["n_updated"] == 0 and got[2]["n_inserted"] == 0
    assert got[2]["stamp"] == got[1]["stamp"] + 1
    util.compare_state(T, fy)


def test_misuse(oracle_lib, product_lib):
    W, H = 160, 128
    f = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H, pipeline_depth=1, extract_batch=2))
    L = product_lib.lib
    rgb, depth = util.frame(0, W, H)
    m = np.zeros((H, W), np.uint8)
    c, d, mp = binding._ptr(rgb), binding._ptr(depth), binding._ptr(m)
    res = binding.SsfFrameResult()
    assert L.ssf_process_frame_pixmask(None, c, d, 0, None, mp, binding.C.byref(res)) == ERR_INVALID_ARG
    assert L.ssf_process_frame_pixmask(f.h, None, d, 0, None, mp, binding.C.byref(res)) == ERR_INVALID_ARG
    assert L.ssf_process_frame_pixmask(f.h, c, None, 0, None, mp, binding.C.byref(res)) == ERR_INVALID_ARG
    assert L.ssf_submit_frame_pixmask(f.h, None, d, 0, mp) == ERR_INVALID_ARG
    assert L.ssf_stage_extract_pixmask(f.h, c, None, 0, mp) == ERR_INVALID_ARG
    arr = (binding.C.c_void_p * 1)(None)
    assert L.ssf_process_sequence_pixmask(f.h, arr, arr, None, 1, 0, None) == ERR_INVALID_ARG
    assert L.ssf_get_dynamic_superpixels(None, mp, None) == ERR_INVALID_ARG
    assert L.ssf_get_dynamic_superpixels(f.h, None, None) == ERR_INVALID_ARG
    # a full pipeline: (1 + 1) x 2 frames pending
    for _ in range(f.pipeline_capacity()):
        assert L.ssf_submit_frame_pixmask(f.h, c, d, 0, mp) == 0
    assert L.ssf_submit_frame_pixmask(f.h, c, d, 0, mp) == ERR_STATE
    assert L.ssf_process_frame_pixmask(f.h, c, d, 0, None, mp, binding.C.byref(res)) == ERR_STATE
    assert L.ssf_stage_extract_pixmask(f.h, c, d, 0, mp) == ERR_STATE
    while f.pending_frames():
        f.process_submitted()
    # the binding refuses masks it would have to cast, and the pair of mask kinds
    with pytest.raises(binding.SsfError, match="pixel mask must be uint8"):
        f.process_frame(rgb, depth, pixel_mask=np.zeros((H, W), np.float32))
    with pytest.raises(binding.SsfError, match="pixel mask must be uint8"):
        f.process_frame(rgb, depth, pixel_mask=np.zeros((W, H), np.uint8))
    with pytest.raises(binding.SsfError, match="do not combine"):
        f.process_frame(rgb, depth, pixel_mask=m, dynamic_mask=np.zeros(f.S, np.uint8))
    # the checker library: the binding names the missing symbol
    fo = binding.Fusion(oracle_lib, util.make_cfg(oracle_lib, W, H))
    with pytest.raises(binding.SsfError, match="ssf_process_frame_pixmask"):
        fo.process_frame(rgb, depth, pixel_mask=m)
    with pytest.raises(binding.SsfError, match="ssf_get_dynamic_superpixels"):
        fo.dynamic_superpixels()
