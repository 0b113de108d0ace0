"""Dense RGB-D odometry (include/ssf_odometry.h) on the MI355X against the numpy restatement (tests/odometry_ref.py): every level of
the pyramid, the 29 integers of the normal equations, the coarse-to-fine estimate and its result at 0 bits; masks, device inputs,
the frame path with the prior, no side effects, the refusals and the profiling names.  The shapes are the smallest at which the
kernels can still go wrong: 64 x 48 (2 levels), 100 x 60 (3 levels: 25 x 15 is odd and no width is a multiple of 64), 160 x 128
(3 levels)."""
import functools

import numpy as np
import pytest

import odometry_ref as orf
import util
from odometry_cases import K4, transforms, true_rel12             # (shared with tests/test_odometry_edges_gpu.py and the CPU conditions)
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
SHAPES = [(64, 48, 2), (100, 60, 3), (160, 128, 3)]
f32 = np.float32
HOLES = 0.25


def handle(lib, W, H, **kw):
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


@functools.lru_cache(maxsize=None)
def frame(k, W, H):
    return util.frame(k, W, H, noise=True, holes=HOLES)


@functools.lru_cache(maxsize=None)
def ref_pyramid(k, W, H):
    rgb, depth = frame(k, W, H)
    return orf.pyramid(rgb, depth, K4(W, H))


def to_device(a):
    import torch
    a = np.array(a, order="C")                                                          # (a copy: the cached frames are read-only)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()       # (the same bytes: only the address is passed on)
    torch.cuda.synchronize()
    return t


def assert_pyramid(f, which, ref, what):
    for l, lv in enumerate(ref):
        got = f.odometry_pyramid(which, l)
        for nm in ("I", "D", "gx", "gy"):
            util.assert_same_bits(got[nm], lv[nm], "%s level %d %s" % (what, l, nm))
        util.assert_same_bits(got["intrinsics"], np.array(lv["K"], f32), "%s level %d intrinsics" % (what, l))
    with pytest.raises(binding.SsfError, match=r"\(-1\)"):
        f.odometry_pyramid(which, len(ref))


def same_estimate(got, want, what):
    util.assert_same_bits(got[0], want[0], what + " rel")
    assert got[1] == want[1], (what, got[1], want[1])
    assert np.isfinite(got[0]).all()


# ---- 1. the pyramid -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,L", SHAPES)
def test_every_level_of_the_pyramid(W, H, L, product_lib):
    f = handle(product_lib, W, H)
    rgb, depth = frame(3, W, H)
    assert 0.15 < (depth == 0).mean() < 0.35
    ref = ref_pyramid(3, W, H)
    assert len(ref) >= L and (ref[-1]["W"], ref[-1]["H"]) == orf.level_sizes(W, H)[-1]
    f.odometry_set_reference(rgb, depth)
    assert_pyramid(f, 0, ref, "reference")
    # the same frame as a sensor delivers it: BGR8 colour, uint16 depth
    scale = 0.0002
    counts = np.clip(np.rint(depth.astype(np.float64) / scale), 0, 65535).astype(np.uint16)
    g = handle(product_lib, W, H)
    g.set_input_format("bgr8", "u16", scale)
    g.odometry_set_reference(np.ascontiguousarray(rgb[..., ::-1]), counts)
    raw = orf.pyramid(np.ascontiguousarray(rgb[..., ::-1]), counts, K4(W, H), order="bgr", depth_scale=scale)
    assert_pyramid(g, 0, raw, "bgr8 + u16")
    f.odometry_set_reference(rgb, orf.convert_depth(counts, scale))
    assert_pyramid(f, 0, raw, "the converted frame through the float path")


# ---- 2. the normal equations ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,L", SHAPES)
def test_linearise_at_five_transforms_on_every_level(W, H, L, product_lib):
    f = handle(product_lib, W, H)
    f.odometry_set_reference(*frame(0, W, H))
    f.odometry_estimate(*frame(1, W, H), params=dict(levels=L, iters=[0] * 6))          # (builds the current pyramid, no iteration)
    ref, cur = ref_pyramid(0, W, H), ref_pyramid(1, W, H)
    assert_pyramid(f, 1, cur, "current")
    p = orf.params(levels=L)
    counts = {}
    for l in range(L):
        for name, T in transforms():
            want = orf.record(ref[l], cur[l], T, p)
            got = f.odometry_linearise(l, T, params=dict(levels=L))
            assert np.array_equal(got, want), (l, name, got, want)
            counts[(l, name)] = int(want[28])
            if name == "none left":
                assert not want.any()
    n0 = ref[0]["W"] * ref[0]["H"]
    assert counts[(0, "identity")] > n0 // 2 and 0 < counts[(0, "mostly out")] < counts[(0, "identity")] // 2
    assert 0 < counts[(0, "behind")] < counts[(0, "identity")]
    with pytest.raises(binding.SsfError, match=r"\(-1\)"):
        f.odometry_linearise(L, orf.IDENTITY12, params=dict(levels=L))
    # a Python-int sum gives the same words
    assert np.array_equal(orf.record(ref[L - 1], cur[L - 1], transforms()[1][1], p, exact=True), f.odometry_linearise(L - 1, transforms()[1][1], params=dict(levels=L)))


# ---- 3. the loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,L", SHAPES)
def test_the_estimate_equals_the_restatements_loop(W, H, L, product_lib, oracle_lib):
    f = handle(product_lib, W, H)
    f.odometry_set_reference(*frame(0, W, H))
    ref, cur = ref_pyramid(0, W, H), ref_pyramid(1, W, H)
    kw = dict(levels=L)
    for init in (None, true_rel12(0)):
        want = orf.estimate(ref, cur, orf.params(**kw), oracle_lib, init12=init)
        got = f.odometry_estimate(*frame(1, W, H), init12=init, params=kw)
        same_estimate(got, want, "init" if init is not None else "no init")
        assert want[1]["levels"] == L and sum(want[1]["iters"]) > 0 and want[1]["iters"][L:] == [0] * (6 - L)
    # the gates: a gate nothing passes, and one iteration per level
    for kw2 in (dict(kw, max_translation=0.0), dict(kw, iters=[1] * 6), dict(kw, min_pixel_share=1.0)):
        want = orf.estimate(ref, cur, orf.params(**kw2), oracle_lib)
        same_estimate(f.odometry_estimate(*frame(1, W, H), params=kw2), want, str(sorted(kw2)))
    assert want[1]["reason"] == "too_few_pixels" and not want[1]["valid"]


# ---- 4. the reference's mask ------------------------------------------------------------------------------------------------
def test_a_ref_mask_changes_the_record_as_the_restatement_says(product_lib, oracle_lib):
    W, H, L = 100, 60, 3
    f = handle(product_lib, W, H)
    rgb, depth = frame(0, W, H)
    mask = (np.random.default_rng(5).random((H, W)) < 0.3).astype(np.uint8) * 200
    f.odometry_set_reference(rgb, depth, ref_mask=mask)
    ref = orf.pyramid(rgb, depth, K4(W, H), mask=mask)
    assert_pyramid(f, 0, ref, "masked reference")
    cur = ref_pyramid(1, W, H)
    same_estimate(f.odometry_estimate(*frame(1, W, H), params=dict(levels=L)), orf.estimate(ref, cur, orf.params(levels=L), oracle_lib), "masked")
    plain = ref_pyramid(0, W, H)
    for l in range(L):
        want = orf.record(ref[l], cur[l], orf.IDENTITY12, orf.params(levels=L))
        assert np.array_equal(f.odometry_linearise(l, orf.IDENTITY12, params=dict(levels=L)), want)
    assert orf.record(ref[0], cur[0], orf.IDENTITY12, orf.params())[28] < orf.record(plain[0], cur[0], orf.IDENTITY12, orf.params())[28]
    # everything masked: invalid, "too few pixels", nothing is NaN
    f.odometry_set_reference(rgb, depth, ref_mask=np.ones((H, W), np.uint8))
    rel, res = f.odometry_estimate(*frame(1, W, H), params=dict(levels=L))
    assert res["valid"] == 0 and res["reason"] == "too_few_pixels" and res["pixels"] == 0 and res["mean_sq_residual"] == 0.0
    assert np.array_equal(rel, orf.IDENTITY12)                        # (never moved; the translation is -(0) = -0)
    same_estimate((rel, res), orf.estimate(orf.pyramid(rgb, depth, K4(W, H), mask=np.ones((H, W), np.uint8)), cur, orf.params(levels=L), oracle_lib),
                  "all masked")
    assert not f.odometry_linearise(0, orf.IDENTITY12).any()


# ---- 5. device inputs, determinism --------------------------------------------------------------------------------------------
def test_device_inputs_give_the_host_inputs_bits_and_two_calls_the_same(product_lib):
    W, H, L = 160, 128, 3
    f, g = handle(product_lib, W, H), handle(product_lib, W, H)
    (rgb0, d0), (rgb1, d1) = frame(0, W, H), frame(1, W, H)
    mask = (np.random.default_rng(6).random((H, W)) < 0.1).astype(np.uint8)
    f.odometry_set_reference(rgb0, d0, ref_mask=mask)
    t = [to_device(a) for a in (rgb0, d0, mask, rgb1, d1)]
    g.odometry_set_reference_device(t[0], t[1], ref_mask=t[2])
    host = f.odometry_estimate(rgb1, d1, params=dict(levels=L))
    for _ in range(2):
        same_estimate(g.odometry_estimate_device(t[3], t[4], params=dict(levels=L)), host, "device")
        same_estimate(f.odometry_estimate(rgb1, d1, params=dict(levels=L)), host, "again")
    for l in range(L):
        assert np.array_equal(f.odometry_linearise(l, true_rel12(0)), g.odometry_linearise(l, true_rel12(0)))
    pf, rf = f.odometry_track(rgb1, d1, params=dict(levels=L))
    pg, rg = g.odometry_track_device(t[3], t[4], params=dict(levels=L))
    assert rf == rg == host[1] and rf["valid"]
    util.assert_same_bits(pf, pg, "prior")
    util.assert_same_bits(pf, orf.compose(f.get_pose(), host[0]), "prior = pose_ref o rel")
    last = f.odometry_last()
    util.assert_same_bits(last["rel"], host[0], "odometry_last rel")
    util.assert_same_bits(last["prior"], pf, "odometry_last prior")
    assert last["result"] == rf


# ---- 6. the frame path with the prior -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", [None, True])
def test_process_frame_odometry_equals_track_then_process_frame(motion, product_lib):
    W, H = 160, 128
    A, B = handle(product_lib, W, H), handle(product_lib, W, H)
    kw = dict(levels=3)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        A.odometry_last()
    extra = {} if motion is None else dict(motion=motion)
    n_prior = 0
    for k in range(5):
        rgb, depth = util.frame(k, W, H)
        ra = A.process_frame(rgb, depth, odometry=kw, **extra)
        if k == 0:
            with pytest.raises(binding.SsfError, match=r"\(-5\)"):
                B.odometry_track(rgb, depth, params=kw)                 # (no reference yet: the first frame runs without a prior)
            rb = B.process_frame(rgb, depth, **extra)
            B.odometry_set_reference(rgb, depth)
        else:
            prior, res = B.odometry_track(rgb, depth, params=kw)
            n_prior += prior is not None
            rb = B.process_frame(rgb, depth, prior_pose=prior, **extra)
            la = A.odometry_last()
            assert la["result"] == res
            util.assert_same_bits(la["prior"], prior, "prior of frame %d" % k)
        util.same_result(ra, rb)
    assert n_prior == 4
    util.compare_state(A, B)
    # the device frame form
    rgb, depth = util.frame(5, W, H)
    d_rgb, d_depth = to_device(rgb), to_device(depth)
    ra = A.process_frame_device(d_rgb.data_ptr(), d_depth.data_ptr(), odometry=kw, **extra).as_dict()
    util.same_result(ra, B.process_frame(rgb, depth, odometry=kw, **extra))
    util.compare_state(A, B)


# ---- 7. no side effects -------------------------------------------------------------------------------------------------------
def test_odometry_calls_between_frames_change_no_later_result(product_lib):
    W, H = 160, 128
    A, B = handle(product_lib, W, H), handle(product_lib, W, H)
    for k in range(0, 12, 2):
        rgb, depth = util.frame(k, W, H)
        A.odometry_set_reference(rgb, depth)
        A.odometry_estimate(*util.frame(k + 1, W, H))
        A.odometry_linearise(1, orf.IDENTITY12)
        A.odometry_track(*util.frame(k + 1, W, H))
        util.same_result(A.process_frame(rgb, depth), B.process_frame(rgb, depth))
    util.compare_state(A, B)


# ---- 8. misuse --------------------------------------------------------------------------------------------------------------
def test_the_refusals(product_lib):
    W, H = 100, 60
    f = handle(product_lib, W, H)
    rgb, depth = util.frame(0, W, H)
    bad_T = orf.IDENTITY12.copy()
    bad_T[10] = np.nan
    for call in (lambda: f.odometry_estimate(rgb, depth), lambda: f.odometry_track(rgb, depth), lambda: f.odometry_linearise(0, orf.IDENTITY12)):
        with pytest.raises(binding.SsfError, match=r"\(-5\)"):
            call()                                                     # no reference
    f.odometry_set_reference(rgb, depth)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        f.odometry_linearise(0, orf.IDENTITY12)                        # a reference, but no current pyramid
    f.odometry_estimate(rgb, depth)
    for kw in (dict(r_max=-0.1), dict(huber=float("nan")), dict(min_pixel_share=float("inf")), dict(tol_rot=-1.0), dict(tol_trans=float("nan")),
               dict(max_translation=-1.0), dict(max_rotation=float("nan")), dict(levels=0), dict(iters=[1, -1])):
        for call in (lambda: f.odometry_estimate(rgb, depth, params=kw), lambda: f.odometry_track(rgb, depth, params=kw),
                     lambda: f.odometry_linearise(0, orf.IDENTITY12, params=kw), lambda: f.process_frame(rgb, depth, odometry=kw)):
            with pytest.raises(binding.SsfError, match=r"\(-1\)"):
                call()
    for call in (lambda: f.odometry_linearise(0, bad_T), lambda: f.odometry_linearise(-1, orf.IDENTITY12), lambda: f.odometry_linearise(9, orf.IDENTITY12),
                 lambda: f.odometry_estimate(rgb, depth, init12=bad_T)):
        with pytest.raises(binding.SsfError, match=r"\(-1\)"):
            call()
    # a device depth pointer not aligned for the input format
    d_rgb, d_depth = to_device(rgb), to_device(np.zeros(H * W + 1, f32))
    for call in (lambda: f.odometry_estimate_device(d_rgb, d_depth.data_ptr() + 2), lambda: f.odometry_set_reference_device(d_rgb, d_depth.data_ptr() + 2),
                 lambda: f.odometry_track_device(d_rgb, d_depth.data_ptr() + 2)):
        with pytest.raises(binding.SsfError, match=r"\(-1\)"):
            call()
    # a device colour pointer of a 4-byte format not aligned to 4 bytes (k_odo_pyramid_base loads the pixel as one uint32_t)
    q = handle(product_lib, W, H)
    q.set_input_format("rgba8", "f32")
    d_rgba, d_ok = to_device(np.zeros(H * W * 4 + 4, np.uint8)), to_device(depth)
    q.odometry_set_reference_device(d_rgba, d_ok)
    for off in (1, 2, 3):
        for call in (lambda: q.odometry_estimate_device(d_rgba.data_ptr() + off, d_ok), lambda: q.odometry_set_reference_device(d_rgba.data_ptr() + off, d_ok),
                     lambda: q.odometry_track_device(d_rgba.data_ptr() + off, d_ok)):
            with pytest.raises(binding.SsfError, match=r"\(-1\)"):
                call()
    # the handle keeps working
    assert f.odometry_estimate(*util.frame(1, W, H))[1]["valid"] == 1
    # frames pending in the extract pipeline
    g = handle(product_lib, W, H, pipeline_depth=2, extract_batch=2)
    g.submit_frame(rgb, depth)
    assert g.pending_frames() > 0
    for call in (lambda: g.odometry_set_reference(rgb, depth), lambda: g.process_frame(rgb, depth, odometry=True)):
        with pytest.raises(binding.SsfError, match=r"\(-5\)"):
            call()
    while g.pending_frames() > 0:
        g.process_submitted()
    g.odometry_set_reference(rgb, depth)
    # a sharded handle
    s = handle(product_lib, W, H, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        s.odometry_set_reference(rgb, depth)


# ---- 9. profiling -------------------------------------------------------------------------------------------------------------
def test_the_kernels_are_timed_under_profile(product_lib):
    W, H = 160, 128
    f = handle(product_lib, W, H, profile=1)
    f.reset_kernel_times()
    f.odometry_set_reference(*util.frame(0, W, H))
    _, res = f.odometry_estimate(*util.frame(1, W, H))
    names = f.kernel_times()
    assert names["odo_pyramid"][1] == 2 and names["odo_linearise"][1] == sum(res["iters"]), names
