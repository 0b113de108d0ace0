"""Dense RGB-D odometry on the MI355X, the paths tests/test_odometry_gpu.py's three shapes never take, against the numpy restatement
(tests/odometry_ref.py) with == and at 0 bits: the strided loop of k_odo_linearise past its 1024 workgroups (644 x 410, the second
trip alone under a mask, 1024 x 513 where every thread strides), all six levels, reductions from an odd size and the level clamp
(102 x 62, 202 x 126, 101 x 63), the eight input formats with random alpha bytes and planted uint16 counts, planted invalid depths
and a narrower range on the device, warped coordinates exactly on the border, and the parameter edges of the loop.  The inputs come
from tests/odometry_cases.py; tests/test_odometry.py asserts on a machine without a GPU that each of them reaches what it is there
for."""
import numpy as np
import pytest

import odometry_cases as oc
import odometry_ref as orf
import util
from supersurfel_fusion_amd import binding
from test_odometry_gpu import assert_pyramid, handle, same_estimate, to_device

pytestmark = pytest.mark.gpu
f32 = np.float32


def build_current(f, rgb, depth, levels=6):
    """the current pyramid without an iteration"""
    f.odometry_estimate(rgb, depth, params=dict(levels=levels, iters=[0] * 6))


def assert_records(f, ref, cur, cases, kw, levels=None, rng=orf.RANGE):
    """the record of every level in `levels` at every (name, T) of `cases` equals the restatement's; returns the pixel counts"""
    p = orf.params(**kw)
    counts = {}
    for l in (range(len(ref)) if levels is None else levels):
        for name, T in cases:
            want = orf.record(ref[l], cur[l], T, p, rng=rng)
            got = f.odometry_linearise(l, T, params=kw)
            assert np.array_equal(got, want), (l, name, got, want)
            counts[(l, name)] = int(want[28])
    return counts


def refused(call):
    with pytest.raises(binding.SsfError, match=r"\(-1\)"):
        call()


# ---- 1. the strided launch and six levels -----------------------------------------------------------------------------------------
def test_644x410_both_pyramids_and_the_record_on_all_six_levels(product_lib):
    W, H = oc.BIG
    f = handle(product_lib, W, H)
    f.odometry_set_reference(*oc.frame(0, W, H))
    build_current(f, *oc.frame(1, W, H))
    ref, cur = oc.pyramid(0, W, H), oc.pyramid(1, W, H)
    assert [(lv["W"], lv["H"]) for lv in ref] == oc.BIG_SIZES
    assert_pyramid(f, 0, ref, "reference")
    assert_pyramid(f, 1, cur, "current")
    counts = assert_records(f, ref, cur, oc.transforms(), dict(levels=6))
    assert all(2 * counts[(l, "identity")] > ref[l]["W"] * ref[l]["H"] for l in range(6))
    for l in (4, 5):
        assert np.array_equal(orf.record(ref[l], cur[l], oc.transform("small"), orf.params(levels=6), exact=True),
                              f.odometry_linearise(l, oc.transform("small"), params=dict(levels=6)))
    # the default asks for four levels: levels 4 and 5 exist in the pyramid but are refused
    refused(lambda: f.odometry_linearise(4, orf.IDENTITY12))
    refused(lambda: f.odometry_linearise(6, orf.IDENTITY12, params=dict(levels=6)))
    refused(lambda: f.odometry_linearise(6, orf.IDENTITY12, params=dict(levels=9)))
    assert np.array_equal(f.odometry_linearise(5, oc.transform("small"), params=dict(levels=9)), orf.record(ref[5], cur[5], oc.transform("small"), orf.params()))


def test_644x410_the_second_trip_alone_and_the_first_alone_share_out_the_record(product_lib):
    W, H = oc.BIG
    rgb, depth = oc.frame(0, W, H)
    head, tail = oc.trip_masks(W, H)
    cur = oc.pyramid(1, W, H)
    f = handle(product_lib, W, H)
    cases = [(nm, oc.transform(nm)) for nm in ("identity", "small")]
    got = {}
    for which, mask in ((0, head), (1, tail), (2, None)):
        f.odometry_set_reference(rgb, depth, ref_mask=mask)
        if which == 0:
            build_current(f, *oc.frame(1, W, H))
        ref = oc.masked_pyramid(which) if which < 2 else oc.pyramid(0, W, H)
        util.assert_same_bits(f.odometry_pyramid(0, 0)["D"], ref[0]["D"], "masked D")
        counts = assert_records(f, ref, cur, cases, dict(levels=6), levels=[0])
        got[which] = {nm: f.odometry_linearise(0, T, params=dict(levels=6)) for nm, T in cases}
        if which == 0:
            assert counts[(0, "identity")] >= 500                                # a kernel without its loop would give zeros here
    for nm, _ in cases:
        assert np.array_equal(got[0][nm] + got[1][nm], got[2][nm]), nm


def test_1024x513_where_every_workgroup_takes_a_second_trip_and_four_a_third(product_lib):
    W, H = oc.THREE_TRIPS
    f = handle(product_lib, W, H)
    f.odometry_set_reference(*oc.frame(0, W, H))
    build_current(f, *oc.frame(1, W, H), levels=1)
    counts = assert_records(f, oc.pyramid(0, W, H), oc.pyramid(1, W, H), oc.three_trip_transforms(), dict(levels=1), levels=[0])
    assert min(counts.values()) > W * H // 2


def test_644x410_the_estimate_over_six_levels(product_lib, oracle_lib):
    W, H = oc.BIG
    f = handle(product_lib, W, H, profile=1)
    f.reset_kernel_times()
    f.odometry_set_reference(*oc.frame(0, W, H))
    ref, cur = oc.pyramid(0, W, H), oc.pyramid(1, W, H)
    kw = dict(levels=6, iters=[2] * 6)
    launches = 0
    for init in (None, oc.true_rel12(0)):
        want = orf.estimate(ref, cur, orf.params(**kw), oracle_lib, init12=init)
        same_estimate(f.odometry_estimate(*oc.frame(1, W, H), init12=init, params=kw), want, "init" if init is not None else "no init")
        assert want[1]["levels"] == 6 and all(1 <= n <= 2 for n in want[1]["iters"])
        launches += sum(want[1]["iters"])
    names = f.kernel_times()
    assert names["odo_pyramid"][1] == 3 and names["odo_linearise"][1] == launches, names


# ---- 2. odd reductions and the level clamp ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,sizes", oc.ODD)
def test_odd_reductions_and_levels_6_clamped_to_what_the_image_offers(W, H, sizes, product_lib, oracle_lib):
    L = len(sizes)
    f = handle(product_lib, W, H)
    f.odometry_set_reference(*oc.frame(0, W, H))
    build_current(f, *oc.frame(1, W, H))
    ref, cur = oc.pyramid(0, W, H), oc.pyramid(1, W, H)
    assert [(lv["W"], lv["H"]) for lv in ref] == sizes
    assert_pyramid(f, 0, ref, "reference")
    assert_pyramid(f, 1, cur, "current")
    assert_records(f, ref, cur, oc.transforms(), dict(levels=6))
    refused(lambda: f.odometry_linearise(L, orf.IDENTITY12, params=dict(levels=6)))
    for init in (None, oc.true_rel12(0)):
        want = orf.estimate(ref, cur, orf.params(levels=6), oracle_lib, init12=init)
        same_estimate(f.odometry_estimate(*oc.frame(1, W, H), init12=init, params=dict(levels=6)), want, "levels=6")
        assert want[1]["levels"] == L and want[1]["iters"][L:] == [0] * (6 - L) and all(want[1]["iters"][:L])


@pytest.mark.parametrize("W,H", oc.DROPPED)
def test_the_dropped_column_of_an_odd_level_changes_no_coarser_level(W, H, product_lib):
    rgb, depth = oc.frame(0, W, H)
    rgb2, depth2, l = oc.dropped_column_changed(rgb, depth)
    f, g = handle(product_lib, W, H), handle(product_lib, W, H)
    f.odometry_set_reference(rgb, depth)
    g.odometry_set_reference(rgb2, depth2)
    a, b = orf.pyramid(rgb, depth, oc.K4(W, H)), orf.pyramid(rgb2, depth2, oc.K4(W, H))
    assert_pyramid(f, 0, a, "as rendered")
    assert_pyramid(g, 0, b, "another dropped column")                             # (level l's gradients next to it change as the restatement says)
    for k in range(len(a)):
        x, y = f.odometry_pyramid(0, k), g.odometry_pyramid(0, k)
        for nm in ("I", "D", "gx", "gy"):
            if k > l:
                util.assert_same_bits(x[nm], y[nm], "level %d %s" % (k, nm))
            else:
                assert not np.array_equal(x[nm], y[nm]), (k, nm)


# ---- 3. the input formats ---------------------------------------------------------------------------------------------------------
def raw_frame(k, color, depth_fmt):
    """frame k of EDGE_SHAPE as the sensor delivers it, and the restatement's pyramid of the THREE-channel frame"""
    W, H = oc.EDGE_SHAPE
    rgb, depth = oc.frame(k, W, H)
    d = oc.u16_counts(depth)[0] if depth_fmt == "u16" else depth
    want = orf.pyramid(rgb, orf.convert_depth(d, oc.U16_SCALE), oc.K4(W, H))
    return oc.colour_as(rgb, color, seed=11 + k), d, want


@pytest.mark.parametrize("depth_fmt", ["f32", "u16"])
@pytest.mark.parametrize("color", ["rgb8", "bgr8", "rgba8", "bgra8"])
def test_every_input_format_gives_the_three_channel_float_frames_bits(color, depth_fmt, product_lib, oracle_lib):
    W, H = oc.EDGE_SHAPE
    (c0, d0, ref), (c1, d1, cur) = raw_frame(0, color, depth_fmt), raw_frame(1, color, depth_fmt)
    last = len(ref) - 1
    want = orf.estimate(ref, cur, orf.params(levels=3), oracle_lib)
    assert want[1]["valid"] == 1
    # the restatement reading the raw arrays in their own order agrees with the three-channel frame it is given above
    raw = orf.pyramid(c0, d0, oc.K4(W, H), order=color[:-1], depth_scale=oc.U16_SCALE)
    assert all(np.array_equal(raw[l][nm], ref[l][nm]) for l in range(len(ref)) for nm in ("I", "D"))
    on_device = [False] + ([True] if (color, depth_fmt) in (("rgba8", "u16"), ("bgra8", "f32")) else [])
    for dev in on_device:
        f = handle(product_lib, W, H)
        f.set_input_format(color, depth_fmt, oc.U16_SCALE if depth_fmt == "u16" else 1.0)
        if dev:
            t = [to_device(a) for a in (c0, d0, c1, d1)]
            f.odometry_set_reference_device(t[0], t[1])
            got = f.odometry_estimate_device(t[2], t[3], params=dict(levels=3))
        else:
            f.odometry_set_reference(c0, d0)
            got = f.odometry_estimate(c1, d1, params=dict(levels=3))
        assert_pyramid(f, 0, ref, "%s + %s reference" % (color, depth_fmt))
        assert_pyramid(f, 1, cur, "%s + %s current" % (color, depth_fmt))
        same_estimate(got, want, "%s + %s" % (color, depth_fmt))
        assert_records(f, ref, cur, [("small", oc.transform("small"))], dict(levels=3), levels=[0, last])


# ---- 4. depth validation and a non-default range on the device ----------------------------------------------------------------------
def test_planted_invalid_depths_on_the_device(product_lib, oracle_lib):
    W, H = 64, 48
    rgb, depth, blocks = oc.planted_depth_frame()
    f = handle(product_lib, W, H)
    f.odometry_set_reference(rgb, depth)
    build_current(f, rgb, depth)
    pyr = orf.pyramid(rgb, depth, oc.K4(W, H))
    assert_pyramid(f, 0, pyr, "reference")
    assert_pyramid(f, 1, pyr, "current")
    D1 = f.odometry_pyramid(0, 1)["D"]
    for (x, y), _, want in blocks:
        util.assert_same_bits(D1[y // 2, x // 2], want, "block at (%d, %d)" % (x, y))
    for l in range(3):
        D = f.odometry_pyramid(0, l)["D"]
        assert np.isfinite(D).all() and not np.signbit(D).any()
    cases = [("identity", orf.IDENTITY12), ("small", oc.transform("small"))]
    assert_records(f, pyr, pyr, cases, dict(levels=3))
    for init in (None, oc.transform("small")):
        got = f.odometry_estimate(rgb, depth, init12=init, params=dict(levels=3))
        same_estimate(got, orf.estimate(pyr, pyr, orf.params(levels=3), oracle_lib, init12=init), "planted")
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]["mean_sq_residual"])
    # the device frame form reads the same bytes
    g = handle(product_lib, W, H)
    t = [to_device(rgb), to_device(depth)]
    g.odometry_set_reference_device(*t)
    assert_pyramid(g, 0, pyr, "device frame")


def test_a_narrower_range_on_the_device(product_lib, oracle_lib):
    W, H = oc.EDGE_SHAPE
    lo, hi = oc.NARROW
    f = handle(product_lib, W, H, range_min=float(lo), range_max=float(hi))
    f.odometry_set_reference(*oc.frame(0, W, H))
    build_current(f, *oc.frame(1, W, H))
    ref, cur = oc.pyramid(0, W, H, oc.NARROW), oc.pyramid(1, W, H, oc.NARROW)
    assert_pyramid(f, 0, ref, "reference")
    assert_pyramid(f, 1, cur, "current")
    cases = [(nm, oc.transform(nm)) for nm in ("small", "behind")]
    counts = assert_records(f, ref, cur, cases, dict(levels=3), rng=oc.NARROW)
    assert all(n > 0 for n in counts.values())
    want = orf.estimate(ref, cur, orf.params(levels=3), oracle_lib, rng=oc.NARROW)
    same_estimate(f.odometry_estimate(*oc.frame(1, W, H), params=dict(levels=3)), want, "narrow range")
    assert want[1]["valid"] == 1


# ---- 5. the warp's border, exactly ----------------------------------------------------------------------------------------------------
def test_warped_coordinates_exactly_on_integers_and_on_the_border(product_lib):
    W, H = 64, 48
    rgb, depth, K = oc.border_frame()
    f = handle(product_lib, W, H, **dict(zip(("fx", "fy", "cx", "cy"), K)))
    f.odometry_set_reference(rgb, depth)
    build_current(f, rgb, depth)
    pyr = orf.pyramid(rgb, depth, K)
    assert_pyramid(f, 0, pyr, "reference")
    kw = dict(levels=3, r_max=1.0)
    cases = [("%+d %+d" % s, oc.shift12(*s)) for s in oc.BORDER_SHIFTS + [(63, 0), (0, 47)]]
    counts = assert_records(f, pyr, pyr, cases, kw)
    for kx, ky in oc.BORDER_SHIFTS:
        assert f.odometry_linearise(0, oc.shift12(kx, ky), params=kw)[28] == oc.border_count(kx, ky) == counts[(0, "%+d %+d" % (kx, ky))]
    assert counts[(0, "+62 +0")] == H - 1 and counts[(0, "+0 +46")] == W - 1 and counts[(0, "+63 +0")] == 0 == counts[(0, "+0 +47")]


# ---- 6. parameter edges of the loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", oc.PARAM_EDGES)
def test_a_parameter_edge_of_the_loop(name, kw, product_lib, oracle_lib):
    W, H = oc.EDGE_SHAPE
    f = handle(product_lib, W, H)
    f.odometry_set_reference(*oc.frame(0, W, H))
    ref, cur = oc.pyramid(0, W, H), oc.pyramid(1, W, H)
    kw = dict(kw, levels=3)
    want = orf.estimate(ref, cur, orf.params(**kw), oracle_lib)
    same_estimate(f.odometry_estimate(*oc.frame(1, W, H), params=kw), want, name)
    rec_kw = {k: v for k, v in kw.items() if k in ("levels", "r_max", "huber")}
    assert_records(f, ref, cur, [(nm, oc.transform(nm)) for nm in ("identity", "small")], rec_kw)


def test_a_few_reference_pixels(product_lib, oracle_lib):
    W, H = oc.EDGE_SHAPE
    rgb, depth = oc.frame(0, W, H)
    cur = oc.pyramid(1, W, H)
    kw = dict(levels=1, min_pixel_share=0.0)
    f = handle(product_lib, W, H)
    for n in (1, 3, 5, 7):
        mask = oc.few_pixel_mask(n)
        f.odometry_set_reference(rgb, depth, ref_mask=mask)
        ref = orf.pyramid(rgb, depth, oc.K4(W, H), mask=mask)
        want = orf.estimate(ref, cur, orf.params(**kw), oracle_lib)
        same_estimate(f.odometry_estimate(*oc.frame(1, W, H), params=kw), want, "%d pixels" % n)
        counts = assert_records(f, ref, cur, [(nm, oc.transform(nm)) for nm in ("identity", "small")], dict(levels=1), levels=[0])
        assert counts[(0, "identity")] == n


def test_the_small_checkerboard_the_largest_terms_through_the_lds_atomics(product_lib):
    W, H = oc.EDGE_SHAPE
    rgb, neg, depth = oc.checkerboard()
    f = handle(product_lib, W, H)
    f.odometry_set_reference(rgb, depth)
    build_current(f, neg, depth)
    ref, cur = orf.pyramid(rgb, depth, oc.K4(W, H)), orf.pyramid(neg, depth, oc.K4(W, H))
    assert_pyramid(f, 0, ref, "checkerboard")
    kw = dict(levels=3, r_max=2.0, huber=2.0)
    counts = assert_records(f, ref, cur, [("identity", orf.IDENTITY12), ("small", oc.transform("small"))], kw)
    assert counts[(0, "identity")] == 6161
    got = f.odometry_linearise(0, orf.IDENTITY12, params=kw)
    assert np.array_equal(got, orf.record(ref[0], cur[0], orf.IDENTITY12, orf.params(**kw), exact=True))
    assert max(int(v).bit_length() for v in got) == 49
