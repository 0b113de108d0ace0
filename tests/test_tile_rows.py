"""tests/tile_rows_ref.py checked on the CPU, so that tests/test_tile_rows_gpu.py cannot pass vacuously: the restatement of bin_of
against the pieces the arithmetic tests already pin (the oracle's pixel_round and m3_mulv, tests/mathops.py) and against a float64
evaluation of the same formula, and every case the GPU file runs against the occupancy its family states."""
import ctypes as C

import numpy as np
import pytest

import mathops as mo
import tile_rows_ref as tr
import util

F = np.float32
ALL_SHAPES = (tr.SMALL,) + tr.OTHER_SHAPES


@pytest.fixture(scope="module")
def orc_batch(oracle_lib):
    fn = oracle_lib.lib.ssf_oracle_mathbatch
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]; fn.restype = C.c_int
    return fn


def test_the_restated_pixel_round_is_the_pinned_one(orc_batch):
    """on every binade (first, last and random mantissas), every k + 0.5 for |k| <= 2^12, the neighbours of +-2^23 and +-2^31, +-0,
    denormals, +-inf, NaNs: the set tests/test_math_device_gpu.py holds the device's pixel_round to"""
    b32 = mo.f32_binade_set()[::4]
    got = tr.pixel_round(b32.view(F)).view(np.uint32).reshape(-1, 1)
    mo.assert_same("pixel_round", b32, got, mo.evaluate(orc_batch, "pixel_round", b32), ("restatement", "oracle"))


def test_the_restated_transform_is_m3_mulv_and_add(orc_batch):
    rng = np.random.default_rng(11)
    n = 4096
    pos = rng.uniform(-5, 5, (n, 3)).astype(F)
    pos[::97] *= F(1e30); pos[5::101, 1] = F(np.inf); pos[7::103] = F(np.nan); pos[11::107] = F(-0.0)
    for name in ("identity", "oblique"):
        T = tr.transform_named(name)
        x = np.ascontiguousarray(np.concatenate([np.tile(T[:9], (n, 1)), pos], axis=1))
        want = mo.evaluate(orc_batch, "m3_mulv", x).view(F)
        with np.errstate(all="ignore"):
            want = want + T[9:]
        got = tr.transform(T, pos)
        util.assert_same_bits(got, want, "transform under " + name)          # (bit patterns; NaN == NaN)
        assert np.isnan(got).any() and np.isinf(got).any()
    R = tr.transform_named("oblique")[:9].astype(np.float64).reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.degrees(np.arccos((np.trace(R) - 1) / 2)) - 20.0) < 1e-4
    assert (np.abs(R) > 0.05).all() and (np.abs(R) < 0.99).all(), "the oblique rotation has an element that makes a product trivial"


@pytest.mark.parametrize("shape", [tr.SMALL, (1056, 1024), (97, 61)])
@pytest.mark.parametrize("name", ["identity", "oblique"])
def test_restated_bins_agree_with_float64_away_from_the_boundaries(shape, name):
    """a sanity check of the restatement against an independent evaluation, not a tolerance on the kernel: where the float64
    projection is more than 1e-3 pixel from a rounding boundary the two name the same bin, and that is nearly every row"""
    W, H = shape
    cam, T = tr.camera(W, H), tr.transform_named(name)
    pos = tr.case("uniform", name, W, H, 5000)[0]["positions"]
    b32 = tr.bin_of(cam, T, pos)
    b64, margin = tr.bin_of_f64(cam, T, pos)
    clear = margin > 1e-3
    assert clear.mean() > 0.99, clear.mean()
    assert np.array_equal(b32[clear], b64[clear]), np.flatnonzero(clear & (b32 != b64))[:10]
    assert len(np.unique(b32)) == min(tr.geometry(W, H)[2], 1 + 4500)


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_edges_hold_exact_halves_and_every_special_value(shape):
    """under the identity the edges family's rows project EXACTLY a half away from an integer on both sides of 0, at a tile border
    and at the image border (from inside and outside), in u and in v; the tie goes away from zero; and the rows with zero,
    denormal, infinite and NaN components and projections beyond 2^23 are there"""
    W, H = shape
    cam, T = tr.camera(W, H), tr.transform_named("identity")
    rows = tr.edge_rows(cam)
    for n in (63, 4097):
        pos = tr.case("edges", "identity", W, H, n)[0]["positions"]
        k = min(n, len(rows))
        assert np.array_equal(pos[:k].view(np.uint32), rows[:k].view(np.uint32))
    assert len(rows) < 4097
    frac, uv = tr.half_fraction(cam, T, rows)
    nbx, nby, nbins = tr.geometry(W, H)
    bins = tr.bin_of(cam, T, rows)
    for axis, size in ((0, W), (1, H)):
        tie = np.abs(frac[:, axis]) == F(0.5)
        at = {float(p): np.flatnonzero(tie & (uv[:, axis] == F(p))) for p in tr.half_targets(size)}
        for p, idx in at.items():
            assert idx.size >= 1, ("no row projects exactly to", p, "along axis", axis, shape)
        assert (frac[at[-0.5], axis] == F(-0.5)).all() and (frac[at[0.5], axis] == F(0.5)).all()
        other = uv[:, 1 - axis]
        plain = (other == F(16.0)) if min(W, H) > 16 else np.ones(len(rows), bool)
        # the tie rule's consequences, on rows whose other coordinate is an ordinary pixel: -0.5 is outside, 0.5 is pixel 1, a half
        # below the tile border is the next tile, size - 1.5 is the last pixel, size - 0.5 is outside
        pick = lambda p: at[p][plain[at[p]]]
        assert pick(-0.5).size and (bins[pick(-0.5)] == nbins - 1).all()
        assert pick(size - 0.5).size and (bins[pick(size - 0.5)] == nbins - 1).all()
        assert pick(0.5).size and (bins[pick(0.5)] == 0).all()
        assert pick(size - 1.5).size and (bins[pick(size - 1.5)] != nbins - 1).all()
        if size > tr.TILE:
            step = 1 if axis == 0 else nbx
            assert pick(tr.TILE - 0.5).size and (bins[pick(tr.TILE - 0.5)] == step).all()
    z = rows[:, 2]
    zbits = z.view(np.uint32)
    assert (zbits == 0).any() and (zbits == 0x80000000).any() and (zbits == 1).any() and (zbits == 0x00400000).any()
    on_axis = (rows[:, 0] == 0) & (rows[:, 1] == 0) & (z > 0) & (z < F(1e-38))
    assert on_axis.any() and (bins[on_axis] != nbins - 1).all(), "0 / denormal is 0: the row is in the image"
    beside = (rows[:, 0] == F(0.05)) & (z >= 0) & (z < F(1e-38))
    assert beside.any() and (bins[beside] == nbins - 1).all()
    for c in range(3):
        assert np.isnan(rows[:, c]).any() and (rows[:, c] == F(np.inf)).any() and (rows[:, c] == F(-np.inf)).any()
    with np.errstate(all="ignore"):
        assert (np.abs(uv[np.isfinite(uv[:, 0]), 0]) > F(8388608.0)).any() and (np.abs(uv[np.isfinite(uv[:, 1]), 1]) > F(8388608.0)).any()
        just_below = (np.abs(uv[:, 0]) < F(8388608.0)) & (np.abs(uv[:, 0]) > F(8000000.0))
    assert just_below.any() and (bins[just_below] == nbins - 1).all()
    bad = ~np.isfinite(rows).all(axis=1)
    assert (bins[bad] == nbins - 1).all()


def occupancy(family, name, W, H, n):
    model, T, aim = tr.case(family, name, W, H, n)
    assert len(model["confidences"]) == n and model["positions"].dtype == F
    nbins = tr.geometry(W, H)[2]
    bins = tr.bin_of(tr.camera(W, H), T, model["positions"])
    assert bins.min() >= 0 and bins.max() < nbins
    return aim, bins, np.bincount(bins, minlength=nbins), nbins


def check_occupancy(family, name, W, H, n):
    aim, bins, tot, nbins = occupancy(family, name, W, H, n)
    if aim["kind"] == "bins":                                       # these bins and no other
        assert sorted(np.flatnonzero(tot)) == sorted(aim["bins"]), (family, name, np.flatnonzero(tot))
    elif aim["kind"] == "alternate":
        assert np.array_equal(bins, np.where(np.arange(n) % 2 == 0, aim["bins"][0], aim["bins"][1]))
    elif aim["kind"] == "uniform":
        inside = n - aim["outside"]
        assert tot[-1] == aim["outside"] and np.count_nonzero(tot[:-1]) == min(nbins - 1, inside)
        if inside >= nbins - 1:
            assert tot[:-1].max() - tot[:-1].min() <= 1
        if n > 1:
            assert (bins[1:] != bins[:-1]).mean() > (0.8 if nbins > 2 else 0.05), "consecutive rows lie in the same tile: not an arrival order"
    else:
        assert aim["kind"] == "edges"
        if n >= 4096:                                              # rows that project nowhere, and rows all over the image
            assert tot[-1] > n // 8 and np.count_nonzero(tot[:-1]) >= min(nbins - 1, 1000)
    return tot


@pytest.mark.parametrize("n", tr.SMALL_SIZES)
def test_every_small_case_has_the_stated_occupancy(n):
    W, H = tr.SMALL
    nbins = tr.geometry(W, H)[2]
    assert nbins == 21
    for family, names in tr.FAMILIES.items():
        for name in names:
            tot = check_occupancy(family, name, W, H, n)
            if family == "uniform" and name != "nan" and n >= 1024:
                assert (tot > 0).all(), "uniform leaves a bin empty"
    assert [c[:2] for c in tr.small_cases() if c[2] == n] == [(f, t) for f in tr.FAMILIES for t in tr.FAMILIES[f]]


@pytest.mark.parametrize("shape", tr.OTHER_SHAPES)
def test_every_other_case_has_the_stated_occupancy(shape):
    W, H = shape
    nbx, nby, nbins = tr.geometry(W, H)
    assert nbins == {(97, 61): 9, (32, 32): 2, (1056, 1024): 1057, (2080, 2016): 4096}[shape] <= tr.MAX_BINS
    for n in tr.OTHER_SIZES:
        for family in ("uniform", "edges"):
            for name in tr.FAMILIES[family]:
                tot = check_occupancy(family, name, W, H, n)
                if family == "uniform" and name != "nan" and n == max(tr.OTHER_SIZES):
                    assert (tot > 0).all(), "uniform leaves a bin empty at the shape's larger size"
    assert sorted(set(c[2:4] for c in tr.other_cases())) == sorted(tr.OTHER_SHAPES)
    assert tr.geometry(*tr.TOO_FINE)[2] == tr.MAX_BINS + 1


def test_the_sizes_cover_the_branches_of_the_chunk_order_and_the_scan():
    """nwg = ceil(n / 4096): the residues nwg & 7 that xcd_block treats apart (a grid below eight, a multiple of eight, one more,
    a partial last round), and for k_bin_scan's eight segments of ceil(nwg / 8) workgroups: empty segments, all full, a partial last"""
    nwg = sorted({-(-n // tr.ROWS_PER_WG) for n in tr.SMALL_SIZES})
    assert nwg == [1, 2, 8, 9, 16, 18]
    assert {w & 7 for w in nwg} >= {0, 1, 2}
    empty = [w for w in nwg if 7 * (-(-w // 8)) >= w]
    assert 1 in empty and 2 in empty and 9 in empty and 8 not in empty
    assert {n % tr.ROWS_PER_WG for n in tr.SMALL_SIZES} >= {0, 1, 4095}
