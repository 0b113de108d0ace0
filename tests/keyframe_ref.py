"""numpy restatement of the keyframe database's rule (include/ssf_keyframes.h, rules 1-7): the fern generator, the coarse image,
codes, packing, diff, the query order and the consider decision.  Integers only (plus the two f32 divisions of the ratios), so
the GPU tests compare with == and nothing else."""
import numpy as np

from supersurfel_fusion_amd.binding import FERN_DTYPE

f32 = np.float32
M64 = (1 << 64) - 1
MAX_CANDIDATES = 8


def splitmix64(s):
    """one draw: (new state, value)"""
    s = (s + 0x9E3779B97F4A7C15) & M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return s, z ^ (z >> 31)


def depth_range_mm(range_min, range_max):
    return int(np.rint(f32(range_min) * f32(1000.0))), int(np.rint(f32(range_max) * f32(1000.0)))


def generate_ferns(seed, n, W, H, B, range_min, range_max):
    """rule 2: six draws per fern in the order x, y, r, g, b, depth_mm"""
    gw, gh = W // B, H // B
    dlo, dhi = depth_range_mm(range_min, range_max)
    assert dhi > dlo
    out = np.zeros(n, FERN_DTYPE)
    s = int(seed) & M64
    for i in range(n):
        v = []
        for _ in range(6):
            s, z = splitmix64(s)
            v.append(z)
        out[i] = (v[0] % gw, v[1] % gh, v[2] % 256, v[3] % 256, v[4] % 256, 0, dlo + v[5] % (dhi - dlo))
    return out


def coarse_image(rgb, plane_depth, B, range_min, range_max):
    """rule 1: (mean GH x GW x 3, cnt GH x GW, depth_mm GH x GW) as int64.  rgb: H x W x 3 uint8 (R, G, B)"""
    H, W = plane_depth.shape
    gh, gw = H // B, W // B
    c = rgb[:gh * B, :gw * B].astype(np.int64).reshape(gh, B, gw, B, 3).sum(axis=(1, 3))
    mean = (c + B * B // 2) // (B * B)
    d = np.ascontiguousarray(plane_depth[:gh * B, :gw * B], f32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d) & (d >= f32(range_min)) & (d <= f32(range_max))
    q = np.where(ok, np.rint(np.where(ok, d, f32(0)) * f32(1000.0)), 0).astype(np.int64)
    cnt = ok.reshape(gh, B, gw, B).sum(axis=(1, 3)).astype(np.int64)
    sq = q.reshape(gh, B, gw, B).sum(axis=(1, 3))
    depth_mm = np.where(cnt > 0, (sq + cnt // 2) // np.maximum(cnt, 1), 0)
    return mean, cnt, depth_mm


def encode(ferns, mean, cnt, depth_mm):
    """rule 3: one code byte per fern"""
    x, y = ferns["x"].astype(np.int64), ferns["y"].astype(np.int64)
    m = mean[y, x]
    code = (m[:, 0] > ferns["r"]).astype(np.uint8) | ((m[:, 1] > ferns["g"]).astype(np.uint8) << 1) | \
           ((m[:, 2] > ferns["b"]).astype(np.uint8) << 2) | \
           (((cnt[y, x] > 0) & (depth_mm[y, x] > ferns["depth_mm"].astype(np.int64))).astype(np.uint8) << 3)
    return code.astype(np.uint8)


def encode_frame(ferns, rgb, plane_depth, B, range_min, range_max):
    return encode(ferns, *coarse_image(rgb, plane_depth, B, range_min, range_max))


def packed_words(n):
    return ((n + 7) // 8 + 63) // 64 * 64


def pack(codes):
    """eight 4-bit codes per u32, fern i in bits 4 (i % 8) .. of word i / 8, zero nibbles up to a multiple of 64 words"""
    codes = np.asarray(codes, np.uint8)
    assert (codes <= 15).all()
    out = np.zeros(packed_words(len(codes)), np.uint32)
    for i, c in enumerate(codes.tolist()):
        out[i >> 3] |= np.uint32(c << (4 * (i & 7)))
    return out


def unpack(words, n):
    i = np.arange(n)
    return ((words[i >> 3] >> (4 * (i & 7)).astype(np.uint32)) & np.uint32(15)).astype(np.uint8)


def diff(a, b):
    """rule 4"""
    return int((np.asarray(a) != np.asarray(b)).sum())


def loop_flag(d, n, loop_ratio):
    return bool(f32(d) / f32(n) <= f32(loop_ratio))


class Database:
    """rules 5-7 on the host: what the device keeps, minus the rows' content (the row COUNT decides `full`)"""

    def __init__(self, n, max_keyframes=256, max_rows=None, min_gap=30, new_ratio=0.3, loop_ratio=0.2):
        self.n, self.max_keyframes, self.max_rows = n, max_keyframes, max_rows
        self.min_gap, self.new_ratio, self.loop_ratio = min_gap, f32(new_ratio), f32(loop_ratio)
        self.codes, self.stamps, self.rows = np.zeros((0, n), np.uint8), [], []

    @property
    def K(self):
        return len(self.stamps)

    def put(self, codes, stamp, n_rows=0):
        self.codes = np.concatenate([self.codes, np.asarray(codes, np.uint8)[None]])
        self.stamps.append(int(stamp)); self.rows.append(int(n_rows))
        return self.K - 1

    def query(self, codes, stamp, min_gap=None, k=MAX_CANDIDATES):
        """rule 5: dict(min_diff_all, candidates [dict(id, diff, stamp, loop)])"""
        min_gap = self.min_gap if min_gap is None else min_gap
        if self.K == 0:
            return dict(min_diff_all=self.n + 1, candidates=[])
        d = (self.codes != np.asarray(codes, np.uint8)[None]).sum(axis=1).astype(np.int64)
        st = np.asarray(self.stamps, np.int64)
        el = np.flatnonzero(st <= int(stamp) - int(min_gap))
        order = el[np.lexsort((el, d[el]))][:k]                      # (diff, id) ascending
        cand = [dict(id=int(i), diff=int(d[i]), stamp=int(st[i]), loop=loop_flag(d[i], self.n, self.loop_ratio)) for i in order]
        return dict(min_diff_all=int(d.min()), candidates=cand)

    def consider(self, codes, stamp, n_rows=0):
        """rule 6: the record of ssf_keyframes_consider"""
        q = self.query(codes, stamp)
        want = self.K == 0 or bool(f32(q["min_diff_all"]) / f32(self.n) >= self.new_ratio)
        full = want and (self.K >= self.max_keyframes or (self.max_rows is not None and sum(self.rows) + n_rows > self.max_rows))
        added = want and not full
        kid = self.put(codes, stamp, n_rows) if added else -1
        return dict(added=added, id=kid, full=full, min_diff_all=q["min_diff_all"], n_keyframes=self.K, candidates=q["candidates"])
