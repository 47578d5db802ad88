"""The inputs of the temporal-filter apply tests, built on the host so that tests/test_oracle_tf_apply_inputs.py can check WITHOUT a GPU
what tests/test_gpu_tf_apply.py then relies on: that the pixel weights, weight = (int)(exp(-scaled_error) * 1000), really vary on them.
A case whose predictors are all far from the source has weight 0 everywhere, returns the source frame and pins nothing.

Families:
  legacy  the five rows the GPU test has always had (smooth content, random MVs of up to +-15 px): frames that are no multiple of 32, an
          absent frame, the full-pel / x-only / y-only copy paths.  Nearly all of their weights are 0.
  flat    a constant level + uniform noise of +-(4 << (bd - 8)) per pixel; random MVs of +-120 eighth-pels (all 64 phases, lengths on both
          sides of 0.1 * min(W, H)); sub-block MSEs in 0 .. 48 << (bd - 8).  Every MV gives a small error that varies per pixel, and the
          noise being per pixel, a wrong tap or phase of the predictor changes the result.
  track   shifted_smooth_pair content that moves by a fixed sub-pel velocity per frame; every sub-block MV is the true displacement
          against the frame to filter + a jitter of +-4 eighth-pels: the predictor on real gradients, both sub-pel axes active.
  branch  one small flat case per branch of the per-call factors: q_factor 127 / 128 (either side of the cutoff), filter_strength 0 (the
          1e-5 clamp: every weight 0), a large strength with a large noise level, the frame to filter first in its window."""
import functools

import numpy as np

F, BORDER = 5, 96


class Case:
    def __init__(self, name, family, W, H, bd, planes, ssx, ssy, q, strength, noise, filt=2):
        self.name, self.family, self.W, self.H, self.bd, self.planes, self.ssx, self.ssy = name, family, W, H, bd, planes, ssx, ssy
        self.q, self.strength, self.noise, self.filt, self.F, self.border = q, strength, noise, filt, F, BORDER
        self.mb_rows, self.mb_cols = (H + 31) // 32, (W + 31) // 32
        self.n = self.mb_rows * self.mb_cols
        self.present = np.ones(F, np.uint8)
        self.frames = self.mvs = self.mses = None    # frames[p][f]: the visible plane

    def plane_size(self, p):
        return ((self.W + self.ssx) >> self.ssx, (self.H + self.ssy) >> self.ssy) if p else (self.W, self.H)

    def covered(self, p):
        """(rows, columns) of plane p that the 32x32 blocks cover"""
        sx, sy = (self.ssx, self.ssy) if p else (0, 0)
        return (self.mb_rows * 32) >> sy, (self.mb_cols * 32) >> sx

    def __repr__(self):
        return self.name


def _dtype(bd):
    return np.uint8 if bd == 8 else np.uint16


LEGACY = [(160, 96, 8, 3, 1, 1, 40, 5), (176, 112, 10, 3, 1, 1, 160, 2), (128, 72, 10, 1, 0, 0, 20, 4), (96, 64, 12, 3, 0, 0, 64, 6),
          (200, 120, 8, 1, 0, 0, 255, 1)]


def _legacy(hip, W, H, bd, planes, ssx, ssy, q, strength):
    c = Case("legacy-%dx%d-%db-%dp" % (W, H, bd, planes), "legacy", W, H, bd, planes, ssx, ssy, q, strength, [1.7, 0.8, 1.2])
    rng = np.random.default_rng(W + 7 * bd + planes)
    wrng = np.random.default_rng(W * 3 + bd)
    c.frames = []
    for p in range(planes):
        w, h = c.plane_size(p)
        fr = []
        for f in range(F):
            base = hip.synth.shifted_smooth_pair(w, h, 3 * p + 1, bd, shift=(f, 2 * f), frac8=(0, 0))[1].astype(np.int64)
            fr.append(np.clip(base + wrng.integers(-(3 << (bd - 8)), (3 << (bd - 8)) + 1, base.shape), 0, (1 << bd) - 1).astype(_dtype(bd)))
        c.frames.append(fr)
    n = c.n
    mvs = rng.integers(-120, 121, (F, n, 4, 2)).astype(np.int16)     # 1/8 pel: up to +-15 pixels, every phase
    mvs[:, ::3] = (mvs[:, ::3] // 8) * 8                             # some full-pel vectors (the copy path), some half-aligned ones
    mvs[:, 1::5, :, 0] = (mvs[:, 1::5, :, 0] // 8) * 8              # x-only
    mvs[:, 2::7, :, 1] = (mvs[:, 2::7, :, 1] // 8) * 8              # y-only
    mses = (rng.integers(0, 90, (F, n, 4)) << (bd - 8)).astype(np.int32)
    mses[:, ::4] = rng.integers(0, 6, (F, (n + 3) // 4, 4))
    mvs[c.filt] = 0; mses[c.filt] = 2147483647
    c.mvs, c.mses = mvs, mses
    c.present[F - 1] = 0                                             # one absent frame
    return c


def _flat(name, family, seed, bd, planes, ssx, ssy, q, strength, noise, filt=2, W=96, H=64):
    c = Case(name, family, W, H, bd, planes, ssx, ssy, q, strength, noise, filt)
    rng = np.random.default_rng(seed)
    amp = 4 << (bd - 8)
    c.frames = []
    for p in range(planes):
        w, h = c.plane_size(p)
        level = ((1 << bd) * (5, 3, 6)[p]) >> 3
        c.frames.append([(level + rng.integers(-amp, amp + 1, (h, w))).astype(_dtype(bd)) for _ in range(F)])
    # random within +-120 and 0 .. 48 << (bd - 8), but not uniformly: a uniform draw makes nearly every vector longer than the distance
    # threshold (6.4 eighth-pels here) and d_factor == 1 all but absent.  A component is 8 * k + phase: the 64 phase pairs are dealt out
    # in turn (shuffled), as -3 .. 4, and each sub-block draws its own reach R for k in -R .. R; R == 0 keeps the vector below 6.4.
    pair = rng.permutation((F - 1) * c.n * 4) % 64          # over the four other frames' 4 n = 96 sub-blocks: every pair at least once
    phase = np.stack([pair >> 3, pair & 7], axis=-1).reshape(F - 1, c.n, 4, 2)
    phase = np.where(phase > 4, phase - 8, phase)
    reach = rng.choice([0, 0, 1, 3, 14], (F - 1, c.n, 4, 1))
    c.mvs = np.insert(8 * rng.integers(-reach, reach + 1, (F - 1, c.n, 4, 2)) + phase, filt, 0, axis=0).astype(np.int16)
    c.mses = rng.integers(0, ((48 << (bd - 8)) >> rng.integers(0, 7, (F, c.n, 4))) + 1).astype(np.int32)
    c.mvs[filt] = 0; c.mses[filt] = 2147483647
    return c


def _track(hip, name, seed, bd, planes, ssx, ssy, q, strength, noise, W=96, H=64, filt=2):
    """Frame f of the luma plane is the content displaced by f * (2, -4) eighth-pels (x, y); a chroma plane by that >> its subsampling,
    in its own pixels.  shifted_smooth_pair's second image is its content displaced by shift + frac8 / 8: ref[y, x] = src[y - dy, x - dx].
    The predictor of a block reads frame f at (y + mv_row, x + mv_col), so it meets the frame to filter where
    mv = displacement(f) - displacement(filt).  The oracle's statistics settle the sign: with it the mean luma weight is about 400 and
    1 % of the weights are 0, with the opposite one about 65 and 50 % (test_oracle_tf_apply_inputs.py asserts the comparison).  The
    velocity is small because d_factor grows with the vector's length in EIGHTH-pels against 0.1 * min(W, H) = 6.4: the neighbours of the
    frame to filter stay below it, the outer frames exceed it."""
    c = Case(name, "track", W, H, bd, planes, ssx, ssy, q, strength, noise, filt)
    rng = np.random.default_rng(seed)
    vx8, vy8 = 2, -4
    amp = 2 << (bd - 8)
    c.frames = []
    for p in range(planes):
        w, h = c.plane_size(p)
        sx, sy = (ssx, ssy) if p else (0, 0)
        fr = []
        for f in range(F):
            dx8, dy8 = (vx8 * f) >> sx, (vy8 * f) >> sy
            base = hip.synth.shifted_smooth_pair(w, h, 3 * p + 1, bd, shift=(dx8 // 8, dy8 // 8), frac8=(dx8 % 8, dy8 % 8))[1].astype(np.int64)
            fr.append(np.clip(base + rng.integers(-amp, amp + 1, base.shape), 0, (1 << bd) - 1).astype(_dtype(bd)))
        c.frames.append(fr)
    mvs = np.empty((F, c.n, 4, 2), np.int16)
    for f in range(F):
        mvs[f, :, :, 0] = vy8 * (f - filt)
        mvs[f, :, :, 1] = vx8 * (f - filt)
    mvs += rng.integers(-4, 5, mvs.shape).astype(np.int16)
    c.mses = rng.integers(0, (6 << (bd - 8)) + 1, (F, c.n, 4)).astype(np.int32)
    mvs[filt] = 0; c.mses[filt] = 2147483647
    c.mvs = mvs
    return c


@functools.lru_cache(maxsize=None)
def _all(hip):
    cases = [_legacy(hip, *row) for row in LEGACY]
    cases += [
        _flat("flat-420-8b", "flat", 11, 8, 3, 1, 1, 40, 5, [1.7, 0.8, 1.2]),
        _flat("flat-422-10b", "flat", 12, 10, 3, 1, 0, 160, 2, [1.7, 0.8, 1.2]),
        _flat("flat-444-12b", "flat", 13, 12, 3, 0, 0, 64, 6, [1.7, 0.8, 1.2]),
        _flat("flat-440-10b", "flat", 14, 10, 3, 0, 1, 200, 4, [2.4, 1.1, 0.6]),
        _flat("flat-luma-12b", "flat", 15, 12, 1, 0, 0, 150, 6, [0.9, 0, 0]),
        _track(hip, "track-420-8b", 21, 8, 3, 1, 1, 40, 5, [1.7, 0.8, 1.2]),
        _track(hip, "track-422-10b", 22, 10, 3, 1, 0, 160, 2, [1.7, 0.8, 1.2]),
        _track(hip, "track-444-12b", 23, 12, 3, 0, 0, 64, 6, [1.7, 0.8, 1.2]),
        _flat("branch-q127", "branch", 31, 8, 3, 1, 1, 127, 4, [1.7, 0.8, 1.2]),
        _flat("branch-q128", "branch", 31, 8, 3, 1, 1, 128, 4, [1.7, 0.8, 1.2]),
        _flat("branch-strength0", "branch", 33, 8, 3, 1, 1, 40, 0, [1.7, 0.8, 1.2]),
        _flat("branch-strong-noisy", "branch", 34, 10, 3, 1, 1, 60, 6, [30.0, 12.0, 20.0]),
        _flat("branch-filter-first", "branch", 35, 8, 3, 1, 1, 40, 5, [1.7, 0.8, 1.2], filt=0),
    ]
    return {c.name: c for c in cases}


NAMES = ["legacy-%dx%d-%db-%dp" % r[:4] for r in LEGACY] + [
    "flat-420-8b", "flat-422-10b", "flat-444-12b", "flat-440-10b", "flat-luma-12b", "track-420-8b", "track-422-10b", "track-444-12b",
    "branch-q127", "branch-q128", "branch-strength0", "branch-strong-noisy", "branch-filter-first"]
NEW_NAMES = [n for n in NAMES if not n.startswith("legacy")]


def case(hip, name):
    return _all(hip)[name]


_REF = {}


def reference(hip, oracle, name):
    """(filtered planes, TfWeightStats) of the oracle for a case, computed once per process; border-extended arrays, not to be modified."""
    if name not in _REF:
        c = case(hip, name)
        host = [[oracle.extend_plane(img, c.border) for img in c.frames[p]] for p in range(c.planes)]
        _REF[name] = oracle.tf_apply_frames(host, c.border, c.W, c.H, c.filt, c.mvs, c.mses, c.noise, c.q, c.strength, bd=c.bd, ss_x=c.ssx,
                                            ss_y=c.ssy, present=c.present, stats=True)
    return _REF[name]


def assert_weights_matter(c, st):
    """The conditions a case must meet before a comparison on it means anything -- from the oracle's statistics alone."""
    assert not any(t.any() for t in st.near_tie), (c.name, [int(t.sum()) for t in st.near_tie], st.min_tie_ulps)
    if c.family in ("flat", "track"):
        for p in range(c.planes):
            assert 2 * st.mid[p] >= st.total[p], (c.name, p, st.summary())
        assert (st.buckets[0] > 0).all(), (c.name, st.summary())
    if c.name == "branch-strength0":
        assert (st.zero == st.total).all(), (c.name, st.summary())
