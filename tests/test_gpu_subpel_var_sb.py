"""aomhip_sub_pixel_variance_sb_batch (csrc/subpel_var_sb.hip: sub-pixel variance out of the LDS strip walk) == oracle
aom_sub_pixel_varianceWxH / aom_highbd_{10,12}_sub_pixel_varianceWxH (aom_dsp/variance.c:91-163,475-561), bit-exact: the 14 block sizes up to
32x32 at 8/10/12 bits with ragged cells and entries beyond the declared range, all 64 (xoff, yoff) pairs including entries at exactly +-range,
the reference's own golden rows, the whole 1080p / 4K Mode-A lists against the direct kernel, the extreme planes, frame edges, refusals and
untouched output tails -- and the staged path is really the one taken (aomhip_debug_subpel_sb_fallbacks)."""
import json
import os

import numpy as np
import pytest

from test_gpu_sad_sb import _lists
from test_gpu_variance_sb import _var_cands

pytestmark = pytest.mark.gpu
SIZES = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (4, 16), (16, 4), (8, 32), (32, 8)]
GUARD = 64   # uint32 elements behind each output array that must stay untouched


def _run(hip, ctx, ps, pr, frame, nf, bw, bh, sbw, sbh, search, vc, W, H, per_frame=False):
    """vc: (n,) shared list or (nf, n) per-frame lists (same source blocks in every frame).  -> bucketed list(s), var, sse, fallbacks"""
    first = vc[0] if per_frame else vc
    perm, off = hip.synth.bucket_order(first["sx"], first["sy"], W, H, sbw, sbh)
    n = len(perm)
    vs = np.ascontiguousarray(vc[:, perm] if per_frame else vc[perm])
    d_c, d_o = ctx.to_device(vs), ctx.to_device(off)
    nbytes = (nf * n + GUARD) * 4
    d_v, d_s = ctx.malloc(nbytes), ctx.malloc(nbytes)
    ctx.memset(d_v, 0xff, nbytes); ctx.memset(d_s, 0xff, nbytes)
    ctx.sub_pixel_variance_sb_batch(ps, pr, frame, nf, bw, bh, sbw, sbh, search, len(off) - 1, d_c, d_o, n, n if per_frame else 0, d_v, d_s)
    fb = ctx.debug_subpel_sb_fallbacks()
    v, s = ctx.from_device(d_v, (nf * n + GUARD,), np.uint32), ctx.from_device(d_s, (nf * n + GUARD,), np.uint32)
    for d in (d_c, d_o, d_v, d_s):
        ctx.free(d)
    assert np.all(v[nf * n:] == 0xFFFFFFFF) and np.all(s[nf * n:] == 0xFFFFFFFF), "wrote behind the outputs"
    return vs, v[:nf * n].reshape(nf, n), s[:nf * n].reshape(nf, n), fb


def _pair(hip, oracle, ctx, W, H, border, bd, src, ref, frames=1, at=0):
    ps, pr = ctx.planes_alloc(W, H, border, bd, frames), ctx.planes_alloc(W, H, border, bd, frames)
    ctx.planes_upload(ps, at, src); ctx.planes_upload(pr, at, ref)
    return ps, pr, oracle.extend_plane(src, border, ps.stride), oracle.extend_plane(ref, border, pr.stride)


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("w,h", SIZES)
def test_block_sizes_and_bit_depths(hip, oracle, ctx, w, h, bd):
    rng = np.random.default_rng(w * 19 + h * 5 + bd)
    W, H, border, search = 400, 272, 160, 32   # not multiples of the 128-wide cell: ragged last column / row of cells
    src = hip.synth.lcg_frame(W, H, 1, 0, bd); ref = hip.synth.lcg_frame(W, H, 2, 1, bd)
    ps, pr, sb, rb = _pair(hip, oracle, ctx, W, H, border, bd, src, ref, frames=2, at=1)
    cands, groups = _lists(hip, rng, W, H, w, h, 24)
    if len(groups) > 59:
        keep = np.sort(rng.choice(len(groups), 59, replace=False)); cands, groups = cands[keep], groups[keep]
    vc = _var_cands(hip, groups, cands)                       # <= 295 entries, every one within 24 <= range of its block
    n_far = 5                                                 # ... except these: 200 pixels away, beyond cell + range on either side
    far = rng.choice(len(vc), n_far, replace=False)
    vc["rx"][far] = np.where(vc["sx"][far] < 200, vc["sx"][far] + 200, vc["sx"][far] - 200)
    off = rng.integers(0, 64, len(vc))
    vc["xoff"], vc["yoff"] = off & 7, off >> 3
    sbw, sbh = (128, 32) if bd > 8 else (128, 64)
    vs, v, s, fb = _run(hip, ctx, ps, pr, 1, 1, w, h, sbw, sbh, search, vc, W, H)
    want = oracle.variance_cands(sb, rb, border, w, h, vs, subpel=True, bd=bd)
    assert np.array_equal(v[0], want[:, 0]) and np.array_equal(s[0], want[:, 1]), (w, h, bd)
    assert fb == n_far, "entries served from global memory: %d, deliberately far: %d" % (fb, n_far)
    ctx.planes_free(ps); ctx.planes_free(pr)


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("w,h", [(16, 16), (8, 8)])
def test_all_64_offsets_including_entries_at_the_range_limit(hip, oracle, ctx, w, h, bd):
    rng = np.random.default_rng(w + bd)
    W, H, border, search = 256, 192, 160, 32
    sbw, sbh = 128, 64
    src = hip.synth.lcg_frame(W, H, 5, 0, bd); ref = hip.synth.lcg_frame(W, H, 6, 1, bd)
    ps, pr, sb, rb = _pair(hip, oracle, ctx, W, H, border, bd, src, ref)
    vc = np.zeros(64 * 5, hip.capi.var_cand_dtype)
    k = np.arange(len(vc))
    vc["xoff"], vc["yoff"] = k & 7, (k >> 3) & 7                  # every pair 5 times
    # source blocks in the corners of their cells, so that +-range from the block is +-range from the cell: the first and the last column /
    # row of the staged window (with the extra column / row of the bilinear taps behind it)
    cx, cy = rng.integers(0, W // sbw, len(vc)), rng.integers(0, H // sbh, len(vc))
    right, low = rng.integers(0, 2, len(vc)).astype(bool), rng.integers(0, 2, len(vc)).astype(bool)
    vc["sx"] = cx * sbw + np.where(right, sbw - w, 0); vc["sy"] = cy * sbh + np.where(low, sbh - h, 0)
    vc["rx"] = vc["sx"] + rng.integers(-search, search + 1, len(vc)); vc["ry"] = vc["sy"] + rng.integers(-search, search + 1, len(vc))
    lim = k < 64 * 4                                              # four of the five rounds sit exactly on the limit in x, y or both
    rnd = k >> 6
    vc["rx"] = np.where(lim & (rnd != 1), vc["sx"] + np.where(right, search, -search), vc["rx"])
    vc["ry"] = np.where(lim & (rnd != 0), vc["sy"] + np.where(low, search, -search), vc["ry"])
    vs, v, s, fb = _run(hip, ctx, ps, pr, 0, 1, w, h, sbw, sbh, search, vc, W, H)
    pairs = set(zip(vs["xoff"].tolist(), vs["yoff"].tolist()))
    assert len(pairs) == 64 and min(np.bincount(vs["xoff"] + 8 * vs["yoff"].astype(int))) >= 4
    want = oracle.variance_cands(sb, rb, border, w, h, vs, subpel=True, bd=bd)
    assert np.array_equal(v[0], want[:, 0]) and np.array_equal(s[0], want[:, 1])
    assert fb == 0, "an entry at +-range was not served from the staged window"
    ctx.planes_free(ps); ctx.planes_free(pr)


def test_reference_golden_rows(hip, ctx):
    """tests/golden/ref_eval_sadvar.npz: plane `a` is the interpolated operand, `b` the compared one (test_gpu_goldens.py)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_eval_sadvar.npz"))
    rows = [r for r in json.loads(bytes(z["cases"]).decode()) if not r.get("extra")]
    expected = sum(len(r.get("subpel", [])) for r in rows if (r["w"], r["h"]) in SIZES)
    assert expected > 0
    checked = 0
    for bd in (8, 10, 12):
        a = z["a%d" % bd].astype(np.uint8 if bd == 8 else np.uint16); b = z["b%d" % bd].astype(a.dtype)
        H, W = a.shape
        ps, pr = ctx.planes_alloc(W, H, 32, bd, 1), ctx.planes_alloc(W, H, 32, bd, 1)
        ctx.planes_upload(ps, 0, b); ctx.planes_upload(pr, 0, a)
        for r in rows:
            if r["bd"] != bd or not r.get("subpel") or r["w"] > 32 or r["h"] > 32:
                continue
            sp = r["subpel"]
            vc = np.zeros(len(sp), hip.capi.var_cand_dtype)
            vc["sx"], vc["sy"], vc["rx"], vc["ry"] = r["rx"], r["ry"], r["ox"], r["oy"]
            vc["xoff"], vc["yoff"] = [q[0] for q in sp], [q[1] for q in sp]
            vs, v, s, fb = _run(hip, ctx, ps, pr, 0, 1, r["w"], r["h"], W, H, 8, vc, W, H)   # one cell covers the plane
            assert v[0].tolist() == [q[2] for q in sp] and s[0].tolist() == [q[3] for q in sp], r
            assert fb == 0
            checked += len(sp)
        ctx.planes_free(ps); ctx.planes_free(pr)
    assert checked >= expected, (checked, expected)


def _mode_a(hip, W, H, F, seed_offsets):
    cands, groups = hip.synth.mode_a_worklist(W, H, 16, seed=3, search=64)
    nb = len(cands)
    vc = np.zeros((F, nb, 5), hip.capi.var_cand_dtype)
    vc["sx"], vc["sy"] = cands["sx"][None, :, None], cands["sy"][None, :, None]
    vc["rx"][:, :, 0], vc["ry"][:, :, 0] = cands["rx"][None], cands["ry"][None]
    vc["rx"][:, :, 1:], vc["ry"][:, :, 1:] = groups["rx"][None], groups["ry"][None]
    off = np.random.default_rng(seed_offsets).integers(1, 64, (F, nb, 5))    # (xoff, yoff) != (0, 0), as benchlib/variance.py draws them
    vc["xoff"], vc["yoff"] = off & 7, off >> 3
    return vc.reshape(F, nb * 5)


@pytest.mark.parametrize("W,H,bd,F,cell", [(1920, 1080, 8, 2, (240, 64)), (3840, 2160, 10, 1, (160, 32))])
def test_whole_mode_a_list_against_the_direct_kernel(hip, ctx, W, H, bd, F, cell):
    border = 160
    ps, pr = ctx.planes_alloc(W, H, border, bd, F), ctx.planes_alloc(W, H, border, bd, F)
    for f in range(F):
        ctx.planes_upload(ps, f, hip.synth.lcg_frame(W, H, 2 * f, 0, bd)); ctx.planes_upload(pr, f, hip.synth.lcg_frame(W, H, 2 * f + 1, 0, bd))
    vc = _mode_a(hip, W, H, F, 4242)
    vs, v, s, fb = _run(hip, ctx, ps, pr, 0, F, 16, 16, cell[0], cell[1], 64, vc, W, H, per_frame=True)
    n = vs.shape[1]
    d_c, d_v, d_s = ctx.to_device(vs), ctx.malloc(F * n * 4), ctx.malloc(F * n * 4)
    ctx.variance_batch(ps, pr, 0, F, 16, 16, d_c, n, n, d_v, d_s, subpel=True)
    dv, ds = ctx.from_device(d_v, (F, n), np.uint32), ctx.from_device(d_s, (F, n), np.uint32)
    assert np.array_equal(v, dv) and np.array_equal(s, ds)
    # every Mode-A entry lies within +-64 of its block, hence of its cell: none may have come from global memory
    assert fb == 0
    for d in (d_c, d_v, d_s):
        ctx.free(d)
    ctx.planes_free(ps); ctx.planes_free(pr)


@pytest.mark.parametrize("flip", [False, True])
def test_extreme_planes_32x32_12bit(hip, oracle, ctx, flip):
    """source all zero against reference all 4095 (and the reverse) at 32x32: sse = 1024 x 4095^2 > 2^32, the widest sums of the family"""
    rng = np.random.default_rng(7)
    W, H, border, bd = 256, 128, 64, 12
    lo, hi = np.zeros((H, W), np.uint16), np.full((H, W), 4095, np.uint16)
    src, ref = (hi, lo) if flip else (lo, hi)
    ps, pr, sb, rb = _pair(hip, oracle, ctx, W, H, border, bd, src, ref)
    cands, groups = _lists(hip, rng, W, H, 32, 32, 16, border=border)
    vc = _var_cands(hip, groups, cands)
    off = rng.integers(0, 64, len(vc))
    vc["xoff"], vc["yoff"] = off & 7, off >> 3
    vs, v, s, fb = _run(hip, ctx, ps, pr, 0, 1, 32, 32, 128, 32, 16, vc, W, H)
    want = oracle.variance_cands(sb, rb, border, 32, 32, vs, subpel=True, bd=bd)
    assert np.array_equal(v[0], want[:, 0]) and np.array_equal(s[0], want[:, 1])
    assert int(want[:, 1].max()) == (1024 * 4095 * 4095 + 128) >> 8 and fb == 0
    ctx.planes_free(ps); ctx.planes_free(pr)


def test_frame_edges_and_an_empty_bucket(hip, oracle, ctx):
    rng = np.random.default_rng(11)
    W, H, border, bd, w, h, search = 256, 192, 160, 8, 16, 16, 64
    sbw, sbh = 128, 64
    src = hip.synth.lcg_frame(W, H, 7, 0, bd); ref = hip.synth.lcg_frame(W, H, 8, 1, bd)
    ps, pr, sb, rb = _pair(hip, oracle, ctx, W, H, border, bd, src, ref)
    bx, by = np.meshgrid(np.arange(0, W, w), np.arange(0, H, h))
    bx, by = bx.ravel(), by.ravel()
    edge = (bx == 0) | (by == 0) | (bx == W - w) | (by == H - h)
    bx, by = bx[edge], by[edge]
    vc = np.zeros(len(bx), hip.capi.var_cand_dtype)
    vc["sx"], vc["sy"] = bx, by
    # footprints pushed a full `range` outwards: into the left / top / right / bottom border
    vc["rx"] = bx + np.where(bx == 0, -search, np.where(bx == W - w, search, 0))
    vc["ry"] = by + np.where(by == 0, -search, np.where(by == H - h, search, 0))
    off = rng.integers(0, 64, len(vc))
    vc["xoff"], vc["yoff"] = off & 7, off >> 3
    for drop_middle in (False, True):
        cur = vc[~((vc["sx"] < sbw) & (vc["sy"] // sbh == 1))] if drop_middle else vc   # bucket 2 of 6 empty, its neighbours full
        vs, v, s, fb = _run(hip, ctx, ps, pr, 0, 1, w, h, sbw, sbh, search, cur, W, H)
        want = oracle.variance_cands(sb, rb, border, w, h, vs, subpel=True, bd=bd)
        assert np.array_equal(v[0], want[:, 0]) and np.array_equal(s[0], want[:, 1])
        assert fb == 0
    ctx.planes_free(ps); ctx.planes_free(pr)


def test_crowded_bucket_goes_through_further_slices(hip, oracle, ctx):
    """4x4 blocks, five entries each, in ONE 128x64 cell: 2560 entries against a slice of at most 1024 -- three slices through the same buffer.
    Every output against the direct kernel, 300 of them against the oracle."""
    rng = np.random.default_rng(13)
    W, H, border, bd, search = 128, 64, 64, 10, 16
    src = hip.synth.lcg_frame(W, H, 9, 0, bd); ref = hip.synth.lcg_frame(W, H, 10, 1, bd)
    ps, pr, sb, rb = _pair(hip, oracle, ctx, W, H, border, bd, src, ref)
    bx, by = np.meshgrid(np.arange(0, W, 4), np.arange(0, H, 4))
    vc = np.zeros(bx.size * 5, hip.capi.var_cand_dtype)
    vc["sx"], vc["sy"] = np.repeat(bx.ravel(), 5), np.repeat(by.ravel(), 5)
    vc["rx"] = vc["sx"] + rng.integers(-search, search + 1, len(vc)); vc["ry"] = vc["sy"] + rng.integers(-search, search + 1, len(vc))
    off = rng.integers(0, 64, len(vc))
    vc["xoff"], vc["yoff"] = off & 7, off >> 3
    vs, v, s, fb = _run(hip, ctx, ps, pr, 0, 1, 4, 4, 128, 64, search, vc, W, H)
    assert len(vs) == 2560 and ctx.debug_subpel_sb_launch_info()["slice_entries"] <= 1024 and fb == 0
    d_c, d_v, d_s = ctx.to_device(vs), ctx.malloc(len(vs) * 4), ctx.malloc(len(vs) * 4)
    ctx.variance_batch(ps, pr, 0, 1, 4, 4, d_c, len(vs), 0, d_v, d_s, subpel=True)
    assert np.array_equal(v[0], ctx.from_device(d_v, (len(vs),), np.uint32)) and np.array_equal(s[0], ctx.from_device(d_s, (len(vs),), np.uint32))
    pick = np.sort(rng.choice(len(vs), 300, replace=False))
    want = oracle.variance_cands(sb, rb, border, 4, 4, vs[pick], subpel=True, bd=bd)
    assert np.array_equal(v[0][pick], want[:, 0]) and np.array_equal(s[0][pick], want[:, 1])
    for d in (d_c, d_v, d_s):
        ctx.free(d)
    ctx.planes_free(ps); ctx.planes_free(pr)


@pytest.mark.parametrize("bd,sbw", [(8, 16), (10, 8), (12, 8), (8, 32), (10, 16)])
@pytest.mark.parametrize("w,h", [(16, 16), (8, 8), (4, 4)])
def test_cells_of_one_or_two_16_byte_chunks(hip, oracle, ctx, bd, sbw, w, h):
    """a source cell one 16-byte chunk wide (sb_w = 16 at 8 bits, 8 at 10/12 bits) and the next width up: every block that fits its cell is
    served from LDS, with the right source rows"""
    rng = np.random.default_rng(bd * 100 + sbw + w)
    W, H, border, search, sbh = 64, 48, 32, 8, 16
    src = hip.synth.lcg_frame(W, H, 11, 0, bd); ref = hip.synth.lcg_frame(W, H, 12, 1, bd)
    ps, pr, sb, rb = _pair(hip, oracle, ctx, W, H, border, bd, src, ref)
    bx, by = np.meshgrid(np.arange(0, W, w), np.arange(0, H, h))
    vc = np.zeros(bx.size * 3, hip.capi.var_cand_dtype)
    vc["sx"], vc["sy"] = np.repeat(bx.ravel(), 3), np.repeat(by.ravel(), 3)
    vc["rx"] = vc["sx"] + rng.integers(-search, search + 1, len(vc)); vc["ry"] = vc["sy"] + rng.integers(-search, search + 1, len(vc))
    off = rng.integers(0, 64, len(vc))
    vc["xoff"], vc["yoff"] = off & 7, off >> 3
    vs, v, s, fb = _run(hip, ctx, ps, pr, 0, 1, w, h, sbw, sbh, search, vc, W, H)
    want = oracle.variance_cands(sb, rb, border, w, h, vs, subpel=True, bd=bd)
    assert np.array_equal(v[0], want[:, 0]) and np.array_equal(s[0], want[:, 1]), (bd, sbw, w, h)
    if w <= sbw:   # (a block wider than its cell is outside the contract: right from wherever it is served)
        assert fb == 0
    ctx.planes_free(ps); ctx.planes_free(pr)


def test_refusals_and_the_empty_list(hip, ctx):
    capi = hip.capi
    ps, pr = ctx.planes_alloc(128, 128, 64, 8, 1), ctx.planes_alloc(128, 128, 64, 8, 1)
    d = ctx.malloc(4096)
    ctx.memset(d, 0xff, 4096)
    off = ctx.to_device(np.zeros(2, np.int32))
    ctx.sub_pixel_variance_sb_batch(ps, pr, 0, 1, 16, 16, 128, 128, 16, 1, None, off, 0, 0, d, d)     # n_cands = 0: a no-op
    assert np.all(ctx.from_device(d, (1024,), np.uint32) == 0xFFFFFFFF)
    with pytest.raises(capi.AomHipError, match="aomhip_sub_pixel_variance_batch"):
        ctx.sub_pixel_variance_sb_batch(ps, pr, 0, 1, 64, 64, 128, 128, 16, 1, d, off, 1, 0, d, d)
    with pytest.raises(capi.AomHipError):
        ctx.sub_pixel_variance_sb_batch(ps, pr, 0, 1, 16, 16, 128, 128, 16, 1, d, off, 1, 0, d, None)     # no sse array
    with pytest.raises(capi.AomHipError):
        ctx.sub_pixel_variance_sb_batch(ps, pr, 0, 1, 16, 16, 128, 128, 16, 1, None, off, 1, 0, d, d)     # entries without a list
    with pytest.raises(capi.AomHipError, match="n_buckets"):
        ctx.sub_pixel_variance_sb_batch(ps, pr, 0, 1, 16, 16, 64, 64, 16, 1, d, off, 1, 0, d, d)          # 4 cells, not 1
    with pytest.raises(capi.AomHipError, match="160 KB"):
        ctx.sub_pixel_variance_sb_batch(ps, pr, 0, 1, 16, 16, 128, 128, 256, 1, d, off, 1, 0, d, d)       # a 641 x 641 window
    odd = capi.Planes.from_buffer_copy(ps)
    odd.stride += 4                                                                                        # rows off the 16-byte grid
    with pytest.raises(capi.AomHipError, match="16-byte"):
        ctx.sub_pixel_variance_sb_batch(odd, pr, 0, 1, 16, 16, 128, 128, 16, 1, d, off, 1, 0, d, d)
    ctx.free(d); ctx.free(off)
    ctx.planes_free(ps); ctx.planes_free(pr)
