"""The strip walk of aomhip_sad_sb_batch / aomhip_variance_sb_batch (csrc/sad_sb.hip) ACROSS ITEM BOUNDARIES == oracle, bit-exact.

A workgroup walks its (frame, strip) items one after the other, and an item's first window arrives through the loaders' pipeline as fill
positions in front of its cells.  The other small tests give every workgroup a single item; here AOMHIP_SB_GRID=8 (read per launch, like
AOMHIP_SB_DESC_CAP) leaves eight workgroups, so each one walks several items: odd and even cell_rows, first windows of one to five batches, rings that
are no multiple of the cell height, the non-affine frame mapping with inactive strips and empty cells, a plane lower than one cell, a first
window clipped by the plane's bottom, crowded buckets in cell 0 of a later item, 16-bit planes, a skip form, a block size without mirror
rows, the variance form and per-frame lists."""
import numpy as np
import pytest

from test_gpu_sad_sb import _lists, _run
from test_gpu_variance_sb import _run as _run_var, _var_cands

pytestmark = pytest.mark.gpu
W, H, BORDER, F = 704, 416, 160, 16


@pytest.fixture(autouse=True)
def _eight_workgroups(monkeypatch):
    monkeypatch.setenv("AOMHIP_SB_GRID", "8")


@pytest.fixture(scope="module")
def ring8(hip, oracle, ctx):
    """16 distinct 8-bit frame pairs (the affine mapping: frames f and f + 8 go to the same workgroups) and their bordered copies."""
    ps, pr = ctx.planes_alloc(W, H, BORDER, 8, F), ctx.planes_alloc(W, H, BORDER, 8, F)
    ext = []
    for f in range(F):
        s, r = hip.synth.lcg_frame(W, H, 40 + f, 0, 8), hip.synth.lcg_frame(W, H, 80 + f, 1, 8)
        ctx.planes_upload(ps, f, s); ctx.planes_upload(pr, f, r)
        ext.append((oracle.extend_plane(s, BORDER, ps.stride), oracle.extend_plane(r, BORDER, pr.stride)))
    yield ps, pr, ext
    ctx.planes_free(ps); ctx.planes_free(pr)


def _check_sad(oracle, ext, out4, out1, gs, cs, bw, bh, border=BORDER, skip=False, bd=8):
    for f, (sb, rb) in enumerate(ext):
        assert np.array_equal(out4[f], oracle.sad_x4d_batch(sb, rb, border, bw, bh, gs, skip=skip, bd=bd)), f
        assert np.array_equal(out1[f], oracle.sad_batch(sb, rb, border, bw, bh, cs, skip=skip, bd=bd)), f


@pytest.mark.parametrize("sbw,sbh,search", [(240, 64, 64), (96, 48, 64), (48, 80, 20), (128, 128, 0), (640, 16, 64)])
def test_affine_frames_several_items_per_workgroup(hip, oracle, ctx, ring8, sbw, sbh, search):
    """cell_rows 7 / 9 / 6 / 4 / 26; first windows of 192 / 176 / 120 / 128 / 144 rows, which come in as 3 / 2 / 1 / 1 / 5 batches, so 10 / 11 / 7 /
    5 / 31 positions per item (an odd count ends in a position without a request); rings of 256 / 224 / 200 / 256 / 160 rows, of which 224 and
    200 are no multiple of the cell height (48, 80)."""
    ps, pr, ext = ring8
    rng = np.random.default_rng(sbw * 7 + sbh + search)
    cands, groups = _lists(hip, rng, W, H, 16, 16, max(search, 1), n_extra_far=12)
    gs, cs, out4, out1 = _run(hip, ctx, ps, pr, 0, F, 16, 16, 0, sbw, sbh, search, cands, groups, W, H)
    _check_sad(oracle, ext, out4, out1, gs, cs, 16, 16)


@pytest.mark.parametrize("w,h,border,sbw,sbh", [(704, 416, 160, 160, 64), (704, 48, 160, 96, 64), (320, 48, 16, 96, 32)])
def test_seven_frames_partial_lists_low_planes(hip, oracle, ctx, w, h, border, sbw, sbh):
    """n_frames < 8 (items = frame x active strip in plain order over 8 workgroups), buckets emptied as in test_geometries_and_partial_lists
    and one strip emptied altogether; a plane lower than one cell (one position per item behind its fill positions, strips 1, 4 and 7 of 8
    empty); a first window cut off by the bottom of a 16-pixel border.  7 frames x 4 / 5 / 3 active strips = 28 / 35 / 21 items: every
    workgroup walks at least two of them, so each of these shapes is met at an item boundary."""
    rng = np.random.default_rng(w + h + border)
    nf = 7
    ps, pr = ctx.planes_alloc(w, h, border, 8, nf), ctx.planes_alloc(w, h, border, 8, nf)
    ext = []
    for f in range(nf):
        s, r = hip.synth.lcg_frame(w, h, 7 + f, 0, 8), hip.synth.lcg_frame(w, h, 17 + f, 1, 8)
        ctx.planes_upload(ps, f, s); ctx.planes_upload(pr, f, r)
        ext.append((oracle.extend_plane(s, border, ps.stride), oracle.extend_plane(r, border, pr.stride)))
    cands, groups = _lists(hip, rng, w, h, 16, 16, 64, border=border)
    keep = (groups["sx"] // sbw + groups["sy"] // sbh) % 3 != 1
    if h > sbh:
        keep &= groups["sx"] // sbw != 1   # an inactive strip
    cands, groups = cands[keep], groups[keep]
    strips, n_active = -(-w // sbw), len(np.unique(groups["sx"] // sbw))
    assert n_active < strips and nf * n_active >= 2 * 8   # inactive strips, and a second item for every one of the 8 workgroups
    occupied = np.unique(groups["sx"] // sbw + strips * (groups["sy"] // sbh))
    assert h <= sbh or len(occupied) < n_active * -(-h // sbh)   # empty cells inside active strips
    gs, cs, out4, out1 = _run(hip, ctx, ps, pr, 0, nf, 16, 16, 0, sbw, sbh, 64, cands, groups, w, h)
    _check_sad(oracle, ext, out4, out1, gs, cs, 16, 16, border=border)
    ctx.planes_free(ps); ctx.planes_free(pr)


def test_crowded_cell_0_of_a_later_item(hip, oracle, ctx, ring8, monkeypatch):
    """8x8 blocks, 128 x 64 cells, descriptor buffers of 24 entries: the cells of strips 1 and 4 hold 128 groups and 171 candidates, every other
    strip at most 23 -- crowded and plain items alternate in every workgroup, and a crowded item's cell 0 comes in behind its fill positions."""
    monkeypatch.setenv("AOMHIP_SB_DESC_CAP", "24")
    ps, pr, ext = ring8
    rng = np.random.default_rng(91)
    cands, groups = _lists(hip, rng, W, H, 8, 8, 16)
    cands = np.concatenate([cands, cands[::3]])
    cands["rx"] += rng.integers(-8, 9, len(cands)).astype(np.int16)
    thin = lambda a: a[((a["sx"] // 128) % 3 == 1) | ((a["sx"] // 8 + 3 * (a["sy"] // 8)) % 8 == 0)]
    cands, groups = thin(cands), thin(groups)
    pg, og = hip.synth.bucket_order(groups["sx"], groups["sy"], W, H, 128, 64)
    pc, oc = hip.synth.bucket_order(cands["sx"], cands["sy"], W, H, 128, 64)
    for off in (og, oc):
        assert (np.diff(off).reshape(-1, 6)[:, [0, 2, 3, 5]] <= 24).all() and (np.diff(off).reshape(-1, 6)[:, [1, 4]] > 24).all()
    gs, cs = groups[pg], cands[pc]
    d_g, d_c, d_og, d_oc = ctx.to_device(gs), ctx.to_device(cs), ctx.to_device(og), ctx.to_device(oc)
    d_o4, d_o1 = ctx.malloc(F * len(gs) * 16), ctx.malloc(F * len(cs) * 4)
    ctx.sad_sb_batch(ps, pr, 0, F, 8, 8, 0, 128, 64, 16, len(og) - 1, d_g, d_og, len(gs), 0, d_o4, d_c, d_oc, len(cs), 0, d_o1)
    out4, out1 = ctx.from_device(d_o4, (F, len(gs), 4), np.uint32), ctx.from_device(d_o1, (F, len(cs)), np.uint32)
    _check_sad(oracle, ext, out4, out1, gs, cs, 8, 8)
    for d in (d_g, d_c, d_og, d_oc, d_o4, d_o1):
        ctx.free(d)


def test_ten_bit_planes(hip, oracle, ctx):
    w, h, bd = 352, 208, 10
    rng = np.random.default_rng(10)
    ps, pr = ctx.planes_alloc(w, h, BORDER, bd, F), ctx.planes_alloc(w, h, BORDER, bd, F)
    ext = []
    for f in range(F):
        s, r = hip.synth.lcg_frame(w, h, 3 + f, 0, bd), hip.synth.lcg_frame(w, h, 33 + f, 1, bd)
        ctx.planes_upload(ps, f, s); ctx.planes_upload(pr, f, r)
        ext.append((oracle.extend_plane(s, BORDER, ps.stride), oracle.extend_plane(r, BORDER, pr.stride)))
    cands, groups = _lists(hip, rng, w, h, 16, 16, 64, n_extra_far=6)
    gs, cs, out4, out1 = _run(hip, ctx, ps, pr, 0, F, 16, 16, 0, 96, 48, 64, cands, groups, w, h)
    _check_sad(oracle, ext, out4, out1, gs, cs, 16, 16, bd=bd)
    ctx.planes_free(ps); ctx.planes_free(pr)


def test_skip_form(hip, oracle, ctx, ring8):
    ps, pr, ext = ring8
    cands, groups = _lists(hip, np.random.default_rng(5), W, H, 16, 16, 64)
    gs, cs, out4, out1 = _run(hip, ctx, ps, pr, 0, F, 16, 16, 1, 240, 64, 64, cands, groups, W, H)
    _check_sad(oracle, ext, out4, out1, gs, cs, 16, 16, skip=True)


def test_32x32_blocks_without_mirror_rows(hip, oracle, ctx, ring8):
    """blocks higher than the mirrored slots read the ring through the per-row wrap, whatever slot the item's first row landed in"""
    ps, pr, ext = ring8
    cands, groups = _lists(hip, np.random.default_rng(32), W, H, 32, 32, 32)
    gs, cs, out4, out1 = _run(hip, ctx, ps, pr, 0, F, 32, 32, 0, 128, 64, 32, cands, groups, W, H)
    _check_sad(oracle, ext, out4, out1, gs, cs, 32, 32)


def test_variance_form(hip, oracle, ctx, ring8):
    ps, pr, ext = ring8
    cands, groups = _lists(hip, np.random.default_rng(6), W, H, 16, 16, 64)
    gs, cs, v4, s4, v1, s1 = _run_var(hip, ctx, ps, pr, 0, F, 16, 16, 240, 64, 64, cands, groups, W, H)
    n, vc = len(gs), _var_cands(hip, gs, cs)
    for f, (sb, rb) in enumerate(ext):
        want = oracle.variance_cands(sb, rb, BORDER, 16, 16, vc, bd=8)
        assert np.array_equal(v4[f].ravel(), want[:4 * n, 0]) and np.array_equal(s4[f].ravel(), want[:4 * n, 1]), f
        assert np.array_equal(v1[f], want[4 * n:, 0]) and np.array_equal(s1[f], want[4 * n:, 1]), f


def test_per_frame_lists_switch_with_the_item(hip, oracle, ctx, ring8):
    """group_frame_stride / cand_frame_stride != 0: frame f + 8 follows frame f in the same workgroup with lists of its own"""
    ps, pr, ext = ring8
    rng = np.random.default_rng(13)
    per = [_lists(hip, rng, W, H, 16, 16, 64) for _ in range(F)]
    cands = np.concatenate([p[0] for p in per]); groups = np.concatenate([p[1] for p in per])
    gs, cs, out4, out1 = _run(hip, ctx, ps, pr, 0, F, 16, 16, 0, 240, 64, 64, cands, groups, W, H, cfs=1, gfs=1)
    n = len(per[0][0])
    assert not np.array_equal(gs[:n], gs[8 * n:9 * n])
    for f, (sb, rb) in enumerate(ext):
        assert np.array_equal(out4[f], oracle.sad_x4d_batch(sb, rb, BORDER, 16, 16, gs[f * n:(f + 1) * n])), f
        assert np.array_equal(out1[f], oracle.sad_batch(sb, rb, BORDER, 16, 16, cs[f * n:(f + 1) * n])), f
