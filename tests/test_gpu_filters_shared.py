"""What the deblocking and CDEF test files leave open: the one-line deblocking kernels, CDEF planes that hold interior and
frame-edge filter blocks at once (filter, chroma and the strength search on the same planes), and the argument checks of the
plane-taking entry points of deblock.hip and cdef.hip -- every condition listed here is rejected, with nothing written."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- 1. the one-line deblocking kernels ----

def _db_content(rng, W, H, bd):
    mx = (1 << bd) - 1
    base = rng.integers(0, mx // 4, (H // 8 + 1, W // 8 + 1))
    pix = np.kron(base, np.ones((8, 8), np.int64))[:H, :W] + rng.integers(-2, 3, (H, W)) + mx // 3
    return np.clip(pix, 0, mx).astype(np.uint8 if bd == 8 else np.uint16)


def _one_pass(params, passes):
    want = params.copy()
    if passes == 1: want[..., 2:] = 0
    if passes == 2: want[..., :2] = 0
    return want


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("border", [4, 10])
def test_one_line_deblocking_kernels(hip, oracle, ctx, bd, border):
    """deblock_vert_kernel / deblock_horz_kernel (one line of an edge per lane).  aomhip_deblock_plane takes them when the plane does not
    keep 4-pixel groups naturally aligned or its border is below 8: border 4 fails `border >= 8`, border 10 fails `(border & 3) == 0` (and
    puts the origin off its natural alignment).  The test cannot observe which kernels ran; the dispatch condition says so.  72 x 40: two
    64-column workgroups in the horizontal pass, three workgroup rows; multiples of 4 keep the oracle's 4x4 unit walk inside its array."""
    W, H = 72, 40
    rng = np.random.default_rng(16 * bd + border)
    pix = _db_content(rng, W, H, bd)
    # transforms up to 32 x 32: a 40-row plane of 64 x 64 transforms would have no horizontal edge at all
    maps = [(oracle.random_edge_params(rng, W, H, max_log2=5, chroma=False), 0), (oracle.random_edge_params(rng, W, H, max_log2=5, chroma=True), 5)]
    for length, spacing, level in ((4, 1, 63), (6, 2, 32), (8, 2, 8), (14, 4, 32)):
        params = np.zeros((H // 4, W // 4, 4), np.uint8)
        params[:, spacing::spacing, 0] = length; params[:, spacing::spacing, 1] = level
        params[spacing::spacing, :, 2] = length; params[spacing::spacing, :, 3] = level
        maps.append((params, 0))
    p = ctx.planes_alloc(W, H, border, bd, 2)
    for params, sharp in maps:
        d = ctx.to_device(params)
        for passes in (1, 2, 3):
            ctx.planes_upload(p, 1, pix)
            ctx.deblock_plane(p, 1, d, params.shape[1], sharp, passes)
            got = ctx.planes_download(p, 1)[border:border + H, border:border + W]
            want = oracle.deblock_plane(pix, _one_pass(params, passes), sharp, bd, order=0)
            assert np.array_equal(got, want), (bd, border, passes)
            assert not np.array_equal(want, pix)
        ctx.free(d)
    ctx.planes_free(p)


# ---- 2. CDEF: interior and frame-edge filter blocks in one plane ----

LW = LH = 200
DAMPING = 5
STRENGTHS = [(0, 0), (5, 2), (4, 0)]
_cases = {}


def _cdef_content(rng, W, H, bd):
    mx = (1 << bd) - 1
    base = rng.integers(mx // 8, mx - mx // 8, (H // 8 + 1, W // 8 + 1))
    i, j = np.indices((H, W))
    pix = np.kron(base, np.ones((8, 8), np.int64))[:H, :W] + ((i * 3 + j * 5) % 17) * (mx // 255 + 1) + rng.integers(-8, 9, (H, W))
    return np.clip(pix, 0, mx).astype(np.uint8 if bd == 8 else np.uint16)


def _noisy(rng, pix, bd):
    a = 5 << (bd - 8)
    return np.clip(pix.astype(np.int64) + rng.integers(-a, a + 1, pix.shape), 0, (1 << bd) - 1).astype(pix.dtype)


def _case(oracle, bd):
    """200 x 200 luma: a 4 x 4 grid of filter blocks.  Blocks (1..2, 1..2) have their whole 68 x 72 footprint inside the frame, the others
    touch a frame edge (row / column 3 is 8 pixels wide).  Computed once per bit depth and left unchanged."""
    if bd not in _cases:
        rng = np.random.default_rng(700 + bd)
        c = {"luma": _cdef_content(rng, LW, LH, bd)}
        c["pri"] = rng.integers(1, 16, (4, 4)).astype(np.uint8)
        c["sec"] = rng.choice([1, 2, 4], (4, 4)).astype(np.uint8)
        c["sec"][2, 1] = 0   # interior block, clip off
        c["pri"][0, 3] = 0   # edge block, clip off
        c["skip"] = (rng.random((LH // 8, LW // 8)) < 0.25).astype(np.uint8)
        c["want"], c["dir"], c["var"] = oracle.cdef_plane_luma(c["luma"], c["pri"], c["sec"], c["skip"], DAMPING, bd)
        c["source"] = _noisy(rng, c["luma"], bd)
        for xdec, ydec in ((1, 1), (1, 0)):
            ch = _cdef_content(rng, LW >> xdec, LH >> ydec, bd)
            c["chroma", xdec, ydec] = ch
            c["chroma_want", xdec, ydec] = oracle.cdef_plane_chroma(ch, xdec, ydec, c["dir"], c["pri"], c["sec"], c["skip"], DAMPING, bd)
            c["chroma_source", xdec, ydec] = _noisy(rng, ch, bd)
        _cases[bd] = c
    return _cases[bd]


@pytest.mark.parametrize("bd", [8, 10])
def test_cdef_luma_interior_and_edge_blocks(hip, oracle, ctx, bd):
    c = _case(oracle, bd)
    ps, pd = ctx.planes_alloc(LW, LH, 32, bd, 1), ctx.planes_alloc(LW, LH, 32, bd, 2)
    ctx.planes_upload(ps, 0, c["luma"])
    d_pri, d_sec, d_skip = ctx.to_device(c["pri"]), ctx.to_device(c["sec"]), ctx.to_device(c["skip"])
    nb = (LH // 8) * (LW // 8)
    d_dir, d_var = ctx.malloc(nb), ctx.malloc(nb * 4)
    ctx.cdef_luma_plane(ps, 0, pd, 1, d_pri, d_sec, 4, d_skip, DAMPING, d_dir, d_var)
    got = ctx.planes_download(pd, 1)[32:32 + LH, 32:32 + LW]
    gdir, gvar = ctx.from_device(d_dir, (LH // 8, LW // 8), np.uint8), ctx.from_device(d_var, (LH // 8, LW // 8), np.int32)
    ctx.planes_free(ps); ctx.planes_free(pd)
    for d in (d_pri, d_sec, d_skip, d_dir, d_var):
        ctx.free(d)
    assert np.array_equal(gdir, c["dir"]) and np.array_equal(gvar, c["var"])
    assert np.array_equal(got, c["want"])
    for fby, fbx in ((1, 1), (2, 2), (2, 1), (0, 3), (3, 0)):   # interior (clip on, clip off) and edge blocks all filter something
        blk = np.s_[fby * 64:fby * 64 + 64, fbx * 64:fbx * 64 + 64]
        assert not np.array_equal(got[blk], c["luma"][blk]), (fby, fbx)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("xdec,ydec", [(1, 1), (1, 0)])
def test_cdef_chroma_interior_and_edge_blocks(hip, oracle, ctx, bd, xdec, ydec):
    """4:2:0 (100 x 100) and 4:2:2 (100 x 200) chroma of the same frame, fed the oracle's luma directions."""
    c = _case(oracle, bd)
    cw, ch = LW >> xdec, LH >> ydec
    ps, pd = ctx.planes_alloc(cw, ch, 32, bd, 1), ctx.planes_alloc(cw, ch, 32, bd, 2)
    ctx.planes_upload(ps, 0, c["chroma", xdec, ydec])
    d_dir, d_pri, d_sec, d_skip = ctx.to_device(c["dir"]), ctx.to_device(c["pri"]), ctx.to_device(c["sec"]), ctx.to_device(c["skip"])
    ctx.cdef_chroma_plane(ps, 0, pd, 1, xdec, ydec, d_dir, d_pri, d_sec, 4, d_skip, DAMPING)
    got = ctx.planes_download(pd, 1)[32:32 + ch, 32:32 + cw]
    ctx.planes_free(ps); ctx.planes_free(pd)
    for d in (d_dir, d_pri, d_sec, d_skip):
        ctx.free(d)
    assert np.array_equal(got, c["chroma_want", xdec, ydec])
    assert not np.array_equal(got, c["chroma", xdec, ydec])


def _search(ctx, recon, source, bd, d_skip, fb_rows, run):
    H, W = recon.shape
    pr, ps = ctx.planes_alloc(W, H, 32, bd, 1), ctx.planes_alloc(W, H, 32, bd, 1)
    ctx.planes_upload(pr, 0, recon); ctx.planes_upload(ps, 0, source)
    d_st = ctx.to_device(np.asarray(STRENGTHS, np.uint8))
    d_sse = ctx.malloc(8 * len(STRENGTHS) * fb_rows * 4)
    run(pr, ps, d_st, d_sse)
    got = ctx.from_device(d_sse, (len(STRENGTHS), fb_rows, 4), np.uint64)
    ctx.free(d_st); ctx.free(d_sse)
    ctx.planes_free(pr); ctx.planes_free(ps)
    return got


@pytest.mark.parametrize("bd", [8, 10])
def test_cdef_search_interior_and_edge_blocks(hip, oracle, ctx, bd):
    """The strength search on the same planes: (0, 0), (5, 2) and (4, 0), expected sums as in tests/test_gpu_cdef_search.py."""
    c = _case(oracle, bd)
    d_skip, d_ldir = ctx.to_device(c["skip"]), ctx.to_device(c["dir"])
    d_dir = ctx.malloc((LH // 8) * (LW // 8))
    got = _search(ctx, c["luma"], c["source"], bd, d_skip, 4,
                  lambda pr, ps, d_st, d_sse: ctx.cdef_search_sse_luma(pr, 0, ps, 0, d_st, len(STRENGTHS), d_skip, DAMPING, 4, d_sse, d_dir, None))
    assert np.array_equal(ctx.from_device(d_dir, (LH // 8, LW // 8), np.uint8), c["dir"])
    want = oracle.cdef_search_sse_luma(c["luma"], c["source"], STRENGTHS, c["skip"], DAMPING, bd)
    assert np.array_equal(got, want)
    assert (want[1] != want[0]).any() and (want[2] != want[0]).any()
    for xdec, ydec in ((1, 1), (1, 0)):
        recon, source = c["chroma", xdec, ydec], c["chroma_source", xdec, ydec]
        got = _search(ctx, recon, source, bd, d_skip, 4,
                      lambda pr, ps, d_st, d_sse: ctx.cdef_search_sse_chroma(pr, 0, ps, 0, xdec, ydec, d_ldir, d_st, len(STRENGTHS), d_skip,
                                                                             DAMPING, 4, d_sse))
        want = oracle.cdef_search_sse_chroma(recon, source, xdec, ydec, c["dir"], STRENGTHS, c["skip"], DAMPING, bd)
        assert np.array_equal(got, want), (xdec, ydec)
    for d in (d_skip, d_ldir, d_dir):
        ctx.free(d)


# ---- 3. argument checks ----

def _filled(ctx, rng, W, H, border, bd, n_frames=1):
    """A ring whose every byte (borders included) is a known pattern -> (ring, [download of each frame])."""
    p = ctx.planes_alloc(W, H, border, bd, n_frames)
    for f in range(n_frames):
        ctx.planes_upload(p, f, rng.integers(0, 1 << bd, (H, W)))
    return p, [ctx.planes_download(p, f) for f in range(n_frames)]


def _unchanged(ctx, p, before):
    return all(np.array_equal(ctx.planes_download(p, f), b) for f, b in enumerate(before))


def test_deblock_plane_rejects(hip, oracle, ctx):
    K = hip.capi
    rng = np.random.default_rng(31)
    W, H = 72, 40
    params = np.zeros((H // 4, W // 4, 4), np.uint8)
    params[:, 2::2, 0] = 8; params[:, 2::2, 1] = 32
    params[2::2, :, 2] = 8; params[2::2, :, 3] = 32
    d = ctx.to_device(params)
    p, before = _filled(ctx, rng, W, H, 32, 8, 2)
    for args in ((p, 1, d, W // 4, 8, 3),          # sharpness 8
                 (p, 2, d, W // 4, 0, 3),          # frame == n_frames
                 (p, 1, d, W // 4 - 1, 0, 3)):     # units_stride one too small
        with pytest.raises(K.AomHipError):
            ctx.deblock_plane(*args)
    assert _unchanged(ctx, p, before)
    ctx.planes_free(p)
    # border 2: the vertical pass is refused, the horizontal pass alone is accepted
    pix = _db_content(rng, W, H, 10)
    q = ctx.planes_alloc(W, H, 2, 10, 1)
    ctx.planes_upload(q, 0, pix)
    before = [ctx.planes_download(q, 0)]
    with pytest.raises(K.AomHipError):
        ctx.deblock_plane(q, 0, d, W // 4, 0, 3)
    assert _unchanged(ctx, q, before)
    ctx.deblock_plane(q, 0, d, W // 4, 0, 2)
    want = oracle.deblock_plane(pix, _one_pass(params, 2), 0, 10, order=0)
    assert np.array_equal(ctx.planes_download(q, 0)[2:2 + H, 2:2 + W], want) and not np.array_equal(want, pix)
    ctx.planes_free(q); ctx.free(d)


def test_deblock_plane_fused_rejects(hip, ctx):
    K = hip.capi
    rng = np.random.default_rng(32)
    W, H = 72, 40
    d = ctx.to_device(np.full((H // 4, W // 4, 4), 8, np.uint8))
    src, _ = _filled(ctx, rng, W, H, 32, 8, 2)
    dst, before = _filled(ctx, rng, W, H, 32, 8, 1)
    small, _ = _filled(ctx, rng, W, H, 4, 8, 1)
    wide, wide_before = _filled(ctx, rng, W + 8, H, 32, 8, 1)
    deep, deep_before = _filled(ctx, rng, W, H, 32, 10, 1)
    for args in ((src, 1, src, 1),     # the same frame of the same ring
                 (small, 0, dst, 0),   # source border 4
                 (src, 0, wide, 0),    # differing width
                 (src, 0, deep, 0)):   # differing bit depth
        with pytest.raises(K.AomHipError):
            ctx.deblock_plane_fused(*args, d, W // 4, 0)
    assert _unchanged(ctx, dst, before) and _unchanged(ctx, wide, wide_before) and _unchanged(ctx, deep, deep_before)
    for p in (src, dst, small, wide, deep):
        ctx.planes_free(p)
    ctx.free(d)


def test_cdef_plane_rejects(hip, ctx):
    K = hip.capi
    rng = np.random.default_rng(33)
    d = ctx.malloc(4096)
    ctx.memset(d, 0, 4096)
    src, _ = _filled(ctx, rng, 200, 64, 32, 8, 2)
    dst, before = _filled(ctx, rng, 200, 64, 32, 8, 1)
    other, other_before = _filled(ctx, rng, 200, 64, 16, 8, 1)     # same visible geometry, another stride
    assert other.stride != src.stride
    n68, n68_before = _filled(ctx, rng, 68, 64, 32, 8, 2)
    for s, sf, t, tf, fbs, damping in ((n68, 0, n68, 1, 2, 5),     # width 68
                                       (src, 1, src, 1, 4, 5),     # the same frame of the same ring
                                       (src, 0, dst, 0, 4, 2), (src, 0, dst, 0, 4, 7),   # damping
                                       (src, 0, dst, 0, 3, 5),     # fb_stride one too small
                                       (src, 0, other, 0, 4, 5)):  # rings of different strides
        with pytest.raises(K.AomHipError):
            ctx.cdef_luma_plane(s, sf, t, tf, d, d, fbs, d, damping)
    assert _unchanged(ctx, dst, before) and _unchanged(ctx, other, other_before) and _unchanged(ctx, n68, n68_before)
    # chroma: xdec = 2; 66 columns are not whole 4-column blocks of 4:2:0
    c66, _ = _filled(ctx, rng, 66, 32, 32, 8, 2)
    with pytest.raises(K.AomHipError):
        ctx.cdef_chroma_plane(src, 0, dst, 0, 2, 1, d, d, d, 4, d, 5)
    with pytest.raises(K.AomHipError):
        ctx.cdef_chroma_plane(c66, 0, c66, 1, 1, 1, d, d, d, 3, d, 5)
    assert _unchanged(ctx, dst, before)
    for p in (src, dst, other, n68, c66):
        ctx.planes_free(p)
    ctx.free(d)


def test_plane_sse_rejects(hip, ctx):
    K = hip.capi
    rng = np.random.default_rng(34)
    a, _ = _filled(ctx, rng, 72, 40, 16, 8, 1)
    b, _ = _filled(ctx, rng, 72, 44, 16, 8, 1)
    d = ctx.to_device(np.array([0x1122334455667788], np.uint64))
    with pytest.raises(K.AomHipError):
        ctx.plane_sse(a, 0, b, 0, d)
    assert int(ctx.from_device(d, (1,), np.uint64)[0]) == 0x1122334455667788   # not even zeroed
    ctx.plane_sse(a, 0, a, 0, d)
    assert int(ctx.from_device(d, (1,), np.uint64)[0]) == 0
    ctx.planes_free(a); ctx.planes_free(b); ctx.free(d)
