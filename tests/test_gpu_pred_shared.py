"""What the inter-prediction kernels share (csrc/pred_device.h) and no other test pins: the position clamp and its limits, the compound finish on one
input through its three users, the 4- and 8-tap sets through both up-sampling searches at every eighth-pel phase, and every argument check of the
predictor entry points (refused, and nothing written)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, BORDER = 64, 48, 16


# ---- 1. the position clamp ---------------------------------------------------------------------------------------------------------------------

def limits(width, height, border, bw, bh):
    """The rule as written: the 8-pixel row load starts 3 left of the integer position and the walk covers rows -3 .. bh + 3."""
    return (3 - border) << 4, ((width + border - bw - 5) << 4) | 15, (3 - border) << 4, ((height + border - bh - 5) << 4) | 15


def grid_blocks(hip, bw, bh):
    gc, gr = W // bw, H // bh
    n = gc * gr
    blocks = np.zeros(n, hip.capi.search_block_dtype)
    blocks["bx"], blocks["by"] = (np.arange(n) % gc) * bw, (np.arange(n) // gc) * bh
    return blocks


def wild_mvs(rng, blocks, lim, mul, high=True):
    """MVs (row, col) in units of mul sixteenths: the first eight blocks far beyond each side and corner, the ninth inside, the others per axis far low / far high /
    inside / a little beyond either limit.  high=False: nothing beyond the high limits."""
    n = len(blocks)
    x_lo, x_hi, y_lo, y_hi = lim
    far = 4000
    cat = rng.integers(0, 5, (n, 2))
    cat[:9] = [(0, 2), (1, 2), (2, 0), (2, 1), (0, 0), (0, 1), (1, 0), (1, 1), (2, 2)]   # (row, col) category: 0 far low, 1 far high, 2 inside
    if not high:
        cat[(cat == 1) | (cat == 4)] = 3
    mv = np.zeros((n, 2), np.int64)
    for axis, (b, lo, hi) in enumerate(((blocks["by"].astype(np.int64), y_lo, y_hi), (blocks["bx"].astype(np.int64), x_lo, x_hi))):
        c = cat[:, axis]
        near = rng.integers(1, 41, n)
        pos = np.select([c == 0, c == 1, c == 2, c == 3], [b * 16 - far, b * 16 + far, b * 16 + rng.integers(-8 * 16, 8 * 16 + 1, n), lo - near], hi + near)
        mv[:, axis] = (pos - b * 16) // mul
    return mv.astype(np.int16)


def clamped_sixteenths(blocks, mv, mul, lim):
    """-> the sixteenth-pel MV that lands exactly on each block's clamped position, and which blocks were clamped low / high on either axis"""
    x_lo, x_hi, y_lo, y_hi = lim
    px, py = blocks["bx"].astype(np.int64) * 16 + mv[:, 1].astype(np.int64) * mul, blocks["by"].astype(np.int64) * 16 + mv[:, 0].astype(np.int64) * mul
    cx, cy = np.clip(px, x_lo, x_hi), np.clip(py, y_lo, y_hi)
    out = np.stack([cy - blocks["by"] * 16, cx - blocks["bx"] * 16], 1).astype(np.int16)
    sides = {"left": px < x_lo, "right": px > x_hi, "top": py < y_lo, "bottom": py > y_hi}
    return out, sides


def assert_covers(sides, high=True):
    for name in ("left", "top") + (("right", "bottom") if high else ()):
        assert sides[name].any(), name
    if high:
        for a, b in (("left", "top"), ("left", "bottom"), ("right", "top"), ("right", "bottom")):
            assert (sides[a] & sides[b]).any(), (a, b)
    assert (~(sides["left"] | sides["right"] | sides["top"] | sides["bottom"])).any()      # some MVs inside the limits among them


def block_view(plane, b, bw, bh):
    return plane[int(b["by"]):int(b["by"]) + bh, int(b["bx"]):int(b["bx"]) + bw]


SIZES = [(4, 4), (8, 8), (16, 16)]   # (the 4 x 4 blocks take the 4-tap sets)


@pytest.mark.parametrize("bd", [8, 10])
def test_single_reference_positions_are_clamped_to_the_written_limits(hip, oracle, ctx, bd):
    rng = np.random.default_rng(500 + bd)
    ref = hip.synth.lcg_frame(W, H, 21, 0, bd)
    pr, pp = ctx.planes_alloc(W, H, BORDER, bd, 1), ctx.planes_alloc(W, H, BORDER, bd, 1)
    ctx.planes_upload(pr, 0, ref)
    rb = oracle.extend_plane(ref, BORDER, pr.stride)
    vis = (slice(BORDER, BORDER + H), slice(BORDER, BORDER + W))

    def device(blocks, mv, bw, bh, fx, fy, ss):
        d_b, d_mv = ctx.to_device(blocks), ctx.to_device(mv)
        ctx.planes_upload(pp, 0, np.zeros_like(ref))
        ctx.build_inter_pred_batch(pr, 0, pp, 0, bw, bh, d_b, d_mv, len(blocks), fx, fy, ss, ss)
        got = ctx.planes_download(pp, 0)[vis].copy()
        ctx.free(d_b); ctx.free(d_mv)
        return got

    for (bw, bh) in SIZES:
        blocks, lim = grid_blocks(hip, bw, bh), limits(W, H, BORDER, bw, bh)
        for fx, fy in ((0, 0), (2, 1)):
            # chroma form: MVs in sixteenths
            mv = wild_mvs(rng, blocks, lim, 1)
            mvc, sides = clamped_sixteenths(blocks, mv, 1, lim)
            assert_covers(sides)
            want = oracle.build_inter_pred(rb, BORDER, W, H, bw, bh, blocks, mvc, fx, fy, bd, 1, 1)
            assert np.array_equal(device(blocks, mv, bw, bh, fx, fy, 1), want), (bw, bh, fx, fy, "chroma")
            # luma form: MVs in eighths.  The low limits are even, the high ones odd: a luma MV cannot express them, the chroma form can
            mv = wild_mvs(rng, blocks, lim, 2)
            mvc, sides = clamped_sixteenths(blocks, mv, 2, lim)
            assert_covers(sides)
            got = device(blocks, mv, bw, bh, fx, fy, 0)
            assert np.array_equal(got, device(blocks, mvc, bw, bh, fx, fy, 1)), (bw, bh, fx, fy, "luma against the chroma form")
            even = ~(sides["right"] | sides["bottom"])
            assert even.sum() >= 3 and not (mvc[even] & 1).any()
            want = oracle.build_inter_pred(rb, BORDER, W, H, bw, bh, blocks[even], mvc[even] // 2, fx, fy, bd)
            for b in blocks[even]:
                assert np.array_equal(block_view(got, b, bw, bh), block_view(want, b, bw, bh)), (bw, bh, fx, fy, "luma low side", b)
    ctx.planes_free(pr); ctx.planes_free(pp)


@pytest.mark.parametrize("bd", [8, 10])
def test_compound_positions_are_clamped_by_the_smaller_border(hip, oracle, ctx, bd):
    rng = np.random.default_rng(520 + bd)
    ref0, ref1 = hip.synth.lcg_frame(W, H, 22, 0, bd), hip.synth.lcg_frame(W, H, 23, 1, bd)
    r0, r1, pp = ctx.planes_alloc(W, H, BORDER, bd, 1), ctx.planes_alloc(W, H, BORDER + 8, bd, 1), ctx.planes_alloc(W, H, BORDER, bd, 1)
    ctx.planes_upload(r0, 0, ref0); ctx.planes_upload(r1, 0, ref1)
    # (the second reference's 24-pixel border replicates the same edge: within 16 pixels it is this array)
    b0, b1 = oracle.extend_plane(ref0, BORDER, r0.stride), oracle.extend_plane(ref1, BORDER, r0.stride)
    vis = (slice(BORDER, BORDER + H), slice(BORDER, BORDER + W))

    def device(blocks, mv0, mv1, bw, bh, fx, fy, fwd, bck, ss):
        d_b, d_0, d_1 = ctx.to_device(blocks), ctx.to_device(mv0), ctx.to_device(mv1)
        ctx.planes_upload(pp, 0, np.zeros_like(ref0))
        ctx.build_compound_pred_batch(r0, 0, r1, 0, pp, 0, bw, bh, d_b, d_0, d_1, len(blocks), fx, fy, fwd, bck, ss, ss)
        got = ctx.planes_download(pp, 0)[vis].copy()
        for d in (d_b, d_0, d_1):
            ctx.free(d)
        return got

    for (bw, bh) in SIZES:
        blocks, lim = grid_blocks(hip, bw, bh), limits(W, H, BORDER, bw, bh)      # the smaller border, the first reference's size
        for fx, fy, fwd, bck in ((0, 0, 0, 0), (1, 2, 9, 7)):
            mv0, mv1 = wild_mvs(rng, blocks, lim, 1), wild_mvs(rng, blocks, lim, 1)[::-1].copy()
            (c0, s0), (c1, s1) = clamped_sixteenths(blocks, mv0, 1, lim), clamped_sixteenths(blocks, mv1, 1, lim)
            assert_covers(s0); assert_covers(s1)
            want = oracle.build_compound_pred(b0, b1, BORDER, W, H, bw, bh, blocks, c0, c1, fx, fy, fwd, bck, bd, 1, 1)
            assert np.array_equal(device(blocks, mv0, mv1, bw, bh, fx, fy, fwd, bck, 1), want), (bw, bh, fx, fy, fwd, "chroma")
            mv0, mv1 = wild_mvs(rng, blocks, lim, 2), wild_mvs(rng, blocks, lim, 2)[::-1].copy()
            (c0, s0), (c1, s1) = clamped_sixteenths(blocks, mv0, 2, lim), clamped_sixteenths(blocks, mv1, 2, lim)
            assert_covers(s0); assert_covers(s1)
            got = device(blocks, mv0, mv1, bw, bh, fx, fy, fwd, bck, 0)
            assert np.array_equal(got, device(blocks, c0, c1, bw, bh, fx, fy, fwd, bck, 1)), (bw, bh, fx, fy, fwd, "luma against the chroma form")
            even = ~(s0["right"] | s0["bottom"] | s1["right"] | s1["bottom"])
            assert even.any()
            want = oracle.build_compound_pred(b0, b1, BORDER, W, H, bw, bh, blocks[even], c0[even] // 2, c1[even] // 2, fx, fy, fwd, bck, bd)
            for b in blocks[even]:
                assert np.array_equal(block_view(got, b, bw, bh), block_view(want, b, bw, bh)), (bw, bh, fx, fy, fwd, "luma low side", b)
    for p in (r0, r1, pp):
        ctx.planes_free(p)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("bw", [8, 16])
def test_fused_block_kernel_clamps_as_the_predictor_does(hip, oracle, ctx, bd, bw):
    """Out-of-range MVs: the fused call equals the three separate calls (as tests/test_gpu_encode_block.py composes them); with nothing beyond the
    high limits, whose clamped positions a luma MV cannot express, it equals the oracle's chain on the clamped MVs as well."""
    capi = hip.capi
    rng = np.random.default_rng(540 + bd + bw)
    ref = hip.synth.lcg_frame(W, H, 24, 0, bd)
    src = np.clip(ref.astype(np.int32) + rng.integers(-30, 31, ref.shape) * (1 << (bd - 8)), 0, (1 << bd) - 1).astype(ref.dtype)
    q = oracle.build_quantizer_y(bd, 90)
    qp = capi.QuantParams.from_tables(q)
    tx, nc = {8: 1, 16: 2}[bw], bw * bw
    blocks, lim = grid_blocks(hip, bw, bw), limits(W, H, BORDER, bw, bw)
    n, gc = len(blocks), W // bw
    ps, pr, pp, pf = (ctx.planes_alloc(W, H, BORDER, bd, 1) for _ in range(4))
    ctx.planes_upload(ps, 0, src); ctx.planes_upload(pr, 0, ref)
    rb = oracle.extend_plane(ref, BORDER, pr.stride)
    vis = (slice(BORDER, BORDER + H), slice(BORDER, BORDER + W))
    d_b = ctx.to_device(blocks)
    bufs = [ctx.malloc(n * nc * 4) for _ in range(4)] + [ctx.malloc(2 * n + 16) for _ in range(2)]
    d_q, d_dq, d_q2, d_dq2, d_e, d_e2 = bufs
    for high in (True, False):
        mv = wild_mvs(rng, blocks, lim, 2, high)
        mvc, sides = clamped_sixteenths(blocks, mv, 2, lim)
        assert_covers(sides, high)
        d_mv = ctx.to_device(mv)
        ctx.build_inter_pred_batch(pr, 0, pp, 0, bw, bw, d_b, d_mv, n, 0, 0)
        ctx.subtract_xform_quant_batch(ps, pp, 0, tx, None, n, gc, 0, qp, None, d_q, d_dq, d_e)
        ctx.inv_txfm_add_batch(d_dq, tx, None, n, gc, 0, d_e, pp, 0)
        ctx.planes_upload(pf, 0, np.zeros_like(ref))
        ctx.encode_inter_blocks_batch(ps, 0, pr, 0, pf, 0, bw, d_b, d_mv, n, qp, d_q2, d_dq2, d_e2, 0, 0, 0)
        rec = ctx.planes_download(pf, 0)[vis].copy()
        qf, dqf, ef = ctx.from_device(d_q2, (n, nc), np.int32), ctx.from_device(d_dq2, (n, nc), np.int32), ctx.from_device(d_e2, (n,), np.uint16)
        assert np.array_equal(rec, ctx.planes_download(pp, 0)[vis])
        assert np.array_equal(qf, ctx.from_device(d_q, (n, nc), np.int32)) and np.array_equal(dqf, ctx.from_device(d_dq, (n, nc), np.int32))
        assert np.array_equal(ef, ctx.from_device(d_e, (n,), np.uint16)) and (ef > 0).any()
        if not high:
            assert not (mvc & 1).any()
            pred_o = oracle.build_inter_pred(rb, BORDER, W, H, bw, bw, blocks, mvc // 2, 0, 0, bd)
            residual = (src.astype(np.int32) - pred_o.astype(np.int32)).astype(np.int16)
            _, q_o, dq_o, e_o = oracle.xform_quant_batch(residual, tx, None, n, gc, 0, q, bd > 8, n * nc, False, 8)
            rec_o = oracle.inv_txfm_add_batch(dq_o, tx, None, n, gc, 0, e_o, pred_o, bd)
            assert np.array_equal(ef, e_o) and np.array_equal(qf.ravel(), q_o) and np.array_equal(dqf.ravel(), dq_o)
            assert np.array_equal(rec, rec_o.astype(rec.dtype))
        ctx.free(d_mv)
    for d in [d_b] + bufs:
        ctx.free(d)
    for p in (ps, pr, pp, pf):
        ctx.planes_free(p)


# ---- 2. the compound finish across its three users ------------------------------------------------------------------------------------------------

def three_compounds(hip, ctx, planes, bd, bw, bh, bx, by, d0, d1, weights):
    """One block at (bx, by) predicted from planes[0] displaced by d0 = (dx, dy) whole pixels and planes[1] by d1: the unscaled compound call, the
    scaled one at step 1024, the compound warp with a translation-only model -> three bw x bh blocks."""
    capi = hip.capi
    B = 32
    pr = [ctx.planes_alloc(W, H, B, bd, 1) for _ in range(2)]
    pp = ctx.planes_alloc(W, H, B, bd, 1)
    for r in range(2):
        ctx.planes_upload(pr[r], 0, planes[r])
    out = []
    here = (slice(B + by, B + by + bh), slice(B + bx, B + bx + bw))
    fwd, bck = weights or (0, 0)
    blk = np.zeros(1, capi.search_block_dtype)
    blk["bx"], blk["by"] = bx, by
    d_b = ctx.to_device(blk)
    d_mv = [ctx.to_device(np.array([[8 * d[1], 8 * d[0]]], np.int16)) for d in (d0, d1)]
    ctx.planes_upload(pp, 0, np.zeros_like(planes[0]))
    ctx.build_compound_pred_batch(pr[0], 0, pr[1], 0, pp, 0, bw, bh, d_b, d_mv[0], d_mv[1], 1, 0, 0, fwd, bck)
    out.append(ctx.planes_download(pp, 0)[here].copy())
    for d in [d_b] + d_mv:
        ctx.free(d)
    d_conv = ctx.to_device(np.zeros(H * W, np.uint16))
    ctx.planes_upload(pp, 0, np.zeros_like(planes[0]))
    for r, d in enumerate((d0, d1)):
        rec = np.zeros(1, capi.scaled_block_dtype)
        rec["src_x"], rec["src_y"], rec["dst_x"], rec["dst_y"] = bx + d[0], by + d[1], bx, by
        d_b = ctx.to_device(rec)
        ctx.scaled_pred_compound_batch(pr[r], 0, pp if r else None, 0, bw, bh, 0, 0, 1024, 1024, d_b, 1, d_conv, W, r, weights)
        ctx.free(d_b)
    out.append(ctx.planes_download(pp, 0)[here].copy())
    ctx.planes_upload(pp, 0, np.zeros_like(planes[0]))
    for r, d in enumerate((d0, d1)):
        rec = np.zeros(1, capi.warp_block_dtype)
        rec["mat"][0] = [d[0] << 16, d[1] << 16, 1 << 16, 0, 0, 1 << 16]
        rec["p_col"], rec["p_row"], rec["p_width"], rec["p_height"] = bx, by, bw, bh
        d_b = ctx.to_device(rec)
        ctx.warp_affine_compound_batch(pr[r], 0, pp if r else None, 0, 0, 0, d_b, 1, bw, bh, d_conv, W, r, weights)
        ctx.free(d_b)
    out.append(ctx.planes_download(pp, 0)[here].copy())
    ctx.free(d_conv)
    for p in pr + [pp]:
        ctx.planes_free(p)
    return out


@pytest.mark.parametrize("weights", [None, (9, 7)])
@pytest.mark.parametrize("bd,bw,bh", [(10, 16, 16), (12, 8, 8), (12, 16, 16), (10, 8, 8)])
def test_compound_finish_is_one_function_of_its_three_users(hip, oracle, ctx, bd, bw, bh, weights):
    """No entry point refuses step 1024 or a translation-only model, so all three legs run.  The reference's warp filter of phase 0 is not the
    identity -- Warped_Filters[64] is { 0, 0, 0, 127, 1, 0, 0, 0 } (av1/common/warped_motion.c), the table this library generates from it -- so a
    translation-only warp copies a pixel only where its right and lower neighbours equal it.  The three-way equality is therefore asserted on
    references that are flat over the block's footprint, at value pairs that reach both ends of the clip and both rounding directions; on textured
    references the unscaled and the scaled call must still agree with each other and with the oracle, and the warp with the oracle's own compound warp."""
    from test_golden_warp import orc_warp_compound
    mx = (1 << bd) - 1
    dt = np.uint16
    bx, by, d0, d1 = 24, 16, (3, -2), (-5, 4)
    fwd, bck = weights or (0, 0)
    one = np.zeros(1, hip.capi.search_block_dtype)
    one["bx"], one["by"] = bx, by
    mvs = [np.array([[8 * d[1], 8 * d[0]]], np.int16) for d in (d0, d1)]

    def oracle_block(planes):
        ext = [oracle.extend_plane(p, 32) for p in planes]
        return block_view(oracle.build_compound_pred(ext[0], ext[1], 32, W, H, bw, bh, one, mvs[0], mvs[1], 0, 0, fwd, bck, bd), one[0], bw, bh)

    for a, b in ((0, 0), (mx, mx), (0, mx), (mx, 0), (1, 2), (mx - 1, mx), (mx // 3, 2 * mx // 3 + 1), (5, 10)):
        planes = [np.full((H, W), a, dt), np.full((H, W), b, dt)]
        plain, scaled, warped = three_compounds(hip, ctx, planes, bd, bw, bh, bx, by, d0, d1, weights)
        want = oracle_block(planes)
        assert np.array_equal(plain, want) and np.array_equal(scaled, want) and np.array_equal(warped, want), (a, b)
    planes = [hip.synth.lcg_frame(W, H, 25 + r, r, bd) for r in range(2)]
    plain, scaled, warped = three_compounds(hip, ctx, planes, bd, bw, bh, bx, by, d0, d1, weights)
    want = oracle_block(planes)
    assert np.array_equal(plain, want) and np.array_equal(scaled, want)
    c = {"mat": [[d[0] << 16, d[1] << 16, 1 << 16, 0, 0, 1 << 16] for d in (d0, d1)], "shear": [[0, 0, 0, 0]] * 2, "p_col": bx, "p_row": by, "pw": bw, "ph": bh,
         "ss": 0, "weights": weights, "round_0": 5 if bd == 12 else 3}
    assert np.array_equal(warped, orc_warp_compound(oracle, planes, bd, c)[1].astype(warped.dtype))


# ---- 3. the tap sets through both searches that build on up_tap -----------------------------------------------------------------------------------

SW, SH, SB = 96, 64, 32


def subpel_inputs(hip, oracle, bd, bw, bh):
    """A smooth reference and, per block, a source that is the reference displaced by the block's own eighth-pel offset (bilinear), so that the trees
    end on MVs of every phase.  -> everything both searches need, as host arrays."""
    capi = hip.capi
    rng = np.random.default_rng(700 + bd + bw)
    _, ref = hip.synth.shifted_smooth_pair(SW, SH, 17, bd)
    mx = (1 << bd) - 1
    rb = oracle.extend_plane(ref, SB, SW + 2 * SB)
    gc, gr = SW // bw, SH // bh
    n = gc * gr
    blocks = np.zeros(n, capi.search_block_dtype)
    blocks["bx"], blocks["by"] = (np.arange(n) % gc) * bw, (np.arange(n) // gc) * bh
    i = np.arange(n)
    off_r, off_c = (i % 8) + 8 * ((i // 3) % 3 - 1), ((3 * i + i // 8) % 8) + 8 * ((i // 5) % 3 - 1)      # eighths: every phase on each axis
    blocks["start_row"], blocks["start_col"] = 8 * np.round(off_r / 8).astype(np.int64), 8 * np.round(off_c / 8).astype(np.int64)
    blocks["ref_row"], blocks["ref_col"] = blocks["start_row"], blocks["start_col"]
    blocks["row_min"], blocks["row_max"] = blocks["start_row"] - 24, blocks["start_row"] + 24
    blocks["col_min"], blocks["col_max"] = blocks["start_col"] - 24, blocks["start_col"] + 24
    f = rb.astype(np.float64)
    sblk = np.zeros((n, bh, bw), np.int64)
    for k in range(n):
        y, x, fy, fx = SB + int(blocks["by"][k]) + (int(off_r[k]) >> 3), SB + int(blocks["bx"][k]) + (int(off_c[k]) >> 3), (int(off_r[k]) & 7) / 8, (int(off_c[k]) & 7) / 8
        t = f[y:y + bh + 1, x:x + bw + 1]
        t = t[:, :-1] * (1 - fx) + t[:, 1:] * fx
        sblk[k] = np.round(t[:-1] * (1 - fy) + t[1:] * fy)
    src = np.zeros((SH, SW), ref.dtype)
    for k in range(n):
        src[blocks["by"][k]:blocks["by"][k] + bh, blocks["bx"][k]:blocks["bx"][k] + bw] = sblk[k]
    sb = oracle.extend_plane(src, SB, SW + 2 * SB)
    # the compound search's other predictor and the OBMC search's weighted source, both close to the source block itself
    second = np.clip(sblk + rng.integers(-2 << (bd - 8), (2 << (bd - 8)) + 1, sblk.shape), 0, mx).astype(ref.dtype)
    om = np.full((n, bh, bw), 4096, np.int64)
    om[:, :bh // 2, :] = (np.linspace(36, 64, bh // 2).astype(np.int64) * 64)[None, :, None]
    nb = np.clip(sblk + rng.integers(-2 << (bd - 8), (2 << (bd - 8)) + 1, sblk.shape), 0, mx)
    ws = (sblk * 4096 - nb * (4096 - om)).astype(np.int32)
    return ref, src, rb, sb, blocks, second, ws, om.astype(np.int32)


def phases_covered(mv):
    return all(len(set((mv[:, a] & 7).tolist())) == 8 for a in (0, 1))


SUBPEL_REFERENCE = {}


def subpel_reference(hip, oracle, bd, bw, bh):
    """The inputs and the oracle's answers for the three tap types, computed once per (bd, size)."""
    key = (bd, bw, bh)
    if key not in SUBPEL_REFERENCE:
        inp = subpel_inputs(hip, oracle, bd, bw, bh)
        ref, src, rb, sb, blocks, second, ws, om = inp
        kw = dict(cost_type=hip.capi.MV_COST_NONE, error_per_bit=0, iters_per_step=2, allow_hp=1, forced_stop=0, bd=bd, threads=8)
        want = {}
        for sst in (1, 2, 3):
            want["compound", sst] = oracle.compound_subpel_tree_batch(sb, rb, SB, bw, bh, blocks, second, None, 0, tree=2, subpel_search_type=sst, **kw)
            want["obmc", sst] = oracle.obmc_subpel_tree_batch(rb, SB, bw, bh, blocks, ws, om, subpel_search_type=sst, **kw)
        SUBPEL_REFERENCE[key] = (inp, want)
    return SUBPEL_REFERENCE[key]


@pytest.mark.parametrize("sst", [1, 2, 3])
@pytest.mark.parametrize("bw,bh", [(8, 8), (16, 16)])
@pytest.mark.parametrize("bd", [8, 10])
def test_up_sampling_searches_use_the_shared_taps_at_every_phase(hip, oracle, ctx, bd, bw, bh, sst):
    capi = hip.capi
    (ref, src, rb, sb, blocks, second, ws, om), want = subpel_reference(hip, oracle, bd, bw, bh)
    n = len(blocks)
    for search in ("compound", "obmc"):
        assert phases_covered(want[search, sst][0]), (search, sst, "the oracle's final MVs must cover all eight phases on each axis")
    ps, pr = ctx.planes_alloc(SW, SH, SB, bd, 1), ctx.planes_alloc(SW, SH, SB, bd, 1)
    ctx.planes_upload(ps, 0, src); ctx.planes_upload(pr, 0, ref)
    d_b, d_sp, d_ws, d_om = ctx.to_device(blocks), ctx.to_device(second), ctx.to_device(ws), ctx.to_device(om)
    outs = [ctx.malloc(n * 4 + 16) for _ in range(4)]
    p = capi.SubpelParams(2, capi.MV_COST_NONE, 0, 2, 1, 0, sst)
    for search in ("compound", "obmc"):
        if search == "compound":
            ctx.compound_subpel_tree_batch(ps, pr, 0, bw, bh, p, d_b, n, d_sp, None, 0, outs[0], outs[1], outs[2], outs[3])
        else:
            ctx.obmc_subpel_tree_batch(pr, 0, bw, bh, p, d_b, n, d_ws, d_om, outs[0], outs[1], outs[2], outs[3])
        got = (ctx.from_device(outs[0], (n, 2), np.int16), ctx.from_device(outs[1], (n,), np.uint32), ctx.from_device(outs[2], (n,), np.int32),
               ctx.from_device(outs[3], (n,), np.uint32))
        for name, g_, w_ in zip(("mv", "err", "distortion", "sse"), got, want[search, sst]):
            assert np.array_equal(g_, w_), (search, sst, name, np.flatnonzero((g_ != w_).reshape(n, -1).any(1))[:6])
    for d in [d_b, d_sp, d_ws, d_om] + outs:
        ctx.free(d)
    ctx.planes_free(ps); ctx.planes_free(pr)


# ---- 4. argument checks ---------------------------------------------------------------------------------------------------------------------------

class Rings:
    """Planes for the argument checks: p8 / q8 / d8 good 8-bit rings (d8 the destination, filled with a pattern), and the ones a call must refuse."""

    def __init__(self, ctx):
        self.ctx = ctx
        mk = ctx.planes_alloc
        self.p8, self.q8, self.d8 = mk(64, 64, 16, 8, 1), mk(64, 64, 16, 8, 1), mk(64, 64, 16, 8, 1)
        self.p10, self.small, self.wide, self.tall = mk(64, 64, 16, 10, 1), mk(64, 64, 4, 8, 1), mk(80, 64, 16, 8, 1), mk(64, 80, 16, 8, 1)
        self.nobase = type(self.p8).from_buffer_copy(self.p8)
        self.nobase.base = None
        self.pattern = (np.arange(64 * 64, dtype=np.uint32) * 37 % 251).astype(np.uint8).reshape(64, 64)
        ctx.planes_upload(self.d8, 0, self.pattern)
        self.before = ctx.planes_download(self.d8, 0).copy()
        self.buf = ctx.to_device(np.full(4096, 0x5A, np.uint8))      # d_pred / d_mask_out / d_conv
        self.lst = ctx.to_device(np.zeros(256, np.uint8))             # a block / MV / item list of zeros: one block at (0, 0), MV 0

    def untouched(self):
        return np.array_equal(self.ctx.planes_download(self.d8, 0), self.before) and (self.ctx.from_device(self.buf, (4096,), np.uint8) == 0x5A).all()

    def close(self):
        for p in (self.p8, self.q8, self.d8, self.p10, self.small, self.wide, self.tall):
            self.ctx.planes_free(p)
        self.ctx.free(self.buf); self.ctx.free(self.lst)


@pytest.fixture(scope="module")
def rings(ctx):
    r = Rings(ctx)
    yield r
    r.close()


def refused(hip, rings, call, good, bad):
    """call(**good) with each of `bad`'s overrides in turn: refused, and nothing written."""
    for over in bad:
        with pytest.raises(hip.capi.AomHipError):
            call(**dict(good, **over))
            pytest.fail("accepted: %r" % (over,))
        assert rings.untouched(), over


COMMON_BAD = [dict(fx=-1), dict(fx=4), dict(fy=-1), dict(fy=4), dict(bw=16, bh=12), dict(bw=128, bh=32), dict(bw=2, bh=2), dict(n=-1), dict(blocks=None), dict(mv=None)]


def test_single_reference_entry_points_refuse_bad_arguments(hip, ctx, rings):
    g = rings

    def ex(ref=g.p8, rf=0, pred=g.d8, pf=0, bw=16, bh=16, blocks=g.lst, mv=g.lst, n=1, fx=0, fy=0, ss_x=1, ss_y=0):
        hip.capi.check(hip.capi.lib.aomhip_build_inter_pred_ex_batch(ctx.h, hip.capi.C.byref(ref), rf, hip.capi.C.byref(pred), pf, bw, bh, blocks, mv, n, fx, fy, ss_x,
                                                                     ss_y), "ex")
    refused(hip, g, ex, {}, COMMON_BAD + [dict(rf=-1), dict(rf=1), dict(pf=-1), dict(pf=1), dict(ref=g.p10), dict(pred=g.p10), dict(ref=g.small), dict(ref=g.nobase),
                                         dict(pred=g.nobase), dict(ss_x=-1), dict(ss_x=2), dict(ss_y=-1), dict(ss_y=2)])
    ex(blocks=None, mv=None, n=0)
    assert g.untouched()

    def contiguous(ref=g.p8, rf=0, pred=g.buf, bw=16, bh=16, blocks=g.lst, mv=g.lst, n=1, fx=0, fy=0):
        ctx.build_inter_pred_contiguous_batch(ref, rf, pred, bw, bh, blocks, mv, n, fx, fy)
    refused(hip, g, contiguous, {}, COMMON_BAD + [dict(rf=-1), dict(rf=1), dict(ref=g.small), dict(ref=g.nobase), dict(pred=None)])
    contiguous(blocks=None, mv=None, n=0)
    assert g.untouched()

    def fullpel(ref=g.p8, rf=0, pred=g.d8, pf=0, bw=16, bh=16, blocks=g.lst, mv=g.lst, n=1):
        ctx.build_pred_fullpel(ref, rf, pred, pf, bw, bh, blocks, mv, n)
    refused(hip, g, fullpel, {}, [dict(bw=16, bh=12), dict(bw=128, bh=32), dict(n=-1), dict(blocks=None), dict(mv=None), dict(blocks=None, n=0), dict(mv=None, n=0),
                                  dict(rf=-1), dict(rf=1), dict(pf=-1), dict(pf=1), dict(ref=g.p10), dict(pred=g.p10), dict(ref=g.nobase), dict(pred=g.nobase)])
    fullpel(n=0)
    assert g.untouched()


def test_compound_entry_points_refuse_bad_arguments(hip, ctx, rings):
    g = rings
    shared = [dict(fx=-1), dict(fx=4), dict(fy=-1), dict(fy=4), dict(bw=16, bh=12), dict(bw=128, bh=32), dict(n=-1), dict(blocks=None), dict(mv0=None), dict(mv1=None),
              dict(f0=-1), dict(f0=1), dict(f1=-1), dict(f1=1), dict(pf=-1), dict(pf=1), dict(r0=g.p10), dict(r1=g.p10), dict(pred=g.p10), dict(r1=g.wide),
              dict(r1=g.tall), dict(r0=g.small), dict(r1=g.small), dict(r0=g.nobase), dict(r1=g.nobase), dict(pred=g.nobase)]
    ss_bad = [dict(ss_x=-1), dict(ss_x=2), dict(ss_y=-1), dict(ss_y=2)]

    def compound(r0=g.p8, f0=0, r1=g.q8, f1=0, pred=g.d8, pf=0, bw=16, bh=16, blocks=g.lst, mv0=g.lst, mv1=g.lst, n=1, fx=0, fy=0, fwd=0, bck=0, ss_x=0, ss_y=0):
        ctx.build_compound_pred_batch(r0, f0, r1, f1, pred, pf, bw, bh, blocks, mv0, mv1, n, fx, fy, fwd, bck, ss_x, ss_y)
    refused(hip, g, compound, {}, shared + ss_bad + [dict(fwd=9, bck=9), dict(fwd=16, bck=1), dict(fwd=-1, bck=17), dict(fwd=17, bck=-1), dict(fwd=8, bck=0)])
    compound(blocks=None, mv0=None, mv1=None, n=0)
    assert g.untouched()

    def masked(r0=g.p8, f0=0, r1=g.q8, f1=0, pred=g.d8, pf=0, bw=16, bh=16, blocks=g.lst, mv0=g.lst, mv1=g.lst, n=1, fx=0, fy=0, mask=g.buf, moff=None, ms=16, subw=0,
               subh=0, ss_x=0, ss_y=0):
        ctx.build_masked_compound_pred_batch(r0, f0, r1, f1, pred, pf, bw, bh, blocks, mv0, mv1, n, fx, fy, mask, moff, ms, subw, subh, ss_x, ss_y)
    refused(hip, g, masked, {}, shared + ss_bad + [dict(mask=None), dict(ms=0), dict(ms=-16), dict(subw=-1), dict(subw=2), dict(subh=-1), dict(subh=2)])
    masked(blocks=None, mv0=None, mv1=None, n=0)
    assert g.untouched()

    def diffwtd(r0=g.p8, f0=0, r1=g.q8, f1=0, pred=g.d8, pf=0, bw=16, bh=16, blocks=g.lst, mv0=g.lst, mv1=g.lst, n=1, fx=0, fy=0, mtype=0, mout=g.buf):
        ctx.build_diffwtd_compound_pred_batch(r0, f0, r1, f1, pred, pf, bw, bh, blocks, mv0, mv1, n, fx, fy, mtype, mout)
    refused(hip, g, diffwtd, {}, shared + [dict(mtype=-1), dict(mtype=2)])
    diffwtd(blocks=None, mv0=None, mv1=None, n=0)
    assert g.untouched()


def test_blend_and_scaled_entry_points_refuse_bad_arguments(hip, ctx, rings):
    g = rings

    def blend(pred=g.d8, pf=0, adj=g.p8, af=0, items=g.lst, n=1, masks=g.lst):
        ctx.blend_a64_1d_batch(pred, pf, adj, af, items, n, masks)
    refused(hip, g, blend, {}, [dict(pf=-1), dict(pf=1), dict(af=-1), dict(af=1), dict(adj=g.p10), dict(adj=g.wide), dict(adj=g.tall), dict(items=None), dict(masks=None),
                                dict(n=-1), dict(adj=g.nobase), dict(pred=g.nobase)])
    blend(items=None, masks=None, n=0)
    assert g.untouched()

    steps_bad = [dict(xs=63), dict(xs=2049), dict(ys=63), dict(ys=2049), dict(xs=0), dict(ys=-1024)]
    shared = [dict(fx=-1), dict(fx=4), dict(fy=-1), dict(fy=4), dict(bw=0), dict(bw=129), dict(bh=0), dict(bh=129), dict(n=-1), dict(blocks=None), dict(rf=-1), dict(rf=1),
              dict(ref=g.nobase)] + steps_bad

    def scaled(ref=g.p8, rf=0, pred=g.d8, pf=0, bw=16, bh=16, fx=0, fy=0, xs=1024, ys=1024, blocks=g.lst, n=1):
        ctx.scaled_pred_batch(ref, rf, pred, pf, bw, bh, fx, fy, xs, ys, blocks, n)
    refused(hip, g, scaled, {}, shared + [dict(pf=-1), dict(pf=1), dict(pred=g.p10), dict(ref=g.p10), dict(pred=g.nobase)])
    scaled(blocks=None, n=0)
    assert g.untouched()

    def scaled_compound(ref=g.p8, rf=0, pred=g.d8, pf=0, bw=16, bh=16, fx=0, fy=0, xs=1024, ys=1024, blocks=g.lst, n=1, conv=g.buf, cs=64, avg=1):
        ctx.scaled_pred_compound_batch(ref, rf, pred if avg else None, pf, bw, bh, fx, fy, xs, ys, blocks, n, conv, cs, avg)
    for avg in (0, 1):
        refused(hip, g, scaled_compound, dict(avg=avg), shared + [dict(conv=None), dict(cs=0), dict(cs=-64)])
        scaled_compound(blocks=None, n=0, avg=avg)
    refused(hip, g, scaled_compound, {}, [dict(pf=-1), dict(pf=1), dict(pred=g.p10), dict(pred=g.nobase)])
    assert g.untouched()
