"""The arithmetic the motion-search kernels share, checked where the other GPU tests do not go on purpose.

a. The clamp of the high-bit-depth variance (aom_dsp/variance.c:383-420 HIGHBD_VAR: `var = sse - sum^2 / N`, `var >= 0 ? var : 0`).  The
   rounding of sse and sum at 10 and 12 bits can make the difference negative: a 4x4 12-bit block whose 16 differences are eight 15s and eight
   16s has sum 248 -> 16, sum^2 >> 4 = 16, sse 3848 -> 15, 15 - 16 < 0.  Such two-valued blocks are searched for with the oracle for 4x4, 8x8
   and 16x16 and driven through every entry point that finishes a variance; the same pattern on 8-bit planes takes the unsigned subtraction.
   The reference plane is constant, so every MV and every sub-pel phase sees the same differences.
b. The MV cost types per search family: the (family, MV_COST_*) pairs no other GPU test runs (see the table in DESIGN.md), L1_MIDRES -- whose
   variance-stage lambda is 0 and SAD-stage lambda 15 -- first among them.  Reference MVs have a negative and a non-multiple-of-8 component.

Everything is compared exactly with the oracle (oracle/pyoracle.py)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = H = 128
B = 96
MV_MAX = (1 << 14) - 1


@functools.lru_cache(maxsize=None)
def _tables():
    v = np.abs(np.arange(-MV_MAX, MV_MAX + 1))
    bits = np.where(v == 0, 0, np.floor(np.log2(np.maximum(v, 1))) + 1).astype(np.int64)
    return np.array([190, 660, 655, 1040], np.int32), (140 + bits * 305).astype(np.int32), (165 + bits * 285 + (v & 7) * 5).astype(np.int32)


def _dev_tables(ctx):
    tj, t0, t1 = _tables()
    own = [ctx.to_device(tj), ctx.to_device(t0), ctx.to_device(t1)]
    return own, (own[0], own[1] + MV_MAX * 4, own[2] + MV_MAX * 4)


# ---- a. the clamp -------------------------------------------------------------------------------------------------------------------------

def _tile(bs, a, k, dtype):
    """bs x bs differences: the first k in raster order a + 1, the others a."""
    t = np.full(bs * bs, a, dtype)
    t[:k] += 1
    return t.reshape(bs, bs)


@functools.lru_cache(maxsize=None)
def _clamp_pattern(bs, bd):
    """(a, k) of the first two-valued difference block whose variance the oracle computes from sse - (sum^2 >> log2 N) < 0, or None."""
    import pyoracle as oracle
    zero = np.zeros((bs, bs), np.uint16)
    cands = [(15, 8)] if bs == 4 else []
    cands += [(a, k) for a in range(1, 64) for k in range(1, bs * bs)]
    for a, k in cands:
        var, sse, s = oracle.variance(_tile(bs, a, k, np.uint16), 0, 0, zero, 0, 0, bs, bs, bd)
        if int(sse) - ((int(s) * int(s)) >> (2 * int(np.log2(bs)))) < 0:
            assert var == 0
            return a, k
    return None


def test_the_hand_checked_block_and_a_12_bit_pattern_for_every_size(oracle):
    var, sse, s = oracle.variance(_tile(4, 15, 8, np.uint16), 0, 0, np.zeros((4, 4), np.uint16), 0, 0, 4, 4, 12)
    assert (var, sse, s) == (0, 15, 16)
    for bs in (4, 8, 16):
        assert _clamp_pattern(bs, 12) is not None, bs
    assert _clamp_pattern(4, 12) == (15, 8)


def _clamp_cases():
    out = []
    for bs in (4, 8, 16):
        for bd in (12, 10, 8):
            for sign in (1, -1):
                out.append(pytest.param(bs, bd, sign, id="%dx%d-%dbit-%s" % (bs, bs, bd, "src_minus_ref" if sign > 0 else "ref_minus_src")))
    return out


def _scene(hip, oracle, ctx, bs, bd, sign):
    """-> None where the search found no clamping block at this depth, else planes, oracle planes, the block lists and the pattern.  sign: +1 puts
    the pattern into src - ref (the order of vf(src, ref): full-pel results, OBMC, the block variance), -1 into ref - src (the order of the
    sub-pel and compound functions, svf(ref, .., src)): the rounded sum of the NEGATED differences is -15, not -16, and does not clamp."""
    pat = _clamp_pattern(bs, 12 if bd == 8 else bd)
    if pat is None:
        assert bd == 10   # (12 bits: asserted above for every size)
        return None
    a, k = pat
    dtype = np.uint8 if bd == 8 else np.uint16
    base = {8: 100, 10: 500, 12: 2000}[bd]
    ref = np.full((H, W), base, dtype)
    src = (base + sign * np.tile(_tile(bs, a, k, np.int32), (H // bs, W // bs))).astype(dtype)
    ps, pr = ctx.planes_alloc(W, H, B, bd, 1), ctx.planes_alloc(W, H, B, bd, 1)
    ctx.planes_upload(ps, 0, src); ctx.planes_upload(pr, 0, ref)
    sb, rb = oracle.extend_plane(src, B, ps.stride), oracle.extend_plane(ref, B, pr.stride)
    pos = [(0, 0), (W - bs, H - bs), (2 * bs, 3 * bs), (bs + 1, 2 * bs + 3)]   # (the tiling has period bs: any bs x bs window holds the pattern's counts)
    n = len(pos)
    full = np.zeros(n, hip.capi.search_block_dtype)
    full["bx"], full["by"] = [p[0] for p in pos], [p[1] for p in pos]
    full["start_row"], full["start_col"] = [0, 1, -2, 3], [0, -1, 2, 1]
    full["ref_row"], full["ref_col"] = [0, -13, 21, -6], [0, 9, -30, 5]
    full["row_min"], full["row_max"], full["col_min"], full["col_max"] = -8, 8, -8, 8
    sub = full.copy()
    for f in ("start_row", "start_col", "row_min", "row_max", "col_min", "col_max"):
        sub[f] = full[f] * 8
    return dict(ps=ps, pr=pr, sb=sb, rb=rb, src=src, full=full, sub=sub, n=n, clamp=bd > 8, sign=sign, a=a, k=k)


def _same(got, want, what):
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(g), np.asarray(w)), (what, g, w)


def _is_clamped(s, sign, var, sse=None):
    """`sign`: the order of the differences this entry point's variance takes (see _scene)."""
    if not s["clamp"]:
        assert (np.asarray(var) > 0).all()
    elif s["sign"] == sign:
        assert (np.asarray(var) == 0).all()
        if sse is not None:
            assert (np.asarray(sse) > 0).all()


@pytest.mark.parametrize("bs,bd,sign", _clamp_cases())
def test_clamp_variance_batch_and_subpel_variance(hip, oracle, ctx, bs, bd, sign):
    s = _scene(hip, oracle, ctx, bs, bd, sign)
    if s is None:
        return
    c = np.zeros(2 * s["n"], hip.capi.var_cand_dtype)
    c["sx"], c["sy"] = np.tile(s["full"]["bx"], 2), np.tile(s["full"]["by"], 2)
    c["rx"], c["ry"] = c["sx"] + 1, c["sy"] - 2
    c["xoff"][s["n"]:], c["yoff"][s["n"]:] = 3, 5    # offset (0, 0), then a non-zero one
    d_c, d_v, d_s = ctx.to_device(c), ctx.malloc(len(c) * 4), ctx.malloc(len(c) * 4)
    for subpel in (False, True):
        ctx.variance_batch(s["ps"], s["pr"], 0, 1, bs, bs, d_c, len(c), len(c), d_v, d_s, subpel=subpel)
        gv, gs = ctx.from_device(d_v, (len(c),), np.uint32), ctx.from_device(d_s, (len(c),), np.uint32)
        want = oracle.variance_cands(s["sb"], s["rb"], B, bs, bs, c, subpel, bd)
        _same((gv, gs), (want[:, 0], want[:, 1]), ("variance_batch", subpel))
        _is_clamped(s, -1 if subpel else 1, want[:, 0], want[:, 1])   # variance(src, ref) / sub_pixel_variance(ref, .., src)
    for d in (d_c, d_v, d_s):
        ctx.free(d)
    ctx.planes_free(s["ps"]); ctx.planes_free(s["pr"])


@pytest.mark.parametrize("bs,bd,sign", _clamp_cases())
def test_clamp_full_pel_search_results(hip, oracle, ctx, bs, bd, sign):
    """get_mvpred_var_cost at the end of the mcomp diamond and of av1_full_pixel_search (MV_COST_NONE: the cost is the variance)."""
    s = _scene(hip, oracle, ctx, bs, bd, sign)
    if s is None:
        return
    capi, n = hip.capi, s["n"]
    d_b, d_mv, d_c = ctx.to_device(s["full"]), ctx.malloc(n * 4), ctx.malloc(n * 4)
    ctx.fullpel_diamond_batch(s["ps"], s["pr"], 0, bs, bs, 0, 4, capi.MV_COST_NONE, d_b, n, d_mv, d_c)
    got = ctx.from_device(d_mv, (n, 2), np.int16), ctx.from_device(d_c, (n,), np.int32)
    want = oracle.fullpel_diamond_batch(s["sb"], s["rb"], B, bs, bs, s["full"], 0, 4, capi.MV_COST_NONE, bd)
    _same(got, want, "diamond")
    _is_clamped(s, 1, want[1])
    for method in ("NSTEP", "DIAMOND", "HEX"):
        ctx.full_pixel_search_batch(s["ps"], s["pr"], 0, bs, bs, capi.SearchParams.make(method, 4, capi.MV_COST_NONE), d_b, n, d_mv, d_c)
        got = ctx.from_device(d_mv, (n, 2), np.int16), ctx.from_device(d_c, (n,), np.int32)
        want = oracle.full_pixel_search_batch(s["sb"], s["rb"], B, bs, bs, s["full"], oracle.search_params(method, 4, capi.MV_COST_NONE), bd=bd)
        _same(got, want[:2], ("full_pixel_search", method))
        _is_clamped(s, 1, want[1])
    for d in (d_b, d_mv, d_c):
        ctx.free(d)
    ctx.planes_free(s["ps"]); ctx.planes_free(s["pr"])


@pytest.mark.parametrize("bs,bd,sign", _clamp_cases())
def test_clamp_subpel_start_errors(hip, oracle, ctx, bs, bd, sign):
    """The start error of the bilinear sub-pel search and of the three trees (2-tap and 8-tap), and every candidate after it."""
    s = _scene(hip, oracle, ctx, bs, bd, sign)
    if s is None:
        return
    capi, n = hip.capi, s["n"]
    d_b = ctx.to_device(s["sub"])
    outs = [ctx.malloc(n * 4) for _ in range(4)]
    read = lambda: (ctx.from_device(outs[0], (n, 2), np.int16), ctx.from_device(outs[1], (n,), np.uint32), ctx.from_device(outs[2], (n,), np.int32),
                    ctx.from_device(outs[3], (n,), np.uint32))
    ctx.subpel_bilinear_batch(s["ps"], s["pr"], 0, bs, bs, capi.MV_COST_NONE, 2, 1, 0, d_b, n, *outs)
    want = oracle.subpel_bilinear_batch(s["sb"], s["rb"], B, bs, bs, s["sub"], capi.MV_COST_NONE, 2, 1, 0, bd)
    _same(read(), want, "subpel_bilinear")
    _is_clamped(s, -1, want[1], want[3])
    for tree, sst in ((2, 0), (0, 0), (1, 0), (2, 3)):
        ctx.subpel_tree_batch(s["ps"], s["pr"], 0, bs, bs, capi.SubpelParams(tree, capi.MV_COST_NONE, 0, 2, 1, 0, sst), d_b, n, *outs)
        want = oracle.subpel_tree_batch(s["sb"], s["rb"], B, bs, bs, s["sub"], tree=tree, cost_type=capi.MV_COST_NONE, subpel_search_type=sst, bd=bd)
        _same(read(), want, ("subpel_tree", tree, sst))
        _is_clamped(s, -1, want[1], want[3])
    for d in [d_b] + outs:
        ctx.free(d)
    ctx.planes_free(s["ps"]); ctx.planes_free(s["pr"])


@pytest.mark.parametrize("bs,bd,sign", _clamp_cases())
def test_clamp_compound_and_obmc(hip, oracle, ctx, bs, bd, sign):
    """av1_get_mvpred_compound_var after the 8-point refinement, the compound sub-pel tree, and the OBMC full-pel / sub-pel searches.  The other
    predictor equals the reference (the average is the reference again); the OBMC mask is 4096 everywhere (wsrc = 4096 src: the plain difference)."""
    s = _scene(hip, oracle, ctx, bs, bd, sign)
    if s is None:
        return
    capi, n = hip.capi, s["n"]
    full, sub = s["full"], s["sub"]
    sp = np.full((n, bs, bs), s["rb"][0, 0], s["rb"].dtype)
    sblk = np.stack([s["src"][b["by"]:b["by"] + bs, b["bx"]:b["bx"] + bs] for b in full]).astype(np.int64)
    ws, om = (sblk * 4096).astype(np.int32), np.full((n, bs, bs), 4096, np.int32)
    d_f, d_s, d_sp, d_ws, d_om = ctx.to_device(full), ctx.to_device(sub), ctx.to_device(sp), ctx.to_device(ws), ctx.to_device(om)
    outs = [ctx.malloc(n * 4) for _ in range(4)]
    read4 = lambda: (ctx.from_device(outs[0], (n, 2), np.int16), ctx.from_device(outs[1], (n,), np.uint32), ctx.from_device(outs[2], (n,), np.int32),
                     ctx.from_device(outs[3], (n,), np.uint32))
    ctx.refining_search_8p_batch(s["ps"], s["pr"], 0, bs, bs, capi.MV_COST_NONE, 0, 0, d_f, n, d_sp, None, 0, outs[0], outs[1], outs[2])
    got = ctx.from_device(outs[0], (n, 2), np.int16), ctx.from_device(outs[1], (n,), np.int32), ctx.from_device(outs[2], (n,), np.int32)
    want = oracle.refining_search_8p_batch(s["sb"], s["rb"], B, bs, bs, full, sp, None, 0, cost_type=capi.MV_COST_NONE, bd=bd)
    _same(got, want, "refining_search_8p")
    _is_clamped(s, -1, want[2])
    ctx.compound_subpel_tree_batch(s["ps"], s["pr"], 0, bs, bs, capi.SubpelParams(2, capi.MV_COST_NONE, 0, 2, 1, 0, 0), d_s, n, d_sp, None, 0, *outs)
    want = oracle.compound_subpel_tree_batch(s["sb"], s["rb"], B, bs, bs, sub, sp, None, 0, tree=2, subpel_search_type=0, cost_type=capi.MV_COST_NONE, bd=bd)
    _same(read4(), want, "compound_subpel_tree")
    _is_clamped(s, -1, want[1], want[3])
    ctx.obmc_full_pixel_search_batch(s["pr"], 0, bs, bs, "NSTEP", 4, 0, capi.MV_COST_NONE, 0, 0, d_f, n, d_ws, d_om, outs[0], outs[1])
    got = ctx.from_device(outs[0], (n, 2), np.int16), ctx.from_device(outs[1], (n,), np.int32)
    want = oracle.obmc_full_pixel_search_batch(s["rb"], B, bs, bs, full, ws, om, "NSTEP", 4, 0, cost_type=capi.MV_COST_NONE, bd=bd)
    _same(got, want, "obmc_full_pixel_search")
    _is_clamped(s, 1, want[1])
    for sst in (0, 3):
        ctx.obmc_subpel_tree_batch(s["pr"], 0, bs, bs, capi.SubpelParams(2, capi.MV_COST_NONE, 0, 2, 1, 0, sst), d_s, n, d_ws, d_om, *outs)
        want = oracle.obmc_subpel_tree_batch(s["rb"], B, bs, bs, sub, ws, om, cost_type=capi.MV_COST_NONE, subpel_search_type=sst, bd=bd)
        _same(read4(), want, ("obmc_subpel_tree", sst))
        _is_clamped(s, 1, want[1], want[3])
    for d in [d_f, d_s, d_sp, d_ws, d_om] + outs:
        ctx.free(d)
    ctx.planes_free(s["ps"]); ctx.planes_free(s["pr"])


@pytest.mark.parametrize("bs,bd,sign", _clamp_cases())
def test_clamp_block_variance_of_the_simple_motion_search(hip, oracle, ctx, bs, bd, sign):
    """launch_block_var through aomhip_simple_motion_search_batch: vf(src, pred) of the EIGHTTAP predictor (a constant plane again)."""
    s = _scene(hip, oracle, ctx, bs, bd, sign)
    if s is None:
        return
    capi, n = hip.capi, s["n"]
    blocks = s["full"].copy()
    blocks["ref_row"] = blocks["ref_col"] = 0
    pp = ctx.planes_alloc(W, H, B, bd, 2)
    own, tabs = _dev_tables(ctx)
    tj, t0, t1 = _tables()
    d_b, d_mv, d_sse, d_var = ctx.to_device(blocks), ctx.malloc(n * 4), ctx.malloc(n * 4), ctx.malloc(n * 4)
    fullp = capi.SearchParams.make("NSTEP", 3, capi.MV_COST_NONE)
    subp = capi.SubpelParams(2, capi.MV_COST_NONE, 0, 2, 1, 0, 3)
    ctx.simple_motion_search_batch(s["ps"], s["pr"], 0, bs, bs, fullp, subp, 0, d_b, n, pp, 1, d_mv, d_sse, d_var, *tabs)
    got = ctx.from_device(d_mv, (n, 2), np.int16), ctx.from_device(d_sse, (n,), np.uint32), ctx.from_device(d_var, (n,), np.uint32)
    want = oracle.simple_motion_search_batch(s["sb"], s["rb"], B, W, H, bs, bs, blocks, oracle.search_params("NSTEP", 3, capi.MV_COST_NONE, no_cost_list=1),
                                             dict(tree="tree", cost_type=capi.MV_COST_NONE, error_per_bit=0, iters=2, allow_hp=1, forced_stop=0, subpel_search_type=3),
                                             0, tj, t0, t1, bd=bd)
    _same(got, want[:3], "simple_motion_search")
    _is_clamped(s, 1, want[2], want[1])
    for d in own + [d_b, d_mv, d_sse, d_var]:
        ctx.free(d)
    for p in (s["ps"], s["pr"], pp):
        ctx.planes_free(p)


# ---- b. the cost types no other GPU test runs for a family --------------------------------------------------------------------------------

EMPTY_CELLS = [("mesh", "L1_MIDRES"), ("bilinear_tree", "L1_MIDRES"), ("eighttap_tree", "L1_LOWRES"), ("eighttap_tree", "L1_MIDRES"), ("compound_refining", "L1_LOWRES"),
               ("compound_refining", "L1_MIDRES"), ("compound_diamond", "L1_MIDRES"), ("obmc_fullpel", "L1_MIDRES"), ("obmc_fullpel", "NONE"),
               ("obmc_subpel", "L1_LOWRES"), ("obmc_subpel", "L1_MIDRES")]
COST = {"ENTROPY": 0, "L1_LOWRES": 1, "L1_MIDRES": 2, "L1_HDRES": 3, "NONE": 4}


@functools.lru_cache(maxsize=None)
def _cost_scene(bs, bd):
    """Planes, <= 64 blocks, their second predictors / OBMC operands: built once per (size, depth), shared by the cells, never written."""
    import aom_av1_psy_amd as hip
    import pyoracle as oracle
    rng = np.random.default_rng(100 * bs + bd)
    mx = (1 << bd) - 1
    src, ref = hip.synth.shifted_smooth_pair(W, H, 3 + bd, bd, shift=(2, -3), frac8=(3, 5))
    ref = np.clip(ref.astype(np.int32) + rng.integers(-3 << (bd - 8), (3 << (bd - 8)) + 1, ref.shape), 0, mx).astype(ref.dtype)
    gc = W // bs
    idx = np.arange(gc * gc)[:: max(1, gc * gc // 64)][:64]
    n = len(idx)
    full = np.zeros(n, hip.capi.search_block_dtype)
    full["bx"], full["by"] = (idx % gc) * bs, (idx // gc) * bs
    full["start_row"], full["start_col"] = rng.integers(-5, 6, n), rng.integers(-5, 6, n)
    # ref_mv: both signs, mostly no multiples of 8 (GET_MV_RAWPEL rounds them), on either side of the start MV
    full["ref_row"], full["ref_col"] = -(rng.integers(1, 60, n) | 1), rng.integers(-59, 60, n)
    full["ref_row"][1::4] = rng.integers(3, 60, n)[1::4]
    full["ref_col"][::5] = -21
    full["row_min"], full["row_max"], full["col_min"], full["col_max"] = -24, 24, -24, 24
    full["row_max"][::7] = 2; full["col_min"][::5] = -1
    sub = full.copy()
    sub["start_row"], sub["start_col"] = full["start_row"] * 8, full["start_col"] * 8
    sub["row_min"], sub["row_max"] = sub["start_row"] - rng.integers(3, 40, n), sub["start_row"] + rng.integers(3, 40, n)
    sub["col_min"], sub["col_max"] = sub["start_col"] - rng.integers(3, 40, n), sub["start_col"] + rng.integers(3, 40, n)
    stride = (W + 2 * B + 63) // 64 * 64
    sb, rb = oracle.extend_plane(src, B, stride), oracle.extend_plane(ref, B, stride)
    sp = np.zeros((n, bs, bs), src.dtype)
    for i in range(n):
        y, x = B + full["by"][i] + int(full["start_row"][i]), B + full["bx"][i] + int(full["start_col"][i])
        sp[i] = np.clip(rb[y:y + bs, x:x + bs].astype(np.int32) + rng.integers(-4 << (bd - 8), (4 << (bd - 8)) + 1, (bs, bs)), 0, mx)
    mask = np.clip((np.arange(bs)[None, None, :] * 64 // bs + rng.integers(-6, 7, (n, bs, bs))), 0, 64).astype(np.uint8)
    om = np.full((n, bs, bs), 4096, np.int64)
    om[:, :bs // 2, :] = (np.linspace(36, 64, bs // 2).astype(np.int64) * 64)[None, :, None]
    sblk = np.stack([src[b["by"]:b["by"] + bs, b["bx"]:b["bx"] + bs] for b in full]).astype(np.int64)
    nb = np.clip(sblk + rng.integers(-8 << (bd - 8), (8 << (bd - 8)) + 1, sblk.shape), 0, mx)
    ws = (sblk * 4096 - nb * (4096 - om)).astype(np.int32)
    out = dict(src=src, ref=ref, sb=sb, rb=rb, full=full, sub=sub, n=n, sp=sp, mask=mask, ws=ws, om=om.astype(np.int32))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("family,cost", EMPTY_CELLS)
@pytest.mark.parametrize("bs,bd", [(16, 8), (8, 8), (16, 10)])
def test_cost_type_of_a_family_matches_the_oracle(hip, oracle, ctx, bs, bd, family, cost):
    capi = hip.capi
    s = _cost_scene(bs, bd)
    n, ct = s["n"], COST[cost]
    assert n <= 64
    tj, t0, t1 = _tables()
    tk = dict(mvjcost=tj, mvcost0=t0, mvcost1=t1)
    ps, pr = ctx.planes_alloc(W, H, B, bd, 1), ctx.planes_alloc(W, H, B, bd, 1)
    ctx.planes_upload(ps, 0, s["src"]); ctx.planes_upload(pr, 0, s["ref"])
    sb, rb = oracle.extend_plane(s["src"], B, ps.stride), oracle.extend_plane(s["ref"], B, pr.stride)
    own, tabs = _dev_tables(ctx)
    full, sub = s["full"], s["sub"]
    own += [ctx.to_device(full), ctx.to_device(sub), ctx.to_device(s["sp"]), ctx.to_device(s["mask"]), ctx.to_device(s["ws"]), ctx.to_device(s["om"])]
    d_f, d_s, d_sp, d_m, d_ws, d_om = own[3:]
    outs = [ctx.malloc(n * 4) for _ in range(4)]
    read4 = lambda: (ctx.from_device(outs[0], (n, 2), np.int16), ctx.from_device(outs[1], (n,), np.uint32), ctx.from_device(outs[2], (n,), np.int32),
                     ctx.from_device(outs[3], (n,), np.uint32))
    read3 = lambda: (ctx.from_device(outs[0], (n, 2), np.int16), ctx.from_device(outs[1], (n,), np.int32), ctx.from_device(outs[2], (n,), np.int32))
    if family == "mesh":
        pat = [(16, 4), (8, 2), (4, 1), (3, 1)]
        ctx.mesh_search_batch(ps, pr, 0, bs, bs, ct, pat, 0, d_f, n, outs[0], outs[1])
        got = ctx.from_device(outs[0], (n, 2), np.int16), ctx.from_device(outs[1], (n,), np.int32)
        want = oracle.mesh_search_batch(sb, rb, B, bs, bs, full, pat, 0, ct, bd)
    elif family in ("bilinear_tree", "eighttap_tree"):
        sst = 3 if family == "eighttap_tree" else 0
        ctx.subpel_tree_batch(ps, pr, 0, bs, bs, capi.SubpelParams(2, ct, 63, 2, 1, 0, sst), d_s, n, *outs, None, *tabs)
        got, want = read4(), oracle.subpel_tree_batch(sb, rb, B, bs, bs, sub, tree="tree", cost_type=ct, error_per_bit=63, subpel_search_type=sst, bd=bd, **tk)
    elif family == "compound_refining":
        ctx.refining_search_8p_batch(ps, pr, 0, bs, bs, ct, 23, 71, d_f, n, d_sp, d_m, 0, outs[0], outs[1], outs[2], *tabs)
        got, want = read3(), oracle.refining_search_8p_batch(sb, rb, B, bs, bs, full, s["sp"], s["mask"], 0, cost_type=ct, sad_per_bit=23, error_per_bit=71, bd=bd, **tk)
    elif family == "compound_diamond":
        ctx.compound_full_pixel_search_batch(ps, pr, 0, bs, bs, capi.SearchParams.make("DIAMOND", 4, ct, 23, 71), d_f, n, d_sp, None, 0, outs[0], outs[1], outs[2], *tabs)
        got = ctx.from_device(outs[0], (n, 2), np.int16), ctx.from_device(outs[1], (n,), np.int32), ctx.from_device(outs[2], (n, 2), np.int16)
        want = oracle.compound_full_pixel_search_batch(sb, rb, B, bs, bs, full, oracle.search_params("DIAMOND", 4, ct, 23, 71, no_cost_list=1), s["sp"], None, 0, bd=bd, **tk)
    elif family == "obmc_fullpel":
        ctx.obmc_full_pixel_search_batch(pr, 0, bs, bs, "NSTEP", 4, 0, ct, 19, 55, d_f, n, d_ws, d_om, outs[0], outs[1], *tabs)
        got = ctx.from_device(outs[0], (n, 2), np.int16), ctx.from_device(outs[1], (n,), np.int32)
        want = oracle.obmc_full_pixel_search_batch(rb, B, bs, bs, full, s["ws"], s["om"], "NSTEP", 4, 0, cost_type=ct, sad_per_bit=19, error_per_bit=55, bd=bd, **tk)
    else:
        assert family == "obmc_subpel"
        ctx.obmc_subpel_tree_batch(pr, 0, bs, bs, capi.SubpelParams(2, ct, 63, 2, 1, 0, 0), d_s, n, d_ws, d_om, *outs, *tabs)
        got, want = read4(), oracle.obmc_subpel_tree_batch(rb, B, bs, bs, sub, s["ws"], s["om"], cost_type=ct, error_per_bit=63, bd=bd, **tk)
    _same(got, want, (family, cost, bs, bd))
    for d in own + outs:
        ctx.free(d)
    ctx.planes_free(ps); ctx.planes_free(pr)
