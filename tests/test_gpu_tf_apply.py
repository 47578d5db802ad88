"""aomhip_tf_apply_frames (csrc/tf_apply.hip) == oracle/aomref_tf.c, which tests/test_golden_tf_apply.py pins to the interpreted reference:
the 12-tap predictors, the pixel weights, accum / count and the normalised frame for every 32x32 block of a window -- luma only and with
4:2:0 / 4:2:2 / 4:4:0 / 4:4:4 chroma, 8 / 10 / 12 bits, frames whose size is not a multiple of 32, absent frames, both sides of the
q_factor cutoff, filter_strength 0, and the FRAME_DIFF sums.  The inputs are those of tests/tf_apply_cases.py, whose weights
tests/test_oracle_tf_apply_inputs.py shows to vary (without a GPU).

The bound.  Everything but the weight is integer arithmetic, and the weight (int)(exp(-scaled_error) * 1000) takes a chain of single
IEEE-754 operations on the same operands on both sides, up to exp().  The device's exp() and the host's may differ by a few ulp, and
only where the product lies within ORC_TF_TIE_ULPS = 25 ulp of an integer (oracle/aomref_tf.c derives the figure from the documented
bounds of both and the product's rounding) can that change a weight, by one, and the pixel, by one.  The oracle flags those pixels
(near_tie); every other pixel must equal the oracle EXACTLY.  At about 25 * 2^-52 * 1000 ~ 10^-11 per evaluation no input here has a
flagged pixel -- each case asserts that from the oracle alone -- so the comparison is np.array_equal, FRAME_DIFF included."""
import numpy as np
import pytest

import tf_apply_cases as tc

pytestmark = pytest.mark.gpu


def assert_equal_off_ties(got, want, near_tie, what):
    """Exact where no weight is near a tie; a flagged pixel may differ by one."""
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert not d[~near_tie].any(), (what, int((d[~near_tie] != 0).sum()), int(d.max()), np.argwhere((d != 0) & ~near_tie)[:8].tolist())
    assert not (d[near_tie] > 1).any(), (what, int(d[near_tie].max()))


@pytest.mark.parametrize("W,H,bd,planes,ssx,ssy,q,strength", tc.LEGACY)
def test_apply_frames_equals_oracle(hip, oracle, ctx, W, H, bd, planes, ssx, ssy, q, strength):
    """Frames that are no multiple of 32, an absent frame, the full-pel / x-only / y-only copy paths -- on inputs nearly all of whose
    weights are 0 (tests/tf_apply_cases.py: legacy)."""
    c = tc.case(hip, "legacy-%dx%d-%db-%dp" % (W, H, bd, planes))
    assert (c.ssx, c.ssy, c.q, c.strength) == (ssx, ssy, q, strength)
    _compare(hip, oracle, ctx, c)


@pytest.mark.parametrize("name", tc.NEW_NAMES)
def test_apply_frames_equals_oracle_where_the_weights_vary(hip, oracle, ctx, name):
    """96x64 (3 x 2 blocks: an interior block column, both half-block boundaries), F = 5: flat level + per-pixel noise, content tracked by
    its MVs, and one case per branch of the per-call factors (tests/tf_apply_cases.py)."""
    _compare(hip, oracle, ctx, tc.case(hip, name))


def _compare(hip, oracle, ctx, c):
    name = c.name
    W, H, bd, planes, ssx, ssy, border, filt = c.W, c.H, c.bd, c.planes, c.ssx, c.ssy, c.border, c.filt
    want, st = tc.reference(hip, oracle, name)
    print(name, st.summary())
    tc.assert_weights_matter(c, st)               # from the oracle alone: no near tie; the content families' weights are mostly mid-range
    rings = []
    for p in range(planes):
        w, h = c.plane_size(p)
        ring = ctx.planes_alloc(w, h, border, bd, c.F)
        for f in range(c.F):
            ctx.planes_upload(ring, f, c.frames[p][f])
        rings.append(ring)
    mb_rows, mb_cols, n = c.mb_rows, c.mb_cols, c.n
    assert n == hip.capi.lib.aomhip_tf_block_list(W, H, border, None)
    outs = [ctx.planes_alloc(r.width, r.height, border, bd, 2) for r in rings]
    d_mvs, d_mses, d_diff = ctx.to_device(c.mvs), ctx.to_device(c.mses), ctx.malloc(16)
    params = hip.capi.TfApplyParams.make(c.noise, c.q, c.strength, planes, ssx, ssy)
    ctx.tf_apply_frames(rings, filt, params, n, d_mvs, d_mses, outs, 1, frame_present=c.present, d_diff=d_diff)
    b = border
    for p in range(planes):
        h32, w32 = c.covered(p)
        got = ctx.planes_download(outs[p], 1)   # the whole bordered plane
        g = got[b:b + h32, b:b + w32].astype(np.int64)
        assert_equal_off_ties(g, want[p][b:b + h32, b:b + w32], st.near_tie[p][b:b + h32, b:b + w32], (name, p))
        if p == 0: luma_dev = g
    # FRAME_DIFF: sse of every luma block (source vs filtered), highbd forms rounded to the 8-bit scale
    diff = ctx.from_device(d_diff, (2,), np.int64)
    src = oracle.extend_plane(c.frames[0][filt], border)[b:b + mb_rows * 32, b:b + mb_cols * 32].astype(np.int64)

    def frame_diff(flt):
        sse = ((src - flt) ** 2).reshape(mb_rows, 32, mb_cols, 32).sum(axis=(1, 3))
        if bd == 10: sse = (sse + 8) >> 4
        if bd == 12: sse = (sse + 128) >> 8
        return int(sse.sum()), int((sse * sse).sum())
    # the sums are those of the plane the device wrote ...
    assert (int(diff[0]), int(diff[1])) == frame_diff(luma_dev)
    # ... and the oracle's, exactly
    assert (int(diff[0]), int(diff[1])) == frame_diff(want[0][b:b + mb_rows * 32, b:b + mb_cols * 32].astype(np.int64))
    if c.strength == 0:   # the 1e-5 clamp: every weight 0, the filtered frame is the source
        assert np.array_equal(luma_dev, src) and (int(diff[0]), int(diff[1])) == (0, 0)
    for d_ in (d_mvs, d_mses, d_diff):
        ctx.free(d_)
    for r in rings + outs:
        ctx.planes_free(r)


@pytest.mark.parametrize("W,H,bd", [(1280, 720, 10), (704, 400, 8)])
def test_search_then_apply_stays_on_the_device(hip, oracle, ctx, W, H, bd):
    """The whole temporal filter of one frame as av1_tf_do_filtering_row runs it -- tf_motion_search for every block and window frame, then
    predictor / weights / accumulation / normalisation -- in two calls with the MVs and errors never leaving HBM; the filtered luma frame
    equals the oracle's chain (search oracle -> apply oracle) and so does FRAME_DIFF."""
    from test_gpu_tf import window, GOOD_MESH
    from test_oracle_tf import oracle_params
    F, filt, border, q = 5, 2, 160, 30
    rng = np.random.default_rng(W + bd)
    frames = window(hip, rng, W, H, bd, F)
    ring = ctx.planes_alloc(W, H, border, bd, F)
    for f, fr in enumerate(frames):
        ctx.planes_upload(ring, f, fr)
    out = ctx.planes_alloc(W, H, border, bd, 1)
    blocks = hip.capi.tf_block_list(W, H, border)
    n = len(blocks)
    d_b = ctx.to_device(blocks)
    d_mv, d_mse, d_ref, d_diff = ctx.malloc(F * n * 16), ctx.malloc(F * n * 16), ctx.malloc(n * 4), ctx.malloc(16)
    tp = hip.capi.TfParams.default(W, H, bd, q, 1, GOOD_MESH, subpel_tree=2, iters_per_step=2, allow_hp=1, use_cost_list=0, use_downsampled_sad=0,
                                   force_integer_mv=0)
    ctx.tf_motion_search_frames(ring, filt, tp, d_b, n, d_mv, d_mse, d_ref, None)
    ap = hip.capi.TfApplyParams.make([2.1, 0, 0], q, 5, 1, 0, 0)
    ctx.tf_apply_frames([ring], filt, ap, n, d_mv, d_mse, [out], 0, d_diff=d_diff)
    got = ctx.planes_download(out, 0)
    mvs, mses = ctx.from_device(d_mv, (F, n, 4, 2), np.int16), ctx.from_device(d_mse, (F, n, 4), np.int32)
    host = [oracle.extend_plane(fr, border, ring.stride) for fr in frames]
    (want,), st = oracle.tf_apply_frames([host], border, W, H, filt, mvs, mses, [2.1, 0, 0], q, 5, bd=bd, stats=True)
    print(W, H, bd, st.summary())
    # from the oracle alone: no weight near a tie (the comparison below is exact everywhere), and the weights are live
    assert not st.near_tie[0].any(), (int(st.near_tie[0].sum()), st.min_tie_ulps)
    assert 2 * st.mid[0] >= st.total[0], st.summary()
    h32, w32 = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    sl = (slice(border, border + h32), slice(border, border + w32))
    assert_equal_off_ties(got[sl], want[sl], st.near_tie[0][sl], (W, H, bd))
    # FRAME_DIFF: the oracle's sums (:892-904), which are then also those of the device's own pixels
    sse = ((host[filt][sl].astype(np.int64) - want[sl].astype(np.int64)) ** 2).reshape(h32 // 32, 32, w32 // 32, 32).sum(axis=(1, 3))
    if bd == 10: sse = (sse + 8) >> 4
    diff = ctx.from_device(d_diff, (2,), np.int64)
    assert (int(diff[0]), int(diff[1])) == (int(sse.sum()), int((sse * sse).sum()))
    # the filter did something: the result differs from the source and is closer to the window's mean than the noisy source is
    src = frames[filt].astype(np.int64)
    assert (got[border:border + H, border:border + W].astype(np.int64) != src).mean() > 0.2
    for d_ in (d_b, d_mv, d_mse, d_ref, d_diff):
        ctx.free(d_)
    ctx.planes_free(ring); ctx.planes_free(out)
