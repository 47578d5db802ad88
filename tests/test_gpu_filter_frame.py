"""The deblocking and CDEF kernels against the reference's own FRAME LOOPS (tests/golden/ref_eval_filter_frame.npz: the
interpreted av1_filter_block_plane_vert / _horz in the order of the single-thread row loop, in place, and av1_cdef_fb_row with its
line / column buffers; tests/golden/gen_ref_eval_filter_frame.py).  The product's structure differs from the reference's here (whole
plane, CDEF out of place, no buffers), so equality with these planes is what shows the two are equivalent.

Only the fixture is read and compared with, never the oracle: the host producers run on the stored mode-info grid, the kernels run
on the stored input (CDEF on the device's own deblocked plane in cases A and B), every plane must equal the stored one exactly,
the border of every destination plane must be bytewise what it was before the launch, and CDEF must leave its source alone."""
import numpy as np
import pytest

import filter_frame_fixture as FF

pytestmark = pytest.mark.gpu

BORDER = 32


def _visible(full, w, h):
    return full[BORDER:BORDER + h, BORDER:BORDER + w]


def _border_unchanged(before, after, w, h):
    a, b = before.copy(), after.copy()
    _visible(a, w, h)[:] = 0
    _visible(b, w, h)[:] = 0
    return a.tobytes() == b.tobytes()


def _where(a, b):
    d = np.argwhere(a != b)
    return "%d pixels differ, first at (y, x) = %s" % (len(d), tuple(d[0]) if len(d) else None)


def _maps(hip, oracle, name):
    arrays, cs = FF.case(name)
    grid, f = FF.grid_of(oracle, arrays, cs)      # (oracle: only the compact per-unit description the producer takes, pinned by test_golden_filter_frame.py)
    edges = [FF.product_edge_params(hip.capi.lib, oracle, grid, f, cs, p) for p in range(3)] if cs["deblock"] else None
    skip, strengths = FF.product_cdef_maps(hip.capi.lib, arrays, cs)
    return arrays, cs, edges, skip, strengths


@pytest.mark.parametrize("name", FF.case_names())
def test_two_pass_deblocking_then_cdef(hip, oracle, ctx, name):
    arrays, cs, edges, skip, (pri, sec, uvpri, uvsec) = _maps(hip, oracle, name)
    bd, nplanes = cs["bd"], FF.n_planes(cs)
    planes = []
    # deblocking, in place, the vertical pass and the horizontal pass as two launches
    for p in range(nplanes):
        w, h, _, _ = FF.plane_dims(cs, p)
        pl = ctx.planes_alloc(w, h, BORDER, bd, 2)      # frame 0: CDEF source (deblocked in place); frame 1: CDEF destination
        ctx.planes_upload(pl, 0, arrays["input_%s_p%d" % (name, p)])
        ctx.planes_upload(pl, 1, np.zeros((h, w), np.uint16))
        planes.append(pl)
        if cs["deblock"]:
            before = ctx.planes_download(pl, 0)
            d = ctx.to_device(edges[p])
            ctx.deblock_plane(pl, 0, d, edges[p].shape[1], cs["sharp"], 1)
            ctx.deblock_plane(pl, 0, d, edges[p].shape[1], cs["sharp"], 2)
            after = ctx.planes_download(pl, 0)
            ctx.free(d)
            want = arrays["deblocked_%s_p%d" % (name, p)]
            assert np.array_equal(_visible(after, w, h), want), (name, p, "deblock", _where(_visible(after, w, h), want))
            assert _border_unchanged(before, after, w, h), (name, p, "deblock border")
    # CDEF, out of place, luma first; its directions feed both chroma planes
    W, H = cs["w"], cs["h"]
    fbw = pri.shape[1]
    d_skip, d_pri, d_sec, d_uvpri, d_uvsec = (ctx.to_device(a) for a in (skip, pri, sec, uvpri, uvsec))
    d_dir = ctx.malloc(max((H // 8) * (W // 8), 16))
    src_before = [ctx.planes_download(pl, 0) for pl in planes]
    dst_before = [ctx.planes_download(pl, 1) for pl in planes]
    ctx.cdef_luma_plane(planes[0], 0, planes[0], 1, d_pri, d_sec, fbw, d_skip, cs["damping"], d_dir, None)
    for p in range(1, nplanes):
        ctx.cdef_chroma_plane(planes[p], 0, planes[p], 1, cs["ssx"], cs["ssy"], d_dir, d_uvpri, d_uvsec, fbw, d_skip, cs["damping"])
    for p in range(nplanes):
        w, h, _, _ = FF.plane_dims(cs, p)
        got = ctx.planes_download(planes[p], 1)
        want = arrays["cdef_%s_p%d" % (name, p)]
        assert np.array_equal(_visible(got, w, h), want), (name, p, "cdef", _where(_visible(got, w, h), want))
        assert _border_unchanged(dst_before[p], got, w, h), (name, p, "cdef border")
        assert ctx.planes_download(planes[p], 0).tobytes() == src_before[p].tobytes(), (name, p, "cdef source")
    for d in (d_skip, d_pri, d_sec, d_uvpri, d_uvsec, d_dir):
        ctx.free(d)
    for pl in planes:
        ctx.planes_free(pl)


@pytest.mark.parametrize("name", ["A", "B"])
def test_fused_deblocking(hip, oracle, ctx, name):
    arrays, cs, edges, _, _ = _maps(hip, oracle, name)
    for p in range(3):
        w, h, _, _ = FF.plane_dims(cs, p)
        src, dst = ctx.planes_alloc(w, h, BORDER, cs["bd"], 1), ctx.planes_alloc(w, h, BORDER, cs["bd"], 1)
        ctx.planes_upload(src, 0, arrays["input_%s_p%d" % (name, p)])
        ctx.planes_upload(dst, 0, np.zeros((h, w), np.uint16))
        src_before, dst_before = ctx.planes_download(src, 0), ctx.planes_download(dst, 0)
        d = ctx.to_device(edges[p])
        ctx.deblock_plane_fused(src, 0, dst, 0, d, edges[p].shape[1], cs["sharp"])
        got = ctx.planes_download(dst, 0)
        want = arrays["deblocked_%s_p%d" % (name, p)]
        assert np.array_equal(_visible(got, w, h), want), (name, p, _where(_visible(got, w, h), want))
        assert _border_unchanged(dst_before, got, w, h), (name, p, "border")
        assert ctx.planes_download(src, 0).tobytes() == src_before.tobytes(), (name, p, "source")
        ctx.free(d)
        ctx.planes_free(src); ctx.planes_free(dst)
