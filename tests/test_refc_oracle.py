"""oracle/liboracle.so against the reference compiled as C (oracle/_ref/libaomref_c.so, tests/refc.py) on FRESH inputs: the committed fixtures
pin the oracle at the points an interpreter visited; here both sides get seeded inputs nobody recorded, a few hundred cases per family,
and must agree bit for bit.  The input classes are those of the GPU tests: random, all-max against all-zero, stride != width, odd
offsets, every sub-pel offset, zero / DC-only / extreme coefficients, +-max checkerboards, pixel lines that fire every loop-filter
mask, CDEF_VERY_LARGE borders, saturated planes for the 64-bit sums.

Families here: SAD / variance (all forms of aom_variance_fn_ptr_t), transforms, quantisers, loop filter, CDEF, Wiener statistics, RD
helpers, wedge helpers, av1_get_shear_params, the restoration filters, the projection statistics.  Further down: the TxfmParam dispatchers, the predictors,
the warp family, av1_cdef_filter_fb, and the projection / average / min-max helpers under their callers."""
import ctypes as C

import numpy as np
import pytest

import refc
from conftest import BLOCK_SIZES
from refc import Ptr, PtrList, byteptr, call, fn
from refc_inputs import TxfmParam  # noqa: F401  (the mirror that param() fills)
from refc_inputs import (FORMS, NC, TX, ConvolveParams, Jcp, SgrParams, WarpedMotionParams, coeff_classes, coeffs_for_inverse, fp_tables,
                         lpf_patch, param, pixels, residual_classes, wide, cdef_fb_reference)

U = C.c_uint
SSZ = C.c_ssize_t
VP = lambda a, at=0: C.c_void_p(a.ctypes.data + at * a.itemsize)


def o(oracle, name, restype=None):
    f = oracle.lib[name]
    f.restype = restype
    return f


# ---------------------------------------------------------------- SAD / variance

def sad_blocks(rng, w, h, bd, kind):
    dt, mx = (np.uint8, 255) if bd == 8 else (np.uint16, (1 << bd) - 1)
    a = rng.integers(0, mx + 1, (h + 3, w + 5)).astype(dt)     # stride != width, origin at an odd offset
    b = rng.integers(0, mx + 1, (h + 7, w + 11)).astype(dt)
    if kind == "max-zero":
        a[:] = mx; b[:] = 0
    if kind == "zero-max":
        a[:] = 0; b[:] = mx
    return a, b


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_sad_variance_every_size(oracle, bd):
    refc.lib()
    rng = np.random.default_rng(100 + bd)
    hb = bd > 8
    pre, vpre = ("aom_highbd_", "aom_highbd_%d_" % bd) if hb else ("aom_", "aom_")
    n = 0
    for (w, h) in BLOCK_SIZES:
        wh = "%dx%d" % (w, h)
        for kind in ("random", "random", "max-zero", "zero-max"):
            a, b = sad_blocks(rng, w, h, bd, kind)
            S, R = a.shape[1], b.shape[1]
            ay, ax, by, bx = 1, 1, 3, 5
            A, B = Ptr(a, ay * S + ax, hb), Ptr(b, by * R + bx, hb)
            assert oracle.sad(a, ay, ax, b, by, bx, w, h, bd=8) == call(fn(pre + "sad%s_c" % wh, U), A, S, B, R), (wh, kind)
            assert oracle.sad(a, ay, ax, b, by, bx, w, h, skip=True, bd=8) == call(fn(pre + "sad_skip_%s_c" % wh, U), A, S, B, R), (wh, kind)
            offs = [(by, bx), (by + 1, bx), (by, bx + 1), (0, 0)]
            for form in ("sad%sx4d", "sad%sx3d", "sad_skip_%sx4d"):
                out = np.full(5, 9, np.uint32)
                call(fn(pre + form % wh + "_c"), A, S, PtrList([Ptr(b, y * R + x, hb) for y, x in offs]), R, out)
                want = [oracle.sad(a, ay, ax, b, y, x, w, h, skip="skip" in form, bd=8) for y, x in offs]
                assert out.tolist() == want + [9], (form, wh, kind)
            sse = np.zeros(1, np.uint32)
            v, wsse, wsum = oracle.variance(a, ay, ax, b, by, bx, w, h, bd=bd)
            assert (v, wsse) == (call(fn(vpre + "variance%s_c" % wh, U), A, S, B, R, sse), int(sse[0])), (wh, kind)
            if (w, h) in ((16, 16), (16, 8), (8, 16), (8, 8)):
                assert call(fn(vpre + "mse%s_c" % wh, U), A, S, B, R, sse) == wsse == int(sse[0])
            if bd == 8 and w == h and w in (8, 16):
                sm = np.zeros(1, np.int32)
                call(fn("aom_get%sx%svar_c" % (w, w)), A, S, B, R, sse, sm)
                assert (int(sse[0]), int(sm[0])) == (wsse, wsum)
            offsets = [(x, y) for x in range(8) for y in range(8)] if (w, h) in ((4, 4), (16, 8), (128, 128)) and kind == "random" \
                else [(int(rng.integers(0, 8)), int(rng.integers(0, 8))), (0, 0), (4, 4)]
            for xo, yo in offsets:
                got = call(fn(vpre + "sub_pixel_variance%s_c" % wh, U), B, R, xo, yo, A, S, sse)
                assert oracle.sub_pixel_variance(b, by, bx, xo, yo, a, ay, ax, w, h, bd=bd) == (got, int(sse[0])), (wh, kind, xo, yo)
            n += 1
    assert n == 22 * 4


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_compound_masked_obmc_forms_every_size(oracle, bd):
    """sdaf / jsdaf / svaf / jsvaf / msdf / msvf / osdf / ovf / osvf of aom_variance_fn_ptr_t"""
    refc.lib()
    rng = np.random.default_rng(200 + bd)
    hb, e16 = bd > 8, int(bd > 8)
    dt, mx = (np.uint16, (1 << bd) - 1) if hb else (np.uint8, 255)
    spre, vpre = ("aom_highbd_", "aom_highbd_%d_" % bd) if hb else ("aom_", "aom_")
    csv = o(oracle, "orc_compound_sub_pixel_variance", C.c_uint32)
    msad, osad, ovar = o(oracle, "orc_masked_sad", U), o(oracle, "orc_obmc_sad", U), o(oracle, "orc_obmc_variance", C.c_uint32)
    q = C.c_uint32()
    n = 0
    for (w, h) in BLOCK_SIZES:
        wh = "%dx%d_c" % (w, h)
        for kind in ("random", "saturated"):
            S = w + 9
            a, b = rng.integers(0, mx + 1, (h + 4, S)).astype(dt), rng.integers(0, mx + 1, (h + 4, S)).astype(dt)
            sp = rng.integers(0, mx + 1, w * h).astype(dt)
            mask = rng.integers(0, 65, (h, w + 2)).astype(np.uint8)
            ws, om = rng.integers(0, mx * 4096 + 1, w * h).astype(np.int32), rng.integers(0, 4097, w * h).astype(np.int32)
            if kind == "saturated":
                a[:] = mx; b[:] = 0; sp[:] = 0; mask[:] = 64; ws[:] = mx * 4096; om[:] = 4096
            A, B, SP = Ptr(a, S + 1, hb), Ptr(b, 2 * S + 3, hb), Ptr(sp, 0, hb)
            Ao, Bo = VP(a, S + 1), VP(b, 2 * S + 3)
            xo, yo, inv = int(rng.integers(0, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 2))
            if (w, h) in ((4, 4), (16, 8), (128, 128)):     # every sub-pel offset for the avg forms
                sse = np.zeros(1, np.uint32)
                for sx in range(8):
                    for sy in range(8):
                        got = call(fn(vpre + "sub_pixel_avg_variance" + wh, U), B, S, sx, sy, A, S, sse, SP)
                        assert (csv(Bo, S, sx, sy, Ao, S, w, h, e16, bd, 0, VP(sp), 0, 0, None, 0, 0, C.byref(q)), q.value) == (got, int(sse[0])), ("svaf", w, h, sx, sy)
                        if kind == "random":
                            jc = Jcp(1, 9 + (sx + sy) % 5, 7 - (sx + sy) % 5)
                            got = call(fn(vpre + "dist_wtd_sub_pixel_avg_variance" + wh, U), B, S, sx, sy, A, S, sse, SP, jc)
                            assert (csv(Bo, S, sx, sy, Ao, S, w, h, e16, bd, 1, VP(sp), jc.fwd_offset, jc.bck_offset, None, 0, 0, C.byref(q)), q.value) == \
                                (got, int(sse[0])), ("jsvaf", w, h, sx, sy)
                            got = call(fn(vpre + "masked_sub_pixel_variance" + wh, U), B, S, sx, sy, A, S, SP, mask, w + 2, inv, sse)
                            assert (csv(Bo, S, sx, sy, Ao, S, w, h, e16, bd, 2, VP(sp), 0, 0, VP(mask), w + 2, inv, C.byref(q)), q.value) == (got, int(sse[0]))
                            got = call(fn(vpre + "obmc_sub_pixel_variance" + wh, U), B, S, sx, sy, ws, om, sse)
                            assert (ovar(Bo, S, 1, sx, sy, VP(ws), VP(om), w, h, e16, bd, C.byref(q)), q.value) == (got, int(sse[0])), ("osvf", w, h, sx, sy)
            fwd, bck = [(9, 7), (11, 5), (12, 4), (13, 3)][int(rng.integers(0, 4))]
            sse = np.zeros(1, np.uint32)
            # SAD forms: source a, reference b (raw kernel values: bd 8 asks the oracle for no wrapper shift)
            cand = np.zeros(1, dtype=[("sx", "<i2"), ("sy", "<i2"), ("rx", "<i2"), ("ry", "<i2")])
            cand["sx"], cand["sy"], cand["rx"], cand["ry"] = 1, 1, 3, 2
            sp3 = sp.reshape(1, h, w)
            assert int(oracle.sad_avg_batch(a, b, 0, w, h, cand, sp3, [0], bd=8)[0]) == call(fn(spre + "sad%dx%d_avg_c" % (w, h), U), A, S, B, S, SP)
            got = call(fn(spre + "dist_wtd_sad%dx%d_avg_c" % (w, h), U), A, S, B, S, SP, Jcp(1, fwd, bck))
            assert int(oracle.sad_avg_batch(a, b, 0, w, h, cand, sp3, [0], fwd_offset=fwd, bck_offset=bck, bd=8)[0]) == got, (w, h, kind)
            assert msad(Ao, S, Bo, S, VP(sp), VP(mask), w + 2, inv, w, h, e16, 8) == call(fn(spre + "masked_sad" + wh, U), A, S, B, S, SP, mask, w + 2, inv)
            assert osad(Bo, S, VP(ws), VP(om), w, h, e16, 8) == call(fn(spre + "obmc_sad" + wh, U), B, S, ws, om)
            # variance forms: b is interpolated, a is the other block
            got = call(fn(vpre + "sub_pixel_avg_variance" + wh, U), B, S, xo, yo, A, S, sse, SP)
            assert (csv(Bo, S, xo, yo, Ao, S, w, h, e16, bd, 0, VP(sp), 0, 0, None, 0, 0, C.byref(q)), q.value) == (got, int(sse[0])), ("svaf", w, h, kind)
            got = call(fn(vpre + "dist_wtd_sub_pixel_avg_variance" + wh, U), B, S, xo, yo, A, S, sse, SP, Jcp(1, fwd, bck))
            assert (csv(Bo, S, xo, yo, Ao, S, w, h, e16, bd, 1, VP(sp), fwd, bck, None, 0, 0, C.byref(q)), q.value) == (got, int(sse[0])), ("jsvaf", w, h)
            got = call(fn(vpre + "masked_sub_pixel_variance" + wh, U), B, S, xo, yo, A, S, SP, mask, w + 2, inv, sse)
            assert (csv(Bo, S, xo, yo, Ao, S, w, h, e16, bd, 2, VP(sp), 0, 0, VP(mask), w + 2, inv, C.byref(q)), q.value) == (got, int(sse[0])), ("msvf", w, h)
            got = call(fn(vpre + "obmc_variance" + wh, U), B, S, ws, om, sse)
            assert (ovar(Bo, S, 0, 0, 0, VP(ws), VP(om), w, h, e16, bd, C.byref(q)), q.value) == (got, int(sse[0])), ("ovf", w, h, kind)
            got = call(fn(vpre + "obmc_sub_pixel_variance" + wh, U), B, S, xo, yo, ws, om, sse)
            assert (ovar(Bo, S, 1, xo, yo, VP(ws), VP(om), w, h, e16, bd, C.byref(q)), q.value) == (got, int(sse[0])), ("osvf", w, h, kind)
            n += 1
    assert n == 44 and len(FORMS) == 16


# ---------------------------------------------------------------- transforms

def test_fwd_and_inv_txfm2d_every_size_type_depth(oracle):
    refc.lib()
    rng = np.random.default_rng(300)
    n_fwd = n_inv = 0
    for tx_size, (w, h) in enumerate(TX):
        nc = NC[tx_size]
        for tx_type in range(16):
            if not oracle.av1_tx_valid(tx_size, tx_type):
                continue
            for bd in (8, 10, 12):
                for kind, res in residual_classes(rng, w, h, w, bd)[:5 if tx_type in (0, 9) else 1]:
                    out = np.zeros(w * h, np.int32)
                    call(fn("av1_fwd_txfm2d_%dx%d_c" % (w, h)), res, out, w, tx_type, bd)
                    assert np.array_equal(oracle.fwd_txfm2d(res, tx_size, tx_type, bd)[:nc], out[:nc]), ("fwd", w, h, tx_type, bd, kind)
                    n_fwd += 1
                for kind in ("random", "zero", "dc", "extreme")[:4 if tx_type in (0, 9) else 1]:
                    co = coeffs_for_inverse(rng, tx_size, bd, kind)
                    dst = pixels(rng, h, w, bd, kind, np.uint16)
                    want = dst.copy()
                    call(fn("av1_inv_txfm2d_add_%dx%d_c" % (w, h)), co, want, w, tx_type, bd)
                    assert np.array_equal(oracle.inv_txfm2d_add(co[:nc], dst, tx_size, tx_type, bd), want), ("inv", w, h, tx_type, bd, kind)
                    n_inv += 1
    assert n_fwd == 873 and n_inv == 774, (n_fwd, n_inv)


def test_lossless_transforms(oracle):
    refc.lib()
    rng = np.random.default_rng(301)
    fw, iw = o(oracle, "orc_fwht4x4"), o(oracle, "orc_iwht4x4_add")
    for trial in range(200):
        res = rng.integers(-255, 256, (4, 4)).astype(np.int16)
        if trial % 4 == 0:
            res[:] = rng.choice([-255, 255], (4, 4))
        got, want = np.zeros(16, np.int32), np.zeros(16, np.int32)
        fw(VP(res), VP(got), 4)
        call(fn("av1_fwht4x4_c"), res, want, 4)
        assert np.array_equal(got, want), trial
        bd, eob = (8, 10, 12)[trial % 3], (0, 1, 2, 16)[trial % 4]
        co = rng.integers(-(1 << (bd + 2)), 1 << (bd + 2), 16).astype(np.int32)
        dst = pixels(rng, 4, 4, bd, "extreme" if trial % 7 == 0 else "random", np.uint16)
        got, want = dst.copy(), dst.copy()
        iw(VP(co), VP(got), 4, eob, bd)
        call(fn("av1_highbd_iwht4x4_add"), co, byteptr(want), 4, eob, bd)
        assert np.array_equal(got, want), (trial, bd, eob)


# ---------------------------------------------------------------- quantisers

def test_quantize_b_family(oracle):
    refc.lib()
    rng = np.random.default_rng(400)
    n = 0
    for hbd in (0, 1):
        for adaptive in (0, 1):
            for tx_size, suffix, ls in ((0, "", 0), (1, "", 0), (2, "", 0), (7, "", 0), (3, "_32x32", 1), (9, "_32x32", 1), (4, "_64x64", 2)):
                name = "aom_%squantize_b%s%s_c" % ("highbd_" if hbd else "", suffix, "_adaptive" if adaptive else "")
                sc, isc = oracle.get_scan(tx_size, 0)
                m = len(sc)
                for qindex in (0, 20, 255):
                    q = oracle.build_quantizer_y(10 if hbd else 8, qindex)
                    t = wide(q)
                    for co in coeff_classes(rng, m, sc, q["dequant"][1], ls, 200000 if hbd else 8191):
                        qc, dq, eob = np.full(m, 77, np.int32), np.full(m, 77, np.int32), np.full(1, 9, np.uint16)
                        call(fn(name), co, SSZ(m), t["zbin"], t["round"], t["quant"], t["quant_shift"], qc, dq, t["dequant"], eob, sc, isc)
                        got = oracle.quantize_b_adaptive(co, q, sc, ls, highbd=bool(hbd)) if adaptive else oracle.quantize_b(co, q, sc, isc, ls, highbd=bool(hbd))
                        assert np.array_equal(got[0], qc) and np.array_equal(got[1], dq) and got[2] == eob[0], (name, tx_size, qindex)
                        n += 1
    assert n == 756


def test_quantize_fp_lp_and_qm(oracle):
    refc.lib()
    rng = np.random.default_rng(401)
    ofp, olp = o(oracle, "orc_quantize_fp"), o(oracle, "orc_quantize_lp")
    n = 0
    for tx_size, ls in ((0, 0), (1, 0), (2, 0), (7, 0), (3, 1), (9, 1), (4, 2)):
        sc, isc = oracle.get_scan(tx_size, 0)
        m = len(sc)
        for qindex in (0, 20, 100, 255):
            for hbd in (0, 1):
                q = oracle.build_quantizer_y(10 if hbd else 8, qindex)
                f2 = fp_tables(q)
                t = wide(f2)
                qm = rng.integers(1, 256, m).astype(np.uint8); iqm = rng.integers(1, 256, m).astype(np.uint8)
                for co in coeff_classes(rng, m, sc, q["dequant"][1], ls, 200000 if hbd else 8191):
                    qc, dq, eob = np.full(m, 77, np.int32), np.full(m, 77, np.int32), np.full(1, 9, np.uint16)
                    args = [co, SSZ(m), t["zbin"], t["round"], t["quant"], t["quant_shift"], qc, dq, t["dequant"], eob, sc, isc]
                    if hbd:
                        call(fn("av1_highbd_quantize_fp_c"), *args, ls)
                    else:
                        call(fn("av1_quantize_fp" + ("", "_32x32", "_64x64")[ls] + "_c"), *args)
                    gq, gd, ge = np.zeros_like(co), np.zeros_like(co), C.c_uint16()
                    ofp(VP(co), SSZ(m), VP(f2["round"]), VP(f2["quant"]), VP(gq), VP(gd), VP(f2["dequant"]), C.byref(ge), VP(sc), ls, hbd)
                    assert np.array_equal(gq, qc) and np.array_equal(gd, dq) and ge.value == eob[0], ("fp", tx_size, qindex, hbd)
                    # the b quantiser with quantisation matrices (aom_[highbd_]quantize_b_helper_c)
                    tb = wide(q)
                    call(fn("aom_highbd_quantize_b_helper_c" if hbd else "aom_quantize_b_helper_c"), co, SSZ(m), tb["zbin"], tb["round"], tb["quant"],
                         tb["quant_shift"], qc, dq, tb["dequant"], eob, sc, isc, qm, iqm, ls)
                    got = oracle.quantize_b(co, q, sc, isc, ls, highbd=bool(hbd), qm=qm, iqm=iqm)
                    assert np.array_equal(got[0], qc) and np.array_equal(got[1], dq) and got[2] == eob[0], ("qm", tx_size, qindex, hbd)
                    if not hbd and ls == 0:
                        c16 = np.clip(co, -32768, 32767).astype(np.int16)
                        q16, d16 = np.full(m, 5, np.int16), np.full(m, 5, np.int16)
                        call(fn("av1_quantize_lp_c"), c16, SSZ(m), t["round"], t["quant"], q16, d16, t["dequant"], eob, sc, isc)
                        g16, h16 = np.zeros(m, np.int16), np.zeros(m, np.int16)
                        olp(VP(c16), SSZ(m), VP(f2["round"]), VP(f2["quant"]), VP(g16), VP(h16), VP(f2["dequant"]), C.byref(ge), VP(sc))
                        assert np.array_equal(g16, q16) and np.array_equal(h16, d16) and ge.value == eob[0], ("lp", tx_size, qindex)
                    n += 1
    assert n == 504


# ---------------------------------------------------------------- loop filter, CDEF

def test_lpf_all_forty(oracle):
    refc.lib()
    rng = np.random.default_rng(500)
    n = 0
    for hb in ("", "highbd_"):
        for direction, vertical in (("horizontal", 0), ("vertical", 1)):
            for length in (4, 6, 8, 14):
                for kind, units in (("", 1), ("_dual", 2)) + ((("_quad", 4),) if not hb else ()):
                    for bd in ((10, 12) if hb else (8,)):
                        for trial in range(18 if not hb else 9):
                            lim = [int(rng.integers(0, 3 * 63 + 5)), int(rng.integers(0, 64)), int(rng.integers(0, 16)),
                                   int(rng.integers(0, 3 * 63 + 5)), int(rng.integers(0, 64)), int(rng.integers(0, 16))]
                            if trial == 1:
                                lim = [255, 63, 0] * 2
                            thr = [np.full(16, v, np.uint8) for v in lim]
                            px = lpf_patch(rng, bd, ("random", "flat", "flat", "step", "checker", "flat")[trial % 6])
                            want, got = px.copy(), px.copy()
                            args = [Ptr(want, 16 * 32 + 16), 32, thr[0], thr[1], thr[2]] + (thr[3:] if kind == "_dual" else []) + ([bd] if hb else [])
                            call(fn("aom_%slpf_%s_%d%s_c" % (hb, direction, length, kind)), *args)
                            for unit in range(units):
                                t = lim[3:] if (kind == "_dual" and unit == 1) else lim[:3]
                                oy, ox = (16 + 4 * unit, 16) if vertical else (16, 16 + 4 * unit)
                                oracle.lpf_edge(got, oy, ox, vertical, length, t[0], t[1], t[2], bd=bd)
                            assert np.array_equal(got, want), (hb, direction, length, kind, bd, trial)
                            n += 1
    assert n == 24 * 18 + 16 * 18


def test_cdef_find_dir_and_filters(oracle):
    refc.lib()
    rng = np.random.default_rng(501)
    for bd in (8, 10, 12):
        for trial in range(40):
            img = rng.integers(0, 1 << bd, (8, 8)).astype(np.uint16)
            if trial % 3 == 0:
                yy, xx = np.mgrid[0:8, 0:8]
                img = np.clip(((yy * (trial % 5) + xx * 3) % 64) << (bd - 6), 0, (1 << bd) - 1).astype(np.uint16)
            if trial == 1:
                img[:] = (1 << bd) - 1
            var = np.zeros(1, np.int32)
            d = call(fn("cdef_find_dir_c", C.c_int), img, 8, var, bd - 8)
            assert oracle.cdef_find_dir(img, bd - 8) == (d, int(var[0])), (bd, trial)
    f = o(oracle, "orc_cdef_filter_block")
    n = 0
    for bits, is16 in ((8, 0), (16, 1)):
        for variant in range(4):
            for trial in range(40):
                bd = 8 if not is16 else (10, 12)[trial % 2]
                bw, bh = [(8, 8), (4, 4), (8, 4), (4, 8)][trial % 4]
                buf = rng.integers(0, 1 << bd, (16, 144)).astype(np.uint16)
                if trial % 2:
                    buf[:, :3] = 0x4000; buf[:2, :] = 0x4000  # CDEF_VERY_LARGE outside the frame
                if trial % 6 == 3:
                    buf[:, 4 + bw:] = 0x4000; buf[3 + bh:, :] = 0x4000
                pri = int(rng.integers(1, 16)) << (bd - 8) if variant in (0, 1) else 0
                sec = int(rng.choice([1, 2, 4])) << (bd - 8) if variant in (0, 2) else 0
                dirn, pd, sd = int(rng.integers(0, 8)), int(rng.integers(3, 7)) + (bd - 8), int(rng.integers(3, 7)) + (bd - 8)
                want = np.full((bh, 11), 99, np.uint16 if is16 else np.uint8)
                got = want.copy()
                call(fn("cdef_filter_%d_%d_c" % (bits, variant)), want, 11, Ptr(buf, 3 * 144 + 4), pri, sec, dirn, pd, sd, bd - 8, bw, bh)
                f(None if is16 else VP(got), VP(got) if is16 else None, 11, VP(buf, 3 * 144 + 4), pri, sec, dirn, pd, sd, bd - 8, bw, bh,
                  int(variant in (0, 1)), int(variant in (0, 2)))
                assert np.array_equal(got, want), (bits, variant, trial)
                n += 1
    assert n == 320


# ---------------------------------------------------------------- Wiener statistics, RD helpers

def test_wiener_statistics(oracle):
    """av1_compute_stats_c (full and down-sampled rows) / av1_compute_stats_highbd_c, 7 x 7 and 5 x 5, random and 0 / max checkerboard"""
    refc.lib()
    rng = np.random.default_rng(600)
    f = o(oracle, "orc_compute_stats")
    n = 0
    for bd in (8, 10, 12):
        hb = bd > 8
        dt, mx = (np.uint16, (1 << bd) - 1) if hb else (np.uint8, 255)
        for win in (7, 5):
            for kind in ("random", "checker"):
                for down in ((0, 1) if not hb else (0,)):
                    dgd, src = rng.integers(0, mx + 1, (40, 48)).astype(dt), rng.integers(0, mx + 1, (40, 44)).astype(dt)
                    if kind == "checker":
                        yy, xx = np.mgrid[0:40, 0:48]
                        dgd = (((yy + xx) & 1) * mx).astype(dt); src[:] = mx - dgd[:, :44]
                    hs, he, vs, ve = 4, 4 + int(rng.integers(9, 33)), 4, 4 + int(rng.integers(9, 30))
                    M, H = np.zeros(49, np.int64), np.zeros(49 * 49, np.int64)
                    if hb:
                        call(fn("av1_compute_stats_highbd_c"), win, byteptr(dgd), byteptr(src), hs, he, vs, ve, 48, 44, M, H, bd)
                    else:
                        call(fn("av1_compute_stats_c"), win, dgd, src, hs, he, vs, ve, 48, 44, M, H, down)
                    gM, gH = np.zeros(win * win, np.int64), np.zeros(win ** 4, np.int64)
                    f(win, VP(dgd), VP(src), hs, he, vs, ve, 48, 44, int(hb), bd, down, VP(gM), VP(gH))
                    assert np.array_equal(gM, M[:win * win]) and np.array_equal(gH, H[:win ** 4]), (bd, win, kind, down)
                    n += 1
    assert n == 16


def test_rd_helpers(oracle):
    """block errors, Hadamard / SATD, aom_[highbd_]sse, av1_txb_init_levels and the residual sums.  aom_sum_sse_2d_i16_c ADDS to *sum
    (aom_dsp/sum_squares.c); the oracle's orc_sum_sse_2d_i16 does the same, the product's aomhip_sum_sse_2d_i16 overwrites (ADVICE.md,
    fourth finding): the last assertion of the loop states the difference."""
    refc.lib()
    rng = np.random.default_rng(700)
    be, belp = o(oracle, "orc_block_error", C.c_int64), o(oracle, "orc_block_error_lp", C.c_int64)
    for n in (16, 17, 64, 100, 1024, 4096):
        for span in (100, 1 << 12, 1 << 15, 1 << 19):
            c = rng.integers(-span, span, n).astype(np.int32)
            d = (c + rng.integers(-span // 4 - 1, span // 4 + 1, n)).astype(np.int32)
            for bd in (0, 8, 10, 12):
                if bd == 0 and span > 1 << 15:
                    continue        # av1_block_error_c squares in `int`: undefined in compiled C past 31 bits
                gs, ws = C.c_int64(), np.zeros(1, np.int64)
                want = call(fn("av1_block_error_c", C.c_int64), c, d, SSZ(n), ws) if bd == 0 else \
                    call(fn("av1_highbd_block_error_c", C.c_int64), c, d, SSZ(n), ws, bd)
                assert (be(VP(c), VP(d), SSZ(n), C.byref(gs), bd), gs.value) == (want, int(ws[0])), (n, span, bd)
            if span <= 1 << 15:
                c16, d16 = np.clip(c, -32768, 32767).astype(np.int16), np.clip(d // 2, -32768, 32767).astype(np.int16)
                assert belp(VP(c16), VP(d16), SSZ(n)) == call(fn("av1_block_error_lp_c", C.c_int64), c16, d16, SSZ(n)), (n, span)
    had = o(oracle, "orc_hadamard", C.c_int)
    names = {0: "aom_hadamard_%dx%d_c", 1: "aom_hadamard_lp_%dx%d_c", 2: "aom_highbd_hadamard_%dx%d_c"}
    for flavour, sizes in ((0, (4, 8, 16, 32)), (1, (8, 16)), (2, (8, 16, 32))):
        for n in sizes:
            for trial in range(12):
                span = (255, 4095, 32767)[trial % 3] if flavour != 1 else (255, 1023)[trial % 2]
                r = rng.integers(-span, span + 1, (n + 2, n + 5)).astype(np.int16)
                if trial >= 9:
                    yy, xx = np.mgrid[0:n + 2, 0:n + 5]; r = np.where((yy + xx) & 1, span, -span).astype(np.int16)
                want = np.zeros(n * n, np.int16 if flavour == 1 else np.int32)
                call(fn(names[flavour] % (n, n)), Ptr(r, n + 5 + 2), SSZ(n + 5), want)
                got = np.zeros(n * n, np.int32)
                satd = had(VP(r, n + 5 + 2), SSZ(n + 5), n, flavour, VP(got))
                assert np.array_equal(got, want.astype(np.int32)), (flavour, n, trial)
                assert satd == call(fn("aom_satd_lp_c" if flavour == 1 else "aom_satd_c", C.c_int), want, n * n), (flavour, n, trial)
    sse = o(oracle, "orc_sse", C.c_int64)
    for bd in (8, 12):
        hb = bd > 8
        dt, mx = (np.uint16, 4095) if hb else (np.uint8, 255)
        for (w, h) in BLOCK_SIZES + [(12, 20), (24, 6)]:
            a, b = rng.integers(0, mx + 1, (h + 2, w + 7)).astype(dt), rng.integers(0, mx + 1, (h + 2, w + 7)).astype(dt)
            if w == h:
                a[:] = mx; b[:] = 0
            want = call(fn("aom_highbd_sse_c" if hb else "aom_sse_c", C.c_int64), Ptr(a, w + 8, hb), w + 7, Ptr(b, 2, hb), w + 7, w, h)
            assert sse(VP(a, w + 8), w + 7, VP(b, 2), w + 7, w, h, int(hb)) == want, (bd, w, h)
    lv = o(oracle, "orc_txb_init_levels")
    for (w, h) in ((4, 4), (8, 8), (16, 16), (32, 32), (4, 16), (16, 4), (8, 32), (32, 8), (16, 32)):
        co = (rng.integers(-300, 301, w * h) * (rng.random(w * h) < 0.5)).astype(np.int32)
        size = (w + 4) * (h + 4) + 16
        got, want = np.full(size, 0xAA, np.uint8), np.full(size, 0xAA, np.uint8)
        lv(VP(co), w, h, VP(got))
        call(fn("av1_txb_init_levels_c"), co, w, h, want)
        assert np.array_equal(got, want), (w, h)
    osum = o(oracle, "orc_sum_sse_2d_i16", C.c_uint64)
    for (w, h) in ((4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (4, 16), (64, 16), (16, 64)):
        for span in (255, 4095, 32767):
            r = rng.integers(-span, span + 1, (h + 1, w + 3)).astype(np.int16)
            if span == 32767:
                r[:] = -32768      # saturated: 128 x 128 x 2^30 = 2^44 needs the 64-bit sum
            start = 12345
            gs, ws = C.c_int(start), np.asarray([start], np.int32)
            want = call(fn("aom_sum_sse_2d_i16_c", C.c_uint64), Ptr(r, 1), w + 3, w, h, ws)
            assert (osum(VP(r, 1), w + 3, w, h, C.byref(gs)), gs.value) == (want, int(ws[0])), (w, h, span)
            assert want == call(fn("aom_sum_squares_2d_i16_c", C.c_uint64), Ptr(r, 1), w + 3, w, h)
            # the reference accumulates: started from 12345 it ends at 12345 + the block's sum (an overwriting entry point would not)
            block_sum = int(r[:h, 1:w + 1].astype(np.int64).sum())
            assert int(ws[0]) == (start + block_sum + 2 ** 31) % 2 ** 32 - 2 ** 31 and (block_sum == 0 or int(ws[0]) != block_sum)


def test_wedge_helpers(oracle):
    refc.lib()
    rng = np.random.default_rng(800)
    wsse, wsign = o(oracle, "orc_wedge_sse_from_residuals", C.c_uint64), o(oracle, "orc_wedge_sign_from_residuals", C.c_int)
    wds = o(oracle, "orc_wedge_compute_delta_squares")
    n = 0
    for N in (64, 128, 256, 1024, 4096, 16384):
        for span in (255, 4095, 32767):
            r1, d = rng.integers(-span, span + 1, N).astype(np.int16), rng.integers(-span, span + 1, N).astype(np.int16)
            m = rng.integers(0, 65, N).astype(np.uint8)
            if span == 32767:       # saturated: every term at its largest
                r1[:] = 32767; d[:] = -32768; m[:] = 64
            assert wsse(VP(r1), VP(d), VP(m), N) == call(fn("av1_wedge_sse_from_residuals_c", C.c_uint64), r1, d, m, N), (N, span)
            a, b = rng.integers(-span, span + 1, N).astype(np.int16), rng.integers(-span, span + 1, N).astype(np.int16)
            got, want = np.zeros(N, np.int16), np.zeros(N, np.int16)
            wds(VP(got), VP(a), VP(b), N)
            call(fn("av1_wedge_compute_delta_squares_c"), want, a, b, N)
            assert np.array_equal(got, want), (N, span)
            acc = int((want.astype(np.int64) * m).sum())
            for limit in (acc - 1, acc, acc + 1, 0, -(1 << 40)):
                assert wsign(VP(want), VP(m), N, C.c_int64(limit)) == call(fn("av1_wedge_sign_from_residuals_c", C.c_int8), want, m, N, C.c_int64(limit))
                n += 1
    assert n == 90


def test_get_shear_params_with_degenerate_models(oracle):
    """av1_get_shear_params on ordinary and degenerate models (first finding): mat[2] <= 0, mat[2] = 1 and INT32_MAX, products that
    reach the int16 clamps, and models on both sides of is_affine_shear_allowed.  Where the reference rejects a model at is_affine_valid
    it leaves alpha .. delta untouched; the four values are compared whenever it got past that."""
    refc.lib()
    rng = np.random.default_rng(801)
    f = o(oracle, "orc_get_shear_params", C.c_int)
    models = []
    for trial in range(300):
        m = [int(rng.integers(-(1 << 20), 1 << 20)), int(rng.integers(-(1 << 20), 1 << 20)), (1 << 16) + int(rng.integers(-(1 << 13), 1 << 13)),
             int(rng.integers(-(1 << 13), 1 << 13)), int(rng.integers(-(1 << 13), 1 << 13)), (1 << 16) + int(rng.integers(-(1 << 13), 1 << 13))]
        if trial % 5 == 0:
            m[2:] = [int(v) for v in rng.integers(-(1 << 18), 1 << 18, 4)]
        models.append(m)
    for m2 in (0, -1, -(1 << 31), 1, 2, 255, 256, 257, (1 << 31) - 1, 1 << 30, (1 << 16) - 1):
        for m3, m4, m5 in ((0, 0, 1 << 16), (32767, -32768, 1 << 16), ((1 << 31) - 1, (1 << 31) - 1, -(1 << 31)), (-(1 << 31), (1 << 31) - 1, (1 << 31) - 1)):
            models.append([0, 0, m2, m3, m4, m5])
    ok = bad = 0
    for m in models:
        wm = WarpedMotionParams((C.c_int32 * 6)(*m), 11, 22, 33, 44, 3, 0)
        want = call(fn("av1_get_shear_params", C.c_int), wm)
        mat, out = np.asarray(m, np.int32), np.asarray([11, 22, 33, 44], np.int16)
        got = f(VP(mat), VP(out))
        assert got == want, (m, got, want)
        if m[2] > 0:
            assert out.tolist() == [wm.alpha, wm.beta, wm.gamma, wm.delta], (m, out.tolist())
        else:
            assert (wm.alpha, wm.beta, wm.gamma, wm.delta) == (11, 22, 33, 44)
        ok += want
        bad += 1 - want
    assert ok >= 100 and bad >= 40, (ok, bad)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_restoration_filters(oracle, bd):
    """av1_selfguided_restoration_c, av1_apply_selfguided_restoration_c and av1_[highbd_]wiener_convolve_add_src_c on units of width 1, 31,
    33 and 72 (one pixel, either side of the 32-pixel processing unit, wider than 64), all 16 self-guided parameter sets, random, flat and
    0 / max checkerboard content."""
    refc.lib()
    rng = np.random.default_rng(900 + bd)
    hb = bd > 8
    dt, mx = (np.uint16, (1 << bd) - 1) if hb else (np.uint8, 255)
    sgr, app, wie = o(oracle, "orc_selfguided_restoration"), o(oracle, "orc_apply_selfguided_restoration"), o(oracle, "orc_wiener_convolve_add_src")
    tmp = np.zeros(1 << 21, np.int32)
    raw = np.zeros(512 + 128, np.int16)
    base = (-raw.ctypes.data % 256) // 2      # the Wiener function masks the kernel's address to find its table (get_filter_base)
    grow = 2 if bd == 12 else 0               # get_conv_params_wiener
    cp = ConvolveParams(0, None, 0, 3 + grow, 11 - grow, 0, 0, 0, 0, 0)
    n = 0
    for w in (1, 31, 33, 72):
        for h in (1, 8, 33):
            for kind in ("random", "flat", "checker"):
                S = w + 8 + 3
                img = rng.integers(0, mx + 1, (h + 8, S)).astype(dt)
                if kind == "flat":
                    img[:] = int(rng.integers(0, mx + 1))
                if kind == "checker":
                    yy, xx = np.mgrid[0:h + 8, 0:S]; img = (((yy + xx) & 1) * mx).astype(dt)
                at = 4 * S + 4
                for idx in ((n % 16), (n * 7 + 10) % 16, 15 - n % 6):
                    g0, g1, w0, w1 = (np.full((h, w + 2), -7, np.int32) for _ in range(4))
                    sgr(VP(img, at), int(hb), w, h, S, VP(g0), VP(g1), w + 2, idx, bd)
                    rc = call(fn("av1_selfguided_restoration_c", C.c_int), Ptr(img, at, hb), w, h, S, w0, w1, w + 2, idx, bd, int(hb))
                    assert rc == 0 and np.array_equal(g0, w0) and np.array_equal(g1, w1), ("sgr", w, h, kind, idx)
                    xqd = np.asarray([int(rng.integers(-96, 32)), int(rng.integers(-32, 96))], np.int32)
                    got, want = np.full((h, w + 3), 5, dt), np.full((h, w + 3), 5, dt)
                    app(VP(img, at), int(hb), w, h, S, idx, VP(xqd), VP(got), w + 3, bd)
                    call(fn("av1_apply_selfguided_restoration_c", C.c_int), Ptr(img, at, hb), w, h, S, idx, xqd, Ptr(want, 0, hb), w + 3, tmp, bd, int(hb))
                    assert np.array_equal(got, want), ("apply", w, h, kind, idx)
                    n += 1
                # Wiener: symmetric 7-tap kernels in the coefficient ranges of av1/common/restoration.h (WIENER_FILT_TAP{0,1,2}_{MINV,MAXV})
                for trial in range(2):
                    ks = []
                    for _ in range(2):
                        t0, t1, t2 = int(rng.integers(-5, 11)), int(rng.integers(-23, 9)), int(rng.integers(-17, 47))
                        if trial:
                            t0, t1, t2 = (10, -23, 46) if _ == 0 else (-5, 8, -17)
                        ks.append([t0, t1, t2, -2 * (t0 + t1 + t2), t2, t1, t0, 0])
                    raw[base:base + 8] = ks[0]; raw[base + 8:base + 16] = ks[1]
                    fx, fy = np.asarray(ks[0], np.int16), np.asarray(ks[1], np.int16)
                    got, want = np.full((h, w + 3), 5, dt), np.full((h, w + 3), 5, dt)
                    wie(VP(img, at), int(hb), S, VP(got), w + 3, VP(fx), VP(fy), w, h, bd)
                    tail = [Ptr(raw, base), 16, Ptr(raw, base + 8), 16, w, h, cp]
                    if hb:
                        call(fn("av1_highbd_wiener_convolve_add_src_c"), Ptr(img, at, True), SSZ(S), Ptr(want, 0, True), SSZ(w + 3), *tail, bd)
                    else:
                        call(fn("av1_wiener_convolve_add_src_c"), Ptr(img, at), SSZ(S), want, SSZ(w + 3), *tail)
                    assert np.array_equal(got, want), ("wiener", w, h, kind, trial)
    assert n == 4 * 3 * 3 * 3


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_projection_statistics_and_errors(oracle, bd):
    """av1_calc_proj_params[_high_bd]_c and av1_{lowbd,highbd}_pixel_proj_error_c: the three radius combinations, odd sizes, saturated planes"""
    refc.lib()
    rng = np.random.default_rng(1000 + bd)
    hb = bd > 8
    dt, mx = (np.uint16, (1 << bd) - 1) if hb else (np.uint8, 255)
    calc, err = o(oracle, "orc_calc_proj_params"), o(oracle, "orc_pixel_proj_error", C.c_int64)
    n = 0
    for (w, h) in ((1, 1), (7, 5), (31, 9), (33, 16), (72, 33), (64, 64)):
        for r in ((2, 1), (2, 0), (0, 1)):
            for kind in ("random", "saturated"):
                S, FS = w + 5, w + 3
                src, dat = rng.integers(0, mx + 1, (h, S)).astype(dt), rng.integers(0, mx + 1, (h, S)).astype(dt)
                f0 = rng.integers(0, (mx + 1) << 4, (h, FS)).astype(np.int32); f1 = rng.integers(0, (mx + 1) << 4, (h, FS)).astype(np.int32)
                if kind == "saturated":
                    src[:] = mx; dat[:] = 0; f0[:] = mx << 4; f1[:] = 0
                prm = SgrParams((C.c_int * 2)(*r), (C.c_int * 2)(0, 0))
                H, Cc, gH, gC = np.zeros(4, np.int64), np.zeros(2, np.int64), np.zeros(4, np.int64), np.zeros(2, np.int64)
                call(fn("av1_calc_proj_params_high_bd_c" if hb else "av1_calc_proj_params_c"), Ptr(src, 0, hb), w, h, S, Ptr(dat, 0, hb), S, f0, FS, f1, FS, H, Cc, prm)
                calc(VP(src), w, h, S, VP(dat), S, VP(f0), FS, VP(f1), FS, int(hb), r[0], r[1], VP(gH), VP(gC))
                assert np.array_equal(gH, H) and np.array_equal(gC, Cc), (w, h, r, kind)
                for xq in ((0, 0), (int(rng.integers(-96, 32)), int(rng.integers(-32, 96))), (-96, 95)):
                    want = call(fn("av1_highbd_pixel_proj_error_c" if hb else "av1_lowbd_pixel_proj_error_c", C.c_int64), Ptr(src, 0, hb), w, h, S,
                                Ptr(dat, 0, hb), S, f0, FS, f1, FS, np.asarray(xq, np.int32), prm)
                    assert err(VP(src), w, h, S, VP(dat), S, VP(f0), FS, VP(f1), FS, int(hb), r[0], r[1], xq[0], xq[1]) == want, (w, h, r, kind, xq)
                    n += 1
    assert n == 6 * 3 * 2 * 3


# ---------------------------------------------------------------- TxfmParam dispatchers

def test_txfm_param_dispatchers(oracle):
    """av1_lowbd_fwd_txfm_c, av1_inv_txfm_add_c and av1_highbd_inv_txfm_add_c (with the lossless branch and its eob rule) against the oracle's
    transforms, every size x valid type.  (av1_round_shift_array has no twin in the oracle: the kernel meets the compiled function
    directly in tests/test_gpu_refc_rtcd.py.)"""
    refc.lib()
    rng = np.random.default_rng(1100)
    iw, fw = o(oracle, "orc_iwht4x4_add"), o(oracle, "orc_fwht4x4")
    n = 0
    for tx_size, (w, h) in enumerate(TX):
        nc = NC[tx_size]
        for tx_type in range(16):
            if not oracle.av1_tx_valid(tx_size, tx_type):
                continue
            for bd in (8, 10, 12):
                kind, res = residual_classes(rng, w, h, w, bd)[(tx_type + bd) % 5 if tx_type in (0, 9) else 0]
                out = np.zeros(w * h, np.int32)
                call(fn("av1_lowbd_fwd_txfm_c"), res, out, w, param(tx_size, tx_type, bd))
                assert np.array_equal(oracle.fwd_txfm2d(res, tx_size, tx_type, bd)[:nc], out[:nc]), ("fwd", w, h, tx_type, bd, kind)
                ckind = ("random", "extreme", "dc")[(tx_type + bd // 2) % 3]
                co = coeffs_for_inverse(rng, tx_size, bd, ckind)
                dst = pixels(rng, h, w, bd, ckind, np.uint16)
                want16 = oracle.inv_txfm2d_add(co[:nc], dst, tx_size, tx_type, bd)
                got = dst.copy()
                call(fn("av1_highbd_inv_txfm_add_c"), co, byteptr(got), w, param(tx_size, tx_type, bd))
                assert np.array_equal(got, want16), ("highbd inv", w, h, tx_type, bd, ckind)
                if bd == 8:
                    got8 = dst.astype(np.uint8)
                    call(fn("av1_inv_txfm_add_c"), co, got8, w, param(tx_size, tx_type, bd))
                    assert np.array_equal(got8, want16.astype(np.uint8)), ("inv", w, h, tx_type, ckind)
                n += 1
    assert n == 159 * 3
    for bd in (8, 10, 12):
        for eob in (0, 1, 2, 16):
            for trial in range(6):
                co = rng.integers(-(1 << (bd + 2)), 1 << (bd + 2), 16).astype(np.int32)
                dst = pixels(rng, 4, 4, bd, "random", np.uint16)
                want = dst.copy()
                iw(VP(co), VP(want), 4, eob, bd)
                got = dst.copy()
                call(fn("av1_highbd_inv_txfm_add_c"), co, byteptr(got), 4, param(0, 0, bd, lossless=1, eob=eob))
                assert np.array_equal(got, want), ("lossless", bd, eob)
                if bd == 8:
                    got8 = dst.astype(np.uint8)
                    call(fn("av1_inv_txfm_add_c"), co, got8, 4, param(0, 0, bd, lossless=1, eob=eob))
                    assert np.array_equal(got8, want.astype(np.uint8)), ("lossless 8", eob)
                res = rng.integers(-255, 256, (4, 4)).astype(np.int16)
                a, b = np.zeros(16, np.int32), np.zeros(16, np.int32)
                fw(VP(res), VP(a), 4)
                call(fn("av1_lowbd_fwd_txfm_c"), res, b, 4, param(0, 0, bd, lossless=1))
                assert np.array_equal(a, b)


# ---------------------------------------------------------------- prediction

def _interp(fx, fy, w, h):
    f = fn("refshim_interp_filter_params", C.c_void_p, refc.shim())
    return (C.c_void_p * 2)(call(f, fx, w), call(f, fy, h))


def _conv_params(cmp_index, buf, stride, is_compound, bd, weights=None):
    cp = ConvolveParams()
    call(fn("refshim_conv_params", None, refc.shim()), cp, cmp_index, 0, buf, stride, is_compound, bd)
    if weights:
        cp.use_dist_wtd_comp_avg, cp.fwd_offset, cp.bck_offset = 1, weights[0], weights[1]
    return cp


def _facade(src, S, dst, w, h, filt, sx, sy, cp, bd):
    hb = bd > 8
    call(fn("av1_highbd_convolve_2d_facade" if hb else "av1_convolve_2d_facade"), src, S, Ptr(dst, 0, hb), w, w, h, filt, sx, 16, sy, 16, 0, cp,
         *([bd] if hb else []))


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_convolve_predictors(oracle, bd):
    """av1_[highbd_]convolve_2d_facade -> av1_[highbd_]convolve_{x,y,2d}_sr_c / aom_[highbd_]convolve_copy_c, and the compound path ->
    av1_[highbd_]dist_wtd_convolve_{2d_copy,x,y,2d}_c (plain and distance-weighted): every block size up to 128 x 128, the four filters,
    all four (x, y) phase kinds, random content with a band of 0 / max pixels"""
    refc.lib()
    rng = np.random.default_rng(1200 + bd)
    hb = bd > 8
    dt, mx = (np.uint16, (1 << bd) - 1) if hb else (np.uint8, 255)
    sr, cmpd = o(oracle, "orc_convolve_sr"), o(oracle, "orc_convolve_compound")
    S, ROWS = 160, 150
    planes = [rng.integers(0, mx + 1, (ROWS, S)).astype(dt) for _ in range(2)]
    for pl in planes:
        pl[:20] = np.where(rng.integers(0, 2, (20, S)) > 0, mx, 0)
    n = 0
    for (w, h) in BLOCK_SIZES:
        for trial in range(4):
            fx, fy = [(0, 0), (1, 2), (2, 1), (3, 3)][trial]
            filt = _interp(fx, fy, w, h)
            pos = [(int(rng.integers(4, S - w - 5)), int(rng.integers(4 if trial else 2, (ROWS - h - 5) if trial else 12))) for _ in range(2)]
            subs = [[(int(rng.integers(1, 16)), 0), (0, int(rng.integers(1, 16))), (int(rng.integers(1, 16)), int(rng.integers(1, 16))), (0, 0)][(trial + r) % 4]
                    for r in range(2)]
            at = [pos[r][1] * S + pos[r][0] for r in range(2)]
            want, got = np.zeros((h, w), dt), np.zeros((h, w), dt)
            _facade(Ptr(planes[0], at[0], hb), S, want, w, h, filt, subs[0][0], subs[0][1], _conv_params(0, None, 0, 0, bd), bd)
            sr(VP(planes[0], at[0]), S, VP(got), w, w, h, fx, fy, subs[0][0], subs[0][1], int(hb), bd)
            assert np.array_equal(got, want), ("sr", w, h, fx, fy, subs[0])
            wts = (None, (9, 7), (4, 12), (13, 3))[trial]
            buf16, want, got = np.zeros(w * h, np.uint16), np.zeros((h, w), dt), np.zeros((h, w), dt)
            for r in range(2):
                _facade(Ptr(planes[r], at[r], hb), S, want, w, h, filt, subs[r][0], subs[r][1], _conv_params(r, buf16, w, 1, bd, wts), bd)
            cmpd(VP(planes[0], at[0]), S, subs[0][0], subs[0][1], VP(planes[1], at[1]), S, subs[1][0], subs[1][1], VP(got), w, w, h, fx, fy,
                 wts[0] if wts else 0, wts[1] if wts else 0, int(hb), bd)
            assert np.array_equal(got, want), ("compound", w, h, fx, fy, subs, wts)
            n += 1
    assert n == 88


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_warp_affine(oracle, bd):
    """av1_[highbd_]warp_affine_c on models whose shear parameters the reference itself derives (av1_get_shear_params): identity, small
    and large affine terms, translations that push the footprint out of the frame, luma and 4:2:0 geometry"""
    refc.lib()
    rng = np.random.default_rng(1300 + bd)
    hb = bd > 8
    dt, mx = (np.uint16, (1 << bd) - 1) if hb else (np.uint8, 255)
    f = o(oracle, "orc_warp_affine")
    W, H = 96, 80
    ref = rng.integers(0, mx + 1, (H, W)).astype(dt)
    ref[:10] = np.where(rng.integers(0, 2, (10, W)) > 0, mx, 0)
    n = 0
    trial = 0
    while n < 60:
        trial += 1
        span = (1 << 10, 1 << 13)[trial % 2]
        m = [int(rng.integers(-(1 << 19), 1 << 19)), int(rng.integers(-(1 << 19), 1 << 19)), (1 << 16) + int(rng.integers(-span, span)),
             int(rng.integers(-span, span)), int(rng.integers(-span, span)), (1 << 16) + int(rng.integers(-span, span))]
        if trial % 7 == 0:
            m = [0, 0, 1 << 16, 0, 0, 1 << 16]
        if trial % 5 == 0:
            m[0], m[1] = int(rng.choice([-1, 1])) * (60 << 16), int(rng.choice([-1, 1])) * (70 << 16)      # footprint outside the frame
        wm = WarpedMotionParams((C.c_int32 * 6)(*m), 0, 0, 0, 0, 3, 0)
        if not call(fn("av1_get_shear_params", C.c_int), wm):
            continue
        ss = trial % 2
        pw, ph = [(8, 8), (16, 8), (32, 32), (8, 32), (64, 16)][trial % 5]
        p_col, p_row = int(rng.integers(0, (W >> 0) - pw) // 8 * 8), int(rng.integers(0, H - ph) // 8 * 8)
        r0 = 3 + (2 if bd == 12 else 0)
        cp = ConvolveParams(0, None, 0, r0, 14 - r0, 0, 0, 0, 0, 0)
        mat = np.asarray(m, np.int32)
        sh = [C.c_int16(v) for v in (wm.alpha, wm.beta, wm.gamma, wm.delta)]
        want, got = np.zeros((ph, pw), dt), np.zeros((ph, pw), dt)
        head = [mat, ref, W, H, W, want, p_col, p_row, pw, ph, pw, ss, ss]
        if hb:
            call(fn("av1_highbd_warp_affine_c"), *head, bd, cp, *sh)
        else:
            call(fn("av1_warp_affine_c"), *head, cp, *sh)
        f(VP(mat), VP(ref), int(hb), W, H, W, VP(got), p_col, p_row, pw, ph, pw, ss, ss, bd, r0, wm.alpha, wm.beta, wm.gamma, wm.delta)
        assert np.array_equal(got, want), (m, ss, pw, ph, p_col, p_row)
        n += 1


def test_find_projection(oracle):
    """av1_find_projection: 1 .. 8 samples, clustered (near-singular) and spread, small and large motion vectors, four block sizes"""
    refc.lib()
    rng = np.random.default_rng(1400)
    ok = bad = 0
    for trial in range(400):
        bsize, (bw, bh) = [(3, (8, 8)), (6, (16, 16)), (9, (32, 32)), (5, (16, 8))][trial % 4]
        npts = int(rng.integers(1, 9))
        mi_row, mi_col = int(rng.integers(0, 60)) * 2, int(rng.integers(0, 60)) * 2
        mv = [int(rng.integers(-200, 201)), int(rng.integers(-200, 201))]
        cx, cy = (mi_col * 4 + bw // 2 - 1) * 8, (mi_row * 4 + bh // 2 - 1) * 8
        spread = (4, 40, 400)[trial % 3]
        pts = np.zeros(16, np.int32); pin = np.zeros(16, np.int32)
        for i in range(npts):
            dx, dy = int(rng.integers(-spread, spread + 1)), int(rng.integers(-spread, spread + 1))
            pts[2 * i], pts[2 * i + 1] = cx + dx, cy + dy
            pin[2 * i] = pts[2 * i] + mv[1] + int(rng.integers(-12, 13))
            pin[2 * i + 1] = pts[2 * i + 1] + mv[0] + int(rng.integers(-12, 13))
        if trial % 25 == 0:
            pts[2:2 * npts] = np.tile(pts[:2], npts - 1); pin[2:2 * npts] = np.tile(pin[:2], npts - 1)     # all samples the same: singular
        wm = WarpedMotionParams((C.c_int32 * 6)(0, 0, 1 << 16, 0, 0, 1 << 16), 0, 0, 0, 0, 3, 0)
        want = call(fn("av1_find_projection", C.c_int), npts, pts.copy(), pin.copy(), bsize, mv[0], mv[1], wm, mi_row, mi_col)
        good, mat, sh = oracle.find_projection(npts, pts, pin, bw, bh, mv, mi_row, mi_col)
        assert int(not good) == want, (trial, want)
        assert mat.tolist() == list(wm.wmmat), (trial, mat.tolist(), list(wm.wmmat))
        if not want:
            assert sh.tolist() == [wm.alpha, wm.beta, wm.gamma, wm.delta], trial
        ok += 1 - want
        bad += want
    assert ok >= 100 and bad >= 10, (ok, bad)


# ---------------------------------------------------------------- projections, averages, min / max

@pytest.mark.parametrize("bd", [8, 10])
def test_int_pro_and_vbp_leaves(oracle, bd):
    """aom_int_pro_row / aom_int_pro_col / aom_vector_var under av1_int_pro_motion_estimation, and aom_[highbd_]avg_8x8 / aom_avg_8x8_quad /
    aom_avg_4x4 / aom_[highbd_]minmax_8x8 under the leaf statistics of variance-based partitioning: the oracle holds these as parts of its
    restatements of the two callers, so the comparison is made at the callers, the reference's through oracle/refshim/."""
    sh = refc.shim()
    rng = np.random.default_rng(1500 + bd)
    hb = bd > 8
    dt, mx = (np.uint16, (1 << bd) - 1) if hb else (np.uint8, 255)
    W = H = 128
    border = 64
    S = W + 2 * border
    src, ref = rng.integers(0, mx + 1, (H + 2 * border, S)).astype(dt), rng.integers(0, mx + 1, (H + 2 * border, S)).astype(dt)
    ref[border:border + H, border:border + W] = np.roll(src[border:border + H, border:border + W], (3, -5), (0, 1))     # a real displacement to find
    ref[border + 64:, :] = np.where(rng.integers(0, 2, (H + border - 64, S)) > 0, mx, 0)
    ipm = o(oracle, "orc_int_pro_motion_estimation", U)
    f = fn("refshim_int_pro_motion_estimation", U, sh)
    n = 0
    for (w, h) in ((8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (16, 8), (8, 16), (32, 16), (64, 32), (128, 64)):
        for trial in range(4):
            bx, by = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
            lim = [-2, 3, -1, 2] if trial == 2 else [-(by + 30), H - by - h + 30, -(bx + 30), W - bx - w + 30]
            rmv = rng.integers(-64, 65, 2).tolist() if trial != 3 else [-(1023 * 8 + 40), 1023 * 8 + 24]
            at = (border + by) * S + border + bx
            mv = np.zeros(2, np.int16)
            want = call(f, Ptr(src, at, hb), Ptr(ref, at, hb), S, W, H, w, h, bd, np.asarray(lim, np.int32), np.asarray(rmv, np.int16), by // 4, bx // 4, mv)
            olim = np.asarray([lim[2], lim[3], lim[0], lim[1]], np.int32)
            out = np.zeros(2, np.int16)
            got = ipm(VP(src, at), S, VP(ref, at), S, w, h, bd, VP(olim), VP(np.asarray(rmv, np.int16)), VP(out))
            assert (got, out.tolist()) == (want, mv.tolist()), (w, h, trial, lim, rmv)
            n += 1
    assert n == 40
    a = rng.integers(0, mx + 1, (64, 72)).astype(dt)
    b = np.clip(a.astype(np.int64) + rng.integers(-(mx >> 3), (mx >> 3) + 1, a.shape), 0, mx).astype(dt)
    b[:16, :16] = mx - a[:16, :16]
    a[16:24, 16:24] = b[16:24, 16:24]
    a[32:48, 32:48] = mx; b[32:48, 32:48] = 0
    flag = 8 if hb else 0
    o8, omm, o4 = o(oracle, "orc_vbp_fill_8x8avg"), o(oracle, "orc_vbp_minmax_8x8", C.c_int), o(oracle, "orc_vbp_fill_4x4avg")
    m = 0
    for (pw, ph) in ((64, 64), (40, 64), (64, 20), (24, 8)):
        for y16 in range(0, 64, 16):
            for x16 in range(0, 64, 16):
                ws, wq, gs, gq = np.zeros(4, np.int32), np.zeros(4, np.uint32), np.zeros(4, np.int32), np.zeros(4, np.uint32)
                call(fn("refshim_vbp_fill_8x8avg", None, sh), Ptr(a, 0, hb), 72, Ptr(b, 0, hb), 72, x16, y16, flag, pw, ph, ws, wq)
                o8(VP(a), 72, VP(b), 72, x16, y16, int(hb), pw, ph, VP(gs), VP(gq))
                assert gs.tolist() == ws.tolist() and gq.tolist() == wq.tolist(), ("8x8", pw, ph, x16, y16)
                want = call(fn("refshim_vbp_minmax_8x8", C.c_int, sh), Ptr(a, 0, hb), 72, Ptr(b, 0, hb), 72, x16, y16, flag, pw, ph)
                assert omm(VP(a), 72, VP(b), 72, x16, y16, int(hb), pw, ph) == want, ("minmax", pw, ph, x16, y16)
                for bo in (0, 4):
                    x8, y8 = x16 + 8 * ((x16 >> 4) & 1), y16 + 8 * ((y16 >> 5) & 1)
                    call(fn("refshim_vbp_fill_4x4avg", None, sh), Ptr(a, 0, hb), 72, x8, y8, flag, pw, ph, bo, ws, wq)
                    o4(VP(a), 72, x8, y8, int(hb), pw, ph, bo, VP(gs), VP(gq))
                    assert gs.tolist() == ws.tolist() and gq.tolist() == wq.tolist(), ("4x4", pw, ph, x8, y8, bo)
                m += 1
    assert m == 64


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_cdef_filter_fb(oracle, bd):
    """av1_cdef_filter_fb on whole 64 x 64 filter blocks against the oracle's plane drivers (direction search, strength adjustment by
    variance, skip list, CDEF_VERY_LARGE at frame edges): luma and 4:2:0 / 4:2:2 / 4:4:0 / 4:4:4 chroma, interior and corner blocks"""
    refc.lib()
    rng = np.random.default_rng(1600 + bd)
    mx = (1 << bd) - 1
    P = 192
    changed = 0
    yy, xx = np.mgrid[0:P, 0:P]
    luma = np.clip(mx // 2 + (mx // 5) * np.sin(xx / 9.0 + yy / 17.0) + (mx // 7) * ((xx // 23 + yy // 29) % 2)
                   + rng.integers(-(6 << (bd - 8)), (6 << (bd - 8)) + 1, (P, P)), 0, mx).astype(np.int64)
    luma[64:80, 64:96] = np.where((yy[64:80, 64:96] + xx[64:80, 64:96]) & 1, mx, 0)      # a 0 / max checkerboard inside the filter block
    n = 0
    for (xdec, ydec, pli) in ((0, 0, 0), (1, 1, 1), (1, 0, 1), (0, 1, 1), (0, 0, 1)):
        for (level, sec, damping, at_edge) in ((4, 2, 6, 0), (9, 0, 5, 0), (0, 4, 3, 0), (15, 1, 4, 1), (1, 2, 6, 1), (63 >> 2, 3, 5, 0)):
            dt = np.uint8 if bd == 8 else np.uint16
            plane = np.ascontiguousarray((luma if not pli else luma[::(1 << ydec), ::(1 << xdec)]).astype(dt))
            pw, ph = 64 >> xdec, 64 >> ydec
            y0, x0 = (0, 0) if at_edge else (ph, pw)
            s8 = (rng.random((8, 8)) < 0.2).astype(np.uint8)
            ld = rng.integers(0, 8, (8, 8)).astype(np.uint8)
            want, wd, wv = cdef_fb_reference(plane.astype(np.int64), pli, xdec, ydec, y0, x0, pw, ph, s8, ld, level, sec, damping, bd)
            fby, fbx = (0, 0) if at_edge else (1, 1)
            skip = np.ones((24, 24), np.uint8)
            skip[fby * 8:fby * 8 + 8, fbx * 8:fbx * 8 + 8] = s8
            pri, secs = np.full((3, 3), level, np.uint8), np.full((3, 3), sec, np.uint8)
            if not pli:
                out, d, v = oracle.cdef_plane_luma(plane, pri, secs, skip, damping, bd)
                keep = s8 == 0
                assert np.array_equal(d[fby * 8:fby * 8 + 8, fbx * 8:fbx * 8 + 8][keep], wd[keep].astype(np.uint8)), (bd, level, sec, at_edge)
                assert np.array_equal(v[fby * 8:fby * 8 + 8, fbx * 8:fbx * 8 + 8][keep], wv[keep]), (bd, level, sec, at_edge)
            else:
                full = np.zeros((24, 24), np.uint8)
                full[fby * 8:fby * 8 + 8, fbx * 8:fbx * 8 + 8] = ld
                out = oracle.cdef_plane_chroma(plane, xdec, ydec, full, pri, secs, skip, damping, bd)
            assert np.array_equal(out[y0:y0 + ph, x0:x0 + pw], want), (bd, xdec, ydec, pli, level, sec, damping, at_edge)
            changed += int(not np.array_equal(want, plane[y0:y0 + ph, x0:x0 + pw]))
            n += 1
    assert n == 30 and changed == 30      # every case does filter
