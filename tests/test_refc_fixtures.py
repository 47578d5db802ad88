"""The committed fixtures tests/golden/ref_eval_*.npz, which the fixture interpreter (tests/golden/ref_c_eval.py) recorded, replayed through
the reference compiled as C (oracle/_ref/libaomref_c.so, tests/refc.py): every recorded output must come out of the compiled *_c function
bit for bit.  A difference would mean that the interpreter, one of its struct views or one of its text patches misread the reference --
and with it every oracle and kernel test that rests on that fixture.  No oracle code runs here (scan orders come from the compiled
reference's own av1_scan_orders).  Every case of a replayed file is replayed; each test asserts the count it saw.

REPLAYED names the fixtures replayed here: every fixture that records plain-argument functions.  Three go through oracle/refshim/ because
what they record is `static` in the reference (qm_fp, vbp) or takes encoder structs (intpro).  DESIGN.md section 2 lists the fixtures whose
functions take encoder structs and stay pinned by the interpreter only."""
import ctypes as C
import json
import os

import numpy as np

import refc
from refc import Ptr, byteptr, call, fn
from refc_inputs import ConvolveParams, SgrParams, WarpedMotionParams, cdef_fb_reference

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SSZ = C.c_ssize_t
N_LOW_BLOCK_ERROR, N_LP_BLOCK_ERROR = 73, 58     # rows of the fixtures whose `int` products stay within 31 bits
REPLAYED = ["quant", "quant_lp", "qm", "qm_adaptive", "lpf", "cdef", "sadvar", "txfm2d", "txfm1d_live", "compound", "rdhelp", "lrstats", "sumsq", "wedge", "sgr", "proj", "obmc_blend", "warp", "lr_apply",
            "convolve", "convolve_compound", "convolve_masked", "qm_fp", "warp_error", "vbp", "intpro", "lpf_flat", "cdef_fb"]


def load(name):
    z = np.load(os.path.join(GOLD, name))
    return z, json.loads(bytes(z["cases"]).decode())


def test_every_replayed_fixture_has_a_test():
    for name in REPLAYED:
        assert os.path.exists(os.path.join(GOLD, "ref_eval_%s.npz" % name)), name
        assert "test_%s" % name in globals(), name


class ScanOrder(C.Structure):
    _fields_ = [("scan", C.POINTER(C.c_int16)), ("iscan", C.POINTER(C.c_int16))]


def ref_scan(tx_size, tx_type, n):
    """av1_scan_orders[TX_SIZES_ALL][TX_TYPES] (av1/common/scan.c) of the compiled reference"""
    tab = (ScanOrder * 16 * 19).in_dll(refc.lib(), "av1_scan_orders")
    so = tab[tx_size][tx_type]
    return (np.ctypeslib.as_array(so.scan, (n,)).copy(), np.ctypeslib.as_array(so.iscan, (n,)).copy())


def rows8(tables):
    """a quantiser row as the encoder stores it: DC, then the AC entry seven times"""
    return {k: np.asarray([v[0]] + [v[1]] * 7, np.int16) for k, v in tables.items()}


def test_quant():
    z, cases = load("ref_eval_quant.npz")
    lib = refc.lib()
    assert len(cases) == 688
    for k, c in enumerate(cases):
        n = c["n"]
        t = rows8(c["tables"])
        sc, isc = ref_scan(c["tx_size"], c["tx_type"], n)
        co = np.ascontiguousarray(z["c%d" % k], np.int32)
        qc, dq, eob = np.full(n, 77, np.int32), np.full(n, 77, np.int32), np.full(1, 9, np.uint16)
        call(fn(c["fn"]), co, SSZ(n), t["zbin"], t["round"], t["quant"], t["quant_shift"], qc, dq, t["dequant"], eob, sc, isc)
        assert eob[0] == c["eob"] and np.array_equal(qc, z["q%d" % k]) and np.array_equal(dq, z["d%d" % k]), (k, c["fn"], c["kind"])
    rows = z["quantize_fp"].tolist()
    assert len(rows) >= 130
    for kk, want_eob, r0, r1, q0, q1 in rows:
        c = cases[kk]
        n = c["n"]
        t = rows8(dict(c["tables"], round=[r0, r1], quant=[q0, q1]))
        sc, isc = ref_scan(c["tx_size"], c["tx_type"], n)
        co = np.ascontiguousarray(z["c%d" % kk], np.int32)
        qc, dq, eob = np.full(n, 77, np.int32), np.full(n, 77, np.int32), np.full(1, 9, np.uint16)
        args = [co, SSZ(n), t["zbin"], t["round"], t["quant"], t["quant_shift"], qc, dq, t["dequant"], eob, sc, isc]
        if c["hbd"]:
            call(fn("av1_highbd_quantize_fp_c"), *args, c["log_scale"])
        else:
            call(fn("av1_quantize_fp" + ("", "_32x32", "_64x64")[c["log_scale"]] + "_c"), *args)
        assert eob[0] == want_eob and np.array_equal(qc, z["fq%d" % kk]) and np.array_equal(dq, z["fd%d" % kk]), (kk, c["fn"])
    rows = z["block_error"]
    assert len(rows) >= 90
    n_low = 0
    for row in rows:
        kk = int(row[0])
        co, dq = np.ascontiguousarray(z["c%d" % kk], np.int32), np.ascontiguousarray(z["d%d" % kk], np.int32)
        for j, bd in enumerate((0, 8, 10, 12)):
            ssz = np.zeros(1, np.int64)
            if bd == 0:
                # the interpreter wraps av1_block_error_c's `int` products; compiled code need not (signed overflow is undefined),
                # so the low-bit-depth form is replayed only where no product leaves 31 bits
                if max(np.abs(co.astype(np.int64)).max(), np.abs(co.astype(np.int64) - dq).max()) >= 46340:
                    continue
                e = call(fn("av1_block_error_c", C.c_int64), co, dq, SSZ(co.size), ssz)
                n_low += 1
            else:
                e = call(fn("av1_highbd_block_error_c", C.c_int64), co, dq, SSZ(co.size), ssz, bd)
            assert (e, int(ssz[0])) == (int(row[1 + 2 * j]), int(row[2 + 2 * j])), (kk, bd)
    assert n_low == N_LOW_BLOCK_ERROR, (n_low, len(rows))     # the rows inside the low-bit-depth form's defined range: not "none"


def test_quant_lp():
    z, cases = load("ref_eval_quant_lp.npz")
    assert len(cases) == 65
    n_err = 0
    for c in cases:
        k, n = c["k"], c["n"]
        t = rows8(c["tables"])
        sc, isc = ref_scan(c["tx_size"], c["tx_type"], n)
        co = np.ascontiguousarray(z["c%d" % k], np.int16)
        qc, dq, eob = np.full(n, 0x55, np.int16), np.full(n, 0x55, np.int16), np.full(1, 77, np.uint16)
        call(fn("av1_quantize_lp_c"), co, SSZ(n), t["round"], t["quant"], qc, dq, t["dequant"], eob, sc, isc)
        assert eob[0] == c["eob"] and np.array_equal(qc, z["q%d" % k]) and np.array_equal(dq, z["d%d" % k]), c
        if np.abs(co.astype(np.int64) - dq).max() < 46340:     # see test_quant: `int` products
            assert call(fn("av1_block_error_lp_c", C.c_int64), co, dq, SSZ(n)) == c["block_error"], c
            n_err += 1
    assert n_err == N_LP_BLOCK_ERROR, n_err


def _qm_replay(fixture, expect):
    z, cases = load(fixture)
    assert len(cases) == expect
    for k, c in enumerate(cases):
        k = c.get("k", k)
        n = c["n"]
        t = rows8(c["tables"])
        sc, isc = ref_scan(c["tx_size"], 0, n)
        co = np.ascontiguousarray(z["c%d" % k], np.int32)
        qm, iqm = np.ascontiguousarray(z["qm_" + c["matrix"]], np.uint8), np.ascontiguousarray(z["iqm_" + c["matrix"]], np.uint8)
        qc, dq, eob = np.full(n, 77, np.int32), np.full(n, 77, np.int32), np.full(1, 9, np.uint16)
        call(fn(c["fn"]), co, SSZ(n), t["zbin"], t["round"], t["quant"], t["quant_shift"], qc, dq, t["dequant"], eob, sc, isc, qm, iqm, c["log_scale"])
        assert eob[0] == c["eob"] and np.array_equal(qc, z["q%d" % k]) and np.array_equal(dq, z["d%d" % k]), (k, c["fn"], c["kind"])


def test_qm():
    _qm_replay("ref_eval_qm.npz", 240)


def test_qm_adaptive():
    _qm_replay("ref_eval_qm_adaptive.npz", 180)


def test_lpf():
    z, cases = load("ref_eval_lpf.npz")
    assert len(cases) == 720
    for k, c in enumerate(cases):
        px = np.ascontiguousarray(z["i%d" % k].astype(np.uint8 if c["bd"] == 8 else np.uint16))
        thr = [np.full(16, c[m], np.uint8) for m in ("blimit", "limit", "thresh")]
        args = [Ptr(px, c["y"] * px.shape[1] + c["x"]), px.shape[1]] + thr + ([c["bd"]] if c["bd"] > 8 else [])
        call(fn(c["fn"]), *args)
        assert np.array_equal(px.astype(np.uint16), z["o%d" % k]), (k, c)


def test_cdef():
    z, cases = load("ref_eval_cdef.npz")
    assert len(cases) == 120 and len(z["find_dir_in"]) == 36
    for img, (bd, d, var) in zip(z["find_dir_in"], z["find_dir_out"]):
        img = np.ascontiguousarray(img, np.uint16)
        v = np.zeros(1, np.int32)
        assert (call(fn("cdef_find_dir_c", C.c_int), img, 8, v, int(bd) - 8), int(v[0])) == (int(d), int(var))
    for k, c in enumerate(cases):
        tile = np.ascontiguousarray(z["t%d" % k], np.uint16)
        dst = np.zeros((c["bh"], c["bw"]), np.uint16 if "_16_" in c["fn"] else np.uint8)
        call(fn(c["fn"]), dst, c["bw"], Ptr(tile, 3 * 144 + 8), c["pri"], c["sec"], c["dir"], c["pri_damping"], c["sec_damping"], c["coeff_shift"],
             c["bw"], c["bh"])
        assert np.array_equal(dst.astype(np.uint16), z["f%d" % k]), (k, c)


def test_sadvar():
    z, rows = load("ref_eval_sadvar.npz")
    n_plain = n_extra = 0
    U = C.c_uint
    for r in rows:
        if r.get("extra"):
            a, b = np.ascontiguousarray(z["a8"].astype(np.uint8)), np.ascontiguousarray(z["b8"].astype(np.uint8))
            S, R = a.shape[1], b.shape[1]
            A, B = Ptr(a, r["oy"] * S + r["ox"]), Ptr(b, r["ry"] * R + r["rx"])
            for (w, h) in ((16, 16), (16, 8), (8, 16), (8, 8)):
                sse = np.zeros(1, np.uint32)
                got = call(fn("aom_mse%dx%d_c" % (w, h), U), A, S, B, R, sse)
                assert [got, int(sse[0])] == r["mse%dx%d" % (w, h)]
            for n in (8, 16):
                sse, sm = np.zeros(1, np.uint32), np.zeros(1, np.int32)
                call(fn("aom_get%dx%dvar_c" % (n, n)), A, S, B, R, sse, sm)
                assert [int(sse[0]), int(sm[0])] == r["get%dvar" % n]
            s8, m8, ts, tm, v8, ts0, tm0 = r["quad"]
            sse8, sum8, var8 = np.zeros(4, np.uint32), np.zeros(4, np.int32), np.zeros(4, np.uint32)
            tsse, tsum = np.asarray([ts0], np.uint32), np.asarray([tm0], np.int32)
            call(fn("aom_get_var_sse_sum_8x8_quad_c"), A, S, B, R, sse8, sum8, tsse, tsum, var8)
            assert (sse8.tolist(), sum8.tolist(), int(tsse[0]), int(tsum[0]), var8.tolist()) == (s8, m8, ts, tm, v8)
            s16, ts, tm, v16, ts0, tm0 = r["dual"]
            sse16, var16 = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
            tsse, tsum = np.asarray([ts0], np.uint32), np.asarray([tm0], np.int32)
            call(fn("aom_get_var_sse_sum_16x16_dual_c"), A, S, B, R, sse16, tsse, tsum, var16)
            assert (sse16.tolist(), int(tsse[0]), int(tsum[0]), var16.tolist()) == (s16, ts, tm, v16)
            n_extra += 1
            continue
        bd, w, h = r["bd"], r["w"], r["h"]
        hb = bd > 8
        dt = np.uint16 if hb else np.uint8
        a, b = np.ascontiguousarray(z["a%d" % bd].astype(dt)), np.ascontiguousarray(z["b%d" % bd].astype(dt))
        S, R = a.shape[1], b.shape[1]
        A, B = Ptr(a, r["oy"] * S + r["ox"], hb), Ptr(b, r["ry"] * R + r["rx"], hb)
        pre, vpre = ("aom_highbd_", "aom_highbd_%d_" % bd) if hb else ("aom_", "aom_")
        assert call(fn(pre + "sad%dx%d_c" % (w, h), U), A, S, B, R) == r["sad"], r
        assert call(fn(pre + "sad_skip_%dx%d_c" % (w, h), U), A, S, B, R) == r["sad_skip"], r
        if "x4d" in r:
            out = np.zeros(4, np.uint32)
            call(fn(pre + "sad%dx%dx4d_c" % (w, h)), A, S, refc.PtrList([Ptr(b, y * R + x, hb) for x, y in r["x4d_offs"]]), R, out)
            assert out.tolist() == r["x4d"], r
        sse = np.zeros(1, np.uint32)
        assert (call(fn(vpre + "variance%dx%d_c" % (w, h), U), A, S, B, R, sse), int(sse[0])) == (r["var"], r["sse"]), r
        for xo, yo, want_v, want_sse in r.get("subpel", []):
            got = call(fn(vpre + "sub_pixel_variance%dx%d_c" % (w, h), U), A, S, xo, yo, B, R, sse)
            assert (got, int(sse[0])) == (want_v, want_sse), (r, xo, yo)
        if "subtract_sum" in r:
            diff = np.zeros((h, w), np.int16)
            call(fn(pre + "subtract_block_c"), h, w, diff, SSZ(w), A, SSZ(S), B, SSZ(R))
            assert int(np.sum(diff.astype(np.int64).ravel() * (np.arange(w * h) % 251 + 1))) == r["subtract_sum"]
            sp = np.random.default_rng(r["second_pred_seed"]).integers(0, (1 << bd), w * h).astype(dt)
            assert call(fn(pre + "sad%dx%d_avg_c" % (w, h), U), A, S, B, R, Ptr(sp, 0, hb)) == r["sad_avg"], r
        n_plain += 1
    assert (n_plain, n_extra) == (63, 6)


def test_txfm2d():
    z, cases = load("ref_eval_txfm2d.npz")
    n_fwd = n_inv = n_wht = 0
    for k, c in enumerate(cases):
        w, h = c["w"], c["h"]
        x = np.ascontiguousarray(z["x%d" % k].reshape(h, w).astype(np.int16))
        out = np.zeros(w * h, np.int32)
        if c.get("wht"):
            call(fn("av1_fwht4x4_c"), x, out, 4)
            assert np.array_equal(out, z["c%d" % k]), c
            dst = np.ascontiguousarray(z["p%d" % k].reshape(4, 4).astype(np.uint16))
            dq = np.ascontiguousarray(z["dq%d" % k], np.int32)
            call(fn("av1_highbd_iwht4x4_add"), dq, byteptr(dst), 4, c["eob"], c["inv_bd"])
            assert np.array_equal(dst, z["r%d" % k]), c
            n_wht += 1
            continue
        call(fn("av1_fwd_txfm2d_%dx%d_c" % (w, h)), x, out, w, c["tx_type"], c["bd"])
        nn = min(w, 32) * min(h, 32)      # 64-point sizes: the re-packed 32 x 32 low frequencies are what the function returns
        assert np.array_equal(out[:nn], z["c%d" % k][:nn]), c
        n_fwd += 1
        if "inv_bd" in c:
            dq = np.zeros(w * h, np.int32); dq[:nn] = z["dq%d" % k][:nn]
            dst = np.ascontiguousarray(z["p%d" % k].reshape(h, w).astype(np.uint16))
            call(fn("av1_inv_txfm2d_add_%dx%d_c" % (w, h)), dq, dst, w, c["tx_type"], c["inv_bd"])
            assert np.array_equal(dst, z["r%d" % k]), c
            n_inv += 1
    assert (n_fwd, n_inv, n_wht) == (322, 287, 24), (n_fwd, n_inv, n_wht)


def test_txfm1d_live():
    g = np.load(os.path.join(GOLD, "ref_eval_txfm1d_live.npz"))
    names = sorted({k.split("/")[0] for k in g.files})
    assert len(names) == 14
    n = 0
    for name in names:
        x = np.ascontiguousarray(g[name + "/in"], np.int32)
        inv = name.startswith("av1_i")
        for key in [k for k in g.files if k.startswith(name + "/cb")]:
            cb, clamp = int(key.split("/")[1][2:]), int(key.split("/")[2][5:])
            stage_range = np.full(16, clamp if inv else 31, np.int8)
            for r in range(x.shape[0]):
                out = np.zeros(x.shape[1], np.int32)
                call(fn(name), np.ascontiguousarray(x[r]), out, C.c_int8(cb), stage_range)
                assert np.array_equal(out, g[key][r]), (name, cb, clamp, r)
                n += 1
    assert n == 20 * (7 * 2 + 7)


def test_compound():
    z, cases = load("ref_eval_compound.npz")
    U = C.c_uint
    checked = 0

    class Jcp(C.Structure):
        _fields_ = [("use_dist_wtd_comp_avg", C.c_int), ("fwd_offset", C.c_int), ("bck_offset", C.c_int)]
    for c in cases:
        bd, w, h, k = c["bd"], c["w"], c["h"], c["k"]
        hb = bool(bd > 8 or c.get("hbd8", 0))
        dt = np.uint16 if hb else np.uint8
        a, b = np.ascontiguousarray(z["a%d" % bd], dt), np.ascontiguousarray(z["b%d" % bd], dt)
        S = a.shape[1]
        A, B = Ptr(a, c["ay"] * S + c["ax"], hb), Ptr(b, c["by"] * S + c["bx"], hb)
        sp = Ptr(np.ascontiguousarray(z["sp%d" % k], dt), 0, hb)
        mask, ms = np.ascontiguousarray(z["mask%d" % k]), c["mask_stride"]
        ws, om = np.ascontiguousarray(z["ws%d" % k], np.int32), np.ascontiguousarray(z["om%d" % k], np.int32)
        vpre = "aom_highbd_%d_" % bd if hb else "aom_"
        spre = "aom_highbd_" if hb else "aom_"
        wh = "%dx%d_c" % (w, h)
        sse = np.zeros(1, np.uint32)
        for xo, yo, v, want in c.get("svaf", []):
            assert (call(fn(vpre + "sub_pixel_avg_variance" + wh, U), A, S, xo, yo, B, S, sse, sp), int(sse[0])) == (v, want), ("svaf", c)
            checked += 1
        for xo, yo, fwd, bck, v, want in c.get("jsvaf", []):
            got = call(fn(vpre + "dist_wtd_sub_pixel_avg_variance" + wh, U), A, S, xo, yo, B, S, sse, sp, Jcp(1, fwd, bck))
            assert (got, int(sse[0])) == (v, want), ("jsvaf", c)
            checked += 1
        for xo, yo, inv, v, want in c.get("msvf", []):
            got = call(fn(vpre + "masked_sub_pixel_variance" + wh, U), A, S, xo, yo, B, S, sp, mask, ms, inv, sse)
            assert (got, int(sse[0])) == (v, want), ("msvf", c)
            checked += 1
        for inv, v in c.get("msdf", []):
            assert call(fn(spre + "masked_sad" + wh, U), B, S, A, S, sp, mask, ms, inv) == v, ("msdf", c)
            checked += 1
        if "osdf" in c:
            assert call(fn(spre + "obmc_sad" + wh, U), A, S, ws, om) == c["osdf"], ("osdf", c)
            checked += 1
        # highbd content at 8 bits: the OBMC variances have no aom_highbd_8_ symbol, the undecorated aom_highbd_ one is the 8-bit form
        opre = vpre if refc.has(vpre + "obmc_variance" + wh) else spre
        assert [call(fn(opre + "obmc_variance" + wh, U), A, S, ws, om, sse), int(sse[0])] == c["ovf"], ("ovf", c)
        checked += 1
        for xo, yo, v, want in c["osvf"]:
            assert (call(fn(opre + "obmc_sub_pixel_variance" + wh, U), A, S, xo, yo, ws, om, sse), int(sse[0])) == (v, want), ("osvf", c)
            checked += 1
    assert len(cases) == 27 and checked >= 336, (len(cases), checked)


def test_rdhelp():
    z, cases = load("ref_eval_rdhelp.npz")
    seen = {}
    for c in cases:
        seen[c["kind"]] = seen.get(c["kind"], 0) + 1
        if c["kind"] == "sse":
            hb = c["bd"] > 8
            dt = np.uint16 if hb else np.uint8
            a, b = np.ascontiguousarray(z["sa%d" % c["bd"]], dt), np.ascontiguousarray(z["sb%d" % c["bd"]], dt)
            S = a.shape[1]
            got = call(fn("aom_highbd_sse_c" if hb else "aom_sse_c", C.c_int64), Ptr(a, c["oy"] * S + c["ox"], hb), S, Ptr(b, 3 * S + 2, hb), S,
                       c["w"], c["h"])
            assert got == c["value"], c
        elif c["kind"] == "hadamard":
            r = np.ascontiguousarray(z["r%d" % c["k"]], np.int16)
            n, fl = c["n"], c["flavour"]
            name = ("aom_hadamard_%dx%d_c", "aom_hadamard_lp_%dx%d_c", "aom_highbd_hadamard_%dx%d_c")[fl] % (n, n)
            out = np.zeros(n * n, np.int16 if fl == 1 else np.int32)
            call(fn(name), Ptr(r, c["y"] * r.shape[1] + c["x"]), SSZ(r.shape[1]), out)
            assert np.array_equal(out.astype(np.int32), z["c%d" % c["k"]]), c
            assert call(fn("aom_satd_lp_c" if fl == 1 else "aom_satd_c", C.c_int), out, n * n) == c["satd"], c
        else:
            coeff = np.ascontiguousarray(z["tc%d" % c["k"]], np.int32)
            want = z["tl%d" % c["k"]]
            lv = np.full(want.size, 0xAA, np.uint8)
            call(fn("av1_txb_init_levels_c"), coeff, c["w"], c["h"], lv)
            assert np.array_equal(lv, want), c
    assert seen == {"sse": 16, "hadamard": 27, "levels": 9}, seen


def test_lrstats():
    z, cases = load("ref_eval_lrstats.npz")
    assert len(cases) == 8
    for c in cases:
        bd, win = c["bd"], c["win"]
        hb = bd > 8
        dt = np.uint16 if hb else np.uint8
        dgd, src = np.ascontiguousarray(z["dgd%d" % bd], dt), np.ascontiguousarray(z["src%d" % bd], dt)
        hs, he, vs, ve = c["rect"]
        M, H = np.zeros(49, np.int64), np.zeros(49 * 49, np.int64)
        if hb:
            call(fn("av1_compute_stats_highbd_c"), win, byteptr(dgd), byteptr(src), hs, he, vs, ve, dgd.shape[1], src.shape[1], M, H, bd)
        else:
            call(fn("av1_compute_stats_c"), win, dgd, src, hs, he, vs, ve, dgd.shape[1], src.shape[1], M, H, c["downsample"])
        assert np.array_equal(M[:win * win], z["M%d" % c["k"]]) and np.array_equal(H[:win ** 4], z["H%d" % c["k"]]), c


def test_sumsq():
    z, cases = load("ref_eval_sumsq.npz")
    assert len(cases) == 54
    for c in cases:
        plane = np.ascontiguousarray(z[c["plane"]], np.int16)
        S = plane.shape[1]
        sm = np.asarray([c["sum_in"]], np.int32)
        ss = call(fn("aom_sum_sse_2d_i16_c", C.c_uint64), Ptr(plane, c["y"] * S + c["x"]), S, c["w"], c["h"], sm)
        assert (ss, int(sm[0])) == (int(c["ss"]), c["sum_out"]), c     # *sum is accumulated into: sum_in is not zero everywhere
        assert call(fn("aom_sum_squares_2d_i16_c", C.c_uint64), Ptr(plane, c["y"] * S + c["x"]), S, c["w"], c["h"]) == int(c["ss"]), c
    assert any(c["sum_in"] for c in cases)


def test_wedge():
    z, cases = load("ref_eval_wedge.npz")
    assert len(cases) == 30
    n = 0
    for c in cases:
        k, N = c["k"], c["N"]
        r1, d, m = (np.ascontiguousarray(z["%s_%d" % (x, k)]) for x in ("r1", "d", "m"))
        assert (r1.dtype, d.dtype, m.dtype) == (np.int16, np.int16, np.uint8)
        assert call(fn("av1_wedge_sse_from_residuals_c", C.c_uint64), r1, d, m, N) == c["sse"], c
        a, b = np.ascontiguousarray(z["a_%d" % k], np.int16), np.ascontiguousarray(z["b_%d" % k], np.int16)
        ds = np.zeros(N, np.int16)
        call(fn("av1_wedge_compute_delta_squares_c"), ds, a, b, N)
        assert np.array_equal(ds, z["ds_%d" % k]), c
        for limit, want in zip(c["limits"], c["signs"]):
            assert call(fn("av1_wedge_sign_from_residuals_c", C.c_int8), ds, m, N, C.c_int64(limit)) == want, (c, limit)
            n += 1
    assert n == 150


def test_sgr():
    z, cases = load("ref_eval_sgr.npz")
    assert len(cases) == 23
    for c in cases:
        k, bd, w, h = c["k"], c["bd"], c["w"], c["h"]
        hb = bd > 8
        img = np.ascontiguousarray(z["img%d" % k], np.uint16 if hb else np.uint8)
        f0, f1 = np.full((h, w), -7, np.int32), np.full((h, w), -7, np.int32)
        rc = call(fn("av1_selfguided_restoration_c", C.c_int), Ptr(img, 3 * img.shape[1] + 3, hb), w, h, img.shape[1], f0, f1, w, c["idx"], bd, int(hb))
        assert rc == 0 and np.array_equal(f0.ravel(), z["f0_%d" % k]) and np.array_equal(f1.ravel(), z["f1_%d" % k]), c


def test_proj():
    z, cases = load("ref_eval_proj.npz")
    assert len(cases) == 72
    n = 0
    for c in cases:
        k, hb = c["k"], c["bd"] > 8
        dt = np.uint16 if hb else np.uint8
        src, dat = np.ascontiguousarray(z["s%d" % k], dt), np.ascontiguousarray(z["d%d" % k], dt)
        f0, f1 = np.ascontiguousarray(z["f0_%d" % k], np.int32), np.ascontiguousarray(z["f1_%d" % k], np.int32)
        prm = SgrParams((C.c_int * 2)(*c["r"]), (C.c_int * 2)(0, 0))
        H, Cc = np.zeros(4, np.int64), np.zeros(2, np.int64)
        call(fn("av1_calc_proj_params_high_bd_c" if hb else "av1_calc_proj_params_c"), Ptr(src, 0, hb), c["w"], c["h"], c["S"], Ptr(dat, 0, hb), c["S"],
             f0, c["FS"], f1, c["FS"], H, Cc, prm)
        assert H.tolist() == c["H"] and Cc.tolist() == c["C"], c
        for xq, want in zip(c["xq"], c["err"]):
            got = call(fn("av1_highbd_pixel_proj_error_c" if hb else "av1_lowbd_pixel_proj_error_c", C.c_int64), Ptr(src, 0, hb), c["w"], c["h"], c["S"],
                       Ptr(dat, 0, hb), c["S"], f0, c["FS"], f1, c["FS"], np.asarray(xq, np.int32), prm)
            assert got == want, (k, xq)
            n += 1
    assert n >= 72


def test_obmc_blend():
    z, cases = load("ref_eval_obmc_blend.npz")
    assert len(cases) == 30
    for c in cases:
        bd, w, h = c["bd"], c["w"], c["h"]
        hb = bd > 8
        dt = np.uint16 if hb else np.uint8
        pred, adj = np.ascontiguousarray(z["pred%d" % bd], dt).copy(), np.ascontiguousarray(z["adj%d" % bd], dt)
        S = pred.shape[1]
        mask = np.ascontiguousarray(z["obmc_mask_%d" % (h if c["vertical"] else w)], np.uint8)
        at = c["y"] * S + c["x"]
        name = "aom_%sblend_a64_%smask_c" % ("highbd_" if hb else "", "v" if c["vertical"] else "h")
        P_, A_ = Ptr(pred, at, hb), Ptr(adj, at, hb)
        call(fn(name), P_, C.c_uint32(S), P_, C.c_uint32(S), A_, C.c_uint32(S), mask, w, h, *([bd] if hb else []))     # in place, as OBMC does
        assert np.array_equal(pred[c["y"]:c["y"] + h, c["x"]:c["x"] + w], z["o%d" % c["k"]]), c


def test_warp():
    z, cases = load("ref_eval_warp.npz")
    assert len(cases) == 42
    for c in cases:
        bd = c["bd"]
        hb = bd > 8
        ref = np.ascontiguousarray(z["ref%d" % bd], np.uint16 if hb else np.uint8)
        h, w = ref.shape
        mat = np.asarray(c["mat"], np.int32)
        out = np.zeros((c["ph"], c["pw"]), ref.dtype)
        # get_conv_params(0, plane, bd) of a single reference: round_1 = 2 * FILTER_BITS - round_0 (av1/common/convolve.h:63-100)
        cp = ConvolveParams(0, None, 0, c["round_0"], 14 - c["round_0"], 0, 0, 0, 0, 0)
        sh = [C.c_int16(v) for v in c["shear"]]
        head = [mat, ref, w, h, w, out, c["p_col"], c["p_row"], c["pw"], c["ph"], c["pw"], c["ss"], c["ss"]]
        if hb:
            call(fn("av1_highbd_warp_affine_c"), *head, bd, cp, *sh)
        else:
            call(fn("av1_warp_affine_c"), *head, cp, *sh)
        assert np.array_equal(out.astype(np.uint16), z["d%d" % c["k"]].reshape(c["ph"], c["pw"])), c


def test_lr_apply():
    """av1_apply_selfguided_restoration_c and av1_[highbd_]wiener_convolve_add_src_c.  The Wiener function finds its kernel through the
    ADDRESS of the filter (get_filter_base masks the low 8 bits, aom_dsp/aom_convolve.c): a 16-byte kernel in the first 256 bytes of a
    256-byte-aligned block, which is where this test puts it -- the compiled function runs as written, no patch."""
    z, cases = load("ref_eval_lr_apply.npz")
    assert len(cases) == 27
    kinds = {"sgr": 0, "wiener": 0}
    tmp = np.zeros(1 << 21, np.int32)       # >= RESTORATION_TMPBUF_SIZE / 4
    raw = np.zeros(512 + 128, np.int16)
    base = (-raw.ctypes.data % 256) // 2    # first 256-byte-aligned element
    for c in cases:
        bd, w, h = c["bd"], c["w"], c["h"]
        hb = bd > 8
        img = np.ascontiguousarray(z["img%d" % c["k"]], np.uint16 if hb else np.uint8)
        S = img.shape[1]
        out = np.zeros((h, w), img.dtype)
        src = Ptr(img, 3 * S + 3, hb)
        if c["kind"] == "sgr":
            call(fn("av1_apply_selfguided_restoration_c", C.c_int), src, w, h, S, c["idx"], np.asarray(c["xqd"], np.int32), Ptr(out, 0, hb), w, tmp, bd, int(hb))
        else:
            raw[base:base + 8] = c["fx"]; raw[base + 8:base + 16] = c["fy"]
            grow = 2 if bd == 12 else 0         # get_conv_params_wiener (av1/common/convolve.h:102-119): intbufrange = bd + 7 - 3 + 2 past 16
            cp = ConvolveParams(0, None, 0, 3 + grow, 11 - grow, 0, 0, 0, 0, 0)
            tail = [Ptr(raw, base), 16, Ptr(raw, base + 8), 16, w, h, cp]
            if hb:
                call(fn("av1_highbd_wiener_convolve_add_src_c"), src, SSZ(S), Ptr(out, 0, True), SSZ(w), *tail, bd)
            else:
                call(fn("av1_wiener_convolve_add_src_c"), src, SSZ(S), out, SSZ(w), *tail)
        assert np.array_equal(out.ravel().astype(np.uint16), z["out%d" % c["k"]]), c
        kinds[c["kind"]] += 1
    assert kinds == {"sgr": 15, "wiener": 12}


def interp_filters(fx, fy, w, h):
    """const InterpFilterParams *interp_filters[2] from av1_get_interp_filter_params_with_block_size (through the shim: its tables are static)"""
    f = fn("refshim_interp_filter_params", C.c_void_p, refc.shim())
    return (C.c_void_p * 2)(call(f, fx, w), call(f, fy, h))


def conv_params(cmp_index, conv_buf, conv_stride, is_compound, bd, weights=None):
    """get_conv_params_no_round (av1/common/convolve.h:63-95, through the shim: it is static inline)"""
    cp = ConvolveParams()
    call(fn("refshim_conv_params", None, refc.shim()), cp, cmp_index, 0, conv_buf, conv_stride, is_compound, bd)
    if weights:
        cp.use_dist_wtd_comp_avg, cp.fwd_offset, cp.bck_offset = 1, weights[0], weights[1]
    return cp


def facade(src, S, dst, w, h, filt, sx, sy, cp, bd):
    hb = bd > 8
    args = [src, S, Ptr(dst, 0, hb), w, w, h, filt, sx, 16, sy, 16, 0, cp]
    call(fn("av1_highbd_convolve_2d_facade" if hb else "av1_convolve_2d_facade"), *args, *([bd] if hb else []))


def test_convolve():
    """av1_[highbd_]convolve_2d_facade as compiled: get_filter_base / get_filter_offset run on real addresses, not on the interpreter's stand-ins"""
    z, cases = load("ref_eval_convolve.npz")
    assert len(cases) == 234
    for c in cases:
        bd, w, h = c["bd"], c["w"], c["h"]
        hb = bd > 8
        p = np.ascontiguousarray(z["p%d" % bd], np.uint16 if hb else np.uint8)
        S = p.shape[1]
        dst = np.zeros((h, w), p.dtype)
        facade(Ptr(p, c["y0"] * S + c["x0"], hb), S, dst, w, h, interp_filters(c["fx"], c["fy"], w, h), c["sx"], c["sy"], conv_params(0, None, 0, 0, bd), bd)
        assert np.array_equal(dst.ravel(), z["d%d" % c["k"]]), c


def _two_refs(z, c):
    bd = c["bd"]
    hb = bd > 8
    planes = [np.ascontiguousarray(z["p%d_%d" % (bd, r)], np.uint16 if hb else np.uint8) for r in range(2)]
    S = planes[0].shape[1]
    return planes, [Ptr(planes[r], c["pos"][r][1] * S + c["pos"][r][0], hb) for r in range(2)], S


def test_convolve_compound():
    z, cases = load("ref_eval_convolve_compound.npz")
    assert len(cases) == 44
    for c in cases:
        bd, w, h = c["bd"], c["w"], c["h"]
        planes, src, S = _two_refs(z, c)
        filt = interp_filters(c["fx"], c["fy"], w, h)
        buf16, dst = np.zeros(w * h, np.uint16), np.zeros((h, w), planes[0].dtype)
        for r in range(2):      # first reference into the CONV_BUF, second averaged in
            facade(src[r], S, dst, w, h, filt, c["subs"][r][0], c["subs"][r][1], conv_params(r, buf16, w, 1, bd, c["weights"]), bd)
        assert np.array_equal(dst.ravel(), z["d%d" % c["k"]]), c


def test_convolve_masked():
    z, cases = load("ref_eval_convolve_masked.npz")
    assert len(cases) == 34
    n_diff = 0
    for c in cases:
        bd, w, h = c["bd"], c["w"], c["h"]
        hb = bd > 8
        planes, src, S = _two_refs(z, c)
        filt = interp_filters(c["fx"], c["fy"], w, h)
        bufs, dst = [np.zeros(w * h, np.uint16) for _ in range(2)], np.zeros((h, w), planes[0].dtype)
        cps = [conv_params(0, bufs[r], w, 1, bd) for r in range(2)]
        for r in range(2):
            facade(src[r], S, dst, w, h, filt, c["subs"][r][0], c["subs"][r][1], cps[r], bd)
        if c.get("diffwtd"):    # the mask is an output of av1_build_compound_diffwtd_mask_d16_c
            mask = np.zeros((h, w), np.uint8)
            call(fn("av1_build_compound_diffwtd_mask_d16_c"), mask, c["diffwtd"] - 1, bufs[0], w, bufs[1], w, h, w, cps[0], bd)
            assert np.array_equal(mask, z["m%d" % c["k"]]), c
            n_diff += 1
        else:
            mask = np.ascontiguousarray(z["m%d" % c["k"]], np.uint8)
        u32 = C.c_uint32
        args = [Ptr(dst, 0, hb), u32(w), bufs[0], u32(w), bufs[1], u32(w), mask, u32(c["mask_stride"]), w, h, c["subw"], c["subh"], cps[0]]
        call(fn("aom_highbd_blend_a64_d16_mask_c" if hb else "aom_lowbd_blend_a64_d16_mask_c"), *args, *([bd] if hb else []))
        assert np.array_equal(dst.ravel(), z["d%d" % c["k"]]), c
    assert n_diff == 12


def test_qm_fp():
    """[highbd_]quantize_fp_helper_c is static: reached through av1_[highbd_]quantize_fp_facade (the shim fills MACROBLOCK_PLANE and
    QUANT_PARAM).  The facade takes the helper only with both matrices, so where the fixture passed one as NULL the other is the flat
    matrix of 1 << AOM_QM_BITS = 32, which is what the helper reads for a NULL pointer."""
    z, cases = load("ref_eval_qm_fp.npz")
    assert len(cases) == 140
    f = fn("refshim_quantize_fp_facade", None, refc.shim())
    for c in cases:
        k, n = c["k"], c["n"]
        t = rows8(c["tables"])
        sc, isc = ref_scan(c["tx_size"], 0, n)
        co = np.ascontiguousarray(z["c%d" % k], np.int32)
        flat = np.full(n, 32, np.uint8)
        qm = np.ascontiguousarray(z["qm_" + c["matrix"]], np.uint8) if c["which"] != "iqm_only" else flat
        iqm = np.ascontiguousarray(z["iqm_" + c["matrix"]], np.uint8) if c["which"] != "qm_only" else flat
        qc, dq, eob = np.full(n, 77, np.int32), np.full(n, 77, np.int32), np.full(1, 9, np.uint16)
        call(f, co, SSZ(n), t["zbin"], t["round"], t["quant"], t["quant_shift"], t["dequant"], qc, dq, eob, sc, isc, qm, iqm, c["log_scale"], c["hbd"])
        assert eob[0] == c["eob"] and np.array_equal(qc, z["q%d" % k]) and np.array_equal(dq, z["d%d" % k]), c


def test_warp_error():
    """av1_get_shear_params, av1_warp_error (av1/encoder/global_motion.c) and av1_segmented_frame_error (av1/common/warped_motion.c)"""
    z, cases = load("ref_eval_warp_error.npz")
    assert len(cases) == 17
    INT64_MAX = (1 << 63) - 1
    seen = {"invalid": 0, "bounded": 0, "frame": 0}
    for c in cases:
        bd = c["bd"]
        hb = bd > 8
        dt = np.uint16 if hb else np.uint8
        ref, cur = np.ascontiguousarray(z["ref%d" % bd].astype(dt)), np.ascontiguousarray(z["cur%d" % bd].astype(dt))
        seg = np.asarray(c["seg"], np.uint8)
        wm = WarpedMotionParams((C.c_int32 * 6)(*c["mat"]), 0, 0, 0, 0, 3, 0)     # wmtype AFFINE
        ok = call(fn("av1_get_shear_params", C.c_int), wm)
        assert ok == c["valid"], c["k"]
        if c["mat"][2] > 0:
            assert [wm.alpha, wm.beta, wm.gamma, wm.delta] == c["shear"], c["k"]
        if not ok:
            seen["invalid"] += 1
            continue

        def err(best):
            return call(fn("av1_warp_error", C.c_int64), wm, int(hb), bd, Ptr(ref, 0, hb), c["W"], c["H"], c["W"], Ptr(cur, 0, hb), c["p_col"], c["p_row"],
                        c["pw"], c["ph"], c["W"], c["ss"], c["ss"], C.c_int64(best), seg, c["seg_stride"])
        assert err(INT64_MAX) == int(c["error"]), c["k"]
        if "best_error" in c:
            assert err(int(c["best_error"])) == INT64_MAX == int(c["error_bounded"])
            seen["bounded"] += 1
        if "frame_error" in c:
            got = call(fn("av1_segmented_frame_error", C.c_int64), int(hb), bd, Ptr(ref, 0, hb), c["W"], Ptr(cur, 0, hb), c["W"], c["H"], c["W"], seg,
                       c["seg_stride"])
            assert got == int(c["frame_error"]), c["k"]
            seen["frame"] += 1
    assert seen["invalid"] >= 2 and seen["bounded"] >= 4 and seen["frame"] >= 6, seen


def test_vbp():
    """fill_variance_8x8avg / compute_minmax_8x8 / fill_variance_4x4avg (static in av1/encoder/var_based_part.c, through the shim that includes it)"""
    z, cases = load("ref_eval_vbp.npz")
    assert len(cases) == 88
    sh = refc.shim()
    kinds = {"8x8": 0, "4x4": 0}
    for c in cases:
        bd = c["bd"]
        hb = bd > 8
        dt = np.uint16 if hb else np.uint8
        src, dst = np.ascontiguousarray(z["src%d" % bd].astype(dt)), np.ascontiguousarray(z["dst%d" % bd].astype(dt))
        S = src.shape[1]
        sm, sq = np.zeros(4, np.int32), np.zeros(4, np.uint32)
        flag = 8 if hb else 0       # YV12_FLAG_HIGHBITDEPTH
        if c["kind"] == "8x8":
            call(fn("refshim_vbp_fill_8x8avg", None, sh), Ptr(src, 0, hb), S, Ptr(dst, 0, hb), S, c["x16"], c["y16"], flag, c["pw"], c["ph"], sm, sq)
            mm = call(fn("refshim_vbp_minmax_8x8", C.c_int, sh), Ptr(src, 0, hb), S, Ptr(dst, 0, hb), S, c["x16"], c["y16"], flag, c["pw"], c["ph"])
            assert (sm.tolist(), sq.tolist(), mm) == (c["sum"], c["sse"], c["minmax"]), c
        else:
            call(fn("refshim_vbp_fill_4x4avg", None, sh), Ptr(src, 0, hb), S, c["x8"], c["y8"], flag, c["pw"], c["ph"], c["border_offset"], sm, sq)
            assert (sm.tolist(), sq.tolist()) == (c["sum"], c["sse"]), c
        kinds[c["kind"]] += 1
    assert kinds == {"8x8": 48, "4x4": 40}, kinds


def test_intpro():
    """av1_int_pro_motion_estimation as compiled (the shim fills the struct members it reads), with aom_int_pro_row / col, aom_vector_var
    and the SAD members under it"""
    z = np.load(os.path.join(GOLD, "ref_eval_intpro.npz"))
    meta = json.loads(bytes(z["meta"]))
    cases, border = meta["cases"], meta["border"]
    assert len(cases) == 20
    f = fn("refshim_int_pro_motion_estimation", C.c_uint, refc.shim())
    for c in cases:
        bd = c["bd"]
        hb = bd > 8
        dt = np.uint16 if hb else np.uint8
        src, ref = np.ascontiguousarray(z["src%d" % bd].astype(dt)), np.ascontiguousarray(z["ref%d" % bd].astype(dt))
        S = src.shape[1]
        at = (border + c["by"]) * S + border + c["bx"]
        mv = np.zeros(2, np.int16)
        sad = call(f, Ptr(src, at, hb), Ptr(ref, at, hb), S, meta["width"], meta["height"], c["w"], c["h"], bd, np.asarray(c["limits"], np.int32),
                   np.asarray(c["ref_mv"], np.int16), c["by"] // 4, c["bx"] // 4, mv)
        assert (sad, mv.tolist()) == (c["best_sad"], c["mv"]), c


def test_lpf_flat():
    """The flat branches of filter6 / filter8 / filter14 (static in aom_dsp/loopfilter.c) through aom_lpf_vertical_{6,8,14}_c: the fixture
    holds what the tap statements make of a row, which is the function's output wherever its masks select the flat branch (all taps of
    the filter within 1 of p0 / q0, limits wide open) -- 200 rows per filter, of which the rows in the flat branch are counted."""
    g = np.load(os.path.join(GOLD, "ref_eval_lpf_flat.npz"))
    thr = [np.full(16, v, np.uint8) for v in (255, 255, 0)]
    taken = {}
    for name, length, reach in (("filter6", 6, 3), ("filter8", 8, 4), ("filter14", 14, 7)):
        rows, want = g[name + "/rows"], g[name + "/want"]
        assert rows.shape == (200, 14)
        taken[name] = 0
        for row, exp in zip(rows.tolist(), want.tolist()):
            p, q = row[6::-1], row[7:]
            if not all(abs(p[i] - p[0]) <= 1 and abs(q[i] - q[0]) <= 1 for i in range(1, reach)):
                continue
            px = np.zeros((4, 16), np.uint8)
            px[:, 1:15] = row
            call(fn("aom_lpf_vertical_%d_c" % length), Ptr(px, 8), 16, *thr)
            assert all(px[r, 1:15].tolist() == exp for r in range(4)), (name, row)
            taken[name] += 1
    assert taken == {"filter6": 92, "filter8": 61, "filter14": 29}, taken     # a property of the recorded rows


def test_cdef_fb():
    """av1_cdef_filter_fb on whole 64 x 64 filter blocks: the input tile is rebuilt from the recorded plane the way the generator built it
    (cdef_prepare_fb semantics: available neighbours copied, frame edges CDEF_VERY_LARGE), the cdef_list from the recorded skip map."""
    z, cases = load("ref_eval_cdef_fb.npz")
    assert len(cases) == 46
    for k, c in enumerate(cases):
        bd, xdec, ydec, pli = c["bd"], c["xdec"], c["ydec"], c["pli"]
        luma = z["luma%d" % bd].astype(np.int64)
        plane = luma if not pli else np.ascontiguousarray(luma[::(1 << ydec), ::(1 << xdec)])
        dst, dirs, var = cdef_fb_reference(plane, pli, xdec, ydec, c["y0"], c["x0"], c["pw"], c["ph"], z["s%d" % k], z["ld%d" % k] if pli else None,
                                           c["level"], c["sec"], c["damping"], bd)
        assert np.array_equal(dst.astype(np.uint16), z["o%d" % k]), c
        if not pli:
            assert np.array_equal(dirs, z["d%d" % k]) and np.array_equal(var, z["v%d" % k]), c
