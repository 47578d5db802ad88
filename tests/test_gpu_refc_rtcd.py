"""Every exact-signature export aomhip_<stem> against the reference ITSELF, compiled as C (oracle/_ref/libaomref_c.so, tests/refc.py): the
kernel and <aom|av1>_<stem>_c are called with the same host buffers and must leave them equal bit for bit -- results, inputs and the
guard regions around every output, which are pre-filled with a pattern.  No oracle and no fixture stands between the two; the oracle
only supplies scan orders and quantiser rows as INPUTS.  For the TxfmParam members equality also proves that the ctypes mirror of
aomhip_txfm_param (tests/test_gpu_rtcd_av1.py) has the reference's struct layout, since one struct object goes to both.

The set of exports driven is the `checked` list of tests/test_rtcd_protos.py (test_driven_set_is_the_checked_list); there is no
exclusion list.  One block per call, the input classes of tests/test_gpu_rtcd_shims.py / test_gpu_rtcd_av1.py: zero, DC only, extreme
DC, +-max checkerboards, random spans, pixel lines that fire every loop-filter mask, CDEF_VERY_LARGE borders, saturated blocks.

Where "bit for bit" is narrowed, it is stated where it applies: the 64-point forward transforms (the reference uses the coefficients past
the 32 x 32 it returns as scratch), and the `int` products of av1_block_error_c / _lp_c and aom_mse_wxh_16bit[_highbd]_c (inputs stay where
they do not overflow: signed overflow is undefined in compiled C)."""
import ctypes as C

import numpy as np
import pytest

import refc
from refc import Ptr, PtrList, byteptr
from refc_inputs import NC, TX, coeff_classes, coeffs_for_inverse, fp_tables, lpf_patch, param, pixels, residual_classes, wide
from test_rtcd_protos import checked_entry_points, reference_protos

pytestmark = pytest.mark.gpu
RESTYPE = {"void": None, "int": C.c_int, "unsigned int": C.c_uint, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
SSZ = C.c_ssize_t

LPF = ["aom_%slpf_%s_%d%s" % (hb, d, n, k) for hb in ("", "highbd_") for d in ("horizontal", "vertical") for n in (4, 6, 8, 14)
       for k in (("", "_dual", "_quad") if not hb else ("", "_dual"))]
QUANT_B = ["aom_%squantize_b%s%s" % (hb, s, a) for hb in ("", "highbd_") for s in ("", "_32x32", "_64x64") for a in ("", "_adaptive")]
FAMILIES = {
    "quantize_b": QUANT_B,
    "quantize_fp_lp": ["av1_quantize_fp", "av1_quantize_fp_32x32", "av1_quantize_fp_64x64", "av1_highbd_quantize_fp", "av1_quantize_lp"],
    "lpf": LPF,
    "fwd_txfm2d": ["av1_fwd_txfm2d_%dx%d" % wh for wh in TX],
    "inv_txfm2d_add": ["av1_inv_txfm2d_add_%dx%d" % wh for wh in TX],
    # the per-size TxfmParam forms: every size that has an add_proto (16x16 has none: the dispatcher handles it inline)
    "txfm_param_inv": ["av1_inv_txfm_add", "av1_highbd_inv_txfm_add"] + [n for n in ("av1_highbd_inv_txfm_add_%dx%d" % wh for wh in TX)
                                                                          if n in reference_protos()],
    "lossless": ["av1_fwht4x4", "av1_highbd_iwht4x4_16_add", "av1_highbd_iwht4x4_1_add"],
    "txfm_param_fwd": ["av1_lowbd_fwd_txfm", "av1_round_shift_array"],
    "block_error": ["av1_block_error", "av1_block_error_lp", "av1_highbd_block_error"],
    "cdef": ["cdef_find_dir", "cdef_find_dir_dual", "cdef_copy_rect8_8bit_to_16bit", "cdef_copy_rect8_16bit_to_16bit"] +
            ["cdef_filter_%d_%d" % (b, v) for b in (8, 16) for v in range(4)],
    "subtract_and_mask": ["aom_subtract_block", "aom_highbd_subtract_block", "aom_comp_mask_pred", "aom_highbd_comp_mask_pred"],
    "sums": ["aom_mse_wxh_16bit", "aom_mse_16xh_16bit", "aom_mse_wxh_16bit_highbd", "aom_get_mb_ss", "aom_get_var_sse_sum_8x8_quad",
             "aom_get_var_sse_sum_16x16_dual", "aom_sad16x16", "aom_sad16x16x4d", "aom_variance16x16"],
}

def test_driven_set_is_the_checked_list():
    checked, bad = checked_entry_points()
    assert not bad, bad
    driven = [n for names in FAMILIES.values() for n in names]
    assert len(driven) == len(set(driven))
    assert set(driven) == set(checked), (sorted(set(checked) - set(driven)), sorted(set(driven) - set(checked)))
    counts = {k: len(v) for k, v in FAMILIES.items()}
    assert counts["lpf"] == 40 and counts["fwd_txfm2d"] == 19 and counts["inv_txfm2d_add"] == 19 and counts["quantize_b"] == 12
    assert counts["cdef"] >= 10 and len(checked) == 148


class Driver:
    """the pair (aomhip_<stem>, <reference name>_c) of one family, with the count of calls per export"""

    def __init__(self, hip, family):
        self.hiplib, self.family, self.calls, self.wrote = hip.capi.lib, FAMILIES[family], {}, set()
        self.protos = reference_protos()
        refc.lib()

    def __call__(self, name, *args, note=None, ignore=None):
        assert name in self.family, name
        stem = name[4:] if name[:4] in ("aom_", "av1_") else name
        rt = RESTYPE[self.protos[name][0]]
        assert len(args) == len(self.protos[name][1]), (name, len(args), self.protos[name][1])
        r, bufs, wrote = refc.run_pair(refc.fn("aomhip_" + stem, rt, self.hiplib), refc.fn(name + "_c", rt), args, (name, note), ignore)
        self.calls[name] = self.calls.get(name, 0) + 1
        if wrote or r:
            self.wrote.add(name)
        return r, bufs

    def done(self):
        """every export of the family was called, and for each the reference wrote or returned something at least once"""
        assert set(self.calls) == set(self.family), sorted(set(self.family) - set(self.calls))
        assert self.wrote == set(self.family), sorted(set(self.family) - self.wrote)
        assert self.hiplib.aomhip_status() == 0, self.hiplib.aomhip_last_error()
        print("%s: %d exports, %d calls" % (self.family[0], len(self.calls), sum(self.calls.values())))


# ---------------------------------------------------------------- quantisers

def test_quantize_b_family(hip, oracle):
    d = Driver(hip, "quantize_b")
    rng = np.random.default_rng(1)
    for hbd in (0, 1):
        for adaptive in ("", "_adaptive"):
            for tx_size, suffix, ls in ((0, "", 0), (1, "", 0), (2, "", 0), (7, "", 0), (3, "_32x32", 1), (9, "_32x32", 1), (4, "_64x64", 2)):
                name = "aom_%squantize_b%s%s" % ("highbd_" if hbd else "", suffix, adaptive)
                sc, isc = oracle.get_scan(tx_size, 0)
                n = len(sc)
                for qindex in (0, 20, 255):
                    t = wide(oracle.build_quantizer_y(10 if hbd else 8, qindex))
                    for co in coeff_classes(rng, n, sc, t["dequant"][1], ls, 200000 if hbd else 8191):
                        qc, dq, eob = np.full(n + 8, 77, np.int32), np.full(n + 8, 77, np.int32), np.full(4, 9, np.uint16)
                        d(name, co, SSZ(n), t["zbin"], t["round"], t["quant"], t["quant_shift"], qc, dq, t["dequant"], eob, sc, isc,
                          note=(tx_size, qindex))
    d.done()


def test_quantize_fp_and_lp(hip, oracle):
    d = Driver(hip, "quantize_fp_lp")
    rng = np.random.default_rng(2)
    for tx_size, ls in ((0, 0), (1, 0), (2, 0), (7, 0), (3, 1), (9, 1), (4, 2)):
        sc, isc = oracle.get_scan(tx_size, 0)
        n = len(sc)
        for qindex in (0, 20, 100, 255):
            for hbd in (0, 1):
                q = oracle.build_quantizer_y(10 if hbd else 8, qindex)
                t = wide(fp_tables(q))
                for co in coeff_classes(rng, n, sc, t["dequant"][1], ls, 200000 if hbd else 8191):
                    qc, dq, eob = np.full(n + 8, 77, np.int32), np.full(n + 8, 77, np.int32), np.full(4, 9, np.uint16)
                    args = [co, SSZ(n), t["zbin"], t["round"], t["quant"], t["quant_shift"], qc, dq, t["dequant"], eob, sc, isc]
                    if hbd:
                        d("av1_highbd_quantize_fp", *args, ls, note=(tx_size, qindex))
                    else:
                        d("av1_quantize_fp" + ("", "_32x32", "_64x64")[ls], *args, note=(tx_size, qindex))
                    if not hbd and ls == 0:
                        co16 = np.clip(co, -32768, 32767).astype(np.int16)
                        qc16, dq16, eob = np.full(n + 8, 0x55, np.int16), np.full(n + 8, 0x55, np.int16), np.full(4, 77, np.uint16)
                        d("av1_quantize_lp", co16, SSZ(n), t["round"], t["quant"], qc16, dq16, t["dequant"], eob, sc, isc, note=(tx_size, qindex))
    d.done()


# ---------------------------------------------------------------- loop filter

def test_lpf_all_forty(hip):
    d = Driver(hip, "lpf")
    rng = np.random.default_rng(3)
    for name in LPF:
        hbd, dual = "highbd" in name, name.endswith("_dual")
        for bd in ((10, 12) if hbd else (8,)):
            for trial in range(18 if not hbd else 9):
                lim = [int(rng.integers(0, 3 * 63 + 5)), int(rng.integers(0, 64)), int(rng.integers(0, 16))] * 2
                if trial == 1:
                    lim = [255, 63, 0] * 2     # everything passes the masks, nothing is "high edge variance"
                if trial == 2:
                    lim = [0, 0, 0] * 2        # nothing passes
                thr = [np.full(16, v, np.uint8) for v in lim]
                px = lpf_patch(rng, bd, ("random", "flat", "flat", "step", "checker", "flat")[trial % 6])
                args = [Ptr(px, 16 * 32 + 16), 32, thr[0], thr[1], thr[2]] + (thr[3:] if dual else []) + ([bd] if hbd else [])
                d(name, *args, note=(bd, trial))
    d.done()


# ---------------------------------------------------------------- transforms

def test_fwd_txfm2d_every_size_and_type(hip, oracle):
    """Past the min(w, 32) x min(h, 32) coefficients a 64-point transform returns, av1_fwd_txfm2d_64xN_c / Nx64_c leave intermediate
    values and zeros (av1/encoder/av1_fwd_txfm2d.c: the zeroing and re-packing after fwd_txfm2d_c); no caller reads them
    (av1_get_max_eob).  There the comparison covers the returned coefficients and the guard after w * h; the 14 other sizes are
    compared whole."""
    d = Driver(hip, "fwd_txfm2d")
    rng = np.random.default_rng(4)
    for tx_size, (w, h) in enumerate(TX):
        name = "av1_fwd_txfm2d_%dx%d" % (w, h)
        for tx_type in range(16):
            if not oracle.av1_tx_valid(tx_size, tx_type):
                continue
            for bd in (8, 10, 12):
                for kind, res in residual_classes(rng, w, h, w + 5, bd)[:5 if tx_type in (0, 9) else 1]:
                    out = np.full(w * h + 16, 0x5a5a5a5a, np.int32)
                    if max(w, h) == 64:
                        d(name, res, out, w + 5, tx_type, bd, note=(tx_type, bd, kind), ignore={1: slice(NC[tx_size], w * h)})
                    else:
                        d(name, res, out, w + 5, tx_type, bd, note=(tx_type, bd, kind))
    d.done()


def test_inv_txfm2d_add_every_size_and_type(hip, oracle):
    d = Driver(hip, "inv_txfm2d_add")
    rng = np.random.default_rng(5)
    for tx_size, (w, h) in enumerate(TX):
        for tx_type in range(16):
            if not oracle.av1_tx_valid(tx_size, tx_type):
                continue
            for bd in (8, 10, 12):
                for kind in ("random", "zero", "dc", "extreme")[:4 if tx_type in (0, 9) else 1]:
                    co = coeffs_for_inverse(rng, tx_size, bd, kind)
                    dst = pixels(rng, h + 1, w + 3, bd, kind, np.uint16)
                    d("av1_inv_txfm2d_add_%dx%d" % (w, h), co, dst, w + 3, tx_type, bd, note=(tx_type, bd, kind))
    d.done()


def test_txfm_param_inverse_dispatchers(hip, oracle):
    d = Driver(hip, "txfm_param_inv")
    rng = np.random.default_rng(6)
    for tx_size, (w, h) in enumerate(TX):
        sized = "av1_highbd_inv_txfm_add_%dx%d" % (w, h)
        for tx_type in range(16):
            if not oracle.av1_tx_valid(tx_size, tx_type):
                continue
            for bd in (8, 10, 12):
                kind = ("random", "extreme", "dc")[(tx_type + bd // 2) % 3]
                co = coeffs_for_inverse(rng, tx_size, bd, kind)
                p = param(tx_size, tx_type, bd)
                dst = pixels(rng, h + 1, w + 3, bd, kind, np.uint16)
                d("av1_highbd_inv_txfm_add", co, byteptr(dst), w + 3, p, note=(tx_size, tx_type, bd, kind))
                if sized in d.family:
                    d(sized, co, byteptr(dst), w + 3, p, note=(tx_type, bd, kind))
                if bd == 8:
                    d("av1_inv_txfm_add", co, dst.astype(np.uint8), w + 3, p, note=(tx_size, tx_type, kind))
    # lossless: the eob rule of av1_highbd_iwht4x4_add through the dispatchers
    for bd in (8, 10, 12):
        for eob in (0, 1, 2, 16):
            co = rng.integers(-(1 << (bd + 2)), 1 << (bd + 2), 16).astype(np.int32)
            p = param(0, 0, bd, lossless=1, eob=eob)
            dst = pixels(rng, 5, 7, bd, "random", np.uint16)
            d("av1_highbd_inv_txfm_add", co, byteptr(dst), 7, p, note=("lossless", bd, eob))
            d("av1_highbd_inv_txfm_add_4x4", co, byteptr(dst), 7, p, note=("lossless", bd, eob))
            if bd == 8:
                d("av1_inv_txfm_add", co, dst.astype(np.uint8), 7, p, note=("lossless", eob))
    d.done()


def test_lossless_transforms(hip):
    d = Driver(hip, "lossless")
    rng = np.random.default_rng(7)
    for trial in range(60):
        res = rng.integers(-255, 256, (4, 9)).astype(np.int16)
        if trial % 4 == 0:
            res[:] = rng.choice([-255, 255], (4, 9))
        if trial == 1:
            res[:] = 0
        d("av1_fwht4x4", res, np.full(24, 7, np.int32), 9, note=trial)
        bd = (8, 10, 12)[trial % 3]
        co = rng.integers(-(1 << (bd + 2)), 1 << (bd + 2), 16).astype(np.int32)
        if trial % 5 == 0:
            co[1:] = 0
        dst = pixels(rng, 5, 7, bd, "extreme" if trial % 7 == 0 else "random", np.uint16)
        d("av1_highbd_iwht4x4_16_add", co, byteptr(dst), 7, bd, note=trial)
        d("av1_highbd_iwht4x4_1_add", co, byteptr(dst), 7, bd, note=trial)
    d.done()


def test_lowbd_fwd_txfm_and_round_shift_array(hip, oracle):
    """av1_lowbd_fwd_txfm_c = av1_highbd_fwd_txfm: the 64-point sizes return min(w, 32) x min(h, 32) coefficients and leave scratch
    after them (see test_fwd_txfm2d_every_size_and_type), so the output buffer there is exactly the returned size plus guard."""
    d = Driver(hip, "txfm_param_fwd")
    rng = np.random.default_rng(8)
    for tx_size, (w, h) in enumerate(TX):
        for tx_type in range(16):
            if not oracle.av1_tx_valid(tx_size, tx_type):
                continue
            for bd in (8, 10):
                kind, res = residual_classes(rng, w, h, w + 5, bd)[(tx_type + bd) % 5 if tx_type in (0, 9) else 0]
                p = param(tx_size, tx_type, bd)
                scratch = {1: slice(NC[tx_size], w * h)} if max(w, h) == 64 else None
                d("av1_lowbd_fwd_txfm", res, np.full(w * h + 16, 0x5a5a5a5a, np.int32), w + 5, p, note=(w, h, tx_type, bd, kind), ignore=scratch)
    for trial in range(12):
        res = rng.integers(-255, 256, (4, 9)).astype(np.int16)
        d("av1_lowbd_fwd_txfm", res, np.full(24, 7, np.int32), 9, param(0, 0, 8, lossless=1), note=("lossless", trial))
    for size in (1, 17, 300, 4096):
        for bit in range(-4, 9):
            a = rng.integers(-(1 << 31), 1 << 31, size + 4, dtype=np.int64).astype(np.int32)
            a[:min(size, 4)] = [-(1 << 31), (1 << 31) - 1, (1 << 28) + 5, -(1 << 28) - 5][:min(size, 4)]
            d("av1_round_shift_array", a, size, bit, note=(size, bit))
    d.done()


# ---------------------------------------------------------------- block error

def test_block_error(hip):
    """av1_block_error_c / _lp_c square 32-bit differences in `int`: inputs keep |coeff|, |diff| < 2^15.5 so the compiled reference's
    arithmetic is defined; av1_highbd_block_error_c is 64-bit throughout and takes the full range."""
    d = Driver(hip, "block_error")
    rng = np.random.default_rng(9)
    for n in (16, 17, 64, 100, 1024, 4096):
        for span in (100, 1 << 12, 1 << 15, 1 << 19):
            c = rng.integers(-span, span, n).astype(np.int32)
            dq = (c + rng.integers(-span // 4 - 1, span // 4 + 1, n)).astype(np.int32)
            for trial in range(3):
                if trial == 1:
                    dq = c.copy()
                if trial == 2:
                    c = np.where(np.arange(n) % 2 == 0, span - 1, -span).astype(np.int32); dq = np.zeros(n, np.int32)
                for bd in (8, 10, 12):
                    d("av1_highbd_block_error", c, dq, SSZ(n), np.full(2, -5, np.int64), bd, note=(n, span, bd))
                if span <= 1 << 15:
                    d("av1_block_error", c, dq, SSZ(n), np.full(2, -5, np.int64), note=(n, span))
                    c16, d16 = np.clip(c, -32768, 32767).astype(np.int16), np.clip(dq // 2, -32768, 32767).astype(np.int16)
                    d("av1_block_error_lp", c16, d16, SSZ(n), note=(n, span))
    d.done()


# ---------------------------------------------------------------- CDEF

def test_cdef(hip):
    d = Driver(hip, "cdef")
    rng = np.random.default_rng(10)
    for bd in (8, 10, 12):
        for trial in range(14):
            img = rng.integers(0, 1 << bd, (9, 24)).astype(np.uint16)
            if trial % 3 == 0:  # a directional ramp
                yy, xx = np.mgrid[0:9, 0:24]
                img = np.clip(((yy * (trial % 5) + xx * 3) % 64) << (bd - 6), 0, (1 << bd) - 1).astype(np.uint16)
            if trial == 1:
                img[:] = (1 << bd) - 1
            if trial == 2:
                yy, xx = np.mgrid[0:9, 0:24]; img = (((yy + xx) & 1) * ((1 << bd) - 1)).astype(np.uint16)
            d("cdef_find_dir", img, 24, np.full(2, -1, np.int32), bd - 8, note=(bd, trial))
            d("cdef_find_dir_dual", img, Ptr(img, 8), 24, np.full(2, -1, np.int32), np.full(2, -1, np.int32), bd - 8, np.full(2, -1, np.int32),
              np.full(2, -1, np.int32), note=(bd, trial))
    for bits, is16 in ((8, 0), (16, 1)):
        for variant in range(4):
            for trial in range(30):
                bd = 8 if not is16 else (10, 12)[trial % 2]
                bw, bh = [(8, 8), (4, 4), (8, 4), (4, 8)][trial % 4]
                buf = rng.integers(0, 1 << bd, (16, 144)).astype(np.uint16)
                if trial % 5 == 4:
                    yy, xx = np.mgrid[0:16, 0:144]; buf = (((yy + xx) & 1) * ((1 << bd) - 1)).astype(np.uint16)
                if trial % 2:
                    buf[:, :3] = 0x4000; buf[:2, :] = 0x4000  # CDEF_VERY_LARGE outside the frame
                if trial % 6 == 3:
                    buf[:, 4 + bw:] = 0x4000; buf[3 + bh:, :] = 0x4000
                # the variants exist for the non-zero strengths they name (av1_cdef_filter_fb picks by pri / sec != 0)
                pri = int(rng.integers(1, 16)) << (bd - 8) if variant in (0, 1) else 0
                sec = int(rng.choice([1, 2, 4])) << (bd - 8) if variant in (0, 2) else 0
                dirn, pd, sd = int(rng.integers(0, 8)), int(rng.integers(3, 7)) + (bd - 8), int(rng.integers(3, 7)) + (bd - 8)
                dst = np.full((bh + 1, 11), 99, np.uint16 if is16 else np.uint8)
                d("cdef_filter_%d_%d" % (bits, variant), dst, 11, Ptr(buf, 3 * 144 + 4), pri, sec, dirn, pd, sd, bd - 8, bw, bh, note=(bd, trial))
    for width, height, sstride, dstride in ((7, 5, 9, 11), (13, 11, 13, 21), (72, 80, 75, 144), (1, 1, 3, 1), (64, 3, 101, 67), (8, 8, 8, 8)):
        for src_t, name in ((np.uint8, "cdef_copy_rect8_8bit_to_16bit"), (np.uint16, "cdef_copy_rect8_16bit_to_16bit")):
            for hi in (256, 65536):
                src = rng.integers(0, min(hi, 256 if src_t == np.uint8 else 65536), (height, sstride)).astype(src_t)
                d(name, np.full((height + 1, dstride), 0xBEEF, np.uint16), dstride, src, sstride, width, height, note=(width, height))
    d.done()


# ---------------------------------------------------------------- subtract, masked prediction

def test_subtract_and_comp_mask_pred(hip):
    d = Driver(hip, "subtract_and_mask")
    rng = np.random.default_rng(11)
    shapes = ((4, 4), (8, 16), (32, 8), (64, 64), (128, 128), (16, 64), (4, 16))
    for bd in (8, 10, 12):
        dt, hb = (np.uint8, False) if bd == 8 else (np.uint16, True)
        for rows, cols in shapes:
            for kind in ("random", "max-zero"):
                src = rng.integers(0, 1 << bd, (rows + 2, cols + 7)).astype(dt); pred = rng.integers(0, 1 << bd, (rows + 1, cols + 3)).astype(dt)
                if kind == "max-zero":
                    src[:] = (1 << bd) - 1 if rows != 8 else 0
                    pred[:] = (1 << bd) - 1 - src[0, 0]
                diff = np.full((rows + 1, cols + 2), 12345, np.int16)
                d("aom_subtract_block" if bd == 8 else "aom_highbd_subtract_block", rows, cols, diff, SSZ(cols + 2), Ptr(src, 1, hb), SSZ(cols + 7),
                  Ptr(pred, 2, hb), SSZ(cols + 3), note=(bd, rows, cols, kind))
                for invert in (0, 1):
                    w, h = cols, rows
                    mask = rng.integers(0, 65, (h, w + 5)).astype(np.uint8)
                    if kind == "max-zero":
                        mask[:] = np.where(np.arange(w + 5) % 2, 64, 0)
                    comp = np.full(w * h + 16, 0xAB, dt)
                    p2 = np.ascontiguousarray(pred[:h, :w])
                    d("aom_comp_mask_pred" if bd == 8 else "aom_highbd_comp_mask_pred", Ptr(comp, 0, hb), Ptr(p2, 0, hb), w, h, Ptr(src, 1, hb),
                      cols + 7, mask, w + 5, invert, note=(bd, w, h, kind, invert))
    d.done()


# ---------------------------------------------------------------- sums of squares, SAD, variance

def test_mse_var_sums_sad_variance(hip):
    """aom_get_var_sse_sum_8x8_quad_c / _16x16_dual_c ADD to *tot_sse and *tot_sum: both sides start from the same non-zero totals.
    aom_mse_wxh_16bit[_highbd]_c square the difference in `int` (aom_dsp/variance.c): the 16-bit operands stay within 12 bits, the widest
    pixels their callers pass; past 46 340 the compiled reference's product is undefined (it wraps, the kernel's 64-bit sum does not)."""
    d = Driver(hip, "sums")
    rng = np.random.default_rng(12)
    for trial in range(24):
        sat = trial % 4 == 3
        for w, h in ((4, 4), (4, 8), (8, 4), (8, 8)):
            dst8 = rng.integers(0, 256, (h + 1, w + 5)).astype(np.uint8)
            dst16 = rng.integers(0, 4096, (h + 1, w + 5)).astype(np.uint16)
            src = rng.integers(0, 4096, (h, w + 3)).astype(np.uint16)
            if sat:
                dst8[:] = 0; dst16[:] = 0; src[:] = 4095
            d("aom_mse_wxh_16bit", dst8, w + 5, src, w + 3, w, h, note=(w, h, trial))
            d("aom_mse_wxh_16bit_highbd", dst16, w + 5, src, w + 3, w, h, note=(w, h, trial))
        for w, h in ((4, 4), (8, 8), (4, 8), (8, 4)):   # 16 / w blocks of w x h side by side, the source packed block after block
            dst8 = rng.integers(0, 256, (h + 1, 16 + 5)).astype(np.uint8)
            src = rng.integers(0, 4096, 16 * h + 3).astype(np.uint16)
            if sat:
                dst8[:] = 0; src[:] = 4095
            d("aom_mse_16xh_16bit", dst8, 16 + 5, src, w, h, note=(w, h, trial))
        res = rng.integers(-255 << (trial % 3 * 2), (255 << (trial % 3 * 2)) + 1, 256).astype(np.int16)
        if sat:
            res[:] = np.where(np.arange(256) % 2, 32767, -32768)
        d("aom_get_mb_ss", res, note=trial)
        a = rng.integers(0, 256, (17, 40)).astype(np.uint8); b = rng.integers(0, 256, (18, 37)).astype(np.uint8)
        if sat:
            a[:] = 255; b[:] = 0
        tot = lambda: (np.asarray([1000 + trial, 7], np.uint32), np.asarray([-300 + trial, 7], np.int32))
        ts, tm = tot()
        d("aom_get_var_sse_sum_8x8_quad", Ptr(a, 3), 40, Ptr(b, 37 + 2), 37, np.full(5, 9, np.uint32), np.full(5, 9, np.int32), ts, tm,
          np.full(5, 9, np.uint32), note=trial)
        ts, tm = tot()
        d("aom_get_var_sse_sum_16x16_dual", Ptr(a, 3), 40, Ptr(b, 37 + 2), 37, np.full(3, 9, np.uint32), ts, tm, np.full(3, 9, np.uint32), note=trial)
        d("aom_sad16x16", Ptr(a, 1), 40, Ptr(b, 37 + 3), 37, note=trial)
        d("aom_variance16x16", Ptr(a, 1), 40, Ptr(b, 37 + 3), 37, np.full(2, 9, np.uint32), note=trial)
        d("aom_sad16x16x4d", Ptr(a, 1), 40, PtrList([Ptr(b, 0), Ptr(b, 1), Ptr(b, 37), Ptr(b, 2 * 37 + 5)]), 37, np.full(5, 9, np.uint32), note=trial)
    d.done()
