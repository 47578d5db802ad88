"""The av1_rtcd transform / quantisation surface (include/aomhip.h, csrc/rtcd_av1.hip) driven through the C ABI on host buffers: the TxfmParam
dispatchers and their per-size forms, the lossless pair, fp / lp quantisers, block errors (the shims and the batched calls on device-resident
blocks), av1_round_shift_array, the CDEF rectangle copies, the installer aomhip_rtcd_av1 and the failure handling.  Every result must equal
the oracle bit for bit (tests/test_golden_ref_eval.py / test_golden_quant_lp.py pin the oracle to the interpreted reference) and, where the
committed fixtures hold the reference's own outputs, those directly."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P = lambda a: C.c_void_p(a.ctypes.data)
HB = lambda a: C.c_void_p(a.ctypes.data >> 1)   # CONVERT_TO_BYTEPTR (aom_ports/mem.h:79-80)
TX = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (4, 8), (8, 4), (8, 16), (16, 8), (16, 32), (32, 16), (32, 64), (64, 32), (4, 16), (16, 4),
      (8, 32), (32, 8), (16, 64), (64, 16)]
NC = [min(w, 32) * min(h, 32) for w, h in TX]


class TxfmParam(C.Structure):
    """TxfmParam (aom_dsp/txfm_common.h:89-101) = aomhip_txfm_param"""
    _fields_ = [("tx_type", C.c_uint8), ("tx_size", C.c_uint8), ("lossless", C.c_int), ("bd", C.c_int), ("is_hbd", C.c_int),
                ("tx_set_type", C.c_uint8), ("eob", C.c_int)]


def param(tx_size, tx_type, bd, lossless=0, eob=0):
    return TxfmParam(tx_type, tx_size, lossless, bd, int(bd > 8), 0, eob)


def load(name):
    z = np.load(os.path.join(GOLD, name))
    return z, json.loads(bytes(z["cases"]).decode())


def _orc(oracle, name, restype=None):
    f = getattr(oracle.lib, name)
    f.restype = restype
    f.argtypes = None
    return f


def inv_oracle(oracle, co, dst, tx_size, tx_type, bd):
    return oracle.inv_txfm2d_add(co[:NC[tx_size]], dst, tx_size, tx_type, bd)


def iwht_oracle(oracle, co, dst, eob, bd):
    out = np.ascontiguousarray(dst, np.uint16).copy()
    _orc(oracle, "orc_iwht4x4_add")(P(np.ascontiguousarray(co, np.int32)), P(out), C.c_int(4), C.c_int(eob), C.c_int(bd))
    return out


def run_inv(lib, name, co, dst, stride, bd, p):
    """one inverse call: bd 8 on the 8-bit entry with uint8 pixels, else a highbd entry with CONVERT_TO_BYTEPTR pixels"""
    got = dst.copy()
    getattr(lib, name)(P(co), P(got) if got.dtype == np.uint8 else HB(got), C.c_int(stride), C.byref(p))
    return got


# ---------------------------------------------------------------- inverse transforms

@pytest.mark.parametrize("bd", [8, 10, 12])
def test_inv_txfm_add_every_size_and_type(hip, oracle, bd):
    lib = hip.capi.lib
    lib.aomhip_status_clear()
    rng = np.random.default_rng(100 + bd)
    pix = np.uint8 if bd == 8 else np.uint16
    for tx_size, (w, h) in enumerate(TX):
        nc = NC[tx_size]
        for tx_type in range(16):
            if not oracle.av1_tx_valid(tx_size, tx_type):
                continue
            for kind in ("random", "extreme"):
                co = np.zeros(nc, np.int32)
                if kind == "random":
                    co[:] = (rng.integers(-(1 << (bd + 3)), 1 << (bd + 3), nc) * (rng.random(nc) < 0.3)).astype(np.int32)
                else:   # beyond the input clamp, DC at the range limits
                    co[:] = rng.integers(-(1 << (bd + 9)), 1 << (bd + 9), nc)
                    co[0] = rng.choice([-(1 << (bd + 7)), (1 << (bd + 7)) - 1])
                stride = w + 3
                dst = rng.integers(0, 1 << bd, (h, stride)).astype(pix)
                want = dst.copy()
                want[:, :w] = inv_oracle(oracle, co, np.ascontiguousarray(dst[:, :w]).astype(np.uint16), tx_size, tx_type, bd).astype(pix)
                p = param(tx_size, tx_type, bd)
                names = ["aomhip_inv_txfm_add"] if bd == 8 else ["aomhip_highbd_inv_txfm_add", "aomhip_highbd_inv_txfm_add_%dx%d" % (w, h)]
                if bd == 8:
                    names.append(None)   # the highbd dispatcher at bd 8 on uint16 pixels
                for name in names:
                    if name is None:
                        got = run_inv(lib, "aomhip_highbd_inv_txfm_add", co, dst.astype(np.uint16), stride, bd, p)
                        assert np.array_equal(got, want.astype(np.uint16)), ("highbd@8", w, h, tx_type, kind)
                        continue
                    if name.endswith("%dx%d" % (w, h)):
                        p.tx_size = (tx_size + 5) % 19   # the per-size forms take their size from their name
                    got = run_inv(lib, name, co, dst, stride, bd, p)
                    p.tx_size = tx_size
                    assert np.array_equal(got, want), (name, w, h, tx_type, bd, kind)
    assert lib.aomhip_status() == 0


def test_inv_txfm_add_matches_reference_evaluation(hip, oracle):
    lib = hip.capi.lib
    z, cases = load("ref_eval_txfm2d.npz")
    n = 0
    for k, c in enumerate(cases):
        if "inv_bd" not in c:
            continue
        w, h, bd = c["w"], c["h"], c["inv_bd"]
        dq = np.ascontiguousarray(z["dq%d" % k], np.int32)
        pred = z["p%d" % k].reshape(h, w)
        if c.get("wht"):
            p = param(0, 0, bd, lossless=1, eob=c["eob"])
        else:
            p = param(c["tx_size"], c["tx_type"], bd)
            dq = np.ascontiguousarray(dq[:NC[c["tx_size"]]])
        if bd == 8:
            got = run_inv(lib, "aomhip_inv_txfm_add", dq, np.ascontiguousarray(pred.astype(np.uint8)), w, bd, p)
        else:
            got = run_inv(lib, "aomhip_highbd_inv_txfm_add", dq, np.ascontiguousarray(pred.astype(np.uint16)), w, bd, p)
        assert np.array_equal(got.astype(np.uint16), z["r%d" % k].reshape(h, w)), c
        n += 1
    assert n >= 200


def test_lossless_4x4_eob_rule(hip, oracle):
    """av1_highbd_iwht4x4_add (idct.c:34-41): _16_add when eob > 1, _1_add otherwise -- eob 0 included (the dispatchers do not skip)."""
    lib = hip.capi.lib
    lib.aomhip_status_clear()
    rng = np.random.default_rng(44)
    for bd in (8, 10, 12):
        for eob in (0, 1, 2, 16):
            for case in ("dc", "ac", "random"):
                co = np.zeros(16, np.int32)
                if case == "dc":
                    co[0] = int(rng.integers(-(1 << (bd + 2)), 1 << (bd + 2)))
                elif case == "ac":   # at eob <= 1, _1_add ignores these
                    co[0] = 40
                    co[[1, 4, 5, 15]] = rng.integers(-300, 300, 4)
                else:
                    co[:] = rng.integers(-(1 << (bd + 2)), 1 << (bd + 2), 16)
                dst = rng.integers(0, 1 << bd, (4, 7)).astype(np.uint16)
                want = dst.copy()
                want[:, :4] = iwht_oracle(oracle, co, np.ascontiguousarray(dst[:, :4]), eob, bd)
                p = param(0, 0, bd, lossless=1, eob=eob)
                for name in ("aomhip_highbd_inv_txfm_add", "aomhip_highbd_inv_txfm_add_4x4"):
                    assert np.array_equal(run_inv(lib, name, co, dst, 7, bd, p), want), (name, bd, eob, case)
                if bd == 8:
                    got = run_inv(lib, "aomhip_inv_txfm_add", co, dst.astype(np.uint8), 7, bd, p)
                    assert np.array_equal(got, want.astype(np.uint8)), ("8-bit", eob, case)
                f = "aomhip_highbd_iwht4x4_16_add" if eob > 1 else "aomhip_highbd_iwht4x4_1_add"
                got = dst.copy()
                getattr(lib, f)(P(co), HB(got), C.c_int(7), C.c_int(bd))
                assert np.array_equal(got, want), (f, bd, eob, case)
    assert lib.aomhip_status() == 0


# ---------------------------------------------------------------- forward transforms

def test_lowbd_fwd_txfm_every_size_and_type(hip, oracle):
    lib = hip.capi.lib
    lib.aomhip_status_clear()
    rng = np.random.default_rng(5)
    for tx_size, (w, h) in enumerate(TX):
        nc = NC[tx_size]
        for tx_type in range(16):
            if not oracle.av1_tx_valid(tx_size, tx_type):
                continue
            for bd in (8, 10):
                stride = w + 5
                res = rng.integers(-(1 << bd) + 1, 1 << bd, (h, stride)).astype(np.int16)
                if tx_type == 0 and bd == 8:
                    res[:] = rng.choice([-255, 255], (h, stride))   # extreme residual
                out = np.full(w * h, 0x5a5a5a5a, np.int32)
                lib.aomhip_lowbd_fwd_txfm(P(res), P(out), C.c_int(stride), C.byref(param(tx_size, tx_type, bd)))
                want = oracle.fwd_txfm2d(np.ascontiguousarray(res[:, :w]), tx_size, tx_type, bd)
                assert np.array_equal(out[:nc], want[:nc]), (w, h, tx_type, bd)
    # lossless: av1_fwht4x4 through the dispatcher and on its own
    for trial in range(40):
        res = rng.integers(-255, 256, (4, 9)).astype(np.int16)
        if trial % 4 == 0:
            res[:] = rng.choice([-255, 255], (4, 9))
        want = np.zeros(16, np.int32)
        _orc(oracle, "orc_fwht4x4")(P(np.ascontiguousarray(res[:, :4])), P(want), C.c_int(4))
        out = np.full(16, 7, np.int32)
        lib.aomhip_lowbd_fwd_txfm(P(res), P(out), C.c_int(9), C.byref(param(0, 0, 8, lossless=1)))
        assert np.array_equal(out, want), trial
        out = np.full(16, 7, np.int32)
        lib.aomhip_fwht4x4(P(res), P(out), C.c_int(9))
        assert np.array_equal(out, want), trial
    assert lib.aomhip_status() == 0


def test_fwd_txfm_matches_reference_evaluation(hip):
    lib = hip.capi.lib
    z, cases = load("ref_eval_txfm2d.npz")
    n_wht = 0
    for k, c in enumerate(cases):
        w, h = c["w"], c["h"]
        x = np.ascontiguousarray(z["x%d" % k].reshape(h, w).astype(np.int16))
        out = np.full(w * h, 0x5a5a5a5a, np.int32)
        if c.get("wht"):
            lib.aomhip_lowbd_fwd_txfm(P(x), P(out), C.c_int(w), C.byref(param(0, 0, c["bd"], lossless=1)))
            assert np.array_equal(out[:16], z["c%d" % k]), c
            out2 = np.zeros(16, np.int32)
            lib.aomhip_fwht4x4(P(x), P(out2), C.c_int(4))
            assert np.array_equal(out2, z["c%d" % k]), c
            n_wht += 1
            continue
        nn = NC[c["tx_size"]]
        lib.aomhip_lowbd_fwd_txfm(P(x), P(out), C.c_int(w), C.byref(param(c["tx_size"], c["tx_type"], c["bd"])))
        assert np.array_equal(out[:nn], z["c%d" % k][:nn]), c
    assert n_wht == 24


# ---------------------------------------------------------------- quantisers

def fp_tables(q):
    """plausible round_fp / quant_fp rows for a dequantiser (av1_build_quantizer's shape); the oracle takes any"""
    dq = q["dequant"].astype(np.int64)
    return {"round": ((dq * 64) >> 7).astype(np.int16), "quant": np.minimum((1 << 16) // dq, 32767).astype(np.int16),
            "dequant": q["dequant"].astype(np.int16), "zbin": q["zbin"].astype(np.int16), "quant_shift": q["quant_shift"].astype(np.int16)}


def input_classes(rng, n, sc, q, ls, hbd):
    """test_gpu_rtcd_shims.test_quantize_b_family's classes: zero, DC only, extreme DC, constant, random spans, a lone level"""
    out = [np.zeros(n, np.int32)]
    dc = np.zeros(n, np.int32); dc[0] = 300; out.append(dc)
    ex = np.zeros(n, np.int32); ex[0] = -8191; out.append(ex)
    out.append(np.full(n, 16, np.int32))
    for span in (32, 1024, 8191 if not hbd else 200000):
        out.append(rng.integers(-span, span + 1, n).astype(np.int32))
    lone = np.zeros(n, np.int32); lone[int(sc[min(5, n - 1)])] = int(q["dequant"][1]) // (1 << ls) + 1; out.append(lone)
    return out


def orc_fp(oracle, co, t, sc, ls, hbd):
    qc, dq, e = np.zeros_like(co), np.zeros_like(co), C.c_uint16()
    _orc(oracle, "orc_quantize_fp")(P(co), C.c_ssize_t(co.size), P(t["round"]), P(t["quant"]), P(qc), P(dq), P(t["dequant"]), C.byref(e), P(sc),
                                    C.c_int(ls), C.c_int(int(hbd)))
    return qc, dq, e.value


def call_fp(lib, co, t, sc, isc, ls, hbd, via_name=None):
    qc, dq, e = np.full(co.size, 77, np.int32), np.full(co.size, 77, np.int32), C.c_uint16(9)
    args = [P(co), C.c_ssize_t(co.size), P(t["zbin"]), P(t["round"]), P(t["quant"]), P(t["quant_shift"]), P(qc), P(dq), P(t["dequant"]),
            C.byref(e), P(sc), P(isc)]
    if hbd:
        lib.aomhip_highbd_quantize_fp(*args, C.c_int(ls))
    else:
        getattr(lib, via_name or "aomhip_quantize_fp" + ("", "_32x32", "_64x64")[ls])(*args)
    return qc, dq, e.value


@pytest.mark.parametrize("hbd", [False, True])
def test_quantize_fp_family(hip, oracle, hbd):
    lib = hip.capi.lib
    lib.aomhip_status_clear()
    rng = np.random.default_rng(17 + hbd)
    for tx_size, ls in ((0, 0), (1, 0), (2, 0), (7, 0), (3, 1), (9, 1), (4, 2)):
        sc, isc = oracle.get_scan(tx_size, 0)
        for qindex in (0, 1, 20, 100, 200, 255):
            q = oracle.build_quantizer_y(10 if hbd else 8, qindex)
            t = fp_tables(q)
            for co in input_classes(rng, len(sc), sc, q, ls, hbd):
                got = call_fp(lib, co, t, sc, isc, ls, hbd)
                want = orc_fp(oracle, co, t, sc, ls, hbd)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (tx_size, qindex, hbd)
    assert lib.aomhip_status() == 0


def test_quantize_fp_matches_reference_evaluation(hip, oracle):
    lib = hip.capi.lib
    z, cases = load("ref_eval_quant.npz")
    rows = z["quantize_fp"]
    assert len(rows) >= 130
    for kk, eob, r0, r1, q0, q1 in rows.tolist():
        c = cases[kk]
        co = np.ascontiguousarray(z["c%d" % kk], np.int32)
        sc, isc = oracle.get_scan(c["tx_size"], c["tx_type"])
        t = {"round": np.asarray([r0, r1], np.int16), "quant": np.asarray([q0, q1], np.int16), "dequant": np.asarray(c["tables"]["dequant"], np.int16),
             "zbin": np.asarray(c["tables"]["zbin"], np.int16), "quant_shift": np.asarray(c["tables"]["quant_shift"], np.int16)}
        qc, dq, e = call_fp(lib, co, t, sc, isc, c["log_scale"], c["hbd"])
        assert e == eob and np.array_equal(qc, z["fq%d" % kk]) and np.array_equal(dq, z["fd%d" % kk]), (kk, c["fn"])


def call_lp(lib, co, t, sc, isc):
    qc, dq, e = np.full(co.size, 0x55, np.int16), np.full(co.size, 0x55, np.int16), C.c_uint16(77)
    lib.aomhip_quantize_lp(P(co), C.c_ssize_t(co.size), P(t["round"]), P(t["quant"]), P(qc), P(dq), P(t["dequant"]), C.byref(e), P(sc), P(isc))
    return qc, dq, e.value


def test_quantize_lp(hip, oracle):
    lib = hip.capi.lib
    lib.aomhip_status_clear()
    z, cases = load("ref_eval_quant_lp.npz")
    for cs in cases:     # the reference's own outputs
        k = cs["k"]
        co = np.ascontiguousarray(z["c%d" % k], np.int16)
        sc, isc = oracle.get_scan(cs["tx_size"], cs["tx_type"])
        t = {m: np.asarray(v, np.int16) for m, v in cs["tables"].items()}
        qc, dq, e = call_lp(lib, co, t, sc, isc)
        assert np.array_equal(qc, z["q%d" % k]) and np.array_equal(dq, z["d%d" % k]) and e == cs["eob"], cs
        assert lib.aomhip_block_error_lp(P(co), P(dq), C.c_ssize_t(co.size)) == cs["block_error"], cs
    rng = np.random.default_rng(23)
    for tx_size in (0, 1, 2, 3, 7, 13):
        for tx_type in ((0, 9) if tx_size == 3 else (0, 4, 10, 11)):
            sc, isc = oracle.get_scan(tx_size, tx_type)
            n = len(sc)
            for qindex in (0, 1, 20, 100, 200, 255):
                t = fp_tables(oracle.build_quantizer_y(8, qindex))
                for co in input_classes(rng, n, sc, oracle.build_quantizer_y(8, qindex), 0, False):
                    co = np.clip(co, -32768, 32767).astype(np.int16)
                    got = call_lp(lib, co, t, sc, isc)
                    wq, wd, we = np.zeros(n, np.int16), np.zeros(n, np.int16), C.c_uint16()
                    _orc(oracle, "orc_quantize_lp")(P(co), C.c_ssize_t(n), P(t["round"]), P(t["quant"]), P(wq), P(wd), P(t["dequant"]), C.byref(we), P(sc))
                    assert np.array_equal(got[0], wq) and np.array_equal(got[1], wd) and got[2] == we.value, (tx_size, tx_type, qindex)
    assert lib.aomhip_status() == 0


# ---------------------------------------------------------------- block error

def orc_block_error(oracle, c, d, bd):
    ssz = C.c_int64()
    e = _orc(oracle, "orc_block_error", C.c_int64)(P(c), P(d), C.c_ssize_t(c.size), C.byref(ssz), C.c_int(bd))
    return e, ssz.value


def orc_block_error_lp(oracle, c, d):
    return _orc(oracle, "orc_block_error_lp", C.c_int64)(P(c), P(d), C.c_ssize_t(c.size))


def shim_block_error(lib, c, d, bd):
    """bd 0: aomhip_block_error (the low-bd form), else aomhip_highbd_block_error"""
    ssz = C.c_int64(-5)
    if bd == 0:
        e = lib.aomhip_block_error(P(c), P(d), C.c_ssize_t(c.size), C.byref(ssz))
    else:
        e = lib.aomhip_highbd_block_error(P(c), P(d), C.c_ssize_t(c.size), C.byref(ssz), C.c_int(bd))
    return e, ssz.value


def test_block_error_shims(hip, oracle):
    lib = hip.capi.lib
    lib.aomhip_status_clear()
    z, _ = load("ref_eval_quant.npz")
    rows = z["block_error"]
    assert len(rows) >= 90
    for row in rows:
        kk = int(row[0])
        c, d = np.ascontiguousarray(z["c%d" % kk], np.int32), np.ascontiguousarray(z["d%d" % kk], np.int32)
        for j, bd in enumerate((0, 8, 10, 12)):
            assert shim_block_error(lib, c, d, bd) == (int(row[1 + 2 * j]), int(row[2 + 2 * j])), (kk, bd)
    rng = np.random.default_rng(31)
    for n in (1, 16, 17, 64, 100, 1024, 4096):
        for span in (100, 1 << 15, 1 << 19):
            c = rng.integers(-span, span, n).astype(np.int32)
            d = (c + rng.integers(-span // 4 - 1, span // 4 + 1, n)).astype(np.int32)
            for bd in (0, 8, 10, 12):
                assert shim_block_error(lib, c, d, bd) == orc_block_error(oracle, c, d, bd), (n, span, bd)
            c16 = np.clip(c, -32768, 32767).astype(np.int16)
            d16 = np.clip(d, -32768, 32767).astype(np.int16)
            assert lib.aomhip_block_error_lp(P(c16), P(d16), C.c_ssize_t(n)) == orc_block_error_lp(oracle, c16, d16), (n, span)
    # 32-bit products that overflow: the low-bd forms wrap like the compiled reference, the highbd form does not
    c = np.full(64, 1 << 17, np.int32); c[1::2] = -(1 << 17) - 3
    d = -c
    lo, hi = shim_block_error(lib, c, d, 0), shim_block_error(lib, c, d, 8)
    assert lo == orc_block_error(oracle, c, d, 0) and hi == orc_block_error(oracle, c, d, 8) and lo != hi
    c16, d16 = np.full(32, 32767, np.int16), np.full(32, -32768, np.int16)   # diff 65535: the square wraps in 32 bits
    got = lib.aomhip_block_error_lp(P(c16), P(d16), C.c_ssize_t(32))
    assert got == orc_block_error_lp(oracle, c16, d16) and got != 32 * 65535 ** 2
    assert lib.aomhip_status() == 0


def test_block_error_batched_on_resident_blocks(hip, oracle, ctx):
    rng = np.random.default_rng(37)
    nb = 1000
    for n in (16, 24, 32, 48, 64, 256, 1000, 4096):
        span = int(rng.choice([200, 1 << 16, 1 << 19]))
        c = rng.integers(-span, span, nb * n).astype(np.int32)
        d = (c + rng.integers(-span // 8 - 1, span // 8 + 1, nb * n)).astype(np.int32)
        c[:n] = 1 << 17; d[:n] = -(1 << 17)      # block 0 overflows the 32-bit products
        dc, dd, do = ctx.to_device(c), ctx.to_device(d), ctx.malloc(nb * 16)
        for is_hbd, bd in ((0, 8), (1, 8), (1, 10), (1, 12)):
            ctx.block_error_batch(dc, dd, n, nb, is_hbd, bd, do)
            got = ctx.from_device(do, (nb, 2), np.int64)
            for i in range(nb):
                want = orc_block_error(oracle, c[i * n:(i + 1) * n], d[i * n:(i + 1) * n], bd if is_hbd else 0)
                assert (int(got[i, 0]), int(got[i, 1])) == want, (n, is_hbd, bd, i)
        c16, d16 = np.clip(c, -32768, 32767).astype(np.int16), np.clip(d, -32768, 32767).astype(np.int16)
        dc16, dd16 = ctx.to_device(c16), ctx.to_device(d16)
        ctx.block_error_lp_batch(dc16, dd16, n, nb, do)
        got = ctx.from_device(do, (nb,), np.int64)
        for i in range(nb):
            assert int(got[i]) == orc_block_error_lp(oracle, c16[i * n:(i + 1) * n], d16[i * n:(i + 1) * n]), (n, i)
        for ptr in (dc, dd, do, dc16, dd16):
            ctx.free(ptr)
    # arguments are checked
    with pytest.raises(hip.capi.AomHipError):
        ctx.block_error_batch(None, None, 4097, 1, 0, 8, None)


# ---------------------------------------------------------------- round_shift_array, CDEF copies

def round_shift_np(a, bit):
    v = a.astype(np.int64)
    if bit > 0:
        return ((v + (1 << (bit - 1))) >> bit).astype(np.int32)
    return np.clip(v * (1 << -bit), -(1 << 31), (1 << 31) - 1).astype(np.int32)


def test_round_shift_array(hip):
    lib = hip.capi.lib
    lib.aomhip_status_clear()
    rng = np.random.default_rng(41)
    for size in (1, 17, 300, 4096):
        for bit in range(-4, 9):
            a = rng.integers(-(1 << 31), 1 << 31, size, dtype=np.int64).astype(np.int32)
            a[:min(size, 4)] = [-(1 << 31), (1 << 31) - 1, (1 << 28) + 5, -(1 << 28) - 5][:min(size, 4)]   # saturate at INT32_MIN / MAX
            got = a.copy()
            lib.aomhip_round_shift_array(P(got), C.c_int(size), C.c_int(bit))
            assert np.array_equal(got, a if bit == 0 else round_shift_np(a, bit)), (size, bit)
    assert lib.aomhip_status() == 0


def test_cdef_copy_rect8(hip):
    lib = hip.capi.lib
    lib.aomhip_status_clear()
    rng = np.random.default_rng(43)
    for width, height, sstride, dstride in ((7, 5, 9, 11), (13, 11, 13, 21), (72, 80, 75, 144), (1, 1, 3, 1), (64, 3, 101, 67)):
        for src_t, name in ((np.uint8, "aomhip_cdef_copy_rect8_8bit_to_16bit"), (np.uint16, "aomhip_cdef_copy_rect8_16bit_to_16bit")):
            src = rng.integers(0, 256 if src_t == np.uint8 else 4096, (height, sstride)).astype(src_t)
            dst = np.full((height, dstride), 0xBEEF, np.uint16)
            getattr(lib, name)(P(dst), C.c_int(dstride), P(src), C.c_int(sstride), C.c_int(width), C.c_int(height))
            want = np.full((height, dstride), 0xBEEF, np.uint16)
            want[:, :width] = src[:, :width]
            assert np.array_equal(dst, want), (name, width, height)
    assert lib.aomhip_status() == 0


# ---------------------------------------------------------------- installer, failure handling

SLOTS = (["aomhip_inv_txfm_add", "aomhip_highbd_inv_txfm_add"] + ["aomhip_highbd_inv_txfm_add_%dx%d" % wh for wh in TX] +
         ["aomhip_highbd_iwht4x4_1_add", "aomhip_highbd_iwht4x4_16_add", "aomhip_lowbd_fwd_txfm", "aomhip_fwht4x4", "aomhip_round_shift_array",
          "aomhip_block_error", "aomhip_block_error_lp", "aomhip_highbd_block_error", "aomhip_quantize_fp", "aomhip_quantize_fp_32x32",
          "aomhip_quantize_fp_64x64", "aomhip_highbd_quantize_fp", "aomhip_quantize_lp", "aomhip_cdef_copy_rect8_8bit_to_16bit",
          "aomhip_cdef_copy_rect8_16bit_to_16bit"])


def test_installer_table(hip, oracle):
    lib = hip.capi.lib
    assert len(SLOTS) == 36
    table = (C.c_void_p * 36)()
    assert lib.aomhip_rtcd_av1(table) == 0
    assert all(table[i] for i in range(36))
    assert [table[i] for i in range(36)] == [C.cast(getattr(lib, n), C.c_void_p).value for n in SLOTS]
    # one call through a table pointer: block_error (slot 28)
    fn = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_void_p, C.c_ssize_t, C.POINTER(C.c_int64))(table[SLOTS.index("aomhip_block_error")])
    rng = np.random.default_rng(47)
    c = rng.integers(-5000, 5000, 256).astype(np.int32)
    d = (c + rng.integers(-300, 300, 256)).astype(np.int32)
    ssz = C.c_int64()
    assert (fn(c.ctypes.data, d.ctypes.data, 256, C.byref(ssz)), ssz.value) == orc_block_error(oracle, c, d, 0)
    # and an inverse transform through the per-size slot of TX_16X8 (index 8)
    inv = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)(table[2 + 8])
    co = rng.integers(-2000, 2000, 128).astype(np.int32)
    dst = rng.integers(0, 1024, (8, 16)).astype(np.uint16)
    want = inv_oracle(oracle, co, dst, 8, 3, 10)
    p = param(8, 3, 10)
    inv(co.ctypes.data, dst.ctypes.data >> 1, 16, C.addressof(p))
    assert np.array_equal(dst, want)


def test_invalid_txfm_param_sets_sticky_status(hip):
    lib = hip.capi.lib
    lib.aomhip_status_clear()
    rng = np.random.default_rng(53)
    dst = rng.integers(0, 1024, (8, 8)).astype(np.uint16)
    co = rng.integers(-100, 100, 64).astype(np.int32)
    # tx_size 19: nothing is written, the message names the value
    keep = dst.copy()
    lib.aomhip_highbd_inv_txfm_add(P(co), HB(dst), C.c_int(8), C.byref(param(19, 0, 10)))
    assert lib.aomhip_status() == 2 and b"tx_size 19" in lib.aomhip_last_error()
    assert np.array_equal(dst, keep)
    lib.aomhip_status_clear()
    # lossless with 8x8: pixels untouched; the forward transform's 64 coefficients zeroed
    lib.aomhip_highbd_inv_txfm_add(P(co), HB(dst), C.c_int(8), C.byref(param(1, 0, 10, lossless=1, eob=5)))
    assert lib.aomhip_status() == 2 and b"lossless with tx_size 1" in lib.aomhip_last_error()
    assert np.array_equal(dst, keep)
    lib.aomhip_status_clear()
    res = rng.integers(-50, 50, (8, 8)).astype(np.int16)
    out = np.full(64, 9, np.int32)
    lib.aomhip_lowbd_fwd_txfm(P(res), P(out), C.c_int(8), C.byref(param(1, 0, 8, lossless=1)))
    assert lib.aomhip_status() == 2 and b"lossless" in lib.aomhip_last_error() and not out.any()
    lib.aomhip_status_clear()
    # the 8-bit entry takes bd 8 only; a 64-point size takes DCT_DCT only
    d8 = rng.integers(0, 256, (4, 4)).astype(np.uint8)
    k8 = d8.copy()
    lib.aomhip_inv_txfm_add(P(co), P(d8), C.c_int(4), C.byref(param(0, 0, 10)))
    assert lib.aomhip_status() == 2 and b"bit depth 10" in lib.aomhip_last_error() and np.array_equal(d8, k8)
    lib.aomhip_status_clear()
    big = np.zeros((64, 64), np.uint16)
    lib.aomhip_highbd_inv_txfm_add_64x64(P(np.zeros(1024, np.int32)), HB(big), C.c_int(64), C.byref(param(4, 9, 10)))
    assert lib.aomhip_status() == 2 and b"tx_type 9" in lib.aomhip_last_error()
    lib.aomhip_status_clear()
    # a block error out of range returns the losing distortion, never 0
    ssz = C.c_int64()
    assert lib.aomhip_block_error(P(co), P(co), C.c_ssize_t(0), C.byref(ssz)) == 1 << 50 and ssz.value == 1 << 50
    assert lib.aomhip_status() == 2 and b"block_size 0" in lib.aomhip_last_error()
    lib.aomhip_status_clear()
    assert lib.aomhip_status() == 0
