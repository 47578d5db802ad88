"""The function-pointer table (aomhip_bind_variance_vtable, csrc/vtable.cpp) against the reference ITSELF, compiled as C
(oracle/_ref/libaomref_c.so, tests/refc.py): every member x the 22 block sizes x 8 / 10 / 12 bit is called THROUGH the bound pointer,
next to the symbol the encoder installs in that slot, on one random and one saturated block, with the same host buffers; return
values and buffers (guards included) must be equal.

The slot's reference counterpart (av1/encoder/encoder.c BFP / encoder_utils.h HIGHBD_BFP_WRAPPER, HIGHBD_MBFP_WRAPPER,
HIGHBD_OBFP_WRAPPER, HIGHBD_SDSFP_WRAPPER):
  8 bit           aom_<member form>WxH_c
  10 / 12 bit     the variance forms have symbols of their own, aom_highbd_{10,12}_<form>WxH_c; the SAD forms are aom_highbd_<form>WxH_c
                  behind the encoder's static _bits10 / _bits12 wrappers, which shift the result (every entry of an x4d array) right
                  by 2 / 4.  Those wrappers are `static` in encoder_utils.h, so the shift is applied here (ShiftedSad)."""
import ctypes as C

import numpy as np
import pytest

import refc
from conftest import BLOCK_SIZES
from refc import Ptr, PtrList
from refc_inputs import FORMS, Jcp
from test_vtable import FIELDS, _bound

pytestmark = pytest.mark.gpu


class ShiftedSad:
    """fnname##_bits10 / _bits12 of encoder_utils.h: the highbd SAD form, its result (or its four results) shifted right"""

    def __init__(self, f, shift, is_array):
        self.f, self.shift, self.is_array, self.argtypes = f, shift, is_array, None

    def __call__(self, *cargs):
        self.f.argtypes = self.argtypes
        r = self.f(*cargs)
        if not self.is_array:
            return r >> self.shift
        out = (C.c_uint32 * 4).from_address(cargs[-1].value)
        for i in range(4):
            out[i] >>= self.shift
        return r


def reference_member(member, w, h, bd):
    pat, is_sad, is_array = FORMS[member]
    restype = None if is_array else C.c_uint
    if bd == 8:
        return refc.fn("aom_" + pat % (w, h) + "_c", restype)
    if not is_sad:
        return refc.fn("aom_highbd_%d_" % bd + pat % (w, h) + "_c", restype)
    return ShiftedSad(refc.fn("aom_highbd_" + pat % (w, h) + "_c", restype), bd - 8, is_array)


def member_args(member, w, h, bd, rng, saturated):
    """the member's argument list on fresh buffers (aom_dsp/variance.h:29-82); strides differ from the width, origins are offset"""
    hb = bd > 8
    dt, mx = (np.uint16, (1 << bd) - 1) if hb else (np.uint8, 255)
    S, R = w + 3, w + 9
    src = rng.integers(0, mx + 1, (h + 2, S)).astype(dt)
    ref = rng.integers(0, mx + 1, (h + 6, R)).astype(dt)
    second = rng.integers(0, mx + 1, w * h + 8).astype(dt)
    mask = rng.integers(0, 65, (h, w + 2)).astype(np.uint8)
    wsrc = rng.integers(0, mx * 4096 + 1, w * h + 8).astype(np.int32)
    omask = rng.integers(0, 4097, w * h + 8).astype(np.int32)
    if saturated:
        src[:] = mx; ref[:] = 0; second[:] = 0; mask[:] = 64; wsrc[:] = mx * 4096; omask[:] = 4096
    xo, yo = (int(rng.integers(0, 8)), int(rng.integers(0, 8))) if not saturated else (4, 4)
    sp, rp = Ptr(src, 1, hb), Ptr(ref, 2 * R + 3, hb)
    sse = lambda: np.full(2, 0xDEAD, np.uint32)
    four = lambda: (PtrList([rp, Ptr(ref, 2 * R + 4, hb), Ptr(ref, 3 * R + 3, hb), Ptr(ref, 4 * R + 7, hb)]), R, np.full(5, 0xDEAD, np.uint32))
    jcp = Jcp(1, *[(9, 7), (11, 5), (12, 4), (13, 3), (7, 9), (4, 12)][int(rng.integers(0, 6))])
    sec = Ptr(second, 0, hb)
    return {
        "sdf": lambda: [sp, S, rp, R], "sdsf": lambda: [sp, S, rp, R], "sdaf": lambda: [sp, S, rp, R, sec],
        "vf": lambda: [sp, S, rp, R, sse()], "svf": lambda: [rp, R, xo, yo, sp, S, sse()], "svaf": lambda: [rp, R, xo, yo, sp, S, sse(), sec],
        "sdx4df": lambda: [sp, S, *four()], "sdx3df": lambda: [sp, S, *four()], "sdsx4df": lambda: [sp, S, *four()],
        "msdf": lambda: [sp, S, rp, R, sec, mask, w + 2, int(rng.integers(0, 2))],
        "msvf": lambda: [rp, R, xo, yo, sp, S, sec, mask, w + 2, int(rng.integers(0, 2)), sse()],
        "osdf": lambda: [rp, R, wsrc, omask], "ovf": lambda: [rp, R, wsrc, omask, sse()], "osvf": lambda: [rp, R, xo, yo, wsrc, omask, sse()],
        "jsdaf": lambda: [sp, S, rp, R, sec, jcp], "jsvaf": lambda: [rp, R, xo, yo, sp, S, sse(), sec, jcp],
    }[member]()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_every_member_and_size_through_the_table(hip, ctx, bd):
    refc.lib()
    assert set(FORMS) == set(FIELDS)
    tbl = _bound(hip, bd)
    rng = np.random.default_rng(60 + bd)
    calls = 0
    for member in FIELDS:
        is_array = FORMS[member][2]
        for i, (w, h) in enumerate(BLOCK_SIZES):
            bound = C.CFUNCTYPE(None if is_array else C.c_uint)(getattr(tbl[i], member))
            ref = reference_member(member, w, h, bd)
            for saturated in (False, True):
                args = member_args(member, w, h, bd, rng, saturated)
                r, bufs, wrote = refc.run_pair(bound, ref, args, (member, w, h, bd, "saturated" if saturated else "random"))
                assert wrote or r, (member, w, h, bd)     # the reference did compute something
                calls += 1
    assert calls == 16 * 22 * 2
    assert hip.capi.lib.aomhip_status() == 0, hip.capi.lib.aomhip_last_error()
    print("vtable %d-bit: %d calls through %d pointers" % (bd, calls, 16 * 22))
