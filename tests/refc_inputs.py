"""Input makers and ctypes mirrors shared by the tests that compare against the compiled reference (tests/test_refc_*.py on the CPU,
tests/test_gpu_refc_*.py on the GPU).  A plain module: it imports no test file."""
import ctypes as C

import numpy as np

# TX_SIZE order of av1/common/enums.h (w, h) and the coefficients a forward transform returns (64-point sizes: the low 32 x 32)
TX = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (4, 8), (8, 4), (8, 16), (16, 8), (16, 32), (32, 16), (32, 64), (64, 32), (4, 16), (16, 4),
      (8, 32), (32, 8), (16, 64), (64, 16)]
NC = [min(w, 32) * min(h, 32) for w, h in TX]


class TxfmParam(C.Structure):
    """TxfmParam (aom_dsp/txfm_common.h:89-101) = aomhip_txfm_param"""
    _fields_ = [("tx_type", C.c_uint8), ("tx_size", C.c_uint8), ("lossless", C.c_int), ("bd", C.c_int), ("is_hbd", C.c_int),
                ("tx_set_type", C.c_uint8), ("eob", C.c_int)]


def param(tx_size, tx_type, bd, lossless=0, eob=0):
    return TxfmParam(tx_type, tx_size, lossless, bd, int(bd > 8), 0, eob)


class ConvolveParams(C.Structure):
    """ConvolveParams (av1/common/convolve.h:21-32)"""
    _fields_ = [("do_average", C.c_int), ("dst", C.c_void_p), ("dst_stride", C.c_int), ("round_0", C.c_int), ("round_1", C.c_int), ("plane", C.c_int),
                ("is_compound", C.c_int), ("use_dist_wtd_comp_avg", C.c_int), ("fwd_offset", C.c_int), ("bck_offset", C.c_int)]


class SgrParams(C.Structure):
    """sgr_params_type (av1/common/restoration.h): the projection functions read the radii only"""
    _fields_ = [("r", C.c_int * 2), ("s", C.c_int * 2)]


class WarpedMotionParams(C.Structure):
    """WarpedMotionParams (av1/common/mv.h:129-134)"""
    _fields_ = [("wmmat", C.c_int32 * 6), ("alpha", C.c_int16), ("beta", C.c_int16), ("gamma", C.c_int16), ("delta", C.c_int16),
                ("wmtype", C.c_uint8), ("invalid", C.c_int8)]


def fp_tables(q):
    """plausible round_fp / quant_fp rows for a dequantiser (av1_build_quantizer's shape)"""
    dq = q["dequant"].astype(np.int64)
    return {"round": ((dq * 64) >> 7).astype(np.int16), "quant": np.minimum((1 << 16) // dq, 32767).astype(np.int16),
            "dequant": q["dequant"].astype(np.int16), "zbin": q["zbin"].astype(np.int16), "quant_shift": q["quant_shift"].astype(np.int16)}


# member -> (name pattern, is a SAD form (shift wrapper at 10 / 12 bit), fills an array of 4)
FORMS = {"sdf": ("sad%dx%d", 1, 0), "sdsf": ("sad_skip_%dx%d", 1, 0), "sdaf": ("sad%dx%d_avg", 1, 0), "vf": ("variance%dx%d", 0, 0),
         "svf": ("sub_pixel_variance%dx%d", 0, 0), "svaf": ("sub_pixel_avg_variance%dx%d", 0, 0), "sdx4df": ("sad%dx%dx4d", 1, 1),
         "sdx3df": ("sad%dx%dx3d", 1, 1), "sdsx4df": ("sad_skip_%dx%dx4d", 1, 1), "msdf": ("masked_sad%dx%d", 1, 0),
         "msvf": ("masked_sub_pixel_variance%dx%d", 0, 0), "osdf": ("obmc_sad%dx%d", 1, 0), "ovf": ("obmc_variance%dx%d", 0, 0),
         "osvf": ("obmc_sub_pixel_variance%dx%d", 0, 0), "jsdaf": ("dist_wtd_sad%dx%d_avg", 1, 0),
         "jsvaf": ("dist_wtd_sub_pixel_avg_variance%dx%d", 0, 0)}


class Jcp(C.Structure):
    """DIST_WTD_COMP_PARAMS (av1/common/blockd.h)"""
    _fields_ = [("use_dist_wtd_comp_avg", C.c_int), ("fwd_offset", C.c_int), ("bck_offset", C.c_int)]


def coeff_classes(rng, n, sc, dequant_ac, ls, span_hi):
    out = [np.zeros(n, np.int32)]
    dc = np.zeros(n, np.int32); dc[0] = 300; out.append(dc)
    ex = np.zeros(n, np.int32); ex[0] = -8191; out.append(ex)
    out.append(np.full(n, 16, np.int32))
    cb = np.where(np.arange(n) % 2 == 0, span_hi, -span_hi).astype(np.int32); out.append(cb)
    for span in (32, 1024, span_hi):
        out.append(rng.integers(-span, span + 1, n).astype(np.int32))
    lone = np.zeros(n, np.int32); lone[int(sc[min(5, n - 1)])] = int(dequant_ac) // (1 << ls) + 1; out.append(lone)
    return out


def wide(t):
    """quantiser rows as the encoder stores them: 8 entries, DC then AC repeated (av1/encoder/av1_quantize.h QUANTS)"""
    return {k: np.ascontiguousarray(np.concatenate([v[:1], np.repeat(v[1:2], 7)]), np.int16) for k, v in t.items()}


def lpf_patch(rng, bd, kind):
    """32 x 32 pixels around an edge at row / column 16: random, nearly flat (flat / flat2 masks fire), a hard step, or +-max checkerboard"""
    mx = (1 << bd) - 1
    if kind == "flat":
        base = int(rng.integers(8 << (bd - 8), mx - (8 << (bd - 8))))
        p = base + rng.integers(-(1 << (bd - 8)), (1 << (bd - 8)) + 1, (32, 32))
        p[16:] += int(rng.integers(-3, 4)) << (bd - 8)
        p[:, 16:] += int(rng.integers(-3, 4)) << (bd - 8)
    elif kind == "step":
        p = np.zeros((32, 32), np.int64); p[16:, :] = mx; p[:, 16:] = mx - p[:, 16:]
    elif kind == "checker":
        yy, xx = np.mgrid[0:32, 0:32]; p = ((yy + xx) & 1) * mx
    else:
        p = rng.integers(0, mx + 1, (32, 32))
    return np.clip(p, 0, mx).astype(np.uint8 if bd == 8 else np.uint16)


def residual_classes(rng, w, h, stride, bd):
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:stride]
    out = [("random", rng.integers(-mx, mx + 1, (h, stride))), ("zero", np.zeros((h, stride))), ("dc", np.full((h, stride), 37)),
           ("extreme dc", np.full((h, stride), -mx)), ("checker", np.where((yy + xx) & 1, mx, -mx))]
    return [(k, np.ascontiguousarray(v, np.int16)) for k, v in out]


def coeffs_for_inverse(rng, tx_size, bd, kind):
    w, h = TX[tx_size]
    nc = NC[tx_size]
    co = np.zeros(w * h, np.int32)
    if kind == "random":
        co[:nc] = (rng.integers(-(1 << (bd + 3)), 1 << (bd + 3), nc) * (rng.random(nc) < 0.3)).astype(np.int32)
    elif kind == "dc":
        co[0] = int(rng.integers(-(1 << (bd + 3)), 1 << (bd + 3)))
    elif kind == "extreme":   # beyond the input clamp, DC at the range limits
        co[:nc] = rng.integers(-(1 << (bd + 9)), 1 << (bd + 9), nc)
        co[0] = rng.choice([-(1 << (bd + 7)), (1 << (bd + 7)) - 1])
    return co


def pixels(rng, h, stride, bd, kind, dtype):
    if kind == "extreme":
        yy, xx = np.mgrid[0:h, 0:stride]
        return np.ascontiguousarray(((yy + xx) & 1) * ((1 << bd) - 1), dtype)
    return rng.integers(0, 1 << bd, (h, stride)).astype(dtype)


def cdef_fb_reference(plane, pli, xdec, ydec, y0, x0, pw, ph, skip, luma_dir, level, sec, damping, bd):
    """av1_cdef_filter_fb (compiled) on the pw x ph filter block at (y0, x0) of `plane`: the input tile is built with cdef_prepare_fb's
    semantics (available neighbours copied, frame edges CDEF_VERY_LARGE, stride CDEF_BSTRIDE = 144), the cdef_list from the 8 x 8 skip
    map.  -> (filtered block, dir[8][8], var[8][8])"""
    import refc
    BS, VL = 144, 0x4000
    tile = np.full((ph + 6, BS), VL, np.uint16)
    for r in range(-2, ph + 2):
        ys = y0 + r
        if 0 <= ys < plane.shape[0]:
            xs0, xs1 = max(x0 - 8, 0), min(x0 + pw + 8, plane.shape[1])
            tile[r + 2, 8 + (xs0 - x0):8 + (xs1 - x0)] = plane[ys, xs0:xs1]
    dl = [(by, bx) for by in range(8) for bx in range(8) if not skip[by, bx]]
    dlist = np.ascontiguousarray(np.asarray(dl, np.uint8).reshape(-1, 2))       # cdef_list { uint8_t by, bx; }
    dirs, var = np.zeros((16, 16), np.int32), np.zeros((16, 16), np.int32)
    if pli:
        dirs[:8, :8] = luma_dir
    use8 = bd == 8
    dst = np.ascontiguousarray(plane[y0:y0 + ph, x0:x0 + pw].astype(np.uint8 if use8 else np.uint16))
    refc.call(refc.fn("av1_cdef_filter_fb"), dst if use8 else None, None if use8 else dst, pw, refc.Ptr(tile, 2 * BS + 8), xdec, ydec, dirs, None, var, pli,
              dlist, len(dl), level, sec, damping, bd - 8)
    return dst, dirs[:8, :8].copy(), var[:8, :8].copy()
