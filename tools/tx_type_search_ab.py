"""A/B of the transform-type search for a frame of 16x16 luma transform blocks, all 16 types allowed: the one device call
(aomhip_search_tx_type_batch) against the type-by-type composition of the entry points that existed before it, on the same seeded frames, in one process:

    python tools/tx_type_search_ab.py [--reps 5] [--out profiles/tx_type_search_ab.json]       (AOMHIP_LIB selects the library)

Points: 1920x1080 8-bit and 3840x2160 10-bit, each in both distortion modes (use_transform_domain_distortion 0: an inverse transform and a pixel SSE per
type; 2: the transform-domain error).
  (a) the new call: wall clock with the context synchronised, and its device time between two events (table + walk; no coefficients requested)
  (b) the composition, per type: aomhip_subtract_xform_quant_ex_batch (with the block error), aomhip_cost_coeffs_txb_batch,
      aomhip_txb_entropy_context_batch and -- mode 0 -- a device copy of the predictor, aomhip_inv_txfm_add_batch and aomhip_sse_batch; then the download
      of rate, eob, context and distortion, the comparison on the host (numpy over all blocks) and, after the last type, the upload of the winners.  Wall
      clock for all of it; the predictor copies are reported on their own.
  (c) the composition's DEVICE SHARE alone: the same launches between two events per type, no downloads, no host work, the predictor copy left out.
Timing follows the measuring guide: >= 0.25 s of warm-up rounds that keep the device busy, then medians of `reps` alternating repetitions; the spread
(max - min over the repetitions) is reported with every figure.  Both sides must choose the same type with the same rd for every block or the tool fails."""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
pkg = importlib.import_module("aom-av1-psy_amd")
capi = pkg.capi

TX_16X16, NC = 2, 256


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return dict(min_ms=float(a[0]), median_ms=float(np.median(a)), max_ms=float(a[-1]), spread_ms=float(a[-1] - a[0]), n=len(a))


def content(rng, W, H, bd):
    mx = (1 << bd) - 1
    i, j = np.indices((H, W))
    pred = np.clip(mx // 2 + (np.sin(i / 9.0) * np.cos(j / 13.0) * (mx // 4)).astype(np.int64), 0, mx)
    amp = np.kron(rng.choice([0, 1, 3, 9, 24], (H // 16 + 1, W // 16 + 1)), np.ones((16, 16), np.int64))[:H, :W] * (mx // 255 + 1)
    src = np.clip(pred + rng.integers(-1, 2, (H, W)) * amp + ((i * 3 + j) % 7) * (amp // 4), 0, mx)
    return src, pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx_type_search_ab.json"))
    ap.add_argument("--points", default="1920x1080x8,3840x2160x10")
    ap.add_argument("--only-new", action="store_true", help="run the new call alone (for a kernel trace)")
    args = ap.parse_args()
    import pyoracle as orc
    hiprt = ctypes.CDLL("libamdhip64.so")
    ctx = capi.Context(0)
    B = 16
    rows_out = []
    for point in args.points.split(","):
        W, H, bd = (int(v) for v in point.split("x"))
        rng = np.random.default_rng(W + bd)
        cols, rows = W // 16, H // 16
        n = cols * rows
        ps, pp, pr = (ctx.planes_alloc(W, H, B, bd, 1) for _ in range(3))
        src, pred = content(rng, W, H, bd)
        ctx.planes_upload(ps, 0, src); ctx.planes_upload(pp, 0, pred)
        plane_bytes = pp.frame_stride * (1 if bd == 8 else 2)
        q = orc.build_quantizer_y(bd, 120)
        qp = capi.QuantParams.from_tables(q)
        costs = rng.integers(10, 4000, 966).astype(np.int32)
        tx_type_costs = rng.integers(0, 1200, 16).astype(np.int64)
        d_costs = ctx.to_device(costs)
        blocks = np.zeros(n, capi.tx_search_block_dtype)
        blocks["x"], blocks["y"] = (np.arange(n) % cols) * 16, (np.arange(n) // cols) * 16
        blocks["ref_best_rd"], blocks["rdmult"], blocks["out_offset"] = (1 << 63) - 1, rng.integers(80, 900, n), np.arange(n) * NC
        blocks["allowed_tx_mask"], blocks["visible_cols"], blocks["visible_rows"] = 0xFFFF, 16, 16
        blocks["txb_skip_ctx"], blocks["dc_sign_ctx"] = rng.integers(0, 13, n), rng.integers(0, 3, n)
        rdmult = blocks["rdmult"].astype(np.int64)
        d_blocks, d_res = ctx.to_device(blocks), ctx.malloc(40 * n)
        cands = np.zeros(n, capi.sad_cand_dtype)
        cands["sx"], cands["sy"], cands["rx"], cands["ry"] = blocks["x"], blocks["y"], blocks["x"], blocks["y"]
        d_cands = ctx.to_device(cands)
        d_tctx = ctx.to_device(np.stack([blocks["txb_skip_ctx"], blocks["dc_sign_ctx"]], 1).astype(np.uint8))
        txbs = []
        for t in range(16):
            txb = np.zeros(n, capi.txb_dtype)
            txb["x"], txb["y"], txb["out_offset"], txb["tx_type"] = blocks["x"], blocks["y"], np.arange(n) * NC, t
            txbs.append(ctx.to_device(txb))
        d_win = ctx.malloc(n * capi.txb_dtype.itemsize)
        d_q, d_dq, d_eob, d_err = ctx.malloc(4 * n * NC), ctx.malloc(4 * n * NC), ctx.malloc(2 * n), ctx.malloc(16 * n)
        d_cost, d_ectx, d_sse, d_sse0 = ctx.malloc(4 * n), ctx.malloc(n), ctx.malloc(8 * n), ctx.malloc(8 * n)
        rnd = (bd - 8) * 2

        def rounded(v):
            return (v + ((1 << rnd) >> 1)) >> rnd if rnd else v

        for mode in (0, 2):
            prm = capi.TxSearchParams.make(tx_type_costs=tx_type_costs, use_transform_domain_distortion=mode)

            def one_call():
                ctx.search_tx_type_batch(ps, pp, 0, TX_16X16, qp, d_costs, prm, d_blocks, n, d_res)

            def launches(t):
                ctx.subtract_xform_quant_ex_batch(ps, pp, 0, TX_16X16, txbs[t], n, 0, 0, qp, 0, None, d_q, d_dq, d_eob, d_err)
                ctx.cost_coeffs_txb_batch(d_q, TX_16X16, txbs[t], n, 0, d_eob, d_tctx, d_costs, d_cost)
                ctx.txb_entropy_context_batch(d_q, TX_16X16, txbs[t], n, 0, d_eob, d_ectx)
                if mode == 0:
                    ctx.inv_txfm_add_batch(d_dq, TX_16X16, txbs[t], n, 0, 0, d_eob, pr, 0)
                    ctx.sse_batch(ps, pr, 0, 16, 16, d_cands, n, d_sse)

            def copy_pred():
                t0 = time.perf_counter()
                assert hiprt.hipMemcpy(ctypes.c_void_p(pr.base), ctypes.c_void_p(pp.base), ctypes.c_size_t(plane_bytes), 3) == 0   # device to device
                return time.perf_counter() - t0

            def composition():
                """-> (winner types, their rd, seconds spent in the predictor copies)"""
                copies = 0.0
                ctx.sse_batch(ps, pp, 0, 16, 16, d_cands, n, d_sse0)
                ctx.sync()
                block_sse = rounded(ctx.from_device(d_sse0, (n,), np.int64)) * 16
                high = block_sse >= 128 * 128 * 256
                best_rd, best_t = np.full(n, (1 << 63) - 1, np.int64), np.zeros(n, np.int64)
                for t in range(16):
                    if mode == 0:
                        ctx.sync()
                        copies += copy_pred()
                    launches(t)
                    ctx.sync()
                    eob, err = ctx.from_device(d_eob, (n,), np.uint16), ctx.from_device(d_err, (n, 2), np.int64)
                    cost, _ectx = ctx.from_device(d_cost, (n,), np.int32).astype(np.int64), ctx.from_device(d_ectx, (n,), np.uint8)
                    rate = cost + np.where(eob > 0, tx_type_costs[t], 0)
                    td = err[:, 0] >> 2                                       # dist_block_tx_domain: RIGHT_SIGNED_SHIFT by (MAX_TX_SCALE - av1_get_tx_scale) * 2 = 2 for 16x16
                    if mode == 0:
                        px = rounded(ctx.from_device(d_sse, (n,), np.int64)) * 16
                        dist = np.where(high & (px < td), td, px)
                    else:
                        dist = td
                    dist = np.where(eob == 0, block_sse, dist)
                    rd = ((rate * rdmult + 256) >> 9) + dist * 128
                    better = rd < best_rd
                    best_rd, best_t = np.where(better, rd, best_rd), np.where(better, t, best_t)
                win = np.zeros(n, capi.txb_dtype)
                win["x"], win["y"], win["out_offset"], win["tx_type"] = blocks["x"], blocks["y"], np.arange(n) * NC, best_t
                ctx.memcpy_h2d(d_win, win)
                ctx.sync()
                return best_t, best_rd, copies

            t0 = time.perf_counter()                         # warm-up: kernels loaded, work memory sized, the clocks up
            while time.perf_counter() - t0 < 0.25:
                one_call(); ctx.sync()
            new_ms, new_dev_ms, seq_ms, seq_dev_ms, copy_ms, per_kernel = [], [], [], [], [], []
            for rep in range(args.reps):
                ctx.sync()
                t0 = time.perf_counter()
                one_call()
                ctx.sync()
                new_ms.append((time.perf_counter() - t0) * 1e3)
                ctx.timer_begin()
                one_call()
                new_dev_ms.append(ctx.timer_end())
                res = ctx.from_device(d_res, (n,), capi.tx_search_result_dtype)
                if args.only_new:
                    continue
                t0 = time.perf_counter()
                best_t, best_rd, copies = composition()
                seq_ms.append((time.perf_counter() - t0) * 1e3)
                copy_ms.append(copies * 1e3)
                if not (np.array_equal(res["best_tx_type"], best_t) and np.array_equal(res["best_rd"], best_rd)):
                    raise SystemExit("the call and the composition differ at %s mode %d" % (point, mode))
                dev = 0.0
                for t in range(16):
                    if mode == 0:
                        ctx.sync(); copy_pred()
                    ctx.timer_begin()
                    launches(t)
                    dev += ctx.timer_end()
                seq_dev_ms.append(dev)
            row = dict(width=W, height=H, bit_depth=bd, tx_size="TX_16X16", blocks=n, types=16, use_transform_domain_distortion=mode, new_wall=stats(new_ms),
                       new_device=stats(new_dev_ms))
            if not args.only_new:
                row.update(identical=True, winners_not_dct=int((res["best_tx_type"] != 0).sum()), composition_wall=stats(seq_ms), composition_device_share=stats(seq_dev_ms),
                           composition_pred_copies=stats(copy_ms))
                row["factor_wall"] = row["composition_wall"]["median_ms"] / row["new_wall"]["median_ms"]
                row["factor_device_share"] = row["composition_device_share"]["median_ms"] / row["new_device"]["median_ms"]
                row["margin_ms"] = max(row["new_device"]["spread_ms"], row["composition_device_share"]["spread_ms"])
                row["new_within_device_share"] = bool(row["new_device"]["median_ms"] <= row["composition_device_share"]["median_ms"] + row["margin_ms"])
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        for d in [d_costs, d_blocks, d_res, d_cands, d_tctx, d_win, d_q, d_dq, d_eob, d_err, d_cost, d_ectx, d_sse, d_sse0] + txbs:
            ctx.free(d)
        for p in (ps, pp, pr):
            ctx.planes_free(p)
    if not args.only_new:
        rec = dict(tool="tools/tx_type_search_ab.py", timing="wall clock around synchronised calls and event pairs around launches, the call and the composition "
                   "alternating, after >= 0.25 s of warm-up rounds; the composition's host share is numpy over all blocks", reps=args.reps, rows=rows_out)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
