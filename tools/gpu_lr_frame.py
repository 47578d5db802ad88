"""Timing of the stripe-exact loop-restoration frame filter (aomhip_loop_restoration_filter_units) against the unit-batch calls it does not replace
(aomhip_wiener_convolve_add_src_batch, aomhip_apply_selfguided_restoration_batch) on the SAME unit list, in one process:

    python tools/gpu_lr_frame.py [--reps 25] [--out profiles/lr_frame.json]       (AOMHIP_LIB selects the library)

Planes: 3840x2160 10-bit luma and 1920x1080 8-bit luma; unit sizes 64 and 256; cases: all-Wiener, all-SGR with both radii, and the mix of the
three types the tests use.  Every repetition is timed on its own with device events (aomhip_timer_begin / _end) after a warm-up, the new call and
the existing call(s) ALTERNATE, and the record holds min / quartiles / max of each, so that a difference can be read against the run-to-run spread.
The unit-batch calls read CDEF-only context (they are not stripe-exact): the comparison is one of cost, not of output.  For the mix the existing
side is the Wiener call on the Wiener units plus the self-guided call on the SGR units (there is no existing copy call for RESTORE_NONE units).
Also recorded: the bytes the new call cannot avoid (one read of `cdef`, one write of `dst`, four deblocked rows per internal stripe boundary) and
the rate they give at the median time."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
pkg = importlib.import_module("aom-av1-psy_amd")
capi = pkg.capi

HBM_PEAK = 8.0e12      # bytes / s (MI355X data sheet)


def quartiles(ms):
    a = np.sort(np.asarray(ms, np.float64)) * 1e3
    return dict(min_us=float(a[0]), p25_us=float(np.percentile(a, 25)), median_us=float(np.median(a)), p75_us=float(np.percentile(a, 75)),
                max_us=float(a[-1]), n=len(a))


def timed(ctx, fn):
    ctx.timer_begin()
    fn()
    return ctx.timer_end()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_frame.json"))
    args = ap.parse_args()
    assert args.reps >= 20
    ctx = capi.Context(0)
    B = 16
    rows = []
    for (W, H, bd) in ((3840, 2160, 10), (1920, 1080, 8)):
        es = 2 if bd > 8 else 1
        deb, cdef = pkg.synth.lcg_frame(W, H, 3, 0, bd), pkg.synth.lcg_frame(W, H, 4, 0, bd)
        pe, pc, pd = (ctx.planes_alloc(W, H, B, bd, 1) for _ in range(3))
        ctx.planes_upload(pe, 0, deb); ctx.planes_upload(pc, 0, cdef); ctx.planes_upload(pd, 0, np.zeros_like(cdef))
        n_bound = len(range(56, H, 64))
        compulsory = (2 * W * H + 4 * n_bound * W) * es
        for U in (64, 256):
            units = capi.lr_units_in_plane(W, H, U, 0)
            n = len(units)
            mw, mh = int((units["h_end"] - units["h_start"]).max()), int((units["v_end"] - units["v_start"]).max())
            d_f0, d_f1 = ctx.malloc(4 * n * mw * mh), ctx.malloc(4 * n * mw * mh)
            for case in ("wiener", "sgr", "mix"):
                types = {"wiener": np.ones(n, np.int32), "sgr": np.full(n, 2, np.int32), "mix": (np.arange(n) % 3 + 1) % 3}[case].astype(np.int32)
                info = np.zeros(n, capi.lr_unit_info_dtype)
                info["restoration_type"] = types
                info["sgr_params_idx"] = 3 if case != "mix" else (np.arange(n) * 5 + 2) % 16      # set 3: both radii
                info["xqd"] = (-30, 40)
                info["hfilter"] = info["vfilter"] = (3, -7, 15, -22, 15, -7, 3, 0)
                d_u, d_i = ctx.to_device(units), ctx.to_device(info)
                new = lambda: ctx.loop_restoration_filter_units(pe, 0, pc, 0, pd, 0, W, H, 0, d_u, units, n, d_i)      # noqa: E731
                old_calls, keep = [], [d_u, d_i]
                wsel, ssel = np.flatnonzero(types == 1), np.flatnonzero(types == 2)
                if len(wsel):
                    uw = np.ascontiguousarray(units[wsel])
                    filt = np.tile(np.array([3, -7, 15, -22, 15, -7, 3, 0] * 2, np.int16), (len(uw), 1))
                    d_uw, d_fw = ctx.to_device(uw), ctx.to_device(filt)
                    keep += [d_uw, d_fw]
                    old_calls.append(lambda uw=uw, d_uw=d_uw, d_fw=d_fw: ctx.wiener_convolve_add_src_batch(pc, 0, pd, 0, d_uw, uw, len(uw), d_fw, mw, mh))
                if len(ssel):
                    us = np.ascontiguousarray(units[ssel])
                    d_us = ctx.to_device(us)
                    d_ix = ctx.to_device(np.ascontiguousarray(info["sgr_params_idx"][ssel]).astype(np.int32))
                    d_xq = ctx.to_device(np.ascontiguousarray(info["xqd"][ssel]).astype(np.int32))
                    keep += [d_us, d_ix, d_xq]
                    old_calls.append(lambda us=us, d_us=d_us, d_ix=d_ix, d_xq=d_xq: ctx.apply_selfguided_restoration_batch(
                        pc, 0, pd, 0, d_us, us, len(us), d_ix, d_xq, mw, mh, d_f0, d_f1, mw, mw * mh))
                old = lambda: [f() for f in old_calls]      # noqa: E731
                for _ in range(3):
                    new(); old()
                ctx.sync()
                t_new, t_old = [], []
                for _ in range(args.reps):
                    t_new.append(timed(ctx, new))
                    t_old.append(timed(ctx, old))
                qn, qo = quartiles(t_new), quartiles(t_old)
                rate = compulsory / (qn["median_us"] * 1e-6)
                row = dict(width=W, height=H, bit_depth=bd, unit_size=U, n_units=n, case=case, new=qn, existing=qo,
                           existing_calls=[c for c, s in (("aomhip_wiener_convolve_add_src_batch", wsel), ("aomhip_apply_selfguided_restoration_batch", ssel)) if len(s)],
                           compulsory_bytes=compulsory, measured_compulsory_bytes_per_s=rate, measured_share_of_8TBps=rate / HBM_PEAK)
                rows.append(row)
                print("%4dx%-4d %2d-bit unit %3d %-6s new %8.1f us [%.1f .. %.1f]   existing %8.1f us [%.1f .. %.1f]   %.2f TB/s compulsory (%.1f %% of 8 TB/s, measured)"
                      % (W, H, bd, U, case, qn["median_us"], qn["p25_us"], qn["p75_us"], qo["median_us"], qo["p25_us"], qo["p75_us"], rate / 1e12,
                         100 * rate / HBM_PEAK), flush=True)
                for d in keep:
                    ctx.free(d)
            ctx.free(d_f0); ctx.free(d_f1)
        for p in (pe, pc, pd):
            ctx.planes_free(p)
    rec = dict(tool="tools/gpu_lr_frame.py", timing="device events per repetition, new and existing calls alternating, after 3 warm-up rounds",
               reps=args.reps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
