"""A/B of av1_pick_filter_level's search (LPF_PICK_FROM_FULL_IMAGE) for a frame: the one device call (aomhip_pick_filter_level_frame) against the
host-driven search over the entry points that existed before it, on the same seeded frames, in one process:

    python tools/lpf_pick_ab.py [--reps 5] [--out profiles/lpf_pick_ab.json]       (AOMHIP_LIB selects the library)

Frames: 1920x1080 8-bit and 3840x2160 10-bit 4:2:0 with a random transform partition, reference and mode deltas on.
  (a) the new call, wall clock with the context synchronised; its split: the five table launches alone (aomhip_lpf_level_sse_table, each synchronised
      on its own), the rest being the five walks and the three producers
  (b) the host-driven search: tests/lpf_pick_model.py's walk, and per trial aomhip_lf_level_table + the per-unit levels (numpy) +
      aomhip_lf_build_edge_params (C) -- the HOST share -- then upload + aomhip_lpf_search_sse + synchronise + download of one number -- the DEVICE
      share; the final producer pass per plane and its upload are counted too.  The trial count is reported.
  (c) the luma table launch divided by its 64 levels, beside one aomhip_lpf_search_sse trial on records already in device memory (lpf_search_trial)
Timing follows the measuring guide: >= 0.25 s of warm-up rounds that keep the device busy, then medians of `reps` alternating repetitions.  Both sides
must choose the same four levels and produce the same edge-parameter planes or the tool fails."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("aom-av1-psy_amd")
capi = pkg.capi
import lpf_pick_model as M  # noqa: E402  (the pinned host walk)

VP = ctypes.c_void_p


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return dict(min_ms=float(a[0]), median_ms=float(np.median(a)), max_ms=float(a[-1]), spread_ms=float(a[-1] - a[0]), n=len(a))


def content(rng, W, H, bd):
    mx = (1 << bd) - 1
    i, j = np.indices((H, W))
    src = np.clip(mx // 2 + (np.sin(i / 9.0) * np.cos(j / 13.0) * (mx // 4)).astype(np.int64) + rng.integers(-2, 3, (H, W)) * (mx // 255 + 1), 0, mx)
    rec = np.clip(0.5 * src + 0.5 * np.kron(src[::8, ::8], np.ones((8, 8), np.int64))[:H, :W] + rng.integers(-3, 4, (H, W)) * (mx // 255 + 1), 0, mx)
    dt = np.uint8 if bd == 8 else np.uint16
    return rec.astype(dt), src.astype(dt)


def partition(rng, w, h, max_log2):
    """search units of a plane with a random square transform partition (4 .. 1 << max_log2 pixels), random skip / reference / mode"""
    rows, cols = (h + 3) // 4, (w + 3) // 4
    u = np.zeros((rows, cols), capi.lf_search_unit_dtype)
    step = (1 << max_log2) // 4
    for y in range(0, rows, step):
        for x in range(0, cols, step):
            def split(y0, x0, n):
                if n > 1 and rng.random() < 0.55:
                    for dy in (0, n // 2):
                        for dx in (0, n // 2):
                            split(y0 + dy, x0 + dx, n // 2)
                    return
                blk = u[y0:y0 + n, x0:x0 + n]
                blk["tx_size"] = int(np.log2(n))
                blk["pb_w_log2"] = blk["pb_h_log2"] = int(np.log2(n)) + 2
                blk["skip_inter"] = int(rng.random() < 0.3)
                ref = int(rng.integers(0, 8))
                blk["ref_mode"] = ref | ((int(rng.integers(0, 2)) if ref else 0) << 3)
            split(y, x, step)
    return np.ascontiguousarray(u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpf_pick_ab.json"))
    ap.add_argument("--points", default="1920x1080x8,3840x2160x10")
    ap.add_argument("--only-new", action="store_true", help="run the new call alone (for a kernel trace)")
    args = ap.parse_args()
    ctx = capi.Context(0)
    lib = capi.lib
    B, last, max_level = 16, [20, 28, 10, 40], 63
    rows_out = []
    for point in args.points.split(","):
        W, H, bd = (int(v) for v in point.split("x"))
        rng = np.random.default_rng(W + bd)
        dims = [(W, H), (W // 2, H // 2), (W // 2, H // 2)]
        pr = [ctx.planes_alloc(w, h, B, bd, 2) for w, h in dims]          # frame 1: the trial's scratch copy
        ps = [ctx.planes_alloc(w, h, B, bd, 1) for w, h in dims]
        for p, (w, h) in enumerate(dims):
            r, s = content(rng, w, h, bd)
            ctx.planes_upload(pr[p], 0, r); ctx.planes_upload(ps[p], 0, s)
        units = [partition(rng, w, h, 6 if p == 0 else 5) for p, (w, h) in enumerate(dims)]
        ustride = [u.shape[1] for u in units]
        d_units = [ctx.to_device(u) for u in units]
        d_edges = [ctx.malloc(4 * u.size) for u in units]
        d_host_edges = [ctx.malloc(4 * u.size) for u in units]
        d_levels, d_tables, d_traces, d_sse, d_t = ctx.malloc(16), ctx.malloc(8 * 5 * 64), ctx.malloc(4 * 5 * capi.LPF_TRACE_INTS), ctx.malloc(8), ctx.malloc(8 * 64)
        fp = capi.LfFrameParams()
        fp.mode_ref_delta_enabled = 1
        for i, v in enumerate((1, 0, 0, 0, -1, 0, -1, -1)):
            fp.ref_deltas[i] = v
        fp.mode_deltas[0], fp.mode_deltas[1] = 0, 1
        mi_rows = (H + 3) // 4

        def one_call():
            ctx.pick_filter_level_frame(pr, 0, ps, 0, 1, 1, d_units, ustride, fp, 0, M.FULL_IMAGE, max_level, mi_rows, last, d_levels, d_edge_params=d_edges,
                                        edge_stride=ustride, d_tables=d_tables, d_traces=d_traces)

        def host_params(plane, levels):
            """the integrator's work for one setting of cm->lf: level table, per-unit levels, set_lpf_parameters -> uint8 [rows, cols, 4]"""
            fp.filter_level[0], fp.filter_level[1], fp.filter_level_u, fp.filter_level_v = levels
            u = units[plane]
            out = np.zeros(u.shape + (4,), np.uint8)
            if not ((levels[0] or levels[1]) if plane == 0 else levels[1 + plane]):
                return out
            tab = np.zeros((8, 2, 8, 2), np.uint8)
            lib.aomhip_lf_level_table(ctypes.byref(fp), ctypes.c_int(plane), VP(tab.ctypes.data))
            ref, mode = u["ref_mode"] & 7, u["ref_mode"] >> 3
            hu = np.zeros(u.shape + (6,), np.uint8)
            for k, nm in enumerate(("tx_size", "skip_inter", "pb_w_log2", "pb_h_log2")):
                hu[..., k] = u[nm]
            hu[..., 4], hu[..., 5] = tab[u["segment_id"], 0, ref, mode], tab[u["segment_id"], 1, ref, mode]
            w, h = dims[plane]
            assert lib.aomhip_lf_build_edge_params(VP(hu.ctypes.data), ctypes.c_int(u.shape[1]), ctypes.c_int(w), ctypes.c_int(h), ctypes.c_int(plane > 0),
                                                   VP(out.ctypes.data), ctypes.c_int(u.shape[1])) == 0
            return out

        clock = dict(host=0.0, device=0.0, trials=0)

        def host_search():
            lv = [0, 0, 0, 0]

            def table_of(plane, d, fixed):
                def get(level):
                    t0 = time.perf_counter()
                    trial = list(lv)
                    if plane == 0:
                        trial[0], trial[1] = (level if d != 1 else fixed), (level if d != 0 else fixed)
                    else:
                        trial[1 + plane] = level
                    p = host_params(plane, trial)
                    t1 = time.perf_counter()
                    ctx.memcpy_h2d(d_host_edges[plane], p)
                    ctx.lpf_search_sse(pr[plane], 0, pr[plane], 1, ps[plane], 0, d_host_edges[plane], p.size, 1, ustride[plane], 0, 3, d_sse)
                    ctx.sync()
                    v = int(ctx.from_device(d_sse, (1,), np.uint64)[0])
                    t2 = time.perf_counter()
                    clock["host"] += t1 - t0; clock["device"] += t2 - t1; clock["trials"] += 1
                    return v
                return get
            levels, traces = M.pick_frame(table_of, M.FULL_IMAGE, False, last, max_level)
            params = []
            for plane in range(3):                      # the chosen levels go through the producer once more before the filter can run
                t0 = time.perf_counter()
                p = host_params(plane, levels)
                t1 = time.perf_counter()
                ctx.memcpy_h2d(d_host_edges[plane], p); ctx.sync()
                clock["host"] += t1 - t0; clock["device"] += time.perf_counter() - t1
                params.append(p)
            return levels, traces, params

        t0 = time.perf_counter()                         # warm-up: kernels loaded, the clocks up
        while time.perf_counter() - t0 < 0.25:
            one_call(); ctx.sync()
        new_ms, tab_ms, trial_ms, seq_ms, seq_host_ms, seq_dev_ms, trials = [], [], [], [], [], [], 0
        for rep in range(args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            one_call()
            ctx.sync()
            new_ms.append((time.perf_counter() - t0) * 1e3)
            got = [int(v) for v in ctx.from_device(d_levels, (4,), np.int32)]
            tr = ctx.from_device(d_traces, (5, capi.LPF_TRACE_INTS), np.int32)
            # the five table launches, each synchronised on its own (the fixed levels are the ones the call chose)
            per = []
            for plane, d in M.SEARCHES:
                ctx.sync()
                t0 = time.perf_counter()
                ctx.lpf_level_sse_table(pr[plane], 0, ps[plane], 0, d_units[plane], ustride[plane], plane, int(plane > 0), d, fp, 0, d_levels, max_level, 0, d_t)
                ctx.sync()
                per.append((time.perf_counter() - t0) * 1e3)
            tab_ms.append(per)
            if args.only_new:
                continue
            clock.update(host=0.0, device=0.0, trials=0)
            t0 = time.perf_counter()
            levels, traces, params = host_search()
            seq_ms.append((time.perf_counter() - t0) * 1e3)
            seq_host_ms.append(clock["host"] * 1e3); seq_dev_ms.append(clock["device"] * 1e3); trials = clock["trials"]
            if got != levels or any(not np.array_equal(ctx.from_device(d_edges[p], units[p].shape + (4,), np.uint8), params[p]) for p in range(3)):
                raise SystemExit("the call and the host-driven search differ at %s: %s against %s" % (point, got, levels))
            assert [int(tr[i][0]) for i in range(5)] == [len(traces[i]) for i in range(5)]
            # one trial on records already in device memory
            ctx.sync()
            t0 = time.perf_counter()
            ctx.lpf_search_sse(pr[0], 0, pr[0], 1, ps[0], 0, d_host_edges[0], params[0].size, 1, ustride[0], 0, 3, d_sse)
            ctx.sync()
            trial_ms.append((time.perf_counter() - t0) * 1e3)
        tab = np.asarray(tab_ms)
        row = dict(width=W, height=H, bit_depth=bd, method="LPF_PICK_FROM_FULL_IMAGE", max_level=max_level, new=stats(new_ms),
                   tables_alone={"%d_%d" % s: stats(tab[:, i]) for i, s in enumerate(M.SEARCHES)}, tables_sum_median_ms=float(np.median(tab.sum(axis=1))),
                   luma_table_per_level_us=float(np.median(tab[:, 0])) * 1e3 / (max_level + 1))
        if not args.only_new:
            row.update(levels=levels, identical=True, trials=trials, sequence_wall=stats(seq_ms), sequence_host_share=stats(seq_host_ms),
                       sequence_device_share=stats(seq_dev_ms), lpf_search_trial_us=float(np.median(trial_ms)) * 1e3)
            row["factor_median"] = row["sequence_wall"]["median_ms"] / row["new"]["median_ms"]
            row["factor_device_share_only"] = row["sequence_device_share"]["median_ms"] / row["new"]["median_ms"]
        rows_out.append(row)
        print(json.dumps(row), flush=True)
        for d in d_units + d_edges + d_host_edges + [d_levels, d_tables, d_traces, d_sse, d_t]:
            ctx.free(d)
        for p in pr + ps:
            ctx.planes_free(p)
    if not args.only_new:
        rec = dict(tool="tools/lpf_pick_ab.py", timing="wall clock around synchronised calls, the call and the host-driven search alternating, after >= 0.25 s of "
                   "warm-up rounds; the host share is Python / numpy around two C producers", reps=args.reps, rows=rows_out)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
