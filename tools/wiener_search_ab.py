"""A/B of the Wiener restoration search: the one device call (aomhip_search_wiener_batch) against the host-driven sequence over the entry points that
existed before it -- aomhip_compute_stats_batch + download of M and H, wiener_decompose_sep_sym / finalize_sym_filter / compute_score on the host, then
finer_tile_search_wiener with every unit's walk advancing in lock-step: per step one aomhip_loop_restoration_filter_units over the units still walking,
one aomhip_sse_batch over their 64 x 8 blocks and one download, because the next filter depends on the last error -- on the same seeded planes, in one
process:

    python tools/wiener_search_ab.py [--reps 5] [--out profiles/wiener_search_ab.json]       (AOMHIP_LIB selects the library)

Planes: 3840x2160 10-bit and 1920x1080 8-bit luma (smooth content with texture, degraded by noise, so that the walks run), restoration units of 64 and
256, window 7.  The sequence is batched over ALL units, which is the
cheapest way to drive it.  Both sides are timed wall-clock with the context synchronised, alternating, after warm-up.  The sequence's host logic is Python
here (tests/test_golden_wiener_search.py's pinned chain: some 25 ms per unit for the solve alone, where C needs microseconds), so its time is also given
WITHOUT the time spent in that logic, and that smaller figure is the one the ratio uses.  The solve of the sequence is computed in the first repetition and
re-used (it does not depend on the repetition; its time is host logic either way and is added to every repetition's wall-clock figure).  A unit wider than
256 -- the last one of a row may be 384 -- is beyond aomhip_compute_stats_batch's limit: the sequence takes its statistics from the CPU oracle and books
that time as host logic too, i.e. in the sequence's favour.  Both sides must give identical records or the tool fails."""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
pkg = importlib.import_module("aom-av1-psy_amd")
capi = pkg.capi
import test_golden_wiener_search as W  # noqa: E402  (the pinned host chain)

WIN = 7
BW, BH = 64, 8          # the SSE blocks a unit is cut into: every unit of these workloads is a multiple of both


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return dict(min_ms=float(a[0]), median_ms=float(np.median(a)), max_ms=float(a[-1]), spread_ms=float(a[-1] - a[0]), n=len(a))


def finer_search(h, v):
    """finer_tile_search_wiener (av1/encoder/pickrst.c:1396-1501) as test_golden_wiener_search.finer_search walks it, as a generator: every `yield` is
    one try_restoration_unit of the filters h, v (changed in place), answered by send(err)"""
    err = yield
    s = W.START_STEP
    while s >= 1:
        for f in (h, v):
            for p in range(W.HALFWIN):
                skip = False
                for d in (-1, 1):
                    while W.TAP_MIN[p] <= f[p] + d * s <= W.TAP_MAX[p]:
                        f[p] += d * s; f[6 - p] += d * s; f[3] -= 2 * d * s
                        err2 = yield
                        if err2 > err:
                            f[p] -= d * s; f[6 - p] -= d * s; f[3] += 2 * d * s
                            break
                        err, skip = err2, skip or d < 0
                        if s != W.START_STEP:
                            break
                    if skip:
                        break
                if skip:
                    break
        s >>= 1
    return err


class Sequence:
    """the host-driven search over preallocated device lists; run() -> (records, seconds spent in host logic)"""

    def __init__(self, ctx, ps, pe, pc, pdst, units, src, cdef, bd):
        self.ctx, self.ps, self.pe, self.pc, self.pdst, self.units, self.n, self.bd = ctx, ps, pe, pc, pdst, units, len(units), bd
        self.src, self.cdef = src, cdef
        n = self.n
        self.wide = np.flatnonzero(units["h_end"] - units["h_start"] > 256)
        self.narrow = np.flatnonzero(units["h_end"] - units["h_start"] <= 256)
        blocks, first = [], [0]
        for u in units:
            xs, ys = np.arange(u["h_start"], u["h_end"], BW), np.arange(u["v_start"], u["v_end"], BH)
            assert (u["h_end"] - u["h_start"]) % BW == 0 and (u["v_end"] - u["v_start"]) % BH == 0
            c = np.zeros(len(xs) * len(ys), capi.sad_cand_dtype)
            c["sx"] = c["rx"] = np.tile(xs, len(ys))
            c["sy"] = c["ry"] = np.repeat(ys, len(xs))
            blocks.append(c)
            first.append(first[-1] + len(c))
        self.blocks, self.first = blocks, np.array(first)
        nb = int(self.first[-1])
        self.d_u, self.d_info, self.d_c, self.d_e = ctx.malloc(16 * n), ctx.malloc(48 * n), ctx.malloc(capi.sad_cand_dtype.itemsize * nb), ctx.malloc(8 * nb)
        self.d_M, self.d_H = ctx.malloc(8 * 49 * n), ctx.malloc(8 * 2401 * n)
        self.solved = None

    def unit_sse(self, a, b, idx):
        """the SSE of ring a against ring b over the units idx -> int64 per unit; host seconds"""
        ctx = self.ctx
        t0 = time.perf_counter()
        cands = np.concatenate([self.blocks[i] for i in idx])
        cuts = np.concatenate([[0], np.cumsum([len(self.blocks[i]) for i in idx])[:-1]])
        host = time.perf_counter() - t0
        ctx.memcpy_h2d(self.d_c, cands)
        ctx.sse_batch(a, b, 0, BW, BH, self.d_c, len(cands), self.d_e)
        e = ctx.from_device(self.d_e, (len(cands),), np.int64)
        t0 = time.perf_counter()
        out = np.add.reduceat(e, cuts)
        return out, host + time.perf_counter() - t0

    def statistics(self):
        """-> (M, H) of every unit; host seconds"""
        ctx, n, host = self.ctx, self.n, 0.0
        M, H = np.zeros((n, 49), np.int64), np.zeros((n, 2401), np.int64)
        if len(self.narrow):
            rec = np.ascontiguousarray(self.units[self.narrow])
            ctx.memcpy_h2d(self.d_u, rec)
            ctx.compute_stats_batch(self.pc, 0, self.ps, 0, WIN, self.d_u, rec, len(rec), 0, self.d_M, self.d_H)
            M[self.narrow], H[self.narrow] = ctx.from_device(self.d_M, (len(rec), 49), np.int64), ctx.from_device(self.d_H, (len(rec), 2401), np.int64)
        if len(self.wide):
            import pyoracle
            t0 = time.perf_counter()
            f = pyoracle.lib.orc_compute_stats
            f.restype = None
            ext, sx = pyoracle.extend_plane(self.cdef, 8), pyoracle.extend_plane(self.src, 8)
            for i in self.wide:
                u = self.units[i]
                f(WIN, ctypes.c_void_p(pyoracle._addr(ext, 8, 8)), ctypes.c_void_p(pyoracle._addr(sx, 8, 8)), int(u["h_start"]), int(u["h_end"]), int(u["v_start"]),
                  int(u["v_end"]), ext.shape[1], sx.shape[1], int(self.bd > 8), self.bd, 0, ctypes.c_void_p(M[i].ctypes.data), ctypes.c_void_p(H[i].ctypes.data))
            host += time.perf_counter() - t0
        return M, H, host

    def run(self):
        ctx, n, units = self.ctx, self.n, self.units
        M, H, host = self.statistics()
        t0 = time.perf_counter()
        if self.solved is None:
            counts = dict.fromkeys(W.BRANCHES, 0)
            solved = []
            for i in range(n):
                Mi, Hi = [int(x) for x in M[i]], [int(x) for x in H[i]]
                a, b, singular = W.decompose(WIN, Mi, Hi, counts)
                vf, hf = W.finalize(WIN, a, counts), W.finalize(WIN, b, counts)
                solved.append((hf, vf, W.compute_score(WIN, Mi, Hi, vf, hf), singular))
            self.solved, self.solve_s = solved, time.perf_counter() - t0
        host += self.solve_s
        t0 = time.perf_counter()
        res = np.zeros(n, capi.wiener_search_result_dtype)
        walks = [None] * n
        filt = [None] * n
        for i, (hf, vf, score, singular) in enumerate(self.solved):
            filt[i] = (list(hf), list(vf))
            res[i] = (hf, vf, W.INT64_MAX, 0, score, 0, singular)
            if not score > 0:
                walks[i] = finer_search(*filt[i])
                next(walks[i])
        host += time.perf_counter() - t0
        none, h = self.unit_sse(self.pc, self.ps, range(n))
        res["sse_none"] = none
        host += h
        while True:
            t0 = time.perf_counter()
            idx = [i for i in range(n) if walks[i] is not None]
            if not idx:
                break
            rec = np.ascontiguousarray(units[idx])
            info = np.zeros(len(idx), capi.lr_unit_info_dtype)
            info["restoration_type"] = 1
            info["hfilter"], info["vfilter"] = [filt[i][0] for i in idx], [filt[i][1] for i in idx]
            host += time.perf_counter() - t0
            ctx.memcpy_h2d(self.d_u, rec); ctx.memcpy_h2d(self.d_info, info)
            ctx.loop_restoration_filter_units(self.pe, 0, self.pc, 0, self.pdst, 0, self.pc.width, self.pc.height, 0, self.d_u, None, len(idx), self.d_info)
            errs, h = self.unit_sse(self.pdst, self.ps, idx)
            t0 = time.perf_counter()
            for k, i in enumerate(idx):
                res["trials"][i] += 1
                try:
                    walks[i].send(int(errs[k]))
                except StopIteration as done:
                    walks[i] = None
                    res["sse"][i] = done.value
                    res["hfilter"][i], res["vfilter"][i] = filt[i]
            host += h + time.perf_counter() - t0
        return res, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wiener_search_ab.json"))
    ap.add_argument("--points", default="3840x2160x10,1920x1080x8")
    ap.add_argument("--units", default="64,256")
    args = ap.parse_args()
    ctx = capi.Context(0)
    B = 16
    rows = []
    for point in args.points.split(","):
        Wd, Hd, bd = (int(v) for v in point.split("x"))
        mx = (1 << bd) - 1
        rng = np.random.default_rng(Wd + bd)
        # smooth content with some texture, degraded by noise: a filter pays, so the walks run (on white noise compute_score sends every unit back to
        # RESTORE_NONE and nothing is walked); tests/test_gpu_wiener_search.py's frame, larger
        yy, xx = np.mgrid[0:Hd, 0:Wd]
        dt = np.uint8 if bd == 8 else np.uint16
        src = np.clip((np.sin(xx / 11.0) + np.cos(yy / 8.0) + 2) * 0.25 * mx + rng.integers(-mx // 30, mx // 30 + 1, (Hd, Wd)), 0, mx).astype(dt)
        cdef = np.clip(src.astype(np.int32) + rng.integers(-mx // 12, mx // 12 + 1, src.shape), 0, mx).astype(dt)
        deb = np.clip(cdef.astype(np.int32) + rng.integers(-mx // 32, mx // 32 + 1, src.shape), 0, mx).astype(src.dtype)
        ps, pe, pc, pdst = (ctx.planes_alloc(Wd, Hd, B, bd, 1) for _ in range(4))
        ctx.planes_upload(ps, 0, src); ctx.planes_upload(pe, 0, deb); ctx.planes_upload(pc, 0, cdef)
        for U in (int(v) for v in args.units.split(",")):
            units = capi.lr_units_in_plane(Wd, Hd, U, 0)
            n = len(units)
            seq = Sequence(ctx, ps, pe, pc, pdst, units, src, cdef, bd)
            d_u, d_r = ctx.to_device(units), ctx.malloc(64 * n)
            new_ms, seq_ms, seq_dev_ms = [], [], []
            for rep in range(args.warmup + args.reps):
                ctx.sync()
                t0 = time.perf_counter()
                ctx.search_wiener_batch(ps, 0, pe, 0, pc, 0, 0, WIN, d_u, units, n, 0, d_r, None)
                ctx.sync()
                t1 = time.perf_counter()
                got = ctx.from_device(d_r, (n,), capi.wiener_search_result_dtype)
                t2 = time.perf_counter()
                want, host = seq.run()
                ctx.sync()
                t3 = time.perf_counter()
                if not np.array_equal(got, want):
                    bad = [i for i in range(n) if got[i] != want[i]]
                    raise SystemExit("the call and the host-driven sequence differ at %s unit size %d: units %s\n%s\n%s" % (point, U, bad[:8], got[bad[0]], want[bad[0]]))
                wall = t3 - t2 + (seq.solve_s if rep else 0.0)       # (the first repetition has run the solve itself)
                if rep >= args.warmup:
                    new_ms.append((t1 - t0) * 1e3); seq_ms.append(wall * 1e3); seq_dev_ms.append((wall - host) * 1e3)
            row = dict(width=Wd, height=Hd, bit_depth=bd, unit_size=U, n_units=n, wiener_win=WIN, identical=True, steps=int(want["trials"].max()),
                       mean_trials=float(want["trials"].mean()), units_with_positive_score=int((want["score"] > 0).sum()),
                       units_wider_than_256=int(len(seq.wide)), host_solve_ms=seq.solve_s * 1e3, new=stats(new_ms), sequence_wall=stats(seq_ms),
                       sequence_without_host_python=stats(seq_dev_ms))
            row["factor_median"] = row["sequence_without_host_python"]["median_ms"] / row["new"]["median_ms"]
            row["factor_worst_case"] = row["sequence_without_host_python"]["min_ms"] / row["new"]["max_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            for d in (d_u, d_r, seq.d_u, seq.d_info, seq.d_c, seq.d_e, seq.d_M, seq.d_H):
                ctx.free(d)
        for p in (ps, pe, pc, pdst):
            ctx.planes_free(p)
    rec = dict(tool="tools/wiener_search_ab.py",
               timing="wall clock around synchronised calls, the call and the sequence alternating, after %d warm-up round(s)" % args.warmup, reps=args.reps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
