"""A/B of the self-guided restoration search: the one device call (aomhip_search_selfguided_restoration_batch) against the host-driven sequence over
the three entry points it is built from (aomhip_selfguided_restoration_batch, aomhip_calc_proj_params_batch, aomhip_pixel_proj_error_batch: one filter
launch and one statistics launch + download per stage of the search, the 2 x 2 solve and encode_xq on the host, one error launch + download per step of
the refinement walk because the next candidate depends on the last error), on the same seeded planes, in one process:

    python tools/sgr_search_ab.py [--reps 7] [--out profiles/sgr_search_ab.json]       (AOMHIP_LIB selects the library)

Planes: 3840x2160 10-bit and 1920x1080 8-bit luma, restoration units of 64 and 256, both pruning settings.  The sequence is batched over ALL units
and all parameter sets of a stage (every unit's walk advances in lock-step, one launch per step), which is the cheapest way to drive it.  Both sides are
timed wall-clock with the context synchronised, alternating, after warm-up; the sequence's time is also given without the time its host logic spends in
Python (a C host would spend close to none), and that smaller figure is the one the ratio uses.  Both must give identical records or the tool fails."""
import argparse
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
import test_golden_sgr_search as W  # noqa: E402  (the pinned host walk: solve, encode_xq, finer_search, the two orders)

SGR_R = np.array(W.SGR_R, np.int32)


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return dict(min_ms=float(a[0]), median_ms=float(np.median(a)), max_ms=float(a[-1]), spread_ms=float(a[-1] - a[0]), n=len(a))


def finer_search(xqd, r, start_step=2):
    """finer_search_pixel_proj_error (av1/encoder/pickrst.c:402-461) as test_golden_sgr_search.finer_search walks it, as a generator: every
    `yield xq` is one get_pixel_proj_error evaluation, answered by send(err)"""
    err = yield W.decode_xq(xqd, r)
    s = start_step
    while s >= 1:
        for p in range(2):
            if r[p] == 0:
                continue
            skip = False
            while xqd[p] - s >= W.TAP_MIN[p]:
                xqd[p] -= s
                err2 = yield W.decode_xq(xqd, r)
                if err2 > err:
                    xqd[p] += s
                    break
                err, skip = err2, True
                if s != start_step:
                    break
            if skip:
                break
            while xqd[p] + s <= W.TAP_MAX[p]:
                xqd[p] += s
                err2 = yield W.decode_xq(xqd, r)
                if err2 > err:
                    xqd[p] -= s
                    break
                err = err2
                if s != start_step:
                    break
        s >>= 1
    return err


class Sequence:
    """the host-driven search over preallocated device lists; run() -> (best records, seconds spent in host Python logic)"""

    def __init__(self, ctx, ps, pd, units):
        self.ctx, self.ps, self.pd, self.units, self.n = ctx, ps, pd, units, len(units)
        self.mw, self.mh = int((units["h_end"] - units["h_start"]).max()), int((units["v_end"] - units["v_start"]).max())
        ne = self.n * 16
        self.pitch = self.mw * self.mh
        self.d_f0, self.d_f1 = ctx.malloc(4 * ne * self.pitch), ctx.malloc(4 * ne * self.pitch)
        self.d_u, self.d_i, self.d_r, self.d_xq = ctx.malloc(16 * ne), ctx.malloc(4 * ne), ctx.malloc(8 * ne), ctx.malloc(8 * ne)
        self.d_H, self.d_C, self.d_e = ctx.malloc(32 * ne), ctx.malloc(16 * ne), ctx.malloc(8 * ne)

    def stage(self, eps):
        """eps[i] = the parameter sets unit i evaluates in this stage -> {(i, ep): (exqd, err)}; host time"""
        ctx, host = self.ctx, 0.0
        t0 = time.perf_counter()
        ent = [(i, ep) for i in range(self.n) for ep in eps[i]]
        ne = len(ent)
        rec = np.ascontiguousarray(self.units[[i for i, _ in ent]])
        idx = np.array([ep for _, ep in ent], np.int32)
        radii = np.ascontiguousarray(SGR_R[idx])
        host += time.perf_counter() - t0
        ctx.memcpy_h2d(self.d_u, rec); ctx.memcpy_h2d(self.d_i, idx); ctx.memcpy_h2d(self.d_r, radii)
        ctx.selfguided_restoration_batch(self.pd, 0, self.d_u, None, ne, self.d_i, self.mw, self.mh, self.d_f0, self.d_f1, self.mw, self.pitch)
        ctx.calc_proj_params_batch(self.ps, 0, self.pd, 0, self.d_u, ne, self.d_f0, self.d_f1, self.mw, self.pitch, self.d_r, self.d_H, self.d_C)
        Hs, Cs = ctx.from_device(self.d_H, (ne, 4), np.int64), ctx.from_device(self.d_C, (ne, 2), np.int64)
        t0 = time.perf_counter()
        counts = dict.fromkeys(W.BRANCHES, 0)
        out, walks, xq = {}, [], np.zeros((ne, 2), np.int32)

        def walk(k):   # one entry's solve, encode_xq and refinement walk as a coroutine: yields the xq it wants the error of
            r = tuple(int(v) for v in radii[k])
            xqd = W.encode_xq(W.solve(Hs[k], Cs[k], r, counts), r)
            err = yield from finer_search(xqd, r)
            out[ent[k]] = (xqd, err)
        for k in range(ne):
            g = walk(k)
            try:
                xq[k] = next(g)
                walks.append(g)
            except StopIteration:
                walks.append(None)
        host += time.perf_counter() - t0
        while any(g is not None for g in walks):
            ctx.memcpy_h2d(self.d_xq, xq)
            ctx.pixel_proj_error_batch(self.ps, 0, self.pd, 0, self.d_u, ne, self.d_f0, self.d_f1, self.mw, self.pitch, self.d_r, self.d_xq, 1, self.d_e)
            errs = ctx.from_device(self.d_e, (ne,), np.int64)
            t0 = time.perf_counter()
            for k, g in enumerate(walks):
                if g is None:
                    continue
                try:
                    xq[k] = g.send(int(errs[k]))
                except StopIteration:
                    walks[k] = None
            host += time.perf_counter() - t0
        return out, host

    def run(self, pruning):
        n, host = self.n, 0.0
        best = [{"ep": 0, "xqd": [0, 0], "err": -1} for _ in range(n)]

        def fold(res, eps):
            for i in range(n):
                for ep in eps[i]:
                    xqd, err = res[i, ep]
                    if best[i]["err"] == -1 or err < best[i]["err"]:
                        best[i] = {"ep": ep, "xqd": xqd, "err": err}
        if not pruning:
            plan = [lambda: [list(range(16))] * n]
        else:
            plan = [lambda: [list(W.GRP1_SEED)] * n, lambda: [[e for e in (b["ep"] - 1, b["ep"] + 1) if 0 <= e <= 9] for b in best],
                    lambda: [[W.GRP2_3[0][b["ep"]]] for b in best], lambda: [[W.GRP2_3[1][b["ep"]]] for b in best]]
        for p in plan:
            eps = p()
            res, h = self.stage(eps)
            t0 = time.perf_counter()
            fold(res, eps)
            host += h + time.perf_counter() - t0
        return best, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgr_search_ab.json"))
    ap.add_argument("--points", default="3840x2160x10,1920x1080x8")
    args = ap.parse_args()
    ctx = capi.Context(0)
    B = 16
    rows = []
    for point in args.points.split(","):
        Wd, Hd, bd = (int(v) for v in point.split("x"))
        mx = (1 << bd) - 1
        rng = np.random.default_rng(Wd + bd)
        src = pkg.synth.lcg_frame(Wd, Hd, 3, 0, bd)
        dat = np.clip(src.astype(np.int32) + rng.integers(-mx // 16, mx // 16 + 1, src.shape), 0, mx).astype(src.dtype)
        ps, pd = ctx.planes_alloc(Wd, Hd, B, bd, 1), ctx.planes_alloc(Wd, Hd, B, bd, 1)
        ctx.planes_upload(ps, 0, src); ctx.planes_upload(pd, 0, dat)
        for U in (64, 256):
            units = capi.lr_units_in_plane(Wd, Hd, U, 0)
            n = len(units)
            seq = Sequence(ctx, ps, pd, units)
            d_u, d_b = ctx.to_device(units), ctx.malloc(24 * n)
            for pruning in (0, 1):
                new_ms, seq_ms, seq_dev_ms = [], [], []
                for rep in range(args.warmup + args.reps):
                    ctx.sync()
                    t0 = time.perf_counter()
                    ctx.search_selfguided_restoration_batch(ps, 0, pd, 0, d_u, units, n, pruning, d_b, None)
                    ctx.sync()
                    t1 = time.perf_counter()
                    got = ctx.from_device(d_b, (n,), capi.sgr_search_result_dtype)
                    t2 = time.perf_counter()
                    want, host = seq.run(pruning)
                    ctx.sync()
                    t3 = time.perf_counter()
                    same = all(int(g["ep"]) == w["ep"] and g["xqd"].tolist() == w["xqd"] and int(g["err"]) == w["err"] for g, w in zip(got, want))
                    if not same:
                        raise SystemExit("the call and the host-driven sequence differ at %s unit %d pruning %d" % (point, U, pruning))
                    if rep >= args.warmup:
                        new_ms.append((t1 - t0) * 1e3); seq_ms.append((t3 - t2) * 1e3); seq_dev_ms.append((t3 - t2 - host) * 1e3)
                row = dict(width=Wd, height=Hd, bit_depth=bd, unit_size=U, n_units=n, pruning=pruning, identical=True, new=stats(new_ms),
                           sequence_wall=stats(seq_ms), sequence_without_host_python=stats(seq_dev_ms))
                row["factor_median"] = row["sequence_without_host_python"]["median_ms"] / row["new"]["median_ms"]
                rows.append(row)
                print(json.dumps(row), flush=True)
            for d in (d_u, d_b):
                ctx.free(d)
        ctx.planes_free(ps); ctx.planes_free(pd)
    rec = dict(tool="tools/sgr_search_ab.py", timing="wall clock around synchronised calls, the call and the sequence alternating, after %d warm-up rounds" % args.warmup,
               reps=args.reps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
