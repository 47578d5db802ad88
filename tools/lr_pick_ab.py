"""A/B of the loop-restoration pick of a plane: the one device call (aomhip_pick_filter_restoration_plane) against the host-driven sequence over the entry
points that existed before it -- aomhip_search_wiener_batch on the units the variance prune leaves -> download -> the Wiener chain on the host -> the
surviving list -> aomhip_search_selfguided_restoration_batch -> aomhip_loop_restoration_filter_units into a spare ring + aomhip_sse_batch for
rusi->sse[RESTORE_SGRPROJ] -> download -> the self-guided and switchable chains and the frame type on the host -> upload of d_info -- on the same seeded
planes, in one process:

    python tools/lr_pick_ab.py [--reps 5] [--out profiles/lr_pick_ab.json]       (AOMHIP_LIB selects the library)

Planes: 1920x1080 and 3840x2160 10-bit luma and their 4:2:0 chroma planes (window 5), restoration units of 64 and 256 (32 and 128 for chroma), pruning
levels 0/0 and 2/2.  Both sides are timed wall-clock with the context synchronised, alternating, after warm-up.  The sequence's host logic is Python here
(tests/lr_pick_model.py's chains, numpy for the per-unit variance and SSE the prune needs before the Wiener search), where C needs microseconds per unit, so
its time is also given WITHOUT the time spent in that logic, and that smaller figure is the one the ratio uses: what remains are the launches, the three
synchronisations and the transfers.  Both sides must give identical plane records and unit infos or the tool fails.  Also timed: the self-guided trial pass
alone (aomhip_lr_trial_sse_units on every unit) against the filter into a spare ring plus aomhip_sse_batch."""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
pkg = importlib.import_module("aom-av1-psy_amd")
capi = pkg.capi
import lr_pick_model as PM  # noqa: E402  (the pinned host chains)

BW, BH = 32, 4          # the SSE blocks a unit is cut into: every unit of these workloads is a multiple of both


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return dict(min_ms=float(a[0]), median_ms=float(np.median(a)), max_ms=float(a[-1]), spread_ms=float(a[-1] - a[0]), n=len(a))


class Results:
    """lr_pick_model's leaves, answered from what the sequence has downloaded"""

    def __init__(self, none, var):
        self.none, self.var, self.w, self.s, self.t = none, var, {}, {}, {}

    def sse_none(self, u): return self.none[u]
    def src_var(self, u): return self.var[u]
    def wiener(self, u, win, ds): return self.w[u]
    def sgr(self, u, pruning): return self.s[u]
    def trial_sgr(self, u, info): return self.t[u]


class Sequence:
    def __init__(self, ctx, ps, pe, pc, pdst, units, src, cdef, bd, ss_y, P):
        self.ctx, self.ps, self.pe, self.pc, self.pdst, self.units, self.n, self.bd, self.ss_y, self.P = ctx, ps, pe, pc, pdst, units, len(units), bd, ss_y, P
        self.keys = [(int(u["h_start"]), int(u["h_end"]), int(u["v_start"]), int(u["v_end"])) for u in units]
        blocks = []
        for u in units:
            xs, ys = np.arange(u["h_start"], u["h_end"], BW), np.arange(u["v_start"], u["v_end"], BH)
            assert (u["h_end"] - u["h_start"]) % BW == 0 and (u["v_end"] - u["v_start"]) % BH == 0
            c = np.zeros(len(xs) * len(ys), capi.sad_cand_dtype)
            c["sx"] = c["rx"] = np.tile(xs, len(ys)); c["sy"] = c["ry"] = np.repeat(ys, len(xs))
            blocks.append(c)
        self.blocks = blocks
        nb = sum(len(b) for b in blocks)
        n = self.n
        self.d_u, self.d_info, self.d_c, self.d_e = ctx.malloc(16 * n), ctx.malloc(48 * n), ctx.malloc(8 * nb), ctx.malloc(8 * nb)
        self.d_w, self.d_s = ctx.malloc(64 * n), ctx.malloc(24 * n)
        t0 = time.perf_counter()      # what the variance prune needs before anything runs: host arithmetic, counted as host logic
        s64, c64 = src.astype(np.int64), cdef.astype(np.int64)
        self.var = {k: PM.unit_var(src, k) for k in self.keys}
        self.none = {k: int(((c64[k[2]:k[3], k[0]:k[1]] - s64[k[2]:k[3], k[0]:k[1]]) ** 2).sum()) for k in self.keys}
        self.prep_s = time.perf_counter() - t0

    def free(self):
        for d in (self.d_u, self.d_info, self.d_c, self.d_e, self.d_w, self.d_s):
            self.ctx.free(d)

    def filter_sse(self, idx, info):
        """filter the units idx into the spare ring, then their SSE against the source -> (int64 per unit, host seconds)"""
        ctx = self.ctx
        t0 = time.perf_counter()
        rec = np.ascontiguousarray(self.units[idx])
        cands = np.concatenate([self.blocks[i] for i in idx])
        cuts = np.concatenate([[0], np.cumsum([len(self.blocks[i]) for i in idx])[:-1]])
        host = time.perf_counter() - t0
        ctx.memcpy_h2d(self.d_u, rec); ctx.memcpy_h2d(self.d_info, info); ctx.memcpy_h2d(self.d_c, cands)
        ctx.loop_restoration_filter_units(self.pe, 0, self.pc, 0, self.pdst, 0, self.pc.width, self.pc.height, self.ss_y, self.d_u, None, len(idx), self.d_info)
        ctx.sse_batch(self.pdst, self.ps, 0, BW, BH, self.d_c, len(cands), self.d_e)
        e = ctx.from_device(self.d_e, (len(cands),), np.int64)
        t0 = time.perf_counter()
        out = np.add.reduceat(e, cuts)
        return out, host + time.perf_counter() - t0

    def run(self, flags):
        """-> (plane record, info records, host seconds)"""
        ctx, P, keys, bd = self.ctx, self.P, self.keys, self.bd
        host = self.prep_s
        t0 = time.perf_counter()
        L = Results(self.none, self.var)
        counts, trace = dict.fromkeys(PM.BRANCHES, 0), []
        rusi = PM.new_rusi(self.n)
        for r, f in zip(rusi, flags):
            r["skip_sgr_eval"] = int(f)
        keep = [i for i, k in enumerate(keys) if not (P["prune_wiener_based_on_src_var"] and (self.var[k] < P["wiener_src_var_thresh"] or self.none[k] == 0))]
        rec = np.ascontiguousarray(self.units[keep])
        host += time.perf_counter() - t0
        if keep:                                                            # 1. the Wiener call, 2. download
            ctx.memcpy_h2d(self.d_u, rec)
            ctx.search_wiener_batch(self.ps, 0, self.pe, 0, self.pc, 0, self.ss_y, P["reduced_wiener_win"], self.d_u, rec, len(keep), 0, self.d_w, None)
            w = ctx.from_device(self.d_w, (len(keep),), capi.wiener_search_result_dtype)
        t0 = time.perf_counter()
        for j, i in enumerate(keep):
            L.w[keys[i]] = dict(score=int(w["score"][j]), sse=int(w["sse"][j]), hfilter=w["hfilter"][j].tolist(), vfilter=w["vfilter"][j].tolist())
        plane = dict(frame_restoration_type=0, searched=15, cost=[0.0] * 4, bits=[0] * 4, sse=[0] * 4)
        res = [PM.search_norestore(L, keys, rusi), PM.search_wiener(L, keys, rusi, P, bd, counts, trace)]
        live = [i for i, r in enumerate(rusi) if not r["skip_sgr_eval"]]    # 3. the surviving list
        rec = np.ascontiguousarray(self.units[live])
        host += time.perf_counter() - t0
        if live:
            ctx.memcpy_h2d(self.d_u, rec)
            ctx.search_selfguided_restoration_batch(self.ps, 0, self.pc, 0, self.d_u, rec, len(live), P["enable_sgr_ep_pruning"], self.d_s, None)
            s = ctx.from_device(self.d_s, (len(live),), capi.sgr_search_result_dtype)
            t0 = time.perf_counter()
            info = np.zeros(len(live), capi.lr_unit_info_dtype)
            info["restoration_type"], info["sgr_params_idx"], info["xqd"] = 2, s["ep"], s["xqd"]
            host += time.perf_counter() - t0
            errs, h = self.filter_sse(live, info)                          # 4. filter into the spare ring + SSE, download
            host += h
        t0 = time.perf_counter()
        for j, i in enumerate(live):
            L.s[keys[i]] = dict(ep=int(s["ep"][j]), xqd=s["xqd"][j].tolist())
            L.t[keys[i]] = int(errs[j])
        res.append(PM.search_sgrproj(L, keys, rusi, P, bd, counts, trace))   # 5. the two remaining chains and the frame type
        res.append(PM.search_switchable(L, keys, rusi, P, bd, counts, trace))
        best_cost, best = 0.0, 0
        for t, (bits, sse) in enumerate(res):
            cost = PM.rdcost_dbl(P["rdmult"], bits, sse, bd)
            plane["cost"][t], plane["bits"][t], plane["sse"][t] = cost, bits, sse
            if t == 0 or cost < best_cost:
                best_cost, best = cost, t
        plane["frame_restoration_type"] = best
        irec = PM.info_records(capi, [PM.unit_info(best, r) for r in rusi])
        host += time.perf_counter() - t0
        ctx.memcpy_h2d(self.d_info, irec)                                   # 6. upload for the frame filter
        ctx.sync()
        return PM.plane_record(capi, plane), irec, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_pick_ab.json"))
    ap.add_argument("--points", default="1920x1080x10,3840x2160x10")
    ap.add_argument("--units", default="64,256")
    args = ap.parse_args()
    ctx = capi.Context(0)
    B = 16
    rows = []
    for point in args.points.split(","):
        Wl, Hl, bd = (int(v) for v in point.split("x"))
        for ss_y in (0, 1):
            Wd, Hd = Wl >> ss_y, Hl >> ss_y
            mx = (1 << bd) - 1
            rng = np.random.default_rng(Wd + bd)
            yy, xx = np.mgrid[0:Hd, 0:Wd]
            src = np.clip((np.sin(xx / 11.0) + np.cos(yy / 8.0) + 2) * 0.25 * mx * (xx > Wd // 3) + mx // 3 + rng.integers(-mx // 30, mx // 30 + 1, (Hd, Wd)) * (xx > Wd // 6),
                          0, mx).astype(np.uint16)                          # (flat on the left: the variance prune has something to prune)
            cdef = np.clip(src.astype(np.int32) + rng.integers(-mx // 12, mx // 12 + 1, src.shape), 0, mx).astype(np.uint16)
            deb = np.clip(cdef.astype(np.int32) + rng.integers(-mx // 32, mx // 32 + 1, src.shape), 0, mx).astype(np.uint16)
            ps, pe, pc, pdst = (ctx.planes_alloc(Wd, Hd, B, bd, 1) for _ in range(4))
            ctx.planes_upload(ps, 0, src); ctx.planes_upload(pe, 0, deb); ctx.planes_upload(pc, 0, cdef)
            for U in (int(v) >> ss_y for v in args.units.split(",")):
                units = capi.lr_units_in_plane(Wd, Hd, U, ss_y)
                n = len(units)
                d_u, d_f, d_i, d_p, d_e = ctx.to_device(units), ctx.malloc(max(n, 16)), ctx.malloc(48 * n), ctx.malloc(104), ctx.malloc(8 * n)
                for levels in ((0, 0), (2, 2)):
                    win = 5 if ss_y else 7
                    var = sorted(PM.unit_var(src, (int(u["h_start"]), int(u["h_end"]), int(u["v_start"]), int(u["v_end"]))) for u in units)
                    P = PM.default_params(rdmult=1200, wiener_win=win, reduced_wiener_win=win, prune_wiener_based_on_src_var=levels[0], prune_sgr_based_on_wiener=levels[1],
                                          enable_sgr_ep_pruning=int(levels[1] > 0), dual_sgr_penalty_level=levels[0], wiener_src_var_thresh=var[n // 4] if levels[0] else 0)
                    prec = PM.params_record(capi, P)
                    seq = Sequence(ctx, ps, pe, pc, pdst, units, src, cdef, bd, ss_y, P)
                    new_ms, seq_ms, seq_dev_ms, trial_ms, fs_ms = [], [], [], [], []
                    for rep in range(args.warmup + args.reps):
                        ctx.memset(d_f, 0, n); ctx.sync()
                        t0 = time.perf_counter()
                        ctx.pick_filter_restoration_plane(ps, 0, pe, 0, pc, 0, ss_y, d_u, units, n, prec, d_f, None, d_i, d_p)
                        ctx.sync()
                        t1 = time.perf_counter()
                        got_p, got_i = ctx.from_device(d_p, (1,), capi.lr_plane_pick_dtype), ctx.from_device(d_i, (n,), capi.lr_unit_info_dtype)
                        t2 = time.perf_counter()
                        want_p, want_i, host = seq.run([0] * n)
                        t3 = time.perf_counter()
                        if got_p.tobytes() != want_p.tobytes() or not np.array_equal(got_i, want_i):
                            raise SystemExit("the call and the host-driven sequence differ at %s ss_y %d unit size %d levels %s\n%s\n%s" % (point, ss_y, U, levels, got_p, want_p))
                        # the self-guided trial alone: every unit with the infos just picked turned into RESTORE_SGRPROJ ones
                        info = got_i.copy(); info["restoration_type"] = 2
                        ctx.memcpy_h2d(d_i, info); ctx.sync()
                        t4 = time.perf_counter()
                        ctx.lr_trial_sse_units(ps, 0, pe, 0, pc, 0, Wd, Hd, ss_y, d_u, None, n, d_i, d_e)
                        ctx.sync()
                        t5 = time.perf_counter()
                        a = ctx.from_device(d_e, (n,), np.int64)
                        t6 = time.perf_counter()
                        b, h = seq.filter_sse(list(range(n)), info)
                        t7 = time.perf_counter()
                        assert np.array_equal(a, b)
                        if rep >= args.warmup:
                            new_ms.append((t1 - t0) * 1e3); seq_ms.append((t3 - t2 + seq.prep_s) * 1e3); seq_dev_ms.append((t3 - t2 + seq.prep_s - host) * 1e3)
                            trial_ms.append((t5 - t4) * 1e3); fs_ms.append((t7 - t6 - h) * 1e3)
                    row = dict(width=Wd, height=Hd, bit_depth=bd, ss_y=ss_y, unit_size=U, n_units=n, levels=list(levels), identical=True,
                               frame_restoration_type=int(got_p["frame_restoration_type"][0]), new=stats(new_ms), sequence_wall=stats(seq_ms),
                               sequence_without_host_python=stats(seq_dev_ms), trial_pass=stats(trial_ms), filter_plus_sse=stats(fs_ms))
                    row["factor_median"] = row["sequence_without_host_python"]["median_ms"] / row["new"]["median_ms"]
                    row["trial_factor_median"] = row["filter_plus_sse"]["median_ms"] / row["trial_pass"]["median_ms"]
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    seq.free()
                for d in (d_u, d_f, d_i, d_p, d_e):
                    ctx.free(d)
            for p in (ps, pe, pc, pdst):
                ctx.planes_free(p)
    rec = dict(tool="tools/lr_pick_ab.py",
               timing="wall clock around synchronised calls, the call and the sequence alternating, after %d warm-up round(s)" % args.warmup, reps=args.reps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
