"""A/B of av1_cdef_search for a frame: the one device call (aomhip_cdef_search_frame) against the host-driven sequence over the entry points that existed
before it -- aomhip_cdef_search_sse_luma + 2 x aomhip_cdef_search_sse_chroma -> synchronise -> download of the three tables -> the entry list, the merge
and the pick on the host (tests/cdef_pick_model.py) -> aomhip_cdef_build_strengths -> upload of the four level planes -- on the same seeded frames, in
one process:

    python tools/cdef_pick_ab.py [--reps 5] [--out profiles/cdef_pick_ab.json]       (AOMHIP_LIB selects the library)

Frames: 1920x1080 and 3840x2160 10-bit 4:2:0, the full list (64 strengths) and CDEF_FAST_SEARCH_LVL1 (32).  Both sides are timed wall-clock with the
context synchronised, alternating, after warm-up rounds that keep the device busy for at least 0.25 s.  The sequence's host logic is Python / numpy here,
where C needs milliseconds, so its time is also given WITHOUT the time spent in that logic, and that smaller figure is the one the ratio uses: what
remains are the three launches, the synchronisation and the transfers -- note that it then contains NO pick at all, which the one call does on the
device.  The host logic is run once per row (its inputs do not change between repetitions) and its time counted in every repetition.  Both sides must give
identical records, index planes and level planes or the tool fails.  Also timed, each synchronised on its own: the three SSE calls alone and
aomhip_cdef_pick_strengths alone on the frame's compacted tables, which give the share of the tables in the one call."""
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
import cdef_pick_model as M  # noqa: E402  (the pinned host pick)


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return dict(min_ms=float(a[0]), median_ms=float(np.median(a)), max_ms=float(a[-1]), spread_ms=float(a[-1] - a[0]), n=len(a))


def content(rng, W, H, bd, shift):
    mx = (1 << bd) - 1
    base = rng.integers(mx // 8, mx - mx // 8, (H // 8 + 1, W // 8 + 1))
    i, j = np.indices((H, W))
    src = np.clip(np.kron(base, np.ones((8, 8), np.int64))[:H, :W] + ((i * 3 + j * 5 + shift) % 17) * (mx // 255 + 1) + rng.integers(-8, 9, (H, W)) * (mx // 255 + 1), 0, mx)
    rec = np.clip(src + rng.integers(-(6 << (bd - 8)), (6 << (bd - 8)) + 1, (H, W)), 0, mx)
    return rec.astype(np.uint16), src.astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdef_pick_ab.json"))
    ap.add_argument("--points", default="1920x1080x10,3840x2160x10")
    ap.add_argument("--methods", default="0,1")
    args = ap.parse_args()
    ctx = capi.Context(0)
    B, damping, rdmult = 16, 5, 1200
    rows = []
    for point in args.points.split(","):
        W, H, bd = (int(v) for v in point.split("x"))
        rng = np.random.default_rng(W + bd)
        dims = [(W, H), (W // 2, H // 2), (W // 2, H // 2)]
        recon, source = [], []
        for p, (w, h) in enumerate(dims):
            r, s = content(rng, w, h, bd, p)
            recon.append(r); source.append(s)
        skip = (rng.random((H // 8, W // 8)) < 0.15).astype(np.uint8)
        nvfb, nhfb = (H + 63) // 64, (W + 63) // 64
        for k in range(0, nvfb * nhfb, 11):                # whole filter blocks skipped
            skip[(k // nhfb) * 8:(k // nhfb) * 8 + 8, (k % nhfb) * 8:(k % nhfb) * 8 + 8] = 1
        pr = [ctx.planes_alloc(w, h, B, bd, 1) for w, h in dims]
        ps = [ctx.planes_alloc(w, h, B, bd, 1) for w, h in dims]
        for p in range(3):
            ctx.planes_upload(pr[p], 0, recon[p]); ctx.planes_upload(ps[p], 0, source[p])
        d_skip = ctx.to_device(skip)
        nfb = nvfb * nhfb
        for method in (int(v) for v in args.methods.split(",")):
            n = M.NB_STRENGTHS[method]
            strengths = M.mapped(M.strength_list(method))
            d_st = ctx.to_device(np.asarray(strengths, np.uint8))
            d_sse = [ctx.malloc(8 * n * nfb) for _ in range(3)]
            d_dir = ctx.malloc((H // 8) * (W // 8))
            # the one call's outputs, and the sequence's uploads
            d_idx, d_lv = ctx.malloc(max(nfb, 16)), [ctx.malloc(max(nfb, 16)) for _ in range(4)]
            d_pick, d_m0, d_m1, d_efb = ctx.malloc(capi.cdef_pick_dtype.itemsize), ctx.malloc(8 * n * nfb), ctx.malloc(8 * n * nfb), ctx.malloc(4 * nfb)
            d_up = [ctx.malloc(max(nfb, 16)) for _ in range(4)]
            d_cnt, d_gi, d_pick2 = ctx.malloc(16), ctx.malloc(max(nfb, 16)), ctx.malloc(capi.cdef_pick_dtype.itemsize)

            def one_call():
                ctx.cdef_search_frame(pr, 0, ps, 0, 1, 1, d_st, n, int(method > 0), d_skip, damping, rdmult, nhfb, d_idx, d_lv[0], d_lv[1], d_pick, d_lv[2], d_lv[3],
                                      None, d_dir, None, d_m0, d_m1, d_efb)

            def tables():
                ctx.cdef_search_sse_luma(pr[0], 0, ps[0], 0, d_st, n, d_skip, damping, nhfb, d_sse[0], d_dir, None)
                for p in (1, 2):
                    ctx.cdef_search_sse_chroma(pr[p], 0, ps[p], 0, 1, 1, d_dir, d_st, n, d_skip, damping, nhfb, d_sse[p])

            t0 = time.perf_counter()                       # warm-up: both sides' kernels loaded, the work memory sized, the clocks up
            while time.perf_counter() - t0 < 0.25:
                one_call(); tables(); ctx.sync()
            host_s, want, levels = None, None, None
            new_ms, seq_ms, seq_dev_ms, tab_ms, pick_ms = [], [], [], [], []
            for rep in range(args.reps):
                ctx.sync()
                t0 = time.perf_counter()
                one_call()
                ctx.sync()
                t1 = time.perf_counter()
                got = (ctx.from_device(d_pick, (1,), capi.cdef_pick_dtype)[0], ctx.from_device(d_idx, (nvfb, nhfb), np.int8),
                       [ctx.from_device(d, (nvfb, nhfb), np.uint8) for d in d_lv])
                cnt = int(got[0]["sb_count"])
                # the sequence
                t2 = time.perf_counter()
                tables()
                ctx.sync()
                raw = [ctx.from_device(d, (n, nvfb, nhfb), np.uint64) for d in d_sse]
                t3 = time.perf_counter()
                if want is None:                           # the host logic: once, its time counted in every repetition
                    h0 = time.perf_counter()
                    want = M.search_frame(raw[0].astype(np.int64), raw[1].astype(np.int64), raw[2].astype(np.int64), skip, None, bd, strengths, method > 0, rdmult,
                                          vector=True)
                    flat = np.ascontiguousarray(want["fb_index"]).ravel()
                    levels = [np.zeros(flat.size, np.uint8) for _ in range(4)]
                    ys, uvs = np.asarray(want["cdef_strengths"], np.int32), np.asarray(want["cdef_uv_strengths"], np.int32)
                    vp = ctypes.c_void_p
                    assert capi.lib.aomhip_cdef_build_strengths(vp(flat.ctypes.data), ctypes.c_int(flat.size), vp(ys.ctypes.data), vp(uvs.ctypes.data),
                                                                *[vp(o.ctypes.data) for o in levels]) == 0
                    host_s = time.perf_counter() - h0
                t4 = time.perf_counter()
                for d, o in zip(d_up, levels):
                    ctx.memcpy_h2d(d, o)
                ctx.sync()
                t5 = time.perf_counter()
                ok = (int(got[0]["cdef_bits"]) == want["cdef_bits"] and [int(v) for v in got[0]["cdef_strengths"]] == want["cdef_strengths"] and
                      [int(v) for v in got[0]["cdef_uv_strengths"]] == want["cdef_uv_strengths"] and int(got[0]["best_rd"]) == want["best_rd"] and
                      cnt == want["sb_count"] and np.array_equal(got[1], want["fb_index"]) and
                      all(np.array_equal(g.ravel(), o) for g, o in zip(got[2], levels)))
                if not ok:
                    raise SystemExit("the call and the host-driven sequence differ at %s method %d\n%s\n%s" % (point, method, got[0], {k: want[k] for k in
                                                                                                                                   ("cdef_bits", "cdef_strengths",
                                                                                                                                    "cdef_uv_strengths", "best_rd",
                                                                                                                                    "sb_count")}))
                # the parts, each synchronised on its own
                t6 = time.perf_counter()
                tables()
                ctx.sync()
                t7 = time.perf_counter()
                ctx.memcpy_h2d(d_cnt, np.array([cnt], np.int32)); ctx.sync()
                t8 = time.perf_counter()
                ctx.cdef_pick_strengths(d_m0, d_m1, d_cnt, nfb, d_st, n, int(method > 0), rdmult, d_pick2, d_gi, None)
                ctx.sync()
                t9 = time.perf_counter()
                assert ctx.from_device(d_pick2, (1,), capi.cdef_pick_dtype)[0].tobytes() == got[0].tobytes()
                new_ms.append((t1 - t0) * 1e3)
                seq_dev_ms.append((t3 - t2 + t5 - t4) * 1e3); seq_ms.append((t3 - t2 + t5 - t4 + host_s) * 1e3)
                tab_ms.append((t7 - t6) * 1e3); pick_ms.append((t9 - t8) * 1e3)
            row = dict(width=W, height=H, bit_depth=bd, method=method, n_strengths=n, filter_blocks=nfb, entries=want["sb_count"], cdef_bits=want["cdef_bits"],
                       identical=True, new=stats(new_ms), sequence_wall=stats(seq_ms), sequence_without_host_python=stats(seq_dev_ms), host_python_ms=host_s * 1e3,
                       sse_tables_alone=stats(tab_ms), pick_alone=stats(pick_ms))
            row["factor_median"] = row["sequence_without_host_python"]["median_ms"] / row["new"]["median_ms"]
            row["tables_share_of_new"] = row["sse_tables_alone"]["median_ms"] / row["new"]["median_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            for d in [d_st, d_dir, d_idx, d_pick, d_m0, d_m1, d_efb, d_cnt, d_gi, d_pick2] + d_sse + d_lv + d_up:
                ctx.free(d)
        for p in pr + ps:
            ctx.planes_free(p)
        ctx.free(d_skip)
    rec = dict(tool="tools/cdef_pick_ab.py",
               timing="wall clock around synchronised calls, the call and the sequence alternating, after >= 0.25 s of warm-up rounds", reps=args.reps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
