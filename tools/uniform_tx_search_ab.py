"""A/B of the uniform transform-size search (three depths, every type of each size's set allowed): the one device call
(aomhip_pick_uniform_tx_size_type_yrd_batch) against the same search driven from the host through aomhip_search_tx_type_batch -- the parent's entry
point -- one call per transform-block position and depth, on the same seeded frames, in one process:

    python tools/uniform_tx_search_ab.py [--reps 5] [--out profiles/uniform_tx_search_ab.json]       (AOMHIP_LIB selects the library)

Points: every 16x16 and every 64x64 luma block that lies wholly inside the frame's mode-info extent of 1920x1080 8-bit and 3840x2160 10-bit; rdmult
80 .. 900, qindex 120, ref_best_rd = INT64_MAX (every transform block of every depth is searched), incoming entropy contexts taken from a previous
call's output (each block's own outgoing contexts).
  (a) the new call: wall clock with the context synchronised, and its device time between two events
  (b) the composition: per depth, per transform-block position k in visiting order (1 + 4 + 16 positions), the host derives every block's TXB_CTX and
      budget from its running contexts (numpy over all blocks), uploads the list, calls aomhip_search_tx_type_batch, downloads the winners, merges and
      updates the contexts; then av1_uniform_txfm_yrd's tail and the depth decision.  Wall clock for all of it.
  (c) the composition's DEVICE SHARE alone: the same launches on the lists of the last round between two events per call, no transfers, no host work.
Timing follows the measuring guide: >= 0.25 s of warm-up rounds that keep the device busy, then medians of `reps` alternating repetitions; the spread
(max - min over the repetitions) is reported with every figure.  Both sides must agree on every block's size, stats, visiting count and winning types or
the tool fails."""
import argparse
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

TXW = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TXH = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
BSIZE = {16: 6, 64: 12}   # BLOCK_16X16, BLOCK_64X64
INT64_MAX = (1 << 63) - 1
SKIP_CONTEXTS = np.array([[1, 2, 2, 2, 3], [2, 4, 4, 4, 5], [2, 4, 4, 4, 5], [2, 4, 4, 4, 5], [3, 5, 5, 5, 6]], np.uint8)


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


def rdcost(rdmult, rate, dist):
    return ((rate * rdmult + 256) >> 9) + dist * 128


def all_types(tx):
    lim = {0: 64, 1: 16, 2: 16, 3: 32}
    vk = [0, 1, 0, 1, 2, 0, 2, 1, 2, 3, 0, 3, 1, 3, 2, 3]
    hk = [0, 0, 1, 1, 0, 2, 2, 2, 1, 3, 3, 0, 3, 1, 3, 2]
    return sum(1 << t for t in range(16) if TXH[tx] <= lim[vk[t]] and TXW[tx] <= lim[hk[t]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uniform_tx_search_ab.json"))
    ap.add_argument("--points", default="1920x1080x8,3840x2160x10")
    ap.add_argument("--sizes", default="16,64")
    ap.add_argument("--only-new", action="store_true", help="run the new call alone (for a kernel trace)")
    args = ap.parse_args()
    import pyoracle as orc
    ctx = capi.Context(0)
    BORDER = 64
    rows_out = []
    for point in args.points.split(","):
        W, H, bd = (int(v) for v in point.split("x"))
        rng = np.random.default_rng(W + bd)
        ps, pp = ctx.planes_alloc(W, H, BORDER, bd, 1), ctx.planes_alloc(W, H, BORDER, bd, 1)
        src, pred = content(rng, W, H, bd)
        ctx.planes_upload(ps, 0, src); ctx.planes_upload(pp, 0, pred)
        q = orc.build_quantizer_y(bd, 120)
        qp = capi.QuantParams.from_tables(q)
        for bs in (int(v) for v in args.sizes.split(",")):
            bsize = BSIZE[bs]
            cols, rows = ((W + 7) & ~7) // bs, ((H + 7) & ~7) // bs
            n = cols * rows
            plan = capi.uniform_tx_depth_plan(bsize, 1, 0, 0, 1, 1, 0)
            entries = plan.entries()
            assert len(entries) == 3
            blocks = np.zeros(n, capi.uniform_tx_block_dtype)
            blocks["x"], blocks["y"] = (np.arange(n) % cols) * bs, (np.arange(n) // cols) * bs
            blocks["rdmult"], blocks["source_variance"], blocks["ref_best_rd"] = rng.integers(80, 900, n), rng.choice([40, 200, 900, 5000], n), INT64_MAX
            blocks["tx_size_rate"] = rng.integers(50, 900, (n, 3))
            blocks["no_skip_txfm_rate"], blocks["skip_txfm_rate"] = rng.integers(20, 600, n), rng.integers(200, 3000, n)
            d_blocks, d_stats, d_txb = ctx.to_device(blocks), ctx.malloc(56 * n), ctx.malloc(4 * 64 * n)
            prms, d_costs, tcosts = [], [], []
            for _, tx in entries:
                tc = [0] * 16 if max(TXW[tx], TXH[tx]) == 64 else [int(v) for v in rng.integers(0, 1200, 16)]
                tcosts.append(tc)
                prms.append(capi.TxSearchParams.make(tx_type_costs=tc, tx_mask_limit=all_types(tx)))
                d_costs.append(ctx.to_device(rng.integers(10, 4000, 966).astype(np.int32)))
            depths = capi.uniform_tx_depths([(prms[k], d_costs[k], None, None) for k in range(3)])

            def one_call():
                ctx.pick_uniform_tx_size_type_yrd_batch(ps, pp, 0, bsize, plan, qp, depths, d_blocks, n, d_stats, d_txb)

            def fetch():
                ctx.sync()
                return ctx.from_device(d_stats, (n,), capi.uniform_tx_stats_dtype), ctx.from_device(d_txb, (n, 64), capi.uniform_tx_txb_dtype)

            orders = []
            for _, tx in entries:   # every block is whole: one visiting order per size (raster; a 64x64 block is one 64x64 unit)
                orders.append([(r, c) for r in range(0, bs // 4, TXH[tx] // 4) for c in range(0, bs // 4, TXW[tx] // 4)])

            # incoming contexts from a previous call's output: each block's own outgoing contexts under all-zero incoming ones
            one_call()
            st0, tb0 = fetch()
            for i in range(n):
                tx = int(st0["tx_size"][i])
                if tx == 255:
                    continue
                k = [e[1] for e in entries].index(tx)
                for j, (r, c) in enumerate(orders[k][:int(st0["n_txb"][i])]):
                    blocks["above_ctx"][i, c:c + TXW[tx] // 4] = tb0["txb_entropy_ctx"][i, j]
                    blocks["left_ctx"][i, r:r + TXH[tx] // 4] = tb0["txb_entropy_ctx"][i, j]
            ctx.memcpy_h2d(d_blocks, blocks)

            n_steps = sum(len(o) for o in orders)
            d_lists = [[ctx.malloc(32 * n) for _ in o] for o in orders]
            d_res = ctx.malloc(40 * n)
            rdmult = blocks["rdmult"].astype(np.int64)

            def composition():
                """the search driven from the host -> (tx_size, rd, rate, dist, sse, skip, n_txb, types of the winning depth [n][64])"""
                best = dict(tx_size=np.full(n, 255, np.int64), rd=np.full(n, INT64_MAX, np.int64), rate=np.full(n, (1 << 31) - 1, np.int64),
                            dist=np.full(n, INT64_MAX, np.int64), sse=np.full(n, INT64_MAX, np.int64), skip=np.zeros(n, np.int64), n_txb=np.zeros(n, np.int64),
                            types=np.full((n, 64), 255, np.int64))
                stop = np.zeros(n, bool)
                rd_prev = None
                for k, (depth, tx) in enumerate(entries):
                    w4, h4 = TXW[tx] // 4, TXH[tx] // 4
                    above, left = blocks["above_ctx"].copy(), blocks["left_ctx"].copy()
                    tsr = blocks["tx_size_rate"][:, k].astype(np.int64)
                    cur = np.minimum(rdcost(rdmult, blocks["no_skip_txfm_rate"] + tsr, 0), rdcost(rdmult, blocks["skip_txfm_rate"].astype(np.int64), 0))
                    rate, dist, sse, skip = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.ones(n, np.int64)
                    types = np.full((n, 64), 255, np.int64)
                    lst = np.zeros(n, capi.tx_search_block_dtype)
                    lst["rdmult"], lst["allowed_tx_mask"], lst["visible_cols"], lst["visible_rows"] = blocks["rdmult"], 0xFFFF, TXW[tx], TXH[tx]
                    for j, (r, c) in enumerate(orders[k]):
                        a, l = above[:, c:c + w4], left[:, r:r + h4]
                        sign = lambda v: (v >> 3 == 2).astype(np.int64) - (v >> 3 == 1).astype(np.int64)
                        dc = sign(a).sum(1) + sign(l).sum(1)
                        top, lft = np.minimum(np.bitwise_or.reduce(a, 1) & 7, 4), np.minimum(np.bitwise_or.reduce(l, 1) & 7, 4)
                        lst["x"], lst["y"] = blocks["x"] + c * 4, blocks["y"] + r * 4
                        lst["ref_best_rd"] = INT64_MAX - cur
                        lst["txb_skip_ctx"] = 0 if len(orders[k]) == 1 else SKIP_CONTEXTS[top, lft]
                        lst["dc_sign_ctx"] = np.where(dc < 0, 1, np.where(dc > 0, 2, 0))
                        ctx.memcpy_h2d(d_lists[k][j], lst)
                        ctx.search_tx_type_batch(ps, pp, 0, tx, qp, d_costs[k], prms[k], d_lists[k][j], n, d_res)
                        ctx.sync()
                        res = ctx.from_device(d_res, (n,), capi.tx_search_result_dtype)
                        above[:, c:c + w4] = res["txb_entropy_ctx"][:, None]
                        left[:, r:r + h4] = res["txb_entropy_ctx"][:, None]
                        r_, d_, s_ = res["rate"].astype(np.int64), res["dist"], res["sse"]
                        cur = cur + np.minimum(rdcost(rdmult, r_, d_), rdcost(rdmult, 0, s_))
                        rate, dist, sse, skip = rate + r_, dist + d_, sse + s_, skip & (res["best_eob"] == 0)
                        types[:, j] = res["best_tx_type"]
                    nsk = blocks["no_skip_txfm_rate"].astype(np.int64)
                    forced = rdcost(rdmult, blocks["skip_txfm_rate"].astype(np.int64), sse)
                    rd = np.where(skip == 1, forced, rdcost(rdmult, rate + nsk + tsr, dist))
                    rate = np.where(skip == 1, rate, rate + tsr)
                    take = (skip == 0) & (forced <= rd)
                    rd, rate, dist, skip = np.where(take, forced, rd), np.where(take, 0, rate), np.where(take, sse, dist), np.where(take, 1, skip)
                    rd = np.where(stop, INT64_MAX, rd)
                    wins = rd < best["rd"]
                    for name, v in (("tx_size", tx), ("rd", rd), ("rate", rate), ("dist", dist), ("sse", sse), ("skip", skip), ("n_txb", len(orders[k]))):
                        best[name] = np.where(wins, v, best[name])
                    best["types"][wins] = types[wins]
                    if depth == 1 and plan.init_depth == 0:
                        stop |= (blocks["source_variance"] < 256) & (rd_prev != INT64_MAX) & (rd > rd_prev)
                    rd_prev = rd
                return best

            def device_share():
                dev = 0.0
                for k, (_, tx) in enumerate(entries):
                    for j in range(len(orders[k])):
                        ctx.timer_begin()
                        ctx.search_tx_type_batch(ps, pp, 0, tx, qp, d_costs[k], prms[k], d_lists[k][j], n, d_res)
                        dev += ctx.timer_end()
                return dev

            t0 = time.perf_counter()                         # warm-up: kernels loaded, work memory sized, the clocks up
            while time.perf_counter() - t0 < 0.25:
                one_call(); ctx.sync()
            new_ms, new_dev_ms, seq_ms, seq_dev_ms = [], [], [], []
            for rep in range(args.reps):
                ctx.sync()
                t0 = time.perf_counter()
                one_call()
                ctx.sync()
                new_ms.append((time.perf_counter() - t0) * 1e3)
                ctx.timer_begin()
                one_call()
                new_dev_ms.append(ctx.timer_end())
                st, tb = fetch()
                if args.only_new:
                    continue
                t0 = time.perf_counter()
                best = composition()
                seq_ms.append((time.perf_counter() - t0) * 1e3)
                same = all(np.array_equal(st[a].astype(np.int64), best[b]) for a, b in (("tx_size", "tx_size"), ("rd", "rd"), ("rate", "rate"), ("dist", "dist"),
                                                                                         ("sse", "sse"), ("skip_txfm", "skip"), ("n_txb", "n_txb")))
                live = np.arange(64)[None, :] < best["n_txb"][:, None]
                same = same and np.array_equal(np.where(live, tb["tx_type"], 255), np.where(live, best["types"], 255))
                if not same:
                    raise SystemExit("the call and the composition differ at %s, %dx%d blocks" % (point, bs, bs))
                seq_dev_ms.append(device_share())
            row = dict(width=W, height=H, bit_depth=bd, block_size="%dx%d" % (bs, bs), blocks=n, tx_sizes=[e[1] for e in entries], search_tx_type_calls=n_steps,
                       new_wall=stats(new_ms), new_device=stats(new_dev_ms))
            if not args.only_new:
                sizes, counts = np.unique(st["tx_size"], return_counts=True)
                row.update(identical=True, winners_by_tx_size={int(s): int(c) for s, c in zip(sizes, counts)}, composition_wall=stats(seq_ms),
                           composition_device_share=stats(seq_dev_ms))
                row["factor_wall"] = row["composition_wall"]["median_ms"] / row["new_wall"]["median_ms"]
                row["factor_device_share"] = row["composition_device_share"]["median_ms"] / row["new_device"]["median_ms"]
                row["margin_ms"] = max(row["new_device"]["spread_ms"], row["composition_device_share"]["spread_ms"])
                row["wall_margin_ms"] = max(row["new_wall"]["spread_ms"], row["composition_wall"]["spread_ms"])
                row["new_wall_below_composition"] = bool(row["new_wall"]["median_ms"] + row["wall_margin_ms"] < row["composition_wall"]["median_ms"])
                row["new_within_device_share"] = bool(row["new_device"]["median_ms"] <= row["composition_device_share"]["median_ms"] + row["margin_ms"])
            rows_out.append(row)
            print(json.dumps(row), flush=True)
            for d in [d_blocks, d_stats, d_txb, d_res] + d_costs + [p for ds in d_lists for p in ds]:
                ctx.free(d)
        ctx.planes_free(ps); ctx.planes_free(pp)
    if not args.only_new:
        rec = dict(tool="tools/uniform_tx_search_ab.py", timing="wall clock around synchronised calls and event pairs around launches, the call and the composition "
                   "alternating, after >= 0.25 s of warm-up rounds; the composition's host share is numpy over all blocks", reps=args.reps, rows=rows_out)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
