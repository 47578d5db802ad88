"""search_tx_type on the device (csrc/tx_type_search.hip): aomhip_search_tx_type_batch against the interpreted reference's fixture and the
plain-integer model (tests/tx_type_model.py) -- table, visit trace, winner and stats, every stored case of every stored shape --, against the existing
entry points run type by type through the C ABI with the host doing the comparison, the winner's coefficients against
aomhip_subtract_xform_quant_ex_batch, one captured graph replayed on two frames, and the refused arguments.  Everything is compared exactly."""
import ctypes as C

import numpy as np
import pytest

import tx_type_model as M

pytestmark = pytest.mark.gpu

BORDER = 16
Z, CASES = M.golden()
SIZES = sorted({c["tx_size"] for c in CASES})


class Run:
    """The outputs of one device call, as numpy records."""

    def __init__(self, ctx, K, src, pred, frame, tx_size, q, d_costs, params, blocks, txk_map=None, coeffs=0):
        n = len(blocks)
        self.d = [ctx.to_device(blocks), ctx.malloc(n * 40), ctx.malloc(n * 16 * 32), ctx.malloc(n * 16), ctx.malloc(n * K.TX_SEARCH_TRACE_BYTES)]
        d_map = ctx.to_device(np.ascontiguousarray(txk_map, np.uint8)) if txk_map is not None else None
        d_q = d_dq = None
        if coeffs:
            d_q, d_dq = ctx.malloc(4 * coeffs), ctx.malloc(4 * coeffs)
            ctx.memset(d_q, 0x5A, 4 * coeffs); ctx.memset(d_dq, 0x5A, 4 * coeffs)
        for p, sz in zip(self.d[1:], (n * 40, n * 16 * 32, n * 16, n * K.TX_SEARCH_TRACE_BYTES)):
            ctx.memset(p, 0xA5, sz)
        self.args = (src, pred, frame, tx_size, K.QuantParams.from_tables(q), d_costs, params, self.d[0], n, self.d[1])
        self.kw = dict(d_txk_map=d_map, d_qcoeff=d_q, d_dqcoeff=d_dq, d_table=self.d[2], d_info=self.d[3], d_trace=self.d[4])
        self.ctx, self.K, self.n, self.coeffs, self.extra = ctx, K, n, coeffs, [p for p in (d_map, d_q, d_dq) if p]
        self.launch()
        self.fetch()

    def launch(self):
        self.ctx.search_tx_type_batch(*self.args, **self.kw)

    def fetch(self):
        ctx, K, n = self.ctx, self.K, self.n
        ctx.sync()
        self.result = ctx.from_device(self.d[1], (n,), K.tx_search_result_dtype)
        self.table = ctx.from_device(self.d[2], (n, 16), K.tx_type_entry_dtype)
        self.info = ctx.from_device(self.d[3], (n,), K.tx_search_info_dtype)
        self.trace = ctx.from_device(self.d[4], (n, K.TX_SEARCH_TRACE_BYTES), np.uint8)
        if self.coeffs:
            self.qcoeff = ctx.from_device(self.kw["d_qcoeff"], (self.coeffs,), np.int32)
            self.dqcoeff = ctx.from_device(self.kw["d_dqcoeff"], (self.coeffs,), np.int32)

    def close(self):
        for p in self.d + self.extra:
            self.ctx.free(p)


def check_block(run, i, info, tab, res, visited, tag):
    """block i of a device run against a model (or fixture) table, result and visit order"""
    di, dt, dr, tr = run.info[i], run.table[i], run.result[i], run.trace[i]
    assert (int(di["block_sse"]), int(di["block_mse_q8"]), int(di["use_transform_domain_distortion"]), int(di["calc_pixel_domain_distortion_final"])) == \
        (info["block_sse"], info["block_mse_q8"], info["use_txd"], info["calc_final"]), tag
    for t in range(16):
        e = tab[t]
        if e is None:
            assert int(dt[t]["valid"]) == 0, (tag, t)
            continue
        got = tuple(int(dt[t][k]) for k in ("valid", "rate", "eob", "txb_entropy_ctx", "dist", "sse", "px_dist"))
        assert got == (1, e["rate"], e["eob"], e["ctx"], e["dist"], e["sse"], e["px_dist"]), (tag, t)
    assert int(tr[0]) == len(visited) and [int(v) for v in tr[1:1 + len(visited)]] == visited and (tr[1 + len(visited):] == 255).all(), tag
    got = tuple(int(dr[k]) for k in ("best_tx_type", "best_eob", "txb_entropy_ctx", "rate", "dist", "sse", "skip_txfm", "best_rd"))
    assert got == (res["best_tx_type"], res["best_eob"], res["txb_entropy_ctx"], res["rate"], res["dist"], res["sse"], res["skip_txfm"], res["best_rd"]), tag


def block_record(K, x, y, c):
    b = np.zeros(1, K.tx_search_block_dtype)[0]
    b["x"], b["y"], b["ref_best_rd"], b["rdmult"] = x, y, c["ref_best_rd"], c["rdmult"]
    b["allowed_tx_mask"], b["visible_cols"], b["visible_rows"] = c["mask"], c["vis_cols"], c["vis_rows"]
    b["txk_allowed_single"], b["txb_skip_ctx"], b["dc_sign_ctx"] = int(c["single"] is not None), c["skip_ctx"], c["dc_ctx"]
    return b


def params_of(K, c, **kw):
    return K.TxSearchParams.make(tx_type_costs=c["tx_type_costs"], use_transform_domain_distortion=0 if c["psy"] else c["use_txd"],
                                 tx_domain_dist_threshold=c["threshold"], low_txfm_rd=c["low_txfm_rd"], adaptive_txb_search_level=c["adaptive"],
                                 skip_tx_search=c["skip_tx_search"], **kw)


@pytest.mark.parametrize("tx_size", SIZES)
def test_fixture_cases(hip, ctx, tx_size):
    """every stored case of the shape: the device's table, trace, winner and stats equal the interpreted reference's record and the model"""
    K = hip.capi
    w, h = M.TXW[tx_size], M.TXH[tx_size]
    planes = {bd: (ctx.planes_alloc(w + 8, h + 4, BORDER, bd, 1), ctx.planes_alloc(w + 8, h + 4, BORDER, bd, 1)) for bd in (8, 10, 12)}
    costs = {}
    n = 0
    for c in [c for c in CASES if c["tx_size"] == tx_size]:
        src, pred = planes[c["bd"]]
        inp = M.case_inputs(Z, c)
        x0, y0 = (4, 2) if c["k"] % 2 else (0, 0)   # (the tile at two places of the plane; the rest is never read)
        for ring, tile in ((src, inp["src"]), (pred, inp["pred"])):
            full = np.zeros((h + 4, w + 8), np.int64)
            full[y0:y0 + h, x0:x0 + w] = tile
            ctx.planes_upload(ring, 0, full)
        if c["costs"] not in costs:
            costs[c["costs"]] = ctx.to_device(np.ascontiguousarray(inp["costs"], np.int32))
        blocks = np.array([block_record(K, x0, y0, c)], K.tx_search_block_dtype)
        run = Run(ctx, K, src, pred, 0, tx_size, inp["q"], costs[c["costs"]], params_of(K, c), blocks, txk_map=[c["txk_map"]] if c["txk_map"] else None)
        info, tab, res, visited = M.model_case(Z, c)
        check_block(run, 0, info, tab, res, visited, c["k"])
        # ... and the record itself (the model is held to it on the CPU; here the device is, directly)
        assert [int(v) for v in run.trace[0][1:1 + int(run.trace[0][0])]] == c["visit"], c["k"]
        for t, (rate, eob, ectx, dist, sse) in c["types"].items():
            e = run.table[0][int(t)]
            assert (int(e["rate"]), int(e["eob"]), int(e["txb_entropy_ctx"]), int(e["dist"]), int(e["sse"])) == (rate, eob, ectx, int(dist), int(sse)), (c["k"], t)
        r = run.result[0]
        assert (int(r["best_tx_type"]), int(r["best_eob"]), int(r["txb_entropy_ctx"]), int(r["rate"]), int(r["dist"]), int(r["sse"]), int(r["skip_txfm"]),
                int(r["best_rd"])) == (c["best_tx_type"], c["best_eob"], c["best_ctx"], c["rate"], int(c["dist"]), int(c["sse"]), c["skip_txfm"], int(c["best_rd"])), c["k"]
        run.close()
        n += 1
    assert n >= 14
    for p in costs.values():
        ctx.free(p)
    for a, b in planes.values():
        ctx.planes_free(a); ctx.planes_free(b)


class Batch:
    """A frame pair with a grid of transform blocks (more than one workgroup, an odd count), per-block masks, orders, contexts and multipliers."""

    def __init__(self, hip, ctx, oracle, tx_size, bd, n_frames=1, seed=5, clip=None):
        self.K, self.ctx, self.orc, self.tx_size, self.bd = hip.capi, ctx, oracle, tx_size, bd
        K = self.K
        w, h = M.TXW[tx_size], M.TXH[tx_size]
        self.w, self.h, self.nc = w, h, min(w, 32) * min(h, 32)
        cols, rows = (7, 5) if w * h <= 256 else (3, 3)
        if max(w, h) == 64:
            cols, rows = 3, 1
        self.W, self.H = cols * w + 3, rows * h + 2
        rng = np.random.default_rng(seed + tx_size * 7 + bd)
        self.rng = rng
        self.src, self.pred = ctx.planes_alloc(self.W, self.H, BORDER, bd, n_frames), ctx.planes_alloc(self.W, self.H, BORDER, bd, n_frames)
        self.q = oracle.build_quantizer_y(bd, 110)
        self.costs = rng.integers(10, 4000, 966).astype(np.int32)
        self.d_costs = ctx.to_device(self.costs)
        self.tx_type_costs = [0] * 16 if max(w, h) == 64 else [int(v) for v in rng.integers(0, 1200, 16)]
        sm = 0x0001 if max(w, h) == 64 else (0x0201 if max(w, h) == 32 else (0x0FFF if max(w, h) == 16 else 0xFFFF))
        n = cols * rows
        self.n = n
        self.blocks = np.zeros(n, K.tx_search_block_dtype)
        self.maps = np.zeros((n, 16), np.uint8)
        for i in range(n):
            b = self.blocks[i]
            b["x"], b["y"] = (i % cols) * w + 3, (i // cols) * h + 2      # (off the grid's origin: unaligned rows)
            b["ref_best_rd"] = int(rng.choice([M.INT64_MAX, 1 << 20, 5000]))
            b["rdmult"] = int(rng.choice([90, 700, 1 << 21]))
            b["out_offset"] = (n - 1 - i) * self.nc                       # (not the natural order)
            m = sm if i % 3 == 0 else (int(rng.integers(1, 1 << 16)) & sm or 1)
            b["allowed_tx_mask"] = m
            b["visible_cols"], b["visible_rows"] = clip if clip else (w, h)
            b["txk_allowed_single"] = int(i % 11 == 5)
            b["txb_skip_ctx"], b["dc_sign_ctx"] = int(rng.integers(0, 13)), int(rng.integers(0, 3))
            p = rng.permutation(16)
            self.maps[i] = np.where(rng.random(16) < 0.15, 255, p) if i % 2 else np.arange(16)
            if not any(int(t) < 16 and (int(m) >> int(t)) & 1 for t in self.maps[i]):
                self.maps[i][0] = int(m).bit_length() - 1

    def content(self, seed):
        rng = np.random.default_rng(seed)
        mx = (1 << self.bd) - 1
        pred = rng.integers(mx // 4, 3 * mx // 4, (self.H, self.W))
        amp = np.repeat(np.repeat(rng.choice([0, 2, 12, 60], (self.H // 4 + 1, self.W // 4 + 1)), 4, 0), 4, 1)[:self.H, :self.W] << (self.bd - 8)
        src = np.clip(pred + (rng.integers(-1, 2, pred.shape) * amp) + (np.add.outer(np.arange(self.H), np.arange(self.W)) % 5) * (amp // 3), 0, mx)
        return src, pred

    def upload(self, frame, src, pred):
        self.ctx.planes_upload(self.src, frame, src); self.ctx.planes_upload(self.pred, frame, pred)

    def params(self, use_txd, **kw):
        return self.K.TxSearchParams.make(tx_type_costs=self.tx_type_costs, use_transform_domain_distortion=use_txd, tx_domain_dist_threshold=kw.pop("threshold", 22 * 256),
                                          adaptive_txb_search_level=kw.pop("adaptive", 1), skip_tx_search=kw.pop("skip_tx_search", 1), **kw)

    def model(self, src, pred, prm, i, tab=None, info=None):
        b = self.blocks[i]
        x, y = int(b["x"]), int(b["y"])
        s, p = src[y:y + self.h, x:x + self.w], pred[y:y + self.h, x:x + self.w]
        vc, vr, mask = int(b["visible_cols"]), int(b["visible_rows"]), int(b["allowed_tx_mask"])
        if info is None:
            info = M.block_scalars(s, p, self.tx_size, self.bd, vc, vr, mask, int(b["txk_allowed_single"]), prm.use_transform_domain_distortion,
                                   prm.tx_domain_dist_threshold, prm.low_txfm_rd)
        if tab is None:
            tab = M.table(s, p, self.tx_size, self.bd, self.q, self.costs, self.tx_type_costs, int(b["txb_skip_ctx"]), int(b["dc_sign_ctx"]), vc, vr, mask, info)
        res, visited = M.walk(tab, info, mask, self.maps[i], int(b["rdmult"]), int(b["ref_best_rd"]), prm.adaptive_txb_search_level, prm.skip_tx_search)
        return info, tab, res, visited

    def close(self):
        self.ctx.free(self.d_costs)
        self.ctx.planes_free(self.src); self.ctx.planes_free(self.pred)


def composition_tables(bt, src, pred, prm):
    """The parent commit's entry points, type by type through the C ABI, the host assembling each block's table from what they return."""
    ctx, K, n, nc, tx_size = bt.ctx, bt.K, bt.n, bt.nc, bt.tx_size
    vc, vr = int(bt.blocks[0]["visible_cols"]), int(bt.blocks[0]["visible_rows"])
    qp = K.QuantParams.from_tables(bt.q)
    rec = ctx.planes_alloc(bt.W, bt.H, BORDER, bt.bd, 1)
    cands = np.zeros(n, K.sad_cand_dtype)
    cands["sx"], cands["sy"], cands["rx"], cands["ry"] = bt.blocks["x"], bt.blocks["y"], bt.blocks["x"], bt.blocks["y"]
    tctx = np.stack([bt.blocks["txb_skip_ctx"], bt.blocks["dc_sign_ctx"]], 1).astype(np.uint8)
    d_cands, d_tctx = ctx.to_device(cands), ctx.to_device(tctx)
    d_q, d_dq, d_eob, d_err = ctx.malloc(4 * n * nc), ctx.malloc(4 * n * nc), ctx.malloc(2 * n), ctx.malloc(16 * n)
    d_cost, d_ectx, d_sse = ctx.malloc(4 * n), ctx.malloc(n), ctx.malloc(8 * n)
    ctx.sse_batch(bt.src, bt.pred, 0, vc, vr, d_cands, n, d_sse)
    ctx.sync()
    sse0 = ctx.from_device(d_sse, (n,), np.int64)
    infos = [M.block_scalars(None, None, tx_size, bt.bd, vc, vr, int(b["allowed_tx_mask"]), int(b["txk_allowed_single"]), prm.use_transform_domain_distortion,
                             prm.tx_domain_dist_threshold, prm.low_txfm_rd, sse=int(sse0[i])) for i, b in enumerate(bt.blocks)]
    tabs = [[None] * 16 for _ in range(n)]
    coeffs = {}
    for t in range(16):
        if not M.tx_type_exists(tx_size, t) or not any((int(b["allowed_tx_mask"]) >> t) & 1 for b in bt.blocks):
            continue
        txb = np.zeros(n, K.txb_dtype)
        txb["x"], txb["y"], txb["out_offset"], txb["tx_type"] = bt.blocks["x"], bt.blocks["y"], np.arange(n) * nc, t
        d_txb = ctx.to_device(txb)
        ctx.subtract_xform_quant_ex_batch(bt.src, bt.pred, 0, tx_size, d_txb, n, 0, 0, qp, 0, None, d_q, d_dq, d_eob, d_err)
        ctx.cost_coeffs_txb_batch(d_q, tx_size, d_txb, n, 0, d_eob, d_tctx, bt.d_costs, d_cost)
        ctx.txb_entropy_context_batch(d_q, tx_size, d_txb, n, 0, d_eob, d_ectx)
        ctx.planes_upload(rec, 0, pred)
        ctx.inv_txfm_add_batch(d_dq, tx_size, d_txb, n, 0, 0, d_eob, rec, 0)
        ctx.sse_batch(bt.src, rec, 0, vc, vr, d_cands, n, d_sse)
        ctx.sync()
        eob, err = ctx.from_device(d_eob, (n,), np.uint16), ctx.from_device(d_err, (n, 2), np.int64)
        cost, ectx, sse = ctx.from_device(d_cost, (n,), np.int32), ctx.from_device(d_ectx, (n,), np.uint8), ctx.from_device(d_sse, (n,), np.int64)
        coeffs[t] = (ctx.from_device(d_q, (n, nc), np.int32), ctx.from_device(d_dq, (n, nc), np.int32))
        for i, b in enumerate(bt.blocks):
            if (int(b["allowed_tx_mask"]) >> t) & 1:
                rate = int(cost[i]) + (bt.tx_type_costs[t] if eob[i] else 0)
                tabs[i][t] = M.entry_from_parts(tx_size, bt.bd, infos[i], int(eob[i]), rate, int(ectx[i]), int(err[i][0]), int(err[i][1]), lambda i=i: int(sse[i]))
        ctx.free(d_txb)
    for p in (d_cands, d_tctx, d_q, d_dq, d_eob, d_err, d_cost, d_ectx, d_sse):
        ctx.free(p)
    ctx.planes_free(rec)
    return infos, tabs, coeffs


@pytest.mark.parametrize("tx_size,bd,use_txd,clip", [(0, 8, 0, None), (1, 10, 1, None), (2, 8, 0, (13, 16)), (2, 12, 2, None), (3, 8, 1, (32, 7)), (4, 10, 0, None),
                                                    (17, 8, 0, (16, 33)), (13, 10, 1, (3, 16)), (14, 12, 0, None), (15, 8, 2, None)])
def test_batch_against_model_and_composition(hip, oracle, ctx, tx_size, bd, use_txd, clip):
    """a grid of blocks with their own masks, orders and multipliers: the device call equals the model, equals the existing entry points composed type by
    type with the host comparing, and its winner's coefficients are aomhip_subtract_xform_quant_ex_batch's for that type"""
    bt = Batch(hip, ctx, oracle, tx_size, bd, clip=clip)
    src, pred = bt.content(3)
    bt.upload(0, src, pred)
    prm = bt.params(use_txd)
    run = Run(ctx, bt.K, bt.src, bt.pred, 0, tx_size, bt.q, bt.d_costs, prm, bt.blocks, txk_map=bt.maps, coeffs=bt.n * bt.nc)
    infos, tabs, coeffs = composition_tables(bt, src, pred, prm)
    winners = set()
    for i in range(bt.n):
        info, tab, res, visited = bt.model(src, pred, prm, i)
        check_block(run, i, info, tab, res, visited, ("model", i))
        _, _, res_c, visited_c = bt.model(src, pred, prm, i, tab=tabs[i], info=infos[i])
        check_block(run, i, infos[i], tabs[i], res_c, visited_c, ("composition", i))
        t, off = res["best_tx_type"], int(bt.blocks[i]["out_offset"])
        assert np.array_equal(run.qcoeff[off:off + bt.nc], coeffs[t][0][i]) and np.array_equal(run.dqcoeff[off:off + bt.nc], coeffs[t][1][i]), i
        winners.add(t)
    assert len(winners) > 1 or max(bt.w, bt.h) == 64
    run.close()
    bt.close()


def test_identity_order_when_no_map_is_given(hip, oracle, ctx):
    bt = Batch(hip, ctx, oracle, 1, 8)
    src, pred = bt.content(9)
    bt.upload(0, src, pred)
    bt.maps[:] = np.arange(16)
    prm = bt.params(0, adaptive=0, skip_tx_search=0)
    run = Run(ctx, bt.K, bt.src, bt.pred, 0, 1, bt.q, bt.d_costs, prm, bt.blocks, txk_map=None)
    for i in range(bt.n):
        check_block(run, i, *bt.model(src, pred, prm, i), tag=i)
    run.close()
    bt.close()


def test_capture_once_replay_twice(hip, oracle, ctx):
    """one captured graph of the call (table, walk, the winner's coefficients) replayed on two frames with different content: each frame's own answer"""
    bt = Batch(hip, ctx, oracle, 2, 10)
    frames = [bt.content(21), bt.content(22)]
    bt.upload(0, *frames[0])
    prm = bt.params(1)
    run = Run(ctx, bt.K, bt.src, bt.pred, 0, 2, bt.q, bt.d_costs, prm, bt.blocks, txk_map=bt.maps, coeffs=bt.n * bt.nc)   # (the warm-up call)
    g = ctx.capture(run.launch)
    answers = []
    for src, pred in (frames[1], frames[0]):
        bt.upload(0, src, pred)
        for p, sz in zip(run.d[1:], (bt.n * 40, bt.n * 16 * 32, bt.n * 16, bt.n * bt.K.TX_SEARCH_TRACE_BYTES)):
            ctx.memset(p, 0xA5, sz)
        ctx.graph_launch(g)
        run.fetch()
        for i in range(bt.n):
            info, tab, res, visited = bt.model(src, pred, prm, i)
            check_block(run, i, info, tab, res, visited, ("replay", i))
            off = int(bt.blocks[i]["out_offset"])
            b = bt.blocks[i]
            e = M.evaluate_type(src[int(b["y"]):int(b["y"]) + bt.h, int(b["x"]):int(b["x"]) + bt.w], pred[int(b["y"]):int(b["y"]) + bt.h, int(b["x"]):int(b["x"]) + bt.w],
                                2, res["best_tx_type"], bt.bd, bt.q, bt.costs, 0, int(b["txb_skip_ctx"]), int(b["dc_sign_ctx"]), bt.w, bt.h, info, want_coeffs=True)
            assert np.array_equal(run.qcoeff[off:off + bt.nc], e["qcoeff"]) and np.array_equal(run.dqcoeff[off:off + bt.nc], e["dqcoeff"]), i
        answers.append([int(v) for v in run.result["best_rd"]])
    assert answers[0] != answers[1]
    ctx.graph_destroy(g)
    run.close()
    bt.close()


def test_refused_arguments_launch_nothing(hip, oracle, ctx):
    K = hip.capi
    lib = K.lib
    bt = Batch(hip, ctx, oracle, 2, 8)
    bt.upload(0, *bt.content(1))
    other_depth, other_size = ctx.planes_alloc(bt.W, bt.H, BORDER, 10, 1), ctx.planes_alloc(bt.W + 8, bt.H, BORDER, 8, 1)
    d_blocks, d_res = ctx.to_device(bt.blocks), ctx.malloc(bt.n * 40)
    d_co = ctx.malloc(4 * bt.n * bt.nc)
    ctx.memset(d_res, 0xA5, bt.n * 40)
    qp, prm = K.QuantParams.from_tables(bt.q), bt.params(0)

    def call(src=bt.src, pred=bt.pred, frame=0, tx_size=2, qp_=C.byref(qp), costs=bt.d_costs, prm_=None, blocks=d_blocks, res=d_res, q=None, dq=None):
        p = prm if prm_ is None else prm_
        return lib.aomhip_search_tx_type_batch(ctx.h, C.byref(src) if src is not None else None, C.byref(pred) if pred is not None else None, frame, tx_size, qp_, costs,
                                               C.byref(p) if p is not False else None, blocks, None, bt.n, res, q, dq, None, None, None)
    bad = [call(pred=other_depth), call(pred=other_size), call(frame=1), call(frame=-1), call(tx_size=19), call(tx_size=-1),
           call(prm_=bt.params(0, tx_mask_limit=0)), call(tx_size=4, prm_=bt.params(0, tx_mask_limit=0xFFFE)), call(tx_size=3, prm_=bt.params(0, tx_mask_limit=0x01FE)),
           call(src=None), call(pred=None), call(qp_=None), call(costs=None), call(prm_=False), call(blocks=None), call(res=None), call(q=d_co), call(dq=d_co)]
    for name in ("predict_dc_level", "enable_trellis", "use_qmatrix", "quant_b_adapt", "lossless", "is_intra"):
        bad.append(call(prm_=bt.params(0, **{name: 1})))
    bad.append(call(prm_=bt.params(3)))
    assert all(rc == K.ERR_INVALID for rc in bad), bad
    ctx.sync()
    assert (ctx.from_device(d_res, (bt.n * 40,), np.uint8) == 0xA5).all()
    assert call() == K.OK
    ctx.sync()
    assert not (ctx.from_device(d_res, (bt.n * 40,), np.uint8) == 0xA5).all()
    # a block whose own mask holds no type of the size: reported by the next synchronisation, the block gets no winner
    blocks = bt.blocks.copy()
    blocks["allowed_tx_mask"][1] = 0
    ctx.memcpy_h2d(d_blocks, blocks)
    assert call() == K.OK
    with pytest.raises(K.AomHipError):
        ctx.sync()
    assert int(ctx.from_device(d_res, (bt.n,), K.tx_search_result_dtype)["best_tx_type"][1]) == 255
    ctx.sync()
    for p in (d_blocks, d_res, d_co):
        ctx.free(p)
    ctx.planes_free(other_depth); ctx.planes_free(other_size)
    bt.close()
