"""The uniform transform-size search on the device (csrc/tx_size_search.hip): aomhip_uniform_txfm_yrd_batch and aomhip_pick_uniform_tx_size_type_yrd_batch
against the plain-integer model (tests/uniform_tx_model.py, which evaluates every transform block under its real entropy contexts) on fresh random
batches at the smallest shapes that reach each path -- blocks crossing the right and the bottom frame edge, 4:1 sizes, a 128-class size --, against the
parent's aomhip_search_tx_type_batch driven transform block by transform block with the host carrying contexts and budget, one captured graph replayed on
two frames, the winner's coefficients against aomhip_subtract_xform_quant_ex_batch, a batch in which the contexts change winning types, the refused
arguments and the device status of a transform block without an allowed type.  Everything is compared exactly."""
import ctypes as C

import numpy as np
import pytest

import tx_type_model as M
import uniform_tx_model as U

pytestmark = pytest.mark.gpu

BORDER = 64   # covers a 64-point transform block whose first 4 columns are all that is left of the frame
ALL_TYPES_OF = lambda tx: sum(1 << t for t in range(16) if M.tx_type_exists(tx, t))


class Frame:
    """A frame pair covered by prediction blocks of one size (the last column and row cross the frame's edges where the size does not divide it), each with
    its own multiplier, budget, header rates and incoming contexts; per plan entry its own cost table, type costs and per-transform-block masks."""

    def __init__(self, hip, ctx, oracle, bw, bh, W, H, bd, plan_args=(1, None, 0, 1, 1, 0), n_frames=1, seed=3, origin=(0, 0), budgets=(M.INT64_MAX, 1 << 33, 1 << 28, 1 << 24, 900),
                 use_txd=0, masks=True, rdmults=(80, 300, 900, 1 << 17)):
        K = self.K = hip.capi
        self.ctx, self.bw, self.bh, self.W, self.H, self.bd = ctx, bw, bh, W, H, bd
        self.bsize = U.bsize_of(bw, bh)
        rng = self.rng = np.random.default_rng(seed * 131 + bw * 7 + bh + bd)
        self.src, self.pred = ctx.planes_alloc(W, H, BORDER, bd, n_frames), ctx.planes_alloc(W, H, BORDER, bd, n_frames)
        self.q = oracle.build_quantizer_y(bd, 120)
        self.qp = K.QuantParams.from_tables(self.q)
        # (tx_select, mode_tx_size (None: tx_size_from_tx_mode under TX_MODE_LARGEST), init_depth, enable_tx64, enable_rect_tx, use_largest)
        tx_select, mode_tx, init_depth, tx64, rect, largest = plan_args
        mode_tx = U.max_rect_tx(self.bsize) if mode_tx is None else mode_tx
        self.plan_c = K.uniform_tx_depth_plan(self.bsize, tx_select, mode_tx, init_depth, tx64, rect, largest)
        self.plan = U.depth_plan(self.bsize, tx_select, mode_tx, init_depth, tx64, rect, largest)
        assert self.plan_c.entries() == self.plan["entries"] and self.plan_c.init_depth == self.plan["init_depth"]
        xs, ys = range(origin[0], W, bw), range(origin[1], H, bh)
        n = self.n = len(xs) * len(ys)
        self.blocks = np.zeros(n, K.uniform_tx_block_dtype)
        for i, (y, x) in enumerate((y, x) for y in ys for x in xs):
            b = self.blocks[i]
            b["x"], b["y"], b["rdmult"] = x, y, int(rng.choice(rdmults))
            b["source_variance"] = int(rng.choice([10, 255, 256, 4000]))
            b["ref_best_rd"] = int(budgets[i % len(budgets)])
            b["tx_size_rate"] = rng.integers(0, 900, 3)
            b["no_skip_txfm_rate"], b["skip_txfm_rate"] = int(rng.integers(20, 600)), int(rng.integers(200, 3000)) if i % 4 else 25
            for name in ("above_ctx", "left_ctx"):
                kind = i % 3   # all zero / small levels / anything, signs included
                lv = np.zeros(32, np.int64) if kind == 0 else rng.integers(0, 4 if kind == 1 else 8, 32)
                sg = np.zeros(32, np.int64) if kind == 0 else rng.integers(0, 3, 32)
                b[name] = lv | (sg << 3)
        self.d_blocks = ctx.to_device(self.blocks)
        self.dps, self.prms, self.dev = [], [], []
        for k, (depth, tx) in enumerate(self.plan["entries"]):
            big = max(M.TXW[tx], M.TXH[tx])
            costs = rng.integers(10, 4000, 966).astype(np.int32)
            type_costs = [0] * 16 if big == 64 else [int(v) for v in rng.integers(0, 1200, 16)]
            limit = ALL_TYPES_OF(tx)
            m = None
            if masks:
                m = (rng.integers(1, 1 << 16, (n, K.UNIFORM_TX_MAX_TXB)) & limit).astype(np.uint16)
                m[m == 0] = 1
                m[::2] = limit
            single = (rng.random((n, K.UNIFORM_TX_MAX_TXB)) < 0.1).astype(np.uint8)
            dp = dict(costs=costs, tx_type_costs=type_costs, use_txd=use_txd, threshold=22 * 256, low_txfm_rd=0, adaptive=1 + k % 2, skip_tx_search=k % 2, mask_limit=limit,
                      all_masks=m, all_single=single)
            self.dps.append(dp)
            self.prms.append(K.TxSearchParams.make(tx_type_costs=type_costs, use_transform_domain_distortion=use_txd, tx_domain_dist_threshold=dp["threshold"],
                                                   adaptive_txb_search_level=dp["adaptive"], skip_tx_search=dp["skip_tx_search"], tx_mask_limit=limit))
            self.dev.append((ctx.to_device(costs), ctx.to_device(m) if m is not None else None, ctx.to_device(single)))
        self.depths = K.uniform_tx_depths([(self.prms[k],) + self.dev[k] for k in range(len(self.dps))])
        self.d_stats, self.d_txb = ctx.malloc(n * 56), ctx.malloc(n * 4 * K.UNIFORM_TX_MAX_TXB)

    def content(self, seed):
        rng = np.random.default_rng(seed)
        mx = (1 << self.bd) - 1
        H, W = self.H, self.W
        pred = rng.integers(mx // 4, 3 * mx // 4, (H, W))
        amp = np.repeat(np.repeat(rng.choice([0, 0, 2, 12, 60], (H // 8 + 1, W // 8 + 1)), 8, 0), 8, 1)[:H, :W] << (self.bd - 8)
        src = np.clip(pred + (rng.integers(-1, 2, pred.shape) * amp) + (np.add.outer(np.arange(H), np.arange(W)) % 5) * (amp // 3), 0, mx)
        return src, pred

    def upload(self, frame, src, pred):
        self.ctx.planes_upload(self.src, frame, src); self.ctx.planes_upload(self.pred, frame, pred)

    def env(self, src, pred):
        return dict(src=np.pad(src, BORDER, mode="edge").astype(np.int64), pred=np.pad(pred, BORDER, mode="edge").astype(np.int64), pad=BORDER, W=self.W, H=self.H,
                    bd=self.bd, q=self.q, bw=self.bw, bh=self.bh)

    def blk(self, i):
        b = self.blocks[i]
        return dict(x=int(b["x"]), y=int(b["y"]), rdmult=int(b["rdmult"]), source_variance=int(b["source_variance"]), ref_best_rd=int(b["ref_best_rd"]),
                    tx_size_rate=[int(v) for v in b["tx_size_rate"]], no_skip_txfm_rate=int(b["no_skip_txfm_rate"]), skip_txfm_rate=int(b["skip_txfm_rate"]),
                    above_ctx=b["above_ctx"], left_ctx=b["left_ctx"])

    def dp(self, k, i):
        d = dict(self.dps[k])
        d["masks"] = d["all_masks"][i] if d["all_masks"] is not None else None
        d["single"] = d["all_single"][i]
        return d

    def clear(self):
        self.ctx.memset(self.d_stats, 0xA5, self.n * 56); self.ctx.memset(self.d_txb, 0xA5, self.n * 4 * self.K.UNIFORM_TX_MAX_TXB)

    def pick(self):
        self.ctx.pick_uniform_tx_size_type_yrd_batch(self.src, self.pred, 0, self.bsize, self.plan_c, self.qp, self.depths, self.d_blocks, self.n, self.d_stats, self.d_txb)

    def uniform(self, k):
        one = self.K.uniform_tx_depths([(self.prms[k],) + self.dev[k]])
        self.ctx.uniform_txfm_yrd_batch(self.src, self.pred, 0, self.bsize, self.plan["entries"][k][1], self.qp, one, self.d_blocks, self.n, self.d_stats, self.d_txb)

    def fetch(self):
        self.ctx.sync()
        return (self.ctx.from_device(self.d_stats, (self.n,), self.K.uniform_tx_stats_dtype),
                self.ctx.from_device(self.d_txb, (self.n, self.K.UNIFORM_TX_MAX_TXB), self.K.uniform_tx_txb_dtype))

    def close(self):
        for p in [self.d_blocks, self.d_stats, self.d_txb] + [q for d in self.dev for q in d if q is not None]:
            self.ctx.free(p)
        self.ctx.planes_free(self.src); self.ctx.planes_free(self.pred)


def check_stats(st, txb, want, rd, tx_size, tag):
    """one block's device stats and records against a model result (pick_uniform's or uniform_txfm_yrd's)"""
    got = (int(st["rd"]), int(st["rate"]), int(st["dist"]), int(st["sse"]), int(st["skip_txfm"]), int(st["tx_size"]), int(st["n_txb"]))
    assert got == (rd, want["rate"], want["dist"], want["sse"], want["skip_txfm"], tx_size, len(want["txbs"])), tag
    for k, t in enumerate(want["txbs"]):
        assert (int(txb[k]["tx_type"]), int(txb[k]["blk_skip"]), int(txb[k]["txb_entropy_ctx"])) == (t["tx_type"], int(t["eob"] == 0), t["ctx"]), (tag, k)


def run_and_check(fr, src, pred, seen=None, search=U.search_txb, tag=""):
    """the pick call and, per plan entry, the one-size call of the whole batch against the model"""
    env = fr.env(src, pred)
    fr.clear()
    fr.pick()
    stats, txb = fr.fetch()
    for i in range(fr.n):
        want = U.pick_uniform(env, fr.blk(i), fr.plan, [fr.dp(k, i) for k in range(len(fr.dps))], search)
        check_stats(stats[i], txb[i], want, want["rd"], want["tx_size"], (tag, "pick", i))
        assert [int(v) for v in stats[i]["depth_rd"]] == want["depth_rd"], (tag, i)
        if seen is not None:
            seen.append(want)
    if fr.plan["use_largest"]:
        return
    for k, (depth, tx) in enumerate(fr.plan["entries"]):
        fr.clear()
        fr.uniform(k)
        stats, txb = fr.fetch()
        for i in range(fr.n):
            blk = fr.blk(i)
            blk["tx_size_rate"] = [blk["tx_size_rate"][0]] * 3   # (the one-size call reads entry 0)
            want = U.uniform_txfm_yrd(env, blk, tx, fr.dp(k, i), 0, search)
            check_stats(stats[i], txb[i], want, want["rd"], tx if want["valid"] else 255, (tag, "uniform", k, i))


SHAPES = [
    # bw, bh, W, H, bd, (tx_select, mode size (None: the block's largest), init_depth, enable_tx64, enable_rect_tx, use_largest), use_txd
    (8, 8, 24, 24, 8, (1, None, 0, 1, 1, 0), 0),
    (16, 16, 40, 24, 10, (1, None, 0, 1, 1, 0), 1),      # the last column and the last row of blocks cross the frame's edges
    (64, 16, 72, 72, 8, (1, None, 0, 1, 1, 0), 0),
    (16, 64, 72, 72, 12, (1, None, 0, 0, 1, 0), 2),      # without 64-point transforms: depth 0 is skipped
    (128, 128, 136, 136, 12, (1, None, 1, 1, 1, 0), 0),  # two depths of a 128-class size: 64x64 units, partially visible transform blocks
    (16, 8, 24, 24, 12, (1, None, 0, 1, 0, 0), 0),       # without rectangular transforms
    (64, 64, 72, 72, 8, (1, None, 2, 0, 1, 0), 0),       # without 64-point transforms at init_depth == MAX_TX_DEPTH: start_tx is demoted to 32x32
    (32, 32, 40, 40, 10, (0, None, 0, 1, 1, 0), 0),      # tx_select == 0: one size
    (16, 16, 24, 24, 8, (1, None, 0, 1, 1, 1), 1),       # choose_largest_tx_size
]


@pytest.mark.parametrize("bw,bh,W,H,bd,plan_args,use_txd", SHAPES)
def test_batches_against_model(hip, oracle, ctx, bw, bh, W, H, bd, plan_args, use_txd):
    origin = (16, 16) if bw == 128 else (0, 0)
    fr = Frame(hip, ctx, oracle, bw, bh, W, H, bd, plan_args, origin=origin, use_txd=use_txd)
    src, pred = fr.content(5)
    fr.upload(0, src, pred)
    seen = []
    run_and_check(fr, src, pred, seen)
    fr.close()


def coverage(seen):
    """what a list of pick_uniform results reached"""
    ds = [d for w in seen for d in w["depths"] if d is not None]
    lowvar = {w["lowvar"] for w in seen if w["lowvar"]}
    return dict(no_winner=any(w["tx_size"] == 255 for w in seen), entry_refused=any(d["entry_refused"] for d in ds), incomplete=any(d["incomplete"] for d in ds),
                out_of_budget_on_the_last=any(d["last_exit"] and d["valid"] for d in ds), forced_skip=any(d.get("forced_skip") for d in ds),
                skip_stays=any(d["valid"] and d["skip_txfm"] and not d.get("forced_skip") for d in ds), lowvar_taken=("taken", None) in lowvar,
                lowvar_variance=("not taken", "variance") in lowvar, lowvar_order=("not taken", "order") in lowvar, lowvar_guard=("not taken", "guard") in lowvar,
                made_contexts=any(t["skip_ctx"] > 0 and k > 0 for d in ds for k, t in enumerate(d["txbs"])),
                skip_ctx_classes={0 if t["skip_ctx"] == 0 else 1 for d in ds for t in d["txbs"]} == {0, 1}, dc_ctx_all={t["dc_ctx"] for d in ds for t in d["txbs"]} == {0, 1, 2},
                winner_depths=len({d for w in seen for d in range(3) if w["tx_size"] != 255 and w["depth_rd"][d] == w["rd"]}) == 3,
                # blocks crossing the right edge only, the bottom edge only and both, each with a partially visible transform block
                crossings={d["crosses"] for d in ds if "crosses" in d and any(t["partly_visible"] for t in d["txbs"])} >= {(True, False), (False, True), (True, True)})


def test_the_batches_reach_every_path(hip, oracle, ctx):
    """the model alone over the batches of test_batches_against_model: between them they take every exit and both sides of every decision"""
    seen, shrunk = [], []

    def search(env, blk, tx_size, dp, k, row, col, skip_ctx, dc_ctx, ref_best_rd):
        r = U.search_txb(env, blk, tx_size, dp, k, row, col, skip_ctx, dc_ctx, ref_best_rd)
        if dp["adaptive"] and ref_best_rd < blk["ref_best_rd"]:   # the same search with the budget the block came in with: does it visit more types?
            shrunk.append(U.search_txb(env, blk, tx_size, dp, k, row, col, skip_ctx, dc_ctx, blk["ref_best_rd"])["n_visited"] > r["n_visited"])
        return r
    plans = []
    for bw, bh, W, H, bd, plan_args, use_txd in SHAPES:
        fr = Frame(hip, ctx, oracle, bw, bh, W, H, bd, plan_args, origin=(16, 16) if bw == 128 else (0, 0), use_txd=use_txd)
        env = fr.env(*fr.content(5))
        seen += [U.pick_uniform(env, fr.blk(i), fr.plan, [fr.dp(k, i) for k in range(len(fr.dps))], search) for i in range(fr.n)]
        plans.append((bw, bh, bd, plan_args, fr.plan["entries"]))
        fr.close()
    missing = [name for name, reached in coverage(seen).items() if not reached]
    assert not missing, missing
    assert sum(shrunk) >= 2, (sum(shrunk), len(shrunk))   # the adaptive break inside search_tx_type taken BECAUSE ref_best_rd had shrunk by current_rd
    # enable_tx64 == 0 at a 64-class start: the `continue` (depth 0 skipped) and the start_tx demotion (init_depth == MAX_TX_DEPTH starts one size down)
    assert any(not p[3][3] and p[3][2] == 0 and p[4][0][0] == 1 for p in plans) and any(not p[3][3] and p[3][2] == 2 and len(p[4]) == 1 and max(p[0], p[1]) == 64 for p in plans)
    assert len({(p[0], p[1]) for p in plans if p[2] == 12}) >= 3 and {p[2] for p in plans} == {8, 10, 12}


def test_contexts_that_change_the_winner(hip, oracle, ctx):
    """a batch whose multipliers let the rate decide: for several transform blocks the winning type under their real contexts is not the winner under
    the contexts (0, 0) the device's table is computed with (found by running the model both ways), and the device still equals the model"""
    fr = Frame(hip, ctx, oracle, 16, 16, 40, 24, 10, budgets=(M.INT64_MAX,), rdmults=(1 << 17, 1 << 20))
    src, pred = fr.content(5)
    fr.upload(0, src, pred)
    other_winner = []

    def search(env, blk, tx_size, dp, k, row, col, skip_ctx, dc_ctx, ref_best_rd):
        r = U.search_txb(env, blk, tx_size, dp, k, row, col, skip_ctx, dc_ctx, ref_best_rd)
        if (skip_ctx, dc_ctx) != (0, 0):
            other_winner.append(U.search_txb(env, blk, tx_size, dp, k, row, col, 0, 0, ref_best_rd)["best_tx_type"] != r["best_tx_type"])
        return r
    run_and_check(fr, src, pred, search=search, tag="winner")
    assert sum(other_winner) >= 2, (sum(other_winner), len(other_winner))
    fr.close()


def device_search(fr):
    """search_tx_type of one transform block through aomhip_search_tx_type_batch (the parent's entry point), the host carrying contexts and budget"""
    ctx, K = fr.ctx, fr.K
    d_blk, d_res = ctx.malloc(32), ctx.malloc(40)

    def search(env, blk, tx_size, dp, k, row, col, skip_ctx, dc_ctx, ref_best_rd):
        _, _, vc, vr = U.txb_tiles(env, blk, tx_size, row, col)
        b = np.zeros(1, K.tx_search_block_dtype)
        b["x"], b["y"], b["ref_best_rd"], b["rdmult"] = blk["x"] + col * 4, blk["y"] + row * 4, ref_best_rd, blk["rdmult"]
        b["allowed_tx_mask"] = dp["masks"][k] if dp["masks"] is not None else 0xFFFF
        b["visible_cols"], b["visible_rows"], b["txk_allowed_single"], b["txb_skip_ctx"], b["dc_sign_ctx"] = vc, vr, dp["single"][k], skip_ctx, dc_ctx
        ctx.memcpy_h2d(d_blk, b)
        kk = [j for j, e in enumerate(fr.plan["entries"]) if e[1] == tx_size][0]
        ctx.search_tx_type_batch(fr.src, fr.pred, 0, tx_size, fr.qp, fr.dev[kk][0], fr.prms[kk], d_blk, 1, d_res)
        ctx.sync()
        r = ctx.from_device(d_res, (1,), K.tx_search_result_dtype)[0]
        return dict(best_tx_type=int(r["best_tx_type"]), best_eob=int(r["best_eob"]), txb_entropy_ctx=int(r["txb_entropy_ctx"]), rate=int(r["rate"]),
                    dist=int(r["dist"]), sse=int(r["sse"]))

    return search, (d_blk, d_res)


@pytest.mark.parametrize("bw,bh,W,H,bd", [(16, 16, 40, 24, 8), (64, 16, 72, 40, 10)])
def test_equals_the_composition_of_search_tx_type_calls(hip, oracle, ctx, bw, bh, W, H, bd):
    """the same batch driven transform block by transform block through aomhip_search_tx_type_batch with the host doing block_rd_txfm, the tail and the
    depth loop: identical stats, sizes, visiting counts and per-transform-block records"""
    fr = Frame(hip, ctx, oracle, bw, bh, W, H, bd, seed=11)
    src, pred = fr.content(8)
    fr.upload(0, src, pred)
    search, bufs = device_search(fr)
    run_and_check(fr, src, pred, search=search, tag="composition")
    for p in bufs:
        ctx.free(p)
    fr.close()


def test_capture_once_replay_twice(hip, oracle, ctx):
    """one captured graph of the pick call (three depths of list, table and walk) replayed on two frames with different content"""
    fr = Frame(hip, ctx, oracle, 16, 16, 40, 24, 10, seed=4)
    frames = [fr.content(21), fr.content(22)]
    fr.upload(0, *frames[0])
    fr.pick()   # (the warm-up call)
    ctx.sync()
    g = ctx.capture(fr.pick)
    answers = []
    for src, pred in (frames[1], frames[0]):
        fr.upload(0, src, pred)
        fr.clear()
        ctx.graph_launch(g)
        stats, txb = fr.fetch()
        env = fr.env(src, pred)
        for i in range(fr.n):
            want = U.pick_uniform(env, fr.blk(i), fr.plan, [fr.dp(k, i) for k in range(len(fr.dps))])
            check_stats(stats[i], txb[i], want, want["rd"], want["tx_size"], ("replay", i))
        answers.append([int(v) for v in stats["rd"]])
    assert answers[0] != answers[1]
    ctx.graph_destroy(g)
    fr.close()


@pytest.mark.parametrize("bw,bh,W,H,bd,plan_args", [(16, 16, 40, 24, 10, (1, None, 0, 1, 1, 0)), (64, 16, 72, 40, 8, (1, None, 0, 1, 1, 0)),
                                                    (16, 16, 24, 24, 8, (1, None, 0, 1, 1, 1))])
def test_winners_coefficients_are_the_transform_kernels(hip, oracle, ctx, bw, bh, W, H, bd, plan_args):
    """d_qcoeff / d_dqcoeff of the pick call against aomhip_subtract_xform_quant_ex_batch run on the reported sizes, positions and types: the same words at
    coeff_offset + k * max_eob for every visited transform block of every block with a winner, and not a word written anywhere else"""
    fr = Frame(hip, ctx, oracle, bw, bh, W, H, bd, plan_args, seed=6)
    K = fr.K
    src, pred = fr.content(7)
    fr.upload(0, src, pred)
    per_block = bw * bh + 16                                               # (16 words between the blocks' areas that nothing may write)
    fr.blocks["coeff_offset"] = (fr.n - 1 - np.arange(fr.n)) * per_block   # (not the natural order)
    ctx.memcpy_h2d(fr.d_blocks, fr.blocks)
    nbytes = 4 * fr.n * per_block
    bufs = [ctx.malloc(nbytes) for _ in range(4)]
    for p in bufs:
        ctx.memset(p, 0x5A, nbytes)
    d_q, d_dq, d_want_q, d_want_dq = bufs
    fr.clear()
    ctx.pick_uniform_tx_size_type_yrd_batch(fr.src, fr.pred, 0, fr.bsize, fr.plan_c, fr.qp, fr.depths, fr.d_blocks, fr.n, fr.d_stats, fr.d_txb, d_q, d_dq)
    stats, txb = fr.fetch()
    env = fr.env(src, pred)
    sizes = set()
    for tx in sorted({int(v) for v in stats["tx_size"] if v != 255}):
        nc = min(M.TXW[tx], 32) * min(M.TXH[tx], 32)
        recs = []
        for i in range(fr.n):
            if int(stats[i]["tx_size"]) != tx:
                continue
            mbw, mbh = U.max_blocks(env, fr.blk(i))
            order = U.visit_order(mbw, mbh, M.TXW[tx] >> 2, M.TXH[tx] >> 2)
            for k in range(int(stats[i]["n_txb"])):
                if int(txb[i][k]["tx_type"]) < 16:
                    recs.append((int(fr.blocks[i]["x"]) + order[k][1] * 4, int(fr.blocks[i]["y"]) + order[k][0] * 4, int(fr.blocks[i]["coeff_offset"]) + k * nc,
                                 int(txb[i][k]["tx_type"])))
        if not recs:
            continue
        sizes.add(tx)
        lst = np.zeros(len(recs), K.txb_dtype)
        lst["x"], lst["y"], lst["out_offset"], lst["tx_type"] = (np.array([r[j] for r in recs]) for j in range(4))
        d_lst, d_eob = ctx.to_device(lst), ctx.malloc(2 * len(recs))
        ctx.subtract_xform_quant_ex_batch(fr.src, fr.pred, 0, tx, d_lst, len(recs), 0, 0, fr.qp, 0, None, d_want_q, d_want_dq, d_eob, None)
        ctx.sync()
        ctx.free(d_lst); ctx.free(d_eob)
    assert sizes and (plan_args[5] or len(sizes) > 1)
    got_q, got_dq = ctx.from_device(d_q, (fr.n * per_block,), np.int32), ctx.from_device(d_dq, (fr.n * per_block,), np.int32)
    want_q, want_dq = ctx.from_device(d_want_q, (fr.n * per_block,), np.int32), ctx.from_device(d_want_dq, (fr.n * per_block,), np.int32)
    assert np.array_equal(got_q, want_q) and np.array_equal(got_dq, want_dq)
    assert (want_q != 0x5A5A5A5A).any() and (want_q == 0x5A5A5A5A).any()
    for p in bufs:
        ctx.free(p)
    fr.close()


def test_refused_arguments_launch_nothing(hip, oracle, ctx):
    K = hip.capi
    lib = K.lib
    fr = Frame(hip, ctx, oracle, 16, 16, 40, 24, 8)
    fr.upload(0, *fr.content(1))
    other_depth, other_size = ctx.planes_alloc(fr.W, fr.H, BORDER, 10, 1), ctx.planes_alloc(fr.W + 8, fr.H, BORDER, 8, 1)
    fr.clear()

    def pick(src=fr.src, pred=fr.pred, frame=0, bsize=fr.bsize, plan=fr.plan_c, qp=C.byref(fr.qp), depths=fr.depths, blocks=fr.d_blocks, stats=fr.d_stats, txb=fr.d_txb,
             q=None, dq=None):
        return lib.aomhip_pick_uniform_tx_size_type_yrd_batch(ctx.h, C.byref(src) if src is not None else None, C.byref(pred) if pred is not None else None, frame, bsize,
                                                              C.byref(plan) if plan is not None else None, qp, depths, blocks, fr.n, stats, txb, q, dq)

    def uniform(tx_size, bsize=fr.bsize, depth=fr.depths, pred=fr.pred):
        return lib.aomhip_uniform_txfm_yrd_batch(ctx.h, C.byref(fr.src), C.byref(pred), 0, bsize, tx_size, C.byref(fr.qp), depth, fr.d_blocks, fr.n, fr.d_stats, fr.d_txb)

    def plan_with(**kw):
        p = K.UniformTxPlan.from_buffer_copy(fr.plan_c)
        for name, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, name)[v[0]] = v[1]
            else:
                setattr(p, name, v)
        return p

    def depths_with(**kw):
        prm = K.TxSearchParams.from_buffer_copy(fr.prms[1])
        for name, v in kw.items():
            setattr(prm, name, v)
        keep.append(prm)
        return K.uniform_tx_depths([(fr.prms[0],) + fr.dev[0], (prm,) + fr.dev[1], (fr.prms[2],) + fr.dev[2]])

    keep = []
    no_costs = K.uniform_tx_depths([(fr.prms[0],) + fr.dev[0], (fr.prms[1], None, None, None), (fr.prms[2],) + fr.dev[2]])
    bad = [pick(pred=other_depth), pick(pred=other_size), pick(frame=1), pick(frame=-1), pick(bsize=22), pick(bsize=-1), pick(src=None), pick(pred=None), pick(plan=None),
           pick(q=fr.d_txb), pick(dq=fr.d_txb), pick(qp=None), pick(depths=None), pick(blocks=None), pick(stats=None), pick(txb=None), pick(depths=no_costs),
           # plans the helper never produces for a 16x16 block: a foreign size, a swapped order, a hole, four entries, a wrong first depth, use_largest with three
           pick(plan=plan_with(tx_size=(0, 3))), pick(plan=plan_with(tx_size=(0, 1), depth=(0, 0))), pick(plan=plan_with(tx_size=(1, 0))), pick(plan=plan_with(n=4)),
           pick(plan=plan_with(init_depth=1)), pick(plan=plan_with(use_largest=1)), pick(bsize=3),
           pick(depths=depths_with(tx_mask_limit=0)), pick(depths=depths_with(use_transform_domain_distortion=3)), pick(depths=depths_with(adaptive_txb_search_level=63)),
           # sizes that are no uniform size of the block
           uniform(3), uniform(7), uniform(19), uniform(-1), uniform(2, bsize=22), uniform(2, pred=other_depth), uniform(4, bsize=9)]
    for name in ("predict_dc_level", "enable_trellis", "use_qmatrix", "quant_b_adapt", "lossless", "is_intra"):
        bad.append(pick(depths=depths_with(**{name: 1})))
    assert all(rc == K.ERR_INVALID for rc in bad), bad
    ctx.sync()
    assert (ctx.from_device(fr.d_stats, (fr.n * 56,), np.uint8) == 0xA5).all()
    assert pick() == K.OK and uniform(2) == K.OK and uniform(1) == K.OK and uniform(0) == K.OK
    ctx.sync()
    assert not (ctx.from_device(fr.d_stats, (fr.n * 56,), np.uint8) == 0xA5).all()
    ctx.planes_free(other_depth); ctx.planes_free(other_size)
    fr.close()


def test_a_transform_block_without_an_allowed_type_sets_the_device_status(hip, oracle, ctx):
    """one block's mask is empty at one depth: aomhip_ctx_sync reports it, that depth of that block is invalid, the other blocks are untouched by it"""
    fr = Frame(hip, ctx, oracle, 16, 16, 40, 24, 8, budgets=(M.INT64_MAX,))
    src, pred = fr.content(2)
    fr.upload(0, src, pred)
    m = fr.dps[1]["all_masks"]
    m[1, 2] = 0
    ctx.memcpy_h2d(fr.dev[1][1], m)
    fr.clear()
    fr.pick()
    with pytest.raises(fr.K.AomHipError):
        ctx.sync()
    stats, txb = fr.fetch()
    env = fr.env(src, pred)
    assert int(stats[1]["depth_rd"][1]) == M.INT64_MAX and int(stats[1]["depth_rd"][0]) != M.INT64_MAX
    for i in range(fr.n):
        want = U.pick_uniform(env, fr.blk(i), fr.plan, [fr.dp(k, i) for k in range(len(fr.dps))])
        check_stats(stats[i], txb[i], want, want["rd"], want["tx_size"], ("status", i))
    fr.close()


# ---- the interpreted reference's record (tests/golden/ref_eval_uniform_tx.npz) through both entry points

def _fixture_groups():
    z, cases = U.golden()
    groups = {}
    for c in cases:
        key = (c["bsize"], c["bd"], c["vis_w"], c["vis_h"], c["tx_select"], c["mode_tx_size"], c["init_depth"], c["enable_tx64"], c["enable_rect_tx"], c["use_largest"],
               c["use_txd"], c["threshold"], c["adaptive"], c["skip_tx_search"], c["qindex"])
        groups.setdefault(key, []).append(c)
    return z, sorted(groups.items())


FIX_Z, FIX_GROUPS = _fixture_groups()


@pytest.mark.parametrize("key,cases", FIX_GROUPS, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else None)
def test_fixture_cases_through_both_entry_points(hip, oracle, ctx, key, cases):
    """every stored case, batched by (block size, bit depth, visible extent, plan, parameters): the whole blocks of a batch lie side by side in one plane pair,
    a block that the frame's edge cuts has planes of its own (the edge is the planes' edge).  Each case's type costs are its own, so the batch is run once
    per case and that case's block is checked: the pick call against the recorded rd[3], stats, size, visiting count, types, blk_skip and contexts, the
    one-size call against every depth the reference tried"""
    K = hip.capi
    bsize, bd, vw, vh = key[0], key[1], key[2], key[3]
    bw, bh = U.BSW[bsize], U.BSH[bsize]
    c0 = cases[0]
    plan_c = K.uniform_tx_depth_plan(bsize, c0["tx_select"], c0["mode_tx_size"], c0["init_depth"], c0["enable_tx64"], c0["enable_rect_tx"], c0["use_largest"])
    entries = plan_c.entries()
    whole = vw == bw and vh == bh
    batches = [cases] if whole else [[c] for c in cases]
    for batch in batches:
        m = len(batch)
        W, H = (m * bw, bh) if whole else (vw, vh)
        src, pred = ctx.planes_alloc(W, H, 128, bd, 1), ctx.planes_alloc(W, H, 128, bd, 1)
        ctx.planes_upload(src, 0, np.concatenate([FIX_Z["src%d" % c["k"]] for c in batch], 1)); ctx.planes_upload(pred, 0, np.concatenate([FIX_Z["pred%d" % c["k"]] for c in batch], 1))
        blocks = np.zeros(m, K.uniform_tx_block_dtype)
        masks = [np.full((m, K.UNIFORM_TX_MAX_TXB), 0xFFFF, np.uint16) for _ in entries]
        for i, c in enumerate(batch):
            env, blk, plan, dps = U.case_inputs(FIX_Z, c)
            assert plan["entries"] == entries
            b = blocks[i]
            b["x"], b["y"], b["rdmult"], b["source_variance"], b["ref_best_rd"] = i * bw if whole else 0, 0, c["rdmult"], c["source_variance"], c["ref_best_rd"]
            b["tx_size_rate"] = blk["tx_size_rate"][:3]
            b["no_skip_txfm_rate"], b["skip_txfm_rate"], b["above_ctx"], b["left_ctx"] = c["no_skip_txfm_rate"], c["skip_txfm_rate"], blk["above_ctx"], blk["left_ctx"]
            for k, dp in enumerate(dps):
                masks[k][i, :len(dp["masks"])] = dp["masks"]
        q = oracle.build_quantizer_y(bd, c0["qindex"])
        qp = K.QuantParams.from_tables(q)
        dev = [(ctx.to_device(U.case_costs(FIX_Z, tx)), ctx.to_device(masks[k])) for k, (_, tx) in enumerate(entries)]
        d_stats, d_txb = ctx.malloc(56 * m), ctx.malloc(4 * K.UNIFORM_TX_MAX_TXB * m)
        for i, c in enumerate(batch):   # per case: its own type costs; the batch's other blocks ride along and are checked in their own turn
            prm = [K.TxSearchParams.make(tx_type_costs=c["type_costs"][str(tx)], use_transform_domain_distortion=c["use_txd"], tx_domain_dist_threshold=c["threshold"],
                                         adaptive_txb_search_level=c["adaptive"], skip_tx_search=c["skip_tx_search"]) for _, tx in entries]
            depths = K.uniform_tx_depths([(prm[k], dev[k][0], dev[k][1], None) for k in range(len(entries))])
            d_blocks = ctx.to_device(blocks)
            if entries:
                ctx.memset(d_stats, 0xA5, 56 * m); ctx.memset(d_txb, 0xA5, 4 * K.UNIFORM_TX_MAX_TXB * m)
                ctx.pick_uniform_tx_size_type_yrd_batch(src, pred, 0, bsize, plan_c, qp, depths, d_blocks, m, d_stats, d_txb)
                ctx.sync()
                st = ctx.from_device(d_stats, (m,), K.uniform_tx_stats_dtype)[i]
                tb = ctx.from_device(d_txb, (m, K.UNIFORM_TX_MAX_TXB), K.uniform_tx_txb_dtype)[i]
                valid = c["rate"] != (1 << 31) - 1
                assert (int(st["rate"]), int(st["dist"]), int(st["sse"]), int(st["skip_txfm"])) == (c["rate"], int(c["dist"]), int(c["sse"]), c["skip_txfm"]), c["k"]
                if not c["use_largest"]:
                    assert [int(v) for v in st["depth_rd"]] == [int(v) for v in c["rd"][:3]], c["k"]
                    assert int(st["tx_size"]) == (c["rd"][3] if valid else 255), c["k"]
                if valid:
                    win = [d for d in c["depths"] if d["tx_size"] == int(st["tx_size"])][0]
                    assert int(st["n_txb"]) == len(win["txbs"]), c["k"]
                    for k, t in enumerate(win["txbs"]):
                        assert (int(tb[k]["tx_type"]), int(tb[k]["blk_skip"]), int(tb[k]["txb_entropy_ctx"])) == (t["tx_type"], int(t["eob"] == 0), t["ctx"]), (c["k"], k)
            for k, d in enumerate(c["depths"]):   # av1_uniform_txfm_yrd at each size the reference tried
                if c["use_largest"]:
                    break
                blocks1 = blocks.copy()
                blocks1["tx_size_rate"][:, 0] = blocks["tx_size_rate"][:, k]
                ctx.memcpy_h2d(d_blocks, blocks1)
                one = K.uniform_tx_depths([(prm[k], dev[k][0], dev[k][1], None)])
                ctx.uniform_txfm_yrd_batch(src, pred, 0, bsize, d["tx_size"], qp, one, d_blocks, m, d_stats, d_txb)
                ctx.sync()
                st = ctx.from_device(d_stats, (m,), K.uniform_tx_stats_dtype)[i]
                tb = ctx.from_device(d_txb, (m, K.UNIFORM_TX_MAX_TXB), K.uniform_tx_txb_dtype)[i]
                assert int(st["rd"]) == int(c["rd"][d["depth"]]) and int(st["n_txb"]) == len(d["txbs"]), (c["k"], k)
                for j, t in enumerate(d["txbs"]):
                    assert (int(tb[j]["tx_type"]), int(tb[j]["blk_skip"]), int(tb[j]["txb_entropy_ctx"])) == (t["tx_type"], int(t["eob"] == 0), t["ctx"]), (c["k"], k, j)
            ctx.free(d_blocks)
        for p in [d_stats, d_txb] + [q_ for d in dev for q_ in d]:
            ctx.free(p)
        ctx.planes_free(src); ctx.planes_free(pred)
