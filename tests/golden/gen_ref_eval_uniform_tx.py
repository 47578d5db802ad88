#!/usr/bin/env python3
"""Golden vectors of the uniform transform-size search from the interpreted reference (build container only; see ref_c_eval.py):

  ref_eval_uniform_tx.npz   choose_tx_size_type_from_rd, choose_largest_tx_size, av1_uniform_txfm_yrd, av1_txfm_rd_in_plane, block_rd_txfm (av1/encoder/tx_search.c),
                            av1_foreach_transformed_block_in_plane (av1/encoder/encodemb.c), get_txb_ctx, av1_set_txb_context and av1_merge_rd_stats AS THEY ARE
                            WRITTEN, on gen_ref_eval_tx_type.py's evaluator (search_tx_type interpreted as there).  Hooks inserted into the text record, per depth,
                            the visiting order and each visited transform block's (blk_row, blk_col, txb_skip_ctx, dc_sign_ctx, the ref_best_rd passed down, the
                            types search_tx_type visited, winner type, eob, entropy context, rate, dist, sse), exit_early / incomplete_exit, the forced skip,
                            the low-variance break and rd[depth]; the final state adds tx_size, tx_type_map and blk_skip.

Supplied as inputs / adaptations (as in gen_ref_eval_tx_type.py unless said):
  * the visitor argument of av1_foreach_transformed_block_in_plane is spelled as the call of block_rd_txfm it is here (the evaluator has no function pointers);
  * block_rd_txfm's intra branch and its CfL store, the NN depth prune (#if !CONFIG_REALTIME_ONLY) and av1_get_tx_size's chroma branch are cut: inter luma only;
  * get_tx_mask returns the case's mask of the transform block (txk_allowed = TX_TYPES, the identity order); get_tx_type_cost the case's table of the size;
  * cpi->oxcf.txfm_cfg.enable_tx64 / enable_rect_tx and the speed features are read through tx_cfg(k); get_search_init_depth(..) and tx_size_from_tx_mode(..)
    are the case's values through uts_cfg(k), as the device call takes them from its caller;
  * av1_zero(args) is spelled out; av1_copy_array is its memcpy without the sizeof assertion; set_blk_skip without its NDEBUG bookkeeping bits;
  * a block that crosses the frame's edge holds the frame's edge pixels repeated beyond it, as the planes' borders do.

The generator runs tests/uniform_tx_model.py on every case -- it must reproduce the record, and run both ways it finds the transform blocks whose winner
under their real contexts differs from the winner under contexts (0, 0), and those whose adaptive break only the shrunken ref_best_rd triggers -- and
asserts its own coverage before it writes (main()).  python tests/golden/gen_ref_eval_uniform_tx.py --write"""
import os
import re
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import ref_c_eval as R  # noqa: E402
import gen_ref_eval_yrd as Y  # noqa: E402
import gen_ref_eval_tx_type as X  # noqa: E402
from gen_ref_eval_golden import REF, save  # noqa: E402


def make_evaluator():
    Y.PRE_VIEWS += "typedef struct { uint8_t blk_skip[1024]; } TxfmSearchInfo;\n"
    Y.MB_MEMBERS += " unsigned int source_variance; TxfmSearchInfo txfm_search_info;"
    ev, state = X.make_evaluator()
    for n, v in (("MAX_TX_DEPTH", 2), ("MAX_MIB_SIZE", 32), ("FTXS_NONE", 0), ("AOM_PLANE_Y", 0), ("TX_MODE_SELECT", 2), ("FULL_TXFM_RD", 0), ("BLOCK_64X64", 12)):
        ev.define(n, "(%d)" % v)
    bd_h = open(REF + "av1/common/blockd.h").read()
    gts = Y.cut(bd_h, "static INLINE TX_SIZE av1_get_tx_size(")
    gts = gts[:gts.index("const MACROBLOCKD_PLANE *pd")] + "return TX_4X4;\n}\n"      # (luma only: the chroma branch is never reached)
    ev.load_text(Y.cut(bd_h, "static INLINE BLOCK_SIZE get_plane_block_size(") + gts + Y.cut(bd_h, "static INLINE int is_rect_tx(") +
                 Y.cut(open(REF + "av1/encoder/block.h").read(), "static INLINE int is_rect_tx_allowed_bsize("), "blockd.h:get_plane_block_size, av1_get_tx_size, is_rect_tx, is_rect_tx_allowed_bsize")
    sb = Y.cut(open(REF + "av1/encoder/block.h").read(), "static INLINE void set_blk_skip(")
    sb = re.sub(r"#ifndef NDEBUG.*?#endif", "", sb, flags=re.S)
    ev.load_text(sb, "block.h:set_blk_skip")
    ev.load_text(Y.cut(open(REF + "av1/encoder/rdopt_utils.h").read(), "static AOM_INLINE int bsize_to_num_blk("), "rdopt_utils.h:bsize_to_num_blk")
    em = open(REF + "av1/encoder/encodemb.c").read()
    fe = Y.cut(em, "void av1_foreach_transformed_block_in_plane(")
    fe, n = re.subn(r"foreach_transformed_block_visitor visit", "int visit", fe); assert n == 1
    fe, n = re.subn(r"visit\(plane, i, blk_row, blk_col, plane_bsize, tx_size, arg\);", "block_rd_txfm(plane, i, blk_row, blk_col, plane_bsize, tx_size, arg);", fe); assert n == 1
    ts = open(REF + "av1/encoder/tx_search.c").read()
    br = Y.cut(ts, "static AOM_INLINE void block_rd_txfm(")
    a = br.index("  if (!is_inter) {"); b = br.index("  TXB_CTX txb_ctx;")
    br = br[:a] + br[b:]
    a = br.index("  if (plane == AOM_PLANE_Y && xd->cfl.store_y) {"); b = br.index("  av1_set_txb_context(x, plane, block, tx_size, a, l);")
    br = br[:a] + br[b:]
    br = br.replace("const AV1_COMMON *cm = &cpi->common;", "")
    br, n = re.subn(r"search_tx_type\(cpi, x, plane, block, blk_row, blk_col, plane_bsize, tx_size,", "uts_hook_txb(blk_row, blk_col, txb_ctx.txb_skip_ctx, txb_ctx.dc_sign_ctx, args->best_rd - args->current_rd);\n  search_tx_type(cpi, x, plane, block, blk_row, blk_col, plane_bsize, tx_size,", br); assert n == 1
    br, n = re.subn(r"av1_merge_rd_stats\(&args->rd_stats, &this_rd_stats\);", "uts_hook_txb_done(blk_row, blk_col, x->plane[plane].eobs[block], x->plane[plane].txb_entropy_ctx[block], this_rd_stats.rate, this_rd_stats.dist, this_rd_stats.sse);\n  av1_merge_rd_stats(&args->rd_stats, &this_rd_stats);", br); assert n == 1
    rp = Y.cut(ts, "void av1_txfm_rd_in_plane(")
    rp, n = re.subn(r"!cpi->oxcf\.txfm_cfg\.enable_tx64", "!tx_cfg(5)", rp); assert n == 1
    rp = rp.replace("av1_zero(args);", "args.exit_early = 0; args.incomplete_exit = 0; args.current_rd = 0; args.best_rd = 0; args.ftxs_mode = 0; args.skip_trellis = 0;")
    rp = rp.replace("args.x = x;", "args.x = x; uts_hook_enter(tx_size);")
    rp, n = re.subn(r"const int invalid_rd = is_inter \? args\.incomplete_exit : args\.exit_early;", "const int invalid_rd = is_inter ? args.incomplete_exit : args.exit_early;\n  uts_hook_leave(args.exit_early, args.incomplete_exit, args.rd_stats.skip_txfm);", rp); assert n == 1
    rp, n = re.subn(r"av1_foreach_transformed_block_in_plane\(xd, plane_bsize, plane, block_rd_txfm,\s*&args\);", "av1_foreach_transformed_block_in_plane(xd, plane_bsize, plane, 0, &args);", rp); assert n == 1
    un = Y.cut(ts, "int64_t av1_uniform_txfm_yrd(")
    un = un.replace(": tx_size_cost(x, bs, tx_size);", ": 0;")
    un, n = re.subn(r"if \(temp_skip_txfm_rd <= rd\) \{", "if (temp_skip_txfm_rd <= rd) {\n      uts_hook_forced();", un); assert n == 1
    cl = Y.cut(ts, "static AOM_INLINE void choose_largest_tx_size(")
    cl, n = re.subn(r"tx_size_from_tx_mode\(bs, txfm_params->tx_mode_search_type\)", "uts_cfg(1)", cl); assert n == 1
    ch = Y.cut(ts, "static AOM_INLINE void choose_tx_size_type_from_rd(")
    ch = re.sub(r"#if !CONFIG_REALTIME_ONLY.*?#endif(  // !CONFIG_REALTIME_ONLY)?", "", ch, flags=re.S)
    ch, n = re.subn(r"get_search_init_depth\(mi_size_wide\[bs\], mi_size_high\[bs\],\s*is_inter_block\(mbmi\), &cpi->sf,\s*txfm_params->tx_size_search_method\)", "uts_cfg(0)", ch); assert n == 1
    ch, n = re.subn(r"tx_size_from_tx_mode\(bs, txfm_params->tx_mode_search_type\)", "uts_cfg(1)", ch); assert n == 1
    ch, n = re.subn(r"rd\[depth\] = av1_uniform_txfm_yrd\(", "uts_hook_depth(depth, tx_size);\n    rd[depth] = av1_uniform_txfm_yrd(", ch); assert n == 1
    ch, n = re.subn(r"if \(rd\[depth - 1\] != INT64_MAX && rd\[depth\] > rd\[depth - 1\]\) break;", "if (rd[depth - 1] != INT64_MAX && rd[depth] > rd[depth - 1]) { uts_hook_lowvar(1); break; }\n      uts_hook_lowvar(0);", ch); assert n == 1
    ch, n = re.subn(r"if \(rd_stats->rate != INT_MAX\) \{", "uts_hook_rd(rd[0], rd[1], rd[2], best_tx_size);\n  if (rd_stats->rate != INT_MAX) {", ch); assert n == 1
    out = []
    for t in (cl, ch):
        for pat, rep in ((r"cpi->oxcf\.txfm_cfg\.enable_tx64", "tx_cfg(5)"), (r"cpi->oxcf\.txfm_cfg\.enable_rect_tx", "tx_cfg(6)")):
            t = re.sub(pat, rep, t)
        out.append(t)
    cl, ch = out
    ev.load_text("#define av1_copy_array(dest, src, n) memcpy(dest, src, (n) * sizeof(*(src)))\n", "common.h:av1_copy_array")
    ev.load_text(br + fe + rp + un + cl + ch, "tx_search.c + encodemb.c: the three layers")
    bad = [s for s in ev.skipped if s[0].startswith(("tx_search", "blockd.h:get_plane", "block.h:set", "rdopt_utils.h:bsize", "common.h:av1_copy"))]
    assert not bad, bad
    return ev, state

# ---------------------------------------------------------------------------------------------------------------- one case
TXW, TXH = X.TXW, X.TXH
INT64_MAX = (1 << 63) - 1
BSW = [4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64]
BSH = [4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16]


def cost_tables(ev, state, rng):
    """one set of coefficient-cost tables for the whole fixture: [5 size contexts][N_COSTS] and [7 eob sizes][22]"""
    if "uts_costs" not in state:
        state["uts_costs"] = (rng.integers(10, 4000, (5, Y.N_COSTS)), rng.integers(10, 4000, (7, 22)))
    return state["uts_costs"]


def run_case(ev, state, orc, rng, cs):
    bsize, bd = cs["bsize"], cs["bd"]
    bw, bh = BSW[bsize], BSH[bsize]
    vw, vh = cs["vis_w"], cs["vis_h"]
    hbd = bd > 8
    mx = (1 << bd) - 1
    pred = rng.integers(mx // 4, 3 * mx // 4, (vh, vw))
    amp = np.repeat(np.repeat(rng.choice(cs["amps"], (vh // 4 + 1, vw // 4 + 1)), 4, 0), 4, 1)[:vh, :vw] << (bd - 8)
    src = np.clip(pred + rng.integers(-1, 2, (vh, vw)) * amp + (np.add.outer(np.arange(vh), np.arange(vw)) % 5) * (amp // 3), 0, mx)
    srcb, predb = np.pad(src, ((0, bh - vh), (0, bw - vw)), mode="edge"), np.pad(pred, ((0, bh - vh), (0, bw - vw)), mode="edge")
    q = orc.build_quantizer_y(bd, cs["qindex"])
    x = ev.new("MACROBLOCK")
    ct = "uint16_t" if hbd else "uint8_t"
    ev.set(x, "plane[0].src.buf", ev.array(srcb.ravel(), ct)); ev.set(x, "plane[0].src.stride", bw)
    ev.set(x, "e_mbd.plane[0].dst.buf", ev.array(predb.ravel(), ct)); ev.set(x, "e_mbd.plane[0].dst.stride", bw)
    ev.set(x, "plane[0].src_diff", ev.array((srcb - predb).ravel(), "int16_t"))
    for nm in ("coeff", "qcoeff", "dqcoeff"):
        ev.set(x, "plane[0]." + nm, ev.array(np.zeros(bw * bh, np.int32), "int32_t"))
    ev.set(x, "plane[0].eobs", ev.array(np.zeros(bw * bh // 16, np.int64), "uint16_t"))
    ev.set(x, "plane[0].txb_entropy_ctx", ev.array(np.zeros(bw * bh // 16, np.int64), "uint8_t"))
    for nm, key in (("zbin_QTX", "zbin"), ("round_QTX", "round"), ("quant_QTX", "quant"), ("quant_shift_QTX", "quant_shift"), ("dequant_QTX", "dequant")):
        ev.set(x, "plane[0]." + nm, ev.array([int(v) for v in q[key]], "int16_t"))
    mbmi = ev.new("MB_MODE_INFO")
    ev.set(mbmi, "bsize", bsize); ev.set(mbmi, "segment_id", 0); ev.set(mbmi, "ref_frame[0]", 1); ev.set(mbmi, "ref_frame[1]", -1); ev.set(mbmi, "use_intrabc", 0)
    ev.set(mbmi, "tx_size", 255)
    ev.set(x, "e_mbd.mi", R.Ptr([mbmi], 0, R.PTR))
    n4w, n4h = bw // 4, bh // 4
    kind = cs["ctx_kind"]
    above = np.zeros(n4w, np.int64) if kind == 0 else (rng.integers(0, 4 if kind == 1 else 8, n4w) | (rng.integers(0, 3, n4w) << 3))
    left = np.zeros(n4h, np.int64) if kind == 0 else (rng.integers(0, 4 if kind == 1 else 8, n4h) | (rng.integers(0, 3, n4h) << 3))
    ev.set(x, "e_mbd.plane[0].above_entropy_context", ev.array(above, "int8_t")); ev.set(x, "e_mbd.plane[0].left_entropy_context", ev.array(left, "int8_t"))
    ev.set(x, "e_mbd.plane[0].subsampling_x", 0); ev.set(x, "e_mbd.plane[0].subsampling_y", 0)
    atx, ltx = int(rng.choice([4, 8, 16, 32, 64])), int(rng.choice([4, 8, 16, 32, 64]))
    ev.set(x, "e_mbd.above_txfm_context", ev.array([atx], "uint8_t")); ev.set(x, "e_mbd.left_txfm_context", ev.array([ltx], "uint8_t"))
    skips = [int(rng.integers(0, 3)) for _ in range(2)]
    for nm, sk in zip(("above_mbmi", "left_mbmi"), skips):
        if sk:
            nb = ev.new("MB_MODE_INFO")
            ev.set(nb, "skip_txfm", sk - 1)
            ev.set(x, "e_mbd." + nm, nb)
        else:
            ev.set(x, "e_mbd." + nm, None)
    ev.set(x, "e_mbd.bd", bd)
    buf = ev.new("YV12_BUFFER_CONFIG")
    ev.set(buf, "flags", Y.YV12_FLAG_HIGHBITDEPTH if hbd else 0)
    ev.set(x, "e_mbd.cur_buf", buf)
    ev.set(x, "e_mbd.mb_to_right_edge", (vw - bw) * 8); ev.set(x, "e_mbd.mb_to_bottom_edge", (vh - bh) * 8)
    ev.set(x, "e_mbd.tx_type_map", ev.array(np.full(32 * 32, 255, np.int64), "uint8_t")); ev.set(x, "e_mbd.tx_type_map_stride", bw // 4)
    ev.set(x, "txfm_search_params.tx_mode_search_type", 2 if cs["tx_select"] else 1)
    ev.set(x, "txfm_search_params.use_qm_dist_metric", 0)
    ev.set(x, "txfm_search_params.use_transform_domain_distortion", cs["use_txd"])
    ev.set(x, "txfm_search_params.tx_domain_dist_threshold", cs["threshold"])
    ev.set(x, "txfm_search_params.predict_dc_level", 0)
    ev.set(x, "txfm_search_params.coeff_opt_thresholds[0]", 4294967295); ev.set(x, "txfm_search_params.coeff_opt_thresholds[1]", 4294967295)
    ev.set(x, "rd_model", 0); ev.set(x, "rdmult", cs["rdmult"]); ev.set(x, "seg_skip_block", 0); ev.set(x, "source_variance", cs["source_variance"])
    mode = rng.integers(20, 3000, 21 * 2 + 3 * 2)
    if cs.get("cheap_skip"):
        mode[42 + 1::2] = 25
    for i in range(21):
        for j in range(2):
            ev.set(x, "mode_costs.txfm_partition_cost[%d][%d]" % (i, j), int(mode[2 * i + j]))
    for i in range(3):
        for j in range(2):
            ev.set(x, "mode_costs.skip_txfm_cost[%d][%d]" % (i, j), int(mode[42 + 2 * i + j]))
    cc, ec = cost_tables(ev, state, rng)
    for c5 in range(5):
        o = 0
        for nm, a_, b_ in Y.COST_NAMES:
            for i in range(a_):
                for j in range(b_):
                    ev.set(x, "coeff_costs.coeff_costs[%d][0].%s[%d][%d]" % (c5, nm, i, j), int(cc[c5][o])); o += 1
    for e7 in range(7):
        for i in range(2):
            for j in range(11):
                ev.set(x, "coeff_costs.eob_costs[%d][0].eob_cost[%d][%d]" % (e7, i, j), int(ec[e7][i * 11 + j]))
    type_costs = {tx: ([0] * 16 if max(TXW[tx], TXH[tx]) == 64 else [int(v) for v in rng.integers(0, 1200, 16)]) for tx in range(19)}
    cpi = ev.new("AV1_COMP")
    ev.set(cpi, "common.features.reduced_tx_set_used", 0)
    stats = ev.new("RD_STATS")
    cfg = {0: 1, 1: cs["adaptive"], 2: cs["skip_tx_search"], 3: 0, 4: 0, 5: cs["enable_tx64"], 6: cs["enable_rect_tx"]}
    ucfg = {0: cs["init_depth"], 1: cs["mode_tx_size"]}
    masks = {}
    log = {"depths": [], "cur": None, "tx_size": None, "type": None, "lowvar": None, "rd": None, "forced": []}

    def mask_of(tx, row, col):
        key = "%d,%d,%d" % (tx, row, col)
        if key not in masks:
            sm = X.set_mask_of(tx) & cs.get("mask_limit", 0xFFFF)
            m = sm if (row + col) % 8 == 0 or cs.get("full_masks") else (int(rng.integers(1, 1 << 16)) & sm or (sm & -sm))
            masks[key] = m
        return masks[key]
    pc = ev.interp.pycalls
    pc["tx_cfg"] = lambda it, a: (cfg[int(a[0][0])], R.I32)
    pc["uts_cfg"] = lambda it, a: (ucfg[int(a[0][0])], R.I32)
    pc["get_tx_type_cost"] = lambda it, a: (type_costs[int(a[-3][0])][int(a[-2][0])], R.I32)

    def get_tx_mask(it, a):
        a[11][0].buf[a[11][0].off] = 16
        return mask_of(int(a[7][0]), int(a[4][0]), int(a[5][0])), R.I32
    pc["get_tx_mask"] = get_tx_mask

    def h_depth(it, a):
        log["depths"].append({"depth": int(a[0][0]), "tx_size": int(a[1][0]), "txbs": [], "entered": 0, "forced": 0})
        return None, R.VOID

    def h_enter(it, a):
        if cs["use_largest"]:
            log["depths"].append({"depth": 0, "tx_size": int(a[0][0]), "txbs": [], "entered": 0, "forced": 0})
        log["depths"][-1]["entered"] = 1
        log["tx_size"] = int(a[0][0])
        return None, R.VOID

    def h_txb(it, a):
        log["cur"] = {"row": int(a[0][0]), "col": int(a[1][0]), "skip_ctx": int(a[2][0]), "dc_ctx": int(a[3][0]), "ref_best_rd": str(int(a[4][0])), "visit": []}
        log["depths"][-1]["txbs"].append(log["cur"])
        return None, R.VOID

    def h_done(it, a):
        c = log["cur"]
        c.update(eob=int(a[2][0]), ctx=int(a[3][0]), rate=int(a[4][0]), dist=str(int(a[5][0])), sse=str(int(a[6][0])))
        tm = ev.field(x, "e_mbd.tx_type_map").deref()[0].buf
        c["tx_type"] = int(tm[c["row"] * n4w + c["col"]])
        return None, R.VOID

    def h_leave(it, a):
        log["depths"][-1].update(exit_early=int(a[0][0]), incomplete=int(a[1][0]), skip=int(a[2][0]))
        return None, R.VOID
    pc["uts_hook_depth"], pc["uts_hook_enter"], pc["uts_hook_txb"], pc["uts_hook_txb_done"], pc["uts_hook_leave"] = h_depth, h_enter, h_txb, h_done, h_leave
    pc["uts_hook_forced"] = lambda it, a: (log["depths"][-1].__setitem__("forced", 1), R.VOID)
    pc["uts_hook_lowvar"] = lambda it, a: (log.__setitem__("lowvar", int(a[0][0])), R.VOID)
    pc["uts_hook_rd"] = lambda it, a: (log.__setitem__("rd", [str(int(a[k][0])) for k in range(3)] + [int(a[3][0])]), R.VOID)

    def h_visit(it, a):
        log["cur"]["visit"].append(int(a[0][0]))
        log["type"] = int(a[0][0])
        return None, R.VOID
    pc["tx_hook_visit"] = h_visit
    for nm in ("tx_hook_flags", "tx_hook_type", "tx_hook_rate_only", "tx_hook_branch", "tx_hook_best"):
        pc[nm] = lambda it, a: (None, R.VOID)

    def py_fwd(it, a):
        s, dst, stride, prm = a[0][0], a[1][0], int(a[2][0]), a[3][0]
        tx = int(ev.get(prm, "tx_size")); w, h = TXW[tx], TXH[tx]
        blk = np.array([[s.buf[s.off + r * stride + c] for c in range(w)] for r in range(h)], np.int16)
        out = orc.fwd_txfm2d(blk, tx, int(ev.get(prm, "tx_type")), bd).ravel()
        for k_, v in enumerate(out):
            dst.buf[dst.off + k_] = int(v)
        return None, R.VOID

    def py_quant(hb):
        def f(it, a):
            co, n = a[0][0], int(a[1][0])
            c = np.array([co.buf[co.off + k_] for k_ in range(n)], np.int32)
            tx, t = log["tx_size"], log["type"]
            scan, iscan = orc.get_scan(tx, t)
            qc, dq, eob = orc.quantize_b(c, q, scan, iscan, int(ev.call("av1_get_tx_scale", tx)), highbd=hb)
            for nm_, arr in ((3, qc), (4, dq)):
                p_ = a[nm_][0]
                for k_, v in enumerate(arr):
                    p_.buf[p_.off + k_] = int(v)
            a[5][0].buf[a[5][0].off] = int(eob)
            return None, R.VOID
        return f

    def py_inv(it, a):
        dqp, t, tx, dst, stride, eob = a[1][0], int(a[3][0]), int(a[4][0]), a[5][0], int(a[6][0]), int(a[7][0])
        if not eob:
            return None, R.VOID
        w, h = TXW[tx], TXH[tx]
        dq = np.array([dqp.buf[dqp.off + k_] for k_ in range(min(w, 32) * min(h, 32))], np.int32)
        tile = np.array([[dst.buf[dst.off + r * stride + c] for c in range(w)] for r in range(h)], np.uint16)
        rec = orc.inv_txfm2d_add(dq, tile, tx, t, bd)
        for r in range(h):
            for c in range(w):
                dst.buf[dst.off + r * stride + c] = int(rec[r, c])
        return None, R.VOID

    def get_scan(it, a):
        scan, iscan = orc.get_scan(int(a[0][0]), int(a[1][0]))
        so = ev.new("SCAN_ORDER")
        ev.set(so, "scan", ev.array(scan, "int16_t")); ev.set(so, "iscan", ev.array(iscan, "int16_t"))
        return so, R.PTR
    saved = {}
    for nm in ("av1_fwd_txfm", "av1_quantize_b_facade", "av1_highbd_quantize_b_facade"):
        saved[nm] = ev.interp.funcs.pop(nm)
    pc["av1_fwd_txfm"] = py_fwd
    pc["av1_quantize_b_facade"] = py_quant(False)
    pc["av1_highbd_quantize_b_facade"] = py_quant(True)
    pc["av1_inverse_transform_block"] = py_inv
    old_scan = pc["get_scan"]
    pc["get_scan"] = get_scan
    try:
        ev.call("choose_largest_tx_size" if cs["use_largest"] else "choose_tx_size_type_from_rd", cpi, x, stats, cs["ref_best_rd"], bsize)
    finally:
        for nm, f in saved.items():
            ev.interp.funcs[nm] = f
            pc.pop(nm, None)
        pc["get_scan"] = old_scan
    skip_ctx = sum(1 for sk in skips if sk == 2)
    tsr = {}
    for tx in range(19):
        tsr[str(tx)] = 0
    if cs["tx_select"] and int(ev.call("block_signals_txsize", bsize)):
        for d in log["depths"]:
            pctx = int(ev.call("txfm_partition_context", ev.array([atx], "uint8_t"), ev.array([ltx], "uint8_t"), bsize, d["tx_size"]))
            tsr[str(d["tx_size"])] = int(mode[2 * pctx])
    blk_skip = [int(v) & 1 for v in ev.field(x, "txfm_search_info.blk_skip").buf[:n4w * n4h]] if hasattr(ev.field(x, "txfm_search_info.blk_skip"), "buf") else None
    rec = dict(cs)
    rec.update(depths=log["depths"], lowvar=log["lowvar"], rd=log["rd"], masks=masks, type_costs={str(k): v for k, v in type_costs.items()}, tx_size_rate=tsr,
               no_skip_txfm_rate=int(mode[42 + 2 * skip_ctx]), skip_txfm_rate=int(mode[42 + 2 * skip_ctx + 1]),
               rate=int(ev.get(stats, "rate")), dist=str(int(ev.get(stats, "dist"))), sse=str(int(ev.get(stats, "sse"))), skip_txfm=int(ev.get(stats, "skip_txfm")),
               mbmi_tx_size=int(ev.get(mbmi, "tx_size")), final_type_map=[int(v) for v in ev.field(x, "e_mbd.tx_type_map").deref()[0].buf[:n4w * n4h]], above=[int(v) for v in above], left=[int(v) for v in left], blk_skip=blk_skip)
    pt = np.uint16 if hbd else np.uint8
    return rec, {"src": src.astype(pt), "pred": pred.astype(pt)}


# ---------------------------------------------------------------------------------------------------------------- the cases


def plan_cases(rng):
    plan = []

    def add(bsize, bd, **kw):
        bw, bh = BSW[bsize], BSH[bsize]
        c = dict(bsize=bsize, bd=bd, vis_w=bw, vis_h=bh, amps=[0, 0, 2, 12, 60], qindex=120, ctx_kind=len(plan) % 3, tx_select=1, use_txd=0, threshold=0,
                 rdmult=int(rng.choice([80, 300, 900, 1 << 17])), source_variance=int(rng.choice([10, 255, 256, 4000])), adaptive=1 + len(plan) % 2, skip_tx_search=len(plan) % 2,
                 enable_tx64=1, enable_rect_tx=1, init_depth=0, mode_tx_size=max_rect_tx(bsize), use_largest=0, ref_best_rd=INT64_MAX)
        c.update(kw)
        if max(bw, bh) >= 64:
            c.setdefault("mask_limit", 0x0207)   # the 64- and 128-class cases are the bulk: DCT_DCT, ADST_DCT, DCT_ADST, IDTX at most
        plan.append(c)
    B = {(BSW[i], BSH[i]): i for i in range(22)}
    small = [B[4, 4], B[8, 8], B[16, 16], B[32, 32], B[16, 8], B[4, 16], B[8, 32]]
    for bs in small:
        for bd in (8, 10):
            add(bs, bd)                                                  # the whole budget: every depth to its end
            add(bs, bd, ref_best_rd=1 << 24)                             # a budget that runs out somewhere
        add(bs, 8, ref_best_rd=900)                                      # ... at once, or at the entry
        add(bs, 10, rdmult=1 << 20, cheap_skip=1)                        # the rate decides: forced skips, winners that depend on the contexts
        add(bs, 8, source_variance=10, rdmult=80)                        # low contrast: the break of :2913
        add(bs, 10, source_variance=255, amps=[0, 0, 0, 2])
        add(bs, 8, amps=[0], qindex=200)                                 # nothing to code: skip_txfm stays 1
    for bs in (B[16, 16], B[8, 8], B[4, 16]):
        add(bs, 12); add(bs, 12, ref_best_rd=1 << 26)
    for j in range(6):                                                   # the rate decides and the neighbours are busy: winners that the contexts change
        add(B[16, 16], 10 if j % 2 else 8, ctx_kind=2, rdmult=1 << (17 + j % 2 * 3), adaptive=1 + j % 2)
    for j in range(4):                                                   # budgets of the size of the block's own cost: the adaptive break by the shrunken budget
        add(B[16, 16], 8 if j % 2 else 10, ref_best_rd=1 << (26 + 2 * j), adaptive=1, skip_tx_search=0, rdmult=300)
    add(B[16, 16], 8, vis_w=8); add(B[16, 16], 10, vis_h=8); add(B[16, 16], 8, vis_w=8, vis_h=8)          # crossing the right edge, the bottom edge, both
    add(B[32, 32], 10, vis_w=24); add(B[32, 32], 8, vis_h=8); add(B[32, 32], 10, vis_w=8, vis_h=24)
    add(B[16, 16], 8, tx_select=0); add(B[32, 32], 10, tx_select=0, ref_best_rd=1 << 26)                  # tx_select == 0
    add(B[16, 16], 8, use_largest=1); add(B[8, 32], 10, use_largest=1, enable_rect_tx=0); add(B[16, 8], 8, use_largest=1, ref_best_rd=900)
    add(B[16, 8], 8, enable_rect_tx=0); add(B[8, 32], 10, enable_rect_tx=0); add(B[4, 16], 8, enable_rect_tx=0)
    add(B[16, 16], 8, init_depth=1); add(B[32, 32], 10, init_depth=2)
    # the 64 class
    add(B[64, 64], 8); add(B[64, 64], 10, ref_best_rd=1 << 30); add(B[64, 16], 8); add(B[64, 16], 10, source_variance=10)
    add(B[64, 64], 8, enable_tx64=0); add(B[64, 16], 10, enable_tx64=0)                                   # the `continue` ...
    add(B[64, 64], 10, enable_tx64=0, init_depth=2); add(B[64, 16], 8, enable_tx64=0, init_depth=2)       # ... and the start_tx demotion
    add(B[64, 64], 8, vis_w=40, vis_h=24)
    # the 128 class: two cases
    add(B[128, 128], 8, init_depth=1, vis_w=120, vis_h=72); add(B[128, 64], 10, init_depth=2)
    return plan


def max_rect_tx(bsize):
    w, h = min(BSW[bsize], 64), min(BSH[bsize], 64)
    return [i for i in range(19) if TXW[i] == w and TXH[i] == h][0]


def coverage(cases, extra):
    n = {}

    def hit(k, c=1):
        n[k] = n.get(k, 0) + c
    for c, ex in zip(cases, extra):
        bw, bh = BSW[c["bsize"]], BSH[c["bsize"]]
        ds = c["depths"]
        valid = c["rate"] != (1 << 31) - 1
        if valid and not c["use_largest"]:
            hit("winner_depth%d" % [d["depth"] for d in ds if d["tx_size"] == c["rd"][3]][0])
        for d in ds:
            if d.get("incomplete"):
                hit("incomplete_exit")
            if d.get("exit_early") and not d.get("incomplete"):
                hit("out_of_budget_on_the_last_valid")
            if not d["entered"]:
                hit("entry_refused")
            if d["forced"]:
                hit("forced_skip")
            if d["entered"] and d.get("skip") and not d.get("incomplete") and not d["forced"]:
                hit("skip_stays")
            right, bottom = c["vis_w"] < bw, c["vis_h"] < bh
            partial = any((t["col"] * 4 + TXW[d["tx_size"]] > c["vis_w"]) or (t["row"] * 4 + TXH[d["tx_size"]] > c["vis_h"]) for t in d["txbs"])
            if partial:
                hit("cross_%s" % ("both" if right and bottom else ("right" if right else "bottom")))
            for k, t in enumerate(d["txbs"]):
                hit("skip_ctx_0" if t["skip_ctx"] == 0 else "skip_ctx_1_6")
                hit("dc_ctx_%d" % t["dc_ctx"])
                if c["ctx_kind"] == 0 and k > 0 and (t["skip_ctx"] > 1 or t["dc_ctx"]):
                    hit("contexts_from_an_earlier_txb")
        if c["lowvar"] == 1:
            hit("lowvar_taken")
        if c["lowvar"] == 0:
            hit("lowvar_not_taken_rd_order")
        if not c["use_largest"] and c["tx_select"] and c["init_depth"] == 0 and c["source_variance"] >= 256 and len(ds) == 3:
            hit("lowvar_not_taken_variance")
        if c["lowvar"] is None and not c["use_largest"] and c["init_depth"] == 0 and c["source_variance"] < 256 and len(ds) >= 2 and ds[1]["depth"] == 1 and ds[1]["tx_size"] != 0:
            hit("lowvar_guard_or_4x4")
        hit("tx_select_0", int(not c["tx_select"] and not c["use_largest"])); hit("use_largest", c["use_largest"])
        if not c["enable_tx64"] and max(bw, bh) >= 64 and not c["use_largest"]:
            hit("tx64_off_demotion" if c["init_depth"] == 2 else "tx64_off_continue")
        hit("rect_off", int(not c["enable_rect_tx"]))
        hit("bd%d" % c["bd"])
        hit("other_winner_under_zero_contexts", ex["other_winner"]); hit("adaptive_break_by_shrunken_budget", ex["shrunk"])
    return n


def model_extras(U, M, c, arrays, z_like):
    """the model run on the case: must reproduce the record; and, both ways, the two cases only a second run can show"""
    env, blk, plan, dps = U.case_inputs(None, c, arrays)
    for dp, (_, tx) in zip(dps, plan["entries"]):
        dp["costs"] = z_like(tx)
    ex = {"other_winner": 0, "shrunk": 0}

    def search(env_, blk_, tx, dp, k, row, col, sc, dc, ref):
        r = U.search_txb(env_, blk_, tx, dp, k, row, col, sc, dc, ref)
        if (sc, dc) != (0, 0) and U.search_txb(env_, blk_, tx, dp, k, row, col, 0, 0, ref)["best_tx_type"] != r["best_tx_type"]:
            ex["other_winner"] += 1
        if dp["adaptive"] and ref < blk_["ref_best_rd"] and U.search_txb(env_, blk_, tx, dp, k, row, col, sc, dc, blk_["ref_best_rd"])["n_visited"] > r["n_visited"]:
            ex["shrunk"] += 1
        return r
    want = U.pick_uniform(env, blk, plan, dps, search)
    return want, ex


def main():
    import pyoracle as orc
    import tx_type_model as M
    import uniform_tx_model as U
    ev, state = make_evaluator()
    rng = np.random.default_rng(20261022)
    arrays, cases, extra = {}, [], []
    t0 = time.time()
    cc, ec = cost_tables(ev, state, rng)
    txs_ctx = [int(ev.call("get_txsize_entropy_ctx", tx)) for tx in range(19)]
    eob_class = [int(ev.global_values("txsize_log2_minus4")[tx]) for tx in range(19)]
    table_of = lambda tx: np.concatenate([cc[txs_ctx[tx]], ec[eob_class[tx]]]).astype(np.int32)
    for k, cs in enumerate(plan_cases(rng)):
        rec, arr = run_case(ev, state, orc, rng, cs)
        rec["k"] = k
        rec.pop("amps")
        want, ex = model_extras(U, M, rec, arr, table_of)
        got = (rec["rd"][:3] if rec["rd"] else None, rec["rate"], rec["dist"], rec["sse"], rec["skip_txfm"])
        exp = ([str(v) for v in want["depth_rd"]] if rec["rd"] else None, want["rate"], str(want["dist"]), str(want["sse"]), want["skip_txfm"])
        print(k, BSW[cs["bsize"]], BSH[cs["bsize"]], cs["bd"], [(d["depth"], d["tx_size"], len(d["txbs"])) for d in rec["depths"]], rec["rd"], rec["rate"], ex,
              "%.0f s" % (time.time() - t0), flush=True)
        assert got == exp, ("the model differs from the record", k, got, exp)
        cases.append(rec); extra.append(ex)
        for nm, v in arr.items():
            arrays["%s%d" % (nm, k)] = v
    cov = coverage(cases, extra)
    print(cov)
    need = ("winner_depth0", "winner_depth1", "winner_depth2", "incomplete_exit", "out_of_budget_on_the_last_valid", "entry_refused", "lowvar_taken", "lowvar_not_taken_rd_order",
            "lowvar_not_taken_variance", "forced_skip", "skip_stays", "cross_right", "cross_bottom", "cross_both", "skip_ctx_0", "skip_ctx_1_6", "dc_ctx_0", "dc_ctx_1", "dc_ctx_2",
            "contexts_from_an_earlier_txb", "other_winner_under_zero_contexts", "adaptive_break_by_shrunken_budget", "tx_select_0", "use_largest", "tx64_off_continue",
            "tx64_off_demotion", "rect_off", "bd8", "bd10", "bd12")
    missing = {k_: cov.get(k_, 0) for k_ in need if cov.get(k_, 0) < 2}
    assert not missing, missing
    assert len({c["bsize"] for c in cases if c["bd"] == 12}) >= 3
    arrays.update(coeff_costs=cc.astype(np.int32), eob_costs=ec.astype(np.int32), txs_ctx=np.array(txs_ctx, np.int32), eob_class=np.array(eob_class, np.int32))
    if "--write" in sys.argv:
        save("ref_eval_uniform_tx.npz", arrays, cases)
    else:
        print("(not written: pass --write)")


if __name__ == "__main__":
    main()
