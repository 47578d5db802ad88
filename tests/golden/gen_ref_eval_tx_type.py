#!/usr/bin/env python3
"""Golden vectors of the transform-type search from the interpreted reference (build container only; see ref_c_eval.py):

  ref_eval_tx_type.npz   search_tx_type (av1/encoder/tx_search.c:2019-2335) AS IT IS WRITTEN -- pixel_diff_dist, the two distortion-mode flags, the loop
                         over txk_map under the mask with its `continue` and `break` statements, the five distortion branches, the strict `rd < best_rd`,
                         the tail with the final pixel-domain recomputation -- with its callees interpreted too: get_txb_dimensions (rdopt_utils.h),
                         aom_sum_squares_2d_i16_c, cost_coeffs -> av1_cost_coeffs_txb, dist_block_tx_domain -> av1_[highbd_]block_error_c,
                         dist_block_px_domain -> aom_[highbd_]convolve_copy_c, pixel_dist, pixel_dist_visible_only -> variance() / highbd_{8,10,12}_variance()
                         (aom_dsp/variance.c: what fn_ptr[].vf computes besides the mean) and aom_[highbd_]sse_odd_size, av1_get_tx_type, update_txk_array,
                         skip_trellis_opt_based_on_satd, recon_intra (a no-op for the inter blocks here), on gen_ref_eval_yrd.py's evaluator and struct views.
                         Per case: the inputs, the final outputs, and -- from hook calls inserted into the loop's text -- the types in visiting
                         order, the {rate, eob, ctx, dist, sse} of every type the loop evaluated fully, the rate-only `continue`s, the two rarer distortion branches, and the
                         block's scalars.

Supplied as inputs / adaptations (as in gen_ref_eval_yrd.py unless said):
  * get_tx_mask is a stub that returns the case's mask, txk_allowed and txk_map; get_tx_type_cost returns the case's 16-entry table's entry;
  * the forward transform, the B quantiser and the inverse transform are the separately pinned restatements (pyoracle), for speed;
  * cpi's speed features and configuration (adaptive_txb_search_level, skip_tx_search, quant_b_adapt, the PSY content test, the quantisation-matrix
    test) are read through tx_cfg(k), a stub over the case's values, because the evaluator's AV1_COMP view does not hold them; trellis is off
    (skip_trellis == 1: is_trellis_used is not consulted);
  * fn_ptr[tx_bsize].vf(..) is spelled as the call of variance() / highbd_N_variance() its VAR / HIGHBD_VAR macro expands to;
  * check_bit_mask's `return mask & (1 << val)` is spelled `!= 0`: the conversion to bool C performs there (the evaluator's bool is a byte);
  * dist_block_px_domain's low-bit-depth `recon = (uint8_t *)recon16` is a uint8_t array of its own (the evaluator's buffers are typed).

The generator asserts its own coverage before it writes (main())."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_c_eval as R  # noqa: E402
import gen_ref_eval_txb_cost as T  # noqa: E402
import gen_ref_eval_yrd as Y  # noqa: E402
from gen_ref_eval_golden import REF, save  # noqa: E402

TXW, TXH = T.TXW, T.TXH
INT64_MAX = (1 << 63) - 1
def set_mask_of(tx_size):
    """av1_ext_tx_used_flag of the inter set av1_get_ext_tx_set_type picks for a size (blockd.h:1087-1111): what get_tx_mask can return at most"""
    m = max(TXW[tx_size], TXH[tx_size])
    return 0x0001 if m == 64 else (0x0201 if m == 32 else (0x0FFF if m == 16 else 0xFFFF))


def make_evaluator():
    Y.PRE_VIEWS = Y.PRE_VIEWS.replace("typedef struct { int tx_mode_search_type; int use_qm_dist_metric; } TxfmSearchParams;",
                                      "typedef struct { int tx_mode_search_type; int use_qm_dist_metric; int use_transform_domain_distortion; "
                                      "unsigned int tx_domain_dist_threshold; int predict_dc_level; unsigned int coeff_opt_thresholds[2]; } TxfmSearchParams;\n"
                                      "struct buf_2d { uint8_t *buf; int stride; };")
    Y.PRE_VIEWS = Y.PRE_VIEWS.replace("struct macroblockd_plane { int subsampling_x;", "struct macroblockd_plane { struct buf_2d dst; int subsampling_x;")
    Y.XD_MEMBERS += " uint8_t *tx_type_map; int tx_type_map_stride;"
    Y.PLANE_MEMBERS += " struct buf_2d src;"
    Y.MB_MEMBERS += " int rd_model;"
    ev, state = Y.make_evaluator()
    ev.interp.funcs.pop("av1_get_ext_tx_set_type", None)
    for n, v in (("TX_TYPE_INVALID", 255), ("LOW_TXFM_RD", 1), ("DRY_RUN_NORMAL", 1), ("USE_B_QUANT_NO_TRELLIS", 1), ("UINT_MAX", 4294967295)):
        ev.define(n, "(%d)" % v)
    for i, n in enumerate(("EXT_TX_SET_DCTONLY", "EXT_TX_SET_DCT_IDTX", "EXT_TX_SET_DTT4_IDTX", "EXT_TX_SET_DTT4_IDTX_1DDCT", "EXT_TX_SET_DTT9_IDTX_1DDCT",
                           "EXT_TX_SET_ALL16", "EXT_TX_SET_TYPES")):
        ev.define(n, "(%d)" % i)
    ev.define("FAST_TX_SEARCH_MODE", "int")
    bd_h = open(REF + "av1/common/blockd.h").read()
    ev.load_text(Y.cut(bd_h, "static const TxSetType av1_ext_tx_set_lookup[2][2] =") + Y.cut(bd_h, "static INLINE TxSetType av1_get_ext_tx_set_type("),
                 "blockd.h:av1_get_ext_tx_set_type")
    ev.load_text(Y.cut(bd_h, "static INLINE void update_txk_array(") + Y.cut(bd_h, "static INLINE TX_TYPE av1_get_tx_type("), "blockd.h:update_txk_array, av1_get_tx_type")
    for f in ("aom_dsp/sum_squares.c", "aom_dsp/variance.h", "aom_dsp/variance.c"):
        ev.load(REF + f)
    ev.define("aom_sum_squares_2d_i16", "aom_sum_squares_2d_i16_c")
    cv = open(REF + "aom_dsp/aom_convolve.c").read()
    ev.load_text(Y.cut(cv, "void aom_convolve_copy_c(") + Y.cut(cv, "void aom_highbd_convolve_copy_c("), "aom_convolve.c:copies")
    ev.define("aom_convolve_copy", "aom_convolve_copy_c"); ev.define("aom_highbd_convolve_copy", "aom_highbd_convolve_copy_c")
    ev.load_text(Y.cut(open(REF + "av1/encoder/rdopt_utils.h").read(), "static AOM_INLINE void get_txb_dimensions("), "rdopt_utils.h:get_txb_dimensions")
    ev.load_text("static unsigned int tx_vf(int bd, int hbd, const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, int w, int h, unsigned int *sse) {\n"
                 "  int sum;\n  if (!hbd) variance(a, a_stride, b, b_stride, w, h, sse, &sum);\n  else if (bd == 8) highbd_8_variance(a, a_stride, b, b_stride, w, h, sse, &sum);\n"
                 "  else if (bd == 10) highbd_10_variance(a, a_stride, b, b_stride, w, h, sse, &sum);\n  else highbd_12_variance(a, a_stride, b, b_stride, w, h, sse, &sum);\n"
                 "  return 0;\n}\n", "fn_ptr[].vf: the VAR / HIGHBD_VAR macros' call")
    ts = open(REF + "av1/encoder/tx_search.c").read()
    pv = Y.cut(ts, "static unsigned pixel_dist_visible_only(")
    pv, n = re.subn(r"cpi->ppi->fn_ptr\[tx_bsize\]\.vf\(src, src_stride, dst, dst_stride, &sse\);",
                    "tx_vf(x->e_mbd.bd, is_cur_buf_hbd(&x->e_mbd), src, src_stride, dst, dst_stride, txb_cols, txb_rows, &sse);", pv)
    assert n == 1
    px = Y.cut(ts, "static INLINE int64_t dist_block_px_domain(")
    px, n = re.subn(r"recon = \(uint8_t \*\)recon16;", "recon = recon8;", px)
    assert n == 2
    px = px.replace("uint8_t *recon;", "uint8_t *recon;\n  uint8_t recon8[MAX_TX_SQUARE];")
    px = px.replace("assert(cpi != NULL);", "")
    ev.load_text(Y.cut(ts, "static INLINE int64_t pixel_diff_dist(") + pv + Y.cut(ts, "static unsigned pixel_dist(") + px, "tx_search.c:pixel distortion")
    cbm, n = re.subn(r"return mask & \(1 << val\);", "return (mask & (1 << val)) != 0;", Y.cut(ts, "static AOM_INLINE bool check_bit_mask("))
    assert n == 1
    ev.load_text(cbm + Y.cut(ts, "static int skip_trellis_opt_based_on_satd("), "tx_search.c:check_bit_mask, satd")
    ri = Y.cut(ts, "static INLINE void recon_intra(")
    ev.load_text(Y.cut(ts, "static AOM_INLINE void inverse_transform_block_facade(") + ri, "tx_search.c:recon_intra")
    body = Y.cut(ts, "static void search_tx_type(")
    subs = ((r"const AV1EncoderConfig \*const oxcf = &cpi->oxcf;\s*const TuneCfg \*tune_params = &oxcf->tune_cfg;", ""),
            (r"skip_trellis \|= !is_trellis_used\(cpi->optimize_seg_arr\[xd->mi\[0\]->segment_id\],\s*DRY_RUN_NORMAL\);", "skip_trellis |= 1;"),
            (r"\(tune_params->content != AOM_CONTENT_PSY\)", "(tx_cfg(0) != 0)"),
            (r"av1_use_qmatrix\(&cm->quant_params, xd, mbmi->segment_id\)", "tx_cfg(4)"),
            (r"cpi->sf\.tx_sf\.tx_type_search\.skip_tx_search", "tx_cfg(2)"),
            (r"const uint16_t \*eobs_ptr = x->plane\[plane\]\.eobs;",
             "tx_hook_flags(block_sse, block_mse_q8, use_transform_domain_distortion, calc_pixel_domain_distortion_final);\n  const uint16_t *eobs_ptr = x->plane[plane].eobs;"),
            (r"txfm_param\.tx_type = tx_type;", "tx_hook_visit(tx_type);\n    txfm_param.tx_type = tx_type;"),
            (r"this_rd_stats\.rate = rate_cost;",
             "this_rd_stats.rate = rate_cost;\n    tx_hook_type(tx_type, rate_cost, eobs_ptr[block], x->plane[plane].txb_entropy_ctx[block], this_rd_stats.dist, this_rd_stats.sse);"),
            (r"if \(RDCOST\(x->rdmult, rate_cost, 0\) > best_rd\) continue;", "if (RDCOST(x->rdmult, rate_cost, 0) > best_rd) { tx_hook_rate_only(tx_type, rate_cost); continue; }"),
            (r"this_rd_stats\.dist = tx_domain_dist;", "{ this_rd_stats.dist = tx_domain_dist; tx_hook_branch(tx_type, 1); }"),
            (r"this_rd_stats\.dist \+= sse_diff;", "this_rd_stats.dist += sse_diff; tx_hook_branch(tx_type, 2);"),
            (r"assert\(best_rd != INT64_MAX\);", "tx_hook_best(best_rd);"))
    for pat, rep in subs:
        body, n = re.subn(pat, rep, body)
        assert n == 1, pat
    for pat, rep in ((r"cpi->sf\.tx_sf\.adaptive_txb_search_level", "tx_cfg(1)"), (r"cpi->oxcf\.q_cfg\.quant_b_adapt", "tx_cfg(3)")):
        body, n = re.subn(pat, rep, body)
        assert n == 2, pat
    body = re.sub(r"#if CONFIG_COLLECT_RD_STATS == 1.*?#endif  // CONFIG_COLLECT_RD_STATS == 1", "", body, flags=re.S)
    body = re.sub(r"#if COLLECT_TX_SIZE_DATA.*?#endif  // COLLECT_TX_SIZE_DATA", "", body, flags=re.S)
    ev.load_text(body, "tx_search.c:search_tx_type")
    bad = [s for s in ev.skipped if s[0].startswith(("tx_search", "blockd.h:update", "blockd.h:av1_get_ext", "rdopt_utils", "aom_convolve", "fn_ptr"))]
    assert not bad, bad
    return ev, state


def run_case(ev, state, orc, rng, cs):
    """One call of search_tx_type; cs: the case's parameters (a dict); returns (record, arrays)."""
    tx_size, bd = cs["tx_size"], cs["bd"]
    w, h = TXW[tx_size], TXH[tx_size]
    hbd = bd > 8
    nc = min(w, 32) * min(h, 32)
    mx = (1 << bd) - 1
    pred = rng.integers(mx // 4, 3 * mx // 4, (h, w))
    amp = cs["amp"]
    if cs.get("saturate"):      # high energy: source and predictor at opposite ends of the range
        pred = rng.integers(0, mx // 16 + 1, (h, w))
        src = mx - rng.integers(0, mx // 16 + 1, (h, w))
        if cs["saturate"] == 2:   # ... and mostly outside the coded quadrant for TX_64X64: a checkerboard
            src = np.where(np.add.outer(np.arange(h), np.arange(w)) % 2 == 0, src, pred)
    else:
        res = rng.integers(-amp, amp + 1, (h, w))
        if amp > 8:
            res = res + (np.add.outer(np.arange(h) * cs.get("gy", 1), np.arange(w) * cs.get("gx", 1)) % 7 * (amp // 4))
        src = np.clip(pred + res, 0, mx)
    q = orc.build_quantizer_y(bd, cs["qindex"])
    x = ev.new("MACROBLOCK")
    ct = "uint16_t" if hbd else "uint8_t"
    psrc, ppred = ev.array(src.ravel(), ct), ev.array(pred.ravel(), ct)
    ev.set(x, "plane[0].src.buf", psrc); ev.set(x, "plane[0].src.stride", w)
    ev.set(x, "e_mbd.plane[0].dst.buf", ppred); ev.set(x, "e_mbd.plane[0].dst.stride", w)
    ev.set(x, "plane[0].src_diff", ev.array((src - pred).ravel(), "int16_t"))
    for nm in ("coeff", "qcoeff", "dqcoeff"):
        ev.set(x, "plane[0]." + nm, ev.array(np.zeros(w * h, np.int32), "int32_t"))
    ev.set(x, "plane[0].eobs", ev.array(np.zeros(max(w * h // 16, 1), np.int64), "uint16_t"))
    ev.set(x, "plane[0].txb_entropy_ctx", ev.array(np.zeros(max(w * h // 16, 1), np.int64), "uint8_t"))
    for nm, key in (("zbin_QTX", "zbin"), ("round_QTX", "round"), ("quant_QTX", "quant"), ("quant_shift_QTX", "quant_shift"), ("dequant_QTX", "dequant")):
        ev.set(x, "plane[0]." + nm, ev.array([int(v) for v in q[key]], "int16_t"))
    bsize = Y.BSIZES.index("BLOCK_%dX%d" % (w, h))
    mbmi = ev.new("MB_MODE_INFO")
    ev.set(mbmi, "bsize", bsize); ev.set(mbmi, "segment_id", 0); ev.set(mbmi, "ref_frame[0]", 1); ev.set(mbmi, "ref_frame[1]", -1); ev.set(mbmi, "use_intrabc", 0)
    ev.set(x, "e_mbd.mi", R.Ptr([mbmi], 0, R.PTR))
    ev.set(x, "e_mbd.plane[0].subsampling_x", 0); ev.set(x, "e_mbd.plane[0].subsampling_y", 0)
    ev.set(x, "e_mbd.bd", bd)
    buf = ev.new("YV12_BUFFER_CONFIG")
    ev.set(buf, "flags", Y.YV12_FLAG_HIGHBITDEPTH if hbd else 0)
    ev.set(x, "e_mbd.cur_buf", buf)
    vc, vr = cs["vis_cols"], cs["vis_rows"]
    ev.set(x, "e_mbd.mb_to_right_edge", (vc - w) * 8); ev.set(x, "e_mbd.mb_to_bottom_edge", (vr - h) * 8)   # get_txb_dimensions: (edge >> 3) + block size
    ev.set(x, "e_mbd.tx_type_map", ev.array(np.zeros(16 * 16, np.int64), "uint8_t")); ev.set(x, "e_mbd.tx_type_map_stride", 16)
    ev.set(x, "txfm_search_params.use_qm_dist_metric", 0)
    ev.set(x, "txfm_search_params.use_transform_domain_distortion", cs["use_txd"])
    ev.set(x, "txfm_search_params.tx_domain_dist_threshold", cs["threshold"])
    ev.set(x, "txfm_search_params.predict_dc_level", 0)
    ev.set(x, "txfm_search_params.coeff_opt_thresholds[0]", 4294967295); ev.set(x, "txfm_search_params.coeff_opt_thresholds[1]", 4294967295)
    ev.set(x, "rd_model", 1 if cs["low_txfm_rd"] else 0)
    ev.set(x, "rdmult", cs["rdmult"]); ev.set(x, "seg_skip_block", 0)
    txs_ctx = int(ev.call("get_txsize_entropy_ctx", tx_size))
    ems = int(ev.global_values("txsize_log2_minus4")[tx_size])
    costs = state.setdefault(("costs", tx_size, bd), rng.integers(10, 4000, Y.N_COSTS + 22))   # one table per (size, depth): the fixture's bulk otherwise
    o = 0
    for nm, a_, b_ in Y.COST_NAMES:
        for i in range(a_):
            for j in range(b_):
                ev.set(x, "coeff_costs.coeff_costs[%d][0].%s[%d][%d]" % (txs_ctx, nm, i, j), int(costs[o])); o += 1
    for i in range(2):
        for j in range(11):
            ev.set(x, "coeff_costs.eob_costs[%d][0].eob_cost[%d][%d]" % (ems, i, j), int(costs[Y.N_COSTS + i * 11 + j]))
    tx_type_costs = [0] * 16 if max(w, h) == 64 else [int(v) for v in rng.integers(0, 1500, 16)]
    if cs.get("equal_types"):
        tx_type_costs = [tx_type_costs[0]] * 16
    cpi = ev.new("AV1_COMP")
    ev.set(cpi, "common.features.reduced_tx_set_used", 0)
    tctx = ev.new("TXB_CTX")
    skip_ctx, dc_ctx = int(rng.integers(0, 13)), int(rng.integers(0, 3))
    ev.set(tctx, "txb_skip_ctx", skip_ctx); ev.set(tctx, "dc_sign_ctx", dc_ctx)
    stats = ev.new("RD_STATS")
    mask, single, txk_map = cs["mask"], cs["single"], cs["txk_map"]
    log = {"visit": [], "types": {}, "rate_only": [], "flags": None, "best_rd": None, "branch": []}
    cfg = {0: int(not cs["psy"]), 1: cs["adaptive"], 2: cs["skip_tx_search"], 3: 0, 4: 0}
    pc = ev.interp.pycalls
    pc["tx_cfg"] = lambda it, a: (cfg[int(a[0][0])], R.I32)
    pc["get_tx_type_cost"] = lambda it, a: (tx_type_costs[int(a[-2][0])], R.I32)   # (.., tx_size, tx_type, reduced_tx_set_used)

    def get_tx_mask(it, a):
        a[11][0].buf[a[11][0].off] = single if single is not None else 16
        if txk_map is not None:
            for i in range(16):
                a[12][0].buf[a[12][0].off + i] = int(txk_map[i])
        return mask, R.I32
    pc["get_tx_mask"] = get_tx_mask
    pc["tx_hook_visit"] = lambda it, a: (log["visit"].append(int(a[0][0])), R.VOID)
    pc["tx_hook_flags"] = lambda it, a: (log.__setitem__("flags", [int(v[0]) for v in a]), R.VOID)
    pc["tx_hook_type"] = lambda it, a: (log["types"].__setitem__(int(a[0][0]), [int(v[0]) for v in a[1:]]), R.VOID)
    pc["tx_hook_rate_only"] = lambda it, a: (log["rate_only"].append([int(a[0][0]), int(a[1][0])]), R.VOID)
    pc["tx_hook_branch"] = lambda it, a: (log["branch"].append([int(a[0][0]), int(a[1][0])]), R.VOID)
    pc["tx_hook_best"] = lambda it, a: (log.__setitem__("best_rd", int(a[0][0])), R.VOID)

    def py_fwd(it, a):
        s, dst, stride, prm = a[0][0], a[1][0], int(a[2][0]), a[3][0]
        blk = np.array([[s.buf[s.off + r * stride + c] for c in range(w)] for r in range(h)], np.int16)
        out = orc.fwd_txfm2d(blk, tx_size, int(ev.get(prm, "tx_type")), bd).ravel()
        for k_, v in enumerate(out):
            dst.buf[dst.off + k_] = int(v)
        return None, R.VOID

    def py_quant(hb):
        def f(it, a):
            co, n = a[0][0], int(a[1][0])
            c = np.array([co.buf[co.off + k_] for k_ in range(n)], np.int32)
            t = log["visit"][-1]
            scan, iscan = orc.get_scan(tx_size, t)
            qc, dq, eob = orc.quantize_b(c, q, scan, iscan, int(ev.call("av1_get_tx_scale", tx_size)), highbd=hb)
            for nm_, arr in ((3, qc), (4, dq)):
                p_ = a[nm_][0]
                for k_, v in enumerate(arr):
                    p_.buf[p_.off + k_] = int(v)
            a[5][0].buf[a[5][0].off] = int(eob)
            return None, R.VOID
        return f

    def py_inv(it, a):   # av1_inverse_transform_block(xd, dqcoeff, plane, tx_type, tx_size, dst, stride, eob, reduced_tx_set)
        dqp, t, dst, stride, eob = a[1][0], int(a[3][0]), a[5][0], int(a[6][0]), int(a[7][0])
        if not eob:
            return None, R.VOID
        dq = np.array([dqp.buf[dqp.off + k_] for k_ in range(nc)], np.int32)
        tile = np.array([[dst.buf[dst.off + r * stride + c] for c in range(w)] for r in range(h)], np.uint16)
        rec = orc.inv_txfm2d_add(dq, tile, tx_size, t, bd)
        for r in range(h):
            for c in range(w):
                dst.buf[dst.off + r * stride + c] = int(rec[r, c])
        return None, R.VOID

    def get_scan(it, a):
        t = int(a[1][0])
        scan, iscan = orc.get_scan(tx_size, t)
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
        ev.call("search_tx_type", cpi, x, 0, 0, 0, 0, bsize, tx_size, tctx, 0, 1, cs["ref_best_rd"], stats)
    finally:
        for nm, f in saved.items():
            ev.interp.funcs[nm] = f
            pc.pop(nm, None)
        pc["get_scan"] = old_scan
    rec = dict(cs)
    rec.update({"skip_ctx": skip_ctx, "dc_ctx": dc_ctx, "tx_type_costs": tx_type_costs, "visit": log["visit"], "rate_only": log["rate_only"], "branch": log["branch"],
                "types": {str(k): [v[0], v[1], v[2], str(v[3]), str(v[4])] for k, v in log["types"].items()},
                "block_sse": str(log["flags"][0]), "block_mse_q8": log["flags"][1], "use_txd_flag": log["flags"][2], "calc_final": log["flags"][3],
                "best_rd": str(log["best_rd"]), "rate": int(ev.get(stats, "rate")), "dist": str(int(ev.get(stats, "dist"))), "sse": str(int(ev.get(stats, "sse"))),
                "skip_txfm": int(ev.get(stats, "skip_txfm")), "best_eob": int(ev.field(x, "plane[0].eobs").deref()[0].buf[0]),
                "best_ctx": int(ev.field(x, "plane[0].txb_entropy_ctx").deref()[0].buf[0]),
                "best_tx_type": int(ev.field(x, "e_mbd.tx_type_map").deref()[0].buf[0])})
    pt = np.uint16 if hbd else np.uint8
    rec["costs"] = "costs_%d_%d" % (tx_size, bd)
    arrays = {"src": src.astype(pt), "pred": pred.astype(pt)}
    return rec, arrays, {rec["costs"]: costs.astype(np.int32)}


def plan_cases(rng):
    plan = []
    per_size = [0]

    def add(tx_size, bd, **kw):
        sm = set_mask_of(tx_size)
        c = dict(tx_size=tx_size, bd=bd, qindex=120, amp=30 << (bd - 8), vis_cols=TXW[tx_size], vis_rows=TXH[tx_size], mask=sm, single=None, txk_map=None,
                 use_txd=0, threshold=0, low_txfm_rd=0, psy=0, adaptive=0, skip_tx_search=0, rdmult=int(rng.integers(60, 3000)), ref_best_rd=INT64_MAX)
        c.update(kw)
        c["mask"] &= sm
        per_size[0] += 1
        if TXW[tx_size] * TXH[tx_size] == 4096 and per_size[0] - 1 not in (0, 2, 4, 15, 16, 18, 21, 23, 25, 27, 28, 29, 30, 31):
            return   # TX_64X64 has one type and 8 KB of pixels per case: the cases that differ from their neighbours in the order or the mask only are left out
        if c["txk_map"] is not None and not any(t < 16 and (c["mask"] >> t) & 1 for t in c["txk_map"]):   # (an order that leaves the loop nothing to visit)
            c["txk_map"] = [c["mask"].bit_length() - 1 if k == c["txk_map"].index(255) else t for k, t in enumerate(c["txk_map"])]
        plan.append(c)
    sizes = (0, 1, 2, 3, 4, 17, 13, 14, 15)   # 4x4 8x8 16x16 32x32 64x64 16x64 4x16 16x4 8x32
    for tx_size in sizes:
        w, h = TXW[tx_size], TXH[tx_size]
        sm = set_mask_of(tx_size)
        per_size[0] = 0
        perm = [int(v) for v in rng.permutation(16)]
        perm2 = [int(v) if k % 3 else 255 for k, v in enumerate(rng.permutation(16))]
        for bd in (8, 10, 12):
            add(tx_size, bd)                                                    # pixel domain, every type of the set
            add(tx_size, bd, use_txd=2, qindex=160)                             # transform domain
        add(tx_size, 8, use_txd=1, txk_map=perm)                                # transform domain + the final recomputation, a permuted order
        add(tx_size, 10, use_txd=1, txk_map=perm2, qindex=60)
        add(tx_size, 8, use_txd=1, single=0, mask=0x0001)                       # ... suppressed through txk_allowed
        add(tx_size, 10, use_txd=1, single=0, mask=0x0001, qindex=90)
        add(tx_size, 8, use_txd=1, mask=0x0001)                                 # ... and through mask 0x0001
        add(tx_size, 12, use_txd=1, mask=0x0001, qindex=90)
        add(tx_size, 8, use_txd=1, low_txfm_rd=1)                               # LOW_TXFM_RD: no final recomputation
        add(tx_size, 8, use_txd=2, threshold=1 << 30)                           # below the mse threshold: pixel domain after all
        add(tx_size, 10, use_txd=1, psy=1)                                      # AOM_CONTENT_PSY switches the transform domain off
        add(tx_size, 8, qindex=255, amp=2)                                      # eob 0 everywhere
        add(tx_size, 10, qindex=255, amp=2 << 2, skip_tx_search=1)              # ... and the skip_tx_search break
        add(tx_size, 8, qindex=255, amp=3, skip_tx_search=1, txk_map=perm)
        add(tx_size, 8, adaptive=1, ref_best_rd=1000)                           # the adaptive_txb_search_level break
        add(tx_size, 10, adaptive=2, ref_best_rd=5000, txk_map=perm)
        add(tx_size, 8, adaptive=1, ref_best_rd=1 << 50)                        # ... not taken
        add(tx_size, 8, rdmult=1 << 22, qindex=40, amp=60)                      # rate dominates: the rate-only `continue`
        add(tx_size, 10, rdmult=1 << 24, qindex=40, amp=60 << 2, txk_map=perm)
        add(tx_size, 8, vis_cols=max(1, w - 3), qindex=100)                     # clipped at the right edge
        add(tx_size, 10, vis_cols=max(1, w // 2), qindex=100)
        add(tx_size, 8, vis_rows=max(1, h - 3), qindex=100)                     # ... at the bottom edge
        add(tx_size, 12, vis_rows=max(1, h // 2), vis_cols=max(1, w - 1), qindex=100)
        add(tx_size, 8, saturate=1, qindex=255)                                 # high energy
        add(tx_size, 10, saturate=1, qindex=200)
        add(tx_size, 8, saturate=2, qindex=255)
        add(tx_size, 12, saturate=2, qindex=230)
        add(tx_size, 8, qindex=255, amp=2, equal_types=1, txk_map=perm)         # every type costs the same: the first visited must win
        add(tx_size, 8, amp=0, qindex=20, equal_types=1, txk_map=perm2)
        if sm != 1:
            add(tx_size, 8, mask=sm & ~1, gx=3, qindex=80)                      # DCT_DCT not allowed
            add(tx_size, 10, mask=sm & 0x0A0A, gy=3, qindex=80)
    return plan


def coverage(cases):
    """How many cases reach each path the issue names (recomputed from the records)."""
    n = {}

    def hit(k):
        n[k] = n.get(k, 0) + 1
    for c in cases:
        w, h = TXW[c["tx_size"]], TXH[c["tx_size"]]
        bs = int(c["block_sse"])
        high = bs >= 128 * 128 * w * h
        tx64 = w == 64 and h == 64
        repl = {t for t, k_ in c["branch"] if k_ == 1}
        added = {t for t, k_ in c["branch"] if k_ == 2}
        br = set()
        for t, (rate, eob, ctx, dist, sse) in c["types"].items():
            if eob == 0:
                br.add("eob0")
            elif c["use_txd_flag"]:
                br.add("txd")
            elif int(t) in added:
                br.add("sse_diff_added")          # TX_64X64 and high energy with sse_diff * 2 >= sse
            elif int(t) in repl:
                br.add("px_replaced")             # high energy with the dist < tx_domain_dist replacement
            else:
                br.add("px")
                if tx64 or high:
                    br.add("px_after_tx_domain")  # TX_64X64 or high energy, pixel domain taken after the transform-domain pass
        for b_ in br:
            hit(b_)
        if c["calc_final"] and c["best_eob"]:
            hit("final")
        if c["use_txd"] == 1 and not c["calc_final"] and c["single"] is not None and c["block_mse_q8"] >= c["threshold"] and not c["psy"] and max(w, h) != 64:
            hit("final_off_txk_allowed")
        if c["use_txd"] == 1 and not c["calc_final"] and c["single"] is None and c["mask"] == 1 and not c["psy"] and max(w, h) != 64 and not c["low_txfm_rd"]:
            hit("final_off_mask1")
        n_allowed = len([t for t in (c["txk_map"] or range(16)) if t < 16 and (c["mask"] >> t) & 1])
        if len(c["visit"]) < n_allowed:
            hit("break_skip" if c["skip_tx_search"] and c["best_eob"] == 0 else "break_adaptive")
        if c["rate_only"]:
            hit("rate_only")
        if c["best_tx_type"] != 0:
            hit("winner_not_dct")
        if c["txk_map"] is not None and len(c["visit"]) > 1:
            hit("txk_map")
        if c["vis_cols"] < w:
            hit("clip_right")
        if c["vis_rows"] < h:
            hit("clip_bottom")
        hit("bd%d" % c["bd"])
        rds = {}
        for t, (rate, eob, ctx, dist, sse) in c["types"].items():
            rds.setdefault(((rate * c["rdmult"] + 256) >> 9) + int(dist) * 128, []).append(int(t))
        if rds and str(min(rds)) == c["best_rd"] and len(rds[min(rds)]) > 1:
            hit("tie")
    return n


def main():
    import time
    import pyoracle as orc
    ev, state = make_evaluator()
    rng = np.random.default_rng(20261021)
    arrays, cases = {}, []
    t0 = time.time()
    for k, cs in enumerate(plan_cases(rng)):
        rec, arr, shared = run_case(ev, state, orc, rng, cs)
        rec["k"] = k
        arrays.update(shared)
        cases.append(rec)
        for nm, v in arr.items():
            arrays["%s%d" % (nm, k)] = v
        print(k, TXW[cs["tx_size"]], TXH[cs["tx_size"]], cs["bd"], rec["visit"], rec["best_tx_type"], rec["best_eob"], rec["rate"], rec["dist"],
              "%.0f s" % (time.time() - t0), flush=True)
    cov = coverage(cases)
    print(cov)
    need = ("eob0", "txd", "px", "sse_diff_added", "px_replaced", "px_after_tx_domain", "final", "final_off_txk_allowed", "final_off_mask1", "break_skip", "break_adaptive", "rate_only",
            "winner_not_dct", "txk_map", "tie", "clip_right", "clip_bottom", "bd8", "bd10", "bd12")
    assert all(cov.get(k_, 0) >= 2 for k_ in need), {k_: cov.get(k_, 0) for k_ in need}
    save("ref_eval_tx_type.npz", arrays, cases)


if __name__ == "__main__":
    main()
