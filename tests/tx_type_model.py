"""search_tx_type (av1/encoder/tx_search.c:2019-2335) in plain integers: the per-type table from oracle calls (forward transform, B quantiser, the
level-map rate, the entropy context, the block error, the inverse transform) and the loop of :2145-2309 with the function's tail as a walk over that
table.  What aomhip_search_tx_type_batch computes on the device, stated once on the host; tests/test_golden_tx_type.py holds it to the interpreted
reference's record, tests/test_gpu_tx_type.py holds the device to it."""
import ctypes as C

import numpy as np

import pyoracle as orc

TXW = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TXH = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
INT64_MAX = (1 << 63) - 1
INVALID = 255
K_SKIP = 0   # txb_skip_cost[13][2] is the head of the 966-int cost table


def tx_type_exists(tx_size, t):
    """av1_get_fwd_txfm_cfg's reach: ADST up to 16 points, identity up to 32, 64 DCT only."""
    vk = [0, 1, 0, 1, 2, 0, 2, 1, 2, 3, 0, 3, 1, 3, 2, 3][t]
    hk = [0, 0, 1, 1, 0, 2, 2, 2, 1, 3, 3, 0, 3, 1, 3, 2][t]
    lim = {0: 64, 1: 16, 2: 16, 3: 32}
    return TXH[tx_size] <= lim[vk] and TXW[tx_size] <= lim[hk]


def tx_scale(tx_size):
    n = TXW[tx_size] * TXH[tx_size]
    return (n > 256) + (n > 1024)


def rdcost(rdmult, rate, dist):
    return ((rate * rdmult + 256) >> 9) + dist * 128   # RDCOST, rd.h:31-33


def round_pow2(v, n):
    return (v + ((1 << n) >> 1)) >> n


def _p(a):
    return C.c_void_p(a.ctypes.data)


def block_scalars(src, pred, tx_size, bd, vis_cols, vis_rows, mask, txk_allowed_single, use_txd_param, threshold, low_txfm_rd, sse=None):
    """:2076-2130: block_sse, block_mse_q8 and the two distortion-mode flags (sse: the visible residual's squared sum where the caller has it already)."""
    if sse is None:
        d = src.astype(np.int64) - pred.astype(np.int64)
        sse = int((d[:vis_rows, :vis_cols] ** 2).sum())
    mse_q8 = (256 * sse) // (vis_cols * vis_rows)
    if bd > 8:
        sse = round_pow2(sse, (bd - 8) * 2)
        mse_q8 = round_pow2(mse_q8, (bd - 8) * 2)
    block_sse = sse * 16
    use_txd = int(use_txd_param > 0 and mse_q8 >= threshold and max(TXW[tx_size], TXH[tx_size]) != 64)
    calc_final = int(use_txd_param == 1 and use_txd and not low_txfm_rd)
    if calc_final and (txk_allowed_single or mask == 0x0001):
        calc_final = use_txd = 0
    return dict(block_sse=block_sse, block_mse_q8=mse_q8, use_txd=use_txd, calc_final=calc_final)


def entry_from_parts(tx_size, bd, info, eob, rate, ctx, err, ssz, px_sse):
    """:2185-2236 on a type's parts: err / ssz = av1_[highbd_]block_error's two results (rounded for the depth), px_sse() = the raw squared error of the
    reconstruction over the visible part.  -> dict(rate, eob, ctx, dist, sse, px_dist)"""
    w, h = TXW[tx_size], TXH[tx_size]
    shift = (1 - tx_scale(tx_size)) * 2
    td, ts = (err << -shift, ssz << -shift) if shift < 0 else (err >> shift, ssz >> shift)   # dist_block_tx_domain's RIGHT_SIGNED_SHIFT

    def px_domain():   # pixel_dist_visible_only's rounding, an unsigned; times 16 in 32 bits (:1015)
        s = px_sse()
        if bd > 8:
            s = round_pow2(s, (bd - 8) * 2)
        return 16 * (s & 0xFFFFFFFF) & 0xFFFFFFFF

    block_sse = info["block_sse"]
    tx64 = w == 64 and h == 64
    high = block_sse >= 128 * 128 * w * h
    px = -1
    if eob == 0:
        dist = sse = block_sse
    elif info["use_txd"]:
        dist, sse = td, ts
        if info["calc_final"]:
            px = px_domain()
    else:
        dist, sse_diff = INT64_MAX, INT64_MAX
        if tx64 or high:
            dist, sse_diff = td, block_sse - ts
        if not tx64 or not high or sse_diff * 2 < ts:
            tx_domain_dist = dist
            dist = px = px_domain()
            if high and dist < tx_domain_dist:
                dist = tx_domain_dist
        else:
            dist += sse_diff
        sse = block_sse
    return dict(rate=rate, eob=int(eob), ctx=ctx, dist=int(dist), sse=int(sse), px_dist=int(px))


def evaluate_type(src, pred, tx_size, t, bd, q, costs, tx_type_cost, skip_ctx, dc_ctx, vis_cols, vis_rows, info, want_coeffs=False):
    """What this_rd_stats, the eob and the entropy context would hold if the loop reached type t: dict(rate, eob, ctx, dist, sse, px_dist)."""
    w, h = TXW[tx_size], TXH[tx_size]
    nc = min(w, 32) * min(h, 32)
    hbd = bd > 8
    res = (src.astype(np.int32) - pred.astype(np.int32)).astype(np.int16)
    coeff = np.ascontiguousarray(orc.fwd_txfm2d(res, tx_size, t, bd)[:nc])
    scan, iscan = orc.get_scan(tx_size, t)
    qc, dq, eob = orc.quantize_b(coeff, q, scan, iscan, tx_scale(tx_size), highbd=hbd)
    sc, cs = np.ascontiguousarray(scan, np.int16), np.ascontiguousarray(costs, np.int32)
    tx_class = 0 if t < 10 else (2 if t % 2 == 0 else 1)
    if eob == 0:
        rate = int(cs[K_SKIP + skip_ctx * 2 + 1])
    else:
        rate = int(orc.lib.orc_cost_coeffs_txb(_p(qc), eob, w, h, tx_class, _p(sc), skip_ctx, dc_ctx, _p(cs))) + int(tx_type_cost)
    ctx = int(orc.lib.orc_get_txb_entropy_context(_p(qc), _p(sc), eob))
    f = orc.lib.orc_block_error
    f.restype = C.c_int64
    ssz = C.c_int64()
    err = int(f(_p(coeff), _p(dq), C.c_ssize_t(nc), C.byref(ssz), C.c_int(bd if hbd else 0)))
    def px_sse():   # the reconstruction's squared error over the visible part (dist_block_px_domain, :969-1017)
        rec = orc.inv_txfm2d_add(dq, pred.astype(np.uint16), tx_size, t, bd).astype(np.int64)
        return int(((src.astype(np.int64) - rec)[:vis_rows, :vis_cols] ** 2).sum())
    out = entry_from_parts(tx_size, bd, info, int(eob), rate, ctx, err, ssz.value, px_sse)
    if want_coeffs:
        out["qcoeff"], out["dqcoeff"] = qc, dq
    return out


def table(src, pred, tx_size, bd, q, costs, tx_type_costs, skip_ctx, dc_ctx, vis_cols, vis_rows, mask, info):
    """The 16 entries of a block: None where the type is outside the mask or does not exist for the size."""
    return [evaluate_type(src, pred, tx_size, t, bd, q, costs, tx_type_costs[t], skip_ctx, dc_ctx, vis_cols, vis_rows, info)
            if (mask >> t) & 1 and tx_type_exists(tx_size, t) else None for t in range(16)]


def walk(tab, info, mask, txk_map, rdmult, ref_best_rd, adaptive_level, skip_tx_search):
    """:2145-2328 on the table -> (result dict, the types visited in order)."""
    best_rd, best_eob, best_type, best_ctx = INT64_MAX, 0, INVALID, 0
    rate, dist, sse = (1 << 31) - 1, INT64_MAX, INT64_MAX   # av1_invalid_rd_stats
    visited = []
    for idx in range(16):
        t = idx if txk_map is None else int(txk_map[idx])
        if t > 15 or not (mask >> t) & 1 or tab[t] is None:
            continue
        e = tab[t]
        visited.append(t)
        if rdcost(rdmult, e["rate"], 0) > best_rd:
            continue
        rd = rdcost(rdmult, e["rate"], e["dist"])
        if rd < best_rd:
            best_rd, best_type, best_ctx, best_eob = rd, t, e["ctx"], e["eob"]
            rate, dist, sse = e["rate"], e["dist"], e["sse"]
        if adaptive_level and (best_rd - (best_rd >> adaptive_level)) > ref_best_rd:
            break
        if skip_tx_search and not best_eob:
            break
    final = bool(best_type != INVALID and info["calc_final"] and best_eob)
    if final:
        dist, sse = tab[best_type]["px_dist"], info["block_sse"]
    return dict(best_rd=best_rd, best_tx_type=best_type, best_eob=best_eob, txb_entropy_ctx=best_ctx, rate=rate, dist=dist, sse=sse,
                skip_txfm=int(best_eob == 0), final_px=int(final)), visited


# ---- the fixture of tests/golden/gen_ref_eval_tx_type.py

def golden():
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_eval_tx_type.npz"))
    return z, json.loads(bytes(z["cases"]))


def case_inputs(z, c):
    """A stored case as the model's (and the device call's) inputs."""
    return dict(src=z["src%d" % c["k"]].astype(np.int64), pred=z["pred%d" % c["k"]].astype(np.int64), costs=z[c["costs"]], q=orc.build_quantizer_y(c["bd"], c["qindex"]),
                use_txd_param=0 if c["psy"] else c["use_txd"], single=int(c["single"] is not None))


def model_case(z, c):
    """-> (info, table, result, visited) of a stored case."""
    i = case_inputs(z, c)
    info = block_scalars(i["src"], i["pred"], c["tx_size"], c["bd"], c["vis_cols"], c["vis_rows"], c["mask"], i["single"], i["use_txd_param"], c["threshold"],
                         c["low_txfm_rd"])
    tab = table(i["src"], i["pred"], c["tx_size"], c["bd"], i["q"], i["costs"], c["tx_type_costs"], c["skip_ctx"], c["dc_ctx"], c["vis_cols"], c["vis_rows"],
                c["mask"], info)
    res, visited = walk(tab, info, c["mask"], c["txk_map"], c["rdmult"], c["ref_best_rd"], c["adaptive"], c["skip_tx_search"])
    return info, tab, res, visited
