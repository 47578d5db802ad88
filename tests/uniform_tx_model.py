"""The uniform transform-size search of an inter block's luma plane (av1/encoder/tx_search.c) in plain integers, on tests/tx_type_model.py's table:
block_rd_txfm under av1_txfm_rd_in_plane (:2935-3014, :3692-3735), av1_uniform_txfm_yrd (:3140-3199) and choose_tx_size_type_from_rd /
choose_largest_tx_size (:2838-2931, :2659-2754).  Every transform block's table is computed under its REAL entropy contexts here -- the device computes
it under (0, 0) and re-bases the rates --, so agreement checks that identity too.  tests/test_golden_uniform_tx.py holds this model to the interpreted
reference's record (tests/golden/ref_eval_uniform_tx.npz), tests/test_gpu_uniform_tx.py holds the device to both."""
import numpy as np

import tx_type_model as M

INT64_MAX = M.INT64_MAX
INT_MAX = (1 << 31) - 1
MAX_TX_DEPTH = 2
# block_size_wide / block_size_high in BLOCK_SIZE order (av1/common/enums.h:99-124)
BSW = [4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64]
BSH = [4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16]


def bsize_of(bw, bh):
    return [i for i in range(22) if BSW[i] == bw and BSH[i] == bh][0]


def tx_of(w, h):
    return [i for i in range(19) if M.TXW[i] == w and M.TXH[i] == h][0]


def sub_tx(tx):
    """sub_tx_size_map from the dimensions: a square halves, 2:1 becomes the square of its shorter side, 4:1 halves its longer side"""
    w, h = M.TXW[tx], M.TXH[tx]
    if w == h:
        return tx if w == 4 else tx_of(w // 2, h // 2)
    if w == 2 * h or h == 2 * w:
        return tx_of(min(w, h), min(w, h))
    return tx_of(w // 2, h) if w > h else tx_of(w, h // 2)


def max_rect_tx(bsize):
    return tx_of(min(BSW[bsize], 64), min(BSH[bsize], 64))


def depth_plan(bsize, tx_select, mode_tx_size, init_depth, enable_tx64, enable_rect_tx, use_largest):
    """-> dict(init_depth, use_largest, entries=[(depth, tx_size)]): the loop of :2880-2917 / choose_largest_tx_size's size"""
    has64 = lambda tx: max(M.TXW[tx], M.TXH[tx]) == 64
    if use_largest:
        w, h = M.TXW[mode_tx_size], M.TXH[mode_tx_size]
        if not enable_rect_tx:
            w = h = min(w, h)
        if not enable_tx64:
            w, h = min(w, 32), min(h, 32)
        return dict(init_depth=0, use_largest=1, entries=[(0, tx_of(w, h))])
    if tx_select:
        start = max_rect_tx(bsize)
        if init_depth == MAX_TX_DEPTH and not enable_tx64 and has64(start):
            start = sub_tx(start)
    else:
        start, init_depth = mode_tx_size, MAX_TX_DEPTH
    entries, tx = [], start
    for depth in range(init_depth, MAX_TX_DEPTH + 1):
        if not ((not enable_tx64 and has64(tx)) or (not enable_rect_tx and M.TXW[tx] != M.TXH[tx])):
            entries.append((depth, tx))
            if tx == 0:
                break
        tx = sub_tx(tx)
    return dict(init_depth=init_depth, use_largest=0, entries=entries)


def visit_order(mbw, mbh, txw4, txh4):
    """av1_foreach_transformed_block_in_plane (encodemb.c:551-591) -> [(blk_row, blk_col)]"""
    out = []
    mu_w, mu_h = min(16, mbw), min(16, mbh)
    for r in range(0, mbh, mu_h):
        for c in range(0, mbw, mu_w):
            for row in range(r, min(mu_h + r, mbh), txh4):
                for col in range(c, min(mu_w + c, mbw), txw4):
                    out.append((row, col))
    return out


def max_blocks(env, blk):
    """max_block_wide / max_block_high: the frame's extent is mi_cols / mi_rows, the size aligned to 8 samples"""
    mi_w4, mi_h4 = ((env["W"] + 7) & ~7) >> 2, ((env["H"] + 7) & ~7) >> 2
    return min(env["bw"] >> 2, mi_w4 - (blk["x"] >> 2)), min(env["bh"] >> 2, mi_h4 - (blk["y"] >> 2))


def get_txb_ctx(whole, a, l):
    """txb_common.h:446-460, plane 0 -> (txb_skip_ctx, dc_sign_ctx)"""
    dc = sum({0: 0, 1: -1, 2: 1}[v >> 3] for v in list(a) + list(l))
    dc_ctx = 1 if dc < 0 else (2 if dc > 0 else 0)
    if whole:
        return 0, dc_ctx
    top = left = 0
    for v in a:
        top |= v
    for v in l:
        left |= v
    top, left = min(top & 7, 4), min(left & 7, 4)
    return [[1, 2, 2, 2, 3], [2, 4, 4, 4, 5], [2, 4, 4, 4, 5], [2, 4, 4, 4, 5], [3, 5, 5, 5, 6]][top][left], dc_ctx


def txb_tiles(env, blk, tx_size, row, col):
    """the transform block's source and predictor tiles (the planes' edges replicated past the frame) and get_txb_dimensions' visible extent"""
    w, h, pad = M.TXW[tx_size], M.TXH[tx_size], env["pad"]
    x, y = blk["x"] + col * 4, blk["y"] + row * 4
    mi_w, mi_h = (env["W"] + 7) & ~7, (env["H"] + 7) & ~7
    s = env["src"][pad + y:pad + y + h, pad + x:pad + x + w]
    p = env["pred"][pad + y:pad + y + h, pad + x:pad + x + w]
    return s, p, min(w, mi_w - x), min(h, mi_h - y)


def search_txb(env, blk, tx_size, dp, k, row, col, skip_ctx, dc_ctx, ref_best_rd):
    """search_tx_type for visited transform block k under its contexts -> tx_type_model.walk's result"""
    s, p, vc, vr = txb_tiles(env, blk, tx_size, row, col)
    mask = (dp["masks"][k] if dp.get("masks") is not None else 0xFFFF) & dp["mask_limit"]
    single = int(dp["single"][k]) if dp.get("single") is not None else 0
    info = M.block_scalars(s, p, tx_size, env["bd"], vc, vr, mask, single, dp["use_txd"], dp["threshold"], dp["low_txfm_rd"])
    tab = M.table(s, p, tx_size, env["bd"], env["q"], dp["costs"], dp["tx_type_costs"], skip_ctx, dc_ctx, vc, vr, mask, info)
    res, visited = M.walk(tab, info, mask, None, blk["rdmult"], ref_best_rd, dp["adaptive"], dp["skip_tx_search"])
    res["n_visited"], res["vis_cols"], res["vis_rows"] = len(visited), vc, vr
    return res


def txfm_rd_in_plane(env, blk, tx_size, dp, current_rd, search=search_txb):
    """av1_txfm_rd_in_plane with block_rd_txfm as the visitor -> dict(valid, rate, dist, sse, skip_txfm, current_rd, txbs); txbs: one record per transform
    block search_tx_type ran on, in visiting order"""
    best_rd = blk["ref_best_rd"]
    out = dict(valid=False, rate=INT_MAX, dist=INT64_MAX, sse=INT64_MAX, skip_txfm=0, current_rd=current_rd, txbs=[], entry_refused=False, incomplete=False,
               last_exit=False)
    if current_rd > best_rd:   # :3705-3708
        out["entry_refused"] = True
        return out
    txw4, txh4 = M.TXW[tx_size] >> 2, M.TXH[tx_size] >> 2
    whole = M.TXW[tx_size] == env["bw"] and M.TXH[tx_size] == env["bh"]
    above, left = [int(v) for v in blk["above_ctx"]], [int(v) for v in blk["left_ctx"]]
    rate, dist, sse, skip = 0, 0, 0, 1
    exit_early = incomplete = False
    mbw, mbh = max_blocks(env, blk)
    for k, (row, col) in enumerate(visit_order(mbw, mbh, txw4, txh4)):
        if exit_early:
            incomplete = True
            break
        skip_ctx, dc_ctx = get_txb_ctx(whole, above[col:col + txw4], left[row:row + txh4])
        ref = best_rd - current_rd
        r = search(env, blk, tx_size, dp, k, row, col, skip_ctx, dc_ctx, ref)
        out["txbs"].append(dict(row=row, col=col, skip_ctx=skip_ctx, dc_ctx=dc_ctx, ref_best_rd=ref, tx_type=r["best_tx_type"], eob=r["best_eob"],
                                ctx=r["txb_entropy_ctx"], rate=r["rate"], dist=r["dist"], sse=r["sse"], n_visited=r.get("n_visited"),
                                partly_visible=r.get("vis_cols", M.TXW[tx_size]) < M.TXW[tx_size] or r.get("vis_rows", M.TXH[tx_size]) < M.TXH[tx_size]))
        if r["best_tx_type"] == M.INVALID:   # (a transform block without an allowed type: the device reports it and invalidates the block)
            incomplete = True
            break
        above[col:col + txw4] = [r["txb_entropy_ctx"]] * txw4   # av1_set_txb_context: not clipped at the frame edge
        left[row:row + txh4] = [r["txb_entropy_ctx"]] * txh4
        rd = min(M.rdcost(blk["rdmult"], r["rate"], r["dist"]), M.rdcost(blk["rdmult"], 0, r["sse"]))
        skip &= int(r["best_eob"] == 0)
        rate, dist, sse = min(rate + r["rate"], INT_MAX), dist + r["dist"], sse + r["sse"]   # av1_merge_rd_stats
        current_rd += rd
        if current_rd > best_rd:
            exit_early = True
    out["incomplete"], out["last_exit"], out["current_rd"] = incomplete, exit_early and not incomplete, current_rd
    out["crosses"] = (mbw < env["bw"] >> 2, mbh < env["bh"] >> 2)   # the right / the bottom frame edge
    if not incomplete and rate != INT_MAX:
        out.update(valid=True, rate=rate, dist=dist, sse=sse, skip_txfm=skip)
    return out


def uniform_txfm_yrd(env, blk, tx_size, dp, entry=0, search=search_txb):
    """av1_uniform_txfm_yrd -> txfm_rd_in_plane's dict with rd (the return value) and the stats after the tail; forced_skip: :3190 taken"""
    rdmult, tsr = blk["rdmult"], blk["tx_size_rate"][entry]
    cur = min(M.rdcost(rdmult, blk["no_skip_txfm_rate"] + tsr, 0), M.rdcost(rdmult, blk["skip_txfm_rate"], 0))
    o = txfm_rd_in_plane(env, blk, tx_size, dp, cur, search)
    o["forced_skip"] = False
    if not o["valid"]:
        o["rd"] = INT64_MAX
        return o
    if o["skip_txfm"]:
        rd = M.rdcost(rdmult, blk["skip_txfm_rate"], o["sse"])
    else:
        rd = M.rdcost(rdmult, o["rate"] + blk["no_skip_txfm_rate"] + tsr, o["dist"])
        o["rate"] += tsr
        forced = M.rdcost(rdmult, blk["skip_txfm_rate"], o["sse"])
        if forced <= rd:
            rd, o["rate"], o["dist"], o["skip_txfm"], o["forced_skip"] = forced, 0, o["sse"], 1, True
    o["rd"] = rd
    return o


def pick_uniform(env, blk, plan, dps, search=search_txb):
    """choose_tx_size_type_from_rd (choose_largest_tx_size when plan["use_largest"]) -> dict(tx_size (255: left alone), rd, rate, dist, sse, skip_txfm,
    depth_rd[3], txbs of the winning depth, depths: per plan entry what uniform_txfm_yrd returned (None: not evaluated), lowvar: the break's outcome)"""
    out = dict(tx_size=255, rd=INT64_MAX, rate=INT_MAX, dist=INT64_MAX, sse=INT64_MAX, skip_txfm=0, depth_rd=[INT64_MAX] * 3, txbs=[], depths=[None] * len(dps),
               lowvar=None)
    if plan["use_largest"]:
        tx = plan["entries"][0][1]
        cur = min(M.rdcost(blk["rdmult"], blk["no_skip_txfm_rate"], 0), M.rdcost(blk["rdmult"], blk["skip_txfm_rate"], 0))
        o = txfm_rd_in_plane(env, blk, tx, dps[0], cur, search)
        out["depths"][0] = o
        out.update(tx_size=tx, txbs=o["txbs"], rate=o["rate"], dist=o["dist"], sse=o["sse"], skip_txfm=o["skip_txfm"])
        if o["valid"]:
            out["rd"] = out["depth_rd"][0] = o["current_rd"]
        return out
    first = True
    for k, (depth, tx) in enumerate(plan["entries"]):
        o = uniform_txfm_yrd(env, blk, tx, dps[k], k, search)
        out["depths"][k] = o
        out["depth_rd"][depth] = o["rd"]
        if o["rd"] < out["rd"]:
            out.update(tx_size=tx, rd=o["rd"], rate=o["rate"], dist=o["dist"], sse=o["sse"], skip_txfm=o["skip_txfm"], txbs=o["txbs"])
        elif first:
            out["txbs"] = o["txbs"]   # (no winner yet: the device leaves the first entry's visit in the per-transform-block records)
        first = False
        if tx == 0:
            break
        if depth > plan["init_depth"] and depth != MAX_TX_DEPTH and blk["source_variance"] < 256:
            prev = out["depth_rd"][depth - 1]
            taken = prev != INT64_MAX and o["rd"] > prev
            out["lowvar"] = ("taken", None) if taken else ("not taken", "order" if prev != INT64_MAX else "guard")
            if taken:
                break
        elif depth > plan["init_depth"] and depth != MAX_TX_DEPTH:
            out["lowvar"] = ("not taken", "variance")
    return out


# ---- host loop of the header's comment: the per-transform-block records -> tx_type_map entries at the visited origins and blk_skip

def maps_from_records(env, blk, tx_size, txbs):
    """-> ({(blk_row, blk_col): tx_type} with update_txk_array's extra 16x16-unit entries for the 64-point sizes, {blk_idx: blk_skip})"""
    txw4, txh4 = M.TXW[tx_size] >> 2, M.TXH[tx_size] >> 2
    mbw, mbh = max_blocks(env, blk)
    type_map, blk_skip = {}, {}
    for (row, col), t in zip(visit_order(mbw, mbh, txw4, txh4), txbs):
        blk_skip[row * (env["bw"] >> 2) + col] = int(t["eob"] == 0)
        type_map[(row, col)] = t["tx_type"]
        if txw4 == 16 or txh4 == 16:
            for idy in range(0, txh4, 4):
                for idx in range(0, txw4, 4):
                    type_map[(row + idy, col + idx)] = t["tx_type"]
    return type_map, blk_skip


# ---- the fixture of tests/golden/gen_ref_eval_uniform_tx.py

def golden():
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_eval_uniform_tx.npz"))
    return z, json.loads(bytes(z["cases"]))


def case_costs(z, tx_size):
    """the 966-int cost table of a transform size: the fixture's table of its size context, then the eob table of its eob size class"""
    return np.concatenate([z["coeff_costs"][int(z["txs_ctx"][tx_size])], z["eob_costs"][int(z["eob_class"][tx_size])]]).astype(np.int32)


def case_inputs(z, c, arrays=None):
    """A stored case as the model's inputs -> (env, blk, plan, dps); arrays: the generator's own src / pred before they are stored"""
    import pyoracle as orc
    bw, bh, W, H = BSW[c["bsize"]], BSH[c["bsize"]], c["vis_w"], c["vis_h"]
    src = (arrays["src"] if arrays else z["src%d" % c["k"]]).astype(np.int64)
    pred = (arrays["pred"] if arrays else z["pred%d" % c["k"]]).astype(np.int64)
    pad = 128
    env = dict(src=np.pad(src, pad, mode="edge"), pred=np.pad(pred, pad, mode="edge"), pad=pad, W=W, H=H, bd=c["bd"], q=orc.build_quantizer_y(c["bd"], c["qindex"]),
               bw=bw, bh=bh)
    plan = depth_plan(c["bsize"], c["tx_select"], c["mode_tx_size"], c["init_depth"], c["enable_tx64"], c["enable_rect_tx"], c["use_largest"])
    blk = dict(x=0, y=0, rdmult=c["rdmult"], source_variance=c["source_variance"], ref_best_rd=c["ref_best_rd"],
               tx_size_rate=[c["tx_size_rate"][str(tx)] for _, tx in plan["entries"]] + [0] * 3, no_skip_txfm_rate=c["no_skip_txfm_rate"],
               skip_txfm_rate=c["skip_txfm_rate"], above_ctx=c["above"] + [0] * (32 - len(c["above"])), left_ctx=c["left"] + [0] * (32 - len(c["left"])))
    mbw, mbh = max_blocks(env, blk)
    dps = []
    for _, tx in plan["entries"]:
        order = visit_order(mbw, mbh, M.TXW[tx] >> 2, M.TXH[tx] >> 2)
        dps.append(dict(costs=case_costs(z, tx) if z is not None else None, tx_type_costs=c["type_costs"][str(tx)], use_txd=c["use_txd"], threshold=c["threshold"], low_txfm_rd=0,
                        adaptive=c["adaptive"], skip_tx_search=c["skip_tx_search"], mask_limit=0xFFFF,
                        masks=[c["masks"].get("%d,%d,%d" % (tx, r, col), 0xFFFF) for r, col in order], single=None))
    return env, blk, plan, dps
