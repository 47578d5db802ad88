"""tests/tx_type_model.py against tests/golden/ref_eval_tx_type.npz: search_tx_type (av1/encoder/tx_search.c:2019-2335) as the interpreted reference ran it
(tests/golden/gen_ref_eval_tx_type.py).  The model must reproduce every recorded intermediate of every case -- the block's scalars and flags, the
order of the visited types, the {rate, eob, ctx, dist, sse} of every type the loop evaluated, the rate-only `continue`s -- and the final outputs; the
fixture must cover what its generator asserted, recomputed here from the data; and the entry point must be declared, exported and bound, with the record
sizes the header states."""
import ctypes
import os
import re

import tx_type_model as M
from conftest import ROOT

Z, CASES = M.golden()
MODEL = {}


def model(c):
    if c["k"] not in MODEL:
        MODEL[c["k"]] = M.model_case(Z, c)
    return MODEL[c["k"]]


def test_model_reproduces_every_recorded_intermediate():
    assert len(CASES) >= 250
    n_types = 0
    for c in CASES:
        info, tab, res, visited = model(c)
        assert (info["block_sse"], info["block_mse_q8"], info["use_txd"], info["calc_final"]) == \
            (int(c["block_sse"]), c["block_mse_q8"], c["use_txd_flag"], c["calc_final"]), c["k"]
        assert visited == c["visit"], c["k"]
        for t, (rate, eob, ctx, dist, sse) in c["types"].items():
            e = tab[int(t)]
            assert (e["rate"], e["eob"], e["ctx"], e["dist"], e["sse"]) == (rate, eob, ctx, int(dist), int(sse)), (c["k"], t)
            n_types += 1
        for t, rate in c["rate_only"]:
            assert tab[t]["rate"] == rate and M.rdcost(c["rdmult"], rate, 0) > 0, (c["k"], t)
        assert set(c["visit"]) == {int(t) for t in c["types"]} | {t for t, _ in c["rate_only"]}, c["k"]
    assert n_types >= 1000


def test_model_reproduces_every_final_output():
    for c in CASES:
        res = model(c)[2]
        got = (res["best_tx_type"], res["best_eob"], res["txb_entropy_ctx"], res["rate"], res["dist"], res["sse"], res["skip_txfm"], res["best_rd"])
        want = (c["best_tx_type"], c["best_eob"], c["best_ctx"], c["rate"], int(c["dist"]), int(c["sse"]), c["skip_txfm"], int(c["best_rd"]))
        assert got == want, c["k"]
        assert res["final_px"] == int(bool(c["calc_final"] and c["best_eob"])), c["k"]


def test_fixture_meets_its_power_conditions():
    seen = {}

    def hit(k):
        seen[k] = seen.get(k, 0) + 1
    sizes = set()
    for c in CASES:
        w, h = M.TXW[c["tx_size"]], M.TXH[c["tx_size"]]
        sizes.add((w, h))
        info, tab, res, visited = model(c)
        repl, added = {t for t, k in c["branch"] if k == 1}, {t for t, k in c["branch"] if k == 2}
        for t, (rate, eob, ctx, dist, sse) in c["types"].items():
            hit("eob0" if eob == 0 else "txd" if c["use_txd_flag"] else "sse_diff_added" if int(t) in added else "px_replaced" if int(t) in repl else "px")
        if res["final_px"]:
            hit("final")
        wants_final = c["use_txd"] == 1 and not c["psy"] and not c["low_txfm_rd"] and c["block_mse_q8"] >= c["threshold"] and max(w, h) != 64
        if wants_final and not c["calc_final"]:
            hit("final_off_txk_allowed" if c["single"] is not None else "final_off_mask1")
        allowed = [t for t in (c["txk_map"] or range(16)) if t < 16 and (c["mask"] >> t) & 1]
        if len(c["visit"]) < len(allowed):
            hit("break_skip" if c["skip_tx_search"] and c["best_eob"] == 0 else "break_adaptive")
        for k, on in (("rate_only", c["rate_only"]), ("winner_not_dct", c["best_tx_type"] != 0), ("txk_map", c["txk_map"] is not None and len(c["visit"]) > 1),
                      ("clip_right", c["vis_cols"] < w), ("clip_bottom", c["vis_rows"] < h), ("bd%d" % c["bd"], True)):
            if on:
                hit(k)
        rds = [M.rdcost(c["rdmult"], e[0], int(e[3])) for e in c["types"].values()]
        if rds.count(min(rds)) > 1 and min(rds) == int(c["best_rd"]):
            assert c["best_tx_type"] == [t for t in c["visit"] if str(t) in c["types"] and M.rdcost(c["rdmult"], c["types"][str(t)][0], int(c["types"][str(t)][3])) == min(rds)][0]
            hit("tie")
    need = ("eob0", "txd", "px", "sse_diff_added", "px_replaced", "final", "final_off_txk_allowed", "final_off_mask1", "break_skip", "break_adaptive", "rate_only",
            "winner_not_dct", "txk_map", "tie", "clip_right", "clip_bottom", "bd8", "bd10", "bd12")
    assert all(seen.get(k, 0) >= 2 for k in need), {k: seen.get(k, 0) for k in need}
    assert sizes == {(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (16, 64), (4, 16), (16, 4), (8, 32)}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_eval_tx_type.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_eval_proj.npz"))


def test_symbol_is_declared_exported_and_bound(hip):
    full = open(os.path.join(ROOT, "include", "aomhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    lib = ctypes.CDLL(hip.capi.LIB_PATH)
    K = hip.capi
    nm = "aomhip_search_tx_type_batch"
    assert re.search(r"\bint %s\s*\(" % nm, src) and hasattr(lib, nm) and nm in K.EXPORTED and hasattr(K.Context, "search_tx_type_batch")
    for name, size in (("aomhip_tx_search_params", ctypes.sizeof(K.TxSearchParams)), ("aomhip_tx_search_block", K.tx_search_block_dtype.itemsize),
                       ("aomhip_tx_type_entry", K.tx_type_entry_dtype.itemsize), ("aomhip_tx_search_info", K.tx_search_info_dtype.itemsize),
                       ("aomhip_tx_search_result", K.tx_search_result_dtype.itemsize)):
        m = re.search(r"\}\s*%s;\s*/\* (\d+) bytes" % name, full)
        assert m and int(m.group(1)) == size, (name, size)
    assert (ctypes.sizeof(K.TxSearchParams), K.tx_search_block_dtype.itemsize, K.tx_type_entry_dtype.itemsize, K.tx_search_info_dtype.itemsize,
            K.tx_search_result_dtype.itemsize) == (112, 32, 32, 16, 40)
    assert K.TX_SEARCH_TRACE_BYTES == 17 and re.search(r"#define AOMHIP_TX_SEARCH_TRACE_BYTES 17\b", full)
