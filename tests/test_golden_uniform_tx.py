"""The uniform transform-size search against the interpreted reference (tests/golden/ref_eval_uniform_tx.npz: choose_tx_size_type_from_rd,
choose_largest_tx_size, av1_uniform_txfm_yrd, av1_txfm_rd_in_plane, block_rd_txfm, av1_foreach_transformed_block_in_plane, get_txb_ctx,
av1_set_txb_context and av1_merge_rd_stats as they are written, with hooks recording every depth and every visited transform block), no GPU:
the coverage the generator asserted is recomputed from the stored data, tests/uniform_tx_model.py is held to every recorded value, and the
depth-plan helper of the C ABI (host only) is held to the recorded plans."""
import numpy as np
import pytest

import tx_type_model as M
import uniform_tx_model as U

Z, CASES = U.golden()
INT_MAX = (1 << 31) - 1


def test_coverage_recomputed_from_the_stored_data():
    n = {}

    def hit(k, c=1):
        n[k] = n.get(k, 0) + c
    for c in CASES:
        bw, bh = U.BSW[c["bsize"]], U.BSH[c["bsize"]]
        ds = c["depths"]
        if c["rate"] != INT_MAX and not c["use_largest"]:
            hit("winner_depth%d" % [d["depth"] for d in ds if d["tx_size"] == c["rd"][3]][0])
        for d in ds:
            hit("incomplete_exit", int(bool(d.get("incomplete"))))
            hit("out_of_budget_on_the_last_valid", int(bool(d.get("exit_early")) and not d.get("incomplete")))
            hit("entry_refused", int(not d["entered"]))
            hit("forced_skip", d["forced"])
            hit("skip_stays", int(bool(d["entered"] and d.get("skip") and not d.get("incomplete") and not d["forced"])))
            right, bottom = c["vis_w"] < bw, c["vis_h"] < bh
            if any(t["col"] * 4 + M.TXW[d["tx_size"]] > c["vis_w"] or t["row"] * 4 + M.TXH[d["tx_size"]] > c["vis_h"] for t in d["txbs"]):
                hit("cross_%s" % ("both" if right and bottom else ("right" if right else "bottom")))
            for k, t in enumerate(d["txbs"]):
                hit("skip_ctx_0" if t["skip_ctx"] == 0 else "skip_ctx_1_6")
                assert t["skip_ctx"] <= 6   # (get_txb_ctx gives plane 0 nothing above 6: 7 .. 12 are the chroma planes')
                hit("dc_ctx_%d" % t["dc_ctx"])
                hit("contexts_from_an_earlier_txb", int(c["ctx_kind"] == 0 and k > 0 and (t["skip_ctx"] > 1 or t["dc_ctx"] > 0)))
        hit("lowvar_taken", int(c["lowvar"] == 1)); hit("lowvar_not_taken_rd_order", int(c["lowvar"] == 0))
        hit("lowvar_not_taken_variance", int(not c["use_largest"] and c["tx_select"] and c["init_depth"] == 0 and c["source_variance"] >= 256 and len(ds) == 3))
        hit("tx_select_0", int(not c["tx_select"] and not c["use_largest"])); hit("use_largest", c["use_largest"])
        if not c["enable_tx64"] and max(bw, bh) >= 64 and not c["use_largest"]:
            hit("tx64_off_demotion" if c["init_depth"] == 2 else "tx64_off_continue")
        hit("rect_off", int(not c["enable_rect_tx"]))
        hit("bd%d" % c["bd"])
    need = ("winner_depth0", "winner_depth1", "winner_depth2", "incomplete_exit", "out_of_budget_on_the_last_valid", "entry_refused", "lowvar_taken", "lowvar_not_taken_rd_order",
            "lowvar_not_taken_variance", "forced_skip", "skip_stays", "cross_right", "cross_bottom", "cross_both", "skip_ctx_0", "skip_ctx_1_6", "dc_ctx_0", "dc_ctx_1", "dc_ctx_2",
            "contexts_from_an_earlier_txb", "tx_select_0", "use_largest", "tx64_off_continue", "tx64_off_demotion", "rect_off", "bd8", "bd10", "bd12")
    assert not {k: n.get(k, 0) for k in need if n.get(k, 0) < 2}
    assert len({c["bsize"] for c in CASES if c["bd"] == 12}) >= 3
    sizes = {(U.BSW[c["bsize"]], U.BSH[c["bsize"]]) for c in CASES}
    assert {(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (4, 16), (8, 32), (64, 16)} <= sizes and sizes & {(128, 64), (128, 128)}


@pytest.mark.parametrize("c", CASES, ids=lambda c: "case%d" % c["k"])
def test_model_against_every_recorded_value(oracle, c):
    env, blk, plan, dps = U.case_inputs(Z, c)
    want = U.pick_uniform(env, blk, plan, dps)
    # the plan the reference walked is the model's, up to a low-variance break
    walked = [(d["depth"], d["tx_size"]) for d in c["depths"]]
    refused_largest = bool(c["use_largest"]) and not walked   # (choose_largest_tx_size refused at av1_txfm_rd_in_plane's entry: the record has no depth)
    assert walked == plan["entries"][:len(walked)] and (len(walked) == len(plan["entries"]) or c["lowvar"] == 1 or refused_largest)
    if refused_largest:
        assert want["depths"][0]["entry_refused"] and c["rate"] == INT_MAX
    for k, d in enumerate(c["depths"]):
        o = want["depths"][k]
        assert o is not None
        assert (int(o["entry_refused"]), int(o["incomplete"])) == (int(not d["entered"]), int(d.get("incomplete", 0))), (c["k"], k)
        if d["entered"]:
            assert int(o["last_exit"] or o["incomplete"]) == d["exit_early"] and int(o.get("forced_skip", False)) == d["forced"], (c["k"], k)
        assert len(o["txbs"]) == len(d["txbs"]), (c["k"], k)
        for t, r in zip(o["txbs"], d["txbs"]):
            got = (t["row"], t["col"], t["skip_ctx"], t["dc_ctx"], t["ref_best_rd"], t["tx_type"], t["eob"], t["ctx"], t["rate"], t["dist"], t["sse"], t["n_visited"])
            assert got == (r["row"], r["col"], r["skip_ctx"], r["dc_ctx"], int(r["ref_best_rd"]), r["tx_type"], r["eob"], r["ctx"], r["rate"], int(r["dist"]), int(r["sse"]),
                           len(r["visit"])), (c["k"], k, r["row"], r["col"])
    if not c["use_largest"]:
        assert want["depth_rd"] == [int(v) for v in c["rd"][:3]], c["k"]
    assert (want["rate"], want["dist"], want["sse"], want["skip_txfm"]) == (c["rate"], int(c["dist"]), int(c["sse"]), c["skip_txfm"]), c["k"]
    if c["rate"] != INT_MAX:
        tx = want["tx_size"]
        assert tx == (c["depths"][0]["tx_size"] if c["use_largest"] else c["rd"][3]) == c["mbmi_tx_size"]
        type_map, blk_skip = U.maps_from_records(env, blk, tx, want["txbs"])   # the host loop of the header's comment
        n4w = env["bw"] >> 2
        for (row, col), t in type_map.items():
            if row * n4w + col < len(c["final_type_map"]) and col < n4w:
                assert c["final_type_map"][row * n4w + col] == t, (c["k"], row, col)
        for idx, v in blk_skip.items():
            assert c["blk_skip"][idx] == v, (c["k"], idx)
    else:
        assert want["tx_size"] == (c["mbmi_tx_size"] if c["use_largest"] else 255)   # (choose_largest_tx_size sets mbmi->tx_size whatever follows)


def test_the_two_cases_only_a_second_run_of_the_model_shows(oracle):
    """a winning type that differs from the winner under contexts (0, 0), and the adaptive break taken because ref_best_rd had shrunk by current_rd: each at
    least twice in the fixture, found by running the model both ways"""
    other_winner = shrunk = 0
    for c in CASES:
        env, blk, plan, dps = U.case_inputs(Z, c)

        def search(env_, blk_, tx, dp, k, row, col, sc, dc, ref):
            nonlocal other_winner, shrunk
            r = U.search_txb(env_, blk_, tx, dp, k, row, col, sc, dc, ref)
            other_winner += (sc, dc) != (0, 0) and U.search_txb(env_, blk_, tx, dp, k, row, col, 0, 0, ref)["best_tx_type"] != r["best_tx_type"]
            shrunk += bool(dp["adaptive"]) and ref < blk_["ref_best_rd"] and \
                U.search_txb(env_, blk_, tx, dp, k, row, col, sc, dc, blk_["ref_best_rd"])["n_visited"] > r["n_visited"]
            return r
        U.pick_uniform(env, blk, plan, dps, search)
    assert other_winner >= 2 and shrunk >= 2, (other_winner, shrunk)


def test_depth_plan_helper_against_the_recorded_plans(hip):
    K = hip.capi
    for c in CASES:
        p = K.uniform_tx_depth_plan(c["bsize"], c["tx_select"], c["mode_tx_size"], c["init_depth"], c["enable_tx64"], c["enable_rect_tx"], c["use_largest"])
        walked = [(d["depth"], d["tx_size"]) for d in c["depths"]]
        assert p.entries()[:len(walked)] == walked and (len(walked) == p.n or c["lowvar"] == 1 or (c["use_largest"] and not walked)), c["k"]
        if c["use_largest"]:
            assert p.entries() == [(0, c["mbmi_tx_size"])], c["k"]
        assert bool(p.use_largest) == bool(c["use_largest"])
        if c["lowvar"] is not None:
            assert p.init_depth == 0
