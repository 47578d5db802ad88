"""The host side of the uniform transform-size search, no GPU: aomhip_uniform_tx_depth_plan (aom-av1-psy_amd/host/uniform_tx_plan.c, which derives every
size step from the transform's dimensions) against the loop of choose_tx_size_type_from_rd / choose_largest_tx_size restated on AV1's own size tables,
for every argument combination; the two legality tests the device calls refuse with; the model's visiting order against the nested loops of
av1_foreach_transformed_block_in_plane; and the identity the device's walk rests on -- a table entry's rate under any TXB_CTX is its rate under (0, 0)
plus two cost-table differences -- on the plain-integer table of tests/tx_type_model.py."""
import ctypes as C

import numpy as np
import pytest

import tx_type_model as M
import uniform_tx_model as U

# AV1's tables in TX_SIZE / BLOCK_SIZE order (the specification's Max_Tx_Size_Rect and Split_Tx_Size; the three demotions of choose_largest_tx_size)
TX_4X4, TX_8X8, TX_16X16, TX_32X32, TX_64X64, TX_4X8, TX_8X4, TX_8X16, TX_16X8, TX_16X32, TX_32X16, TX_32X64, TX_64X32, TX_4X16, TX_16X4, TX_8X32, TX_32X8, TX_16X64, \
    TX_64X16 = range(19)
MAX_RECT = [TX_4X4, TX_4X8, TX_8X4, TX_8X8, TX_8X16, TX_16X8, TX_16X16, TX_16X32, TX_32X16, TX_32X32, TX_32X64, TX_64X32, TX_64X64, TX_64X64, TX_64X64, TX_64X64,
            TX_4X16, TX_16X4, TX_8X32, TX_32X8, TX_16X64, TX_64X16]
SUB_TX = [TX_4X4, TX_4X4, TX_8X8, TX_16X16, TX_32X32, TX_4X4, TX_4X4, TX_8X8, TX_8X8, TX_16X16, TX_16X16, TX_32X32, TX_32X32, TX_4X8, TX_8X4, TX_8X16, TX_16X8,
          TX_16X32, TX_32X16]
MAX_32 = [TX_4X4, TX_8X8, TX_16X16, TX_32X32, TX_32X32, TX_4X8, TX_8X4, TX_8X16, TX_16X8, TX_16X32, TX_32X16, TX_32X32, TX_32X32, TX_4X16, TX_16X4, TX_8X32, TX_32X8,
          TX_16X32, TX_32X16]
MAX_SQUARE = [TX_4X4, TX_8X8, TX_16X16, TX_32X32, TX_64X64, TX_4X4, TX_4X4, TX_8X8, TX_8X8, TX_16X16, TX_16X16, TX_32X32, TX_32X32, TX_4X4, TX_4X4, TX_8X8, TX_8X8,
              TX_16X16, TX_16X16]
MAX_32_SQUARE = [TX_4X4, TX_8X8, TX_16X16, TX_32X32, TX_32X32, TX_4X4, TX_4X4, TX_8X8, TX_8X8, TX_16X16, TX_16X16, TX_32X32, TX_32X32, TX_4X4, TX_4X4, TX_8X8, TX_8X8,
                 TX_16X16, TX_16X16]


def legal_sizes(bsize):
    tx = MAX_RECT[bsize]
    return {tx, SUB_TX[tx], SUB_TX[SUB_TX[tx]]}


def restated_plan(bsize, tx_select, mode_tx, init_depth, tx64, rect, largest):
    """tx_search.c:2659-2741 and :2850-2917 on the tables above -> (init_depth, use_largest, [(depth, tx_size)])"""
    sqr_up_64 = lambda tx: max(M.TXW[tx], M.TXH[tx]) == 64
    if largest:
        tx = mode_tx
        if not tx64 and rect:
            tx = MAX_32[tx]
        elif tx64 and not rect:
            tx = MAX_SQUARE[tx]
        elif not tx64 and not rect:
            tx = MAX_32_SQUARE[tx]
        return 0, 1, [(0, tx)]
    if tx_select:
        start = MAX_RECT[bsize]
        if init_depth == 2 and not tx64 and sqr_up_64(start):
            start = SUB_TX[start]
    else:
        start, init_depth = mode_tx, 2
    entries, tx, depth = [], start, init_depth
    while depth <= 2:
        if not ((not tx64 and sqr_up_64(tx)) or (not rect and M.TXW[tx] != M.TXH[tx])):
            entries.append((depth, tx))
            if tx == TX_4X4:
                break
        depth, tx = depth + 1, SUB_TX[tx]
    return init_depth, 0, entries


@pytest.mark.parametrize("bsize", range(22))
def test_depth_plan_helper_against_the_loop_on_the_size_tables(hip, bsize):
    K = hip.capi
    n = 0
    for tx_select in (0, 1):
        for mode_tx in range(19):
            for init_depth in (0, 1, 2):
                for tx64 in (0, 1):
                    for rect in (0, 1):
                        for largest in (0, 1):
                            args = (bsize, tx_select, mode_tx, init_depth, tx64, rect, largest)
                            if (largest or not tx_select) and mode_tx not in legal_sizes(bsize):
                                with pytest.raises(ValueError):
                                    K.uniform_tx_depth_plan(*args)
                                continue
                            p = K.uniform_tx_depth_plan(*args)
                            want = restated_plan(*args)
                            assert (p.init_depth, p.use_largest, p.entries()) == want, args
                            m = U.depth_plan(*args)
                            assert (m["init_depth"], m["use_largest"], m["entries"]) == want, args
                            assert K.lib.aomhip_uniform_tx_plan_legal(bsize, C.byref(p)) == 1
                            assert all(K.lib.aomhip_uniform_tx_size_legal(bsize, tx) == 1 for _, tx in p.entries())
                            n += 1
    assert n >= 2 * 3 * 4 + 4
    for bad in ((bsize, 1, 0, 3, 1, 1, 0), (bsize, 1, 0, -1, 1, 1, 0), (22, 1, 0, 0, 1, 1, 0), (-1, 1, 0, 0, 1, 1, 0)):
        with pytest.raises(ValueError):
            K.uniform_tx_depth_plan(*bad)


def test_legality_of_sizes_and_plans(hip):
    K = hip.capi
    for bsize in range(22):
        for tx in range(-1, 20):
            assert K.lib.aomhip_uniform_tx_size_legal(bsize, tx) == int(tx in legal_sizes(bsize)), (bsize, tx)
    assert K.lib.aomhip_uniform_tx_size_legal(22, 0) == 0 and K.lib.aomhip_uniform_tx_size_legal(-1, 0) == 0
    good = K.uniform_tx_depth_plan(12, 1, 0, 0, 1, 1, 0)   # 64x64: 64x64, 32x32, 16x16
    assert good.entries() == [(0, TX_64X64), (1, TX_32X32), (2, TX_16X16)]

    def changed(**kw):
        p = K.UniformTxPlan.from_buffer_copy(good)
        for name, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, name)[v[0]] = v[1]
            else:
                setattr(p, name, v)
        return K.lib.aomhip_uniform_tx_plan_legal(12, C.byref(p))
    assert changed() == 1 and changed(n=2) == 0 and changed(n=4) == 0 and changed(n=-1) == 0 and changed(tx_size=(1, TX_16X16)) == 0 and changed(depth=(2, 1)) == 0
    assert changed(init_depth=1) == 0 and changed(use_largest=1) == 0 and changed(tx_size=(0, TX_64X32)) == 0
    assert K.lib.aomhip_uniform_tx_plan_legal(9, C.byref(good)) == 0 and K.lib.aomhip_uniform_tx_plan_legal(12, None) == 0
    empty = K.uniform_tx_depth_plan(12, 0, TX_64X64, 0, 0, 1, 0)   # !tx_select at a 64-point size without enable_tx64: nothing is tried
    assert empty.n == 0 and K.lib.aomhip_uniform_tx_plan_legal(12, C.byref(empty)) == 1 and K.lib.aomhip_uniform_tx_plan_legal(6, C.byref(empty)) == 0


@pytest.mark.parametrize("bw,bh,tx,mbw,mbh", [(128, 128, TX_64X64, 32, 32), (128, 128, TX_32X32, 30, 17), (128, 64, TX_16X16, 19, 16), (64, 128, TX_64X64, 3, 31),
                                              (64, 16, TX_32X16, 9, 4), (16, 64, TX_16X32, 4, 16), (8, 8, TX_4X4, 2, 1), (64, 64, TX_16X16, 16, 5)])
def test_visiting_order_is_the_reference_loops(bw, bh, tx, mbw, mbh):
    """encodemb.c:551-591 as nested loops with the running `unit` bounds, against the model's order and its count against the slot count"""
    txw4, txh4 = M.TXW[tx] >> 2, M.TXH[tx] >> 2
    want = []
    mu_w, mu_h = min(16, mbw), min(16, mbh)
    r = 0
    while r < mbh:
        unit_height = min(mu_h + r, mbh)
        c = 0
        while c < mbw:
            unit_width = min(mu_w + c, mbw)
            blk_row = r
            while blk_row < unit_height:
                blk_col = c
                while blk_col < unit_width:
                    want.append((blk_row, blk_col))
                    blk_col += txw4
                blk_row += txh4
            c += mu_w
        r += mu_h
    assert U.visit_order(mbw, mbh, txw4, txh4) == want
    assert len(want) <= (bw // M.TXW[tx]) * (bh // M.TXH[tx]) <= 64
    if mbw > 16 and mbh > 16:
        assert want.index((0, 16)) < want.index((16, 0))   # 64x64 units in raster order: the unit to the right comes before the unit below
        if txh4 < 16:
            assert want.index((txh4, 0)) < want.index((0, 16))   # ... and after the whole first unit


@pytest.mark.parametrize("tx_size,bd", [(TX_4X4, 8), (TX_8X8, 10), (TX_16X8, 8), (TX_16X16, 12), (TX_32X32, 8)])
def test_rate_under_any_context_is_the_rate_under_zero_contexts_plus_two_table_differences(oracle, tx_size, bd):
    """what the device's walk does to a table computed under TXB_CTX (0, 0), stated on the model's table: exact for every type, every txb_skip_ctx and
    dc_sign_ctx, zero and non-zero DC levels, eob 0 included; everything but the rate does not depend on the contexts at all"""
    rng = np.random.default_rng(tx_size * 5 + bd)
    w, h = M.TXW[tx_size], M.TXH[tx_size]
    mx = (1 << bd) - 1
    costs = rng.integers(10, 4000, 966).astype(np.int32)
    type_costs = [int(v) for v in rng.integers(0, 1200, 16)]
    q = oracle.build_quantizer_y(bd, 120)
    mask = sum(1 << t for t in range(16) if M.tx_type_exists(tx_size, t))
    K_DC_SIGN = 392   # dc_sign_cost[3][2] in the 966-int table
    seen = set()
    for amp in (0, 3, 40):
        pred = rng.integers(mx // 4, 3 * mx // 4, (h, w))
        src = np.clip(pred + rng.integers(-amp, amp + 1, (h, w)) * (1 << (bd - 8)), 0, mx)
        info = M.block_scalars(src, pred, tx_size, bd, w, h, mask, 0, 0, 0, 0)
        base = M.table(src, pred, tx_size, bd, q, costs, type_costs, 0, 0, w, h, mask, info)
        for skip_ctx in (0, 1, 4, 6):
            for dc_ctx in (0, 1, 2):
                tab = M.table(src, pred, tx_size, bd, q, costs, type_costs, skip_ctx, dc_ctx, w, h, mask, info)
                for t in range(16):
                    if tab[t] is None:
                        continue
                    e0, e = base[t], tab[t]
                    z = int(e0["eob"] == 0)
                    rate = e0["rate"] + int(costs[M.K_SKIP + skip_ctx * 2 + z]) - int(costs[M.K_SKIP + z])
                    s = e0["ctx"] >> 3
                    if e0["eob"] and s:
                        rate += int(costs[K_DC_SIGN + dc_ctx * 2 + (s == 1)]) - int(costs[K_DC_SIGN + (s == 1)])
                    assert e["rate"] == rate, (amp, skip_ctx, dc_ctx, t)
                    assert {k: v for k, v in e.items() if k != "rate"} == {k: v for k, v in e0.items() if k != "rate"}
                    seen.add((z, s))
    assert {(1, 0), (0, 1), (0, 2)} <= seen
