#!/usr/bin/env python3
"""Golden vectors of the decision layer of av1_pick_filter_level from the interpreted reference (build container only; see ref_c_eval.py):

  ref_eval_lpf_pick.npz   search_filter_level and the search branch of av1_pick_filter_level (av1/encoder/picklpf.c:88-193, 195-328), and
                          av1_get_max_filter_level (:40-47), interpreted from the reference's own text where it lies, on synthetic tables.

The static functions are not exported by the compiled reference, and the oracle takes no new shim: the interpreter is the pin here.

What is bound instead of interpreted.  try_filter_frame (:49-86) is a lookup in the case's synthetic tables, keyed by (plane, dir, level, the other
luma direction's level read from the cm->lf view as :58-60 read it); the binding stores the trial's levels into cm->lf as :63-70 do, because later
trials read them back, and records every call.  yv12_copy_plane and aom_realloc_frame_buffer (plane copies and allocation) do nothing;
is_stat_consumption_stage_twopass, av1_num_planes and frame_is_intra_only return the case's values; av1_cyclic_refresh_disable_lf_cdef is bound
and never reached.  AV1_COMP, AV1_PRIMARY, AV1_COMMON, SequenceHeader, FeatureFlags, the speed-feature structs, AV1EncoderConfig and struct
loopfilter are views of the members these functions read (cpi->sf.lpf_sf.use_coarse_filter_level_search, cpi->ppi->twopass.section_intra_rating,
cm->features.tx_mode, cpi->ppi->filter_level[] / _u / _v, cm->lf, the oxcf members of the early returns, which every case leaves at "filter").

Only data goes into the .npz: per case the inputs, every table the reference asked for (values up to 2^40, so that a 32-bit bias fails), the four
chosen levels, and per search_filter_level call its plane, dir, start, fixed level, result and the levels of its try_filter_frame calls in order.

The generator asserts (through tests/lpf_pick_model.py's event log, after the model has reproduced the case) that the reference alone reaches: a
downward move accepted through the bias that is no improvement; an upward move; a level requested twice and tried once; a walk that ends on 0 and
one that reaches max_level through a clamped partial step; max_level 47; the coarse stop; a rating below 20 and one of 20 or above; ONLY_4X4;
starts below 16 and at 60 or above; NON_DUAL; monochrome; a dir 0 search whose table depends on the dir 2 result; all-zero starts."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
import ref_c_eval as R  # noqa: E402
from gen_ref_eval_golden import REF, evaluator, save  # noqa: E402
from gen_ref_eval_composites import view  # noqa: E402
import lpf_pick_model as M  # noqa: E402

I32, U8 = R.I32, R.U8


def load_enum(ev, path, name):
    m = re.search(r"(?:typedef )?enum(?: \w+)? \{[^}]*\} (?:UENUM1BYTE\()?%s\)?;" % name, open(REF + path).read(), re.S)
    assert m, name
    ev.load_text(m.group(0), path + ":" + name)


def const(ev, name):
    return int(ev.interp.ev(R.Parser(ev.pp.expand(R.tokenize(name)), ev.typedefs, ev.globs, ev.interp, ev.structs).expr())[0])


def make_evaluator(state):
    ev = evaluator([])
    load_enum(ev, "av1/encoder/speed_features.h", "LPF_PICK_METHOD")
    load_enum(ev, "av1/encoder/encoder.h", "AQ_MODE")
    load_enum(ev, "av1/encoder/encoder.h", "LOOPFILTER_CONTROL")
    load_enum(ev, "aom/aomcx.h", "aom_tune_content")
    m = re.search(r"#define MAX_LOOP_FILTER (\d+)", open(REF + "av1/common/av1_loopfilter.h").read())
    ev.define("MAX_LOOP_FILTER", m.group(1))
    ev.define("assert", "((void)0)", ["x"])      # (one assert of the closed-form branch concatenates two string literals, outside the subset)
    ev.load(REF + "av1/encoder/picklpf.c")
    it = ev.interp
    for nm in ("search_filter_level", "av1_pick_filter_level", "try_filter_frame", "av1_get_max_filter_level"):
        assert nm in it.funcs, "%s was not loaded from the reference" % nm
    assert [const(ev, n) for n in ("LPF_PICK_FROM_FULL_IMAGE", "LPF_PICK_FROM_FULL_IMAGE_NON_DUAL", "LPF_PICK_FROM_SUBIMAGE")] == [M.FULL_IMAGE, M.NON_DUAL, M.SUBIMAGE]
    state["ONLY_4X4"], state["TX_MODE_SELECT"] = const(ev, "ONLY_4X4"), const(ev, "TX_MODE_SELECT")
    state["LOOPFILTER_ALL"] = const(ev, "LOOPFILTER_ALL")

    yv12 = view(ev, "YV12_BUFFER_CONFIG", [("unused", I32)])
    seq = view(ev, "SequenceHeader", [("subsampling_x", I32), ("subsampling_y", I32), ("use_highbitdepth", U8), ("bit_depth", I32)])
    feat = view(ev, "FeatureFlags", [("tx_mode", I32), ("byte_alignment", I32)], opaque=False)
    lf = view(ev, "loopfilter", [("filter_level", ("arr", I32, 2)), ("filter_level_u", I32), ("filter_level_v", I32), ("sharpness_level", I32)], opaque=False)
    rcb = view(ev, "RefCntBuffer", [("buf", yv12)])
    cm = view(ev, "AV1_COMMON", [("seq_params", ("ptr", seq)), ("lf", lf), ("features", feat), ("cur_frame", ("ptr", rcb)), ("width", I32), ("height", I32)])
    tp = view(ev, "TWO_PASS", [("section_intra_rating", I32)], opaque=False)
    rtc = view(ev, "RTC_REF", [("non_reference_frame", I32)], opaque=False)
    ppi = view(ev, "AV1_PRIMARY", [("twopass", tp), ("filter_level", ("arr", I32, 2)), ("filter_level_u", I32), ("filter_level_v", I32), ("rtc_ref", rtc)])
    lpf_sf = view(ev, "LOOP_FILTER_SPEED_FEATURES", [("use_coarse_filter_level_search", I32)], opaque=False)
    rt_sf = view(ev, "REAL_TIME_SPEED_FEATURES", [("skip_lf_screen", I32)], opaque=False)
    sf = view(ev, "SPEED_FEATURES", [("lpf_sf", lpf_sf), ("rt_sf", rt_sf)], opaque=False)
    tune = view(ev, "TuneCfg", [("content", I32)], opaque=False)
    qcfg = view(ev, "QuantizationCfg", [("aq_mode", I32)], opaque=False)
    algo = view(ev, "AlgoCfg", [("loopfilter_control", I32)], opaque=False)
    oxcf = view(ev, "AV1EncoderConfig", [("tune_cfg", tune), ("q_cfg", qcfg), ("algo_cfg", algo), ("border_in_pixels", I32)])
    view(ev, "AV1_COMP", [("common", cm), ("ppi", ("ptr", ppi)), ("sf", sf), ("oxcf", oxcf), ("last_frame_uf", yv12)])

    def nothing(_, a):
        return None, R.VOID

    def hook_try(_, a):
        """try_filter_frame(sd, cpi, filt_level, partial_frame, plane, dir)"""
        cpi, level, partial, plane, d = a[1][0], int(a[2][0]), int(a[3][0]), int(a[4][0]), int(a[5][0])
        assert partial == int(state["method"] == M.SUBIMAGE)
        fl = [level, level]
        if plane == 0 and d == 0:
            fl[1] = int(ev.get(cpi, "common.lf.filter_level[1]"))
        if plane == 0 and d == 1:
            fl[0] = int(ev.get(cpi, "common.lf.filter_level[0]"))
        if plane == 0:
            ev.set(cpi, "common.lf.filter_level[0]", fl[0]); ev.set(cpi, "common.lf.filter_level[1]", fl[1])
        else:
            ev.set(cpi, "common.lf.filter_level_u" if plane == 1 else "common.lf.filter_level_v", fl[0])
        fixed = fl[1] if (plane, d) == (0, 0) else (fl[0] if (plane, d) == (0, 1) else -1)
        state["calls"].append((plane, d, fixed, level))
        return int(state["table"](plane, d, fixed)[level]), R.I64
    it.pycalls.update(try_filter_frame=hook_try, yv12_copy_plane=nothing, aom_realloc_frame_buffer=lambda _, a: (0, I32),
                      is_stat_consumption_stage_twopass=lambda _, a: (state["twopass"], I32), av1_num_planes=lambda _, a: (1 if state["mono"] else 3, I32),
                      frame_is_intra_only=lambda _, a: (0, I32), av1_cyclic_refresh_disable_lf_cdef=lambda _, a: (0, I32))
    for nm in ("try_filter_frame", "yv12_copy_plane", "aom_realloc_frame_buffer", "is_stat_consumption_stage_twopass", "av1_num_planes",
               "frame_is_intra_only", "av1_cyclic_refresh_disable_lf_cdef"):
        it.funcs.pop(nm, None)
    return ev


def make_table(seed, shape, plane, d, fixed, n=64):
    """a synthetic ss_err[]: non-negative Python integers up to 2^40"""
    rng = np.random.default_rng([seed, plane, d, fixed + 1])
    lv = np.arange(n, dtype=np.int64)
    big = int(rng.integers(1 << 36, 1 << 40))
    kind = shape["kind"]
    if kind == "v":            # a minimum whose place depends on the search and on the fixed level
        at = (shape["at"] + 7 * plane + 11 * d + 3 * max(fixed, 0)) % n
        t = big + np.abs(lv - at) * (big >> shape.get("slope", 7)) + rng.integers(0, big >> 12, n)
    elif kind == "down":       # ever better towards max_level
        t = big - lv * (big >> 7) + rng.integers(0, big >> 14, n)
    elif kind == "up":         # ever worse: the walk goes to 0
        t = big + lv * (big >> 7) + rng.integers(0, big >> 14, n)
    elif kind == "flat":       # differences far below the bias: lower levels are taken without an improvement
        t = big + rng.integers(0, 64, n) + lv
    else:                      # noisy
        t = big + rng.integers(-(big >> 6), big >> 6, n)
    return [int(v) for v in t]


def run_case(ev, state, cs):
    tables = {}

    def table(plane, d, fixed):
        key = (plane, d, fixed)
        if key not in tables:
            tables[key] = make_table(cs["seed"], cs["shape"], plane, d, fixed)
        return tables[key]
    state.update(method=cs["method"], mono=cs["mono"], twopass=cs["twopass"], table=table, calls=[])
    cpi, ppi, seq, cur = ev.new("AV1_COMP"), ev.new("AV1_PRIMARY"), ev.new("SequenceHeader"), ev.new("RefCntBuffer")
    ev.set(cpi, "ppi", ppi); ev.set(cpi, "common.seq_params", seq); ev.set(cpi, "common.cur_frame", cur)
    ev.set(ppi, "twopass.section_intra_rating", cs["rating"])
    for i in range(2):
        ev.set(ppi, "filter_level[%d]" % i, cs["last"][i])
    ev.set(ppi, "filter_level_u", cs["last"][2]); ev.set(ppi, "filter_level_v", cs["last"][3])
    ev.set(cpi, "sf.lpf_sf.use_coarse_filter_level_search", cs["coarse"])
    ev.set(cpi, "common.features.tx_mode", state["ONLY_4X4"] if cs["only_4x4"] else state["TX_MODE_SELECT"])
    ev.set(cpi, "oxcf.algo_cfg.loopfilter_control", state["LOOPFILTER_ALL"])
    ev.set(cpi, "common.lf.sharpness_level", 5)
    for nm in ("filter_level[0]", "filter_level[1]", "filter_level_u", "filter_level_v"):
        ev.set(cpi, "common.lf." + nm, 0)
    max_level = int(ev.call("av1_get_max_filter_level", cpi))
    ev.call("av1_pick_filter_level", None, cpi, cs["method"])
    assert int(ev.get(cpi, "common.lf.sharpness_level")) == 0
    levels = [int(ev.get(cpi, "common.lf." + nm)) for nm in ("filter_level[0]", "filter_level[1]", "filter_level_u", "filter_level_v")]
    # split the recorded calls into the search_filter_level calls they belong to: (plane, dir) changes in the order of M.SEARCHES
    searches = []
    for plane, d, fixed, level in state["calls"]:
        if not searches or (searches[-1]["plane"], searches[-1]["dir"]) != (plane, d):
            searches.append(dict(idx=M.SEARCHES.index((plane, d)), plane=plane, dir=d, fixed=fixed, calls=[]))
        assert searches[-1]["fixed"] == fixed           # the other direction's level does not move during a search
        assert level not in searches[-1]["calls"]       # the reference tries a level once
        searches[-1]["calls"].append(level)
    return max_level, levels, searches, tables


CASES = [
    # name, method, mono, last, coarse, twopass, rating, only_4x4, shape, seed
    ("v_mid", M.FULL_IMAGE, 0, [20, 28, 10, 40], 0, 0, 0, 0, dict(kind="v", at=33), 1),
    ("v_mid_b", M.FULL_IMAGE, 0, [20, 28, 10, 40], 0, 0, 0, 0, dict(kind="v", at=9), 1),          # the same family, another dir 2 result
    ("v_low_start", M.FULL_IMAGE, 0, [3, 9, 15, 0], 0, 0, 0, 0, dict(kind="v", at=21), 2),
    ("v_high_start", M.FULL_IMAGE, 0, [63, 60, 62, 61], 0, 0, 0, 0, dict(kind="v", at=40), 3),
    ("zeros", M.FULL_IMAGE, 0, [0, 0, 0, 0], 0, 0, 0, 0, dict(kind="v", at=17), 4),
    ("down_to_max", M.FULL_IMAGE, 0, [30, 30, 30, 30], 0, 0, 0, 0, dict(kind="down"), 5),
    ("down_to_max_47", M.FULL_IMAGE, 0, [30, 41, 22, 47], 0, 1, 12, 0, dict(kind="down"), 6),
    ("up_to_zero", M.FULL_IMAGE, 0, [30, 22, 13, 50], 0, 0, 0, 0, dict(kind="up"), 7),
    ("flat", M.FULL_IMAGE, 0, [25, 35, 45, 55], 0, 0, 0, 0, dict(kind="flat"), 8),
    ("flat_4x4", M.FULL_IMAGE, 0, [25, 35, 45, 55], 0, 0, 0, 1, dict(kind="flat"), 9),
    ("noisy", M.FULL_IMAGE, 0, [31, 17, 48, 5], 0, 0, 0, 0, dict(kind="noisy"), 10),
    ("noisy_4x4", M.FULL_IMAGE, 0, [31, 17, 48, 5], 0, 0, 0, 1, dict(kind="noisy"), 10),
    ("coarse", M.FULL_IMAGE, 0, [20, 28, 10, 40], 1, 0, 0, 0, dict(kind="v", at=33), 11),
    ("coarse_noisy", M.FULL_IMAGE, 0, [44, 12, 33, 60], 1, 0, 0, 0, dict(kind="noisy"), 12),
    ("rating_5", M.FULL_IMAGE, 0, [36, 30, 20, 28], 0, 1, 5, 0, dict(kind="noisy"), 13),
    ("rating_0", M.FULL_IMAGE, 0, [36, 30, 20, 28], 0, 1, 0, 0, dict(kind="noisy"), 13),
    ("rating_8", M.FULL_IMAGE, 0, [50, 63, 20, 28], 0, 1, 8, 0, dict(kind="v", at=58, slope=9), 14),
    ("rating_15_47", M.FULL_IMAGE, 0, [50, 63, 20, 60], 0, 1, 15, 0, dict(kind="v", at=44, slope=9), 15),
    ("rating_20_47", M.FULL_IMAGE, 0, [36, 30, 20, 28], 0, 1, 20, 0, dict(kind="noisy"), 13),
    ("rating_35_47", M.FULL_IMAGE, 0, [12, 47, 48, 2], 0, 1, 35, 1, dict(kind="flat"), 16),
    ("rating_ignored", M.FULL_IMAGE, 0, [36, 30, 20, 28], 0, 0, 5, 0, dict(kind="noisy"), 13),      # not the consumption stage: the rating is not read
    ("non_dual", M.NON_DUAL, 0, [20, 28, 10, 40], 0, 0, 0, 0, dict(kind="v", at=33), 1),
    ("non_dual_noisy", M.NON_DUAL, 0, [8, 61, 33, 33], 0, 0, 0, 0, dict(kind="noisy"), 17),
    ("subimage", M.SUBIMAGE, 0, [20, 28, 10, 40], 0, 0, 0, 0, dict(kind="v", at=27), 18),
    ("subimage_coarse", M.SUBIMAGE, 0, [40, 41, 42, 43], 1, 1, 3, 0, dict(kind="flat"), 19),
    ("mono", M.FULL_IMAGE, 1, [20, 28, 10, 40], 0, 0, 0, 0, dict(kind="v", at=33), 20),
    ("mono_non_dual", M.NON_DUAL, 1, [62, 2, 0, 0], 0, 0, 0, 0, dict(kind="noisy"), 21),
    ("mono_subimage", M.SUBIMAGE, 1, [0, 0, 0, 0], 0, 1, 30, 0, dict(kind="down"), 22),
    ("steep_v", M.FULL_IMAGE, 0, [16, 15, 60, 59], 0, 0, 0, 0, dict(kind="v", at=50, slope=4), 23),
    ("shallow_v", M.FULL_IMAGE, 0, [16, 15, 60, 59], 0, 0, 0, 0, dict(kind="v", at=50, slope=12), 24),
]


def main():
    state = {}
    ev = make_evaluator(state)
    arrays, cases, seen = {}, [], set()
    for name, method, mono, last, coarse, twopass, rating, only_4x4, shape, seed in CASES:
        cs = dict(name=name, method=method, mono=mono, last=last, coarse=coarse, twopass=twopass, rating=rating, only_4x4=only_4x4, shape=shape, seed=seed)
        max_level, levels, searches, tables = run_case(ev, state, cs)
        cs.update(max_level=max_level, levels=levels)
        kw = dict(coarse=coarse, twopass=twopass, rating=rating, only_4x4=only_4x4)
        starts = [(last[0] + last[1] + 1) >> 1, last[0], last[1], last[2], last[3]]
        for s in searches:
            t = tables[(s["plane"], s["dir"], s["fixed"])]
            s["start"] = starts[s["idx"]]
            s["table"] = "t_%s_%d" % (name, s["idx"])
            arrays[s["table"]] = np.array(t[:max_level + 1] + [-1] * (63 - max_level), np.int64)
            events = []
            s["best"], calls = M.walk(t, s["start"], max_level, events=events, **kw)
            assert calls == s["calls"], (name, s["idx"], calls, s["calls"])          # the model walks as the reference did
            seen.update(events)
            seen.update(["start<16"] if min(max(s["start"], 0), max_level) < 16 else [])
            seen.update(["start>=60"] if min(s["start"], max_level) >= 60 else [])
            if "clamped_up" in events and events[-1] == "max":
                seen.add("max_by_clamped_step")
        want, _ = M.pick_frame(lambda p, d, f: tables[(p, d, -1 if f is None else f)], method, mono, last, max_level, **kw)
        n = 2 if mono else 4
        assert want[:n] == levels[:n], (name, want, levels)
        assert [s["idx"] for s in searches] == [i for i in range(5) if (i == 0 or (i in (1, 2) and method != M.NON_DUAL) or (i > 2 and not mono))]
        seen.update(["max47"] if max_level == 47 else [])
        seen.update(["coarse"] if coarse else []); seen.update(["only_4x4"] if only_4x4 else [])
        seen.update(["rating<20"] if twopass and rating < 20 else []); seen.update(["rating>=20"] if twopass and rating >= 20 else [])
        seen.update(["non_dual"] if method == M.NON_DUAL else []); seen.update(["mono"] if mono else []); seen.update(["zeros"] if not any(last) else [])
        cs["searches"] = searches
        del cs["shape"], cs["seed"]
        cases.append(cs)
        print(name, max_level, levels, [len(s["calls"]) for s in searches])
    a, b = cases[0], cases[1]          # one family: the dir 0 table follows the dir 2 result
    assert a["searches"][1]["fixed"] != b["searches"][1]["fixed"] and not np.array_equal(arrays[a["searches"][1]["table"]], arrays[b["searches"][1]["table"]])
    seen.add("dir0_depends_on_dir2")
    need = {"down_by_bias", "up", "again", "zero", "max_by_clamped_step", "max47", "coarse", "rating<20", "rating>=20", "only_4x4", "start<16", "start>=60",
            "non_dual", "mono", "dir0_depends_on_dir2", "zeros"}
    assert need <= seen, need - seen
    save("ref_eval_lpf_pick.npz", arrays, cases)


if __name__ == "__main__":
    main()
