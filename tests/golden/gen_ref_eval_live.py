#!/usr/bin/env python3
"""Recorded results of the checks that used to read the reference's sources while the tests ran (run where the reference tree is present).

Outputs, all read by the tests instead of the reference tree:
  * ref_eval_lpf_flat.npz      -- the flat branches of filter6/8/14: the reference's own `*opN = ROUND_POWER_OF_TWO(<expr>, s);` statements
                                  (aom_dsp/loopfilter.c) evaluated on the seeded flat rows of tests/test_oracle_lpf.py;
  * ref_eval_txfm1d_live.npz   -- every 1-D butterfly network of av1_fwd_txfm1d.c / av1_inv_txfm1d.c evaluated (ref_txfm1d_eval.py) on the
                                  seeded inputs of tests/test_oracle_txfm_quant.py::test_txfm1d_networks_live_reference;
  * ref_eval_live_tables.json  -- av1_cospi_arr_data, av1_sinpi_arr_data (av1/common/av1_txfm.c) and default_scan_16x16 (av1/common/scan.c);
  * ref_eval_rtcd_protos.json  -- the `add_proto` lines of aom_dsp/aom_dsp_rtcd_defs.pl and av1/common/av1_rtcd_defs.pl as
                                  {name: [return type, [parameter types]]}, normalised by tests/test_rtcd_protos.py's _signature (names dropped)."""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
import ref_txfm1d_eval as rt  # noqa: E402

REF = rt.REF   # the reference tree the other generators read

LPF_FILTERS = (("filter6", 6), ("filter8", 8), ("filter14", 14))
LPF_TRIALS = 200
TXFM_LIVE_SEED, TXFM_LIVE_ROWS = 7, 20


def lpf_flat_rows():
    """The seeded rows of the flat-filter test: (filter name, rows [trials, 14] in p6..p0 q0..q6 order); same rng stream as the test."""
    rng = np.random.default_rng(1)
    out = []
    for name, _ in LPF_FILTERS:
        rows = np.zeros((LPF_TRIALS, 14), np.int64)
        for t in range(LPF_TRIALS):
            base = int(rng.integers(2, 250))
            p = [base + int(rng.integers(-1, 2)) for _ in range(7)]
            q = [base + int(rng.integers(-1, 2)) for _ in range(7)]
            rows[t] = p[::-1] + q
        out.append((name, rows))
    return out


def gen_lpf():
    src = open(REF + "/aom_dsp/loopfilter.c").read()
    arrays = {}
    for name, rows in lpf_flat_rows():
        body = re.search(r"static INLINE void %s\(.*?\n\}" % name, src, re.S).group(0)
        stm = [(t, re.sub(r"\s+", " ", e), int(s)) for t, e, s in re.findall(r"\*o([pq]\d) = ROUND_POWER_OF_TWO\((.*?),\s*(\d)\);", body, re.S)]
        want = rows.copy()
        for i, row in enumerate(rows):
            taps = {("p%d" % k): int(row[6 - k]) for k in range(7)}
            taps.update({("q%d" % k): int(row[7 + k]) for k in range(7)})
            for t, e, s in stm:
                v = (eval(e, {}, taps) + (1 << (s - 1))) >> s
                want[i, 6 - int(t[1]) if t[0] == "p" else 7 + int(t[1])] = v
        arrays[name + "/rows"], arrays[name + "/want"] = rows, want
        arrays[name + "/statements"] = np.array(len(stm))
    np.savez_compressed(os.path.join(HERE, "ref_eval_lpf_flat.npz"), **arrays)


def gen_txfm1d_live():
    fns, cospi, _ = rt.load_reference_networks()
    rng = np.random.default_rng(TXFM_LIVE_SEED)
    arrays = {}
    for name, fn in fns.items():
        inv, size = name.startswith("av1_i"), fn[0]
        x = rng.integers(-(1 << 17), 1 << 17, size=(TXFM_LIVE_ROWS, size), dtype=np.int64)
        arrays[name + "/in"] = x
        for cb in (10, 13) if not inv else (12,):
            clamp = 18 if inv else 0
            arrays["%s/cb%d/clamp%d" % (name, cb, clamp)] = np.asarray(rt.evaluate(fn, x, cb, cospi[cb - 10], clamp), np.int64)
    np.savez_compressed(os.path.join(HERE, "ref_eval_txfm1d_live.npz"), **arrays)


def gen_tables():
    t = {"av1_cospi_arr_data": rt.parse_int_table(REF + "/av1/common/av1_txfm.c", "av1_cospi_arr_data"),
         "av1_sinpi_arr_data": rt.parse_int_table(REF + "/av1/common/av1_txfm.c", "av1_sinpi_arr_data"),
         "default_scan_16x16": rt.parse_int_table(REF + "/av1/common/scan.c", "default_scan_16x16")}
    with open(os.path.join(HERE, "ref_eval_live_tables.json"), "w") as f:
        json.dump(t, f, separators=(",", ":"))
        f.write("\n")


def gen_rtcd_protos():
    from conftest import BLOCK_SIZES
    from test_rtcd_protos import _signature
    protos = {}
    for rel in ("aom_dsp/aom_dsp_rtcd_defs.pl", "av1/common/av1_rtcd_defs.pl"):
        text = open(os.path.join(REF, rel)).read()
        for m in re.finditer(r'add_proto\s+qw/([^/]*)/\s*,\s*(?:"([^"]+)"\s*,\s*)?"([^"]*)"\s*;', text):
            head, name, args = m.group(1).split(), m.group(2), m.group(3)
            if name is None:
                name, head = head[-1], head[:-1]
            ret = " ".join(head)
            names = [name]
            if "${w}" in name or "${h}" in name:
                names = [name.replace("${w}", str(w)).replace("${h}", str(h)) for w, h in BLOCK_SIZES]
            for n in names:
                protos[n] = _signature(ret, args)  # (a name declared twice: the later add_proto wins, build/cmake/rtcd.pl add_proto)
    with open(os.path.join(HERE, "ref_eval_rtcd_protos.json"), "w") as f:
        json.dump({n: [r, list(p)] for n, (r, p) in sorted(protos.items())}, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    gen_lpf()
    gen_txfm1d_live()
    gen_tables()
    gen_rtcd_protos()
