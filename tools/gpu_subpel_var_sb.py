"""A/B on one MI355X: aomhip_sub_pixel_variance_batch (every evaluation gathered from global memory) against
aomhip_sub_pixel_variance_sb_batch (the same list bucketed by cell, served from the LDS strip walk) on the two Mode-A sub-pel workloads of
benchlib/variance.py -- same seeds, same lists, same ring of frames.
    python tools/gpu_subpel_var_sb.py [--repeats 5] [--reps 10] [--frames-1080p 64] [--frames-4k 32] [--out profiles/subpel_var_sb.json]
Per workload and repeat both calls are timed in this process with HIP events after the clock ramp (benchlib.common.kernel_avg_ms), every
evaluation of the first and the last ring slot is compared between the two, and the result goes to profiles/subpel_var_sb.json.
For the kernel trace: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/gpu_subpel_var_sb.py --repeats 1 --out /dev/null"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aom_av1_psy_amd as pkg  # noqa: E402
from benchlib.common import HBM_PEAK_GBS, kernel_avg_ms  # noqa: E402
from benchlib.variance import VAR_WORKLOADS  # noqa: E402

# candidate cells per workload: each is timed once, the fastest takes the repeats (--cell WxH pins one)
CELLS = {"sub_pixel_variance16x16_modeA_1080p_8bit": [(240, 64), (240, 32), (480, 32), (320, 48)],
         "sub_pixel_variance16x16_modeA_4k_10bit": [(160, 32), (80, 32), (128, 32), (240, 16)]}
RANGE = 64


def run(ctx, name, frames, repeats, reps, pinned=None):
    cfg = VAR_WORKLOADS[name]
    W, H, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    F = frames or cfg["frames"]
    capi, synth = pkg.capi, pkg.synth
    border = 160
    src, ref = ctx.planes_alloc(W, H, border, bd, F), ctx.planes_alloc(W, H, border, bd, F)
    for f in range(F):
        ctx.planes_upload(src, f, synth.lcg_frame(W, H, 2 * f, 0, bd)); ctx.planes_upload(ref, f, synth.lcg_frame(W, H, 2 * f + 1, 0, bd))
    # the list of benchlib/variance.py run_variance(), draw for draw (the ring length sets the shape of the draws: use the bench's F to get
    # the bench's lists)
    base_c, _ = synth.mode_a_worklist(W, H, 16, seed=1, search=64)
    nb = len(base_c)
    n = 5 * nb
    rng = np.random.default_rng(4242)
    cands = np.zeros((F, nb, 5), capi.var_cand_dtype)
    cands["sx"], cands["sy"] = base_c["sx"][None, :, None], base_c["sy"][None, :, None]
    cands["rx"], cands["ry"] = cands["sx"], cands["sy"]
    cands["rx"][:, :, 1:] += rng.integers(-64, 65, (F, nb, 4), dtype=np.int16)
    cands["ry"][:, :, 1:] += rng.integers(-64, 65, (F, nb, 4), dtype=np.int16)
    off = rng.integers(1, 64, (F, nb, 5))    # (xoff, yoff) != (0, 0)
    cands["xoff"], cands["yoff"] = off & 7, off >> 3
    cands = cands.reshape(F, n)
    d_c = ctx.to_device(np.ascontiguousarray(cands))
    d_var, d_sse, d_var2, d_sse2 = (ctx.malloc(F * n * 4) for _ in range(4))
    state = {}

    def use(cell):
        for d in state.get("dev", ()):
            ctx.free(d)
        perm, boff = synth.bucket_order(cands[0]["sx"], cands[0]["sy"], W, H, *cell)
        state.update(cell=cell, perm=perm, nb=len(boff) - 1, dev=(ctx.to_device(np.ascontiguousarray(cands[:, perm])), ctx.to_device(boff)))

    def direct():
        ctx.variance_batch(src, ref, 0, F, 16, 16, d_c, n, n, d_var, d_sse, subpel=True)

    def bucketed():
        ctx.sub_pixel_variance_sb_batch(src, ref, 0, F, 16, 16, state["cell"][0], state["cell"][1], RANGE, state["nb"], state["dev"][0], state["dev"][1],
                                        n, n, d_var2, d_sse2)

    tried = {}
    for cell in ([pinned] if pinned else CELLS[name]):
        use(cell)
        try:
            tried["%dx%d" % cell] = kernel_avg_ms(ctx, bucketed, reps)
        except capi.AomHipError as e:   # (a window beyond the LDS budget)
            tried["%dx%d" % cell] = str(e)
    best = min((v, k) for k, v in tried.items() if isinstance(v, float))[1]
    cell = tuple(int(x) for x in best.split("x"))
    use(cell)
    perm = state["perm"]
    ctx.memset(d_var2, 0xff, F * n * 4); ctx.memset(d_sse2, 0xff, F * n * 4)
    t_direct, t_sb = [], []
    for _ in range(repeats):
        t_direct.append(kernel_avg_ms(ctx, direct, reps))
        t_sb.append(kernel_avg_ms(ctx, bucketed, reps))
    fallbacks = ctx.debug_subpel_sb_fallbacks()
    info = ctx.debug_subpel_sb_launch_info()
    same = True
    for f in sorted({0, F - 1}):
        for a, b in ((d_var, d_var2), (d_sse, d_sse2)):
            same &= bool(np.array_equal(ctx.from_device(a + f * n * 4, (n,), np.uint32)[perm], ctx.from_device(b + f * n * 4, (n,), np.uint32)))
    es = 1 if bd == 8 else 2
    compulsory = F * (2 * W * H * es + n * (12 + 8))    # benchlib/variance.py: every visible byte once + list + results
    frac = lambda ms: compulsory / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS  # noqa: E731
    avg_d, avg_s = float(np.mean(t_direct)), float(np.mean(t_sb))
    res = {"workload": name, "frames": F, "evaluations_per_launch": F * n, "cell": list(cell), "range": RANGE,
           "direct": {"kernel": "variance_kernel<SUBPEL>", "avg_launch_ms": avg_d, "repeats_ms": t_direct, "spread_ms": max(t_direct) - min(t_direct),
                      "frac_compulsory": frac(avg_d)},
           "bucketed": {"kernel": "subpel_strip_kernel", "avg_launch_ms": avg_s, "repeats_ms": t_sb, "spread_ms": max(t_sb) - min(t_sb),
                        "frac_compulsory": frac(avg_s), "entries_served_from_global_memory": fallbacks},
           "speedup_over_direct": avg_d / avg_s, "slowest_bucketed_lt_fastest_direct": bool(max(t_sb) < min(t_direct)),
           "frac_compulsory": frac(avg_s), "frac_compulsory_target": 0.20, "compulsory_bytes_per_launch": compulsory,
           "identical_to_direct_slot0_and_last": same, "launch": info, "vgprs": info["registers_per_lane"], "lds_bytes": info["lds_bytes"],
           "workgroups_per_cu_by_lds": 160 * 1024 // info["lds_bytes"], "cells_tried_avg_launch_ms": tried}
    for d in (d_c, d_var, d_sse, d_var2, d_sse2) + tuple(state["dev"]):
        ctx.free(d)
    ctx.planes_free(src); ctx.planes_free(ref)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="launches per timed repeat")
    ap.add_argument("--frames-1080p", type=int, default=0, help="ring length (0 = the bench's 64)")
    ap.add_argument("--frames-4k", type=int, default=0, help="ring length (0 = the bench's 32)")
    ap.add_argument("--cell", default="", help="WxH[,WxH]: pin the cell of the 1080p[, 4K] workload instead of trying the candidates")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subpel_var_sb.json"))
    args = ap.parse_args()
    ctx = pkg.capi.Context(0)
    out = {"tool": "tools/gpu_subpel_var_sb.py", "hbm_peak_GBs": HBM_PEAK_GBS, "workloads": []}
    pins = [tuple(int(x) for x in c.split("x")) for c in args.cell.split(",") if c] + [None, None]
    for k, (name, frames) in enumerate((("sub_pixel_variance16x16_modeA_1080p_8bit", args.frames_1080p), ("sub_pixel_variance16x16_modeA_4k_10bit", args.frames_4k))):
        r = run(ctx, name, frames, args.repeats, args.reps, pins[k])
        print(json.dumps(r), flush=True)
        out["workloads"].append(r)
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ok = all(w["identical_to_direct_slot0_and_last"] and w["slowest_bucketed_lt_fastest_direct"] for w in out["workloads"])
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
