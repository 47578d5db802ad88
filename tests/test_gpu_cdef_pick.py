"""aomhip_cdef_pick_strengths and aomhip_cdef_search_frame through the C ABI, every comparison exact: the fixture of the interpreted reference
(tests/golden/ref_eval_cdef_pick.npz) field by field with its trace; synthetic tables against tests/cdef_pick_model.py at the entry counts where the
kernels' chunking changes (32 entries per staging round, 256 lanes, 32 workgroups), with 64-bit sums and forced ties; whole frames against the model fed
with the oracle's distortion tables; one captured graph of search + filter replayed on two frames; the refused arguments."""
import ctypes

import numpy as np
import pytest

import cdef_pick_model as M
from test_golden_cdef_pick import CASES, Z, tables_of

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
FILL = 0x5a


def strengths_bytes(strengths):
    return np.asarray(strengths, np.uint8).reshape(-1, 2)


def run_pick(hip, ctx, m0, m1, n, fast, rdmult, strengths, count=None, capacity=None):
    """-> (record, entry_gi, trace) with every output pre-filled with 0x5a"""
    K = hip.capi
    count = len(m0) if count is None else count
    capacity = max(len(m0), 1) if capacity is None else capacity
    d_m0 = ctx.to_device(np.ascontiguousarray(m0, np.uint64))
    d_m1 = ctx.to_device(np.ascontiguousarray(m1, np.uint64)) if m1 is not None else None
    d_cnt, d_st = ctx.to_device(np.array([count], np.int32)), ctx.to_device(strengths_bytes(strengths))
    sizes = (K.cdef_pick_dtype.itemsize, max(capacity, 16), K.CDEF_PICK_MAX_CALLS * K.cdef_pick_trace_dtype.itemsize)
    d_pick, d_gi, d_tr = (ctx.malloc(s) for s in sizes)
    for d, s in zip((d_pick, d_gi, d_tr), sizes):
        ctx.memset(d, FILL, s)
    ctx.cdef_pick_strengths(d_m0, d_m1, d_cnt, capacity, d_st, n, int(fast), rdmult, d_pick, d_gi, d_tr)
    rec = ctx.from_device(d_pick, (1,), K.cdef_pick_dtype)[0]
    gi = ctx.from_device(d_gi, (max(capacity, 16),), np.int8)
    tr = ctx.from_device(d_tr, (K.CDEF_PICK_MAX_CALLS,), K.cdef_pick_trace_dtype)
    for d in (d_m0, d_m1, d_cnt, d_st, d_pick, d_gi, d_tr):
        if d is not None:
            ctx.free(d)
    return rec, gi, tr


def check_record(rec, want, what):
    assert (int(rec["cdef_bits"]), int(rec["nb_cdef_strengths"]), int(rec["sb_count"]), int(rec["reserved"])) == \
        (want["cdef_bits"], want["nb_cdef_strengths"], want["sb_count"], 0), what
    assert [int(v) for v in rec["cdef_strengths"]] == want["cdef_strengths"] and [int(v) for v in rec["cdef_uv_strengths"]] == want["cdef_uv_strengths"], what
    assert int(rec["best_rd"]) == want["best_rd"], what
    assert [int(v) for v in rec["tot_mse"]] == want["tot_mse"] and [int(v) for v in rec["rd"]] == want["rd"], what


def check_pick(rec, gi, tr, want, what):
    check_record(rec, want, what)
    cnt, calls = want["sb_count"], len(want["trace"])
    assert [int(v) for v in gi[:cnt]] == want["entry_gi"], what
    assert (gi[cnt:] == FILL).all(), what                              # nothing past the entries
    got = [[int(t["id0"]), int(t["id1"]), int(t["best_tot_mse"])] for t in tr[:calls]]
    assert got == [list(t) for t in want["trace"]], (what, [k for k in range(calls) if got[k] != list(want["trace"][k])][:3])
    assert (tr[calls:].view(np.uint8) == FILL).all(), what


@pytest.mark.parametrize("k", range(len(CASES)))
def test_fixture_cases(hip, ctx, k):
    """every case of the interpreted reference, compared with what the reference recorded"""
    c = CASES[k]
    m0, m1 = tables_of(c)
    strengths = M.mapped([tuple(s) for s in c["strengths"]])
    rec, gi, tr = run_pick(hip, ctx, m0, m1, c["n"], c["method"] > 0, c["rdmult"], strengths)
    nb = c["nb_cdef_strengths"]
    joint = [int(v) for v in c["joint"]]
    want = dict(cdef_bits=c["cdef_bits"], nb_cdef_strengths=nb, sb_count=c["sb_count"], cdef_strengths=c["cdef_strengths"] + [0] * (8 - nb),
                cdef_uv_strengths=c["cdef_uv_strengths"] + [0] * (8 - nb), best_rd=int(c["best_rd"]), tot_mse=joint + [M64] * (4 - len(joint)),
                rd=[int(v) for v in c["rd"]], entry_gi=c["entry_gi"], trace=c["trace"])
    check_pick(rec, gi, tr, want, k)


def synthetic(seed, count, n, dual, kind):
    rng = np.random.default_rng(seed)

    def one():
        hi = 1 << 40 if kind == "big" else 1 << 20
        base = rng.integers(hi >> 6, hi >> 1, n)
        t = (base[None, :] + rng.integers(0, hi >> 1, (count, n))).astype(np.int64)
        for i in range(0, count, 3):                      # entries that favour one column strongly: several strengths pay off
            t[i, (i * 5) % n] >>= 6
        if kind == "ties":
            t[:, n - 1] = t[:, 0]
            if n > 3:
                t[:, n // 2] = t[:, 1]
        return t
    return one(), (one() if dual else None)


# (entries, n_strengths, dual, fast, rdmult, kind): the entry counts around the chunk (32), the workgroup (256) and a 4K frame's 2040 (more than
# 32 workgroups x 32 entries: a workgroup loops); 2^40 values; duplicated columns; rdmult 0, typical, huge
SYNTH = [(0, 4, True, True, 1200, "spread"), (1, 4, True, True, 1200, "spread"), (0, 10, False, False, 1200, "spread"), (1, 10, False, True, 0, "spread"),
         (255, 10, True, True, 1200, "ties"), (256, 20, True, True, 0, "big"), (257, 64, True, False, 30000, "big"), (257, 2, True, True, 1200, "ties"),
         (2040, 32, True, True, 1200, "big"), (2040, 64, True, False, 1200, "spread"), (2040, 64, False, False, 2000000000, "big"), (2040, 64, False, True, 1200, "ties"), (33, 64, True, False, 1200, "ties"),
         (1056, 20, False, False, 1200, "spread"), (31, 32, False, True, 2000000000, "spread")]


@pytest.mark.parametrize("case", range(len(SYNTH)))
def test_synthetic_tables_against_model(hip, ctx, case):
    count, n, dual, fast, rdmult, kind = SYNTH[case]
    m0, m1 = synthetic(100 + case, count, n, dual, kind)
    method = M.NB_STRENGTHS.index(n)
    strengths = M.mapped(M.strength_list(method))
    want = M.pick(m0, m1, n, fast, rdmult, strengths, vector=True)
    if kind == "big" and count > 1:
        assert max(want["tot_mse"][0], 0) > 1 << 32
    rec, gi, tr = run_pick(hip, ctx, m0, m1, n, fast, rdmult, strengths, capacity=max(count, 1))
    check_pick(rec, gi, tr, want, SYNTH[case])


def test_count_is_read_from_the_device(hip, ctx):
    """tables with room for 300 entries of which the device word says 70: the launches are sized by the capacity, the result is the 70's"""
    m0, m1 = synthetic(7, 300, 10, True, "spread")
    strengths = M.mapped(M.strength_list(3))
    want = M.pick(m0[:70], m1[:70], 10, True, 900, strengths, vector=True)
    rec, gi, tr = run_pick(hip, ctx, m0, m1, 10, True, 900, strengths, count=70, capacity=300)
    check_pick(rec, gi, tr, want, "count 70 of 300")


# ---- whole frames
def content(rng, W, H, bd, seed_shift=0):
    mx = (1 << bd) - 1
    base = rng.integers(mx // 8, mx - mx // 8, (H // 8 + 1, W // 8 + 1))
    i, j = np.indices((H, W))
    pix = np.kron(base, np.ones((8, 8), np.int64))[:H, :W] + ((i * 3 + j * 5 + seed_shift) % 17) * (mx // 255 + 1) + rng.integers(-8, 9, (H, W)) * (mx // 255 + 1)
    src = np.clip(pix, 0, mx)
    rec = np.clip(src + rng.integers(-(6 << (bd - 8)), (6 << (bd - 8)) + 1, (H, W)), 0, mx)
    dt = np.uint8 if bd == 8 else np.uint16
    return rec.astype(dt), src.astype(dt)


def make_frame(seed, W, H, bd, planes, xdec, ydec, all_skip=(), skip_rate=0.25):
    rng = np.random.default_rng(seed)
    recon, source = [], []
    for p in range(planes):
        r, s = content(rng, W >> (xdec if p else 0), H >> (ydec if p else 0), bd, p)
        recon.append(r); source.append(s)
    skip = (rng.random((H // 8, W // 8)) < skip_rate).astype(np.uint8)
    for (r, c) in all_skip:
        skip[r * 8:r * 8 + 8, c * 8:c * 8 + 8] = 1
    return recon, source, skip


class FrameRun:
    """the device side of one aomhip_cdef_search_frame call: rings, inputs, outputs pre-filled with 0x5a"""

    def __init__(self, hip, ctx, W, H, bd, planes, xdec, ydec, n, fb_stride=None, border=16):
        K = hip.capi
        self.K, self.ctx, self.W, self.H, self.bd, self.planes, self.xdec, self.ydec, self.n = K, ctx, W, H, bd, planes, xdec, ydec, n
        self.nvfb, self.nhfb = (H + 63) // 64, (W + 63) // 64
        self.fbs = fb_stride or self.nhfb
        self.border = border
        dims = [(W >> (xdec if p else 0), H >> (ydec if p else 0)) for p in range(planes)]
        self.recon = [ctx.planes_alloc(w, h, border, bd, 1) for w, h in dims]
        self.source = [ctx.planes_alloc(w, h, border, bd, 1) for w, h in dims]
        self.filtered = [ctx.planes_alloc(w, h, border, bd, 1) for w, h in dims]
        rows = self.nvfb * self.fbs
        self.sizes = dict(index=max(rows, 16), pri=max(rows, 16), sec=max(rows, 16), uv_pri=max(rows, 16), uv_sec=max(rows, 16), pick=K.cdef_pick_dtype.itemsize,
                          dir=max((H // 8) * (W // 8), 16), var=4 * (H // 8) * (W // 8), mse0=8 * rows * n, mse1=8 * rows * n, entry_fb=4 * rows)
        self.d = {k: ctx.malloc(v) for k, v in self.sizes.items()}
        self.d_skip = ctx.malloc(max((H // 8) * (W // 8), 16))
        self.d_class = ctx.malloc(max(rows, 16))
        self.d_st = ctx.malloc(128)

    def upload(self, recon, source, skip, classes=None, strengths=None):
        for p in range(self.planes):
            self.ctx.planes_upload(self.recon[p], 0, recon[p]); self.ctx.planes_upload(self.source[p], 0, source[p])
        self.ctx.memcpy_h2d(self.d_skip, np.ascontiguousarray(skip, np.uint8))
        if classes is not None:
            full = np.zeros((self.nvfb, self.fbs), np.uint8)
            full[:, :self.nhfb] = classes
            self.ctx.memcpy_h2d(self.d_class, full)
        if strengths is not None:
            self.ctx.memcpy_h2d(self.d_st, strengths_bytes(strengths))

    def fill(self):
        for k, v in self.sizes.items():
            self.ctx.memset(self.d[k], FILL, v)

    def search(self, fast, damping, rdmult, with_classes=False):
        d = self.d
        self.ctx.cdef_search_frame(self.recon, 0, self.source, 0, self.xdec, self.ydec, self.d_st, self.n, int(fast), self.d_skip, damping, rdmult, self.fbs,
                                   d["index"], d["pri"], d["sec"], d["pick"], d["uv_pri"] if self.planes > 1 else None, d["uv_sec"] if self.planes > 1 else None,
                                   self.d_class if with_classes else None, d["dir"], d["var"], d["mse0"], d["mse1"] if self.planes > 1 else None, d["entry_fb"])

    def filter(self, damping):
        d = self.d
        self.ctx.cdef_luma_plane(self.recon[0], 0, self.filtered[0], 0, d["pri"], d["sec"], self.fbs, self.d_skip, damping, d["dir"], None)
        for p in range(1, self.planes):
            self.ctx.cdef_chroma_plane(self.recon[p], 0, self.filtered[p], 0, self.xdec, self.ydec, d["dir"], d["uv_pri"], d["uv_sec"], self.fbs, self.d_skip, damping)

    def get(self, k, shape, dtype):
        return self.ctx.from_device(self.d[k], shape, dtype)

    def plane(self, rings, p):
        b = self.border
        w, h = self.W >> (self.xdec if p else 0), self.H >> (self.ydec if p else 0)
        return self.ctx.planes_download(rings[p], 0)[b:b + h, b:b + w]

    def close(self):
        for p in self.recon + self.source + self.filtered:
            self.ctx.planes_free(p)
        for v in list(self.d.values()) + [self.d_skip, self.d_class, self.d_st]:
            self.ctx.free(v)


def oracle_tables(oracle, recon, source, skip, strengths, damping, bd, xdec, ydec):
    raw = [oracle.cdef_search_sse_luma(recon[0], source[0], strengths, skip, damping, bd)]
    _, ldir, lvar = oracle.cdef_plane_luma(recon[0], np.ones(raw[0].shape[1:], np.uint8), np.zeros(raw[0].shape[1:], np.uint8), skip, damping, bd)
    for p in range(1, len(recon)):
        raw.append(oracle.cdef_search_sse_chroma(recon[p], source[p], xdec, ydec, ldir, strengths, skip, damping, bd))
    return raw, ldir, lvar


def check_frame(hip, run, want, raw, ldir, lvar, classes, strengths_model, what):
    K = hip.capi
    nvfb, nhfb, fbs, n = run.nvfb, run.nhfb, run.fbs, run.n
    rec = run.get("pick", (1,), K.cdef_pick_dtype)[0]
    check_record(rec, want, what)
    cnt = want["sb_count"]
    # the index plane, and the four level planes = aomhip_cdef_build_strengths on the same index and the record
    idx = run.get("index", (nvfb, fbs), np.int8)
    assert np.array_equal(idx[:, :nhfb], want["fb_index"]), what
    assert (idx[:, nhfb:] == FILL).all()
    flat = np.ascontiguousarray(idx[:, :nhfb]).ravel()
    outs = [np.zeros(flat.size, np.uint8) for _ in range(4)]
    ys, uvs = np.ascontiguousarray(rec["cdef_strengths"], np.int32), np.ascontiguousarray(rec["cdef_uv_strengths"], np.int32)
    vp = ctypes.c_void_p
    assert K.lib.aomhip_cdef_build_strengths(vp(flat.ctypes.data), ctypes.c_int(flat.size), vp(ys.ctypes.data), vp(uvs.ctypes.data),
                                             *[vp(o.ctypes.data) for o in outs]) == 0
    for key, o in zip(("pri", "sec", "uv_pri", "uv_sec"), outs):
        got = run.get(key, (nvfb, fbs), np.uint8)
        if run.planes == 1 and key.startswith("uv"):
            assert (got == FILL).all()
        else:
            assert np.array_equal(got[:, :nhfb], o.reshape(nvfb, nhfb)), (what, key)
    assert np.array_equal(run.get("dir", ldir.shape, np.uint8), ldir) and np.array_equal(run.get("var", lvar.shape, np.int32), lvar), what
    # the optional outputs: the compacted tables and the entry -> filter block map
    m0 = run.get("mse0", (nvfb * fbs, n), np.uint64)
    assert np.array_equal(m0[:cnt], np.asarray(want["mse0"], np.uint64).reshape(cnt, n)), what
    if run.planes > 1:
        m1 = run.get("mse1", (nvfb * fbs, n), np.uint64)
        assert np.array_equal(m1[:cnt], np.asarray(want["mse1"], np.uint64).reshape(cnt, n)), what
    efb = run.get("entry_fb", (nvfb * fbs,), np.int32)
    assert [int(v) for v in efb[:cnt]] == [r * fbs + c for r, c in want["entries"]], what
    return rec


FRAMES = [
    # name, W, H, bd, planes, xdec, ydec, method, rdmult, damping, all-skip blocks, fb_stride
    ("420_8_full", 336, 208, 8, 3, 1, 1, 0, 1200, 5, [(0, 2), (2, 3), (3, 5)], None),
    ("420_10_lvl1", 336, 208, 10, 3, 1, 1, 1, 40000, 4, [(1, 1), (1, 2)], 7),
    ("420_10_lvl2", 336, 208, 10, 3, 1, 1, 2, 0, 6, [(0, 0)], None),
    ("420_12_lvl3", 336, 208, 12, 3, 1, 1, 3, 700, 3, [(2, 2)], None),
    ("420_12_lvl4", 336, 208, 12, 3, 1, 1, 4, 2000000000, 5, [(0, 4)], None),
    ("420_8_lvl5", 336, 208, 8, 3, 1, 1, 5, 300, 5, [(3, 0), (3, 1)], None),
    ("mono_10_lvl2", 200, 136, 10, 1, 0, 0, 2, 900, 5, [(1, 1)], None),
    ("444_8_lvl3", 136, 200, 8, 3, 0, 0, 3, 900, 4, [(2, 1)], None),
]


@pytest.mark.parametrize("case", range(len(FRAMES)))
def test_search_frame_against_model(hip, oracle, ctx, case):
    name, W, H, bd, planes, xdec, ydec, method, rdmult, damping, all_skip, fb_stride = FRAMES[case]
    n = M.NB_STRENGTHS[method]
    strengths = M.mapped(M.strength_list(method))
    recon, source, skip = make_frame(50 + case, W, H, bd, planes, xdec, ydec, all_skip)
    raw, ldir, lvar = oracle_tables(oracle, recon, source, skip, strengths, damping, bd, xdec, ydec)
    want = M.search_frame(raw[0].astype(np.int64), raw[1].astype(np.int64) if planes > 1 else None, raw[2].astype(np.int64) if planes > 1 else None, skip, None, bd,
                          strengths, method > 0, rdmult, vector=True)
    assert all(e not in want["entries"] for e in all_skip) and 0 < want["sb_count"] < ((H + 63) // 64) * ((W + 63) // 64)
    run = FrameRun(hip, ctx, W, H, bd, planes, xdec, ydec, n, fb_stride)
    run.upload(recon, source, skip, None, strengths)
    run.fill()
    run.search(method > 0, damping, rdmult)
    check_frame(hip, run, want, raw, ldir, lvar, None, strengths, name)
    run.close()


def test_search_frame_128_classes(hip, oracle, ctx):
    """320 x 256 with 128 classes: a 128x128 at the right edge whose second column lies outside the frame, a 128x64 pair, 64x128 columns, an all-skip
    block inside a 128x128 and one that is a 128x128's top-left (the entry is then left out although its other blocks are not skipped)"""
    W, H, bd, method, damping, rdmult = 320, 256, 10, 3, 5, 600
    c = M
    classes = np.array([[c.FB_128X128, c.FB_128X128, c.FB_128X64, c.FB_128X64, c.FB_128X128],
                        [c.FB_128X128, c.FB_128X128, c.FB_64, c.FB_64, c.FB_128X128],
                        [c.FB_64X128, c.FB_64, c.FB_128X128, c.FB_128X128, c.FB_64X128],
                        [c.FB_64X128, c.FB_64, c.FB_128X128, c.FB_128X128, c.FB_64X128]], np.uint8)
    n = M.NB_STRENGTHS[method]
    strengths = M.mapped(M.strength_list(method))
    recon, source, skip = make_frame(77, W, H, bd, 3, 1, 1, [(0, 1), (1, 2), (2, 2)])
    raw, ldir, lvar = oracle_tables(oracle, recon, source, skip, strengths, damping, bd, 1, 1)
    want = M.search_frame(raw[0].astype(np.int64), raw[1].astype(np.int64), raw[2].astype(np.int64), skip, classes, bd, strengths, True, rdmult, vector=True)
    assert want["entries"] == [(0, 0), (0, 2), (0, 4), (1, 3), (2, 0), (2, 1), (2, 4), (3, 1)] and len(M.covered((0, 4), classes, 4, 5)) == 2
    idx = want["fb_index"]
    assert idx[1, 1] == idx[0, 0] >= 0 and idx[0, 3] == idx[0, 2] >= 0 and idx[3, 0] == idx[2, 0] >= 0 and idx[1, 4] == idx[0, 4] >= 0
    assert (idx[2:, 2:4] == -1).all() and idx[1, 2] == -1
    run = FrameRun(hip, ctx, W, H, bd, 3, 1, 1, n)
    run.upload(recon, source, skip, classes, strengths)
    run.fill()
    run.search(True, damping, rdmult, with_classes=True)
    check_frame(hip, run, want, raw, ldir, lvar, classes, strengths, "classes")
    run.close()


def test_capture_once_replay_twice(hip, oracle, ctx):
    """the frame call followed by the three filter calls, which take the device-written levels, captured once and replayed on two uploaded frames: both
    filtered frames equal the oracle's CDEF at the model's strengths (so the launch sequence does not depend on the data)"""
    W, H, bd, method, damping, rdmult = 200, 136, 10, 3, 5, 800
    n = M.NB_STRENGTHS[method]
    strengths = M.mapped(M.strength_list(method))
    run = FrameRun(hip, ctx, W, H, bd, 3, 1, 1, n)
    frames = [make_frame(90, W, H, bd, 3, 1, 1, [(0, 1)], 0.2), make_frame(91, W, H, bd, 3, 1, 1, [(1, 2), (2, 0), (2, 1)], 0.5)]
    run.upload(*frames[0], None, strengths)

    def work():
        run.search(True, damping, rdmult)
        run.filter(damping)
    work()                       # sizes the work memory; nothing is allocated inside the capture
    g = ctx.capture(work)
    picks = []
    for recon, source, skip in (frames[1], frames[0]):
        run.upload(recon, source, skip)
        run.fill()
        ctx.graph_launch(g)
        ctx.sync()
        raw, ldir, lvar = oracle_tables(oracle, recon, source, skip, strengths, damping, bd, 1, 1)
        want = M.search_frame(raw[0].astype(np.int64), raw[1].astype(np.int64), raw[2].astype(np.int64), skip, None, bd, strengths, True, rdmult, vector=True)
        rec = check_frame(hip, run, want, raw, ldir, lvar, None, strengths, "replay")
        picks.append((want["sb_count"], [int(v) for v in rec["cdef_strengths"]]))
        pri, sec = M.levels(want["fb_index"], want["cdef_strengths"])
        upri, usec = M.levels(want["fb_index"], want["cdef_uv_strengths"])
        fy, _, _ = oracle.cdef_plane_luma(recon[0], pri, sec, skip, damping, bd)
        assert np.array_equal(run.plane(run.filtered, 0), fy)
        for p in (1, 2):
            assert np.array_equal(run.plane(run.filtered, p), oracle.cdef_plane_chroma(recon[p], 1, 1, ldir, upri, usec, skip, damping, bd)), p
    assert picks[0][0] != picks[1][0]            # the two frames have different entry counts
    ctx.graph_destroy(g)
    run.close()


def test_refused_arguments(hip, ctx):
    K = hip.capi
    d = ctx.malloc(1 << 16)
    for args in ((None, d, d, 4, d, 4, 1, 100, d, d), (d, d, None, 4, d, 4, 1, 100, d, d), (d, d, d, -1, d, 4, 1, 100, d, d), (d, d, d, 4, d, 0, 1, 100, d, d),
                 (d, d, d, 4, d, 65, 1, 100, d, d), (d, d, d, 4, None, 4, 1, 100, d, d), (d, d, d, 4, d, 4, 1, 100, None, d), (d, d, d, 4, d, 4, 1, 100, d, None)):
        with pytest.raises(K.AomHipError):
            ctx.cdef_pick_strengths(*args)
    y8, y10, c8, c10 = (ctx.planes_alloc(128, 64, 16, 8, 1), ctx.planes_alloc(128, 64, 16, 10, 1), ctx.planes_alloc(64, 32, 16, 8, 1),
                        ctx.planes_alloc(64, 32, 16, 10, 1))
    odd = ctx.planes_alloc(124, 64, 16, 8, 1)

    ctx.memset(d, 0, 1 << 16)                                # strengths { 0, 0 } and a skip map of zeros; every output gets its own 4 KB
    o = [d + 4096 * q for q in range(1, 8)]

    def call(recon=(y8, c8, c8), source=(y8, c8, c8), rf=0, sf=0, xdec=1, ydec=1, n=4, damping=5, fbs=2, index=o[0], pick=o[3], uv=(o[4], o[5])):
        ctx.cdef_search_frame(recon, rf, source, sf, xdec, ydec, d, n, 1, d, damping, 100, fbs, index, o[1], o[2], pick, uv[0], uv[1])
    for p in (y8, c8):
        ctx.planes_upload(p, 0, np.full((p.height, p.width), 100, np.uint8))
    call()                                                   # the baseline is accepted
    for kw in (dict(source=(y10, c10, c10)),                 # mismatched bit depths
               dict(recon=(y8, c10, c10), source=(y8, c10, c10)),   # chroma depth differs from luma
               dict(recon=(y8, y8, y8), source=(y8, y8, y8)),        # chroma geometry does not match xdec / ydec
               dict(recon=(odd, c8, c8), source=(odd, c8, c8)),      # not whole 8x8 blocks
               dict(n=0), dict(n=65), dict(damping=2), dict(damping=7),
               dict(recon=(y8, c8, None)), dict(source=(y8, None, c8)),  # a missing U or V ring
               dict(rf=1), dict(sf=-1),                              # a bad frame index
               dict(fbs=1), dict(xdec=2), dict(index=None), dict(pick=None), dict(uv=(d, None))):
        with pytest.raises(K.AomHipError):
            call(**kw)
    ctx.sync()
    for p in (y8, y10, c8, c10, odd):
        ctx.planes_free(p)
    ctx.free(d)
