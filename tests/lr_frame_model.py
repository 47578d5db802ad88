"""A small model of the stripe-exact loop-restoration frame filter (av1_loop_restoration_filter_unit, av1/common/restoration.c:1024-1090), independent of
the device code: it applies the ROW RULE of the processing stripes and hands every stripe of every unit, as a padded image, to the oracle's two
unit filters (orc_lr of tests/test_golden_lr_apply.py, pinned bit for bit by ref_eval_lr_apply.npz).

Stripe k of a plane covers rows [max(0, k SH - off), min((k + 1) SH - off, plane_h)), SH = 64 >> ss_y, off = 8 >> ss_y.  A filter call on stripe [y0, y1)
reads rows y0 - 3 .. y1 + 2:
    rows y0 .. y1 - 1                  cdef[y]
    y0 - 3, y0 - 2     y0 > 0          deblocked[y0 - 2]
    y0 - 1             y0 > 0          deblocked[y0 - 1]
    y0 - 3 .. y0 - 1   y0 == 0         cdef[0]
    y1                 y1 < plane_h    deblocked[y1]
    y1 + 1, y1 + 2     y1 < plane_h    deblocked[min(y1 + 1, plane_h - 1)]
    y1 .. y1 + 2       y1 == plane_h   cdef[plane_h - 1]
and columns clamped to [0, plane_w - 1].  tests/test_golden_lr_frame.py checks the model against the interpreted reference
(tests/golden/ref_eval_lr_frame.npz), tests/test_gpu_lr_frame.py checks the device against both."""
import numpy as np

from test_golden_lr_apply import orc_lr

RESTORE_NONE, RESTORE_WIENER, RESTORE_SGRPROJ = 0, 1, 2


def stripe_of(y, ss_y):
    return (y + (8 >> ss_y)) // (64 >> ss_y)


def stripe_rows(k, plane_h, ss_y):
    sh, off = 64 >> ss_y, 8 >> ss_y
    return max(0, k * sh - off), min((k + 1) * sh - off, plane_h)


def internal_boundaries(plane_h, ss_y):
    """First rows of the stripes 1, 2, ... of the plane."""
    out, k = [], 1
    while stripe_rows(k, plane_h, ss_y)[0] < plane_h:
        out.append(stripe_rows(k, plane_h, ss_y)[0])
        k += 1
    return out


def source_row(y, y0, y1, plane_h, cdef_only=False):
    """-> (from_deblocked, row) for row y of a filter call on stripe [y0, y1)."""
    if cdef_only:                       # the unit filters "as the search applies them": every context row from the extended CDEF plane
        return False, min(max(y, 0), plane_h - 1)
    if y < y0:
        return (True, max(y, y0 - 2)) if y0 > 0 else (False, 0)
    if y >= y1:
        return (True, min(y, y1 + 1, plane_h - 1)) if y1 < plane_h else (False, plane_h - 1)
    return False, y


def stripe_image(deb, cdef, u, y0, y1, cdef_only=False):
    """Rows y0 - 3 .. y1 + 4 and columns h_start - 3 .. h_end + 4 of what the filter call on rows [y0, y1) of unit u sees; the pixel (h_start, y0)
    is element [3, 3].  (Row y1 + 3 and column h_end + 3 are only ever multiplied by the Wiener filters' tap 7 = 0.)"""
    plane_h, plane_w = cdef.shape
    xs = np.clip(np.arange(u[0] - 3, u[1] + 5), 0, plane_w - 1)
    rows = []
    for y in range(y0 - 3, y1 + 5):
        d, ry = source_row(min(y, y1 + 2), y0, y1, plane_h, cdef_only)
        rows.append((deb if d else cdef)[ry, xs])
    return np.stack(rows)


def filter_units(oracle, deb, cdef, bd, ss_y, units, infos, out, cdef_only=False):
    """units: rows (h_start, h_end, v_start, v_end); infos: dicts with type [, idx, xqd | fx, fy].  Writes the units' pixels into `out` in place."""
    plane_h = cdef.shape[0]
    for u, inf in zip(units, infos):
        hs, he, vs, ve = (int(v) for v in u)
        if inf["type"] not in (RESTORE_WIENER, RESTORE_SGRPROJ):
            out[vs:ve, hs:he] = cdef[vs:ve, hs:he]
            continue
        for k in range(stripe_of(vs, ss_y), stripe_of(ve - 1, ss_y) + 1):
            s0, s1 = stripe_rows(k, plane_h, ss_y)
            y0, y1 = max(s0, vs), min(s1, ve)
            img = stripe_image(deb, cdef, (hs, he), y0, y1, cdef_only)
            c = dict(bd=bd, w=he - hs, h=y1 - y0)
            if inf["type"] == RESTORE_SGRPROJ:
                c.update(kind="sgr", idx=int(inf["idx"]), xqd=[int(v) for v in inf["xqd"]])
            else:
                c.update(kind="wiener", fx=[int(v) for v in inf["fx"]], fy=[int(v) for v in inf["fy"]])
            out[y0:y1, hs:he] = orc_lr(oracle, img, c)
    return out


def units_in_plane(plane_w, plane_h, unit_size, ss_y):
    """foreach_rest_unit_in_tile / av1_foreach_rest_unit_in_row (restoration.c:1206-1294) for the whole-frame tile -> [(h_start, h_end, v_start, v_end)]"""
    def cut(size):
        pos, out = 0, []
        while pos < size:
            n = size - pos if size - pos < unit_size * 3 // 2 else unit_size
            out.append((pos, pos + n))
            pos += n
        return out
    off = 8 >> ss_y
    res = []
    for (a, b) in cut(plane_h):
        vs, ve = max(0, a - off), (b - off if b < plane_h else b)
        res += [(x0, x1, vs, ve) for (x0, x1) in cut(plane_w)]
    return res


def random_infos(rng, n_units, first=0, sgr_first=0):
    """Per-unit parameters: the three types in turn (starting with `first`), SGR sets with both radii / r1 == 0 (10 .. 13) / r0 == 0 (14, 15) in turn (starting
    with `sgr_first`),
    xqd over its coded range, symmetric Wiener taps in their coded ranges (centre stored minus 128, tap 7 = 0)."""
    infos, n_sgr = [], sgr_first
    for i in range(n_units):
        t = (RESTORE_WIENER, RESTORE_SGRPROJ, RESTORE_NONE)[(i + first) % 3]
        inf = dict(type=t, idx=0, xqd=[0, 0], fx=[0] * 8, fy=[0] * 8)
        if t == RESTORE_SGRPROJ:
            inf["idx"] = int((rng.integers(0, 10), rng.integers(10, 14), rng.integers(14, 16))[n_sgr % 3])
            inf["xqd"] = [int(rng.integers(-96, 32)), int(rng.integers(-32, 96))]
            n_sgr += 1
        elif t == RESTORE_WIENER:
            for key in ("fx", "fy"):
                t0, t1, t2 = int(rng.integers(-5, 11)), int(rng.integers(-23, 9)), int(rng.integers(-17, 47))
                inf[key] = [t0, t1, t2, -2 * (t0 + t1 + t2), t2, t1, t0, 0]
        infos.append(inf)
    return infos


def seeded_planes(rng, w, h, bd, ss_y=0):
    """-> (deblocked, cdef): one smooth image plus INDEPENDENT noise for each, with 0 / maximum patches; the deblocked plane alone also gets 8-pixel
    runs of 0 / maximum in the two rows on either side of every stripe boundary, so that the context rows differ strongly between the two."""
    i, j = np.indices((h, w))
    mx = (1 << bd) - 1
    base = (mx // 2 + (mx // 5) * np.sin(i / 9.0) * np.cos(j / 7.0)).astype(np.int64) + ((i * 3 + j * 5) % 17) * (1 << (bd - 8))
    planes = []
    for _ in range(2):
        p = base + rng.integers(-16, 17, (h, w)) * (1 << (bd - 8))
        for n in range(4):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            p[max(y - 2, 0):y + 3, max(x - 3, 0):x + 4] = 0 if n % 2 else mx
        if not planes:
            for b in internal_boundaries(h, ss_y):
                for n, x in enumerate(range(int(rng.integers(0, 8)), w, 20)):
                    p[b - 2:b + 2, x:x + 8] = 0 if n % 2 else mx
        planes.append(np.clip(p, 0, mx).astype(np.uint8 if bd == 8 else np.uint16))
    return planes
