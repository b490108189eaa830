"""numpy restatement of tiled inference (yms.tiles; csrc/tile.hip) -- TEST INFRASTRUCTURE ONLY.

* ``slice_grid``: the window rule, restated from its definition with a plain start list per axis.
* ``slots``: per image the (frame, bounds, window) of every slot, full view first, and ``table``:
  the [n, S] records (tile, gain_x, gain_y, pad_x, pad_y, lo_x, lo_y, hi_x, hi_y) as a float64 array
  (tile -1 in unused slots), tile inputs numbered image by image, slot by slot.
* ``merge``: row by row in fp32 scalars, one operation per line, so that nothing can be contracted;
  scores copied as bits, -1 for a suppressed row, (0, 0, 0, 0, -1, ...) for an empty or out-of-range slot."""
from __future__ import annotations

import numpy as np

F32 = np.float32
INF = float("inf")


def axis_windows(size, span, step):
    if size <= span:
        return [(0, size)]
    starts = []
    s = 0
    while True:
        starts.append(s)
        if s + span >= size:
            break
        s += step
    if starts[-1] + span > size:
        starts[-1] = max(0, size - span)
    if len(starts) >= 2 and starts[-1] == starts[-2]:
        starts.pop()
    return [(s, s + span) for s in starts]


def slice_grid(h0, w0, tile, overlap=0.2, zoom=1.0):
    span = tile / zoom
    assert span == int(span)
    span = int(span)
    step = span - int(span * overlap)
    return [(x0, y0, x1, y1) for y0, y1 in axis_windows(h0, span, step) for x0, x1 in axis_windows(w0, span, step)]


def letterbox_frame(h0, w0, H, W):
    """yms.data.Letterbox's gain and corner, restated."""
    r = min(H / h0, W / w0)
    nw, nh = min(W, max(1, round(w0 * r))), min(H, max(1, round(h0 * r)))
    return r, r, float(max(0, round((W - nw) / 2 - 0.1))), float(max(0, round((H - nh) / 2 - 0.1)))


def slots(shapes, tile, overlap=0.2, zoom=1.0, full_view=True, edge=None):
    out = []
    for h0, w0 in shapes:
        rows = []
        if full_view:
            rows.append((letterbox_frame(h0, w0, tile, tile), (-INF, -INF, INF, INF), None))
        for x0, y0, x1, y1 in slice_grid(h0, w0, tile, overlap, zoom):
            b = [-INF, -INF, INF, INF]
            if edge is not None:
                if x0 > 0:
                    b[0] = edge
                if y0 > 0:
                    b[1] = edge
                if x1 < w0:
                    b[2] = (x1 - x0) * zoom - edge
                if y1 < h0:
                    b[3] = (y1 - y0) * zoom - edge
            rows.append(((zoom, zoom, -x0 * zoom, -y0 * zoom), tuple(b), (x0, y0, x1, y1)))
        out.append(rows)
    return out


def table(sl):
    S = max(len(r) for r in sl)
    tab = np.zeros((len(sl), S, 9), np.float64)
    tab[..., 0] = -1
    tab[..., 1:3] = 1
    tab[..., 5:7] = -INF
    tab[..., 7:9] = INF
    t = 0
    for b, rows in enumerate(sl):
        for s, (frame, bounds, _) in enumerate(rows):
            tab[b, s] = (t, *frame, *bounds)
            t += 1
    return tab


def merge_row(row, rec, out):
    """One row [4+nc] fp32 through record rec = (gx, gy, px, py, lox, loy, hix, hiy) as fp32 scalars."""
    gx, gy, px, py, lox, loy, hix, hiy = (F32(v) for v in rec)
    cx, cy, w, h = row[0], row[1], row[2], row[3]
    half = F32(0.5)
    with np.errstate(all="ignore"):
        hw = F32(half * w)
        hh = F32(half * h)
        x0 = F32(cx - hw)
        y0 = F32(cy - hh)
        x1 = F32(cx + hw)
        y1 = F32(cy + hh)
        cut = bool(x0 < lox) or bool(y0 < loy) or bool(x1 > hix) or bool(y1 > hiy)
        dx = F32(cx - px)
        dy = F32(cy - py)
        out[0] = F32(dx / gx)
        out[1] = F32(dy / gy)
        out[2] = F32(w / gx)
        out[3] = F32(h / gy)
    if cut:
        out[4:] = F32(-1)
    else:
        out[4:] = row[4:]
    return cut


def merge(pred, tab):
    """pred [T, A, 4+nc] fp32, tab [n, S, 9] (tile index first; any integer) -> [n, S * A, 4+nc]."""
    pred = np.asarray(pred, F32)
    T, A, no = pred.shape
    n, S = tab.shape[:2]
    out = np.zeros((n, S * A, no), F32)
    out[..., 4:] = F32(-1)
    for b in range(n):
        for s in range(S):
            t = int(tab[b, s, 0])
            if not 0 <= t < T:
                continue
            for a in range(A):
                merge_row(pred[t, a], tab[b, s, 1:], out[b, s * A + a])
    return out
