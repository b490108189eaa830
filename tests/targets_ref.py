"""yms_box_targets (csrc/targets.hip) restated: Python floats are IEEE doubles and Python never fuses
a multiply with an add, so every line below is the kernel's operation, in the kernel's order, and
the float32 rounding of the result is the kernel's store.  Input: the tables of
yms.cache.target_tables and the annotation table; output: the padded float32 [m_cap, 6] array --
(image, class, cx, cy, w, h) for a surviving box, (-1, 0, 0, 0, 0, 0) for any other row."""
import math

import numpy as np

MIN_VISIBILITY, MIN_AREA = 0.1, 1.0
IGNORED = (-1.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def _div(a, b):
    """IEEE a / b (Python raises on a zero divisor)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _min(a, b):
    return b if b < a else a


def _max(a, b):
    return b if b > a else a


def envelope(stages, bx0, by0, bx1, by1):
    """(x0, y0, x1, y1) of the box's corners after the forward stage matrices (each 9 floats)."""
    e = None
    for cx, cy in ((bx0, by0), (bx1, by0), (bx1, by1), (bx0, by1)):
        X, Y = cx - 0.5, cy - 0.5
        for F in stages:
            q0 = (F[0] * X + F[1] * Y) + F[2]
            q1 = (F[3] * X + F[4] * Y) + F[5]
            q2 = (F[6] * X + F[7] * Y) + F[8]
            X, Y = _div(q0, q2), _div(q1, q2)
        X, Y = X + 0.5, Y + 0.5
        e = [X, Y, X, Y] if e is None else [_min(e[0], X), _min(e[1], Y), _max(e[2], X), _max(e[3], Y)]
    return e


def box_row(box, label, image, clip, gx, gy, ox, oy, rect, stages, out_w, out_h):
    """One candidate's row (six Python floats, before the float32 store)."""
    x, y, w, h = (float(v) for v in box)
    u = (ox + x * gx, oy + y * gy, ox + (x + w) * gx, oy + (y + h) * gy)
    k = u
    if clip:
        k = (_max(u[0], rect[0]), _max(u[1], rect[1]), _min(u[2], rect[2]), _min(u[3], rect[3]))
        if k[2] <= k[0] or k[3] <= k[1]:
            return IGNORED
    eu = envelope(stages, *u)
    ek = envelope(stages, *k) if clip else eu
    W, H = float(out_w), float(out_h)
    area = (eu[2] - eu[0]) * (eu[3] - eu[1])
    cx0, cy0 = _min(_max(ek[0], 0.0), W), _min(_max(ek[1], 0.0), H)
    cx1, cy1 = _min(_max(ek[2], 0.0), W), _min(_max(ek[3], 0.0), H)
    carea = _max(cx1 - cx0, 0.0) * _max(cy1 - cy0, 0.0)
    if area <= 0.0 or _div(carea, area) < MIN_VISIBILITY or carea < MIN_AREA:
        return IGNORED
    bw, bh = cx1 - cx0, cy1 - cy0
    cxn, cyn, wn, hn = (cx0 + bw / 2.0) / W, (cy0 + bh / 2.0) / H, bw / W, bh / H
    if wn > 1e-3 and hn > 1e-3 and 0.0 <= cxn <= 1.0 and 0.0 <= cyn <= 1.0 and 0.0 <= wn <= 1.0 and 0.0 <= hn <= 1.0:
        return (float(image), float(label), cxn, cyn, wn, hn)
    return IGNORED


def box_targets(tiles, layers, m_cap, boxes, labels):
    out = np.empty((m_cap, 6), np.float32)
    out[:] = IGNORED
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    for t in tiles:
        ly = layers[int(t["layer"])]
        stages = [[float(v) for v in ly["m"][s]] for s in range(int(ly["nst"]))]
        rect = [float(v) for v in t["rect"]]
        for k in range(int(t["count"])):
            a = int(t["ann0"]) + k
            out[int(t["out0"]) + k] = box_row(boxes[a], int(labels[a]), int(t["image"]), int(t["clip"]),
                                              float(t["gx"]), float(t["gy"]), float(t["ox"]), float(t["oy"]), rect,
                                              stages, int(ly["out_w"]), int(ly["out_h"]))
    return out


def compact(rows):
    return rows[rows[:, 0] >= 0]
