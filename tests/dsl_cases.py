"""Seeded inputs of the dynamic soft-label loss tests: tests/test_dsl_gpu.py runs every case through
csrc/dsl_loss.hip against tests/dsl_ref.py, and tests/test_dsl_cpu.py checks for every case that the
restatement's decision margins are far above fp32 rounding (or that the case is an exact tie built on
purpose), so the fp32 kernels must reproduce the assignment and every dynamic k exactly.

A case is a dict: maps (fp32 CPU [B, 64 + nc, H, W] per level), targets [M, 6], nc, img (h, w),
strides, topk, radius, iou_weight, beta, gains, dtype (the maps are rounded to it before either side
sees them), exact_ties (some margins are zero by construction)."""
import torch

from tal_cases import STRIDES, maps, rand_targets


def case(maps_, targets, nc, img, strides=STRIDES, topk=13, radius=3.0, iou_weight=3.0, beta=2.0,
         gains=(2.0, 1.0, 0.0), dtype=torch.float32, exact_ties=False):
    return dict(maps=maps_, targets=targets, nc=nc, img=img, strides=tuple(strides[:len(maps_)]), topk=topk,
                radius=radius, iou_weight=iou_weight, beta=beta, gains=tuple(gains), dtype=dtype,
                exact_ties=exact_ties)


# ---- the unselecting-winner construction ---------------------------------------------------------
# Image WIN_IMG of a 64 x 96 image, levels (8,12) (4,6) (2,3).  Every anchor of the image predicts a
# box of a few pixels (one-hot DFL bin 0 plus noise) and has class logits -6, except:
#   STAR = level 0 (gx 3, gy 3), centre (28, 28): predicts E = (8, 8, 56, 56) itself (two-hot bins 2|3
#     left/top, 3|4 right/bottom); logits: class WIN_CLS -5, classes 0 and 1 -3;
#   Q0..Q3 = the level-1 anchors with centres (24|40, 24|40): each predicts two thirds of E (one-hot
#     bins: 1 towards the near sides, 1 and 2 towards the far ones), IoU 2/3; class WIN_CLS logits
#     4, 3.5, 3, 2.5 (distinct costs), classes 0 and 1 -4.
# GTs: E (class WIN_CLS), S1 (class 0, 10 x 10 px) and S2 (class 1, 10 x 12 px), which contain only
# STAR's centre.  E: IoU sum 1 + 4 * 2/3 + ~0 = 3.67 -> k = 3; its three cheapest candidates are Qs
# (box cost -3 log(2/3) = 1.2) and not STAR (class cost BCE(-5, 1) = 5).  S1, S2: IoU sum < 1 -> k = 1,
# and STAR is their cheapest candidate (IoU 0.043 / 0.052 -> 9.4 / 8.9; a Q costs them its IoU 0.065 /
# 0.078 -> 8.2 / 7.7 plus the background term of its class-WIN_CLS logit >= 2.2; every other anchor has
# IoU ~ 0 -> 48).  STAR is contested between S1 and S2 and goes to the lowest cost among ALL GTs: E (5.0),
# which had not selected it.
WIN_IMG, WIN_CLS = 2, 4
STAR = 3 * 12 + 3
# level-1 (gy, gx) -> one-hot bins (left, top, right, bottom) of 16 px from the centre (8 + 16 gx, 8 + 16 gy):
# boxes (8,8,40,56), (8,8,56,40), (8,24,56,56), (24,8,56,56)
Q_BINS = {(1, 1): (1, 1, 1, 2), (1, 2): (2, 1, 1, 1), (2, 1): (1, 1, 2, 1), (2, 2): (1, 2, 1, 1)}
WIN_ROWS = [[WIN_IMG, WIN_CLS, 32 / 96, 32 / 64, 48 / 96, 48 / 64],       # E
            [WIN_IMG, 0, 29 / 96, 28 / 64, 10 / 96, 10 / 64],            # S1
            [WIN_IMG, 1, 28 / 96, 29 / 64, 10 / 96, 12 / 64]]            # S2


def winner_maps(B, nc, seed):
    m = maps(B, nc, [(8, 12), (4, 6), (2, 3)], seed, scale=2.0)
    g = torch.Generator().manual_seed(seed + 1000)
    for lv in m:
        x = lv[WIN_IMG]
        x[:64] = torch.randn(x[:64].shape, generator=g) * 0.5
        for side in range(4):
            x[side * 16] += 8.0
        x[64:] = -6.0 + torch.randn(x[64:].shape, generator=g) * 0.1
    star = m[0][WIN_IMG][:, 3, 3]
    star[:64] = 0.0
    for side, lo in enumerate((2, 2, 3, 3)):
        star[side * 16 + lo] = 12.0
        star[side * 16 + lo + 1] = 12.0
    star[64 + WIN_CLS] = -5.0
    star[64 + 0] = -3.0
    star[64 + 1] = -3.0
    for ((gy, gx), bins), logit in zip(Q_BINS.items(), (4.0, 3.5, 3.0, 2.5)):
        a = m[1][WIN_IMG][:, gy, gx]
        a[:64] = 0.0
        for side, b_ in enumerate(bins):
            a[side * 16 + b_] = 30.0
        a[64:] = -6.0
        a[64 + WIN_CLS] = logit
        a[64 + 0] = -4.0
        a[64 + 1] = -4.0
    return m


def composite(seed_maps=21, seed_targets=22):
    """B = 3, nc = 5: image 0 with a GT that contains no anchor centre (and still gets its k = 1 anchor),
    two classes sharing anchors and a small GT; image 1 empty; image 2 the unselecting-winner
    construction; rows that must be ignored (image -1, image >= B, class >= nc, class < 0)."""
    B, nc = 3, 5
    extra = [[0, 2, 0.5, 0.5, 2 / 96, 2 / 64],                    # between centres: contains none
             [0, 4, 0.5, 0.5, 0.5, 0.5], [0, 1, 0.52, 0.5, 0.5, 0.5],   # two classes, shared anchors
             [0, 3, 0.2, 0.25, 20 / 96, 20 / 64],
             [-1, 1, 0.5, 0.5, 0.6, 0.6], [3, 1, 0.5, 0.5, 0.6, 0.6], [0, 5, 0.5, 0.5, 0.6, 0.6],
             [1, -1, 0.5, 0.5, 0.6, 0.6]] + WIN_ROWS
    tg = rand_targets(B, nc, [2, 0, 0], seed_targets, extra)
    return case(winner_maps(B, nc, seed_maps), tg, nc, (64, 96))


N_RAND = 2              # composite: random rows before the extras
CENTRELESS_ROW = N_RAND


def _small(nc, seed, **kw):
    return case(maps(2, nc, [(8, 8), (4, 4), (2, 2)], seed, scale=1.5), rand_targets(2, nc, 4, seed + 1), nc,
                (64, 64), **kw)


def _many_rows(seed, n_pad):
    """Hundreds / thousands of target rows: 30 real GTs among ignored padding rows (image -1 or >= B; a
    valid 1 px row would select its k = 1 anchor and identical padding rows would tie exactly)."""
    B, nc = 3, 6
    real = rand_targets(B, nc, 10, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    pad = torch.zeros(n_pad, 6)
    pad[:, 0] = torch.randint(0, 2, (n_pad,), generator=g).float() * (B + 1) - 1         # -1 or B
    pad[:, 1] = torch.randint(0, nc, (n_pad,), generator=g).float()
    pad[:, 2] = torch.randint(1, 4, (n_pad,), generator=g).float() * 16 / 64
    pad[:, 3] = torch.randint(1, 4, (n_pad,), generator=g).float() * 16 / 64
    pad[:, 4:] = 1 / 64
    tg = torch.cat([pad[:n_pad // 2], real, pad[n_pad // 2:]])
    return case(maps(B, nc, [(8, 8), (4, 4)], seed, scale=1.5), tg, nc, (64, 64))


def prior_ties():
    """One level, image (64, 400), 8 x 50 anchors of stride 8.  A real GT at the left, (20, 8, 100, 56),
    holds every candidate (x <= 92).  A 1 px GT at x = 384 (between the centres 380 and 388) is more than
    33 strides from all of them: exponent capped at 30, prior 1e30, which absorbs the other terms in
    fp32 and fp64 alike: its costs all tie exactly, its IoUs are 0 (k = 1), and it takes the lowest-index
    candidate, (gx 3, gy 1)."""
    m = maps(1, 3, [(8, 50)], 81, scale=1.5)
    tg = torch.tensor([[0, 1, 60 / 400, 32 / 64, 80 / 400, 48 / 64], [0, 2, 384 / 400, 32 / 64, 1 / 400, 1 / 64]])
    return case(m, tg, 3, (64, 400), strides=(8.0,), exact_ties=True)


PRIOR_TIES_PICK = 1 * 50 + 3


def full640(seed=31):
    return case(maps(2, 80, [(80, 80), (40, 40), (20, 20)], seed, scale=3.0), rand_targets(2, 80, 8, seed + 1), 80,
                (640, 640))


def _composite_m(n):
    c = composite()
    c["targets"] = c["targets"][:n]
    return c


CASES = {
    "composite": composite,
    "m0": lambda: _composite_m(0),
    "m1": lambda: _composite_m(1),
    "nc1": lambda: _small(1, 41),
    "nc7_ld72": lambda: _small(7, 43),
    "nc33": lambda: _small(33, 45),
    "nc80": lambda: _small(80, 47),
    "level1": lambda: case(maps(2, 4, [(8, 8)], 51, 1.5), rand_targets(2, 4, 4, 52), 4, (64, 64)),
    "level4": lambda: case(maps(2, 4, [(16, 16), (8, 8), (4, 4), (2, 2)], 53, 1.5), rand_targets(2, 4, 5, 54), 4,
                           (128, 128), strides=(8.0, 16.0, 32.0, 64.0)),
    "anchors5": lambda: case(maps(2, 3, [(1, 5)], 55, 1.5), rand_targets(2, 3, 3, 56), 3, (32, 160), strides=(32.0,)),
    "topk1": lambda: _small(5, 57, topk=1),
    "r1_w1_beta1": lambda: _small(5, 59, radius=1.0, iou_weight=1.0, beta=1.0),
    "beta3": lambda: _small(5, 65, beta=3.0),
    "dfl_gain": lambda: _small(5, 67, gains=(2.0, 1.0, 1.5)),
    "bf16": lambda: case(maps(2, 80, [(16, 16), (8, 8), (4, 4)], 61, 1.5), rand_targets(2, 80, 6, 62), 80, (128, 128),
                         dtype=torch.bfloat16),
    "f16": lambda: case(maps(2, 80, [(16, 16), (8, 8), (4, 4)], 63, 1.5), rand_targets(2, 80, 6, 64), 80, (128, 128),
                        dtype=torch.float16),
    "rows300": lambda: _many_rows(77, 270),
    "rows5000": lambda: _many_rows(73, 4970),
    "prior_ties": prior_ties,
    "full640": full640,
}


_REF = {}


def reference(name):
    """dsl_ref on case `name` (maps rounded to the case's dtype, fp64 arithmetic), computed once per
    process and shared: -> (case, result dict with detached values, [d total / d map] per level)."""
    if name not in _REF:
        import dsl_ref
        c = CASES[name]()
        ins = [m.to(c["dtype"]).double().requires_grad_(True) for m in c["maps"]]
        r = dsl_ref.dsl_loss(ins, c["targets"], c["nc"], c["img"], c["strides"], c["topk"], c["radius"],
                             c["iou_weight"], c["beta"], c["gains"])
        r["total"].backward()
        r = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in r.items()}
        _REF[name] = (c, r, [i.grad for i in ins])
    return _REF[name]
