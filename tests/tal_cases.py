"""Seeded inputs of the task-aligned loss tests: tests/test_tal_gpu.py runs every case through
csrc/tal_loss.hip against tests/tal_ref.py, and tests/test_tal_cpu.py checks for every case that
the restatement's assignment margins are far above fp32 rounding (or that the case is an exact tie
built on purpose), so the fp32 kernels must reproduce the assignment exactly.

A case is a dict: maps (fp32 CPU [B, 64 + nc, H, W] per level), targets [M, 6], nc, img (h, w),
strides, topk, alpha, beta, dtype (the maps are rounded to it before either side sees them),
exact_ties (margins are zero by construction)."""
import torch

STRIDES = (8.0, 16.0, 32.0)


def maps(B, nc, shapes, seed, scale=1.0):
    """Random head maps whose DFL logits favour bins 1..3: predicted boxes of ~2 strides per side,
    the size range of the GTs, so that most inside pairs have a positive CIoU."""
    g = torch.Generator().manual_seed(seed)
    out = [torch.randn(B, 64 + nc, h, w, generator=g) * scale for h, w in shapes]
    for m in out:
        for side in range(4):
            m[:, side * 16 + 1:side * 16 + 4] += 3.0
    return out


def rand_targets(B, nc, n_per_img, seed, extra=()):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(B):
        for _ in range(n_per_img[b] if isinstance(n_per_img, (list, tuple)) else n_per_img):
            wh = torch.rand(2, generator=g) * 0.4 + 0.05
            c = torch.rand(2, generator=g) * (1 - wh) + wh / 2
            rows.append([b, int(torch.randint(0, nc, (1,), generator=g)), float(c[0]), float(c[1]), float(wh[0]),
                         float(wh[1])])
    rows += [list(r) for r in extra]
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 6)


def case(maps_, targets, nc, img, strides=STRIDES, topk=10, alpha=0.5, beta=6.0, dtype=torch.float32,
         exact_ties=False):
    return dict(maps=maps_, targets=targets, nc=nc, img=img, strides=tuple(strides[:len(maps_)]), topk=topk,
                alpha=alpha, beta=beta, dtype=dtype, exact_ties=exact_ties)


# ---- the third-GT construction -------------------------------------------------------------------
# Level 0 of a 64 x 96 image (8 x 12 anchors, stride 8), image THIRD_IMG.  E = [8, 56]^2 px holds the 36
# centres gx, gy in 1..6.  Every level-0 anchor of the image predicts a ~32 px box (one-hot DFL bin 2
# plus noise), so dozens of E's candidates have overlap ~0.4 and metric ~1e-3; the anchor STAR =
# (gx 3, gy 3), centre (28, 28), predicts E itself (two-hot bins 2|3 left/top, 3|4 right/bottom) but
# its class-THIRD_CLS logit is -40 (metric ~2e-9), so E's top-10 rejects it.  Two small GTs S1, S2 of
# other classes contain only STAR's centre and claim it; the contested anchor goes to the largest
# overlap among ALL GTs it lies inside: E.
THIRD_IMG, THIRD_CLS = 2, 4
STAR = 3 * 12 + 3
THIRD_ROWS = [[THIRD_IMG, THIRD_CLS, 32 / 96, 32 / 64, 48 / 96, 48 / 64],       # E
              [THIRD_IMG, 0, 29 / 96, 28 / 64, 10 / 96, 10 / 64],              # S1
              [THIRD_IMG, 1, 28 / 96, 29 / 64, 10 / 96, 12 / 64]]              # S2


def third_gt_maps(B, nc, seed):
    m = maps(B, nc, [(8, 12), (4, 6), (2, 3)], seed, scale=2.0)
    g = torch.Generator().manual_seed(seed + 1000)
    l0 = m[0][THIRD_IMG]
    l0[:64] = torch.randn(64, 8, 12, generator=g) * 0.5
    for side in range(4):
        l0[side * 16 + 2] += 6.0
    star = l0[:, 3, 3]
    star[:64] = 0.0
    for side, lo in enumerate((2, 2, 3, 3)):
        star[side * 16 + lo] = 12.0
        star[side * 16 + lo + 1] = 12.0
    star[64 + THIRD_CLS] = -40.0
    star[64 + 0] = 3.0
    star[64 + 1] = 3.0
    return m


def composite(seed_maps=21, seed_targets=22):
    """B = 3, nc = 5: image 0 with a GT that contains no anchor centre, two classes sharing anchors and
    a GT with fewer than 10 inside anchors; image 1 empty; image 2 the third-GT construction; rows
    that must be ignored (image -1, image >= B, class >= nc, class < 0)."""
    B, nc = 3, 5
    extra = [[0, 2, 0.5, 0.5, 2 / 96, 2 / 64],                    # between centres: no candidate
             [0, 4, 0.5, 0.5, 0.5, 0.5], [0, 1, 0.52, 0.5, 0.5, 0.5],   # two classes, shared anchors
             [0, 3, 0.2, 0.25, 20 / 96, 20 / 64],                 # #inside < 10
             [-1, 1, 0.5, 0.5, 0.6, 0.6], [3, 1, 0.5, 0.5, 0.6, 0.6], [0, 5, 0.5, 0.5, 0.6, 0.6],
             [1, -1, 0.5, 0.5, 0.6, 0.6]] + THIRD_ROWS
    tg = rand_targets(B, nc, [2, 0, 0], seed_targets, extra)
    return case(third_gt_maps(B, nc, seed_maps), tg, nc, (64, 96))


def _small(nc, seed, **kw):
    return case(maps(2, nc, [(8, 8), (4, 4), (2, 2)], seed, scale=1.5), rand_targets(2, nc, 4, seed + 1), nc,
                (64, 64), **kw)


def _many_rows(seed, n_pad):
    """Thousands of target rows: 30 real GTs among rows that contain no anchor centre or are ignored."""
    B, nc = 3, 6
    real = rand_targets(B, nc, 10, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    pad = torch.zeros(n_pad, 6)
    pad[:, 0] = torch.randint(-1, B + 1, (n_pad,), generator=g).float()
    pad[:, 1] = torch.randint(0, nc, (n_pad,), generator=g).float()
    # 1 px boxes centred on multiples of 16 px: anchor centres are 4 + 8 i (stride 8) and 8 + 16 i (16)
    pad[:, 2] = torch.randint(1, 4, (n_pad,), generator=g).float() * 16 / 64
    pad[:, 3] = torch.randint(1, 4, (n_pad,), generator=g).float() * 16 / 64
    pad[:, 4:] = 1 / 64
    tg = torch.cat([pad[:n_pad // 2], real, pad[n_pad // 2:]])
    return case(maps(B, nc, [(8, 8), (4, 4)], seed, scale=1.5), tg, nc, (64, 64))


def _zero_metric_ties(seed):
    """Every predicted box is (nearly) a point at its anchor centre and no GT centre is an anchor
    centre: CIoU < 0, overlap and metric exactly 0 for every pair; the top-k falls to the anchor index."""
    B, nc = 2, 3
    m = maps(B, nc, [(8, 8), (4, 4)], seed)
    for l in m:
        l[:, :64] = 0.0
        for side in range(4):
            l[:, side * 16] = 30.0
    tg = torch.tensor([[0, 1, 0.47, 0.53, 0.6, 0.5], [0, 2, 0.4, 0.45, 0.5, 0.7], [1, 0, 0.55, 0.52, 0.7, 0.3]])
    return case(m, tg, nc, (64, 64), exact_ties=True)


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
    "alpha1_beta2_topk3": lambda: _small(5, 59, topk=3, alpha=1.0, beta=2.0),
    "bf16": lambda: case(maps(2, 80, [(16, 16), (8, 8), (4, 4)], 61, 1.5), rand_targets(2, 80, 6, 62), 80, (128, 128),
                         dtype=torch.bfloat16),
    "f16": lambda: case(maps(2, 80, [(16, 16), (8, 8), (4, 4)], 63, 1.5), rand_targets(2, 80, 6, 64), 80, (128, 128),
                        dtype=torch.float16),
    "rows300": lambda: _many_rows(71, 270),
    "rows5000": lambda: _many_rows(73, 4970),
    "zero_metric_ties": lambda: _zero_metric_ties(75),
    "full640": full640,
}


_REF = {}


def reference(name):
    """tal_ref on case `name` (maps rounded to the case's dtype, fp64 arithmetic), computed once per
    process and shared: -> (case, result dict with detached values, [d total / d map] per level)."""
    if name not in _REF:
        import tal_ref
        c = CASES[name]()
        ins = [m.to(c["dtype"]).double().requires_grad_(True) for m in c["maps"]]
        r = tal_ref.tal_loss(ins, c["targets"], c["nc"], c["img"], c["strides"], c["topk"], c["alpha"], c["beta"])
        r["total"].backward()
        r = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in r.items()}
        _REF[name] = (c, r, [i.grad for i in ins])
    return _REF[name]
