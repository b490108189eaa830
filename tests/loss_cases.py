"""Inputs for the detection-loss edge tests, built and qualified with the fp64 oracle alone
(oracle/loss_ref.py).  Nothing here touches the GPU path: tests/test_loss_cases_cpu.py asserts, on
the CPU, that every case has the property it was built for, and tests/test_loss_edges_gpu.py runs
the same inputs through csrc/det_loss.hip.

A case is a dict: ``maps`` (list of fp32 [B, 64 + nc, H, W] CPU tensors), ``targets`` ([M, 6] fp32
rows image, class, cx, cy, w, h normalised), ``nc``, ``img`` (h, w), ``strides``.
"""
import functools

import torch

from oracle import loss_ref as R

DFL = 16


# ----------------------------------------------------------------------------------------------
# oracle views of a case
def rounded(maps, dtype):
    """The maps as the kernel sees them (rounded to ``dtype``), in fp64."""
    return [m.to(dtype).double() for m in maps]


def _flat(maps):
    B = maps[0].shape[0]
    return torch.cat([m.reshape(B, m.shape[1], -1).permute(0, 2, 1) for m in maps], 1)


def decoded(maps, strides):
    """-> (decoded boxes [B, A, 4], anchor centres [A, 2], anchor strides [A]) in the maps' dtype."""
    dt = maps[0].dtype
    anc, st = R.anchors([(m.shape[2], m.shape[3]) for m in maps], strides, dt)
    dist = _flat(maps)[..., :4 * DFL]
    return torch.stack([R.decode(d, anc) for d in dist]), anc, st


def image_rows(targets, b):
    """Indices of image b's rows, in target order (the oracle's float ``==`` match)."""
    return torch.nonzero(targets[:, 0] == b).flatten()


def gt_boxes(targets, rows, img, dt):
    """Pixel (cx, cy, w, h) of the given rows, scaled as the oracle's forward scales them."""
    g = targets[rows, 2:].clone().to(dt)
    g[:, 0::2] *= img[1]
    g[:, 1::2] *= img[0]
    return g


def row_ious(maps, targets, img, strides):
    """{row index: IoU of every anchor with that row's GT} for the rows of images 0..B-1."""
    dt = maps[0].dtype
    pb, _, _ = decoded(maps, strides)
    out = {}
    for b in range(maps[0].shape[0]):
        rows = image_rows(targets, b)
        if rows.numel() == 0:
            continue
        iou = R.bbox_iou(pb[b].unsqueeze(1), gt_boxes(targets, rows, img, dt).unsqueeze(0), xywh=True)
        for c, j in enumerate(rows.tolist()):
            out[j] = iou[:, c]
    return out


def chosen_sets(maps, targets, img, strides):
    """{row index: sorted anchors the assigner picks for it} (ties -> lower anchor index)."""
    out = {}
    for j, col in row_ious(maps, targets, img, strides).items():
        k = min(R.TOPK, int((col > R.IOU_MIN).sum()))
        out[j] = sorted(R._topk_lower_index(col, k)) if k else []
    return out


def assignment(maps, targets, nc, img, strides):
    """Per image: (fg [A] bool, DFL side targets in stride units [A, 4], class targets [A, nc])."""
    dt = maps[0].dtype
    pb, anc, st = decoded(maps, strides)
    out = []
    for b in range(maps[0].shape[0]):
        rows = image_rows(targets, b)
        _, ts, fg, tl = R.assign(pb[b], gt_boxes(targets, rows, img, dt), targets[rows, 1], anc, nc)
        out.append((fg, tl / st.unsqueeze(1), ts))
    return out


# det_loss's lambdas (box, cls, dfl) that isolate each term, and the oracle's name of it
TERMS = {"total": (R.LAMBDA_BOX, R.LAMBDA_CLS, R.LAMBDA_DFL), "loss_box": (1.0, 0.0, 0.0),
         "loss_cls": (0.0, 1.0, 0.0), "loss_dfl": (0.0, 0.0, 1.0)}


def reference(case, dtype, iou_type="ciou", pos_weight=None):
    """fp64 oracle on the dtype-rounded maps -> {"values": {term: float}, "grads": {term: [d term /
    d map per level]}, "fg": [B, A] bool}: one forward, one backward per term."""
    maps = [m.requires_grad_(True) for m in rounded(case["maps"], dtype)]
    tg = case["targets"].double()
    pw = None if pos_weight is None else torch.as_tensor(pos_weight, dtype=torch.float64)
    total, items = R.compute_loss(maps, tg, case["nc"], case["img"], case["strides"], iou_type=iou_type,
                                  pos_weight=pw)
    terms = dict(items, total=total)
    grads = {}
    for name, t in terms.items():
        if t.requires_grad:
            g = torch.autograd.grad(t, maps, retain_graph=True, allow_unused=True)
            grads[name] = [torch.zeros_like(m) if x is None else x for x, m in zip(g, maps)]
        else:                                    # no foreground anywhere: the term is the constant 0
            grads[name] = [torch.zeros_like(m) for m in maps]
    with torch.no_grad():
        fg = torch.stack([a[0] for a in assignment([m.detach() for m in maps], tg, case["nc"], case["img"],
                                                   case["strides"])])
    return {"values": {k: float(v.detach()) for k, v in terms.items()}, "grads": grads, "fg": fg}


# ----------------------------------------------------------------------------------------------
def prune_ambiguous(preds, targets, img, strides, margin=1e-4):
    """Drop the target rows whose assignment sits within ``margin`` (in IoU) of flipping.

    The kernel ranks IoUs in fp32, the oracle in fp64; a row whose top-k set depends on the last bits
    of an IoU is no test of the kernel.  ``preds`` are the dtype-rounded maps in fp64.  Per row, with
    n = #(IoU > 0.1): n <= 10 -> distance min |IoU - 0.1| over the anchors (the set is "all above the
    threshold"); n > 10 -> IoU[10th] - IoU[11th] (order inside the set does not matter).  Decoded
    boxes do not depend on the targets, so dropping a row changes nothing for the others.  Rows of
    no image of the batch are never assigned and are kept.  -> (kept rows, number dropped)."""
    keep = torch.ones(targets.shape[0], dtype=torch.bool)
    for j, col in row_ious(preds, targets.double(), img, strides).items():
        n = int((col > R.IOU_MIN).sum())
        if n <= R.TOPK:
            d = (col - R.IOU_MIN).abs().min().item()
        else:
            s = torch.sort(col, descending=True).values
            d = (s[R.TOPK - 1] - s[R.TOPK]).item()
        keep[j] = d >= margin
    return targets[keep], int((~keep).sum())


def grad_blocks(g, dfl_lanes=4 * DFL):
    """One level's gradient [B, 64 + nc, H, W] -> (DFL lanes [B, 64 * H * W], class lanes
    [B, nc * H * W]): row b of each is one (image, level) block."""
    B = g.shape[0]
    return g[:, :dfl_lanes].reshape(B, -1), g[:, dfl_lanes:].reshape(B, -1)


# ----------------------------------------------------------------------------------------------
# cases
def random_maps(B, nc, shapes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 4 * DFL + nc, h, w, generator=g) * scale for h, w in shapes]


def random_rows(n, B, nc, seed, wh_lo=0.05, wh_span=0.4):
    """n rows with random image ids (rows of different images interleave), classes and boxes."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, B, (n,), generator=g).float()
    cls = torch.randint(0, nc, (n,), generator=g).float()
    wh = torch.rand(n, 2, generator=g) * wh_span + wh_lo
    c = torch.rand(n, 2, generator=g) * (1 - wh) + wh / 2
    return torch.cat([ids[:, None], cls[:, None], c, wh], 1)


def _case(maps, targets, nc, img, strides):
    return {"maps": maps, "targets": targets, "nc": nc, "img": img, "strides": tuple(float(s) for s in strides)}


def pruned(case, dtype):
    """The case with its ambiguous rows (for maps rounded to ``dtype``) dropped -> (case, dropped)."""
    kept, dropped = prune_ambiguous(rounded(case["maps"], dtype), case["targets"], case["img"], case["strides"])
    return dict(case, targets=kept), dropped


@functools.lru_cache(maxsize=None)
def many_case(n):
    """B = 3, 126 anchors, n random rows: n = 300 needs two staging rounds of assign_kernel's
    256-row compaction, n = 4300 is past its 4096-row LDS list (the unstaged scan)."""
    B, nc = 3, 5
    return _case(random_maps(B, nc, [(8, 12), (4, 6), (2, 3)], 1, scale=2.0), random_rows(n, B, nc, 100 + n),
                 nc, (64, 96), (8.0, 16.0, 32.0))


@functools.lru_cache(maxsize=None)
def many_pruned(n, dtype):
    return pruned(many_case(n), dtype)


def swap_case():
    """Three images, a few GTs each; image 0's LAST two rows are two classes on overlapping boxes,
    so they share anchors and no later GT overwrites them: swapping the two changes the result."""
    B, nc = 3, 5
    rows = random_rows(9, B, nc, 21)
    rows = torch.cat([rows, torch.tensor([[0, 4, 0.5, 0.5, 0.5, 0.5], [0, 1, 0.52, 0.5, 0.5, 0.5]])])
    return _case(random_maps(B, nc, [(8, 12), (4, 6), (2, 3)], 1, scale=2.0), rows, nc, (64, 96),
                 (8.0, 16.0, 32.0))


def tie_case(scale=1):
    """Exact arithmetic: every DFL logit 0 -> every side expectation exactly 7.5 in fp32 and fp64,
    every predicted box 15 x 15 px with edges on x.5; GTs with power-of-two normalised coordinates
    -> integer pixel edges (never equal to a predicted edge).  Anchors at the same offset from a GT
    then have bit-equal IoUs, in one level and across levels.  ``scale`` 1: 64 x 64 image, 84 anchors
    (one per top-k thread, two waves); 2: 128 x 128, 336 anchors (top-k threads holding two anchors),
    with a fourth GT (14..22 x 12..40 px) whose rank 10 / 11 tie is between anchors 17 and 273 =
    17 + 256, the two anchors of ONE top-k thread."""
    nc, s = 3, 64 * scale
    maps = random_maps(1, nc, [(s // 8, s // 8), (s // 16, s // 16), (s // 32, s // 32)], 31)
    for m in maps:
        m[:, :4 * DFL] = 0.0
    t = [[0, 0, 0.25, 0.25, 0.25, 0.25], [0, 1, 0.5, 0.5, 0.5, 0.5], [0, 2, 0.75, 0.5, 0.125, 0.25]]
    if scale == 2:
        t.append([0, 1, 18 / 128, 26 / 128, 8 / 128, 28 / 128])
    return _case(maps, torch.tensor(t), nc, (s, s), (8.0, 16.0, 32.0))


def tied_at_cut(col):
    """Anchors tied with the 10th-ranked IoU of ``col`` -> (chosen ones, left-out ones); both
    non-empty means a tied group straddles the top-k cut."""
    n = int((col > R.IOU_MIN).sum())
    if n <= R.TOPK:
        return [], []
    order = R._topk_lower_index(col, col.numel())
    cut = col[order[R.TOPK - 1]]
    tied = [a for a in order if col[a] == cut]
    return [a for a in tied if a in order[:R.TOPK]], [a for a in tied if a not in order[:R.TOPK]]


def dfl_edge_case():
    """Foreground anchors whose DFL side targets hit box_dfl's bin edges: below 0 (anchor centres
    outside a 6 x 6 px GT that their predictions still cover), at or above 15 (a 170 x 20 px GT in a
    192 px wide image; image 0's DFL logits carry a +0.5 * bin ramp so its predictions are ~27 px
    and clear IoU 0.1), exactly integer (a GT with power-of-two coordinates: edges at 12 / 36 px)."""
    B, nc, img = 2, 4, (64, 192)
    maps = random_maps(B, nc, [(8, 24), (4, 12), (2, 6)], 44)    # a seed with every row >= 1e-3 from flipping
    ramp = (0.5 * torch.arange(DFL, dtype=torch.float32)).repeat(4)
    for m in maps:
        m[1, :4 * DFL] *= 0.4
        m[0, :4 * DFL] += ramp[:, None, None]
    t = torch.tensor([[0, 1, 96 / 192, 0.5, 170 / 192, 20 / 64],
                      [1, 2, 40 / 192, 24 / 64, 6 / 192, 6 / 64],
                      [1, 0, 0.125, 0.5, 0.125, 0.25],
                      [0, 3, 0.25, 0.25, 0.0625, 0.25]])
    return _case(maps, t, nc, img, (8.0, 16.0, 32.0))


def dfl_side_conditions(case, dtype):
    """-> (#side targets < 0, #side targets >= 15, #exactly integer side targets) over the oracle's
    foreground anchors."""
    neg = hi = integer = 0
    for fg, t, _ in assignment(rounded(case["maps"], dtype), case["targets"].double(), case["nc"], case["img"],
                               case["strides"]):
        s = t[fg]
        neg += int((s < 0).sum())
        hi += int((s >= DFL - 1).sum())
        integer += int((s == s.floor()).sum())
    return neg, hi, integer


def batch_case(B):
    """More images than flags_kernel's 64 per block (65) and finalize_kernel's 256 threads (260);
    five anchors in all, so k < 10 because there are fewer than ten anchors; ~1.5 rows per image with
    random image ids, so a fifth of the images have no GT."""
    nc = 3
    rows = random_rows(B * 20 // 13, B, nc, 51 + B, wh_lo=0.4, wh_span=0.5)
    return _case(random_maps(B, nc, [(2, 2), (1, 1)], 52), rows, nc, (16, 16), (8.0, 16.0))


def levels_case(nl):
    B, nc = 2, 5
    if nl == 1:
        return _case(random_maps(B, nc, [(2, 3)], 61), random_rows(6, B, nc, 62, wh_lo=0.3, wh_span=0.5), nc,
                     (16, 24), (8.0,))
    assert nl == 4
    return _case(random_maps(B, nc, [(8, 8), (4, 4), (2, 2), (1, 1)], 63), random_rows(10, B, nc, 64), nc, (64, 64),
                 (8.0, 16.0, 32.0, 64.0))


def classes_case(nc):
    """nc = 1; nc = 33: one box carrying classes 2 and 32 (two class words, the last 8-chunk one
    class wide); nc = 80: classes 31 / 32 / 79 on one box (shared anchors, both class words)."""
    B = 2
    rows = random_rows(5, B, nc, 70 + nc)
    labs = {1: [0], 33: [2, 32], 80: [31, 32, 79]}[nc]
    rows = torch.cat([rows, torch.tensor([[1, c, 0.5, 0.5, 0.4, 0.5] for c in labs], dtype=torch.float32)])
    return _case(random_maps(B, nc, [(8, 8), (4, 4), (2, 2)], 71), rows, nc, (64, 64), (8.0, 16.0, 32.0))


def saturated_case():
    """Class logits of +-50 and DFL sides with one bin raised by 40 (a one-hot softmax).  About half
    of the sides are saturated and at least one side of every anchor is not: a saturated side's box
    gradient is ~e^-40 in any arithmetic (fp32 cannot resolve bin - expectation there), so an anchor
    or a block made of such sides alone would compare rounding noise."""
    B, nc = 2, 5
    maps = random_maps(B, nc, [(8, 8), (4, 4), (2, 2)], 81)
    g = torch.Generator().manual_seed(82)
    for m in maps:
        _, _, h, w = m.shape
        sign = torch.randint(0, 2, (B, nc, h, w), generator=g).float() * 2 - 1
        m[:, 4 * DFL:] = 50.0 * sign
        hot = torch.randint(0, DFL, (B, 4, 1, h, w), generator=g)
        sat = torch.randint(0, 2, (B, 4, 1, h, w), generator=g).float()
        sat.scatter_(1, torch.randint(0, 4, (B, 1, 1, h, w), generator=g), 0.0)
        bump = 40.0 * sat * torch.zeros(B, 4, DFL, h, w).scatter_(2, hot, 1.0)
        m[:, :4 * DFL] += bump.reshape(B, 4 * DFL, h, w)
    return _case(maps, random_rows(12, B, nc, 83, wh_lo=0.1, wh_span=0.3), nc, (64, 64), (8.0, 16.0, 32.0))
