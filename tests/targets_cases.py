"""Batches for the yms_box_targets tests (CPU and GPU): B = 3 -- one plain sample, one Mosaic, one
MixUp -- for a 64 x 96 output over 13 synthetic sources, one per source slot, whose annotation counts
sum to a chosen M_cap.  Every box carries its own class id (its row in the annotation table), so a
kept SET is readable from the class column."""
import functools

import numpy as np
import torch

from yms import cache as C
from yms import data as D

AUG_FULL = {"hsv_h": 0.015, "hsv_s": 0.7, "hsv_v": 0.4, "degrees": 20.0, "translate": 0.1, "scale": 0.5,
            "shear": 8.0, "perspective": 0.08, "flipud": 0.5, "fliplr": 0.5}
H, W = 64, 96
NSRC = 13
EIGHT_SEED = 106         # sample_augmentation draws all seven optional transforms for a 40 x 56 source
# the committed list; should a change to the sampler land a box of one of these within rounding of a
# filter threshold, that seed is replaced here -- the comparison is never loosened
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)


def eight_stage_plan():
    plan = D.sample_augmentation(np.random.default_rng(EIGHT_SEED), AUG_FULL, 40, 56, H, W)
    assert len(plan.stages) == D.AUG_MAX_STAGES, plan.applied
    return plan


def random_boxes(rng, h, w, n):
    """n COCO xywh boxes inside an h x w image; about one in eight is tiny."""
    rows = []
    for _ in range(n):
        x, y = rng.uniform(0, w - 1), rng.uniform(0, h - 1)
        bw, bh = max(1e-2, (w - x) * rng.random()), max(1e-2, (h - y) * rng.random())
        if rng.random() < 0.125:
            bw, bh = bw * 0.03, bh * 0.03
        rows.append([x, y, bw, bh])
    return rows


@functools.lru_cache(maxsize=None)
def loss_batch(seed=0, n=60, size=64, nc=3):
    """B = 2 (one Mosaic, one MixUp sample) for a size x size input, classes in 0..nc-1: the tables
    and annotation table for the losses' padded-versus-compact comparison."""
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(16, 80)), int(rng.integers(16, 80))) for _ in range(12)]
    counts = [int(c) for c in rng.multinomial(n, [1.0 / 12] * 12)]
    boxes = np.array([b for (h, w), c in zip(sizes, counts) for b in random_boxes(rng, h, w, c)], np.float64)
    labels = rng.integers(0, nc, n).astype(np.int32)
    layers = [D.sample_mosaic(rng, AUG_FULL, sizes[4 * k:4 * k + 4], size, size) for k in range(3)]
    for t in layers[2].tiles:
        t.src += 4
    samples = [([0, 1, 2, 3], D.MosaicPlan(layers[:1])), (list(range(4, 12)), D.MosaicPlan(layers[1:], 0.5))]
    offsets = np.zeros(13, np.int64)
    np.cumsum(counts, out=offsets[1:])
    tiles, ltab, m = C.target_tables(samples, offsets)
    assert m == n
    return dict(boxes=boxes.reshape(-1, 4), labels=labels, tiles=tiles, layers=ltab, m_cap=n)


@functools.lru_cache(maxsize=None)
def make_batch(seed, m_cap, eight=False):
    """-> dict: samples [(sources, plan)] x 3, the annotation table (boxes float64 [N, 4], labels
    int32 [N], ann_offsets), the tables of target_tables and the host path's [M, 6] targets."""
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(8, 80)), int(rng.integers(8, 80))) for _ in range(NSRC)]
    if eight:
        sizes[0] = (40, 56)
    counts = [int(c) for c in rng.multinomial(m_cap, [1.0 / NSRC] * NSRC)]
    anns, label = [], 0
    for (h, w), n in zip(sizes, counts):
        anns.append((random_boxes(rng, h, w, n), list(range(label, label + n))))
        label += n
    plain = eight_stage_plan() if eight else D.sample_augmentation(rng, AUG_FULL, *sizes[0], H, W)
    mosaic = D.MosaicPlan([D.sample_mosaic(rng, AUG_FULL, sizes[1:5], H, W)])
    layers = [D.sample_mosaic(rng, AUG_FULL, sizes[5:9], H, W), D.sample_mosaic(rng, AUG_FULL, sizes[9:13], H, W)]
    for t in layers[1].tiles:
        t.src += 4
    mixup = D.MosaicPlan(layers, rng.beta(32.0, 32.0))
    samples = [([0], plain), ([1, 2, 3, 4], mosaic), (list(range(5, 13)), mixup)]
    offsets = np.zeros(NSRC + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    boxes = np.array([b for bx, _ in anns for b in bx], np.float64).reshape(-1, 4)
    labels = np.arange(m_cap, dtype=np.int32)
    tiles, ltab, m = C.target_tables(samples, offsets)
    assert m == m_cap
    host = [D.transform_boxes(*anns[0], plain), D.mosaic_targets(mosaic, [anns[i] for i in samples[1][0]]),
            D.mosaic_targets(mixup, [anns[i] for i in samples[2][0]])]
    host = torch.cat([torch.cat([torch.full((t.shape[0], 1), float(i)), t], 1) for i, t in enumerate(host)], 0)
    return dict(samples=samples, anns=anns, boxes=boxes, labels=labels, ann_offsets=offsets, tiles=tiles,
                layers=ltab, m_cap=m_cap, host=host.numpy())
