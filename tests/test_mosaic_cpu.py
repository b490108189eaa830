"""Mosaic / MixUp host half (yms/data.py: sample_mosaic, mosaic_boxes, the MosImage record, the
COCODataset opt-in) and known answers of the kernel's restatement (tests/mosaic_ref.py).  The
semantics are YOLOv5's load_mosaic / random_perspective / mixup restated; parity with ultralytics
and cv2 is unpinned (neither is installed)."""
import ctypes

import numpy as np
import torch

import mosaic_ref as MR
from oracle import preprocess_ref as P
from yms import _lib as L
from yms import data as D

AUG_FULL = {"hsv_h": 0.015, "hsv_s": 0.7, "hsv_v": 0.4, "degrees": 20.0, "translate": 0.1, "scale": 0.5,
            "shear": 8.0, "perspective": 0.08, "flipud": 0.5, "fliplr": 0.5}
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
COLOURS = [(200, 30, 40), (20, 180, 60), (10, 50, 220), (240, 230, 20)]


def _view(ly, ax, ay):
    """Replace the layer's stages by the W x H window of the canvas whose corner is (ax, ay)."""
    w, h = ly.frame
    ly.stages, ly.applied = [], []
    ly.add(np.array([[1, 0, -ax], [0, 1, -ay], [0, 0, 1]], np.float64), w, h, D.AUG_CONSTANT, "view")


def _pixels(ly, images, out_h, out_w, r=1.0):
    """HWC 0..255 values of the restatement for a one-layer plan."""
    layers, r = MR.record_of(D.MosaicPlan([ly], r), images)
    return MR.mosaic_normalize(layers, r, out_h, out_w, ZERO, ONE).transpose(1, 2, 0) * 255.0


def _flat(colour, h=4, w=4):
    return np.broadcast_to(np.array(colour, np.uint8), (h, w, 3)).copy()


def test_record_layout_and_null_arguments():
    lib = L.lib()
    assert ctypes.sizeof(D.MosImage) == lib.yms_mosaic_image_bytes()
    assert "yms_mosaic_normalize" in L.EXPORTED and "yms_mosaic_image_bytes" in L.EXPORTED
    mean, std = (ctypes.c_float * 3)(*D.IMAGENET_MEAN), (ctypes.c_float * 3)(*D.IMAGENET_STD)
    buf = ctypes.create_string_buffer(ctypes.sizeof(D.MosImage))
    p = ctypes.addressof(buf)
    assert lib.yms_mosaic_normalize(0, 0, None, 8, 8, None, None, None, None) == 0       # n <= 0: nothing to do
    assert lib.yms_mosaic_normalize(0, 1, None, 8, 8, mean, std, p, None) == 1
    assert lib.yms_mosaic_normalize(0, 1, p, 8, 8, mean, std, None, None) == 1
    assert lib.yms_mosaic_normalize(0, 1, p, 8, 8, None, std, p, None) == 1
    assert lib.yms_mosaic_normalize(0, 1, p, 8, 8, mean, None, p, None) == 1
    assert lib.yms_mosaic_normalize(0, 1, p, 0, 8, mean, std, p, None) == 1
    bad = (ctypes.c_float * 3)(0.2, 0.0, 0.2)                                              # non-positive std
    assert lib.yms_mosaic_normalize(0, 1, p, 8, 8, mean, bad, p, None) == 1


def test_four_quadrants_by_hand():
    """Output 8x8, four flat 4x4 sources (letterboxed x2 to 8x8), centre (8, 8), identity affine: T
    moves the canvas centre to the output centre, so the output is canvas [4, 12)^2 -- four 4x4
    quadrants in the colours of the sources at TL, TR, BL, BR."""
    ly = D.sample_mosaic(np.random.default_rng(0), {}, [(4, 4)] * 4, 8, 8, center=(8, 8))
    assert [t.rect for t in ly.tiles] == [(0, 0, 8, 8), (8, 0, 16, 8), (0, 8, 8, 16), (8, 8, 16, 16)]
    assert sorted(t.src for t in ly.tiles) == [0, 1, 2, 3] and ly.applied == ["affine"]
    assert np.allclose(ly.stages[0][0], [[1, 0, -4], [0, 1, -4], [0, 0, 1]])
    got = _pixels(ly, [_flat(c) for c in COLOURS], 8, 8)
    for k, (ys, xs) in enumerate([(slice(0, 4), slice(0, 4)), (slice(0, 4), slice(4, 8)),
                                  (slice(4, 8), slice(0, 4)), (slice(4, 8), slice(4, 8))]):
        want = np.array(COLOURS[ly.tiles[k].src], np.float32)
        assert np.abs(got[ys, xs] - want).max() < 1e-3, (k, got[ys, xs])


def test_cropped_tile_and_fill_by_hand():
    """Centre (4, 4): TL's resized 8x8 image starts at (-4, -4), the canvas edge crops it to [0, 4)^2
    and its BOTTOM-RIGHT quarter shows there; BR covers [4, 12)^2 and the canvas beyond 12 is fill."""
    ly = D.sample_mosaic(np.random.default_rng(1), {}, [(4, 4)] * 4, 8, 8, center=(4, 4))
    assert [t.rect for t in ly.tiles] == [(0, 0, 4, 4), (4, 0, 12, 4), (0, 4, 4, 12), (4, 4, 12, 12)]
    assert (ly.tiles[0].ox, ly.tiles[0].oy) == (-4, -4)
    A, B = np.array([10, 20, 30], np.float32), np.array([250, 120, 90], np.float32)
    images = [_flat(c) for c in COLOURS]
    tl = _flat(A.astype(np.uint8))
    tl[2:, 2:] = B.astype(np.uint8)
    images[ly.tiles[0].src] = tl
    _view(ly, 0, 0)                                    # canvas [0, 8)^2
    got = _pixels(ly, images, 8, 8)
    # canvas 1..3 <- source 2.25, 2.75, 3.25 (clamped to 3): inside the B quarter; canvas 0 <- source
    # 1.75: three A taps and one B tap at fx = fy = 0.75 -> A + 0.5625 (B - A)
    assert np.abs(got[1:4, 1:4] - B).max() < 1e-3
    assert np.abs(got[0, 0] - (A + 0.5625 * (B - A))).max() < 1e-3
    for k, (ys, xs) in {1: (slice(0, 4), slice(4, 8)), 2: (slice(4, 8), slice(0, 4)),
                        3: (slice(4, 8), slice(4, 8))}.items():
        assert np.abs(got[ys, xs] - np.array(COLOURS[ly.tiles[k].src], np.float32)).max() < 1e-3
    _view(ly, 8, 8)                                    # canvas [8, 16)^2: BR in [8, 12)^2, fill elsewhere
    got = _pixels(ly, images, 8, 8)
    br = images[ly.tiles[3].src].astype(np.float32)[0, 0]
    assert np.abs(got[:4, :4] - br).max() < 1e-3
    assert np.abs(got[4:] - 114.0).max() < 1e-3 and np.abs(got[:, 4:] - 114.0).max() < 1e-3
    # the stage's constant border is the fill too, and the HSV shift reaches the fill: V + 20 -> 134 grey
    _view(ly, 12, 12)
    ly.hsv = (0.0, 0.0, 20.0)
    got = _pixels(ly, images, 8, 8)
    assert np.abs(got - 134.0).max() < 1e-3


def test_tile_rects_disjoint_anchored_inside_canvas():
    rng = np.random.default_rng(7)
    for d in range(200):
        H, W = ((64, 96), (96, 64))[d % 2]
        sizes = [(int(rng.integers(1, 701)), int(rng.integers(1, 301))) for _ in range(4)]
        if d == 0:
            sizes = [(1, 1), (700, 300), (1, 300), (700, 1)]
        ly = D.sample_mosaic(rng, AUG_FULL, sizes, H, W)
        xc, yc = ly.center
        assert W / 2 <= xc < 3 * W / 2 and H / 2 <= yc < 3 * H / 2
        assert sorted(t.src for t in ly.tiles) == [0, 1, 2, 3]
        for k, t in enumerate(ly.tiles):
            h0, w0 = sizes[t.src]
            r = min(W / w0, H / h0)
            assert (t.h, t.w) == (h0, w0) and (t.nw, t.nh) == (max(1, round(w0 * r)), max(1, round(h0 * r)))
            assert t.nw <= W and t.nh <= H
            x0, y0, x1, y1 = t.rect
            assert 0 <= x0 < x1 <= 2 * W and 0 <= y0 < y1 <= 2 * H, (sizes, t.rect)
            want = ((max(xc - t.nw, 0), xc) if k in (0, 2) else (xc, min(xc + t.nw, 2 * W))) + \
                   ((max(yc - t.nh, 0), yc) if k in (0, 1) else (yc, min(yc + t.nh, 2 * H)))
            assert (x0, x1, y0, y1) == want
            assert (t.ox, t.oy) == (xc - t.nw if k in (0, 2) else xc, yc - t.nh if k in (0, 1) else yc)
            sx, sy, tx, ty = t.map                         # column 0 of the resized image sits at ox
            assert abs(sx * t.ox + tx - (0.5 * sx - 0.5)) < 1e-9 and abs(sy * t.oy + ty - (0.5 * sy - 0.5)) < 1e-9
        for a in range(4):
            for b in range(a + 1, 4):
                p, q = ly.tiles[a].rect, ly.tiles[b].rect
                assert min(p[2], q[2]) <= max(p[0], q[0]) or min(p[3], q[3]) <= max(p[1], q[1]), (p, q)


def _box_layer(center, tp=None, seed=0):
    """Output 64x64, four 32x32 sources (x2 to 64x64); -> layer and an empty annotation list."""
    ly = D.sample_mosaic(np.random.default_rng(seed), tp or {}, [(32, 32)] * 4, 64, 64, center=center)
    return ly, [([], []) for _ in range(4)]


def test_boxes_by_hand():
    # wholly inside TL, identity affine: source [20, 28]^2 -> canvas [40, 56]^2 -> output (canvas - 32) [8, 24]^2
    ly, anns = _box_layer((64, 64))
    anns[ly.tiles[0].src] = ([[20, 20, 8, 8]], [5])
    t = D.mosaic_boxes(ly, anns)
    assert t.shape == (1, 5) and torch.allclose(t[0], torch.tensor([5.0, 0.25, 0.25, 0.25, 0.25]), atol=1e-6)
    # the same box in BR: canvas [104, 120]^2 -> output [72, 88]^2, outside the frame: dropped
    anns = [([], []) for _ in range(4)]
    anns[ly.tiles[3].src] = ([[20, 20, 8, 8]], [5])
    assert D.mosaic_boxes(ly, anns).shape == (0, 5)
    # a flipped layer (fliplr drawn with probability 1): X -> 64 - X, [8, 24] -> [40, 56]
    ly, anns = _box_layer((64, 64), {"fliplr": 1.0})
    assert ly.applied == ["affine", "fliplr"]
    anns[ly.tiles[0].src] = ([[20, 20, 8, 8]], [5])
    t = D.mosaic_boxes(ly, anns)
    assert t.shape == (1, 5) and torch.allclose(t[0], torch.tensor([5.0, 0.75, 0.25, 0.25, 0.25]), atol=1e-6)


def test_boxes_cut_by_the_canvas_edge():
    """Centre (32, 32): TL starts at canvas (-32, -32) and shows in [0, 32)^2; the output is canvas [0, 64)^2."""
    ly, anns = _box_layer((32, 32))
    _view(ly, 0, 0)
    src = ly.tiles[0].src
    # source [10, 20]^2 -> canvas [-12, 8]^2 (400 px^2), clipped by the tile's rect to [0, 8]^2 (64 px^2):
    # visibility 0.16 against the UNCLIPPED envelope -> kept, as the clipped box
    anns[src] = ([[10, 10, 10, 10]], [2])
    t = D.mosaic_boxes(ly, anns)
    assert t.shape == (1, 5) and torch.allclose(t[0], torch.tensor([2.0, 4 / 64, 4 / 64, 8 / 64, 8 / 64]), atol=1e-6)
    # source [8, 18]^2 -> canvas [-16, 4]^2, clipped [0, 4]^2: 16 / 400 = 0.04 < 0.1 -> dropped (16 px^2 would
    # pass the area filter, and against its own clipped area the visibility would be 1)
    anns[src] = ([[8, 8, 10, 10]], [2])
    assert D.mosaic_boxes(ly, anns).shape == (0, 5)
    # source [4, 14]^2 -> canvas [-24, -4]^2: nothing left inside the tile's rect
    anns[src] = ([[4, 4, 10, 10]], [2])
    assert D.mosaic_boxes(ly, anns).shape == (0, 5)
    # both survivors and the drop together keep their order
    anns[src] = ([[10, 10, 10, 10], [8, 8, 10, 10], [20, 20, 4, 4]], [2, 3, 4])
    assert D.mosaic_boxes(ly, anns)[:, 0].tolist() == [2.0, 4.0]


def test_mixup_concatenates_targets():
    la, anns = _box_layer((64, 64), seed=1)
    lb, more = _box_layer((64, 64), {"fliplr": 1.0}, seed=2)
    for t in lb.tiles:
        t.src += 4
    anns = anns + more
    anns[la.tiles[0].src] = ([[20, 20, 8, 8]], [5])
    anns[lb.tiles[0].src] = ([[20, 20, 8, 8]], [6])
    plan = D.MosaicPlan([la, lb], 0.4)
    assert plan.applied[:2] == ["mosaic", "mixup"] and plan.frame == (64, 64)
    t = D.mosaic_targets(plan, anns)
    assert torch.allclose(t, torch.tensor([[5.0, 0.25, 0.25, 0.25, 0.25], [6.0, 0.75, 0.25, 0.25, 0.25]]), atol=1e-6)


def _sig(plan):
    """Everything a plan holds, as plain python values."""
    if isinstance(plan, D.MosaicPlan):
        return ("mosaic", plan.r, [(ly.center, ly.fill, [(t.src, t.rect, t.map) for t in ly.tiles], _sig_aug(ly))
                                   for ly in plan.layers])
    return _sig_aug(plan)


def _sig_aug(pl):
    return (pl.src_h, pl.src_w, pl.hsv, list(pl.applied),
            [(F.tolist(), iw, ih, ow, oh, b) for F, iw, ih, ow, oh, b in pl.stages])


def test_same_seed_same_plan():
    sizes = [(48, 64), (333, 517), (1, 1), (90, 40)]
    a = D.sample_mosaic(np.random.default_rng(5), AUG_FULL, sizes, 64, 96)
    b = D.sample_mosaic(np.random.default_rng(5), AUG_FULL, sizes, 64, 96)
    c = D.sample_mosaic(np.random.default_rng(6), AUG_FULL, sizes, 64, 96)
    assert _sig(D.MosaicPlan([a])) == _sig(D.MosaicPlan([b])) != _sig(D.MosaicPlan([c]))
    assert len(a.stages) <= 3 and a.stages[0][1:3] == (192, 128) and a.stages[0][5] == D.AUG_CONSTANT


def _items(ds, epochs=2):
    return [ds[i] for _ in range(epochs) for i in range(len(ds))]


def _same(a, b):
    ims = lambda v: v if isinstance(v, list) else [v]
    return len(a) == len(b) and all(
        len(ims(x[0])) == len(ims(y[0])) and all(np.array_equal(p, q) for p, q in zip(ims(x[0]), ims(y[0])))
        and torch.equal(x[1], y[1]) and _sig(x[2]) == _sig(y[2]) for x, y in zip(a, b))


def test_dataset_opt_in_and_unchanged_default(tmp_path):
    from test_data_cpu import _coco
    ann = _coco(tmp_path, [(32, 48), (40, 40), (21, 57), (64, 30), (48, 48)])
    make = lambda tp, **kw: D.COCODataset(str(tmp_path), str(ann), tp, True, (64, 96), 3, seed=3, **kw)
    base = _items(make(AUG_FULL))
    assert all(isinstance(p, D.AugPlan) and not isinstance(p, D.MosaicLayer) for _, _, p in base)
    # the reference's config dict with the feature off: the keys stay ignored, the draw stream untouched
    assert _same(base, _items(make(dict(AUG_FULL, mosaic=1.0, mixup=1.0))))
    assert _same(base, _items(make(dict(AUG_FULL, mosaic=1.0, mixup=1.0), mosaic=False)))
    # opted in with both probabilities 0 (or absent): the same again
    assert _same(base, _items(make(dict(AUG_FULL, mosaic=0.0, mixup=0.0), mosaic=True)))
    assert _same(base, _items(make(AUG_FULL, mosaic=True)))
    # opted in: mosaic samples carry their image list; MixUp doubles it; evaluation never mosaics
    ds = make(dict(AUG_FULL, mosaic=1.0, mixup=0.0), mosaic=True)
    for images, t, plan in _items(ds, 1):
        assert isinstance(plan, D.MosaicPlan) and len(plan.layers) == 1 and plan.r == 1.0 and len(images) == 4
        assert t.dim() == 2 and t.shape[1] == 5 and plan.frame == (96, 64)
    ds = make(dict(AUG_FULL, mosaic=1.0, mixup=1.0), mosaic=True)
    items = _items(ds, 1)
    for i, (images, t, plan) in enumerate(items):
        assert len(plan.layers) == 2 and len(images) == 8 and 0.0 < plan.r < 1.0
        assert np.array_equal(images[0], base[i][0])          # the indexed sample is the first source
        assert sorted(q.src for q in plan.layers[1].tiles) == [4, 5, 6, 7]
        assert torch.all((t[:, 1:] >= 0) & (t[:, 1:] <= 1))
    assert _same(items, _items(make(dict(AUG_FULL, mosaic=1.0, mixup=1.0), mosaic=True), 1))   # reproducible
    ds.mosaic = False                                          # closing mosaic: a plain attribute
    assert all(isinstance(p, D.AugPlan) for _, _, p in _items(ds, 1))
    ev = D.COCODataset(str(tmp_path), str(ann), dict(AUG_FULL, mosaic=1.0), False, (64, 96), 3, mosaic=True)
    assert ev[0][2].applied == ["resize"]
    # collate: a mosaic sample's image list stays one entry
    images, plans, tg = D.collate_targets(items[:2] + base[:1])
    assert [len(im) if isinstance(im, list) else 1 for im in images] == [8, 8, 1] and tg.shape[1] == 6


def test_degenerate_record_is_the_plain_kernel():
    """A plain AugPlan as one layer {fill 0, one identity tile}: the restatement gives
    oracle.preprocess_ref.augment_normalize's array exactly."""
    from test_augment_cpu import stages_of
    rng = np.random.default_rng(9)
    seen = set()
    for h, w in [(37, 53), (64, 64), (17, 200), (90, 120), (2, 3), (48, 31), (40, 40), (33, 71)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        plan = D.sample_augmentation(rng, AUG_FULL, h, w, 40, 56)
        seen |= set(plan.applied)
        st, hsv = stages_of(plan)
        layers, r = MR.record_of(plan, img)
        assert len(layers) == 1 and layers[0]["fill"] == 0 and layers[0]["do_hsv"] in (0, 1)
        assert layers[0]["tiles"][0][1] == (0, 0, w, h)
        got = MR.mosaic_normalize(layers, r, 40, 56, D.IMAGENET_MEAN, D.IMAGENET_STD)
        assert np.array_equal(got, P.augment_normalize(img, hsv, st, 40, 56, D.IMAGENET_MEAN, D.IMAGENET_STD))
    assert {"hsv", "rotate", "shift", "scale", "shear", "perspective", "fliplr", "flipud"} <= seen, seen
