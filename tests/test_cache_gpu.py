"""CachedCOCODataset + collate_cached against COCODataset(mosaic=True) + collate_to_gpu on a tiny
on-disk COCO: the same batch and the same boxes from arena-resident images and device-computed
targets, with two launches and no host sync."""
import json

import numpy as np
import pytest
import torch

from yms import cache as C
from yms import data as D

pytestmark = pytest.mark.gpu
AUG_FULL = {"hsv_h": 0.015, "hsv_s": 0.7, "hsv_v": 0.4, "degrees": 20.0, "translate": 0.1, "scale": 0.5,
            "shear": 8.0, "perspective": 0.08, "flipud": 0.5, "fliplr": 0.5}
TP = dict(AUG_FULL, mosaic=0.5, mixup=0.5)
SIZES = [(33, 47), (41, 39), (35, 45), (43, 37), (39, 41)]      # 4653 .. 4797 bytes decoded, 4864 per slot
SIZE = (64, 96)
NB = 6


def _coco5(root):
    """Five PNGs of odd sizes, four to six boxes each (one image's include a sliver), three classes."""
    from PIL import Image
    rng = np.random.default_rng(7)
    images, anns = [], []
    for i, (h, w) in enumerate(SIZES):
        fn = f"im{i}.png"
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / fn)
        images.append({"id": 20 + i, "file_name": fn, "height": h, "width": w})
        for _ in range(4 + i % 3):
            x, y = rng.uniform(0, w - 4), rng.uniform(0, h - 4)
            bw, bh = rng.uniform(2, w - x), rng.uniform(2, h - y)
            anns.append({"id": len(anns) + 1, "image_id": 20 + i, "category_id": int(rng.integers(1, 4)),
                         "bbox": [x, y, bw, bh], "area": bw * bh, "iscrowd": 0})
    anns.append({"id": len(anns) + 1, "image_id": 20, "category_id": 1, "bbox": [3.0, 3.0, 0.05, 20.0], "area": 1.0,
                 "iscrowd": 0})
    p = root / "ann.json"
    p.write_text(json.dumps({"images": images, "annotations": anns,
                             "categories": [{"id": k, "name": str(k)} for k in (1, 2, 3)]}))
    return p


@pytest.fixture
def coco(tmp_path, monkeypatch):
    """(COCODataset, its host batch on the GPU, a factory of CachedCOCODatasets that draw the same plans)."""
    ann = _coco5(tmp_path)
    monkeypatch.setattr(torch, "initial_seed", lambda: 0)      # the main-process draw stream, whatever ran before
    args = (str(tmp_path), str(ann), TP, True, SIZE, 3)
    ds = D.COCODataset(*args, seed=0, mosaic=True)
    batch = [ds[i % 5] for i in range(NB)]
    kinds = [len(p.layers) if isinstance(p, D.MosaicPlan) else 0 for _, _, p in batch]
    assert 0 in kinds and 1 in kinds and 2 in kinds, kinds        # plain, Mosaic and MixUp samples together
    x, tg = D.collate_to_gpu(batch, SIZE, "cuda")
    assert tg.shape[0] > 0
    return ds, (x, tg), lambda resident: C.CachedCOCODataset(*args, seed=0, mosaic=True, resident=resident)


def _cached_batch(cd):
    return [cd[i % 5] for i in range(NB)]


def _check(got, want):
    x, tg = got
    assert x.dtype == want[0].dtype and torch.equal(x, want[0])
    assert tg.dim() == 2 and tg.shape[1] == 6 and tg.shape[0] >= want[1].shape[0] and tg.dtype == torch.float32
    assert torch.equal(C.compact_targets(tg), want[1])
    pad = tg[tg[:, 0] < 0]
    assert pad.shape[0] == tg.shape[0] - want[1].shape[0] and not pad[:, 1:].any() and bool((pad[:, 0] == -1).all())


def test_all_resident_batch_equals_the_host_path(coco, monkeypatch):
    ds, want, make = coco
    cache = C.DeviceImageCache.for_dataset(ds, 1 << 20, "cuda", chunk_bytes=1 << 14)
    assert cache.fill(ds) == 5 and cache.num_resident == 5
    for i in range(5):
        v = cache.image(i)
        assert v.is_cuda and v.data_ptr() % 256 == 0 and np.array_equal(v.cpu().numpy(), ds._load(i)[0])
    batch = _cached_batch(make(cache.resident))
    assert all(not images for _, _, images in batch)              # nothing decoded: every source is resident
    calls = []
    real = C.L.call
    monkeypatch.setattr(C.L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    got = C.collate_cached(batch, cache, SIZE, "cuda")
    assert calls == ["yms_mosaic_normalize", "yms_box_targets"], calls
    # padded: one row per candidate box of every source of every tile, not per surviving box
    assert got[1].shape[0] == sum(int(cache.ann_offsets[i + 1] - cache.ann_offsets[i]) for s, _, _ in batch for i in s)
    _check(got, want)


def test_first_touch_fills_the_cache(coco):
    ds, want, make = coco
    cache = C.DeviceImageCache.for_dataset(ds, 1 << 20, "cuda", chunk_bytes=1 << 14)
    cd = make(cache.resident)
    assert cache.num_resident == 0
    first = cd[0]
    assert set(first[2]) == set(first[0])                          # everything decoded: nothing is resident yet
    C.collate_cached([first], cache, SIZE, "cuda")
    assert cache.num_resident == len(set(first[0])) > 0
    again = cd[0]
    assert not (set(again[2]) & set(first[0]))                     # a worker now skips those decodes
    n1 = cache.num_resident
    C.collate_cached([cd[k] for k in range(5)], cache, SIZE, "cuda")
    assert cache.num_resident == 5 >= n1
    for i in range(5):
        assert np.array_equal(cache.image(i).cpu().numpy(), ds._load(i)[0])
    # the same six draws as the host batch, from a fresh dataset over the now full cache
    _check(C.collate_cached(_cached_batch(make(cache.resident)), cache, SIZE, "cuda"), want)


def test_capacity_for_two_of_five(coco):
    """10000 bytes hold two 4864-byte slots: the other three sources stay transient uploads, in the
    first batch and in every later one."""
    ds, want, make = coco
    cache = C.DeviceImageCache.for_dataset(ds, 10000, "cuda", chunk_bytes=1 << 14)
    batch = _cached_batch(make(cache.resident))
    _check(C.collate_cached(batch, cache, SIZE, "cuda"), want)
    assert cache.num_resident == 2 and cache.allocated_bytes == 10000
    again = _cached_batch(make(cache.resident))
    decoded = {i for _, _, images in again for i in images}
    assert decoded and not any(cache.is_resident(i) for i in decoded)
    _check(C.collate_cached(again, cache, SIZE, "cuda"), want)
    assert cache.num_resident == 2


def test_all_resident_collate_does_not_sync(coco):
    ds, want, make = coco
    cache = C.DeviceImageCache.for_dataset(ds, 1 << 20, "cuda")
    cache.fill(ds)
    C.collate_cached(_cached_batch(make(cache.resident)), cache, SIZE, "cuda")      # warm-up: pinned block, code objects
    batch = _cached_batch(make(cache.resident))
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            want[1][0, 0].item()                      # the mode does catch a sync in this build
        got = C.collate_cached(batch, cache, SIZE, "cuda")
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    _check(got, want)


def test_bf16_batch_and_argument_errors(coco):
    ds, want, make = coco
    cache = C.DeviceImageCache.for_dataset(ds, 1 << 20, "cuda")
    batch = _cached_batch(make(cache.resident))
    x, _ = C.collate_cached(batch, cache, SIZE, "cuda", dtype=torch.bfloat16)
    assert x.dtype == torch.bfloat16 and torch.equal(x, want[0].to(torch.bfloat16))    # one rounding, at the store
    with pytest.raises(ValueError, match="batch size"):
        C.collate_cached(batch, cache, (32, 32), "cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.collate_cached(batch, C.DeviceImageCache.for_dataset(ds, 1 << 20, "cpu"), SIZE, "cuda")
    with pytest.raises(ValueError, match="empty batch"):
        C.collate_cached([], cache, SIZE, "cuda")
