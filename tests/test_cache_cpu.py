"""yms.cache on its CPU seam (DeviceImageCache(device="cpu") stores and looks up as on the GPU): the
arena's placement rules, and CachedCOCODataset drawing COCODataset's plans."""
import numpy as np
import pytest
import torch

from test_data_cpu import _coco
from yms import cache as C
from yms import data as D

AUG_FULL = {"hsv_h": 0.015, "hsv_s": 0.7, "hsv_v": 0.4, "degrees": 20.0, "translate": 0.1, "scale": 0.5,
            "shear": 8.0, "perspective": 0.08, "flipud": 0.5, "fliplr": 0.5}
SIZES = [(32, 48), (40, 40), (21, 57), (64, 30), (48, 48)]


def _cache(sizes, capacity, chunk):
    return C.DeviceImageCache(sizes, [([], [])] * len(sizes), capacity, device="cpu", chunk_bytes=chunk)


def _image(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_slots_are_aligned_write_once_views():
    rng = np.random.default_rng(0)
    sizes = [(5, 7), (1, 1), (9, 3), (16, 16)]
    cache = _cache(sizes, 1 << 16, 1 << 14)
    images = [_image(rng, h, w) for h, w in sizes]
    for i, im in enumerate(images):
        assert not cache.is_resident(i)
        assert cache.insert(i, im)
    assert cache.num_resident == 4 and cache.resident.tolist() == [1, 1, 1, 1] and cache.resident.is_shared()
    for i, im in enumerate(images):
        v = cache.image(i)
        assert v.data_ptr() % 256 == 0 and v.is_contiguous() and v.dtype == torch.uint8
        assert v.data_ptr() == cache.slot(i).data_ptr() and cache.slot(i).stride(0) == 3 * sizes[i][1]
        assert tuple(cache.slot(i).shape) == tuple(v.shape)
        assert np.array_equal(v.numpy(), im)
        assert cache.image(i).data_ptr() == v.data_ptr()          # a view of the arena, not a copy
    assert len({cache.image(i).data_ptr() for i in range(4)}) == 4


def test_no_image_spans_two_chunks():
    rng = np.random.default_rng(1)
    sizes = [(30, 30)] * 4                          # 2700 bytes -> 2816 with the alignment: one per 4096 chunk
    cache = _cache(sizes, 4 * 4096, 4096)
    images = [_image(rng, h, w) for h, w in sizes]
    assert all(cache.insert(i, im) for i, im in enumerate(images))
    assert len(cache._chunks) == 4 and cache.allocated_bytes == 4 * 4096
    for i, im in enumerate(images):
        c, off = cache._where[i]
        assert c == i and off == 0 and off + 2700 <= 4096
        assert np.array_equal(cache.image(i).numpy(), im)
    # a small image still fits behind the first one, in its chunk
    small = _cache([(30, 30), (10, 10), (30, 30)], 2 * 4096, 4096)
    for i, (h, w) in enumerate(small.sizes):
        assert small.insert(i, _image(rng, h, w))
    assert [small._where[i] for i in range(3)] == [(0, 0), (0, 2816), (1, 0)]


def test_capacity_refusal_and_lazy_chunks():
    rng = np.random.default_rng(2)
    sizes = [(30, 30), (30, 30), (30, 30), (40, 40), (4, 4)]
    cache = _cache(sizes, 2 * 4096 + 1000, 4096)
    assert cache.allocated_bytes == 0                # nothing allocated before the first insert
    assert cache.insert(0, _image(rng, 30, 30)) and cache.allocated_bytes == 4096
    assert cache.insert(1, _image(rng, 30, 30)) and cache.allocated_bytes == 2 * 4096
    assert not cache.insert(2, _image(rng, 30, 30))  # the last chunk may only be 1000 bytes
    assert not cache.insert(3, _image(rng, 40, 40))  # 4800 bytes: larger than any chunk
    assert cache.resident.tolist() == [1, 1, 0, 0, 0] and cache.allocated_bytes == 2 * 4096
    assert cache.insert(4, _image(rng, 4, 4))        # but a small one still finds room
    with pytest.raises(KeyError):
        cache.image(2)
    with pytest.raises(KeyError, match="neither resident"):
        cache.slot(2)
    assert not _cache([(4, 4)], 0, 4096).insert(0, _image(rng, 4, 4))


def test_duplicate_insert_is_a_no_op():
    rng = np.random.default_rng(3)
    cache = _cache([(8, 8)], 1 << 14, 4096)
    first = _image(rng, 8, 8)
    assert cache.insert(0, first)
    ptr, used = cache.image(0).data_ptr(), cache._chunks[0][3]
    assert cache.insert(0, _image(rng, 8, 8))        # other pixels: write-once, the first stay
    assert cache.image(0).data_ptr() == ptr and cache._chunks[0][3] == used and cache.num_resident == 1
    assert np.array_equal(cache.image(0).numpy(), first)


def test_size_mismatch_raises():
    rng = np.random.default_rng(4)
    cache = _cache([(8, 6)], 1 << 14, 4096)
    with pytest.raises(ValueError, match="annotation file says 8x6"):
        cache.insert(0, _image(rng, 6, 8))
    with pytest.raises(ValueError):
        cache.insert(0, np.zeros((8, 6), np.uint8))
    with pytest.raises(ValueError):
        cache.insert(0, np.zeros((8, 6, 3), np.float32))
    assert cache.num_resident == 0
    assert cache.insert(0, _image(rng, 8, 6))
    with pytest.raises(ValueError):                  # also once resident
        cache.insert(0, _image(rng, 6, 8))


def test_for_dataset_annotation_table_and_fill(tmp_path):
    ann = _coco(tmp_path, SIZES)
    ds = D.COCODataset(str(tmp_path), str(ann), AUG_FULL, True, (64, 96), 3)
    cache = C.DeviceImageCache.for_dataset(ds, 1 << 20, device="cpu", chunk_bytes=1 << 16)
    assert len(cache) == len(ds) == 5 and cache.sizes == [ds._load(i)[0].shape[:2] for i in range(5)]
    counts = [len(ds.annotations(i)[1]) for i in range(5)]
    assert cache.ann_offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist() and sum(counts) == cache.nann
    assert cache.boxes.dtype == torch.float64 and cache.labels.dtype == torch.int32
    for i in range(5):
        bx, lab = ds.annotations(i)
        a0, a1 = cache.ann_offsets[i], cache.ann_offsets[i + 1]
        assert cache.boxes[a0:a1].tolist() == [[float(v) for v in b] for b in bx] and cache.labels[a0:a1].tolist() == lab
    assert cache.fill(ds, [3, 1, 3]) == 2 and cache.resident.tolist() == [0, 1, 0, 1, 0]
    assert cache.fill(ds) == 3 and cache.num_resident == 5 and cache.fill(ds) == 0
    for i in range(5):
        assert np.array_equal(cache.image(i).numpy(), ds._load(i)[0])


def test_json_size_that_is_not_the_decoded_size_raises(tmp_path):
    import json
    ann = _coco(tmp_path, SIZES)
    d = json.loads(ann.read_text())
    d["images"][0]["height"] += 1
    ann.write_text(json.dumps(d))
    ds = C.CachedCOCODataset(str(tmp_path), str(ann), AUG_FULL, True, (64, 96), 3)
    bad = ds.image_ids.index(d["images"][0]["id"])
    with pytest.raises(ValueError, match="annotation file says"):
        ds._decode(bad)
    cache = C.DeviceImageCache.for_dataset(ds, 1 << 20, device="cpu")
    with pytest.raises(ValueError, match="annotation file says"):
        cache.fill(ds, [bad])


def test_batch_tables_on_the_cpu_seam(tmp_path, monkeypatch):
    """The host half of collate_cached over a CPU cache: the MosImage records are mosaic_struct's over
    the arena views, byte for byte (pointers included: the views are zero-copy), and the restatement
    over the tile / layer tables and the cache's annotation table gives collate_targets' rows."""
    import ctypes
    import targets_ref as R
    ann = _coco(tmp_path, SIZES)
    monkeypatch.setattr(torch, "initial_seed", lambda: 0)
    tp = dict(AUG_FULL, mosaic=0.5, mixup=0.5)
    ds = D.COCODataset(str(tmp_path), str(ann), tp, True, (64, 96), 3, seed=0, mosaic=True)
    cache = C.DeviceImageCache.for_dataset(ds, 1 << 20, device="cpu", chunk_bytes=1 << 14)
    assert cache.fill(ds, [0, 1, 2, 3]) == 4
    cd = C.CachedCOCODataset(str(tmp_path), str(ann), tp, True, (64, 96), 3, seed=0, mosaic=True,
                             resident=cache.resident)
    host = [ds[i % 5] for i in range(6)]
    batch = [cd[i % 5] for i in range(6)]
    assert {i for _, _, ims in batch for i in ims} == {4}           # the one source that is not resident
    transient = {4: torch.from_numpy(ds._load(4)[0])}
    rec, tiles, layers, m = C.batch_tables(batch, cache, (64, 96), transient)
    for b, (srcs, plan, _) in enumerate(batch):
        want = D.mosaic_struct(plan, [transient[i] if i in transient else cache.image(i) for i in srcs])
        assert bytes(rec[b]) == bytes(want) and ctypes.sizeof(want) == ctypes.sizeof(D.MosImage)
    assert m == sum(int(cache.ann_offsets[i + 1] - cache.ann_offsets[i]) for s, _, _ in batch for i in s)
    ref = R.box_targets(tiles, layers, m, cache.boxes.numpy(), cache.labels.numpy())
    _, _, want = D.collate_targets(host)
    assert want.shape[0] > 0 and np.array_equal(R.compact(ref), want.numpy())
    with pytest.raises(ValueError, match="batch size"):
        C.batch_tables(batch, cache, (32, 32), transient)
    with pytest.raises(KeyError, match="neither resident"):
        C.batch_tables(batch, cache, (64, 96))


def _same_plan(a, b):
    if isinstance(a, D.MosaicPlan) != isinstance(b, D.MosaicPlan):
        return False
    la, lb = (a.layers, b.layers) if isinstance(a, D.MosaicPlan) else ([a], [b])
    if len(la) != len(lb) or getattr(a, "r", 1.0) != getattr(b, "r", 1.0):
        return False
    for x, y in zip(la, lb):
        if x.hsv != y.hsv or x.applied != y.applied or len(x.stages) != len(y.stages):
            return False
        if (x.src_h, x.src_w) != (y.src_h, y.src_w):
            return False
        for (F, *fa), (G, *ga) in zip(x.stages, y.stages):
            if not np.array_equal(F, G) or fa != ga:
                return False
        ta, tb = getattr(x, "tiles", []), getattr(y, "tiles", [])
        if [vars(t) for t in ta] != [vars(t) for t in tb] or getattr(x, "center", None) != getattr(y, "center", None):
            return False
    return True


def test_cached_dataset_draws_the_same_plans(tmp_path, monkeypatch):
    """Same seed, same indices, same call count -> the same plans (stages, tiles, r, hsv) and the same
    sources as COCODataset decodes; only the non-resident sources come back decoded."""
    ann = _coco(tmp_path, SIZES)
    monkeypatch.setattr(torch, "initial_seed", lambda: 0)      # the main-process draw stream, whatever ran before
    tp = dict(AUG_FULL, mosaic=0.5, mixup=0.5)
    ds = D.COCODataset(str(tmp_path), str(ann), tp, True, (64, 96), 3, seed=0, mosaic=True)
    resident = torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8)
    cd = C.CachedCOCODataset(str(tmp_path), str(ann), tp, True, (64, 96), 3, seed=0, mosaic=True, resident=resident)
    kinds = set()
    for k in range(12):
        images, _, plan = ds[k % 5]
        srcs, cplan, decoded = cd[k % 5]
        assert _same_plan(plan, cplan), k
        kinds.add(len(plan.layers) if isinstance(plan, D.MosaicPlan) else 0)
        images = images if isinstance(images, list) else [images]
        assert len(srcs) == len(images) and srcs[0] == k % 5
        assert set(decoded) == {i for i in srcs if not resident[i]}
        for i, im in zip(srcs, images):
            assert cd.size(i) == im.shape[:2]
            if i in decoded:
                assert np.array_equal(decoded[i], im)
    assert kinds == {0, 1, 2}, kinds                             # plain, Mosaic and MixUp samples
    # is_train=False keeps only the Resize, as there; letterbox batches are out of scope
    ev, cev = D.COCODataset(str(tmp_path), str(ann), tp, False, (64, 96), 3), \
        C.CachedCOCODataset(str(tmp_path), str(ann), tp, False, (64, 96), 3)
    assert _same_plan(ev[1][2], cev[1][1]) and cev[1][1].applied == ["resize"] and set(cev[1][2]) == {1}
    with pytest.raises(NotImplementedError):
        C.CachedCOCODataset(str(tmp_path), str(ann), tp, False, (64, 96), 3, letterbox=True)
