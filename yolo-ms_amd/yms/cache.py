"""Device-resident input pipeline (opt-in): decoded images and the annotation table stay on the
GPU, and a batch's targets are computed there.

With Mosaic / MixUp on, ``COCODataset.__getitem__`` decodes four to eight JPEGs per output image and
walks every source box through the stage chain in Python.  Here each image is decoded ONCE and kept
in HBM (``DeviceImageCache``: a write-once arena without eviction -- COCO train2017 decoded is about
100 GB, the card has 288), the annotations live in one device table, and per step the host only
samples the plans (``CachedCOCODataset``, same draws as ``COCODataset``) and fills three small tables
(``collate_cached``): the MosImage records of ``yms_mosaic_normalize`` pointing into the arena, and
the tile / layer tables of ``yms_box_targets`` (csrc/targets.hip), which writes every candidate box
into a row fixed by the host -- ``(image, class, cx, cy, w, h)`` if it survives the filters of
``transform_boxes`` / ``mosaic_boxes``, ``(-1, 0, 0, 0, 0, 0)`` otherwise.  The losses skip rows whose
image index is negative, so nothing is compacted, counted or read back: the targets tensor is
PADDED, ``targets.shape[0]`` is the number of candidates, not of boxes (``compact_targets`` drops the
padding, with a host sync, for logging and tests).

Out of scope: evaluation / letterbox batches, eviction, downscaling on insert, sampling on the
device; under data parallelism each rank keeps its own cache.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib as L
from . import data as D

SLOT_ALIGN = 256

# csrc/targets.hip TgtTile / TgtLayer (checked against yms_tgt_tile_bytes() / yms_tgt_layer_bytes())
TILE_DT = np.dtype([("image", "<i4"), ("layer", "<i4"), ("ann0", "<i4"), ("count", "<i4"), ("out0", "<i4"),
                    ("clip", "<i4"), ("gx", "<f8"), ("gy", "<f8"), ("ox", "<f8"), ("oy", "<f8"), ("rect", "<f8", (4,))])
LAYER_DT = np.dtype([("nst", "<i4"), ("out_w", "<i4"), ("out_h", "<i4"), ("pad_", "<i4"),
                     ("m", "<f8", (D.AUG_MAX_STAGES, 9))])


def target_tables(samples, ann_offsets):
    """The tile and layer tables of yms_box_targets for a batch.  samples: per output image
    (source dataset indices, plan) -- a MosaicPlan whose tiles' ``src`` index the list, or a plain
    AugPlan over its one source; ann_offsets: [n + 1] first annotation row per dataset index.
    -> (tiles [TILE_DT], layers [LAYER_DT], m_cap).  Rows follow the host's order: samples in batch
    order, a MixUp sample's layer 0 before its layer 1, tiles TL, TR, BL, BR, a source's boxes in
    annotation order.  Sources without annotations get no tile."""
    tiles, layers, m = [], [], 0
    for b, (srcs, plan) in enumerate(samples):
        mosaic = isinstance(plan, D.MosaicPlan)
        for ly in (plan.layers if mosaic else [plan]):
            if len(ly.stages) > D.AUG_MAX_STAGES:
                raise ValueError("yms: a layer has at most AUG_MAX_STAGES stages")
            if mosaic:
                parts = [(srcs[t.src], 1, t.nw / t.w, t.nh / t.h, float(t.ox), float(t.oy),
                          tuple(float(v) for v in t.rect)) for t in ly.tiles]
            else:
                parts = [(srcs[0], 0, 1.0, 1.0, 0.0, 0.0, (0.0, 0.0, float(ly.src_w), float(ly.src_h)))]
            for src, clip, gx, gy, ox, oy, rect in parts:
                a0, a1 = int(ann_offsets[src]), int(ann_offsets[src + 1])
                if a1 > a0:
                    tiles.append((b, len(layers), a0, a1 - a0, m, clip, gx, gy, ox, oy, rect))
                    m += a1 - a0
            layers.append(ly)
    tt = np.array(tiles, dtype=TILE_DT) if tiles else np.zeros(0, TILE_DT)
    lt = np.zeros(len(layers), LAYER_DT)
    for j, ly in enumerate(layers):
        out_w, out_h = ly.frame
        lt[j]["nst"], lt[j]["out_w"], lt[j]["out_h"] = len(ly.stages), out_w, out_h
        for k, (F, *_) in enumerate(ly.stages):
            lt["m"][j, k] = np.asarray(F, np.float64).reshape(9)
    return tt, lt, m


def _check_layouts():
    if L.lib().yms_tgt_tile_bytes() != TILE_DT.itemsize or L.lib().yms_tgt_layer_bytes() != LAYER_DT.itemsize:
        raise RuntimeError("yms: target table layouts differ from the library's")
    if L.lib().yms_mosaic_image_bytes() != ctypes.sizeof(D.MosImage):
        raise RuntimeError("yms: MosImage layout differs from the library's")


def box_targets(tiles, layers, m_cap, boxes, labels, out=None):
    """yms_box_targets over host tables (``target_tables``) and the device annotation table
    (float64 [N, 4], int32 [N]) -> padded float32 [m_cap, 6] targets.  The tables go up with a plain
    blocking copy: a convenience for tests and tools -- ``collate_cached`` stages them in pinned memory."""
    dev = boxes.device
    if dev.type != "cuda":
        raise RuntimeError("yms: box_targets runs on ROCm GPU tensors only (no CPU fallback)")
    if boxes.dtype != torch.float64 or labels.dtype != torch.int32 or labels.device != dev \
            or not boxes.is_contiguous() or not labels.is_contiguous():
        raise ValueError("yms: annotation table must be contiguous float64 [N, 4] boxes and int32 [N] labels")
    _check_layouts()
    if tiles.dtype != TILE_DT or layers.dtype != LAYER_DT:
        raise ValueError("yms: tables must come from target_tables")
    raw = np.concatenate([np.ascontiguousarray(tiles).view(np.uint8), np.ascontiguousarray(layers).view(np.uint8)])
    tab = torch.from_numpy(raw).to(dev) if raw.size else torch.empty(0, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty((m_cap, 6), dtype=torch.float32, device=dev)
    L.call("yms_box_targets", len(tiles), tab.data_ptr(), len(layers), tab.data_ptr() + tiles.nbytes,
           boxes.data_ptr(), labels.data_ptr(), labels.shape[0], m_cap, out.data_ptr(), L.stream_ptr(dev))
    tab.record_stream(torch.cuda.current_stream(dev))
    return out


def compact_targets(t):
    """Padded [M_cap, 6] targets -> the [M, 6] rows of real boxes, order kept.  Syncs with the host
    (the row count is read back): for logging and tests, not for the training step."""
    return t[t[:, 0] >= 0]


class _Slot:
    """What mosaic_struct reads of an image tensor, for an arena slot (no tensor view per source)."""
    __slots__ = ("ptr", "shape")

    def __init__(self, ptr, h, w):
        self.ptr, self.shape = ptr, (h, w, 3)

    def data_ptr(self):
        return self.ptr

    def stride(self, d):
        return (3 * self.shape[1], 3, 1)[d]


class _Decoder(torch.utils.data.Dataset):
    def __init__(self, ds, indices):
        self.ds, self.indices = ds, indices

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, k):
        i = self.indices[k]
        return i, self.ds._load(i)[0]


class DeviceImageCache:
    """Decoded HWC uint8 images (tight rows) of a dataset, write-once, in an arena of chunks on
    ``device`` allocated lazily up to ``capacity_bytes``; every slot starts 256-byte aligned, no image
    spans two chunks, nothing is evicted.  Also the dataset's annotation table: ``boxes`` float64
    [N, 4] COCO xywh and ``labels`` int32 [N] on the device, ``ann_offsets`` [n + 1] on the host.
    ``resident`` (uint8, one entry per dataset index) lives in shared memory, so DataLoader workers
    started before an insert still see it.  ``device="cpu"`` stores and looks up the same way (tests).
    Inserts and the kernels that read the arena are ordered by the caller's current stream: use one."""

    def __init__(self, sizes, annotations, capacity_bytes, device="cuda", chunk_bytes=1 << 30, resident=None):
        """resident: a shared-memory uint8 [n] tensor of zeros to use as the flags (for workers that
        were started, with it, before the cache could be built); by default one is made here."""
        self.device = torch.device(device)
        self.capacity_bytes, self.chunk_bytes = int(capacity_bytes), int(chunk_bytes)
        if self.capacity_bytes < 0 or self.chunk_bytes <= 0:
            raise ValueError("yms: capacity_bytes >= 0 and chunk_bytes > 0")
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        n = len(self.sizes)
        counts = [len(lab) for _, lab in annotations]
        if len(counts) != n:
            raise ValueError("yms: one annotation entry per image")
        self.ann_offsets = np.zeros(n + 1, np.int64)
        np.cumsum(counts, out=self.ann_offsets[1:])
        self.nann = int(self.ann_offsets[-1])
        boxes = np.zeros((max(self.nann, 1), 4), np.float64)
        labels = np.zeros(max(self.nann, 1), np.int32)
        for i, (bx, lab) in enumerate(annotations):
            if counts[i]:
                boxes[self.ann_offsets[i]:self.ann_offsets[i + 1]] = np.asarray(bx, np.float64).reshape(-1, 4)
                labels[self.ann_offsets[i]:self.ann_offsets[i + 1]] = np.asarray(lab, np.int32)
        self.boxes = torch.from_numpy(boxes).to(self.device)[:self.nann]
        self.labels = torch.from_numpy(labels).to(self.device)[:self.nann]
        if resident is None:
            resident = torch.zeros(n, dtype=torch.uint8).share_memory_()
        if resident.dtype != torch.uint8 or tuple(resident.shape) != (n,) or not resident.is_shared() or resident.any():
            raise ValueError("yms: resident must be a zeroed shared-memory uint8 tensor, one entry per image")
        self.resident = resident
        self._res = self.resident.numpy()          # the same shared bytes, cheap to index
        self._chunks = []                          # [buffer, base, size, used]
        self._where = {}                           # index -> (chunk, offset)
        self._slots = {}                           # index -> _Slot
        self.allocated_bytes = 0

    @classmethod
    def for_dataset(cls, ds, capacity_bytes, device="cuda", chunk_bytes=1 << 30, resident=None):
        """Sizes from the JSON's height / width (no decode), annotations from ``ds.annotations``."""
        sizes = [(ds.imgs[i]["height"], ds.imgs[i]["width"]) for i in ds.image_ids]
        return cls(sizes, [ds.annotations(i) for i in range(len(ds))], capacity_bytes, device, chunk_bytes, resident)

    def __len__(self):
        return len(self.sizes)

    @property
    def num_resident(self):
        return int(self._res.sum())

    def is_resident(self, i):
        return bool(self._res[i])

    def _place(self, nbytes):
        for c, ch in enumerate(self._chunks):
            off = -(-ch[3] // SLOT_ALIGN) * SLOT_ALIGN
            if off + nbytes <= ch[2]:
                ch[3] = off + nbytes
                return c, off
        size = min(self.chunk_bytes, self.capacity_bytes - self.allocated_bytes)
        if nbytes > size:
            return None
        pad = 0 if self.device.type == "cuda" else SLOT_ALIGN - 1     # the device allocator aligns further
        buf = torch.empty(size + pad, dtype=torch.uint8, device=self.device)
        base = -buf.data_ptr() % SLOT_ALIGN
        if base > pad:
            raise RuntimeError("yms: arena chunk is not 256-byte aligned")
        self._chunks.append([buf, base, size, nbytes])
        self.allocated_bytes += size
        return len(self._chunks) - 1, 0

    def insert(self, i, image):
        """Store dataset index ``i``'s decoded image (numpy or tensor, host or device).  -> False when
        it does not fit; True once resident (a second insert is a no-op).  A shape other than the
        JSON's height / width raises: the loader samples from the JSON sizes before any decode."""
        i = int(i)
        t = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
        h, w = self.sizes[i]
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"yms: expected an HWC uint8 RGB image, got {tuple(t.shape)} {t.dtype}")
        if (t.shape[0], t.shape[1]) != (h, w):
            raise ValueError(f"yms: image {i} decodes to {t.shape[0]}x{t.shape[1]}, its annotation file says {h}x{w}")
        if self._res[i]:
            return True
        nbytes = h * w * 3
        at = self._place(nbytes)
        if at is None:
            return False
        c, off = at
        buf, base = self._chunks[c][0], self._chunks[c][1]
        view = buf[base + off:base + off + nbytes].view(h, w, 3)
        if self.device.type == "cuda" and t.device.type != "cuda":
            t = t.contiguous().pin_memory()
        view.copy_(t, non_blocking=True)
        self._where[i] = (c, off)
        self._slots[i] = _Slot(buf.data_ptr() + base + off, h, w)
        self._res[i] = 1
        return True

    def image(self, i):
        """Zero-copy [h, w, 3] uint8 view of a resident image."""
        c, off = self._where[int(i)]
        h, w = self.sizes[int(i)]
        buf, base = self._chunks[c][0], self._chunks[c][1]
        return buf[base + off:base + off + h * w * 3].view(h, w, 3)

    def slot(self, i):
        try:
            return self._slots[i]
        except KeyError:
            raise KeyError(f"yms: image {i} is neither resident nor part of the batch") from None

    def fill(self, ds, indices=None, num_workers=0):
        """Decode (in ``num_workers`` DataLoader workers) and insert (here) the given dataset indices,
        all by default, until one does not fit.  -> the number inserted."""
        idx = [int(i) for i in (range(len(ds)) if indices is None else indices)]
        idx = [i for i in dict.fromkeys(idx) if not self._res[i]]
        loader = torch.utils.data.DataLoader(_Decoder(ds, idx), batch_size=None, shuffle=False,
                                             num_workers=num_workers)
        n = 0
        for i, im in loader:
            if not self.insert(int(i), im):
                break
            n += 1
        return n


class CachedCOCODataset(D.COCODataset):
    """COCODataset for ``collate_cached``: ``__getitem__`` -> (source dataset indices, plan, {index:
    decoded image} for the sources not yet resident).  It draws from ``sample_rng`` in exactly
    COCODataset's order (the loads there draw nothing), so the same seed gives the same plans; source
    sizes come from the JSON.  ``resident`` is the cache's shared-memory flag tensor (None: decode
    everything) -- workers read only that and never touch the GPU."""

    def __init__(self, *args, resident=None, **kw):
        super().__init__(*args, **kw)
        if self.letterbox:
            raise NotImplementedError("yms: the cached loader covers training batches only")
        self.resident = resident

    def size(self, idx):
        info = self.imgs[self.image_ids[idx]]
        return int(info["height"]), int(info["width"])

    def _decode(self, idx):
        image = self._load(idx)[0]
        if tuple(image.shape[:2]) != self.size(idx):
            raise ValueError(f"yms: image {idx} decodes to {image.shape[0]}x{image.shape[1]}, "
                             f"its annotation file says {self.size(idx)[0]}x{self.size(idx)[1]}")
        return image

    def _cached_layer(self, rng, idxs, srcs):
        base = len(srcs)
        srcs += [int(i) for i in idxs]
        ly = D.sample_mosaic(rng, self.transform_params, [self.size(i) for i in srcs[base:]], self.img_h, self.img_w)
        for t in ly.tiles:
            t.src += base
        return ly

    def __getitem__(self, idx):
        if torch.is_tensor(idx):
            idx = idx.item()
        if not isinstance(idx, int):
            raise TypeError(f"Index should be an integer, got {type(idx).__name__} instead.")
        rng = self.sample_rng(idx)
        tp = self.transform_params
        srcs = []
        if self.mosaic and self.is_train and tp.get("mosaic", 0) > 0 and rng.random() < tp["mosaic"]:
            layers = [self._cached_layer(rng, [idx, *rng.integers(0, len(self), 3)], srcs)]
            r = 1.0
            if tp.get("mixup", 0) > 0 and rng.random() < tp["mixup"]:
                layers.append(self._cached_layer(rng, rng.integers(0, len(self), 4), srcs))
                r = rng.beta(32.0, 32.0)
            plan = D.MosaicPlan(layers, r)
        else:
            srcs.append(idx)
            h0, w0 = self.size(idx)
            plan = D.sample_augmentation(rng, tp, h0, w0, self.img_h, self.img_w, self.is_train)
        res = None if self.resident is None else self.resident.numpy()     # the shared bytes, cheap to index
        images = {i: self._decode(i) for i in dict.fromkeys(srcs) if res is None or not res[i]}
        return srcs, plan, images


def batch_tables(batch, cache, img_size, transient=None):
    """The host half of ``collate_cached``: (MosImage records, tile table, layer table, M_cap) of a
    batch whose sources are arena slots or, for the indices in ``transient``, the given tensors."""
    H, W = img_size
    transient = transient or {}
    rec = (D.MosImage * len(batch))()
    for b, (srcs, plan, _) in enumerate(batch):
        if plan.frame != (W, H):
            raise ValueError("yms: plan does not produce the batch size")
        rec[b] = D.mosaic_struct(plan, [transient[i] if i in transient else cache.slot(i) for i in srcs])
    tiles, layers, m_cap = target_tables([(srcs, plan) for srcs, plan, _ in batch], cache.ann_offsets)
    return rec, tiles, layers, m_cap


def collate_cached(batch, cache, img_size, device, dtype=torch.float32, mean=D.IMAGENET_MEAN, std=D.IMAGENET_STD):
    """[(sources, plan, {index: decoded image})] of a CachedCOCODataset -> ([B, 3, H, W] batch, padded
    [M_cap, 6] targets) with two launches, yms_mosaic_normalize and yms_box_targets, and no host sync.
    Images that came decoded are uploaded as collate_to_gpu uploads them and inserted into the cache
    while room remains (the first epoch is the fill); the rest are read from the arena.  The three
    tables go up in one copy from pinned memory (torch's pinned caching allocator keeps the block
    until the copy has run)."""
    dev = torch.device(device)
    if dev.type != "cuda" or cache.device.type != "cuda":
        raise RuntimeError("yms: collate_cached runs on a ROCm GPU cache only (no CPU fallback)")
    if not batch:
        raise ValueError("yms: empty batch")
    _check_layouts()
    H, W = img_size
    stream = torch.cuda.current_stream(dev)
    pending = {}
    for _, _, images in batch:
        for i, im in images.items():
            if not cache.is_resident(i) and i not in pending:
                pending[i] = im
    transient = {}
    if pending:
        keys = list(pending)
        for i, t in zip(keys, D.to_device([pending[i] for i in keys], dev)):
            if not cache.insert(i, t):
                transient[i] = t
            t.record_stream(stream)
    n = len(batch)
    rec, tiles, layers, m_cap = batch_tables(batch, cache, img_size, transient)
    # one pinned block: [records | tiles | layers], each part 16-byte aligned
    parts = [np.frombuffer(rec, np.uint8), tiles.view(np.uint8), layers.view(np.uint8)]
    offs, total = [], 0
    for p in parts:
        offs.append(total)
        total += -(-p.nbytes // 16) * 16
    stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    sv = stage.numpy()
    for o, p in zip(offs, parts):
        sv[o:o + p.nbytes] = p
    tab = stage.to(dev, non_blocking=True)
    base = tab.data_ptr()
    x = torch.empty((n, 3, H, W), dtype=dtype, device=dev)
    targets = torch.empty((m_cap, 6), dtype=torch.float32, device=dev)
    sp = stream.cuda_stream
    L.call("yms_mosaic_normalize", L.dtype_code(dtype), n, base + offs[0], H, W, (ctypes.c_float * 3)(*mean),
           (ctypes.c_float * 3)(*std), x.data_ptr(), sp)
    L.call("yms_box_targets", len(tiles), base + offs[1], len(layers), base + offs[2], cache.boxes.data_ptr(),
           cache.labels.data_ptr(), cache.nann, m_cap, targets.data_ptr(), sp)
    tab.record_stream(stream)
    return x, targets
