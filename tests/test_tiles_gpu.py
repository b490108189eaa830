"""Tiled inference on the GPU: yms_tile_merge (csrc/tile.hip) bit for bit against tests/tiles_ref.py --
both access widths, ragged and out-of-range slots, the strict suppression comparisons at one fp32 ulp,
the item-stride loop -- predict_tiles' inputs against letterbox_normalize on the same crops, and
detect_tiles end to end at toy size (YOLOv8-n, 3 classes, tile 64: A = 64 + 16 + 4 = 84 rows).

Every comparison is exact: the merge's arithmetic is four separately rounded fp32 operations per box
that the restatement replays one per line, and runs of the model are compared at equal batch size only
(batch-invariance of the forward is not claimed)."""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

import detect_ref as R
import tiles_ref as TR
from yms import _lib as L
from yms import data as D
from yms import ops, tiles

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = float("inf")
A, T, N, S = 21, 5, 2, 3
FIELDS = ("tile", "gain_x", "gain_y", "pad_x", "pad_y", "lo_x", "lo_y", "hi_x", "hi_y")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def records(tab):
    """tiles_ref's [n, S, 9] table -> device bytes of the yms_tile_slot records."""
    rec = np.zeros(tab.shape[:2], tiles.SLOT_DTYPE)
    for k, name in enumerate(FIELDS):
        rec[name] = tab[..., k]
    return torch.from_numpy(rec.reshape(-1).view(np.uint8).copy()).cuda()


def gpu_merge(pred, tab):
    p = pred if isinstance(pred, torch.Tensor) else torch.tensor(pred).cuda()
    out = tiles.merge_slots(p, records(tab), *tab.shape[:2])
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------
# 1. the merge
# ------------------------------------------------------------------------------------------
# image 0: three live slots (tiles 3, 0, 4), every kind of bound; image 1: one slot, two empty
TABLE = np.array([[[3, 1, 1, -52, -104, 4, 6, 60, 58], [0, 0.4, 0.4, 0, 12, -INF, -INF, INF, INF],
                   [4, 2, 2, -76, 0, 3.5, -INF, INF, 61.25]],
                  [[1, 1, 1, 0, 0, -INF, 2, 62, INF], [-1, 1, 1, 0, 0, -INF, -INF, INF, INF],
                   [-1, 1, 1, 0, 0, -INF, -INF, INF, INF]]], np.float64)
TABLE.setflags(write=False)


@functools.lru_cache(maxsize=None)
def merge_case(nc, rows=A, ntiles=T):
    """Boxes in a 64-pixel tile input: centres anywhere, sides 1..30, so some cross each bound."""
    rng = np.random.default_rng(nc)
    p = np.zeros((ntiles, rows, 4 + nc), F32)
    p[..., :2] = rng.uniform(0, 64, (ntiles, rows, 2))
    p[..., 2:4] = rng.uniform(1, 30, (ntiles, rows, 2))
    p[..., 4:] = rng.uniform(0, 1, (ntiles, rows, nc))
    if rows > 7 and ntiles > 4:
        p[3, 2, 4 + nc - 1] = np.nan
        p[0, 5, 4] = np.inf
        p[4, 7, :4] = (np.nan, 30, 10, 10)                    # a NaN coordinate: copied, the row kept
        p[1, 3, 1] = -7.25
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("nc", [3, 4, 80])
def test_merge_bit_for_bit(nc):
    """nc = 3: rows of 7 floats, the scalar walk; 4 and 80: the float4 walk (80: two chunks per slot)."""
    pred = merge_case(nc)
    want = TR.merge(pred, TABLE)
    got = gpu_merge(pred, TABLE)
    assert got.shape == want.shape == (N, S * A, 4 + nc)
    cut = (want[0, :, 4:] == -1).all(-1)
    print("nc", nc, "suppressed rows per live slot", [int(cut[s * A:(s + 1) * A].sum()) for s in range(S)])
    assert 0 < cut[:A].sum() < A and cut[A:2 * A].sum() == 0 and 0 < cut[2 * A:].sum() < A
    assert np.isnan(want[0, 2 * A + 7, 0]) and not cut[2 * A + 7]
    assert np.array_equal(bits(got), bits(want))
    # ragged: image 1's two empty slots are exactly (0, 0, 0, 0, -1, ...)
    empty = np.concatenate([np.zeros(4, F32), np.full(nc, -1, F32)])
    assert np.array_equal(bits(got[1, A:]), bits(np.tile(empty, (2 * A, 1))))
    # a row that is not suppressed carries its scores as bits (NaN included)
    assert np.array_equal(bits(got[0, A:2 * A, 4:]), bits(pred[0, :, 4:]))


def test_merge_misaligned_base():
    """nc = 4 from a view that starts 4 bytes into a larger buffer: the scalar walk on 8-float rows."""
    pred = merge_case(4)
    flat = torch.zeros(pred.size + 1, device="cuda")
    flat[1:] = torch.tensor(pred).cuda().reshape(-1)
    p = flat[1:].view(pred.shape)
    assert p.data_ptr() % 16 == 4 and p.is_contiguous()
    assert np.array_equal(bits(gpu_merge(p, TABLE)), bits(TR.merge(pred, TABLE)))


@pytest.mark.parametrize("nc", [3, 4])
def test_merge_tile_index_outside_pred(nc):
    """tile = -1, T, 2^30 and a large negative index give the empty-slot rows; the live neighbour is
    untouched.  The index is device data: the kernel checks it and reads nothing of pred for it."""
    pred = merge_case(nc)
    tab = np.array(TABLE)
    tab[0, 0, 0], tab[0, 2, 0], tab[1, 0, 0], tab[1, 1, 0] = T, 2 ** 30, -(2 ** 31), -1
    want = TR.merge(pred, tab)
    got = gpu_merge(pred, tab)
    empty = np.concatenate([np.zeros(4, F32), np.full(nc, -1, F32)])
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got[0, :A]), bits(np.tile(empty, (A, 1))))
    assert np.array_equal(bits(got[0, 2 * A:]), bits(np.tile(empty, (A, 1))))
    assert np.array_equal(bits(got[1]), bits(np.tile(empty, (S * A, 1))))
    assert (got[0, A:2 * A, 4:] != -1).any()


@pytest.mark.parametrize("nc", [3, 4])
def test_suppression_is_strict_to_one_ulp(nc):
    """Bounds lo (4, 6), hi (60, 58).  Per side one box whose side equals the bound (kept) and one whose
    centre is one fp32 ulp further out (the half side 10 is exact, so the side is one ulp of the centre
    beyond the bound: suppressed).  Then the same boxes with infinite bounds, boxes of huge and infinite
    size under infinite bounds, and a NaN coordinate under finite ones: all kept."""
    down, up = F32(-INF), F32(INF)
    boxes = [(14, 30, 20, 20), (np.nextafter(F32(14), down), 30, 20, 20),
             (30, 16, 20, 20), (30, np.nextafter(F32(16), down), 20, 20),
             (50, 30, 20, 20), (np.nextafter(F32(50), up), 30, 20, 20),
             (30, 48, 20, 20), (30, np.nextafter(F32(48), up), 20, 20),
             (30, 30, 1e30, 1e30), (30, 30, INF, 20), (np.nan, 30, 20, 20), (30, 30, 20, np.nan)]
    rng = np.random.default_rng(1)
    pred = np.zeros((1, len(boxes), 4 + nc), F32)
    pred[0, :, :4] = boxes
    pred[0, :, 4:] = rng.uniform(0.1, 1, (len(boxes), nc))
    tab = np.array([[[0, 1, 1, 0, 0, 4, 6, 60, 58], [0, 1, 1, 0, 0, -INF, -INF, INF, INF]]], np.float64)
    want = TR.merge(pred, tab)
    got = gpu_merge(pred, tab)
    assert np.array_equal(bits(got), bits(want))
    m = len(boxes)
    kept = (got[0, :, 4:] != -1).all(-1)
    assert kept[:m].tolist() == [True, False] * 4 + [False, False, True, True]
    assert kept[m:].all()                                      # infinite bounds never suppress
    assert np.array_equal(bits(got[0, m:, 4:]), bits(pred[0, :, 4:]))
    assert np.isnan(got[0, 10, 0]) and np.isnan(got[0, 11, 3])  # the NaN is copied through the un-map


@pytest.mark.parametrize("nc", [3, 8])
def test_merge_item_stride_loop(nc):
    """More (slot, chunk) work items than the launch has blocks, so every block walks more than one:
    A = 2 makes one chunk per slot, and n * S exceeds yms_tile_merge_max_blocks() by a few."""
    cap = L.lib().yms_tile_merge_max_blocks()
    n, s, rows, nt = 2, cap // 2 + 3, 2, 7
    assert n * s > cap
    rng = np.random.default_rng(nc)
    pred = merge_case(nc, rows, nt)
    tab = np.zeros((n, s, 9), np.float64)
    tab[..., 0] = rng.integers(-1, nt, (n, s))
    tab[..., 1:3] = rng.choice([0.5, 1.0, 2.0], (n, s, 1))
    tab[..., 3:5] = -rng.integers(0, 2000, (n, s, 2))
    tab[..., 5:7] = rng.choice([-INF, 4.0], (n, s, 2))
    tab[..., 7:9] = rng.choice([INF, 60.0], (n, s, 2))
    got = gpu_merge(pred, tab)
    assert got.shape == (n, s * rows, 4 + nc)
    assert np.array_equal(bits(got), bits(TR.merge(pred, tab)))


@pytest.mark.parametrize("nc", [3, 8])
def test_merge_several_chunks_per_slot(nc):
    """A = 100: 700 single-float units (3 chunks) at nc = 3, 300 float4 units (2 chunks) at nc = 8; the
    last chunk of a slot is partly idle."""
    pred = merge_case(nc, 100, T)
    assert np.array_equal(bits(gpu_merge(pred, TABLE)), bits(TR.merge(pred, TABLE)))


def test_merge_argument_errors():
    p = torch.zeros(T, A, 7, device="cuda")
    tab = records(np.array(TABLE))
    o = torch.empty(N, S * A, 7, device="cuda")
    fn, st = L.lib().yms_tile_merge, L.stream_ptr(p.device)
    ok = dict(n=N, S=S, A=A, nc=3, T=T, pred=p.data_ptr(), table=tab.data_ptr(), out=o.data_ptr())
    call = lambda **kw: fn(*{**ok, **kw}.values(), st)
    assert call() == 0
    for kw in (dict(n=0), dict(n=65536), dict(S=0), dict(A=0), dict(nc=0), dict(T=0), dict(pred=None), dict(table=None),
               dict(out=None), dict(pred=p.data_ptr() + 2), dict(table=tab.data_ptr() + 1), dict(out=o.data_ptr() + 2),
               dict(A=2 ** 27, nc=12),                         # A * (4 + nc) = 2^31
               dict(S=2 ** 16, A=2 ** 10, nc=32)):             # S * A * nc = 2^31
        assert call(**kw) == 1, kw                             # YMS_ERR_INVALID, nothing launched
    assert L.lib().yms_status_string(1)
    torch.cuda.synchronize()
    for bad in (dict(n=0), dict(S=0), dict(n=N + 1)):
        with pytest.raises(ValueError):
            tiles.merge_slots(p, tab, **{**dict(n=N, S=S), **bad})
    with pytest.raises(ValueError):
        tiles.merge_slots(p.double(), tab, N, S)
    with pytest.raises(ValueError):
        tiles.merge_slots(p[:, :, :4], tab, N, S)


# ------------------------------------------------------------------------------------------
# 2. tile drawing, 3. end to end
# ------------------------------------------------------------------------------------------
TILE = 64
DET_KW = dict(conf=0.05, iou=0.6, multi_label=True, max_det=20)


class Spy(torch.nn.Module):
    """The model, recording every input batch it is given."""

    def __init__(self, model):
        super().__init__()
        self.model, self.head, self.seen = model, model.head, []

    def forward(self, x):
        self.seen.append(x)
        return self.model(x)


@functools.lru_cache(maxsize=None)
def toy_model():
    from yolov8.yolov8 import YOLOv8
    torch.manual_seed(0)
    model = YOLOv8("n", 3).cuda().eval()
    model.head.stride = torch.tensor([8.0, 16.0, 32.0])
    with torch.no_grad():
        for branch in model.head.cls:                         # random weights clear no threshold: lift the class biases
            branch[2].bias.fill_(-2.0)
    return model


def image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_tile_inputs_are_the_crops():
    """150 x 200 (windows 0, 52, 86 by 0, 52, 104, 136) and a short 40 x 100 image (0, 36), no full
    view, tile_batch 5: 12 + 2 inputs in 3 chunks.  An interior window's input is letterbox_normalize of the
    torch slice of that window, bit for bit; a short image's input is that in its valid rows and the
    normalised fill below; the padding inputs that fill up the last chunk do not exist in the table."""
    ims = [image(150, 200, 1), image(40, 100, 2)]
    dev = D.to_device(ims, "cuda")
    spy = Spy(toy_model()).eval()
    t = tiles.predict_tiles(spy, dev, tile=TILE, full_view=False, tile_batch=5)
    assert [tuple(x.shape) for x in spy.seen] == [(5, 3, TILE, TILE)] * 3
    assert tuple(t.pred.shape) == (15, 84, 7) and t.pred.dtype == torch.float32 and t.slots == 12
    assert t.windows[0] == TR.slice_grid(150, 200, TILE) and t.windows[1] == TR.slice_grid(40, 100, TILE)
    assert t.table_host["tile"].tolist() == [list(range(12)), [12, 13] + [-1] * 10]
    assert np.array_equal(t.table.cpu().numpy(), t.table_host.reshape(-1).view(np.uint8))
    x = torch.cat(spy.seen).cpu().numpy()
    k = t.windows[0].index((52, 52, 116, 116))                # touches no border
    want, _ = D.letterbox_normalize([dev[0][52:116, 52:116]], (TILE, TILE))
    assert np.array_equal(bits(x[k]), bits(want[0].cpu().numpy()))
    for j, (x0, y0, x1, y1) in enumerate(t.windows[1]):
        lb, fr = D.letterbox_normalize([dev[1][y0:y1, x0:x1]], (TILE, TILE))
        lb = lb[0].cpu().numpy()
        assert fr.host[0, :4].tolist() == [1, 1, 0, 12]       # the letterbox centres the 40 rows
        assert np.array_equal(bits(x[12 + j][:, :40]), bits(lb[:, 12:52]))
        assert np.array_equal(bits(x[12 + j][:, 40:]), bits(np.broadcast_to(lb[:, :1, :1], (3, 24, TILE))))


def test_padding_inputs_are_blank():
    """One 64 x 64 image at tile_batch 3: inputs 1 and 2 of the chunk are all fill."""
    dev = D.to_device([image(64, 64, 3)], "cuda")
    spy = Spy(toy_model()).eval()
    t = tiles.predict_tiles(spy, dev, tile=TILE, full_view=False, tile_batch=3)
    (x,) = spy.seen
    assert tuple(x.shape) == (3, 3, TILE, TILE) and t.table_host["tile"].tolist() == [[0]]
    lb, _ = D.letterbox_normalize([dev[0][:8]], (TILE, TILE))  # its row 0 is padding: the normalised fill
    fill = lb[0, :, :1, :1].expand(3, TILE, TILE)
    assert torch.equal(x[1], fill) and torch.equal(x[2], fill) and not torch.equal(x[0], fill)


def check_det(det, want):
    assert np.array_equal(det.counts.cpu().numpy(), want["count"])
    assert np.array_equal(det.candidates.cpu().numpy(), want["candidates"])
    assert np.array_equal(det.anchors.cpu().numpy(), want["anchor"])
    assert np.array_equal(det.labels.cpu().numpy(), want["det"][..., 5].astype(np.int32))
    assert np.array_equal(bits(det.scores.cpu().numpy()), bits(want["det"][..., 4]))
    assert np.array_equal(bits(det.boxes.cpu().numpy()), bits(want["det"][..., :4]))


def test_single_tile_equals_plain_detect():
    """(a) one 64 x 64 image, no full view: tiling is the identity.  Both runs at batch 1."""
    model = toy_model()
    dev = D.to_device([image(64, 64, 4)], "cuda")
    with torch.no_grad():
        x, fr = D.letterbox_normalize(dev, (TILE, TILE))
        want = ops.detect(model(x).float(), frames=fr, **DET_KW)
    det = tiles.detect_tiles(model, dev, tile=TILE, overlap=0, full_view=False, tile_batch=1, **DET_KW)
    assert int(want.counts[0]) > 0
    for k in ("counts", "candidates", "anchors", "labels", "scores", "boxes"):
        assert torch.equal(getattr(det, k), getattr(want, k)), k


@functools.lru_cache(maxsize=None)
def halves():
    """(b) a 64 x 128 image of two different halves -> (device image, model output on the two halves
    as one batch of 2 [2, 84, 7] numpy)."""
    im = np.concatenate([image(64, 64, 5), image(64, 64, 6)], 1)
    dev = D.to_device([im], "cuda")
    with torch.no_grad():
        x, _ = D.letterbox_normalize([dev[0][:, :64], dev[0][:, 64:]], (TILE, TILE))
        pred = toy_model()(x).float().cpu().numpy()
    pred.setflags(write=False)
    return dev, pred


def test_two_halves():
    dev, pred = halves()
    model = toy_model()
    t = tiles.predict_tiles(model, dev, tile=TILE, overlap=0, full_view=False, tile_batch=2)
    assert t.windows == [[(0, 0, 64, 64), (64, 0, 128, 64)]] and t.slots == 2
    assert np.array_equal(bits(t.pred.cpu().numpy()), bits(pred))
    merged = tiles.merge_tiles(t).cpu().numpy()
    want = TR.merge(pred, TR.table(TR.slots([(64, 128)], TILE, 0, 1.0, False)))
    assert merged.shape == (1, 168, 7) and np.array_equal(bits(merged), bits(want))
    assert np.array_equal(merged[0, :84], pred[0])
    assert np.array_equal(merged[0, 84:, 0], pred[1, :, 0] + F32(64))       # the right half, 64 further
    assert np.array_equal(merged[0, 84:, 1:], pred[1, :, 1:])
    ident = F32([[1, 1, 0, 0, 128, 64]])
    ref = R.detect(want, DET_KW["conf"], DET_KW["iou"], True, False, None, DET_KW["max_det"], 30000, ident)
    print("candidates", ref["candidates"], "count", ref["count"])
    assert ref["count"][0] > 0
    det = tiles.detect_tiles(model, dev, tile=TILE, overlap=0, full_view=False, tile_batch=2, **DET_KW)
    check_det(det, ref)
    with pytest.raises(ValueError):
        tiles.detect_tiles(model, dev, tile=TILE, frames=None)
    # edge = 0 on the same image: rows whose box sticks out over the cut at x = 64 are gone, no other
    te = tiles.predict_tiles(model, dev, tile=TILE, overlap=0, full_view=False, edge=0, tile_batch=2)
    we = TR.merge(pred, TR.table(TR.slots([(64, 128)], TILE, 0, 1.0, False, 0)))
    ge = tiles.merge_tiles(te).cpu().numpy()
    assert np.array_equal(bits(ge), bits(we))
    assert np.array_equal(bits(ge[..., :4]), bits(merged[..., :4]))
    gone = (ge[0, :, 4:] == -1).all(-1)
    right_side, left_side = pred[0, :, 0] + F32(0.5) * pred[0, :, 2], pred[1, :, 0] - F32(0.5) * pred[1, :, 2]
    print("rows suppressed by edge=0:", int(gone.sum()), "of", gone.size)
    assert 0 < gone.sum() < gone.size
    assert np.array_equal(gone, np.concatenate([right_side > 64, left_side < 0]))


def test_two_images_full_view():
    """(c) 100 x 150 and 64 x 64 in one call with the full view: S = 1 + 6 and 1 + 1 slots."""
    model = toy_model()
    shapes = [(100, 150), (64, 64)]
    dev = D.to_device([image(h, w, 7 + h) for h, w in shapes], "cuda")
    t = tiles.predict_tiles(model, dev, tile=TILE, overlap=0.25, full_view=True, edge=2, tile_batch=3)
    sl = TR.slots(shapes, TILE, 0.25, 1.0, True, 2)
    tab = TR.table(sl)
    assert t.slots == 7 and [len(s) for s in sl] == [7, 2] and tuple(t.pred.shape) == (9, 84, 7)
    pred = t.pred.cpu().numpy()
    want = TR.merge(pred, tab)
    assert np.array_equal(bits(tiles.merge_tiles(t).cpu().numpy()), bits(want))
    ident = F32([[1, 1, 0, 0, w, h] for h, w in shapes])
    ref = R.detect(want, DET_KW["conf"], DET_KW["iou"], True, False, None, DET_KW["max_det"], 30000, ident)
    det = ops.detect(tiles.merge_tiles(t), frames=torch.tensor(ident).cuda(), **DET_KW)
    check_det(det, ref)
    assert (ref["count"] > 0).all()
    for b, (h0, w0) in enumerate(shapes):
        k = int(det.counts[b])
        bx = det.boxes[b, :k]
        assert (bx >= 0).all() and (bx[:, [0, 2]] <= w0).all() and (bx[:, [1, 3]] <= h0).all()
        for a, lab, sc in zip(det.anchors[b, :k].tolist(), det.labels[b, :k].tolist(), det.scores[b, :k].tolist()):
            slot, window, anchor = t.locate(b, a)
            assert slot < len(sl[b]) and window == sl[b][slot][2] and (window is None) == (slot == 0)
            assert sc == pred[int(tab[b, slot, 0]), anchor, 4 + lab]
    with pytest.raises(IndexError):
        t.locate(1, 2 * 84)                                     # image 1 has two slots


def test_existing_detect_is_untouched():
    """detect on an unrelated prediction tensor gives the same bytes before and after yms.tiles is
    imported anew and used (edge=None, the two halves)."""
    rng = np.random.default_rng(11)
    p = np.zeros((2, 300, 7), F32)
    p[..., :2] = rng.uniform(0, 320, (2, 300, 2))
    p[..., 2:4] = rng.uniform(4, 120, (2, 300, 2))
    p[..., 4:] = rng.uniform(0, 1, (2, 300, 3))
    d = torch.tensor(p).cuda()
    fn = ops.detect
    before = ops.detect(d, **DET_KW)
    mod = importlib.reload(importlib.import_module("yms.tiles"))
    dev, _ = halves()
    assert int(mod.detect_tiles(toy_model(), dev, tile=TILE, overlap=0, full_view=False, tile_batch=2, **DET_KW).counts[0]) > 0
    after = ops.detect(d, **DET_KW)
    assert ops.detect is fn and int(before.counts.sum()) > 0
    for k in ("counts", "candidates", "anchors", "labels", "scores", "boxes"):
        assert getattr(before, k).cpu().numpy().tobytes() == getattr(after, k).cpu().numpy().tobytes(), k


def test_merge_tiles_does_not_sync():
    """After a warm-up call, merge_tiles + detect make no synchronising call."""
    dev, _ = halves()
    t = tiles.predict_tiles(toy_model(), dev, tile=TILE, overlap=0, full_view=False, tile_batch=2)
    fr = torch.tensor([[1, 1, 0, 0, 128, 64]], dtype=torch.float32).cuda()
    ops.detect(tiles.merge_tiles(t), frames=fr, **DET_KW)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        det = ops.detect(tiles.merge_tiles(t), frames=fr, **DET_KW)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert int(det.counts.sum()) > 0
