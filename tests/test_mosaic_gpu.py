"""yms_mosaic_normalize (csrc/preprocess.hip mosaic_normalize_kernel via yms.data.mosaic_normalize)
against its numpy fp32 replay (tests/mosaic_ref.py), against augment_normalize on plain plans (bit for
bit), and the COCODataset(mosaic=True) -> collate_to_gpu path.  The gate is the augmentation kernel's
(tests/test_data_gpu.py): fewer than 1e-3 of the values differ by more than 1e-6 and none by more
than two intensity levels; bf16 against the bf16-rounded replay."""
import functools

import numpy as np
import pytest
import torch

import mosaic_ref as MR
from yms import data as D

pytestmark = pytest.mark.gpu
MEAN, STD = D.IMAGENET_MEAN, D.IMAGENET_STD
LEVEL = 1.0 / (255.0 * min(STD))                      # one intensity step after Normalize
AUG_FULL = {"hsv_h": 0.015, "hsv_s": 0.7, "hsv_v": 0.4, "degrees": 20.0, "translate": 0.1, "scale": 0.5,
            "shear": 8.0, "perspective": 0.08, "flipud": 0.5, "fliplr": 0.5}
H, W, N = 96, 128, 8
POOL = [(17, 200), (333, 517), (1, 1), (64, 64), (250, 250), (90, 120), (300, 40), (120, 333)]
SEED = 0                                              # chosen on the CPU for the coverage asserted below


def make_batch(seed):
    """N mosaic samples over a pool of random images: (image lists, plans); MixUp with probability 0.5."""
    rng = np.random.default_rng(seed)
    pool = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in POOL]
    samples, plans = [], []
    for _ in range(N):
        layers, images = [], []
        for _ in range(2 if rng.random() < 0.5 else 1):
            idx = [int(i) for i in rng.integers(0, len(pool), 4)]
            ly = D.sample_mosaic(rng, AUG_FULL, [POOL[i] for i in idx], H, W)
            for t in ly.tiles:
                t.src += len(images)
            images += [pool[i] for i in idx]
            layers.append(ly)
        plans.append(D.MosaicPlan(layers, rng.beta(32.0, 32.0) if len(layers) > 1 else 1.0))
        samples.append(images)
    return samples, plans


def coverage(plans, sels):
    """What the batch exercises, from the plans and the restatement's per-pixel tile choice."""
    layers = [ly for p in plans for ly in p.layers]
    share = [max(float((s == k).mean()) for ss in sels for s in ss) for k in range(4)]
    return {
        "every tile position > 1% of some output": min(share) > 0.01,
        "visible fill": any((s == -1).any() for ss in sels for s in ss),
        "tile cropped by the canvas edge": any(t.rect[2] - t.rect[0] < t.nw or t.rect[3] - t.rect[1] < t.nh
                                               for ly in layers for t in ly.tiles),
        "upscaled tile": any(t.nw > t.w and t.nh > t.h for ly in layers for t in ly.tiles),
        "1x1 source sampled": any(t.h == 1 and t.w == 1 and (s == k).any() for p, ss in zip(plans, sels)
                                  for ly, s in zip(p.layers, ss) for k, t in enumerate(ly.tiles)),
        "perspective, flips, hsv": {"perspective", "fliplr", "flipud", "hsv"} <= {a for p in plans for a in p.applied},
        "three MixUp outputs": sum(len(p.layers) > 1 for p in plans) >= 3,
    }


@functools.lru_cache(maxsize=None)
def reference():
    """The batch, its restatement (computed once, shared, never modified) and its coverage."""
    samples, plans = make_batch(SEED)
    refs, sels = [], []
    for ims, pl in zip(samples, plans):
        layers, r = MR.record_of(pl, ims)
        ref, sel = MR.mosaic_normalize(layers, r, H, W, MEAN, STD, return_sel=True)
        ref.setflags(write=False)
        refs.append(ref)
        sels.append(sel)
    return samples, plans, refs, coverage(plans, sels)


def gate(out, ref, dtype, what):
    if dtype == torch.bfloat16:
        ref = torch.from_numpy(np.array(ref)).to(torch.bfloat16).float().numpy()
    diff = np.abs(out - ref)
    share = (diff > 1e-6).mean()
    print(what, "share > 1e-6:", share, "max:", diff.max())
    assert share < 1e-3, (what, share)
    assert diff.max() <= 2 * LEVEL, (what, diff.max())


def run(samples, plans, size, dtype):
    dev = [D.to_device(ims, "cuda") for ims in samples]
    return D.mosaic_normalize(dev, plans, size, MEAN, STD, dtype).float().cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mosaic_normalize_vs_restatement(dtype):
    samples, plans, refs, cov = reference()
    assert all(cov.values()), cov
    out = run(samples, plans, (H, W), dtype)
    assert out.shape == (N, 3, H, W)
    for i, pl in enumerate(plans):
        gate(out[i], refs[i], dtype, (i, pl.applied))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_plain_plans_equal_augment_normalize(dtype):
    """Plain AugPlans as degenerate records: the output of the kernel they had, bit for bit (the
    eight-size batch of test_augment_normalize_vs_restatement)."""
    rng = np.random.default_rng(11)
    sizes = [(480, 640), (333, 517), (64, 64), (17, 200), (640, 480), (250, 250), (90, 120), (300, 40)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    prng = np.random.default_rng(5)
    plans = [D.sample_augmentation(prng, AUG_FULL, h, w, 160, 192) for h, w in sizes]
    applied = set(a for p in plans for a in p.applied)
    assert {"hsv", "rotate", "shift", "scale", "shear", "perspective", "fliplr", "flipud"} <= applied, applied
    dev = D.to_device(imgs, "cuda")
    want = D.augment_normalize(dev, plans, (160, 192), MEAN, STD, dtype)
    got = D.mosaic_normalize(dev, plans, (160, 192), MEAN, STD, dtype)
    assert got.dtype == dtype and torch.equal(got, want)


def test_mixup_weight():
    samples, plans, refs, _ = reference()
    i = next(k for k, p in enumerate(plans) if len(p.layers) > 1)
    ims, pl = samples[i], plans[i]
    quarter = D.MosaicPlan(pl.layers, 0.25)
    layers, r = MR.record_of(quarter, ims)
    assert r == np.float32(0.25)
    ref = MR.mosaic_normalize(layers, r, H, W, MEAN, STD)
    assert np.abs(ref - refs[i]).max() > LEVEL            # the weight matters on this sample
    one, first = D.MosaicPlan(pl.layers, 1.0), D.MosaicPlan(pl.layers[:1])
    out = run([ims, ims, ims], [quarter, one, first], (H, W), torch.float32)
    gate(out[0], ref, torch.float32, "r = 0.25")
    # r = 1: b + 1 * (a - b) is a up to the two roundings of the blend, each at most half an ulp of a
    # value below 256 (2^-17), i.e. 1.6e-5 of a level-unit -> 2.7e-7 after Normalize's 1 / (255 std),
    # plus at most two ulps (2.4e-7 each below 4) where that moves the output's own roundings: < 1e-6,
    # the gate's "differs" threshold
    diff = np.abs(out[1] - out[2])
    print("r = 1: values not identical:", (diff > 0).mean(), "max:", diff.max())
    assert diff.max() <= 1e-6, diff.max()


def test_mosaic_dataset_to_gpu_batch(tmp_path, monkeypatch):
    """COCODataset(mosaic=True, mosaic 0.5, mixup 0.5) -> collate_to_gpu: a batch of mosaic and plain
    samples is ONE launch, every output is the restatement of its plan, targets are the host's."""
    from test_data_cpu import _coco
    ann = _coco(tmp_path, [(32, 48), (40, 40), (21, 57), (64, 30), (48, 48)])
    monkeypatch.setattr(torch, "initial_seed", lambda: 0)      # the main-process draw stream, whatever ran before
    ds = D.COCODataset(str(tmp_path), str(ann), dict(AUG_FULL, mosaic=0.5, mixup=0.5), True, (64, 96), 3, seed=0,
                       mosaic=True)
    batch = [ds[i % len(ds)] for i in range(6)]
    kinds = [len(p.layers) if isinstance(p, D.MosaicPlan) else 0 for _, _, p in batch]
    assert 0 in kinds and 1 in kinds and 2 in kinds, kinds        # plain, Mosaic and MixUp samples together
    calls = []
    real = D.L.call
    monkeypatch.setattr(D.L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    x, tg = D.collate_to_gpu(batch, (64, 96), "cuda")
    assert calls == ["yms_mosaic_normalize"], calls
    assert x.shape == (6, 3, 64, 96) and tg.device.type == "cuda" and tg.dim() == 2 and tg.shape[1] == 6
    out = x.cpu().numpy()
    for i, (ims, t, pl) in enumerate(batch):
        layers, r = MR.record_of(pl, ims)
        gate(out[i], MR.mosaic_normalize(layers, r, 64, 96, MEAN, STD), torch.float32, (i, pl.applied))
    _, _, t_host = D.collate_targets(batch)
    assert torch.equal(tg.cpu(), t_host) and t_host.shape[0] == sum(t.shape[0] for _, t, _ in batch)
