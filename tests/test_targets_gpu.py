"""yms_box_targets (csrc/targets.hip) against its float64 restatement (tests/targets_ref.py), bit for
bit, ignored rows included, over a NaN-poisoned output buffer; and the three fused losses on the
padded tensor against the compacted one."""
import functools

import numpy as np
import pytest
import torch

import targets_cases as TC
import targets_ref as R
from yms import cache as C
from yolov8.tools.dsl_loss import dsl_loss
from yolov8.tools.loss import det_loss
from yolov8.tools.tal_loss import tal_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _device_rows(case):
    boxes = torch.from_numpy(case["boxes"]).to(DEV)
    labels = torch.from_numpy(case["labels"]).to(DEV)
    out = torch.full((case["m_cap"], 6), float("nan"), dtype=torch.float32, device=DEV)
    got = C.box_targets(case["tiles"], case["layers"], case["m_cap"], boxes, labels, out=out)
    assert got is out
    return out


@pytest.mark.parametrize("m_cap", [0, 1, 255, 256, 257])
def test_device_rows_equal_the_restatement(m_cap):
    """B = 3 (plain with eight stages, Mosaic, MixUp), 64 x 96 output; 256 rows are one thread block, so
    255 / 256 / 257 put the last row on either side of its edge."""
    case = TC.make_batch(5, m_cap, eight=True)
    assert len(case["samples"][0][1].stages) == 8
    ref = R.box_targets(case["tiles"], case["layers"], m_cap, case["boxes"], case["labels"])
    out = _device_rows(case).cpu()
    assert out.shape == (m_cap, 6) and not torch.isnan(out).any()      # every row written
    kept = int((ref[:, 0] >= 0).sum())
    print(f"M_cap {m_cap}: {kept} kept, {m_cap - kept} ignored")
    if m_cap >= 255:
        assert 0 < kept < m_cap and set(ref[ref[:, 0] >= 0][:, 0]) == {0.0, 1.0, 2.0}
    assert torch.equal(out, torch.from_numpy(ref))


@functools.lru_cache(maxsize=None)
def _loss_inputs():
    case = TC.loss_batch()
    padded = _device_rows(case)
    compact = C.compact_targets(padded)
    ref = R.box_targets(case["tiles"], case["layers"], case["m_cap"], case["boxes"], case["labels"])
    assert torch.equal(padded.cpu(), torch.from_numpy(ref)) and torch.equal(compact.cpu(), torch.from_numpy(R.compact(ref)))
    M = compact.shape[0]
    assert 0 < M < padded.shape[0] and set(compact[:, 0].tolist()) == {0.0, 1.0} and compact[:, 1].max() <= 2
    g = torch.Generator().manual_seed(0)
    maps = [torch.randn(2, 64 + 3, 64 // s, 64 // s, generator=g).to(DEV) for s in (8, 16, 32)]
    return padded, compact, maps


@pytest.mark.parametrize("loss", [det_loss, tal_loss, dsl_loss])
def test_losses_ignore_the_padding(loss):
    """B = 2, nc = 3, 64 x 64 input, random maps: loss and gradients with the padded tensor are those
    with compact_targets of it, bit for bit."""
    padded, compact, maps = _loss_inputs()
    a, ga = loss(maps, padded, 3, (64, 64))
    b, gb = loss(maps, compact, 3, (64, 64))
    assert torch.isfinite(a).all() and float(a[0]) > 0
    assert any(bool(g.any()) for g in ga)
    assert torch.equal(a, b)
    assert all(torch.equal(x, y) for x, y in zip(ga, gb))
