"""The weight gradient's route and split geometry (wgrad_route, wgrad_splits in csrc/wgrad.hip), pinned from
the one query that shows them: yms_conv_wgrad_ws_bytes = splits x slabs per split x slab bytes.

tests/golden/wgrad_ws_bytes.npz (made by tests/golden/make_wgrad_ws.py) holds that query's answers from the
library as it was BEFORE the three kernels' planners were given one split rule and one route record, for every
dense conv of the YOLOv8-s / YOLOv8-l / YOLO-MS-S training graphs at B = 64 and the suite's own weight-gradient
shapes, in bf16 / f16 / f32, under CU-count overrides 1 / 64 / 256 / 2048 and the YMS_WG_* settings the suite
uses.  The library must reproduce the table exactly.  Runs without a GPU: the query is host arithmetic."""
import ctypes
import os

import numpy as np
import pytest

from make_wgrad_ws import ENV_KEYS, env_of          # the fixture's generator (tests/golden)
from tile_walk_cases import cu_count  # noqa: F401  (fixture: the CU-count seam, restored after each test)
from yms import _lib as L

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_ws_bytes.npz"))
SHAPES = [tuple(int(v) for v in s) for s in GOLD["shapes"]]


def set_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def ws_bytes(shp, dt):
    n, cin, h, w, cout, k, s = shp
    p = k // 2
    sh = L.ConvShape(n, h, w, cin, cout, k, s, p, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1, int(dt))
    return L.lib().yms_conv_wgrad_ws_bytes(ctypes.pointer(sh))


def test_fixture_covers_what_it_claims():
    assert GOLD["ws"].dtype == np.int64 and GOLD["ws"].shape == (len(GOLD["envs"]), 4, 3, len(SHAPES))
    assert list(GOLD["cus"]) == [1, 64, 256, 2048] and list(GOLD["dtypes"]) == [L.BF16, L.F16, L.F32]
    envs = [env_of(r) for r in GOLD["envs"]]
    for want in ({}, {"YMS_WG_RING": "0", "YMS_WG_HALO": "0"}, {"YMS_WG_RING": "2", "YMS_WG_HALO": "0"},
                 {"YMS_WG_HALO": "2"}, {"YMS_WG_HALO_NB2": "0"}, {"YMS_WG_SLAB_RATIO": "1.0"},
                 {"YMS_WG_RING": "0", "YMS_WG_HALO": "0", "YMS_WG_SLAB_RATIO": "0.0"}):
        assert want in envs, want
    # the step's streaming and deep layers, the head's 80-class 1x1, and the two shapes of the GPU seam test
    # the fused box + cls first conv of each head level (SiblingConvOp: one weight gradient over 64 + 80 outputs),
    for shp in ((64, 32, 160, 160, 32, 3, 1), (64, 256, 20, 20, 256, 3, 1), (64, 80, 80, 80, 80, 1, 1),
                (64, 128, 80, 80, 144, 3, 1), (64, 256, 40, 40, 144, 3, 1), (64, 512, 20, 20, 144, 3, 1),
                (64, 256, 80, 80, 144, 3, 1), (64, 160, 80, 80, 144, 3, 1),
                (2, 64, 24, 24, 64, 3, 1), (2, 128, 12, 12, 128, 1, 1)):
        assert shp in SHAPES, shp
    assert len(SHAPES) == len(set(SHAPES)) >= 100 and (GOLD["ws"] > 0).all()


@pytest.mark.parametrize("e", range(len(GOLD["envs"])), ids=lambda e: "-".join(
    f"{k[7:]}={v}" for k, v in env_of(GOLD["envs"][e]).items()) or "default")
def test_ws_bytes_as_before_the_route_record(e, cu_count, monkeypatch):
    """(the last setting is YMS_WG_SLAB_RATIO=0 on the TT route, where 0 has always meant "no cap")"""
    set_env(monkeypatch, env_of(GOLD["envs"][e]))
    bad = []
    for c, cu in enumerate(GOLD["cus"]):
        cu_count(cu)
        for d, dt in enumerate(GOLD["dtypes"]):
            got = np.array([ws_bytes(shp, dt) for shp in SHAPES], dtype=np.int64)
            for i in np.flatnonzero(got != GOLD["ws"][e, c, d]):
                bad.append((int(cu), int(dt), SHAPES[i], int(got[i]), int(GOLD["ws"][e, c, d, i])))
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("route", [{"YMS_WG_RING": "2", "YMS_WG_HALO": "0"}, {"YMS_WG_HALO": "2"}],
                         ids=["ring", "halo"])
def test_slab_ratio_zero_lifts_the_cap_on_ring_and_halo(route, cu_count, monkeypatch):
    """YMS_WG_SLAB_RATIO=0 means "uncapped" on every route (before the shared rule the ring and halo planners
    read it as "cap at ceil(256 / tiles)"): never fewer splits than under 1.0, and more on the deep layers"""
    more = 0
    for cu in GOLD["cus"]:
        cu_count(cu)
        for dt in (L.BF16, L.F16):
            set_env(monkeypatch, dict(route, YMS_WG_SLAB_RATIO="1.0"))
            capped = [ws_bytes(shp, dt) for shp in SHAPES]
            set_env(monkeypatch, dict(route, YMS_WG_SLAB_RATIO="0"))
            free = [ws_bytes(shp, dt) for shp in SHAPES]
            assert all(f >= c for f, c in zip(free, capped)), (cu, dt)
            more += sum(f > c for f, c in zip(free, capped))
    assert more > 0
