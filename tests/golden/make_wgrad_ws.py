"""Generate tests/golden/wgrad_ws_bytes.npz: yms_conv_wgrad_ws_bytes over shapes x dtypes x CU-count
overrides x YMS_WG_* settings, as the library named by YMS_LIB answers (CPU only: host arithmetic).

Run:  YMS_LIB=<baseline libyms.so> python tests/golden/make_wgrad_ws.py

The fixture pins the weight gradient's route and split geometry across a refactor, so the library must be
the one built from the commit BEFORE the change under test (tools/ab_lib.sh in a checkout of it), never the
tree's own.  tests/test_wgrad_route_cpu.py then asserts the tree's library reproduces the table exactly.

Arrays (int64 only):
  shapes [S, 7]   (n, cin, h, w, cout, k, stride): every distinct 1x1 / 3x3 dense conv of the YOLOv8-s, YOLOv8-l
                  and YOLO-MS-S training graphs at B = 64, 640 x 640 (traced on the meta device from the oracle
                  restatements), each followed by the fused shape the plan runs instead when two of them read
                  the same input (the head's box / cls pair of a level: one weight gradient over cout_a + cout_b,
                  SiblingConvOp), then the weight-gradient shapes of tests/test_conv_gpu.py and tile_walk_cases.py
  dtypes [3]      yms dtype codes (bf16, f16, f32)
  cus    [4]      yms_cu_count_set overrides
  envs   [E, 4]   YMS_WG_RING, YMS_WG_HALO, YMS_WG_HALO_NB2, YMS_WG_SLAB_RATIO in hundredths; -1 = unset
  ws     [E, 4, 3, S]  bytes
"""
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yolo-ms_amd"), os.path.join(ROOT, "tests")]
from oracle import model_ref, ms_ref  # noqa: E402
from yms import _lib as L  # noqa: E402

ENV_KEYS = ("YMS_WG_RING", "YMS_WG_HALO", "YMS_WG_HALO_NB2", "YMS_WG_SLAB_RATIO")
# default; TT only; ring wherever it applies; halo on every 3x3; halo without its 64-input-channel block;
# the round-3 slab cap; no slab cap on the TT route
ENVS = [(-1, -1, -1, -1), (0, 0, -1, -1), (2, 0, -1, -1), (-1, 2, -1, -1), (-1, -1, 0, -1), (-1, -1, -1, 100),
        (0, 0, -1, 0)]
CUS = (1, 64, 256, 2048)
DTYPES = (L.BF16, L.F16, L.F32)
BATCH, SIZE = 64, 640


def env_of(row):
    """fixture row -> {name: value} of the switches it sets"""
    env = {k: str(int(v)) for k, v in zip(ENV_KEYS[:3], row[:3]) if v >= 0}
    if row[3] >= 0:
        env[ENV_KEYS[3]] = str(int(row[3]) / 100)
    return env


def model_shapes(ref, version):
    """(n, cin, h, w, cout, k, stride) of the dense 1x1 / 3x3 convs of one training forward; where a second
    bias-free conv of the same geometry reads the same input tensor as an earlier one (Builder.sibling_convs'
    pairs, the head's box / cls first convs: the plan gives them one weight gradient), also the fused shape
    with cout_a + cout_b"""
    rec, readers = [], {}          # id(input) -> (input, shapes of the bias-free convs that read it so far)
    orig = F.conv2d

    def hook(x, wt, b=None, stride=1, padding=0, dilation=1, groups=1):
        s = stride if isinstance(stride, int) else stride[0]
        if groups == 1 and wt.shape[0] != 1 and wt.shape[2] in (1, 3):      # not depthwise, not the DFL projection
            shp = (BATCH, wt.shape[1], x.shape[2], x.shape[3], wt.shape[0], wt.shape[2], s)
            rec.append(shp)
            if b is None:
                earlier = readers.setdefault(id(x), (x, []))[1]
                rec.extend(shp[:4] + (ps[4] + shp[4],) + shp[5:] for ps in earlier
                           if ps[:4] + ps[5:] == shp[:4] + shp[5:] and ps[4] % 8 == 0)
                earlier.append(shp)
        return orig(x, wt, b, stride, padding, dilation, groups)

    sd = {k: torch.zeros(s, device="meta") for k, s in ref.state_keys(version, 80)}
    F.conv2d = hook
    try:
        ref.forward(sd, version, 80, torch.zeros(1, 3, SIZE, SIZE, device="meta"), True)
    finally:
        F.conv2d = orig
    return rec


def suite_shapes():
    import test_conv_gpu as C
    import tile_walk_cases as T
    slab_cap = [(8, 64, 40, 40, 64, 3, 1), (8, 128, 20, 20, 256, 1, 1), (4, 32, 80, 80, 32, 3, 1),
                (8, 96, 40, 40, 128, 3, 2)]                                   # test_wgrad_split_k_slab_cap
    resized = [(2, 64, 24, 24, 64, 3, 1), (2, 128, 12, 12, 128, 1, 1)]        # test_wgrad_workspace_from_another_route
    return ([(n, cin, h, w, cout, 3, s) for n, cin, h, w, cout, s in C.WGH] + C.WGR + T.WG_GEMM + T.WG_HALO
            + slab_cap + resized)


def main():
    assert os.environ.get("YMS_LIB"), "name the baseline library with YMS_LIB"
    shapes = []
    for s in (model_shapes(model_ref, "s") + model_shapes(model_ref, "l") + model_shapes(ms_ref, "ms-s")
              + suite_shapes()):
        if s not in shapes:
            shapes.append(tuple(int(v) for v in s))
    lib = L.lib()
    ws = np.zeros((len(ENVS), len(CUS), len(DTYPES), len(shapes)), dtype=np.int64)
    prev = lib.yms_cu_count_set(-1)
    for e, row in enumerate(ENVS):
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(env_of(row))
        for c, cu in enumerate(CUS):
            lib.yms_cu_count_set(cu)
            for d, dt in enumerate(DTYPES):
                for i, (n, cin, h, w, cout, k, s) in enumerate(shapes):
                    p = k // 2
                    sh = L.ConvShape(n, h, w, cin, cout, k, s, p, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1, dt)
                    ws[e, c, d, i] = lib.yms_conv_wgrad_ws_bytes(ctypes.pointer(sh))
    lib.yms_cu_count_set(prev)
    assert ws.min() > 0
    out = os.path.join(HERE, "wgrad_ws_bytes.npz")
    np.savez_compressed(out, shapes=np.array(shapes, dtype=np.int64), dtypes=np.array(DTYPES, dtype=np.int64),
                        cus=np.array(CUS, dtype=np.int64), envs=np.array(ENVS, dtype=np.int64), ws=ws)
    print(f"{out}: {len(shapes)} shapes, {ws.size} values, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
