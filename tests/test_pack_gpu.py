"""The batched weight pack (yms_pack_job_init + yms_conv_pack_weights_batched: one launch for all of
a plan's packs, every training step) against the single-job yms_conv_pack_weight of the same
shape, bit for bit over all yms_conv_packed_elems elements, padding rows and K padding included:
forward and stride-1 dgrad layouts, ragged channel counts, the two-source (w2 / split) job that
packs the sibling head convs' transposed weight as one, absolute destinations (dst_base NULL) and
byte offsets into one arena.  Destinations start as 0xFF bytes (NaN in every dtype): every packed
element must be written, and the guard bytes between and after the jobs must stay 0xFF."""
import ctypes

import pytest
import torch

from hiputil import DT, shape
from yms import _lib as L

pytestmark = pytest.mark.gpu

SHAPES = [(16, 32, 3), (64, 64, 1), (20, 36, 3), (24, 40, 1), (128, 144, 3), (64, 67, 3)]
TWO_SOURCE = [(64, 3), (64, 80), (64, 64)]       # (cout_a, cout_b): split = cout_a
GUARD = 256


def _single(sp, w, fd, dtype):
    """yms_conv_pack_weight into a 0xFF-filled buffer -> raw bytes"""
    es = 4 if dtype == torch.float32 else 2
    nb = L.lib().yms_conv_packed_elems(sp, fd) * es
    out = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    L.call("yms_conv_pack_weight", sp, w.data_ptr(), out.data_ptr(), fd, L.stream_ptr())
    return out


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_batched_pack_matches_single(dt):
    dtype = DT[dt]
    es = 4 if dtype == torch.float32 else 2
    g = torch.Generator().manual_seed(11)
    specs = []            # (shape, w, for_dgrad, w2, split, reference weight)
    for cin, cout, k in SHAPES:
        w = torch.randn(cout, cin, k, k, generator=g).cuda()
        for fd in (0, 1):
            specs.append((shape(1, 8, 8, cin, cout, k, 1, dtype), w, fd, None, 0, w))
    for ca, cb in TWO_SOURCE:
        wa = torch.randn(ca, 20, 3, 3, generator=g).cuda()
        wb = torch.randn(cb, 20, 3, 3, generator=g).cuda()
        specs.append((shape(1, 8, 8, 20, ca + cb, 3, 1, dtype), wa, 1, wb, ca, torch.cat([wa, wb]).contiguous()))
    nj = len(specs)
    nbytes = [L.lib().yms_conv_packed_elems(ctypes.pointer(sh), fd) * es for sh, _, fd, _, _, _ in specs]
    assert all(nb > 0 for nb in nbytes)
    refs = [_single(ctypes.pointer(sh), wr, fd, dtype) for sh, _, fd, _, _, wr in specs]
    offs, total = [], GUARD
    for nb in nbytes:
        offs.append(total)
        total += (nb + GUARD + 255) // 256 * 256

    def launch(base, dsts):
        jobs = (L.PackJob * nj)()
        for j, (sh, w, fd, w2, split, _) in enumerate(specs):
            st = L.lib().yms_pack_job_init(ctypes.pointer(sh), w.data_ptr(), dsts[j], fd, ctypes.byref(jobs[j]))
            assert st == 0
            assert jobs[j].w2 is None and jobs[j].split == 0
            if w2 is not None:
                jobs[j].w2, jobs[j].split = w2.data_ptr(), split
        table = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).cuda()
        L.call("yms_conv_pack_weights_batched", nj, table.data_ptr(), base, L.stream_ptr())
        torch.cuda.synchronize()

    def check(arena):
        lo = 0
        for j, (off, nb) in enumerate(zip(offs, nbytes)):
            assert (arena[lo:off] == 0xFF).all(), j                 # guard before job j untouched
            got = arena[off:off + nb]
            assert not torch.isnan(got.view(dtype)).any(), j        # every element written
            assert torch.equal(got, refs[j]), (j, specs[j][0].cin, specs[j][0].cout, specs[j][2])
            lo = off + nb
        assert (arena[lo:] == 0xFF).all()

    # byte offsets from one arena
    arena = torch.full((total,), 0xFF, dtype=torch.uint8, device="cuda")
    launch(arena.data_ptr(), offs)
    check(arena)
    # absolute destinations
    arena2 = torch.full((total,), 0xFF, dtype=torch.uint8, device="cuda")
    launch(None, [arena2.data_ptr() + o for o in offs])
    check(arena2)


def test_pack_job_init_rejects_stride2_dgrad():
    """stride-2 dgrad weights use the parity-class packing of yms_conv_pack_weight only"""
    sh = shape(1, 8, 8, 16, 32, 3, 2, torch.bfloat16)
    job = L.PackJob()
    dummy = ctypes.c_float(0)
    assert L.lib().yms_pack_job_init(ctypes.pointer(sh), ctypes.addressof(dummy), None, 1, ctypes.byref(job)) == 2
    assert L.lib().yms_pack_job_init(ctypes.pointer(sh), ctypes.addressof(dummy), None, 0, ctypes.byref(job)) == 0
