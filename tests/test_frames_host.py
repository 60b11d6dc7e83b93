"""CPU tests of the uint8 camera-frame input (fvp.frames, fvp_frame_spec): the reference
table against torch's own ToTensor + Normalize chain, planted faults that the table must
tell apart, Frames on CPU tensors against the table for every layout, and the host checks
of the three C entry points (no launch is made)."""
import ctypes

import numpy as np
import pytest
import torch

import frames_ref as R


def _torch_chain(view_hwc, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD):
    """transforms.ToTensor() then transforms.Normalize(mean, std) on one HWC uint8 view."""
    mean = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    std = torch.tensor(std, dtype=torch.float32)[:, None, None]
    return view_hwc.permute(2, 0, 1).contiguous().float().div(255).sub_(mean).div_(std)


def _rand_u8(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def test_table_equals_torch_chain_on_a_mosaic():
    H, W = 24, 40
    frame = _rand_u8((2 * H, 2 * W, 3), 1)
    tab = R.table()
    # all 768 (channel, byte) pairs
    allv = torch.arange(256, dtype=torch.uint8)[None, :, None].expand(1, 256, 3).contiguous()
    assert np.array_equal(R.bits(_torch_chain(allv)[:, 0, :]), R.bits(tab))
    # service.py's split_frame order: TL, TR, BL, BR
    views = [frame[r * H:(r + 1) * H, c * W:(c + 1) * W] for r in (0, 1) for c in (0, 1)]
    ref = torch.stack([_torch_chain(v) for v in views])
    from fvp._lib import FrameSpec

    spec = FrameSpec(H, W, 2, 2, 0, H * 2 * W * 3, W * 3, 2 * W * 3, 3, 0, (ctypes.c_float * 3)(*R.IMAGENET_MEAN),
                     (ctypes.c_float * 3)(*R.IMAGENET_STD))
    got = R.views_ref(frame.reshape(-1).numpy(), 1, spec)[0]
    assert np.array_equal(R.bits(got), R.bits(ref))


def test_planted_faults_differ_from_the_table():
    """b * (1/255) and the folded b*k + m are not the contract: the all-values GPU case
    can tell them from the table."""
    tab = R.table()
    rec = int(np.count_nonzero(R.bits(R.table_reciprocal()) != R.bits(tab)))
    fold = int(np.count_nonzero(R.bits(R.table_folded()) != R.bits(tab)))
    print(f"of 768 entries: reciprocal differs in {rec}, folded affine in {fold}")
    assert (rec, fold) == (322, 521)  # the ImageNet constants; IEEE fp32, so the counts are fixed
    assert np.abs(R.table_reciprocal() - tab).max() < 1e-6 and np.abs(R.table_folded() - tab).max() < 1e-5


def _check(frames, want):
    got = frames.views()
    assert got.dtype == torch.float32 and tuple(got.shape) == frames.shape == (frames.B, frames.V, 3, frames.H, frames.W)
    ref = R.views_ref(R.buffer_of(frames.data), frames.B, frames.spec)
    assert np.array_equal(R.bits(got), R.bits(ref))
    f = R.spec_fields(frames.spec)
    assert f == want, (f, want)
    assert frames.device == frames.data.device


def test_frames_cpu_layouts_and_specs():
    from fvp.frames import Frames

    B, V, H, W = 2, 3, 10, 14
    pv = _rand_u8((B, V, H, W, 3), 2)
    _check(Frames(pv), dict(H=H, W=W, VR=V, VC=1, frame_stride=V * H * W * 3, vr_stride=H * W * 3, vc_stride=0,
                            row_stride=W * 3, pix_stride=3, swap_rb=0))
    _check(Frames(pv, swap_rb=True), dict(H=H, W=W, VR=V, VC=1, frame_stride=V * H * W * 3, vr_stride=H * W * 3,
                                          vc_stride=0, row_stride=W * 3, pix_stride=3, swap_rb=1))
    # swap_rb is cv2.cvtColor(BGR2RGB): the flipped pixels without the swap
    assert torch.equal(Frames(pv, swap_rb=True).views(), Frames(pv.flip(-1).contiguous()).views())
    mo = _rand_u8((B, 2 * H, 2 * W, 3), 3)
    fm = Frames(mo, mosaic=(2, 2))
    _check(fm, dict(H=H, W=W, VR=2, VC=2, frame_stride=4 * H * W * 3, vr_stride=H * 2 * W * 3, vc_stride=W * 3,
                    row_stride=2 * W * 3, pix_stride=3, swap_rb=0))
    assert (fm.B, fm.V) == (B, 4)
    # view 1 is the top-right quadrant (split_frame order)
    assert torch.equal(fm.views()[:, 1], Frames(mo[:, None, :H, W:].contiguous()).views()[:, 0])
    p4 = _rand_u8((B, V, H, W, 4), 4)
    _check(Frames(p4, swap_rb=True), dict(H=H, W=W, VR=V, VC=1, frame_stride=V * H * W * 4, vr_stride=H * W * 4,
                                          vc_stride=0, row_stride=W * 4, pix_stride=4, swap_rb=1))
    assert torch.equal(Frames(p4).views(), Frames(p4[..., :3].contiguous()).views())  # the 4th byte is ignored
    # a batch slice and a crop are read in place
    big = _rand_u8((5, 2 * H + 3, 2 * W + 5, 3), 5)
    sl = big[1::2, 2:2 * H + 2, 1:2 * W + 1]
    assert not sl.is_contiguous()
    row = (2 * W + 5) * 3
    _check(Frames(sl, mosaic=(2, 2)), dict(H=H, W=W, VR=2, VC=2, frame_stride=2 * (2 * H + 3) * row,
                                           vr_stride=H * row, vc_stride=W * 3, row_stride=row, pix_stride=3,
                                           swap_rb=0))
    assert torch.equal(Frames(sl, mosaic=(2, 2)).views(), Frames(sl.contiguous(), mosaic=(2, 2)).views())
    # other constants
    _check(Frames(pv, mean=(0.5, 0.25, 0.125), std=(0.3, 1.0, 2.5)),
           dict(H=H, W=W, VR=V, VC=1, frame_stride=V * H * W * 3, vr_stride=H * W * 3, vc_stride=0,
                row_stride=W * 3, pix_stride=3, swap_rb=0))


def test_frames_rejects_bad_shapes_and_strides():
    from fvp._lib import FvpError
    from fvp.frames import Frames

    ok = torch.zeros((2, 3, 8, 12, 3), dtype=torch.uint8)
    Frames(ok)
    bad = [
        lambda: Frames(ok.float()),                                  # not uint8
        lambda: Frames(ok[0]),                                       # 4-D without a mosaic
        lambda: Frames(ok, mosaic=(2, 2)),                           # 5-D with one
        lambda: Frames(torch.zeros((2, 3, 8, 12, 2), dtype=torch.uint8)),  # 2 bytes per pixel
        lambda: Frames(torch.zeros((2, 9, 12, 3), dtype=torch.uint8), mosaic=(2, 2)),  # 9 rows, 2 views
        lambda: Frames(ok[:, :, :, ::2]),                            # pixel stride 6
        lambda: Frames(ok.permute(0, 1, 2, 4, 3)),                   # last stride not 1
        lambda: Frames(ok[:, :, :, :1].expand(2, 3, 8, 12, 3)),      # pixel stride 0
        lambda: Frames(ok[:, :, :1].expand(2, 3, 8, 12, 3)),         # rows overlap
        lambda: Frames(ok[:0]),                                      # empty
        lambda: Frames(ok, mosaic=(0, 2)),
        lambda: Frames(ok, std=(0.2, 0.0, 0.2)),
        lambda: Frames(ok, std=(0.2, float("inf"), 0.2)),
        lambda: Frames(ok, mean=(float("nan"), 0.0, 0.0)),
        lambda: Frames(ok, mean=(0.0, 0.0)),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(FvpError):
            f()
            pytest.fail(f"case {i} was accepted")


def _spec(**kw):
    from fvp._lib import FrameSpec

    f = dict(H=16, W=32, VR=2, VC=2, frame_stride=4 * 16 * 32 * 3, vr_stride=16 * 64 * 3, vc_stride=32 * 3,
             row_stride=64 * 3, pix_stride=3, swap_rb=0, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD)
    f.update(kw)
    mean, std = f.pop("mean"), f.pop("std")
    return FrameSpec(mean=(ctypes.c_float * 3)(*mean), std=(ctypes.c_float * 3)(*std), **f)


NULL, SHAPE = 1001, 1002
P = 4096  # a non-NULL, 16-B aligned stand-in: every call below returns before any launch


def _calls(lib):
    """name -> f(frames, B, spec, *rest): the three entry points with stand-in pointers."""
    return {
        "views": lambda fr, B, sp, out=P: lib.fvp_frames_to_views(fr, B, sp, out, None),
        "f32": lambda fr, B, sp, w=P, sc=P, sh=P, out=P: lib.fvp_conv_stem7_u8_f32(fr, B, sp, w, sc, sh, out, None),
        "bf16": lambda fr, B, sp, w=P, sc=P, sh=P, out=P: lib.fvp_conv_stem7_u8_bf16(fr, B, sp, w, sc, sh, out, None),
    }


@pytest.mark.parametrize("name", ["views", "f32", "bf16"])
def test_entry_points_check_arguments_without_gpu(name):
    from fvp import _lib

    lib = _lib.load()
    call = _calls(lib)[name]
    good = ctypes.byref(_spec())
    assert call(None, 1, good) == NULL
    assert call(P, 1, None) == NULL
    if name == "views":
        assert call(P, 1, good, None) == NULL
    else:
        for k in range(4):
            rest = [P] * 4
            rest[k] = None
            assert call(P, 1, good, *rest) == NULL
            rest[k] = P + 8  # the existing stems' 16-B alignment rule
            assert call(P, 1, good, *rest) == SHAPE
    assert call(P, 0, good) == SHAPE
    assert call(P, -1, good) == SHAPE
    for kw in (dict(H=0), dict(W=0), dict(VR=0), dict(VC=0), dict(H=-3), dict(pix_stride=2), dict(pix_stride=5),
               dict(pix_stride=0), dict(row_stride=32 * 3 - 1), dict(pix_stride=4, row_stride=32 * 4 - 1),
               dict(std=(0.2, 0.0, 0.2)), dict(std=(0.2, 0.2, float("inf"))), dict(std=(float("nan"), 0.2, 0.2)),
               dict(mean=(0.0, float("inf"), 0.0)), dict(mean=(0.0, 0.0, float("nan")))):
        assert call(P, 1, ctypes.byref(_spec(**kw))) == SHAPE, kw
    # more tiles than INT_MAX (the stems: 8 x 32 outputs; the pass: 8 x 256 pixels), and more views
    huge = _spec(H=1024, W=1024, VR=1, VC=1, row_stride=1024 * 3)
    assert call(P, 1 << 23, ctypes.byref(huge)) == SHAPE
    assert call(P, 1 << 30, ctypes.byref(_spec())) == SHAPE


def test_abi_version_and_signatures():
    from fvp import _lib

    lib = _lib.load()
    assert lib.fvp_abi_version() == _lib.ABI_VERSION == 22
    for n in ("fvp_frames_to_views", "fvp_conv_stem7_u8_f32", "fvp_conv_stem7_u8_bf16"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert ctypes.sizeof(_lib.FrameSpec) == 4 * 4 + 4 * 8 + 2 * 4 + 6 * 4  # no padding: the C struct's layout


def test_op_is_registered():
    from fvp import ops

    assert torch.ops.fvp.frames_to_views is not None and ops.frames_to_views.op is not None
    with pytest.raises(Exception):  # device implementation only: a CPU tensor has no kernel
        torch.ops.fvp.frames_to_views(torch.zeros((1, 1, 2, 2, 3), dtype=torch.uint8), [], False,
                                      list(R.IMAGENET_MEAN), list(R.IMAGENET_STD))


def test_fused_forward_hands_views_to_every_other_route():
    """Without the fvp backbone route (here: CPU frames, default options) fused_fvp_forward
    passes frames.views() -- the tensor the reference would have been given -- to the
    original forward; a tensor goes through untouched."""
    from fvp import integration
    from fvp.frames import Frames

    class Net:
        training = False

        def forward(self, backbone=None, views=None, **kw):
            return views

    Net._fvp_original_forward = Net.forward
    fr = Frames(_rand_u8((1, 2 * 6, 2 * 8, 3), 9), mosaic=(2, 2))
    got = integration.fused_fvp_forward(Net(), backbone=object(), views=fr)
    assert isinstance(got, torch.Tensor) and torch.equal(got, fr.views()) and tuple(got.shape) == (1, 4, 3, 6, 8)
    t = torch.zeros((1, 4, 3, 6, 8))
    assert integration.fused_fvp_forward(Net(), backbone=object(), views=t) is t
