"""GPU tests of the uint8 camera-frame input: fvp_frames_to_views against the numpy table
bit for bit (every byte value, strided and misaligned layouts, guard floats), the u8 stems
against the existing stems run on the reference views (torch.equal: they share the MFMA
loop, so anything else is a halo-loader bug), and the backbone / fused-forward routes."""
import ctypes
import math

import numpy as np
import pytest
import torch

import frames_ref as R

pytestmark = pytest.mark.gpu

VH, VW = 37, 83  # a view with partial 8 x 32 stem tiles in both directions (3 x 2 of them)


def _rand_u8(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def _frames(data_cpu, dev, **kw):
    """Frames over a device copy of data_cpu's whole buffer with the same strides, and its
    reference views (numpy, from the CPU bytes)."""
    from fvp.frames import Frames

    buf = R.buffer_of(data_cpu)
    off = data_cpu.storage_offset()  # kept on the device: a misaligned base stays misaligned
    dbuf = torch.zeros((off + buf.size,), dtype=torch.uint8, device=dev)
    dbuf[off:] = torch.from_numpy(buf).to(dev)
    fr = Frames(torch.as_strided(dbuf, data_cpu.shape, data_cpu.stride(), off), **kw)
    return fr, R.views_ref(buf, fr.B, fr.spec)


def _mosaic_in_buffer(B, seed, misalign=1):
    """B 2 x 2 mosaics of VH x VW views inside a larger buffer: row pitch 2*VW*3 + 5, base
    offset 1 byte, every other frame slot (a non-contiguous batch)."""
    pitch = 2 * VW * 3 + 5
    slot = 2 * VH * pitch
    buf = _rand_u8((misalign + 2 * B * slot,), seed)
    return torch.as_strided(buf, (B, 2 * VH, 2 * VW, 3), (2 * slot, pitch, 3, 1), misalign)


def _all_values(pix):
    """One 16 x 48 view holding all 256 byte values in each channel."""
    p = torch.arange(16 * 48, dtype=torch.int64)
    px = torch.stack([p, p + 85, 255 - p] + ([p * 7 + 3] if pix == 4 else []), dim=1) % 256
    return px.to(torch.uint8).reshape(1, 1, 16, 48, pix)


@pytest.mark.parametrize("pix", [3, 4])
@pytest.mark.parametrize("swap_rb", [False, True])
def test_every_byte_value(gpu_device, swap_rb, pix):
    data = _all_values(pix)
    for c in range(3):
        assert len(set(data[..., c].reshape(-1).tolist())) == 256
    fr, ref = _frames(data, gpu_device, swap_rb=swap_rb)
    got = fr.views()
    torch.cuda.synchronize()
    assert np.array_equal(R.bits(got), R.bits(ref))
    # and the table is what the reference computes: torch's CPU chain on the same bytes
    from fvp.frames import Frames

    assert np.array_equal(R.bits(Frames(data, swap_rb=swap_rb).views()), R.bits(ref))


@pytest.mark.parametrize("layout", ["per_view", "mosaic_pitched_misaligned"])
def test_layouts_and_guards(gpu_device, layout):
    """The output sits in a NaN-filled buffer between guard floats, which stay untouched."""
    from fvp import _lib
    from fvp.ops import _ptr, _stream

    if layout == "per_view":
        fr, ref = _frames(_rand_u8((2, 3, VH, VW, 3), 11), gpu_device)
    else:
        data = _mosaic_in_buffer(2, 12)
        fr, ref = _frames(data, gpu_device, mosaic=(2, 2))
        assert fr.data.data_ptr() % 2 == 1 and fr.spec.row_stride == 2 * VW * 3 + 5
        assert not fr.data.is_contiguous() and fr.spec.frame_stride == 2 * 2 * VH * fr.spec.row_stride
    G, n = 64, ref.size
    out = torch.full((G + n + G,), float("nan"), device=gpu_device)
    _lib.call("fvp_frames_to_views", _ptr(fr.data), fr.B, ctypes.byref(fr.spec), out.data_ptr() + 4 * G, _stream(out))
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool(torch.isnan(out[:G]).all()) and bool(torch.isnan(out[G + n:]).all())
    assert np.array_equal(R.bits(out[G:G + n]).reshape(ref.shape), R.bits(ref))
    assert np.array_equal(R.bits(fr.views()), R.bits(ref))  # the op, into its own allocation


# ------------------------------------------------------------------ the u8 stems
_NETS = {}


def _net(dev, bf16):
    """FvpPoseResNet of cnn_arch.PoseResNet(18, 15) with randomised weights and running statistics."""
    if bf16 not in _NETS:
        import cnn_arch
        from fvp import synthetic
        from fvp.backbone import FvpPoseResNet

        m = cnn_arch.PoseResNet(18, 15).eval()
        m.load_state_dict(synthetic.seeded_state_dict(m, 21))
        _NETS[bf16] = FvpPoseResNet(m.to(dev), torch.bfloat16 if bf16 else torch.float32)
    return _NETS[bf16]


def _stem_case(case, dev):
    """-> (data on the CPU, Frames keyword arguments)"""
    if case == "one_view":  # 3 x 2 tiles, partial both ways, the halo crosses all four borders; tiles < blocks
        return _rand_u8((1, 1, VH, VW, 3), 31), {}
    if case == "mosaic_many_tiles":  # 24 tiles per frame: more tiles than the 2-per-CU persistent blocks
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        return _mosaic_in_buffer(math.ceil((2 * cus + 64) / 24), 32), dict(mosaic=(2, 2))
    if case == "exact_tiles":
        return _rand_u8((1, 2, 16, 64, 3), 33), {}
    if case == "one_pixel":
        return _rand_u8((2, 1, 1, 1, 3), 34), {}
    if case == "bgrx_swap":
        return _rand_u8((1, 2, VH, VW, 4), 35), dict(swap_rb=True)
    if case == "all_255":  # padding is 0, not normalise(0) -- and not normalise(255) either
        return torch.full((1, 1, VH, VW, 3), 255, dtype=torch.uint8), {}
    if case == "all_0":
        return torch.zeros((1, 1, VH, VW, 3), dtype=torch.uint8), {}
    raise KeyError(case)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ["one_view", "mosaic_many_tiles", "exact_tiles", "one_pixel", "bgrx_swap",
                                  "all_255", "all_0"])
def test_u8_stem_equals_stem_on_reference_views(gpu_device, case, bf16):
    from fvp import _lib
    from fvp.ops import _ptr, _stream

    bb = _net(gpu_device, bf16)
    assert (bb.stem7 if bf16 else bb.stem7_f32) is not None
    data, kw = _stem_case(case, gpu_device)
    fr, ref = _frames(data, gpu_device, **kw)
    views = torch.from_numpy(ref).to(gpu_device).flatten(0, 1)
    want = (bb._stem7 if bf16 else bb._stem7_f32)(views).t
    if case == "mosaic_many_tiles":
        cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
        assert views.shape[0] * 6 > 2 * cus  # some blocks walk a second tile through the register prefetch
    got = torch.full_like(want, float("nan"))
    _lib.call("fvp_conv_stem7_u8_bf16" if bf16 else "fvp_conv_stem7_u8_f32", _ptr(fr.data), fr.B,
              ctypes.byref(fr.spec), _ptr(bb.stem7 if bf16 else bb.stem7_f32), _ptr(bb.stem.scale),
              _ptr(bb.stem.shift), _ptr(got), _stream(got))
    torch.cuda.synchronize()
    assert got.shape == (fr.B * fr.V, (fr.H - 1) // 2 + 1, (fr.W - 1) // 2 + 1, 64)
    assert not bool(torch.isnan(got.float()).any())
    assert torch.equal(got, want)
    assert float(want.float().abs().max()) > 0  # not a comparison of zeros


# ------------------------------------------------------------------ routes and integration
def _route_frames(dev):
    return _frames(_rand_u8((2, 2 * 64, 2 * 96, 3), 41), dev, mosaic=(2, 2))[0]


@pytest.mark.parametrize("dtype", [None, torch.float16], ids=["f32_heatmaps", "f16_heatmaps"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_heatmaps_cl_frames_equals_heatmaps_cl_of_views(gpu_device, bf16, dtype):
    bb = _net(gpu_device, bf16)
    fr = _route_frames(gpu_device)
    assert bb.frames_route() == ("stem7_u8_bf16" if bf16 else "stem7_u8_f32")
    bb.last_frames_route = None
    got = bb.heatmaps_cl_frames(fr, dtype=dtype)
    assert bb.last_frames_route == bb.frames_route()
    want = bb.heatmaps_cl(fr.views(), dtype=dtype)
    torch.cuda.synchronize()
    assert got.t.dtype == want.t.dtype == (torch.float16 if dtype == torch.float16 else torch.float32)
    assert got.shape == want.shape == (2, 4, 15, 16, 24)
    assert torch.equal(got.t, want.t)
    f = bb.features_nhwc_frames(fr)
    assert torch.equal(f.t, bb.features_nhwc(fr.views().flatten(0, 1)).t)


@pytest.mark.parametrize("dtype", [None, torch.float16], ids=["f32_heatmaps", "f16_heatmaps"])
def test_fallback_route_on_a_forced_algo(gpu_device, dtype):
    import cnn_arch
    from fvp import cnn, synthetic
    from fvp.backbone import FvpPoseResNet

    m = cnn_arch.PoseResNet(18, 15).eval()
    m.load_state_dict(synthetic.seeded_state_dict(m, 21))
    bb = FvpPoseResNet(m.to(gpu_device), algo=cnn.CONV_PER_TAP)
    assert bb.stem7 is None and bb.stem7_f32 is None and bb.frames_route() == "views"
    fr = _route_frames(gpu_device)
    got = bb.heatmaps_cl_frames(fr, dtype=dtype)
    assert bb.last_frames_route == "views"
    want = bb.heatmaps_cl(fr.views(), dtype=dtype)
    torch.cuda.synchronize()
    assert torch.equal(got.t, want.t)


def test_frames_on_the_cpu_are_rejected_by_the_gpu_routes(gpu_device):
    from fvp._lib import FvpError
    from fvp.frames import Frames

    with pytest.raises(FvpError):
        _net(gpu_device, False).heatmaps_cl_frames(Frames(_rand_u8((1, 1, 16, 16, 3), 1)))


@pytest.mark.parametrize("backbone", [True, "bf16"], ids=["f32", "bf16"])
def test_fused_forward_takes_frames(gpu_device, backbone):
    """install(backbone=...): model(views=Frames) equals model(views=frames.views()) on every
    returned tensor (the model of test_backbone's installed-views test); without the fvp
    backbone route the original forward gets frames.views()."""
    import cnn_arch
    from fvp import integration, synthetic
    from fvp.frames import Frames
    from test_backbone import _c2_layer, _fake_reference, _restore

    class ResNet(cnn_arch.PoseResNet):
        pass

    w, layer, cams, seq, rt = _c2_layer(gpu_device)
    mods, FVP = _fake_reference(ResNet)
    m = ResNet(18, 15).eval()
    m.load_state_dict(synthetic.seeded_state_dict(m, 4))
    m = m.to(gpu_device)
    model = FVP(layer).eval()
    B, V = 2, 5
    H, W = w.heatmap_size[1], w.heatmap_size[0]
    fr = Frames(_rand_u8((B, V, 4 * H, 4 * W, 3), 6).to(gpu_device))
    meta = {"seq": [seq] * B}
    with torch.no_grad():
        try:
            integration.install(fused=True, modules=mods, backbone=backbone)
            net = integration.fvp_backbone.cached(m, torch.bfloat16 if backbone == "bf16" else torch.float32)
            net.last_frames_route = None
            got = model(backbone=m, views=fr, meta=meta, cameras=cams, resize_transform=rt)
            assert net.last_frames_route == ("stem7_u8_bf16" if backbone == "bf16" else "stem7_u8_f32")
            want = model(backbone=m, views=fr.views(), meta=meta, cameras=cams, resize_transform=rt)
            # no fvp backbone route (options without it): the original forward is handed frames.views()
            integration.set_options(model, backbone=False)
            handed, original = [], FVP._fvp_original_forward
            FVP._fvp_original_forward = lambda self, views=None, **kw: handed.append(views)
            try:
                model(backbone=m, views=fr, meta=meta, cameras=cams, resize_transform=rt)
            finally:
                FVP._fvp_original_forward = original
        finally:
            _restore(ResNet)
            _restore(FVP)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert len(handed) == 1 and isinstance(handed[0], torch.Tensor) and torch.equal(handed[0], fr.views())
