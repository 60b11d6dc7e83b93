"""GPU tests: fp16 channels-last heatmaps written at their source -- the keypoint
renderer (fvp_render_keypoints_f16), the backbone's last layer (fvp_conv1x1_cl_f16) --
and the option that carries the choice through the fused forwards.

Renderer: rounding is monotone, so the fp16 render must equal the fp32 render followed
by .half() bit for bit.  Head: the interval criterion of tests/half_ref.py (the fp16
rounding of some value within the derived fp32 bound of tests/conv_ref.py), with its
cap.  Consumers and the switch: bit-identity with the routes that existed before (the
fp32 producer, then the cast / layout pass).  Small shapes throughout."""
import dataclasses
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import half_ref as HR
import render_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(48, 32), (50, 37)]  # heatmap (W, H): a partial tile (50 = 32 + 18) and a partial band (37 = 9 * 4 + 1)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def _eq_bits(a, b, what):
    assert a.dtype == b.dtype == torch.float16 and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


# ------------------------------------------------------------------ renderer
def _dev(a, dev, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _both(dev, joints, count, vis, heatmap_size, dtype=torch.float64, image_size=R.IMAGE_SIZE, sigma=R.SIGMA):
    """(fp16 render, fp32 render) of one input."""
    from fvp.heatmaps import render_keypoints

    j, c, v = _dev(joints, dev, dtype), _dev(count, dev), _dev(vis, dev)
    kw = dict(image_size=image_size, heatmap_size=heatmap_size, sigma=sigma)
    h = render_keypoints(j, c, v, dtype=torch.float16, **kw)
    f = render_keypoints(j, c, v, **kw)
    assert h.dtype == torch.float16 and f.dtype == torch.float32 and h.shape == f.shape and h.cp == f.cp
    return h, f


def _assert_render_equal(h, f, what):
    _eq_bits(h.t, f.t.half(), what)
    pad = _bits(h.t[..., h.J:])
    assert not pad.any(), f"{what}: padding channels must be +0 bit for bit"


@functools.lru_cache(maxsize=None)
def _people(seed, J, hm):
    """R.make_people for any J >= 1 (its people pin two joints: J = 1 keeps the first of two)."""
    joints, count = R.make_people(seed, max(J, 2), hm)
    joints = np.ascontiguousarray(joints[:, :, :, :J])
    for a in (joints, count):
        a.setflags(write=False)
    return joints, count


@pytest.mark.parametrize("case", range(4))
def test_render_golden_cases(gpu_device, case):
    c = R.golden_cases()[case]
    h, f = _both(gpu_device, c["joints"], c["count"], c["vis"], c["heatmap_size"], torch.float64, c["image_size"],
                 c["sigma"])
    assert f.t.any()
    _assert_render_equal(h, f, f"golden case {case}")


@pytest.mark.parametrize("hm", SHAPES, ids=["48x32", "50x37"])
@pytest.mark.parametrize("with_vis", [False, True], ids=["all-visible", "vis"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("J", [1, 8, 9, 15, 17, 32])
def test_render_random_people(gpu_device, J, f32, with_vis, hm):
    joints, count = _people(20 + J, J, hm)
    vis = R.make_vis(J, J) if with_vis else None
    h, f = _both(gpu_device, joints, count, vis, hm, torch.float32 if f32 else torch.float64)
    assert h.cp == (16 if J <= 16 else 32) and f.t.any()
    _assert_render_equal(h, f, f"J={J} f32={f32} vis={with_vis} hm={hm}")


def test_render_full_kept_lists(gpu_device):
    """32 people x 32 joints piled on one tile: every channel group of that tile keeps
    8 x 32 records, the capacity of its list."""
    rng = np.random.default_rng(5)
    hm = (50, 37)
    stride = np.asarray(R.IMAGE_SIZE, np.float64) / np.asarray(hm, np.float64)
    joints = np.stack([R._person(rng, 32, (12.0 + rng.uniform(-1, 1), 9.0 + rng.uniform(-1, 1)), rng.uniform(1, 4),
                                 stride) for _ in range(32)])[None, None]
    count = np.array([[32]], np.int32)
    h, f = _both(gpu_device, joints, count, None, hm)
    # every window (13 x 13 around a centre within 2 px of (12, 9)) meets tile 0 of band rows 8..11
    assert (f.t[0, 0, 9, 12, :] > 0).all()
    _assert_render_equal(h, f, "P = J = 32 on one tile")


def test_render_empty_view_and_nan_person(gpu_device):
    joints, count = _people(31, 17, SHAPES[1])
    count0 = count.copy()
    count0[1, 0] = 0
    h, f = _both(gpu_device, joints, count0, None, SHAPES[1])
    assert not _bits(h.t[1, 0]).any()  # +0 everywhere
    _assert_render_equal(h, f, "empty view")
    bad = joints.copy()
    bad[0, 0, 1, 3, 0] = np.nan
    bad[0, 1, 2, 0, 1] = np.inf
    h2, f2 = _both(gpu_device, bad, count, None, SHAPES[1])
    _assert_render_equal(h2, f2, "person with a NaN joint")
    assert not torch.equal(f2.t, _both(gpu_device, joints, count, None, SHAPES[1])[1].t)  # (they were painted before)
    assert torch.isfinite(h2.t).all()


def test_render_overwrites_prefilled_buffer_and_stops_at_its_end(gpu_device):
    from fvp import ops

    hm = SHAPES[1]
    joints, count = _people(33, 15, hm)
    _, f = _both(gpu_device, joints, count, None, hm)
    want = f.t.half()
    n = want.numel()
    buf = torch.full((n + 64,), 9.0, dtype=torch.float16, device=gpu_device)
    out = buf[:n].view(want.shape)
    ops.render_keypoints_into(_dev(joints, gpu_device), _dev(count, gpu_device), None, R.IMAGE_SIZE[0],
                              R.IMAGE_SIZE[1], R.SIGMA, out)
    _eq_bits(out, want, "prefilled with 9.0")
    assert (buf[n:] == 9.0).all(), "the sentinel after the buffer must stay untouched"


def _shelf(hm, **kw):
    from fvp.workloads import WORKLOADS

    return dataclasses.replace(WORKLOADS["shelf_native"], heatmap_size=hm, voxels_per_axis=(24, 16, 5),
                               space_size=(2000.0, 2000.0, 2000.0), ind_space_size=(2000.0, 2000.0, 2000.0),
                               ind_voxels_per_axis=(16, 16, 16), **kw)


def _rt(w, dev):
    from fvp import geometry

    return torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(dev)


def test_consumers_read_the_fp16_render_in_place(gpu_device):
    """ProjectLayer.forward_fused and the person layer's forward_planes on the fp16 render ==
    the same calls on to_channels_last(planar fp32 render, dtype=float16), bit for bit."""
    from fvp.heatmaps import to_channels_last
    from fvp.project_individual import ProjectLayer as PersonLayer
    from fvp.project_whole import ProjectLayer

    w = _shelf((50, 37))
    B, P = 2, 3
    rng = np.random.default_rng(21)
    W, H = w.heatmap_size
    stride = np.asarray(w.image_size, np.float64) / np.asarray(w.heatmap_size, np.float64)
    cams, seq = w.cameras()
    V = len(cams[seq])
    joints = np.stack([R._person(rng, w.num_joints, (rng.uniform(0, W), rng.uniform(0, H)), rng.uniform(4, 40), stride)
                       for _ in range(B * V * P)]).reshape(B, V, P, w.num_joints, 2)
    count = rng.integers(1, P + 1, size=(B, V)).astype(np.int32)
    h, f = _both(gpu_device, joints, count, None, w.heatmap_size, image_size=w.image_size)
    via_cast = to_channels_last(f.planar().clone(), dtype=torch.float16)
    _eq_bits(h.t, via_cast.t, "render vs layout pass")

    rt, meta = _rt(w, gpu_device), {"seq": [seq] * B}
    layer = ProjectLayer(w.cfg(str(gpu_device)))
    layer.verbose = False
    cube, xy = layer.forward_fused(h, meta, cams, rt)
    cube_ref, xy_ref = layer.forward_fused(via_cast, meta, cams, rt)
    assert cube_ref.any() and torch.equal(cube, cube_ref) and torch.equal(xy, xy_ref)

    person = PersonLayer(w.cfg(str(gpu_device)))
    person.verbose = False
    person.on_the_fly = False  # (the on-the-fly person path has no fp16 channels-last kernel)
    c = w.space_center
    props = torch.tensor([[c[0], c[1], c[2], 0, 0.9, 0.5, 0.5], [c[0] + 300, c[1] - 200, c[2] - 100, 0, 0.8, 0.2, 0.9]],
                         dtype=torch.float32, device=gpu_device)
    a = person.forward_planes(h, 1, meta, props, cams, rt)
    b = person.forward_planes(via_cast, 1, meta, props, cams, rt)
    assert b[0].any() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------ head
LDW = 128  # the weight row pitch of a 1x1 ConvLayer's wpack


def _head(dev, x_rows, w, scale, shift, cp, tail=64, fill=9.0):
    """fvp_conv1x1_cl_f16 on x_rows [npix, Cpi] fp32 (device) and w [J, Cin] -> ([npix, cp] fp16, the
    `tail` sentinel elements after it).  scale / shift are passed at exactly J elements."""
    from fvp import _lib
    from fvp.ops import _ptr, _stream

    npix, cpi = x_rows.shape
    J, cin = w.shape
    wp = torch.zeros((cpi, LDW), dtype=torch.float32)
    wp[:cin, :J] = torch.from_numpy(np.asarray(w, np.float32)).t()
    wp, sc, sh = wp.to(dev), _dev(np.asarray(scale, np.float32), dev), _dev(np.asarray(shift, np.float32), dev)
    buf = torch.full((npix * cp + tail,), fill, dtype=torch.float16, device=dev)
    assert x_rows.is_contiguous() and x_rows.dtype == torch.float32 and sc.numel() == J and sh.numel() == J
    _lib.call("fvp_conv1x1_cl_f16", _ptr(x_rows), npix, cpi, _ptr(wp), LDW, J, _ptr(sc), _ptr(sh), cp, _ptr(buf),
              _stream(buf))
    return buf[:npix * cp].view(npix, cp), buf[npix * cp:]


def _rows(x):
    """[N, C, H, W] numpy -> [N H W, C] fp32 rows."""
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1).reshape(-1, x.shape[1])))


def _planes(out, shape, J):
    """[npix, cp] fp16 device -> [N, J, H, W] float64 numpy."""
    N, H, W = shape
    return out[:, :J].double().cpu().numpy().reshape(N, H, W, J).transpose(0, 3, 1, 2)


@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 3, 33), (1, 1, 1)], ids=["1x5x7", "2x3x33", "1x1x1"])
@pytest.mark.parametrize("cin", [16, 32, 64, 256])
@pytest.mark.parametrize("J", [1, 15, 16, 17, 32])
def test_head_interval_criterion(gpu_device, J, cin, shape):
    c = HR.case(1000 + 37 * cin + J, *shape, cin, J)
    cp = 16 if J <= 16 else 32
    out, tail = _head(gpu_device, _rows(c["x"]).to(gpu_device), c["w"][:, :, 0, 0], c["scale"], c["shift"], cp)
    ok = HR.inside(_planes(out, shape, J), c["ref"], c["tol"])
    print(f"{shape} Cin {cin} J {J}: wide intervals {c['share']:.3f} (seed {c['seed']}), "
          f"outside {np.count_nonzero(~ok)}")
    assert c["share"] <= HR.CAP
    assert ok.all(), f"{np.count_nonzero(~ok)} of {ok.size} elements outside their interval"
    assert not _bits(out[:, J:]).any(), "padding channels must be +0 bit for bit"
    assert (tail == 9.0).all(), "the sentinel after out must stay untouched"


def test_head_overflow_gives_inf(gpu_device):
    shape, cin, J = (2, 3, 33), 64, 17
    c = HR.case(5, *shape, cin, J)
    scale = c["scale"].copy()
    scale[3], scale[16] = 3e7, -3e7  # |scale * sum| far beyond 65504 wherever the sum is not tiny
    shift = np.zeros_like(c["shift"])
    ref, tol = HR.ref_tol(c["x"], c["w"], scale, shift)
    out, _ = _head(gpu_device, _rows(c["x"]).to(gpu_device), c["w"][:, :, 0, 0], scale, shift, 32)
    got = _planes(out, shape, J)
    assert HR.inside(got, ref, tol).all()
    for ch in (3, 16):
        big = np.abs(ref[:, ch]) - tol[:, ch] > 65520.0
        assert big.mean() > 0.5
        assert np.array_equal(got[:, ch][big], np.sign(ref[:, ch][big]) * np.inf)
        assert (ref[:, ch][big] > 0).any() and (ref[:, ch][big] < 0).any()  # both +inf and -inf


def test_head_nonfinite_pixel_stays_in_its_row(gpu_device):
    shape, cin, J = (2, 3, 33), 256, 15
    c = HR.case(6, *shape, cin, J)
    rows = _rows(c["x"])
    clean, _ = _head(gpu_device, rows.to(gpu_device), c["w"][:, :, 0, 0], c["scale"], c["shift"], 16)
    dirty_rows = rows.clone()
    p = 40  # (in the second 32-pixel tile)
    dirty_rows[p, 7], dirty_rows[p, 200] = float("nan"), float("inf")
    dirty, _ = _head(gpu_device, dirty_rows.to(gpu_device), c["w"][:, :, 0, 0], c["scale"], c["shift"], 16)
    keep = torch.ones(rows.shape[0], dtype=torch.bool)
    keep[p] = False
    _eq_bits(dirty[keep.to(gpu_device)], clean[keep.to(gpu_device)], "other pixels")
    assert torch.isnan(dirty[p, :J]).all() and not _bits(dirty[p, J:]).any()


def test_head_position_invariance(gpu_device):
    """The same 35 rows alone, at the end of a 1,000-pixel launch and across a tile boundary."""
    cin, J = 256, 17
    c = HR.case(8, 1, 5, 7, cin, J)
    rows = _rows(c["x"])
    assert rows.shape[0] == 35
    filler = torch.from_numpy(np.maximum(np.random.default_rng(9).standard_normal((1000, cin)), 0).astype(np.float32))
    args = (c["w"][:, :, 0, 0], c["scale"], c["shift"], 32)
    alone, _ = _head(gpu_device, rows.to(gpu_device), *args)
    assert HR.inside(_planes(alone, (1, 5, 7), J), c["ref"], c["tol"]).all()
    for start in (965, 20, 29):  # the launch's end (a partial last tile); inside; across tiles 0 / 1
        big = filler.clone()
        big[start:start + 35] = rows
        out, tail = _head(gpu_device, big.to(gpu_device), *args)
        _eq_bits(out[start:start + 35], alone, f"rows at {start}")
        assert (tail == 9.0).all()


# ------------------------------------------------------------------ backbone
def _backbone(dev, J, dtype=torch.float32, final_kernel=1, seed=3):
    import cnn_arch
    from fvp import synthetic
    from fvp.backbone import FvpPoseResNet

    m = cnn_arch.PoseResNet(18, J, final_kernel=final_kernel).eval()
    m.load_state_dict(synthetic.seeded_state_dict(m, seed))
    return FvpPoseResNet(m.to(dev), dtype), m


def _views(dev, B=2, V=2, seed=5):
    return torch.randn((B, V, 3, 64, 96), generator=torch.Generator().manual_seed(seed)).to(dev)


@pytest.mark.parametrize("J", [15, 17])
def test_backbone_writes_fp16_heatmaps_from_its_last_layer(gpu_device, J):
    """heatmaps_cl(dtype=float16) takes the head kernel; its values meet the interval
    criterion against the float64 final layer on features_nhwc (real activations: the share
    of wide intervals is printed, the cap belongs to the head cases' prescribed inputs);
    forward_nhwc is still final(features), bit for bit."""
    bb, m = _backbone(gpu_device, J)
    views = _views(gpu_device)
    images = views.reshape((4,) + tuple(views.shape[2:]))
    cl = bb.heatmaps_cl(views, dtype=torch.float16)
    assert bb.last_head_route == bb.head_route() == "conv1x1_cl_f16"
    assert cl.dtype == torch.float16 and cl.shape == (2, 2, J, 16, 24) and cl.cp == (16 if J == 15 else 32)
    feats = bb.features_nhwc(images)
    assert feats.t.dtype == torch.float32 and tuple(feats.t.shape) == (4, 16, 24, 256)
    x = feats.t.cpu().numpy().transpose(0, 3, 1, 2)
    fl = m.final_layer
    wt, bias = fl.weight.detach().cpu().numpy(), fl.bias.detach().cpu().numpy()
    ref, tol = HR.ref_tol(x, wt, np.ones(J, np.float32), bias)
    got = cl.t.view(4, 16, 24, cl.cp)[..., :J].double().cpu().numpy().transpose(0, 3, 1, 2)
    ok = HR.inside(got, ref, tol)
    print(f"J {J}: wide intervals {HR.wide_share(ref, tol):.3f}, outside {np.count_nonzero(~ok)} of {ok.size}")
    assert ok.all()
    assert not _bits(cl.t[..., J:]).any()
    # the fp32 route is what it was: forward_nhwc == final(features), and heatmaps_cl() is that
    a = bb.forward_nhwc(images)
    b = bb.final(bb.features_nhwc(images), relu=False)
    assert torch.equal(a.t, b.t)
    assert torch.equal(bb.heatmaps_cl(views).t.view_as(a.t), a.t)


@pytest.mark.parametrize("kind", ["final3x3", "bf16"])
def test_backbone_fallback_route_is_the_cast(gpu_device, kind):
    bb, _ = _backbone(gpu_device, 15, torch.bfloat16 if kind == "bf16" else torch.float32,
                      3 if kind == "final3x3" else 1)
    views = _views(gpu_device)
    cl = bb.heatmaps_cl(views, dtype=torch.float16)
    assert bb.last_head_route == "cast" and cl.dtype == torch.float16
    _eq_bits(cl.t, bb.heatmaps_cl(views).half().t, kind)


# ------------------------------------------------------------------ switch
def test_share_channels_last_lays_out_fp16(gpu_device):
    from fvp import synthetic
    from fvp.heatmaps import channels_last_of, release, share_channels_last
    from fvp.project_whole import ProjectLayer

    w = _shelf((45, 31))
    B = 2
    cams, seq = w.cameras()
    rt, meta = _rt(w, gpu_device), {"seq": [seq] * B}
    layer = ProjectLayer(w.cfg(str(gpu_device)))
    layer.verbose = False
    hm = synthetic.uniform_heatmaps(w, B, seed=4).to(gpu_device)
    want = layer.forward_fused(hm.half().float(), meta, cams, rt)
    cl = share_channels_last(hm, dtype=torch.float16)
    assert cl is not None and cl.dtype == torch.float16 and channels_last_of(hm) is cl
    got = layer.forward_fused(hm, meta, cams, rt)
    release(hm)
    assert want[0].any() and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(want[0], layer.forward_fused(hm, meta, cams, rt)[0])  # (fp32 differs: the option matters)


def _fake_reference(mods_cls):
    """Stand-ins for models.resnet / models.faster_voxelpose with the reference's forward flow on
    the views path (faster_voxelpose.py:73-86), as tests/test_backbone.py builds them."""
    import types

    rn = types.ModuleType("models.resnet")
    rn.ResNet = mods_cls

    class FasterVoxelPoseNet(nn.Module):
        def __init__(self, project_layer):
            super().__init__()
            self.project_layer = project_layer
            self.seen = None

        def forward(self, backbone=None, views=None, meta=None, targets=None, input_heatmaps=None, cameras=None,
                    resize_transform=None):
            if views is not None:
                input_heatmaps = torch.stack([backbone(views[:, c]) for c in range(views.shape[1])], dim=1)
            from fvp.heatmaps import channels_last_of
            self.seen = channels_last_of(input_heatmaps)  # what the HDN / JLN are handed
            cube = self.project_layer(input_heatmaps, meta, cameras, resize_transform)
            return cube, input_heatmaps

    fv = types.ModuleType("models.faster_voxelpose")
    fv.FasterVoxelPoseNet = FasterVoxelPoseNet
    return {"models.resnet": rn, "models.faster_voxelpose": fv}, FasterVoxelPoseNet


def _restore(cls):
    if hasattr(cls, "_fvp_original_forward"):
        cls.forward = cls._fvp_original_forward
        del cls._fvp_original_forward
    if "fvp_options" in cls.__dict__:
        del cls.fvp_options


def test_installed_views_path_hands_the_model_fp16_heatmaps(gpu_device):
    """install(backbone=True, heatmaps_dtype=float16): the model is handed the fp16
    channels-last copy the backbone's last layer wrote, the copy does not outlive the forward,
    and the cube equals the planar voxelize of the returned heatmaps bit for bit."""
    import cnn_arch
    from fvp import integration, synthetic
    from fvp.heatmaps import channels_last_of
    from fvp.project_whole import ProjectLayer

    class ResNet(cnn_arch.PoseResNet):
        pass

    w = _shelf((24, 16))
    cams, seq = w.cameras()
    B, V = 2, len(cams[seq])
    layer = ProjectLayer(w.cfg(str(gpu_device)))
    layer.verbose = False
    rt, meta = _rt(w, gpu_device), {"seq": [seq] * B}
    mods, FVP = _fake_reference(ResNet)
    m = ResNet(18, w.num_joints).eval()
    m.load_state_dict(synthetic.seeded_state_dict(m, 4))
    m = m.to(gpu_device)
    model = FVP(layer).eval()
    views = torch.randn((B, V, 3, 64, 96), generator=torch.Generator().manual_seed(6)).to(gpu_device)
    with torch.no_grad():
        try:
            patched = integration.install(fused=True, modules=mods, backbone=True, heatmaps_dtype=torch.float16)
            assert patched["models.resnet.ResNet.fvp_options"].heatmaps_dtype == torch.float16
            cube, hm = model(backbone=m, views=views, meta=meta, cameras=cams, resize_transform=rt)
            seen = model.seen
            assert seen is not None and seen.dtype == torch.float16  # the model saw the fp16 copy
            assert integration.fvp_backbone.cached(m).last_head_route == "conv1x1_cl_f16"
            assert channels_last_of(hm) is None  # and it does not outlive the forward
            integration.install(fused=True, modules=mods, backbone=True)
            cube32, hm32 = model(backbone=m, views=views, meta=meta, cameras=cams, resize_transform=rt)
            assert model.seen.dtype == torch.float32 and hm32.dtype == torch.float32
        finally:
            _restore(ResNet)
            _restore(FVP)
        assert tuple(hm.shape) == (B, V, w.num_joints, 16, 24)
        planar = layer(hm.float().clone(), meta, cams, rt)
    torch.cuda.synchronize()
    assert cube.any() and torch.equal(cube, planar)
    assert hm.dtype == torch.float16 and cube32.any()
