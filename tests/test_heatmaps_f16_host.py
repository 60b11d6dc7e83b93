"""CPU tests of the fp16 heatmap producers (fvp_render_keypoints_f16,
fvp_conv1x1_cl_f16) and their switch: the symbols are exported and declared, the host
checks refuse bad arguments before any launch (no GPU), the new op's fake kernel keeps
shape and dtype, and the option defaults to fp32."""
import os
import re

import pytest
import torch

from conftest import REPO

HEADER = os.path.join(REPO, "include", "fvp.h")
NEW = ["fvp_render_keypoints_f16", "fvp_conv1x1_cl_f16"]
P = 4096  # a fake, 16-B aligned device pointer: every case below is refused before it is read


def test_symbols_exported_declared_and_bound_at_abi_22():
    from fvp import _lib

    names = set(re.findall(r"\b(fvp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    assert set(NEW) <= names and names == set(_lib.SIGNATURES)
    lib = _lib.load()
    for n in NEW:
        assert hasattr(lib, n), n
    assert lib.fvp_abi_version() == _lib.ABI_VERSION == 22  # additive change


def test_render_f16_host_checks():
    from fvp import _lib

    f = _lib.load().fvp_render_keypoints_f16

    def call(joints=P, count=P, out=P, B=1, V=2, Pn=3, J=15, H=32, W=48, iw=192.0, ih=128.0, sigma=3.0, cp=16):
        return f(joints, 1, count, None, B, V, Pn, J, H, W, iw, ih, sigma, cp, out, None)

    assert call(joints=None) == 1001 and call(count=None) == 1001 and call(out=None) == 1001
    assert call(cp=8, J=8) == 1002             # Cp = 8: a lane owns 8 channels, a pixel is >= 2 lanes
    assert call(cp=16, J=17) == 1002           # Cp < J
    assert call(cp=48, J=15) == 1002 and call(cp=24, J=15) == 1002
    assert call(J=33, cp=32) == 1002 and call(Pn=33) == 1002 and call(B=0) == 1002 and call(H=0) == 1002
    assert call(sigma=0.0) == 1002 and call(iw=float("nan")) == 1002
    for off in (2, 4, 8):
        assert call(out=P + off) == 1002       # 16-B stores
    # the fp32 entry point applies the same checks (and keeps its 4-B alignment)
    g = _lib.load().fvp_render_keypoints
    assert g(None, 1, P, None, 1, 2, 3, 15, 32, 48, 192.0, 128.0, 3.0, 16, P, None) == 1001
    assert g(P, 1, P, None, 1, 2, 3, 17, 32, 48, 192.0, 128.0, 3.0, 16, P, None) == 1002


def test_conv1x1_cl_f16_host_checks():
    from fvp import _lib

    f = _lib.load().fvp_conv1x1_cl_f16

    def call(x=P, npix=35, cpi=256, w=P, ldw=128, cout=15, scale=P, shift=P, cp=16, out=P):
        return f(x, npix, cpi, w, ldw, cout, scale, shift, cp, out, None)

    for k in ("x", "w", "scale", "shift", "out"):
        assert call(**{k: None}) == 1001, k
    assert call(cp=8, cout=8) == 1002          # Cp = 8
    assert call(cp=16, cout=17) == 1002        # Cout > Cp
    assert call(cp=32, cout=33) == 1002
    assert call(cp=48, cout=40) == 1002
    assert call(cpi=24) == 1002                # Cpi % 16
    assert call(cpi=1024) == 1002 and call(cpi=0) == 1002 and call(cpi=528) == 1002
    assert call(npix=0) == 1002 and call(npix=-1) == 1002
    assert call(cout=0) == 1002 and call(ldw=8) == 1002  # a weight row shorter than Cout
    for off in (2, 4, 8):
        assert call(out=P + off) == 1002       # misaligned out
        assert call(x=P + off) == 1002


def test_fake_kernel_of_render_keypoints_f16():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from fvp import ops

    out = torch.ops.fvp.render_keypoints_f16(torch.zeros((1, 2, 3, 17, 2), dtype=torch.float64, device="meta"),
                                             torch.ones((1, 2), dtype=torch.int32, device="meta"), None, 192.0, 128.0,
                                             32, 48, 3.0)
    assert tuple(out.shape) == (1, 2, 32, 48, 32) and out.dtype == torch.float16
    with FakeTensorMode():
        j = torch.empty((2, 5, 4, 15, 2), dtype=torch.float32, device="cuda")
        c = torch.empty((2, 5), dtype=torch.int32, device="cuda")
        h = ops.render_keypoints_f16(j, c, None, 960.0, 512.0, 128, 240, 3.0)
        f = ops.render_keypoints(j, c, None, 960.0, 512.0, 128, 240, 3.0)
    assert tuple(h.shape) == (2, 5, 128, 240, 16) and h.dtype == torch.float16
    assert tuple(f.shape) == (2, 5, 128, 240, 16) and f.dtype == torch.float32


def test_option_defaults_and_dtype_checks():
    from fvp import _lib, integration
    from fvp.heatmaps import render_keypoints, share_channels_last

    assert integration.FvpOptions().heatmaps_dtype == torch.float32
    assert integration.install(modules={}) == {}  # (nothing to patch: just the options' construction)
    with pytest.raises(_lib.FvpError, match="heatmaps_dtype"):
        integration.install(modules={}, heatmaps_dtype=torch.bfloat16)

    class M:
        pass

    m = M()
    assert integration.set_options(m, heatmaps_dtype=torch.float16).heatmaps_dtype == torch.float16
    assert integration.options_of(m).heatmaps_dtype == torch.float16
    assert integration.set_options(m, heatmaps_dtype=None).heatmaps_dtype == torch.float32
    with pytest.raises(_lib.FvpError, match="heatmaps_dtype"):
        integration.set_options(m, heatmaps_dtype=torch.float64)

    joints = torch.zeros((1, 2, 3, 17, 2), dtype=torch.float64)
    count = torch.ones((1, 2), dtype=torch.int32)
    kw = dict(image_size=(192, 128), heatmap_size=(48, 32), sigma=3.0)
    with pytest.raises(_lib.FvpError, match="dtype"):
        render_keypoints(joints, count, dtype=torch.bfloat16, **kw)
    with pytest.raises(_lib.FvpError, match="dtype"):
        render_keypoints(joints, count, dtype=torch.float64, **kw)
    with pytest.raises(_lib.FvpError, match="HIP device"):  # fp16 is accepted: the next check speaks
        render_keypoints(joints, count, dtype=torch.float16, **kw)
    with pytest.raises(_lib.FvpError, match="dtype"):
        share_channels_last(torch.zeros((1, 2, 3, 4, 5)), dtype=torch.bfloat16)
    assert share_channels_last(torch.zeros((1, 2, 3, 4, 5)), dtype=torch.float16) is None  # CPU tensor: no copy


def test_head_route_of_cpu_built_backbones():
    """The route is decided from the final layer alone: 1x1 fp32 with J <= 32 -> the head kernel."""
    import cnn_arch
    from fvp.backbone import FvpPoseResNet

    for J, fk, dtype, want in ((15, 1, torch.float32, "conv1x1_cl_f16"), (32, 1, torch.float32, "conv1x1_cl_f16"),
                               (33, 1, torch.float32, "cast"), (15, 3, torch.float32, "cast"),
                               (15, 1, torch.bfloat16, "cast")):
        m = cnn_arch.PoseResNet(18, J, final_kernel=fk).eval()
        assert FvpPoseResNet(m, dtype).head_route() == want, (J, fk, dtype)
