"""CPU tests of the fp16 channels-last entry points: the host-side argument checks
run before any launch (no GPU), the header and the ctypes table agree, and
ChannelsLastHeatmaps describes fp16 tensors."""
import os
import re

import pytest
import torch

from conftest import REPO

HEADER = os.path.join(REPO, "include", "fvp.h")
NEW = ["fvp_voxelize_cl_f16", "fvp_voxelize_cl_cams_f16", "fvp_voxelize_cl_cams_slab_f16",
       "fvp_person_planes_cl_f16", "fvp_nchw_to_nhwc_f16"]
P = 4096  # a fake, 16-B aligned device pointer: every case below is refused before it is read


def test_declared_set_equals_signatures_at_abi_22():
    from fvp import _lib

    names = set(re.findall(r"\b(fvp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    assert set(NEW) <= names
    assert names == set(_lib.SIGNATURES)
    lib = _lib.load()
    for n in NEW:
        assert hasattr(lib, n), n
    assert lib.fvp_abi_version() == _lib.ABI_VERSION == 22  # additive change


def _grid_img():
    from fvp import _lib

    g = _lib.GridSpec((-4000.0,) * 3, (4000.0,) * 3, (0.0,) * 3, (8, 8, 4))
    im = _lib.ImageSpec(1920.0, 960.0, 512.0, 45, 31)
    return g, im


def _calls(lib):
    """name -> f(hm, cp, J) with every other argument valid."""
    from fvp import _lib

    g, im = _grid_img()
    spec = _lib.PersonSpec((32, 32, 32), (0.03,) * 3, (0.0,) * 3, (2000.0,) * 3, (2000.0,) * 3, (32, 32, 32))
    return {
        "fvp_voxelize_cl_f16": lambda hm, cp, J: lib.fvp_voxelize_cl_f16(hm, cp, 1, 5, J, 31, 45, P, None, 8, 8, 4, P,
                                                                         None, None),
        "fvp_voxelize_cl_cams_f16": lambda hm, cp, J: lib.fvp_voxelize_cl_cams_f16(hm, cp, 1, 5, J, 31, 45, P, None, P,
                                                                                   g, im, P, None, None),
        "fvp_voxelize_cl_cams_slab_f16": lambda hm, cp, J: lib.fvp_voxelize_cl_cams_slab_f16(
            hm, cp, 1, 5, J, 31, 45, P, None, P, g, im, 0, 4, P, None, None),
        "fvp_person_planes_cl_f16": lambda hm, cp, J: lib.fvp_person_planes_cl_f16(hm, cp, 1, 5, J, 31, 45, P, spec, P,
                                                                                   None, 1, None, P, None, None),
    }


@pytest.mark.parametrize("name", NEW[:4])
def test_gather_entry_points_check_arguments_on_the_host(name):
    from fvp import _lib

    f = _calls(_lib.load())[name]
    assert f(None, 16, 15) == 1001                # NULL heatmaps
    assert f(P, 12, 9) == 1002                    # cp % 8 != 0
    assert f(P, 20, 15) == 1002
    assert f(P, 8, 9) == 1002                     # cp < J
    assert f(P, 1032, 1025) == 1002               # J > FVP_MAX_JOINTS (1024)
    for off in (2, 4, 8):
        assert f(P + off, 16, 15) == 1002         # base pointer not 16-B aligned


def test_other_null_pointers_and_32_bit_offsets():
    from fvp import _lib

    lib = _lib.load()
    g, im = _grid_img()
    assert lib.fvp_voxelize_cl_f16(P, 16, 1, 5, 15, 31, 45, None, None, 8, 8, 4, P, None, None) == 1001  # no grid
    assert lib.fvp_voxelize_cl_cams_f16(P, 16, 1, 5, 15, 31, 45, None, None, P, g, im, P, None, None) == 1001
    assert lib.fvp_voxelize_cl_cams_f16(P, 16, 1, 5, 15, 31, 45, P, None, P, None, im, P, None, None) == 1001
    assert lib.fvp_voxelize_cl_cams_slab_f16(P, 16, 1, 5, 15, 31, 45, P, None, P, g, im, 4, 4, P, None, None) == 1002
    assert lib.fvp_person_planes_cl_f16(P, 16, 1, 5, 15, 31, 45, None, None, P, None, 1, None, P, None, None) == 1001
    # one camera image beyond 32-bit tap offsets: H * W * cp * 2 bytes >= 2^31
    assert lib.fvp_voxelize_cl_f16(P, 1024, 1, 5, 15, 1024, 1024, P, None, 8, 8, 4, P, None, None) == 1002
    assert lib.fvp_nchw_to_nhwc_f16(None, 0, 1, 15, 31, 45, 16, P, None) == 1001
    assert lib.fvp_nchw_to_nhwc_f16(P, 0, 1, 15, 31, 45, 16, None, None) == 1001
    assert lib.fvp_nchw_to_nhwc_f16(P, 0, 1, 15, 31, 45, 12, P, None) == 1002       # Cp % 8
    assert lib.fvp_nchw_to_nhwc_f16(P, 1, 1, 15, 31, 45, 8, P, None) == 1002        # Cp < C
    assert lib.fvp_nchw_to_nhwc_f16(P, 0, 1, 15, 31, 45, 16, P + 8, None) == 1002   # 16-B stores
    assert lib.fvp_nchw_to_nhwc_f16(P, 0, 0, 15, 31, 45, 16, P, None) == 1002


def test_channels_last_heatmaps_describe_fp16_cpu_tensors():
    from fvp import _lib
    from fvp.heatmaps import ChannelsLastHeatmaps

    t = torch.zeros((2, 5, 31, 45, 16), dtype=torch.float16)
    cl = ChannelsLastHeatmaps(t, 15)
    assert cl.shape == (2, 5, 15, 31, 45) and cl.cp == 16 and cl.dtype == torch.float16 and cl.half() is cl
    assert cl.device.type == "cpu"
    f32 = ChannelsLastHeatmaps(torch.zeros((1, 1, 2, 2, 4)), 3)
    assert f32.dtype == torch.float32 and f32.cp == 4  # fp32 keeps any pitch
    for bad in (torch.zeros((2, 5, 31, 45, 16), dtype=torch.bfloat16), torch.zeros((2, 5, 31, 45, 16), dtype=torch.float64),
                torch.zeros((2, 5, 31, 45, 12), dtype=torch.float16), torch.zeros((2, 5, 31, 45, 32), dtype=torch.float16)[..., :16],
                torch.zeros((2 * 5 * 31 * 45 * 16 + 8,), dtype=torch.float16)[4:-4].view(2, 5, 31, 45, 16)):
        with pytest.raises(_lib.FvpError):
            ChannelsLastHeatmaps(bad, 15)


def test_fake_kernels_keep_shapes_for_fp16():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from fvp import ops

    with FakeTensorMode():
        hm = torch.empty((2, 5, 16, 24, 16), dtype=torch.float16, device="cuda")
        cube, xy = ops.voxelize_cl(hm, 15, torch.empty((4 * 4 * 3, 6, 2), device="cuda"), None, 4, 4, 3, True, True)
        cols = ops.voxel_columns(hm, 15, torch.empty((4 * 4 * 3, 6, 2), device="cuda"), None, None, None, [0.0] * 3,
                                 [0.0] * 3, [0.0] * 3, [4, 4, 3], 0.0, 0.0, 0.0,
                                 torch.empty((2, 3), dtype=torch.int64, device="cuda"))
        pl = ops.person_planes_cl(hm, 15, torch.empty((8 * 8 * 4, 6, 2), device="cuda"),
                                  torch.empty((3, 7), device="cuda"), None, [8, 8, 4], [1.0] * 3, [0.0] * 3, [1.0] * 3,
                                  [1.0] * 3, [4, 4, 4], False, True)
    assert tuple(cube.shape) == (2, 15, 4, 4, 3) and cube.dtype == torch.float32
    assert tuple(xy.shape) == (2, 15, 4, 4) and xy.dtype == torch.float32
    assert tuple(cols.shape) == (2, 3, 15, 3) and cols.dtype == torch.float32
    assert tuple(pl[1].shape) == (9, 15, 4, 4) and pl[1].dtype == torch.float32 and pl[2].dtype == torch.float32
