"""GPU tests: fp16 channels-last heatmaps [B,V,H,W,Cp] read in place by every
gather (fvp_voxelize_cl_f16 and its _cams / _cams_slab twins, fvp_person_planes_cl_f16,
fvp_voxel_columns, fvp_nchw_to_nhwc_f16).

The contract is the planar fp16 route's: fp16 -> fp32 is exact and every fp32
operation after it is the reference's, so the results equal the oracle run on
``hm.half().float()`` bit for bit.  Expectations come from code these kernels
do not share: oracle.fvp_oracle (numpy), oracle.torch_cpu (F.grid_sample, for
non-finite pixels, where the oracle does not speak), the planar fp16 route
(pixel-pair table) and the fp32 channels-last person path.

Small geometry throughout: Shelf cameras, a 13 x 11 x 7 grid, 31 x 45 heatmaps.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle import fvp_oracle as O

pytestmark = pytest.mark.gpu

BINS, HM = (13, 11, 7), (45, 31)  # heatmap_size is (W, H)
NAN16 = 0x7E00


def _workload(J, base="c2", bins=BINS, hm=HM, **kw):
    from fvp.workloads import WORKLOADS

    return dataclasses.replace(WORKLOADS[base], num_joints=J, voxels_per_axis=bins, heatmap_size=hm, **kw)


def _layer(w, dev, otf):
    from fvp.project_whole import ProjectLayer

    layer = ProjectLayer(w.cfg(str(dev)))
    layer.verbose = False
    layer.on_the_fly = otf
    return layer


def _rt(w):
    from fvp import geometry

    return torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float)


@functools.lru_cache(maxsize=None)
def _oracle_grid(base, bins, hm, space, shift):
    """The oracle's sample grid [V, N, 2] (J does not enter)."""
    from fvp import geometry

    w = _workload(1, base=base, bins=bins, hm=hm, **({"space_size": space} if space else {}))
    cams, seq = w.cameras()
    rt = _rt(w).numpy().copy()
    if shift is not None:
        rt[:, 2] = shift
    grid = O.compute_grid(w.space_size, w.space_center, bins)
    return np.stack([O.project_grid(grid, c, w.ori_image_size, w.image_size, hm, rt)
                     for c in geometry.camera_list(cams, seq)])


def _to_cl(hm16, cp, fill=NAN16):
    """[B,V,J,H,W] fp16 -> [B,V,H,W,cp] fp16 with the bit pattern `fill` (a NaN) in channels J..cp-1."""
    B, V, J, H, W = hm16.shape
    cl = torch.full((B, V, H, W, cp), fill, dtype=torch.int16).view(torch.float16)
    cl[..., :J] = hm16.permute(0, 1, 3, 4, 2)
    return cl


def _obj(hm16, cp, dev):
    from fvp.heatmaps import ChannelsLastHeatmaps

    return ChannelsLastHeatmaps(_to_cl(hm16, cp).to(dev), hm16.shape[2])


def _eq(a, b, what):
    np.testing.assert_array_equal(a.cpu().numpy() if isinstance(a, torch.Tensor) else a,
                                  b.cpu().numpy() if isinstance(b, torch.Tensor) else b, err_msg=what)


# -- 1. lane-group sizes and pitches ------------------------------------------------------------
@pytest.mark.parametrize("otf", [False, True], ids=["grid", "onthefly"])
@pytest.mark.parametrize("J,cp", [(3, 8), (8, 8), (9, 16), (15, 16), (15, 32), (16, 16), (17, 32), (32, 32), (40, 48)])
def test_lane_groups_and_pitches_vs_oracle(gpu_device, J, cp, otf):
    """1 / 2 / 4 lanes per voxel, pitches beyond the joints (NaN bit patterns in the
    padding channels must not reach the output) and the 32-joint slices of J = 40."""
    from fvp import synthetic

    w = _workload(J)
    layer = _layer(w, gpu_device, otf)
    cams, seq = w.cameras()
    rt = _rt(w).to(gpu_device)
    hm = synthetic.uniform_heatmaps(w, 3, seed=100 * J + cp).half()
    meta = {"seq": [seq] * 3}
    cube, xy = layer.forward_fused(_obj(hm, cp, gpu_device), meta, cams, rt)
    assert cube.dtype == torch.float32 and tuple(cube.shape) == (3, J) + BINS
    sg = _oracle_grid("c2", BINS, HM, None, None)
    for b in range(3):
        ref = O.voxelize(hm[b].float().numpy(), sg).reshape(J, *BINS)
        _eq(cube[b], ref, f"cube frame {b}")
        _eq(xy[b], O.xy_plane(ref), f"xy frame {b}")
    c_pl, x_pl = layer.forward_fused(hm.to(gpu_device), meta, cams, rt)  # the planar fp16 route
    _eq(cube, c_pl, "cube vs planar fp16")
    _eq(xy, x_pl, "xy vs planar fp16")


# -- 2. every image edge ------------------------------------------------------------------------
EDGE_SPACE, EDGE_SHIFT = (12000.0, 12000.0, 6000.0), -8.0


@pytest.mark.parametrize("otf", [False, True], ids=["grid", "onthefly"])
def test_every_image_edge_nonfinite_ring(gpu_device, otf):
    """The border ring of view 0 is NaN, of view 1 +inf; the grid reaches past all
    four sides of every view, so taps straddle every edge (x0 = -1, W-1; y0 = -1,
    H-1): zero padding must hold per tap -- what a pair load or a row wrap breaks.

    Shelf's own resize transform adds +3.2 px in y after the reference's clip of the
    projected pixel to >= -1, so y0 = -1 cannot occur with it; the test passes the
    same scale with a translation of -8 px (the transform is an argument of forward)
    and a 12 x 12 x 6 m space."""
    from oracle import torch_cpu

    J, cp, W, H = 15, 16, HM[0], HM[1]
    w = _workload(J, space_size=EDGE_SPACE)
    sg = _oracle_grid("c2", BINS, HM, EDGE_SPACE, EDGE_SHIFT)
    ix = (sg[..., 0] + np.float32(1)) * np.float32((W - 1) / 2)
    iy = (sg[..., 1] + np.float32(1)) * np.float32((H - 1) / 2)
    x0, y0 = np.floor(ix).astype(int), np.floor(iy).astype(int)
    for v in range(sg.shape[0]):
        for name, hit in (("x0=-1", x0[v] == -1), ("x0=W-1", x0[v] == W - 1), ("y0=-1", y0[v] == -1),
                          ("y0=H-1", y0[v] == H - 1)):
            assert hit.any(), f"view {v}: no tap with {name}"
    layer = _layer(w, gpu_device, otf)
    cams, seq = w.cameras()
    rt = _rt(w)
    rt[:, 2] = EDGE_SHIFT
    g = torch.Generator().manual_seed(2)
    hm = torch.rand((3, 5, J, H, W), generator=g)
    for v, val in ((0, float("nan")), (1, float("inf"))):
        hm[:, v, :, 0, :] = val
        hm[:, v, :, H - 1, :] = val
        hm[:, v, :, :, 0] = val
        hm[:, v, :, :, W - 1] = val
    hm = hm.half()
    meta = {"seq": [seq] * 3}
    cube, xy = layer.forward_fused(_obj(hm, cp, gpu_device), meta, cams, rt.to(gpu_device))
    c_pl, x_pl = layer.forward_fused(hm.to(gpu_device), meta, cams, rt.to(gpu_device))
    _eq(cube, c_pl, "cube vs planar fp16 (NaN positions included)")
    _eq(xy, x_pl, "xy vs planar fp16")
    dsg = layer.build_sample_grid(cams, seq, rt.to(gpu_device), gpu_device).cpu().contiguous()
    ref = torch_cpu.voxelize(hm.float(), dsg, BINS)
    assert torch.isnan(ref).any() and not torch.isnan(ref).all()
    _eq(cube, ref, "cube vs torch grid_sample")
    _eq(xy, torch.max(ref, dim=4)[0], "xy vs torch")


# -- 3. buffer ends -----------------------------------------------------------------------------
def test_buffer_ends_guarded_by_nan(gpu_device):
    """The tensor is a view 16 B into a larger buffer and ends 16 B before its end,
    the guard bytes hold NaN.  A sample grid assigned from outside puts voxel 0 of
    every view on pixel (0, 0) and the last voxel on pixel (H-1, W-1) exactly (the
    three other taps of the latter lie past the image: past the buffer's end for
    the last view of the last frame), the rest anywhere in [-1.1, 1.1]."""
    from fvp.heatmaps import ChannelsLastHeatmaps

    J, cp, B, V, W, H = 15, 16, 3, 5, HM[0], HM[1]
    w = _workload(J)
    layer = _layer(w, gpu_device, False)
    cams, seq = w.cameras()
    N = BINS[0] * BINS[1] * BINS[2]
    g = torch.Generator().manual_seed(3)
    sg = torch.rand((V, N, 2), generator=g) * 2.2 - 1.1
    sg[:, 0] = -1.0
    sg[:, N - 1] = 1.0
    hm = torch.rand((B, V, J, H, W), generator=g).half()
    hm[0, 0, :, 0, 0] = 1.0   # the first pixel of the buffer
    hm[B - 1, V - 1, :, H - 1, W - 1] = 1.0   # the last
    n = B * V * H * W * cp
    buf = torch.full((n + 16,), NAN16, dtype=torch.int16).view(torch.float16).to(gpu_device)
    view = buf[8:8 + n].view(B, V, H, W, cp)
    view.copy_(_to_cl(hm, cp).to(gpu_device))
    assert view.data_ptr() == buf.data_ptr() + 16 and view.data_ptr() % 16 == 0
    assert torch.isnan(buf[:8]).all() and torch.isnan(buf[-8:]).all()
    layer.sample_grid[seq] = sg.unsqueeze(1).to(gpu_device)
    cube, xy = layer.forward_fused(ChannelsLastHeatmaps(view, J), {"seq": [seq] * B}, cams, _rt(w).to(gpu_device))
    assert not torch.isnan(cube).any()
    for b in range(B):
        ref = O.voxelize(hm[b].float().numpy(), sg.numpy()).reshape(J, *BINS)
        _eq(cube[b], ref, f"cube frame {b}")
        _eq(xy[b], O.xy_plane(ref), f"xy frame {b}")
    # voxel 0 of frame 0 and the last voxel of the last frame see the marked pixels through 1 of V views
    first = O.voxelize(hm[0].float().numpy(), sg.numpy())[:, 0]
    assert (first >= np.float32(1.0) / np.float32(V)).all()
    assert (cube[B - 1].reshape(J, N)[:, N - 1].cpu().numpy() >= np.float32(1.0) / np.float32(V)).all()


# -- 4 / 5. the 16-camera cascade, x-slabs ------------------------------------------------------
RING_BINS = (24, 20, 12)


@functools.lru_cache(maxsize=None)
def _ring_case():
    from fvp import synthetic

    w = _workload(15, base="c5", bins=RING_BINS)
    hm = synthetic.uniform_heatmaps(w, 4, seed=31).half()
    sg = _oracle_grid("c5", RING_BINS, HM, None, None)
    assert sg.shape[0] == 31
    ref0 = O.voxelize(hm[0].float().numpy(), sg).reshape(15, *RING_BINS)
    return w, hm, ref0


@pytest.mark.parametrize("otf", [False, True], ids=["grid", "onthefly"])
@pytest.mark.parametrize("B", [1, 4])
def test_cascade_31_cameras(gpu_device, B, otf):
    """31 ring cameras: the mean folds complete blocks of 16 cameras (torch's CPU
    sum order); == the planar fp16 route, frame 0 == the oracle."""
    w, hm4, ref0 = _ring_case()
    hm = hm4[:B]
    layer = _layer(w, gpu_device, otf)
    cams, seq = w.cameras()
    rt = _rt(w).to(gpu_device)
    meta = {"seq": [seq] * B}
    cube, xy = layer.forward_fused(_obj(hm, 16, gpu_device), meta, cams, rt)
    c_pl, x_pl = layer.forward_fused(hm.to(gpu_device), meta, cams, rt)
    _eq(cube, c_pl, "cube vs planar fp16")
    _eq(xy, x_pl, "xy vs planar fp16")
    _eq(cube[0], ref0, "frame 0 vs oracle")
    _eq(xy[0], O.xy_plane(ref0), "xy frame 0 vs oracle")


@pytest.mark.parametrize("otf", [False, True], ids=["grid", "onthefly"])
def test_cascade_two_complete_blocks_40_views(gpu_device, otf):
    """40 views (the ring and its first 9 cameras again): two complete 16-camera
    blocks fold before the remainder -- the cached-grid kernel keeps their sum in
    LDS, so the second fold adds to a parked value.  J = 32: 4 lanes per voxel."""
    from fvp import geometry

    J, V, bins = 32, 40, (8, 6, 5)
    w = _workload(J, base="c5", bins=bins)
    ring, seq = w.cameras()
    cams = {seq: list(ring[seq]) + list(ring[seq])[:V - 31]}
    layer = _layer(w, gpu_device, otf)
    rt = _rt(w)
    g = torch.Generator().manual_seed(40)
    hm = torch.rand((2, V, J, HM[1], HM[0]), generator=g).half()
    meta = {"seq": [seq] * 2}
    cube, xy = layer.forward_fused(_obj(hm, 32, gpu_device), meta, cams, rt.to(gpu_device))
    c_pl, x_pl = layer.forward_fused(hm.to(gpu_device), meta, cams, rt.to(gpu_device))
    _eq(cube, c_pl, "cube vs planar fp16")
    _eq(xy, x_pl, "xy vs planar fp16")
    grid = O.compute_grid(w.space_size, w.space_center, bins)
    sg = np.stack([O.project_grid(grid, c, w.ori_image_size, w.image_size, HM, rt.numpy())
                   for c in geometry.camera_list(cams, seq)])
    ref = O.voxelize(hm[1].float().numpy(), sg).reshape(J, *bins)
    _eq(cube[1], ref, "frame 1 vs oracle")
    _eq(xy[1], O.xy_plane(ref), "xy frame 1 vs oracle")


@pytest.mark.parametrize("otf", [False, True], ids=["grid", "onthefly"])
def test_x_slabs_equal_unsplit_cube(gpu_device, otf):
    """Two x-slabs (on the fly: fvp_voxelize_cl_cams_slab_f16) == the rows of the whole-grid cube."""
    w, hm, _ = _ring_case()
    layer = _layer(w, gpu_device, otf)
    cams, seq = w.cameras()
    rt = _rt(w).to(gpu_device)
    meta = {"seq": [seq] * hm.shape[0]}
    obj = _obj(hm, 16, gpu_device)
    cube, xy = layer.forward_fused(obj, meta, cams, rt)
    X = RING_BINS[0]
    for x0, x1 in ((0, X // 2), (X // 2, X)):
        c, p = layer.forward_slab(obj, meta, cams, rt, x0, x1)
        _eq(c, cube[:, :, x0:x1], f"slab [{x0},{x1}) cube")
        _eq(p, xy[:, :, x0:x1], f"slab [{x0},{x1}) xy")


# -- 6. batch position, mixed sequences ---------------------------------------------------------
@pytest.mark.parametrize("otf", [False, True], ids=["grid", "onthefly"])
def test_batch_position_invariance_mixed_sequences(gpu_device, otf):
    from fvp import synthetic
    from fvp.heatmaps import ChannelsLastHeatmaps

    J = 15
    w = _workload(J)
    layer = _layer(w, gpu_device, otf)
    cams, seq = w.cameras()
    shelf = cams[seq]
    order = sorted(shelf.keys(), reverse=True) if isinstance(shelf, dict) else None
    other = {i: shelf[k] for i, k in enumerate(order)} if order is not None else list(reversed(shelf))
    cams2 = {"a": shelf, "b": other}
    rt = _rt(w).to(gpu_device)
    hm = synthetic.uniform_heatmaps(w, 5, seed=6).half()
    obj = _obj(hm, 16, gpu_device)
    meta = {"seq": ["a", "b", "b", "a", "b"]}
    cube, xy = layer.forward_fused(obj, meta, cams2, rt)
    for b, s in enumerate(meta["seq"]):
        one = ChannelsLastHeatmaps(obj.t[b:b + 1], J)
        c1, x1 = layer.forward_fused(one, {"seq": [s]}, cams2, rt)
        _eq(c1[0], cube[b], f"frame {b} cube")
        _eq(x1[0], xy[b], f"frame {b} xy")
    assert not torch.equal(cube[0], layer.forward_fused(ChannelsLastHeatmaps(obj.t[0:1], J), {"seq": ["b"]}, cams2,
                                                        rt)[0][0])


# -- 7. columns ---------------------------------------------------------------------------------
@pytest.mark.parametrize("otf", [False, True], ids=["grid", "onthefly"])
@pytest.mark.parametrize("J,cp", [(15, 16), (40, 48)])
def test_columns_equal_cube_columns(gpu_device, J, cp, otf):
    from fvp import synthetic

    w = _workload(J)
    layer = _layer(w, gpu_device, otf)
    cams, seq = w.cameras()
    rt = _rt(w).to(gpu_device)
    hm = synthetic.uniform_heatmaps(w, 3, seed=100 * J + cp).half()
    obj = _obj(hm, cp, gpu_device)
    meta = {"seq": [seq] * 3}
    cube, _ = layer.forward_fused(obj, meta, cams, rt)
    XY = BINS[0] * BINS[1]
    flat = torch.tensor([[0, XY - 1, 57, XY], [5, 5, -1, 100], [XY - 1, 0, 1, 2]], dtype=torch.int64, device=gpu_device)
    cols = layer.columns(obj, meta, cams, rt, flat)
    assert tuple(cols.shape) == (3, 4, J, BINS[2])
    c = cube.reshape(3, J, XY, BINS[2]).cpu()
    for b in range(3):
        for k in range(4):
            f = int(flat[b, k])
            if 0 <= f < XY:
                _eq(cols[b, k], c[b, :, f], f"column b={b} k={k}")
            else:
                assert torch.isnan(cols[b, k]).all()


# -- 8. person planes ---------------------------------------------------------------------------
def _person_case(dev, J, S, frames=2):
    from fvp import geometry, synthetic
    from fvp.project_individual import ProjectLayer
    from fvp.workloads import WORKLOADS

    space = 2000.0  # a 2 m capture space keeps the fine grid small (S^3 x 6 slots)
    w = dataclasses.replace(WORKLOADS["c3"], num_joints=J, space_size=(space,) * 3, ind_space_size=(space,) * 3,
                            ind_voxels_per_axis=(S, S, S), heatmap_size=HM)
    layer = ProjectLayer(w.cfg(str(dev)))
    layer.verbose = False
    layer.on_the_fly = False
    cams, seq = w.cameras()
    cams = dict(cams)
    cams["other"] = list(reversed(list(cams[seq])))
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(dev)
    hm = synthetic.uniform_heatmaps(w, frames, seed=J + S).half()
    return w, layer, cams, seq, rt, hm


def _cl32(hm16, cp, dev):
    """The fp32 channels-last copy of hm.half().float() (junk 9.0 in the padding)."""
    from fvp.heatmaps import ChannelsLastHeatmaps

    B, V, J, H, W = hm16.shape
    cl = torch.full((B, V, H, W, cp), 9.0)
    cl[..., :J] = hm16.float().permute(0, 1, 3, 4, 2)
    return ChannelsLastHeatmaps(cl.to(dev), J)


@pytest.mark.parametrize("J", [15, 17, 40])
@pytest.mark.parametrize("S", [32, 80])
def test_person_planes_equal_fp32_channels_last(gpu_device, J, S):
    """6 proposals over 2 frames of two sequences: in-window, clipped (window cut by
    the space's border), skipped (window outside the space) and masked-out ones;
    32^3 and 80^3 (two 64-deep z chunks); 2 / 4 lanes per voxel and a 32 + 8 joint
    slice pair.  Planes, cubes and offsets == the fp32 channels-last person path on
    hm.half().float(), bit for bit."""
    w, layer, cams, seq, rt, hm = _person_case(gpu_device, J, S)
    c = w.space_center
    props = torch.tensor([[[c[0], c[1], c[2], 0, 0.9, 0.5, 0.5],
                           [c[0] + 800, c[1] - 900, c[2] - 300, 0, 0.8, 0.2, 0.9],      # clipped
                           [c[0] + 9000, c[1], c[2], 0, 0.7, 0.5, 0.5],                 # skipped
                           [c[0] - 100, c[1] + 50, c[2], 0, 0.6, 1.1, 0.3]],
                          [[c[0] - 700, c[1] + 500, c[2] + 300, 0, 0.7, 1.1, 0.3],      # clipped
                           [c[0] + 300, c[1] - 200, c[2] - 100, 0, 0.8, -0.2, 0.9],
                           [c[0], c[1], c[2], 0, 0.1, 0.5, 0.5],
                           [c[0] + 50, c[1] + 50, c[2] + 50, 0, 0.9, 0.4, 0.6]]], dtype=torch.float32).to(gpu_device)
    mask = torch.tensor([[True, True, True, False], [True, True, False, True]], device=gpu_device)
    cp = 8 * ((J + 7) // 8)
    h16, f32 = _obj(hm, cp, gpu_device), _cl32(hm, 4 * ((J + 3) // 4) if J > 32 else 32, gpu_device)
    for meta in ({"seq": [seq, seq]}, {"seq": [seq, "other"]}):
        p1, o1, f1 = layer.forward_batch(h16, meta, props, mask, cams, rt)
        p2, o2, f2 = layer.forward_batch(f32, meta, props, mask, cams, rt)
        assert p1.shape[0] == 3 * 6 and p1.dtype == torch.float32
        _eq(p1, p2, f"planes {meta}")
        _eq(o1, o2, "offsets")
        assert torch.equal(f1, f2)
        assert p1.max() > 0 and (p1[2] == 0).all()  # the skipped proposal's xy planes are empty
    meta = {"seq": [seq, "other"]}
    a = layer.forward_planes(h16, 1, meta, props[1], cams, rt)
    b = layer.forward_planes(f32, 1, meta, props[1], cams, rt)
    _eq(a[0], b[0], "forward_planes")
    _eq(a[1], b[1], "forward_planes offset")
    ca, cb = layer(h16, 0, meta, props[0, :3], cams, rt), layer(f32, 0, meta, props[0, :3], cams, rt)
    _eq(ca[0], cb[0], "cubes")
    _eq(ca[1], cb[1], "cube offsets")


def test_person_planes_many_proposals_direct_xy(gpu_device):
    """128 proposals x 32 rows = 4096 rows: one x part per row, so each block stores
    its row's xy maxima from LDS without atomics (the route of full JLN batches)."""
    J, S = 15, 32
    w, layer, cams, seq, rt, hm = _person_case(gpu_device, J, S)
    c = w.space_center
    g = torch.Generator().manual_seed(8)
    props = torch.zeros((2, 64, 7))
    props[..., :3] = torch.tensor(c) + (torch.rand((2, 64, 3), generator=g) - 0.5) * 1800.0
    props[..., 4] = 0.9
    props[..., 5:] = torch.rand((2, 64, 2), generator=g) * 1.2
    props = props.to(gpu_device)
    mask = torch.ones((2, 64), dtype=torch.bool, device=gpu_device)
    meta = {"seq": [seq, seq]}
    p1, o1, _ = layer.forward_batch(_obj(hm, 16, gpu_device), meta, props, mask, cams, rt)
    p2, o2, _ = layer.forward_batch(_cl32(hm, 16, gpu_device), meta, props, mask, cams, rt)
    _eq(p1, p2, "planes")
    _eq(o1, o2, "offsets")
    assert p1.max() > 0


# -- 9. the layout kernel -----------------------------------------------------------------------
@pytest.mark.parametrize("src", [torch.float32, torch.float16], ids=["from_f32", "from_f16"])
@pytest.mark.parametrize("shape", [(1, 2, 15, 31, 45), (1, 1, 3, 2, 2), (3, 1, 32, 5, 7)])
def test_planar_to_channels_last_half(gpu_device, shape, src):
    """== x.half() permuted, zeros in the padding channels: round to nearest even at
    fp16 ties, subnormals, +-inf, NaN and overflow beyond 65504.  Non-NaN values are
    compared by bits; NaN by position (its payload is not part of the rounding rule)."""
    from fvp.heatmaps import to_channels_last

    B, V, J, H, W = shape
    g = torch.Generator().manual_seed(9)
    x = torch.rand(shape, generator=g) * 2 - 1
    special = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 2.0 ** -24,
                            2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25, 6.0e-8, -6.0e-8, 0.0, -0.0,
                            float("inf"), float("-inf"), float("nan"), 65504.0, 65519.0, 65520.0, 1.0e9, -70000.0,
                            1.0e-40, 2.0 ** -126])
    flat = x.view(-1)
    n = min(flat.numel(), special.numel())
    pos = torch.randperm(flat.numel(), generator=g)[:n]
    flat[pos] = special[:n]
    x = x.to(src)
    cl = to_channels_last(x.to(gpu_device), dtype=torch.float16)
    cp = 16 * ((J + 15) // 16)
    assert cl.dtype == torch.float16 and cl.cp == cp and cl.shape == shape and cl.t.is_contiguous()
    want = torch.zeros((B, V, H, W, cp), dtype=torch.float16)
    want[..., :J] = x.half().permute(0, 1, 3, 4, 2)
    got = cl.t.cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
    back = cl.planar()
    assert back.dtype == torch.float16 and tuple(back.shape) == shape
    bn = torch.isnan(x.half())
    assert torch.equal(back.cpu().view(torch.int16)[~bn], x.half().view(torch.int16)[~bn])
    from fvp.heatmaps import channels_last_of
    assert channels_last_of(back) is cl and cl.half() is cl
    # the fp32 object's .half(): a cast of the same values
    if src == torch.float32 and J <= 32 and not torch.isnan(x).any():
        h = to_channels_last(x.to(gpu_device)).half()
        assert h.dtype == torch.float16 and torch.equal(h.t[..., :J].cpu(), want[..., :J])


# -- 10. rejections -----------------------------------------------------------------------------
def test_rejections(gpu_device):
    from fvp import _lib, synthetic
    from fvp.heatmaps import ChannelsLastHeatmaps, attach, to_channels_last

    J = 15
    w = _workload(J)
    layer = _layer(w, gpu_device, False)
    cams, seq = w.cameras()
    rt = _rt(w).to(gpu_device)
    hm = synthetic.uniform_heatmaps(w, 1, seed=1).half()
    meta = {"seq": [seq]}
    good = _to_cl(hm, 16, 0).to(gpu_device)
    with pytest.raises(_lib.FvpError, match="bfloat16"):
        ChannelsLastHeatmaps(good.to(torch.bfloat16), J)
    with pytest.raises(_lib.FvpError, match="bfloat16"):
        to_channels_last(hm.to(gpu_device), dtype=torch.bfloat16)
    with pytest.raises(_lib.FvpError, match="Cp % 8"):
        ChannelsLastHeatmaps(_to_cl(hm, 20, 0).to(gpu_device), J)
    with pytest.raises(_lib.FvpError, match="contiguous"):
        ChannelsLastHeatmaps(_to_cl(hm, 32, 0).to(gpu_device)[..., :16], J)
    buf = torch.zeros((good.numel() + 8,), dtype=torch.float16, device=gpu_device)
    off = buf[4:4 + good.numel()].view(good.shape)  # 8 B into the buffer
    with pytest.raises(_lib.FvpError, match="aligned"):
        ChannelsLastHeatmaps(off, J)
    from fvp import ops
    with pytest.raises(_lib.FvpError):  # the C ABI's own check, behind the constructor's
        grids, index = layer._grids_for_batch(hm.to(gpu_device), meta, cams, rt)
        ops.voxelize_cl.impl(off, J, grids, index, *BINS, True, True)
    with pytest.raises(_lib.FvpError, match="HIP device"):
        layer.forward_fused(ChannelsLastHeatmaps(good.cpu(), J), meta, cams, rt)
    planar = hm.to(gpu_device).float().requires_grad_(True)
    with pytest.raises(_lib.FvpError, match="requires grad"):
        layer.forward_fused(attach(planar, ChannelsLastHeatmaps(good, J)), meta, cams, rt)
    # no fp16 channels-last kernel projects the fine grid on the fly: an error naming the dtype, never a conversion
    wp, player, pcams, pseq, prt, phm = _person_case(gpu_device, J, 32, frames=1)
    player.on_the_fly = True
    c = wp.space_center
    props = torch.tensor([[c[0], c[1], c[2], 0, 0.9, 0.5, 0.5]], dtype=torch.float32, device=gpu_device)
    obj = _obj(phm, 16, gpu_device)
    for call in (lambda: player.forward_planes(obj, 0, {"seq": [pseq]}, props, pcams, prt),
                 lambda: player(obj.planar(), 0, {"seq": [pseq]}, props, pcams, prt)):
        with pytest.raises(_lib.FvpError, match="float16"):
            call()
