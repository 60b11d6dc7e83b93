"""GPU: every case of the voxelize case table (voxelize_cases.py: each gather
instantiation, each gather_cfg class, the stage / epilogue classes, the frame
groupings and multi-chunk calls, the joint slices, the camera counts) through
the product's own op for its entry kind and through that kind's C entry point on
caller-owned, guarded buffers, bit for bit against oracle.fvp_oracle.voxelize /
xy_plane, frame by frame.  Before the calls the plan reported for the arguments
must be the class the case stands for."""
import numpy as np
import pytest
import torch

import voxelize_cases as VC
from oracle import fvp_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4
FILL = 0.90  # least share of nonzero voxels, and of distinct values per joint, in the oracle cube of a case


def _assert_same(got, ref, what):
    assert got.shape == ref.shape, what
    diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    assert not np.isnan(got).any(), f"{what}: NaN in the output"
    assert np.nanmax(diff) <= TOL, f"{what}: max |diff| {np.nanmax(diff)} > {TOL}"
    assert np.array_equal(got, ref), f"{what}: not bit-exact ({np.count_nonzero(diff)} of {diff.size} differ, " \
                                     f"max {np.nanmax(diff)})"


def _channels_last(hm, J, half):
    from fvp import heatmaps

    if half or J <= 32:
        return heatmaps.to_channels_last(hm, dtype=torch.float16 if half else None)
    B, V, _, H, W = hm.shape
    t = torch.zeros((B, V, H, W, 16 * ((J + 15) // 16)), dtype=torch.float32, device=hm.device)
    t[..., :J] = hm.permute(0, 1, 3, 4, 2)
    return heatmaps.ChannelsLastHeatmaps(t, J)


def _assert_plan(c, recs):
    """The plan reported for the case's arguments is the class the case stands for."""
    assert all(r.status == 0 for r in recs), recs
    fam = ((4 if c.otf else 3) if c.kind == "cl_f16" else (2 if c.otf else 1))
    assert {r.family for r in recs} == {fam} and {r.casc for r in recs} == {int(c.V > 16)}, recs
    if c.place == "inst":
        r = recs[0]
        assert VC.inst_of(r) == c.cls[:5] and (r.last_cols == r.cols) == (c.cls[5] == "full"), recs
    elif c.place == "cfg":
        assert VC.cfg_class(c) == c.cls
    elif c.place == "stage" and c.cls[0] != "only":
        assert VC.stage_class(c) == c.cls
    elif c.place == "stage":
        assert len(recs) == 1 and recs[0].pair == (c.kind == "planar_f16") and \
            recs[0].jpl == (8 if c.kind == "cl_f16" else 4), recs
    elif c.place == "frames" and c.cls[0] == "groups":
        assert tuple(dict.fromkeys(r.nf for r in recs)) == c.cls[1:-1], recs
    elif c.place == "frames":
        assert tuple(r.nb for r in recs) == c.cls[2], recs
    elif c.place == "slices":
        assert [r.j0 for r in recs] == [0, 32] and recs[0].lpv > recs[1].lpv, recs
    elif c.place == "cams":
        assert len(recs) == 1 and recs[0].nb == 1 and recs[0].lpv == (2 if c.kind == "cl_f16" else 4), recs


GUARD = 64  # floats before and after each output; 4 * GUARD bytes before and after the workspace


def _guarded_call(c, dev, gpu_device, layer, w, off):
    """The C entry point of the case's kind on caller-owned buffers: cube and xy pre-filled with NaN inside
    larger buffers, a workspace of exactly fvp_voxelize*_workspace_bytes between guard bytes; the cube starts
    `off` floats past a 256-B aligned address.  Returns (cube, xy) as numpy after checking the guards."""
    from fvp import _lib, geometry, ops
    from fvp.ops import _f3, _i3, _ptr

    X, Y, Z = c.bins
    N, XY = X * Y * Z, X * Y
    H, W = c.hm[1], c.hm[0]
    half = c.kind.endswith("f16")
    lib = _lib.load()
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    seqs = ("a", "b") if c.gi else ("a",)
    gi = torch.tensor([b % 2 for b in range(c.B)], dtype=torch.int32, device=gpu_device) if c.gi else None
    cams = VC.cameras(c.V, c.gi)
    if c.otf:
        coords = torch.from_numpy(np.stack([geometry.pack_cameras(cams, s) for s in seqs])).to(gpu_device)
        rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float32
                             ).contiguous().to(gpu_device)
        start, end, center, nb = layer.grid_spec()
        geo = (_ptr(rt), _lib.GridSpec(_f3(start), _f3(end), _f3(center), _i3(nb)),
               _lib.ImageSpec(float(max(w.ori_image_size)), float(w.image_size[0]), float(w.image_size[1]), W, H))
    else:
        coords = torch.stack([ops.pack_grid(torch.from_numpy(np.array(VC.sample_grid(c.V, s, c.bins, c.hm))
                                                             ).to(gpu_device)) for s in seqs])
        geo = (X, Y, Z)
    cl = c.kind.startswith("cl")
    ws_bytes = 0 if cl else (lib.fvp_voxelize_f16_workspace_bytes if half else lib.fvp_voxelize_workspace_bytes)(
        c.B, c.V, c.J, H, W)
    assert cl or ws_bytes > 0
    cbuf = torch.full((2 * GUARD + 4 + c.B * c.J * N,), float("nan"), device=gpu_device)
    xbuf = torch.full((2 * GUARD + c.B * c.J * XY,), float("nan"), device=gpu_device)
    cube = cbuf[GUARD + off:GUARD + off + c.B * c.J * N]
    xy = xbuf[GUARD:GUARD + c.B * c.J * XY]
    assert cube.data_ptr() % 16 == 4 * off
    wbuf = torch.full((ws_bytes + 8 * GUARD,), 0xA5, dtype=torch.uint8, device=gpu_device)
    ws = wbuf[4 * GUARD:4 * GUARD + ws_bytes]
    pc = _ptr(cube) if c.want != "xy" else None
    px = _ptr(xy) if c.want != "cube" else None
    if cl:
        name = ("fvp_voxelize_cl_cams" if c.otf else "fvp_voxelize_cl") + ("_f16" if half else "")
        _lib.call(name, _ptr(dev.t), dev.t.shape[4], c.B, c.V, c.J, H, W, _ptr(coords), _ptr(gi), *geo, pc, px, stream)
    elif c.otf:
        _lib.call("fvp_voxelize_cams", _ptr(dev), int(half), c.B, c.V, c.J, H, W, _ptr(coords), _ptr(gi), *geo, pc, px,
                  _ptr(ws), ws_bytes, stream)
    else:
        _lib.call("fvp_voxelize_f16" if half else "fvp_voxelize", _ptr(dev), c.B, c.V, c.J, H, W, _ptr(coords),
                  _ptr(gi), *geo, pc, px, _ptr(ws), ws_bytes, stream)
    cg, xg, wg = cbuf.cpu().numpy(), xbuf.cpu().numpy(), wbuf.cpu().numpy()
    lo = GUARD + off
    assert np.isnan(cg[:lo]).all() and np.isnan(cg[lo + c.B * c.J * N:]).all(), "cube guard touched"
    assert np.isnan(xg[:GUARD]).all() and np.isnan(xg[GUARD + c.B * c.J * XY:]).all(), "xy guard touched"
    assert (wg[:4 * GUARD] == 0xA5).all() and (wg[4 * GUARD + ws_bytes:] == 0xA5).all(), "workspace guard touched"
    got_c = cg[lo:lo + c.B * c.J * N].reshape(c.B, c.J, X, Y, Z)
    got_x = xg[GUARD:GUARD + c.B * c.J * XY].reshape(c.B, c.J, X, Y)
    assert pc or np.isnan(got_c).all(), "cube written without being asked for"
    assert px or np.isnan(got_x).all(), "xy written without being asked for"
    return got_c, got_x


@pytest.mark.parametrize("case", VC.build(), ids=VC.case_id)
def test_case_vs_oracle(gpu_device, case):
    """Per case: the plan is the case's class; the product's op (ProjectLayer.forward_fused) and the C entry point
    on NaN-filled, guarded buffers with an exact-size workspace both give the oracle's cube and xy bit for bit,
    frame by frame, with no NaN left and no guard touched; where the aligned call takes the vector epilogue, a
    cube 4 B off alignment (cube16 false) gives the same values."""
    from fvp import geometry
    from fvp.project_whole import ProjectLayer

    c = case
    X, Y, Z = c.bins
    recs = VC.plan_of(c)
    _assert_plan(c, recs)
    w = VC.workload(c.bins, c.J, c.hm)
    layer = ProjectLayer(w.cfg(str(gpu_device)))
    layer.verbose = False
    layer.on_the_fly = c.otf
    cams = VC.cameras(c.V, c.gi)
    seqs = [("b" if c.gi and b % 2 else "a") for b in range(c.B)]
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float)
    g = torch.Generator().manual_seed(1000 * c.V + 10 * c.J + c.B)
    hm = torch.rand((c.B, c.V, c.J, c.hm[1], c.hm[0]), generator=g)   # every frame differs: a wrong f0 shows
    half = c.kind.endswith("f16")
    if half:
        hm = hm.half()
    dev = hm.to(gpu_device)
    if c.kind.startswith("cl"):
        dev = _channels_last(dev.float() if half else dev, c.J, half)
    cube, xy = layer.forward_fused(dev, {"seq": seqs}, cams, rt.to(gpu_device), want_cube=c.want != "xy",
                                   want_xy=c.want != "cube")
    outs = [("op", cube.cpu().numpy(), xy.cpu().numpy())]
    outs.append(("entry point",) + _guarded_call(c, dev, gpu_device, layer, w, 0))
    if any(r.vec_full or r.vec_last for r in recs):
        off = VC.plan_of(c, aligned=False)
        assert not any(r.vec_full or r.vec_last for r in off if (r.j0 * X * Y * Z) % 4 == 0), off
        outs.append(("entry point, cube 4 B off alignment",) + _guarded_call(c, dev, gpu_device, layer, w, 1))
    fill, distinct = 1.0, 1.0
    for b in range(c.B):
        sg = VC.sample_grid(c.V, seqs[b], c.bins, c.hm)
        ref = O.voxelize(hm[b].float().numpy(), sg).reshape(c.J, *c.bins)
        ref_xy = O.xy_plane(ref)
        fill = min(fill, np.count_nonzero(ref) / ref.size)
        distinct = min(distinct, min(len(np.unique(ref[j])) for j in range(c.J)) / (X * Y * Z))
        for what, got_c, got_x in outs:
            if c.want != "xy":
                _assert_same(got_c[b], ref, f"{what}: cube frame {b}")
            if c.want != "cube":
                _assert_same(got_x[b], ref_xy, f"{what}: xy frame {b}")
    print(f"fill {fill:.3f} distinct {distinct:.3f}")
    # no pass of the kernel may work on zeros only, and a voxel moved to another place must show
    # (tests/test_voxelize_cases.py asserts the same on the CPU for every camera set and grid of the table)
    assert fill >= FILL and distinct >= FILL, (fill, distinct)
