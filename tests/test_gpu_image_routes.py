"""GPU: every case of the heatmap-size and image-border table (image_cases.py) bit for bit
against oracle.fvp_oracle.voxelize / xy_plane / gather_columns, frame by frame.

* the projected cases (portrait image: x leaves the image by projection) through the
  product's op (ProjectLayer.forward_fused / columns) and through the C entry point;
* the planted cases (image_ref.planted_grid: all 25 tap classes, corners included) through
  the C entry point of their kind on caller-owned, guarded buffers (the call of
  test_gpu_voxelize_routes.py) with the packed grid of the planted grid and a workspace
  pre-filled with a NaN pattern of the table's element type, so a border entry the layout
  pass fails to write poisons the cube;
* where the call is one layout launch (or one per joint slice of one frame), the workspace
  read back: its first tab_bytes equal the numpy table of image_ref bit for bit, everything
  after is still the fill pattern;
* fvp_voxel_columns on guarded, NaN-filled output against the oracle cube's columns.
"""
import numpy as np
import pytest
import torch

import image_cases as IC
import image_ref as R
from oracle import fvp_oracle as O
from test_gpu_voxelize_routes import GUARD, _assert_same, _channels_last

pytestmark = pytest.mark.gpu

FILL, DISTINCT = 0.60, 0.50   # tests/test_image_cases.py
SLACK = 1024                  # bytes of workspace beyond what the call needs: a layout that overshoots its table shows
NAN16, NAN32 = 0x7E007E00, 0x7FC00000   # two fp16 NaNs / one fp32 NaN per 4 bytes


def _device_heatmaps(c, gpu_device):
    """The case's heatmaps on the device in the layout of its kind.  Planar fp16: carved out of a larger
    buffer so that the data starts c.amod bytes past a 16-B boundary."""
    hm = IC.heatmaps(c)
    half = c.kind.endswith("f16")
    if c.kind.startswith("cl"):
        return _channels_last(hm.float().to(gpu_device) if half else hm.to(gpu_device), c.J, half)
    if not half:
        return hm.to(gpu_device)
    buf = torch.empty(hm.numel() + 16, dtype=torch.float16, device=gpu_device)
    assert buf.data_ptr() % 16 == 0
    dev = buf[c.amod // 2:c.amod // 2 + hm.numel()].view(hm.shape)
    dev.copy_(hm)
    assert dev.is_contiguous() and dev.data_ptr() % 16 == c.amod
    return dev


def _coords(c, gpu_device, w, layer):
    """(coords tensor, grid_index tensor or None, the geometry arguments of the entry point)."""
    from fvp import _lib, geometry, ops
    from fvp.ops import _f3, _i3, _ptr

    X, Y, Z = c.bins
    H, W = c.hm[1], c.hm[0]
    seqs = ("a", "b") if c.gi else ("a",)
    gi = torch.tensor([b % 2 for b in range(c.B)], dtype=torch.int32, device=gpu_device) if c.gi else None
    if c.otf:
        cams = IC.VC.cameras(c.V, c.gi)
        coords = torch.from_numpy(np.stack([geometry.pack_cameras(cams, s) for s in seqs])).to(gpu_device)
        rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float32
                             ).contiguous().to(gpu_device)
        start, end, center, nb = layer.grid_spec()
        geo = (_ptr(rt), _lib.GridSpec(_f3(start), _f3(end), _f3(center), _i3(nb)),
               _lib.ImageSpec(float(max(w.ori_image_size)), float(w.image_size[0]), float(w.image_size[1]), W, H))
        return coords, gi, geo, rt
    coords = torch.stack([ops.pack_grid(torch.from_numpy(np.array(IC.sample_grid(c, s))).to(gpu_device)) for s in seqs])
    return coords, gi, (X, Y, Z), None


def _guarded_call(c, dev, gpu_device, w, layer):
    """The C entry point of the case's kind on caller-owned buffers (test_gpu_voxelize_routes._guarded_call):
    cube and xy pre-filled with NaN inside larger buffers; the workspace, SLACK bytes larger than
    fvp_voxelize*_workspace_bytes, and its guards pre-filled with NaNs of the table's element type.  Returns
    (cube, xy, workspace bytes as uint8 numpy) after checking the guards."""
    from fvp import _lib
    from fvp.ops import _ptr

    X, Y, Z = c.bins
    N, XY = X * Y * Z, X * Y
    H, W = c.hm[1], c.hm[0]
    half = c.kind.endswith("f16")
    lib = _lib.load()
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    coords, gi, geo, _ = _coords(c, gpu_device, w, layer)
    cl = c.kind.startswith("cl")
    need = 0 if cl else (lib.fvp_voxelize_f16_workspace_bytes if half else lib.fvp_voxelize_workspace_bytes)(
        c.B, c.V, c.J, H, W)
    assert cl or (need > 0 and need % 4 == 0)
    ws_bytes = 0 if cl else need + SLACK
    cbuf = torch.full((2 * GUARD + 4 + c.B * c.J * N,), float("nan"), device=gpu_device)
    xbuf = torch.full((2 * GUARD + c.B * c.J * XY,), float("nan"), device=gpu_device)
    cube = cbuf[GUARD:GUARD + c.B * c.J * N]
    xy = xbuf[GUARD:GUARD + c.B * c.J * XY]
    assert cube.data_ptr() % 16 == 0
    pattern = NAN16 if (half and c.J <= 16) else NAN32
    wbuf = torch.full(((ws_bytes + 8 * GUARD) // 4,), pattern, dtype=torch.int32, device=gpu_device).view(torch.uint8)
    ws = wbuf[4 * GUARD:4 * GUARD + ws_bytes]
    pc, px = _ptr(cube), _ptr(xy)
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
    fill = np.full(1, pattern, np.uint32).view(np.uint8)
    assert np.isnan(cg[:GUARD]).all() and np.isnan(cg[GUARD + c.B * c.J * N:]).all(), "cube guard touched"
    assert np.isnan(xg[:GUARD]).all() and np.isnan(xg[GUARD + c.B * c.J * XY:]).all(), "xy guard touched"
    assert (wg[:4 * GUARD].reshape(-1, 4) == fill).all() and (wg[4 * GUARD + ws_bytes:].reshape(-1, 4) == fill).all(), \
        "workspace guard touched"
    got_c = cg[GUARD:GUARD + c.B * c.J * N].reshape(c.B, c.J, X, Y, Z)
    got_x = xg[GUARD:GUARD + c.B * c.J * XY].reshape(c.B, c.J, X, Y)
    return got_c, got_x, wg[4 * GUARD:4 * GUARD + ws_bytes]


def _expected_tables(c, recs):
    """[(bytes, what)] in launch order: the table each launch's layout pass writes at the start of the workspace,
    for a call that is one layout launch per joint slice (one chunk of B == NF frames); None otherwise."""
    if c.kind.startswith("cl") or any(r.nb != c.B or r.nf != c.B or r.f0 != 0 for r in recs):
        return None
    hm = IC.heatmaps(c)
    out = []
    for r in recs:
        if r.pair:
            tab = R.pair_table(hm.numpy().view(np.uint16), r.nf)
        else:
            tab = R.cl_table(hm.float().numpy(), r.j0, r.joints, r.lpv)
        assert tab.nbytes == r.tab_bytes, (tab.nbytes, r)
        out.append((np.frombuffer(tab.tobytes(), np.uint8), f"table of joints {r.j0}.."))
    return out


def _check_workspace(c, recs, ws):
    """The workspace after the call: the last slice's table over the first's, then the fill pattern."""
    tabs = _expected_tables(c, recs)
    assert tabs is not None or c.kind.startswith("cl") or c.place in ("border", "border_otf"), recs
    if tabs is None:
        return False
    pattern = NAN16 if recs[0].pair else NAN32
    want = np.tile(np.full(1, pattern, np.uint32).view(np.uint8), len(ws) // 4)
    for t, _ in tabs:
        want[:len(t)] = t
    end = max(len(t) for t, _ in tabs)
    if not np.array_equal(ws[:end], want[:end]):
        bad = np.nonzero(ws[:end] != want[:end])[0]
        unit = 64 if recs[0].pair else 16 * recs[0].lpv
        raise AssertionError(f"layout table differs from image_ref in {len(bad)} of {end} bytes, first at byte "
                             f"{bad[0]} (entry {bad[0] // unit}, byte {bad[0] % unit}), last at {bad[-1]}")
    assert np.array_equal(ws[end:], want[end:]), "the layout pass wrote past its table"
    return True


def _assert_kind(c, recs):
    assert all(r.status == 0 for r in recs), recs
    assert {r.otf for r in recs} == {int(c.otf)} and {r.casc for r in recs} == {int(c.V > 16)}, recs
    if c.place in ("pairs", "joints"):
        assert IC.layout_of(c) == R.LAYOUT_NAMES.index(c.cls[0]) == R.pair_layout_model(c.B, c.hm[0], c.amod)
        assert len(recs) == 1 and (recs[0].pair, recs[0].nf, recs[0].nb) == (1, c.B, c.B), recs


VOX = [c for c in IC.build() if c.place != "columns"]
COL = [c for c in IC.build() if c.place == "columns"]


@pytest.mark.parametrize("case", VOX, ids=IC.case_id)
def test_case_vs_oracle(gpu_device, case):
    """Per case: the plan (and for the pair table the layout kernel) is the one the case stands for; the C entry
    point on NaN-filled, guarded buffers -- and for the projected cases the product's op -- gives the oracle's
    cube and xy bit for bit, frame by frame, with no NaN left and no guard touched; a call that is one layout
    launch leaves exactly image_ref's table in the workspace and the fill pattern behind it."""
    from fvp import geometry
    from fvp.project_whole import ProjectLayer

    c = case
    recs = IC.plan_of(c)
    _assert_kind(c, recs)
    w = IC.workload(c)
    layer = ProjectLayer(w.cfg(str(gpu_device)))
    layer.verbose = False
    layer.on_the_fly = c.otf
    dev = _device_heatmaps(c, gpu_device)
    outs = []
    if c.src == "portrait":
        cams = IC.VC.cameras(c.V, c.gi)
        rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float)
        cube, xy = layer.forward_fused(dev, {"seq": IC.seqs_of(c)}, cams, rt.to(gpu_device))
        outs.append(("op", cube.cpu().numpy(), xy.cpu().numpy()))
    got_c, got_x, ws = _guarded_call(c, dev, gpu_device, w, layer)
    outs.append(("entry point", got_c, got_x))
    # the table first: it localises a failure to the layout pass or the gather
    checked = _check_workspace(c, recs, ws)
    assert checked or c.place not in ("pairs", "joints", "layout")
    ref = IC.oracle_cube(c)
    fill, distinct = 1.0, 1.0
    for b in range(c.B):
        ref_xy = O.xy_plane(ref[b])
        fill = min(fill, np.count_nonzero(ref[b]) / ref[b].size)
        distinct = min(distinct, min(len(np.unique(ref[b, j])) for j in range(c.J)) / ref[b, 0].size)
        for what, cube, xy in outs:
            _assert_same(cube[b], ref[b], f"{what}: cube frame {b}")
            _assert_same(xy[b], ref_xy, f"{what}: xy frame {b}")
    print(f"fill {fill:.3f} distinct {distinct:.3f} table {'checked' if checked else 'not read'}")
    assert fill >= FILL and distinct >= DISTINCT, (fill, distinct)


@pytest.mark.parametrize("case", COL, ids=IC.case_id)
def test_columns_vs_oracle(gpu_device, case):
    """fvp_voxel_columns (all 8 instantiations, planar and channels-last strides) with flat = every index of the
    map once, then -1 and X * Y, on guarded, NaN-filled output: the oracle cube's columns
    (oracle.fvp_oracle.gather_columns) bit for bit, NaN for the two indices outside the map; the projected
    cases also through ProjectLayer.columns."""
    from fvp import _lib, geometry, heatmaps
    from fvp.ops import _ptr
    from fvp.project_whole import ProjectLayer

    c = case
    X, Y, Z = c.bins
    H, W = c.hm[1], c.hm[0]
    half = c.kind.endswith("f16")
    w = IC.workload(c)
    layer = ProjectLayer(w.cfg(str(gpu_device)))
    layer.verbose = False
    layer.on_the_fly = c.otf
    planar = IC.heatmaps(c).to(gpu_device)
    if c.strides == "cl":
        src = heatmaps.to_channels_last(planar, dtype=torch.float16 if half else None)
        cp = src.t.shape[4]
        hm_t, strides = src.t, (H * W * cp, 1, cp)
    else:
        src, hm_t, strides = planar, planar, (c.J * H * W, H * W, 1)
    assert hm_t.dtype == (torch.float16 if half else torch.float32) and hm_t.is_contiguous()
    flat_np = IC.flat_of(c)
    K = flat_np.shape[1]
    flat = torch.from_numpy(flat_np).to(gpu_device)
    coords, gi, geo, rt = _coords(c, gpu_device, w, layer)
    n = c.B * K * c.J * Z
    obuf = torch.full((2 * GUARD + n,), float("nan"), device=gpu_device)
    out = obuf[GUARD:GUARD + n]
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    if c.otf:
        args = (None, _ptr(coords), geo[0], geo[1], geo[2])
    else:
        args = (_ptr(coords), None, None, None, None)
    _lib.call("fvp_voxel_columns", _ptr(hm_t), int(half), *strides, c.B, c.V, c.J, H, W, *args, _ptr(gi), X, Y, Z,
              _ptr(flat), K, _ptr(out), stream)
    og = obuf.cpu().numpy()
    assert np.isnan(og[:GUARD]).all() and np.isnan(og[GUARD + n:]).all(), "columns guard touched"
    outs = [("entry point", og[GUARD:GUARD + n].reshape(c.B, K, c.J, Z))]
    if c.src == "portrait":
        cams = IC.VC.cameras(c.V, c.gi)
        got = layer.columns(src, {"seq": IC.seqs_of(c)}, cams, rt, flat)
        outs.append(("ProjectLayer.columns", got.cpu().numpy()))
    ref = O.gather_columns(np.array(IC.oracle_cube(c)), flat_np[:, :K - 2])
    for what, got in outs:
        assert got.shape == (c.B, K, c.J, Z), what
        assert np.isnan(got[:, K - 2:]).all(), f"{what}: an index outside the map must give NaN"
        for b in range(c.B):
            _assert_same(got[b, :K - 2], ref[b], f"{what}: columns of frame {b}")


def _person_geometry(c, gpu_device):
    """The geo tuple of test_gpu_person_routes (_op): constants, the op's list arguments, the packed fine grid of
    the case's own sample grid, camera records, resize transform, the fine grid's start / end / centre."""
    from fvp import geometry, ops

    w, ind = IC.person_workload(c)
    k = geometry.individual_constants(w.space_size, w.space_center, ind, c.bins)
    args = ([int(v) for v in k["fine"]], [float(v) for v in k["scale"]], [float(v) for v in k["bias"]],
            [float(v) for v in k["whole_size"]], [float(v) for v in k["ind_size"]], [int(v) for v in k["ind_bins"]])
    cams = IC.VC.cameras(c.V, False)
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float32
                         ).contiguous().to(gpu_device)
    grid = None if c.otf else ops.pack_grid(torch.from_numpy(np.array(IC.person_fine_grid(c))).to(gpu_device))
    rec = torch.from_numpy(geometry.pack_cameras(cams, "a")).to(gpu_device)
    start = [float(np.float32(-float(v) / 2)) for v in k["whole_size"]]
    end = [float(np.float32(float(v) / 2)) for v in k["whole_size"]]
    return w, args, grid, cams, rec, rt, (start, end, [float(v) for v in k["whole_center"]])


def _person_entry_point(c, dev, geo, props, gpu_device):
    """The C entry point of the case's kind (test_gpu_person_routes._entry_point) with cubes, planes and offset
    pre-filled with NaN between guards and, for the planar kinds, a workspace SLACK bytes larger than
    fvp_person_workspace_bytes pre-filled with fp32 NaNs.  Returns (cubes, planes, offset, workspace bytes)."""
    from fvp import _lib
    from fvp.ops import _f3, _i3, _ptr

    w, args, grid, cams, rec, rt, (start, end, center) = geo
    lib = _lib.load()
    P, J, H, W = c.P, c.J, c.hm[1], c.hm[0]
    S = c.bins[0]
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    bufs = [torch.full((2 * GUARD + n,), float("nan"), device=gpu_device) for n in (P * J * S ** 3, 3 * P * J * S * S, 3 * P)]
    cubes, planes, offset = (b[GUARD:b.numel() - GUARD] for b in bufs)
    planar = c.kind in ("planar", "cams")
    need = lib.fvp_person_workspace_bytes(c.B, c.V, J, H, W) if planar else 0
    ws_bytes = need + SLACK if planar else 0
    wbuf = torch.full(((ws_bytes + 8 * GUARD) // 4,), NAN32, dtype=torch.int32, device=gpu_device).view(torch.uint8)
    ws = wbuf[4 * GUARD:4 * GUARD + ws_bytes]
    spec = _lib.PersonSpec(_i3(args[0]), _f3(args[1]), _f3(args[2]), _f3(args[3]), _f3(args[4]), _i3(args[5]))
    out = (_ptr(cubes), _ptr(planes), _ptr(offset))
    if c.kind == "planar":
        _lib.call("fvp_person_planes", _ptr(dev), c.B, c.V, J, H, W, _ptr(grid), spec, _ptr(props), None, P, *out,
                  _ptr(ws), ws_bytes, stream)
    elif c.kind == "cams":
        g = _lib.GridSpec(_f3(start), _f3(end), _f3(center), _i3(args[0]))
        im = _lib.ImageSpec(float(max(w.ori_image_size)), float(w.image_size[0]), float(w.image_size[1]), W, H)
        _lib.call("fvp_person_planes_cams", _ptr(dev), c.B, c.V, J, H, W, _ptr(rec), _ptr(rt), g, im, spec,
                  _ptr(props), None, P, *out, _ptr(ws), ws_bytes, stream)
    else:
        _lib.call("fvp_person_planes_cl_f16" if c.kind == "cl_f16" else "fvp_person_planes_cl", _ptr(dev.t),
                  dev.t.shape[4], c.B, c.V, J, H, W, _ptr(grid), spec, _ptr(props), None, P, *out, stream)
    torch.cuda.synchronize(gpu_device)
    host = [b.cpu().numpy() for b in bufs]
    for name, h in zip(("cubes", "planes", "offset"), host):
        assert np.isnan(h[:GUARD]).all() and np.isnan(h[-GUARD:]).all(), f"{name} guard touched"
    wg = wbuf.cpu().numpy()
    fill = np.full(1, NAN32, np.uint32).view(np.uint8)
    assert (wg[:4 * GUARD].reshape(-1, 4) == fill).all() and (wg[4 * GUARD + ws_bytes:].reshape(-1, 4) == fill).all(), \
        "workspace guard touched"
    got_c, got_p, got_o = (h[GUARD:-GUARD] for h in host)
    return (got_c.reshape(P, J, S, S, S), got_p.reshape(3 * P, J, S, S), got_o.reshape(P, 3),
            wg[4 * GUARD:4 * GUARD + ws_bytes])


@pytest.mark.parametrize("case", IC.person_cases(), ids=IC.person_id)
def test_person_case_vs_oracle(gpu_device, case):
    """The four per-person entry kinds at heatmaps of 61 x 33 and 10 x 6 (the on-the-fly kind: 33 x 61 and 6 x 10
    on the portrait image): cubes, planes and offsets of the C entry point on NaN-filled, guarded buffers -- and
    of the product's layer and op for the projected kind -- equal person_cases.sliced_reference's construction on
    the case's own fine grid bit for bit; the planar kinds' workspace holds image_ref's fp32 table and the fill
    pattern behind it."""
    import person_cases as PC
    from fvp import heatmaps, ops
    from fvp.project_individual import ProjectLayer
    from test_gpu_person_routes import _op

    c = case
    o = IC.person_individual(c)
    st, recs = ops.person_plan(c.kind, c.B, c.V, c.J, c.hm[1], c.hm[0], c.bins, o.fine_bins, c.P,
                               cp=16 if c.kind.startswith("cl") else 0)
    assert st == 0 and len(recs) == 1 and recs[0].otf == int(c.otf) and recs[0].layout == int(not c.kind.startswith("cl"))
    geo = _person_geometry(c, gpu_device)
    hm = IC.person_heatmaps(c)
    dev = hm.to(gpu_device)
    if c.kind.startswith("cl"):
        dev = heatmaps.to_channels_last(dev.float(), dtype=torch.float16 if c.kind == "cl_f16" else None)
    props = torch.from_numpy(IC.person_proposals(c)).to(gpu_device)
    ref_c, ref_o = IC.person_reference(c)
    ref_p = O.max_planes(np.array(ref_c))
    outs = []
    if c.otf:
        w, cams, rt = geo[0], geo[3], geo[5]
        layer = ProjectLayer(w.cfg(str(gpu_device)))
        layer.verbose = False
        layer.on_the_fly = True
        cubes, offset = layer(dev, 0, {"seq": ["a"]}, props, cams, rt)
        planes, offset2 = layer.forward_planes(dev, 0, {"seq": ["a"]}, props, cams, rt)
        assert torch.equal(offset, offset2)
        outs.append(("ProjectLayer", cubes.cpu().numpy(), planes.cpu().numpy(), offset.cpu().numpy()))
        cubes, planes, offset = _op(c, dev, geo, props, None, True, True)
        outs.append(("torch.ops.fvp.person_planes_cams", cubes.cpu().numpy(), planes.cpu().numpy(), offset.cpu().numpy()))
    got_c, got_p, got_o, ws = _person_entry_point(c, dev, geo, props, gpu_device)
    outs.append(("entry point", got_c, got_p, got_o))
    if recs[0].layout:
        tab = np.frombuffer(R.cl_table(hm.float().numpy(), 0, c.J, recs[0].lpv).tobytes(), np.uint8)
        assert len(tab) == len(ws) - SLACK
        assert np.array_equal(ws[:len(tab)], tab), "layout table differs from image_ref"
        assert (ws[len(tab):].reshape(-1, 4) == np.full(1, NAN32, np.uint32).view(np.uint8)).all(), \
            "the layout pass wrote past its table"
    for what, cubes, planes, offset in outs:
        _assert_same(offset, ref_o, f"{what}: offset")
        for p in range(c.P):
            _assert_same(cubes[p], ref_c[p], f"{what}: cube of proposal {p}")
            for k, name in enumerate(("xy", "xz", "yz")):
                _assert_same(planes[k * c.P + p], ref_p[k * c.P + p], f"{what}: {name} plane of proposal {p}")
    fill = np.count_nonzero(ref_c) / ref_c.size
    distinct = min(len(np.unique(ref_c[p, j])) for p in range(c.P) for j in range(c.J)) / ref_c[0, 0].size
    assert fill >= FILL and distinct >= DISTINCT, (fill, distinct)
