"""GPU: every case of the per-person gather's case table (person_cases.py: each kernel
instantiation, the x splits, the z chunks, the joint slices, the camera counts, the frames
and the window borders) through the product path (ProjectLayer.forward / forward_planes /
forward_batch, and the op itself where cubes and planes are asked for together) and through
the C entry point of the case's kind on caller-owned, guarded, NaN-filled buffers, bit for
bit against oracle.fvp_oracle.Individual.person_cubes / max_planes.  Before the calls the
plan reported for the arguments must be the class the case stands for.  A second test runs
fvp_max_planes on small, odd and 64-straddling cubes of signed and non-finite values."""
import numpy as np
import pytest
import torch

import person_cases as PC
from oracle import fvp_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4   # the north-star bound, asserted before the bit-exact bar so a failure shows which one broke
FILL = 0.90  # least share of nonzero in-window voxels and of distinct values per joint (tests/test_person_cases.py)
GUARD = 64   # floats before and after each output; 4 * GUARD bytes before and after the workspace
NAN = float("nan")


def _assert_same(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    assert not np.isnan(got).any(), f"{what}: NaN left in the output"
    diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    assert diff.max(initial=0) <= TOL, f"{what}: max |diff| {diff.max()} > {TOL}"
    assert np.array_equal(got, ref), f"{what}: not bit-exact ({np.count_nonzero(diff)} of {diff.size} differ, " \
                                     f"max {diff.max()})"


def _check(c, what, cubes, planes, offset):
    """cubes / planes / offset (numpy, or None where not asked for) against the case's reference, proposal by
    proposal, with the proposal's class in the message."""
    ref_c, ref_o = PC.reference(c)
    cls = PC.classes(c)
    P = c.P
    if offset is not None:
        _assert_same(offset, ref_o, f"{what}: offset")
    ref_p = O.max_planes(ref_c) if planes is not None else None
    for p in range(P):
        if cubes is not None:
            _assert_same(cubes[p], ref_c[p], f"{what}: cube of proposal {p} ({cls[p]})")
        if planes is not None:
            for k, name in enumerate(("xy", "xz", "yz")):
                _assert_same(planes[k * P + p], ref_p[k * P + p], f"{what}: {name} plane of proposal {p} ({cls[p]})")


def _device_heatmaps(c, gpu_device):
    """The case's heatmaps on the device in the layout of its kind: planar [B,V,J,H,W] fp32, or channels-last
    (fvp.heatmaps.ChannelsLastHeatmaps) fp32 / fp16 with cp = person_cases.cp_of channels; unused channels hold
    NaN in the fp32 'padded' case and zeros otherwise."""
    from fvp import heatmaps

    hm = PC.heatmaps(c).to(gpu_device)
    if not c.kind.startswith("cl"):
        return hm
    B, V, J, H, W = hm.shape
    t = torch.full((B, V, H, W, PC.cp_of(c)), NAN if "padded" in c.cls else 0.0, dtype=hm.dtype, device=gpu_device)
    t[..., :J] = hm.permute(0, 1, 3, 4, 2)
    return heatmaps.ChannelsLastHeatmaps(t, J)


def _geometry(c, gpu_device):
    """(constants, the op's six list arguments, packed fine grid of the ORACLE's sample grid, camera records,
    resize transform, grid start / end / centre) of the case."""
    from fvp import geometry, ops

    ind = PC.ind_size(c)
    w = PC.workload(c.bins, c.J, ind)
    k = geometry.individual_constants(w.space_size, w.space_center, ind, c.bins)
    args = ([int(v) for v in k["fine"]], [float(v) for v in k["scale"]], [float(v) for v in k["bias"]],
            [float(v) for v in k["whole_size"]], [float(v) for v in k["ind_size"]], [int(v) for v in k["ind_bins"]])
    cams = PC.VC.cameras(c.V, False)
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float32
                         ).contiguous().to(gpu_device)
    grid = None
    if not c.otf:
        sg = np.array(PC.fine_sample_grid(c.V, c.bins, ind)).reshape(c.V, -1, 2)
        grid = ops.pack_grid(torch.from_numpy(sg).to(gpu_device))
    rec = torch.from_numpy(geometry.pack_cameras(cams, "a")).to(gpu_device)
    start = [float(np.float32(-float(v) / 2)) for v in k["whole_size"]]
    end = [float(np.float32(float(v) / 2)) for v in k["whole_size"]]
    return w, args, grid, cams, rec, rt, (start, end, [float(v) for v in k["whole_center"]])


def _op(c, dev, geo, props, fo, want_cubes, want_planes):
    """torch.ops.fvp.person_planes* of the case's kind."""
    w, args, grid, cams, rec, rt, (start, end, center) = geo
    if c.kind == "cams":
        return torch.ops.fvp.person_planes_cams(dev, rec, rt, start, end, center, float(max(w.ori_image_size)),
                                                float(w.image_size[0]), float(w.image_size[1]), props, fo, *args,
                                                want_cubes, want_planes)
    if c.kind == "planar":
        return torch.ops.fvp.person_planes(dev, grid, props, fo, *args, want_cubes, want_planes)
    return torch.ops.fvp.person_planes_cl(dev.t, c.J, grid, props, fo, *args, want_cubes, want_planes)


def _entry_point(c, dev, geo, props, fo, gpu_device):
    """The C entry point of the case's kind on caller-owned buffers: cubes, planes and offset pre-filled with
    NaN inside larger buffers with GUARD floats on both sides; the planar kinds get a workspace of exactly
    fvp_person_workspace_bytes between 0xA5 guard bytes.  Returns (status, cubes, planes, offset) as numpy
    (an output not asked for: None, after checking that it is still all NaN) after checking the guards."""
    from fvp import _lib
    from fvp.ops import _f3, _i3, _ptr

    w, args, grid, cams, rec, rt, (start, end, center) = geo
    lib = _lib.load()
    P, J, H, W = c.P, c.J, c.hm[1], c.hm[0]
    SX, SY, SZ = c.bins
    n_c, n_p = P * J * SX * SY * SZ, 3 * P * J * SX * SY
    want_c, want_p = c.want != "planes", c.want != "cubes"
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    bufs = [torch.full((2 * GUARD + n,), NAN, device=gpu_device) for n in (n_c, n_p, 3 * P)]
    cubes, planes, offset = (b[GUARD:b.numel() - GUARD] for b in bufs)
    planar = c.kind in ("planar", "cams")
    ws_bytes = lib.fvp_person_workspace_bytes(c.B, c.V, J, H, W) if planar else 0
    assert not planar or ws_bytes > 0 or PC.error_of(c)
    wbuf = torch.full((ws_bytes + 8 * GUARD,), 0xA5, dtype=torch.uint8, device=gpu_device)
    ws = wbuf[4 * GUARD:4 * GUARD + ws_bytes]
    spec = _lib.PersonSpec(_i3(args[0]), _f3(args[1]), _f3(args[2]), _f3(args[3]), _f3(args[4]), _i3(args[5]))
    out = (_ptr(cubes) if want_c else None, _ptr(planes) if want_p else None, _ptr(offset))
    if c.kind == "planar":
        st = lib.fvp_person_planes(_ptr(dev), c.B, c.V, J, H, W, _ptr(grid), spec, _ptr(props), _ptr(fo), P, *out,
                                   _ptr(ws), ws_bytes, stream)
    elif c.kind == "cams":
        g = _lib.GridSpec(_f3(start), _f3(end), _f3(center), _i3(args[0]))
        im = _lib.ImageSpec(float(max(w.ori_image_size)), float(w.image_size[0]), float(w.image_size[1]), W, H)
        st = lib.fvp_person_planes_cams(_ptr(dev), c.B, c.V, J, H, W, _ptr(rec), _ptr(rt), g, im, spec, _ptr(props),
                                        _ptr(fo), P, *out, _ptr(ws), ws_bytes, stream)
    else:
        fn = lib.fvp_person_planes_cl_f16 if c.kind == "cl_f16" else lib.fvp_person_planes_cl
        st = fn(_ptr(dev.t), dev.t.shape[4], c.B, c.V, J, H, W, _ptr(grid), spec, _ptr(props), _ptr(fo), P, *out, stream)
    torch.cuda.synchronize(gpu_device)
    host = [b.cpu().numpy() for b in bufs]
    for name, h in zip(("cubes", "planes", "offset"), host):
        assert np.isnan(h[:GUARD]).all() and np.isnan(h[-GUARD:]).all(), f"{name} guard touched"
    wg = wbuf.cpu().numpy()
    assert (wg[:4 * GUARD] == 0xA5).all() and (wg[4 * GUARD + ws_bytes:] == 0xA5).all(), "workspace guard touched"
    got_c, got_p, got_o = (h[GUARD:-GUARD] for h in host)
    if st != 0:
        assert np.isnan(got_c).all() and np.isnan(got_p).all() and np.isnan(got_o).all(), "an output written on error"
        return st, None, None, None
    assert want_c or np.isnan(got_c).all(), "cubes written without being asked for"
    assert want_p or np.isnan(got_p).all(), "planes written without being asked for"
    return (st, got_c.reshape(P, J, SX, SY, SZ) if want_c else None,
            got_p.reshape(3 * P, J, SX, SY) if want_p else None, got_o.reshape(P, 3))


def _assert_plan(c, recs):
    """The plan reported for the case's arguments is the class the case stands for."""
    r = recs[0]
    assert r.otf == int(c.otf) and r.casc == int(c.V > 16) and r.jpl == (8 if PC.is_half(c) else 4), recs
    assert r.layout == int(c.kind in ("planar", "cams")), recs
    assert r.zeroed_planes == (0 if c.want == "cubes" else 3 if r.xsplit > 1 else 2), recs
    if c.place in ("inst", "split", "depth", "cams", "window") and len(c.cls) == 7:
        assert PC.inst_of(r) + (r.xsplit, r.zsplit, r.xy_direct) == c.cls and len(recs) == 1, recs
    if c.place == "slices":
        assert [q.j0 for q in recs] == list(range(0, c.J, 32)), recs
        assert c.J == 64 or recs[0].lpv != recs[-1].lpv, recs


@pytest.mark.parametrize("case", PC.build(), ids=PC.case_id)
def test_case_vs_oracle(gpu_device, case):
    """Per case: the plan is the case's class; the product path and the C entry point on NaN-filled, guarded
    buffers with an exact-size workspace both give the oracle's cubes, planes and offsets bit for bit, proposal
    by proposal, with no NaN left in a requested output, an output not asked for untouched and no guard
    touched.  The fp16 cases are compared with the oracle on the fp16-rounded heatmaps.  An error case returns
    its status from the plan and from the entry point, and writes nothing."""
    from fvp.project_individual import ProjectLayer

    c = case
    st, recs = PC.plan_of(c)
    assert st == PC.error_of(c), (st, recs)
    geo = _geometry(c, gpu_device)
    dev = _device_heatmaps(c, gpu_device)
    props = torch.from_numpy(PC.proposals(c)).to(gpu_device)
    fo_np = PC.frame_of(c)
    fo = None if fo_np is None else torch.from_numpy(fo_np).to(gpu_device)
    if st:
        assert _entry_point(c, dev, geo, props, fo, gpu_device)[0] == st
        return
    _assert_plan(c, recs)
    want_c, want_p = c.want != "planes", c.want != "cubes"
    npy = lambda t: t.cpu().numpy()

    # the product path
    cubic = c.bins[0] == c.bins[1] == c.bins[2]
    if cubic:
        w, cams = geo[0], geo[3]
        layer = ProjectLayer(w.cfg(str(gpu_device)))
        layer.verbose = False
        layer.on_the_fly = c.otf
        rt = geo[5]
        if fo is None:
            meta = {"seq": ["a"]}
            if want_c:
                cubes, offset = layer(dev, 0, meta, props, cams, rt)
                _check(c, "ProjectLayer.forward", npy(cubes), None, npy(offset))
            if want_p:
                planes, offset = layer.forward_planes(dev, 0, meta, props, cams, rt)
                _check(c, "ProjectLayer.forward_planes", None, npy(planes), npy(offset))
        else:
            idx = torch.stack([fo.long(), torch.arange(c.P, device=gpu_device)], dim=1)
            planes, offset, _ = layer.forward_batch(dev, {"seq": ["a"] * c.B}, None, None, cams, rt, sel=(idx, fo, props))
            _check(c, "ProjectLayer.forward_batch", None, npy(planes), npy(offset))
    if c.want == "both" or not cubic:
        cubes, planes, offset = _op(c, dev, geo, props, fo, want_c, want_p)
        _check(c, "torch.ops.fvp.person_planes*", npy(cubes) if want_c else None, npy(planes) if want_p else None,
               npy(offset))

    # the C entry point on guarded buffers
    st, cubes, planes, offset = _entry_point(c, dev, geo, props, fo, gpu_device)
    assert st == 0, st
    _check(c, "entry point", cubes, planes, offset)

    fill, distinct, at_one = PC.fill_of(c)
    print(f"fill {fill:.3f} distinct {distinct:.3f}")
    assert fill >= FILL and distinct >= FILL and not at_one, (fill, distinct, at_one)


@pytest.mark.parametrize("P,J", [(1, 1), (3, 5)])
@pytest.mark.parametrize("S", [1, 2, 3, 7, 33, 63, 64, 65, 66])
def test_max_planes_edges(gpu_device, S, P, J):
    """fvp_max_planes (the block kernel up to 64, one thread per cell beyond) on cubes of signed normal values
    with -inf, +inf, -0.0, +0.0 and NaN planted at known cells: torch.max semantics (NaN wins), written as
    person_cases.nan_max_planes and held to torch.max on the CPU by tests/test_person_cases.py.  Bit for bit,
    including the sign of a zero maximum wherever it is defined (person_cases.zero_sign_defined: all zeros of
    the reduced line share one sign).  Only a line whose maximum is held by both +0 and -0 is compared with ==:
    there torch.max's own choice depends on the order it visits them."""
    rng = np.random.default_rng(100 * S + J)
    cubes = rng.standard_normal((P, J, S, S, S)).astype(np.float32)
    flat = cubes.reshape(-1)
    special = np.array([-np.inf, np.inf, -0.0, 0.0, np.nan], np.float32)
    idx = rng.choice(flat.size, min(flat.size, 10 * P * J), replace=False)
    flat[idx] = np.resize(special, len(idx))
    if S >= 3:   # whole lines of one value: all -inf along z, all -0.0 along y, NaN at both ends of an x line;
        #          then zero maxima above negatives: -0.0 alone, +0.0 alone, and both signs in one y line
        cubes[0, 0, 0, 0, :] = -np.inf
        cubes[0, 0, 1, :, :] = -1 - rng.random((S, S)).astype(np.float32)
        cubes[0, 0, 1, :, 1] = -0.0
        cubes[0, 0, 1, 1, 0] = -0.0
        cubes[0, 0, 1, S - 1, 2] = 0.0
        if S > 3:
            cubes[0, 0, 1, 0, 3], cubes[0, 0, 1, S - 1, 3] = 0.0, -0.0
        cubes[-1, -1, 0, 2, 2] = cubes[-1, -1, S - 1, 2, 2] = np.nan
    ref = PC.nan_max_planes(cubes)
    got = torch.ops.fvp.max_planes(torch.from_numpy(cubes).to(gpu_device)).cpu().numpy()
    assert got.shape == ref.shape == (3 * P, J, S, S)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN cells differ"
    ok = ~np.isnan(ref)
    assert np.array_equal(got[ok], ref[ok])
    exact = ok & ((ref != 0) | PC.zero_sign_defined_planes(cubes))
    assert np.array_equal(got[exact].view(np.uint32), ref[exact].view(np.uint32)), \
        f"{np.count_nonzero(got[exact].view(np.uint32) != ref[exact].view(np.uint32))} cells differ in bits"
    if S >= 3:   # the xz plane (max over y) of (0, 0): x = 1, z = 1 is the all -0.0 line, z = 0 -0.0 above negatives
        xz = got[P:2 * P][0, 0].view(np.uint32)
        assert xz[1, 1] == xz[1, 0] == 0x80000000 and xz[1, 2] == 0 and exact[P:2 * P][0, 0][1, :3].all()
        assert S == 3 or (not exact[P:2 * P][0, 0][1, 3] and got[P:2 * P][0, 0][1, 3] == 0)
    assert np.isnan(ref).any() or S == 1
