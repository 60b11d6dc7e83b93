"""The JLN post-processing kernels on every code path, against float64 (tests/jln_ref.py) or,
where the operation is a selection, bit for bit against torch on the CPU:

  fvp_soft_argmax       every row-length class of its three kernels, float4 and scalar loads,
                        peaks on every thread / pass / row boundary, constant and non-finite rows
  fvp_fuse_poses        joint counts around its 64-thread stride, NaN weights, NULL outputs
  fvp_proposal_centers  two blocks, Z from 1 to 200, ties, NaN, -inf, the strict threshold
  fvp_weight_net        guarded channels, the hidden-layer loop, the smallest and largest maps
  fvp_scatter_poses, fvp_mask_select, fvp_max_planes   strided operands, seams, every S class

Each test prints what it measured before it asserts (pytest -s shows it).
"""
import copy
import functools

import numpy as np
import pytest
import torch

import jln_ref as R

pytestmark = pytest.mark.gpu
U = R.U


# ---- soft-argmax ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(S2, P, J):
    c = R.make_case(S2, P, J)
    c["ref"] = R.soft_argmax_ref(c["features"], c["center_grid"], c["offset"])
    c["ref_no_offset"] = R.soft_argmax_ref(c["features"], c["center_grid"], None)
    return c


def _run(dev, features, grid, offset):
    from fvp import ops

    pose, maxprob = ops.soft_argmax(torch.from_numpy(features).to(dev), torch.from_numpy(grid).to(dev),
                                    None if offset is None else torch.from_numpy(offset).to(dev), R.BETA)
    return pose.cpu().numpy(), maxprob.cpu().numpy()


def _within(pose, maxprob, ref, what):
    pr, mr = R.ratios(pose, maxprob, ref)
    print(f"{what}: pose error {pr:.4f} x bound (bound <= {np.nanmax(ref['bound']):.4f} mm), "
          f"maxprob error {mr:.4f} x allowance")
    assert pr <= 1.0, f"{what}: pose error {pr:.3f} x bound"
    assert mr <= 1.0, f"{what}: maxprob error {mr:.3f} x allowance"


@pytest.mark.parametrize("S2,P,J", R.CASES, ids=lambda v: str(v))
def test_soft_argmax_vs_float64(gpu_device, S2, P, J):
    """Peaks on every float4 / pass / kernel / row boundary; with the offsets and without."""
    c = _case(S2, P, J)
    pose, maxprob = _run(gpu_device, c["features"], c["center_grid"], c["offset"])
    assert pose.shape == (3, P, J, 2) and maxprob.shape == (3, P, J)
    _within(pose, maxprob, c["ref"], f"S2={S2} P={P} J={J}")
    pose0, maxprob0 = _run(gpu_device, c["features"], c["center_grid"], None)
    _within(pose0, maxprob0, c["ref_no_offset"], f"S2={S2} P={P} J={J} offset=None")
    assert np.array_equal(maxprob0, maxprob)


@pytest.mark.parametrize("S2", R.CONSTANT_S2)
def test_soft_argmax_constant_rows(gpu_device, S2):
    """All cells equal: every cell counts exactly once (maxprob = 1 / S2, pose = the grid mean)."""
    c = R.constant_case(S2)
    ref = R.soft_argmax_ref(c["features"], c["center_grid"], c["offset"])
    pose, maxprob = _run(gpu_device, c["features"], c["center_grid"], c["offset"])
    count = np.abs(maxprob.astype(np.float64) * S2 - 1.0).max()
    print(f"constant S2={S2}: |maxprob * S2 - 1| = {count / U:.3f} u")
    assert count <= 4 * U
    mean = c["center_grid"].astype(np.float64).mean(axis=1)
    np.testing.assert_allclose(ref["coords"], np.broadcast_to(mean[:, None, None, :], pose.shape), rtol=1e-13)
    _within(pose, maxprob, ref, f"constant S2={S2}")


@pytest.mark.parametrize("S2", [81, 4096, 6400, 9216])
def test_soft_argmax_non_finite_rows(gpu_device, S2):
    """A row with a NaN, one of all -inf and one with +inf are NaN as in torch.softmax; the other
    rows of the launch are untouched."""
    c = _case(S2, 2, 4)
    f = c["features"].copy()
    f[0, 0, 1, S2 // 3], f[1, 1, 0], f[2, 0, 3, S2 - 1] = np.nan, -np.inf, np.inf
    bad = np.zeros((3, 2, 4), bool)
    bad[0, 0, 1] = bad[1, 1, 0] = bad[2, 0, 3] = True
    tpose, tmax = R.torch_f32_soft_argmax(f, c["center_grid"], c["offset"])
    assert np.array_equal(np.isnan(tmax), bad) and np.array_equal(np.isnan(tpose).all(axis=3), bad)
    pose, maxprob = _run(gpu_device, f, c["center_grid"], c["offset"])
    assert np.array_equal(np.isnan(maxprob), bad)
    assert np.array_equal(np.isnan(pose).all(axis=3), bad) and np.array_equal(np.isnan(pose).any(axis=3), bad)
    _within(pose, maxprob, R.soft_argmax_ref(f, c["center_grid"], c["offset"]), f"non-finite S2={S2}")
    clean, cleanmax = _run(gpu_device, c["features"], c["center_grid"], c["offset"])
    assert np.array_equal(pose[~bad], clean[~bad]) and np.array_equal(maxprob[~bad], cleanmax[~bad])


def _offset_view(t, elems):
    """A contiguous copy of t that starts `elems` elements into its buffer."""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=t.device)
    v = buf[elems:].view(t.shape)
    v.copy_(t)
    return v


def test_soft_argmax_unaligned_views(gpu_device):
    """features (S2 % 4 == 0) and center_grid as contiguous views 4 bytes into their buffers:
    the scalar-load path and a realigned grid, equal bit for bit to the aligned call."""
    from fvp import ops

    c = _case(4096, 2, 4)
    f, g, o = (torch.from_numpy(c[k]).to(gpu_device) for k in ("features", "center_grid", "offset"))
    pose, maxprob = ops.soft_argmax(f, g, o, R.BETA)
    fv, gv = _offset_view(f, 1), _offset_view(g, 1)
    assert f.data_ptr() % 16 == 0 and fv.data_ptr() % 16 == 4 and fv.is_contiguous()
    assert g.data_ptr() % 8 == 0 and gv.data_ptr() % 8 == 4 and gv.is_contiguous()
    for feats, grid in ((fv, g), (f, gv), (fv, gv)):
        p2, m2 = ops.soft_argmax(feats, grid, o, R.BETA)
        assert torch.equal(p2, pose) and torch.equal(m2, maxprob)
    _within(pose.cpu().numpy(), maxprob.cpu().numpy(), c["ref"], "aligned S2=4096")
    # the C entry point refuses a grid it cannot read as pairs, before any launch
    from fvp import _lib

    out_p, out_m = torch.full_like(pose, -7.0), torch.full_like(maxprob, -7.0)
    with pytest.raises(_lib.FvpError, match="1002"):
        _lib.call("fvp_soft_argmax", fv.data_ptr(), 2, 4, 4096, gv.data_ptr(), o.data_ptr(), R.BETA,
                  out_p.data_ptr(), out_m.data_ptr(), ops._stream(f))
    torch.cuda.synchronize()
    assert (out_p == -7.0).all() and (out_m == -7.0).all()


# ---- fusion --------------------------------------------------------------------------------
def _fuse_inputs(J, P=5):
    rng = np.random.default_rng(100 + J)
    pose = rng.uniform(-5000.0, 5000.0, (3, P, J, 2)).astype(np.float32)
    w = rng.uniform(0.05, 0.95, (3 * P, J, 1)).astype(np.float32)
    w.reshape(-1)[::7] = 1e-30
    mp = rng.uniform(0.0, 1.0, (3, P, J)).astype(np.float32)
    return pose, w, mp


@pytest.mark.parametrize("J", [1, 15, 64, 65, 130])
def test_fuse_poses_vs_float64(gpu_device, J):
    from fvp import _lib, ops

    P = 5
    pose, w, mp = _fuse_inputs(J, P)
    wv = w.reshape(3, P, J)  # weight pairs that sum to 0: 0 / 0 on the x axis of one joint, the z axis of another
    wv[0, 1, 3 % J] = wv[1, 1, 3 % J] = 0.0
    wv[1, 4, J - 1] = wv[2, 4, J - 1] = 0.0
    fused_ref, allow, confs_ref, crel = R.fuse_ref(pose, w, mp)
    tp, tw, tm = (torch.from_numpy(a).to(gpu_device) for a in (pose, w, mp))
    fused, confs = ops.fuse_poses(tp, tw, tm)
    got, gc = fused.cpu().numpy(), confs.cpu().numpy()
    nan = np.isnan(fused_ref)
    assert nan.sum() == 2 and nan[1, 3 % J, 0] and nan[4, J - 1, 2] and np.array_equal(np.isnan(got), nan)
    err = np.abs(got - fused_ref)[~nan] / allow[~nan]
    cerr = np.abs(gc - confs_ref) / (crel * confs_ref)
    print(f"fuse J={J}: error {err.max() * 8:.3f} u of the larger coordinate (allowed 8), "
          f"confs {cerr.max():.3f} x allowance")
    assert err.max() <= 1.0 and cerr.max() <= 1.0
    # either output may be NULL; the other is unchanged
    f2, c2 = torch.full_like(fused, -7.0), torch.full_like(confs, -7.0)
    _lib.call("fvp_fuse_poses", tp.data_ptr(), tw.data_ptr(), tm.data_ptr(), P, J, f2.data_ptr(), None,
              ops._stream(tp))
    _lib.call("fvp_fuse_poses", tp.data_ptr(), None, tm.data_ptr(), P, J, None, c2.data_ptr(), ops._stream(tp))
    assert torch.equal(c2, confs) and np.array_equal(f2.cpu().numpy(), got, equal_nan=True)


# ---- proposal centres ----------------------------------------------------------------------
SCALE, BIAS, MIN_SCORE = [100.0, 100.5, 105.26316], [-4000.0, -3200.25, 0.0], 0.3


def _centers_ref(index3, conf, bbox, min_score):
    """human_detection_net.py:99-124 with torch ops on the CPU (as test_gpu_fullsize restates it)."""
    B, K = conf.shape
    ref = torch.zeros(B, K, 7)
    ref[:, :, 0:3] = index3.float() * torch.tensor(SCALE) + torch.tensor(BIAS)
    ref[:, :, 4] = conf
    ref[:, :, 3] = (conf > torch.tensor(min_score, dtype=torch.float32)).float() - 1.0
    ref[:, :, 5:7] = bbox
    return ref


def _same_bits(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0, posinf=7e30, neginf=-7e30),
                       torch.nan_to_num(b, nan=-7.0, posinf=7e30, neginf=-7e30)) and \
        torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b))


@pytest.mark.parametrize("min_score", [MIN_SCORE, -0.25])
@pytest.mark.parametrize("Z", [1, 2, 64, 65, 200])
def test_proposal_centers_z_pick(gpu_device, Z, min_score):
    """B * K = 300 (two blocks).  z by the header's rule: NaN first, then the largest value,
    the lowest index on ties."""
    from fvp import ops

    B, K = 3, 100
    g = torch.Generator().manual_seed(Z)
    idx2 = torch.randint(0, 80, (B, K, 2), generator=g)
    hm = torch.rand((B, K, Z), generator=g)
    confs = torch.rand((B, K), generator=g) * 2.0 - 0.5  # some negative, for the negative threshold
    bbox = torch.rand((B, K, 2), generator=g)
    last = Z - 1
    hm[0, 0, 0] = hm[0, 0, last] = 2.0            # tie of the first and last z: the first
    hm[0, 1, last] = float("nan")                 # NaN at the last z wins
    hm[0, 2, Z // 2] = hm[0, 2, last] = float("nan")  # two NaNs: the lower index
    hm[2, 99] = float("-inf")                     # all -inf: z = 0 (the last thread of block 2)
    hm[1, 50, last] = 3.0                         # plain maximum at the last z
    hm[2, 43, Z // 2] = 1.0                       # conf_2d * 1.0 == min_score exactly: invalid (strict)
    confs[2, 43] = min_score
    z = torch.zeros((B, K), dtype=torch.int64)
    for b in range(B):
        for k in range(K):
            row = hm[b, k]
            nan = torch.isnan(row).nonzero()
            z[b, k] = int(nan[0]) if len(nan) else int((row == row.max()).nonzero()[0])
    assert z[0, 0] == 0 and z[0, 1] == last and z[0, 2] == Z // 2 and z[2, 99] == 0 and z[1, 50] == last
    conf = confs * hm.gather(2, z[..., None]).squeeze(2)
    ref = _centers_ref(torch.cat([idx2, z[..., None]], dim=2), conf, bbox, min_score)
    assert ref[2, 43, 4] == torch.tensor(min_score, dtype=torch.float32) and ref[2, 43, 3] == -1.0
    to = lambda t: t.to(gpu_device)  # noqa: E731
    got = ops.proposal_centers(to(idx2), to(hm), to(confs), to(bbox), SCALE, BIAS, min_score).cpu()
    assert _same_bits(got, ref), f"{(got != ref).sum().item()} cells differ (NaN cells included)"
    assert 0 < (got[:, :, 3] == 0).sum() < B * K  # both verdicts occur


def test_proposal_centers_full_index(gpu_device):
    """index_dims == 3 (no 1-D maps) at B * K = 300."""
    from fvp import ops

    B, K = 3, 100
    g = torch.Generator().manual_seed(9)
    idx3 = torch.randint(0, 80, (B, K, 3), generator=g)
    confs = torch.rand((B, K), generator=g)
    confs[2, 99], confs[1, 0] = MIN_SCORE, float("nan")
    confs[0, 5] = float(np.nextafter(np.float32(MIN_SCORE), np.float32(1.0)))
    bbox = torch.rand((B, K, 2), generator=g)
    ref = _centers_ref(idx3, confs, bbox, MIN_SCORE)
    assert ref[2, 99, 3] == -1.0 and ref[0, 5, 3] == 0.0 and ref[1, 0, 3] == -1.0
    to = lambda t: t.to(gpu_device)  # noqa: E731
    got = ops.proposal_centers(to(idx3), None, to(confs), to(bbox), SCALE, BIAS, MIN_SCORE).cpu()
    assert _same_bits(got, ref)


# ---- WeightNet -----------------------------------------------------------------------------
REL = 2e-5  # of the output maximum, the bar of tests/test_cnn_1d_weight.py


def _weight_net(dev, feat, hidden, hw, J=2):
    import cnn_arch
    from fvp import synthetic
    from fvp.cnn import FvpWeightNet

    wn = cnn_arch.WeightNet(J, hw, feat, hidden).eval()
    wn.load_state_dict(synthetic.seeded_state_dict(wn, feat + hidden))
    return wn, FvpWeightNet(copy.deepcopy(wn).to(dev))


@pytest.mark.parametrize("feat,hidden,hw", [
    (33, 64, (16, 16)),    # the 64-wide template with 31 guarded channels
    (1, 64, (16, 16)),
    (32, 257, (16, 16)),   # the hidden-layer loop's second trip: one unit, then 44
    (32, 300, (16, 16)),
    (32, 64, (2, 2)),      # one pooled cell
    (32, 64, (3, 2)),
    (32, 64, (33, 19)),    # floor pooling on both axes, two trips of the pooled-cell loop
    (32, 64, (124, 124)),  # 64,160 B of LDS
    (32, 64, (125, 124)),  # 64,664 B: the limit is 64 KiB of LDS, not 124 rows
    (32, 64, (126, 124)),  # 65,168 B: the largest map of this width that fits
])
def test_weight_net_shapes_vs_float64(gpu_device, feat, hidden, hw):
    wn, fvp_wn = _weight_net(gpu_device, feat, hidden, hw)
    x = torch.randn((3, 1, 2) + hw, generator=torch.Generator().manual_seed(hw[0] * 1000 + hw[1] + feat))
    with torch.no_grad():
        ref = copy.deepcopy(wn).double()(x.double()).numpy()
    got = fvp_wn(x.to(gpu_device)).cpu().numpy()
    assert got.shape == ref.shape == (3, 2, 1)
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)
    print(f"WeightNet C={feat} Hd={hidden} {hw}: error {err:.3g} of the output maximum (allowed {REL})")
    assert err <= REL
    assert np.ptp(ref) > 100 * REL * np.abs(ref).max()  # the six maps' weights are told apart


def test_weight_net_map_beyond_lds_is_refused(gpu_device):
    """(H + 2) * (W + 2) + 5 * 32 + 4 floats must fit 64 KiB (fvp.h): 127 x 124 is the first map
    of that width that does not.  FVP_ERR_SHAPE, and nothing is launched."""
    from fvp import _lib
    from fvp.ops import _stream

    assert ((126 + 2) * 126 + 164) * 4 <= 64 * 1024 < ((127 + 2) * 126 + 164) * 4
    _, net = _weight_net(gpu_device, 32, 64, (127, 124))
    x = torch.randn((6, 127, 124), device=gpu_device)
    out = torch.full((6,), -7.0, device=gpu_device)
    with pytest.raises(_lib.FvpError, match="1002"):
        _lib.call("fvp_weight_net", x.data_ptr(), 6, 127, 124, net.conv_w.data_ptr(), net.scale.data_ptr(),
                  net.shift.data_ptr(), 32, net.w1.data_ptr(), net.b1.data_ptr(), 64, net.w2.data_ptr(),
                  net.b2.data_ptr(), out.data_ptr(), _stream(out))
    torch.cuda.synchronize()
    assert (out == -7.0).all()


def test_weight_net_nan_pixel_stays_in_its_map(gpu_device):
    _, net = _weight_net(gpu_device, 32, 64, (16, 16))
    x = torch.randn((3, 1, 2, 16, 16), generator=torch.Generator().manual_seed(2)).to(gpu_device)
    clean = net(x)
    x[1, 0, 1, 8, 8] = float("nan")
    got = net(x)
    bad = torch.zeros((3, 2, 1), dtype=torch.bool, device=gpu_device)
    bad[1, 1, 0] = True
    assert torch.equal(torch.isnan(got), bad) and not torch.isnan(clean).any()
    assert torch.equal(got[~bad], clean[~bad])


# ---- scatter, selection, max planes --------------------------------------------------------
SENTINEL = -12345.0


def _scatter_case(dev, B, K, J, p_keep, conf_col, layout, seed):
    from fvp import ops

    g = torch.Generator().manual_seed(seed)
    mask = torch.rand((B, K), generator=g) < p_keep
    idx = mask.nonzero()
    P = idx.shape[0]
    fused = torch.randn((P, J, 3), generator=g)
    pose = torch.randn((3, P, J, 2), generator=g)
    confs = torch.rand((P,), generator=g)
    if layout == "wide":        # a [B, K, 7] view of a [B, K, 9] buffer
        base = torch.randn((B, K, 9), generator=g)
        view = lambda t: t[:, :, 1:8]  # noqa: E731
    elif layout == "transposed":  # a [K, B, 7] tensor seen as [B, K, 7]
        base = torch.randn((K, B, 7), generator=g)
        view = lambda t: t.transpose(0, 1)  # noqa: E731
    else:
        base = torch.randn((B, K, 7), generator=g)
        view = lambda t: t  # noqa: E731
    dbase = base.clone().to(dev)
    af = torch.full((B, K, J, 3), SENTINEL, device=dev)
    ap = torch.full((3, B, K, J, 2), SENTINEL, device=dev)
    assert view(dbase).stride(2) == 1 and (layout == "plain") != (not view(dbase).is_contiguous())
    ops.scatter_poses(idx.to(dev), fused.to(dev), pose.to(dev), confs.to(dev), af, ap, view(dbase), conf_col)
    rf, rp, rbase = torch.full((B, K, J, 3), SENTINEL), torch.full((3, B, K, J, 2), SENTINEL), base.clone()
    rf[mask] = fused
    rp[:, mask] = pose
    view(rbase)[mask, conf_col] = confs
    torch.cuda.synchronize()
    assert torch.equal(af.cpu(), rf) and torch.equal(ap.cpu(), rp)
    assert torch.equal(dbase.cpu(), rbase)  # the other columns, rows and the buffer around the view
    assert P == 0 or (rbase != base).sum() == P
    return P


@pytest.mark.parametrize("B,K,J,p_keep,conf_col,layout", [
    (4, 10, 15, 0.6, 4, "wide"),
    (4, 10, 15, 0.6, 0, "transposed"),
    (3, 7, 5, 0.5, 6, "wide"),
    (4, 10, 3, 2.0, 6, "transposed"),   # P = B * K: every slot
    (30, 20, 1, 0.7, 0, "plain"),       # J = 1 with P * J > 256: thread = proposal, two blocks
    (30, 20, 1, 2.0, 4, "wide"),
])
def test_scatter_poses_strided_centers(gpu_device, B, K, J, p_keep, conf_col, layout):
    P = _scatter_case(gpu_device, B, K, J, p_keep, conf_col, layout, seed=B * K + J)
    assert P == B * K if p_keep > 1 else 0 < P < B * K
    assert J > 1 or P * J > 256


@pytest.mark.parametrize("B,K,W,on", [
    (5, 9, 1, None),             # rows one float wide
    (6, 1, 7, None),             # K = 1
    (4, 10, 7, [(3, 9)]),        # only the last element
    (1, 1025, 3, [(0, 1023), (0, 1024)]),   # the two sides of the 1,024-entry tile seam
    (2, 1025, 2, [(0, 1023), (0, 1024), (1, 1022), (1, 1023), (1, 1024)]),
])
def test_mask_select_edges(gpu_device, B, K, W, on):
    from fvp import ops

    g = torch.Generator().manual_seed(B * K + W)
    if on is None:
        mask = torch.rand((B, K), generator=g) < 0.5
    else:
        mask = torch.zeros((B, K), dtype=torch.bool)
        for b, k in on:
            mask[b, k] = True
    big = torch.randn((B, K, W + 2), generator=g)
    rows = big.to(gpu_device)[:, :, 1:1 + W]
    idx, frame_of, sel = ops.mask_select(mask.to(gpu_device), rows)
    ref = mask.nonzero()
    assert len(ref) > 0
    assert torch.equal(idx.cpu(), ref) and torch.equal(frame_of.cpu(), ref[:, 0].to(torch.int32))
    assert torch.equal(sel.cpu(), big[:, :, 1:1 + W][mask])
    assert torch.equal(ops.mask_nonzero(mask.to(gpu_device)).cpu(), ref)


@pytest.mark.parametrize("S", [1, 2, 7, 33, 63, 64, 65])
def test_max_planes_every_size_class(gpu_device, S):
    """The 16-rows-per-wave kernel up to its last rows (63, 64) and the per-cell kernel's first
    size (65): negatives, a NaN and a -inf, bit for bit torch.max over each axis."""
    from fvp import ops

    P, J = 2, 3
    cubes = torch.randn((P, J, S, S, S), generator=torch.Generator().manual_seed(S))
    cubes[0, 1, S - 1, S // 2, S - 1] = float("nan")
    cubes[1, 2, 0, S - 1, S // 3] = float("-inf")
    cubes[1, 0, S // 2] = float("-inf")          # a whole x-slab: -inf cells in the xy and xz planes
    ref = torch.cat([cubes.max(dim=4).values, cubes.max(dim=3).values, cubes.max(dim=2).values])
    got = ops.max_planes(cubes.to(gpu_device)).cpu()
    assert got.shape == ref.shape == (3 * P, J, S, S)
    assert torch.isnan(ref).sum() == 3 and torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.isinf(ref).sum() >= 2 * S
    assert torch.equal(torch.nan_to_num(got, nan=0.0, neginf=-1e30), torch.nan_to_num(ref, nan=0.0, neginf=-1e30))
    assert torch.equal(torch.isinf(got), torch.isinf(ref))
