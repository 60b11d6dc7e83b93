"""nms_select_kernel where no other test takes it: the over-capacity fallback (more than
kSelCap = 4096 candidates: K rounds of the largest key below the previous winner), a list
exactly at capacity, the instantiations <2,false>, <8,false> and <16,false>, and the
boundaries between the kernels nms_any chooses from.

Everything is compared bit for bit with oracle.fvp_oracle.nms2d -- the values as uint32 where
finite, NaN positions equal, then the flat indices, then the decoded xy -- and the fused
column gather with torch indexing.  tests/nms_select_model.py says how many candidates each
map makes and which kernel its shape reaches; a test asserts that first, so a fallback test
cannot pass by the list path.  (Before round 0 of the fallback could take any key, the maps
with a NaN at flat index 0 came back as the oracle's list shifted by one, the NaN missing.)"""
import numpy as np
import pytest
import torch

import nms_select_model as S
from oracle import fvp_oracle as O

pytestmark = pytest.mark.gpu

J, Z = 2, 3  # the small cube of the fused column gather


def _assert_bitwise(got, ref, what):
    v, xy, fl = (t.cpu().numpy() for t in got)
    ov, oxy, ofl = ref
    nan = np.isnan(ov)
    assert np.array_equal(np.isnan(v), nan), f"{what}: NaN positions differ: {v} vs {ov}"
    assert np.array_equal(v.view(np.uint32)[~nan], ov.view(np.uint32)[~nan]), f"{what}: values differ: {v} vs {ov}"
    assert np.array_equal(fl, ofl), f"{what}: flat indices differ: {fl} vs {ofl}"
    assert np.array_equal(xy, oxy), f"{what}: xy differs"


def _check(prob, K, dev, columns=True):
    """prob [B, X, Y] (numpy): nms2D, and nms2D_columns with its gather, against the oracle."""
    from fvp.proposal import nms2D, nms2D_columns

    prob = np.ascontiguousarray(prob[:, None])
    B, _, X, Y = prob.shape
    ref = O.nms2d(prob, K)
    pd = torch.from_numpy(prob).to(dev)
    _assert_bitwise(nms2D(pd, K), ref, "nms2D")
    if columns:
        g = torch.Generator().manual_seed(X * Y + K)
        cube = torch.rand((B, J, X, Y, Z), generator=g).to(dev)
        v, xy, fl, cols = nms2D_columns(pd, K, cube)
        _assert_bitwise((v, xy, fl), ref, "nms2D_columns")
        ofl = torch.from_numpy(ref[2]).to(dev)
        ref_cols = torch.stack([cube[b].reshape(J, X * Y, Z)[:, ofl[b]].permute(1, 0, 2) for b in range(B)])
        assert torch.equal(cols, ref_cols), "the fused gather's columns differ"
    return ref


def _counts(prob, K):
    return [S.candidate_count(S.masked_map(p), K) for p in prob]


@pytest.mark.parametrize("nan0", [True, False], ids=["nan0", "clean"])
@pytest.mark.parametrize("X,Y,K", S.OVER_CAPACITY)
def test_fallback_vs_oracle(gpu_device, X, Y, K, nan0):
    """More than 4096 candidates (7665, 4389, 4192 and 4311 of them): K - 1 rows of tied ones,
    five peaks whose values do not follow their indices, with and without a NaN at flat index
    0 -- the one element whose key is ~0."""
    assert S.dispatch(X, Y, K) == ("select", 32, False)
    p = S.over_capacity_map(X, Y, K, nan0)
    assert _counts([p], K)[0] > S.SEL_CAP
    ov, _, ofl = _check(p[None], K, gpu_device)
    assert np.isnan(ov[0, 0]) == nan0 and (ofl[0, 0] == 0) == nan0
    assert (ov[0, int(nan0):int(nan0) + 5] > 1).all()  # then the five peaks, by value


def test_fallback_two_nans_vs_oracle(gpu_device):
    """NaNs at flat index 0 and at a second index: both first, in index order."""
    X, Y, K = S.OVER_CAPACITY[0]
    p = S.over_capacity_map(X, Y, K, True, extra_nans=1)
    assert _counts([p], K)[0] > S.SEL_CAP
    ov, _, ofl = _check(p[None], K, gpu_device)
    assert np.isnan(ov[0, :2]).all() and not np.isnan(ov[0, 2:]).any() and ofl[0, 0] == 0 < ofl[0, 1]


@pytest.mark.parametrize("nan0", [False, True], ids=["clean", "nan0"])
def test_fallback_signed_zero_plateau_vs_oracle(gpu_device, nan0):
    """The plateau at -0.0 / +0.0 (both have the key of zero: ordered by index, each returned
    with its own sign) under five positive peaks, 5044 candidates.  On 12 x 2048 rather than
    one of the maps above: a -1.0 next to a zero becomes -0.0 and ties with the plateau, and
    only where the map's width is a multiple of 1024 do those cells stay within two 16-lane
    rows -- on the other maps they fill more than K rows and the list stays short
    (nms_select_model.zero_plateau_map)."""
    X, Y, K = S.ZERO_PLATEAU
    assert S.dispatch(X, Y, K) == ("select", 32, False)
    p = S.zero_plateau_map(X, Y, K, peaks=5, seed=3, nan0=nan0)
    assert _counts([p], K)[0] > S.SEL_CAP
    ov, _, _ = _check(p[None], K, gpu_device)
    zeros = ov[0][ov[0] == 0]
    assert len(zeros) == K - 5 - int(nan0)
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()  # both signs among the winners


@pytest.mark.parametrize("X,Y,K,drop,count", S.CAPACITY_EDGE, ids=[f"C{c[4]}" for c in S.CAPACITY_EDGE])
def test_list_at_capacity_vs_oracle(gpu_device, X, Y, K, drop, count):
    """C = 4097 is the first count that takes the fallback, C = 4096 fills the list to its last
    slot, C = 4001 is well within it."""
    p = S.adversarial_map(X, Y, K, drop=drop)
    assert _counts([p], K)[0] == count
    _check(p[None], K, gpu_device)


@pytest.mark.parametrize("K", [9, 16])
def test_mixed_batch_vs_oracle(gpu_device, K):
    """B = 3 at 180 x 180: a frame over capacity with a NaN at index 0, an ordinary quantised
    map and a frame exactly at capacity in one launch (a block per frame: the fallback of one
    leaves the others alone) -- contiguous, and as a channel slice of a [B, 2, X, Y] tensor,
    where the frame stride is 2 * X * Y and the other channel holds other values."""
    from fvp.proposal import nms2D, nms2D_columns

    prob = S.mixed_batch(K)
    over, plain, at_cap = _counts(prob, K)
    assert over > S.SEL_CAP and plain < 100 and at_cap == S.SEL_CAP
    ref = _check(prob, K, gpu_device)
    B, X, Y = prob.shape
    both = np.stack([np.random.default_rng(K).random(prob.shape).astype(np.float32), prob], axis=1)
    sl = torch.from_numpy(both).to(gpu_device)[:, 1:2]
    assert sl.stride()[0] == 2 * X * Y and not sl.is_contiguous()
    _assert_bitwise(nms2D(sl, K), ref, "nms2D on a channel slice")
    cube = torch.rand((B, J, X, Y, Z), generator=torch.Generator().manual_seed(K)).to(gpu_device)
    v, xy, fl, cols = nms2D_columns(sl, K, cube)
    _assert_bitwise((v, xy, fl), ref, "nms2D_columns on a channel slice")
    ofl = torch.from_numpy(ref[2]).to(gpu_device)
    assert torch.equal(cols, torch.stack([cube[b].reshape(J, X * Y, Z)[:, ofl[b]].permute(1, 0, 2) for b in range(B)]))


@pytest.mark.parametrize("name,X,Y,K,kernel", S.INSTANTIATIONS, ids=[c[0] for c in S.INSTANTIATIONS])
def test_instantiations_and_boundaries_vs_oracle(gpu_device, name, X, Y, K, kernel):
    """nms_select_kernel<2,false> (1 x 1500), <8,false> (4 x 1500), <16,false> (120 x 129), and
    both sides of each boundary in nms_any: strips of 16 against 17 (128 x 128 / 129 x 128),
    Y = 1024 against 1025, the select kernel's largest map against the K-round kernel's first
    (M = 32512 / 32513) and the largest map accepted (192 x 193).  Quantised maps (ties) with
    one NaN away from index 0, B = 2 with different frames."""
    assert S.dispatch(X, Y, K) == kernel
    prob = np.stack([S.instantiation_map(X, Y), S.quantised_map(X, Y, seed=X + Y)])
    assert max(_counts(prob, K)) <= S.SEL_CAP
    ov, _, _ = _check(prob, K, gpu_device)
    assert np.isnan(ov[0, 0]) and not np.isnan(ov[1]).any()


def test_map_beyond_the_largest_is_refused(gpu_device):
    """193 x 193 is one row past the largest map nms_any takes (192 x 193, above)."""
    from fvp import _lib
    from fvp.proposal import nms2D

    X, Y, K = S.REJECTED
    assert S.dispatch(X, Y, K) is None
    with pytest.raises(_lib.FvpError):
        nms2D(torch.zeros((1, 1, X, Y), device=gpu_device), K)
