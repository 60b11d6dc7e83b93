"""tests/nms_select_model.py itself (no device): the maps of test_gpu_nms_select.py land on
the intended side of the select kernel's list capacity and on the intended kernel, the
candidate count never exceeds its bound, and the modelled fallback reproduces the oracle --
and, as the kernel was before round 0 could take any key, the oracle's list shifted by one
when a NaN sits at flat index 0."""
import numpy as np
import pytest

import nms_select_model as S
from oracle import fvp_oracle as O


def _count(p, K):
    return S.candidate_count(S.masked_map(p), K)


def _oracle_flat(p, K):
    return O.nms2d(p[None, None], K)[2][0]


@pytest.mark.parametrize("X,Y,K", S.OVER_CAPACITY)
@pytest.mark.parametrize("nan0", [True, False], ids=["nan0", "clean"])
def test_over_capacity_maps_reach_the_fallback(X, Y, K, nan0):
    assert S.dispatch(X, Y, K) == ("select", 32, False)
    p = S.over_capacity_map(X, Y, K, nan0)
    C = _count(p, K)
    print(f"{X}x{Y} K={K} nan0={nan0}: C = {C}")
    assert S.SEL_CAP < C <= S.capacity_bound(X * Y, K)
    peaks = p.reshape(-1)[p.reshape(-1) > 1]  # in index order
    assert len(peaks) == 5 and len(set(peaks)) == 5
    assert not np.array_equal(peaks, np.sort(peaks)[::-1])  # value order is not index order
    assert np.isnan(p.reshape(-1)[0]) == nan0


def test_second_nan_and_zero_plateau_maps_reach_the_fallback():
    X, Y, K = S.OVER_CAPACITY[0]
    p = S.over_capacity_map(X, Y, K, True, extra_nans=1)
    nans = np.flatnonzero(np.isnan(p.reshape(-1)))
    assert len(nans) == 2 and nans[0] == 0 and nans[1] > 400
    assert _count(p, K) > S.SEL_CAP
    X, Y, K = S.ZERO_PLATEAU
    assert S.dispatch(X, Y, K) == ("select", 32, False)
    for nan0 in (False, True):
        p = S.zero_plateau_map(X, Y, K, peaks=5, seed=3, nan0=nan0)
        flat = p.reshape(-1)
        zeros = flat[flat == 0]
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()  # both signs of zero
        assert (flat > 0).sum() == 5
        assert _count(p, K) > S.SEL_CAP
    # the same values on a map whose width is no multiple of 1024 stay on the list path: the
    # -0.0 cells next to the plateau then spread over more than K rows (why ZERO_PLATEAU is 12 x 2048)
    wide = S.zero_plateau_map(12, 2048, K, peaks=5, seed=3).reshape(-1)[:24 * 1000].reshape(24, 1000)
    assert _count(wide, K) <= S.SEL_CAP


@pytest.mark.parametrize("X,Y,K,drop,want", S.CAPACITY_EDGE)
def test_capacity_edge_counts_are_exact(X, Y, K, drop, want):
    assert S.dispatch(X, Y, K) == ("select", 32, False)
    assert _count(S.adversarial_map(X, Y, K, drop=drop), K) == want
    assert want + drop == S.capacity_bound(X * Y, K)  # the undropped map meets the bound exactly


@pytest.mark.parametrize("K", [9, 16])
def test_mixed_batch_counts(K):
    over, plain, at_cap = (_count(p, K) for p in S.mixed_batch(K))
    assert over > S.SEL_CAP and plain < 100 and at_cap == S.SEL_CAP
    assert np.isnan(S.mixed_batch(K)[0, 0, 0])


@pytest.mark.parametrize("name,X,Y,K,want", S.INSTANTIATIONS, ids=[c[0] for c in S.INSTANTIATIONS])
def test_instantiation_shapes_reach_the_intended_kernel(name, X, Y, K, want):
    assert S.dispatch(X, Y, K) == want
    p = S.instantiation_map(X, Y)
    nans = np.flatnonzero(np.isnan(p.reshape(-1)))
    assert len(nans) == 1 and nans[0] > 0
    assert _count(p, K) <= S.SEL_CAP


def test_dispatch_boundaries():
    """nms_any's arithmetic at its edges: M = 32512 is the select kernel's largest map (what
    sel_lds <= 159 KiB admits), M = 37236 the largest map of all (lds <= 150 KiB)."""
    assert S.dispatch(127, 256, 16) == ("select", 32, False) and S.dispatch(1, 32513, 16) == ("topk",)
    assert S.dispatch(127, 256, 17) == ("topk",)
    assert S.dispatch(1, 37236, 16) == ("topk",) and S.dispatch(1, 37237, 16) is None
    assert S.dispatch(*S.REJECTED) is None
    assert S.dispatch(4, 4, 17) is None  # K > X * Y
    # every instantiation nms_any can launch has a shape in the suite's NMS tests
    # (test_gpu_parity.py: 4x4, 37x53, 60x60, 80x80, 300x1, 2x1500; test_gpu_nms_select.py: the rest)
    shapes = [(4, 4), (37, 53), (60, 60), (80, 80), (128, 128), (300, 1), (2, 1500)]
    shapes += [(X, Y) for _, X, Y, _, _ in S.INSTANTIATIONS] + [(180, 180)]
    seen = {S.dispatch(X, Y, 4) for X, Y in shapes}
    assert {("select", E, True) for E in (1, 2, 4, 8, 16)} <= seen
    assert {("select", E, False) for E in (2, 4, 8, 16, 32)} <= seen and ("topk",) in seen


def _random_maps():
    rng = np.random.default_rng(5)
    for X, Y in [(1, 1), (4, 4), (3, 5), (37, 53), (80, 80), (1, 1500), (129, 128), (136, 129), (180, 180),
                 (127, 256)]:
        M = X * Y
        u = rng.random((X, Y)).astype(np.float32)
        sparse = np.where(u > 0.995, u, 0).astype(np.float32)
        nans = S.quantised_map(X, Y, seed=M)
        nans.reshape(-1)[rng.integers(0, M, size=max(1, M // 200))] = np.nan
        yield from (u, -u, sparse, np.zeros((X, Y), np.float32), S.quantised_map(X, Y, seed=M + 1), nans,
                    np.full((X, Y), np.nan, np.float32))
        yield (np.arange(M) % 1024 < 100).astype(np.float32).reshape(X, Y)  # an unaligned band of ones


def test_candidate_count_never_exceeds_its_bound():
    """C <= (K - 1) * 16 * ceil(M / 1024) + 1 and C >= K, on random, sparse, constant, NaN and
    banded maps; the modelled selection equals the oracle's on each."""
    n = 0
    for p in _random_maps():
        masked = S.masked_map(p)
        for K in (1, 2, 9, 16):
            if K > p.size:
                continue
            C = S.candidate_count(masked, K)
            assert K <= C <= S.capacity_bound(p.size, K), (p.shape, K, C)
            assert np.array_equal(S.select(masked, K), _oracle_flat(p, K)), (p.shape, K)
            n += 1
    assert n > 250


def test_model_fallback_is_the_oracle_and_the_old_rounds_drop_a_nan_at_zero():
    """Over capacity the modelled rounds give the oracle's list; with round 0 bounded by ~0 (the
    kernel before its fix) a NaN at flat index 0 is skipped, and the list is the oracle's top
    K + 1 without its first entry.  Without that NaN both agree with the oracle."""
    cases = [(S.over_capacity_map(X, Y, K, nan0), K, nan0) for X, Y, K in S.OVER_CAPACITY for nan0 in (True, False)]
    X, Y, K = S.ZERO_PLATEAU
    cases += [(S.zero_plateau_map(X, Y, K, peaks=5, seed=3, nan0=n), K, n) for n in (True, False)]
    for p, K, nan0 in cases:
        masked = S.masked_map(p)
        assert S.candidate_count(masked, K) > S.SEL_CAP
        ref = _oracle_flat(p, K + 1)
        assert np.array_equal(S.select(masked, K), ref[:K])
        old = S.select(masked, K, round0_takes_any=False)
        assert np.array_equal(old, ref[1:] if nan0 else ref[:K])
        assert (ref[0] == 0) == nan0
