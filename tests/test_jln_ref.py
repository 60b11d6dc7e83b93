"""The references and inputs of tests/jln_ref.py themselves (no device): the bound admits an
honest fp32 evaluation, and the designed inputs expose a lost cell by orders of magnitude."""
import numpy as np
import pytest

import jln_ref as R
from oracle import fvp_oracle as O


def _id(c):
    return f"S2={c[0]}-P{c[1]}-J{c[2]}"


@pytest.fixture(scope="module", params=R.CASES, ids=_id)
def case(request):
    c = R.make_case(*request.param)
    c["ref"] = R.soft_argmax_ref(c["features"], c["center_grid"], c["offset"])
    return c


def test_reference_is_the_oracle(case):
    coords, confs = O.soft_argmax(case["features"], case["center_grid"], R.BETA)
    ref = case["ref"]
    assert np.array_equal(coords, ref["coords"])
    assert np.array_equal(O.add_offsets(coords, case["offset"]), ref["pose"])
    np.testing.assert_allclose(ref["maxprob"].mean(axis=(0, 2)), confs, rtol=1e-14, atol=0)


def test_peaks_cover_every_boundary(case):
    S2, peak = case["S2"], case["peak"]
    cells = R.peak_cells(S2)
    assert {0, S2 - 1} <= set(cells) and all(0 <= c < S2 for c in cells)
    assert set(peak.ravel()) == set(cells)  # 24 rows or more: every cell is some row's peak
    p = case["ref"]["maxprob"]
    assert (p > 0.9).all() if S2 > 1 else (p == 1.0).all()  # the peak holds about all the mass


def test_bound_is_tight_and_admits_fp32(case):
    ref = case["ref"]
    assert 0.0 < ref["bound"].max() <= 0.05  # mm; at or below the bar it replaces
    pose, maxprob = R.torch_f32_soft_argmax(case["features"], case["center_grid"], case["offset"])
    pr, mr = R.ratios(pose, maxprob, ref)
    print(f"S2={case['S2']}: bound {ref['bound'].min():.4f}..{ref['bound'].max():.4f} mm, "
          f"torch fp32 at {pr:.3f} x bound, maxprob {mr:.3f} x allowance")
    assert pr <= 1.0 and mr <= 1.0


def test_a_lost_peak_cell_is_seen(case):
    """Without the peak cell of each row the float64 pose moves by more than 1000 x bound."""
    S2 = case["S2"]
    drop = np.zeros((3, case["P"], case["J"], S2), bool)
    np.put_along_axis(drop, case["peak"][..., None], True, axis=3)
    lost = R.soft_argmax_ref(case["features"], case["center_grid"], case["offset"], drop=drop)
    if S2 == 1:  # nothing is left of a one-cell row
        assert np.isnan(lost["pose"]).all()
        return
    shift = (np.abs(lost["pose"] - case["ref"]["pose"]) / case["ref"]["bound"]).max(axis=3)
    assert shift.min() > 1000.0, f"row moved by only {shift.min():.1f} x bound"


@pytest.mark.parametrize("S2", R.CONSTANT_S2)
def test_constant_rows_give_the_grid_mean(S2):
    c = R.constant_case(S2)
    ref = R.soft_argmax_ref(c["features"], c["center_grid"], None)
    assert np.array_equal(ref["maxprob"] * S2, np.ones_like(ref["maxprob"]))
    mean = c["center_grid"].astype(np.float64).mean(axis=1)  # [3, 2]
    np.testing.assert_allclose(ref["pose"], np.broadcast_to(mean[:, None, None, :], ref["pose"].shape), rtol=1e-13)


def test_non_finite_rows_are_nan_in_the_reference():
    c = R.make_case(81)
    f = c["features"].copy()
    f[0, 0, 1, 5], f[1, 1, 0], f[2, 0, 3, 80] = np.nan, -np.inf, np.inf
    ref = R.soft_argmax_ref(f, c["center_grid"], c["offset"])
    bad = np.zeros((3, 2, 4), bool)
    bad[0, 0, 1] = bad[1, 1, 0] = bad[2, 0, 3] = True
    assert np.array_equal(np.isnan(ref["maxprob"]), bad) and np.array_equal(np.isnan(ref["pose"]).all(axis=3), bad)
    pose, maxprob = R.torch_f32_soft_argmax(f, c["center_grid"], c["offset"])
    assert np.array_equal(np.isnan(maxprob), bad) and np.array_equal(np.isnan(pose).all(axis=3), bad)
    pr, mr = R.ratios(pose, maxprob, ref)
    assert pr <= 1.0 and mr <= 1.0


def test_fuse_ref_allowance_admits_fp32():
    rng = np.random.default_rng(4)
    P, J = 5, 65
    pose = rng.uniform(-5000, 5000, (3, P, J, 2)).astype(np.float32)
    w = rng.uniform(0.05, 0.95, (3 * P, J, 1)).astype(np.float32)
    w.reshape(-1)[::7] = 1e-30
    mp = rng.uniform(0, 1, (3, P, J)).astype(np.float32)
    fused, allow, confs, crel = R.fuse_ref(pose, w, mp)
    wp = w.reshape(3, P, J)
    x32 = (wp[0] / (wp[0] + wp[1])) * pose[0, :, :, 0] + (wp[1] / (wp[0] + wp[1])) * pose[1, :, :, 0]
    assert x32.dtype == np.float32
    assert (np.abs(x32 - fused[:, :, 0]) <= allow[:, :, 0]).all()
    assert (np.abs(mp.mean(axis=(0, 2), dtype=np.float32) - confs) <= crel * confs).all()
