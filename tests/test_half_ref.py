"""CPU tests of tests/half_ref.py, the criterion the fp16 backbone head
(fvp_conv1x1_cl_f16) is held to: a correct fp32 evaluation followed by .half() passes,
every planted fault fails, and each case keeps the cap on elements whose interval holds
more than one fp16 value."""
import numpy as np
import pytest
import torch

import half_ref as HR

SHAPES = [(256, 15), (256, 17), (64, 15), (16, 1), (32, 32)]


def test_half_is_tensor_half():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-9, 6, 4096),
                        [0.0, -0.0, 65504.0, 65519.99, 65520.0, -65520.0, 1e9, 2.0 ** -25, 2.0 ** -24 * 1.5,
                         1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]])  # ties go to even, 65520 is the first inf
    want = torch.from_numpy(a).half().double().numpy()
    assert np.array_equal(HR.half(a), want)
    assert HR.half(np.array([65520.0]))[0] == np.inf and HR.half(np.array([65519.99]))[0] == 65504.0


def test_round_toward_zero_model():
    a = np.array([1.0 + 2.0 ** -11 * 1.5, -(1.0 + 2.0 ** -11 * 1.5), 1e6, -1e6, 0.5, 2.0 ** -26], np.float32)
    assert np.array_equal(HR.half_rtz(a), [1.0, -1.0, 65504.0, -65504.0, 0.5, 0.0])
    r = np.random.default_rng(1).standard_normal(2000).astype(np.float32)
    z = HR.half_rtz(r)
    assert (np.abs(z) <= np.abs(r.astype(np.float64))).all()
    assert (np.abs(HR.half(r) - z) <= np.abs(r) * 2.0 ** -10).all()


@pytest.mark.parametrize("cin,J", SHAPES)
def test_fp32_evaluation_passes_and_cap_holds(cin, J):
    c = HR.case(100 + cin + J, 2, 3, 33, cin, J)
    print(f"Cin {cin} J {J}: share of wide intervals {c['share']:.3f} (seed {c['seed']})")
    assert c["share"] <= HR.CAP
    g = HR.emulate(c["x"], c["w"], c["scale"], c["shift"])
    ok = HR.inside(g, c["ref"], c["tol"])
    assert ok.all(), f"{np.count_nonzero(~ok)} of {ok.size} outside"


@pytest.mark.parametrize("fault", HR.FAULTS)
@pytest.mark.parametrize("cin,J", SHAPES[:3])
def test_planted_faults_fail(cin, J, fault):
    c = HR.case(100 + cin + J, 2, 3, 33, cin, J)
    g = HR.emulate(c["x"], c["w"], c["scale"], c["shift"], fault=fault)
    bad = ~HR.inside(g, c["ref"], c["tol"])
    print(f"Cin {cin} J {J} fault {fault}: {bad.mean():.3f} of the elements leave their interval")
    assert bad.any()
    if fault == "rtz":  # a systematic fault: about half the conversions differ from nearest-even
        assert bad.mean() > 0.3
    if fault == "row":  # only the last pixel is wrong
        bad[-1, :, -1, -1] = False
        assert not bad.any()


def test_overflow_and_nan_follow_the_same_inequality():
    ref = np.array([7e4, -7e4, 65519.0, 65521.0, np.nan, 1.0])
    tol = np.array([1.0, 1.0, 0.5, 0.5, 0.0, 0.0])
    assert HR.inside(np.array([np.inf, -np.inf, 65504.0, np.inf, np.nan, 1.0]), ref, tol).all()
    assert not HR.inside(np.array([65504.0, -65504.0, np.inf, 65504.0, 0.0, np.nan]), ref, tol).any()
    # an interval that straddles the overflow threshold admits both
    assert HR.inside(np.array([65504.0, np.inf]), np.array([65520.0, 65520.0]), np.array([1.0, 1.0])).all()


def test_tiny_cases_redraw_until_the_cap_holds():
    for J in (1, 15):
        c = HR.case(7, 1, 1, 1, 16, J)
        assert c["share"] <= HR.CAP and c["seed"] >= 7
