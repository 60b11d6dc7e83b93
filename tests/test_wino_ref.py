"""CPU checks of the Winograd grid sweep's own parts (tests/wino_ref.py, tests/wino_cases.py):
the float64 reference is torch's, the float64 Winograd restatement equals it (which pins the
transform matrices, the deconvolution's parity classes and tap order), a correct fp32
evaluation stays inside the derived bound on every image size of the table while each
planted fault leaves it, and the table reaches every tile grid under every kernel
instantiation with the plans the host planner returns."""
import copy

import numpy as np
import pytest
import torch

import wino_cases as C
import wino_ref as R

KERNELS = ("conv", "deconv")


def _torch64(c, x, res_pre, res_post):
    conv, bn = (copy.deepcopy(m).double() for m in C.modules(c))
    with torch.no_grad():
        y = bn(conv(torch.from_numpy(x).double()))
        if res_pre is not None:
            y = y + torch.from_numpy(res_pre).double()
        if c.relu:
            y = torch.relu(y)
        if res_post is not None:
            y = y + torch.from_numpy(res_post).double()
    return y.numpy()


def _ref(c, x, res_pre, res_post):
    fn = R.conv3x3_ref if c.kernel == "conv" else R.deconv4s2_ref
    return fn(x, *C.modules(c), relu=c.relu, res_pre=res_pre, res_post=res_post)


def _pin_cases():
    out = []
    for kernel in KERNELS:
        out += [C.grid_cases(kernel, g)[0] for g in ((2, 2), (3, 4), (5, 5), (2, 14))]
        out += [C.variant_cases(kernel, (4, 8), name)[0] for name in ("linear", "pre+post", "post-linear", "cin20")]
    return out


@pytest.mark.parametrize("c", _pin_cases(), ids=C.case_id)
def test_reference_is_torch_float64_and_winograd_restates_it(c):
    x, res_pre, res_post = C.inputs(c, n=2)
    want = _torch64(c, x, res_pre, res_post)
    scale = np.abs(want).max()
    got = _ref(c, x, res_pre, res_post)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * scale
    p = R.params(*C.modules(c))
    raw = (R.conv3x3_raw if c.kernel == "conv" else R.deconv4s2_raw)(x, p["w"])
    if c.kernel == "deconv":  # the gathered sum is the scattered definition
        assert np.abs(R.deconv4s2_scatter(x, p["w"]) - raw).max() <= 1e-12 * np.abs(raw).max()
    wino = R.winograd(x, p["w"])
    assert np.abs(wino - raw).max() <= 1e-12 * np.abs(raw).max()
    babs = R.winograd(x, p["w"], absolute=True)
    assert (babs >= np.abs(raw)).all()


def _shapes(kernel):
    """One case per distinct (H, W, Cin) of the table; every other one with both residuals."""
    seen = {}
    for c in C.all_cases(kernel):
        res = len(seen) % 2 == 1
        seen.setdefault((c.H, c.W, c.Cin), c._replace(inst=(1, 2), Cout=32, N=2, relu=True, pool=False,
                                                      res_pre=res, res_post=res))
    return list(seen.values())


@pytest.mark.parametrize("kernel", KERNELS)
def test_fp32_emulation_inside_bound_planted_faults_outside(kernel):
    """On every distinct (H, W, Cin) of the table (two images, so that the pixel past the
    last row's right edge exists in memory too): the fp32 emulation is inside tol
    everywhere; each planted fault puts at least one element outside it."""
    worst, least = 0.0, {f: np.inf for f in R.FAULTS}
    for c in _shapes(kernel):
        x, res_pre, res_post = C.inputs(c, n=2)
        conv, bn = C.modules(c)
        kw = dict(relu=c.relu, res_pre=res_pre, res_post=res_post)
        ref = _ref(c, x, res_pre, res_post)
        tol = R.tolerance(x, conv, bn, res_pre, res_post)
        assert tol.shape == ref.shape and (tol > 0).all()
        ratio = (np.abs(R.emulate(x, conv, bn, **kw) - ref) / tol).max()
        assert ratio <= 1.0, f"{C.case_id(c)}: fp32 emulation at {ratio:.3g} x tol"
        worst = max(worst, ratio)
        for fault in R.FAULTS:
            r = (np.abs(R.emulate(x, conv, bn, fault=fault, **kw) - ref) / tol).max()
            assert r > 1.0, f"{C.case_id(c)}: planted fault {fault!r} stays inside tol ({r:.3g} x)"
            least[fault] = min(least[fault], r)
    print(f"{kernel}: fp32 emulation <= {worst:.4f} x tol; planted faults >= "
          + ", ".join(f"{f} {v:.3g} x" for f, v in least.items()))


def test_table_reaches_every_grid_under_every_instantiation():
    grids = C.legal_grids()
    assert len(grids) == 52
    for kernel in KERNELS:
        reached = {}
        for c in C.all_cases(kernel):
            reached.setdefault(c.grid, set()).add(c.inst)
        assert set(reached) == set(grids)
        assert all(v == set(C.INSTS[kernel]) for v in reached.values()), reached
    multi = C.multi_images()
    assert set(multi) <= set(grids) and set(C.VARIANT_GRIDS) <= set(multi)
    assert {g: multi[g] for g in ((4, 8), (8, 4), (5, 5), (2, 14))} == \
        {(4, 8): (7, 29), (8, 4): (29, 7), (5, 5): (9, 17), (2, 14): (1, 53)}
    assert len(multi) == 35 and len(C.no_multi()) == 17
    print("grids without a multi-block case:", " ".join(f"{a}x{b}" for a, b in C.no_multi()))


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_case_states_the_host_planners_plan(kernel):
    from fvp import cnn

    cases = C.all_cases(kernel)
    assert len({C.case_id(c) for c in cases}) == len(cases)
    for c in cases:
        plan = cnn.wino_plan(c.N, c.H, c.W, R.rup(c.Cout, 32))
        assert plan[:2] == c.grid and plan[2:4] == c.inst, (C.case_id(c), plan)
        assert c.H % 2 == 1 and c.W % 2 == 1
        per = C.blocks_per_image(c.grid, c.H, c.W)
        assert plan[4] == c.N * per * (R.rup(c.Cout, 32) // 32) // c.inst[0]
        if c.kind == "single":
            assert per == 1
        else:
            assert per >= 2 and (c.H % (2 * c.grid[0]) or c.W % (2 * c.grid[1]))
        if c.inst == (1, 1):
            assert plan[4] > 256
        if c.inst[0] == 2:
            assert plan[4] >= 512
