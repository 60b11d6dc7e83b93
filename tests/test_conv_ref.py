"""tests/conv_ref.py on the CPU: the float64 reference against loops over the definitions,
and the bound against an fp32 emulation of the kernels' accumulation orders with and without
planted faults, on every case of tests/conv_cases.py small enough to emulate (EMULATE_MAX
products: 163 of the table's 327 cases, every family, mode, stride and channel variation).

Measured here (numbers to read the GPU ratios of tests/test_gpu_conv_routes.py against, not
tolerances): the largest emulation err / tol is 0.118 (fp32 operands) and 0.044 (bf16).  The
smallest err / tol a planted fault reaches on a case it applies to is 428 ("chunk"; "tap" 477,
"seam" 1.6e3, "twice" 2.3e3, "shift" 4.1e3, "res" 5.0e3, "parity" 5.6e4; "row" leaves a NaN,
counted as infinite).
"""
import numpy as np
import pytest

import conv_cases as C
import conv_ref as R

EMULATE_MAX = 5_000_000  # N Ho Wo Cout K products


def _emulated():
    out = []
    for c in C.all_cases():
        kh, kw, ho, wo = C.geometry(c)
        if c.N * ho * wo * c.Cout * kh * kw * (c.cpi or R.rup(c.Cin, 16)) <= EMULATE_MAX:
            out.append(c)
    return out


def _setup(c):
    """(positional args, keyword args) of reference / tolerance / emulate, and the route."""
    import torch

    from fvp import cnn

    conv, bn = C.modules(c)
    layer = cnn.ConvLayer(conv, bn, dtype=torch.bfloat16 if c.bf16 else torch.float32, cpi=c.cpi, algo=c.algo)
    layer.act_bf16 = c.out_bf16
    route = cnn.conv_route(layer, c.N, c.H, c.W, in_bf16=c.in_bf16)
    x, res_pre, res_post = C.inputs(c)
    args = (x, conv.weight.detach().numpy(), layer.scale[:c.Cout].numpy(), layer.shift[:c.Cout].numpy(), c.mode)
    kw = dict(stride=c.stride, pad=c.pad, res_pre=res_pre, res_post=res_post, bf16=c.bf16)
    return args, kw, route, layer.Cpi


def _ratio(got, ref, tol):
    err = np.abs(got.astype(np.float64) - ref)
    err[~np.isfinite(err)] = np.inf
    return float((err / tol).max())


@pytest.mark.parametrize("mode, k, stride, pad", [
    (0, (3, 3), (1, 1), (1, 1)), (0, (3, 3), (2, 2), (2, 2)), (0, (2, 5), (1, 3), (1, 4)), (0, (1, 1), (4, 2), (0, 0)),
    (0, (7, 3), (4, 2), (0, 1)), (1, (2, 2), None, None), (2, (2,), None, None), (3, (4, 4), None, None)],
    ids=lambda v: str(v).replace(" ", ""))
def test_reference_matches_the_definition(mode, k, stride, pad):
    """conv_raw (torch's float64 conv2d / conv_transpose2d) against conv_def's loops: every mode,
    strides with padding, non-square kernels, odd sizes."""
    rng = np.random.default_rng(mode * 100 + k[0])
    n, cin, cout, h, w = 2, 3, 5, (1 if mode == 2 else 7), 9
    x = rng.standard_normal((n, cin, h, w))
    wt = rng.standard_normal((cout, cin) + k if mode == 0 else (cin, cout) + k)
    a = R.conv_raw(x, wt, mode, stride or (1, 1), pad or (0, 0))
    b = R.conv_def(x, wt, mode, stride or (1, 1), pad or (0, 0))
    assert a.shape == b.shape == (n, cout) + R.out_hw(h, w, R.w4(wt, mode).shape[2], R.w4(wt, mode).shape[3], mode,
                                                      stride, pad)
    assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()


def test_bf16_rounding_is_nearest_even():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.14159], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.140625], np.float32)
    assert np.array_equal(R.bf16_round(a), want)


def test_emulation_inside_the_bound_and_every_fault_outside():
    """An fp32 evaluation in the kernels' summation orders (the route's K depth, split-K factor
    and family order) stays at or below 1.0 x tol on every emulated case; every planted fault
    that applies to a case exceeds tol there on at least one element."""
    cases = _emulated()
    assert len(cases) >= 150
    worst, planted, bad, seen = {False: 0.0, True: 0.0}, {}, [], set()
    for c in cases:
        args, kw, route, cpi = _setup(c)
        assert isinstance(route[0], int), (C.case_id(c), route)
        ref = R.reference(*args, relu=c.relu, **kw)
        tol = R.tolerance(*args, cpi=cpi, **{k: v for k, v in kw.items()})
        ekw = dict(kw, relu=c.relu, cpi=cpi, order="chunk" if route[0] == 2 else "tap", kc=route[3], ks=route[5],
                   bn=route[2])
        r = _ratio(R.emulate(*args, **ekw), ref, tol)
        worst[c.bf16] = max(worst[c.bf16], r)
        if not r <= 1.0:
            bad.append(f"{C.case_id(c)}: emulation at {r:.3g} x tol")
        last = c.Cout - (c.Cout - 1) // route[2] * route[2]
        faults = ["tap", "chunk", "row", "seam"] + (["shift"] if last >= 2 else []) + \
            (["res"] if c.res_pre and c.res_post and c.relu else []) + (["parity"] if c.mode == 3 else []) + \
            (["twice"] if route[5] > 1 else [])
        for f in faults:
            fr = _ratio(R.emulate(*args, fault=f, **ekw), ref, tol)
            seen.add(f)
            planted[f] = min(planted.get(f, np.inf), fr)
            if not fr > 1.0:
                bad.append(f"{C.case_id(c)}: fault {f} stays inside tol ({fr:.3g})")
    print(f"emulation err / tol: fp32 {worst[False]:.3g}, bf16 {worst[True]:.3g}; smallest planted ratios: "
          + ", ".join(f"{k} {v:.3g}" for k, v in sorted(planted.items())))
    assert seen == set(R.FAULTS), set(R.FAULTS) - seen
    assert not bad, "\n".join(bad)
