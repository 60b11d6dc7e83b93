"""Both Winograd kernels of csrc/fvp_wino.hip -- conv_wino_kernel<NB, XS> (F(2x2, 3x3)) and
deconv_wino_kernel<NB> (F(2x2, 2x2) per output parity) -- on every tile grid the planner
can choose, under every instantiation, against float64 (tests/wino_ref.py; the cases and
how they are chosen: tests/wino_cases.py).

Every case asserts the plan it was built for (grid and instantiation, from the host
planner), that the layer ran the Winograd kernel, every output element against the derived
worst-case bound tol = (Cpi + 16) u (|scale| Babs + |shift| + |res_pre| + |res_post|), the
2e-5-of-scale criterion of tests/test_cnn.py against the float64 reference, the fused pool
exactly where it is asked for, and exact zeros in the padding channels of the NHWC output.
A test runs all instantiations of its grid (or variant) and collects every failure before
it asserts; it prints the largest err / tol it saw (pytest -s).

Largest err / tol per instantiation over the whole file, measured on an MI355X (a record,
not a tolerance: the bound is worst-case, a ratio above 1 is a defect of the kernel):

    conv_wino_kernel<1,2>   0.036        deconv_wino_kernel<1>   0.085
    conv_wino_kernel<1,1>   0.053        deconv_wino_kernel<2>   0.151
    conv_wino_kernel<2,1>   0.052

(tests/test_wino_ref.py: the fp32 emulation of the same operation sequences reaches 0.034
for the conv and 0.085 for the deconv on the CPU; the planted faults start at 22.)  No case
found a defect.
"""
import numpy as np
import pytest
import torch

import wino_cases as C
import wino_ref as R

pytestmark = pytest.mark.gpu


def _run(dev, c):
    """Run one case; returns (err / tol, list of failures)."""
    from fvp import cnn

    what, bad = C.case_id(c), []
    conv, bn = C.modules(c)
    x, res_pre, res_post = C.inputs(c)
    ref_fn = R.conv3x3_ref if c.kernel == "conv" else R.deconv4s2_ref
    ref = ref_fn(x, conv, bn, relu=c.relu, res_pre=res_pre, res_post=res_post)
    tol = R.tolerance(x, conv, bn, res_pre, res_post)

    layer = cnn.ConvLayer(conv.to(dev), bn.to(dev), algo=cnn.CONV_WINO)
    plan = cnn.wino_plan(c.N, c.H, c.W, layer.Cpo)
    if plan[:2] != c.grid or plan[2:4] != c.inst:
        return 0.0, [f"{what}: plan {plan}, the case was built for grid {c.grid}, (NB, XS) {c.inst}"]
    act = [None if a is None else cnn.to_nhwc(torch.from_numpy(a).to(dev)) for a in (x, res_pre, res_post)]
    kw = dict(pool=True) if c.pool else {}
    y = layer(act[0], relu=c.relu, res_pre=act[1], res_post=act[2], **kw)
    torch.cuda.synchronize()
    kinds = [k for _, k in layer._ws.values()]
    if kinds != ["wino" if c.kernel == "conv" else "wino_dc"]:
        bad.append(f"{what}: ran {kinds}")
    got_t = cnn.to_nchw(y)
    got = got_t.cpu().numpy()
    if got.shape != ref.shape:
        return 0.0, bad + [f"{what}: output shape {got.shape}, expected {ref.shape}"]
    err = np.abs(got.astype(np.float64) - ref)
    err[~np.isfinite(err)] = np.inf
    ratio = err / tol
    worst = float(ratio.max())
    if worst > 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        bad.append(f"{what}: {int((ratio > 1).sum())} of {ratio.size} elements outside tol, worst {worst:.3g} x tol "
                   f"at (n, c, y, x) = {tuple(int(v) for v in i)}: got {got[i]!r}, float64 {ref[i]!r}")
    close = R.close_ratio(got, ref)
    if not close <= 1.0:
        bad.append(f"{what}: max error {close * R.REL:.3g} of the output scale (> {R.REL})")
    pad = y.t[..., c.Cout:]
    if pad.numel() and int(torch.count_nonzero(pad)):
        bad.append(f"{what}: {int(torch.count_nonzero(pad))} non-zero values in padding channels {c.Cout}..{y.t.shape[3] - 1}")
    if c.pool:
        if y.pooled is None:
            bad.append(f"{what}: no fused pool output")
        elif not torch.equal(cnn.to_nchw(y.pooled), torch.nn.functional.max_pool2d(got_t, 2, 2)):
            bad.append(f"{what}: fused pool differs from max_pool2d of the launch's own output")
    return worst, bad


def _run_all(dev, cases):
    assert cases
    worst, bad = {}, []
    for c in cases:
        r, b = _run(dev, c)
        name = C.INST_NAME[c.kernel, c.inst]
        worst[name] = max(worst.get(name, 0.0), r)
        bad += b
    print("err / tol: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert not bad, "\n".join(bad)


def _grid_id(g):
    return f"{g[0]}x{g[1]}"


def _variant_id(v):
    return f"{v[0][0]}x{v[0][1]}-{v[1]}"


@pytest.mark.parametrize("grid", C.legal_grids(), ids=_grid_id)
def test_conv_grid_vs_float64(gpu_device, grid):
    """conv_wino_kernel<1,2>, <1,1> and <2,1> on the grid's single-block and multi-block image."""
    _run_all(gpu_device, C.grid_cases("conv", grid))


@pytest.mark.parametrize("grid", C.legal_grids(), ids=_grid_id)
def test_deconv_grid_vs_float64(gpu_device, grid):
    """deconv_wino_kernel<1> and <2> on the grid's single-block and multi-block image."""
    _run_all(gpu_device, C.grid_cases("deconv", grid))


@pytest.mark.parametrize("variant", C.variant_ids("conv"), ids=_variant_id)
def test_conv_variant_vs_float64(gpu_device, variant):
    """Epilogue and channel variants (wino_cases.VARIANTS) under every conv instantiation."""
    _run_all(gpu_device, C.variant_cases("conv", *variant))


@pytest.mark.parametrize("variant", C.variant_ids("deconv"), ids=_variant_id)
def test_deconv_variant_vs_float64(gpu_device, variant):
    """Epilogue and channel variants (wino_cases.VARIANTS) under both deconv instantiations."""
    _run_all(gpu_device, C.variant_cases("deconv", *variant))
