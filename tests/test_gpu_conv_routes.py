"""Every kernel instantiation conv_launch of csrc/fvp_conv.hip can start -- conv_mfma_kernel
(per tap, 12 variants), conv_halo_kernel (14), conv_bf16_kernel (12), conv_dma_kernel (8) --
against float64 (tests/conv_ref.py; the cases and how they are chosen: tests/conv_cases.py).

Every case asserts the route it was built for (fvp.cnn.conv_route: the decision the launcher
itself switches on) and that the layer ran the direct kernel, every output element against
the derived worst-case bound tol = c (K + 8) u (|scale| Babs + |shift| + |res_pre| +
|res_post|) (c = 1 fp32, 2 bf16 operands, against the reference on bf16-rounded operands), the
2e-5-of-scale criterion of tests/test_cnn.py against float64 (fp32 operands), exact zeros in
the padding channels, and that nothing outside the output was written and everything inside
was: the output is the middle of a larger buffer, pre-filled with NaN between two guard
regions of a sentinel.  bf16 outputs are not bounded: they must equal the same layer's fp32
output rounded to bf16, bit for bit.  A test runs all cases of its variant (or variation) and
collects every failure before it asserts; it prints the largest err / tol it saw (pytest -s).

Largest err / tol per instantiation (conv_cases.variant_id: family, operands, BM x BN, K
depth, variant, split-K) over the whole file, measured on an MI355X (a record, not a
tolerance: the bound is worst-case, a ratio above 1 is a defect of the kernel):

    per-tap-f32-256x16-k16-v1         0.038    halo-f32-64x64-k16-v7             0.013
    per-tap-f32-64x16-k16-v2          0.018    halo-f32-32x64-k16-v3             0.028
    per-tap-f32-64x16-k16-v2-split    0.013    halo-f32-32x64-k16-v7             0.009
    per-tap-f32-128x32-k16-v1         0.093    bf16-bf16-128x32-k16-v0           0.024
    per-tap-f32-64x32-k16-v1          0.081    bf16-bf16-128x32-k16-v1           0.004
    per-tap-f32-64x32-k16-v1-split    0.016    bf16-bf16-128x32-k32-v0           0.002
    per-tap-f32-64x32-k32-v1          0.011    bf16-bf16-128x32-k32-v1           0.011
    per-tap-f32-64x32-k32-v1-split    0.014    bf16-bf16-128x64-k16-v0           0.046
    per-tap-f32-128x64-k16-v1         0.208    bf16-bf16-128x64-k16-v1           0.007
    per-tap-f32-64x64-k16-v1          0.034    bf16-bf16-128x64-k32-v0           0.003
    per-tap-f32-32x64-k16-v1          0.118    bf16-bf16-128x64-k32-v1           0.027
    per-tap-f32-32x64-k16-v1-split    0.016    bf16-bf16-64x64-k16-v0            0.033
    halo-f32-256x16-k16-v3            0.038    bf16-bf16-64x64-k16-v1            0.004
    halo-f32-256x16-k16-v7            0.016    bf16-bf16-64x64-k32-v0            0.002
    halo-f32-64x16-k16-v3             0.016    bf16-bf16-64x64-k32-v1            0.019
    halo-f32-64x16-k16-v7             0.006    dma-f32-128x32-k32-v4             0.045
    halo-f32-128x32-k16-v3            0.068    dma-f32-128x64-k32-v4             0.127
    halo-f32-128x32-k16-v7            0.052    dma-f32-128x64-k16-v4             0.020
    halo-f32-64x32-k16-v3             0.042    dma-bf16-128x32-k64-v4            0.004
    halo-f32-64x32-k16-v7             0.037    dma-bf16-128x64-k64-v4            0.013
    halo-f32-128x64-k16-v3            0.036    dma-bf16-128x128-k64-v8           0.015
    halo-f32-128x64-k16-v7            0.016    dma-bf16-128x64-k32-v4            0.002
    halo-f32-64x64-k16-v3             0.032    dma-bf16-128x128-k32-v8           0.002

The largest ratios (0.1 - 0.2) are the transposed modes 1 and 2 with K = Cpi = 16 products,
where the epilogue's few roundings weigh most; the bf16 ratios stay below the fp32 ones, so
the matrix instruction's accumulation uses none of the factor 2 the bound grants it.  No
case found a defect.

(tests/test_conv_ref.py: the fp32 emulation of the same summation orders reaches 0.118 with
fp32 and 0.044 with bf16 operands on the CPU; the planted faults start at 428.)
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_cases as C
import conv_ref as R

pytestmark = pytest.mark.gpu

GUARD = 4096        # elements of each guard region (keeps the output 16-byte aligned)
SENTINEL = -8192.0  # exact in bf16 and fp32


def _layer(dev, c, conv, bn, algo=None):
    from fvp import cnn

    layer = cnn.ConvLayer(conv.to(dev), bn.to(dev), dtype=torch.bfloat16 if c.bf16 else torch.float32, cpi=c.cpi,
                          algo=c.algo if algo is None else algo)
    return layer


def _acts(dev, c, x, res_pre, res_post, out_bf16):
    """(x, res_pre, res_post) as NHWC activations on the device in the storage the case asks for."""
    from fvp import cnn

    xa = cnn.to_nhwc(torch.from_numpy(x).to(dev), c.cpi)
    if c.in_bf16:
        xa = cnn.Act(xa.t.to(torch.bfloat16), xa.C)
    res = []
    for r in (res_pre, res_post):
        a = None if r is None else cnn.to_nhwc(torch.from_numpy(r).to(dev))
        res.append(cnn.Act(a.t.to(torch.bfloat16), a.C) if a is not None and out_bf16 else a)
    return xa, res[0], res[1]


def _guarded(dev, layer, c, dtype):
    """(whole buffer, the [N, Ho, Wo, Cpo] output view in its middle): guards hold SENTINEL, the
    output NaN."""
    ho, wo = C.geometry(c)[2:]
    n = c.N * ho * wo * layer.Cpo
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n].view(c.N, ho, wo, layer.Cpo)


def _call(dev, layer, c, x, res_pre, res_post, out_bf16, what, bad):
    """Run the layer into a guarded buffer; returns the output Act (fp32 or bf16)."""
    layer.act_bf16 = out_bf16
    xa, rp, rq = _acts(dev, c, x, res_pre, res_post, out_bf16)
    buf, out = _guarded(dev, layer, c, torch.bfloat16 if out_bf16 else torch.float32)
    layer._ws.clear()
    y = layer(xa, relu=c.relu, res_pre=rp, res_post=rq, out=out)
    torch.cuda.synchronize()
    kinds = [k for _, k in layer._ws.values()]
    if kinds != [c.algo == C.DMA and not c.bf16]:
        bad.append(f"{what}: the layer planned {kinds}, not the direct kernel")
    n = out.numel()
    for name, g in (("before", buf[:GUARD]), ("after", buf[GUARD + n:])):
        if not bool((g == SENTINEL).all()):
            bad.append(f"{what}: {int((g != SENTINEL).sum())} elements written {name} the output")
    if y.t.data_ptr() != out.data_ptr():
        bad.append(f"{what}: the result is not the out= buffer")
    return y


def _run(dev, c):
    """Run one case; returns (err / tol, list of failures)."""
    from fvp import cnn

    what, bad = C.case_id(c), []
    conv, bn = C.modules(c)
    x, res_pre, res_post = C.inputs(c)
    layer = _layer(dev, c, conv, bn)
    layer.act_bf16 = c.out_bf16
    route = cnn.conv_route(layer, c.N, c.H, c.W, in_bf16=c.in_bf16, residual=c.res_pre or c.res_post)
    if not isinstance(route[0], int) or C.route_variant(route, c.bf16) != c.variant:
        return 0.0, [f"{what}: route {route}, the case was built for {c.variant}"]
    scale, shift = layer.scale[:c.Cout].cpu().numpy(), layer.shift[:c.Cout].cpu().numpy()
    args = (x, conv.weight.detach().cpu().numpy(), scale, shift, c.mode)
    kw = dict(stride=c.stride, pad=c.pad, res_pre=res_pre, res_post=res_post, bf16=c.bf16)
    ref = R.reference(*args, relu=c.relu, **kw)
    tol = R.tolerance(*args, cpi=layer.Cpi, **kw)

    y = _call(dev, layer, c, x, res_pre, res_post, False, what, bad)
    got = cnn.to_nchw(y).cpu().numpy()
    if got.shape != ref.shape:
        return 0.0, bad + [f"{what}: output shape {got.shape}, expected {ref.shape}"]
    err = np.abs(got.astype(np.float64) - ref)
    err[~np.isfinite(err)] = np.inf  # (a NaN left from the pre-fill: an element never written)
    ratio = err / tol
    worst = float(ratio.max())
    if worst > 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        bad.append(f"{what}: {int((ratio > 1).sum())} of {ratio.size} elements outside tol, worst {worst:.3g} x tol "
                   f"at (n, c, y, x) = {tuple(int(v) for v in i)}: got {got[i]!r}, float64 {ref[i]!r}")
    if not c.bf16:
        close = R.close_ratio(got, ref)
        if not close <= 1.0:
            bad.append(f"{what}: max error {close * R.REL:.3g} of the output scale (> {R.REL})")
    pad = y.t[..., c.Cout:]
    if pad.numel() and int(torch.count_nonzero(pad)):
        bad.append(f"{what}: {int(torch.count_nonzero(pad))} non-zero values in padding channels "
                   f"{c.Cout}..{y.t.shape[3] - 1}")
    if c.out_bf16:  # the same epilogue value, cast: bit-identical to the fp32 output rounded to bf16
        yb = _call(dev, layer, c, x, res_pre, res_post, True, what + " (bf16 out)", bad)
        want = y.t.to(torch.bfloat16)
        if yb.t.dtype != torch.bfloat16 or not torch.equal(yb.t.view(torch.int16), want.view(torch.int16)):
            d = (yb.t.view(torch.int16) != want.view(torch.int16))
            bad.append(f"{what}: bf16 output differs from the fp32 output rounded to bf16 in {int(d.sum())} of "
                       f"{d.numel()} elements")
    return worst, bad


def _run_all(dev, cases):
    assert cases
    worst, bad = {}, []
    for c in cases:
        r, b = _run(dev, c)
        name = C.variant_id(c.variant)
        worst[name] = max(worst.get(name, 0.0), r)
        bad += b
    print("err / tol: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("variant", C.variants(), ids=C.variant_id)
def test_variant_vs_float64(gpu_device, variant):
    """The variant's full and ragged base case."""
    cases = C.base_cases(variant)
    assert [c.kind for c in cases] == ["full", "ragged"]
    _run_all(gpu_device, cases)


@pytest.mark.parametrize("name", list(C.VARIATIONS))
def test_variation_vs_float64(gpu_device, name):
    """Epilogue, stride, kernel-shape, mode and channel variations (conv_cases.VARIATIONS) on a
    small and a large launch of every family that takes them."""
    _run_all(gpu_device, C.variation_cases(name))


def test_split_k_without_workspace_equals_nosplit(gpu_device):
    """fvp_conv2d_nhwc_ex with a NULL workspace on a shape that splits K when it has one: the
    route says no split, and the result equals CONV_PER_TAP_NOSPLIT's bit for bit (and differs in
    summation order, so in bits, from the split launch -- or the comparison would show nothing)."""
    from fvp import _lib, cnn
    from fvp.ops import _ptr, _stream

    dev = gpu_device
    c = C.base_case(next(v for v in C.variants() if v.family == 1 and v.split and v.KC == 32), "ragged")
    conv, bn = C.modules(c)
    x = C.inputs(c)[0]
    split, nosplit = _layer(dev, c, conv, bn, cnn.CONV_PER_TAP), _layer(dev, c, conv, bn, cnn.CONV_PER_TAP_NOSPLIT)
    assert cnn.conv_route(split, c.N, c.H, c.W)[5] > 1 and cnn.conv_route(nosplit, c.N, c.H, c.W)[5] == 1
    xa = cnn.to_nhwc(torch.from_numpy(x).to(dev))
    y_split = split(xa, relu=True).t
    y_nosplit = nosplit(xa, relu=True).t
    plan = (ctypes.c_int * 8)()
    geo = (c.N, c.H, c.W, split.Cpi, split.KH, split.KW, split.Cpo, *split.geom())
    assert _lib.load().fvp_conv2d_ex_plan(*geo, 0, cnn.CONV_PER_TAP, 0, plan) == 0
    assert tuple(plan)[:6] == cnn.conv_route(nosplit, c.N, c.H, c.W)[:6]
    out = torch.full_like(y_split, float("nan"))
    _lib.call("fvp_conv2d_nhwc_ex", _ptr(xa.t), c.N, c.H, c.W, split.Cpi, _ptr(split.wpack), split.KH, split.KW,
              split.Cpo, split.Cpo_w, _ptr(split.scale), _ptr(split.shift), None, None, 1, *split.geom(), 0,
              cnn.CONV_PER_TAP, _ptr(out), None, 0, _stream(out))
    torch.cuda.synchronize()
    assert torch.equal(out, y_nosplit)
    assert not torch.equal(y_split, y_nosplit)
    assert float((y_split - y_nosplit).abs().max()) <= 1e-5 * float(y_nosplit.abs().max())
