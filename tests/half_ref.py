"""The criterion for fp16 results of the backbone head (fvp_conv1x1_cl_f16), numpy /
torch-CPU only.  tests/test_half_ref.py pins this file on the CPU,
tests/test_gpu_heatmaps_f16.py holds the kernel to it.

Criterion.  With ref and tol from tests/conv_ref.py (reference(..., relu=False) and
tolerance(...), both float64: tol is the derived worst case of an fp32 evaluation in any
summation order), an fp16 result g is right iff

    half(ref - tol) <= g <= half(ref + tol)

half() being the rounding to nearest even of Tensor.half().  Rounding is monotone, so this
is exactly "g is the fp16 rounding of some value within the derived fp32 bound"; results
beyond +-65504 round to +-inf and are covered by the same inequality.

Cap (a condition on a case, not a measurement of the kernel): at most CAP of a case's
elements may have an interval that holds more than one fp16 value -- otherwise the case
pins too little.  case() draws x = max(N(0, 1), 0), w = N(0, 1) 0.016 / sqrt(Cin),
shift = N(0, 0.1), scale = 1 and, should the cap not hold (a tiny case: one wide element of
three), draws again with the next seed; only ref and tol enter that choice, never a result
of the code under test.

Planted faults (emulate(fault=...)), which the criterion must catch:
  rtz    the conversion rounds toward zero instead of to nearest even
  shift  the shift is not added
  chunk  the last 16 input channels are not added
  row    the last pixel is computed from its neighbour's row
"""
import numpy as np
import torch

import conv_ref

CAP = 0.30
FAULTS = ("rtz", "shift", "chunk", "row")


def half(a):
    """float64 / float32 array -> fp16 values (round to nearest even, +-inf beyond 65504) as float64."""
    with np.errstate(over="ignore"):
        return np.asarray(a).astype(np.float16).astype(np.float64)


def half_rtz(a):
    """float32 array -> fp16 values rounded toward zero (the planted fault), as float64."""
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore"):
        h = a.astype(np.float16)
    big = np.isinf(h) & np.isfinite(a)
    h = np.where(big, np.copysign(np.float16(65504.0), h), h).astype(np.float16)
    away = np.abs(h.astype(np.float64)) > np.abs(a.astype(np.float64))
    return np.where(away, np.nextafter(h, np.float16(0.0)), h).astype(np.float64)


def interval(ref, tol):
    return half(ref - tol), half(ref + tol)


def inside(g, ref, tol):
    """Elementwise: the fp16 values g (any float array) meet the criterion.  A NaN reference
    (a non-finite input) asks for NaN."""
    g = np.asarray(g, np.float64)
    lo, hi = interval(ref, tol)
    return np.where(np.isnan(ref), np.isnan(g), (lo <= g) & (g <= hi))


def wide_share(ref, tol):
    """Share of elements whose interval holds more than one fp16 value."""
    lo, hi = interval(ref, tol)
    return float(np.mean(lo != hi))


def draw(seed, N, H, W, cin, J):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((N, cin, H, W)), 0).astype(np.float32)
    w = (rng.standard_normal((J, cin, 1, 1)) * 0.016 / np.sqrt(cin)).astype(np.float32)
    shift = (rng.standard_normal(J) * 0.1).astype(np.float32)
    scale = np.ones(J, np.float32)
    return x, w, scale, shift


def ref_tol(x, w, scale, shift):
    """(ref, tol) float64 [N, J, H, W] of the 1x1 layer."""
    cpi = conv_ref.rup(x.shape[1], 16)
    return (conv_ref.reference(x, w, scale, shift, 0, relu=False),
            conv_ref.tolerance(x, w, scale, shift, 0, cpi=cpi))


def case(seed, N, H, W, cin, J, tries=64):
    """dict(x, w, scale, shift, ref, tol, share, seed): the first draw from `seed` on whose cap holds."""
    for s in range(seed, seed + tries):
        x, w, scale, shift = draw(s, N, H, W, cin, J)
        ref, tol = ref_tol(x, w, scale, shift)
        share = wide_share(ref, tol)
        if share <= CAP:
            return dict(x=x, w=w, scale=scale, shift=shift, ref=ref, tol=tol, share=share, seed=s)
    raise AssertionError(f"no draw of {(N, H, W, cin, J)} within the cap from seed {seed}")


def emulate(x, w, scale, shift, fault=None):
    """A torch-CPU fp32 evaluation followed by .half(), [N, J, H, W] fp16 values as float64."""
    assert fault is None or fault in FAULTS, fault
    xt, wt = torch.from_numpy(x), torch.from_numpy(w[:, :, 0, 0])
    if fault == "chunk":
        c0 = (x.shape[1] - 1) // 16 * 16
        xt = xt.clone()
        xt[:, c0:] = 0
    if fault == "row":
        xt = xt.clone()
        flat = xt.permute(0, 2, 3, 1).reshape(-1, x.shape[1])
        flat[-1] = flat[-2] if flat.shape[0] > 1 else 0
        xt = flat.reshape(x.shape[0], x.shape[2], x.shape[3], x.shape[1]).permute(0, 3, 1, 2)
    y = torch.einsum("nchw,jc->njhw", xt, wt) * torch.from_numpy(scale)[None, :, None, None]
    if fault != "shift":
        y = y + torch.from_numpy(shift)[None, :, None, None]
    assert y.dtype == torch.float32
    if fault == "rtz":
        return half_rtz(y.numpy())
    return y.half().double().numpy()
