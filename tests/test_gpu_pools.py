"""The memory-movement kernels of the CNNs (csrc/fvp_conv.hip, csrc/fvp_copy.hip) bit for bit: the
eleven max-pool instantiations (maxpool_kernel<KH,KW> and maxpool_bf16_kernel<KH,KW> at KH, KW in
{1, 2}, maxpool_pad_kernel, maxpool3s2_kernel, maxpool_pad_bf16_kernel), heatmaps_to_cl_kernel<1|2|4|8>
and nchw_to_nhwc_kernel behind fvp_nchw_to_nhwc, both kernels behind fvp_nhwc_to_nchw, and
copy_f4_kernel.  Reference: tests/pool_ref.py (pinned to torch's CPU max_pool2d by
tests/test_pool_ref.py); cases and inputs: tests/pool_cases.py, whose docstring says which case
reaches which kernel.

Every launch goes through the C entry points with _lib.call.  Every input is a view in the middle
of a NaN-filled buffer: a pool propagates NaN, so a tap read outside the input turns an output into
NaN.  Every output is the middle of a buffer whose guards hold SENTINEL and whose inside is prefilled
with a value no input holds (NaN will not do: it is a legitimate result here): everything inside
must be written, nothing outside may change.  Pools: NaN at the reference's positions, every other
element equal as int32 (int16 for bf16), so -0 and +0 differ.  Layouts and the copy: all bits equal,
padding channels +0.  A test runs all cases of its entry point and collects every failure before it
asserts.

Not covered: the fast pool's guard at H*W*C/4 >= 2^31 (it needs a 32-GiB input), grids beyond 2^31
blocks, and planar_to_cl_half_kernel (tests/test_gpu_cl_half.py holds it to bits).  The refusals,
the 16-B alignment rule among them, are checked on the CPU only (tests/test_pool_ref.py): no kernel
is launched on a misaligned pointer.

What ran on an MI355X when the file was written (a record, not a tolerance: the criterion is bit
equality): 40 unpadded and 97 padded pool launches (7 of the fp32 ones on maxpool3s2_kernel, the
N = 65536 case on maxpool_pad_kernel), 44 + 30 layout launches, 5 copies and 10 wrapper calls; every
one equal to the reference in every bit, nothing written outside an output, nothing inside left
unwritten.  No defect found in a kernel.  The file takes 3 s, tests/test_pool_ref.py 8 s on the CPU.
"""
import numpy as np
import pytest
import torch

import pool_cases as C
import pool_ref as R
from test_gpu_cnn_edges import IN_GUARD, _nan_view
from test_gpu_conv_routes import GUARD, SENTINEL

pytestmark = pytest.mark.gpu


def _call(fn, *args):
    from fvp import _lib

    _lib.call(fn, *args)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _guarded(dev, n, dtype):
    """(whole buffer, the n output elements in its middle): guards hold SENTINEL, the inside PREFILL."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    buf[GUARD:GUARD + n] = R.PREFILL
    return buf, buf[GUARD:GUARD + n]


def _guards(buf, n, what, bad):
    for name, g in (("before", buf[:GUARD]), ("after", buf[GUARD + n:])):
        if not bool((g == SENTINEL).all()):
            bad.append(f"{what}: {int((g != SENTINEL).sum())} elements written {name} the output")


def _judge_pool(got, ref, what, bad):
    """got: device tensor; ref: float32 numpy of the same shape.  NaN by position, the rest by bits."""
    got = got.cpu()
    want = torch.from_numpy(ref).to(got.dtype)
    it = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    gn, wn = got.isnan(), want.isnan()
    diff = (gn != wn) | (~wn & (got.view(it) != want.view(it)))
    if bool(diff.any()):
        i = tuple(int(v) for v in diff.nonzero()[0])
        bad.append(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ ({int((gn != wn).sum())} by NaN, "
                   f"{int((got == R.PREFILL).sum())} not written), the first at {i}: got {float(got[i])!r}, "
                   f"reference {float(want[i])!r}")


def _run_pool(dev, c, fn, args, bad, what=None):
    what = what or C.pool_id(c)
    dt = torch.bfloat16 if c.bf16 else torch.float32
    x = C.data(c)
    ref = R.pool(x, c.k, c.s, c.p)
    xin = _nan_view(dev, torch.from_numpy(x).to(dt))
    buf, out = _guarded(dev, ref.size, dt)
    _call(fn, xin.data_ptr(), c.N, c.H, c.W, c.C, *args, out.data_ptr(), _stream(out))
    torch.cuda.synchronize()
    _guards(buf, ref.size, what, bad)
    _judge_pool(out.view(ref.shape), ref, what, bad)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_maxpool_nhwc_every_window(gpu_device, bf16):
    """fvp_maxpool_nhwc / _bf16: KH, KW in {1, 2}, floor mode; fvp_maxpool2_nhwc on the 2 x 2 cases."""
    bad, n = [], 0
    for c in C.unpadded(bf16):
        _run_pool(gpu_device, c, "fvp_maxpool_nhwc_bf16" if bf16 else "fvp_maxpool_nhwc", c.k, bad)
        n += 1
        if not bf16 and c.k == (2, 2):
            _run_pool(gpu_device, c, "fvp_maxpool2_nhwc", (), bad, C.pool_id(c) + " (fvp_maxpool2_nhwc)")
            n += 1
    print(f"fvp_maxpool_nhwc{'_bf16' if bf16 else ''}: {n} launches, {len(bad)} failures")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_maxpool_pad_nhwc_every_geometry(gpu_device, bf16):
    """fvp_maxpool_pad_nhwc / _bf16 on the ten (K, S, P); fp32 (3, 2, 1) on the fast kernel up to the
    grid boundary and on the generic kernel one image past it."""
    bad, cases = [], C.padded(bf16)
    for c in cases:
        _run_pool(gpu_device, c, "fvp_maxpool_pad_nhwc_bf16" if bf16 else "fvp_maxpool_pad_nhwc",
                  (c.k[0], c.s[0], c.p[0]), bad)
    print(f"fvp_maxpool_pad_nhwc{'_bf16' if bf16 else ''}: {len(cases)} launches ({sum(map(C.fast, cases))} on the "
          f"fast kernel), {len(bad)} failures")
    assert not bad, "\n".join(bad)


def _bits_view(dev, x):
    """int32 numpy x as a float32 device view in the middle of a NaN-filled buffer."""
    return _nan_view(dev, torch.from_numpy(x).view(torch.float32))


def _judge_bits(got, ref, what, bad):
    got = got.cpu().view(torch.int32).numpy().reshape(ref.shape)
    if not np.array_equal(got, ref):
        d = got != ref
        i = tuple(int(v) for v in np.argwhere(d)[0])
        bad.append(f"{what}: {int(d.sum())} of {d.size} elements differ ({int((got == C.PREFILL_BITS).sum())} not "
                   f"written), the first at {i}: got {int(got[i]):#x}, reference {int(ref[i]):#x}")


def test_nchw_to_nhwc_every_pitch(gpu_device):
    """fvp_nchw_to_nhwc: the float4 layout kernel at Cp 4, 8, 16, 32, the element kernel otherwise;
    padding channels +0; pixel counts that do not fill a wave."""
    bad, cases = [], C.to_nhwc_cases()
    for c in cases:
        x = C.bits((c.N, c.C, c.H, c.W), *c)
        ref = R.nchw_to_nhwc(x, c.Cp, C.PREFILL_BITS)
        xin = _bits_view(gpu_device, x)
        buf, out = _guarded(gpu_device, ref.size, torch.float32)
        _call("fvp_nchw_to_nhwc", xin.data_ptr(), c.N, c.C, c.H, c.W, c.Cp, out.data_ptr(), _stream(out))
        torch.cuda.synchronize()
        _guards(buf, ref.size, str(c), bad)
        _judge_bits(out, ref, str(c), bad)
    print(f"fvp_nchw_to_nhwc: {len(cases)} launches, {len(bad)} failures")
    assert not bad, "\n".join(bad)


def test_nhwc_to_nchw_every_tile_edge(gpu_device):
    """fvp_nhwc_to_nchw: the tiled kernel at 63, 64, 65 and 129 pixels and C up to 128, the element
    kernel at C = 129 and at a pitch of 6; what lies between C and Cp never reaches the output."""
    bad, cases = [], C.to_nchw_cases()
    for c in cases:
        x = C.bits((c.N, c.H, c.W, c.Cp), *c)
        ref = R.nhwc_to_nchw(x, c.C, C.PREFILL_BITS)
        xin = _bits_view(gpu_device, x)
        buf, out = _guarded(gpu_device, ref.size, torch.float32)
        _call("fvp_nhwc_to_nchw", xin.data_ptr(), c.N, c.C, c.H, c.W, c.Cp, out.data_ptr(), _stream(out))
        torch.cuda.synchronize()
        _guards(buf, ref.size, str(c), bad)
        _judge_bits(out, ref, str(c), bad)
    print(f"fvp_nhwc_to_nchw: {len(cases)} launches, {len(bad)} failures")
    assert not bad, "\n".join(bad)


def test_copy_f4_every_block_edge(gpu_device):
    """fvp_copy_f4 (bench.py's measured_copy_gbs): 0, 1, 255, 256 and 257 float4."""
    bad = []
    for nb in C.COPY_BYTES:
        x = C.bits((nb // 4,), "copy", nb)
        # (pointers from the whole buffers: an empty view's data_ptr() is NULL)
        src = torch.full((x.size + 2 * IN_GUARD,), float("nan"), device=gpu_device)
        src[IN_GUARD:IN_GUARD + x.size].view(torch.int32).copy_(torch.from_numpy(x))
        buf, dst = _guarded(gpu_device, x.size, torch.float32)
        _call("fvp_copy_f4", src.data_ptr() + 4 * IN_GUARD, buf.data_ptr() + 4 * GUARD, nb, _stream(buf))
        torch.cuda.synchronize()
        _guards(buf, x.size, f"{nb} bytes", bad)
        _judge_bits(dst, R.copy_f4(x, C.PREFILL_BITS), f"{nb} bytes", bad)
    assert not bad, "\n".join(bad)


def test_python_wrappers_on_odd_sizes(gpu_device):
    """fvp.cnn.maxpool2 (both dims), maxpool_pad (both precisions each) and to_nchw_from (c0 = 1: a
    pointer 4 B off, the element kernel; c0 = 4: the tiled kernel) against the same references: a
    wrong output shape in a wrapper shows too."""
    from fvp import cnn

    bad = []
    for bf16 in (False, True):
        dt, ch = (torch.bfloat16, 24) if bf16 else (torch.float32, 20)
        for c, run in ((C.Pool(False, bf16, 3, 5, 7, ch, (2, 2), (2, 2), (0, 0)), lambda a: cnn.maxpool2(a)),
                       (C.Pool(False, bf16, 2, 1, 9, ch, (1, 2), (1, 2), (0, 0)), lambda a: cnn.maxpool2(a, dim=1)),
                       (C.Pool(True, bf16, 3, 5, 7, ch, (3, 3), (2, 2), (1, 1)), lambda a: cnn.maxpool_pad(a, 3, 2, 1)),
                       (C.Pool(True, bf16, 3, 5, 7, ch, (2, 2), (3, 3), (1, 1)), lambda a: cnn.maxpool_pad(a, 2, 3, 1))):
            x = C.data(c)
            ref = R.pool(x, c.k, c.s, c.p)
            y = run(cnn.Act(_nan_view(gpu_device, torch.from_numpy(x).to(dt)), c.C))
            torch.cuda.synchronize()
            what = "wrapper " + C.pool_id(c)
            if tuple(y.t.shape) != ref.shape or y.t.dtype != dt or y.C != c.C:
                bad.append(f"{what}: output {tuple(y.t.shape)} {y.t.dtype}, C {y.C}; reference {ref.shape}")
            else:
                _judge_pool(y.t, ref, what, bad)
    for f in C.FROM:
        x = C.bits((f.N, f.H, f.W, f.Cp), *f)
        ref = R.nhwc_to_nchw(np.ascontiguousarray(x[..., f.c0:]), f.C, C.PREFILL_BITS)
        y = cnn.to_nchw_from(cnn.Act(_bits_view(gpu_device, x), f.Cp), f.c0, f.C)
        torch.cuda.synchronize()
        if tuple(y.shape) != ref.shape:
            bad.append(f"{f}: output {tuple(y.shape)}, reference {ref.shape}")
        else:
            _judge_bits(y, ref, str(f), bad)
    assert not bad, "\n".join(bad)
