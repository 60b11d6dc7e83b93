"""The hand-tiled kernels at the two ends of the networks (csrc/fvp_conv.hip) against float64:
conv_stem7_f32 / _bf16 (whose bodies also back the uint8 stems, tests/test_gpu_frames.py),
conv_front7_f32 / _bf16, conv1x1_nchw<4|8|16> and up2_head_nchw.  References, bounds and
criteria: tests/cnn_edge_ref.py (pinned on the CPU by tests/test_cnn_edge_ref.py); cases and
packed weights: tests/cnn_edge_cases.py.

Every launch goes through _lib.call with the production packers' weights.  fp32 outputs:
every element within the derived worst-case bound tol; bf16 outputs: every element inside
the interval of the bf16 values its pre-activation +- tol can round to, with the cap on wide
intervals asserted per case.  The output is the middle of a larger buffer, NaN between two
guard regions of a sentinel: everything inside must be written, nothing outside.  Every
input, weight, scale and shift array is a view in the middle of a NaN-filled buffer, so a
read past its end that reaches a result shows as NaN (plain in-bounds reads of one
allocation).  The persistent walks (stems, front7_f32, tail) repeat a case already checked
against float64 along N until every block walks two tiles or items and some three: every
copy must equal the small launch bit for bit.  A test runs all cases of its kernel and
collects every failure before it asserts; pytest -s prints what it measured.

Measured on an MI355X (a record, not a tolerance: the bound is worst-case, a ratio above 1 is
a defect of the kernel; nothing here is tuned to these numbers):

    conv_stem7_f32       err / tol 0.040         walk: 1,032 tiles on 512 blocks, 129 copies equal
    conv_stem7_bf16      wide share 0.031, 0 outside   walk: the same launch shape, equal
    conv_front7_f32      err / tol 0.014         walk: 1,032 tiles on 512 blocks, 129 copies equal
    conv_front7_bf16     wide share 0.089, 0 outside   (one tile per block: no walk)
    conv1x1_nchw<4>      err / tol 0.107 (Cin 1), 0.159 (15), 0.218 (16)
    conv1x1_nchw<8>      err / tol 0.085 (Cin 17), 0.106 (32)
    conv1x1_nchw<16>     err / tol 0.058 (Cin 33), 0.062 (50), 0.059 (64)
    conv1x1_nchw at a channel offset (FvpCNN._conv1x1_nchw, c0 16 and 36)   err / tol 0.129
    up2_head_nchw        err / tol 0.033 (Cpi 16, 1 K step), 0.034 (48, 3), 0.033 (64, 4),
                         0.023 (80, 5), 0.012 (128, 8); the two-launch path the same to every
                         digit printed (elsewhere asserted bit-equal)
                         walks: 4,098 items (Cpi 16) and 4,104 items (Cpi 80) on at most 2,048
                         blocks, 2,049 and 228 copies equal

The fp32 ratios are the CPU emulation's (tests/test_cnn_edge_ref.py) to two digits: the matrix
instructions' accumulation loses no more than a float32 summation does.

What these cases found when they were written: up2_head_nchw reads the folded BatchNorm of
all 32 y channels, and FvpCNN._compile_tail handed it the deconvolution layer's Cpo = 16
values where Cout <= 16 -- 64 bytes read past both arrays.  On all five Cs = 1 cases the NaN
of the guard reached every output (err / tol infinite); with the packer's 32 zero-padded
values they are at 0.012 to 0.034 of tol.  P2PNet itself has Cout = 32 and never read past
its arrays.
"""
import numpy as np
import pytest
import torch

import cnn_edge_cases as C
import cnn_edge_ref as E
from test_gpu_conv_routes import GUARD, SENTINEL

pytestmark = pytest.mark.gpu

IN_GUARD = 64  # elements of NaN on both sides of every input (a multiple of 4 floats: 16-B alignment stays)


def _nan_view(dev, t, reps=1):
    """CPU tensor t on the device, repeated `reps` times along dim 0, as a view in the middle
    of a NaN-filled buffer."""
    t = t.detach().contiguous()
    n = t.numel()
    buf = torch.full((n * reps + 2 * IN_GUARD,), float("nan"), dtype=t.dtype, device=dev)
    v = buf[IN_GUARD:IN_GUARD + n * reps].view(reps, n)
    v.copy_(t.reshape(1, n).to(dev))
    return v.view((reps * t.shape[0],) + tuple(t.shape[1:]))


def _guarded(dev, n, dtype=torch.float32):
    """(whole buffer, the n output elements in its middle): guards hold SENTINEL, the output NaN."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n]


def _guards(buf, n, what, bad):
    for name, g in (("before", buf[:GUARD]), ("after", buf[GUARD + n:])):
        if not bool((g == SENTINEL).all()):
            bad.append(f"{what}: {int((g != SENTINEL).sum())} elements written {name} the output")


def _bound(got, ref, tol, what, bad):
    """The fp32 criterion; returns the largest err / tol."""
    r = E.ratio(got, ref, tol)
    worst = float(r.max())
    if not worst <= 1.0:
        i = np.unravel_index(int(r.argmax()), r.shape)
        bad.append(f"{what}: {int((r > 1).sum())} of {r.size} elements outside tol ({int((~np.isfinite(got)).sum())} "
                   f"not finite), worst {worst:.3g} x tol at {tuple(int(v) for v in i)}: got {got[i]!r}, "
                   f"float64 {ref[i]!r}")
    return worst


def _same_bits(big, small, reps, what, bad):
    """Every one of the `reps` copies in big equals small bit for bit."""
    it = torch.int16 if small.dtype == torch.bfloat16 else torch.int32
    diff = (big.reshape(reps, -1).view(it) != small.reshape(1, -1).view(it)).any(dim=1)
    if bool(diff.any()):
        bad.append(f"{what}: {int(diff.sum())} of {reps} copies differ from the small launch, the first at copy "
                   f"{int(diff.nonzero()[0])}")


# ---- stems and front layers --------------------------------------------------------------
def _params7(dev, d):
    return tuple(_nan_view(dev, d[k]) for k in ("wpack", "scale_t", "shift_t"))


def _launch7(dev, k, c, x, params, what, bad):
    """One launch on the images x [N', C, H, W] (device); -> the [N', Ho, Wo, Cout] output view."""
    from fvp import _lib
    from fvp.ops import _ptr, _stream

    n_img = x.shape[0]
    ho, wo = E.out_hw7(k, c.H, c.W)
    n = n_img * ho * wo * k.cout
    buf, out = _guarded(dev, n, torch.bfloat16 if k.bf16 else torch.float32)
    wp, sc, sh = params
    _lib.call(k.fn, _ptr(x), n_img, c.C, c.H, c.W, _ptr(wp), _ptr(sc), _ptr(sh), _ptr(out), _stream(out))
    torch.cuda.synchronize()
    _guards(buf, n, what, bad)
    return out.view(n_img, ho, wo, k.cout)


def _judge7(k, d, y, what, bad):
    """-> (largest err / tol or 0, elements outside their interval or 0)."""
    got = y.permute(0, 3, 1, 2).double().cpu().numpy()
    if not k.bf16:
        return _bound(got, d["ref"], d["tol"], what, bad), 0
    ok = E.inside(got, d["pre"], d["tol"])
    if d["share"] > E.CAP:
        bad.append(f"{what}: wide share {d['share']:.3f} above the cap")
    if not ok.all():
        bad.append(f"{what}: {np.count_nonzero(~ok)} of {ok.size} elements outside their interval "
                   f"({int(np.isnan(got).sum())} NaN)")
    return 0.0, int(np.count_nonzero(~ok))


@pytest.mark.parametrize("name", sorted(E.KERNELS))
def test_7x7_vs_float64(gpu_device, name):
    """fvp_conv_stem7_f32 / _bf16 and fvp_conv_front7_f32 / _bf16 on every case of cnn_edge_cases.cases7."""
    k = E.KERNELS[name]
    worst, outside, share, bad = 0.0, 0, 0.0, []
    for c in C.cases7(name):
        d = C.data7(c)
        y = _launch7(gpu_device, k, c, _nan_view(gpu_device, torch.from_numpy(d["x"])), _params7(gpu_device, d),
                     C.id7(c), bad)
        r, o = _judge7(k, d, y, C.id7(c), bad)
        worst, outside, share = max(worst, r), outside + o, max(share, d["share"])
    print(f"{name}: " + (f"largest wide share {share:.3f}, {outside} elements outside their interval" if k.bf16
                         else f"largest err / tol {worst:.4f}"))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["stem7_bf16", "stem7_f32", "front7_f32"])
def test_7x7_persistent_walk(gpu_device, name):
    """min(tiles, 2 CUs) blocks walk the tiles: with more than twice that many (plus a remainder)
    every block computes two ragged tiles and some three, and a tile's result may not depend on
    the block or iteration that computes it."""
    k, c = E.KERNELS[name], C.walk_base7(name)
    d = C.data7(c)
    blocks = 2 * torch.cuda.get_device_properties(gpu_device).multi_processor_count
    ty, tx = E.tiles7(k, c.H, c.W)
    per = c.N * ty * tx
    reps = 2 * blocks // per + 1
    assert (ty, tx) == (2, 2) and 2 * blocks < reps * per < 3 * blocks
    bad, params, xs = [], _params7(gpu_device, d), torch.from_numpy(d["x"])
    small = _launch7(gpu_device, k, c, _nan_view(gpu_device, xs), params, "small launch", bad)
    r, o = _judge7(k, d, small, "small launch", bad)
    big = _launch7(gpu_device, k, c, _nan_view(gpu_device, xs, reps), params, "walk", bad)
    _same_bits(big, small, reps, f"{name} walk", bad)
    print(f"{name}: {reps * per} tiles on {blocks} blocks, {reps} copies bit-equal to the small launch "
          f"(err / tol {r:.4f}, outside {o})")
    assert not bad, "\n".join(bad)


# ---- the 1x1 head ------------------------------------------------------------------------
@pytest.mark.parametrize("cin", C.CIN1)
def test_conv1x1_nchw_vs_float64(gpu_device, cin):
    """fvp_conv1x1_nchw: Cout, ReLU, pixel counts around one block and blocks that straddle
    images, pitches at and above the 4 t4 channels read; finite random values in the padding
    channels, which the weights' zero rows must cancel."""
    from fvp import _lib
    from fvp.ops import _ptr, _stream

    dev, worst, bad, params = gpu_device, 0.0, [], {}
    for i, c in enumerate(C.cases1(cin)):
        conv, layer = C.packed1(c.Cin, c.Cout)
        if c.Cout not in params:
            params[c.Cout] = tuple(_nan_view(dev, t) for t in (layer.wpack, layer.scale, layer.shift))
        wp, sc, sh = params[c.Cout]
        rows = C.rows1(100 * cin + i, c.N, c.H, c.W, c.pitch)
        x = _nan_view(dev, torch.from_numpy(rows))
        n = c.N * c.Cout * c.H * c.W
        buf, out = _guarded(dev, n)
        _lib.call("fvp_conv1x1_nchw", _ptr(x), c.N, c.H, c.W, c.pitch, c.Cin, _ptr(wp), layer.Cpo_w, c.Cout, _ptr(sc),
                  _ptr(sh), c.relu, _ptr(out), _stream(out))
        torch.cuda.synchronize()
        _guards(buf, n, str(c), bad)
        ref, tol = E.ref1x1(C.nchw(rows, 0, c.Cin), conv.weight.detach().numpy()[:, :, 0, 0],
                            layer.scale[:c.Cout].numpy(), layer.shift[:c.Cout].numpy(), c.relu)
        worst = max(worst, _bound(out.view(ref.shape).double().cpu().numpy(), ref, tol, str(c), bad))
    print(f"conv1x1_nchw<{E.t4_of(cin)}> Cin {cin}: largest err / tol {worst:.4f}")
    assert not bad, "\n".join(bad)


def test_conv1x1_nchw_channel_offset(gpu_device):
    """FvpCNN._conv1x1_nchw(y, c0, o), the call CenterNet's merged heads make: channels c0 ..
    c0 + Cin - 1 of a wider Act, finite random values in every other channel."""
    from fvp import cnn

    dev, worst, bad = gpu_device, 0.0, []
    for i, c in enumerate(C.cases_off()):
        conv, bn = C.layer1(c.Cin, c.Cout, 8000 + i)
        layer = cnn.ConvLayer(conv.to(dev), bn.to(dev))
        rows = C.rows1(8100 + i, c.N, c.H, c.W, c.Cp)
        out = cnn.FvpCNN._conv1x1_nchw(cnn.Act(_nan_view(dev, torch.from_numpy(rows)), c.C), c.c0, layer)
        torch.cuda.synchronize()
        if out is None or tuple(out.shape) != (c.N, c.Cout, c.H, c.W):
            bad.append(f"{c}: no NCHW launch")
            continue
        ref, tol = E.ref1x1(C.nchw(rows, c.c0, c.Cin), conv.weight.detach().cpu().numpy()[:, :, 0, 0],
                            layer.scale[:c.Cout].cpu().numpy(), layer.shift[:c.Cout].cpu().numpy(), 0)
        worst = max(worst, _bound(out.double().cpu().numpy(), ref, tol, str(c), bad))
    print(f"conv1x1_nchw at a channel offset: largest err / tol {worst:.4f}")
    assert not bad, "\n".join(bad)


# ---- the fused tail ----------------------------------------------------------------------
def _params_tail(dev, d):
    wd, _, wh, _, scale, shift = d["f"].tail
    return tuple(_nan_view(dev, t) for t in (wd, scale, shift, wh, d["f"].out.scale, d["f"].out.shift))


def _launch_tail(dev, c, d, params, reps, what, bad):
    """fvp_up2_head_nchw on the case's images repeated `reps` times; -> [reps N, J, 2H, 2W]."""
    from fvp import _lib
    from fvp.ops import _ptr, _stream

    x = _nan_view(dev, torch.from_numpy(np.ascontiguousarray(d["x"].transpose(0, 2, 3, 1))), reps)
    skip = _nan_view(dev, torch.from_numpy(d["skip_rows"]), reps)
    n_img = reps * c.N
    n = n_img * c.J * 4 * c.H * c.W
    buf, out = _guarded(dev, n)
    wd, sc, sh, wh, hs, hb = params
    _lib.call("fvp_up2_head_nchw", _ptr(x), n_img, c.H, c.W, c.Cpi, _ptr(wd), _ptr(sc), _ptr(sh), _ptr(skip), c.Cps,
              c.Cs, _ptr(wh), _ptr(hs), _ptr(hb), c.J, _ptr(out), _stream(out))
    torch.cuda.synchronize()
    _guards(buf, n, what, bad)
    return out.view(n_img, c.J, 2 * c.H, 2 * c.W)


def _two_launches(dev, c, d):
    """The same tail as the deconvolution GEMM (+ skip) and fvp_conv1x1_nchw, with the folded
    BatchNorm values of the CPU packing."""
    from fvp import cnn

    f = C.compile_tail(*(m.to(dev) for m in C.modules_tail(c)))
    for mine, theirs in ((f.tail[1], d["f"].tail[1]), (f.out, d["f"].out)):
        mine.scale.copy_(theirs.scale)
        mine.shift.copy_(theirs.shift)
    xa = cnn.to_nhwc(torch.from_numpy(d["x"]).to(dev), c.Cpi)
    sa = cnn.to_nhwc(torch.from_numpy(d["skip"]).to(dev), f.tail[1].Cpo)
    two = f._head_nchw(f.encdec.parts["decoder_upsample1"](xa, res_post=sa))
    torch.cuda.synchronize()
    return two.double().cpu().numpy()


@pytest.mark.parametrize("cpi", [16, 48, 64, 80, 128])
def test_up2_head_nchw_vs_float64(gpu_device, cpi):
    """fvp_up2_head_nchw at 1, 3, 4, 5 and 8 K steps x Cs in {1, 20, 29, 32}, against the
    two-stage bound; the two-launch path meets the same bound (its head's fma chain is no
    longer than 32), so the two differ by at most both bounds."""
    worst, worst2, bad = 0.0, 0.0, []
    cases = [c for c in C.cases_tail() if c.Cpi == cpi]
    assert len(cases) == 4
    for c in cases:
        d, what = C.data_tail(c), C.id_tail(c)
        got = _launch_tail(gpu_device, c, d, _params_tail(gpu_device, d), 1, what, bad).double().cpu().numpy()
        worst = max(worst, _bound(got, d["ref"], d["tol"], what, bad))
        two = _two_launches(gpu_device, c, d)
        worst2 = max(worst2, _bound(two, d["ref"], d["tol"], what + " (two launches)", bad))
        if not (np.abs(got - two) <= 2 * d["tol"]).all():
            bad.append(f"{what}: one launch and two launches differ by more than both bounds")
    print(f"up2_head_nchw Cpi {cpi} ({cpi // 16} K steps): largest err / tol {worst:.4f} (two launches {worst2:.4f})")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("which", [0, 1], ids=["Cpi16", "Cpi80"])
def test_up2_head_nchw_persistent_walk(gpu_device, which):
    """At most CUs x (threads per CU / 256) blocks are resident: with more than twice that many
    items every block walks at least two (the register prefetch one item ahead, barrier B1
    guarding the z staging) -- one K step with clamped loads, and weights loaded per item."""
    c = C.walk_bases_tail()[which]
    d = C.data_tail(c)
    props = torch.cuda.get_device_properties(gpu_device)
    slots = props.multi_processor_count * (props.max_threads_per_multi_processor // 256)
    per = c.N * c.H * (c.W // 32)
    reps = 2 * slots // per + 1
    assert 2 * slots < reps * per < 3 * slots
    bad, params = [], _params_tail(gpu_device, d)
    small = _launch_tail(gpu_device, c, d, params, 1, "small launch", bad)
    r = _bound(small.double().cpu().numpy(), d["ref"], d["tol"], "small launch", bad)
    big = _launch_tail(gpu_device, c, d, params, reps, "walk", bad)
    _same_bits(big, small, reps, f"tail {C.id_tail(c)} walk", bad)
    print(f"up2_head_nchw {C.id_tail(c)}: {reps * per} items on at most {slots} blocks, {reps} copies bit-equal to the "
          f"small launch (err / tol {r:.4f})")
    assert not bad, "\n".join(bad)
