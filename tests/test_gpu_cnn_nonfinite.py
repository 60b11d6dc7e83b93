"""Non-finite activations through the convolution family (csrc/fvp_conv.hip, fvp_wino.hip,
fvp_c2c.hip) against the float64 CPU reference of tests/cnn_nonfinite.py: one NaN or +Inf
element in image 1 of N, every kernel run once clean and once poisoned.

(a) class parity   isnan / == +inf / == -inf on the real channels equal the reference's
                   (torch.relu keeps NaN: a kernel whose ReLU is fmaxf(v, 0) returns 0 instead).
(b) finite values  where the reference is finite the error is within the project's bar, REL = 2e-5
                   of the largest finite reference value (2e-2 with bf16 operands), tests/test_cnn.py.
(c) isolation      outside the element's geometric window, and in every other image, the poisoned
                   run is bit-equal to the clean run of the same kernel (stale LDS, tile-edge
                   over-reads and leaks across images change bits a tolerance cannot see).
(d) Winograd       transforms whole input patches: NaN wherever the reference is NaN; finite and
                   bit-equal to the clean run outside the tiles whose patch holds the element;
                   inside those tiles and outside the window either outcome passes.  With +Inf the
                   transforms' differences may turn an Inf into NaN (Inf - Inf), never into a
                   finite value or the other sign: inside the window NaN or the reference's class.

Each test prints what it measured before it asserts (pytest -s).  Single layers compare real
channels only: a padded output channel may hold NaN where an Inf met its zero weight.

What these cases caught when they were written: every ReLU of the family was fmaxf(v, 0) (no NaN
in any output: 54 of the 92 cases failed); conv_front7_bf16_kernel's zero 50th tap read the
window's first pixel (Inf x 0 = NaN at output (y + 3, x + 3), hidden by that fmaxf); and
conv_stem7_bf16_kernel's zero eighth tap read input column 2 ox + 4, one past the window (192
NaNs outside it for a pixel in an even column -- why the stem cases poison both column parities).
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_nonfinite as cn

pytestmark = pytest.mark.gpu

POS = ("corner", "last", "seam")
VALS = ("nan", "inf")


# ------------------------------------------------------------------------------------- checks
def _bits(t):
    return t.contiguous().view(torch.int32)


def _full(mask2d, shape):
    """[Ho][Wo] window of image POISONED -> bool [n][c][Ho][Wo]"""
    m = torch.zeros(shape, dtype=torch.bool)
    m[cn.POISONED] = torch.from_numpy(np.ascontiguousarray(mask2d))
    return m


def _finite_err(got, ref):
    fin = torch.isfinite(ref) & torch.isfinite(got)
    scale = max(float(ref[torch.isfinite(ref)].abs().max()), 1e-6)
    return float((got.double() - ref)[fin].abs().max()) / scale if bool(fin.any()) else 0.0


def _check(what, got, clean, ref, window, rel, tiles=None, superset=False):
    """got / clean: fp32 CPU outputs of the poisoned / clean run; ref: float64; window: bool, the
    outputs the element may reach (None: whole networks, image POISONED).  tiles: the Winograd
    allowance (assertion (d)); superset: a network with Winograd layers, NaN set >= the reference's.
    -> list of failures (empty: passed)."""
    got, clean = got.detach().float().cpu(), clean.detach().float().cpu()
    assert got.shape == ref.shape == clean.shape, (what, got.shape, ref.shape, clean.shape)
    if window is None:
        window = torch.zeros(ref.shape, dtype=torch.bool)
        window[cn.POISONED] = True
    fails = []
    gn, gp, gm = cn.classes(got)
    rn, rp, rm = cn.classes(ref)
    err = _finite_err(got, ref)
    leak = int((_bits(got) != _bits(clean))[~(window if tiles is None else tiles)].sum())
    print(f"{what}: NaN {int(gn.sum())} (reference {int(rn.sum())}), +Inf {int(gp.sum())} ({int(rp.sum())}), "
          f"-Inf {int(gm.sum())} ({int(rm.sum())}), window {int(window.sum())}"
          + (f", tiles {int(tiles.sum())}" if tiles is not None else "")
          + f"; finite error {err:.3g} (bar {rel}); {leak} values outside differ from the clean run")
    if not bool(torch.isfinite(clean).all()):
        fails.append(f"{what}: the clean run is not finite")
    if tiles is None and not superset:
        for name, g, r in (("NaN", gn, rn), ("+Inf", gp, rp), ("-Inf", gm, rm)):  # (a)
            if not torch.equal(g, r):
                fails.append(f"{what}: {name} at {int(g.sum())} outputs, the reference at {int(r.sum())} "
                             f"({int((g & ~r).sum())} extra, {int((r & ~g).sum())} missing)")
    else:  # (d)
        if bool((rn & ~gn).any()):
            fails.append(f"{what}: {int((rn & ~gn).sum())} of the reference's {int(rn.sum())} NaNs are missing")
        same = (gn == rn) & (gp == rp) & (gm == rm)
        if bool((window & ~gn & ~same).any()):
            fails.append(f"{what}: {int((window & ~gn & ~same).sum())} outputs in the window are neither NaN "
                         "nor of the reference's class")
        if tiles is not None and not bool(torch.isfinite(got[~tiles]).all()):
            fails.append(f"{what}: non-finite outputs outside the tile mask")
        if tiles is not None:  # in a tile, outside the window: non-finite, or the clean run's value
            odd = tiles & ~window & torch.isfinite(got) & (_bits(got) != _bits(clean))
            if bool(odd.any()):
                fails.append(f"{what}: {int(odd.sum())} finite outputs in the tiles differ from the clean run")
    if err > rel:  # (b)
        fails.append(f"{what}: finite error {err:.3g} of the output scale (> {rel})")
    if leak:  # (c)
        fails.append(f"{what}: {leak} outputs outside the {'tiles' if tiles is not None else 'window'} "
                     "differ from the clean run")
    return fails


def _on(module, dev):
    """A copy of a cached CPU module on the device."""
    return copy.deepcopy(module).to(dev)


def _kinds(layers):
    return [k for l in layers for _, k in l._ws.values()]


# ------------------------------------------------------------------------------ ConvLayer cases
def _conv_layer(name, dev, algo=None, dtype=torch.float32):
    from fvp import cnn

    c = cn.LAYERS[name]
    seq = _on(cn.layer_module(name), dev)  # (a copy: the float64 reference keeps the CPU module)
    return cnn.ConvLayer(seq[0], seq[1] if c.bn else None, dtype, algo=algo)


def _run_layer(c, layer, x, r, dev, pool=False):
    """-> (NCHW fp32 output on the device, the Act the layer returned)"""
    from fvp import cnn

    ra = cnn.to_nhwc(r.to(dev)) if r is not None else None
    y = layer(cnn.to_nhwc(x.to(dev), layer.Cpi), relu=c.relu, res_pre=ra if c.res == "pre" else None,
              res_post=ra if c.res == "post" else None, pool=pool)
    return cnn.to_nchw(y), y


def _layer_case(name, value, dev, algo=None, want_kind=None, tile_fn=None, pool=False, scratch=False):
    """One ConvLayer on the clean input and on every poisoned position: (a) (b) (c), or (d) with tile_fn."""
    c = cn.LAYERS[name]
    layer = _conv_layer(name, dev, algo)
    x, r = cn.layer_inputs(name)
    clean, _ = _run_layer(c, layer, x, r, dev, pool)
    if want_kind is not None:
        assert _kinds([layer]) == [want_kind], (name, layer._ws)
    if scratch:  # split-K scratch reserved: conv_splitk_reduce applies the ReLU
        assert [nws > 0 for nws, _ in layer._ws.values()] == [True], (name, layer._ws)
    fails = []
    for pos in c.positions():
        xp = cn.poison(x, c.where(pos), cn.VALUES[value])
        got, act = _run_layer(c, layer, xp, r, dev, pool)
        ref = cn.layer_reference(name, pos, value)
        tiles = _full(tile_fn(c.hw, c.positions()[pos]), ref.shape) if tile_fn else None
        fails += _check(f"{name} {value} {pos} algo {algo}", got, clean, ref, _full(c.window(pos), ref.shape),
                        c.rel, tiles)
        if pool:  # the fused 2 x 2 pool: max_pool2d of the output the same launch wrote, NaN included
            from fvp import cnn

            assert act.pooled is not None
            pooled, want = cnn.to_nchw(act.pooled), F.max_pool2d(got, 2, 2)
            print(f"  pooled: NaN {int(torch.isnan(pooled).sum())} (max_pool2d of the output "
                  f"{int(torch.isnan(want).sum())})")
            if not (torch.equal(torch.isnan(pooled), torch.isnan(want))
                    and torch.equal(torch.nan_to_num(pooled, 7.0), torch.nan_to_num(want, 7.0))):
                fails.append(f"{name} {value} {pos}: the fused pool is not max_pool2d of the output")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("value", VALS)
@pytest.mark.parametrize("name", ["conv_k3", "conv_k7", "conv_k1", "conv_k5"])
def test_conv_layer_nonfinite(gpu_device, conv_kernel, name, value):
    """16->32 k3 at 9 x 18 (+ residual; column 15 | 16 is the halo kernel's tile seam), 15->16 k7
    at 13 x 10, 32->15 k1 at 6 x 7, 40->70 k5 at 9 x 11 (+ residual) on the halo, per-tap,
    per-tap without split-K, LDS-DMA and Winograd choices."""
    from fvp import cnn

    wino = conv_kernel == cnn.CONV_WINO and name == "conv_k3"
    _layer_case(name, value, gpu_device, conv_kernel, want_kind="wino" if wino else None,
                tile_fn=cn.wino_tile_mask if wino else None, pool=wino)


@pytest.mark.parametrize("value", VALS)
def test_split_k_reduce_nonfinite(gpu_device, value):
    """128->128 k3 at 16 x 16 (+ residual) on the per-tap kernel with split-K: the ReLU is
    conv_splitk_reduce's."""
    from fvp import cnn

    _layer_case("splitk", value, gpu_device, cnn.CONV_PER_TAP, scratch=True)


@pytest.mark.parametrize("value", VALS)
def test_transposed_conv_nonfinite(gpu_device, value):
    """ConvTranspose2d(64, 32, 2, 2) at 5 x 7 with the skip added after the ReLU;
    ConvTranspose2d(48, 32, 4, 2, 1) at 5 x 7 as four parity GEMMs and as Winograd F(2x2, 2x2)."""
    from fvp import cnn

    _layer_case("deconv2", value, gpu_device)
    _layer_case("deconv4", value, gpu_device, cnn.CONV_PER_TAP, want_kind=False)
    _layer_case("deconv4", value, gpu_device, cnn.CONV_WINO, want_kind="wino_dc", tile_fn=cn.wino_deconv_tile_mask)


@pytest.mark.parametrize("value", VALS)
@pytest.mark.parametrize("name", ["s2_k3", "s2_k1"])
def test_strided_conv_nonfinite(gpu_device, conv_kernel, name, value):
    """3 x 3 stride 2 (32->64 at 11 x 9) and 1 x 1 stride 2 (64->32 at 9 x 7) + BN + ReLU."""
    _layer_case(name, value, gpu_device, conv_kernel)


@pytest.mark.parametrize("value", VALS)
def test_bf16_conv_nonfinite(gpu_device, value):
    """bf16 operands: 32->32 k3 at 9 x 18 from fp32 activations (the register-staged kernel), and
    64->64 k3 at 9 x 18 on bf16 activations by the LDS-DMA and the register-staged kernels, which
    must stay bit-equal to each other on the poisoned input too."""
    from fvp import cnn

    dev = gpu_device
    fails = []
    c = cn.LAYERS["bf16_32"]
    layer = _conv_layer("bf16_32", dev, None, torch.bfloat16)
    x, _ = cn.layer_inputs("bf16_32")
    clean, _ = _run_layer(c, layer, x, None, dev)
    for pos in c.positions():
        got, _ = _run_layer(c, layer, cn.poison(x, c.where(pos), cn.VALUES[value]), None, dev)
        ref = cn.layer_reference("bf16_32", pos, value)
        fails += _check(f"bf16_32 {value} {pos}", got, clean, ref, _full(c.window(pos), ref.shape), c.rel)

    c = cn.LAYERS["bf16_64"]
    x, _ = cn.layer_inputs("bf16_64")
    dma = _conv_layer("bf16_64", dev, None, torch.bfloat16)
    reg = _conv_layer("bf16_64", dev, cnn.CONV_PER_TAP_NOSPLIT, torch.bfloat16)
    dma.act_bf16 = reg.act_bf16 = True

    def run(layer, xin):
        xn = cnn.to_nhwc(xin.to(dev))
        y = layer(cnn.Act(xn.t.to(torch.bfloat16), xn.C), relu=True)
        assert y.t.dtype == torch.bfloat16
        return y.t

    cleans = {k: run(l, x) for k, l in (("dma", dma), ("reg", reg))}
    for pos in c.positions():
        xp = cn.poison(x, c.where(pos), cn.VALUES[value])
        ref = cn.layer_reference("bf16_64", pos, value)
        raw = {}
        for k, l in (("dma", dma), ("reg", reg)):
            raw[k] = run(l, xp)
            got = raw[k][..., :c.cout].float().permute(0, 3, 1, 2)
            fails += _check(f"bf16_64 {k} {value} {pos}", got, cleans[k][..., :c.cout].float().permute(0, 3, 1, 2),
                            ref, _full(c.window(pos), ref.shape), c.rel)
        diff = int((raw["dma"][..., :c.cout].contiguous().view(torch.int16)
                    != raw["reg"][..., :c.cout].contiguous().view(torch.int16)).sum())
        print(f"  bf16_64 {value} {pos}: {diff} values differ in bits between the DMA and the register-staged kernel")
        if diff:
            fails.append(f"bf16_64 {value} {pos}: DMA and register-staged outputs differ in {diff} values")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("value", VALS)
@pytest.mark.parametrize("name", ["stem7", "stem7_bf16"])
def test_stem7_nonfinite(gpu_device, name, value):
    """fvp_conv_stem7_f32 / _bf16 (7x7 / s2 / p3 -> 64 + BN + ReLU from NCHW images) at
    2 x 3 x 37 x 70: exact class parity -- an Inf pixel reaches no output outside the windows that
    hold it (the padded K row reads no image data)."""
    from fvp.backbone import FvpPoseResNet

    c = cn.LAYERS[name]
    m = _on(cn.source_net(c.source, c.seed), gpu_device)
    bb = FvpPoseResNet(m, torch.bfloat16 if c.bf16 else torch.float32)
    stem = bb._stem7 if c.bf16 else bb._stem7_f32
    assert (bb.stem7 if c.bf16 else bb.stem7_f32) is not None
    x, _ = cn.layer_inputs(name)
    clean = stem(x.to(gpu_device)).t.float().permute(0, 3, 1, 2)
    fails = []
    for pos in c.positions():
        got = stem(cn.poison(x, c.where(pos), cn.VALUES[value]).to(gpu_device)).t.float().permute(0, 3, 1, 2)
        ref = cn.layer_reference(name, pos, value)
        fails += _check(f"{name} {value} {pos}", got, clean, ref, _full(c.window(pos), ref.shape), c.rel)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("value", VALS)
@pytest.mark.parametrize("name", ["front7", "front7_bf16"])
def test_front7_nonfinite(gpu_device, name, value):
    """fvp_conv_front7_f32 / _bf16 (Basic2DBlock(15, 16, 7) from the NCHW maps) at 2 x 15 x 13 x 20."""
    from fvp import _lib, cnn
    from fvp.ops import _ptr, _stream

    c = cn.LAYERS[name]
    m = _on(cn.source_net(c.source, c.seed), gpu_device)
    f = cnn.FvpCNN(m, torch.bfloat16 if c.bf16 else torch.float32)
    fn, wp, conv = f.front7
    assert fn == ("fvp_conv_front7_bf16" if c.bf16 else "fvp_conv_front7_f32")

    def run(xin):
        xin = xin.to(gpu_device).contiguous()
        out = torch.empty((c.n,) + c.hw + (16,), dtype=torch.bfloat16 if c.bf16 else torch.float32,
                          device=gpu_device)
        _lib.call(fn, _ptr(xin), c.n, c.cin, c.hw[0], c.hw[1], _ptr(wp), _ptr(conv.scale), _ptr(conv.shift),
                  _ptr(out), _stream(out))
        return out.float().permute(0, 3, 1, 2)

    x, _ = cn.layer_inputs(name)
    clean = run(x)
    fails = []
    for pos in c.positions():
        got = run(cn.poison(x, c.where(pos), cn.VALUES[value]))
        ref = cn.layer_reference(name, pos, value)
        fails += _check(f"{name} {value} {pos}", got, clean, ref, _full(c.window(pos), ref.shape), c.rel)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("value", VALS)
def test_head_1x1_nchw_nonfinite(gpu_device, value):
    """fvp_conv1x1_nchw 32->15 at 6 x 7 as FvpCNN._head_nchw calls it (no ReLU) and with its ReLU,
    and the GEMM + layout-pass path: class parity on all of them."""
    from fvp import _lib, cnn
    from fvp.ops import _ptr, _stream

    dev = gpu_device
    c = cn.LAYERS["head1x1"]
    layer = _conv_layer("head1x1", dev)
    f = cnn.FvpCNN.__new__(cnn.FvpCNN)
    f.out = layer

    def relu_head(a):  # the kernel's ReLU path (cnn._conv1x1_nchw passes relu = 0)
        out = torch.empty((a.N, layer.Cout, a.H, a.W), device=dev)
        _lib.call("fvp_conv1x1_nchw", _ptr(a.t), a.N, a.H, a.W, a.Cp, layer.Cin, _ptr(layer.wpack), layer.Cpo_w,
                  layer.Cout, _ptr(layer.scale), _ptr(layer.shift), 1, _ptr(out), _stream(out))
        return out

    paths = {"head": ("head1x1", lambda a: f._conv1x1_nchw(a, 0, layer)),
             "head + ReLU": ("head1x1_relu", relu_head),
             "GEMM + layout": ("head1x1", lambda a: cnn.to_nchw(layer(a, relu=False)))}
    x, _ = cn.layer_inputs("head1x1")
    fails = []
    for what, (name, run) in paths.items():
        clean = run(cnn.to_nhwc(x.to(dev), layer.Cpi))
        assert clean is not None
        for pos in POS:
            got = run(cnn.to_nhwc(cn.poison(x, c.where(pos), cn.VALUES[value]).to(dev), layer.Cpi))
            ref = cn.layer_reference(name, pos, value)
            fails += _check(f"{what} {value} {pos}", got, clean, ref, _full(c.window(pos), ref.shape), c.rel)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("value", VALS)
@pytest.mark.parametrize("which", ["input", "skip"])
def test_p2p_tail_nonfinite(gpu_device, which, value):
    """fvp_up2_head_nchw (FvpCNN._tail_nchw) 48->20->16 with the skip, the element in the input or
    in the skip, and the two-launch path (the deconvolution GEMM, then fvp_conv1x1_nchw)."""
    import types

    from fvp import cnn

    dev = gpu_device
    up, head = (_on(m, dev) for m in cn.tail_modules())
    f = cnn.FvpCNN.__new__(cnn.FvpCNN)
    f.module = types.SimpleNamespace(encoder_decoder=types.SimpleNamespace(decoder_upsample1=up),
                                     output_layer=head)
    f.encdec = types.SimpleNamespace(parts={"decoder_upsample1": cnn._Plan(up)})
    f.out = cnn.ConvLayer(head, None)
    f.tail = f._compile_tail()
    assert f.tail is not None
    cpi = f.tail[1].Cpi

    def one(x, skip):
        y = f._tail_nchw(cnn.to_nhwc(x.to(dev), cpi), cnn.to_nhwc(skip.to(dev), 32))
        assert y is not None, "fvp_up2_head_nchw was not taken"
        return y

    def two(x, skip):
        return f._head_nchw(f.encdec.parts["decoder_upsample1"](cnn.to_nhwc(x.to(dev), cpi),
                                                                res_post=cnn.to_nhwc(skip.to(dev), 32)))

    fails = []
    for what, run in (("one launch", one), ("two launches", two)):
        clean = run(*cn.tail_inputs())
        for pos in POS:
            got = run(*cn.tail_poisoned(which, pos, value))
            ref = cn.tail_reference(which, pos, value)
            fails += _check(f"tail {what}, {which} {value} {pos}", got, clean, ref,
                            _full(cn.tail_window(which, pos), ref.shape), cn.REL_F32)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------- whole networks
def _net_check(what, name, outs, cleans, superset):
    c = cn.NETS[name]
    refs = cn.net_reference(name, True)
    assert len(outs) == len(refs)
    fails = []
    for i, (got, clean, ref) in enumerate(zip(outs, cleans, refs)):
        fails += _check(f"{what} output {i}", got, clean, ref, None, c.rel, superset=superset)
    return fails


@pytest.mark.parametrize("algo", ["pertap", "halo", "dma", "auto"])
def test_p2pnet_nan_pixel(gpu_device, algo):
    """P2PNet on 2 x 15 x 64 x 64, NaN at (1, 3, 5, 6): the reference's NaN set covers about 47 %
    of image 1 and none of image 0.  A choice that runs a layer on Winograd may widen it."""
    from fvp import cnn

    a = {"pertap": cnn.CONV_PER_TAP, "halo": cnn.CONV_HALO, "dma": cnn.CONV_DMA, "auto": None}[algo]
    m = _on(cn.net_module("p2p", cn.NETS["p2p"].seed), gpu_device)
    net = cnn.FvpCNN(m, algo=a)
    clean = net(cn.net_input("p2p", False).to(gpu_device))
    got = net(cn.net_input("p2p", True).to(gpu_device))
    wino = any(k in ("wino", "wino_dc") for k in _kinds(net.front.layers() + net.encdec.layers() + [net.out]))
    print(f"P2PNet {algo}: Winograd layers {wino}")
    fails = _net_check(f"P2PNet {algo}", "p2p", (got,), (clean,), wino)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("merged", [True, False])
def test_centernet_nan_pixel(gpu_device, merged):
    """CenterNet.from_xy on 2 x 15 x 40 x 40, both outputs, the heads merged and separate."""
    from fvp import cnn

    m = _on(cn.net_module("centernet", cn.NETS["centernet"].seed), gpu_device)
    net = cnn.FvpCNN(m)
    assert net.heads is not None
    if not merged:
        net.heads = None
    clean = net.from_xy(cn.net_input("centernet", False).to(gpu_device))
    got = net.from_xy(cn.net_input("centernet", True).to(gpu_device))
    fails = _net_check(f"CenterNet merged {merged}", "centernet", got, clean, True)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", ["c2c_20_end", "c2c_20_mid", "c2c_64_end", "c2c_64_mid"])
def test_c2cnet_nan_element(gpu_device, name):
    """C2CNet on 3 columns of length 20 and 64 (the latter on 8,192-float weight chunks), NaN at a
    column end and mid-column, through the one-launch net -- every layer's rows of a column in one
    LDS block -- and per layer."""
    from fvp import cnn

    c = cn.NETS[name]
    L = c.shape[2]
    m = _on(cn.net_module("c2c", c.seed), gpu_device)
    x, xp = cn.net_input(name, False).to(gpu_device), cn.net_input(name, True).to(gpu_device)
    net = cnn.FvpCNN(m)
    clean, got = net(x), net(xp)
    n1 = net.net1d[(15, L)]
    assert n1 is not None, "the one-launch path was not taken"
    assert n1.wchunk == (8192 if L == 64 else 12288)
    fails = _net_check(f"C2CNet one launch {name}", name, (got,), (clean,), False)
    per = cnn.FvpCNN(m, algo=cnn.CONV_PER_TAP)
    fails += _net_check(f"C2CNet per layer {name}", name, (per(xp),), (per(x),), False)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", ["resnet18", "resnet18_bf16"])
def test_pose_resnet_nan_pixel(gpu_device, name):
    """PoseResNet-18 on 2 x 3 x 64 x 96, NaN at (1, 0, 3, 3): image 1 is NaN everywhere, image 0
    is the clean run's."""
    from fvp.backbone import FvpPoseResNet

    c = cn.NETS[name]
    m = _on(cn.net_module(c.kind, c.seed), gpu_device)
    bb = FvpPoseResNet(m, torch.bfloat16 if c.bf16 else torch.float32)
    clean = bb(cn.net_input(name, False).to(gpu_device))
    got = bb(cn.net_input(name, True).to(gpu_device))
    fails = _net_check(f"PoseResNet-18 {name}", name, (got,), (clean,), True)
    assert not fails, "\n".join(fails)
