"""The cases of tests/cnn_nonfinite.py, checked on the CPU before any kernel sees them: each
one is non-trivial (the poisoned element reaches some outputs and leaves others alone), the
float64 reference's NaN set is exactly the geometric window the GPU tests hold the kernels to,
and the allowance the Winograd kernels get is bounded."""
import numpy as np
import pytest
import torch

import cnn_nonfinite as cn

POS = ("corner", "last", "seam")


def _real(mask2d, cout):
    """[Ho][Wo] -> [cout][Ho][Wo]"""
    return np.broadcast_to(mask2d, (cout,) + mask2d.shape)


@pytest.mark.parametrize("name", sorted(cn.LAYERS))
def test_layer_reference_nan_set_is_the_window(name):
    c = cn.LAYERS[name]
    clean = cn.layer_reference(name, None, None)
    assert tuple(clean.shape) == (c.n, c.cout) + c.out_hw and bool(torch.isfinite(clean).all())
    for pos in c.positions():
        win = c.window(pos)
        assert win.shape == c.out_hw
        ref = cn.layer_reference(name, pos, "nan")
        nan = torch.isnan(ref).numpy()
        print(f"{name} {pos} {c.where(pos)}: {int(win.sum())} of {win.size} outputs in the window")
        assert np.array_equal(nan[cn.POISONED], _real(win, c.cout)), (name, pos)
        assert 0 < win.sum() < win.size                         # NaN and finite outputs in the poisoned image
        others = np.delete(ref.numpy(), cn.POISONED, axis=0)
        assert np.isfinite(others).all() and not np.isinf(ref.numpy()).any()
        # +Inf: the same window at most (ReLU sends -Inf to 0), no NaN, every other value the clean run's
        inf = cn.layer_reference(name, pos, "inf").numpy()
        bad = ~np.isfinite(inf)
        assert not np.isnan(inf).any() and bad[cn.POISONED].any()
        assert not (bad[cn.POISONED] & ~_real(win, c.cout)).any()
        assert np.isfinite(np.delete(inf, cn.POISONED, axis=0)).all()
        out = np.ones(inf.shape, bool)
        out[cn.POISONED] = ~_real(win, c.cout)
        assert np.array_equal(inf[out], clean.numpy()[out]) and np.array_equal(ref.numpy()[out], clean.numpy()[out])


@pytest.mark.parametrize("which", ["input", "skip"])
def test_tail_reference_nan_set_is_the_window(which):
    s = cn.TAIL_SHAPE
    clean = cn.tail_reference(None, None, None)
    assert bool(torch.isfinite(clean).all())
    for pos in POS:
        win = cn.tail_window(which, pos)
        ref = cn.tail_reference(which, pos, "nan").numpy()
        assert win.sum() == (4 if which == "input" else 1)
        assert np.array_equal(np.isnan(ref)[cn.POISONED], _real(win, s["j"]))
        assert np.isfinite(np.delete(ref, cn.POISONED, axis=0)).all()
        inf = cn.tail_reference(which, pos, "inf").numpy()
        bad = ~np.isfinite(inf)
        assert bad[cn.POISONED].any() and not (bad[cn.POISONED] & ~_real(win, s["j"])).any()
        assert np.isfinite(np.delete(inf, cn.POISONED, axis=0)).all()


@pytest.mark.parametrize("name", ["conv_k3", "splitk", "deconv4"])
def test_winograd_tile_masks_bound_the_allowance(name):
    """The tile mask holds the window mask and at most 4x as many outputs: the Winograd
    allowance cannot hide a leak past the tiles that read the element."""
    c = cn.LAYERS[name]
    for pos in c.positions():
        p = c.positions()[pos]
        tile = cn.wino_deconv_tile_mask(c.hw, p) if c.transposed else cn.wino_tile_mask(c.hw, p)
        win = c.window(pos)
        print(f"{name} {pos}: window {int(win.sum())}, tiles {int(tile.sum())}")
        assert tile.shape == win.shape and not (win & ~tile).any()
        assert tile.sum() <= 4 * win.sum()
        assert tile.sum() < tile.size


def test_winograd_tile_masks_match_a_transform_of_the_patch():
    """The masks against their definition: F(2x2, 3x3) computes a tile's outputs from
    B^T d B of its 4 x 4 patch, the deconvolution's F(2x2, 2x2) from its 3 x 3 patch per parity --
    an element is in a tile's mask iff it lies in that patch (zero padding outside the image)."""
    H, W = 5, 7
    for py in range(H):
        for px in range(W):
            want = np.zeros((H, W), bool)
            for ty in range((H + 1) // 2):
                for tx in range((W + 1) // 2):
                    if 2 * ty - 1 <= py <= 2 * ty + 2 and 2 * tx - 1 <= px <= 2 * tx + 2:
                        want[2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = True
            assert np.array_equal(cn.wino_tile_mask((H, W), (py, px)), want)
            want = np.zeros((2 * H, 2 * W), bool)
            for ry in range(2):
                for rx in range(2):
                    for ty in range((H + 1) // 2):
                        for tx in range((W + 1) // 2):
                            y0, x0 = 2 * ty - 1 + ry, 2 * tx - 1 + rx
                            if y0 <= py <= y0 + 2 and x0 <= px <= x0 + 2:
                                for dy in range(2):
                                    for dx in range(2):
                                        oy, ox = 2 * (2 * ty + dy) + ry, 2 * (2 * tx + dx) + rx
                                        if oy < 2 * H and ox < 2 * W:
                                            want[oy, ox] = True
            assert np.array_equal(cn.wino_deconv_tile_mask((H, W), (py, px)), want)


@pytest.mark.parametrize("name", sorted(n for n, c in cn.NETS.items() if not c.bf16 or c.kind == "resnet18"))
def test_net_reference_is_non_trivial(name):
    c = cn.NETS[name]
    clean, ref = cn.net_reference(name, False), cn.net_reference(name, True)
    for y0, y in zip(clean, ref):
        assert bool(torch.isfinite(y0).all()) and not bool(torch.isinf(y).any())
        nan = torch.isnan(y)
        frac = float(nan[cn.POISONED].float().mean())
        print(f"{name}: {100 * frac:.1f} % of image {cn.POISONED}'s {tuple(y.shape[1:])} output is NaN")
        if c.full:
            assert frac == 1.0
        else:
            assert 0.0 < frac < 1.0
        others = [i for i in range(y.shape[0]) if i != cn.POISONED]
        assert others and not bool(nan[others].any())            # an image with no NaN anywhere
        assert torch.equal(y[others], y0[others])


def test_split_k_case_reserves_scratch():
    """The split-K case's plan on the per-tap kernel asks for scratch, so conv_splitk_reduce (not
    the GEMM's epilogue) applies its ReLU -- from the host-side planner, on any device count."""
    from fvp import _lib

    c = cn.LAYERS["splitk"]
    nbytes = _lib.load().fvp_conv2d_ex_workspace_bytes(c.n, c.hw[0], c.hw[1], c.cin, c.k, c.k, c.cout,
                                                        0, 1, 1, c.padding, c.padding, 1)
    assert nbytes > 0
