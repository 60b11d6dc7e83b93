"""fvp_conv2d_ex_plan (the decision conv_launch switches on, csrc/fvp_conv.hip conv_route)
against the independent model of tests/conv_route_model.py -- no GPU.  The sweep takes every
algo, every bf16 flag combination (the illegal ones too), modes 0-3, strides 1-4 and shapes
on both sides of every threshold of the rules; the last tests assert that it did, so a
sweep that stops reaching a threshold fails instead of passing on less."""
import ctypes
import functools
import itertools

import pytest

import conv_route_model as M

ALGOS = (0, 1, 2, 3)
FLAGS = (0, 8, 1, 3, 5, 7)           # fp32, fp32 LDS-DMA, bf16 x (in, out)
BAD_FLAGS = (2, 4, 6, 9, 11, 16)     # in / out without operands, DMA with bf16, an unknown bit
SEEN = set()                         # threshold sides the sweeps reached (test_sweep_reached_...)


def _lib():
    from fvp import _lib

    return _lib.load()


def _check(lib, args, algo, flags, ws):
    """One comparison; returns the model's (status, plan)."""
    plan = (ctypes.c_int * 8)(*([-1] * 8))
    st = lib.fvp_conv2d_ex_plan(*args, flags, algo, ws, plan)
    want = M.route(*args, flags, algo, ws)
    got = (st, tuple(plan) if st == 0 else None)
    assert got == want, f"(N H W Cpi KH KW Cpo mode sy sx py px) {args} flags {flags} algo {algo} ws {ws}: " \
                        f"library {got}, model {want}"
    return want


def _note(args, algo, flags, plan):
    """Record which side of which threshold this case sits on."""
    N, H, W, Cpi, KH, KW, Cpo, mode, sy, sx, py, px = args
    _, g = M.geom(H, W, Cpi, KH, KW, mode, sy, sx, py, px)
    Ntot, G = (1, 4, 2, 1)[mode] * Cpo, 4 if mode == 3 else 1
    Mr = N * g["Hm"] * g["Wm"]
    cls = 16 if Ntot <= 16 else 32 if Ntot <= 32 else 64
    SEEN.add(("Ntot", Ntot))
    SEEN.add(("family", plan[0], plan[1], plan[2], plan[3], plan[4], plan[5] > 1))
    if flags & 1:
        SEEN.add(("b128", G * M.cdiv(Mr, 128) * M.cdiv(Ntot, 64)))
        SEEN.add(("bf16 Cpi % 64", Cpi % 64, plan[0]))
    if flags == 0:
        big = {16: 1, 32: 3, 64: 5}[cls]
        if plan[0] == 1:
            SEEN.add(("per-tap big", cls, G * M.cdiv(Mr, M.TILE_BM[big]) * M.cdiv(Ntot, M.TILE_BN[big])))
            nchunks = M.cdiv(KH * KW * Cpi, 16)
            nb = plan[7] // plan[5]
            if algo != 3 and g["Hm"] > 1:
                if nchunks >= 8:
                    SEEN.add(("nb", nb))
                if nb < 256:
                    SEEN.add(("nchunks", nchunks, plan[5] > 1))
            SEEN.add(("Cpi % 32", cls, Cpi % 32 == 0, plan[3]))
        same = mode == 0 and (sy, sx) == (1, 1) and 2 * py == KH - 1 and 2 * px == KW - 1 and KH * KW > 1
        if same and algo in (0, 2) and Cpi % 16 == 0 and KH <= 7 and KW <= 7:
            SEEN.add(("halo W", W, plan[0] == 2))
            if plan[0] == 2 or W >= 16 and (M.cdiv(W, 16) * 16 - W) * 8 <= W:
                SEEN.add(("halo big", cls, N * M.cdiv(W, 16) * M.cdiv(H, M.TILE_BM[big] // 16)
                          * M.cdiv(Ntot, M.TILE_BN[big])))
                if cls == 64 and algo == 2:
                    SEEN.add(("halo mid", N * M.cdiv(W, 16) * M.cdiv(H, 4) * M.cdiv(Ntot, 64)))


def _sweep(shapes):
    """Every algo x flag x workspace (the model's size, one byte less, none) of every shape."""
    lib = _lib()
    n = 0
    for args in shapes:
        for algo, flags in itertools.product(ALGOS, FLAGS):
            need = M.workspace_bytes(*args, algo) if flags == 0 else 0
            if flags == 0:
                assert lib.fvp_conv2d_ex_workspace_bytes(*args, algo) == need, (args, algo)
            for ws in ((need, need - 1, 0) if need else (0,)):
                st, plan = _check(lib, args, algo, flags, ws)
                n += 1
                if st == 0:
                    assert plan[5] == 1 or ws == need
                    _note(args, algo, flags, plan)
    return n


def _same(N, H, W, Cpi, KH, KW, Cpo):
    return (N, H, W, Cpi, KH, KW, Cpo, 0, 1, 1, KH // 2, KW // 2)


@functools.lru_cache(maxsize=None)
def _sweep_blocks():
    shapes = [_same(N, H, W, Cpi, K, K, Cpo)
              for H, W in ((4, 8), (8, 8), (8, 16), (16, 16), (1, 64), (2, 16), (4, 16))
              for N in (63, 64, 127, 128, 129, 255, 256, 257, 510, 511, 512, 513, 1022, 1023, 1024)
              for Cpi in (4, 12, 16, 32, 48, 64, 128)
              for K in (1, 3)
              for Cpo in (16, 32, 48, 64, 80, 128)]
    return _sweep(shapes)


@functools.lru_cache(maxsize=None)
def _sweep_halo():
    shapes = [_same(N, H, W, Cpi, KH, KW, Cpo)
              for W in list(range(13, 42)) + [63, 64, 65, 112, 113, 127, 128, 129]
              for H in (1, 5, 8, 9, 17)
              for N in (1, 2, 33, 65)
              for KH, KW in ((3, 3), (5, 5), (7, 7), (1, 5), (5, 1), (3, 7), (9, 9), (1, 1))
              for Cpi, Cpo in ((16, 16), (16, 32), (32, 64), (16, 128), (8, 16))]
    return _sweep(shapes)


@functools.lru_cache(maxsize=None)
def _sweep_modes():
    shapes = []
    for N, H, W in ((1, 5, 5), (2, 5, 5), (9, 20, 20), (2, 7, 33), (40, 1, 40), (3, 64, 48), (130, 16, 16)):
        for Cpi in (4, 8, 12, 16, 32, 64, 112, 128):
            for Cpo in (16, 32, 48, 64, 80, 144):
                for K in (1, 2, 3, 4, 5, 7):
                    for sy, sx in ((1, 1), (2, 2), (1, 3), (4, 2), (3, 4)):
                        for p in sorted({0, K // 2, K - 1}):
                            shapes.append((N, H, W, Cpi, K, K, Cpo, 0, sy, sx, p, p))
                shapes.append((N, H, W, Cpi, 1, 7, Cpo, 0, 1, 1, 0, 3))
                shapes.append((N, H, W, Cpi, 7, 1, Cpo, 0, 2, 1, 3, 0))
                for mode, K in ((1, 1), (2, 1), (3, 2)):
                    shapes.append((N, H, W, Cpi, K, K, Cpo, mode, 0, 0, 0, 0))
    return _sweep(shapes)


def test_block_count_thresholds():
    """255 / 256 and 511 / 512 blocks of every tile: maps of 32 .. 256 pixels x the batch."""
    assert _sweep_blocks() > 100000


def test_halo_width_rule_and_kernel_sizes():
    """W around the halo tile's 1/8-waste rule and its 16-pixel minimum, kernels up to 7 (and 9),
    non-square ones, odd heights."""
    assert _sweep_halo() > 50000


def test_modes_strides_paddings_and_chunk_counts():
    """Modes 0-3, strides 1-4 with padding 0 .. K - 1, 4 .. 128 input channels (7 / 8 K chunks:
    112 / 128 channels at 1x1, 1x7 at 16), Ntot 16 / 32 / 64 and one past each through the
    transposed modes' column multipliers."""
    assert _sweep_modes() > 100000


def _swept():
    """SEEN after all three sweeps (each runs once per process)."""
    _sweep_blocks(), _sweep_halo(), _sweep_modes()
    return SEEN


def test_statuses_of_illegal_arguments():
    """Every rejection of fvp_conv2d_nhwc_ex that needs no pointer: flags, algo, channel
    pitches, geometry, the LDS-DMA kernel's limits (more than 32 taps, 2^24 rows)."""
    lib = _lib()
    ok = (2, 8, 8, 32, 3, 3, 32, 0, 1, 1, 1, 1)
    for flags in BAD_FLAGS:
        assert _check(lib, ok, 0, flags, 0)[0] == M.ERR_SHAPE
    for algo in (-1, 4, 5):
        assert _check(lib, ok, algo, 0, 0)[0] == M.ERR_SHAPE
    for i, v in ((0, 0), (3, 20), (3, 6), (6, 20), (6, 0), (7, 4), (8, 5), (10, 3), (1, 0), (4, 0)):
        bad = list(ok)
        bad[i] = v
        for flags in FLAGS:
            assert _check(lib, tuple(bad), 0, flags, 0)[0] == M.ERR_SHAPE, (i, v, flags)
    assert _check(lib, (2, 8, 8, 32, 3, 3, 32, 1, 0, 0, 0, 0), 0, 0, 0)[0] == M.ERR_SHAPE  # mode 1: 1x1 only
    assert _check(lib, (2, 8, 8, 32, 3, 3, 32, 3, 0, 0, 0, 0), 0, 0, 0)[0] == M.ERR_SHAPE  # mode 3: 2x2 taps
    assert _check(lib, (2, 2, 2, 16, 7, 7, 16, 0, 1, 1, 0, 0), 0, 0, 0)[0] == M.ERR_SHAPE  # kernel > input
    assert _check(lib, (2, 8, 8, 8, 3, 3, 32, 0, 1, 1, 1, 1), 0, 3, 0)[0] == M.ERR_SHAPE   # bf16 input, 8 channels
    assert _check(lib, (2, 8, 8, 8, 3, 3, 32, 0, 1, 1, 1, 1), 0, 8, 0)[0] == M.ERR_SHAPE   # DMA, 8 channels
    for flags, fam in ((8, None), (3, 3), (1, 3), (0, 1)):  # 49 taps: not the DMA kernel's
        st, plan = _check(lib, (2, 16, 16, 32, 7, 7, 32, 0, 1, 1, 3, 3), 0, flags, 0)
        assert (plan and plan[0]) == fam
    for flags, fam in ((8, None), (3, 3)):                   # 2^24 GEMM rows likewise; one fewer fits
        assert (_check(lib, (4096, 64, 64, 32, 1, 1, 32, 0, 1, 1, 0, 0), 0, flags, 0)[1] or (None,))[0] == fam
        assert _check(lib, (4095, 64, 64, 32, 1, 1, 32, 0, 1, 1, 0, 0), 0, flags, 0)[1][0] == 4
    assert lib.fvp_conv2d_ex_plan(*ok, 0, 0, 0, None) == 1001
    # the 2^33-element limit of the output (and so of the block count: the INT_MAX clamp of slot 7
    # cannot be reached below it; the model applies it all the same)
    assert _check(lib, (8191, 256, 256, 4, 1, 1, 16, 0, 1, 1, 0, 0), 0, 0, 0)[0] == 0
    assert _check(lib, (8192, 256, 256, 4, 1, 1, 16, 0, 1, 1, 0, 0), 0, 0, 0)[0] == M.ERR_SHAPE


@pytest.mark.parametrize("what", [
    [("nb", 255), ("nb", 256)],                                           # split-K's block threshold
    [("nchunks", 7, False), ("nchunks", 8, True)],                        # and its K-walk threshold
    [("per-tap big", c, b) for c in (16, 32, 64) for b in (511, 512)],   # large / small per-tap tile
    [("halo big", c, b) for c in (16, 32, 64) for b in (511, 512)],      # large halo tile
    [("halo mid", 510), ("halo mid", 512)],                               # 64 x 64 / 32 x 64 under HALO (even counts)
    [("b128", 511), ("b128", 512)],                                       # bf16 128 x 64 / 64 x 64
    [("Ntot", n) for n in (16, 32, 48, 64, 80)],                          # 16 / 17, 32 / 33, 64 / 65 in units of 16
    [("Cpi % 32", 32, True, 32), ("Cpi % 32", 32, False, 16)],           # TileN32sK
    [("bf16 Cpi % 64", 0, 4), ("bf16 Cpi % 64", 32, 4)],                 # DMA 128-B / 64-B rows
    [("halo W", 15, False), ("halo W", 16, True), ("halo W", 28, False), ("halo W", 29, True),
     ("halo W", 112, True), ("halo W", 113, False)],                      # the 16-pixel minimum, the 1/8 waste rule
], ids=lambda w: str(w[0][0]))
def test_sweep_reached_both_sides(what):
    missing = [w for w in what if w not in _swept()]
    assert not missing, missing


def test_sweep_reached_every_instantiation():
    """Every (family, BM, BN, K depth, variant, split) the issue's variant list names was returned."""
    fams = {s[1:] for s in _swept() if s[0] == "family"}
    want = set()
    for bm, bn, kc, pf, split in ((256, 16, 16, 1, 0), (64, 16, 16, 2, 1), (128, 32, 16, 1, 0), (64, 32, 16, 1, 1),
                                  (64, 32, 32, 1, 1), (128, 64, 16, 1, 0), (64, 64, 16, 1, 0), (32, 64, 16, 1, 1)):
        want |= {(1, bm, bn, kc, pf, s) for s in ((False, True) if split else (False,))}
    want |= {(2, bm, bn, 16, k, False) for bm, bn in zip(M.TILE_BM[1:], M.TILE_BN[1:]) for k in (3, 7)}
    want |= {(3, bm, bn, kc, i, False)
             for bm, bn in ((128, 32), (128, 64), (64, 64)) for kc in (16, 32) for i in (0, 1)}
    want |= {(4, 128, bn, bk, 4, False) for bn, bk in ((32, 32), (64, 32), (64, 16), (32, 64), (64, 64))}
    want |= {(4, 128, 64, 32, 4, False), (4, 128, 128, 64, 8, False), (4, 128, 128, 32, 8, False)}
    assert len(want) == 12 + 14 + 12 + 7  # (<64, 32, 4> counts once here: fp32 and bf16 share the tuple)
    assert want <= fams, sorted(want - fams)
    assert fams <= want, sorted(fams - want)
