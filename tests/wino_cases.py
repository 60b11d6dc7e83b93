"""The case table of the Winograd grid sweep (tests/test_wino_ref.py on the CPU,
tests/test_gpu_wino_grids.py on the GPU), built with the host planner
(fvp.cnn.wino_plan: fvp_conv3x3_wino_plan, no GPU needed) so that each case states the
plan it must get: the tile grid from the image size, the kernel instantiation from the
launch size (N and Cout).

Per grid (the 52 legal ones: tr, tc in 2 .. 16, tr tc <= 32, (2 tr + 2)(2 tc + 2) <= 180):
  single  the smallest image that selects it: 2 t - 1 rows / columns for t tiles (1 for
          t = 2, the smallest grid side there is), odd, so the last tile row and column
          are partial
  multi   the smallest odd H x W <= 69 x 69 on which the planner picks the grid for two or
          more blocks with a partial last block (NO_MULTI: the grids that have none,
          because a larger grid wins on every image that large)
each under every instantiation: conv <1,2> (N = 2, Cout = 32), <1,1> (Cout = 32, more than
256 blocks), <2,1> (Cout = 64, >= 512 blocks); deconv <1> (N = 2, Cout = 32), <2>
(Cout = 64, >= 512 blocks; the plan is taken on the input size).  Cin = 16.

On VARIANT_GRIDS, again under every instantiation (on the grid's multi-block image): the
epilogue variants and the channel variants of VARIANTS.
"""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "kernel grid kind inst N Cin Cout H W relu res_pre res_post pool")

INSTS = {"conv": ((1, 2), (1, 1), (2, 1)), "deconv": ((1, 2), (2, 1))}  # wino_plan(...)[2:4] = (NB, XS)
INST_NAME = {("conv", (1, 2)): "conv<1,2>", ("conv", (1, 1)): "conv<1,1>", ("conv", (2, 1)): "conv<2,1>",
             ("deconv", (1, 2)): "deconv<1>", ("deconv", (2, 1)): "deconv<2>"}
VARIANT_GRIDS = ((4, 8), (8, 4), (5, 5))
SEARCH = 69
# name -> (fields that differ from the per-grid case, kernels, NB it runs under or None for both)
VARIANTS = collections.OrderedDict([
    ("linear", (dict(relu=False), ("conv", "deconv"), None)),
    ("pre+post", (dict(res_pre=True, res_post=True), ("conv", "deconv"), None)),
    ("post-linear", (dict(relu=False, res_post=True), ("conv", "deconv"), None)),
    ("pool", (dict(pool=True), ("conv",), None)),
    ("cin48", (dict(Cin=48), ("conv", "deconv"), None)),    # three K steps
    ("cin20", (dict(Cin=20), ("conv", "deconv"), None)),    # padded to 32
    ("cout96", (dict(Cout=96), ("conv", "deconv"), 1)),     # three 32-column blocks
    ("cout128", (dict(Cout=128), ("conv", "deconv"), 2)),   # two 64-column blocks
    ("cout17", (dict(Cout=17), ("conv", "deconv"), 1)),     # padded to 32
])


def _plan(n, h, w, cpo):
    from fvp import cnn

    return cnn.wino_plan(n, h, w, cpo)


def legal_grids():
    return tuple((tr, tc) for tr in range(2, 17) for tc in range(2, 17)
                 if tr * tc <= 32 and (2 * tr + 2) * (2 * tc + 2) <= 180)


def single_image(grid):
    return tuple(1 if t == 2 else 2 * t - 1 for t in grid)


@functools.lru_cache(maxsize=None)
def multi_images():
    """grid -> the smallest odd (H, W) <= SEARCH with >= 2 blocks and a partial last block."""
    best = {}
    for h in range(1, SEARCH + 1, 2):
        for w in range(1, SEARCH + 1, 2):
            tr, tc = _plan(1, h, w, 32)[:2]
            blocks = -(-h // (2 * tr)) * -(-w // (2 * tc))
            if blocks >= 2 and (h % (2 * tr) or w % (2 * tc)):
                if (tr, tc) not in best or h * w < best[tr, tc][0] * best[tr, tc][1]:
                    best[tr, tc] = (h, w)
    return best


def blocks_per_image(grid, h, w):
    return -(-h // (2 * grid[0])) * -(-w // (2 * grid[1]))


def batch(inst, per_image, cpo):
    """The smallest batch of at least two images that launches ``inst`` (wino_plan's rule:
    NB = 2 from 1,024 32-column blocks where Cpo % 64 == 0, XS = 2 up to 256 blocks)."""
    col = per_image * (cpo // 32)
    if inst == (1, 2):
        return 2
    if inst == (1, 1):
        return max(2, 256 // col + 1)
    return max(2, -(-1024 // col))


def _case(kernel, grid, kind, inst, h, w, **kw):
    f = dict(Cin=16, Cout=64 if inst[0] == 2 else 32, relu=True, res_pre=False, res_post=False, pool=False)
    f.update(kw)
    n = batch(inst, blocks_per_image(grid, h, w), -(-f["Cout"] // 32) * 32)
    return Case(kernel=kernel, grid=grid, kind=kind, inst=inst, N=n, H=h, W=w, **f)


@functools.lru_cache(maxsize=None)
def grid_cases(kernel, grid):
    """The per-grid cases of one kernel: single (and multi) image x every instantiation."""
    images = [("single", single_image(grid))]
    if grid in multi_images():
        images.append(("multi", multi_images()[grid]))
    return tuple(_case(kernel, grid, kind, inst, h, w) for kind, (h, w) in images for inst in INSTS[kernel])


@functools.lru_cache(maxsize=None)
def variant_cases(kernel, grid, name):
    fields, kernels, nb = VARIANTS[name]
    assert kernel in kernels, (kernel, name)
    h, w = multi_images()[grid]
    return tuple(_case(kernel, grid, name, inst, h, w, **fields) for inst in INSTS[kernel] if nb in (None, inst[0]))


def variant_ids(kernel):
    return [(grid, name) for grid in VARIANT_GRIDS for name, (_, kernels, _) in VARIANTS.items() if kernel in kernels]


def all_cases(kernel):
    out = [c for grid in legal_grids() for c in grid_cases(kernel, grid)]
    return out + [c for grid, name in variant_ids(kernel) for c in variant_cases(kernel, grid, name)]


def no_multi():
    return tuple(g for g in legal_grids() if g not in multi_images())


def case_id(c):
    return f"{INST_NAME[c.kernel, c.inst]} grid {c.grid[0]}x{c.grid[1]} {c.kind} N={c.N} {c.Cin}->{c.Cout} {c.H}x{c.W}"


def seed(c):
    return (c.Cin * 131 + c.Cout) * 4099 + c.H * 67 + c.W + (1 << 20) * (c.kernel == "deconv")


def modules(c):
    """(conv, bn) of a case on the CPU, eval mode, weights and BatchNorm statistics from
    fvp.synthetic.seeded_state_dict (as the other CNN tests take them)."""
    import torch.nn as nn

    from fvp import synthetic

    conv = (nn.Conv2d(c.Cin, c.Cout, 3, padding=1) if c.kernel == "conv"
            else nn.ConvTranspose2d(c.Cin, c.Cout, 4, stride=2, padding=1, bias=False))
    seq = nn.Sequential(conv, nn.BatchNorm2d(c.Cout)).eval()
    seq.load_state_dict(synthetic.seeded_state_dict(seq, seed(c)))
    return seq[0], seq[1]


def inputs(c, n=None):
    """(x, res_pre, res_post) float32 NCHW: x uniform in (-0.5, 0.5), residuals in (-1, 1)
    or None, every image different.  n: the batch (default the case's)."""
    n = c.N if n is None else n
    rng = np.random.default_rng(seed(c) + 7)
    x = rng.uniform(-0.5, 0.5, (n, c.Cin, c.H, c.W)).astype(np.float32)
    ho, wo = (2 * c.H, 2 * c.W) if c.kernel == "deconv" else (c.H, c.W)
    res = [rng.uniform(-1.0, 1.0, (n, c.Cout, ho, wo)).astype(np.float32) if on else None
           for on in (c.res_pre, c.res_post)]
    return x, res[0], res[1]
