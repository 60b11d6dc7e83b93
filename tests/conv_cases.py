"""The case table of the direct-convolution route sweep (tests/test_conv_ref.py on the CPU,
tests/test_gpu_conv_routes.py on the GPU), built with the host route query
(fvp.cnn.conv_route: fvp_conv2d_ex_plan, no GPU needed) so that each case states the kernel
instantiation it must get.

Variants (46: the instantiations conv_launch of csrc/fvp_conv.hip can start, read off its
switch statements; tests/test_conv_route_model.py asserts that the route query returns these
and no others over its sweep):
  per-tap fp32  conv_mfma_kernel: tiles 256x16, 64x16 (PF 2), 128x32, 64x32 (KC 16), 64x32
                (KC 32, Cpi % 32 == 0), 128x64, 64x64, 32x64; the four small ones (64x16, both
                64x32, 32x64) also with split-K                                          12
  halo fp32     conv_halo_kernel: the seven tiles x KMAX 3 / 7 (the small four under
                CONV_HALO only)                                                           14
  bf16          conv_bf16_kernel: 128x32, 128x64, 64x64 x KC 16 / 32 x in_bf16 0 / 1
                (in_bf16 with KC 32 under CONV_PER_TAP_NOSPLIT only: else the DMA kernel)   12
  LDS-DMA       conv_dma_kernel: fp32 <32,32,4> <64,32,4> <64,16,4>; bf16 <32,64,4>
                <64,64,4> <128,64,8> <64,32,4> <128,32,8>                                   8
(The fp32 <128, ., 8> DMA instantiations the launcher used to name could never be chosen --
fp32 takes 64-column tiles above 64 columns -- and are no longer instantiated.)

Base cases, two per variant: the cheapest shape of the search (SQUARES / HALO_* images, N =
2 .. 80, 3x3 -- 5x5 for KMAX 7 -- stride 1 "same", ReLU, no residual, Cin 16 / 32 / 64, more
than one block) that selects the variant,
  full    the block grid divides evenly (halo: W % 16 == 0 and H a multiple of the tile rows)
  ragged  a partial last row tile, a partial last column tile where the column class has one
          (Cout 80 on 64-column tiles, Cout 16 on the 32-column tiles of the bf16 and DMA
          kernels, 48 / 80 on the DMA kernel's 64 / 128), halo: odd H, W % 16 != 0.
Variation cases (VARIATIONS) run on a small and a large launch of every family that takes
them; what "large" means per family is in _large().
"""
import collections
import functools
import itertools

import numpy as np

# fvp.cnn's kernel choices (CONV_*)
PER_TAP, HALO, NOSPLIT, DMA = 1, 2, 3, 4

Variant = collections.namedtuple("Variant", "family BM BN KC var split bf16")
Case = collections.namedtuple(
    "Case", "variant kind algo bf16 in_bf16 out_bf16 N Cin cpi Cout H W KH KW mode stride pad relu res_pre res_post")

FAMILY = {1: "per-tap", 2: "halo", 3: "bf16", 4: "dma"}
SQUARES = (5, 8, 16, 31, 32, 63, 64)                       # H = W of the per-tap / bf16 / DMA search
HALO_FULL = tuple((h, w) for h in (4, 8, 16, 32, 64) for w in (16, 32, 64))
HALO_RAGGED = tuple((h, w) for h in (5, 9, 17, 33, 63) for w in (29, 30, 31, 47, 63))
BATCHES = range(2, 81)


def variants():
    v = []
    for bm, bn, kc, pf, splits in ((256, 16, 16, 1, 0), (64, 16, 16, 2, 1), (128, 32, 16, 1, 0), (64, 32, 16, 1, 1),
                                   (64, 32, 32, 1, 1), (128, 64, 16, 1, 0), (64, 64, 16, 1, 0), (32, 64, 16, 1, 1)):
        v += [Variant(1, bm, bn, kc, pf, s, False) for s in ((False, True) if splits else (False,))]
    v += [Variant(2, bm, bn, 16, k, False, False)
          for bm, bn in ((256, 16), (64, 16), (128, 32), (64, 32), (128, 64), (64, 64), (32, 64)) for k in (3, 7)]
    v += [Variant(3, bm, bn, kc, i, False, True)
          for bm, bn in ((128, 32), (128, 64), (64, 64)) for kc in (16, 32) for i in (0, 1)]
    v += [Variant(4, 128, bn, bk, 4, False, False) for bn, bk in ((32, 32), (64, 32), (64, 16))]
    v += [Variant(4, 128, bn, bk, nw, False, True)
          for bn, bk, nw in ((32, 64, 4), (64, 64, 4), (128, 64, 8), (64, 32, 4), (128, 32, 8))]
    return tuple(v)


def variant_id(v):
    s = f"{FAMILY[v.family]}-{'bf16' if v.bf16 else 'f32'}-{v.BM}x{v.BN}-k{v.KC}-v{v.var}"
    return s + ("-split" if v.split else "")


def route_variant(route, bf16):
    """The Variant of a fvp_conv2d_ex_plan tuple."""
    return Variant(route[0], route[1], route[2], route[3], route[4], route[5] > 1, bool(bf16))


def geometry(c):
    """(KH, KW of the ABI, Ho, Wo) of a case."""
    if c.mode == 0:
        return (c.KH, c.KW, (c.H + 2 * c.pad[0] - c.KH) // c.stride[0] + 1,
                (c.W + 2 * c.pad[1] - c.KW) // c.stride[1] + 1)
    return (2, 2, 2 * c.H, 2 * c.W) if c.mode == 3 else (1, 1, c.H if c.mode == 2 else 2 * c.H, 2 * c.W)


def _rup(x, m):
    return -(-x // m) * m


def query(c):
    """fvp_conv2d_ex_plan for a case, with the arguments fvp.cnn.ConvLayer passes for it
    (bf16 layers: no workspace; fp32 CONV_DMA: FVP_CONV_F32_KC; else the size
    fvp_conv2d_ex_workspace_bytes gives) -- the search's fast path; the coverage test holds
    every case of the table to fvp.cnn.conv_route on the layer itself."""
    import ctypes

    from fvp import _lib

    lib = _lib.load()
    kh, kw = geometry(c)[:2]
    cpi = c.cpi or _rup(c.Cin, 16)
    geo = (c.N, c.H, c.W, cpi, kh, kw, _rup(c.Cout, 16), c.mode, c.stride[0], c.stride[1], c.pad[0], c.pad[1])
    algo = 0 if c.algo == DMA else c.algo
    if c.bf16:
        flags, ws = 1 | (2 if c.in_bf16 and cpi % 16 == 0 else 0) | (4 if c.out_bf16 else 0), 0
    elif c.algo == DMA:
        flags, ws = 8, 0
    else:
        flags, ws = 0, lib.fvp_conv2d_ex_workspace_bytes(*geo, algo)
    plan = (ctypes.c_int * 8)()
    st = lib.fvp_conv2d_ex_plan(*geo, flags, algo, ws, plan)
    return tuple(plan) if st == 0 else None


def _base(v, kind, **kw):
    f = dict(variant=v, kind=kind, algo=PER_TAP, bf16=bool(v and v.bf16), in_bf16=False, out_bf16=False, N=2, Cin=16,
             cpi=None, Cout=16, H=8, W=8, KH=3, KW=3, mode=0, stride=(1, 1), pad=(1, 1), relu=True, res_pre=False,
             res_post=False)
    f.update(kw)
    return Case(**f)


def _choices(v, kind):
    """(algos, Cin, Cout, K) the search tries for a variant."""
    ragged = kind == "ragged"
    if v.family == 1:
        cout = {16: 16, 32: 32, 64: 80 if ragged else 64}[v.BN]
        return (PER_TAP, NOSPLIT), 32 if v.KC == 32 else 16, cout, 3
    if v.family == 2:
        cout = {16: (16,), 32: (32,), 64: (80, 144) if ragged else (64, 128)}[v.BN]
        return (HALO,), 16, cout, 3 if v.var == 3 else 5
    if v.family == 3:
        cout = (16 if ragged else 32) if v.BN == 32 else (80 if ragged else 64)
        return (NOSPLIT if v.var and v.KC == 32 else PER_TAP,), v.KC, cout, 3
    if not v.bf16:
        cout = (16 if ragged else 32) if v.BN == 32 else (80 if ragged else 64)
        return (DMA,), v.KC, cout, 3
    cout = {32: (16, 32), 64: (48, 64), 128: (80, 128)}[v.BN][0 if ragged else 1]
    return (PER_TAP,), v.KC, cout, 3


def _shape_ok(v, kind, n, h, w, cout):
    """full / ragged as the module docstring defines them, and more than one block."""
    cols = _rup(cout, 16)
    if v.family == 2:
        rows = v.BM // 16
        return (w % 16 == 0 and h % rows == 0 and cols % v.BN == 0) if kind == "full" else \
            (w % 16 != 0 and h % 2 == 1 and h % rows != 0)
    m = n * h * w
    if m <= v.BM:
        return False
    return (m % v.BM == 0 and cols % v.BN == 0) if kind == "full" else m % v.BM != 0


@functools.lru_cache(maxsize=None)
def base_case(v, kind):
    """The cheapest case (N H W Cout K^2: the reference's work) that selects variant v, or None."""
    algos, cin, couts, k = _choices(v, kind)
    couts = couts if isinstance(couts, tuple) else (couts,)
    images = (HALO_FULL if kind == "full" else HALO_RAGGED) if v.family == 2 else tuple((s, s) for s in SQUARES)
    cand = sorted((n * h * w * co, n, h, w, co) for n in BATCHES for h, w in images for co in couts
                  if _shape_ok(v, kind, n, h, w, co))
    for _, n, h, w, co in cand:
        for algo in algos:
            c = _base(v, kind, algo=algo, in_bf16=bool(v.family == 3 and v.var) or (v.family == 4 and v.bf16),
                      N=n, Cin=cin, Cout=co, H=h, W=w, KH=k, KW=k, pad=(k // 2, k // 2))
            r = query(c)
            if r is not None and route_variant(r, v.bf16) == v:
                return c
    return None


def base_cases(v):
    return tuple(c for c in (base_case(v, "full"), base_case(v, "ragged")) if c is not None)


# ---- variations ----------------------------------------------------------------------------
# name -> (fields that differ from the family's plain 3x3 case, families that take it)
ALL, NOT_HALO = (1, 2, 3, 4), (1, 3, 4)
VARIATIONS = collections.OrderedDict([
    ("linear", (dict(relu=False), ALL)),
    ("pre+post", (dict(res_pre=True, res_post=True), ALL)),
    ("post-linear", (dict(relu=False, res_post=True), ALL)),
    ("s22p0", (dict(stride=(2, 2), pad=(0, 0)), NOT_HALO)),
    ("s22pK", (dict(stride=(2, 2), pad=(2, 2)), NOT_HALO)),
    ("s13p0", (dict(stride=(1, 3), pad=(0, 0)), NOT_HALO)),
    ("s13pK", (dict(stride=(1, 3), pad=(2, 2)), NOT_HALO)),
    ("s42p0", (dict(stride=(4, 2), pad=(0, 0)), NOT_HALO)),
    ("s42pK", (dict(stride=(4, 2), pad=(2, 2)), NOT_HALO)),
    ("k1x5", (dict(KH=1, KW=5, pad=(0, 2)), ALL)),
    ("k5x1", (dict(KH=5, KW=1, pad=(2, 0)), ALL)),
    ("k3x7", (dict(KH=3, KW=7, pad=(1, 3)), ALL)),
    ("k7x7", (dict(KH=7, KW=7, pad=(3, 3)), ALL)),     # 49 taps: the DMA kernel refuses (left out there)
    ("mode1", (dict(mode=1, KH=2, KW=2, pad=(0, 0)), NOT_HALO)),
    ("mode2", (dict(mode=2, KH=1, KW=2, pad=(0, 0), H=1), NOT_HALO)),
    ("mode3", (dict(mode=3, KH=4, KW=4, pad=(1, 1)), NOT_HALO)),
    ("rows1", (dict(H=1, KH=1, KW=3, pad=(0, 1)), ALL)),                 # the Conv1d shape
    ("cpi4", (dict(Cin=3, cpi=4), (1, 3))),      # fp32 input only: a K chunk spans four taps,
    ("cpi8", (dict(Cin=7, cpi=8), (1, 3))),      # two taps,
    ("cpi12", (dict(Cin=12, cpi=12), (1, 3))),   # 1 1/3 taps; k past the taps reads zero
    ("cout17", (dict(Cout=17), ALL)),            # padded to 32
    ("cout80", (dict(Cout=80), ALL)),            # a partial 64-column tile, weights padded to 128
    ("mode1-cpo48", (dict(mode=1, KH=2, KW=2, pad=(0, 0), Cout=48), NOT_HALO)),   # 192 columns
    ("mode3-split", (dict(mode=3, KH=4, KW=4, pad=(1, 1), Cin=32), (1,))),        # split-K x 4 parity groups
    ("bf16-out", (dict(out_bf16=True, res_pre=True, res_post=True), (3, 4))),     # (bf16 operands only)
])
# flavours of a family a variation runs under: (family, bf16 operands, in_bf16, algo, Cin)
FLAVOURS = ((1, False, False, PER_TAP, 16), (2, False, False, HALO, 16), (3, True, False, PER_TAP, 16),
            (3, True, True, NOSPLIT, 32), (4, False, False, DMA, 32), (4, True, True, PER_TAP, 64))
def _large(fam, route):
    """Whether a route is the family's large launch: per-tap / halo -- the 256- or 128-row tile
    of its column class (>= 512 blocks); bf16 -- 128 rows on 64-column tiles (>= 512 blocks), on
    32 columns (one tile size) >= 512 blocks; DMA (one tile per class) -- >= 512 blocks."""
    if fam in (1, 2):
        return route[1] == (256 if route[2] == 16 else 128)
    if fam == 3 and route[2] == 64:
        return route[1] == 128
    return route[7] >= 512


SIZES = (9, 17, 33, 129, 1025)   # H = W of the variations (the field overrides apply: rows of height 1 stay so)
HALO_SIZES = (31, 63, 127, 255)  # W >= 16 within the 1/8-waste rule


@functools.lru_cache(maxsize=None)
def variation_cases(name):
    """For every flavour that takes the variation: the cheapest small launch (N = 2) and the
    cheapest large one (N <= 80), by N H W."""
    fields, fams = VARIATIONS[name]
    out = []
    for fam, bf16, inb, algo, cin in FLAVOURS:
        if fam not in fams or (fields.get("out_bf16") and not bf16) or (fields.get("cpi") and inb):
            continue
        if fam == 4 and fields.get("mode", 0) == 0 and fields.get("KH", 3) * fields.get("KW", 3) > 32:
            continue
        cand = []
        for s, n in itertools.product(HALO_SIZES if fam == 2 else SIZES, BATCHES):
            f = dict(algo=algo, bf16=bf16, in_bf16=inb, Cin=cin, N=n, H=s, W=s, Cout=32)
            f.update(fields)
            if name == "mode3-split":
                f.update(H=5, W=5)
            cand.append(_base(None, name, **f))
        cand.sort(key=lambda c: (c.N * c.H * c.W, c.N))
        for size in ("small", "large"):
            for c in cand:
                if size == "small" and c.N > 2:
                    continue
                r = query(c)
                if r is None or r[0] != fam or (name == "mode3-split" and not (r[5] > 1 and r[6] == 4)):
                    continue
                if _large(fam, r) == (size == "large"):
                    out.append(c._replace(variant=route_variant(r, bf16), kind=f"{name}/{size}"))
                    break
    return tuple(out)


def all_cases():
    out = [c for v in variants() for c in base_cases(v)]
    return out + [c for name in VARIATIONS for c in variation_cases(name)]


def case_id(c):
    g = {0: f"{c.KH}x{c.KW} s{c.stride[0]}{c.stride[1]} p{c.pad[0]}{c.pad[1]}", 1: "deconv2s2", 2: "deconv1d",
         3: "deconv4s2p1"}[c.mode]
    return (f"{variant_id(c.variant)} {c.kind} algo {c.algo} N={c.N} {c.Cin}({c.cpi or _rup(c.Cin, 16)})->{c.Cout} "
            f"{c.H}x{c.W} {g}")


def seed(c):
    return ((c.Cin * 131 + c.Cout) * 4099 + c.H * 67 + c.W) * 31 + c.KH * 7 + c.KW + (c.mode << 24)


def modules(c):
    """(conv, bn) of a case on the CPU, eval mode, weights and BatchNorm statistics from
    fvp.synthetic.seeded_state_dict (as the other CNN tests take them)."""
    import torch.nn as nn

    from fvp import synthetic

    if c.mode == 0:
        conv = nn.Conv2d(c.Cin, c.Cout, (c.KH, c.KW), stride=c.stride, padding=c.pad)
        bn = nn.BatchNorm2d(c.Cout)
    elif c.mode == 2:
        conv, bn = nn.ConvTranspose1d(c.Cin, c.Cout, 2, stride=2), nn.BatchNorm1d(c.Cout)
    else:
        k = 2 if c.mode == 1 else 4
        conv, bn = nn.ConvTranspose2d(c.Cin, c.Cout, k, stride=2, padding=k // 2 - 1, bias=c.mode == 1), \
            nn.BatchNorm2d(c.Cout)
    seq = nn.Sequential(conv, bn).eval()
    seq.load_state_dict(synthetic.seeded_state_dict(seq, seed(c)))
    return seq[0], seq[1]


def inputs(c):
    """(x, res_pre, res_post) float32 NCHW: x uniform in (-0.5, 0.5), residuals in (-1, 1) or
    None, every image different; x rounded to bf16 where the layer reads bf16 activations,
    the residuals where it writes them (so they are bf16-representable in either storage)."""
    import conv_ref as R

    rng = np.random.default_rng(seed(c) + 7)
    x = rng.uniform(-0.5, 0.5, (c.N, c.Cin, c.H, c.W)).astype(np.float32)
    if c.in_bf16:
        x = R.bf16_round(x)
    ho, wo = geometry(c)[2:]
    res = [rng.uniform(-1.0, 1.0, (c.N, c.Cout, ho, wo)).astype(np.float32) if on else None
           for on in (c.res_pre, c.res_post)]
    if c.out_bf16:
        res = [None if r is None else R.bf16_round(r) for r in res]
    return x, res[0], res[1]
