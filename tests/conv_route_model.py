"""An independent model of which kernel fvp_conv2d_nhwc_ex launches (plain Python, no
library call): the rules of conv_geom, conv_plan and conv_launch of csrc/fvp_conv.hip
restated from their text as it stood before the launcher was made to switch on
conv_route.  tests/test_conv_route_model.py holds fvp_conv2d_ex_plan to it on a sweep of
both sides of every threshold, which pins that factoring the decision out changed no choice.

route(...) returns (status, plan): status 0 / 1002 (FVP_ERR_SHAPE) and plan the 8 slots of
fvp_conv2d_ex_plan (include/fvp.h) or None.
"""
OK, ERR_SHAPE = 0, 1002
AUTO, PER_TAP, HALO, NOSPLIT = 0, 1, 2, 3
BF16, BF16_IN, BF16_OUT, F32_KC = 1, 2, 4, 8
INT_MAX = 2 ** 31 - 1

TILE_BM = (0, 256, 64, 128, 64, 128, 64, 32)
TILE_BN = (0, 16, 16, 32, 32, 64, 64, 64)


def cdiv(a, b):
    return -(-a // b)


def geom(H, W, Cpi, KH, KW, mode, sy, sx, py, px):
    """(status, dict Hm Wm Ho Wo sy sx py px) -- conv_geom."""
    if H <= 0 or W <= 0 or KH <= 0 or KW <= 0 or Cpi <= 0 or Cpi % 4 or (Cpi > 16 and Cpi % 16):
        return ERR_SHAPE, None
    if mode == 0:
        if sy < 1 or sx < 1 or sy > 4 or sx > 4 or py < 0 or px < 0 or py >= KH or px >= KW:
            return ERR_SHAPE, None
        if H + 2 * py < KH or W + 2 * px < KW:
            return ERR_SHAPE, None
        ho, wo = (H + 2 * py - KH) // sy + 1, (W + 2 * px - KW) // sx + 1
        return OK, dict(Hm=ho, Wm=wo, Ho=ho, Wo=wo, sy=sy, sx=sx, py=py, px=px)
    g = dict(Hm=H, Wm=W, sy=1, sx=1, py=0, px=0)
    if mode in (1, 2):
        if (KH, KW) != (1, 1):
            return ERR_SHAPE, None
        g.update(Ho=2 * H if mode == 1 else H, Wo=2 * W)
        return OK, g
    if mode == 3:
        if (KH, KW) != (2, 2):
            return ERR_SHAPE, None
        g.update(Ho=2 * H, Wo=2 * W)
        return OK, g
    return ERR_SHAPE, None


def plan_f32(N, Cpi, KH, KW, Ntot, G, mode, g, algo):
    """(halo tile id or 0, per-tap tile id, split-K) -- conv_plan."""
    M = N * g["Hm"] * g["Wm"]
    W, H = g["Wm"], g["Hm"]
    tx = cdiv(W, 16)
    same = mode == 0 and g["sy"] == 1 and g["sx"] == 1 and 2 * g["py"] == KH - 1 and 2 * g["px"] == KW - 1
    halo = (algo in (AUTO, HALO) and same and Cpi % 16 == 0 and (KH > 1 or KW > 1) and KH <= 7 and KW <= 7
            and W >= 16 and (tx * 16 - W) * 8 <= W)

    def hblocks(i):
        return N * tx * cdiv(H, TILE_BM[i] // 16) * cdiv(Ntot, TILE_BN[i])

    if halo:
        big = 1 if Ntot <= 16 else 3 if Ntot <= 32 else 5
        if hblocks(big) >= 512:
            return big, 0, 1
        if algo == HALO:
            return ((6 if hblocks(6) >= 512 else 7) if big == 5 else big + 1), 0, 1

    def blocks(i):
        return G * cdiv(M, TILE_BM[i]) * cdiv(Ntot, TILE_BN[i])

    if Ntot <= 16:
        tile = 1 if blocks(1) >= 512 else 2
    elif Ntot <= 32:
        tile = 3 if blocks(3) >= 512 else 4
    else:
        tile = 5 if blocks(5) >= 512 else 6 if blocks(6) >= 512 else 7
    ks = 1
    nchunks = cdiv(KH * KW * Cpi, 16)
    nb = blocks(tile)
    if algo != NOSPLIT and g["Hm"] > 1 and nb < 256 and nchunks >= 8:
        ks = min(cdiv(512, nb), nchunks // 4, 8)
        if ks < 2:
            ks = 1
    return 0, tile, ks


def route(N, H, W, Cpi, KH, KW, Cpo, mode, sy, sx, py, px, bf16, algo, workspace_bytes):
    st, g = geom(H, W, Cpi, KH, KW, mode, sy, sx, py, px)
    if st:
        return st, None
    if bf16 & ~(BF16 | BF16_IN | BF16_OUT | F32_KC):
        return ERR_SHAPE, None
    if bf16 & (BF16_IN | BF16_OUT) and not bf16 & BF16:
        return ERR_SHAPE, None
    if bf16 & F32_KC and bf16 & BF16:
        return ERR_SHAPE, None
    if N <= 0 or Cpo <= 0 or Cpo % 16:
        return ERR_SHAPE, None
    if algo < AUTO or algo > NOSPLIT:
        return ERR_SHAPE, None
    Ntot = (1, 4, 2, 1)[mode] * Cpo
    Cpo_w = cdiv(Ntot, 128) * 128
    G = 4 if mode == 3 else 1
    M = N * g["Hm"] * g["Wm"]
    if N * g["Ho"] * g["Wo"] * Cpo > INT_MAX * 4 or N * H * W * Cpi > INT_MAX * 4:
        return ERR_SHAPE, None
    es = 2 if bf16 & BF16 else 4
    fits = (N * H * W * Cpi * es < 1 << 31 and Cpo_w * KH * KW * Cpi * es < 1 << 31 and KH * KW <= 32
            and M < 1 << 24)

    def dma(E):
        row128 = Cpi * E % 128 == 0
        if Ntot > 64:
            BN = 64 if E == 4 else 128
        else:
            BN = 64 if (Ntot > 32 or not row128) else 32
        BK = (128 if row128 else 64) // E  # (BN == 32 only with 128-B rows)
        return OK, (4, 128, BN, BK, 8 if BN == 128 else 4, 1, G, min(cdiv(M, 128) * cdiv(Ntot, BN) * G, INT_MAX))

    if bf16 & F32_KC:
        if Cpi % 16 or not fits:
            return ERR_SHAPE, None
        return dma(4)
    if bf16:
        inb = 1 if bf16 & BF16_IN else 0
        if Cpi % 16 and inb:
            return ERR_SHAPE, None
        if inb and Cpi % 32 == 0 and algo != NOSPLIT and fits:
            return dma(2)
        KC = 32 if Cpi % 32 == 0 else 16
        if Ntot <= 32:
            BM, BN = 128, 32
        elif G * cdiv(M, 128) * cdiv(Ntot, 64) >= 512:
            BM, BN = 128, 64
        else:
            BM, BN = 64, 64
        return OK, (3, BM, BN, KC, inb, 1, G, min(cdiv(M, BM) * cdiv(Ntot, BN) * G, INT_MAX))
    halo, tile, ks = plan_f32(N, Cpi, KH, KW, Ntot, G, mode, g, algo)
    if halo:
        BM, BN = TILE_BM[halo], TILE_BN[halo]
        blocks = N * cdiv(W, 16) * cdiv(H, BM // 16) * cdiv(Ntot, BN)
        return OK, (2, BM, BN, 16, 3 if KH <= 3 and KW <= 3 else 7, 1, G, min(blocks, INT_MAX))
    if ks > 1 and workspace_bytes < G * ks * M * Ntot * 4:
        ks = 1
    BM, BN = TILE_BM[tile], TILE_BN[tile]
    KC = 32 if tile == 4 and Cpi % 32 == 0 else 16
    PF = 2 if tile == 2 else 1
    return OK, (1, BM, BN, KC, PF, ks, G, min(cdiv(M, BM) * cdiv(Ntot, BN) * G * ks, INT_MAX))


def workspace_bytes(N, H, W, Cpi, KH, KW, Cpo, mode, sy, sx, py, px, algo):
    """fvp_conv2d_ex_workspace_bytes: the scratch of the fp32 kernels' split-K (0: none)."""
    st, g = geom(H, W, Cpi, KH, KW, mode, sy, sx, py, px)
    if st or N <= 0 or Cpo <= 0 or Cpo % 16 or algo < AUTO or algo > NOSPLIT:
        return 0
    Ntot, G = (1, 4, 2, 1)[mode] * Cpo, 4 if mode == 3 else 1
    halo, _, ks = plan_f32(N, Cpi, KH, KW, Ntot, G, mode, g, algo)
    return G * ks * N * g["Hm"] * g["Wm"] * Ntot * 4 if ks > 1 and not halo else 0
