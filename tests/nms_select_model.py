"""A plain numpy restatement of the selection bookkeeping of ``nms_select_kernel``
(faster-voxelpose_amd/csrc/fvp_proposal.hip) and of ``nms_any``'s choice of kernel, plus the
maps that drive the kernel into its over-capacity fallback.  Not a conftest: the CPU tests
(test_nms_select_model.py) and the GPU tests (test_gpu_nms_select.py) import it.

It models WHICH elements become candidates and in what order they are picked, nothing of how
the kernel computes it (no LDS, no DPP): the masked map comes from the oracle's formula, and
the result the tests compare against is always ``oracle.fvp_oracle.nms2d``, never this model.
The model's only job in a GPU test is ``candidate_count``: a test of the fallback asserts it
against kSelCap first, so it cannot pass by the list path.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
U64 = np.uint64

# each constant with the line of fvp_proposal.hip it copies
SEL_THREADS = 1024     # :165 kSelThreads
SEL_WAVES = 16         # :166 kSelWaves = kSelThreads / 64: the select kernel takes K <= 16 (:522)
SEL_CAP = 4096         # :167 kSelCap, the candidate list's capacity; :376 "if (C <= kSelCap)", else the fallback
SEL_MAX_E = 32         # :168 kSelMaxE: elements per thread, :331 "e = tid + i * kSelThreads"
ROW_LANES = 16         # :345 "(lane & 15) == 15": the threshold comes from the maxima of 16-lane rows
ROWS = SEL_THREADS // ROW_LANES  # :263 gmax[4 * kSelWaves]: 64 rows
SEL_LDS_MAX = 159 * 1024         # :522 "sel_lds <= 159 * 1024"
TOPK_LDS_MAX = 150 * 1024        # :516 "lds > 150 * 1024" -> FVP_ERR_SHAPE
MAX_STRIP = 16         # :530 "if (nxb && es <= 16)"


# ---------------------------------------------------------------------------------------------
# nms_any's arithmetic
def dispatch(X: int, Y: int, K: int):
    """The kernel ``nms_any`` (:510-555) launches for an X x Y map and K winners:
    ("select", E, STRIP) for nms_select_kernel<E, STRIP>, ("topk",) for nms_topk_kernel, or
    None where it returns FVP_ERR_SHAPE."""
    M = X * Y
    if X <= 0 or Y <= 0 or K <= 0 or K > M:
        return None
    if M * 4 + ((M + 31) // 32) * 4 > TOPK_LDS_MAX:
        return None
    E = (M + SEL_THREADS - 1) // SEL_THREADS
    sel_lds = ((M * 4 + 15) & ~15) + SEL_CAP * 8
    if not (K <= SEL_WAVES and E <= SEL_MAX_E and sel_lds <= SEL_LDS_MAX):
        return ("topk",)
    nxb = SEL_THREADS // Y if Y <= SEL_THREADS else 0
    es = (X + nxb - 1) // nxb if nxb else 0
    pow2 = lambda n: next(e for e in (1, 2, 4, 8, 16, 32) if n <= e)
    if nxb and es <= MAX_STRIP:
        return ("select", pow2(es), True)
    return ("select", pow2(E), False)


def capacity_bound(M: int, K: int) -> int:
    """At most K - 1 of the 64 rows have a maximum above the threshold, a row owns 16 elements
    of each 1024-element slice, and the threshold element itself is the + 1."""
    return (K - 1) * ROW_LANES * ((M + SEL_THREADS - 1) // SEL_THREADS) + 1


# ---------------------------------------------------------------------------------------------
# the bookkeeping
def masked_map(p: np.ndarray) -> np.ndarray:
    """The flat masked map of one frame p [X, Y], as oracle.fvp_oracle.nms2d computes it:
    keep * p with keep = (p == 3x3 maximum, -inf padded, NaN propagating)."""
    p = np.asarray(p, F32)
    X, Y = p.shape
    pad = np.full((X + 2, Y + 2), -np.inf, F32)
    pad[1:-1, 1:-1] = p
    mx = np.full((X, Y), -np.inf, F32)
    for dx in range(3):
        for dy in range(3):
            mx = np.maximum(mx, pad[dx:dx + X, dy:dy + Y])
    return ((p == mx).astype(F32) * p).reshape(-1)


def order_keys(masked: np.ndarray) -> np.ndarray:
    """cand_key (:38-42): ord << 32 | ~index with ord = 0xffffffff for NaN, the sign-flipped bits for
    numbers (+-0 both 0x80000000); a larger key is picked earlier."""
    v = np.asarray(masked, F32).reshape(-1)
    u = v.view(np.uint32).astype(U64)
    u = np.where(v == 0, U64(0), u)
    neg = (u & U64(0x80000000)) != 0
    ord_ = np.where(neg, ~u & U64(0xffffffff), u | U64(0x80000000))
    ord_ = np.where(np.isnan(v), U64(0xffffffff), ord_)
    idx = np.arange(v.size, dtype=U64)
    return (ord_ << U64(32)) | (~idx & U64(0xffffffff))


def row_of(e):
    """The 16-lane row whose maximum covers element e (:331, :345): thread e % 1024, row tid / 16."""
    return (np.asarray(e) % SEL_THREADS) // ROW_LANES


def row_maxima(keys: np.ndarray) -> np.ndarray:
    """gmax[64] (:340-345): the largest key of each row, 0 for a row without elements."""
    g = np.zeros(ROWS, U64)
    np.maximum.at(g, row_of(np.arange(keys.size)), keys)
    return g


def threshold(keys: np.ndarray, K: int) -> int:
    """t (:347-355): the row maximum that exactly K - 1 others exceed (thr stays 0 when none has that
    rank), and never below 1, the smallest key a real element can have."""
    g = row_maxima(keys)
    rank = (g[None, :] > g[:, None]).sum(axis=1)
    hit = g[rank == K - 1]
    return max(int(hit[0]) if hit.size else 0, 1)


def candidate_count(masked: np.ndarray, K: int) -> int:
    """C (:358-375): how many keys reach the threshold.  C > SEL_CAP takes the fallback."""
    keys = order_keys(masked)
    return int((keys >= U64(threshold(keys, K))).sum())


def select(masked: np.ndarray, K: int, round0_takes_any: bool = True) -> np.ndarray:
    """The flat indices the kernel writes (:376-418): by rank within the candidate list, or -- over
    capacity -- K rounds of the largest key below the previous winner.  round0_takes_any=False
    is the kernel before its fix: round 0 also kept only keys < ~0, so a NaN at flat index 0
    (whose key is exactly ~0) could not be picked."""
    keys = order_keys(masked)
    cand = keys[keys >= U64(threshold(keys, K))]
    if cand.size <= SEL_CAP:
        win = np.sort(cand)[::-1][:K]
    else:
        win, prev = [], ~U64(0)
        for r in range(K):
            ok = keys if (r == 0 and round0_takes_any) else keys[keys < prev]
            prev = ok.max() if ok.size else U64(0)
            win.append(prev)
        win = np.array(win, U64)
    return (~win & U64(0xffffffff)).astype(np.int64)


# ---------------------------------------------------------------------------------------------
# maps
def _isolated_cells(ok: np.ndarray, X: int, Y: int, n: int, rng) -> list:
    """n cells among ok (flat indices), in seeded order, whose 5x5 neighbourhoods hold no other
    chosen cell and not cell 0: their 3x3 windows never overlap."""
    chosen = [0]
    for e in rng.permutation(ok):
        if len(chosen) == n + 1:
            break
        ex, ey = divmod(int(e), Y)
        if all(max(abs(ex - c // Y), abs(ey - c % Y)) > 2 for c in chosen):
            chosen.append(int(e))
    assert len(chosen) == n + 1, "map too small for that many isolated cells"
    return chosen[1:]


def adversarial_map(X: int, Y: int, K: int, drop: int = 0, nan0: bool = False, peaks: int = 0, seed: int = 0,
                    extra_nans: int = 0) -> np.ndarray:
    """A frame [X, Y] that fills K - 1 rows: 1.0 where e % 1024 < 16 * (K - 1), 0.0 elsewhere.
    The ones tie with their neighbours, so each survives the 3x3 mask, the K - 1 rows of ones
    have the largest maxima, the threshold is the first zero's key, and every one is a
    candidate: C = capacity_bound(X * Y, K) when the last slice is full.

    drop: the last `drop` ones are zeroed (C shrinks by `drop`).
    peaks: that many isolated ones with flat index > 400 are raised to distinct values
      2.0, 2.25, ... handed out in seeded order, not index order -- the fallback must order by
      value before index (a peak's neighbours lose the mask and drop out or stay as zeros).
    extra_nans: that many further isolated ones (index > 400) become NaN.
    nan0: p[0] = NaN, the element whose key is ~0."""
    M = X * Y
    e = np.arange(M)
    p = np.where(e % SEL_THREADS < ROW_LANES * (K - 1), F32(1), F32(0)).astype(F32)
    ones = np.flatnonzero(p)
    if drop:
        p[ones[-drop:]] = 0
        ones = ones[:-drop]
    if peaks or extra_nans:
        rng = np.random.default_rng(seed)
        cells = _isolated_cells(ones[ones > 400], X, Y, peaks + extra_nans, rng)
        for j, c in enumerate(cells[:peaks]):
            p[c] = F32(2.0 + 0.25 * j)
        for c in cells[peaks:]:
            p[c] = np.nan
    if nan0:
        p[0] = np.nan
    return p.reshape(X, Y)


def zero_plateau_map(X: int, Y: int, K: int, peaks: int = 0, seed: int = 0, nan0: bool = False) -> np.ndarray:
    """The plateau at zero: -0.0 / +0.0 (seeded signs) where e % 1024 < 16 * (K - 3), -1.0
    elsewhere, optional positive peaks among the zeros.  Needs Y % 1024 == 0, so that the zeros
    are vertical stripes: a -1.0 cell next to a zero loses the mask and becomes -0.0, which
    ties with the plateau, and only with stripes do those cells stay within two rows (columns
    16 * (K - 3) and 1023 of each slice: rows K - 3 and 63).  K - 3 rows of zeros and those two
    make K - 1 rows above the threshold, which is then a -1.0: every zero is a candidate.  On a
    map whose width is no multiple of 1024 the -0.0 cells spread over more than K rows, the
    threshold becomes a zero of small index, and the list stays short."""
    assert Y % SEL_THREADS == 0 and K >= 4
    M = X * Y
    rng = np.random.default_rng(seed)
    e = np.arange(M)
    band = e % SEL_THREADS < ROW_LANES * (K - 3)
    p = np.where(band, np.where(rng.random(M) < 0.5, F32(-0.0), F32(0.0)), F32(-1)).astype(F32)
    if peaks:
        zeros = np.flatnonzero(band)
        for j, c in enumerate(_isolated_cells(zeros[zeros > 400], X, Y, peaks, rng)):
            p[c] = F32(0.5 + 0.125 * j)
    if nan0:
        p[0] = np.nan
    return p.reshape(X, Y)


def quantised_map(X: int, Y: int, seed: int, nan_at: int | None = None) -> np.ndarray:
    """floor(rand * 64) / 64: an ordinary map with ties; optionally one NaN at flat index nan_at."""
    p = (np.floor(np.random.default_rng(seed).random((X, Y)) * 64) / 64).astype(F32)
    if nan_at is not None:
        p.reshape(-1)[nan_at] = np.nan
    return p


# ---------------------------------------------------------------------------------------------
# the cases of test_gpu_nms_select.py, shared with the CPU tests that check their counts
# (X, Y, K): the over-capacity maps, each run with 5 peaks, with and without the NaN at 0.
# Only nms_select_kernel<32, false> can get there: C <= capacity_bound needs ceil(M / 1024) >= 18
# for more than 4096, the strip kernels stop at M = 16384, so 17408 < M <= 32512 and K >= 9.
OVER_CAPACITY = [(180, 180, 16), (160, 160, 12), (136, 129, 16), (12, 1500, 16)]
ZERO_PLATEAU = (12, 2048, 16)
# (X, Y, K, drop, expected C): the list exactly over, exactly at, and well within capacity
CAPACITY_EDGE = [(180, 180, 9, 0, 4097), (180, 180, 9, 1, 4096), (160, 160, 11, 0, 4001)]

# (name, X, Y, K, expected dispatch): the instantiations and boundaries no other test reaches
INSTANTIATIONS = [
    ("e2", 1, 1500, 5, ("select", 2, False)),
    ("e8", 4, 1500, 10, ("select", 8, False)),
    ("e16", 120, 129, 16, ("select", 16, False)),
    ("strip16", 128, 128, 16, ("select", 16, True)),        # strip length 16 ...
    ("strip17", 129, 128, 16, ("select", 32, False)),       # ... against 17
    ("y1024", 3, 1024, 10, ("select", 4, True)),            # Y = 1024: one thread row per map row ...
    ("y1025", 3, 1025, 10, ("select", 4, False)),           # ... against a row wider than the block
    ("select_max", 127, 256, 16, ("select", 32, False)),    # M = 32512: the select kernel's largest map
    ("topk_min", 533, 61, 16, ("topk",)),                   # M = 32513: the first for the K-round kernel
    ("topk_max", 192, 193, 16, ("topk",)),                  # M = 37056: the largest map accepted
]
REJECTED = (193, 193, 16)                                   # M = 37249: FVP_ERR_SHAPE


def over_capacity_map(X, Y, K, nan0, extra_nans=0):
    return adversarial_map(X, Y, K, nan0=nan0, peaks=5, seed=X * Y + K, extra_nans=extra_nans)


def instantiation_map(X, Y):
    """A quantised random map with one NaN away from index 0 (two thirds into the map)."""
    return quantised_map(X, Y, seed=X * 4099 + Y, nan_at=(2 * X * Y) // 3)


def mixed_batch(K: int = 9) -> np.ndarray:
    """[3, 180, 180]: over capacity with a NaN at 0 / an ordinary quantised map / exactly at
    capacity (C = 4096)."""
    over = adversarial_map(180, 180, K, nan0=True, peaks=0 if K == 9 else 5, seed=K)
    at_cap = adversarial_map(180, 180, K, drop=capacity_bound(180 * 180, K) - SEL_CAP)
    return np.stack([over, quantised_map(180, 180, seed=77), at_cap])
