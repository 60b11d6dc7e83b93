"""Float64 reference, a derived error bound and an fp32 emulation for the one-launch 1-D net
kernel of csrc/fvp_c2c.hip (c2c_net_kernel<4> / <8>, fvp_conv1d_net) -- numpy only.
tests/test_c2c_ref.py pins this file on the CPU, tests/test_gpu_c2c_ops.py holds the kernel
to it op by op.

Program.  An op is 12 ints (C2COp): kind (0 conv, 1 ConvTranspose1d(2, 2), 2 max_pool1d(2, 2)),
cin, cout, k, L (input length), src, dst, res_pre, res_post (buffer ids, -1 none), relu, w_off
(params offset: W [cin][k][cout], then scale [cout], shift [cout]) and cic (input channels per
staged weight chunk).  Activations live in nbuf buffers of `slot` floats as rows
[3 zeros, L values, 3 zeros] (pitch L + 6); buffer 0 receives the input, its channels padded
to a multiple of 4 with zero rows.

    conv   out[co][l]      = act(scale[co] sum_{ci,t} W[ci][t][co] in[ci][l + t - p] + shift[co]
                                 (+ res_pre[co][l])) (+ res_post[co][l]),   p = (k - 1) / 2
    convt  out[co][2l + d] = the same with the one product W[ci][d][co] in[ci][l] per channel
    pool   out[c][l]       = nanmax(in[c][2l], in[c][2l + 1])   (b > a or b != b ? b : a)

run_program() interprets a program in float64 on flat buffers that start as NaN: only what the
kernel writes is written (the input's cin4 x (L0 + 6), each conv's valid region and its two
pads, each pool's C x (L / 2 + 6)), and a conv reads its taps from the row as it is held, pads
included.  A program whose correctness leans on an unwritten pad or on a stale row therefore
gives NaN or a wrong value here, on the CPU.

Bound.  op_reference() evaluates one op in float64 from given fp32 inputs.  With K products per
output (K = cin k for conv, cin for convt, cin counting the zero-padded channels),
Babs = sum |W| |in| over the same products and u = 2^-24,

    tol = (K + 8) u (|scale| Babs + |shift| + |res_pre| + |res_post|)

the first-order worst case of K roundings of partial sums in any order (each partial sum is
at most Babs; the K product roundings together add at most u Babs, inside the + 8 with the at
most 3 split adds and the epilogue's at most 4 roundings).  ReLU is 1-Lipschitz.  Derived, not
measured.  Pool and the final copy-out are exact: tol is None and the comparison is bit for
bit (same_bits(): NaN equals NaN).

Emulation.  emulate() evaluates the op in float32 as the kernel does (-ffp-contract=off: the
product rounded, then the sum rounded): the weight chunks of cic channels in order; within a
chunk split ks of KS takes the channel steps U ks, U ks + U KS, ... (U = 2 channels for
k >= 5, else 4), channels then taps within a step; the KS partial sums added in split order;
the epilogue as written -- and takes a planted fault (FAULTS).  It shows on the CPU that a
correct fp32 evaluation stays inside tol and that each fault leaves it; on the GPU the
criterion is tol, not equality with emulate().
"""
import numpy as np

U = 2.0 ** -24
PAD = 3
THREADS = 1024
STAGE = 4 * THREADS   # floats per stage: one float4 load per thread
MAX_STAGE = 3
LDS_LIMIT = 160 * 1024

KIND, CIN, COUT, K, L, SRC, DST, RES_PRE, RES_POST, RELU, W_OFF, CIC = range(12)
CONV, CONVT, POOL = 0, 1, 2

FAULTS = ("chunk", "split", "tap", "parity", "ragged", "lpad", "rpad", "pre-late", "post-early", "neighbour",
          "pool-first", "pool-finite")
STALE = 1.0  # what a stale pad holds under the lpad / rpad faults


# ---- the kernel's plan of one op, restated ---------------------------------------------------
def out_len(op):
    return 2 * op[L] if op[KIND] == CONVT else op[L] // 2 if op[KIND] == POOL else op[L]


def splits(items, cic):
    """c2c_splits: threads that share one item's input channels."""
    ks = 1
    while ks < 4 and items * ks * 2 <= THREADS and cic >= 4 * ks * 2:
        ks *= 2
    return ks


def chunking(op):
    """The channels of each staged weight chunk (chunk c holds nci[c] k cout floats)."""
    n = -(-op[CIN] // op[CIC])
    return tuple(op[CIC] if c + 1 < n else op[CIN] - c * op[CIC] for c in range(n))


def nstage(wchunk):
    return wchunk // STAGE


def groups(op, lg):
    """(position groups, thread items = cout x groups, Lout % lg)."""
    lo = out_len(op)
    ng = -(-lo // lg)
    return ng, op[COUT] * ng, lo % lg


def lds_bytes(slot, nbuf, wchunk, lg):
    return 4 * (2 * wchunk + THREADS * lg + slot * nbuf)


def weights(op, params):
    """(W [cin][k][cout], scale [cout], shift [cout]) of a conv op, as stored (float32)."""
    p = np.asarray(params, np.float32)
    n = op[CIN] * op[K] * op[COUT]
    o = op[W_OFF]
    return p[o:o + n].reshape(op[CIN], op[K], op[COUT]), p[o + n:o + n + op[COUT]], p[o + n + op[COUT]:o + n + 2 * op[COUT]]


# ---- float64 ---------------------------------------------------------------------------------
def nanmax(a, b):
    return np.where((b > a) | (b != b), b, a)


def same_bits(a, b):
    """Equal float32 arrays, NaN equal to NaN, -0 different from +0."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


def _padded(x):
    """[N][C][L] -> rows [N][C][L + 6] with zero pads."""
    return np.pad(x, ((0, 0), (0, 0), (PAD, PAD)))


def _products(op, w, rows):
    """sum over (ci, t) of w[ci][t][co] rows[ci][...] from padded rows [N][cin][L + 6]."""
    n, lin = rows.shape[0], op[L]
    if op[KIND] == CONVT:
        out = np.zeros((n, op[COUT], 2 * lin), rows.dtype)
        for d in (0, 1):
            out[:, :, d::2] = np.einsum("ic,nil->ncl", w[:, d, :], rows[:, :, PAD:PAD + lin])
        return out
    p = (op[K] - 1) // 2
    out = np.zeros((n, op[COUT], lin), rows.dtype)
    for t in range(op[K]):
        out += np.einsum("ic,nil->ncl", w[:, t, :], rows[:, :, PAD + t - p:PAD + t - p + lin])
    return out


def _epilogue(acc, sc, sh, relu, pre, post):
    v = acc * sc[None, :, None] + sh[None, :, None]
    if pre is not None:
        v = v + pre
    if relu:
        v = np.where(v < 0, 0, v)  # reluf: NaN stays
    if post is not None:
        v = v + post
    return v


def op_reference(op, params, src, res_pre=None, res_post=None):
    """One op in float64 from fp32 inputs [N][C][L]: (ref, tol), both float64 [N][cout][Lout];
    tol None for a pool (exact)."""
    f64 = np.float64
    src = np.asarray(src, np.float32).astype(f64)
    if op[KIND] == POOL:
        lo = op[L] // 2
        return nanmax(src[:, :, 0:2 * lo:2], src[:, :, 1:2 * lo:2]), None
    w, sc, sh = (a.astype(f64) for a in weights(op, params))
    pre = None if res_pre is None else np.asarray(res_pre, np.float32).astype(f64)
    post = None if res_post is None else np.asarray(res_post, np.float32).astype(f64)
    ref = _epilogue(_products(op, w, _padded(src)), sc, sh, op[RELU], pre, post)
    t = np.abs(sc)[None, :, None] * _products(op, np.abs(w), _padded(np.abs(src))) + np.abs(sh)[None, :, None]
    for r in (pre, post):
        if r is not None:
            t = t + np.abs(r)
    kk = op[CIN] * (1 if op[KIND] == CONVT else op[K])
    return ref, (kk + 8) * U * t


def run_program(ops, params, x, *, slot, nbuf, upto=None, inputs=None, fetch=None, trace=None):
    """The program in float64 on the kernel's buffer layout.  x [N][cin0][L0]; `upto`: run only
    the first `upto` ops; `inputs`: {buffer: [N][C][L]} rows written (with zero pads) before
    the first op, standing for earlier work; `fetch`: (buffer, C, L) to return instead of the
    last op's dst; `trace`: a list that receives per op (src, res_pre, res_post, out), the
    valid regions at the time the op ran.
    -> [N][C][L] float64, the valid region as the kernel's copy-out reads it."""
    x = np.asarray(x, np.float64)
    n, cin0, l0 = x.shape
    act = np.full((n, nbuf, slot), np.nan)

    def rows(b, c, ln):
        assert 0 <= b < nbuf and c * (ln + 2 * PAD) <= slot, "row block outside its buffer"
        return act[:, b, :c * (ln + 2 * PAD)].reshape(n, c, ln + 2 * PAD)

    cin4 = (cin0 + 3) & ~3
    r = rows(0, cin4, l0)
    r[:] = 0.0
    r[:, :cin0, PAD:PAD + l0] = x
    for b, v in (inputs or {}).items():
        v = np.asarray(v, np.float64)
        rows(b, v.shape[1], v.shape[2])[:] = _padded(v)
    ops = [tuple(int(v) for v in o) for o in ops]
    run = ops if upto is None else ops[:upto]
    for op in run:
        lo = out_len(op)
        src = rows(op[SRC], op[CIN], op[L])
        assert op[DST] != op[SRC]
        if op[KIND] == POOL:
            out = rows(op[DST], op[CIN], lo)  # written whole: pads included
            val = nanmax(src[:, :, PAD:PAD + 2 * lo:2], src[:, :, PAD + 1:PAD + 2 * lo:2])
            out[:] = 0.0
            out[:, :, PAD:PAD + lo] = val
            if trace is not None:
                trace.append((src[:, :, PAD:PAD + op[L]].copy(), None, None, val.copy()))
            continue
        w, sc, sh = (a.astype(np.float64) for a in weights(op, params))
        pre = rows(op[RES_PRE], op[COUT], lo)[:, :, PAD:PAD + lo] if op[RES_PRE] >= 0 else None
        post = rows(op[RES_POST], op[COUT], lo)[:, :, PAD:PAD + lo] if op[RES_POST] >= 0 else None
        val = _epilogue(_products(op, w, src), sc, sh, op[RELU], pre, post)
        if trace is not None:
            trace.append((src[:, :, PAD:PAD + op[L]].copy(), None if pre is None else pre.copy(),
                          None if post is None else post.copy(), val.copy()))
        out = rows(op[DST], op[COUT], lo)
        out[:, :, PAD:PAD + lo] = val
        out[:, :, :PAD] = 0.0          # the pads the kernel writes; nothing else of the slot
        out[:, :, PAD + lo:] = 0.0
    if fetch is None:
        fetch = (run[-1][DST], run[-1][CIN] if run[-1][KIND] == POOL else run[-1][COUT], out_len(run[-1]))
    b, c, ln = fetch
    return rows(b, c, ln)[:, :, PAD:PAD + ln].copy()


# ---- fp32 emulation --------------------------------------------------------------------------
def applicable(fault, op, lg):
    """Whether a planted fault changes what emulate() computes for this op at this lg."""
    if op[KIND] == POOL:
        return fault in ("pool-first", "pool-finite")
    ng, items, rag = groups(op, lg)
    return {"chunk": len(chunking(op)) > 1, "split": splits(items, op[CIC]) > 1, "tap": op[KIND] == CONV,
            "parity": op[KIND] == CONVT, "ragged": rag != 0, "lpad": op[KIND] == CONV and op[K] >= 3,
            "rpad": op[KIND] == CONV and op[K] >= 3, "pre-late": op[RES_PRE] >= 0 and bool(op[RELU]),
            "post-early": op[RES_POST] >= 0 and bool(op[RELU]), "neighbour": op[COUT] > 1,
            "pool-first": False, "pool-finite": False}[fault]


def emulate(op, params, src, res_pre=None, res_post=None, *, lg, fault=None):
    """The op in float32 in the kernel's order: float32 [N][cout][Lout] (NaN where a fault
    leaves an element unwritten).  Faults:
      chunk       the last weight chunk is not added
      split       the last split's partial sum is not added
      tap         the centre tap reads one position to the right
      parity      (convt) the two taps change places
      ragged      the positions past the last full group of lg are not written
      lpad, rpad  the row's left / right pad holds STALE where it should hold zeros
      pre-late    res_pre is added after the ReLU
      post-early  res_post is added before the ReLU
      neighbour   scale and shift of channel co + 1
      pool-first  the window's first element
      pool-finite the larger element, a NaN only where both are (fmax)"""
    assert fault is None or fault in FAULTS, fault
    f32 = np.float32
    src = np.asarray(src, f32)
    n, lin, lo = src.shape[0], op[L], out_len(op)
    if op[KIND] == POOL:
        a, b = src[:, :, 0:2 * lo:2], src[:, :, 1:2 * lo:2]
        return a.copy() if fault == "pool-first" else np.fmax(a, b) if fault == "pool-finite" else nanmax(a, b)
    w, sc, sh = weights(op, params)
    rows = np.zeros((n, op[CIN], lin + 2 * PAD + 1), f32)  # (+ 1: the tap fault's reach)
    rows[:, :, PAD:PAD + lin] = src
    if fault == "lpad":
        rows[:, :, :PAD] = STALE
    if fault == "rpad":
        rows[:, :, PAD + lin:] = STALE
    ct = op[KIND] == CONVT
    k, p = op[K], 0 if ct else (op[K] - 1) // 2
    ng, items, _ = groups(op, lg)
    nks = splits(items, op[CIC])
    step = 2 if (not ct and k >= 5) else 4
    nci = chunking(op)
    acc = [np.zeros((n, op[COUT], lo), f32) for _ in range(nks)]
    for c, nc in enumerate(nci):
        if fault == "chunk" and c == len(nci) - 1:
            continue
        for ks in range(nks):
            a = acc[ks]
            for ci in range(step * ks, nc, step * nks):
                for u in range(step):
                    ch = c * op[CIC] + ci + u
                    for t in range(k):
                        wv = w[ch, t, :][None, :, None]
                        if ct:
                            d = 1 - t if fault == "parity" else t
                            a[:, :, d::2] = a[:, :, d::2] + wv * rows[:, ch, None, PAD:PAD + lin]
                        else:
                            o = PAD + t - p + (1 if fault == "tap" and t == p else 0)
                            a[...] = a + wv * rows[:, ch, None, o:o + lo]
    v = acc[0]
    for q in range(1, nks):
        if not (fault == "split" and q == nks - 1):
            v = v + acc[q]
    if fault == "neighbour":
        sc, sh = np.roll(sc, -1), np.roll(sh, -1)
    pre = None if res_pre is None else np.asarray(res_pre, f32)
    post = None if res_post is None else np.asarray(res_post, f32)
    v = v * sc[None, :, None] + sh[None, :, None]
    if pre is not None and fault != "pre-late":
        v = v + pre
    if post is not None and fault == "post-early":
        v = v + post
    if op[RELU]:
        v = np.where(v < 0, f32(0), v)
    if pre is not None and fault == "pre-late":
        v = v + pre
    if post is not None and fault != "post-early":
        v = v + post
    assert v.dtype == f32
    if fault == "ragged":
        v = v.copy()
        v[:, :, lo // lg * lg:] = np.nan
    return v


def within(got, ref, tol):
    """Largest |got - ref| / tol (0 where both are 0; inf where got is not finite or the
    shapes differ) -- inside the bound when <= 1."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape or not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    return float(r.max()) if r.size else 0.0


def _clean(a):
    return None if a is None else np.where(np.isfinite(a), a, np.float32(0)).astype(np.float32)


def check_op(op, params, src, res_pre, res_post, got, lg):
    """Holds one op's fp32 output `got` to its reference given the fp32 inputs it read;
    -> the largest error / tol (0 for a pool); AssertionError outside the bound.
    Non-finite inputs: an output whose receptive field (taps and residuals) holds a NaN or an
    Inf, or that overflows fp32 in emulate(), must equal emulate() bit for bit -- NaN, +-Inf
    or the 0 a ReLU makes of -Inf, none of which depends on the summation order; every other
    output must be within tol of the reference computed without the non-finite elements'
    contributions."""
    got = np.asarray(got, np.float32)
    src = np.asarray(src, np.float32)
    if op[KIND] == POOL:
        ref = op_reference(op, params, src)[0].astype(np.float32)
        assert same_bits(got, ref), "pool differs from nanmax over its windows"
        return 0.0
    ins = [src] + [np.asarray(r, np.float32) for r in (res_pre, res_post) if r is not None]
    mask = np.zeros(got.shape, bool)
    if not all(np.isfinite(a).all() and np.abs(a).max(initial=0) < 1e30 for a in ins):
        ones = np.concatenate([np.ones((op[CIN] * op[K] + 1) * op[COUT], np.float32), np.zeros(op[COUT], np.float32)])
        o1 = list(op)
        o1[W_OFF], o1[RELU] = 0, 0
        bad = [None if a is None else (~np.isfinite(np.asarray(a, np.float32))).astype(np.float32)
               for a in (src, res_pre, res_post)]
        em = emulate(op, params, src, res_pre, res_post, lg=lg)
        mask = (op_reference(o1, ones, *bad)[0] > 0) | ~np.isfinite(em)
        assert same_bits(got[mask], em[mask]), "non-finite outputs differ from the fp32 evaluation"
    ref, tol = op_reference(op, params, _clean(src), _clean(res_pre), _clean(res_post))
    assert got.shape == ref.shape and np.isfinite(got[~mask]).all(), "non-finite output from finite inputs"
    ratio = within(np.where(mask, 0, got), np.where(mask, 0, ref), tol)
    assert ratio <= 1.0, f"error {ratio:.3g} x tol"
    return ratio
