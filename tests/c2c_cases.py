"""The case list of the one-launch 1-D net kernel (csrc/fvp_c2c.hip) for tests/test_c2c_ref.py
(CPU) and tests/test_gpu_c2c_ops.py (GPU).  Every program is built with fvp.cnn.Net1D's own
builder methods (conv / pool / _buf / _release / _finish) on small seeded nn.Conv1d,
nn.ConvTranspose1d and nn.BatchNorm1d modules (fvp.synthetic.seeded_state_dict), so the
buffers, offsets and chunk sizes are the host compiler's, not a restatement's.

A case is a short list of steps over named activations ("x" is the input):
    ("conv" | "convt", name, src, {cout, k, relu, pre, post, bn, neg, huge, pos, cancel})
    ("pool", name, src)        ("free", name, ...)
`pre` / `post` name the residual activations, `neg` flips the sign of every other channel's
BatchNorm gamma (negative scales), `huge` gives a conv without BatchNorm a bias of 1e30.

Which dimensions are crossed.  The kernel's code takes a decision in four places, and the
list crosses the classes within each place in full (coverage(), asserted by the CPU test):
  products   c2c_products<K, CT, LG> and its two loops: (k | convt) x lg x KS x chunk count
             class (1, 2, an odd count >= 3 whose last chunk is shorter than cic) -- these
             share the unrolled body, the channel-step stride and the chunk loop;
  staging    load_chunk / store_chunk: nstage x how the first chunk fills its loads (exactly
             wchunk floats, a few float4s, a ragged count) -- nothing else reads nstage;
  store      the epilogue's position guard and pad writes: lg x Lout % lg, and Lout < lg;
  epilogue   (conv | convt) x (none, relu, pre, post, pre-relu-post, pre-relu, relu-post,
             negative scale).
The four places do not share state (the accumulators reach the epilogue as LG registers
whatever produced them), so the list crosses within a place and not between places.
KS < 4 is reached both ways: by cic (4 gives 1, 8 or 12 give 2) and by the item count.
"""
import collections
import functools
import zlib

import numpy as np

import c2c_ref as R

Case = collections.namedtuple("Case", "name group cin0 L0 wchunk steps net")
LGS = (4, 8)
KOPS = (1, 3, 5, 7, "t")
NCLASSES = ("1", "2", "odd")
EPILOGUES = ("none", "relu", "pre", "post", "pre-relu-post", "pre-relu", "relu-post", "neg")
FILLS = ("exact", "few", "ragged")


def _case(name, group, cin0, L0, steps, wchunk=12288, net=None):
    return Case(name, group, cin0, L0, wchunk, tuple(steps), net)


def _conv(name, src, cout, k, **kw):
    return ("conv", name, src, dict(cout=cout, k=k, **kw))


def _convt(name, src, cout, **kw):
    return ("convt", name, src, dict(cout=cout, k=2, **kw))


# ---- the products search ---------------------------------------------------------------------
def _plan(kop, cin, cout, ln, wchunk):
    """The op Net1D.conv would append for a first conv on a cin-channel input (cin % 4 == 0)."""
    k = 2 if kop == "t" else kop
    cic = min(cin, (wchunk // (k * cout)) // 4 * 4)
    if cic < 4:
        return None
    return (1 if kop == "t" else 0, cin, cout, k, ln, 0, 1, -1, -1, 1, 0, cic)


def nchunk_class(op):
    nci = R.chunking(op)
    if len(nci) <= 2:
        return str(len(nci))
    return "odd" if len(nci) % 2 == 1 and nci[-1] < op[R.CIC] else None


def split_way(op, lg):
    """(KS, what limits it): "cic", "items", "both" or "-" (KS = 4)."""
    items = R.groups(op, lg)[1]
    kc = 1 if op[R.CIC] < 8 else 2 if op[R.CIC] < 16 else 4
    ki = 1 if items > 512 else 2 if items > 256 else 4
    ks = min(kc, ki)
    assert ks == R.splits(items, op[R.CIC])
    return ks, "-" if ks == 4 else "both" if kc == ki else "cic" if kc < ki else "items"


def _fits(op, lg, wchunk):
    lo = R.out_len(op)
    slot = max(op[R.CIN] * (op[R.L] + 6), op[R.COUT] * (lo + 6)) + 16
    return R.groups(op, lg)[1] <= R.THREADS and R.lds_bytes(slot, 2, wchunk, lg) <= R.LDS_LIMIT


@functools.lru_cache(maxsize=None)
def product_cases():
    """Per (k | convt, lg, KS, chunk count class): the cheapest single op (by its products)
    on a cin-channel input that reaches the class -- {class: Case}."""
    best = {}
    for wchunk in (4096, 8192, 12288):
        for kop in KOPS:
            for cout in (1, 4, 5, 8, 16, 32, 33, 64, 128, 160, 256):
                for cin in (4, 8, 12, 16, 20, 24, 28, 36, 40, 72, 136):
                    for ln in (1, 2, 3, 5, 6, 8, 9, 12, 17, 20, 33, 40):
                        op = _plan(kop, cin, cout, ln, wchunk)
                        nc = op and nchunk_class(op)
                        if not nc:
                            continue
                        cost = cin * op[R.K] * cout * R.out_len(op)
                        for lg in LGS:
                            if not _fits(op, lg, wchunk):
                                continue
                            cls = (kop, lg, split_way(op, lg)[0], nc)
                            if cls not in best or cost < best[cls][0]:
                                best[cls] = (cost, cin, cout, ln, wchunk)
    out = {}
    for cls, (_, cin, cout, ln, wchunk) in sorted(best.items(), key=str):
        kop, lg, ks, nc = cls
        step = _convt("y", "x", cout) if kop == "t" else _conv("y", "x", cout, kop)  # linear: nothing hides in a ReLU
        out[cls] = _case(f"prod-k{kop}-lg{lg}-ks{ks}-n{nc}", "products", cin, ln, [step], wchunk)
    return out


# ---- the hand-written cases --------------------------------------------------------------------
def _residual_steps(kop, pre, post, **kw):
    """x (-> pool for convt, whose residuals have twice its input's length) -> the op, with
    its residuals made by k = 1 convs of x."""
    steps = []
    if pre:
        steps.append(_conv("rp", "x", 8, 1))
    if post:
        steps.append(_conv("rq", "x", 8, 1))
    kw = dict(kw, pre="rp" if pre else None, post="rq" if post else None)
    if kop == "t":
        return steps + [("pool", "p", "x"), _convt("y", "p", 8, **kw)]
    return steps + [_conv("y", "x", 8, kop, **kw)]


def single_cases():
    c = []
    # staging: nstage x the first chunk's fill
    for wchunk in (4096, 8192, 12288):
        exact = {4096: (64, 1, 128), 8192: (64, 1, 128), 12288: (64, 3, 128)}[wchunk]  # (cin, k, cout)
        c.append(_case(f"stage{wchunk}-exact", "staging", exact[0], 5, [_conv("y", "x", exact[2], exact[1], relu=True)],
                       wchunk))
        c.append(_case(f"stage{wchunk}-few", "staging", 4, 5, [_conv("y", "x", 1, 1)], wchunk))
        c.append(_case(f"stage{wchunk}-ragged", "staging", 16, 5, [_conv("y", "x", 5, 3, relu=True)], wchunk))
    # store: every Lout % lg of both lg, Lout < lg, convt from L = 1
    for ln in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16):
        c.append(_case(f"len{ln}-k3", "store", 4, ln, [_conv("y", "x", 5, 3, relu=True)]))
    for ln in (1, 2, 3, 4, 5, 8):
        c.append(_case(f"len{ln}-convt", "store", 4, ln, [_convt("y", "x", 5, relu=True)]))
    c.append(_case("len3-k7", "store", 4, 3, [_conv("y", "x", 5, 7)]))
    # items exactly 1024 (lg 4: 128 x 8 groups; lg 8: 128 x 8 groups of the longer row)
    c.append(_case("items1024-lg4", "items", 8, 32, [_conv("y", "x", 128, 3, relu=True)], 4096))
    c.append(_case("items1024-lg8", "items", 8, 64, [_conv("y", "x", 128, 3, relu=True)], 4096))
    # channels: the input's zero rows up to a multiple of 4; output channel counts off 16
    for cin0, cout in ((1, 1), (3, 5), (4, 33), (5, 5), (15, 33)):
        c.append(_case(f"chan{cin0}-{cout}", "channels", cin0, 6, [_conv("y", "x", cout, 7, relu=True)]))
    # epilogues
    for kop in (3, "t"):
        for name, pre, post, kw in (("none", 0, 0, {}), ("relu", 0, 0, dict(relu=True)), ("pre", 1, 0, {}),
                                    ("post", 0, 1, {}), ("pre-relu-post", 1, 1, dict(relu=True)),
                                    ("pre-relu", 1, 0, dict(relu=True)), ("relu-post", 0, 1, dict(relu=True)),
                                    ("neg", 0, 0, dict(relu=True, neg=True))):
            c.append(_case(f"epi-k{kop}-{name}", "epilogue", 4, 10, _residual_steps(kop, pre, post, **kw)))
    # k = 5 and 7 with res_pre, two chunks, KS 1 (cic 4) and 2 (cic 8 / 12)
    for k, cout, cin in ((7, 64, 16), (7, 128, 8), (5, 64, 24), (5, 128, 8)):
        c.append(_case(f"pre-k{k}-c{cout}", "wide-pre", cin, 6,
                       [_conv("rp", "x", cout, 1), _conv("y", "x", cout, k, relu=True, pre="rp")], 4096))
    # pool: even and odd (floor) lengths, L = 2, a channel count off 4
    for ln in (8, 7, 2, 3):
        c.append(_case(f"pool{ln}", "pool", 5, ln, [("pool", "p", "x"), _conv("y", "p", 4, 1)]))
    c.append(_case("pool-c5", "pool", 4, 9, [_conv("a", "x", 5, 1), ("pool", "y", "a")]))
    return c


def reuse_cases():
    """A buffer holds a [32][16] activation of about 1e30, is released, is rewritten as
    [12][8] by a conv, a transposed conv or a pool, and a k = 7 conv reads the new rows, pads
    included (reused_buffer() tells which buffer it is; the tests assert the reuse)."""
    big = _conv("big", "x", 32, 1, bn=False, huge=True)
    tail = [_conv("y", "b", 5, 7, relu=True)]
    return [
        _case("reuse-conv", "reuse", 4, 16, [big, ("pool", "p", "x"), ("free", "big"), _conv("b", "p", 12, 3, relu=True)]
              + tail),
        _case("reuse-convt", "reuse", 4, 16, [big, ("pool", "p", "x"), ("pool", "q", "p"), ("free", "big"),
                                              _convt("b", "q", 12, relu=True)] + tail),
        _case("reuse-pool", "reuse", 4, 16, [big, _conv("a", "x", 12, 1), ("free", "big"), ("pool", "b", "a")] + tail),
    ]


def nonfinite_cases():
    """Single ops whose inputs nonfinite_inputs() plants NaN / Inf into: each kernel size with
    input channel 1's weights made positive (`pos`); a conv with both residuals, each holding
    one NaN born in its k = 1 conv (`cancel`: weights +40 and -40 on two inputs of 1e37, whose
    products overflow to +Inf and -Inf); a pool."""
    c = [_case(f"nf-k{kop}", "nonfinite", 4, 10,
               [_convt("y", "x", 8, relu=True, pos=1) if kop == "t" else _conv("y", "x", 8, kop, relu=True, pos=1)])
         for kop in KOPS]
    c.append(_case("nf-res", "nonfinite", 4, 10, [_conv("rp", "x", 8, 1, bn=False, cancel=(2, 0, 1)),
                                                  _conv("rq", "x", 8, 1, bn=False, cancel=(5, 2, 3)),
                                                  _conv("y", "x", 8, 3, relu=True, pre="rp", post="rq")]))
    c.append(_case("nf-pool", "nonfinite", 4, 10, [("pool", "p", "x"), _conv("y", "p", 8, 1)]))
    return c


NF_AT = (1, 4)        # (channel, position) of the planted NaN / +Inf / -Inf of the nf-k cases
NF_RES = ((2, 4), (5, 7))  # (channel, position) of the NaN in res_pre and in res_post of nf-res


def nonfinite_inputs(case):
    """nf-k*: column 0 holds a NaN at NF_AT, column 1 +Inf, column 2 -Inf.  nf-res: 1e37 at the
    two inputs of each `cancel` pair, at the positions of NF_RES.  nf-pool (column 0): a NaN in
    the first slot of window 1 of channel 1 and in the second slot of window 2 of channel 2."""
    x = inputs(case)
    if case.name == "nf-res":
        x[:, 0:2, NF_RES[0][1]] = 1e37
        x[:, 2:4, NF_RES[1][1]] = 1e37
    elif case.name == "nf-pool":
        x[0, 1, 2] = x[0, 2, 5] = np.nan
    else:
        for col, v in enumerate((np.nan, np.inf, -np.inf)):
            x[col][NF_AT] = v
    return x


def net_cases():
    return [_case(f"net{cin0}-{cout}-z{z}", "net", cin0, z, (), net=(cin0, cout))
            for cin0, cout, z in ((15, 1, 4), (15, 1, 20), (15, 1, 32), (15, 1, 64), (17, 5, 8))]


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(list(product_cases().values()) + single_cases() + reuse_cases() + nonfinite_cases() + net_cases())


# ---- building ----------------------------------------------------------------------------------
def seed(case):
    return zlib.crc32(case.name.encode()) & 0x7FFFFFFF


def net_module(cin0, cout):
    import cnn_arch
    from fvp import synthetic

    m = cnn_arch.C2CNet(cin0, cout).eval()
    m.load_state_dict(synthetic.seeded_state_dict(m, 14))
    return m


def _module(case, i, kind, cin, kw):
    import torch
    import torch.nn as nn

    from fvp import synthetic

    conv = nn.ConvTranspose1d(cin, kw["cout"], 2, stride=2) if kind == "convt" else \
        nn.Conv1d(cin, kw["cout"], kw["k"], padding=(kw["k"] - 1) // 2)
    seq = nn.Sequential(conv, nn.BatchNorm1d(kw["cout"])).eval()
    seq.load_state_dict(synthetic.seeded_state_dict(seq, seed(case) + i))
    with torch.no_grad():
        if kw.get("neg"):
            seq[1].weight[0::2] *= -1.0
        if kw.get("huge"):
            seq[0].bias.fill_(1e30)
        if kw.get("pos") is not None:
            w = seq[0].weight[kw["pos"]] if kind == "convt" else seq[0].weight[:, kw["pos"]]
            w.abs_()
        if kw.get("cancel"):
            co, c1, c2 = kw["cancel"]
            seq[0].weight[co, c1, 0], seq[0].weight[co, c2, 0] = 40.0, -40.0
    return seq[0], seq[1] if kw.get("bn", True) else None


_BUILT = {}


def build(case, lg, device="cpu"):
    """The case's Net1D at `lg` positions per item (prog / param tensors on `device`), or None
    where the case cannot run at that lg (more than 1,024 items, or LDS).  Built once."""
    key = (case.name, lg, str(device))
    if key not in _BUILT:
        _BUILT[key] = _build(case, lg, device)
    return _BUILT[key]


def _build(case, lg, device):
    from fvp.cnn import Net1D

    if case.net:
        m = net_module(*case.net).to(device)
        for wchunk in Net1D.W_CHUNKS:
            n = Net1D._build(m, case.cin0, case.L0, wchunk)
            if n and n.lg != lg:
                n = n._finish(n.cin0, n.L0, n.out_buf, n.cout, n.Lout, device, lg=lg)
            if n is not False:
                return n
        return None
    n = Net1D(case.wchunk)
    cin4 = (case.cin0 + 3) // 4 * 4
    bufs = {"x": (n._buf(cin4, case.L0), cin4, case.L0)}
    last = None
    for i, s in enumerate(case.steps):
        if s[0] == "free":
            n._release(*[bufs[b][0] for b in s[1:]])
        elif s[0] == "pool":
            bufs[s[1]] = n.pool(*bufs[s[2]])
            last = s[1]
        else:
            kind, name, src, kw = s
            b, C, L = bufs[src]
            conv, bn = _module(case, i, kind, case.cin0 if src == "x" else C, kw)
            res = [bufs[kw[r]][0] if kw.get(r) else None for r in ("pre", "post")]
            bufs[name] = n.conv(conv, bn, b, C, L, bool(kw.get("relu")), res[0], res[1])
            for r in ("pre", "post"):
                assert not kw.get(r) or bufs[kw[r]][1:] == bufs[name][1:], "residual shape"
            last = name
    n.bufs = bufs
    return n._finish(case.cin0, case.L0, *bufs[last], device, lg=lg) or None


def legal_lgs(case):
    return tuple(lg for lg in LGS if build(case, lg) is not None)


def inputs(case, ncols=3):
    """[ncols][cin0][L0] float32, magnitudes in (0.5, 1.5) with random signs, every column
    different."""
    rng = np.random.default_rng(seed(case) + 7)
    x = rng.uniform(0.5, 1.5, (ncols, case.cin0, case.L0)) * rng.choice((-1.0, 1.0), (ncols, case.cin0, case.L0))
    return x.astype(np.float32)


def reused_buffer(net):
    """reuse cases: (the buffer "big" was in, the buffer "b" is in)."""
    return net.bufs["big"][0], net.bufs["b"][0]


# ---- coverage ------------------------------------------------------------------------------------
def epilogue_class(op, params):
    neg = bool((R.weights(op, params)[1] < 0).any())
    key = (op[R.RES_PRE] >= 0, bool(op[R.RELU]), op[R.RES_POST] >= 0)
    if neg and key == (False, True, False):
        return "neg"
    return {(False, False, False): "none", (False, True, False): "relu", (True, False, False): "pre",
            (False, False, True): "post", (True, True, True): "pre-relu-post", (True, True, False): "pre-relu",
            (False, True, True): "relu-post"}.get(key)


def fill_class(op, wchunk):
    f = R.chunking(op)[0] * op[R.K] * op[R.COUT]
    return "exact" if f == wchunk else "few" if f <= 16 else "ragged" if (f // 4) % R.THREADS else None


def coverage():
    """The classes the list reaches: {"products": {(k | "t", lg, KS, chunk class)},
    "staging": {(nstage, fill)}, "store": {(lg, Lout % lg)} and {(lg, "short")} for Lout < lg,
    "epilogue": {(conv | convt, epilogue)}, "ways": {(KS, "cic" | "items")}}."""
    cov = collections.defaultdict(set)
    for case in all_cases():
        for lg in legal_lgs(case):
            n = build(case, lg)
            par = n.param.numpy()
            for op in n.ops:
                if op[R.KIND] == R.POOL:
                    continue
                kop = "t" if op[R.KIND] == R.CONVT else op[R.K]
                ks, way = split_way(op, lg)
                if nchunk_class(op):
                    cov["products"].add((kop, lg, ks, nchunk_class(op)))
                cov["ways"].add((ks, way))
                if fill_class(op, n.wchunk):
                    cov["staging"].add((R.nstage(n.wchunk), fill_class(op, n.wchunk)))
                lo = R.out_len(op)
                cov["store"].add((lg, lo % lg))
                if lo < lg:
                    cov["store"].add((lg, "short"))
                if epilogue_class(op, par):
                    cov["epilogue"].add(("convt" if kop == "t" else "conv", epilogue_class(op, par)))
    return cov
