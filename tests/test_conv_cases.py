"""Coverage of tests/conv_cases.py (no GPU): the table holds a full and a ragged case for each
of the 46 kernel instantiations conv_launch can start, none left out, and the route of every
case -- fvp.cnn.conv_route on the ConvLayer the GPU test builds, so with the flags, algo and
workspace size ConvLayer.__call__ passes -- is the variant the case was built for."""
import collections

import conv_cases as C


def _layer_route(c):
    import torch

    from fvp import cnn

    conv, bn = C.modules(c)
    layer = cnn.ConvLayer(conv, bn, dtype=torch.bfloat16 if c.bf16 else torch.float32, cpi=c.cpi, algo=c.algo)
    layer.act_bf16 = c.out_bf16
    return cnn.conv_route(layer, c.N, c.H, c.W, in_bf16=c.in_bf16, residual=c.res_pre or c.res_post)


def test_every_instantiation_has_a_full_and_a_ragged_case():
    vs = C.variants()
    assert len(vs) == len(set(vs)) == 46
    assert collections.Counter(v.family for v in vs) == {1: 12, 2: 14, 3: 12, 4: 8}
    left_out = [(C.variant_id(v), kind) for v in vs for kind in ("full", "ragged") if C.base_case(v, kind) is None]
    assert len(left_out) == 0, left_out
    for v in vs:
        full, ragged = C.base_cases(v)
        assert (full.kind, ragged.kind) == ("full", "ragged") and full.variant == ragged.variant == v
        for c in (full, ragged):
            assert c.N >= 2 and c.Cin in (16, 32, 64) and c.KH * c.KW * c.Cin <= 1600, C.case_id(c)
            assert c.relu and not c.res_pre and not c.res_post and c.mode == 0 and c.stride == (1, 1)
            assert (2 * c.pad[0], 2 * c.pad[1]) == (c.KH - 1, c.KW - 1)
        cols = -(-ragged.Cout // 16) * 16
        if v.family == 2:
            assert full.W % 16 == 0 and full.H % (v.BM // 16) == 0 and ragged.H % 2 == 1 and ragged.W % 16
        else:
            assert full.N * full.H * full.W % v.BM == 0 and ragged.N * ragged.H * ragged.W % v.BM
            assert ragged.N * ragged.H * ragged.W > v.BM
        # a partial last column tile wherever the column class has one (16- and fp32 32-column
        # classes hold exactly one full tile: Ntot is a multiple of 16 and selects the class)
        if v.BN >= 64 or (v.BN == 32 and (v.family in (3, 4))):
            assert cols % v.BN != 0, C.case_id(ragged)


def test_every_case_gets_the_route_it_was_built_for():
    cases = C.all_cases()
    assert len(cases) == len(set(cases)) >= 300
    bad = []
    for c in cases:
        r = _layer_route(c)
        if not isinstance(r[0], int) or C.route_variant(r, c.bf16) != c.variant:
            bad.append(f"{C.case_id(c)}: route {r}")
    assert not bad, "\n".join(bad)


def test_variations_reach_a_small_and_a_large_launch_of_every_family():
    for name, (fields, fams) in C.VARIATIONS.items():
        got = collections.Counter((c.variant.family, c.kind.split("/")[1]) for c in C.variation_cases(name))
        for fam in fams:
            if fam == 4 and name == "k7x7":
                continue  # 49 taps: the LDS-DMA kernel takes at most 32
            sizes = ("small",) if name == "mode3-split" else ("small", "large")  # (split-K: < 256 blocks)
            for size in sizes:
                assert got[fam, size] >= 1, (name, fam, size)
