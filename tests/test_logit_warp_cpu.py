"""The logit warp of the PV -> SMILES search where there is no GPU: decode.warp_logits against the float64 brute force of
tests/warp_reference.py on the kernel test's grid, its edge rules, the distance of every committed row from its cut, and the guided /
truncated searches on the CPU oracle model (cached=False: two whole-prefix decoders and warp_logits)."""
import pytest
import torch

import warp_reference as WR
from prefix_reference import peaky_lm
from spmm_amd import decode

CASES = WR.cases()
warp_logits, check_warp = decode.warp_logits, decode.check_warp            # (the feature under test: without it nothing here can be collected)


def _kept(x):
    return torch.isfinite(x)


@pytest.mark.parametrize("c", CASES, ids=[WR.case_id(c) for c in CASES])
def test_warp_logits_equals_the_brute_force(c):
    """Same kept set, kept values to 1e-12 in float64, dropped entries exactly -inf."""
    lc, lu = WR.case_inputs(c)
    V, kw = c["V"], WR.case_kwargs(c)
    lc, lu = lc[:, :V].double(), (None if lu is None else lu[:, :V].double())
    want = WR.brute_force(lc, lu, **kw)
    got = decode.warp_logits(lc, lu, guidance=kw["w"], temperature=kw["temperature"], top_k=kw["top_k"], top_p=kw["top_p"], min_keep=kw["min_keep"])
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert torch.equal(_kept(got), _kept(want))
    assert bool((got[~_kept(got)] == -float("inf")).all())
    assert (got[_kept(got)] - want[_kept(want)]).abs().max().item() <= 1e-12
    assert int(_kept(want).sum(1).min()) >= c["min_keep"]


def test_the_grid_covers_every_value_of_every_factor():
    assert 24 <= len(CASES) <= 60
    for name, vals in (("V", WR.VS), ("R", WR.RS), ("temperature", WR.TEMPS), ("top_p", WR.TOPPS), ("min_keep", WR.KEEPS)):
        assert {c[name] for c in CASES} == set(vals), name
    assert {c["w"] for c in CASES if c["has_lu"]} == set(WR.WS)
    assert {c["has_lu"] for c in CASES} == {True, False} and {c["alias"] for c in CASES} == {True, False}
    assert any(c["pad_in"] for c in CASES) and any(c["pad_out"] for c in CASES)
    for V in WR.VS:                                                         # every top_k form somewhere, none of them at one V only
        assert len({c["top_k"] for c in CASES if c["V"] == V}) >= 4
    seen = {spec for spec in WR.TOPKS for c in CASES if c["top_k"] == WR._top_k(spec, c["V"], c["min_keep"])}
    assert seen == set(WR.TOPKS)


def test_no_committed_row_sits_on_its_cut():
    """The kernel works in fp32: a row whose cut lies within rounding of the boundary cannot be judged against float64.  Every row of every
    case of the GPU test is farther than 1e-4 from flipping (the ties case is judged by the index rule, exactly, and is not part of this).
    A failure here is answered with another seed (warp_reference.BUMP), never with another bound."""
    worst = float("inf")
    for i, c in enumerate(CASES):
        lc, lu = WR.case_inputs(c)
        V = c["V"]
        m = WR.cut_margin(lc[:, :V], None if lu is None else lu[:, :V], **WR.case_kwargs(c))
        worst = min(worst, float(m.min()))
        assert float(m.min()) > 1e-4, (i, WR.case_id(c), m.tolist())
    print(f"smallest cut margin over {len(CASES)} cases: {worst:.3e}")


def test_the_defaults_are_the_identity():
    x = torch.randn(7, 300, generator=torch.Generator().manual_seed(1)) * 2
    assert decode.warp_logits(x) is x
    for dt in (torch.float32, torch.float64, torch.bfloat16):
        y = x.to(dt)
        assert torch.equal(decode.warp_logits(y, None, guidance=1.0, temperature=1.0, top_k=0, top_p=1.0, min_keep=3), y)
    assert torch.equal(decode.warp_logits(x, top_k=300), x) and torch.equal(decode.warp_logits(x, top_k=305), x)
    assert torch.equal(decode.warp_logits(x, x * 0.5, guidance=1.0), x * 0.5 + 1.0 * (x - x * 0.5))


@pytest.mark.parametrize("K", [1, 2, 17, 299])
def test_top_k_keeps_exactly_k(K):
    x = torch.randn(6, 300, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 2
    out = decode.warp_logits(x, top_k=K)
    assert _kept(out).sum(1).tolist() == [K] * 6
    assert torch.equal(_kept(out), torch.zeros_like(x, dtype=torch.bool).scatter(1, torch.topk(x, K, dim=1).indices, True))
    assert torch.equal(out[_kept(out)], x[_kept(out)])


@pytest.mark.parametrize("min_keep", [1, 2, 8])
def test_a_vanishing_nucleus_keeps_exactly_min_keep(min_keep):
    x = torch.randn(6, 300, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2
    for top_p in (1e-6, 1e-30, 5e-324):
        out = decode.warp_logits(x, top_p=top_p, min_keep=min_keep)
        assert _kept(out).sum(1).tolist() == [min_keep] * 6
        assert torch.equal(_kept(out), torch.zeros_like(x, dtype=torch.bool).scatter(1, torch.topk(x, min_keep, dim=1).indices, True))


@pytest.mark.parametrize("top_k", [0, 40])
@pytest.mark.parametrize("top_p", [0.3, 0.9, 0.99])
def test_the_nucleus_is_the_smallest_set_that_reaches_top_p(top_p, top_k):
    """The kept mass (of the distribution renormalised over the top_k best) is >= top_p, and without the last kept token it is below."""
    x = torch.randn(8, 300, generator=torch.Generator().manual_seed(4), dtype=torch.float64) * 2
    out = decode.warp_logits(x, temperature=0.8, top_k=top_k, top_p=top_p)
    z = x / 0.8
    zk = z if top_k == 0 else torch.where(_kept(decode.warp_logits(z, top_k=top_k)), z, torch.full_like(z, -float("inf")))
    q = torch.softmax(zk, dim=1)
    for i in range(8):
        kept = _kept(out[i])
        mass = float(q[i][kept].sum())
        assert mass >= top_p and mass - float(q[i][kept].min()) < top_p, (i, mass)
        assert float(q[i][kept].min()) >= float(q[i][~kept].max())          # and it is made of the most probable tokens


def test_a_block_of_equal_values_is_cut_after_the_lower_indices():
    lc, kw = WR.ties_case()
    out = decode.warp_logits(lc.double(), None, guidance=kw["w"], temperature=kw["temperature"], top_k=kw["top_k"], top_p=kw["top_p"],
                             min_keep=kw["min_keep"])
    kept = [row.nonzero().flatten().tolist() for row in _kept(out)]
    assert kept[0] == list(range(10, 19))                                   # 17 of the 30 equal values survive top-k: each 1/17; 9 reach 0.5
    assert kept[1] == [3, 250, 251]
    assert kept[2] == [100, 101, 102, 103, 104]
    assert kept[3] == [0, 50, 100, 150]
    assert kept[4] == list(range(9))
    assert torch.equal(_kept(out), _kept(WR.brute_force(lc, None, **kw)))
    only_k = decode.warp_logits(lc.double(), top_k=17)
    assert only_k[0].isfinite().nonzero().flatten().tolist() == list(range(10, 27))
    assert only_k[4].isfinite().nonzero().flatten().tolist() == list(range(17))


# ------------------------------------------------------------------------------------------------------------------ the searches, CPU oracle
@pytest.fixture(scope="module")
def oracle():
    import spmm_oracle as O
    sd = peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), seed=11, sep_gap=0.5)
    props = torch.randn(4, 53, generator=torch.Generator().manual_seed(12)) * 2
    return O.OracleModule(sd, O.tiny_cfg()), props


def _same(a, b, tol):
    assert [[h[1] for h in m] for m in a] == [[h[1] for h in m] for m in b] and any(any(m) for m in a)
    for x, y in zip(a, b):
        for (px, _), (py, _) in zip(x, y):
            assert abs(px - py) <= tol, (px, py)


def test_guidance_zero_is_the_all_masked_search(oracle):
    om, props = oracle
    kw = dict(k=3, max_steps=8, cached=False)
    masked = decode.beam_search_batched(om, props, prop_mask=torch.ones(53), **kw)
    assert decode.last_run["baseline_rows"] == 0 and decode.last_run["guidance"] == 1.0
    guided = decode.beam_search_batched(om, props, guidance=0.0, **kw)
    assert decode.last_run["baseline_rows"] == 12 and decode.last_run["guidance"] == 0.0
    _same(guided, masked, 1e-5)
    seeded = dict(kw, stochastic=True, seed=5)
    _same(decode.beam_search_batched(om, props, guidance=0.0, **seeded), decode.beam_search_batched(om, props, prop_mask=torch.ones(53), **seeded), 1e-5)


def test_the_defaults_are_the_plain_search(oracle, monkeypatch):
    om, props = oracle
    plain = decode.beam_search_batched(om, props, k=3, max_steps=8, cached=False, stochastic=True, seed=5)

    def boom(*a, **kw):
        raise AssertionError("a guided decoder was built at the defaults")

    monkeypatch.setattr(decode.GuidedRecompute, "__init__", boom)
    monkeypatch.setattr(decode.GuidedDecoder, "__init__", boom)
    again = decode.beam_search_batched(om, props, k=3, max_steps=8, cached=False, stochastic=True, seed=5, guidance=1.0, temperature=1.0, top_k=0, top_p=1.0)
    assert again == plain and any(plain)
    assert {f: decode.last_run[f] for f in ("guidance", "temperature", "top_k", "top_p", "baseline_rows")} == dict(decode.NO_WARP, baseline_rows=0)
    gen = decode.generate_with_property(om, props[0], 5, k=2, seed=3, max_steps=8)
    assert decode.generate_with_property(om, props[0], 5, k=2, seed=3, max_steps=8, guidance=1.0, temperature=1.0, top_k=0, top_p=1.0) == gen
    assert decode.last_generate["baseline_rows"] == 0 and decode.last_generate["top_p"] == 1.0


def test_truncation_is_applied_and_recorded(oracle):
    """The whole-prefix guided decoder's step is warp_logits of the two conditions' own steps (the baseline: the all-masked PV, whatever the
    PV), with min_keep = k; the searches record what they ran with, and chunking does not change the samples."""
    om, props = oracle
    pe = decode.encode_properties(om, props)
    kw = dict(guidance=2.0, temperature=0.8, top_k=20, top_p=0.9)
    g = decode.GuidedRecompute(om, pe, 3, 10, base_embeds=decode._baseline_embeds(om, props[:1]), **kw)
    c = decode.RecomputeDecoder(om, pe, 3, 10)
    u = decode.RecomputeDecoder(om, decode.encode_properties(om, props, torch.ones(53)), 3, 10)
    ids = torch.full((12,), decode.CLS_ID, dtype=torch.long)
    for t in range(2):
        got = g.step(ids, t)
        want = decode.warp_logits(c.step(ids, t).float(), u.step(ids, t).float(), min_keep=3, **kw)
        assert torch.equal(got, want)
        assert 3 <= int(torch.isfinite(got).sum(1).min()) and int(torch.isfinite(got).sum(1).max()) <= 20
        ids = torch.full((12,), 10 + t, dtype=torch.long)
    cut = decode.beam_search_batched(om, props, k=3, max_steps=8, cached=False, stochastic=True, seed=5, top_k=3, temperature=0.9)
    assert decode.last_run["top_k"] == 3 and decode.last_run["temperature"] == 0.9 and decode.last_run["baseline_rows"] == 0
    assert any(cut)
    gen = decode.generate_with_property(om, props[0], 6, k=2, seed=3, max_steps=8, guidance=2.0, top_k=20)
    assert decode.last_generate["guidance"] == 2.0 and decode.last_generate["top_k"] == 20 and decode.last_generate["baseline_rows"] == 12
    assert decode.generate_with_property(om, props[0], 6, k=2, seed=3, max_steps=8, guidance=2.0, top_k=20, chunk=4) == gen


@pytest.mark.parametrize("bad,msg", [(dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
                                     (dict(temperature=float("inf")), "temperature"), (dict(temperature=float("nan")), "temperature"),
                                     (dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"), (dict(top_p=float("nan")), "top_p"),
                                     (dict(top_k=-1), "top_k"), (dict(top_k=2), "top_k=2 is below the k=3"), (dict(top_k=1.5), "top_k"),
                                     (dict(guidance=float("inf")), "guidance"), (dict(guidance=float("nan")), "guidance")])
def test_bad_arguments_raise_before_anything_runs(bad, msg):
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name}) before the arguments were checked")

    props = torch.zeros(2, 53)
    with pytest.raises(ValueError, match=msg):
        decode.beam_search_batched(Boom(), props, k=3, max_steps=4, cached=False, **bad)
    with pytest.raises(ValueError, match=msg):
        decode.generate_with_property(Boom(), props[0], 4, k=3, max_steps=4, **bad)
    with pytest.raises(ValueError, match=msg):
        decode.check_warp(**dict(dict(guidance=1.0, temperature=1.0, top_k=0, top_p=1.0, k=3), **bad))


def test_top_k_equal_to_k_is_accepted():
    assert decode.check_warp(1.0, 1.0, 3, 1.0, 3) == dict(guidance=1.0, temperature=1.0, top_k=3, top_p=1.0)
    assert decode.check_warp(1.0, 1.0, 0, 1.0, 3) is None


def test_the_reaction_decoder_refuses_guidance():
    """predict_products decodes against a memory of reactant tokens (CachedDecoder(memory=...)): there is no all-masked baseline to contrast."""
    with pytest.raises(ValueError, match="reaction prediction"):
        decode.GuidedDecoder(None, None, 3, 12, memory=dict(N=2, Lmax=8, xkv={}), guidance=2.0)
    with pytest.raises(ValueError, match="reaction prediction"):
        decode.GuidedDecoder(None, None, 3, 12, memory=dict(N=2, Lmax=8, xkv={}), top_p=0.9)
    import inspect
    assert "guidance" not in inspect.signature(decode.predict_products).parameters
