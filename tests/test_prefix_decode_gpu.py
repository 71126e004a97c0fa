"""Prefix-constrained PV -> SMILES decoding on the GPU: CachedDecoder.prefill (one packed pass, spmm_kv_prefill, one shared cache row) and
its stepping twin against the whole-prefix forward, the searches started at position P against the fp32 oracle and against each other,
and the driver.  Tiny configuration (H = 128, 2 heads, 2 text layers, fusion_layer = 1) with closed-form weights, as the decode tests use."""
import os
import subprocess
import sys

import pytest
import torch

from prefix_reference import beam_search_with_prefix, peaky_lm, prefixes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# LM-head bias of the search tests, picked on the CPU (seeds 1 .. 15 x sep_gap 0.3 / 0.5 / 0.8, k = 3, the 12 molecules and prefixes below): with
# seed 11 and sep_gap 0.5 the oracle search alone finishes 3 hypotheses for every molecule, and the bias's entries are 4.49, 4.34, 3.99
# ([SEP]), 3.40: the k-th and (k+1)-th are 0.59 apart, far outside the bf16 noise of the logits (the hidden states of the closed-form model
# move a logit by ~0.4 at most).  Seed 4 / 0.5 also finishes everything but has its 3rd and 4th entries 0.02 apart.
SEARCH_SEED, SEARCH_GAP = 11, 0.5


def _mk(SPMM, cfg, sd):
    m = SPMM(config=None, spmm_config=cfg)
    m.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    return m.eval()


@pytest.fixture(scope="module")
def peaky(env):
    O, SPMM, tiny_config, *_ = env
    return _mk(SPMM, tiny_config(), peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), sep_gap=0.4))    # (0.4: sampled searches end within a few positions)


@pytest.fixture(scope="module")
def searcher(env):
    """(HIP model, oracle model, props [12, 53], prefixes [12, 5]) of the search tests."""
    O, SPMM, tiny_config, *_ = env
    sd = peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), seed=SEARCH_SEED, sep_gap=SEARCH_GAP)
    props = torch.randn(12, 53, generator=torch.Generator().manual_seed(12)) * 2
    return _mk(SPMM, tiny_config(), sd), O.OracleModule(sd, O.tiny_cfg()), props, prefixes(12, 5, seed=35)


@pytest.fixture(scope="module")
def searched(searcher):
    """The prompted search of the 12 molecules, computed once: (prefill=True result, prefill=False result)."""
    from spmm_amd import decode
    m, _, props, pre = searcher
    a = decode.beam_search_batched(m, props, k=3, max_steps=12, prefix=pre)
    assert decode.last_run["prefix_tokens"] == 5 and decode.last_run["prefill"]
    b = decode.beam_search_batched(m, props, k=3, max_steps=12, prefix=pre, prefill=False)
    assert not decode.last_run["prefill"]
    return a, b


def _toks(res):
    return [[h[1] for h in mol] for mol in res]


def _check_prefill_then_steps(m, N, k, P, T, by_steps, seed=2):
    """Prefill logits, then T further steps with random tokens and random reorders, against the whole-prefix forward: 3e-2 on
    log-probabilities at every step (the bound of test_cached_decoder_step_matches_full_prefix_forward for exactly this pair of paths)."""
    from spmm_amd import decode
    g = torch.Generator().manual_seed(seed)
    props = torch.randn(N, 53, generator=g)
    pre = prefixes(N, P, seed=seed + P)
    pe = decode.encode_properties(m, props)
    Lmax = P + T + 2
    cached = decode.CachedDecoder(m, pe, k, Lmax)
    full = decode.RecomputeDecoder(m, pe, k, Lmax)
    lc = torch.log_softmax(cached.prefill(pre, range(N), by_steps=by_steps).float(), -1)
    lf = torch.log_softmax(full.prefill(pre, range(N)).float(), -1)
    assert lc.shape == (N, 300) and (lc - lf).abs().max().item() < 3e-2, (P, by_steps, (lc - lf).abs().max().item())
    dst = (torch.arange(N) * k).repeat_interleave(k).cuda().int()            # beam 0's row of the molecule
    own = torch.arange(N * k).cuda().int()

    def names_the_prefix_rows():
        a = cached.anc[:, :P]
        if by_steps:                                                         # the twin: every row holds its own copy; reorders stay inside the molecule
            return bool((a // k == own[:, None] // k).all())
        return bool((a == dst[:, None]).all())

    assert names_the_prefix_rows() and bool((cached.anc[:, P:] == own[:, None]).all())
    worst = 0.0
    for t in range(P, P + T):
        ids = torch.randint(4, 300, (N * k,), generator=g).cuda()
        a = torch.log_softmax(cached.step(ids, t).float(), -1)
        b = torch.log_softmax(full.step(ids, t).float(), -1)
        worst = max(worst, (a - b).abs().max().item())
        assert worst < 3e-2, (P, by_steps, t, worst)
        parent = torch.randint(0, k, (N, k), generator=g).cuda()
        cached.reorder(parent, t + 1)
        full.reorder(parent, t + 1)
        assert names_the_prefix_rows()
    return worst


@pytest.mark.parametrize("by_steps", [False, True])
@pytest.mark.parametrize("P", [2, 5, 17])
def test_prefill_matches_the_whole_prefix_forward(peaky, P, by_steps):
    """N = 3, k = 4.  P = 17 crosses a 16-key block of the decode-attention kernel's shared-key loop."""
    worst = _check_prefill_then_steps(peaky, 3, 4, P, 4, by_steps)
    print(f"prefill P={P} by_steps={by_steps}: worst |d log p| over 4 further steps {worst:.4f}")


@pytest.mark.parametrize("by_steps", [False, True])
def test_the_longest_prefix(peaky, by_steps):
    """P = 253 with max_steps = 1 fills the decode kernels' 256 positions (one molecule, k = 2); one more step does not fit."""
    from spmm_amd import decode
    worst = _check_prefill_then_steps(peaky, 1, 2, 253, 1, by_steps)
    print(f"prefill P=253 by_steps={by_steps}: worst |d log p| {worst:.4f}")
    if not by_steps:
        pre = prefixes(1, 253, seed=9)
        props = torch.randn(1, 53, generator=torch.Generator().manual_seed(3))
        res = decode.beam_search_batched(peaky, props, k=2, max_steps=1, prefix=pre)
        assert all(s[:253] == pre[0].tolist() and len(s) <= 256 for _, s in res[0])
        with pytest.raises(ValueError, match=r"253 \+ 2 \+ 2 = 257"):
            decode.beam_search_batched(peaky, props, k=2, max_steps=2, prefix=pre)


def test_many_samples_of_one_pv_share_one_cache_row(peaky):
    """A generate_with_property-style decoder (repeat = 6, ONE pair): every row's anc[:, :P] is 0, the first-step logits of all samples are
    identical, and a reaction-style decoder refuses."""
    from spmm_amd import decode
    m, k, P = peaky, 2, 5
    pe = decode.encode_properties(m, torch.randn(1, 53, generator=torch.Generator().manual_seed(8)))
    dec = decode.CachedDecoder(m, pe, k, P + 6, repeat=6)
    pre = prefixes(1, P, seed=4)
    logits = dec.prefill(pre, [0] * 6)
    assert logits.shape == (1, 300)
    assert bool((dec.anc[:, :P] == 0).all()) and bool((dec.anc[:, P:] == torch.arange(12, device="cuda")[:, None]).all())
    ids = torch.full((12,), 7, dtype=torch.long, device="cuda")
    first = dec.step(ids, P)
    assert bool((first == first[0:1]).all())
    full = decode.RecomputeDecoder(m, pe.expand(6, -1, -1), k, P + 6)
    full.prefill(pre, [0] * 6)
    ref = torch.log_softmax(full.step(ids, P).float(), -1)
    assert (torch.log_softmax(first.float(), -1) - ref).abs().max().item() < 3e-2
    dec.mem = {}
    with pytest.raises(ValueError, match="reaction prediction"):
        dec.prefill(pre, [0] * 6)


def test_prompted_search_against_the_oracle(searcher, searched):
    """The method of test_batched_decode_of_many_molecules_against_the_oracle_search at N = 12, k = 3, P = 5, max_steps = 12: every hypothesis
    starts with its prefix, ends in [SEP] with none inside, its score is the oracle's teacher-forced log-probability of the GENERATED tokens
    within 3e-2 per token, and the best hypothesis is token for token the reference search's for at least 90 % of the molecules."""
    m, om, props, pre = searcher
    from spmm_amd import decode
    got, P = searched[0], 5
    pe_o = decode.encode_properties(om, props)
    same = n_hyp = 0
    worst = 0.0
    for n in range(12):
        for p_, seq in got[n]:
            assert seq[:P] == pre[n].tolist() and seq[-1] == decode.SEP_ID and decode.SEP_ID not in seq[1:-1]
            text = torch.tensor([seq])
            logits = om.text_encoder(text, attention_mask=torch.ones_like(text), encoder_hidden_states=pe_o[n:n + 1],
                                     encoder_attention_mask=torch.ones(1, pe_o.shape[1], dtype=torch.long), return_dict=True, is_decoder=True,
                                     return_logits=True)
            lp = torch.log_softmax(logits[0, :-1].float(), -1).gather(1, text[0, 1:, None])[P - 1:].sum().item()
            worst = max(worst, abs(p_ - lp) / (len(seq) - P))
            n_hyp += 1
        ref = beam_search_with_prefix(om, props[n], pre[n].tolist(), k=3, max_steps=12)
        assert ref, f"the oracle search finishes nothing for molecule {n}: pick another bias"
        same += int(bool(got[n]) and got[n][0][1] == ref[0][1])
    # measured on an MI355X: 36 hypotheses, best hypothesis identical for 12 / 12, worst per-token difference 2.8e-3
    print(f"prompted decode vs oracle: {n_hyp} hypotheses, worst |score - oracle| per generated token {worst:.4f}; best identical for {same} / 12")
    assert n_hyp >= 12 and worst < 3e-2
    assert same >= 0.9 * 12


def test_prefill_and_stepping_give_the_same_search(searched):
    a, b = searched
    same, worst = 0, 0.0
    for ha, hb in zip(a, b):
        same += int(bool(ha) and bool(hb) and ha[0][1] == hb[0][1])
        for (pa, sa), (pb, sb) in zip(ha, hb):
            if sa == sb:
                worst = max(worst, abs(pa - pb) / (len(sa) - 5))
    print(f"prefill vs stepping: best identical for {same} / 12, worst per-token score difference {worst:.5f}")
    assert worst < 3e-2 and same >= 0.9 * 12


def test_fused_and_tensor_op_bookkeeping_agree_with_a_prefix(searcher, searched, monkeypatch):
    from spmm_amd import decode
    m, _, props, pre = searcher
    monkeypatch.setattr(decode, "FUSED_BEAM_STEP", False)
    plain = decode.beam_search_batched(m, props, k=3, max_steps=12, prefix=pre)
    assert _toks(plain) == _toks(searched[0]) and any(_toks(plain))
    for x, y in zip(plain, searched[0]):
        for (px, _), (py, _) in zip(x, y):
            assert abs(px - py) < 1e-4


def test_seeded_generation_from_a_prefix(peaky):
    """generate_with_property(seed=3, prefix=P5): the same samples whatever the chunking, other samples for another seed, every sample starts
    with the prefix; and the seeded prompted search with finished molecules dropped equals the one that keeps them."""
    from spmm_amd import decode
    m = peaky
    pv = torch.randn(53, generator=torch.Generator().manual_seed(31)) * 2
    pre = prefixes(1, 5, seed=6)[0].tolist()
    got = decode.generate_with_property(m, pv, 12, k=2, seed=3, max_steps=16, prefix=pre)
    assert decode.last_generate["prefix_tokens"] == 5 and decode.last_generate["chunks"] == 1
    chunked = decode.generate_with_property(m, pv, 12, k=2, seed=3, max_steps=16, prefix=pre, chunk=5)
    assert decode.last_generate["chunks"] == 3
    assert chunked == got
    other = decode.generate_with_property(m, pv, 12, k=2, seed=4, max_steps=16, prefix=pre)
    assert other != got
    done = [s for s in got if s]
    assert len(done) >= 6 and all(s[:5] == pre and s[-1] == decode.SEP_ID for s in done)
    assert len({tuple(s) for s in done}) > 1                                  # (it does sample)


def test_seeded_prompted_search_with_compaction_equals_the_whole_batch(env):
    """Sizes and bias of test_seeded_search_with_compaction_equals_the_whole_batch, every molecule started from its own 5-token prefix: the
    ancestry rows that `compact` gathers keep naming the prefix's cache row."""
    O, SPMM, tiny_config, *_ = env
    from spmm_amd import decode
    m = _mk(SPMM, tiny_config(), peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), seed=5, sep_gap=0.9))
    props = torch.randn(32, 53, generator=torch.Generator().manual_seed(12)) * 10.0
    pre = prefixes(32, 5, seed=13)
    kw = dict(k=5, max_steps=40, stochastic=True, seed=7, prefix=pre)
    whole = decode.beam_search_batched(m, props, compact=False, **kw)
    assert decode.last_run["compactions"] == 0
    small = decode.beam_search_batched(m, props, compact=True, **kw)
    run = dict(decode.last_run)
    print(f"seeded prompted decode with compaction: {run}")
    assert run["compactions"] >= 1 and run["final_batch"] < 32
    assert _toks(small) == _toks(whole)
    for a, b in zip(small, whole):
        for (pa, _), (pb, _) in zip(a, b):
            assert abs(pa - pb) < 1e-4


def test_no_prefix_means_no_change(peaky, monkeypatch):
    """prefix=None and prefix=[CLS] are the same call, on the old launch path: CachedDecoder.prefill is never entered."""
    from spmm_amd import decode
    m = peaky
    props = torch.randn(6, 53, generator=torch.Generator().manual_seed(4)) * 2

    def boom(*a, **kw):
        raise AssertionError("prefill entered without a prefix")

    monkeypatch.setattr(decode.CachedDecoder, "prefill", boom)
    plain = decode.beam_search_batched(m, props, k=5, max_steps=14)           # (the inputs of test_batched_cached_beam_search at sep_gap 0.4)
    assert decode.last_run["prefix_tokens"] == 1 and not decode.last_run["prefill"]
    assert decode.beam_search_batched(m, props, k=5, max_steps=14, prefix=[decode.CLS_ID]) == plain and any(plain)
    pv = props[0]
    gen = decode.generate_with_property(m, pv, 8, k=2, seed=3, max_steps=14)
    assert decode.generate_with_property(m, pv, 8, k=2, seed=3, max_steps=14, prefix=torch.tensor([decode.CLS_ID])) == gen
    assert decode.last_generate["prefix_tokens"] == 1


def test_driver_writes_molecules_that_start_with_the_fragment(tmp_path):
    """pv2smiles.py --synthetic --tiny --prefix c1cN (two pieces of the synthetic vocabulary) in a fresh process, twice: every written
    molecule starts with the fragment, and the same seed gives the same file."""
    outs = []
    for i in range(2):
        out = tmp_path / f"gen{i}.txt"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "pv2smiles.py"), "--synthetic", "--tiny", "--n_generate", "8", "--prefix", "c1cN",
                            "--seed", "1", "--output", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "prefix: c1cN (3 tokens)" in r.stdout
        outs.append(out.read_text())
    lines = outs[0].splitlines()
    assert len(lines) == 8 and all(s.startswith("c1cN") for s in lines), lines
    assert outs[0] == outs[1]
