"""Prefix-constrained PV -> SMILES search where there is no GPU: the batched search on the CPU oracle (fp32, whole-prefix forwards,
cached=False) against the sequential one-molecule search started from the same prefix (tests/prefix_reference.py), the argument checks,
and the driver's --prefix argument path."""
import os
import sys

import pytest
import torch

import spmm_oracle as O
from prefix_reference import beam_search_with_prefix, peaky_lm, prefixes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS_ID, SEP_ID = 2, 3
# LM-head bias picked on the CPU (seeds 1 .. 15 x sep_gap 0.3 / 0.5 / 0.8 tried; most finish nothing in 10 positions): with seed 7 [SEP] is the
# third largest entry at every gap, and the reference search finishes 3 hypotheses for every one of the 4 molecules at both prefix lengths --
# asserted below, so the comparison cannot be vacuous
BIAS_SEED, SEP_GAP = 7, 0.8
N, K, STEPS = 4, 3, 10


@pytest.fixture(scope="module")
def om():
    return O.OracleModule(peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), seed=BIAS_SEED, sep_gap=SEP_GAP), O.tiny_cfg())


@pytest.fixture(scope="module")
def props():
    return torch.randn(N, 53, generator=torch.Generator().manual_seed(12)) * 2


@pytest.mark.parametrize("P", [2, 5])
def test_batched_search_from_a_prefix_equals_the_sequential_search(om, props, P):
    """beam_search_batched(cached=False, prefix=...) against beam_search_with_prefix per molecule: token for token, scores within 1e-5
    (both fp32 on the same model: the bound test_oracle_golden uses for fp32 restatements); every hypothesis starts with its prefix."""
    from spmm_amd.decode import beam_search_batched
    pre = prefixes(N, P, seed=30 + P)
    got = beam_search_batched(om, props, k=K, max_steps=STEPS, cached=False, prefix=pre)
    for n in range(N):
        want = beam_search_with_prefix(om, props[n], pre[n].tolist(), k=K, max_steps=STEPS)
        assert len(want) >= 1, f"the reference search finishes nothing for molecule {n}: pick another bias"
        assert len(got[n]) == len(want), (n, got[n], want)
        for (pg, sg), (pw, sw) in zip(got[n], want):
            assert sg == sw and abs(pg - pw) < 1e-5, (n, sg, sw, pg, pw)
            assert sg[:P] == pre[n].tolist() and sg[-1] == SEP_ID
    # one prefix for all molecules, as a list: the [P] form
    one = pre[0].tolist()
    got1 = beam_search_batched(om, props, k=K, max_steps=STEPS, cached=False, prefix=one)
    assert got1[0] == got[0] and all(h and all(s[:P] == one for _, s in h) for h in got1)


def test_a_cls_only_prefix_is_no_prefix(om, props):
    from spmm_amd import decode
    plain = decode.beam_search_batched(om, props, k=K, max_steps=STEPS, cached=False)
    for pre in ([CLS_ID], torch.tensor([CLS_ID]), torch.full((N, 1), CLS_ID)):
        assert decode.beam_search_batched(om, props, k=K, max_steps=STEPS, cached=False, prefix=pre) == plain
    assert any(plain)


def test_generate_with_property_from_a_prefix_on_the_module_api(om, props):
    """The deterministic generate_with_property (module API) returns the best hypothesis of the prefix search for each sample."""
    from spmm_amd import decode
    pre = prefixes(1, 5, seed=35)[0].tolist()
    out = decode.generate_with_property(om, props[0], 2, k=K, stochastic=False, max_steps=STEPS, prefix=pre)
    want = beam_search_with_prefix(om, props[0], pre, k=K, max_steps=STEPS)
    assert want and out == [want[0][1], want[0][1]]
    assert decode.last_generate["prefix_tokens"] == 5


@pytest.mark.parametrize("prefix,msg", [
    ([[CLS_ID, 5, 6], [CLS_ID, 5], [CLS_ID, 7, 8], [CLS_ID, 9, 9]], "group the molecules by prefix length"),
    ([5, 6, 7], r"first token must be \[CLS\]"),
    ([CLS_ID, 5, SEP_ID, 6], r"\[SEP\] \(3\) or PAD \(0\) inside"),
    ([CLS_ID, 5, SEP_ID], r"\[SEP\] \(3\) or PAD \(0\) inside"),
    ([CLS_ID, 0, 6], r"\[SEP\] \(3\) or PAD \(0\) inside"),
    ([CLS_ID, 5, 300], "outside the vocabulary of 300"),
    ([CLS_ID, 5, -4], "outside the vocabulary"),
    (torch.full((2, 2, 2), CLS_ID), "3 dimensions"),
    (torch.full((3, 2), CLS_ID), r"neither \[P\] nor \[N, P\]"),
])
def test_bad_prefixes_are_refused(om, props, prefix, msg):
    from spmm_amd.decode import beam_search_batched
    with pytest.raises(ValueError, match=msg):
        beam_search_batched(om, props, k=K, max_steps=STEPS, cached=False, prefix=prefix)


def test_a_prefix_that_leaves_no_room_is_refused(om, props):
    from spmm_amd.decode import beam_search_batched, generate_with_property
    pre = [CLS_ID] + [5] * 9
    with pytest.raises(ValueError, match=r"10 \+ 245 \+ 2 = 257"):
        beam_search_batched(om, props, k=K, max_steps=245, cached=False, prefix=pre)
    with pytest.raises(ValueError, match=r"10 \+ 245 \+ 2 = 257"):
        generate_with_property(om, props[0], 2, max_steps=245, prefix=pre)


def test_beam_book_with_a_prefix_counts_from_it():
    """BeamBook(prefix=...): histories start with the prefix, `first` writes column P, finals carry the prefix and their length, scores
    hold the generated tokens only -- tensor-op bookkeeping, one molecule whose second beam ends at the first update."""
    from spmm_amd.decode import BeamBook
    pre = torch.tensor([[CLS_ID, 9, 8, 7]])
    book = BeamBook(1, 2, 3, "cpu", prefix=pre)
    assert book.Lmax == 4 + 3 + 2 and book.t == 4 and book.tokens[0, :, :4].tolist() == [[CLS_ID, 9, 8, 7]] * 2
    book.first(torch.tensor([[-0.1, -0.2]]), torch.tensor([[11, 12]]))
    assert book.t == 5 and book.tokens[0, :, 4].tolist() == [11, 12]
    book.update(torch.tensor([[[-0.5, -0.7], [-0.3, -0.9]]]), torch.tensor([[[20, 21], [SEP_ID, 22]]]))
    assert book.t == 6
    (p, seq), = book.results()[0]
    assert seq == [CLS_ID, 9, 8, 7, 12, SEP_ID] and abs(p - (-0.2 - 0.3)) < 1e-6
    assert book.tokens[0].tolist()[0][:6] == [CLS_ID, 9, 8, 7, 11, 20]


# ------------------------------------------------------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def driver():
    sys.path.insert(0, ROOT)
    import pv2smiles
    return pv2smiles


def test_driver_prefix_argument(driver):
    from spmm_amd.tokenizer import SmilesWordPiece
    args = driver.parse_args(["--synthetic", "--tiny", "--n_generate", "8", "--prefix", "CCl", "--seed", "1"])
    assert args.prefix == "CCl" and driver.parse_args(["--synthetic"]).prefix == ""
    vocab = driver.synthetic_vocab(300)
    tok = SmilesWordPiece(vocab)
    ids = driver.prefix_ids(tok, "CCl")
    # '[CLS]' + 'CCl' is one word: the literal [CLS] piece, then greedy longest match over '##' pieces: '##CCl' (C + Cl) is in the vocabulary
    assert ids[0] == CLS_ID and [vocab[i] for i in ids[1:]] == ["##CCl"]
    ids = driver.prefix_ids(tok, "c1cN")
    assert [vocab[i] for i in ids] == ["[CLS]", "##c1", "##cN"] and tok.decode(ids) == "c1cN"
    assert tok.decode(ids + [vocab.index("##O"), SEP_ID]).startswith("c1cN")


@pytest.mark.parametrize("fragment", ["CX", "C C", "Zz"])
def test_driver_refuses_a_fragment_it_cannot_spell(driver, fragment):
    from spmm_amd.tokenizer import SmilesWordPiece
    tok = SmilesWordPiece(driver.synthetic_vocab(300))
    with pytest.raises(SystemExit, match=repr(fragment).replace("\\", "\\\\")):
        driver.prefix_ids(tok, fragment)
