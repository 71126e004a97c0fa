"""decode.sample_distinct where there is no GPU: the whole-prefix decoder (cached=False) on the CPU oracle's module API with the float64
tensor-op step (DistinctBook.update) -- the same search the GPU runs on the cached decoder and the one-launch step.  Scores are exact
here (fp32 forwards, float64 bookkeeping): the log-probability of a hypothesis is the teacher-forced score of its tokens to 1e-4."""
import os

import numpy as np
import pytest
import torch

import spmm_oracle as O
from prefix_reference import peaky_lm

from spmm_amd import decode
from spmm_amd import smiles_syntax as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(seed=3, max_steps=10)


@pytest.fixture(scope="module")
def om():
    from spmm_amd.tokenizer import SmilesWordPiece
    m = O.OracleModule(peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), seed=5, sep_gap=0.9), O.tiny_cfg())
    m.tokenizer = SmilesWordPiece([str(x) for x in np.load(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab300.npz"))["vocab"]])
    return m


@pytest.fixture(scope="module")
def props():
    return torch.randn(2, 53, generator=torch.Generator().manual_seed(12)) * 10.0


def _toks(hyps):
    return [h[1] for h in hyps]


def test_distinct_nested_and_each_vector_its_own(om, props):
    both = decode.sample_distinct(om, props, 12, **KW)
    run = dict(decode.last_distinct)
    assert run["groups"] == 2 and run["W"] == 16 and not run["fused"] and run["min_gap"] > 0
    assert all(f + u + e == 12 for f, u, e in zip(run["finished"], run["unfinished"], run["empty"]))
    for g, hyps in enumerate(both):
        assert len(hyps) >= 2 and len({tuple(t) for t in _toks(hyps)}) == len(hyps)
        assert all(s[0] == decode.CLS_ID and s[-1] == decode.SEP_ID and decode.SEP_ID not in s[1:-1] for s in _toks(hyps))
        assert decode.sample_distinct(om, props[g], 12, pv_base=g, **KW)[0] == hyps          # the vector alone: the same list, bit for bit
    eight = decode.sample_distinct(om, props, 8, **KW)
    assert decode.last_distinct["W"] == 8 and all(a == b[:len(a)] for a, b in zip(eight, both))
    assert _toks(decode.sample_distinct(om, props[0], 12, **dict(KW, seed=4))[0]) != _toks(both[0])


def test_the_scores_are_teacher_forced_scores(om, props):
    warp = dict(temperature=1.3, top_p=0.9)
    for kw, w in ((dict(), None), (warp, warp), (dict(prefix=[2, 30, 40]), None)):
        hyps = decode.sample_distinct(om, props[0], 16, **kw, **dict(KW, max_steps=14))[0]
        assert hyps, kw
        P = len(kw.get("prefix", [2]))
        pe = decode.encode_properties(om, props[:1])
        for p, seq in hyps:
            text = torch.tensor([seq])
            logits = om.text_encoder(text, attention_mask=torch.ones_like(text), encoder_hidden_states=pe,
                                     encoder_attention_mask=torch.ones(1, pe.shape[1], dtype=torch.long), return_dict=True, is_decoder=True,
                                     return_logits=True)[0, :-1].double()
            if w is not None:
                logits = decode.warp_logits(logits, **w, min_keep=1)
            lp = torch.log_softmax(logits, -1).gather(1, text[0, 1:, None])[P - 1:].sum().item()
            assert seq[:P] == kw.get("prefix", [2]) and abs(p - lp) < 1e-4, (kw, p, lp)


def test_syntax_prefix_and_a_small_top_k(om, props):
    res = decode.sample_distinct(om, props[0], 8, syntax=True, prefix=[2, 30], top_k=5, **KW)[0]
    run = dict(decode.last_distinct)
    assert run["syntax"] and run["top_k"] == 5 and run["prefix_tokens"] == 2 and run["dropped_masked"] == 0
    assert len(res) == 8 and len({tuple(t) for t in _toks(res)}) == 8          # the budget forces every hypothesis shut
    assert all(s[:2] == [2, 30] and SS.well_formed(om.tokenizer.decode(s)) for s in _toks(res))


def test_refusals(om, props):
    with pytest.raises(ValueError, match="guidance=2.0.*out of scope"):
        decode.sample_distinct(om, props, 8, guidance=2.0)
    for n in (1025, 0, 2.5):
        with pytest.raises(ValueError, match=r"outside \[1, 1024\]"):
            decode.sample_distinct(om, props, n)
    with pytest.raises(ValueError, match="temperature=0.0"):
        decode.sample_distinct(om, props, 8, temperature=0.0)


def test_min_keep_leaves_the_existing_decoders_as_they_were():
    """GuidedDecoder / GuidedRecompute: min_keep=None is k, today's value (check_warp still refuses a top_k below k there)."""
    import inspect
    for cls in (decode.GuidedDecoder, decode.GuidedRecompute):
        assert inspect.signature(cls.__init__).parameters["min_keep"].default is None
    with pytest.raises(ValueError, match="top_k=3 is below the k=5"):
        decode.check_warp(1.0, 1.0, 3, 1.0, 5)
