"""decode.sample_distinct on the GPU: stochastic beam search on the cached decoder and the one-launch step (ops.sbs_step).  Tiny
configuration, the closed-form weights with the peaky LM-head bias of tests/prefix_reference.py, the published 300-piece vocabulary.

Tolerances.  DELTA is tests/test_sbs_step_gpu.py's (the kernel's keys against float64): a seed is admitted to the fused-against-tensor-op
comparison only if no decision of the float64 form hung on a key gap below it (last_distinct["min_gap"], asserted first), and then the two
forms must return the same token lists, all of them.
LOGP_TOL is 2 x the largest |reported log-probability - score_smiles| of the existing seeded sampled search (beam_search_batched, k = 2,
stochastic, seed 7, 24 molecules of the same property vector, the same model and max_steps; 32 hypotheses of up to 24 tokens) measured on
an MI355X: 2 x 1.265e-2 (sample_distinct itself measured 1.24e-2 at most over seeds 1 .. 12).  The two paths share the weights and differ
in their attention kernels (K/V-cache decode against packed rows): a few bf16 roundings of the activations per token.  score_smiles does
not count a [PAD] target (id 0, which an untrained decoder emits now and then): hypotheses that hold one are left out of this comparison,
in the measurement and in the test alike.
Prefill against stepping is held to what tests/test_prefix_decode_gpu.py asks of these two routes: per-token score difference < 3e-2 where
the tokens agree, identical token lists for at least 0.9 of the samples (their logits differ by bf16 roundings, so a draw may flip)."""
import os
import sys

import numpy as np
import pytest
import torch

from prefix_reference import peaky_lm
from sbs_reference import DELTA

from spmm_amd import smiles_syntax as SS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS_ID, SEP_ID = 2, 3
LOGP_TOL = 2 * 1.265e-2
KW = dict(seed=3, max_steps=28)


@pytest.fixture(scope="module")
def tok():
    from spmm_amd.tokenizer import SmilesWordPiece
    return SmilesWordPiece([str(x) for x in np.load(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab300.npz"))["vocab"]])


@pytest.fixture(scope="module")
def model(env, tok):
    O, SPMM, tiny_config, *_ = env
    m = SPMM(config=None, spmm_config=tiny_config())
    m.load_state_dict({k: v.detach().clone() for k, v in peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), seed=5, sep_gap=0.9).items()})
    m.tokenizer = tok
    return m.eval()


@pytest.fixture(scope="module")
def props():
    return torch.randn(2, 53, generator=torch.Generator().manual_seed(12)) * 10.0


@pytest.fixture(scope="module")
def base24(model, props):
    """sample_distinct(n = 24) of the first property vector, computed once: (result, last_distinct)."""
    from spmm_amd import decode
    res = decode.sample_distinct(model, props[0], 24, **KW)
    return res, dict(decode.last_distinct)


def _toks(hyps):
    return [h[1] for h in hyps]


def _wellformed_ends(hyps):
    for p, ids in hyps:
        assert ids[0] == CLS_ID and ids[-1] == SEP_ID and SEP_ID not in ids[1:-1] and np.isfinite(p) and p < 0, (p, ids)


def _teacher_forced(model, pv, hyps, P=1, warp=None):
    """log-probability of the generated tokens (positions >= P) of every hypothesis by one whole-sequence forward through the module API;
    warp: decode.warp_logits' arguments, applied on the host in float64 (the yard-stick of the warped searches)."""
    from spmm_amd import decode
    pe = decode.encode_properties(model, pv.reshape(1, -1).cuda())
    out = []
    for _, seq in hyps:
        text = torch.tensor([seq], device=pe.device)
        logits = model.text_encoder(text, attention_mask=torch.ones_like(text), encoder_hidden_states=pe,
                                    encoder_attention_mask=torch.ones(1, pe.shape[1], dtype=torch.long, device=pe.device), return_dict=True,
                                    is_decoder=True, return_logits=True)[0, :-1].double().cpu()
        if warp is not None:
            logits = decode.warp_logits(logits, **warp, min_keep=1)
        out.append(torch.log_softmax(logits, -1).gather(1, torch.tensor(seq[1:])[:, None])[P - 1:].sum().item())
    return out


def test_the_samples_are_distinct_and_seeded(model, props, base24):
    from spmm_amd import decode
    (res,), run = base24
    print(f"sample_distinct(24): {run}")
    assert run["fused"] and run["W"] == 24 and run["finished"] == [len(res)] and run["finished"][0] + run["unfinished"][0] + run["empty"][0] == 24
    assert len(res) >= 12, "too few hypotheses finished for the test to mean much: pick another bias"
    _wellformed_ends(res)
    assert len({tuple(t) for t in _toks(res)}) == len(res)
    again = decode.sample_distinct(model, props[0], 24, **KW)[0]
    assert again == res                                                   # the same seed: the same list, scores bit for bit
    other = decode.sample_distinct(model, props[0], 24, **dict(KW, seed=4))[0]
    assert _toks(other) != _toks(res)


def test_eight_samples_are_the_first_eight_of_24(model, props, base24):
    from spmm_amd import decode
    (res,), _ = base24
    eight = decode.sample_distinct(model, props[0], 8, **KW)[0]
    run = dict(decode.last_distinct)
    print(f"n = 8: {run}")
    assert run["W"] == 8 and len(eight) >= 1
    assert _toks(eight) == _toks(res)[:len(eight)]
    assert max(abs(a[0] - b[0]) for a, b in zip(eight, res)) < 1e-4       # (another batch: the project's bound between batch compositions)
    five = decode.sample_distinct(model, props[0], 5, **KW)[0]            # n not a multiple of 8: the first 5 slots of the 8-slot search
    assert decode.last_distinct["W"] == 8 and _toks(five) == _toks(eight)[:len(five)] and len(five) <= 5


def test_the_one_launch_step_and_the_tensor_op_form_return_the_same_lists(model, props, base24, monkeypatch):
    from spmm_amd import decode, ops
    (res,), _ = base24
    calls = []
    inner = ops.sbs_step
    monkeypatch.setattr(ops, "sbs_step", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    monkeypatch.setattr(decode, "FUSED_BEAM_STEP", False)
    plain = decode.sample_distinct(model, props[0], 24, **KW)[0]
    run = dict(decode.last_distinct)
    print(f"tensor-op form: {run}")
    assert not run["fused"] and not calls
    assert run["min_gap"] > DELTA, f"a decision of the float64 form hung on a key gap of {run['min_gap']:.3e} <= DELTA: pick another seed"
    assert _toks(plain) == _toks(res)                                     # cap: 0 differing samples
    assert max(abs(a[0] - b[0]) for a, b in zip(plain, res)) <= DELTA


def test_every_logp_is_the_teacher_forced_score_of_its_own_tokens(model, props, base24):
    from spmm_amd import score
    (res,), _ = base24
    res = [h for h in res if 0 not in h[1]]                               # (score_smiles does not count a [PAD] target)
    assert len(res) >= 8
    L = max(len(s) for _, s in res)
    ids = torch.zeros(len(res), L, dtype=torch.long)
    for i, (_, s) in enumerate(res):
        ids[i, :len(s)] = torch.tensor(s)
    mask = (torch.arange(L)[None, :] < torch.tensor([len(s) for _, s in res])[:, None]).long()       # (an untrained decoder also emits id 0)
    sc = score.score_smiles(model, props[:1], ids, mask, torch.tensor([[0, i] for i in range(len(res))]))
    worst = max(abs(p - lp) for (p, _), lp in zip(res, sc.logp.cpu().tolist()))
    print(f"sample_distinct against score_smiles: {len(res)} hypotheses of up to {L - 1} tokens, largest |logp - score| {worst:.3e} (bound {LOGP_TOL:.3e})")
    assert worst <= LOGP_TOL


def test_syntax_gives_well_formed_strings_only(model, tok, props):
    from spmm_amd import decode
    res = decode.sample_distinct(model, props[0], 24, syntax=True, **KW)[0]
    run = dict(decode.last_distinct)
    print(f"syntax=True: {run}; e.g. {[tok.decode(s) for s in _toks(res)[:3]]}")
    assert run["syntax"] and run["dropped_masked"] == 0 and len(res) == 24 and run["unfinished"] == [0]      # the budget forces every hypothesis shut
    _wellformed_ends(res)
    assert len({tuple(t) for t in _toks(res)}) == 24
    assert all(SS.well_formed(tok.decode(s)) for s in _toks(res))


def test_a_prefix_starts_every_sample_and_is_not_scored(model, tok, props):
    from spmm_amd import decode
    sys.path.insert(0, ROOT)
    import pv2smiles
    pre = pv2smiles.prefix_ids(tok, "c1ccc(")
    P = len(pre)
    a = decode.sample_distinct(model, props[0], 16, prefix=pre, syntax=True, **KW)[0]
    assert decode.last_distinct["prefix_tokens"] == P and len(a) == 16
    b = decode.sample_distinct(model, props[0], 16, prefix=pre, syntax=True, prefill=False, **KW)[0]
    assert all(s[:P] == pre and tok.decode(s).startswith("c1ccc(") and SS.well_formed(tok.decode(s)) for s in _toks(a) + _toks(b))
    same = sum(x == y for x, y in zip(_toks(a), _toks(b)))
    worst = max([abs(pa - pb) / (len(sa) - P) for (pa, sa), (pb, sb) in zip(a, b) if sa == sb] or [0.0])
    print(f"prefix, prefill vs stepping: {same} / 16 samples identical, worst per-token score difference {worst:.5f}")
    assert same >= 0.9 * 16 and worst < 3e-2
    # the scores count the generated tokens only: the teacher-forced score of the positions after the prefix, renormalised over the allowed tokens
    c = decode.sample_distinct(model, props[0], 16, prefix=pre, **KW)[0]
    assert len(c) >= 4, "too little finished without the constraint: pick another bias"
    want = _teacher_forced(model, props[0], c, P=P)
    worst = max(abs(p - w) for (p, _), w in zip(c, want))
    print(f"prefix: {len(c)} hypotheses, largest |logp - teacher-forced score of the generated tokens| {worst:.3e}")
    assert worst <= LOGP_TOL


def test_the_scores_of_a_warped_search_are_those_of_the_warped_distribution(model, props):
    from spmm_amd import decode
    warp = dict(temperature=1.25, top_p=0.9)
    res = decode.sample_distinct(model, props[0], 24, **warp, **KW)[0]
    run = dict(decode.last_distinct)
    assert run["temperature"] == 1.25 and run["top_p"] == 0.9 and len(res) >= 8
    assert len({tuple(t) for t in _toks(res)}) == len(res)
    want = _teacher_forced(model, props[0], res, warp=warp)
    worst = max(abs(p - w) for (p, _), w in zip(res, want))
    print(f"temperature 1.25, top_p 0.9: {len(res)} hypotheses, largest |logp - warped teacher-forced score| {worst:.3e}")
    assert worst <= LOGP_TOL
    # a top_k below the 8 rows of a decoder molecule: min_keep is 1 here.  (Under the grammar mask: [SEP] is rarely among the 3 most
    # probable tokens of this model, and the budget then forces every hypothesis shut.)
    res = decode.sample_distinct(model, props[0], 8, top_k=3, syntax=True, **KW)[0]
    assert decode.last_distinct["top_k"] == 3 and len(res) == 8 and len({tuple(t) for t in _toks(res)}) == 8


def test_refusals(model, props):
    from spmm_amd import decode
    with pytest.raises(ValueError, match="guidance=2.0.*out of scope"):
        decode.sample_distinct(model, props[0], 8, guidance=2.0)
    for n in (1025, 0):
        with pytest.raises(ValueError, match=r"outside \[1, 1024\]"):
            decode.sample_distinct(model, props[0], n)


def test_two_property_vectors_give_each_its_own_result(model, props):
    from spmm_amd import decode
    both = decode.sample_distinct(model, props, 16, **KW)
    run = dict(decode.last_distinct)
    assert run["groups"] == 2 and len(both) == 2 and _toks(both[0]) != _toks(both[1])
    for g in range(2):
        alone = decode.sample_distinct(model, props[g], 16, pv_base=g, **KW)[0]
        assert _toks(alone) == _toks(both[g]) and len(alone) >= 1
        assert max(abs(a[0] - b[0]) for a, b in zip(alone, both[g])) < 1e-4
