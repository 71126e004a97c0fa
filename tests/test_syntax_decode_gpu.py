"""Syntax-constrained PV -> SMILES decoding on the GPU: the grammar mask (ops.smiles_mask) in the fused searches -- deterministic, seeded
sampled, guided and truncated, from a prefix, through compaction and chunking -- against the host automaton (every hypothesis returned is
well-formed) and against its twins (the tensor-op bookkeeping with the host mask, compaction off).  Tiny configuration, the closed-form
weights with the peaky LM-head bias of tests/prefix_reference.py, the published 300-piece vocabulary."""
import os
import sys

import numpy as np
import pytest
import torch

from prefix_reference import peaky_lm

from spmm_amd import smiles_syntax as SS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS_ID, SEP_ID = 2, 3
GUIDED = dict(guidance=1.5, temperature=1.3, top_k=20, top_p=0.9)
SAMPLED = dict(k=2, max_steps=24, stochastic=True, seed=7)


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
def closing(env, tok):
    """The same weights with the LM-head bias lowered by 6 for every piece that opens a branch, a ring or a bracket, or that cannot follow an
    atom: under the constraint the plain model keeps opening branches until the budget forces them shut, so every molecule ends at the last
    position; this one ends molecules at different positions, which is what compaction needs."""
    O, SPMM, tiny_config, *_ = env
    sd = peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), seed=5, sep_gap=0.9)
    table = SS.SyntaxTable.from_vocab(tok.itos)
    b = sd["text_encoder.cls.predictions.bias"].clone()
    for v, text in enumerate(table.text):
        if text and (table.delta[v, 0] > 0 or table.toggle[v, 0] or int(table.end[v, SS.ATOM]) not in (SS.ATOM, SS.RING, SS.CLOSE)):
            b[v] -= 6.0
    sd["text_encoder.cls.predictions.bias"] = sd["text_encoder.cls.predictions.decoder.bias"] = b
    m = SPMM(config=None, spmm_config=tiny_config())
    m.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    m.tokenizer = tok
    return m.eval()


@pytest.fixture(scope="module")
def props64():
    return torch.randn(64, 53, generator=torch.Generator().manual_seed(12)) * 10.0


def _prefix(tok, fragment):
    sys.path.insert(0, ROOT)
    import pv2smiles
    return pv2smiles.prefix_ids(tok, fragment)


def _toks(res):
    return [[h[1] for h in mol] for mol in res]


def _all_well_formed(tok, res, starts=""):
    hyps = [h for mol in res for h in mol]
    assert len(hyps) >= 1
    for score, ids in hyps:
        text = tok.decode(ids)
        assert ids[0] == CLS_ID and ids[-1] == SEP_ID and SEP_ID not in ids[1:-1], ids
        assert SS.well_formed(text) and text.startswith(starts), (text, ids)
        assert score > -1e29 and np.isfinite(score), (score, text)
    return hyps


CASES = {
    "deterministic k5 N6": (6, dict(k=5, max_steps=24), ""),
    "sampled k2 N64": (64, SAMPLED, ""),
    "guided": (64, dict(SAMPLED, **GUIDED), ""),
    "guidance 0": (64, dict(SAMPLED, **dict(GUIDED, guidance=0.0)), ""),
    "prefix": (64, SAMPLED, "c1ccc("),
    "prefix guided": (64, dict(SAMPLED, **GUIDED), "c1ccc("),
    "prefix guided stepped": (64, dict(SAMPLED, prefill=False, **GUIDED), "c1ccc("),
    "prefix deterministic": (6, dict(k=5, max_steps=24), "c1ccc("),
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_hypothesis_of_a_constrained_search_is_well_formed(model, tok, props64, case, monkeypatch):
    from spmm_amd import decode, ops
    N, kw, fragment = CASES[case]
    kw = dict(kw, prefix=_prefix(tok, fragment)) if fragment else kw
    seen = []
    inner = ops.smiles_mask
    monkeypatch.setattr(ops, "smiles_mask", lambda lg, *a, **k: (seen.append((lg.shape[0], k.get("logits2") is not None)), inner(lg, *a, **k))[1])
    res = decode.beam_search_batched(model, props64[:N], syntax=True, **kw)
    run = dict(decode.last_run)
    hyps = _all_well_formed(tok, res, fragment)
    print(f"{case}: {len(hyps)} hypotheses from {N} molecules, {run['dropped_masked']} dropped, e.g. {tok.decode(hyps[0][1])!r}; {run}")
    assert run["syntax"] is True and sum(1 for mol in res if mol) >= N // 2
    # one mask launch for the first pick and one per position, on both halves exactly when there is a guidance baseline
    assert len(seen) == 1 + run["positions"]
    assert all(two == (run["baseline_rows"] > 0) for _, two in seen)


def test_the_constraint_bites(model, tok, props64):
    """The unconstrained seeded sampled search of the same molecules returns strings the automaton rejects (an untrained decoder emits
    pieces with no regard for syntax: with seed 7, 98 of the 100 hypotheses fail, the first of them '[NH+])ccCCN(CCN(' -- an unopened ')'
    and two open branches); with the constraint none does (the "sampled k2 N64" case above)."""
    from spmm_amd import decode
    res = decode.beam_search_batched(model, props64, **SAMPLED)
    texts = [tok.decode(ids) for mol in res for _, ids in mol]
    bad = [t for t in texts if not SS.well_formed(t)]
    print(f"unconstrained, seed {SAMPLED['seed']}: {len(bad)} of {len(texts)} hypotheses are not well-formed, the first: {bad[:1]}")
    assert len(texts) >= 1 and len(bad) >= 1


def test_the_fused_route_and_the_tensor_op_route_with_the_host_mask_agree(model, tok, props64, monkeypatch):
    """Seeded, guided and truncated, N = 12, k = 3, 12 positions: the kernel route (mask, warp and beam step as launches) against the
    tensor-op bookkeeping with smiles_syntax.allowed and warp_logits, held to what tests/test_guided_decode_gpu.py asks of these two routes:
    identical hypotheses for at least 0.9 N molecules, scores within 1e-4 where the tokens agree.  The masks themselves are decisions and
    equal exactly; what differs is the rounding of the warp and the softmax."""
    from spmm_amd import decode, ops
    kw = dict(k=3, max_steps=12, stochastic=True, seed=9, guidance=2.0, temperature=0.8, top_p=0.9, syntax=True)
    calls = []
    inner = ops.smiles_mask
    monkeypatch.setattr(ops, "smiles_mask", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    for prefix in (None, _prefix(tok, "C1CC(")):
        monkeypatch.setattr(decode, "FUSED_BEAM_STEP", True)
        fused = decode.beam_search_batched(model, props64[:12], prefix=prefix, **kw)
        n_fused = len(calls)
        monkeypatch.setattr(decode, "FUSED_BEAM_STEP", False)
        plain = decode.beam_search_batched(model, props64[:12], prefix=prefix, **kw)
        assert n_fused >= 2 and len(calls) == n_fused                      # the tensor-op route never launches the kernel
        _all_well_formed(tok, fused)
        _all_well_formed(tok, plain)
        same, worst = 0, 0.0
        for ha, hb in zip(fused, plain):
            same += int(bool(ha) and _toks([ha]) == _toks([hb]))
            for (pa, sa), (pb, sb) in zip(ha, hb):
                if sa == sb:
                    worst = max(worst, abs(pa - pb))
        print(f"constrained search, fused vs tensor-op route (prefix: {prefix is not None}): identical for {same} / 12, worst score difference {worst:.2e}")
        assert same >= 0.9 * 12 and worst < 1e-4
        calls.clear()


def test_compaction_does_not_change_a_constrained_search(closing, tok, props64):
    """The mask reads the histories of a compacted batch through `mol`: compaction on against off, token for token, scores to 1e-4 (what
    the project allows between a compacted and a whole batch)."""
    from spmm_amd import decode
    kw = dict(k=2, max_steps=40, stochastic=True, seed=7, syntax=True)
    on = decode.beam_search_batched(closing, props64, **kw)
    run = dict(decode.last_run)
    off = decode.beam_search_batched(closing, props64, compact=False, **kw)
    print(f"constrained, compaction on: {run}")
    assert run["compactions"] >= 1 and run["final_batch"] < 64 and decode.last_run["compactions"] == 0
    assert _toks(on) == _toks(off) and any(_toks(on))
    for x, y in zip(on, off):
        for (px, _), (py, _) in zip(x, y):
            assert abs(px - py) < 1e-4, (px, py)
    _all_well_formed(tok, on)


def test_constrained_generation_does_not_depend_on_the_chunking(model, tok):
    from spmm_amd import decode
    pv = torch.randn(53, generator=torch.Generator().manual_seed(31)) * 2
    kw = dict(k=2, max_steps=16, seed=3, syntax=True)
    got = decode.generate_with_property(model, pv, 24, **kw)
    gen = dict(decode.last_generate)
    assert gen["syntax"] is True and gen["chunks"] == 1
    assert decode.generate_with_property(model, pv, 24, chunk=7, **kw) == got
    assert decode.last_generate["chunks"] == 4 and decode.last_generate["dropped_masked"] == gen["dropped_masked"]
    done = [s for s in got if s]
    assert len(done) >= 12 and all(SS.well_formed(tok.decode(s)) for s in done)
    guided = decode.generate_with_property(model, pv, 24, prefix=_prefix(tok, "c1ccc("), **kw, **GUIDED)
    assert decode.generate_with_property(model, pv, 24, chunk=7, prefix=_prefix(tok, "c1ccc("), **kw, **GUIDED) == guided
    done = [s for s in guided if s]
    assert done and all(SS.well_formed(tok.decode(s)) and tok.decode(s).startswith("c1ccc(") for s in done)


def test_an_open_prefix_is_closed_exactly_or_refused(model, tok, props64):
    """'C1CC(' leaves a ring and a branch open and needs an atom: cost 3.  max_steps = 3 is exactly enough, max_steps = 2 is refused."""
    from spmm_amd import decode
    pre = _prefix(tok, "C1CC(")
    assert [tok.itos[i] for i in pre] == ["[CLS]", "##C1", "##CC("]
    for kw in (dict(k=5), dict(k=2, stochastic=True, seed=7)):
        res = decode.beam_search_batched(model, props64[:6], max_steps=3, prefix=pre, syntax=True, **kw)
        hyps = _all_well_formed(tok, res, "C1CC(")
        assert all(len(ids) <= len(pre) + 3 + 1 for _, ids in hyps) and all(mol for mol in res)
        with pytest.raises(ValueError, match="needs 3 more tokens to close; max_steps=2"):
            decode.beam_search_batched(model, props64[:6], max_steps=2, prefix=pre, syntax=True, **kw)


def test_syntax_off_is_the_search_of_today_launch_for_launch(model, props64, monkeypatch):
    from spmm_amd import decode, ops
    log = []
    inner = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (log.append(name), inner(name, *a))[1])
    for kw in (dict(k=5, max_steps=12), dict(SAMPLED, max_steps=12), dict(SAMPLED, max_steps=12, **GUIDED)):
        log.clear()
        plain = decode.beam_search_batched(model, props64[:6], **kw)
        run, launches = dict(decode.last_run), list(log)
        for off in (None, False):
            log.clear()
            assert decode.beam_search_batched(model, props64[:6], syntax=off, **kw) == plain
            assert dict(decode.last_run) == run and run["syntax"] is False and log == launches
        assert "spmm_smiles_mask" not in launches and any(plain)
        log.clear()
        decode.beam_search_batched(model, props64[:6], syntax=True, **kw)
        assert log.count("spmm_smiles_mask") == 1 + decode.last_run["positions"]
        assert [n for n in log if n != "spmm_smiles_mask"][:50] == launches[:50]      # the same sequence with the mask slotted in
    pv = props64[0] / 5
    a = decode.generate_with_property(model, pv, 8, k=2, seed=3, max_steps=12)
    gen = dict(decode.last_generate)
    assert decode.generate_with_property(model, pv, 8, k=2, seed=3, max_steps=12, syntax=False) == a and dict(decode.last_generate) == gen


def test_a_constrained_search_stays_eager(model, props64, monkeypatch):
    from spmm_amd import decode
    monkeypatch.setattr(decode, "_decode_graphed", lambda *a, **k: (_ for _ in ()).throw(AssertionError("graph replay under syntax=True")))
    assert any(decode.beam_search_batched(model, props64[:4], k=3, max_steps=8, graph=True, syntax=True))
