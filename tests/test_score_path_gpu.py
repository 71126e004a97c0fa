"""spmm_amd.score on the GPU: `score_smiles` / `score_products` against the fp32 CPU oracle (oracle.spmm_oracle's module API and
tests/rxn_reference.py, log_softmax in float64), tiny configuration, closed-form weights, eval mode; the searches' reported
log-probabilities against teacher-forced scoring of their own hypotheses; the drivers.

Tolerances.  DESIGN.md section 5's rule: a new path may be 1.5 x as far from the oracle as the path that is already trusted, measured in
the same run on the same inputs -- here `engine=False`, the dense module-facade call the parent commit already had.  Measured on an
MI355X, largest |log p - oracle| over the pairs, per token / per sequence sum:
  score_smiles    engine=False 4.122e-3 / 4.385e-3     engine, fused 4.122e-3 / 4.385e-3     engine, composite ending 4.122e-3 / 4.385e-3
  score_products  engine=False 6.946e-3 / 1.135e-2     engine, fused 6.946e-3 / 1.135e-2     engine, composite ending 6.946e-3 / 1.135e-2
(the engine path runs the same GEMM, LayerNorm and attention kernels on the same rows as the facade call, so the largest deviation is the
same element to four digits).  With the closed-form weights the condition barely moves the score (the oracle's log p of one molecule under
the three vectors spreads by 1.2e-3, less than the deviation), so `test_score_smiles_on_seeded_weights_follows_the_vector` repeats the
comparison on seeded, scaled full-rank weights, where a sequence bound to the wrong vector shows.
Every figure is printed before it is asserted."""
import csv
import math
import os
import subprocess
import sys

import pytest
import torch

from helpers_gpu import f32_bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = 1.5
CLS, SEP = 2, 3
LENS = (2, 3, 9, 16, 9, 9)                      # 6 molecules; three of one length
PAIRS = [(0, 0), (1, 2), (0, 2), (2, 2), (1, 3), (2, 1), (0, 4), (1, 2)]       # (1, 2) twice; molecule 2 under all three vectors; molecule 5 unused


def _sequences(lens, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), max(lens), dtype=torch.long)
    for i, n in enumerate(lens):
        ids[i, 0] = CLS
        ids[i, 1:n - 1] = torch.randint(4, 300, (n - 2,), generator=g)
        ids[i, n - 1] = SEP
    return ids, (ids != 0).long()


def _dev(sc, ref_tok):
    """Largest deviation of a Scores from the reference's per-token log-probabilities [P, L - 1] (zero beyond the labels): per token, per sum."""
    tok = sc.token_logp.detach().double().cpu()
    assert tuple(tok.shape) == tuple(ref_tok.shape), (tok.shape, ref_tok.shape)
    return (tok - ref_tok).abs().max().item(), (sc.logp.detach().double().cpu() - ref_tok.sum(1)).abs().max().item()


def _within(tag, new, old):
    print(f"[score] {tag}: per token {new[0]:.3e} (engine=False {old[0]:.3e}), per sequence {new[1]:.3e} (engine=False {old[1]:.3e}); rule {RULE} x")
    assert new[0] <= RULE * old[0] and new[1] <= RULE * old[1], (tag, new, old)


def _well_formed(sc, P, L, n_ref):
    assert tuple(sc.logp.shape) == (P,) and sc.logp.dtype == torch.float32 and tuple(sc.token_logp.shape) == (P, L - 1)
    assert sc.n_tokens.dtype == torch.int64 and sc.n_tokens.cpu().tolist() == n_ref
    assert torch.isfinite(sc.logp).all() and (sc.logp < 0).all()


# ------------------------------------------------------------------------------------------------------------------ score_smiles
@pytest.fixture(scope="module")
def world(env):
    """The tiny model with closed-form weights, 3 property vectors (the second with 20 properties unknown), 6 molecules, the oracle's
    per-token log-probabilities of the 8 pairs (computed once) and the three routes' scores."""
    from helpers_gpu import _tiny_train_model
    from spmm_amd import decode, score
    O = env[0]
    oc = O.tiny_cfg()
    sd = O.closed_form_state_dict(oc)
    m = _tiny_train_model(env, dropout=False).eval()
    g = torch.Generator().manual_seed(31)
    pv = torch.randn(3, 53, generator=g)
    pm = torch.zeros(3, 53)
    pm[1, torch.randperm(53, generator=g)[:20]] = 1
    ids, mask = _sequences(LENS, seed=32)
    pairs = torch.tensor(PAIRS)
    om = O.OracleModule(sd, oc)
    pe = decode.encode_properties(om, pv, pm)
    ref = torch.zeros(len(PAIRS), ids.shape[1] - 1, dtype=torch.float64)
    for p, (q, mol) in enumerate(PAIRS):
        n = LENS[mol]
        logits = om.text_encoder(ids[mol:mol + 1, :n], attention_mask=torch.ones(1, n, dtype=torch.long), encoder_hidden_states=pe[q:q + 1],
                                 encoder_attention_mask=torch.ones(1, pe.shape[1], dtype=torch.long), is_decoder=True, return_logits=True)
        ref[p, :n - 1] = torch.log_softmax(logits.double(), -1)[0, :-1].gather(1, ids[mol, 1:n, None])[:, 0]
    w = dict(O=O, m=m, pv=pv, pm=pm, ids=ids, mask=mask, pairs=pairs, ref=ref)
    w["facade"] = score.score_smiles(m, pv.cuda(), ids, mask, pairs, prop_mask=pm.cuda(), engine=False)
    w["fused"] = score.score_smiles(m, pv, ids, mask, pairs, prop_mask=pm)
    w["unfused"] = score.score_smiles(m, pv, ids, mask, pairs, prop_mask=pm, fused=False)
    return w


def test_score_smiles_matches_the_oracle(world):
    w = world
    n_ref = [LENS[mol] - 1 for _, mol in PAIRS]
    old = _dev(w["facade"], w["ref"])
    spread = (w["ref"].sum(1)[[1, 2, 3]].max() - w["ref"].sum(1)[[1, 2, 3]].min()).item()
    print(f"[score] oracle log p of molecule 2 under the three vectors: {w['ref'].sum(1)[[1, 2, 3]].tolist()} (spread {spread:.3e})")
    for tag in ("fused", "unfused"):
        _well_formed(w[tag], len(PAIRS), w["ids"].shape[1], n_ref)
        _within(f"score_smiles, {tag}", _dev(w[tag], w["ref"]), old)
    assert torch.equal(w["fused"].logp[1], w["fused"].logp[7]) and torch.equal(w["fused"].token_logp[1], w["fused"].token_logp[7])   # the repeated pair
    assert not w["fused"].token_logp[0, 1:].any()                                  # the 2-token molecule: one label, zeros beyond it
    # device inputs and the default pairing (row i with row i)
    from spmm_amd import score
    sc = score.score_smiles(w["m"], w["pv"].cuda(), w["ids"][:3].cuda(), w["mask"][:3].cuda(), prop_mask=w["pm"].cuda())
    want = score.score_smiles(w["m"], w["pv"], w["ids"][:3], w["mask"][:3], torch.tensor([[0, 0], [1, 1], [2, 2]]), prop_mask=w["pm"])
    assert torch.equal(sc.logp, want.logp) and torch.equal(sc.token_logp, want.token_logp)


def test_score_smiles_on_seeded_weights_follows_the_vector(env):
    """Seeded full-rank weights (oracle.init_state_dict) with the cross-attention output projections scaled by 10 and the tied word embedding
    by 20, so that the next-token distribution is far from uniform and follows the vector: the oracle's scores of ONE molecule under the
    three vectors are 0.16 .. 0.35 apart.  Both GPU routes share the bf16 error of the text path (0.13 on a log p of -111), so the binding is
    checked where that error cancels: the engine path against engine=False, which gathers every pair's vector itself.  A sequence bound to
    another pair's vector would be a gap away; the two routes must agree within a quarter of the smallest gap."""
    O, SPMM, tiny_config, *_ = env
    from spmm_amd import decode, score
    oc = O.tiny_cfg()
    sd = dict(O.init_state_dict(oc, seed=21))
    for name in list(sd):
        if name.startswith("text_encoder.bert.") and name.endswith("crossattention.output.dense.weight"):
            sd[name] = sd[name] * 10
    word = sd["text_encoder.bert.embeddings.word_embeddings.weight"] * 20
    sd["text_encoder.bert.embeddings.word_embeddings.weight"] = sd["text_encoder.cls.predictions.decoder.weight"] = word
    m = SPMM(config=None, spmm_config=tiny_config())
    m.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    m.eval()
    pv = torch.randn(3, 53, generator=torch.Generator().manual_seed(33)) * 2
    ids, mask = _sequences(LENS, seed=32)
    pe = decode.encode_properties(O.OracleModule(sd, oc), pv)
    om = O.OracleModule(sd, oc)
    ref = torch.zeros(len(PAIRS), ids.shape[1] - 1, dtype=torch.float64)
    for p, (q, mol) in enumerate(PAIRS):
        n = LENS[mol]
        logits = om.text_encoder(ids[mol:mol + 1, :n], attention_mask=torch.ones(1, n, dtype=torch.long), encoder_hidden_states=pe[q:q + 1],
                                 encoder_attention_mask=torch.ones(1, pe.shape[1], dtype=torch.long), is_decoder=True, return_logits=True)
        ref[p, :n - 1] = torch.log_softmax(logits.double(), -1)[0, :-1].gather(1, ids[mol, 1:n, None])[:, 0]
    pairs = torch.tensor(PAIRS)
    facade, engine = score.score_smiles(m, pv.cuda(), ids, mask, pairs, engine=False), score.score_smiles(m, pv, ids, mask, pairs)
    _within("score_smiles, seeded weights", _dev(engine, ref), _dev(facade, ref))
    three = ref.sum(1)[[1, 2, 3]]
    gaps = [abs(float(three[i] - three[j])) for i, j in ((0, 1), (0, 2), (1, 2))]
    apart = (engine.logp - facade.logp).abs().max().item()
    print(f"[score] seeded weights: oracle log p of molecule 2 under the three vectors {[round(x, 4) for x in three.tolist()]} (gaps "
          f"{[round(g, 4) for g in gaps]}); engine path {apart:.3e} from engine=False, which gathers the vector of every pair itself")
    assert 4 * apart < min(gaps), (apart, gaps)


def test_pairs_scored_one_at_a_time(world):
    """Every pair in a call of its own: within the same tolerance of the oracle, and the same ranking as the batch."""
    from spmm_amd import score
    w = world
    one = [score.score_smiles(w["m"], w["pv"], w["ids"], w["mask"], w["pairs"][p:p + 1], prop_mask=w["pm"]) for p in range(len(PAIRS))]
    sc = score.Scores(torch.cat([s.logp for s in one]), torch.cat([s.n_tokens for s in one]), torch.cat([s.token_logp for s in one]))
    _within("score_smiles, one pair per call", _dev(sc, w["ref"]), _dev(w["facade"], w["ref"]))
    uniq = list(range(7))                                                        # (without the repeated pair: a tie has no ranking)
    r_one, r_all, r_ref = (torch.argsort(x[uniq], descending=True).tolist() for x in (sc.logp.cpu(), w["fused"].logp.cpu(), w["ref"].sum(1).float()))
    print(f"[score] ranking of the 7 distinct pairs: one at a time {r_one}, batch {r_all}, oracle {r_ref}")
    assert r_one == r_all


def test_fused_against_the_composite_ending(world, monkeypatch):
    """Same rows, same weights: the two endings evaluate one formula in fp32, so they agree within the kernel test's bound -- max(8 E32, 4 ulp)
    from the fp32 twin of the float64 evaluation of THESE rows (helpers_gpu.f32_bound) -- per token, times the token count per sequence."""
    from spmm_amd import ops, score
    w = world
    seen = {}
    real = ops.lm_score

    def spy(y, Wd, bias, ids, **kw):
        seen.update(y=y.float().cpu(), Wd=Wd.float().cpu(), bias=bias.cpu(), ids=ids.cpu().long(), row_of=kw["row_of"].cpu(), L=kw["L"])
        return real(y, Wd, bias, ids, **kw)
    monkeypatch.setattr(ops, "lm_score", spy)
    fused = score.score_smiles(w["m"], w["pv"], w["ids"], w["mask"], w["pairs"], prop_mask=w["pm"])
    monkeypatch.undo()
    assert torch.equal(fused.logp, w["fused"].logp)
    d = seen["row_of"]
    lab = torch.where(d % seen["L"] < seen["L"] - 1, seen["ids"][(d + 1).clamp(max=seen["ids"].numel() - 1)], torch.zeros_like(d))

    def twin(dtype):
        lp = torch.log_softmax(seen["y"].to(dtype) @ seen["Wd"].to(dtype).T + seen["bias"].to(dtype), -1).gather(1, lab[:, None])[:, 0]
        return torch.where(lab > 0, lp, torch.zeros_like(lp))
    E32, bound = f32_bound(twin(torch.float64), twin(torch.float32))
    dt = (w["fused"].token_logp - w["unfused"].token_logp).abs().max().item()
    ds = ((w["fused"].logp - w["unfused"].logp).abs() / w["fused"].n_tokens.float()).max().item()
    print(f"[score] fused against composite ending: per token {dt:.3e}, per sequence / tokens {ds:.3e}; E32 {E32:.3e}, bound {bound:.3e}")
    assert dt <= bound and ds <= bound
    assert torch.equal(w["fused"].n_tokens, w["unfused"].n_tokens)


def test_errors_and_the_empty_call(world):
    from spmm_amd import ops, score
    w, m = world, world["m"]
    holes = w["mask"].clone()
    holes[3, 4] = 0
    empty_row = w["mask"].clone()
    empty_row[1] = 0
    for bad in (holes, empty_row):
        for engine in (True, False):
            with pytest.raises(ValueError, match="non-empty prefix"):
                score.score_smiles(m, w["pv"], w["ids"], bad, w["pairs"], engine=engine)
    for bad in ([[3, 0]], [[0, 6]], [[-1, 0]]):
        with pytest.raises(IndexError, match="not there"):
            score.score_smiles(m, w["pv"], w["ids"], w["mask"], torch.tensor(bad))
    with pytest.raises(ValueError, match="row i is paired with row i"):
        score.score_smiles(m, w["pv"], w["ids"], w["mask"])
    long_ids = torch.full((1, ops.ATTN_MAXL + 1), 5, dtype=torch.long)
    with pytest.raises(ValueError, match=f"exceeds the {ops.ATTN_MAXL}"):
        score.score_smiles(m, w["pv"][:1], long_ids, torch.ones_like(long_ids))
    for engine in (True, False):
        sc = score.score_smiles(m, w["pv"].cuda(), w["ids"], w["mask"], torch.zeros(0, 2, dtype=torch.long), engine=engine)
        assert tuple(sc.logp.shape) == (0,) and tuple(sc.n_tokens.shape) == (0,) and tuple(sc.token_logp.shape) == (0, w["ids"].shape[1] - 1)


# ---------------------------------------------------------------------------------------------------------------- score_products
S_LENS, C_LENS = (1, 7, 17), (2, 3, 9, 16, 9)
R_PAIRS = [(0, 0), (1, 2), (0, 2), (2, 2), (1, 3), (2, 1), (1, 2)]             # (1, 2) twice; candidate 2 under all three sources; candidate 4 unused


@pytest.fixture(scope="module")
def rxn_world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import rxn_reference as R
    import spmm_oracle as O
    from test_rxn_path_gpu import build          # tests/test_rxn_path_gpu.py: the tiny SPMMRxn on the closed-form weights and its state dict
    from spmm_amd import score
    sd, o_dec, o_enc, m = build(O, bias=R.ranked_lm_bias(300, BIAS_SEED, 2, BIAS_MARGIN))
    g = torch.Generator().manual_seed(41)
    sids = torch.zeros(3, max(S_LENS), dtype=torch.long)
    for i, n in enumerate(S_LENS):
        sids[i, :n] = torch.randint(4, 300, (n,), generator=g)
    smask = (sids != 0).long()
    pids, pmask = _sequences(C_LENS, seed=42)
    ref = torch.zeros(len(R_PAIRS), pids.shape[1] - 1, dtype=torch.float64)
    for p, (s, c) in enumerate(R_PAIRS):
        n, ns = C_LENS[c], S_LENS[s]
        emb = R.encode(sd, o_enc, sids[s:s + 1, :ns], smask[s:s + 1, :ns])
        logits = R.decoder_logits(sd, o_dec, emb, smask[s:s + 1, :ns], pids[c:c + 1, :n])
        ref[p, :n - 1] = torch.log_softmax(logits.double(), -1)[0, :-1].gather(1, pids[c, 1:n, None])[:, 0]
    pairs = torch.tensor(R_PAIRS)
    w = dict(m=m, sids=sids, smask=smask, pids=pids, pmask=pmask, pairs=pairs, ref=ref, sd=sd, o_dec=o_dec, o_enc=o_enc, R=R)
    w["facade"] = score.score_products(m, sids, smask, pids, pmask, pairs, engine=False)
    w["fused"] = score.score_products(m, sids, smask, pids, pmask, pairs)
    w["unfused"] = score.score_products(m, sids, smask, pids, pmask, pairs, fused=False)
    return w


def test_score_products_matches_the_restatement(rxn_world):
    w = rxn_world
    n_ref = [C_LENS[c] - 1 for _, c in R_PAIRS]
    old = _dev(w["facade"], w["ref"])
    for tag in ("fused", "unfused"):
        _well_formed(w[tag], len(R_PAIRS), w["pids"].shape[1], n_ref)
        _within(f"score_products, {tag}", _dev(w[tag], w["ref"]), old)
    assert torch.equal(w["fused"].logp[1], w["fused"].logp[6])
    from spmm_amd import ops, score
    with pytest.raises(ValueError, match="non-empty prefix"):
        score.score_products(w["m"], w["sids"], torch.zeros_like(w["smask"]), w["pids"], w["pmask"], w["pairs"])
    with pytest.raises(IndexError, match="not there"):
        score.score_products(w["m"], w["sids"], w["smask"], w["pids"], w["pmask"], torch.tensor([[3, 0]]))
    long_ids = torch.full((1, ops.ATTN_MAXL + 1), 5, dtype=torch.long)
    with pytest.raises(ValueError, match=f"limited to {ops.ATTN_MAXL}"):
        score.score_products(w["m"], long_ids, torch.ones_like(long_ids), w["pids"][:1], w["pmask"][:1])
    sc = score.score_products(w["m"], w["sids"], w["smask"], w["pids"], w["pmask"], torch.zeros(0, 2, dtype=torch.long))
    assert tuple(sc.logp.shape) == (0,) and tuple(sc.token_logp.shape) == (0, w["pids"].shape[1] - 1)


# ------------------------------------------------------------------------------------------------------------- decode cross-check
# Largest |reported log-probability - teacher-forced score| per hypothesis, measured on an MI355X with this file's inputs:
#   beam_search_batched against score_smiles    6.302e-3 (8 hypotheses of 4 tokens: 1.6e-3 per token)
#   predict_products against score_products     7.13e-4 (hypotheses of 4 and 6 tokens)
# The two paths share the weights and differ in their attention kernels (K/V-cache decode kernels against the packed-row kernels), so the
# difference is a few bf16 roundings of the activations per token (the logits reach 9, where one bf16 step is 0.06): noise of the number
# format, not a defect of either path.  The assertion is 1.5 x the measured maximum.
X_PV, X_RXN = 6.31e-3, 7.14e-4
BIAS_SEED, BIAS_MARGIN = 23, 0.6            # rxn_reference.ranked_lm_bias: [SEP] is the 2nd largest LM-head bias, so a 2-beam search ends hypotheses


def _rescored(hyps, score_fn):
    """hyps: per condition a list of (log-probability, ids incl. [CLS]); -> [(reported, teacher-forced, tokens)] over every hypothesis."""
    flat = [(n, p, seq) for n, hs in enumerate(hyps) for p, seq in hs]
    assert flat, "the search finished no hypothesis: the cross-check would be vacuous"
    L = max(len(seq) for _, _, seq in flat)
    ids = torch.zeros(len(flat), L, dtype=torch.long)
    for i, (_, _, seq) in enumerate(flat):
        assert seq[0] == CLS
        ids[i, :len(seq)] = torch.tensor(seq)
    pairs = torch.tensor([[n, i] for i, (n, _, _) in enumerate(flat)])
    sc = score_fn(ids, (ids != 0).long(), pairs)
    assert sc.n_tokens.cpu().tolist() == [len(seq) - 1 for _, _, seq in flat]
    return [(p, float(lp), len(seq) - 1) for (_, p, seq), lp in zip(flat, sc.logp.cpu().tolist())]


def _cross_check(tag, rows, tol):
    worst = max(abs(p - lp) for p, lp, _ in rows)
    per_tok = max(abs(p - lp) / n for p, lp, n in rows)
    print(f"[score] {tag}: {len(rows)} hypotheses of {min(n for *_, n in rows)}..{max(n for *_, n in rows)} tokens; largest |reported - teacher-forced| "
          f"{worst:.3e} ({per_tok:.3e} per token)")
    assert tol is not None and worst <= RULE * tol, (tag, worst, tol)


def test_beam_search_scores_are_the_teacher_forced_scores(env):
    O, SPMM, tiny_config, *_ = env
    import rxn_reference as R
    from spmm_amd import decode, score
    sd = dict(O.closed_form_state_dict(O.tiny_cfg()))
    sd["text_encoder.cls.predictions.bias"] = sd["text_encoder.cls.predictions.decoder.bias"] = R.ranked_lm_bias(300, BIAS_SEED, 2, BIAS_MARGIN)
    m = SPMM(config=None, spmm_config=tiny_config())
    m.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    m.eval()
    props = torch.randn(4, 53, generator=torch.Generator().manual_seed(4)) * 2
    hyps = decode.beam_search_batched(m, props, k=2, max_steps=12)
    rows = _rescored(hyps, lambda ids, mask, pairs: score.score_smiles(m, props, ids, mask, pairs))
    _cross_check("beam_search_batched against score_smiles", rows, X_PV)


def test_predict_products_scores_are_the_teacher_forced_scores(rxn_world):
    from test_rxn_path_gpu import reactions
    from spmm_amd import decode, score
    m = rxn_world["m"]
    ids, mask = reactions(6)
    hyps = decode.predict_products(m, ids, mask, k=2, max_steps=12)
    rows = _rescored(hyps, lambda pids, pmask, pairs: score.score_products(m, ids, mask, pids, pmask, pairs))
    _cross_check("predict_products against score_products", rows, X_RXN)


# ---------------------------------------------------------------------------------------------------------------------- drivers
def _run(script, *argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), *argv], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("rxn", [False, True], ids=["pv", "rxn"])
def test_score_driver_in_a_fresh_process(tmp_path, rxn):
    """score.py --synthetic 8 --tiny: a CSV with 8 rows in input order and perplexity == exp(-logp / tokens)."""
    import score as D
    from pv2smiles import synthetic_vocab
    from rxn_predict import synthetic_reactions
    from smiles2pv import synthetic_smiles
    out = str(tmp_path / "scores.csv")
    _run("score.py", *(["--rxn"] if rxn else []), "--synthetic", "8", "--tiny", "--batch_size", "3", "--output", out)
    vocab = synthetic_vocab(300)
    want = synthetic_reactions(vocab, 8, 0)[1] if rxn else synthetic_smiles(vocab, 8, 0)
    with open(out, newline="") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0].keys()) == D.COLUMNS and len(rows) == 8
    assert [r["smiles"] for r in rows] == want and [int(r["line"]) for r in rows] == list(range(1, 9))
    for r in rows:
        lp, n = float(r["logp"]), int(r["tokens"])
        assert n >= 2 and lp < 0
        assert float(r["logp_per_token"]) == lp / n and float(r["perplexity"]) == math.exp(-lp / n)


def test_retrieve_driver_reranks_by_likelihood_only_when_asked(tmp_path):
    a, b = str(tmp_path / "lik.csv"), str(tmp_path / "match.csv")
    _run("retrieve.py", "--synthetic", "32", "--tiny", "--top_k", "8", "--rerank", "4", "--rerank_by", "likelihood", "--output", a)
    _run("retrieve.py", "--synthetic", "32", "--tiny", "--top_k", "8", "--rerank", "4", "--output", b)
    with open(a, newline="") as f:
        lik = list(csv.DictReader(f))
    with open(b, newline="") as f:
        match = list(csv.DictReader(f))
    assert "logp_per_token" in lik[0] and "logp_per_token" not in match[0]
    assert list(match[0].keys()) == ["rank", "library_line", "smiles", "cosine", "match_probability"]
    vals = [float(r["logp_per_token"]) for r in lik[:4]]
    assert vals == sorted(vals, reverse=True) and all(r["logp_per_token"] == "" for r in lik[4:])
    assert all(r["match_probability"] == "" for r in lik) and all(r["match_probability"] != "" for r in match[:4])
    assert sorted(r["library_line"] for r in lik) == sorted(r["library_line"] for r in match)        # the same shortlist, another order
