"""Reaction prediction on the engine (spmm_amd.decode.RxnDecoder / predict_products / greedy_products, spmm_amd.rxn.SPMMRxn) against the
sequential CPU restatement of the reference's `evaluate` / `evaluate_beam` (tests/rxn_reference.py), at the tiny configuration: decoder
configs/config_bert_tiny.json (2 layers, 1 fusion layer), encoder the same with num_hidden_layers = fusion_layer; reactions with source
lengths 1, 3, 7, 16, 17 and 24 tokens in one batch.

Two models.  (a) FULL-RANK seeded random weights (rxn_reference.random_state_dict): what the decoder reads from its memory decides the
hypotheses -- the end-to-end comparisons (free-running search, greedy, batch independence) run on it, after asserting on the CPU that the
restatement's results differ between reactions.  Its LM bias (leaders_lm_bias, seed 23, N(0, 0.3^2)) lifts the two largest entries by 0.5
and puts [SEP] 0.8 above the third: the bias's own k-th and (k+1)-th entries are 0.5 apart for k = 3 (asserted; the reason given at
tests/test_step_gpu.py:891), but here the hidden state moves a logit by ~0.6, so a margin in the bias cannot rule near-ties out.  The
reactions are therefore chosen on the CPU, by the restatement's own margins: candidates (rxn_reference.reaction) whose best hypothesis
does not change under three N(0, 0.015^2) perturbations of the logits (SEL: the first four per length of candidates 0..43; the greedy rows
GSEL: every argmax leads its runner-up by >= 0.04).  bf16 moves a log-probability by ~0.012 at most here.
(b) The oracle's CLOSED-FORM weights with [SEP] third in a N(0, 3^2) bias (ranked_lm_bias): rank-2 matrices, every reaction behaves alike
-- kept for what does not need the memory to matter: the k*k stopping rule and the compaction."""
import csv
import os
import subprocess
import sys
from dataclasses import replace

import pytest
import torch

import rxn_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [1, 3, 7, 16, 17, 24]
K, T = 3, 14
SEED, MARGIN = 23, 0.6
BIAS_MARGIN, SEP_MARGIN = 0.5, 0.8      # model (a): leaders_lm_bias
SEL = [0, 13, 2, 3, 4, 5, 6, 25, 8, 9, 10, 11, 12, 31, 14, 15, 16, 17, 18, 43, 26, 21, 22, 23]       # candidate c has LENS[c % 6] tokens
GSEL = [48, 55, 38, 39, 4, 35, 66, 67, 56, 111, 40, 47]
TOL = 3e-2                      # log-probabilities, cached step against the whole-prefix forward (test_cached_decoder_step_matches_full_prefix_forward)
# Where 3e-2 is not met, DESIGN.md section 5's rule: 1.5 x the deviation of the trusted path -- the facade loop on the HIP model -- from the same
# restatement on the same GPU.  Measured on an MI355X (cached step / facade loop): closed-form weights 1.19e-2 / 1.19e-2 (2 layers) and
# 1.75e-2 / 1.75e-2 (3 layers); full-rank weights 2.93e-2 / 2.93e-2 (2 layers: within 3e-2) and 3.84e-2 / 3.84e-2 (3 layers: 1.5 x 3.84e-2).
TOL_BY_CASE = {(3, "random"): 1.5 * 3.84e-2}


def reactions(N, seed=4):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(N, max(LENS), dtype=torch.long)
    for n in range(N):
        L = LENS[n % len(LENS)]
        ids[n, :L] = torch.randint(4, 300, (L,), generator=g)
    return ids, (ids != 0).long()


def build(O, layers=2, bias=None, xscale=1.0, init="closed"):
    """-> (state dict, oracle decoder / encoder configs, HIP model).  init: "closed" (model (b)) or "random" (model (a), needs `bias`)."""
    from spmm_amd.config import tiny_config
    from spmm_amd.rxn import SPMMRxn
    o_dec = replace(O.tiny_cfg().text, num_hidden_layers=layers)
    o_enc = R.encoder_cfg(o_dec)
    sd = R.closed_form_state_dict(o_dec, o_enc) if init == "closed" else R.random_state_dict(o_dec, o_enc, seed=1)
    if xscale != 1.0:                                             # let the memory decide the hidden state: reactions then differ from one another
        for name in list(sd):
            if "crossattention.output.dense.weight" in name:
                sd[name] = sd[name] * xscale
    sd = R.with_lm_bias(sd, bias=R.ranked_lm_bias(o_dec.vocab_size, SEED, K, MARGIN) if bias is None else bias)
    m = SPMMRxn(bert_config=replace(tiny_config().text, num_hidden_layers=layers))
    res = m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return sd, o_dec, o_enc, m.eval()


@pytest.fixture(scope="module")
def env24():
    """Model (a), its 24 reactions and the restatement's searches, computed once."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import spmm_oracle as O
    b = R.leaders_lm_bias(300, SEED, K, BIAS_MARGIN, SEP_MARGIN)
    top = torch.topk(b, K + 1).values
    assert float(top[K - 1] - top[K]) >= 0.5                       # the bias's k-th and (k+1)-th entries
    sd, o_dec, o_enc, m = build(O, bias=b, init="random")
    ids, mask = R.pad_reactions(SEL)
    assert mask.sum(1).tolist() == LENS * 4
    ref = [R.evaluate_beam(sd, o_dec, o_enc, ids[n], mask[n], K, max_steps=T) for n in range(24)]
    best = [tuple(r[0][1]) for r in ref]                           # (every reaction finishes something: r[0] exists)
    assert len(set(best)) >= 8, "the restatement's best hypotheses must depend on the reactants"
    return dict(sd=sd, o_dec=o_dec, o_enc=o_enc, m=m, ids=ids, mask=mask, ref=ref)


@pytest.fixture(scope="module")
def envk():
    """Model (b), 24 reactions, and the restatement's searches under both stopping rules (need = k*k and need = k), computed once."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import spmm_oracle as O
    sd, o_dec, o_enc, m = build(O)
    ids, mask = reactions(24)
    ref = [R.evaluate_beam(sd, o_dec, o_enc, ids[n], mask[n], K, max_steps=T) for n in range(24)]
    ref_k = [R.evaluate_beam(sd, o_dec, o_enc, ids[n], mask[n], K, max_steps=T, need=K) for n in range(24)]
    return dict(sd=sd, o_dec=o_dec, o_enc=o_enc, m=m, ids=ids, mask=mask, ref=ref, ref_k=ref_k)


@pytest.mark.parametrize("layers,init", [(2, "closed"), (3, "closed"), (2, "random"), (3, "random")])
def test_one_decode_position_matches_the_whole_prefix_restatement(layers, init):
    """RxnDecoder.step (K/V cache, masked-memory cross-attention, one token per beam) against the CPU restatement's whole-prefix logits,
    teacher-forced over 8 positions with random beam reorders; 3 decoder layers = 2 fusion layers reading the memory; on the closed-form and
    on the full-rank weights (where reading another source's memory moves the log-probabilities far beyond the bound).  Both deviations from
    the restatement are printed: the cached path's and the facade loop's (whole prefix on the HIP model)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import spmm_oracle as O
    from spmm_amd import decode
    sd, o_dec, o_enc, m = build(O, layers=layers, init=init, bias=None if init == "closed" else R.leaders_lm_bias(300, SEED, K, BIAS_MARGIN, SEP_MARGIN))
    N, k, steps = len(LENS), 3, 8
    ids, mask = reactions(N, seed=8)
    dec = decode.RxnDecoder(m, ids, mask, k, steps + 3)
    cut = [R._cut(ids[n], mask[n]) for n in range(N)]
    emb_o = [R.encode(sd, o_enc, i, mk) for i, mk in cut]
    emb_h = m.text_encoder2.bert(ids.cuda(), attention_mask=mask.cuda(), return_dict=True, mode="text").last_hidden_state
    for n in range(N):                                            # the encoder itself (valid rows)
        assert (emb_h[n, :LENS[n]].cpu() - emb_o[n][0]).abs().max().item() < 6e-2
    g = torch.Generator().manual_seed(2)
    hist = torch.full((N * k, 1), R.CLS_ID, dtype=torch.long)
    worst_c = worst_f = 0.0
    for t in range(steps):
        lc = torch.log_softmax(dec.step(hist[:, t].cuda(), t).float(), -1).cpu()
        lo = torch.cat([torch.log_softmax(R.decoder_logits(sd, o_dec, emb_o[n], cut[n][1], hist[n * k:(n + 1) * k])[:, -1].float(), -1) for n in range(N)])
        lf = m.text_encoder(hist.cuda(), attention_mask=torch.ones_like(hist).cuda(), encoder_hidden_states=emb_h.repeat_interleave(k, 0),
                            encoder_attention_mask=mask.repeat_interleave(k, 0).cuda(), return_dict=True, is_decoder=True, return_logits=True)[:, -1]
        lf = torch.log_softmax(lf.float(), -1).cpu()
        worst_c, worst_f = max(worst_c, (lc - lo).abs().max().item()), max(worst_f, (lf - lo).abs().max().item())
        parent = torch.randint(0, k, (N, k), generator=g)
        dec.reorder(parent.cuda(), t + 1)
        hist = hist.view(N, k, -1).gather(1, parent[:, :, None].expand(N, k, t + 1)).reshape(N * k, t + 1)
        hist = torch.cat([hist, torch.randint(4, 300, (N * k, 1), generator=g)], dim=1)
    print(f"{layers} decoder layers, {init} weights: max |log-prob - restatement| cached step {worst_c:.4f}, facade loop {worst_f:.4f}")
    assert worst_c < TOL_BY_CASE.get((layers, init), TOL)


def test_free_running_search_against_the_restatement(env24):
    """N = 24, k = 3, 14 positions: every hypothesis is well formed and, re-scored teacher-forced by the CPU restatement, agrees within 3e-2
    per token; the best hypothesis is token for token the sequential restatement's for at least 90 % of the reactions.  Model (a): the
    restatement's 24 best hypotheses are at least 8 different sequences (asserted in the fixture)."""
    from spmm_amd import decode
    e = env24
    assert all(len(r) >= 1 for r in e["ref"])                      # the restatement itself finishes something for every reaction
    got = decode.predict_products(e["m"], e["ids"], e["mask"], k=K, max_steps=T)
    assert len(got) == 24
    same, worst, n_hyp = 0, 0.0, 0
    for n in range(24):
        ps = [p for p, _ in got[n]]
        assert ps == sorted(ps, reverse=True) and 1 <= len(got[n]) <= K
        for p, seq in got[n]:
            assert seq[0] == R.CLS_ID and seq[-1] == R.SEP_ID and R.SEP_ID not in seq[2:-1] and len(seq) <= T + 3
            lp = R.score(e["sd"], e["o_dec"], e["o_enc"], e["ids"][n], e["mask"][n], seq).sum().item()
            worst = max(worst, abs(p - lp) / (len(seq) - 1))
            n_hyp += 1
        same += int(got[n][0][1] == e["ref"][n][0][1])
    print(f"rxn search vs restatement: {n_hyp} hypotheses, worst |score - teacher-forced score| per token {worst:.4f}; best identical for {same} / 24 "
          f"({len(set(tuple(r[0][1]) for r in e['ref']))} distinct sequences, lengths {sorted(set(len(r[0][1]) for r in e['ref']))})")
    assert worst < 3e-2
    assert same >= 0.9 * 24


def test_the_search_needs_k_squared_finals(envk):
    """Every reaction holds k finals after the first bookkeeping position (each beam offers [SEP]); `evaluate_beam` keeps searching until k*k.
    The restatement's two rules return different sets (asserted on the CPU first), and the engine returns the k*k rule's."""
    from spmm_amd import decode
    e = envk
    ref, ref_k = e["ref"], e["ref_k"]
    assert all(len(r) == K for r in ref_k) and all(max(len(s) for _, s in r) <= 5 for r in ref_k)        # k finals within three positions
    differ = [n for n in range(24) if [s for _, s in ref[n]] != [s for _, s in ref_k[n]]]
    assert differ, "the two stopping rules agree on this state dict: the test would show nothing"
    got = decode.predict_products(e["m"], e["ids"], e["mask"], k=K, max_steps=T)
    ok = sum(int([s for _, s in got[n]] == [s for _, s in ref[n]]) for n in range(24))
    ok_d = sum(int([s for _, s in got[n]] == [s for _, s in ref[n]]) for n in differ)
    print(f"k*k finals: engine's set equals the restatement's for {ok} / 24 reactions ({ok_d} / {len(differ)} of those where need = k differs)")
    assert ok == 24
    assert decode.last_run["positions"] < T                       # and it stopped at the finals, not at the position limit


def test_compaction_returns_the_same_hypotheses():
    """Finished reactions leave the decoded batch (only kv_seq, the ancestry rows and the row map are gathered; memory and caches stay): same
    hypotheses; the scores are compared within 1e-4, not bit for bit: the GEMMs of a smaller batch may take another tile kernel, whose
    accumulation order differs (the bound of test_batched_decode_drops_finished_molecules; the largest difference is printed).  State dict: the memory decides the hidden state (cross-attention output x 100) and [SEP] ties the k-th
    bias entry, so the reactions finish at different positions (3..6 on the CPU restatement)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import spmm_oracle as O
    from spmm_amd import decode
    sd, o_dec, o_enc, m = build(O, bias=R.ranked_lm_bias(300, SEED, K, 0.0), xscale=100.0)
    ids, mask = reactions(24)
    whole = decode.predict_products(m, ids, mask, k=K, max_steps=T, compact=False, sync_every=1)
    assert decode.last_run["compactions"] == 0
    small = decode.predict_products(m, ids, mask, k=K, max_steps=T, compact=True, sync_every=1)
    run = dict(decode.last_run)
    print(f"rxn decode with compaction: {run}")
    assert run["compactions"] >= 1 and run["final_batch"] < 24
    assert [[h[1] for h in r] for r in small] == [[h[1] for h in r] for r in whole]
    worst = max(abs(pa - pb) for a, b in zip(small, whole) for (pa, _), (pb, _) in zip(a, b))
    print(f"rxn decode with compaction: largest |score difference| {worst:.3e}")
    assert worst < 1e-4


def test_batch_independence(env24):
    """A reaction decoded alone and inside the batch of 24 gives the same best hypothesis: nothing leaks between sources of different lengths
    sharing a launch, for 1, 2, 3 and 8 beams.  Model (a): on the CPU first, the restatement finishes a hypothesis for every tested reaction
    and beam count within the 6 positions, and its best hypotheses differ between the tested reactions -- a decoder that read another
    reaction's memory, or another reaction's length, would not return them."""
    from spmm_amd import decode
    e = env24
    tested = [0, 1, 8, 15, 4, 23]                                  # lengths 1, 3, 7, 16, 17, 24
    assert [int(e["mask"][n].sum()) for n in tested] == LENS
    for k in (1, 2, 3, 8):
        if k == 1:
            cpu = [R.evaluate_oracle(e["sd"], e["o_dec"], e["o_enc"], e["ids"][n], e["mask"][n], max_steps=6) for n in tested]
        else:
            cpu = [R.evaluate_beam(e["sd"], e["o_dec"], e["o_enc"], e["ids"][n], e["mask"][n], k, max_steps=6) for n in tested]
            assert all(len(r) >= 1 for r in cpu), k
            cpu = [r[0][1] for r in cpu]
        assert len(set(map(tuple, cpu))) >= (3 if k >= 3 else 2), (k, cpu)
        batch = decode.predict_products(e["m"], e["ids"], e["mask"], k=k, max_steps=6) if k != 1 else \
            [[(0.0, s)] for s in decode.greedy_products(e["m"], e["ids"], e["mask"], max_steps=6)]
        worst = 0.0
        for n in tested:
            one_ids, one_mask = R._cut(e["ids"][n], e["mask"][n])
            alone = decode.predict_products(e["m"], one_ids, one_mask, k=k, max_steps=6) if k != 1 else \
                [[(0.0, s)] for s in decode.greedy_products(e["m"], one_ids, one_mask, max_steps=6)]
            assert alone[0] and batch[n], (k, n)
            assert alone[0][0][1] == batch[n][0][1], (k, n)
            worst = max(worst, abs(alone[0][0][0] - batch[n][0][0]))
        same = sum(int(batch[n][0][1] == c) for n, c in zip(tested, cpu))
        print(f"batch independence k={k}: alone == in batch for all {len(tested)}; largest |score difference| {worst:.3e}; {same} / {len(tested)} equal to the restatement; "
              f"{len(set(map(tuple, cpu)))} distinct")


def test_greedy_search():
    """greedy_products equals `evaluate` run on the HIP model's own facade loop token for token, and the CPU restatement's for >= 90 % of the
    rows.  Full-rank weights with [SEP] 0.4 above the third bias entry; 12 reactions (GSEL) for which every argmax of the restatement leads
    its runner-up by >= 0.04 and whose rows differ: asserted on the CPU first."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import spmm_oracle as O
    from spmm_amd import decode
    sd, o_dec, o_enc, m = build(O, bias=R.ranked_lm_bias(300, SEED, K, 0.4, scale=0.3), init="random")
    ids, mask = R.pad_reactions(GSEL)
    cpu = [R.evaluate_oracle(sd, o_dec, o_enc, ids[n], mask[n], max_steps=12) for n in range(12)]
    assert len(set(map(tuple, cpu))) >= 6 and len(set(len(r) for r in cpu)) >= 3, cpu
    got = decode.greedy_products(m, ids, mask, max_steps=12)
    loop = [R.evaluate_module(m, ids[n].cuda(), mask[n].cuda(), max_steps=12) for n in range(12)]
    same = sum(int(a == b) for a, b in zip(got, cpu))
    print(f"greedy: {sum(int(a == b) for a, b in zip(got, loop))} / 12 rows identical to the facade loop, {same} / 12 to the CPU restatement; "
          f"{len(set(map(tuple, cpu)))} distinct rows, lengths {sorted(set(len(r) for r in got))}")
    assert got == loop
    assert same >= 0.9 * 12
    assert all(r[0] == R.CLS_ID and (r[-1] == R.SEP_ID or len(r) == 13) and R.SEP_ID not in r[1:-1] for r in got)
    assert decode.greedy_products(m, ids, mask, max_steps=12, cached=False) == got       # the batched facade loop


@pytest.mark.parametrize("n_beam", [3, 1])
def test_driver_end_to_end(tmp_path, n_beam):
    """rxn_predict.py --synthetic --tiny in a fresh process: exit 0, a CSV with one line per input in input order."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, ROOT)
    import rxn_predict as D
    from pv2smiles import synthetic_vocab
    out = tmp_path / "c.csv"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "rxn_predict.py"), "--synthetic", "--tiny", "--n_beam", str(n_beam), "--max_steps", "20",
                        "--output", str(out)], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = list(csv.reader(open(out)))
    sources, _ = D.synthetic_reactions(synthetic_vocab(300), 8, 0)
    assert rows[0] == ["source"] + [f"candidate_{i + 1}" for i in range(n_beam)]
    assert [row[0] for row in rows[1:]] == sources and all(len(row) == n_beam + 1 for row in rows[1:])
    assert "Accuracy (top-1):" in r.stdout
