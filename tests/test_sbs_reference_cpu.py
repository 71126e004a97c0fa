"""The float64 restatement of stochastic beam search (tests/sbs_reference.py) on the toy model, and decode.DistinctBook.update -- the
tensor-op form of spmm_sbs_step -- against it.  The checks used here are the ones the GPU tests hold the kernel to; the last test shows
that they reject four seeded defects.
Statistics: observed frequency against exact probability, deviation <= 5 sigma, sigma = sqrt(p (1 - p) / n), n = 4 096 seeded runs at
W = 2: the first slot is a draw from p(seq), the pair a draw of two without replacement.  With the project's counter noise (seed 11) the
correct algorithm sits at 1.58 sigma (first slot) and 1.83 sigma (inclusion); leaving out the conditioning at 11.0 and 12.8, the
log-sum-exp over masked tokens too at 9.5 on inclusion."""
import numpy as np
import pytest
import torch

import sbs_reference as R

N_RUNS = 4096


def _toy_run(W, seed, G=1, defect=None, steps=R.TOY_STEPS):
    return R.search_ref(R.toy_model, R.toy_noise(seed), G, W, steps, R.TOY_L, defect=defect, raw_model=R.toy_raw)


def _stats(defect=None):
    state = _toy_run(2, 11, G=N_RUNS, defect=defect)                      # the groups of one launch are independent runs
    seqs = R.sequences(state)
    return R.toy_statistics([s[0] if s else None for s in seqs], seqs)


def test_the_toy_model_has_15_sequences_whose_probabilities_sum_to_one():
    table = R.toy_sequences()
    assert len(table) == 15 and abs(sum(table.values()) - 1.0) < 1e-12
    assert all(s[0] == R.CLS and s[-1] == R.SEP and all(v > R.SEP for v in s[1:-1]) for s in table)
    assert abs(R.inclusion_w2(list(table.values())).sum() - 2.0) < 1e-12


def test_a_search_wider_than_the_support_returns_every_sequence_once():
    state = _toy_run(16, 5)
    seqs = R.sequences(state)[0]
    assert len(seqs) == 15 and len(set(seqs)) == 15 and set(seqs) == set(R.toy_sequences())
    gum, phi = state["gum"][0], state["phi"][0]
    assert np.all(np.diff(gum[:15]) <= 0) and gum[15] == R.NEG            # slot order is key order; the 16th slot is empty
    table = R.toy_sequences()
    assert max(abs(np.exp(phi[i]) - table[s]) for i, s in enumerate(seqs)) < 1e-12


def test_the_returned_sequences_are_distinct():
    for seed in range(20):
        for W in (2, 4, 8):
            seqs = R.sequences(_toy_run(W, seed))[0]
            assert len(seqs) == W and len(set(seqs)) == W, (seed, W, seqs)


def test_four_samples_are_the_first_four_of_sixteen_for_50_seeds():
    for seed in range(50):
        a, b = _toy_run(4, seed), _toy_run(16, seed)
        assert R.sequences(a)[0] == R.sequences(b, 4)[0], seed
        assert np.array_equal(a["gum"][0], b["gum"][0, :4]) and np.array_equal(a["phi"][0], b["phi"][0, :4])


def test_first_slot_and_inclusion_frequencies_meet_the_5_sigma_bound():
    d1, d2 = _stats()
    print(f"toy model, {N_RUNS} runs at W = 2: first slot {d1:.2f} sigma, inclusion {d2:.2f} sigma")
    assert d1 <= R.SIGMA_BOUND and d2 <= R.SIGMA_BOUND


def test_the_tie_rules_hold():
    R.check_tie_order(R.step_ref)


def _book_step(fused_dtype=False):
    """DistinctBook.update behind step_ref's interface."""
    from spmm_amd import decode

    def step(logits, noise, state, t):
        G, W, V = logits.shape
        L = state["tokens"].shape[-1]
        book = decode.DistinctBook(G, W, L - 3, "cpu", fused=False)
        assert book.Lmax == L
        c = book.cur
        c["phi"], c["gum"] = torch.from_numpy(state["phi"].copy()), torch.from_numpy(state["gum"].copy())
        c["fin"], c["len"] = torch.from_numpy(np.asarray(state["fin"]).astype(np.uint8)), torch.from_numpy(np.asarray(state["len"]).astype(np.int64))
        c["tokens"] = torch.from_numpy(np.asarray(state["tokens"]).astype(np.int64))
        c["anc"] = torch.from_numpy(np.asarray(state["anc"]).astype(np.int32))
        book.t = t
        ids = book.update(torch.from_numpy(logits.reshape(G * W, V)), torch.from_numpy(noise.reshape(G * W, V)))
        n = book.cur
        out = {f: n[f].numpy() for f in ("phi", "gum", "len", "tokens", "anc")}
        out.update(fin=n["fin"].numpy().astype(bool), ids=ids.numpy(), parent=book.parent.numpy(), open=book.open.numpy())
        return out
    return step


def test_the_tensor_op_form_is_the_reference():
    """DistinctBook.update against step_ref, state by state over the toy search (W = 8, 64 groups) and on the tie case."""
    step = _book_step()
    R.check_tie_order(step)
    G, W = 64, 8
    state, t = R.start_state(G, W, R.TOY_L)
    noise = R.toy_noise(4)
    for _ in range(R.TOY_STEPS):
        lg, nz = R.toy_model(t, state["tokens"]), noise(t - 1, G, W)
        want, got = R.step_ref(lg, nz, state, t), step(lg, nz, state, t)
        for f in ("phi", "gum"):
            assert np.allclose(got[f], want[f], rtol=0, atol=1e-12, equal_nan=True), f
        for f in ("fin", "len", "tokens", "anc", "ids", "parent", "open"):
            assert np.array_equal(np.asarray(got[f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)), f
        state, t = want, t + 1
    assert all(len(s) == 8 and len(set(s)) == 8 for s in R.sequences(state))


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_the_checks_reject_seeded_defects(defect):
    """Each defect fails the check that is there for it: the statistics (keys not conditioned on the parent's; log-sum-exp over tokens
    that are masked), the tie rule (ties to the higher index), distinctness (a finished slot with two candidates)."""
    if defect in ("unconditioned", "lse_all"):
        d1, d2 = _stats(defect)
        print(f"{defect}: first slot {d1:.2f} sigma, inclusion {d2:.2f} sigma")
        assert max(d1, d2) > R.SIGMA_BOUND
    elif defect == "ties_high":
        with pytest.raises(AssertionError):
            R.check_tie_order(lambda lg, nz, st, t: R.step_ref(lg, nz, st, t, defect=defect))
    else:
        dup = 0
        for seed in range(20):
            seqs = R.sequences(_toy_run(8, seed, defect=defect))[0]
            dup += len(seqs) - len(set(seqs))
        assert dup > 0
