"""The SMILES grammar of the syntax-constrained search where there is no GPU: the character automaton on hand-written strings, the
per-token table against the automaton, the invariant of the mask rule (allowed tokens always lead to [SEP] inside the budget, whatever the
logits prefer), the refusals, and the constrained search end to end on the CPU oracle's tiny model (cached=False: whole-prefix forwards,
tensor-op bookkeeping, the host mask)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import spmm_oracle as O
from prefix_reference import peaky_lm

from spmm_amd import smiles_syntax as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLS_ID, SEP_ID = 2, 3

ACCEPTED = ["C", "c1ccccc1", "CC(=O)[O-]", "C1CC(C)1", "[NH3+]CC.Cl", "CC", "C=C", "C#N", "C-C", "C(C)C", "C(=O)O", "C(C)(C)C", "C1CC1", "C=1CC=1",
            "C1=CC=CC=C1", "[Na+].[Cl-]", "[nH]", "c1cc[nH]c1", "C(C(C))C", "C12CC1C2", "C1CC1(C)", "CC(C)1CC1", "[13C]", "[N+](=O)[O-]", "Cl", "C.C",
            "C(#N)C", "C(-C)C", "C0CC0", "C11", "C(C.C)C", "[Fe+2]", "[O-]C", "C1CCCCC1C2CCCCC2", "N[C-]"]
REJECTED = ["", "C(", "C)", "C()", "C1CC", "C=", "C(=)C", "[]", "[N", "C..C", "(C)", "1CC1", "C%10", "C%", ".C", "C.", "=C", "C==C", "C=#C", "C(.C)", "C((C))",
            "C)(", "C(C", "C(C))", "C[", "C]", "[C", "[C(]", "[C.]", "[C=]", "[[C]]", "[C]]", "C=(C)", "C(1)", "C.1", "(", ")", "1", "C(=1)", "C@H", "C/C",
            "C*", "C:C", "C C", "[C@H]", "C(=", "C1(", "C#", "C-", "[+", "C=)"]


def published_vocab():
    return [str(x) for x in np.load(os.path.join(GOLDEN, "tokenizer_vocab300.npz"))["vocab"]]


def synthetic_vocab():
    sys.path.insert(0, ROOT)
    import pv2smiles
    return pv2smiles.synthetic_vocab(300)


VOCABS = {"published": published_vocab, "synthetic": synthetic_vocab}


@pytest.fixture(scope="module", params=list(VOCABS))
def table(request):
    return SS.SyntaxTable.from_vocab(VOCABS[request.param]())


def test_well_formed_on_hand_written_strings():
    assert len(ACCEPTED) >= 25 and len(REJECTED) >= 25
    assert [s for s in ACCEPTED if not SS.well_formed(s)] == []
    assert [s for s in REJECTED if SS.well_formed(s)] == []


@pytest.mark.parametrize("text,state", [
    ("", (SS.START, 0, 0)), ("C", (SS.ATOM, 0, 0)), ("C1", (SS.RING, 0, 2)), ("C(", (SS.OPEN, 1, 0)), ("C(C)", (SS.CLOSE, 0, 0)),
    ("C=", (SS.BOND_A, 0, 0)), ("C(=", (SS.BOND_B, 1, 0)), ("C.", (SS.DOT, 0, 0)), ("C[", (SS.BRK0, 0, 0)), ("C[N", (SS.BRK, 0, 0)),
    ("C[N1", (SS.BRK, 0, 0)), ("C[N-", (SS.BRK, 0, 0)), ("C=1", (SS.RING, 0, 2)), ("C1C2C(C(", (SS.OPEN, 2, 6)), ("C19", (SS.RING, 0, 0b1000000010)),
])
def test_states_and_costs(text, state):
    assert SS.run(text) == state
    q, depth, rings = state
    assert SS.cost(state) == depth + bin(rings).count("1") + {SS.START: 1, SS.OPEN: 1, SS.BOND_A: 1, SS.BOND_B: 1, SS.DOT: 1, SS.BRK0: 2, SS.BRK: 1}.get(q, 0)


def test_the_table_fold_equals_the_character_automaton(table):
    """2 000 seeded random piece sequences of 1 .. 40 pieces: the fold over the table and the automaton over the characters give the same
    (q, depth, rings), or both reject.  Half of the sequences are steered (each piece drawn among those the table accepts next) so that
    long accepted histories occur; the others are uniform and mostly reject early."""
    rng = random.Random(5)
    V, agree_live = table.V, 0
    for i in range(2000):
        n, ids, state = rng.randint(1, 40), [], SS.INITIAL
        for _ in range(n):
            if i % 2 == 0 and state[0] != SS.REJECT:
                ok = [v for v in range(4, V) if table.step_token(state, v)[0] != SS.REJECT]
                v = rng.choice(ok) if ok and rng.random() < 0.97 else rng.randrange(V)
            else:
                v = rng.randrange(V)
            ids.append(v)
            state = table.step_token(state, v)
        a, b = table.fold(ids), table.state_of(ids)
        assert (a == b) if a[0] != SS.REJECT and b[0] != SS.REJECT else (a[0] == b[0] == SS.REJECT), (ids, a, b)
        assert a == state
        agree_live += a[0] != SS.REJECT
    assert agree_live >= 500, agree_live            # not vacuous: many long histories that do not reject


def test_the_packed_table_holds_the_table(table):
    p = table.packed.view(np.uint32).astype(np.int64)
    assert table.packed.dtype == np.int32 and table.packed.shape == (table.V, 4) and table.packed.flags["C_CONTIGUOUS"]
    for s in range(10):
        w, sh = (p[:, 0], 4 * s) if s < 8 else (p[:, 1], 4 * (s - 8))
        assert ((w >> sh) & 15).tolist() == table.end[:, s].tolist()
    for c in (0, 1):
        w = p[:, 2 + c]
        assert (w & 1023).tolist() == table.toggle[:, c].tolist() and ((w >> 10) & 255).tolist() == table.need[:, c].tolist()
        assert (((w >> 18) & 255) - 128).tolist() == table.delta[:, c].tolist()
    assert (table.end[[0, 1, 2]] == SS.REJECT).all()
    assert table.end[SEP_ID].tolist() == [SS.REJECT, SS.ACCEPT, SS.ACCEPT, SS.REJECT, SS.ACCEPT] + [SS.REJECT] * 5


def _preference(table, kind, rng):
    """Fixed adversarial logits: a vector that always prefers pieces that open something."""
    V = table.V
    x = np.zeros(V)
    if kind == "uniform":
        return rng.standard_normal(V)
    for v, text in enumerate(table.text):
        if not text:
            continue
        if kind == "paren":
            x[v] = 10.0 * text.count("(") - 5.0 * text.count(")")
        elif kind == "bracket":
            x[v] = 10.0 * text.count("[") - 5.0 * text.count("]")
        elif kind == "ring":
            x[v] = 10.0 * bin(int(table.toggle[v, 0])).count("1")
    x[SEP_ID] = -20.0
    return x + 1e-3 * rng.standard_normal(V)


@pytest.mark.parametrize("kind", ["paren", "bracket", "ring", "uniform"])
@pytest.mark.parametrize("max_steps", [1, 2, 3, 5, 40])
def test_a_greedy_walk_under_the_mask_always_ends_well_formed(table, kind, max_steps):
    """The invariant: whatever the logits prefer, following the most preferred ALLOWED token reaches [SEP] at or before t_last with a
    well-formed string, and the allowed set is never empty on the way."""
    rng = np.random.default_rng(3)
    for trial in range(3):
        x = _preference(table, kind, rng)
        hist, t_last = [CLS_ID], 1 + max_steps
        while True:
            t = len(hist)
            assert t <= t_last, (kind, max_steps, hist)
            ok = SS.allowed(table, hist, t_last)
            assert ok.any(), (kind, max_steps, hist)
            state = table.state_of(hist[1:])
            assert SS.cost(state) <= t_last - t
            v = int(np.argmax(np.where(ok, x, -np.inf)))
            hist.append(v)
            if v == SEP_ID:
                break
        assert SS.well_formed(table.decode(hist[1:-1])), table.decode(hist[1:-1])
        if kind != "uniform" and max_steps == 40:
            assert len(hist) >= 20, hist              # the adversary did push the walk towards the end of the budget


def test_allowed_of_a_rejecting_history_is_empty(table):
    close = table.pieces.index("##)")
    assert not SS.allowed(table, [CLS_ID, close], 20).any()
    assert not SS.allowed(table, [CLS_ID, table.pieces.index("##C"), SEP_ID], 20).any()


def test_vocabularies_that_cannot_pay_the_cost_are_refused():
    base = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "##C", "##(", "##)", "##1", "##C1", "##[", "##]", "##[N"]
    SS.SyntaxTable.from_vocab(base)
    with pytest.raises(ValueError, match=r"lacks the single piece '\)'"):
        SS.SyntaxTable.from_vocab([p for p in base if p != "##)"])
    with pytest.raises(ValueError, match=r"ring bond 1 open but the vocabulary lacks the single piece '1'"):
        SS.SyntaxTable.from_vocab([p for p in base if p != "##1"])
    with pytest.raises(ValueError, match=r"lacks the single piece '\]'"):
        SS.SyntaxTable.from_vocab([p for p in base if p != "##]"])
    with pytest.raises(ValueError, match="no one-letter piece"):
        SS.SyntaxTable.from_vocab([p for p in base if p != "##C"])
    with pytest.raises(ValueError, match=r"lacks \[SEP\]"):
        SS.SyntaxTable.from_vocab(base[:3] + base[4:])


# ------------------------------------------------------------------------------------------------------------------ end to end
N, K, STEPS = 4, 3, 10


@pytest.fixture(scope="module")
def om():
    from spmm_amd.tokenizer import SmilesWordPiece
    m = O.OracleModule(peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), seed=7, sep_gap=0.8), O.tiny_cfg())
    m.tokenizer = SmilesWordPiece(published_vocab())
    return m


@pytest.fixture(scope="module")
def props():
    return torch.randn(N, 53, generator=torch.Generator().manual_seed(12)) * 2


def _ids(om, fragment):
    return [CLS_ID] + [om.tokenizer.vocab["##" + p] for p in fragment]


def test_prefixes_that_reject_or_cannot_close_are_refused(om, props):
    from spmm_amd import decode
    with pytest.raises(ValueError, match="not the beginning of a well-formed SMILES"):
        decode.beam_search_batched(om, props, k=K, max_steps=STEPS, cached=False, prefix=_ids(om, ["C", ")"]), syntax=True)
    open_ring_and_branch = _ids(om, ["C1", "CC", "("])                    # cost 3: ring 1, depth 1, an atom after '('
    with pytest.raises(ValueError, match="needs 3 more tokens to close; max_steps=2"):
        decode.beam_search_batched(om, props, k=K, max_steps=2, cached=False, prefix=open_ring_and_branch, syntax=True)
    with pytest.raises(ValueError, match="needs 3 more tokens to close; max_steps=2"):
        decode.generate_with_property(om, props[0], 2, max_steps=2, prefix=open_ring_and_branch, syntax=True)
    with pytest.raises(ValueError, match="needs 1 more tokens to close; max_steps=0"):
        decode.beam_search_batched(om, props, k=K, max_steps=0, cached=False, syntax=True)
    got = decode.beam_search_batched(om, props, k=K, max_steps=3, cached=False, prefix=open_ring_and_branch, syntax=True)
    assert any(got) and all(SS.well_formed(om.tokenizer.decode(s)) and s[:4] == open_ring_and_branch for h in got for _, s in h)


def test_a_model_without_a_tokenizer_is_refused(props):
    from spmm_amd import decode
    bare = O.OracleModule(O.closed_form_state_dict(O.tiny_cfg()), O.tiny_cfg())
    with pytest.raises(ValueError, match="model.tokenizer and this model has none"):
        decode.beam_search_batched(bare, props, k=K, max_steps=STEPS, cached=False, syntax=True)
    table = SS.SyntaxTable.from_vocab(published_vocab())
    assert any(decode.beam_search_batched(bare, props, k=K, max_steps=STEPS, cached=False, syntax=table))     # a table is accepted as it is


@pytest.mark.parametrize("mode", ["deterministic-k3", "multinomial-k2", "seeded-k2", "guided-k2"])
def test_constrained_search_on_the_oracle_returns_well_formed_strings_only(om, props, mode):
    from spmm_amd import decode
    kw = {"deterministic-k3": dict(k=3), "multinomial-k2": dict(k=2, stochastic=True, generator=torch.Generator().manual_seed(3)),
          "seeded-k2": dict(k=2, stochastic=True, seed=11),
          "guided-k2": dict(k=2, stochastic=True, seed=11, guidance=1.5, temperature=1.3, top_k=20, top_p=0.9)}[mode]
    got = decode.beam_search_batched(om, props, max_steps=STEPS, cached=False, syntax=True, **kw)
    run = dict(decode.last_run)
    assert run["syntax"] is True and run["dropped_masked"] >= 0
    hyps = [h for mol in got for h in mol]
    assert len(hyps) >= 1
    for score, ids in hyps:
        assert ids[0] == CLS_ID and ids[-1] == SEP_ID and SEP_ID not in ids[1:-1] and len(ids) <= 1 + STEPS + 1
        assert SS.well_formed(om.tokenizer.decode(ids)), om.tokenizer.decode(ids)
        assert score > -1e29 and np.isfinite(score)


def test_syntax_false_is_the_call_without_the_argument(om, props):
    from spmm_amd import decode
    for kw in (dict(k=3), dict(k=2, stochastic=True, seed=5)):
        plain = decode.beam_search_batched(om, props, max_steps=STEPS, cached=False, **kw)
        run = dict(decode.last_run)
        for off in (None, False):
            assert decode.beam_search_batched(om, props, max_steps=STEPS, cached=False, syntax=off, **kw) == plain
            assert dict(decode.last_run) == run and run["syntax"] is False
    a = decode.generate_with_property(om, props[0], 3, k=2, seed=4, max_steps=STEPS)
    gen = dict(decode.last_generate)
    assert decode.generate_with_property(om, props[0], 3, k=2, seed=4, max_steps=STEPS, syntax=False) == a and dict(decode.last_generate) == gen
    assert gen["syntax"] is False and gen["dropped_masked"] == 0


def test_generate_with_property_constrained(om, props):
    from spmm_amd import decode
    out = decode.generate_with_property(om, props[1], 6, k=2, seed=4, max_steps=STEPS, syntax=True)
    assert decode.last_generate["syntax"] is True
    done = [s for s in out if s]
    assert done and all(SS.well_formed(om.tokenizer.decode(s)) for s in done)


def test_driver_flag_and_report(capsys):
    sys.path.insert(0, ROOT)
    import pv2smiles
    assert pv2smiles.parse_args(["--synthetic"]).syntax is False and pv2smiles.parse_args(["--synthetic", "--syntax"]).syntax is True
    pv2smiles.report([[2, 5, 3], [2, 6, 3], []], ["CC", "C(", ""], None, None, None, None)
    assert "well-formed: 1 / 2" in capsys.readouterr().out
