"""spmm_smiles_mask (csrc/syntax.hip) against its host reference smiles_syntax.allowed.  Equality is exact: a mask is a decision -- masked
entries are the sentinel -1e30, every other entry keeps its bits, the pad columns [V, ld) (NaN-poisoned here) are never touched, and
state_out is the (q, depth, rings, cost) of the character automaton."""
import os
import random

import numpy as np
import pytest
import torch

from spmm_amd import smiles_syntax as SS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS_ID, SEP_ID = 2, 3
MASKED = np.float32(-1e30)
SINGLES = list("CcNnOoSF()=#.-[]+0123456789") + ["Cl", "Br"]


def made_up_vocab(V, seed=0):
    """Specials, then single pieces, then seeded random 2 .. 4 character pieces over a SMILES alphabet (many reject from most states)."""
    rng = random.Random(seed)
    pieces = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + ["##" + s for s in SINGLES]
    alphabet = "CCCCccccNOnos()()==#.-[]+1234567890"
    seen = set(pieces)
    while len(pieces) < V:
        p = "##" + "".join(rng.choice(alphabet) for _ in range(rng.randint(2, 4)))
        if p not in seen:
            seen.add(p)
            pieces.append(p)
    return pieces[:V]


@pytest.fixture(scope="module")
def tables():
    pub = [str(x) for x in np.load(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab300.npz"))["vocab"]]
    out = {V: SS.SyntaxTable.from_vocab(made_up_vocab(V, seed=V)) for V in (5, 64, 65, 320, 321, 512)}
    out[300] = SS.SyntaxTable.from_vocab(pub)
    return out


def walk(table, n, rng, t_last=255):
    """A history [CLS] + n pieces the grammar accepts (a random walk over allowed tokens, by proposals), never [SEP]."""
    hist, state = [CLS_ID], SS.INITIAL
    live = [v for v in range(table.V) if table.text[v]]
    while len(hist) < n + 1:
        for _ in range(4000):
            v = rng.choice(live)
            nxt = table.step_token(state, v)
            if nxt[0] != SS.REJECT and SS.cost(nxt) <= t_last - len(hist) - 1:
                break
        else:
            raise AssertionError("no allowed token found")
        hist.append(v)
        state = nxt
    return hist


def launch(table, hists, t, t_last, *, k=1, mol=None, Lmax=256, pad=4, seed=0, rows=None, t_ptr=None, t_off=0, with2=True):
    """hists: the history rows (lists, padded to Lmax here).  rows: number of logits rows (default: one per history).  -> dict of host arrays."""
    from spmm_amd import ops
    R = len(hists) if rows is None else rows
    V, ld = table.V, table.V + pad
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(2, R, ld, generator=g)
    raw[:, :, V:] = float("nan")
    both = raw.cuda()
    tok = torch.zeros(len(hists), Lmax, dtype=torch.int32)
    for i, h in enumerate(hists):
        tok[i, :len(h)] = torch.tensor(h, dtype=torch.int32)
    state = torch.full((R, 4), -7, dtype=torch.int32).cuda()
    ops.smiles_mask(both[0, :, :V], tok.cuda(), torch.from_numpy(table.packed).cuda(), t=t, t_last=t_last, k=k, Lmax=Lmax,
                    mol=None if mol is None else torch.tensor(mol, dtype=torch.int32).cuda(), logits2=both[1, :, :V] if with2 else None,
                    t_ptr=None if t_ptr is None else torch.tensor([t_ptr], dtype=torch.int32).cuda(), t_off=t_off, state_out=state)
    torch.cuda.synchronize()
    return dict(raw=raw.numpy(), out=both.cpu().numpy(), state=state.cpu().numpy())


def expect_row(table, hist, t, t_last):
    ok = SS.allowed(table, hist[:t], t_last)
    st = table.state_of(hist[1:t])
    return ok, ([SS.REJECT, 0, 0, -1] if st[0] == SS.REJECT else [st[0], st[1], st[2], SS.cost(st)])


def check(table, res, row_hists, t, t_last, with2=True):
    """row_hists[i]: the history logits row i must have been masked by."""
    V = table.V
    for i, h in enumerate(row_hists):
        ok, st = expect_row(table, h, t, t_last)
        for half in ((0, 1) if with2 else (0,)):
            want = np.where(ok, res["raw"][half, i, :V], MASKED).astype(np.float32)
            assert np.array_equal(want.view(np.int32), res["out"][half, i, :V].view(np.int32)), (i, half, h[:t], t, t_last)
        assert res["state"][i].tolist() == st, (i, h[:t], res["state"][i].tolist(), st)
    assert np.isnan(res["out"][:, :, V:]).all()
    if not with2:
        assert np.array_equal(res["out"][1, :, :V].view(np.int32), res["raw"][1, :, :V].view(np.int32))


@pytest.mark.parametrize("V", [5, 64, 65, 300, 320, 321, 512])
def test_mask_equals_the_reference_over_shapes_and_positions(tables, V):
    """R in {1, 3, 4, 5, 37} (k = 1), 4 and 6 (k = 2), 8 and 16 (k = 8) x t in {1, 2, 63, 64, 65, 254}; the budgets t_last - t cycle through
    0, 1, 2 and "plenty".  Histories are random walks of the reference, cut at t."""
    table, rng = tables[V], random.Random(100 + V)
    walks = [walk(table, 254, rng) for _ in range(6)]
    n_masked = n_kept = 0
    for ci, (R, k) in enumerate([(1, 1), (3, 1), (4, 1), (5, 1), (37, 1), (4, 2), (6, 2), (8, 8), (16, 8)]):
        for ti, t in enumerate([1, 2, 63, 64, 65, 254]):
            t_last = min(255, t + (0, 1, 2, 40)[(ci + ti) % 4])
            # rows share a few walks but differ: each row's history is a walk cut at t with its last tokens re-drawn
            hists = []
            for r in range(R):
                base = walks[(r + ci) % len(walks)][:max(1, t - (r % 3))]
                hists.append(base + walk_on(table, base, t - len(base), rng, t_last))
            res = launch(table, hists, t, t_last, k=k, seed=V + R + t)
            check(table, res, hists, t, t_last)
            n_masked += int((res["out"][0, :, :V] == MASKED).sum())
            n_kept += int((res["out"][0, :, :V] != MASKED).sum())
    assert n_masked > 0 and n_kept > 0


def walk_on(table, base, n, rng, t_last):
    """n more accepted tokens after `base` (any budget: the walk itself only needs the grammar)."""
    state, out = table.state_of(base[1:]), []
    live = [v for v in range(table.V) if table.text[v]]
    while len(out) < n:
        v = rng.choice(live)
        nxt = table.step_token(state, v)
        if nxt[0] != SS.REJECT:
            out.append(v)
            state = nxt
    return out


def _ids(table, pieces):
    return [CLS_ID] + [table.pieces.index("##" + p) for p in pieces]


def test_hand_made_extremes_at_every_budget_around_the_cost(tables):
    """Depth 100, all ten rings open, inside a bracket, right after '(', a bond, '.', and the start state: t_last - t in
    {0, 1, 2, cost - 1, cost, cost + 1}."""
    table = tables[300]
    cases = {"depth100": ["C("] * 100, "ten rings": ["C"] + list("1234567890"), "bracket0": ["C", "["], "bracket": ["C", "[N"], "open": ["C", "("],
             "bond": ["C", "="], "bond in branch": ["C(", "="], "dot": ["C", "."], "start": [], "closed": ["c1ccccc1"], "deep ring": ["C1", "C(", "C2", "C("]}
    for name, pieces in cases.items():
        hist = _ids(table, pieces)
        t, c = len(hist), SS.cost(table.state_of(hist[1:]))
        if name == "depth100":
            assert (c, t) == (101, 101)
        if name == "ten rings":
            assert table.state_of(hist[1:])[2] == 1023 and c == 10
        for extra in sorted({0, 1, 2, c - 1, c, c + 1}):
            if extra < 0 or t + extra > 255:
                continue
            res = launch(table, [hist], t, t + extra, seed=extra)
            check(table, res, [hist], t, t + extra)
            kept = int((res["out"][0, 0, :300] != MASKED).sum())
            assert kept > 0 or c > extra, (name, extra, c, kept)               # the invariant: something is allowed whenever the cost fits


def test_rows_whose_history_rejects_are_masked_whole(tables):
    table = tables[300]
    bad = [_ids(table, [")"]), _ids(table, ["C", "("]) + [SEP_ID] + _ids(table, ["C"])[1:], _ids(table, ["C"]) + [999, 5], _ids(table, ["C", "C"]) + [-4],
           _ids(table, ["C", "%", "1"]), [CLS_ID, 0, 5], [CLS_ID, CLS_ID, 5], _ids(table, ["C", "(", ")"])]
    good = _ids(table, ["C", "C", "C"])
    hists = [h + [26] * (4 - len(h)) for h in bad] + [good]
    res = launch(table, hists, 4, 30)
    check(table, res, hists, 4, 30)
    assert (res["out"][:, :len(bad), :300] == MASKED).all() and (res["state"][:len(bad)] == np.array([SS.REJECT, 0, 0, -1])).all()
    assert (res["out"][0, len(bad), :300] != MASKED).any()


def test_mol_map_strided_view_device_position_and_no_second_matrix(tables):
    from spmm_amd import ops
    table, rng = tables[300], random.Random(9)
    N, k, t, t_last = 7, 2, 9, 14
    hists = [walk(table, 8, rng, t_last) for _ in range(N * k)]               # the book's [N, k, L] histories, row n * k + b
    # a compacted batch: molecules 5, 0, 3 in that order
    mol = [5, 0, 3]
    res = launch(table, hists, t, t_last, k=k, mol=mol, rows=len(mol) * k, Lmax=16)
    check(table, res, [hists[m * k + b] for m in mol for b in range(k)], t, t_last)
    # the position from device memory: *t_ptr + t_off = 6 + 3; the host t argument is ignored
    res = launch(table, hists, 1, t_last, k=k, Lmax=16, t_ptr=6, t_off=3)
    check(table, res, hists, t, t_last)
    # no second matrix: it is left alone
    res = launch(table, hists, t, t_last, k=k, Lmax=16, with2=False)
    check(table, res, hists, t, t_last, with2=False)
    # the first pick's strided view: logits [N, V], history of molecule n = beam 0's row of tokens [N, k, L]
    tok = torch.zeros(N, k, 16, dtype=torch.int32)
    for i, h in enumerate(hists):
        tok[i // k, i % k, :len(h)] = torch.tensor(h, dtype=torch.int32)
    tok = tok.cuda()
    raw = torch.randn(N, 300, generator=torch.Generator().manual_seed(4))
    out = ops.smiles_mask(raw.cuda(), tok[:, 0], torch.from_numpy(table.packed).cuda(), t=t, t_last=t_last, k=1, Lmax=16).cpu().numpy()
    for n in range(N):
        ok = SS.allowed(table, hists[n * k][:t], t_last)
        assert np.array_equal(np.where(ok, raw[n].numpy(), MASKED).astype(np.float32).view(np.int32), out[n].view(np.int32))


def test_a_row_does_not_depend_on_the_launch_it_is_in(tables):
    table, rng = tables[300], random.Random(21)
    hists = [walk(table, 30, rng, 60) for _ in range(37)]
    many = launch(table, hists, 31, 60, seed=1)
    check(table, many, hists, 31, 60)
    for i in (0, 17, 36):
        alone = launch(table, [hists[i]], 31, 60, seed=1)
        keep_many, keep_alone = many["out"][0, i, :300] != MASKED, alone["out"][0, 0, :300] != MASKED
        assert np.array_equal(keep_many, keep_alone) and many["state"][i].tolist() == alone["state"][0].tolist()
