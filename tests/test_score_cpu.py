"""Host logic of likelihood scoring, no GPU: the drivers' flags, the input order after length sorting, the CSV arithmetic, pair-list and mask
validation, and `score_smiles(engine=False)` running on the CPU oracle's module API."""
import csv
import math

import pytest
import torch

import retrieve as RD
import score as D


# ------------------------------------------------------------------------------------------------------------------------- flags
def test_driver_flags():
    a = D.parse_args(["--synthetic", "8", "--tiny"])
    assert (a.synthetic, a.tiny, a.rxn, a.batch_size, a.output, a.device) == (8, True, False, 256, "scores.csv", "cuda")
    a = D.parse_args(["--rxn", "--library", "pairs.txt", "--checkpoint", "ck.pth", "--batch_size", "32", "--output", "o.csv"])
    assert a.rxn and a.library == "pairs.txt" and a.checkpoint == "ck.pth" and a.batch_size == 32 and D.check_args(a) is a
    a = D.parse_args(["--checkpoint", "c", "--vocab_filename", "v", "--input", "i.csv", "--property_names", "n.txt", "--normalize", "n.pkl", "--library", "l.txt"])
    assert D.check_args(a).normalize == "n.pkl"
    for argv, msg in ((["--tiny"], "give the molecules"), (["--library", "l", "--batch_size", "0"], "batch_size"),
                      (["--library", "l", "--input", "i.csv"], "--property_names"), (["--rxn", "--library", "l", "--input", "i.csv"], "--rxn scores"),
                      (["--synthetic", "-1"], "synthetic")):
        with pytest.raises(SystemExit, match=msg):
            D.check_args(D.parse_args(argv))
    with pytest.raises(SystemExit, match="no CPU / eager fallback"):
        D.main(D.parse_args(["--synthetic", "4", "--tiny", "--device", "cpu"]))


def test_retrieve_driver_takes_the_rerank_criterion():
    assert RD.parse_args(["--synthetic", "8"]).rerank_by == "match"
    assert RD.parse_args(["--synthetic", "8", "--rerank_by", "likelihood"]).rerank_by == "likelihood"
    with pytest.raises(SystemExit):
        RD.parse_args(["--rerank_by", "cosine"])
    nan = float("nan")
    idx, cos, match = torch.tensor([4, 2, -1, 7]), torch.tensor([0.9, 0.8, 0.0, 0.7]), torch.tensor([nan] * 4)
    rows = RD.ranked_rows(idx, cos, match, None, torch.tensor([-1.5, -2.0, nan, nan]))
    assert [r[0] for r in rows] == [1, 2, 3] and [r[1] for r in rows] == [5, 3, 8] and [r[5] for r in rows] == ["-1.5", "-2.0", ""]
    assert all(len(r) == 5 for r in RD.ranked_rows(idx, cos, match, None))          # the default layout is unchanged


# ------------------------------------------------------------------------------------------------------- order, CSV arithmetic
def test_scores_come_back_in_input_order():
    """Batches are cut from the length-sorted order; every sequence's score lands on its own line."""
    rows = [[2] + [5] * n + [3] for n in (7, 1, 4, 9, 1, 3, 8)]
    seen = []

    def score_batch(idx, ids, mask):
        seen.append(idx.tolist())
        assert ids.shape[1] == int(mask.sum(1).max()) and bool((mask.sum(1) == torch.tensor([len(rows[i]) for i in idx])).all())
        return -mask.sum(1).float() * 0.5, mask.sum(1) - 1
    logp, tokens = D.score_all(rows, 3, score_batch)
    assert [len(b) for b in seen] == [3, 3, 1]
    lens = [len(r) for r in rows]
    assert [lens[i] for b in seen for i in b] == sorted(lens)
    assert logp == [-0.5 * n for n in lens] and tokens == [n - 1 for n in lens]


def test_csv_arithmetic(tmp_path):
    rows = D.score_rows(["CCO", "c1ccccc1", "C"], [-6.0, -12.5, 0.0], [4, 5, 0])
    assert rows[0][:4] == (1, "CCO", "-6.0", 4) and float(rows[0][4]) == -1.5 and float(rows[0][5]) == math.exp(1.5)
    assert float(rows[1][4]) == -2.5 and float(rows[1][5]) == math.exp(2.5)
    assert rows[2][3:] == (0, "", "")                                          # no scored token: no mean, no perplexity
    path = str(tmp_path / "s.csv")
    D.write_csv(path, rows)
    with open(path, newline="") as f:
        back = list(csv.DictReader(f))
    assert list(back[0].keys()) == D.COLUMNS == ["line", "smiles", "logp", "tokens", "logp_per_token", "perplexity"]
    for r in back[:2]:
        assert float(r["perplexity"]) == math.exp(-float(r["logp"]) / int(r["tokens"]))


def test_pair_file(tmp_path):
    p = tmp_path / "pairs.txt"
    p.write_text("CC.O\tCCO\n\nc1ccccc1\tC1CCCCC1\n")
    assert D.read_pairs(str(p)) == (["CC.O", "c1ccccc1"], ["CCO", "C1CCCCC1"])
    p.write_text("CC.O\n")
    with pytest.raises(SystemExit, match="expected source<TAB>candidate"):
        D.read_pairs(str(p))


# ------------------------------------------------------------------------------------------------------------------ validation
def test_pair_list_and_mask_validation():
    from spmm_amd import score as S
    assert S.check_pairs(None, 3, 3, "t").tolist() == [[0, 0], [1, 1], [2, 2]]
    assert S.check_pairs(torch.tensor([[2, 5], [0, 0]], dtype=torch.int32), 3, 6, "t").dtype == torch.int64
    assert tuple(S.check_pairs(torch.zeros(0, 2, dtype=torch.long), 3, 6, "t").shape) == (0, 2)
    with pytest.raises(ValueError, match="row i is paired with row i"):
        S.check_pairs(None, 3, 6, "t")
    for bad in ([[3, 0]], [[0, 6]], [[-1, 0]], [[0, -1]]):
        with pytest.raises(IndexError, match="t: a pair names"):
            S.check_pairs(torch.tensor(bad), 3, 6, "t")
    assert S.host_lens(torch.tensor([[1, 1, 0], [1, 0, 0]]), "t").tolist() == [2, 1]
    for bad in ([[1, 0, 1]], [[0, 0, 0]], [[0, 1, 1]]):
        with pytest.raises(ValueError, match="non-empty prefix"):
            S.host_lens(torch.tensor(bad), "t")
    class NoEngine:
        pass
    with pytest.raises(TypeError, match="no CPU / eager fallback"):
        S.score_smiles(NoEngine(), torch.zeros(1, 53), torch.tensor([[2, 5, 3]]), torch.ones(1, 3, dtype=torch.long))


# ------------------------------------------------------------------------------------------- the yard-stick on the CPU oracle
def test_dense_route_runs_on_the_oracle_module():
    """Two pairs on oracle.spmm_oracle.OracleModule: the scores are the oracle's own log_softmax, gathered; a token under a zero mask is no
    target; a padded molecule scores what it scores alone (the decoder is causal)."""
    import spmm_oracle as O
    from spmm_amd import decode, score as S
    oc = O.tiny_cfg()
    sd = O.closed_form_state_dict(oc)
    om = O.OracleModule(sd, oc)
    pv = torch.randn(2, 53, generator=torch.Generator().manual_seed(1))
    ids = torch.tensor([[2, 17, 250, 9, 3, 0, 0], [2, 44, 3, 0, 0, 0, 0]])
    mask = (ids != 0).long()
    ids_dirty = ids.clone()
    ids_dirty[1, 4] = 99                                                        # under a zero mask
    sc = S.score_smiles(om, pv, ids_dirty, mask, torch.tensor([[1, 0], [0, 1]]), engine=False)
    assert tuple(sc.logp.shape) == (2,) and tuple(sc.token_logp.shape) == (2, 6) and sc.n_tokens.tolist() == [4, 2]
    pe = decode.encode_properties(om, pv)
    for p, (q, mol, n) in enumerate(((1, 0, 5), (0, 1, 3))):
        logits = om.text_encoder(ids[mol:mol + 1, :n], attention_mask=torch.ones(1, n, dtype=torch.long), encoder_hidden_states=pe[q:q + 1],
                                 encoder_attention_mask=torch.ones(1, 54, dtype=torch.long), is_decoder=True, return_logits=True)
        want = torch.log_softmax(logits.double(), -1)[0, :-1].gather(1, ids[mol, 1:n, None])[:, 0]
        assert (sc.token_logp[p, :n - 1].double() - want).abs().max().item() < 1e-4
        assert not sc.token_logp[p, n - 1:].any() and abs(float(sc.logp[p]) - float(want.sum())) < 1e-4
    assert torch.allclose(sc.per_token(), sc.logp / sc.n_tokens)
    empty = S.score_smiles(om, pv, ids, mask, torch.zeros(0, 2, dtype=torch.long), engine=False)
    assert tuple(empty.logp.shape) == (0,) and tuple(empty.token_logp.shape) == (0, 6)
