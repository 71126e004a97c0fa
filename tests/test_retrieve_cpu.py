"""CPU checks of the retrieval feature: the reference module of the GPU tests (tests/retrieve_reference.py) against the oracle's own forward,
the index's save / load round trip, and the driver's flag parsing and file handling.  No kernel is launched."""
import csv
import math
import os
import subprocess
import sys

import pytest
import torch

import spmm_oracle as O
import retrieve_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def forward():
    """One oracle forward of the closed-form tiny model with every random draw pinned, and its intermediates."""
    cfg = O.tiny_cfg()
    sd = O.closed_form_state_dict(cfg)
    B, Lt = 4, 16
    prop, ids, mask = O.synthetic_batch(B, Lt, seed=7)
    mpm = (torch.arange(B * 53).reshape(B, 53) % 3 == 0).float()
    neg = (torch.arange(B).roll(1), torch.arange(B).roll(2))
    aux = {}
    with torch.no_grad():
        O.spmm_forward({k: v.clone() for k, v in sd.items()}, cfg, prop, ids, mask, 0.4, mpm_mask=mpm, neg_idx=neg, aux=aux)
    return dict(cfg=cfg, sd=sd, B=B, prop=prop, ids=ids, mask=mask, mpm=mpm, neg=neg, aux=aux)


def test_reference_features_are_the_forwards(forward):
    """prop_feat / text_feat of SPMM.forward (SPMM_models.py:92, :95): the masked-property path is the MPM substitution with a given
    mask, and a molecule encoded alone at its own length equals its row of the padded batch (a padded key's probability is exactly 0)."""
    w = forward
    pf, h = R.pv_features(w["sd"], w["cfg"], w["prop"], w["mpm"])
    assert (pf - w["aux"]["prop_feat"]).abs().max().item() < 1e-6
    assert (h - w["aux"]["prop_embeds"]).abs().max().item() < 1e-5
    tf = R.smiles_features(w["sd"], w["cfg"], w["ids"], w["mask"])
    assert (tf - w["aux"]["text_feat"]).abs().max().item() < 2e-6
    assert (pf.norm(dim=1) - 1).abs().max().item() < 1e-6 and (tf.norm(dim=1) - 1).abs().max().item() < 1e-6


def test_reference_matching_probability_is_the_forwards(forward):
    """The 3 B rows of vl_output (:199-202): B positive pairs (i, i), B pairs (prop_neg[i], i), B pairs (i, text_neg[i])."""
    w = forward
    B, ar = w["B"], torch.arange(w["B"])
    pairs = torch.cat([torch.stack([ar, ar], 1), torch.stack([w["neg"][0], ar], 1), torch.stack([ar, w["neg"][1]], 1)])
    got = R.match_prob(w["sd"], w["cfg"], w["aux"]["prop_embeds"], w["ids"], w["mask"], pairs)
    want = torch.softmax(w["aux"]["vl_output"], dim=-1)[:, 1]
    assert got.shape == want.shape == (3 * B,)
    assert (got - want).abs().max().item() < 1e-5, (got, want)


def test_matching_probability_is_a_softmax_over_two_logits(forward):
    w = forward
    sd = dict(w["sd"])
    sd["itm_head.weight"] = torch.zeros_like(sd["itm_head.weight"])
    sd["itm_head.bias"] = torch.tensor([0.3, -1.1])
    got = R.match_prob(sd, w["cfg"], w["aux"]["prop_embeds"], w["ids"], w["mask"], torch.tensor([[0, 1], [2, 2]]))
    assert (got - 1.0 / (1.0 + math.exp(0.3 + 1.1))).abs().max().item() < 1e-7
    H = w["cfg"].text.hidden_size
    a, b = torch.randn(3, H), torch.randn(3, H)
    lg = R.itm_logits(w["sd"], a, b)
    assert lg.shape == (3, 2)
    assert torch.allclose(lg, torch.cat([a, b], 1) @ w["sd"]["itm_head.weight"].T + w["sd"]["itm_head.bias"], atol=1e-6)


def test_masked_properties_do_not_reach_the_features(forward):
    w = forward
    cfg, sd, pv = w["cfg"], w["sd"], w["prop"][:2]
    none, _ = R.pv_features(sd, cfg, pv)
    zeros, _ = R.pv_features(sd, cfg, pv, torch.zeros(53))
    assert torch.equal(none, zeros)
    m = torch.zeros(53)
    m[5:25] = 1
    pv2 = pv.clone()
    pv2[:, 5:25] += 3.0                                   # values under the mask are never read
    a, ha = R.pv_features(sd, cfg, pv, m)
    b, hb = R.pv_features(sd, cfg, pv2, m)
    assert torch.equal(a, b) and torch.equal(ha, hb)
    assert (a - none).abs().max().item() > 1e-6           # and the mask token is not the value's embedding
    allm, _ = R.pv_features(sd, cfg, pv, torch.ones(2, 53))
    assert torch.equal(allm[0], allm[1])


def test_dense_path_on_the_oracle_module_and_the_error_without_an_engine(forward):
    """match_scores(engine=False) is written against the module API: on the oracle's module view it must give the reference's numbers
    (padded batch against one pair at a time).  engine=True on a module without an engine is refused in words."""
    from spmm_amd import retrieve
    ids, mask, pv, pm, pairs = R.path_case()
    cfg = O.tiny_cfg()
    sd = O.closed_form_state_dict(cfg)
    om = R.RetrieveModule(sd, cfg)
    _, h = R.pv_features(sd, cfg, pv, pm)
    want = R.match_prob(sd, cfg, h, ids, mask, pairs)
    got = retrieve.match_scores(om, h, ids, mask, pairs, engine=False)
    assert (got - want).abs().max().item() < 1e-5
    assert (want.max() - want.min()).item() > 1e-3        # the seven probabilities differ: the comparison of the GPU tests is not vacuous
    with pytest.raises(TypeError, match="needs a model with an engine"):
        retrieve.match_scores(om, h, ids, mask, pairs)
    with pytest.raises(TypeError, match="needs a model with an engine"):
        retrieve.smiles_features(om, ids, mask)
    with pytest.raises(IndexError):
        retrieve.match_scores(om, h, ids, mask, torch.tensor([[0, 5]]), engine=False)


def test_index_save_load_round_trip(tmp_path):
    from spmm_amd.retrieve import MoleculeIndex, length_sorted_batches, pad_rows
    g = torch.Generator().manual_seed(2)
    feats = torch.nn.functional.normalize(torch.randn(7, 64, generator=g), dim=1)
    ids, mask = pad_rows([[2, 5, 3], [2, 3], [2, 9, 8, 7, 3], [2, 4, 3], [2, 6, 6, 3], [2, 3], [2, 8, 3]])
    idx = MoleculeIndex(feats, ids, mask, ["a", "b", "c", "d", "e", "f", "g"])
    path = str(tmp_path / "lib.idx")
    idx.save(path)
    back = MoleculeIndex.load(path, device="cpu")
    assert len(back) == 7 and torch.equal(back.feats, feats) and torch.equal(back.ids, ids) and torch.equal(back.mask, mask)
    assert back.smiles == idx.smiles and back.feats.dtype == torch.float32
    torch.save({"feats": feats}, path)
    with pytest.raises(ValueError, match="not a saved MoleculeIndex"):
        MoleculeIndex.load(path, device="cpu")
    # batches in order of token length, every molecule exactly once
    batches = length_sorted_batches(mask.sum(1).numpy(), 3)
    assert sorted(i for b in batches for i in b.tolist()) == list(range(7)) and [len(b) for b in batches] == [3, 3, 1]
    assert batches[0].tolist() == [1, 5, 0] and batches[2].tolist() == [2]


def test_driver_flags_and_csv(tmp_path):
    import retrieve as drv
    a = drv.parse_args([])
    assert (a.top_k, a.rerank, a.batch_size, a.device, a.synthetic, a.tiny) == (100, 16, 256, "cuda", 0, False)
    assert a.checkpoint == "./Pretrain/checkpoint_SPMM.ckpt" and a.vocab_filename == "./vocab_bpe_300.txt" and a.output == "retrieved_molecules.csv"
    a = drv.parse_args(["--synthetic", "64", "--tiny", "--top_k", "5", "--rerank", "3", "--output", "x.csv", "--index", "i", "--save_index", "s",
                        "--query_smiles", "CCO", "--library", "l", "--input", "q.csv", "--property_names", "n.txt", "--normalize", "m.pkl"])
    assert (a.synthetic, a.tiny, a.top_k, a.rerank, a.output, a.index, a.save_index, a.query_smiles, a.library) == (64, True, 5, 3, "x.csv", "i", "s", "CCO", "l")
    for bad, msg in ((["--top_k", "0", "--library", "l"], "--top_k"), ([], "give the library"), (["--library", "l", "--index", "i"], "alternatives"),
                     (["--library", "l", "--input", "q.csv"], "--property_names"), (["--library", "l", "--rerank", "-1"], "--rerank"),
                     (["--library", "l", "--query_smiles", "C", "--input", "q", "--property_names", "n"], "alternatives")):
        with pytest.raises(SystemExit, match=msg):
            drv.check_args(drv.parse_args(bad))
    # the query CSV is read as pv2smiles.py reads it: absent properties are masked
    names = tmp_path / "names.txt"
    names.write_text("MolWt\nLogP\nTPSA\n")
    q = tmp_path / "q.csv"
    q.write_text("property,input_value\nLogP,2.5\n")
    val, msk = drv.read_condition(str(q), str(names))
    assert val.tolist() == [0.0, 2.5, 0.0] and msk.tolist() == [1.0, 0.0, 1.0]
    lib = tmp_path / "lib.txt"
    lib.write_text("CCO\n\nc1ccccc1\n")
    assert drv.read_smiles(str(lib)) == ["CCO", "c1ccccc1"]
    # rows: empty slots dropped, ranks consecutive, 1-based library lines, no probability beyond the re-ranked head
    rows = drv.ranked_rows(torch.tensor([1, 0, -1]), torch.tensor([0.9, 0.8, float("-inf")]), torch.tensor([0.7, float("nan"), float("nan")]),
                           ["CCO", "c1ccccc1"])
    assert [r[:3] for r in rows] == [(1, 2, "c1ccccc1"), (2, 1, "CCO")] and rows[0][4] != "" and rows[1][4] == ""
    out = tmp_path / "out.csv"
    drv.write_csv(str(out), rows)
    back = list(csv.reader(open(out)))
    assert back[0] == ["rank", "library_line", "smiles", "cosine", "match_probability"] and len(back) == 3 and back[1][:3] == ["1", "2", "c1ccccc1"]


def test_driver_refuses_a_cpu_device(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "retrieve.py"), "--synthetic", "8", "--tiny", "--device", "cpu"], capture_output=True,
                       text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode != 0 and "no CPU / eager fallback" in r.stderr
