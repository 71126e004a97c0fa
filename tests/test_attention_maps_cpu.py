"""The reference of the attention-map tests checked against the oracle and against seeded defects, and attend.py's host logic on made-up
maps -- no GPU."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import attn_map_reference as A         # noqa: E402
import spmm_oracle as O                # noqa: E402


def test_the_reference_s_probabilities_are_the_ones_the_oracle_uses():
    """pr @ V through the output projection and the LayerNorm reproduces oracle.attention's output to fp32 round-off, for a self- and a
    cross-attention block under a mask: attention_probs is the `pr` the oracle discards, not merely some softmax."""
    oc = O.tiny_cfg()
    sd = A.path_state_dict(oc)
    c = oc.text
    g = torch.Generator().manual_seed(1)
    hidden, enc = torch.randn(2, 7, c.hidden_size, generator=g), torch.randn(2, 11, c.hidden_size, generator=g)
    emask = O.inverted_enc_mask(torch.tensor([[1] * 11, [1] * 4 + [0] * 7]))
    smask = O.extended_self_mask(torch.tensor([[1] * 7, [1] * 5 + [0] * 2]), False)
    p = "text_encoder.bert.encoder.layer.1."
    with torch.no_grad():
        for blk, mask, e in ((p + "crossattention", emask, enc), (p + "attention", smask, None)):
            pr = A.attention_probs(sd, blk, c, hidden, mask, e)
            assert tuple(pr.shape) == (2, c.num_attention_heads, 7, 7 if e is None else 11)
            want = O.attention(sd, blk, c, hidden, mask, e)
            got = A.attention_from_probs(sd, blk, c, hidden, pr, e)
            assert (got - want).abs().max().item() <= 4 * 2.0 ** -23 * want.abs().max().item()
    assert bool((A.attention_probs(sd, p + "crossattention", c, hidden, emask, enc)[1, :, :, 4:] == 0).all())


def test_probs_agrees_with_the_oracle_s_softmax():
    """attn_map_reference.probs (the kernel's contract, written per sequence and head in float64) against the oracle's formula on a dense
    case under a key mask."""
    c = [x for x in A.kernel_cases() if x["name"] == "dense-3x2x54x77"][0]
    Q, K = A.case_qk(c)
    ref = A.probs(Q, K, **A.case_layout(c))
    q = Q.double().view(3, 54, 2, 64).permute(0, 2, 1, 3)
    k = K.double().view(3, 77, 2, 64).permute(0, 2, 1, 3)
    s = q @ k.transpose(-1, -2) / 8.0 + O.inverted_enc_mask(c["kmask"]).double()
    pr = torch.softmax(s, dim=-1).permute(1, 0, 2, 3).reshape(2, 3 * 54, 77)
    assert (pr - ref["heads"]).abs().max().item() < 1e-14
    assert (pr.mean(0) - ref["mean"]).abs().max().item() < 1e-14


CASES = A.kernel_cases()


@pytest.mark.parametrize("defect", A.DEFECTS)
def test_the_kernel_comparison_rejects_seeded_defects(defect):
    """Each defect moves the comparison of tests/test_attn_probs_gpu.py above 1e-4 -- the ceiling the kernel's tolerance must stay below --
    at every case where it changes the arithmetic at all (attn_map_reference.defect_applies says where it cannot, and why)."""
    assert A.KERNEL_TOL < A.TOL_CEILING
    hit = 0
    for c in CASES:
        if not A.defect_applies(c, defect):
            continue
        ref = A.probs(*A.case_qk(c), **A.case_layout(c))
        bad = A.probs(*A.case_qk(c), **A.case_layout(c), defect=defect)
        d = A.compare(bad, ref)
        assert d > A.TOL_CEILING, (defect, c["name"], d)
        hit += 1
    assert hit >= (1 if defect == "self_mask" else 2), (defect, hit)


def test_the_path_reference_is_not_vacuous():
    """The guards of tests/test_attention_maps_gpu.py on the reference alone: no near-uniform map, two molecules under one PV apart."""
    oc = O.tiny_cfg()
    oc.text.num_hidden_layers = 3
    ids, mask, pv, pm, pairs = A.path_case()
    ref = A.fusion_maps(A.path_state_dict(oc), oc, pv, pm, ids, mask, pairs)
    lens = mask.sum(1).tolist()
    for p, (qi, mi) in enumerate(pairs.tolist()):
        assert set(ref[p]) == {(0, "pv2text"), (1, "pv2text"), (0, "text2pv"), (1, "text2pv")}
        for (li, d), m in ref[p].items():
            assert tuple(m.shape) == ((2, 54, lens[mi]) if d == "pv2text" else (2, lens[mi], 54))
            assert A.contrast_share(m) >= 0.5
            assert (m.sum(-1) - 1).abs().max().item() < 1e-5
    for li in (0, 1):
        a, b = ref[1][(li, "pv2text")].mean(0), ref[2][(li, "pv2text")].mean(0)
        assert (a[:, :20] - b[:, :20]).abs().max().item() > 0.05


# ---------------------------------------------------------------------------------------------------------------- attend.py's host logic
def test_labels_and_character_spans():
    import attend
    itos = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "##C", "##Cl", "##(", "##[nH]", "##c1"]
    assert attend.token_labels(itos, [2, 4, 5, 6, 7, 8, 3]) == ["[CLS]", "C[0:1]", "Cl[1:3]", "([3:4]", "[nH][4:8]", "c1[8:10]", "[SEP]"]
    assert attend.token_labels(itos, [2, 1, 3]) == ["[CLS]", "[UNK]", "[SEP]"]
    assert attend.property_labels(["a", "b"]) == ["[CLS]", "a", "b"]
    names = attend.read_property_names("")
    assert len(names) == 53 and attend.mask_from_names("property_3, property_52", names).nonzero().flatten().tolist() == [3, 52]
    with pytest.raises(SystemExit, match="unknown property 'x'"):
        attend.mask_from_names("x", names)


def test_csv_rows_and_order():
    import attend
    m = np.array([[0.25, 0.75], [1.0, 0.0], [0.5, 0.5]], dtype=np.float32)
    rows = attend.map_rows(7, 1, "pv2text", m, ["[CLS]", "a", "b"], ["[CLS]", "C[0:1]"])
    assert len(rows) == 6 and rows[0] == (7, 1, "pv2text", "mean", 0, "[CLS]", 0, "[CLS]", "0.25")
    assert [(r[4], r[6]) for r in rows] == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)] and rows[3][5:] == ("a", 1, "C[0:1]", "0.0")
    rows = attend.map_rows(1, 0, "text2pv", np.stack([m, m[::-1]]), ["x", "y", "z"], ["p", "q"])
    assert len(rows) == 12 and [r[3] for r in rows] == ["0"] * 6 + ["1"] * 6 and rows[6][8] == "0.5"
    with pytest.raises(AssertionError):
        attend.map_rows(1, 0, "text2pv", m, ["x", "y"], ["p", "q"])
    assert attend.COLUMNS == ["line", "layer", "direction", "head", "query_index", "query_label", "key_index", "key_label", "weight"]


def test_entropy_ranking():
    import attend
    m = np.array([[1.0, 0.0, 0.0, 0.0],              # [CLS]: the most concentrated row, never reported
                  [0.25, 0.25, 0.25, 0.25],
                  [0.0, 0.9, 0.1, 0.0],
                  [0.4, 0.0, 0.0, 0.6],
                  [0.0, 0.0, 1.0, 0.0]])
    r = attend.entropy_ranking(m, ["[CLS]", "a", "b", "c", "d"], ["k0", "k1", "k2", "k3"], k=3, top=2)
    assert [x[0] for x in r] == ["d", "b", "c"]
    assert r[0][1] == 0.0 and r[0][2][0] == ("k2", 1.0) and r[1][2] == [("k1", 0.9), ("k2", 0.1)]
    assert abs(r[2][1] - (-(0.4 * np.log(0.4) + 0.6 * np.log(0.6)))) < 1e-12
    assert [x[0] for x in attend.entropy_ranking(np.stack([m, m]), ["[CLS]", "a", "b", "c", "d"], ["k0", "k1", "k2", "k3"])] == ["d", "b", "c"]


def test_input_order_is_restored():
    import attend
    lengths = [9, 2, 30, 2, 17, 5, 11]
    seen = []

    def run(idx):
        seen.append(idx.tolist())
        return [f"r{i}" for i in idx.tolist()]
    assert attend.attend_all(lengths, 3, run) == [f"r{i}" for i in range(7)]
    assert seen == [[1, 3, 5], [0, 6, 4], [2]]


def _ns(**kw):
    base = dict(batch_size=4, synthetic=0, input_file="x.txt", rxn=False, pv_csv="", property_names="", normalize="", mask_properties="",
                direction="both", layer="-1")
    base.update(kw)
    return argparse.Namespace(**base)


def test_argument_refusals(tmp_path):
    import attend
    assert attend.check_args(_ns()).layers == (-1,)
    assert attend.check_args(_ns(layer="all")).layers == "all" and attend.check_args(_ns(layer="0,-1")).layers == (0, -1)
    for kw, msg in ((dict(batch_size=0), "--batch_size"), (dict(synthetic=-1), "--synthetic"), (dict(input_file=""), "--input_file"),
                    (dict(rxn=True, pv_csv="a.csv"), "--rxn maps products"), (dict(rxn=True, direction="pv2text"), "one direction"),
                    (dict(mask_properties="a"), "needs --property_names"), (dict(layer="top"), "--layer 'top'")):
        with pytest.raises(SystemExit, match=msg):
            attend.check_args(_ns(**kw))
    p = tmp_path / "pv.csv"
    p.write_text("h," * 52 + "h\n" + ",".join(["1.5"] * 53) + "\n" + ",".join(["2"] * 53) + "\n")
    assert tuple(attend.read_pv_csv(str(p), 2).shape) == (2, 53)
    with pytest.raises(SystemExit, match="2 property vectors for 3 molecules"):
        attend.read_pv_csv(str(p), 3)
    p.write_text("1,2,3\n")
    with pytest.raises(SystemExit, match="3 values, 53 expected"):
        attend.read_pv_csv(str(p), 1)


def test_the_module_s_refusals_need_no_gpu():
    from spmm_amd import attribution as AT
    assert AT.resolve_layers((-1,), 2, "x") == (1,) and AT.resolve_layers("all", 3, "x") == (0, 1, 2) and AT.resolve_layers([1, 0, -2], 2, "x") == (0, 1)
    for bad in ((2,), (-3,), (), "last", (1.5,)):
        with pytest.raises(ValueError):
            AT.resolve_layers(bad, 2, "x")
    with pytest.raises(ValueError, match="heads='max'"):
        AT._check_modes("max", "both", "x")
    with pytest.raises(ValueError, match="direction='up'"):
        AT._check_modes("mean", "up", "x")
    m = AT.AttentionMaps(torch.tensor([[0, 0], [0, 1]]), (0, 1), ("pv2text", "text2pv"), "mean")
    m.maps[(1, 1, "text2pv")] = torch.ones(2, 3)
    assert m.get(1, -1, "text2pv") is m.maps[(1, 1, "text2pv")] and m.get(1, 1, "text2pv") is m.get(1, -1, "text2pv")
    with pytest.raises(ValueError, match="name one direction"):
        m.get(0)
    with pytest.raises(IndexError):
        m.get(2, 0, "pv2text")
    with pytest.raises(KeyError):
        m.get(0, 5, "pv2text")
