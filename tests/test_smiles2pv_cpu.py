"""CPU-side checks of the SMILES -> PV product path: the driver's metrics, de-normalisation, batching, tokenisation and flags; the
fallback of decode.predict_properties for models without an engine; the argument validation of spmm_s2p_append; the launch sequence of
the engine path against the header's prototypes (no launch)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spmm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import smiles2pv as S      # noqa: E402


# ------------------------------------------------------------------------------------------------------------------- metrics
def test_r2_on_a_4x3_example():
    """Hand-computed: column 0 perfect (1), column 1 predicts the mean (0), column 2: SS_res = 1 + 0 + 1 + 4 = 6, SS_tot = 20 -> 0.7."""
    y = np.array([[1.0, 2.0, 1.0], [2.0, 4.0, 3.0], [3.0, 6.0, 5.0], [4.0, 8.0, 7.0]])
    p = np.array([[1.0, 5.0, 2.0], [2.0, 5.0, 3.0], [3.0, 5.0, 4.0], [4.0, 5.0, 9.0]])
    r2 = [S.r2_score(y[:, i], p[:, i]) for i in range(3)]
    assert r2[0] == 1.0 and r2[1] == 0.0 and abs(r2[2] - 0.7) < 1e-12
    assert S.r2_score(np.ones(4), np.ones(4)) == 1.0 and S.r2_score(np.ones(4), np.zeros(4)) == 0.0     # constant truth: sklearn's convention
    assert abs(S.r2_score(y[:, 0], y[::-1, 0]) - (1.0 - 20.0 / 5.0)) < 1e-12                              # worse than the mean: negative


def test_metric_eval_matches_hand_computed_numbers():
    """Normalised RMSE per property: sqrt(mean((ref - cand)^2)) = sqrt((0 + 0 + 0 + 4) / 4) = 1 and sqrt((1 + 1 + 1 + 1) / 4) = 1 and 0 ->
    mean 2/3.  r^2 is taken on the de-normalised values; an affine map per property leaves it unchanged: column 0: SS_res 4, SS_tot 5 -> 0.2;
    column 1: SS_res 4, SS_tot 20 -> 0.8; column 2 perfect -> 1: mean 2/3."""
    ref = torch.tensor([[1.0, 2.0, 0.0], [2.0, 4.0, 1.0], [3.0, 6.0, 2.0], [4.0, 8.0, 3.0]])
    cand = torch.tensor([[1.0, 3.0, 0.0], [2.0, 3.0, 1.0], [3.0, 7.0, 2.0], [2.0, 7.0, 3.0]])
    mean, std = torch.tensor([10.0, -3.0, 0.5]), torch.tensor([2.0, 0.5, 7.0])
    n_rmse, r2 = S.metric_eval(ref, cand, mean, std)
    assert abs(n_rmse - 2.0 / 3.0) < 1e-6
    assert abs(r2 - (0.2 + 0.8 + 1.0) / 3.0) < 1e-6


def test_denormalize_and_csv_round_trip(tmp_path):
    mean, std = torch.tensor([1.0, -2.0]), torch.tensor([3.0, 0.5])
    x = torch.tensor([[0.0, 0.0], [1.0, -2.0]])
    raw = S.denormalize(x, mean, std)
    assert torch.equal(raw, torch.tensor([[1.0, -2.0], [4.0, -3.0]]))
    out = tmp_path / "p.csv"
    S.write_csv(str(out), ["CCO", "c1ccccc1"], raw, ["a", "b"])
    lines = out.read_text().strip().splitlines()
    assert lines[0] == "smiles,a,b" and lines[1] == "CCO,1.0,-2.0" and lines[2] == "c1ccccc1,4.0,-3.0"
    ref = tmp_path / "r.csv"
    ref.write_text("a,b\n1.0,-2.0\n4.0,-3.0\n")
    assert torch.equal(S.read_reference(str(ref), 2, 2), raw)
    with pytest.raises(SystemExit, match="expected 3 molecules"):
        S.read_reference(str(ref), 3, 2)


def test_read_normalize_is_the_generation_drivers(tmp_path):
    import pv2smiles
    assert S.read_normalize is pv2smiles.read_normalize
    np.savez(tmp_path / "n.npz", mean=np.arange(53.0), std=np.full(53, 2.0))
    mean, std = S.read_normalize(str(tmp_path / "n.npz"))
    assert mean.dtype == torch.float32 and float(mean[52]) == 52.0 and float(std[0]) == 2.0


# ------------------------------------------------------------------------------------------------------------------ batching
def test_length_sorted_batches_restore_input_order():
    lengths = [7, 3, 9, 3, 1, 12, 5]
    batches = S.length_sorted_batches(lengths, 3)
    assert [b.tolist() for b in batches] == [[4, 1, 3], [6, 0, 2], [5]]                    # by length, ties in input order
    assert sorted(i for b in batches for i in b.tolist()) == list(range(7))

    class Tok:                                                                             # one token id per character
        pad_token_id = 0

        def encode(self, s, max_length=None):
            return [2] + [ord(c) for c in s[5:]] + [3]

    smiles = ["a" * (n - 1) for n in lengths]
    seen = []

    def predict(model, ids, mask, n_props):
        seen.append(tuple(ids.shape))
        assert torch.equal(mask, (ids != 0).long()) and int(mask[:, 0].min()) == 1
        return mask.sum(1, keepdim=True).float().expand(-1, n_props) * 1.0                 # "prediction" = the molecule's token count

    out = S.predict_all(None, Tok(), smiles, 3, n_props=2, predict=predict)
    assert out[:, 0].tolist() == [float(n) for n in lengths]                               # input order, whatever the batches were
    assert seen == [(3, 3), (3, 9), (1, 12)]                                                # padded to the batch's longest only


# -------------------------------------------------------------------------------------------------------------- tokenisation
@pytest.fixture(scope="module")
def golden_tok(golden_dir):
    from spmm_amd.tokenizer import SmilesWordPiece
    g = np.load(os.path.join(golden_dir, "tokenizer_vocab300.npz"))
    return SmilesWordPiece([str(v) for v in g["vocab"]]), g


def test_cls_prefix_and_truncation(golden_tok):
    tok, g = golden_tok
    lines = ["Cc1cc(C(=O)NCCN2CCCC2=O)c(C)n1-c1ccc(C#N)cc1", "[CLS]N#Cc1cc(C#N)c(NCCc2cnc(N)s2)nc1Cl", "C(" * 120]
    assert S.with_cls(lines)[0].startswith("[CLS]Cc1") and S.with_cls(lines)[1] == lines[1]
    rows = S.encode(tok, lines)
    full = tok(S.with_cls(lines), padding="longest", truncation=True, max_length=100)
    for r, ids, m in zip(rows, full.input_ids, full.attention_mask):
        assert r == ids[1:1 + int(m.sum()) - 1].tolist()                                   # the tokenizer's own [CLS] dropped, nothing else
    for r in rows[:2]:
        assert r[0] == tok.cls_token_id and r[-1] == tok.sep_token_id and tok.unk_token_id not in r and len(r) < 99
    assert len(rows[2]) == 99 and rows[2][-1] == tok.sep_token_id                          # max_length = 100 counts the dropped [CLS]
    # the golden file's molecules (tokenised by the reference's tokenizer as '[CLS]' + smiles): the driver feeds the same ids
    smiles = [str(s) for s in g["smiles"]]
    smiles = [s[5:] if s.startswith("[CLS]") else s for s in smiles]
    for r, ids, m in zip(S.encode(tok, smiles), g["input_ids"], g["attention_mask"]):
        assert r == ids[1:int(m.sum())].tolist()


def test_read_smiles_skips_blank_lines(tmp_path):
    f = tmp_path / "in.txt"
    f.write_text("CCO\n\n  c1ccccc1  \n")
    assert S.read_smiles(str(f)) == ["CCO", "c1ccccc1"]


# --------------------------------------------------------------------------------------------------------------------- flags
def test_argument_parsing():
    a = S.parse_args([])
    assert (a.checkpoint, a.vocab_filename, a.device, a.batch_size) == ("./Pretrain/checkpoint_SPMM.ckpt", "./vocab_bpe_300.txt", "cuda", 64)
    assert a.input_file and not a.synthetic and not a.tiny and a.reference_space == "normalized"
    a = S.parse_args(["--input_file", "x.txt", "--batch_size", "1000", "--normalize", "n.pkl", "--property_names", "p.txt", "--output", "o.csv",
                      "--reference_csv", "r.csv", "--reference_space", "raw", "--synthetic", "--tiny", "--device", "cpu"])
    assert (a.input_file, a.batch_size, a.normalize, a.property_names, a.output) == ("x.txt", 1000, "n.pkl", "p.txt", "o.csv")
    assert a.reference_csv == "r.csv" and a.reference_space == "raw" and a.synthetic and a.tiny and a.device == "cpu"


def test_driver_refuses_the_cpu_with_the_products_message():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "smiles2pv.py"), "--synthetic", "--tiny", "--device", "cpu"], capture_output=True,
                       text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "no CPU / eager fallback" in r.stderr and "Traceback" not in r.stderr, r.stdout + r.stderr
    h = subprocess.run([sys.executable, os.path.join(ROOT, "smiles2pv.py"), "--help"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert h.returncode == 0 and "--reference_csv" in h.stdout and "--batch_size" in h.stdout


# ------------------------------------------------------------------------------------------------------------------ fallback
def test_predict_properties_falls_back_to_the_module_loop_on_the_oracle():
    from spmm_amd import decode
    sd = O.closed_form_state_dict(O.tiny_cfg())
    om = O.OracleModule(sd, O.tiny_cfg())
    _, ids, mask = O.synthetic_batch(3, 12, seed=3)
    want = decode.smiles_to_pv(om, ids, mask, n_props=4)
    got = decode.predict_properties(om, ids, mask, n_props=4)
    assert torch.equal(got, want) and tuple(got.shape) == (3, 4)


# ----------------------------------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def built():
    so = os.path.join(ROOT, "spmm_amd", "libspmm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return so


def _s2p_args(**kw):
    a = dict(y=64, ldy=768, w3=64, b3=64, pe_w=64, pe_b=64, pos=64, type0=None, gamma=64, beta=64, eps=1e-12, pred=64, ldp=53, xcache=64, rows=4, H=768,
             n_props=53, i=0)
    a.update(kw)
    return tuple(a.values()) + (None,)


def test_s2p_append_validates_its_arguments_without_touching_the_gpu(built):
    """Every refusal happens before the launch (the non-null pointers here are never dereferenced)."""
    from spmm_amd._lib import lib
    L = lib()
    for kw, msg in ((dict(H=100), "multiple of 64"), (dict(H=2048), "multiple of 64"), (dict(i=53), r"0 <= i < n_props"), (dict(i=-1), r"0 <= i < n_props"),
                    (dict(ldy=512), "ldy=512"), (dict(ldp=52), "ldp=52"), (dict(rows=0), "rows=0"), (dict(y=None), "are required"),
                    (dict(xcache=None), "appends a cache row"), (dict(pos=None), "appends a cache row"), (dict(gamma=72), "misaligned"), (dict(y=68), "misaligned")):
        with pytest.raises(RuntimeError, match=msg):
            L.call("spmm_s2p_append", *_s2p_args(**kw))


def test_engine_path_launch_sequence_matches_the_header():
    """predict_properties on the engine with launches replaced by prototype checks (ops._DRY_RUN): every call matches include/spmm_hip.h,
    a step gathers the prefix once, appends once, embeds nothing again, and the cross-attention keys / values are projected once per fusion
    layer for the whole run -- not once per step as the module loop does."""
    from spmm_amd import decode, ops
    from spmm_amd.config import tiny_config
    from spmm_amd.model import SPMM
    cfg = tiny_config()
    cfg.text.num_hidden_layers, cfg.prop.num_hidden_layers = 3, 2                       # two fusion layers: one below the last-rows-only one
    old = ops._DRY_RUN
    ops._DRY_RUN = True
    try:
        m = SPMM(spmm_config=cfg, no_train=True, device="cpu").eval()
        _, ids, mask = O.synthetic_batch(5, 20, seed=3)
        n = 6
        ops._dry_log.clear()
        out = decode.predict_properties(m, ids, mask, n_props=n)
        new = list(ops._dry_log)
        ops._dry_log.clear()
        decode.smiles_to_pv(m, ids, mask, n_props=n)
        loop = list(ops._dry_log)
    finally:
        ops._DRY_RUN = old
    assert tuple(out.shape) == (5, n) and out.dtype == torch.float32
    assert new.count("spmm_s2p_append") == n and new.count("spmm_gather_rows") == 2 * n and new.count("spmm_embed_ln_fwd") == 2
    assert "spmm_rows_linear" not in new and new.count("spmm_pack_plan") == 1
    # GEMMs: the module loop projects the text's keys | values in both fusion layers at every step (2 n launches); the engine path twice
    # in all, and its last layer spends one launch per step on the self-attention keys | values of the whole prefix (engine.SelfKV)
    assert loop.count("spmm_gemm_nt") - new.count("spmm_gemm_nt") == 2 * n - (2 + n), (loop.count("spmm_gemm_nt"), new.count("spmm_gemm_nt"))
