"""The library paths through a device TokenLibrary (spmm_amd/wordpiece_device.py) against the host one, tiny model: the index build, likelihood
scoring and property prediction take their batches from rows tokenised on the GPU.  The rows are identical, the paths are batch-invariant by
their own tests, so the model outputs must be the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    from spmm_amd import wordpiece_device as W
    from spmm_amd.config import tiny_config
    from spmm_amd.model import SPMM
    from spmm_amd.tokenizer import SmilesWordPiece
    g = np.load(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab300.npz"), allow_pickle=False)
    tok = SmilesWordPiece([str(v) for v in g["vocab"]])
    torch.manual_seed(0)
    model = SPMM(config=None, spmm_config=tiny_config(), no_train=True)
    model.eval()
    rng = np.random.default_rng(11)
    pieces = [p[2:] for p in tok.itos if p.startswith("##")]
    strings = ["".join(pieces[j] for j in rng.integers(0, len(pieces), size=int(rng.integers(1, 40)))) for _ in range(36)]
    long = ""
    while len(long) < 130:                                              # 130 pieces: a character is kept only if it adds one
        c = "CNOc()=1"[int(rng.integers(0, 8))]
        if len(tok.tokenize("[CLS]" + long + c)) == len(long) + 2:
            long += c
    strings += ["CC~O", "CC O", long, "c1ccccc1"]                       # an [UNK] row, a row the host tokenises, a truncated row
    host = W.TokenLibrary.from_strings(tok, strings)
    dev = W.TokenLibrary.from_strings(tok, strings, device=model.device_)
    return dict(W=W, tok=tok, model=model, strings=strings, host=host, dev=dev)


def test_the_rows_and_the_batch_order_are_the_host_s(world):
    host, dev, tok, W = world["host"], world["dev"], world["tok"], world["W"]
    assert dev.on_device and dev.host_rows() == host.rows
    assert host.rows[36] == [tok.unk_token_id, tok.sep_token_id] and len(host.rows[38]) == 99
    _, _, status = W.encode_smiles_device(tok, world["strings"], device=world["model"].device_, return_status=True)
    assert status[36] == W.STATUS_UNK and status[37] == W.STATUS_HOST and (np.delete(status, [36, 37]) == W.STATUS_OK).all()
    for (ia, a_ids, a_mask, a_n), (ib, b_ids, b_mask, b_n) in zip(host.batches(7), dev.batches(7)):
        assert np.array_equal(ia, ib) and a_n == b_n == int(a_mask.sum())
        assert torch.equal(a_ids, b_ids.cpu().long()) and torch.equal(a_mask, b_mask.cpu().long())


def test_molecule_index_build(world):
    from spmm_amd.retrieve import MoleculeIndex
    model, tok, strings = world["model"], world["tok"], world["strings"]
    a = MoleculeIndex.build(model, tok, strings, batch_size=7)
    b = MoleculeIndex.build(model, tok, strings, batch_size=7, tokenizer_device=model.device_)
    c = MoleculeIndex.from_library(model, world["host"], batch_size=7, smiles=strings)
    assert torch.equal(a.ids, b.ids) and torch.equal(a.mask, b.mask) and b.ids.dtype == torch.int64 and not b.ids.is_cuda
    assert torch.equal(a.feats, b.feats) and torch.equal(a.feats, c.feats) and b.smiles == strings
    assert torch.isfinite(a.feats).all()


def test_score_smiles_and_the_driver_s_batch_loop(world):
    import score as D
    from spmm_amd import score as S
    model = world["model"]
    pv = torch.randn(1, 53, generator=torch.Generator().manual_seed(5))

    def score_batch(idx, ids, mask):
        pairs = torch.stack([torch.zeros(len(idx), dtype=torch.int64), torch.arange(len(idx))], dim=1)
        r = S.score_smiles(model, pv, ids, mask, pairs=pairs)
        return r.logp.cpu(), r.n_tokens.cpu()
    a = D.score_all(world["host"], 9, score_batch)
    b = D.score_all(world["dev"], 9, score_batch)
    c = D.score_all(world["host"].rows, 9, score_batch, world["tok"].pad_token_id)
    assert a == b == c and all(np.isfinite(a[0])) and a[1] == [len(r) - 1 for r in world["host"].rows]


def test_predict_properties(world):
    import smiles2pv as D
    model, tok, strings = world["model"], world["tok"], world["strings"]
    strings = strings[28:]                                              # 12 molecules, the [UNK], host and truncated rows among them
    a = D.predict_all(model, tok, strings, 5, n_props=6, host_tokenizer=True)
    b = D.predict_all(model, tok, strings, 5, n_props=6, host_tokenizer=False)
    assert torch.equal(a, b) and torch.isfinite(a).all() and tuple(a.shape) == (len(strings), 6)
