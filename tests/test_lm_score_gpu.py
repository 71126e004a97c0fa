"""spmm_lm_score (csrc/score.hip) -- tied LM head, log_softmax and the label gather in one launch -- against a float64 restatement computed
from the bf16-rounded y and Wd (logits = y Wd^T + bias, log_softmax, gather, per-sequence sums in row order) and its fp32 twin
(helpers_gpu.check_ref: the bound comes from the fp32 evaluation of the same formula; no hand-set tolerance).

Every launch of this file reads y and Wd through row strides longer than H whose slack columns are NaN, takes its bias from the middle of a
NaN-filled buffer and writes outputs that were pre-filled with NaN: anything read outside the contract or left unwritten shows as a NaN.

The shared batch is that of tests/test_s2s_loss_gpu.py: L = 20, lengths (1, 2, 5, 12, 20, 8, 3, 20) -> 71 packed rows, 63 labels; sequence 0
has no label at all, and the last rows of sequences 4 and 7 are position L - 1."""
import numpy as np
import pytest
import torch

from helpers_gpu import check_ref

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LENS, L20 = (1, 2, 5, 12, 20, 8, 3, 20), 20


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops
    return ops


def _ids(lens, L, V, seed):
    """[CLS] tokens PAD...: every token after position 0 is a label in 1 .. V - 1."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), L, dtype=torch.int32)
    for i, n in enumerate(lens):
        ids[i, 0] = 1
        if n > 1:
            ids[i, 1:n] = torch.randint(1, V, (n - 1,), generator=g).int()
    return ids


def _shared(V):
    ids = _ids(LENS, L20, V, seed=7)
    ids[3, 4], ids[4, 9] = V - 1, 1                    # the largest label and the smallest one that counts
    rows = torch.cat([torch.arange(n) + s * L20 for s, n in enumerate(LENS)])
    assert rows.numel() == 71
    return ids, rows


def _spans(lens):
    r0 = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return torch.tensor(r0, dtype=torch.int32), torch.tensor(lens, dtype=torch.int32)


def _labels(ids, row_of, V):
    """The kernel's rule: row r is dense row d; its label is ids[d + 1] unless d is a last position; 0 and anything outside [0, V) is ignored."""
    nseq, L = ids.shape
    flat = ids.reshape(-1).long()
    d = torch.arange(nseq * L) if row_of is None else row_of.long()
    lab = torch.where(d % L < L - 1, flat[(d + 1).clamp(max=nseq * L - 1)], torch.zeros_like(d))
    return torch.where((lab > 0) & (lab < V), lab, torch.zeros_like(lab))


def _data(rows, H, V, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(rows, H, generator=g) * scale).to(BF)
    Wd = (torch.randn(V, H, generator=g) * 0.5).to(BF)
    bias = torch.randn(V, generator=g)
    return y, Wd, bias


def _ref(y, Wd, bias, lab, dtype):
    lp = torch.log_softmax(y.to(dtype) @ Wd.to(dtype).T + bias.to(dtype), dim=-1)
    t = lp.gather(1, lab[:, None])[:, 0]
    return torch.where(lab > 0, t, torch.zeros_like(t))


def _seq_sums(tok, row0, lens, np_dtype):
    """Left-to-right sums in row order (np.add.accumulate is sequential)."""
    t = tok.numpy().astype(np_dtype)
    return torch.tensor(np.array([np.add.accumulate(t[r:r + n], dtype=np_dtype)[-1] if n else 0 for r, n in zip(row0.tolist(), lens.tolist())]))


def _launch(ops, y, Wd, bias, ids, row_of=None, spans=None, slack=(8, 16)):
    rows, H = y.shape
    V = Wd.shape[0]
    nseq, L = ids.shape
    nan = float("nan")
    yd = torch.full((rows, H + slack[0]), nan, dtype=BF, device="cuda")
    yd[:, :H] = y.cuda()
    wd = torch.full((V, H + slack[1]), nan, dtype=BF, device="cuda")
    wd[:, :H] = Wd.cuda()
    guard = torch.full((V + 64,), nan, device="cuda")
    guard[32:32 + V] = bias.cuda()
    tok = torch.full((rows,), nan, device="cuda")
    slp = torch.full((nseq,), nan, device="cuda")
    sn = torch.full((nseq,), -7, dtype=torch.int32, device="cuda")
    r0, ln = (None, None) if spans is None else (spans[0].cuda(), spans[1].cuda())
    ops.lm_score(yd[:, :H], wd[:, :H], guard[32:32 + V], ids.cuda().view(-1).contiguous(), nseq=nseq, L=L,
                 row_of=None if row_of is None else row_of.cuda(), seq_row0=r0, seq_len=ln, tok_lp=tok, seq_lp=slp, seq_n=sn)
    torch.cuda.synchronize()
    return tok.cpu(), slp.cpu(), sn.cpu()


def _check(ops, tag, y, Wd, bias, ids, row_of=None, spans=None, slack=(8, 16)):
    nseq, L = ids.shape
    V = Wd.shape[0]
    tok, slp, sn = _launch(ops, y, Wd, bias, ids, row_of, spans, slack)
    assert torch.isfinite(tok).all() and torch.isfinite(slp).all() and (sn >= 0).all(), tag     # every element written over the NaN fill
    lab = _labels(ids, row_of, V)
    yf, wf = y.float(), Wd.float()
    t64, t32 = _ref(yf, wf, bias, lab, F64), _ref(yf, wf, bias, lab, F32)
    check_ref(f"lm_score[{tag}] tok_lp", tok, t64, t32)
    assert not tok[lab == 0].any(), tag                                       # a row without a label holds an exact zero
    r0, ln = spans if spans is not None else (torch.arange(nseq, dtype=torch.int32) * L, torch.full((nseq,), L, dtype=torch.int32))
    check_ref(f"lm_score[{tag}] seq_lp", slp, _seq_sums(t64, r0, ln, np.float64), _seq_sums(t32, r0, ln, np.float32))
    assert torch.equal(slp, _seq_sums(tok, r0, ln, np.float32).float()), tag   # the fp32 left-to-right sum of its own tok_lp, exactly
    n_ref = torch.tensor([int((lab[r:r + n] > 0).sum()) for r, n in zip(r0.tolist(), ln.tolist())], dtype=torch.int32)
    assert torch.equal(sn, n_ref), (tag, sn, n_ref)
    return dict(tok=tok, slp=slp, sn=sn, lab=lab)


@pytest.mark.parametrize("H,V", [(64, 2), (64, 50), (64, 64), (128, 300), (768, 300), (1024, 512)])
def test_shape_edges_on_the_shared_batch_packed_and_dense(ops, H, V):
    ids, rows = _shared(V)
    lab = _labels(ids, rows, V)
    assert int((lab != 0).sum()) == 63 and int(lab.max()) == V - 1 and int(lab[lab != 0].min()) == 1
    assert not lab[rows < L20].any() and int(rows[-1]) == 8 * L20 - 1             # sequence 0: no label; the last packed row is a position L - 1
    y, Wd, bias = _data(8 * L20, H, V, seed=H + V)
    dense = _check(ops, f"dense H={H} V={V}", y, Wd, bias, ids)
    packed = _check(ops, f"packed H={H} V={V}", y[rows], Wd, bias, ids, rows, _spans(LENS))
    assert int(packed["sn"].sum()) == 63 and packed["sn"][0] == 0 and packed["slp"][0] == 0
    assert torch.equal(dense["tok"][rows], packed["tok"])                         # the kept rows agree bit for bit
    assert torch.equal(dense["slp"], packed["slp"]) and torch.equal(dense["sn"], packed["sn"])   # the dropped rows had no label


def test_one_row(ops):
    y, Wd, bias = _data(1, 768, 300, seed=1)
    ids = torch.tensor([[2, 7]], dtype=torch.int32)
    out = _check(ops, "1 row", y, Wd, bias, ids, torch.tensor([0]), _spans([1]))
    assert int(out["sn"][0]) == 1 and float(out["slp"][0]) < 0


def test_contiguous_operands(ops):
    ids, rows = _shared(300)
    y, Wd, bias = _data(71, 768, 300, seed=2)
    _check(ops, "ldy = ldw = H", y, Wd, bias, ids, rows, _spans(LENS), slack=(0, 0))


@pytest.fixture(scope="module")
def big(ops):
    """33 x 128 = 4224 dense rows, H = 768, V = 300: the batch the determinism tests cut rows from.  Sequences 0, 1 and 32 are full, sequence 2
    is one token long."""
    nseq, L, V = 33, 128, 300
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(1, L + 1, (nseq,), generator=g).tolist()
    lens[0], lens[1], lens[2], lens[-1] = L, L, 1, L
    ids = _ids(lens, L, V, seed=5)
    y, Wd, bias = _data(nseq * L, 768, V, seed=4)
    out = _check(ops, "33x128", y, Wd, bias, ids)
    assert int(out["sn"].sum()) == sum(n - 1 for n in lens)
    return dict(y=y, Wd=Wd, bias=bias, ids=ids, lens=lens, L=L, V=V, **out)


def test_more_than_one_row_block_and_a_ragged_last_block(ops, big):
    """4224 rows are 33 row blocks of 128; packed to the valid tokens the count is no multiple of the block."""
    lens, L = big["lens"], big["L"]
    rows = torch.cat([torch.arange(n) + s * L for s, n in enumerate(lens)])
    assert rows.numel() % 128 != 0 and rows.numel() > 128
    out = _check(ops, "33x128 packed", big["y"][rows], big["Wd"], big["bias"], big["ids"], rows, _spans(lens))
    assert torch.equal(out["tok"], big["tok"][rows]) and torch.equal(out["slp"], big["slp"])


def test_more_rows_than_one_pass_of_the_grid(ops):
    """1024 workgroups stride over the 128-row blocks: 1027 blocks, the last one ragged."""
    nseq, L, V, H = 1027 * 2, 64, 50, 64
    g = torch.Generator().manual_seed(8)
    lens = torch.randint(1, L + 1, (nseq,), generator=g).tolist()
    ids = _ids(lens, L, V, seed=6)
    y, Wd, bias = _data(nseq * L - 37, H, V, seed=9)
    rows = torch.arange(nseq * L - 37)                                          # (packed = the dense rows without the last 37)
    r0 = torch.arange(nseq, dtype=torch.int32) * L
    ln = torch.full((nseq,), L, dtype=torch.int32)
    ln[-1] = L - 37
    _check(ops, "1027 blocks", y, Wd, bias, ids, rows, (r0, ln))


def test_labels_outside_the_vocabulary_are_ignored(ops):
    ids, rows = _shared(50)
    ids[5, 3], ids[5, 5], ids[3, 7] = 50, 4000, -3
    y, Wd, bias = _data(71, 64, 50, seed=10)
    out = _check(ops, "out of range", y, Wd, bias, ids, rows, _spans(LENS))
    assert int(out["sn"].sum()) == 60


def test_no_label_at_all_gives_zeros_not_nan(ops):
    ids = _ids((1,) * 6, 12, 300, seed=1)
    y, Wd, bias = _data(72, 128, 300, seed=11)
    out = _check(ops, "n=0 dense", y, Wd, bias, ids)
    assert not out["tok"].any() and not out["slp"].any() and not out["sn"].any()
    rows = torch.arange(6) * 12
    out = _check(ops, "n=0 packed", y[rows], Wd, bias, ids, rows, _spans([1] * 6))
    assert not out["tok"].any() and not out["slp"].any() and not out["sn"].any()


def test_large_logits_do_not_overflow(ops):
    """y scaled (exact bf16 values) until the logits reach about +-80: exp(80) overflows nothing because the row maximum goes first."""
    ids, rows = _shared(300)
    y, Wd, bias = _data(71, 128, 300, seed=12, scale=3.5)
    big_logit = (y.double() @ Wd.double().T).abs().max().item()
    assert 60 < big_logit < 140, big_logit
    _check(ops, f"logits to {big_logit:.0f}", y, Wd, bias, ids, rows, _spans(LENS))


def test_two_launches_agree_bit_for_bit(ops, big):
    tok, slp, sn = _launch(ops, big["y"], big["Wd"], big["bias"], big["ids"])
    assert torch.equal(tok, big["tok"]) and torch.equal(slp, big["slp"]) and torch.equal(sn, big["sn"])


@pytest.mark.parametrize("r", [0, 15, 16, 31, 32, 126, 128, 2000, 4222])
def test_a_row_scores_the_same_alone_as_inside_the_batch(ops, big, r):
    """First, last labelled, middle (the first labelled row from 2000 on), and the rows either side of a 16-row half's, a wave's and a
    workgroup's boundary."""
    L = big["L"]
    r += int((big["lab"][r:] > 0).nonzero()[0])
    label = int(big["lab"][r])
    assert label > 0
    ids = torch.tensor([[1, label]], dtype=torch.int32)
    tok, slp, sn = _launch(ops, big["y"][r:r + 1], big["Wd"], big["bias"], ids, torch.tensor([0]), _spans([1]))
    assert torch.equal(tok, big["tok"][r:r + 1]) and torch.equal(slp, tok) and int(sn[0]) == 1
    # ... and as the first and the last row of another batch
    other = torch.cat([big["y"][r:r + 1], big["y"][300:340], big["y"][r:r + 1]])
    ids2 = torch.zeros(42, 2, dtype=torch.int32)
    ids2[:, 0], ids2[:, 1] = 1, label
    tok2, _, _ = _launch(ops, other, big["Wd"], big["bias"], ids2, torch.arange(42) * 2, _spans([1] * 42))
    assert torch.equal(tok2[[0, 41]], big["tok"][[r, r]])
    assert L == 128
