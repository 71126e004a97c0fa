"""spmm_s2s_loss (csrc/losses.hip) -- next-token cross-entropy with label 0 ignored on the decoder's packed or dense rows -- against a float64
restatement and its fp32 twin (helpers_gpu.check_ref: the bound comes from the fp32 evaluation of the same formula; dlogits is a bf16 output).

The shared batch: L = 20, product lengths (1, 2, 5, 12, 20, 8, 3, 20) -> 71 packed rows, 63 labels; sequence 0 has no label at all, and the
last rows of sequences 4 and 7 are position L - 1."""
import pytest
import torch
import torch.nn.functional as F

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
    """[CLS] tokens [SEP] PAD...; the tokens cover 1 and V - 1."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), L, dtype=torch.int32)
    for i, n in enumerate(lens):
        ids[i, 0] = 2
        if n > 2:
            ids[i, 1:n - 1] = torch.randint(4, V, (n - 2,), generator=g).int()
        if n > 1:
            ids[i, n - 1] = 3
    return ids


def _shared(V):
    ids = _ids(LENS, L20, V, seed=7)
    ids[3, 4], ids[4, 9] = V - 1, 1                    # the largest label and the smallest one that counts
    rows = torch.cat([torch.arange(n) + s * L20 for s, n in enumerate(LENS)])
    assert rows.numel() == 71
    return ids, rows


def _labels(ids, row_of, V):
    """The kernel's rule: row r is dense row d; its label is ids[d + 1] unless d is a last position; 0 and anything outside [0, V) is ignored."""
    nseq, L = ids.shape
    flat = ids.reshape(-1).long()
    d = torch.arange(nseq * L) if row_of is None else row_of.long()
    lab = torch.where(d % L < L - 1, flat[(d + 1).clamp(max=nseq * L - 1)], torch.zeros_like(d))
    return torch.where((lab > 0) & (lab < V), lab, torch.zeros_like(lab))


def _ref(logits, lab, gscale, dtype):
    x = logits.to(dtype).clone().requires_grad_(True)
    keep = lab != 0
    n = int(keep.sum())
    if n == 0:
        return torch.zeros((), dtype=dtype), torch.zeros_like(x), 0
    loss = -torch.log_softmax(x, -1)[keep, lab[keep]].sum() / n
    (gscale * loss).backward()
    return loss.detach(), x.grad, n


def _run(ops, tag, ids, row_of, V, Vpad, *, ldl=320, gscale=0.7, with_grad=True, seed=11, ws=None, check=True):
    nseq, L = ids.shape
    rows = nseq * L if row_of is None else row_of.numel()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g) * 2.0
    xd = torch.full((rows, ldl), float("nan"), device="cuda")          # (columns V.. must never be read)
    xd[:, :V] = x.cuda()
    losses = torch.tensor([0.5, 0.25, 2.0, 1.0], device="cuda")
    ws = torch.zeros(4, dtype=torch.int32, device="cuda") if ws is None else ws
    dl = torch.full((rows, Vpad), float("nan"), dtype=BF, device="cuda") if with_grad else None
    gs = None if gscale is None else torch.tensor([gscale], device="cuda")
    ops.s2s_loss(xd[:, :V], ids.cuda().view(-1), nseq=nseq, L=L, V=V, ws=ws, losses=losses, slot=1, row_of=None if row_of is None else row_of.cuda(),
                 dlogits=dl, gscale=gs)
    torch.cuda.synchronize()
    lab = _labels(ids, row_of, V)
    gv = 1.0 if gscale is None else float(torch.tensor(gscale, dtype=F32))
    l64, d64, n = _ref(x, lab, gv, F64)
    l32, d32, _ = _ref(x, lab, gv, F32)
    out = dict(loss=losses.cpu()[1] - 0.25, dl=None if dl is None else dl.cpu(), n=n, lab=lab, l64=l64, x=x)
    if not check:
        return out
    assert int(ws[0]) == n, (tag, int(ws[0]), n)
    assert torch.equal(losses.cpu()[[0, 2, 3]], torch.tensor([0.5, 2.0, 1.0])), tag
    check_ref(f"s2s_loss[{tag}] loss", losses[1], 0.25 + l64, (0.25 + l32).float())
    if with_grad:
        assert torch.isfinite(dl.float()).all(), tag                              # every element was written over the NaN fill
        check_ref(f"s2s_loss[{tag}] dlogits", dl[:, :V], d64, d32, bf16=True)
        assert not dl[:, V:].float().any(), tag                                   # the padding columns are exact zeros
        assert not dl.cpu()[lab == 0].float().any(), tag                          # so is every row without a label
    return out


def test_one_labelled_row(ops):
    ids = torch.tensor([[2, 7]], dtype=torch.int32)
    out = _run(ops, "1x2", ids, None, 300, 320)
    assert out["n"] == 1


@pytest.mark.parametrize("V,Vpad", [(50, 64), (64, 64), (300, 320)])
def test_shared_batch_packed_and_dense(ops, V, Vpad):
    ids, rows = _shared(V)
    lab = _labels(ids, rows, V)
    assert int((lab != 0).sum()) == 63 and int(lab.max()) == V - 1 and int(lab[lab != 0].min()) == 1
    assert not lab[rows < L20].any() and int(rows[-1]) == 8 * L20 - 1             # sequence 0: no label; the last packed row is a position L - 1
    dense = _run(ops, f"dense V={V}", ids, None, V, Vpad)
    assert dense["n"] == 63
    # the packed launch on the SAME logits rows: gather the dense logits
    x = dense["x"]
    xd = torch.zeros(71, 320, device="cuda")
    xd[:, :V] = x[rows].cuda()
    losses = torch.zeros(4, device="cuda")
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    dl = torch.full((71, Vpad), float("nan"), dtype=BF, device="cuda")
    ops.s2s_loss(xd[:, :V], ids.cuda().view(-1), nseq=8, L=L20, V=V, ws=ws, losses=losses, slot=1, row_of=rows.cuda(), dlogits=dl,
                 gscale=torch.tensor([0.7], device="cuda"))
    torch.cuda.synchronize()
    assert int(ws[0]) == 63
    l64, d64, _ = _ref(x[rows], lab, float(torch.tensor(0.7)), F64)
    l32, d32, _ = _ref(x[rows], lab, float(torch.tensor(0.7)), F32)
    check_ref(f"s2s_loss[packed V={V}] loss", losses[1], l64, l32)
    check_ref(f"s2s_loss[packed V={V}] dlogits", dl[:, :V], d64, d32, bf16=True)
    assert not dl[:, V:].float().any() and torch.isfinite(dl.float()).all()
    # packed against dense: every dense row that was dropped is a zero row, the kept rows agree bit for bit (same row, same n)
    assert torch.equal(dense["dl"][rows], dl.cpu())
    gone = torch.ones(8 * L20, dtype=torch.bool)
    gone[rows] = False
    assert not dense["dl"][gone].float().any()
    assert abs(float(losses[1]) - float(dense["loss"])) <= 4 * 2.0 ** -23 * max(1.0, abs(float(l64)))       # another split over the workgroups
    # ... and the float64 restatement is torch's CrossEntropyLoss(ignore_index=0) on the shifted product (SPMM_models_rxn.py:44-45)
    ce = F.cross_entropy(x.double().view(8, L20, V)[:, :-1].permute(0, 2, 1), ids[:, 1:].long(), ignore_index=0)
    assert abs(float(ce) - float(dense["l64"])) < 1e-12


def test_more_rows_than_one_pass_of_the_grid(ops):
    nseq, L, V = 33, 128, 300                                                     # 4224 rows > 1024 workgroups x 4 waves
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(1, L + 1, (nseq,), generator=g).tolist()
    lens[0], lens[1] = L, 1
    out = _run(ops, "33x128", _ids(lens, L, V, seed=5), None, V, 320)
    assert out["n"] == sum(n - 1 for n in lens)


def test_no_label_at_all_gives_zero_not_nan(ops):
    """Every sequence is one token long: n = 0.  The reference divides 0 by 0; the kernel returns loss 0 and an all-zero gradient."""
    ids = _ids((1,) * 6, 12, 300, seed=1)
    out = _run(ops, "n=0", ids, None, 300, 320)
    assert out["n"] == 0 and float(out["loss"]) == 0.0 and not out["dl"].float().any()
    rows = torch.arange(6) * 12
    out = _run(ops, "n=0 packed", ids, rows, 300, 320)
    assert out["n"] == 0 and float(out["loss"]) == 0.0 and not out["dl"].float().any()


def test_labels_outside_the_vocabulary_are_ignored(ops):
    ids, rows = _shared(50)
    ids[5, 3], ids[5, 5], ids[3, 7] = 50, 4000, -3
    out = _run(ops, "out of range", ids, rows, 50, 64)
    assert out["n"] == 60


def test_loss_only_and_gscale(ops):
    ids, rows = _shared(300)
    lo = _run(ops, "loss only", ids, rows, 300, 320, with_grad=False)
    none = _run(ops, "gscale None", ids, rows, 300, 320, gscale=None)
    one = _run(ops, "gscale 1", ids, rows, 300, 320, gscale=1.0)
    assert torch.equal(none["dl"], one["dl"]) and torch.equal(none["loss"], one["loss"]) and torch.equal(lo["loss"], one["loss"])
    _run(ops, "gscale 0.7", ids, rows, 300, 320, gscale=0.7)


def test_repeated_launch_is_bit_identical_and_the_workspace_reusable(ops):
    ids, rows = _shared(300)
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    big = _ids([40] * 33, 128, 300, seed=9)
    a = _run(ops, "first", big, None, 300, 320, ws=ws)
    b = _run(ops, "second", big, None, 300, 320, ws=ws, check=False)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dl"], b["dl"])
    c = _run(ops, "other batch, same workspace", ids, rows, 300, 320, ws=ws)          # checked against the reference, count included
    assert c["n"] == 63
    fresh = _run(ops, "other batch, fresh workspace", ids, rows, 300, 320, check=False)
    assert torch.equal(c["loss"], fresh["loss"]) and torch.equal(c["dl"], fresh["dl"])
