"""Shape and edge coverage of the loss-side kernels (csrc/losses.hip) against a float64 evaluation of the reference's formulas
(SPMM_models.py lines cited in the kernel header) in plain torch on the CPU: ita_rows, sample_neg, lm_loss, itm_head, mpm_head,
l2norm, enqueue, queue_shadow.  Inputs come from a seeded CPU generator and are rounded to bf16 first where the kernel reads bf16.

Tolerances (tests/helpers_gpu.py::check_ref) come from the reference, never from the kernel: E32 is the largest error of the same
formula in fp32 torch on the CPU against float64; an fp32 output may be max(8 * E32, 4 fp32 ulp of the output's magnitude) away, a bf16
output one bf16 ulp of the reference (relative 2^-7) more.  Casts, shadows, sentinels and skip paths are compared with torch.equal.
Every comparison prints `[tol] name: E32 kernel bound` (pytest -s).

Measured on an MI355X: per case the output with the least margin (kernel error / bound); for a bf16 output the kernel column is what
remains past one bf16 ulp of the reference.

| case | output | E32 | kernel | bound |
|---|---|---|---|---|
| ita_rows[J1028] | dtemp | 1.1e-05 | 4.5e-06 | 8.6e-05 |
| ita_rows[J2053_ld2060] | dtemp | 2.3e-05 | 2.3e-05 | 1.8e-04 |
| ita_rows[J2053_ld2053] | loss | 1.2e-06 | 7.2e-07 | 9.5e-06 |
| ita_rows[J1028_misaligned] | dtemp | 1.1e-05 | 1.1e-05 | 8.6e-05 |
| ita_rows[J1028_dS1030] | dtemp | 1.1e-05 | 4.5e-06 | 8.6e-05 |
| ita_rows[J36868] | dtemp | 5.9e-05 | 4.8e-05 | 4.7e-04 |
| lm_loss[4224rows] | loss | 4.3e-07 | 4.2e-08 | 3.5e-06 |
| lm_loss[V50] | loss | 3.2e-07 | 1.5e-07 | 2.6e-06 |
| lm_loss[ldl320] | loss | 2.1e-07 | 2.7e-07 | 1.9e-06 |
| lm_loss[allpad] | loss | 7.9e-08 | 7.9e-08 | 1.9e-06 |
| lm_loss[loss only] | loss | 2.1e-07 | 2.7e-07 | 1.9e-06 |
| lm_loss[gscale None] | loss | 2.1e-07 | 2.7e-07 | 1.9e-06 |
| lm_loss[gscale 1] | loss | 2.1e-07 | 2.7e-07 | 1.9e-06 |
| mpm_head[40x54x768 bf16] | loss | 2.2e-06 | 1.6e-06 | 1.7e-05 |
| mpm_head[40x54x768 fp32] | db | 3.7e-07 | 2.0e-06 | 3.0e-06 |
| mpm_head[6x54x1024 bf16] | db | 4.9e-07 | 4.9e-07 | 3.9e-06 |
| mpm_head[6x54x1024 fp32] | dw | 4.0e-06 | 1.9e-06 | 3.2e-05 |
| mpm_head[6x54x200 bf16] | loss | 4.8e-07 | 4.8e-07 | 3.8e-06 |
| mpm_head[6x54x200 fp32] | db | 6.4e-08 | 6.5e-07 | 9.5e-07 |
| mpm_head[3x2x128 bf16] | loss | 1.1e-06 | 1.8e-06 | 8.9e-06 |
| mpm_head[3x2x128 fp32] | loss | 2.4e-07 | 1.2e-06 | 1.9e-06 |
| mpm_head fwd[40x54x768 bf16] | loss | 2.2e-06 | 1.6e-06 | 1.7e-05 |
| mpm_head fwd[40x54x768 fp32] | pred | 3.1e-06 | 8.5e-07 | 2.5e-05 |
| mpm_head fwd[6x54x1024 bf16] | pred | 3.1e-06 | 1.1e-06 | 2.5e-05 |
| mpm_head fwd[6x54x1024 fp32] | pred | 2.5e-06 | 1.1e-06 | 2.0e-05 |
| mpm_head fwd[6x54x200 bf16] | loss | 4.8e-07 | 4.8e-07 | 3.8e-06 |
| mpm_head fwd[6x54x200 fp32] | pred | 8.0e-07 | 3.3e-07 | 6.4e-06 |
| mpm_head fwd[3x2x128 bf16] | loss | 1.1e-06 | 1.8e-06 | 8.9e-06 |
| mpm_head fwd[3x2x128 fp32] | loss | 2.4e-07 | 1.2e-06 | 1.9e-06 |
| itm_head[B5 H768 bf16] | db | 7.2e-09 | 2.3e-08 | 6.0e-08 |
| itm_head[B5 H768 fp32] | db | 6.4e-08 | 1.1e-07 | 5.1e-07 |
| itm_head[B1 H128 bf16] | fwd logits | 1.2e-07 | 1.9e-07 | 9.9e-07 |
| itm_head[B1 H128 fp32] | dW | 1.6e-07 | 1.6e-07 | 1.3e-06 |
| itm_head[B6 H1024 bf16] | db | 3.8e-08 | 1.3e-07 | 3.0e-07 |
| itm_head[B6 H1024 fp32] | loss | 6.0e-08 | 5.4e-07 | 1.9e-06 |
| l2norm[1x64] | y | 1.4e-08 | 1.0e-08 | 1.2e-07 |
| l2norm[1x64 zero row] | nrm | 4.0e-21 | 4.0e-21 | 4.3e-19 |
| l2norm[5x256 zero row] | y | 1.1e-08 | 1.1e-08 | 8.7e-08 |
| l2norm[130x100 zero row] | nrm | 1.1e-06 | 8.5e-07 | 8.7e-06 |
"""
import numpy as np

import pytest
import torch

from helpers_gpu import _host_rng_uniform, check_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32, F64 = torch.float32, torch.float64
SENT = 7.0                                   # sentinel of the buffers a kernel must only partly write


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops as o
    return o


def randn(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def f32v(v):
    """The value a kernel reads from an fp32 scalar holding v, as a Python float."""
    return float(np.float32(v))


def dev_scalar(v, dtype=F32):
    return torch.tensor([v], dtype=dtype, device="cuda")


def sliced(t, extra=8, fill=0.0):
    """A CUDA copy of the 2-D CPU tensor t that is a column slice of a wider matrix -> (view, whole buffer)."""
    buf = torch.full((t.shape[0], t.shape[1] + extra), fill, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    buf = buf.cuda()
    return buf[:, :t.shape[1]], buf


# ------------------------------------------------------------------------------------------------ ita_rows
def _ita_ref(S, SM, B, alpha, temp, dtype):
    """SPMM_models.py:113-131 for the 2B rows of one feature bank: loss, dS (gradient w.r.t. the sims as given), dtemp (s = raw / temp)."""
    s = S.to(dtype).requires_grad_(True)
    sm = SM.to(dtype)
    rows, J = s.shape
    tgt = torch.zeros(rows, J, dtype=dtype)
    tgt[torch.arange(rows), torch.arange(rows) % B] = 1
    tg = alpha * torch.softmax(sm, dim=1) + (1 - alpha) * tgt
    loss = (-(torch.log_softmax(s, dim=1) * tg).sum(1)).view(2, B).mean(1).sum() / 2
    loss.backward()
    dtemp = -(s.grad * s.detach()).sum() / temp
    return loss.detach(), s.grad, dtemp


ITA_CASES = {                      # name: (B, J, layout)
    "J1028": (8, 1028, "contig"),                  # second float4 iteration of the j += 1024 loops
    "J2053_ld2060": (8, 2053, "slice2060"),        # float4 part + a scalar tail
    "J2053_ld2053": (8, 2053, "contig"),           # ldj % 4 != 0: the whole row on the scalar path
    "J1028_misaligned": (8, 1028, "offset1"),      # base one float past a 16-byte boundary: scalar path
    "J1028_dS1030": (8, 1028, "dS1030"),           # J4d = 0 with J4 != 0
    "J36868": (4, 4 + 36864, "contig"),            # the product's row length
}


def _ita_inputs(name):
    B, J, layout = ITA_CASES[name]
    S = (randn(2 * B, J, seed=101, scale=0.3) / f32v(0.07)).float()
    SM = (randn(2 * B, J, seed=102, scale=0.3) / f32v(0.07)).float()
    return B, J, layout, S, SM


def _ita_place(t, layout):
    if layout == "slice2060":
        return sliced(t, extra=2060 - t.shape[1])[0]
    if layout == "offset1":
        flat = torch.zeros(t.numel() + 4, device="cuda")
        assert flat.data_ptr() % 16 == 0
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        return v
    return t.cuda()


@pytest.mark.parametrize("name", list(ITA_CASES))
def test_ita_rows_paths(ops, name):
    B, J, layout, S, SM = _ita_inputs(name)
    alpha, temp = f32v(0.4), f32v(0.07)
    Sd = _ita_place(S, layout)
    SMd = SM.cuda() if layout == "offset1" else _ita_place(SM, layout)      # (one misaligned base is enough to leave the float4 path)
    assert SMd.stride() == Sd.stride() and (Sd.data_ptr() % 16 != 0) == (layout == "offset1")
    if layout == "dS1030":
        Jpad, wide = 1030, 1030
    else:
        Jpad = (J + 63) // 64 * 64
        wide = Jpad + 8
    dbuf = torch.full((2 * B, wide), SENT, dtype=BF, device="cuda")
    dS = dbuf[:, :Jpad]
    losses = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0], device="cuda")
    l0 = losses.clone()
    dtemp, flag = dev_scalar(-2.0), torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.ita_rows(Sd, SMd, dS, B=B, J=J, alpha=dev_scalar(0.4), temp=dev_scalar(0.07), losses=losses, slot=2, dtemp=dtemp, nan_flag=flag)
    l64, d64, t64 = _ita_ref(S, SM, B, alpha, temp, F64)
    l32, d32, t32 = _ita_ref(S, SM, B, alpha, temp, F32)
    check_ref(f"ita_rows[{name}] loss", losses[2], 1.0 + l64, (1.0 + l32).float())
    check_ref(f"ita_rows[{name}] dtemp", dtemp, -2.0 + t64.view(1), (-2.0 + t32).float().view(1))
    check_ref(f"ita_rows[{name}] dS", dS[:, :J], d64, d32, bf16=True)
    keep = torch.arange(8) != 2
    assert torch.equal(losses.cpu()[keep], l0.cpu()[keep]), "another loss slot was written"
    assert (dS[:, J:] == 0).all(), "columns J..Jpad must be exactly 0"
    assert (dbuf[:, Jpad:] == SENT).all(), "columns beyond Jpad were written"
    assert flag.item() == 0


def test_ita_rows_nan_flag(ops):
    B, J, _, S, SM = _ita_inputs("J1028")
    S[3, 517] = float("nan")
    dS = torch.empty(2 * B, 1088, dtype=BF, device="cuda")
    losses, dtemp = torch.zeros(8, device="cuda"), dev_scalar(0.0)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.ita_rows(S.cuda(), SM.cuda(), dS, B=B, J=J, alpha=dev_scalar(0.4), temp=dev_scalar(0.07), losses=losses, slot=0, dtemp=dtemp, nan_flag=flag)
    assert flag.item() == 1
    assert not torch.isnan(dS[4].float()).any(), "the NaN of row 3 leaked into another row"


# ------------------------------------------------------------------------------------------------ sample_neg
def _expected_picks(S, B, u):
    """(pick, comparable) per row: the first non-diagonal j whose float64 cumulative weight exceeds u * total; a row is comparable
    unless u * total lies within 1e-5 * total of a bucket boundary (the kernel's fp32 prefix sums may then fall on either side)."""
    s = S[:, :B].double()
    w = torch.exp(s - s.max(1, keepdim=True).values)
    w[torch.arange(B), torch.arange(B)] = 0
    cum = w.cumsum(1)
    total = cum[:, -1:]
    target = torch.from_numpy(u).view(B, 1) * total
    hit = (cum > target) & (w > 0)
    assert hit.any(1).all()
    pick = hit.float().argmax(1)
    comparable = ((cum - target).abs() > 1e-5 * total).all(1)
    return pick, comparable


SEEDS_SALTS = [(1, 0), (20260931, 3), (2 ** 40 + 7, 977), (7919, 2 ** 33 + 5), (123456789, 12)]


@pytest.mark.parametrize("B", [2, 16, 64, 65, 128, 200])
def test_sample_neg_draws_exactly(ops, B):
    S = randn(B, B + 40, seed=200 + B, scale=2.0)
    S[:, B:] = 50.0                                            # queue columns: must be ignored
    Sd = S.cuda()
    out = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    ar = torch.arange(B)
    left_out = total = 0
    for sv, salt in SEEDS_SALTS:
        seed.fill_(sv)
        ops.sample_neg(Sd, B, out, seed=seed, salt=salt)
        o = out.cpu()
        assert ((o >= 0) & (o < B) & (o != ar)).all(), (sv, salt, o.tolist())
        pick, ok = _expected_picks(S, B, _host_rng_uniform(sv, salt, np.arange(B)))
        bad = ok & (o != pick)
        assert not bad.any(), f"seed {sv} salt {salt}: rows {bad.nonzero().flatten().tolist()} got {o[bad].tolist()} want {pick[bad].tolist()}"
        left_out += int((~ok).sum())
        total += B
    print(f"[draw] sample_neg B={B}: {left_out}/{total} rows left out (within 1e-5 * total of a bucket boundary)")
    assert left_out <= 0.02 * total


def test_sample_neg_carries_the_running_sum_between_chunks(ops):
    """Two equal weights, one per 64-wide chunk: the pick is the first iff u < 0.5, which needs `run` carried into the second chunk."""
    B, c1, c2 = 128, 10, 100
    S = torch.full((B, B + 40), -1e4)
    S[:, c1] = S[:, c2] = 0.0
    S[:, B:] = 50.0
    out = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    seen = set()
    for sv, salt in SEEDS_SALTS:
        seed.fill_(sv)
        ops.sample_neg(S.cuda(), B, out, seed=seed, salt=salt)
        u = torch.from_numpy(_host_rng_uniform(sv, salt, np.arange(B)))
        want = torch.where(u < 0.5, c1, c2)
        want[c1], want[c2] = c2, c1                             # the diagonal carries no weight
        assert torch.equal(out.cpu(), want), (sv, salt, (out.cpu() != want).nonzero().flatten().tolist())
        seen |= set(want.tolist())
    assert seen == {c1, c2}


def test_sample_neg_forced_indices_with_offset(ops):
    B = 128
    S = randn(B, B + 40, seed=333).cuda()
    forced = torch.arange(B).roll(37).cuda()
    out = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    ops.sample_neg(S, B, out, forced=forced, offset=3 * B)
    assert torch.equal(out, forced + 3 * B)


# ------------------------------------------------------------------------------------------------ lm_loss
def _lm_ref(logits, logits_m, ids, alpha, gscale, dtype):
    """SPMM_models.py:233-238: (1 - alpha) * CE over ALL next-token targets + alpha * distillation over the non-PAD ones."""
    nseq, L = ids.shape
    V = logits.shape[1]
    x = logits.to(dtype).view(nseq, L, V).clone().requires_grad_(True)
    out, lm = x[:, :-1], logits_m.to(dtype).view(nseq, L, V)[:, :-1]
    labels = ids[:, 1:].long()
    ce = torch.nn.functional.cross_entropy(out.permute(0, 2, 1), labels)
    dist = -(torch.log_softmax(out, -1) * torch.softmax(lm, -1)).sum(-1)
    nz = labels != 0
    loss = (1 - alpha) * ce
    if nz.any():
        loss = loss + alpha * dist[nz].mean()
    (gscale * loss).backward()
    return loss.detach(), x.grad.view(nseq * L, V)


def _lm_ids(nseq, L, V, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ids = torch.randint(1, V, (nseq, L), generator=g)
    for b in range(0, nseq, 3):
        ids[b, L - 1 - (b * 5) % (L - 2):] = 0                   # PAD tails of different lengths
    return ids.int()


def _run_lm(ops, tag, nseq, L, V, Vpad, *, ldl=None, ids=None, with_grad=True, gscale=2.0, alpha=0.3):
    ids = _lm_ids(nseq, L, V, 300 + V) if ids is None else ids
    lg, lgm = randn(nseq * L, V, seed=301), randn(nseq * L, V, seed=302)
    lgd, lgmd = (lg.cuda(), lgm.cuda()) if ldl is None else (sliced(lg, ldl - V)[0], sliced(lgm, ldl - V)[0])
    losses = torch.tensor([0.5, 0.25, 2.0, 1.0], device="cuda")
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    dl = torch.full((nseq * L, Vpad), 5.0, dtype=BF, device="cuda") if with_grad else None
    gs = None if gscale is None else dev_scalar(gscale)
    ops.lm_loss(lgd, lgmd, ids.cuda(), nseq=nseq, L=L, V=V, alpha=dev_scalar(alpha), ws=ws, losses=losses, slot=1, dlogits=dl, gscale=gs)
    g = 1.0 if gscale is None else f32v(gscale)
    l64, d64 = _lm_ref(lg, lgm, ids, f32v(alpha), g, F64)
    l32, d32 = _lm_ref(lg, lgm, ids, f32v(alpha), g, F32)
    check_ref(f"lm_loss[{tag}] loss", losses[1], 0.25 + l64, (0.25 + l32).float())
    assert torch.equal(losses.cpu()[[0, 2, 3]], torch.tensor([0.5, 2.0, 1.0]))
    assert ws[0].item() == int((ids[:, 1:] != 0).sum())
    if with_grad:
        check_ref(f"lm_loss[{tag}] dlogits", dl[:, :V], d64, d32, bf16=True)
        assert (dl[:, V:] == 0).all(), "columns V..Vpad must be exactly 0"
        assert (dl.view(nseq, L, Vpad)[:, L - 1] == 0).all(), "the last position has no label: its gradient rows are 0"
    return dl


@pytest.mark.parametrize("tag,nseq,L,V,Vpad,ldl", [
    ("4224rows", 33, 128, 300, 320, None),           # > 4096 rows: some waves take two rows (grid capped at 1024 workgroups)
    ("V50", 5, 12, 50, 64, None),                    # V < 64: idle lanes in every pass
    ("ldl320", 5, 12, 300, 320, 320),                # logits are a column slice
])
def test_lm_loss_shapes(ops, tag, nseq, L, V, Vpad, ldl):
    _run_lm(ops, tag, nseq, L, V, Vpad, ldl=ldl)


def test_lm_loss_all_pad_labels(ops):
    """Every label is PAD: the distillation term vanishes (n_nonpad = 0 is not divided by) and the CE over PAD targets remains."""
    nseq, L, V = 5, 12, 300
    ids = torch.zeros(nseq, L, dtype=torch.int32)
    ids[:, 0] = 2
    dl = _run_lm(ops, "allpad", nseq, L, V, 320, ids=ids)
    assert torch.isfinite(dl.float()).all()


def test_lm_loss_without_gradient_and_without_gscale(ops):
    nseq, L, V = 5, 12, 300
    _run_lm(ops, "loss only", nseq, L, V, 320, with_grad=False)
    d_none = _run_lm(ops, "gscale None", nseq, L, V, 320, gscale=None)
    d_one = _run_lm(ops, "gscale 1", nseq, L, V, 320, gscale=1.0)
    assert torch.equal(d_none, d_one)


# ------------------------------------------------------------------------------------------------ mpm_head
def _mpm_ref(h, w, b, target, mask, gscale, dtype):
    """SPMM_models.py:250-256: pred = h[:, :-1] . w + b, 5 * MSE over the properties that are not masked."""
    hr = h.to(dtype).clone().requires_grad_(True)
    wr, br = w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)
    pred = hr[:, :-1] @ wr + br
    keep = mask == 0
    loss = torch.nn.functional.mse_loss(pred[keep], target.to(dtype)[keep]) * 5 if keep.any() else pred.sum() * 0
    (gscale * loss).backward()
    return pred.detach(), loss.detach(), hr.grad, wr.grad, br.grad


def _mpm_inputs(B, Lp, H, xdtype, all_masked=False):
    h = randn(B, Lp, H, seed=400 + H).to(xdtype)
    w, b = randn(H, seed=401, scale=0.1), randn(1, seed=402)
    target = randn(B, Lp - 1, seed=403)
    g = torch.Generator(device="cpu").manual_seed(404)
    mask = torch.ones(B, Lp - 1) if all_masked else torch.bernoulli(torch.full((B, Lp - 1), 0.5), generator=g)
    return h, w, b, target, mask


MPM_SHAPES = [(40, 54, 768), (6, 54, 1024), (6, 54, 200), (3, 2, 128)]      # 2160 rows > 2048: the grid-stride loop; register chunks 2..15


@pytest.mark.parametrize("xdtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,Lp,H", MPM_SHAPES)
def test_mpm_head_fwd_bwd(ops, B, Lp, H, xdtype):
    h, w, b, target, mask = _mpm_inputs(B, Lp, H, xdtype)
    tag = f"mpm_head[{B}x{Lp}x{H} {'bf16' if xdtype == BF else 'fp32'}]"
    losses = torch.tensor([0.5, 0.25, 2.0, 1.0], device="cuda")
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    dh = torch.full((B * Lp, H), SENT, dtype=BF, device="cuda")
    dw0, db0 = randn(H, seed=405, scale=0.01), torch.tensor([0.125])
    dw, db = dw0.cuda(), db0.cuda()
    pred = torch.full((B, Lp - 1), SENT, device="cuda")
    ops.mpm_head(h.view(B * Lp, H).cuda(), Lp, H, w.cuda(), b.cuda(), target.cuda(), mask.cuda(), B=B, ws=ws, losses=losses, slot=3, pred=pred,
                 dh=dh, dw=dw, db=db, gscale=dev_scalar(0.75))
    r64, r32 = _mpm_ref(h, w, b, target, mask, 0.75, F64), _mpm_ref(h, w, b, target, mask, 0.75, F32)
    check_ref(f"{tag} pred", pred, r64[0], r32[0])
    check_ref(f"{tag} loss", losses[3], 1.0 + r64[1], (1.0 + r32[1]).float())
    check_ref(f"{tag} dh", dh.view(B, Lp, H), r64[2], r32[2], bf16=True)
    check_ref(f"{tag} dw", dw, dw0.double() + r64[3], dw0 + r32[3])
    check_ref(f"{tag} db", db, db0.double() + r64[4], db0 + r32[4])
    assert ws[0].item() == int((mask == 0).sum())
    assert (dh.view(B, Lp, H)[:, Lp - 1] == 0).all() and not (dh == SENT).any(), "dh must be fully overwritten, zeros at position Lp-1"
    assert torch.equal(losses.cpu()[:3], torch.tensor([0.5, 0.25, 2.0]))


@pytest.mark.parametrize("xdtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,Lp,H", MPM_SHAPES)
def test_mpm_head_forward_only(ops, B, Lp, H, xdtype):
    h, w, b, target, mask = _mpm_inputs(B, Lp, H, xdtype)
    tag = f"mpm_head fwd[{B}x{Lp}x{H} {'bf16' if xdtype == BF else 'fp32'}]"
    losses = torch.tensor([0.5, 0.25, 2.0, 1.0], device="cuda")
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    dw, db = torch.full((H,), SENT, device="cuda"), torch.full((1,), SENT, device="cuda")
    pred = torch.full((B, Lp - 1), SENT, device="cuda")
    ops.mpm_head(h.view(B * Lp, H).cuda(), Lp, H, w.cuda(), b.cuda(), target.cuda(), mask.cuda(), B=B, ws=ws, losses=losses, slot=0, pred=pred,
                 dw=dw, db=db)
    r64, r32 = _mpm_ref(h, w, b, target, mask, 1.0, F64), _mpm_ref(h, w, b, target, mask, 1.0, F32)
    check_ref(f"{tag} pred", pred, r64[0], r32[0])
    check_ref(f"{tag} loss", losses[0], 0.5 + r64[1], (0.5 + r32[1]).float())
    assert (dw == SENT).all() and (db == SENT).all(), "a forward-only call must not touch dw / db"


@pytest.mark.parametrize("B,Lp,H", [(40, 54, 768), (3, 2, 128)])
def test_mpm_head_every_property_masked(ops, B, Lp, H):
    h, w, b, target, mask = _mpm_inputs(B, Lp, H, BF, all_masked=True)
    losses = torch.tensor([0.5, 0.25, 2.0, 1.0], device="cuda")
    ws = torch.full((4,), 9, dtype=torch.int32, device="cuda")
    dh = torch.full((B * Lp, H), SENT, dtype=BF, device="cuda")
    dw0 = randn(H, seed=405, scale=0.01)
    dw, db = dw0.cuda(), torch.tensor([0.125], device="cuda")
    ops.mpm_head(h.view(B * Lp, H).cuda(), Lp, H, w.cuda(), b.cuda(), target.cuda(), mask.cuda(), B=B, ws=ws, losses=losses, slot=2, dh=dh, dw=dw, db=db)
    assert ws[0].item() == 0
    assert torch.equal(losses.cpu(), torch.tensor([0.5, 0.25, 2.0, 1.0])), "no kept property: the loss contribution is 0"
    assert (dh == 0).all() and torch.equal(dw.cpu(), dw0) and db.item() == 0.125, "no kept property: every gradient is 0"


# ------------------------------------------------------------------------------------------------ itm_head
def _itm_ref(a, b, W, bias, B, gscale, dtype):
    """SPMM_models.py:201-206: Linear(2H, 2) on [a | b] + cross entropy against 1 for the first B rows, 0 for the rest."""
    ar, br = a.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)
    Wr, biasr = W.to(dtype).clone().requires_grad_(True), bias.to(dtype).clone().requires_grad_(True)
    lg = torch.cat([ar, br], -1) @ Wr.t() + biasr
    n = a.shape[0]
    lab = torch.cat([torch.ones(B), torch.zeros(n - B)]).long()
    loss = torch.nn.functional.cross_entropy(lg, lab)
    (gscale * loss).backward()
    return lg.detach(), loss.detach(), ar.grad, br.grad, Wr.grad, biasr.grad


@pytest.mark.parametrize("xdtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H", [(5, 768), (1, 128), (6, 1024)])
def test_itm_head_fwd_bwd_and_forward_only(ops, B, H, xdtype):
    n, La, Lb = 3 * B, 3, 2                                    # row strides La * H and Lb * H: the [CLS] row of sequences of different lengths
    tag = f"itm_head[B{B} H{H} {'bf16' if xdtype == BF else 'fp32'}]"
    xa, xb = randn(n, La, H, seed=500 + H).to(xdtype), randn(n, Lb, H, seed=501 + H).to(xdtype)
    W, bias = randn(2, 2 * H, seed=502, scale=0.1), randn(2, seed=503)
    xad, xbd, Wd, biasd = xa.view(n * La, H).cuda(), xb.view(n * Lb, H).cuda(), W.cuda(), bias.cuda()
    r64, r32 = _itm_ref(xa[:, 0], xb[:, 0], W, bias, B, 1.5, F64), _itm_ref(xa[:, 0], xb[:, 0], W, bias, B, 1.5, F32)
    # forward only
    losses = torch.tensor([0.5, 0.25, 2.0, 1.0], device="cuda")
    logits = torch.full((n, 2), SENT, device="cuda")
    dW, db = torch.full((2, 2 * H), SENT, device="cuda"), torch.full((2,), SENT, device="cuda")
    ops.itm_head(xad, La * H, xbd, Lb * H, H, Wd, biasd, n=n, B=B, losses=losses, slot=1, logits=logits, dW=dW, db=db, gscale=dev_scalar(1.5))
    check_ref(f"{tag} fwd logits", logits, r64[0], r32[0])
    check_ref(f"{tag} fwd loss", losses[1], 0.25 + r64[1], (0.25 + r32[1]).float())
    assert (dW == SENT).all() and (db == SENT).all(), "a forward-only call must not touch dW / db"
    # forward + backward, gscale = 1.5, accumulation onto non-zero dW / db
    losses = torch.tensor([0.5, 0.25, 2.0, 1.0], device="cuda")
    logits.fill_(SENT)
    dxa = torch.full((n, La, H), SENT, dtype=BF, device="cuda")
    dxb = torch.full((n, Lb, H), SENT, dtype=BF, device="cuda")
    dW0, db0 = randn(2, 2 * H, seed=504, scale=0.01), torch.tensor([0.125, -0.25])
    dW, db = dW0.cuda(), db0.cuda()
    ops.itm_head(xad, La * H, xbd, Lb * H, H, Wd, biasd, n=n, B=B, losses=losses, slot=3, logits=logits, dxa=dxa, dxb=dxb, dW=dW, db=db,
                 gscale=dev_scalar(1.5))
    check_ref(f"{tag} logits", logits, r64[0], r32[0])
    check_ref(f"{tag} loss", losses[3], 1.0 + r64[1], (1.0 + r32[1]).float())
    check_ref(f"{tag} dxa", dxa[:, 0], r64[2], r32[2], bf16=True)
    check_ref(f"{tag} dxb", dxb[:, 0], r64[3], r32[3], bf16=True)
    check_ref(f"{tag} dW", dW, dW0.double() + r64[4], dW0 + r32[4])
    check_ref(f"{tag} db", db, db0.double() + r64[5], db0 + r32[5])
    assert (dxa[:, 1:] == SENT).all() and (dxb[:, 1:] == SENT).all(), "rows 1..L-1 of dxa / dxb must stay untouched"
    assert torch.equal(losses.cpu()[:3], torch.tensor([0.5, 0.25, 2.0]))


# ------------------------------------------------------------------------------------------------ l2norm
@pytest.mark.parametrize("rows,E,zero_row", [(1, 64, None), (1, 64, 0), (5, 256, 2), (130, 100, 77)])
def test_l2norm_fwd_split_and_bwd(ops, rows, E, zero_row):
    tag = f"l2norm[{rows}x{E}{'' if zero_row is None else ' zero row'}]"
    x = randn(rows, E, seed=600 + E)
    if zero_row is not None:
        x[zero_row] = 0
    xd, _ = sliced(x, extra=8, fill=SENT)                       # x is a column slice
    y, nrm = torch.full((rows, E), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda")
    a3, w3 = torch.full((rows, 3 * E), SENT, dtype=BF, device="cuda"), torch.full((rows, 3 * E), SENT, dtype=BF, device="cuda")
    ldt = (rows + 63) // 64 * 64 + 8
    yT = torch.full((E, ldt), SENT, dtype=BF, device="cuda")
    ops.l2norm_fwd(xd, y, nrm, a3=a3, w3=w3, yT=yT)
    live = torch.ones(rows, dtype=torch.bool)
    if zero_row is not None:
        live[zero_row] = False
        assert (y[zero_row] == 0).all() and nrm[zero_row].item() == f32v(1e-12), "a zero row: y = 0 and the norm is the 1e-12 clamp"
    assert torch.isfinite(y).all() and torch.isfinite(nrm).all()

    def ref(dtype):
        xr = x.to(dtype).clone().requires_grad_(True)
        return xr, torch.nn.functional.normalize(xr, dim=-1), xr.detach().norm(dim=-1).clamp_min(1e-12)
    (x64, y64, n64), (x32, y32, n32) = ref(F64), ref(F32)
    check_ref(f"{tag} y", y, y64.detach(), y32.detach())
    check_ref(f"{tag} nrm", nrm, n64, n32)
    # the bf16 hi / lo split of the kernel's own y, bit for bit
    yc = y.cpu()
    hi = yc.to(BF)
    lo = (yc - hi.float()).to(BF)
    assert torch.equal(a3.cpu(), torch.cat([hi, lo, hi], 1)) and torch.equal(w3.cpu(), torch.cat([hi, hi, lo], 1))
    assert torch.equal(yT[:, :rows].cpu(), hi.t()) and (yT[:, rows:] == SENT).all(), "yT: columns >= rows must stay untouched"
    # a3 . w3 = hi.hi + lo.hi + hi.lo misses y.y by lo.lo + 2 r.(hi + lo) + r.r with |lo| <= 2^-8 |y| and r = y - hi - lo, |r| <= 2^-16 |y|:
    # at most (2^-16 + 2 * 2^-16 * (1 + 2^-8) + 2^-32) < 4 * 2^-16 of sum_i |y_a,i| |y_b,i| for every pair of rows (a, b)
    sim = a3.cpu().double() @ w3.cpu().double().t()
    yy = yc.double() @ yc.double().t()
    assert ((sim - yy).abs() <= 4 * 2.0 ** -16 * (yc.double().abs() @ yc.double().abs().t())).all()
    # backward, with and without gscale (the zero row is left out: its 1e12 scale is not a gradient anyone reads)
    dy = randn(rows, E, seed=601)
    y64.backward(dy.double())
    y32.backward(dy)
    for gs in (None, 0.5):
        dx = torch.full((rows, E), SENT, dtype=BF, device="cuda")
        ops.l2norm_bwd(dy.cuda(), y, nrm, dx, gscale=None if gs is None else dev_scalar(gs))
        g = 1.0 if gs is None else gs
        if live.any():
            check_ref(f"{tag} dx gscale={gs}", dx.cpu()[live], g * x64.grad[live], g * x32.grad[live], bf16=True)
        assert not (dx == SENT).any()


# ------------------------------------------------------------------------------------------------ enqueue / queue_shadow
def _split(v):
    hi = v.to(BF)
    return hi, (v - hi.float()).to(BF)


def test_enqueue_many_rows_wrap_advance_and_skip(ops):
    """n = 512 > the 256 workgroups of the launch (the i += gridDim.x loop); pointer wrap; advance = False; skip_flag."""
    n, E, Q, Bloc = 512, 256, 1024, 8
    ldt = Bloc + Q + 8
    q0 = torch.nn.functional.normalize(randn(E, Q, seed=700), dim=0)
    queue = q0.cuda()
    w3 = torch.full((Bloc + Q, 3 * E), SENT, dtype=BF, device="cuda")
    qT = torch.full((E, ldt), SENT, dtype=BF, device="cuda")
    ptr = torch.tensor([512], device="cuda")
    feats = [torch.nn.functional.normalize(randn(n, E, seed=701 + i), dim=1) for i in range(3)]

    def check(ref, written):
        assert torch.equal(queue.cpu(), ref)
        hi, lo = _split(ref.t().contiguous())
        w, t = w3.cpu(), qT.cpu()
        assert torch.equal(w[Bloc:][written], torch.cat([hi, hi, lo], 1)[written]) and (w[Bloc:][~written] == SENT).all()
        assert torch.equal(t[:, Bloc:Bloc + Q][:, written], hi.t()[:, written]) and (t[:, Bloc:Bloc + Q][:, ~written] == SENT).all()
        assert (w[:Bloc] == SENT).all() and (t[:, :Bloc] == SENT).all() and (t[:, Bloc + Q:] == SENT).all(), "local rows / columns were touched"

    ref, written = q0.clone(), torch.zeros(Q, dtype=torch.bool)
    # advance = False: the columns are written, the pointer stays
    ops.enqueue(feats[0].cuda(), queue, w3, qT, ptr, Bloc=Bloc, advance=False)
    ref[:, 512:] = feats[0].t(); written[512:] = True
    assert ptr.item() == 512
    check(ref, written)
    # skip_flag = 1: nothing moves
    skip = torch.ones(1, dtype=torch.int32, device="cuda")
    ops.enqueue(feats[1].cuda(), queue, w3, qT, ptr, Bloc=Bloc, skip_flag=skip)
    assert ptr.item() == 512
    check(ref, written)
    # two real calls (skip_flag = 0); the second starts after the pointer wrapped
    skip.zero_()
    ops.enqueue(feats[1].cuda(), queue, w3, qT, ptr, Bloc=Bloc, skip_flag=skip)
    ref[:, 512:] = feats[1].t()
    assert ptr.item() == 0
    check(ref, written)
    ops.enqueue(feats[2].cuda(), queue, w3, qT, ptr, Bloc=Bloc)
    ref[:, :512] = feats[2].t(); written[:512] = True
    assert ptr.item() == 512
    check(ref, written)


def test_queue_shadow_grid_stride(ops):
    E, Q, Bloc = 256, 2048, 8                                   # E * Q = 524 288 > the 262 144 threads of the launch
    ldt = Bloc + Q + 8
    q0 = torch.nn.functional.normalize(randn(E, Q, seed=710), dim=0)
    w3 = torch.full((Bloc + Q, 3 * E), SENT, dtype=BF, device="cuda")
    qT = torch.full((E, ldt), SENT, dtype=BF, device="cuda")
    ops.queue_shadow(q0.cuda(), w3, qT, Bloc=Bloc)
    hi, lo = _split(q0.t().contiguous())
    assert torch.equal(w3[Bloc:].cpu(), torch.cat([hi, hi, lo], 1)) and torch.equal(qT[:, Bloc:Bloc + Q].cpu(), hi.t())
    assert (w3[:Bloc] == SENT).all() and (qT[:, :Bloc] == SENT).all() and (qT[:, Bloc + Q:] == SENT).all()
