"""spmm_logit_warp (csrc/warp.hip) on the GPU against the float64 brute force of tests/warp_reference.py: the kept set exactly, kept
values within the four-rounding bound, dropped entries exactly -inf, padding and rows past R untouched; equal values cut by the index
rule; a row's result independent of the launch it is in.  The cases and their seeds are warp_reference's: the CPU suite asserts that no
row of them sits within 1e-4 of its cut."""
import pytest
import torch

import warp_reference as WR

pytestmark = pytest.mark.gpu

CASES = WR.cases()
SENTINEL = -12345.0


def _run(c, lc, lu):
    """The case on the device -> (out [R + 2, ldo] on the host, with two guard rows behind the R rows, its input buffers afterwards)."""
    from spmm_amd import ops
    R, V = c["R"], c["V"]
    kw = WR.case_kwargs(c)
    guard = torch.full((2, lc.shape[1]), 7.5)
    lc_d = torch.cat([lc, guard]).cuda()
    lu_d = None if lu is None else torch.cat([lu, guard]).cuda()
    if c["alias"]:
        out_d = lc_d
    else:
        out_d = torch.full((R + 2, V + c["pad_out"]), SENTINEL, device="cuda")
    got = ops.logit_warp(lc_d[:R, :V], None if lu_d is None else lu_d[:R, :V], out=out_d[:R, :V], **kw)
    assert got.data_ptr() == out_d.data_ptr()
    torch.cuda.synchronize()
    return out_d.cpu(), lc_d.cpu(), None if lu_d is None else lu_d.cpu()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("c", CASES, ids=[WR.case_id(c) for c in CASES])
def test_the_kernel_equals_the_brute_force(c):
    lc, lu = WR.case_inputs(c)
    R, V = c["R"], c["V"]
    kw = WR.case_kwargs(c)
    want = WR.brute_force(lc[:, :V], None if lu is None else lu[:, :V], **kw)
    out, lc_after, lu_after = _run(c, lc, lu)
    got = out[:R, :V].double()
    kept = torch.isfinite(want)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(torch.isfinite(got), kept), (torch.isfinite(got) != kept).nonzero()[:8].tolist()
    assert bool((got[~kept] == -float("inf")).all())
    bound = WR.value_bound(lc[:, :V], None if lu is None else lu[:, :V], kw["w"], kw["temperature"])
    err = (got - want)[kept].abs()
    ratio = float((err / bound[kept]).max())
    print(f"{WR.case_id(c)}: kept {int(kept.sum())} of {kept.numel()}, worst |error| / bound {ratio:.3f}")
    assert bool((err <= bound[kept]).all()), ratio
    if lu is None and kw["temperature"] == 1.0:
        assert _same_bits(out[:R, :V][kept], lc[:, :V][kept])               # nothing to round: the bits of lc
    # padding, guard rows, and the inputs
    if c["alias"]:
        assert bool(torch.isnan(out[:R, V:]).all()) and bool((out[R:] == 7.5).all())
    else:
        assert bool((out[:R, V:] == SENTINEL).all()) and bool((out[R:] == SENTINEL).all())
        assert _same_bits(lc_after[:R], lc) and bool((lc_after[R:] == 7.5).all())
    if lu is not None:
        assert _same_bits(lu_after[:R], lu) and bool((lu_after[R:] == 7.5).all())


def test_equal_values_are_cut_by_the_index_rule():
    """lu absent, temperature 1, blocks of exactly equal logits across the top-k cut and the nucleus cut: the kept set is the brute force's,
    which keeps the lower indices of a block, and the kept values are lc's bits."""
    from spmm_amd import ops
    lc, kw = WR.ties_case()
    want = WR.brute_force(lc, None, **kw)
    out = ops.logit_warp(lc.cuda().clone(), None, **kw).cpu()
    kept = torch.isfinite(want)
    assert torch.equal(torch.isfinite(out), kept) and bool((out[~kept] == -float("inf")).all())
    assert _same_bits(out[kept], lc[kept])
    rows = [r.nonzero().flatten().tolist() for r in torch.isfinite(out)]
    assert rows[0] == list(range(10, 19)) and rows[1] == [3, 250, 251] and rows[2] == [100, 101, 102, 103, 104]
    assert rows[3] == [0, 50, 100, 150] and rows[4] == list(range(9))
    only_k = ops.logit_warp(lc.cuda().clone(), None, top_k=17, min_keep=2).cpu()
    assert torch.isfinite(only_k[0]).nonzero().flatten().tolist() == list(range(10, 27))
    assert torch.isfinite(only_k[4]).nonzero().flatten().tolist() == list(range(17))


@pytest.mark.parametrize("V", [300, 512])
def test_a_row_alone_and_in_a_batch_gives_the_same_bits(V):
    from spmm_amd import ops
    g = torch.Generator().manual_seed(77 + V)
    lc, lu = (torch.randn(9, V, generator=g) * 2).cuda(), (torch.randn(9, V, generator=g) * 2).cuda()
    kw = dict(w=1.5, temperature=0.7, top_k=40, top_p=0.9, min_keep=2)
    batch = ops.logit_warp(lc, lu, out=torch.empty_like(lc), **kw)
    for r in (0, 3, 4, 8):                                                   # every wave slot of a workgroup, and the last, lone row
        alone = ops.logit_warp(lc[r:r + 1], lu[r:r + 1], out=torch.empty(1, V, device="cuda"), **kw)
        assert _same_bits(alone.cpu()[0], batch.cpu()[r]), r
    assert 2 <= int(torch.isfinite(batch).sum(1).min()) and int(torch.isfinite(batch).sum(1).max()) <= 40


def test_the_defaults_pass_the_logits_through():
    """Everything at its default is a copy (in place: nothing changes), bit for bit, -0 and denormals included."""
    from spmm_amd import ops
    x = torch.randn(5, 300, generator=torch.Generator().manual_seed(5)) * 2
    x[0, 0], x[1, 7], x[2, 299] = -0.0, 1e-41, -1e-40
    d = x.cuda()
    assert _same_bits(ops.logit_warp(d, min_keep=8).cpu(), x)
    assert _same_bits(ops.logit_warp(x.cuda(), out=torch.zeros(5, 300, device="cuda"), top_k=300, min_keep=1).cpu(), x)
