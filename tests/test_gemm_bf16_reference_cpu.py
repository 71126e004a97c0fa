"""tests/gemm_bf16_reference.py checked on the CPU, at every problem tests/test_gemm_bf16_epilogues_gpu.py runs: the float64 reference is the
documented formula, the float32 model of the kernels' arithmetic (two bf16 roundings, the 7.1.26 erf) stays inside the per-element bound,
and the output of a kernel with any one of the seeded defects does not -- so the GPU tests cannot pass a kernel that truncates, drops a
K-tile, reads bias / R / G from the wrong place, exchanges outputs or tiles, writes past N or M, or sums the wrong rows or values."""
import pytest
import torch
import torch.nn.functional as F

import gemm_bf16_reference as G

IDS = [p.name for p in G.PROBLEMS]
ALL_K = G.SHARED_KERNELS + G.P8_KERNELS


def test_constants_are_those_of_the_package():
    from spmm_amd import ops
    assert (G.EPI_BF16, G.EPI_GELU, G.EPI_GELU_GRAD, G.EPI_GELU_DERIV, G.EPI_MUL) == \
           (ops.EPI_BF16, ops.EPI_GELU, ops.EPI_GELU_GRAD, ops.EPI_GELU_DERIV, ops.EPI_MUL)
    hdr = open(ops.__file__.replace("spmm_amd/ops.py", "include/spmm_hip.h")).read()
    for name, v in (("K128", G.K128), ("K256x128", G.K256x128), ("K256", G.K256), ("K128PC", G.K128PC), ("K256P8", G.K256P8),
                    ("K256P8_TILES", G.K256P8_TILES)):
        assert f"#define SPMM_GEMM_{name} {v}\n" in hdr
    assert torch.tensor(G.SENTINEL).to(G.BF).item() == G.SENTINEL


def test_case_lists_cover_what_the_issue_sets():
    assert len(set(IDS)) == len(IDS)
    sel = lambda cases, k: [p for p, kk in cases if kk == k]
    # a. every M, N, K value on every selector that takes it; the corner at every K; both forms; the automatic choice once per problem
    for k in ALL_K:
        ps = sel(G.CASES_RAGGED, k)
        p8 = k in G.P8_KERNELS
        assert {p.M for p in ps} == {1, 72, 129, 257, 264, 520} and {p.form for p in ps} == set(G.FORMS_A)
        assert {p.N for p in ps} == ({8, 72, 136, 264} if p8 else {8, 72, 136, 264, 12, 132, 260})
        assert {p.K for p in ps} == ({128, 256, 384} if p8 else {64, 192, 320})
        assert {p.K for p in ps if p.M == 520 and p.N in (260, 264)} == {p.K for p in ps}
        assert all(p.N % 8 == 0 and p.K % 128 == 0 for p in ps) if p8 else all(p.N % 4 == 0 and p.K % 64 == 0 for p in ps)
    for cases in (G.CASES_RAGGED, G.CASES_FORMS, G.CASES_LAYOUTS, G.CASES_MDEV):
        assert sorted(p.name for p in sel(cases, 0)) == sorted({p.name for p, k in cases if k != 0})
    assert G.FORMS["bf16-bias-R"] == dict(epi=G.EPI_BF16, bias=True, R=True) and G.FORMS["mul-cs"] == dict(epi=G.EPI_MUL, colsum=True)
    # b. every form on every selector at 520 x 264 x 256, N = 260 on the shared-epilogue kernels
    assert {(p.form, k) for p, k in G.CASES_FORMS if p.N == 264 and k} == {(f, k) for f in G.FORMS_B for k in ALL_K}
    assert {(p.form, k) for p, k in G.CASES_FORMS if p.N == 260 and k} == {(f, k) for f in G.FORMS_B for k in G.SHARED_KERNELS}
    assert all((p.M, p.K) == (520, 256) for p, _ in G.CASES_FORMS)
    f = G.FORMS
    assert f["bf16-full"] == dict(epi=G.EPI_BF16, bias=True, alpha=0.5, div=0.07, R=True, colsum=True) and f["bf16"] == dict(epi=G.EPI_BF16)
    assert f["gelu-c2"]["C2"] and "C2" not in f["gelu"] and f["deriv"]["C2"] and f["grad-cs"]["colsum"] and f["mul-bias"]["bias"]
    assert f["mul-alpha-cs"] == dict(epi=G.EPI_MUL, alpha=0.5, colsum=True)
    # c, d, f
    assert {(p.layout, k) for p, k in G.CASES_LAYOUTS if k} == {(lay, k) for lay in G.LAYOUTS for k in ALL_K}
    assert {(p.form, p.M, k) for p, k in G.CASES_MDEV if k and p.M_launch == 700} == {(f, m, k) for f in G.FORMS_B for m in (1, 300, 700) for k in ALL_K}
    assert {k for p, k in G.CASES_MDEV if (p.M, p.M_launch) == (264, 520)} == set(ALL_K) | {0}
    assert {k for _, k in G.CASES_ACCUM} == {3, 8} and all(p.launches == 2 and p.colsum for p, _ in G.CASES_ACCUM)
    # e. 256 CUs: 17 x 17 = 289 tiles, not a multiple of 8, between one and two grid rounds; the two device-side regimes
    assert G.persistent_shape(256) == (17, 4104) and G.persistent_shape(304) == (19, 4616)
    pc = G.persistent_cases(256)
    assert [(p.form, p.K) for p in pc if p.M_launch is None] == G.PERSISTENT_FORMS and all(p.N == 4104 and p.rows == 4104 for p in pc)
    tiles = sorted(-(-p.M // 256) * 17 for p in pc if p.M_launch)
    assert tiles == [255, 272] and all(p.M % 256 == 8 for p in pc)


def test_operand_views_have_the_strides_the_cases_are_about():
    for lay in G.LAYOUTS:
        p = next(q for q, _ in G.CASES_LAYOUTS if q.layout == lay)
        x = G.bases(p)
        A, W, kw = G.operands(p, x)
        assert A.shape[0] == p.M and W.shape[0] == p.N and A.stride(1) == 1 and W.stride(1) == 1
        if lay == "cls":
            assert A.stride(0) == G.CLS_L * p.K and A.shape[1] == p.K and torch.equal(A[3], x["A"][0][3 * G.CLS_L])
        if lay == "wslice":
            assert W.stride(0) == 2 * p.K and W.storage_offset() == p.K and W.shape[1] == p.K
        if lay == "wrows":
            assert W.storage_offset() == G.WROWS_OFF * p.K and W.is_contiguous()
        if lay == "knarrow":
            assert kw["K"] == p.K and A.shape[1] == 2 * p.K and W.shape[1] == p.K + 64
        if lay == "cslice":
            C = G.c_view(G.initial_buffers(p)["C"][0], p)
            assert C.storage_offset() == G.C_OFF and C.stride(0) == G.C_OFF + p.N + 8
    p = next(q for q, _ in G.CASES_MDEV if q.M == 300 and q.form == "mul-alpha-cs")
    A, W, kw = G.operands(p, G.bases(p))
    for t in (A, kw["G"], G.bases(p)["R"]):
        assert t.shape[0] == 700 and bool(torch.isnan(t[300:].float()).all()) and bool(torch.isfinite(t[:300].float()).all())
    for q in G.PROBLEMS:                 # 16-B aligned rows everywhere, strides of their own
        b = G.initial_buffers(q)
        assert b["C"][0].shape[1] % 8 == 0 and b["C"][0].shape == (q.rows + G.PAD_ROWS, q.c_off + G.ceil8(q.N) + 8)
        assert len({G.bases(q)["R"].shape[1], G.bases(q)["G"].shape[1], b["C"][0].shape[1], G.ceil8(q.N) + 16}) == 4
        assert not q.C2 or b["C2"][0].shape[1] == G.ceil8(q.N) + 16
        assert not q.colsum or bool((b["colsum"].abs() > 0).all())


def test_ref_is_the_documented_formula():
    """ref() in float64 against torch's own erf-GELU and its derivative by autograd."""
    for form in G.FORMS_B:
        p = G.Problem(129, 72, 192, form)
        A, W, kw = G.operands(p, G.bases(p))
        pre = p.alpha * (A.double() @ W.double().t())
        pre = (pre / kw["div"].double() if p.div else pre) + (kw["bias"].double() if p.bias else 0)
        xg = (kw["G"].double() if p.epi == G.EPI_GELU_GRAD else pre).clone().requires_grad_(True)
        dg, = torch.autograd.grad(F.gelu(xg).sum(), xg)
        want = {G.EPI_BF16: (pre + kw["R"].double() if p.R else pre, None), G.EPI_GELU: (F.gelu(pre), pre), G.EPI_GELU_DERIV: (F.gelu(pre), dg),
                G.EPI_GELU_GRAD: (pre * dg, None), G.EPI_MUL: (pre * kw["G"].double() if p.has_G else None, None)}[p.epi]
        got = G.ref(p, torch.float64)
        assert torch.allclose(got["pre"], pre, rtol=1e-13, atol=1e-13) and torch.allclose(got["C"], want[0], rtol=1e-12, atol=1e-13)
        assert (got["C2"] is None) == (want[1] is None) and (want[1] is None or torch.allclose(got["C2"], want[1], rtol=1e-12, atol=1e-13))
        assert (got["colsum"] is not None) == p.colsum and (not p.colsum or torch.allclose(got["colsum"], want[0].sum(0), rtol=1e-12))


def test_model_uses_the_erf_of_the_kernels():
    x = torch.linspace(-6, 6, 4001)
    assert (G.fast_erf(x.double()) - torch.erf(x.double())).abs().max().item() <= G.ERF_ERR        # the formula and its stated error
    assert (G.fast_erf(x).double() - torch.erf(x.double())).abs().max().item() <= G.ERF_ERR + 4 * 2.0 ** -23   # + its fp32 evaluation
    g, d = G.fast_gelu_both(x)
    assert torch.allclose(g, G.fast_gelu(x), atol=1e-6) and torch.allclose(d, G.fast_dgelu(x), atol=1e-6)
    assert (d.double() - G.dgelu(x.double())).abs().max().item() < 5e-7
    t = torch.tensor([1.00390625, -1.00390625, 1.0078125])                                         # 1 + 2^-8: a tie; 1 + 2^-7: exact
    assert G.truncate_bf16(t).tolist() == [1.0, -1.0, 1.0078125] and t.to(G.BF).tolist() == [1.0, -1.0, 1.0078125]
    assert G.truncate_bf16(torch.tensor([1.0077])).item() == 1.0 and torch.tensor([1.0077]).to(G.BF).item() == 1.0078125


@pytest.mark.parametrize("p", G.PROBLEMS, ids=IDS)
def test_model_passes_and_every_seeded_defect_fails(p):
    ratio = G.check_output(f"{p.name} model", G.model(p), p)
    assert ratio <= 1.0
    kinds = G.applicable_defects(p)
    assert {"truncated_store", "k_tile_missing", "chunk_past_N", "row_past_M"} <= set(kinds)
    assert ("colsum_unrounded" in kinds) == p.colsum and ("C_and_C2_exchanged" in kinds) == p.C2
    assert ("operand_row_off" in kinds) == ((p.R or p.has_G) and p.M > 1) and ("R_skips_last_chunk" in kinds) == p.R
    assert ("colsum_past_M_dev" in kinds) == (p.colsum and p.M_launch is not None)
    assert ("tiles_exchanged" in kinds) == (p.M > 128 or p.N > 128)
    for kind in kinds:
        with pytest.raises(AssertionError):
            G.check_output(f"{p.name} {kind}", G.defective(p, kind), p)
    out = G.model(p)                                          # one sentinel overwritten, in the padding right of the last row
    out["C"][-1][p.rows + G.PAD_ROWS - 1, -1] = 0.0
    with pytest.raises(AssertionError):
        G.check_output(f"{p.name} sentinel", out, p)


@pytest.mark.parametrize("p", [q for q in G.persistent_cases(256) if q.K == 128], ids=lambda q: q.name)
def test_model_passes_at_the_289_tile_shape(p):
    assert G.check_output(f"{p.name} model", G.model(p), p) <= 1.0
    G._acc.cache_clear()                 # (the 4104 x 4104 products of this shape: not kept for the rest of the session)
    G._bases.cache_clear()
