"""tests/gemm_f32_reference.py checked on the CPU, at every problem tests/test_gemm_f32_epilogues_gpu.py runs: the float32 evaluation of the
reference passes the project's rule (helpers_gpu.check_ref) against the float64 one, and the output of a kernel with any one of the
seeded defects does not -- so the GPU tests cannot pass a kernel that drops a K-tile or a K-slice, adds the bias or R once per slice,
leaves the ragged column group unwritten, writes a row past M, or forgets alpha or *div."""
import pytest
import torch

import gemm_f32_reference as G

IDS = [p.name for p in G.PROBLEMS]


def test_case_list_is_the_one_the_issue_sets():
    from spmm_amd import ops
    assert (G.EPI_BF16, G.EPI_F32, G.EPI_F32_ATOMIC, G.EPI_F32_ACC) == (ops.EPI_BF16, ops.EPI_F32, ops.EPI_F32_ATOMIC, ops.EPI_F32_ACC)
    assert len(set(IDS)) == len(IDS)
    assert len(G.CASES_RAGGED) == 6 * 11 and {k for _, k in G.CASES_RAGGED} == {0, 1, 2, 5}
    assert not any(k == 2 and p.epi == G.ATOMIC for p, k in G.ALL_CASES)            # (the 256x128 kernel has no atomic epilogue)
    assert not any(k == 2 and p.splits > 1 for p, k in G.ALL_CASES)
    # split-K slicing as spmm_gemm_nt does it: 3 + 2 tiles, one tile each, 7 clamped to 5, 16 x 256
    sl = {(p.K, p.splits): (p.ksplit, p.nslices) for p, _ in G.CASES_SPLITK}
    assert sl == {(320, 2): (192, 2), (320, 5): (64, 5), (320, 7): (64, 5), (4096, 16): (256, 16)}
    assert G.DFEAT.nslices == 16 and all(p.bias and p.c0 == "rand" for p, _ in G.CASES_SPLITK)
    # the padded buffer keeps the entry point's alignment rules
    assert all((p.N + G.PAD_COLS) % 4 == 0 and p.N % 4 == 0 and p.K % 64 == 0 for p in G.PROBLEMS)


def test_operand_views_have_the_strides_the_cases_are_about():
    for lay in ("cls", "wslice", "knarrow"):
        p = next(q for q, _ in G.CASES_STRIDED if q.layout == lay)
        A, W, kw = G.operands(p, G.bases(p))
        assert A.shape[0] == p.M and W.shape[0] == p.N and A.stride(1) == 1 and W.stride(1) == 1
        if lay == "cls":
            assert A.stride(0) == G.CLS_L * p.K and A.shape[1] == p.K and torch.equal(A[3], G.bases(p)["A"][0][3 * G.CLS_L])
        if lay == "wslice":
            assert W.stride(0) == 3 * p.K and W.storage_offset() == p.K and W.shape[1] == p.K
        if lay == "knarrow":
            assert kw["K"] == p.K and A.shape[1] == 2 * p.K and W.shape[1] == p.K + 64
    p = G.CASES_MDEV[0][0]
    A = G.operands(p, G.bases(p))[0]
    assert A.shape[0] == 700 and bool(torch.isnan(A[300:].float()).all()) and bool(torch.isfinite(A[:300].float()).all())
    assert G.initial_buffer(p).shape == (703, 144) and bool((G.initial_buffer(p)[300:] == G.SENTINEL).all())


def test_ref_is_the_documented_formula():
    """ref() against the formula written out element by element in Python floats (a small case)."""
    A, W = G.rnd(3, 64, seed=1), G.rnd(4, 64, seed=2)
    bias, C0, R = G.rnd(4, seed=3, dtype=torch.float32), G.rnd(3, 4, seed=4, dtype=torch.float32), G.rnd(3, 4, seed=5)
    div = torch.tensor([0.07], dtype=torch.float32)
    for epi in (G.F32, G.ACC, G.ATOMIC):
        got = G.ref(A, W, bias=bias, alpha=0.5, div=div, R=R, C0=C0, epi=epi, dtype=torch.float64)
        for m in range(3):
            for n in range(4):
                acc = sum(float(A[m, k]) * float(W[n, k]) for k in range(64))
                want = 0.5 * acc / float(div) + float(bias[n]) + float(R[m, n]) + (0.0 if epi == G.F32 else float(C0[m, n]))
                assert abs(got[m, n].item() - want) <= 1e-12 * max(1.0, abs(want))


@pytest.mark.parametrize("p", G.PROBLEMS, ids=IDS)
def test_fp32_reference_passes_and_every_seeded_defect_fails(p):
    ref64, ref32 = G.reference(p)
    buf = G.initial_buffer(p)
    buf[:p.M, :p.N] = ref32
    G.check_output(f"{p.name} fp32 reference", buf, p)
    G.check_output(f"{p.name} fp32, slice by slice", G.defective(None, p), p)     # another summation order stays inside the bound
    kinds = G.applicable_defects(p)
    assert {"k_tile_dropped", "ragged_cols_unwritten", "row_past_M_written"} <= set(kinds)
    assert ("R_per_slice" in kinds) == (p.R and p.nslices > 1) and ("bias_per_slice" in kinds) == (p.bias and p.nslices > 1)
    for kind in kinds:
        with pytest.raises(AssertionError):
            G.check_output(f"{p.name} {kind}", G.defective(kind, p), p)
