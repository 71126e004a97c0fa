"""tests/gemm_tn_reference.py checked on the CPU, at every problem tests/test_gemm_tn_edges_gpu.py runs: the float32 evaluation of the
reference passes the project's rule (helpers_gpu.check_ref) against the float64 one, and the output of a kernel with any one of the seeded
defects does not -- so the GPU tests cannot pass a kernel that drops or doubles a reduction row at a slice, step or remainder boundary,
reads a row past the device-side count, loses or doubles a slab, scales or overwrites C0, leaks its column clamp into stored outputs,
transposes the tile or writes outside [N, K].  The slicing table of the case list is re-derived here from the launcher's rule."""
import pytest
import torch

import gemm_tn_reference as G

PROBLEMS = list(dict.fromkeys(G.ALL_CASES))
IDS = [p.name for p in PROBLEMS]


def test_ref_is_the_documented_formula():
    """ref() against a hand-written triple loop in Python floats (130 rows: two whole 64-row blocks and a ragged one)."""
    A, B, C0 = G.rnd(130, 3, seed=1), G.rnd(130, 4, seed=2), G.rnd(3, 4, seed=3, dtype=torch.float32)
    got = G.ref(A, B, C0, -2.0, torch.float64)
    got32 = G.ref(A, B, C0, -2.0, torch.float32)
    assert got.dtype == torch.float64 and got32.dtype == torch.float32
    for n in range(3):
        for k in range(4):
            want = float(C0[n, k])
            for m in range(130):
                want += -2.0 * float(A[m, n]) * float(B[m, k])
            assert abs(got[n, k].item() - want) <= 1e-12 * max(1.0, abs(want))
            assert abs(got32[n, k].item() - want) <= 1e-4 * max(1.0, abs(want))
    assert torch.equal(G.ref(A[:0], B[:0], C0, 0.5, torch.float32), C0)                 # no rows: C0 bit for bit


def test_slicing_table_is_what_the_launcher_derives():
    """(ns, rlast, ndup) of every row of the table from the rule in include/spmm_hip.h, written out again here; and the rule itself cuts
    [0, M) into slices that cover every row exactly once, each an even number (>= 2) of 64-row steps that stays inside [0, M)."""
    assert len(G.SLICING_TABLE) == 17
    for (M, splits, ns, rlast, ndup) in G.SLICING_TABLE:
        rs = -(-(-(-M // 128)) // splits) * 128
        n = -(-M // rs)
        over = n * rs - M
        want = (1, M // 128 * 128, 0) if n == 1 else (n, rs - over // 128 * 128, over % 128)
        assert (ns, rlast, ndup) == want == G.slicing8(M, splits)[:3], (M, splits)
    for M in range(128, 1500):
        for splits in range(1, 12):
            ns, rlast, ndup, rs = G.slicing8(M, splits)
            assert 1 <= ns <= splits and rlast % 128 == 0 and rlast >= 128 and 0 <= ndup < 128
            if ns == 1:
                assert ndup == 0 and M - rlast == M % 128
                continue
            end = 0                                                     # rows [0, end) are covered exactly once so far
            for z in range(ns):
                beg, rows, skip = (z * rs, rs, 0) if z < ns - 1 else (M - rlast, rlast, ndup)
                assert beg >= 0 and beg + rows <= M and rows % 128 == 0 and rows >= 128 and beg + skip == end, (M, splits, z)
                end = beg + rows
            assert end == M, (M, splits)
            assert G._cut8(M, splits) == [(z * rs, (z + 1) * rs) for z in range(ns - 1)] + [(M - rlast + ndup, M)]


def test_case_lists_are_the_ones_the_issue_sets():
    assert len(set(IDS)) == len(IDS)
    assert all(p.kernel == 8 and p.M >= 128 and (p.N, p.K, p.alpha) == (256, 256, 0.5) for p in G.CASES_SLICING)
    assert len(G.CASES_COLUMNS) == 15 and {p.alpha for p in G.CASES_COLUMNS} == {1.0, -2.0}
    tiles = lambda p: -(-p.N // 256) * -(-p.K // 256)
    Gs = {tiles(p) * G.slicing8(p.M, p.splits)[0] for p in G.CASES_COLUMNS}
    assert {1, 2, 3, 5, 6, 12, 15, 30} <= Gs and any(g % 8 for g in Gs) and min(Gs) < 8 < max(Gs)
    assert len(G.CASES_COUNT_SPLIT) == 40 and all(p.plan[:2] == (8, 3) and len(p.plan[2]) == 3 for p in G.CASES_COUNT_SPLIT)
    assert all(p.plan[:2] == (1, 0) for p in G.CASES_COUNT_SINGLE + G.CASES_COUNT_SHORT)     # both go to the 128x128 kernel, one slice
    assert all(p.rows == 256 and p.M == 200 for p in G.CASES_COUNT_SHORT)
    # the 128x128 kernel: 7 row counts x 4 shapes, every distinct slicing of splits 1..3 once
    assert {(p.M, p.N, p.K) for p in G.CASES_K1} == {(M, N, K) for M in G.K1_ROWS for (N, K) in G.K1_SHAPES}
    per_M = {M: sorted(p.splits for p in G.CASES_K1 if p.M == M and p.N == 4) for M in G.K1_ROWS}
    assert per_M == {1: [1], 63: [1], 64: [1], 65: [1, 2], 127: [1, 2], 130: [1, 2, 3], 1000: [1, 2, 3]}
    assert G.K1_COUNT_BASE in G.CASES_K1 and G.K1_COUNT_BASE.plan == (1, 3, [(0, 384), (384, 768), (768, 1000)])
    assert [p.plan[2] for p in G.CASES_K1_COUNT][3] == [(0, 64), (64, 64), (64, 64)]          # later slices empty: zero slabs
    # every slice list partitions [0, meff)
    for p in PROBLEMS:
        cuts = p.plan[2]
        assert cuts[0][0] == 0 and cuts[-1][1] == p.meff and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])), p.name
    # alignment rules of the entry point hold for every buffer; no case is near the 32-bit operand-offset limit
    for p in PROBLEMS:
        assert p.N % 4 == 0 and p.K % 4 == 0 and p.ldc % 4 == 0 and p.lda % 8 == 0 and p.ldb % 8 == 0
        assert p.kernel != 8 or (p.N % 8 == 0 and p.K % 8 == 0)
        assert p.rows * max(p.lda, p.ldb) * 2 < 2 ** 31


def test_buffers_are_what_the_cases_are_about():
    p = G.Problem(200, 256, 256, splits=2, count=100, rows_buf=256)
    A, B, C = G.operand_buffers(p)
    assert tuple(A.shape) == (256, 272) and tuple(B.shape) == (256, 264) and tuple(C.shape) == (259, 268)
    for X, n in ((A, 256), (B, 256)):
        assert bool(torch.isfinite(X[:100, :n].float()).all()) and bool(torch.isnan(X[100:].float()).all()) and bool(torch.isnan(X[:, n:].float()).all())
    assert bool((C[256:] == G.SENTINEL).all()) and bool((C[:, 256:] == G.SENTINEL).all()) and torch.equal(C[:256, :256], G.bases(p)[2])
    assert bool(torch.isfinite(G.bases(p)[0][:, :256].float()).all())                         # (the bases stay finite: row_past_count reads them)
    q = G.Problem(130, 300, 132, kernel=1)
    A, B, _ = G.operand_buffers(q)
    assert (A.shape[1], B.shape[1]) == (320, 144) and bool(torch.isnan(A[:, 300:].float()).all()) and bool(torch.isfinite(A[:, :300].float()).all())


@pytest.mark.parametrize("p", PROBLEMS, ids=IDS)
def test_fp32_reference_passes_and_every_seeded_defect_fails(p):
    ref64, ref32 = G.reference(p)
    buf = G.initial_buffer(p)
    buf[:p.N, :p.K] = ref32
    G.check_output(f"{p.name} fp32 reference", buf, p)
    G.check_output(f"{p.name} fp32, no defect", G.defective(p, None), p)
    kinds = G.applicable_defects(p)
    assert {"overwritten", "pad_column_written", "row_N_written"} <= set(kinds)
    assert len([k for k in kinds if k.startswith("row_dropped")]) == len(G.defect_rows(p.meff)) >= min(p.meff, 1)
    assert ("row_past_count" in kinds) == (p.count is not None and p.count < p.rows)
    assert ("slab_missing" in kinds) == (p.plan[1] > 1 and p.meff > 0) and ("transposed" in kinds) == (p.N == p.K and p.meff > 0)
    for kind in kinds:
        with pytest.raises(AssertionError):
            G.check_output(f"{p.name} {kind}", G.defective(p, kind), p)
