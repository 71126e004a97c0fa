"""The bf16-output epilogues of spmm_gemm_nt (SPMM_EPI_BF16, _GELU, _GELU_DERIV, _GELU_GRAD, _MUL) on every launch form that builds them -- the
128x128 kernel (selector 1), its loader + compute wave variant (5), the 256x128 ring kernel (2), the 256x256 one-barrier kernel (3), the
256x256 8-phase kernel launched persistently (8) and with one workgroup per tile (9), and the automatic choice (0) -- against the float64
reference of tests/gemm_bf16_reference.py under its per-element bound: the fp32 part from the float32 evaluation of the reference, half a
bf16 ulp at each point where the kernels round, the stated error of the erf formula; no fixed tolerance.  Every output is a view of a
larger buffer full of a sentinel, every element outside the view must keep the sentinel's bits, and the fused column sums are checked
against the float64 sums of the C the kernel itself stored.  The `[tol]` line of each check is the record of the measured error
(profiles/gemm_bf16_epilogues_tol.txt holds one run's).  The case lists, and the reason these checks cannot pass a subtly wrong kernel,
are in the reference module and tests/test_gemm_bf16_reference_cpu.py."""
import pytest
import torch

import gemm_bf16_reference as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops as o
    return o


def run_case(ops, p, kernel, keep_on_device=False):
    """The launches of problem p on `kernel` into the padded sentinel buffers -> the buffers (on the CPU unless keep_on_device)."""
    x = G.bases(p, "cuda")
    out = G.initial_buffers(p, "cuda")
    md = torch.tensor([p.M], dtype=torch.int32, device="cuda") if p.M_launch else None
    for l in range(p.launches):
        A, W, kw = G.operands(p, x, l)
        C = G.c_view(out["C"][l], p)
        C2 = G.c2_view(out["C2"][l], p) if p.C2 else None
        assert A.shape[0] == p.rows and C.shape == (p.rows, p.N) and C.stride(0) == p.c_off + G.ceil8(p.N) + 8
        ops.gemm_nt(A, W, C, C2=C2, colsum=out["colsum"], kernel=kernel, M_dev=md, **kw)
    torch.cuda.synchronize()
    if keep_on_device:
        return out
    return {k: [t.cpu() for t in v] if isinstance(v, list) else (None if v is None else v.cpu()) for k, v in out.items()}


def check_case(ops, case):
    p, kernel = case
    G.check_output(G.case_id(case), run_case(ops, p, kernel), p)


@pytest.mark.parametrize("case", G.CASES_RAGGED, ids=G.case_id)
def test_ragged_edges_on_every_kernel(ops, case):
    """a. One row; M % 16 == 8 (the 8-row store predicate of the 8-phase blocks); one row past each tile height; more than two tiles; N of
    one chunk, one chunk past a tile, the half chunk (N % 8 == 4) of the shared epilogue; the K-ring exactly full, its first restage, one
    to three K-tile pairs of the 8-phase kernel.  `+ bias + R`, and `* G` with column sums."""
    check_case(ops, case)


@pytest.mark.parametrize("case", G.CASES_FORMS, ids=G.case_id)
def test_every_epilogue_form_on_every_kernel(ops, case):
    """b. 520 x 264 (260) x 256: plain; bias + alpha + *div + R + column sums; GELU with and without its second output (the form the
    decoder launches); GELU with the derivative; GELU-grad and the multiply with column sums, alpha, bias."""
    check_case(ops, case)


@pytest.mark.parametrize("case", G.CASES_LAYOUTS, ids=G.case_id)
def test_operand_layouts_of_the_engine(ops, case):
    """c. A = the position-0 rows of a [B, L, H] batch, W = a column slice / a row slice of a wider matrix, K= narrower than A, C = a
    column slice of a wider buffer."""
    check_case(ops, case)


@pytest.mark.parametrize("case", G.CASES_MDEV, ids=G.case_id)
def test_device_side_row_count(ops, case):
    """d. Sized for 700 rows, *M_dev = 1, 300, 700 (264 of 520): NaN in the rows of A, R, G past *M_dev; the rows below it pass against the
    float64 reference, every other element keeps the sentinel, the column sums stay finite and hold the rows computed only."""
    check_case(ops, case)


@pytest.mark.parametrize("case", G.CASES_ACCUM, ids=G.case_id)
def test_column_sums_accumulate_over_launches(ops, case):
    """f. Two launches with operands of their own add into one (random, non-zero) colsum vector."""
    check_case(ops, case)


N_PERSISTENT = len(G.persistent_cases(256))


@pytest.mark.parametrize("i", range(N_PERSISTENT), ids=[p.name.split("-", 1)[1] + f"-K{p.K}" for p in G.persistent_cases(256)])
def test_persistent_walk(ops, i):
    """e. s x s tiles, s the smallest odd number with s * s past the persistent grid (17 x 17 = 289 on 256 CUs: some workgroups walk two
    tiles, others one; the count is no multiple of 8), the last tile row and column ragged; K = 128 (tile order 2) and 1152 (order 0).
    The persistent launch (8) and the per-tile launch (9) each against float64 -- a wrong tile order, XCD remap or edge predicate is
    common to both and invisible to a comparison of the two -- and bit-identical to one another.  Two device-side row counts: tile count
    below the grid (some workgroups exit at once) and between one and two grid rounds.  (Reference evaluated on the device.)"""
    cases = G.persistent_cases(torch.cuda.get_device_properties(0).multi_processor_count)
    if i >= len(cases):                  # (a CU count that leaves no such device-side row count)
        return
    p = cases[i]
    outs = {}
    for kernel in G.P8_KERNELS:
        outs[kernel] = run_case(ops, p, kernel, keep_on_device=True)
        G.check_output(G.case_id((p, kernel)), outs[kernel], p, device="cuda")
    a, b = outs[G.K256P8], outs[G.K256P8_TILES]
    assert torch.equal(a["C"][0].view(torch.int16), b["C"][0].view(torch.int16))
    if p.C2:
        assert torch.equal(a["C2"][0].view(torch.int16), b["C2"][0].view(torch.int16))
    G._acc.cache_clear()                 # (the 4104 x 4104 float64 products of this shape: not kept for the rest of the session)
    G._bases.cache_clear()
