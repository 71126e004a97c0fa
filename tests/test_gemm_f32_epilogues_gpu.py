"""The fp32-output epilogues of spmm_gemm_nt (SPMM_EPI_F32, _F32_ACC, _F32_ATOMIC) on every kernel that builds them -- the 128x128 kernel
(selector 1), its loader + compute wave variant (5), the 256x128 ring kernel (2, an epilogue of its own) and the automatic choice (0) --
against the float64 reference of tests/gemm_f32_reference.py under helpers_gpu.check_ref (bound = max(8 E32, 4 fp32 ulp), from the fp32
evaluation of the reference alone; the `[tol]` line each check prints is the record of the measured error).  Every output is a view of a
larger buffer full of a sentinel, and every element outside the view must keep the sentinel's bits.  The case list and the reason these
checks cannot pass a subtly wrong kernel are in the reference module and tests/test_gemm_f32_reference_cpu.py.

Also here: the K-ring edges (nk = 1, 3, 4, 5 K-tiles) of the bf16 epilogue on the ring kernels, and the device-side row count on the
bf16 epilogue of the 256x128 and 256x256 kernels."""
import pytest
import torch

import gemm_f32_reference as G

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def rnd(*shape, **kw):
    return G.rnd(*shape, **kw).cuda()


def close(got, ref, atol, rtol, name=""):           # test_kernels_gpu.py::close
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.numel()} off; max err {err.max().item():.4g} " \
                          f"(ref max {ref.abs().max().item():.4g}) first bad idx {bad.nonzero()[0].tolist()}"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops as o
    return o


def run_case(ops, p, kernel):
    """The launches of problem p on `kernel`, into the padded sentinel buffer -> the buffer on the CPU."""
    x = G.to_device(G.bases(p), "cuda")
    buf = G.initial_buffer(p).cuda()
    C = buf[:p.rows, :p.N]
    md = torch.tensor([p.M], dtype=torch.int32, device="cuda") if p.M_launch else None
    for l in range(p.launches):
        A, W, kw = G.operands(p, x, l)
        assert A.shape[0] == p.rows and C.stride(0) == p.N + G.PAD_COLS
        ops.gemm_nt(A, W, C, kernel=kernel, M_dev=md, **kw)
    torch.cuda.synchronize()
    return buf.cpu()


def check_case(ops, case):
    p, kernel = case
    G.check_output(G.case_id(case), run_case(ops, p, kernel), p)


@pytest.mark.parametrize("case", G.CASES_RAGGED, ids=G.case_id)
def test_ragged_shapes_on_every_kernel(ops, case):
    """a. One row; N = 44 / 132 / 300 (N % 8 == 4: the last 4-column group), M one past / one short of a tile, several tiles both ways,
    nk = 1 .. 12 K-tiles; bias, alpha = 0.5 and a device scalar div together."""
    check_case(ops, case)


@pytest.mark.parametrize("case", G.CASES_R, ids=G.case_id)
def test_R_is_added_exactly_once(ops, case):
    """b. include/spmm_hip.h: the fp32 epilogues add bias and R once per element, whatever `splits` is (five K-slices here)."""
    check_case(ops, case)


@pytest.mark.parametrize("case", G.CASES_STRIDED, ids=G.case_id)
def test_strided_operands(ops, case):
    """c. A = the position-0 rows of a [B, L, H] batch (row stride L * H), W = a column slice of a wider matrix, K= narrower than A."""
    check_case(ops, case)


@pytest.mark.parametrize("case", G.CASES_SPLITK, ids=G.case_id)
def test_split_k_slices_and_bias_once(ops, case):
    """d. K = 320 in slices of 3 + 2 tiles, of one tile each, with a split count past K / 64; K = 4096 sixteen ways (the step's rule);
    bias once, on a non-zero C."""
    check_case(ops, case)


@pytest.mark.parametrize("case", G.CASES_SITES, ids=G.case_id)
def test_the_four_call_sites(ops, case):
    """e. LM-head logits (M >= 6000: the 256x128 kernel, also forced; M = 5000), the similarity matrices, dfeat (two 16-way split atomic
    launches into one zeroed buffer), the K/V data gradients (two accumulating launches into one buffer)."""
    check_case(ops, case)


@pytest.mark.parametrize("case", G.CASES_MDEV, ids=G.case_id)
def test_device_side_row_count_fp32(ops, case):
    """f. Sized for 700 rows, *M_dev = 300, NaN in A's rows [300, 700): rows below 300 pass, every other element keeps the sentinel."""
    check_case(ops, case)


@pytest.mark.parametrize("kernel", [2, 3])
def test_device_side_row_count_bf16_on_the_256_row_kernels(ops, kernel):
    """f. The check of test_kernels_gpu.py::test_device_side_row_counts at the same shape on the 256x128 and 256x256 kernels."""
    M, N, K, Md = 700, 132, 128, 300
    md = torch.tensor([Md], dtype=torch.int32, device="cuda")
    A, W, R = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05), rnd(M, 136, seed=3)[:, :N]
    A[Md:] = float("nan"); R[Md:] = float("nan")
    bias = rnd(N, seed=4, dtype=torch.float32)
    outs = []
    for dyn in (True, False):
        rows = M if dyn else Md
        Cb = torch.full((M, 136), 7.0, dtype=BF, device="cuda")
        ops.gemm_nt(A[:rows], W, Cb[:rows, :N], bias=bias, R=R[:rows], kernel=kernel, M_dev=md if dyn else None)
        outs.append(Cb)
    assert torch.equal(outs[0][:Md], outs[1][:Md])
    assert bool((outs[0][Md:] == 7.0).all()) and bool((outs[0][:, N:] == 7.0).all())
    close(outs[0][:Md, :N], A[:Md].float() @ W.float().t() + bias + R[:Md].float(), 3e-2, 1e-2, f"kernel {kernel} under M_dev")


@pytest.mark.parametrize("K", [64, 192, 256, 320])
@pytest.mark.parametrize("kernel", [1, 2, 3, 5])
def test_k_ring_edges_bf16(ops, kernel, K):
    """g. nk = 1, 3 (the four-stage ring of kernel 5 exactly full), 4 and 5 (its first restage; the three-stage ring of kernel 2 restages
    from nk = 3 on) with the bf16 epilogue, bias and R: the tolerances of test_kernels_gpu.py::test_gemm_tile_kernels."""
    M, N = 257, 136
    A, W = rnd(M, K, seed=21), rnd(N, K, scale=0.05, seed=22)
    bias, R = rnd(N, seed=23, dtype=torch.float32), rnd(M, N + 8, seed=24)[:, :N]
    Cbuf = torch.full((M + 3, N + 8), 7.0, dtype=BF, device="cuda")
    ops.gemm_nt(A, W, Cbuf[:M, :N], bias=bias, R=R, kernel=kernel)
    close(Cbuf[:M, :N], A.float() @ W.float().t() + bias + R.float(), 3e-2, 1e-2, f"gemm kernel {kernel}, K = {K}")
    assert bool((Cbuf[:, N:] == 7.0).all()) and bool((Cbuf[M:] == 7.0).all())
