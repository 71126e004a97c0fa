"""Every launch path of the weight-gradient GEMM spmm_gemm_tn (spmm_amd/csrc/gemm_tn.hip: tn_run, the 8-phase body, the 128x128 kernel, the
slab reduce) at the smallest shapes at which the path exists, against the float64 reference of tests/gemm_tn_reference.py under
helpers_gpu.check_ref (bound = max(8 E32, 4 fp32 ulp), from the fp32 evaluation of the reference alone; the `[tol]` line each check prints
is the record of the measured error).  The case lists, and the reason these checks cannot pass a subtly wrong kernel, are in the reference
module and tests/test_gemm_tn_reference_cpu.py.

The entry point is called directly with a workspace of the test's own.  Around every launch:
  * C is a view of a larger buffer full of a sentinel, A and B are column views of wider buffers with NaN in the padding columns and in
    every row past the rows to reduce: C must come out finite, and every element outside the view must keep the sentinel's bits;
  * the workspace is filled with NaN and followed by 64 sentinel floats: slabs are written before they are read, slices left without rows
    write zeros, nothing is written past spmm_gemm_tn_workspace_bytes;
  * every case runs twice into fresh buffers and the two results are torch.equal: no atomics, and a missing wait shows as a flicker.

Measured on an MI355X, the case of each family with the least margin (kernel error / bound; full listing: profiles/gemm_tn_edges_tol.txt):
  a. row slicing           k8-257x256x256-s2-a0.5             E32=3.517e-06 kernel=6.555e-06 bound=2.813e-05   (0.23)
  b. column shapes         k8-320x264x520-s2-a1               E32=9.596e-06 kernel=1.798e-05 bound=7.677e-05   (0.23)
  c. count, re-cut         k8-641x256x256-s4-a0.5-count385    E32=5.171e-06 kernel=7.942e-06 bound=4.137e-05   (0.19)
  c. count, 128x128 route  k8-641x256x256-s1-a0.5-count641    E32=8.618e-06 kernel=2.148e-05 bound=6.895e-05   (0.31)
  d. 128x128 kernel        k1-1000x4x4-s1-a0.5                E32=2.757e-06 kernel=1.000e-05 bound=2.205e-05   (0.45)
  d. 128x128, count        k1-1000x300x132-s3-a0.5-count333   E32=4.977e-06 kernel=1.132e-05 bound=3.982e-05   (0.28)
The single-slice launches of the 128x128 kernel sit highest: one workgroup adds all 1000 rows into one fp32 accumulator."""
import ctypes

import pytest
import torch

import gemm_tn_reference as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd._lib import lib
    return lib()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def launch(L, A, B, C, M, N, K, splits, alpha, kernel, count=None):
    """One spmm_gemm_tn call on the current stream with a NaN-filled workspace of exactly the documented size + WS_GUARD sentinel floats;
    asserts the guard afterwards."""
    nws = L.cdll.spmm_gemm_tn_workspace_bytes(M, N, K, splits)
    assert nws == (splits * N * K * 4 if splits > 1 else 0)
    ws = torch.full((nws // 4 + G.WS_GUARD,), G.SENTINEL, dtype=torch.float32, device="cuda")
    ws[:nws // 4] = G.NAN
    md = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    assert A.stride(1) == 1 and B.stride(1) == 1 and C.stride(1) == 1 and tuple(C.shape) == (N, K)
    L.call("spmm_gemm_tn", _ptr(A), A.stride(0), _ptr(B), B.stride(0), M, N, K, splits, float(alpha), _ptr(C), C.stride(0), _ptr(ws), kernel,
           None if md is None else _ptr(md), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    guard = ws[nws // 4:].cpu()
    assert bool((guard.view(torch.int32) == torch.tensor(G.SENTINEL, dtype=torch.float32).view(torch.int32)).all()), "written past the workspace"


def run_once(L, p):
    Ab, Bb, Cb = (t.cuda() for t in G.operand_buffers(p))
    A, B, C = Ab[:p.M, :p.N], Bb[:p.M, :p.K], Cb[:p.N, :p.K]
    assert (A.stride(0), B.stride(0), C.stride(0)) == (p.lda, p.ldb, p.ldc) and Ab.shape[0] == p.rows
    launch(L, A, B, C, p.M, p.N, p.K, p.splits, p.alpha, p.kernel, p.count)
    return Cb.cpu()


def run_case(L, p):
    """Problem p twice into fresh buffers: both padded buffers equal bit for bit, and the rule of check_output -> the buffer (CPU)."""
    buf, again = run_once(L, p), run_once(L, p)
    G.check_output(p.name, buf, p)
    assert torch.equal(buf, again), f"{p.name}: two runs differ in {int((buf != again).sum())} elements"
    return buf


@pytest.mark.parametrize("p", G.CASES_SLICING, ids=G.case_id)
def test_row_slicing_of_the_8_phase_kernel(L, p):
    """a. One slice accumulated into C (M % 128 == 0), one slice + the 128x128 remainder pass (1 and 127 rows), several slices into slabs +
    the reduce: the last slice moved back to end at row M with 1 .. 127 overlap rows zeroed in LDS (TP_MASK(0) alone up to 64, TP_MASK(1)
    past it), whole 128-row pairs dropped, fewer slices than asked.  N = K = 256, alpha = 0.5."""
    run_case(L, p)


@pytest.mark.parametrize("p", G.CASES_COLUMNS, ids=G.case_id)
def test_column_shapes_of_the_8_phase_kernel(L, p):
    """b. One 8-column tile; full tiles followed by an 8-column ragged tile in N, in K and in both (the clamp of ca / cb, the guards of the
    stores); three tiles: with 1, 2 and 5 slices the XCD-contiguous remap runs at G = 1 .. 30 workgroups, G % 8 != 0 and G < 8 included.
    alpha = 1.0 / -2.0."""
    run_case(L, p)


@pytest.mark.parametrize("p", G.CASES_COUNT_SPLIT, ids=G.case_id)
def test_device_side_row_count_recut_on_the_8_phase_kernel(L, p):
    """c. Sized for 641 rows in 3 slices (splits = 4), *M_dev from -3 to 700: the slices re-cut on the device, counts below 256 masked in
    both operands (TP_MASK_TAIL), slices left empty writing zero slabs; NaN in every row past the count.  A count <= 0 leaves C0 bit for
    bit; a count >= M equals the launch without a count bit for bit."""
    buf = run_case(L, p)
    if p.count <= 0:
        assert torch.equal(buf, G.initial_buffer(p))
    if p.count >= p.M:
        assert torch.equal(buf, run_once(L, G.Problem(p.M, p.N, p.K, splits=p.splits, kernel=p.kernel, alpha=p.alpha)))


@pytest.mark.parametrize("p", G.CASES_COUNT_SINGLE + G.CASES_COUNT_SHORT, ids=G.case_id)
def test_device_side_row_count_routed_to_the_128x128_kernel(L, p):
    """c. A single slice, and M = 200 < 256 at splits = 2 (operands = the first 200 rows of 256-row buffers whose other rows hold NaN),
    under a device-side count: both run on the 128x128 kernel, which reads no row past the count."""
    buf = run_case(L, p)
    if p.count <= 0:
        assert torch.equal(buf, G.initial_buffer(p))


@pytest.mark.parametrize("p", G.CASES_K1, ids=G.case_id)
def test_the_128x128_kernel(L, p):
    """d. One row; one short of, exactly and one past a 64-row step (the register-staged ragged last step); N % 8 == 4 (N = 4, 300, 132);
    one, two and three grid.z slices into slabs."""
    run_case(L, p)


@pytest.mark.parametrize("p", G.CASES_K1_COUNT, ids=G.case_id)
def test_device_side_row_count_on_the_128x128_kernel(L, p):
    """d. Three grid.z slices of 384 rows under *M_dev from -1 to 1200: slices past the count write zero slabs."""
    buf = run_case(L, p)
    if p.count <= 0:
        assert torch.equal(buf, G.initial_buffer(p))
    if p.count >= p.M:
        assert torch.equal(buf, run_once(L, G.K1_COUNT_BASE))


@pytest.mark.parametrize("shape,forced", G.CASES_AUTO, ids=[f"{s[0]}x{s[1]}x{s[2]}-is-k{k}" for s, k in G.CASES_AUTO])
def test_automatic_choice_either_side_of_the_threshold(L, shape, forced):
    """e. kernel = 0 at 4096 and 16384 rows x 768 x 768 (tn_pick's M x tiles threshold lies between): bit for bit the forced kernel the
    threshold names, at the split count spmm_gemm_tn_splits gives the automatic choice."""
    M, N, K = shape
    splits = L.cdll.spmm_gemm_tn_splits(M, N, K, 0)
    assert splits == L.cdll.spmm_gemm_tn_splits(M, N, K, forced) > 1
    A, B = G.rnd(M, N, seed=16).cuda(), G.rnd(M, K, scale=0.5, seed=17).cuda()
    C0 = G.rnd(N, K, seed=18, dtype=torch.float32).cuda()
    out = []
    for kernel in (0, forced):
        C = C0.clone()
        launch(L, A, B, C, M, N, K, splits, 1.0, kernel)
        out.append(C)
    assert torch.equal(out[0], out[1]) and bool(torch.isfinite(out[0]).all()) and not torch.equal(out[0], C0)
    # (Measured on an MI355X: at these two shapes and split counts the OTHER forced kernel gives the same bits too -- both reduce the same
    # row slices in row order.  This pins the result of the automatic choice; which kernel ran is tn_pick's business.)
