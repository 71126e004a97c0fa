"""The tile boundary of the persistent 8-phase NT GEMM (`gemm_nt_p8_kernel`): a workgroup that walks several tiles writes each
tile's epilogue between two K loops, with the two wave rows brought together for it.  The one-workgroup-per-tile launch (kernel 9)
runs the same tiles with the same accumulation order and a single boundary per workgroup, so the persistent launch (kernel 8) must
match it bit for bit on every epilogue, on shapes with several tiles per workgroup, ragged edges and a device-side row count."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops as o
    return o


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    g = torch.Generator(device="cuda").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype)


def close(got, ref, atol, rtol, name=""):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.numel()} off; max err {err.max().item():.4g}"


# (name, epilogue, extra operands): every bf16-output epilogue the training step launches on the 8-phase kernel
CASES = [("bf16", "EPI_BF16", dict(bias=True)),
         ("bf16_R", "EPI_BF16", dict(bias=True, R=True)),
         ("bf16_colsum", "EPI_BF16", dict(colsum=True)),
         ("gelu_deriv", "EPI_GELU_DERIV", dict(bias=True, C2=True)),
         ("mul_colsum", "EPI_MUL", dict(G=True, colsum=True)),
         ("gelu_grad", "EPI_GELU_GRAD", dict(G=True, colsum=True))]


def run_both(ops, A, W, M, N, epi_name, extra, seed, M_dev=None, rows=None):
    """The same GEMM through kernel 8 (persistent) and kernel 9 (one workgroup per tile); returns [(C, C2, colsum)] x 2."""
    rows = M if rows is None else rows
    bias = rnd(N, seed=seed + 1, dtype=torch.float32) if extra.get("bias") else None
    R = rnd(M, N, seed=seed + 2) if extra.get("R") else None
    G = rnd(M, N, seed=seed + 3) if extra.get("G") else None
    outs = []
    for kernel in (8, 9):
        C = torch.full((M, N), 7.0, dtype=BF, device="cuda")
        C2 = torch.full((M, N), 7.0, dtype=BF, device="cuda") if extra.get("C2") else None
        cs = torch.zeros(N, device="cuda") if extra.get("colsum") else None
        ops.gemm_nt(A[:rows], W, C[:rows], bias=bias, epi=getattr(ops, epi_name), R=None if R is None else R[:rows],
                    G=None if G is None else G[:rows], C2=None if C2 is None else C2[:rows], colsum=cs, kernel=kernel, M_dev=M_dev)
        outs.append((C, C2, cs))
    return outs, bias, R, G


def check_equal(outs, name, Mv):
    (C8, C28, cs8), (C9, C29, cs9) = outs
    assert torch.equal(C8, C9), f"{name}: persistent and per-tile launches differ"
    if C28 is not None:
        assert torch.equal(C28, C29), f"{name}: second output differs"
    if cs8 is not None:     # (float atomics: the order of the additions is not fixed)
        close(cs8, cs9, 2e-2 * math.sqrt(Mv) / 30, 1e-3, f"{name}: column sums")


@pytest.mark.parametrize("M,N,K", [(84256, 768, 768), (84256, 2304, 768), (84256, 3072, 768), (70000, 768, 3072), (70000, 3072, 768),
                                   (70001, 776, 768)])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_persistent_matches_per_tile_launch(ops, M, N, K, case):
    name, epi, extra = case
    A, W = rnd(M, K, seed=11), rnd(N, K, scale=0.05, seed=12)
    outs, _, _, _ = run_both(ops, A, W, M, N, epi, extra, seed=20)
    check_equal(outs, f"{name} {M}x{N}x{K}", M)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_side_row_count(ops, case):
    """The launch sized for M rows computes *M_dev < M of them: rows past *M_dev stay untouched, the rest match the per-tile launch."""
    name, epi, extra = case
    M, Md, N, K = 84256, 61111, 2304, 768
    A, W = rnd(M, K, seed=41), rnd(N, K, scale=0.05, seed=42)
    md = torch.tensor([Md], dtype=torch.int32, device="cuda")
    outs, _, _, _ = run_both(ops, A, W, M, N, epi, extra, seed=50, M_dev=md)
    check_equal(outs, f"{name} M_dev", Md)
    for C, C2, _ in outs:
        assert bool((C[Md:] == 7.0).all())
        if C2 is not None:
            assert bool((C2[Md:] == 7.0).all())


@pytest.mark.parametrize("M,N,K", [(70000, 768, 768), (30001, 3072, 768), (20000, 776, 3072)])
def test_persistent_against_fp32(ops, M, N, K):
    """Several tiles per workgroup against fp32 torch (the tolerances of the existing GEMM tests)."""
    A, W = rnd(M, K, seed=61), rnd(N, K, scale=0.05, seed=62)
    bias, R, G = rnd(N, seed=63, dtype=torch.float32), rnd(M, N, seed=64), rnd(M, N, seed=65)
    ref = A.float() @ W.float().t()
    C = torch.empty(M, N, dtype=BF, device="cuda")
    ops.gemm_nt(A, W, C, bias=bias, R=R, kernel=8)
    close(C, ref + bias + R.float(), 3e-2, 1e-2, "bias + residual")
    C2 = torch.empty(M, N, dtype=BF, device="cuda")
    ops.gemm_nt(A, W, C, bias=bias, epi=ops.EPI_GELU_DERIV, C2=C2, kernel=8)
    pre = (ref + bias).requires_grad_(True)
    torch.nn.functional.gelu(pre).sum().backward()
    close(C, torch.nn.functional.gelu(pre.detach()), 3e-2, 1e-2, "gelu")
    close(C2, pre.grad, 1e-2, 1e-2, "gelu'")
    cs = torch.zeros(N, device="cuda")
    D = torch.empty(M, N, dtype=BF, device="cuda")
    ops.gemm_nt(A, W, D, epi=ops.EPI_MUL, G=G, colsum=cs, kernel=8)
    close(D, ref * G.float(), 3e-2, 1.5e-2, "multiply")
    close(cs, D.float().sum(0), 5e-2 * math.sqrt(M / 256), 2e-3, "column sums")
