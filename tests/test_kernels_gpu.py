"""Per-kernel parity of the HIP kernels (through the C ABI) against plain fp32 PyTorch of the same op.
Inputs are asymmetric random data rounded to bf16 first, so the only differences are accumulation order and the
bf16 rounding of outputs; tolerances are stated per test."""
import math

import numpy as np

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
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def close(got, ref, atol, rtol, name=""):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    bound = atol + rtol * ref.abs()
    bad = err > bound
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.numel()} off; max err {err.max().item():.4g} " \
                          f"(ref max {ref.abs().max().item():.4g}) first bad idx {bad.nonzero()[0].tolist()}"


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 768), (216, 300, 128), (6912, 768, 768), (100, 64, 3072),
                                   (512, 2304, 768)])
def test_gemm_bf16_bias(ops, M, N, K):
    A, W = rnd(M, K, seed=1), rnd(N, K, scale=0.05, seed=2)
    bias = rnd(N, seed=3, dtype=torch.float32)
    Cbuf = torch.full((M, (N + 7) // 8 * 8), 7.0, dtype=BF, device="cuda")     # bf16 rows must be 16-B aligned
    C = Cbuf[:, :N]
    ops.gemm_nt(A, W, C, bias=bias)
    ref = A.float() @ W.float().t() + bias
    close(C, ref, 2e-2, 1e-2, "gemm bf16")
    assert (Cbuf[:, N:] == 7.0).all()


# kernel selector of spmm_gemm_nt (include/spmm_hip.h): 1 = 128x128, 2 = 256x128 ring, 3 = 256x256, 5 = 128x128 with loader + compute waves,
# 8 = 256x256 8-phase (persistent), 9 = the same kernel with one workgroup per tile
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (6912, 768, 768), (1000, 2304, 128), (216, 300, 128), (513, 520, 3072), (70000, 768, 128),
                                   (66000, 1024, 256)])
@pytest.mark.parametrize("kernel", [1, 2, 3, 5, 8, 9])
def test_gemm_tile_kernels(ops, M, N, K, kernel):
    """Every tile kernel forced on small / ragged / large shapes (the heuristic alone would never run the big tiles there):
    bias + residual epilogue, GELU with pre-activation output, and untouched padding columns."""
    if kernel in (8, 9) and N % 8:
        pytest.skip("the 8-phase kernel stores whole 16-B chunks: N % 8 == 0")
    A, W = rnd(M, K, seed=21), rnd(N, K, scale=0.05, seed=22)
    bias = rnd(N, seed=23, dtype=torch.float32)
    R = rnd(M, (N + 7) // 8 * 8, seed=24)[:, :N]
    Cbuf = torch.full((M, (N + 7) // 8 * 8), 7.0, dtype=BF, device="cuda")
    ops.gemm_nt(A, W, Cbuf[:, :N], bias=bias, R=R, kernel=kernel)
    ref = A.float() @ W.float().t() + bias + R.float()
    close(Cbuf[:, :N], ref, 3e-2, 1e-2, f"gemm kernel {kernel}")
    assert (Cbuf[:, N:] == 7.0).all()
    C, C2 = torch.empty(M, Cbuf.shape[1], dtype=BF, device="cuda"), torch.empty(M, Cbuf.shape[1], dtype=BF, device="cuda")
    ops.gemm_nt(A, W, C[:, :N], bias=bias, epi=ops.EPI_GELU, C2=C2[:, :N], kernel=kernel)
    pre = A.float() @ W.float().t() + bias
    close(C2[:, :N], pre, 3e-2, 1e-2, "pre-activation")
    close(C[:, :N], torch.nn.functional.gelu(pre), 3e-2, 1e-2, "gelu")
    G = rnd(M, (N + 7) // 8 * 8, seed=25)[:, :N]
    D = torch.empty(M, Cbuf.shape[1], dtype=BF, device="cuda")
    cs = torch.ones(N, device="cuda")
    ops.gemm_nt(A, W, D[:, :N], epi=ops.EPI_GELU_GRAD, G=G, colsum=cs, kernel=kernel)
    close(cs, 1.0 + D[:, :N].float().sum(0), 5e-2 * math.sqrt(M / 256), 2e-3, "fused column sums")
    g = G.float().requires_grad_(True)
    torch.nn.functional.gelu(g).sum().backward()
    close(D[:, :N], (A.float() @ W.float().t()) * g.grad, 3e-2, 1.5e-2, "gelu grad")
    # the pair the FFN uses: forward keeps gelu'(pre) as the second output, backward multiplies by it
    ops.gemm_nt(A, W, C[:, :N], bias=bias, epi=ops.EPI_GELU_DERIV, C2=C2[:, :N], kernel=kernel)
    pg = pre.clone().requires_grad_(True)
    torch.nn.functional.gelu(pg).sum().backward()
    close(C[:, :N], torch.nn.functional.gelu(pre), 3e-2, 1e-2, "gelu (deriv epilogue)")
    close(C2[:, :N], pg.grad, 1e-2, 1e-2, "gelu' output")
    cs.fill_(1.0)
    ops.gemm_nt(A, W, D[:, :N], epi=ops.EPI_MUL, G=C2[:, :N], colsum=cs, kernel=kernel)
    close(D[:, :N], (A.float() @ W.float().t()) * C2[:, :N].float(), 3e-2, 1.5e-2, "multiply epilogue")
    close(cs, 1.0 + D[:, :N].float().sum(0), 5e-2 * math.sqrt(M / 256), 2e-3, "fused column sums (multiply epilogue)")


def test_gemm_one_workgroup_per_tile_mode_is_bit_identical(ops):
    """`ops.nt_tiles_per_workgroup()` (what the data-parallel backward switches on while collectives hold CUs): automatically chosen
    NT GEMMs launch one workgroup per tile; the tiles and their accumulation order are the persistent kernel's, so every output --
    including the fused column sums' inputs -- is identical bit for bit, and the switch is restored on exit."""
    for (M, N, K, epi) in [(70000, 768, 768, ops.EPI_BF16), (33000, 3072, 768, ops.EPI_GELU_DERIV), (33000, 768, 3072, ops.EPI_BF16),
                           (33000, 3072, 768, ops.EPI_MUL), (520, 256, 128, ops.EPI_BF16)]:
        A, W = rnd(M, K, seed=31), rnd(N, K, scale=0.05, seed=32)
        bias = rnd(N, seed=33, dtype=torch.float32)
        G = rnd(M, N, seed=34) if epi == ops.EPI_MUL else None
        outs = []
        for tiles in (False, True):
            C = torch.zeros(M, N, dtype=BF, device="cuda")
            C2 = torch.zeros(M, N, dtype=BF, device="cuda") if epi == ops.EPI_GELU_DERIV else None
            with ops.nt_tiles_per_workgroup(tiles):
                assert ops._nt_auto == (ops.GEMM_AUTO_TILES if tiles else ops.GEMM_AUTO)
                ops.gemm_nt(A, W, C, bias=None if epi == ops.EPI_MUL else bias, epi=epi, C2=C2, G=G)
            assert ops._nt_auto == ops.GEMM_AUTO
            outs.append((C, C2))
        assert torch.equal(outs[0][0], outs[1][0]), (M, N, K, epi)
        if outs[0][1] is not None:
            assert torch.equal(outs[0][1], outs[1][1])
        if epi == ops.EPI_BF16:
            close(outs[1][0], A.float() @ W.float().t() + bias, 3e-2, 1e-2, "per-tile launch")


def test_gemm_kernel_selector_rejects_unsupported(ops):
    A, W = rnd(256, 192), rnd(256, 192)
    C = torch.empty(256, 256, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="8-phase"):
        ops.gemm_nt(A, W, C, kernel=8)          # K = 192 is not a multiple of 128
    with pytest.raises(RuntimeError, match="bf16-output"):
        ops.gemm_nt(A, W, torch.empty(256, 256, device="cuda"), epi=ops.EPI_F32, kernel=3)
    with pytest.raises(RuntimeError, match="selector"):
        ops.gemm_nt(A, W, C, kernel=4)


def test_gemm_strided_operands_and_residual(ops):
    M, N, K = 300, 128, 256
    big = rnd(M, 3 * K, seed=5)
    A = big[:, K:2 * K]                       # row stride 3K, unit column stride
    W = rnd(N, K, scale=0.05, seed=6)
    R = rnd(M, N, seed=7)
    Cbig = torch.zeros(M, 2 * N, dtype=BF, device="cuda")
    ops.gemm_nt(A, W, Cbig[:, N:], R=R, alpha=0.5)
    ref = 0.5 * (A.float() @ W.float().t()) + R.float()
    close(Cbig[:, N:], ref, 2e-2, 1e-2, "gemm strided")
    assert Cbig[:, :N].abs().max().item() == 0.0


def test_gemm_gelu_and_grad_epilogues(ops):
    M, N, K = 384, 512, 128
    A, W = rnd(M, K, seed=8), rnd(N, K, scale=0.1, seed=9)
    bias = rnd(N, seed=10, dtype=torch.float32)
    C, C2 = torch.empty(M, N, dtype=BF, device="cuda"), torch.empty(M, N, dtype=BF, device="cuda")
    ops.gemm_nt(A, W, C, bias=bias, epi=ops.EPI_GELU, C2=C2)
    pre = A.float() @ W.float().t() + bias
    close(C2, pre, 2e-2, 1e-2, "pre-activation")
    close(C, torch.nn.functional.gelu(pre), 2e-2, 1e-2, "gelu")
    # GELU-grad epilogue: out = (A W^T) * gelu'(G)
    G = rnd(M, N, seed=11)
    D = torch.empty(M, N, dtype=BF, device="cuda")
    cs = torch.ones(N, device="cuda")
    ops.gemm_nt(A, W, D, epi=ops.EPI_GELU_GRAD, G=G, colsum=cs)
    close(cs, 1.0 + D.float().sum(0), 5e-2, 1e-3, "fused column sums of the GELU-grad output")
    g = G.float().requires_grad_(True)
    torch.nn.functional.gelu(g).sum().backward()
    close(D, (A.float() @ W.float().t()) * g.grad, 3e-2, 1.5e-2, "gelu grad")


def test_gemm_f32_epilogues_and_splitk(ops):
    M, N, K = 256, 256, 2048
    A, W = rnd(M, K, seed=12), rnd(N, K, scale=0.05, seed=13)
    ref = A.float() @ W.float().t()
    div = torch.tensor([0.07], device="cuda")
    C = torch.empty(M, N, device="cuda")
    for kernel in (0, 1, 5):                    # the automatic choice, the 128x128 kernel, the 128x128 kernel with loader waves
        ops.gemm_nt(A, W, C, epi=ops.EPI_F32, div=div, kernel=kernel)
        close(C, ref / 0.07, 1e-2, 1e-4, f"f32 + div, kernel {kernel}")
        C.fill_(1.0)
        ops.gemm_nt(A, W, C, epi=ops.EPI_F32_ACC, kernel=kernel)
        close(C, ref + 1.0, 2e-3, 1e-4, f"f32 acc, kernel {kernel}")
        for splits in (1, 4, 7, 32):
            C.fill_(2.0)
            ops.gemm_nt(A, W, C, epi=ops.EPI_F32_ATOMIC, splits=splits, kernel=kernel)
            close(C, ref + 2.0, 2e-3, 1e-4, f"atomic split {splits}, kernel {kernel}")


@pytest.mark.parametrize("M,N,K,splits", [(64, 128, 128, 1), (216, 128, 256, 1), (216, 128, 256, 3), (6912, 768, 768, None),
                                          (4096, 2304, 768, None), (1000, 300, 128, 2), (130, 64, 192, 1), (8192, 768, 3072, None),
                                          (2100, 300, 520, 2), (13824, 768, 768, None),
                                          # M % 128 = 1, 63, 64, 65, 127, 32: the last row slice of the 8-phase kernel overlaps the one before (masked in LDS)
                                          (4097, 768, 768, None), (8255, 768, 768, None), (8256, 2304, 768, None), (8257, 768, 3072, None),
                                          (4223, 768, 768, None), (84256, 768, 768, None), (5000, 768, 768, 1), (5000, 768, 768, 3)])
@pytest.mark.parametrize("kernel", [1, 8])      # 128x128 tiles | 256x256 tiles on the 8-phase schedule (+ the 128x128 kernel for M % 128 rows)
def test_gemm_tn_weight_gradient(ops, M, N, K, splits, kernel):
    if kernel == 8 and (N % 8 or K % 8):
        pytest.skip("the 8-phase weight-gradient kernel reads whole 16-B chunks: N, K % 8 == 0")
    lda = (N + 7) // 8 * 8 + 16
    Abig = rnd(M, lda, seed=14)
    A = Abig[:, :N]                            # strided dY (e.g. dlogits[:, :V] inside a padded buffer)
    B = rnd(M, K, scale=0.5, seed=15)
    C = torch.full((N, K), 3.0, device="cuda")
    ops.gemm_tn(A, B, C, alpha=0.5, splits=splits, kernel=kernel)
    ref = 3.0 + 0.5 * (A.float().t() @ B.float())
    close(C, ref, 2e-3 * math.sqrt(M), 1e-4, f"gemm_tn kernel {kernel}")
    cs = torch.ones(N, device="cuda")
    ops.colsum_bf16(A, cs) if N % 4 == 0 else None
    close(cs, 1.0 + A.float().sum(0), 1e-3 * math.sqrt(M), 1e-5, "colsum")


def test_gemm_tn_default_choice_matches_both_kernels(ops):
    """The shape-based choice (the training step's path) against both forced kernels at a step-like shape with a ragged row count."""
    M, N, K = 33000, 768, 3072
    A, B = rnd(M, N, seed=16), rnd(M, K, scale=0.5, seed=17)
    out = []
    for kernel in (0, 1, 8):
        C = torch.zeros(N, K, device="cuda")
        ops.gemm_tn(A, B, C, kernel=kernel)
        out.append(C)
    close(out[0], out[1], 2e-3 * math.sqrt(M), 1e-4, "default vs 128x128")
    close(out[2], out[1], 2e-3 * math.sqrt(M), 1e-4, "8-phase vs 128x128")


def test_gemm_rejects_bad_shapes(ops):
    A, W = rnd(64, 96), rnd(64, 96)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        ops.gemm_nt(A, W, torch.empty(64, 64, dtype=BF, device="cuda"))


# ------------------------------------------------------------------------------------------- attention
def ref_attention(q, k, v, mask, nH, causal_from, is_cross, drop_mask=None, p=0.0):
    """q [nseq,Lq,nH*64] fp32 etc.; returns O [nseq,Lq,nH*64], lse [nseq,nH,Lq] (reference arithmetic of xbert.py:305-354)."""
    nseq, Lq, _ = q.shape
    Lkv = k.shape[1]
    qh = q.view(nseq, Lq, nH, 64).permute(0, 2, 1, 3)
    kh = k.view(nseq, Lkv, nH, 64).permute(0, 2, 1, 3)
    vh = v.view(nseq, Lkv, nH, 64).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2) / 8.0
    m = mask.float() if mask is not None else torch.ones(nseq, Lkv, device=q.device)
    if is_cross:
        add = (1 - m)[:, None, None, :] * torch.finfo(torch.float32).min
    else:
        ext = m[:, None, None, :].expand(nseq, 1, Lq, Lkv).clone()
        ids = torch.arange(Lq, device=q.device)
        causal = (torch.arange(Lkv, device=q.device)[None, :] <= ids[:, None]).float()
        for sidx in range(causal_from, nseq):
            ext[sidx, 0] = ext[sidx, 0] * causal
        add = (1 - ext) * -10000.0
    s = s + add
    lse = torch.logsumexp(s, dim=-1)
    pr = torch.softmax(s, dim=-1)
    if drop_mask is not None:
        pr = pr * drop_mask / (1 - p)
    o = (pr @ vh).permute(0, 2, 1, 3).reshape(nseq, Lq, nH * 64)
    return o, lse


ATT_CASES = [  # nseq, nH, Lq, Lkv, causal_from, is_cross
    (3, 2, 54, 54, 3, False), (4, 2, 54, 54, 2, False), (2, 12, 128, 128, 1, False), (3, 2, 54, 128, 3, True),
    (3, 2, 128, 54, 3, True), (5, 2, 16, 16, 2, False), (2, 2, 24, 54, 2, True), (2, 3, 100, 77, 2, True),
    (2, 2, 33, 33, 0, False),
    # 128 < L <= 256: the K/V panel still sits in LDS, a wave's 32 x Lkv score tile in registers; the forward runs one workgroup per
    # 128-query chunk, the backward one launch per chunk (later chunks add to dK / dV)
    (2, 2, 256, 256, 1, False), (3, 2, 200, 200, 1, False), (2, 3, 192, 192, 0, False), (3, 2, 54, 256, 3, True), (2, 2, 256, 54, 2, True),
    (2, 2, 130, 54, 2, True), (2, 2, 160, 224, 2, True), (2, 12, 129, 129, 1, False),
]


def _attn_inputs(nseq, nH, Lq, Lkv, seed):
    H = nH * 64
    qkv = rnd(nseq * Lq, 3 * H, seed=seed)            # fused buffer: exercises row strides
    kv = rnd(nseq * Lkv, 2 * H, seed=seed + 1)
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(max(2, Lkv // 2), Lkv + 1, (nseq,), generator=g)
    lens[0] = Lkv
    mask = (torch.arange(Lkv)[None, :] < lens[:, None]).int().cuda()
    return qkv, kv, mask


@pytest.mark.parametrize("nseq,nH,Lq,Lkv,causal_from,is_cross", ATT_CASES)
def test_attention_forward(ops, nseq, nH, Lq, Lkv, causal_from, is_cross):
    H = nH * 64
    qkv, kv, mask = _attn_inputs(nseq, nH, Lq, Lkv, seed=20)
    if is_cross:
        Q, K, V = qkv[:, :H], kv[:, :H], kv[:, H:]
    else:
        Q, K, V = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    O = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda")
    lse = torch.zeros(nseq, nH, Lq, device="cuda")
    ops.attn_fwd(Q, K, V, O, lse, nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, kmask=mask, causal_from=causal_from, is_cross=is_cross)
    ro, rl = ref_attention(Q.float().reshape(nseq, Lq, H), K.float().reshape(nseq, Lkv, H), V.float().reshape(nseq, Lkv, H),
                           mask, nH, causal_from, is_cross)
    close(lse, rl, 2e-3, 1e-4, "lse")
    close(O.view(nseq, Lq, H), ro, 1.5e-2, 1e-2, "attention out")


@pytest.mark.parametrize("nseq,nH,Lq,Lkv,causal_from,is_cross", ATT_CASES)
def test_attention_backward(ops, nseq, nH, Lq, Lkv, causal_from, is_cross):
    H = nH * 64
    qkv, kv, mask = _attn_inputs(nseq, nH, Lq, Lkv, seed=30)
    if is_cross:
        Q, K, V = qkv[:, :H], kv[:, :H], kv[:, H:]
    else:
        Q, K, V = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    dO = rnd(nseq * Lq, H, seed=31)
    O = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda")
    lse = torch.zeros(nseq, nH, Lq, device="cuda")
    ops.attn_fwd(Q, K, V, O, lse, nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, kmask=mask, causal_from=causal_from, is_cross=is_cross)
    dqkv = torch.zeros_like(qkv)
    dkv = torch.zeros_like(kv)
    if is_cross:
        dQ, dK, dV = dqkv[:, :H], dkv[:, :H], dkv[:, H:]
    else:
        dQ, dK, dV = dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:]
    ops.attn_bwd(Q, K, V, O, lse, dO, dQ, dK, dV, nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, kmask=mask, causal_from=causal_from,
                 is_cross=is_cross)
    q = Q.float().reshape(nseq, Lq, H).requires_grad_(True)
    k = K.float().reshape(nseq, Lkv, H).requires_grad_(True)
    v = V.float().reshape(nseq, Lkv, H).requires_grad_(True)
    ro, _ = ref_attention(q, k, v, mask, nH, causal_from, is_cross)
    ro.backward(dO.float().view(nseq, Lq, H))
    for got, ref, nm in ((dQ, q.grad, "dQ"), (dK, k.grad, "dK"), (dV, v.grad, "dV")):
        ref2 = ref.reshape(got.shape)
        close(got, ref2, 3e-2 * max(1.0, ref2.abs().max().item() / 8), 2e-2, nm)


def test_attention_backward_dk_dv_across_two_query_chunks(ops):
    """128 < Lq <= 256: the backward runs one launch per 128-query chunk and the second chunk ADDS its dK / dV to the first one's bf16
    result (csrc/attention.hip, spmm_attn_bwd) -- one more bf16 rounding than the single-chunk form.  Held tight here: the whole-tensor
    relative L2 error of dK and dV against fp32 autograd at Lq = Lkv = 256 must stay within a rounding or two of bf16 (2^-9 / sqrt 3 =
    1.1e-3 per rounding) and within 1.6 x the single-chunk error at Lq = 128 on the same keys.  Measured: dK 2.85e-3 -> 3.37e-3, dV 2.33e-3 ->
    2.94e-3 (dQ 2.90e-3 both): the extra rounding costs 18-26 %, bound 4e-3."""
    nseq, nH, Lkv = 6, 4, 256
    H = nH * 64
    err = {}
    for Lq in (128, 256):
        qkv, kv, mask = _attn_inputs(nseq, nH, Lq, Lkv, seed=77)
        Q, K, V = qkv[:, :H], kv[:, :H], kv[:, H:]
        dO = rnd(nseq * Lq, H, seed=78)
        O = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda")
        lse = torch.zeros(nseq, nH, Lq, device="cuda")
        ops.attn_fwd(Q, K, V, O, lse, nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, kmask=mask, is_cross=True)
        dQ = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda")
        dKV = torch.zeros(nseq * Lkv, 2 * H, dtype=BF, device="cuda")
        ops.attn_bwd(Q, K, V, O, lse, dO, dQ, dKV[:, :H], dKV[:, H:], nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, kmask=mask, is_cross=True)
        q = Q.float().reshape(nseq, Lq, H).requires_grad_(True)
        k = K.float().reshape(nseq, Lkv, H).requires_grad_(True)
        v = V.float().reshape(nseq, Lkv, H).requires_grad_(True)
        ro, _ = ref_attention(q, k, v, mask, nH, nseq, True)
        ro.backward(dO.float().view(nseq, Lq, H))
        rel = lambda got, ref: ((got.float() - ref.reshape(got.shape)).norm() / ref.norm()).item()
        err[Lq] = (rel(dKV[:, :H], k.grad), rel(dKV[:, H:], v.grad), rel(dQ, q.grad))
        print(f"Lq={Lq}: relative L2 error dK {err[Lq][0]:.2e} dV {err[Lq][1]:.2e} dQ {err[Lq][2]:.2e}")
    for i, nm in enumerate(("dK", "dV")):
        assert err[256][i] < 4e-3, (nm, err)
        assert err[256][i] < 1.6 * err[128][i] + 2e-4, (nm, err)


@pytest.mark.parametrize("nseq,U,nH,Lq,Lkv", [(8, 3, 2, 54, 128), (8, 2, 12, 128, 54), (5, 5, 2, 40, 40)])
def test_cross_attention_with_shared_kv_sources(ops, nseq, U, nH, Lq, Lkv):
    """kv_seq: query sequence s reads K/V of source kv_seq[s].  Outputs and dQ equal the kernel run on physically gathered
    K/V copies bit for bit; segment_sum of the per-query dK/dV equals (fp32 sum, one bf16 rounding) the sum over sharers."""
    H = nH * 64
    g = torch.Generator().manual_seed(nseq + U)
    Q = rnd(nseq * Lq, H, seed=40)
    kvu = rnd(U * Lkv, 2 * H, seed=41)
    idx = torch.randint(0, U, (nseq,), generator=g)
    idx[:U] = torch.arange(U)                                     # every source used at least once
    idx = idx.cuda()
    mask = (torch.rand(nseq, Lkv, generator=g) > 0.2).int().cuda()
    mask[:, 0] = 1
    dO = rnd(nseq * Lq, H, seed=42)
    kvg = kvu.view(U, Lkv, 2 * H)[idx].reshape(nseq * Lkv, 2 * H).contiguous()   # the gathered copies the reference path builds
    outs = []
    for K, V, ks in ((kvu[:, :H], kvu[:, H:], idx.to(torch.int32)), (kvg[:, :H], kvg[:, H:], None)):
        O = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda")
        lse = torch.zeros(nseq, nH, Lq, device="cuda")
        ops.attn_fwd(Q, K, V, O, lse, nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, kmask=mask, is_cross=True, kv_seq=ks)
        dQ = torch.zeros_like(Q)
        dKV = torch.zeros(nseq * Lkv, 2 * H, dtype=BF, device="cuda")
        ops.attn_bwd(Q, K, V, O, lse, dO, dQ, dKV[:, :H], dKV[:, H:], nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, kmask=mask, is_cross=True, kv_seq=ks)
        outs.append((O, lse, dQ, dKV))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    order = torch.sort(idx, stable=True).indices.to(torch.int32)
    start = torch.zeros(U + 1, dtype=torch.int32, device="cuda")
    start[1:] = torch.cumsum(torch.bincount(idx, minlength=U), 0)
    W = Lkv * 2 * H
    dKV = outs[0][3].view(nseq, W)
    folded = ops.segment_sum_bf16(dKV, start, order, torch.zeros(U, W, dtype=BF, device="cuda"))
    ref = torch.zeros(U, W, device="cuda").index_add_(0, idx, dKV.float())
    assert torch.equal(folded, ref.to(BF))


def _xattn_composite(ops, Q, K, V, Wo, bo, R, gamma, beta, *, nseq, nH, Lq, Lkv, eps, pa, ph, seed, salt_a, salt_h, row_base, **lay):
    """The five-launch form the fused block replaces: attention core -> output GEMM -> LayerNorm(dropout(x) + residual)."""
    M, H = Q.shape
    ctx = torch.zeros(M, H, dtype=BF, device="cuda")
    lse = torch.zeros(nseq, nH, Lq, device="cuda")
    ops.attn_fwd(Q, K, V, ctx, lse, nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, is_cross=True, dropout_p=pa, seed=seed, salt=salt_a, **lay)
    x = torch.zeros(M, H, dtype=BF, device="cuda")
    ops.gemm_nt(ctx, Wo, x, bias=bo)
    # spmm_ln_fwd counts dropout rows from the first row it is given: embed the group at row_base of a larger batch
    xb = torch.zeros(row_base + M, H, dtype=BF, device="cuda"); xb[row_base:] = x
    rb = torch.zeros(row_base + M, H, dtype=BF, device="cuda"); rb[row_base:] = R
    y, z = torch.zeros_like(xb), torch.zeros_like(xb)
    mean, rstd = torch.zeros(row_base + M, device="cuda"), torch.zeros(row_base + M, device="cuda")
    ops.ln_fwd(xb, rb, gamma, beta, y, zout=z, mean=mean, rstd=rstd, eps=eps, dropout_p=ph, seed=seed, salt=salt_h)
    return dict(y=y[row_base:], z=z[row_base:], mean=mean[row_base:], rstd=rstd[row_base:], ctx=ctx, lse=lse)


@pytest.mark.parametrize("nH,nseq,U,Lq,Lkv,packed,drop", [
    (12, 6, 3, 54, 128, False, False),      # property queries -> SMILES keys, shared sources, key mask (P5 | P7 | P12 shape)
    (12, 5, 2, 128, 54, False, False),      # SMILES queries -> property keys: two 64-row panels per sequence
    (12, 6, 3, 54, 128, True, False),       # packed key/value sources (kv_row0 / kv_len)
    (12, 5, 2, 128, 54, True, False),       # packed query rows (q_row0 / q_len), ragged panels
    (12, 6, 3, 54, 128, False, True),       # both dropouts: the masks of spmm_attn_fwd / spmm_ln_fwd
    (12, 4, 4, 128, 54, True, True),
    (2, 5, 2, 40, 24, False, False),        # H = 128 (the tiny configuration), one head pair, one key tile
    (4, 3, 3, 70, 90, True, True),          # H = 256, three key tiles
    (12, 1, 1, 1, 1, False, False),         # one query row, one key: every tile is padding but one element
    (12, 3, 2, 65, 33, True, False),        # a second panel with a single valid row; 33 keys = one full tile + one key
    (2, 7, 7, 128, 128, False, True),       # full 128 x 128 at H = 128, dropout
])
def test_fused_cross_attention_block(ops, nH, nseq, U, Lq, Lkv, packed, drop):
    """spmm_xattn_fwd (ONE launch: attention core + output projection + dropout + residual + LayerNorm) against (a) the composite
    it replaces -- same kernels' dropout masks, so y / z / ctx / lse / mean / rstd must agree to bf16 rounding of the intermediate
    x (both forms round it to bf16, the fused kernel in its epilogue "exactly as the projection GEMM of the composite rounds it"; the two
    fp32 sums run in different orders, so a rounding may fall the other way) -- and (b) plain fp32 torch of xbert.py:305-354 + :369-373
    (dropout off).  Every instantiation, panel count and output configuration against float64: tests/test_xattn_block_gpu.py."""
    H = nH * 64
    g = torch.Generator().manual_seed(nseq * 7 + Lq)
    idx = torch.randint(0, U, (nseq,), generator=g); idx[:U] = torch.arange(U)
    i32 = lambda t: t.to(torch.int32).cuda()
    qlen = torch.randint(min(3, Lq), Lq + 1, (nseq,), generator=g); qlen[0] = Lq
    kvlen = torch.randint(min(2, Lkv), Lkv + 1, (U,), generator=g); kvlen[0] = Lkv
    if packed:
        q_row0 = torch.cumsum(qlen, 0) - qlen
        kv_row0 = torch.cumsum(kvlen, 0) - kvlen
        M, Mkv = int(qlen.sum()), int(kvlen.sum())
        lay = dict(q_row0=i32(q_row0), q_len=i32(qlen), kv_row0=i32(kv_row0), kv_len=i32(kvlen), kmask=None, kv_seq=i32(idx))
    else:
        M, Mkv = nseq * Lq, U * Lkv
        kmask = (torch.rand(nseq, Lkv, generator=g) > 0.25).int(); kmask[:, 0] = 1
        lay = dict(kmask=kmask.cuda(), kv_seq=i32(idx))
    Q = rnd(M, H, seed=60, scale=1.5)
    KV = rnd(Mkv, 2 * H, seed=61)
    R = rnd(M, H, seed=62)
    Wo = rnd(H, H, seed=63, scale=0.04)
    bo = torch.randn(H, generator=g).cuda() * 0.1
    gamma = (1.0 + 0.1 * torch.randn(H, generator=g)).cuda()
    beta = (0.1 * torch.randn(H, generator=g)).cuda()
    seed = torch.tensor([1234567], dtype=torch.int64, device="cuda")
    pa, ph = (0.1, 0.1) if drop else (0.0, 0.0)
    row_base, eps = 1000, 1e-12
    ref = _xattn_composite(ops, Q, KV[:, :H], KV[:, H:], Wo, bo, R, gamma, beta, nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, eps=eps, pa=pa, ph=ph,
                           seed=seed, salt_a=11, salt_h=22, row_base=row_base, **lay)
    WoF = ops.xattn_pack_wo(Wo)
    out = {k: torch.full_like(v, float("nan")) for k, v in ref.items()}
    ops.xattn_fwd(Q, KV[:, :H], KV[:, H:], WoF, bo, R, gamma, beta, out["y"], nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, eps=eps, Z=out["z"],
                  mean=out["mean"], rstd=out["rstd"], CTX=out["ctx"], lse=out["lse"], attn_dropout_p=pa, salt_a=11, hidden_dropout_p=ph,
                  salt_h=22, seed=seed, row_base=row_base, **lay)
    torch.cuda.synchronize()
    if packed:                                                     # lse keeps the dense [nseq, nH, Lq] indexing: compare the valid positions
        valid = (torch.arange(Lq)[None, :] < qlen[:, None]).cuda()
        assert torch.equal(out["lse"].transpose(1, 2)[valid], ref["lse"].transpose(1, 2)[valid])
    else:
        assert torch.equal(out["lse"], ref["lse"])
    assert torch.equal(out["ctx"], ref["ctx"])                   # the same arithmetic, MFMA for MFMA
    # x is rounded to bf16 between projection and LayerNorm in both forms, from fp32 sums taken in different orders: where the rounding
    # falls the other way |dz| <= 2^-8 |x| (x up to ~4 here), LayerNorm divides by ~1.5
    close(out["z"], ref["z"], atol=4e-2, rtol=1e-2, name="z")
    close(out["y"], ref["y"], atol=4e-2, rtol=1e-2, name="y")
    close(out["mean"], ref["mean"], atol=2e-3, rtol=1e-3, name="mean")
    close(out["rstd"], ref["rstd"], atol=0, rtol=4e-3, name="rstd")
    if drop:         # (a different dropout mask in either place would move ~10 % of the elements by O(1): the bounds above pin the masks)
        return
    # (b) fp32 torch
    qs = torch.cumsum(qlen, 0) - qlen if packed else torch.arange(nseq) * Lq
    ks = torch.cumsum(kvlen, 0) - kvlen if packed else torch.arange(U) * Lkv
    Qf, KVf, Rf, Wf = Q.float(), KV.float(), R.float(), Wo.float()
    for s_ in range(nseq):
        lq = int(qlen[s_]) if packed else Lq
        u = int(idx[s_]); lk = int(kvlen[u]) if packed else Lkv
        q = Qf[int(qs[s_]):int(qs[s_]) + lq].view(lq, nH, 64).transpose(0, 1)
        kv = KVf[int(ks[u]):int(ks[u]) + lk]
        k = kv[:, :H].view(lk, nH, 64).transpose(0, 1); v = kv[:, H:].view(lk, nH, 64).transpose(0, 1)
        sc = q @ k.transpose(1, 2) / 8.0
        if not packed:
            sc = sc + (1.0 - lay["kmask"][s_].float())[None, None, :] * torch.finfo(torch.float32).min
        c = (torch.softmax(sc, -1) @ v).transpose(0, 1).reshape(lq, H)
        zz = c @ Wf.t() + bo + Rf[int(qs[s_]):int(qs[s_]) + lq]
        yy = torch.nn.functional.layer_norm(zz, (H,), gamma, beta, eps)
        close(out["y"][int(qs[s_]):int(qs[s_]) + lq], yy, atol=6e-2, rtol=2e-2, name=f"y vs fp32 torch, sequence {s_}")


@pytest.mark.parametrize("Lq", [100, 230])
@pytest.mark.parametrize("is_cross,shared", [(False, False), (True, False), (True, True)])
def test_attention_packed_variable_length_layout(ops, is_cross, shared, Lq):
    """Packed rows (q_row0/q_len, kv_row0/kv_len) give bit-identical O, LSE, dQ, dK, dV on the valid rows to the dense
    padded layout with a key mask: the padded positions are simply never computed."""
    nseq, nH, Lkv = 6, 2, 54 if is_cross else Lq
    H = nH * 64
    g = torch.Generator().manual_seed(77)
    qlen = torch.randint(5, Lq + 1, (nseq,), generator=g); qlen[0] = Lq
    U = 3 if shared else nseq
    kvlen = qlen.clone() if not is_cross else torch.randint(3, Lkv + 1, (U,), generator=g)
    idx = torch.randint(0, U, (nseq,), generator=g) if shared else torch.arange(nseq)
    Qd = rnd(nseq * Lq, H, seed=50); dOd = rnd(nseq * Lq, H, seed=51)
    # padded query rows exist in the dense layout; in the model their upstream gradient is exactly zero (no loss reads them)
    dOd = dOd * (torch.arange(Lq)[None, :] < qlen[:, None]).reshape(-1, 1).to(BF).cuda()
    KVd = rnd(U * Lkv, 2 * H, seed=52) if is_cross else None
    if not is_cross:
        KVd = torch.cat([rnd(nseq * Lq, H, seed=53), rnd(nseq * Lq, H, seed=54)], dim=1)
    kmask_u = (torch.arange(Lkv)[None, :] < kvlen[:, None]).int()
    kmask = kmask_u[idx].contiguous().cuda()                             # dense path: per query sequence
    i32 = lambda t: t.to(torch.int32).cuda()
    # dense run
    Od = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda"); lsed = torch.zeros(nseq, nH, Lq, device="cuda")
    kw = dict(nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, is_cross=is_cross, kv_seq=i32(idx) if shared else None)
    ops.attn_fwd(Qd, KVd[:, :H], KVd[:, H:], Od, lsed, kmask=kmask, **kw)
    dQd = torch.zeros_like(Qd); dKVd = torch.zeros(nseq * Lkv, 2 * H, dtype=BF, device="cuda")
    ops.attn_bwd(Qd, KVd[:, :H], KVd[:, H:], Od, lsed, dOd, dQd, dKVd[:, :H], dKVd[:, H:], kmask=kmask, **kw)
    # packed run
    qsel = torch.cat([torch.arange(int(qlen[s])) + s * Lq for s in range(nseq)]).cuda()
    ksel = torch.cat([torch.arange(int(kvlen[u])) + u * Lkv for u in range(U)]).cuda()
    q0 = torch.cumsum(qlen, 0) - qlen; k0 = torch.cumsum(kvlen, 0) - kvlen
    Qp, dOp, KVp = Qd[qsel].contiguous(), dOd[qsel].contiguous(), KVd[ksel].contiguous()
    Op = torch.zeros_like(Qp); lsep = torch.zeros(nseq, nH, Lq, device="cuda")
    pk = dict(q_row0=i32(q0), q_len=i32(qlen), kv_row0=i32(k0), kv_len=i32(kvlen))
    ops.attn_fwd(Qp, KVp[:, :H], KVp[:, H:], Op, lsep, **kw, **pk)
    dQp = torch.zeros_like(Qp)
    dKVp = torch.zeros(nseq * Lkv if shared else KVp.shape[0], 2 * H, dtype=BF, device="cuda")
    ops.attn_bwd(Qp, KVp[:, :H], KVp[:, H:], Op, lsep, dOp, dQp, dKVp[:, :H], dKVp[:, H:], **kw, **pk)
    assert torch.equal(Op, Od[qsel]) and torch.equal(dQp, dQd[qsel])
    valid_q = (torch.arange(Lq)[None, :] < qlen[:, None]).cuda()
    assert torch.equal(lsep[valid_q[:, None, :].expand(nseq, nH, Lq)], lsed[valid_q[:, None, :].expand(nseq, nH, Lq)])
    if shared:      # dK/dV stay dense per query sequence; rows past the source's length are not written
        vk = kmask.bool().reshape(-1)
        assert torch.equal(dKVp[vk], dKVd[vk])
    else:
        assert torch.equal(dKVp, dKVd[ksel])


@pytest.mark.parametrize("nseq,nH,Lq,Lkv,causal_from,is_cross", [(3, 2, 300, 300, 1, False), (2, 2, 512, 512, 0, False), (3, 2, 54, 400, 3, True),
                                                               (2, 2, 300, 54, 2, True), (2, 2, 256, 256, 1, False)])
def test_attention_long_sequences_by_chunks(ops, nseq, nH, Lq, Lkv, causal_from, is_cross):
    """Sequences beyond the 256 rows the kernels keep on chip (up to the 512 positions of config_bert.json): chunked launches merged
    by log-sum-exp in forward, two-pass D in backward, against the fp32 reference arithmetic (<= 256: the single-launch kernels)."""
    H = nH * 64
    qkv, kv, _ = _attn_inputs(nseq, nH, Lq, Lkv, seed=60)
    g = torch.Generator().manual_seed(61)
    lens = torch.randint(Lkv // 2, Lkv + 1, (nseq,), generator=g); lens[0] = Lkv
    mask = (torch.arange(Lkv)[None, :] < lens[:, None]).int().cuda()
    if is_cross:
        Q, K, V = qkv[:, :H], kv[:, :H], kv[:, H:]
    else:
        Q, K, V = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    dO = rnd(nseq * Lq, H, seed=62)
    O = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda"); lse = torch.zeros(nseq, nH, Lq, device="cuda")
    kw = dict(nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, kmask=mask, causal_from=causal_from, is_cross=is_cross)
    ops.attn_fwd_long(Q, K, V, O, lse, **kw)
    q = Q.float().reshape(nseq, Lq, H).requires_grad_(True)
    k = K.float().reshape(nseq, Lkv, H).requires_grad_(True)
    v = V.float().reshape(nseq, Lkv, H).requires_grad_(True)
    ro, rl = ref_attention(q, k, v, mask, nH, causal_from, is_cross)
    close(lse, rl.detach(), 2e-3, 1e-4, "lse")
    close(O.view(nseq, Lq, H), ro.detach(), 1.5e-2, 1e-2, "attention out")
    dQ = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda"); dK = torch.zeros(nseq * Lkv, H, dtype=BF, device="cuda"); dV = torch.zeros_like(dK)
    ops.attn_bwd_long(Q, K, V, O, lse, dO, dQ, dK, dV, **kw)
    ro.backward(dO.float().view(nseq, Lq, H))
    for got, ref, nm in ((dQ, q.grad, "dQ"), (dK, k.grad, "dK"), (dV, v.grad, "dV")):
        ref2 = ref.reshape(got.shape)
        close(got, ref2, 3e-2 * max(1.0, ref2.abs().max().item() / 8), 2e-2, nm)


@pytest.mark.parametrize("L", [96, 256])
def test_attention_causal_rows_with_key0_masked(ops, L):
    """The reference's causal mask is ADDITIVE (-10000, xbert.py:889-948), not -inf: a row whose visible keys are all masked spreads
    over the future keys too, and with large scores a future key keeps a non-zero weight.  The kernels therefore never skip key tiles
    above the diagonal (a first version of the 256-long kernels did, and the closed-form-weight golden -- scores up to 1e4 -- caught
    it); rows with key 0 masked and scores of both scales are checked here."""
    nseq, nH = 3, 2
    H = nH * 64
    qkv = rnd(nseq * L, 3 * H, seed=70)
    qkv[:L] *= 40.0                                  # sequence 0: |scores| of several thousand, future keys outweigh -10000 for some rows
    mask = torch.ones(nseq, L, dtype=torch.int32)
    mask[1, 0] = 0; mask[2, :5] = 0; mask[2, L - 7:] = 0
    mask = mask.cuda()
    Q, K, V = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    dO = rnd(nseq * L, H, seed=71)
    O = torch.zeros(nseq * L, H, dtype=BF, device="cuda"); lse = torch.zeros(nseq, nH, L, device="cuda")
    kw = dict(nseq=nseq, nH=nH, Lq=L, Lkv=L, kmask=mask, causal_from=0)
    ops.attn_fwd(Q, K, V, O, lse, **kw)
    q = Q.float().reshape(nseq, L, H).requires_grad_(True)
    k = K.float().reshape(nseq, L, H).requires_grad_(True)
    v = V.float().reshape(nseq, L, H).requires_grad_(True)
    ro, rl = ref_attention(q, k, v, mask, nH, 0, False)
    close(lse, rl.detach(), 2e-3, 1e-4, "lse")
    close(O.view(nseq, L, H)[1:], ro.detach()[1:], 1.5e-2, 1e-2, "attention out")
    # (sequence 0: one-hot rows, values up to 170; a near-tie between two scores of several thousand moves an output by a few tenths)
    close(O.view(nseq, L, H)[:1], ro.detach()[:1], 1e-2 * ro[0].abs().max().item(), 1e-2, "attention out, large scores")
    dqkv = torch.zeros_like(qkv)
    ops.attn_bwd(Q, K, V, O, lse, dO, dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:], **kw)
    ro.backward(dO.float().view(nseq, L, H))
    # (gradients: sequences 1 and 2 only -- at sequence 0's score scale the softmax is one-hot up to near-ties whose gradient is decided
    # by the last bits of the fp32 scores, in the reference as much as here)
    for got, ref, nm in ((dqkv[:, :H], q.grad, "dQ"), (dqkv[:, H:2 * H], k.grad, "dK"), (dqkv[:, 2 * H:], v.grad, "dV")):
        ref2 = ref.reshape(got.shape)[L:]
        close(got[L:], ref2, 3e-2 * max(1.0, ref2.abs().max().item() / 8), 2e-2, nm)
        assert torch.isfinite(got.float()).all()


def test_attention_backward_near_constant_values(ops):
    """Regression: in a real model V rows (hence dP) are nearly constant across keys, so ds = P (dP - D) is a small
    difference of large numbers.  D must be the fp32 sum_kv P dP; taking it from rowsum(dO * bf16(O)) gave 50-300 %
    relative error on dQ / dK inside the model while every random-data test passed."""
    nseq, nH, Lq, Lkv = 4, 2, 54, 54
    H = nH * 64
    Q, K = rnd(nseq * Lq, H, scale=0.5, seed=44), rnd(nseq * Lkv, H, scale=0.5, seed=45)
    base = rnd(1, H, scale=2.0, seed=46).float()
    V = (base + 0.02 * rnd(nseq * Lkv, H, seed=47).float()).to(BF)
    dO = rnd(nseq * Lq, H, seed=48)
    O = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda")
    lse = torch.zeros(nseq, nH, Lq, device="cuda")
    kw = dict(nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, causal_from=2)
    ops.attn_fwd(Q, K, V, O, lse, **kw)
    dQ, dK, dV = torch.zeros_like(Q), torch.zeros_like(K), torch.zeros_like(V)
    ops.attn_bwd(Q, K, V, O, lse, dO, dQ, dK, dV, **kw)
    q = Q.float().reshape(nseq, Lq, H).requires_grad_(True)
    k = K.float().reshape(nseq, Lkv, H).requires_grad_(True)
    v = V.float().reshape(nseq, Lkv, H).requires_grad_(True)
    ro, _ = ref_attention(q, k, v, None, nH, 2, False)
    ro.backward(dO.float().view(nseq, Lq, H))
    for got, ref, nm in ((dQ, q.grad, "dQ"), (dK, k.grad, "dK"), (dV, v.grad, "dV")):
        rel = ((got.float().reshape(ref.shape) - ref).norm() / ref.norm()).item()
        assert rel < 2e-2, (nm, rel, ref.norm().item())


@pytest.mark.parametrize("Lq,Lkv", [(54, 64), (200, 256)])
def test_attention_dropout_consistency(ops, Lq, Lkv):
    """The dense, unmasked, non-causal self-attention form only: recover the dropout mask from forwards with V = a shifted identity (one
    pass per 64 keys), then check fwd/bwd against torch using THAT mask.  The layouts the training step launches with dropout on (packed
    rows, shared sources, causal_from, key masks, Lq = 1, the chunked path) and the mask each backward path applies, decision by
    decision, are in tests/test_attention_dropout_gpu.py."""
    nseq, nH, p = 3, 2, 0.1
    H = nH * 64
    Q, K = rnd(nseq * Lq, H, seed=40), rnd(nseq * Lkv, H, seed=41)
    seed = torch.tensor([1234567], dtype=torch.int64, device="cuda")
    O = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda")
    lse = torch.zeros(nseq, nH, Lq, device="cuda")
    kw = dict(nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, dropout_p=p, seed=seed, salt=99)

    def dropped_probabilities():
        parts = []
        for off in range(0, Lkv, 64):                                      # V[kv][d] = [kv == off + d] per head
            eye = torch.zeros(Lkv, 64, dtype=BF, device="cuda")
            eye[off:off + 64] = torch.eye(64, dtype=BF, device="cuda")
            ops.attn_fwd(Q, K, eye.repeat(nseq, nH), O, lse, **kw)
            parts.append(O.float().view(nseq, Lq, nH, 64).permute(0, 2, 1, 3).clone())
        return torch.cat(parts, dim=-1)                                    # [nseq, nH, Lq, Lkv]

    pd = dropped_probabilities()
    keep = (pd != 0).float()
    rate = 1 - keep.mean().item()
    assert abs(rate - p) < 0.02, rate
    V, dO = rnd(nseq * Lkv, H, seed=42), rnd(nseq * Lq, H, seed=43)
    ops.attn_fwd(Q, K, V, O, lse, **kw)
    q = Q.float().reshape(nseq, Lq, H).requires_grad_(True)
    k = K.float().reshape(nseq, Lkv, H).requires_grad_(True)
    v = V.float().reshape(nseq, Lkv, H).requires_grad_(True)
    ro, _ = ref_attention(q, k, v, None, nH, nseq, False, drop_mask=keep, p=p)
    close(O.view(nseq, Lq, H), ro, 2e-2, 1e-2, "dropout fwd")
    dQ, dK, dV = torch.zeros_like(Q), torch.zeros_like(K), torch.zeros_like(V)
    ops.attn_bwd(Q, K, V, O, lse, dO, dQ, dK, dV, **kw)
    ro.backward(dO.float().view(nseq, Lq, H))
    for got, ref, nm in ((dQ, q.grad, "dQ"), (dK, k.grad, "dK"), (dV, v.grad, "dV")):
        close(got, ref.reshape(got.shape), 4e-2, 2e-2, "dropout " + nm)
    # a different seed gives a different mask
    seed.fill_(7654321)
    assert ((dropped_probabilities() != 0) != (pd != 0)).float().mean().item() > 0.05


from helpers_gpu import _host_dropout_keep      # noqa: E402  (the host model of the generator lives in tests/helpers_gpu.py)


def test_dropout_masks_equal_the_host_model_of_the_hash(ops):
    """The keep masks the kernels draw (attention probabilities: recovered with Q = 0 and V = identity; hidden dropout: recovered from the
    pre-LayerNorm sum of a ones matrix) are bit for bit the host model's, so what was checked about that function's statistics holds for
    the device.  1.5 M + 3.1 M decisions; the drop rate is also checked to four standard deviations."""
    p, seed_v = 0.1, 20260931
    seed = torch.tensor([seed_v], dtype=torch.int64, device="cuda")
    # ---- attention: element (seq, head, q, kv) uses row counter (seq * nH + head) * Lq + q
    nseq, nH, Lq, Lkv = 16, 12, 128, 64
    H = nH * 64
    Q = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda")               # uniform softmax: every probability is 1 / 64 > 0
    K = rnd(nseq * Lkv, H, seed=44)
    eye = torch.eye(64, dtype=BF, device="cuda").repeat(nseq, nH)
    O = torch.zeros(nseq * Lq, H, dtype=BF, device="cuda")
    lse = torch.zeros(nseq, nH, Lq, device="cuda")
    ops.attn_fwd(Q, K, eye, O, lse, nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, dropout_p=p, seed=seed, salt=4242)
    got = (O.float().view(nseq, Lq, nH, 64).permute(0, 2, 1, 3) != 0).cpu().numpy().reshape(nseq * nH * Lq, Lkv)
    want = _host_dropout_keep(seed_v, 4242, np.arange(nseq * nH * Lq), Lkv, p)
    assert np.array_equal(got, want), f"attention mask: {np.mean(got != want):.4f} of the decisions differ from the host model"
    # ---- hidden dropout of the LayerNorm kernels: element (row, col) uses row counter row
    rows, Hh = 4099, 768
    x = torch.ones(rows, Hh, dtype=BF, device="cuda")
    z, y = torch.empty_like(x), torch.empty_like(x)
    ops.ln_fwd(x, None, torch.ones(Hh, device="cuda"), torch.zeros(Hh, device="cuda"), y, zout=z, dropout_p=p, seed=seed, salt=77)
    got2 = (z.float() != 0).cpu().numpy()
    want2 = _host_dropout_keep(seed_v, 77, np.arange(rows), Hh, p)
    assert np.array_equal(got2, want2), f"hidden-dropout mask: {np.mean(got2 != want2):.4f} of the decisions differ from the host model"
    for m in (got, got2):
        n, pt = m.size, int(p * 65536 + 0.5) / 65536
        assert abs((1 - m.mean()) - pt) < 4 * (pt * (1 - pt) / n) ** 0.5, (1 - m.mean(), pt)


# ------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("rows,H", [(7, 128), (1000, 768), (1003, 768), (333, 256), (64, 1024), (61, 512), (5, 1000)])
def test_layernorm_fwd_bwd(ops, rows, H):
    x, res = rnd(rows, H, seed=50), rnd(rows, H, seed=51)
    gamma = (1 + 0.1 * torch.randn(H)).cuda()
    beta = (0.1 * torch.randn(H)).cuda()
    y = torch.empty_like(x)
    z = torch.empty_like(x)
    mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    ops.ln_fwd(x, res, gamma, beta, y, zout=z, mean=mean, rstd=rstd, eps=1e-12)
    zr = (x.float() + res.float()).requires_grad_(True)
    g = gamma.clone().requires_grad_(True)
    b = beta.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(zr, (H,), g, b, 1e-12)
    close(y, yr, 2e-2, 1e-2, "ln fwd")
    close(z, zr, 2e-2, 1e-2, "ln z")
    dy = rnd(rows, H, seed=52)
    dy2 = rnd(rows, H, seed=53)
    # backward from the bf16-rounded z the kernel stored, exactly what the product does
    zr2 = z.float().requires_grad_(True)
    yr2 = torch.nn.functional.layer_norm(zr2, (H,), g, b, 1e-12)
    yr2.backward(dy.float() + dy2.float())
    dz = torch.empty_like(x)
    dg, db = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
    dxs = torch.ones(H, device="cuda")
    ops.ln_bwd(dy, z, mean, rstd, gamma, dz, dy2=dy2, dgamma=dg, dbeta=db, dxsum=dxs)
    close(dz, zr2.grad, 3e-2, 2e-2, "ln dz")
    close(dxs, 1.0 + dz.float().sum(0), 2e-3 * math.sqrt(rows), 1e-4, "ln dxsum (bias gradient of the producing dense)")
    close(dg, g.grad, 2e-2 * math.sqrt(rows), 1e-2, "ln dgamma")
    close(db, b.grad, 2e-2 * math.sqrt(rows), 1e-2, "ln dbeta")


@pytest.mark.parametrize("rows,H,p", [(1000, 768, 0.1), (1003, 768, 0.0), (333, 256, 0.1), (61, 512, 0.0), (5, 1000, 0.1), (20000, 768, 0.1)])
def test_layernorm_backward_from_the_output(ops, rows, H, p):
    """spmm_ln_bwd with `beta_from_y`: the forward keeps NO pre-norm sum; the backward reads the LayerNorm's output y and recovers the
    normalised values as (y - beta) / gamma.  Against fp32 autograd through the exact sum, next to the stored-sum form on the same inputs:
    dz, dx (same dropout mask), dgamma, dbeta and the bias-gradient column sums must be as close as the stored-sum form's (one bf16-rounded
    tensor is read either way), incl. a channel with gamma == 0 (no information about the normalised value there: it contributes nothing)."""
    x, res = rnd(rows, H, seed=60), rnd(rows, H, seed=61)
    gamma = (1 + 0.2 * torch.randn(H)).cuda()
    gamma[7] = 0.0
    gamma[11] = -0.03
    beta = (0.2 * torch.randn(H)).cuda()
    seed = torch.full((1,), 4242, dtype=torch.int64, device="cuda")
    y, z = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    ops.ln_fwd(x, res, gamma, beta, y, zout=z, mean=mean, rstd=rstd, eps=1e-12, dropout_p=p, seed=seed, salt=9)
    y_only = torch.empty_like(x)
    rstd2 = torch.empty(rows, device="cuda")
    ops.ln_fwd(x, res, gamma, beta, y_only, zout=None, mean=torch.empty(rows, device="cuda"), rstd=rstd2, eps=1e-12, dropout_p=p, seed=seed, salt=9)
    assert torch.equal(y_only, y) and torch.equal(rstd2, rstd)                      # the forward without the stored sum writes the same output
    dy = rnd(rows, H, seed=62)
    out = {}
    for mode in ("z", "y"):
        dz, dx = torch.empty_like(x), torch.empty_like(x)
        dg, db, dxs = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
        ops.ln_bwd(dy, z if mode == "z" else y, mean if mode == "z" else None, rstd, gamma, dz, dx=dx if p > 0 else None, dgamma=dg, dbeta=db, dxsum=dxs,
                   dropout_p=p, seed=seed, salt=9, beta_from_y=beta if mode == "y" else None)
        out[mode] = (dz, dx if p > 0 else dz, dg, db, dxs)
    # fp32 reference from the UNROUNDED sum the kernel formed (z is its bf16 copy: use the stored copy's fp32 value + the forward's statistics)
    zr = z.float().requires_grad_(True)
    g = gamma.clone().requires_grad_(True)
    b = beta.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(zr, (H,), g, b, 1e-12).backward(dy.float())
    keep = out["z"][1].float() != 0 if p > 0 else None
    usual = torch.ones(H, dtype=torch.bool, device="cuda")
    usual[7] = usual[11] = False                            # gamma == 0 and |gamma| = 0.03: looked at separately below
    for i, nm in enumerate(("dz", "dx", "dgamma", "dbeta", "dxsum")):
        a_z, a_y = out["z"][i].float(), out["y"][i].float()
        ref = {"dz": zr.grad, "dgamma": g.grad, "dbeta": b.grad}.get(nm, a_z)          # dx / dxsum: same mask, the two forms against each other
        sel = (lambda t: t[usual]) if nm in ("dgamma", "dbeta", "dxsum") else (lambda t: t[:, usual])
        scale = sel(ref).abs().max().item() + 1e-6
        e_z, e_y = (sel(a_z) - sel(ref)).abs().max().item() / scale, (sel(a_y) - sel(ref)).abs().max().item() / scale
        print(f"  {nm}: relative max error stored-sum form {e_z:.2e}, from-output form {e_y:.2e}")
        assert e_y < 2.0 * e_z + 1.2e-2, (nm, e_z, e_y)
    assert float(out["y"][2][7]) == 0.0                     # gamma == 0: the output says nothing about xhat, the channel's d(gamma) is reported as 0
    sc = g.grad.abs().max().item()
    assert abs(float(out["y"][2][11]) - float(g.grad[11])) < 0.15 * sc       # |gamma| = 0.03: the rounding of y is amplified 1 / |gamma| times
    if p > 0:
        assert torch.equal(out["y"][1].float() != 0, keep) or ((out["y"][1].float() != 0) ^ keep).float().mean().item() < 1e-3   # same dropout mask (zeros of dz aside)


def test_layernorm_dropout_masks_match(ops):
    rows, H, p = 256, 768, 0.1
    x = torch.ones(rows, H, dtype=BF, device="cuda")
    gamma, beta = torch.ones(H, device="cuda"), torch.zeros(H, device="cuda")
    seed = torch.tensor([42], dtype=torch.int64, device="cuda")
    y, z = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    ops.ln_fwd(x, None, gamma, beta, y, zout=z, mean=mean, rstd=rstd, dropout_p=p, seed=seed, salt=5)
    keep = z.float() != 0
    assert abs(1 - keep.float().mean().item() - p) < 0.01
    assert torch.allclose(z.float()[keep], torch.full_like(z.float()[keep], 1 / (1 - p)), atol=1e-2)
    dy = rnd(rows, H, seed=54)
    dz, dx = torch.empty_like(x), torch.empty_like(x)
    dxs = torch.zeros(H, device="cuda")
    ops.ln_bwd(dy, z, mean, rstd, gamma, dz, dx=dx, dropout_p=p, seed=seed, salt=5, dxsum=dxs)
    close(dxs, dx.float().sum(0), 2e-2, 1e-3, "dxsum with dropout")
    assert ((dx.float() != 0) & ~keep).sum().item() == 0            # dropped inputs get no gradient
    close(dx.float()[keep], dz.float()[keep] / (1 - p), 1e-2, 1e-2, "dropout dx")


def test_layernorm_backward_fast_path_equals_general_path(ops):
    """The all-outputs training combination has its own instantiation (rowops.hip ln_bwd_kernel<3, true, true>); a zero second
    gradient forces the general one: same masks, same values, same column sums."""
    rows, H, p = 1237, 768, 0.1
    x, res = rnd(rows, H, seed=60), rnd(rows, H, seed=61)
    gamma, beta = (1 + 0.1 * torch.randn(H)).cuda(), (0.1 * torch.randn(H)).cuda()
    seed = torch.tensor([7], dtype=torch.int64, device="cuda")
    y, z = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    ops.ln_fwd(x, res, gamma, beta, y, zout=z, mean=mean, rstd=rstd, dropout_p=p, seed=seed, salt=9)
    dy = rnd(rows, H, seed=62)
    out = []
    for dy2 in (None, torch.zeros_like(dy)):
        dz, dx = torch.empty_like(x), torch.empty_like(x)
        dg, db, dxs = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
        ops.ln_bwd(dy, z, mean, rstd, gamma, dz, dy2=dy2, dx=dx, dgamma=dg, dbeta=db, dropout_p=p, seed=seed, salt=9, dxsum=dxs)
        out.append((dz, dx, dg, db, dxs))
    for a, b, nm in zip(out[0], out[1], ("dz", "dx", "dgamma", "dbeta", "dxsum")):
        # dz / dx may differ by one bf16 ulp where the fma contraction differs; the column sums inherit a few of those
        close(a, b, 2e-3 if nm in ("dz", "dx") else 5e-2, 1e-2, "fast vs general " + nm)
    assert torch.equal(out[0][1] != 0, out[1][1] != 0)
    # the forward's mask: dropped elements of x have z == res exactly
    dropped = (out[0][1].float() == 0) & (out[0][0].float() != 0)
    assert abs(dropped.float().mean().item() - p) < 0.01
    assert torch.equal(z[dropped], res[dropped])


def test_layernorm_dropout_masks_differ_between_rows_steps_and_sites(ops):
    rows, H, p = 512, 768, 0.5
    x = torch.ones(rows, H, dtype=BF, device="cuda")
    gamma, beta = torch.ones(H, device="cuda"), torch.zeros(H, device="cuda")

    def mask(seed, salt):
        z, y = torch.empty_like(x), torch.empty_like(x)
        ops.ln_fwd(x, None, gamma, beta, y, zout=z, dropout_p=p, seed=torch.tensor([seed], dtype=torch.int64, device="cuda"), salt=salt)
        return (z.float() != 0).float()
    m0, m1, m2 = mask(100, 3), mask(101, 3), mask(100, 4)
    assert abs(m0.mean().item() - 0.5) < 0.01
    for a, b in ((m0, m1), (m0, m2), (m0[:-1], m0[1:]), (m0[:, :-1], m0[:, 1:]), (m0[:, :-2], m0[:, 2:])):
        agree = (a == b).float().mean().item()
        assert abs(agree - 0.5) < 0.01, agree
    assert abs(m0.mean(0) - 0.5).max().item() < 0.12 and abs(m0.mean(1) - 0.5).max().item() < 0.1


# ------------------------------------------------------------------------------------------ embeddings
def test_text_embedding_fwd_bwd(ops):
    nseq, L, H, V = 6, 24, 128, 300
    ids = torch.randint(0, V, (nseq, L))
    ids[:, -5:] = 0
    word, pos, typ = torch.randn(V, H).cuda(), torch.randn(512, H).cuda(), torch.randn(2, H).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(H)).cuda(), (0.1 * torch.randn(H)).cuda()
    idc = ids.int().cuda()
    y = torch.empty(nseq * L, H, dtype=BF, device="cuda")
    z = torch.empty_like(y)
    mean, rstd = torch.empty(nseq * L, device="cuda"), torch.empty(nseq * L, device="cuda")
    ops.embed_ln_fwd(0, y, nseq=nseq, L=L, H=H, pos=pos, type0=typ[0], gamma=gamma, beta=beta, ids=idc, word=word, zout=z,
                     mean=mean, rstd=rstd)
    w, pp, tt = word.clone().requires_grad_(True), pos.clone().requires_grad_(True), typ.clone().requires_grad_(True)
    e = torch.nn.functional.embedding(ids.cuda(), w, padding_idx=0) + tt[0] + pp[:L]
    yr = torch.nn.functional.layer_norm(e, (H,), gamma, beta, 1e-12)
    close(y.view(nseq, L, H), yr, 2e-2, 1e-2, "embed fwd")
    dz = rnd(nseq * L, H, seed=60)
    e.backward(dz.float().view(nseq, L, H))
    dword, dpos, dtyp = torch.zeros_like(word), torch.zeros_like(pos), torch.zeros(H, device="cuda")
    ops.embed_bwd(0, dz, nseq=nseq, L=L, H=H, dpos=dpos, dtype0=dtyp, ids=idc, dword=dword)
    close(dword, w.grad, 1e-3, 1e-4, "dword")
    close(dpos, pp.grad, 1e-3, 1e-4, "dpos")
    close(dtyp, tt.grad[0], 1e-2, 1e-4, "dtype")
    assert dword[0].abs().max().item() == 0.0      # padding_idx


def test_pv_embedding_fwd_bwd(ops):
    B, H, Lp = 5, 128, 54
    x = torch.randn(B, 53).cuda()
    m = torch.bernoulli(torch.full((B, 53), 0.5)).cuda()
    w, b, cls, mt = [torch.randn(H).cuda().requires_grad_(True) for _ in range(4)]
    pos, typ = torch.randn(512, H).cuda().requires_grad_(True), torch.randn(2, H).cuda().requires_grad_(True)
    gamma, beta = (1 + 0.1 * torch.randn(H)).cuda(), (0.1 * torch.randn(H)).cuda()
    nseq = 2 * B                                    # P1 | P11 share the source batch (src_mod = B)
    y = torch.empty(nseq * Lp, H, dtype=BF, device="cuda")
    z = torch.empty_like(y)
    mean, rstd = torch.empty(nseq * Lp, device="cuda"), torch.empty(nseq * Lp, device="cuda")
    ops.embed_ln_fwd(1, y, nseq=nseq, L=Lp, H=H, pos=pos.detach(), type0=typ.detach()[0], gamma=gamma, beta=beta,
                     pv_x=x, pv_mask=m, pv_w=w.detach(), pv_b=b.detach(), pv_cls=cls.detach(), pv_masktok=mt.detach(),
                     src_mod=B, zout=z, mean=mean, rstd=rstd)
    feat = x[:, :, None] * w + b
    masked = feat * (1 - m[:, :, None]) + mt * m[:, :, None]
    props = torch.cat([cls.expand(B, 1, H), masked], dim=1).repeat(2, 1, 1)
    e = props + typ[0] + pos[:Lp]
    yr = torch.nn.functional.layer_norm(e, (H,), gamma, beta, 1e-12)
    close(y.view(nseq, Lp, H), yr, 2e-2, 1e-2, "pv embed fwd")
    dz = rnd(nseq * Lp, H, seed=61)
    e.backward(dz.float().view(nseq, Lp, H))
    d = {k: torch.zeros(H, device="cuda") for k in ("w", "b", "cls", "mt", "typ")}
    dpos = torch.zeros(512, H, device="cuda")
    ops.embed_bwd(1, dz, nseq=nseq, L=Lp, H=H, dpos=dpos, dtype0=d["typ"], pv_x=x, pv_mask=m, src_mod=B, d_w=d["w"],
                  d_b=d["b"], d_cls=d["cls"], d_masktok=d["mt"])
    for got, ref, nm in ((d["w"], w.grad, "dw"), (d["b"], b.grad, "db"), (d["cls"], cls.grad, "dcls"),
                         (d["mt"], mt.grad, "dmask"), (d["typ"], typ.grad[0], "dtype"), (dpos, pos.grad, "dpos")):
        close(got, ref, 2e-3 * max(1, ref.abs().max().item()), 1e-4, nm)


# ------------------------------------------------------------------------------------- layout helpers
def test_transpose_cast_gather_acc(ops):
    R, C = 216, 300
    big = rnd(R, C + 20, seed=70)
    x = big[:, 10:10 + C]
    Rpad = 256
    out = torch.full((C, Rpad), 9.0, dtype=BF, device="cuda")
    cs = torch.zeros(C, device="cuda")
    ops.transpose_bf16(x, out, colsum=cs)
    assert torch.equal(out[:, :R], x.t())
    assert out[:, R:].abs().max().item() == 0
    close(cs, x.float().sum(0), 1e-3, 1e-5, "colsum")
    w = torch.randn(130, 70).cuda()
    o, oT = torch.empty(130, 70, dtype=BF, device="cuda"), torch.empty(70, 130, dtype=BF, device="cuda")
    ops.cast_transpose(w, o, oT)
    assert torch.equal(o, w.to(BF)) and torch.equal(oT, w.to(BF).t())
    f = torch.randn(1000).cuda()
    ob = torch.empty(1000, dtype=BF, device="cuda")
    ops.cast_f32_bf16(f, ob)
    assert torch.equal(ob, f.to(BF))
    back = torch.empty(1000, device="cuda")
    ops.cast_bf16_f32(ob, back)
    assert torch.equal(back, ob.float())
    src = rnd(10, 128, seed=71)
    idx = torch.tensor([3, 3, 9, 0, 1], device="cuda")
    dst = torch.empty(5, 128, dtype=BF, device="cuda")
    ops.gather_rows(dst, src, idx)
    assert torch.equal(dst, src[idx])
    acc = torch.ones(10, 128, device="cuda")
    ops.acc_rows(acc, dst, idx=idx, atomic=True)
    ref = torch.ones(10, 128, device="cuda").index_add_(0, idx, dst.float())
    close(acc, ref, 1e-5, 1e-6, "scatter add")
    ops.acc_rows(acc, src)
    close(acc, ref + src.float(), 1e-5, 1e-6, "acc")


# ------------------------------------------------------------------------------------------ loss side
def test_l2norm_and_split(ops):
    rows, E, H = 16, 256, 768
    big = torch.randn(rows, E + 8).cuda()
    x = big[:, :E]
    y, nrm = torch.empty(rows, E, device="cuda"), torch.empty(rows, device="cuda")
    a3, w3 = torch.empty(rows, 3 * E, dtype=BF, device="cuda"), torch.empty(rows, 3 * E, dtype=BF, device="cuda")
    yT = torch.zeros(E, 64, dtype=BF, device="cuda")
    ops.l2norm_fwd(x, y, nrm, a3=a3, w3=w3, yT=yT)
    xr = x.clone().requires_grad_(True)
    yr = torch.nn.functional.normalize(xr, dim=-1)
    close(y, yr, 1e-6, 1e-5, "normalize")
    # split-bf16 product reproduces the fp32 dot products to ~1e-5
    sim = torch.empty(rows, rows, device="cuda")
    ops.gemm_nt(a3, w3, sim, epi=ops.EPI_F32)
    close(sim, yr.detach() @ yr.detach().t(), 3e-5, 0, "split-bf16 sim")
    assert torch.equal(yT[:, :rows], y.to(BF).t())
    dy = torch.randn(rows, E).cuda()
    yr.backward(dy)
    dx = torch.empty(rows, E, dtype=BF, device="cuda")
    gs = torch.tensor([0.5], device="cuda")
    ops.l2norm_bwd(dy, y, nrm, dx, gscale=gs)
    close(dx, 0.5 * xr.grad, 1e-3, 1e-2, "normalize bwd")


def test_ita_rows(ops):
    B, Q = 8, 100
    J = B + Q
    Jpad = 128
    temp = torch.tensor([0.07], device="cuda")
    alpha = torch.tensor([0.4], device="cuda")
    raw = (torch.randn(2 * B, J) * 0.3).cuda()
    rawm = (torch.randn(2 * B, J) * 0.3).cuda()
    S, SM = raw / temp, rawm / temp
    dS = torch.empty(2 * B, Jpad, dtype=BF, device="cuda")
    losses, dtemp = torch.zeros(8, device="cuda"), torch.zeros(1, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.ita_rows(S, SM, dS, B=B, J=J, alpha=alpha, temp=temp, losses=losses, slot=2, dtemp=dtemp, nan_flag=flag)
    t = temp.clone().requires_grad_(True)
    r = raw.clone().requires_grad_(True)
    s = r / t
    tgt = torch.zeros(2 * B, J, device="cuda")
    tgt[torch.arange(2 * B), torch.arange(2 * B) % B] = 1
    tg = 0.4 * torch.softmax(SM, dim=1) + 0.6 * tgt
    loss = (-(torch.log_softmax(s, dim=1) * tg).sum(1)).view(2, B).mean(1).sum() / 2
    loss.backward()
    assert abs(losses[2].item() - loss.item()) < 2e-4 * abs(loss.item())
    close(dS[:, :J].float() / 0.07, r.grad, 2e-4, 1e-2, "dS")
    assert dS[:, J:].abs().max().item() == 0
    assert abs(dtemp.item() - t.grad.item()) < 2e-3 * abs(t.grad.item())
    assert flag.item() == 0


def test_sample_neg_distribution_and_forced(ops):
    B = 16
    S = (torch.randn(B, B + 40) * 2).cuda()
    out = torch.zeros(B, dtype=torch.int64, device="cuda")
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(B, B)
    n = 400
    for i in range(n):
        seed.fill_(i * 7919 + 1)
        ops.sample_neg(S, B, out, seed=seed, salt=3)
        o = out.cpu()
        assert (o != torch.arange(B)).all() and (o >= 0).all() and (o < B).all()
        counts[torch.arange(B), o] += 1
    w = torch.softmax(S[:, :B].cpu(), dim=1)
    w.fill_diagonal_(0)
    w = w / w.sum(1, keepdim=True)
    assert (counts / n - w).abs().max().item() < 0.12
    forced = torch.arange(B, device="cuda").roll(1)
    ops.sample_neg(S, B, out, forced=forced, offset=B)
    assert torch.equal(out, forced + B)


def test_lm_loss(ops):
    nseq, L, V, Vpad = 5, 12, 300, 320
    ids = torch.randint(1, V, (nseq, L))
    ids[2, 7:] = 0
    ids[4, 3:] = 0
    logits = torch.randn(nseq * L, V).cuda()
    logits_m = torch.randn(nseq * L, V).cuda()
    alpha = torch.tensor([0.3], device="cuda")
    losses = torch.zeros(8, device="cuda")
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    dl = torch.full((nseq * L, Vpad), 5.0, dtype=BF, device="cuda")
    gs = torch.tensor([2.0], device="cuda")
    ops.lm_loss(logits, logits_m, ids.int().cuda(), nseq=nseq, L=L, V=V, alpha=alpha, ws=ws, losses=losses, slot=0,
                dlogits=dl, gscale=gs)
    x = logits.view(nseq, L, V).clone().requires_grad_(True)
    out = x[:, :-1]
    lm = logits_m.view(nseq, L, V)[:, :-1]
    labels = ids[:, 1:].cuda()
    ce = torch.nn.functional.cross_entropy(out.permute(0, 2, 1), labels)
    dist = -(torch.log_softmax(out, -1) * torch.softmax(lm, -1)).sum(-1)
    loss = 0.7 * ce + 0.3 * dist[labels != 0].mean()
    (2.0 * loss).backward()
    assert abs(losses[0].item() - loss.item()) < 1e-4
    close(dl.view(nseq, L, Vpad)[:, :, :V], x.grad, 1e-5, 1e-2, "dlogits")
    assert dl[:, V:].abs().max().item() == 0


def test_itm_and_mpm_heads(ops):
    B, H = 6, 128
    n = 3 * B
    La, Lb = 54, 20
    xa, xb = rnd(n * La, H, seed=80), rnd(n * Lb, H, seed=81)
    W, bias = (torch.randn(2, 2 * H) * 0.1).cuda(), torch.randn(2).cuda()
    losses = torch.zeros(8, device="cuda")
    dxa, dxb = torch.zeros_like(xa), torch.zeros_like(xb)
    dW, db = torch.zeros_like(W), torch.zeros_like(bias)
    logits = torch.empty(n, 2, device="cuda")
    ops.itm_head(xa, La * H, xb, Lb * H, H, W, bias, n=n, B=B, losses=losses, slot=3, logits=logits, dxa=dxa, dxb=dxb, dW=dW, db=db)
    a = xa.float().view(n, La, H)[:, 0].clone().requires_grad_(True)
    b2 = xb.float().view(n, Lb, H)[:, 0].clone().requires_grad_(True)
    Wr, br = W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    lg = torch.cat([a, b2], -1) @ Wr.t() + br
    lab = torch.cat([torch.ones(B), torch.zeros(2 * B)]).long().cuda()
    loss = torch.nn.functional.cross_entropy(lg, lab)
    loss.backward()
    assert abs(losses[3].item() - loss.item()) < 1e-4
    close(logits, lg, 1e-3, 1e-4, "itm logits")
    close(dxa.view(n, La, H)[:, 0], a.grad, 1e-4, 1e-2, "itm dxa")
    close(dxb.view(n, Lb, H)[:, 0], b2.grad, 1e-4, 1e-2, "itm dxb")
    assert dxa.view(n, La, H)[:, 1:].abs().max().item() == 0
    close(dW, Wr.grad, 1e-4, 1e-3, "itm dW")
    close(db, br.grad, 1e-5, 1e-3, "itm db")
    # MPM
    Lp = 54
    h = rnd(B * Lp, H, seed=82)
    w3, b3 = (torch.randn(H) * 0.1).cuda(), torch.randn(1).cuda()
    target = torch.randn(B, 53).cuda()
    mask = torch.bernoulli(torch.full((B, 53), 0.5)).cuda()
    ws = torch.zeros(4, dtype=torch.int32, device="cuda")
    dh = torch.full_like(h, 3.0)
    dw, dbb = torch.zeros_like(w3), torch.zeros_like(b3)
    pred = torch.zeros(B, 53, device="cuda")
    ops.mpm_head(h, Lp, H, w3, b3, target, mask, B=B, ws=ws, losses=losses, slot=1, pred=pred, dh=dh, dw=dw, db=dbb)
    hr = h.float().view(B, Lp, H).clone().requires_grad_(True)
    wr, brr = w3.clone().requires_grad_(True), b3.clone().requires_grad_(True)
    pr = (hr[:, :-1] @ wr) + brr
    keep = mask == 0
    lossm = torch.nn.functional.mse_loss(pr[keep], target[keep]) * 5
    lossm.backward()
    assert abs(losses[1].item() - lossm.item()) < 1e-4 * max(1, lossm.item())
    close(pred, pr, 1e-3, 1e-4, "mpm pred")
    close(dh.view(B, Lp, H), hr.grad, 1e-4 * hr.grad.abs().max().item() + 1e-6, 1e-2, "mpm dh")
    close(dw, wr.grad, 1e-3 * wr.grad.abs().max().item(), 1e-3, "mpm dw")
    close(dbb, brr.grad, 1e-4, 1e-3, "mpm db")


def test_enqueue_and_shadows(ops):
    E, Q, B, n = 64, 32, 4, 8
    queue = torch.nn.functional.normalize(torch.randn(E, Q), dim=0).cuda()
    ldt = 64
    w3 = torch.zeros(B + Q, 3 * E, dtype=BF, device="cuda")
    qT = torch.zeros(E, ldt, dtype=BF, device="cuda")
    ops.queue_shadow(queue, w3, qT, Bloc=B)
    assert torch.equal(qT[:, B:B + Q], queue.to(BF))
    hi = queue.t().to(BF)
    assert torch.equal(w3[B:, :E], hi) and torch.equal(w3[B:, 2 * E:], (queue.t() - hi.float()).to(BF))
    ptr = torch.tensor([24], device="cuda")
    ref = queue.clone()
    for _ in range(2):                      # second call wraps around
        feats = torch.nn.functional.normalize(torch.randn(n, E), dim=1).cuda()
        p0 = int(ptr.item())
        ops.enqueue(feats, queue, w3, qT, ptr, Bloc=B)
        ref[:, p0:p0 + n] = feats.t()
        assert int(ptr.item()) == (p0 + n) % Q
        assert torch.equal(queue, ref) and torch.equal(qT[:, B:B + Q], ref.to(BF)) and torch.equal(w3[B:, :E], ref.t().to(BF))


# ------------------------------------------------------------------------------------------ optimiser
def test_adamw_clip_ema_match_torch(ops):
    n = 4096 * 3 + 64
    p0 = torch.randn(n)
    p = p0.clone().cuda()
    pr = p0.clone().cuda().requires_grad_(True)
    opt = torch.optim.AdamW([pr], lr=1e-3, weight_decay=0.02)
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    shadow = torch.zeros(n, dtype=BF, device="cuda")
    lr = torch.tensor([1e-3], device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    scal = torch.zeros(ops.adam_scalars_bytes() // 4, device="cuda")
    for it in range(4):
        g = torch.randn(n).cuda() * (10.0 if it % 2 == 0 else 0.01)     # clipped and un-clipped steps
        nsq = torch.zeros(1, device="cuda")
        ops.grad_sqnorm(g, nsq)
        assert abs(nsq.item() - (g.double() ** 2).sum().item()) < 1e-3 * nsq.item()
        ops.adamw_step(p, g, m, v, shadow, lr=lr, normsq=nsq, step=step, scalars=scal)
        pr.grad = g.clone()
        gn = torch.nn.utils.clip_grad_norm_([pr], 5.0)
        opt.step()
        assert abs(scal[4].item() - gn.item()) < 1e-3 * gn.item()
        close(p, pr.detach(), 1e-6, 1e-5, f"adamw step {it}")
        assert torch.equal(shadow, p.to(BF))
    assert step.item() == 4
    # non-finite gradient: nothing moves
    before = p.clone()
    g = torch.full((n,), float("nan"), device="cuda")
    nsq = torch.zeros(1, device="cuda")
    ops.grad_sqnorm(g, nsq)
    ops.adamw_step(p, g, m, v, shadow, lr=lr, normsq=nsq, step=step, scalars=scal)
    assert torch.equal(p, before) and step.item() == 4
    pm = torch.randn(n).cuda()
    ref = pm * 0.995 + p * 0.005
    ops.ema_update(pm, p, shadow, 0.995)
    close(pm, ref, 1e-6, 1e-6, "ema")
    assert torch.equal(shadow, pm.to(BF))


@pytest.mark.parametrize("R,nH,Lkv,Lmax,kv_div,group", [(10, 2, 1, 16, 0, 1), (15, 12, 37, 64, 0, 5), (20, 12, 54, 54, 5, 5), (64, 4, 130, 160, 0, 4),
                                                    (6, 2, 256, 256, 3, 3), (35, 12, 9, 16, 0, 7), (12, 4, 70, 80, 0, 2), (18, 2, 33, 40, 0, 6),
                                                    (500, 12, 100, 100, 0, 5), (12, 2, 54, 54, 6, 6), (12, 2, 200, 256, 0, 6), (16, 2, 40, 48, 0, 8),
                                                    (16, 2, 54, 54, 8, 8), (10, 3, 17, 32, 0, 5)])
@pytest.mark.parametrize("coalesced", [False, True, "pairs"])
def test_decode_attention_over_kv_cache(ops, R, nH, Lkv, Lmax, kv_div, group, coalesced):
    """Single-query attention against a cache addressed through the beam ancestry table (kv_div == 0) or shared per molecule
    (kv_div > 0), vs fp32 torch on the same bf16 inputs (xbert.py:305-354 for the last position).  Groups of 2-8 beams run on the
    one-wave-per-(molecule, head) MFMA kernel, which loads a key row once for all beams whose ancestor at that position is the same cache
    row: `coalesced` makes the beams of a molecule share their ancestors except at the last six positions (what beam search produces);
    "pairs" additionally lets beams 2k and 2k+1 share their rows in that tail (distinct rows < beams: one key per distinct row, read by
    both); the plain case gives every beam unrelated ancestors everywhere (group x Lkv keys per molecule)."""
    if coalesced and (kv_div or group == 1):
        pytest.skip("ancestry tables only")
    H = nH * 64
    g = torch.Generator().manual_seed(R + Lkv)
    q = (torch.randn(R, 3 * H, generator=g)).to(BF).cuda()                     # strided view like the fused QKV output
    nseq = R if kv_div == 0 else (R + kv_div - 1) // kv_div
    wide = 2 * H if kv_div else H                                               # cross K/V live side by side in one buffer
    cache = torch.randn(nseq, Lmax, wide, generator=g).to(BF).cuda()
    Kc = cache[:, :, :H]
    Vc = cache[:, :, H:] if kv_div else torch.randn(nseq, Lmax, H, generator=g).to(BF).cuda()
    anc = None if kv_div else torch.randint(0, R, (R, Lmax), generator=g).to(torch.int32).cuda()
    if coalesced and R % group == 0:
        lead = anc.view(R // group, group, Lmax)[:, :1, :].expand(R // group, group, Lmax).reshape(R, Lmax)
        old = torch.arange(Lmax, device="cuda")[None, :] < max(Lkv - 6, 0)
        if coalesced == "pairs":
            even = anc.view(R // group, group, Lmax)[:, (torch.arange(group) // 2 * 2).tolist(), :].reshape(R, Lmax)
            anc = even
        anc = torch.where(old, lead, anc).contiguous()
    out = torch.zeros(R, H, dtype=BF, device="cuda")
    ops.decode_attn(q[:, :H], Kc, Vc, out, nH=nH, Lkv=Lkv, seq_stride=Lmax * wide, tok_stride=wide, anc=anc, kv_div=max(kv_div, 1), group=group)
    j = torch.arange(Lkv, device="cuda")
    seq = anc[:, :Lkv].long() if kv_div == 0 else (torch.arange(R, device="cuda") // kv_div)[:, None].expand(R, Lkv)
    K = Kc.float()[seq, j[None, :]].view(R, Lkv, nH, 64)
    V = Vc.float()[seq, j[None, :]].view(R, Lkv, nH, 64)
    s = torch.einsum("rhd,rjhd->rhj", q[:, :H].float().view(R, nH, 64), K) * 0.125
    ref = torch.einsum("rhj,rjhd->rhd", torch.softmax(s, -1), V).reshape(R, H)
    close(out.float(), ref, 2e-2, 2e-2, "decode_attn")


@pytest.mark.parametrize("R,nH,Lkv,Lmax,group,tail", [(500, 12, 100, 100, 5, 6), (5000, 12, 60, 103, 5, 6), (64, 4, 130, 160, 4, 0)])
def test_decode_attention_is_stable_over_repeated_launches(ops, R, nH, Lkv, Lmax, group, tail):
    """Race screen (tools/stress_decode_attn.py in small): the kernel streams keys and values through an LDS-DMA ring behind counted waits --
    a first version that loaded keys into registers was wrong on 1-100 % of the launches depending on the shape.  Six random ancestry tables
    per shape against fp32 torch, and every launch repeated: bit-identical."""
    H = nH * 64
    for trial in range(6):
        g = torch.Generator().manual_seed(1000 * trial + R + Lkv)
        q = torch.randn(R, H, generator=g).to(BF).cuda()
        Kc = torch.randn(R, Lmax, H, generator=g).to(BF).cuda()
        Vc = torch.randn(R, Lmax, H, generator=g).to(BF).cuda()
        anc = torch.randint(0, R, (R, Lmax), generator=g).to(torch.int32).cuda()
        if tail:
            lead = anc.view(R // group, group, Lmax)[:, :1, :].expand(R // group, group, Lmax).reshape(R, Lmax)
            old = torch.arange(Lmax, device="cuda")[None, :] < max(Lkv - tail, 0)
            anc = torch.where(old, lead, anc).contiguous()
        out = [torch.zeros(R, H, dtype=BF, device="cuda") for _ in range(2)]
        for o in out:
            ops.decode_attn(q, Kc, Vc, o, nH=nH, Lkv=Lkv, seq_stride=Lmax * H, tok_stride=H, anc=anc, group=group)
        assert torch.equal(out[0], out[1]), trial
        j = torch.arange(Lkv, device="cuda")
        seq = anc[:, :Lkv].long()
        K = Kc.float()[seq, j[None, :]].view(R, Lkv, nH, 64)
        V = Vc.float()[seq, j[None, :]].view(R, Lkv, nH, 64)
        sc = torch.einsum("rhd,rjhd->rhj", q.float().view(R, nH, 64), K) * 0.125
        ref = torch.einsum("rhj,rjhd->rhd", torch.softmax(sc, -1), V).reshape(R, H)
        close(out[0].float(), ref, 2e-2, 2e-2, f"decode_attn trial {trial}")


@pytest.mark.parametrize("R,nH,Lkv,Lmax,group", [(15, 12, 37, 64, 5), (10, 2, 1, 16, 1), (35, 4, 9, 16, 7), (500, 12, 100, 103, 5), (12, 2, 54, 64, 6)])
@pytest.mark.parametrize("head_major", [False, True])
def test_decode_attention_writes_the_newest_position_into_the_cache(ops, R, nH, Lkv, Lmax, group, head_major):
    """With knew / vnew the launch takes the newest position's key / value from the projection output (a strided view of QKV) and writes
    them into the cache itself (one copy launch in front of the attention kernel): the output equals the copy-then-attend sequence, the
    cache afterwards holds the new rows at position Lkv - 1 and nothing else changed.  head_major: the decoder's cache layout
    [R, nH, Lmax, 64] (tok_stride 64, head_stride Lmax * 64) against the same data in token-major rows [R, Lmax, H]."""
    H = nH * 64
    g = torch.Generator().manual_seed(R * 7 + Lkv)
    qkv = torch.randn(R, 3 * H, generator=g).to(BF).cuda()
    Kt, Vt = torch.randn(R, Lmax, H, generator=g).to(BF).cuda(), torch.randn(R, Lmax, H, generator=g).to(BF).cuda()      # token-major truth
    anc = torch.randint(0, R, (R, Lmax), generator=g).to(torch.int32).cuda()
    anc[:, Lkv - 1:] = torch.arange(R, dtype=torch.int32, device="cuda")[:, None]           # the newest position is the row's own
    K2, V2 = Kt.clone(), Vt.clone()
    K2[:, Lkv - 1] = qkv[:, H:2 * H]
    V2[:, Lkv - 1] = qkv[:, 2 * H:]
    want = torch.zeros(R, H, dtype=BF, device="cuda")
    ops.decode_attn(qkv[:, :H], K2, V2, want, nH=nH, Lkv=Lkv, seq_stride=Lmax * H, tok_stride=H, anc=anc, group=group)

    def lay(x):          # [R, Lmax, H] -> the layout under test
        return x.view(R, Lmax, nH, 64).permute(0, 2, 1, 3).contiguous() if head_major else x.clone()

    def back(x):
        return x.permute(0, 2, 1, 3).reshape(R, Lmax, H) if head_major else x

    strides = dict(seq_stride=Lmax * H, tok_stride=64, head_stride=Lmax * 64) if head_major else dict(seq_stride=Lmax * H, tok_stride=H)
    Kc, Vc = lay(Kt), lay(Vt)
    got = torch.zeros(R, H, dtype=BF, device="cuda")
    ops.decode_attn(qkv[:, :H], Kc, Vc, got, nH=nH, Lkv=Lkv, anc=anc, group=group, knew=qkv[:, H:2 * H], vnew=qkv[:, 2 * H:], **strides)
    assert torch.equal(got, want)
    assert torch.equal(back(Kc), K2) and torch.equal(back(Vc), V2)
    # the same through a device-resident position (graph replay)
    K3 = K2.clone()
    K3[:, Lkv - 1] = 0
    Kc3, Vc3 = lay(K3), lay(V2)
    t_dev = torch.tensor([Lkv - 1], dtype=torch.int32, device="cuda")
    got3 = torch.zeros(R, H, dtype=BF, device="cuda")
    ops.decode_attn(qkv[:, :H], Kc3, Vc3, got3, nH=nH, Lkv=Lmax, anc=anc, group=group, t_ptr=t_dev, knew=qkv[:, H:2 * H], vnew=qkv[:, 2 * H:], **strides)
    assert torch.equal(got3, want) and torch.equal(back(Kc3), K2)


def test_decode_attention_rejects_bad_arguments(ops):
    q = torch.zeros(4, 128, dtype=BF, device="cuda")
    kv = torch.zeros(4, 300, 128, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError):
        ops.decode_attn(q, kv, kv, q.clone(), nH=2, Lkv=300, seq_stride=300 * 128, tok_stride=128, kv_div=1)
    with pytest.raises(RuntimeError):
        ops.decode_attn(q, kv, kv, q.clone(), nH=2, Lkv=8, seq_stride=300 * 128 + 4, tok_stride=128, kv_div=1)


def test_embed_step_matches_full_embedding(ops):
    """Embedding one token at position t equals row t of the whole-sequence embedding kernel (same arithmetic, bit-exact)."""
    H, V, L, n = 256, 50, 12, 9
    g = torch.Generator().manual_seed(3)
    word, pos, typ = (torch.randn(s, H, generator=g).cuda() for s in (V, 32, 2))
    gamma, beta = torch.rand(H, generator=g).cuda() + 0.5, torch.randn(H, generator=g).cuda()
    ids = torch.randint(1, V, (n, L), generator=g).to(torch.int32).cuda()
    full = torch.empty(n * L, H, dtype=BF, device="cuda")
    ops.embed_ln_fwd(0, full, nseq=n, L=L, H=H, pos=pos, type0=typ, gamma=gamma, beta=beta, ids=ids, word=word)
    for t in (0, 5, 11):
        y = torch.empty(n, H, dtype=BF, device="cuda")
        ops.embed_step_ln_fwd(ids[:, t].contiguous(), t, y, word=word, pos=pos, type0=typ, gamma=gamma, beta=beta)
        assert torch.equal(y, full.view(n, L, H)[:, t])


@pytest.mark.parametrize("N,k,V", [(37, 5, 300), (9, 8, 300), (20, 1, 70), (6, 3, 500)])
def test_beam_step_kernel_matches_tensor_bookkeeping(N, k, V):
    """csrc/decode.hip::beam_step_kernel (one launch per decode position) against decode.BeamBook.update + CachedDecoder.reorder (the
    tensor-op form of d_pv2smiles_batched.py:36-50) on random logits in which [SEP] is a frequent top-k member: same finals in the same
    slots, same survivors, token histories, scores, ancestry table and tokens to feed, position by position until every molecule is done."""
    from spmm_amd import decode
    T = 16
    L, R = T + 3, N * k
    g = torch.Generator().manual_seed(3)
    ref, fus = decode.BeamBook(N, k, T, "cuda"), decode.BeamBook(N, k, T, "cuda", fused=True)
    v0, i0 = torch.randn(N, k, generator=g).cuda(), torch.randint(4, V, (N, k), generator=g).cuda()
    ref.first(v0, i0)
    fus.first(v0, i0)
    rows = torch.arange(R, dtype=torch.int32, device="cuda")
    anc_ref = rows[:, None].repeat(1, L).contiguous()
    anc_fus = anc_ref.clone()
    n_fin = 0
    for s in range(T):
        logits = torch.randn(R, V, generator=g) * 2.0
        boost = torch.rand(R, generator=g) < 0.12
        logits[:, decode.SEP_ID] += torch.where(boost, torch.full((R,), 6.0), torch.full((R,), -2.0))
        logits = logits.cuda()
        was_done = ref.done.clone()
        values, indices = decode._pick(torch.softmax(logits.view(N, k, -1), dim=-1), k, False)
        parent, tok = ref.update(values, indices)
        anc_ref = anc_ref.view(N, k, L).gather(1, parent[:, :, None].expand(N, k, L).long()).reshape(R, L).contiguous()
        anc_ref[:, s + 2:] = rows[:, None]
        ids = fus.step_fused(logits, anc_fus)
        live = ~ref.done
        assert torch.equal(fus.done, ref.done) and int(fus.n_done) == int(ref.done.sum()), s
        assert torch.equal(fus.fin_n.long(), ref.fin_n), s
        assert torch.equal(fus.tokens.long(), ref.tokens), s
        torch.testing.assert_close(fus.cur_p, ref.cur_p, rtol=0, atol=2e-5)
        F = ref.F
        fp_f, fp_r = fus.fin_p[:, :F], ref.fin_p[:, :F]
        assert torch.equal(torch.isinf(fp_f), torch.isinf(fp_r)), s
        torch.testing.assert_close(torch.where(torch.isinf(fp_f), torch.zeros_like(fp_f), fp_f), torch.where(torch.isinf(fp_r), torch.zeros_like(fp_r), fp_r),
                                   rtol=0, atol=2e-5)
        used = torch.arange(F, device="cuda")[None, :] < ref.fin_n[:, None]
        assert torch.equal(fus.fin_len[:, :F].long()[used], ref.fin_len[:, :F][used]), s
        assert torch.equal(fus.fin_tok[:, :F].long()[used], ref.fin_tok[:, :F][used]), s
        lr = live[:, None].expand(N, k).reshape(R)
        assert torch.equal(ids.long()[lr], tok.reshape(R)[lr]), s
        assert torch.equal(anc_fus[lr], anc_ref[lr]), s
        anc_ref = torch.where(lr[:, None], anc_ref, anc_fus)         # finished molecules: the tensor form permutes rows nobody reads
        # a finished molecule stays in the batch until a compaction: the kernel gives all its beams beam 0's ancestry (one shared cache row
        # per position instead of k unrelated ones per position after its end -- the attention kernel's expensive case)
        af = anc_fus.view(N, k, L)
        assert torch.equal(af[ref.done], af[ref.done][:, :1].expand(-1, k, -1)), s
        n_fin = int(ref.fin_n.sum())
        if bool(ref.done.all()):
            break
    assert n_fin >= min(N, 8) and bool(ref.done.any())
    got, want = fus.results(), ref.results()
    assert [[h[1] for h in m] for m in got] == [[h[1] for h in m] for m in want]


# ------------------------------------------------------------------------------------------------------------------
# row bookkeeping kernels (csrc/plan.hip) against the tensor-library forms they replace
@pytest.mark.parametrize("B,Lt", [(8, 37), (128, 128), (12, 200)])
def test_pack_plan_matches_tensor_bookkeeping(ops, B, Lt):
    g = torch.Generator().manual_seed(B + Lt)
    lens = torch.randint(1, Lt + 1, (B,), generator=g); lens[0] = Lt
    mask = (torch.arange(Lt)[None, :] < lens[:, None]).int().cuda()
    M = int(lens.sum())
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    pk = ops.pack_plan(mask, M, bad)
    rows = torch.argsort((mask.view(-1) == 0), stable=True)[:M]
    row0 = (torch.cumsum(lens, 0) - lens).cuda()
    assert int(bad) == 0 and torch.equal(pk["rows"], rows) and torch.equal(pk["row0_64"], row0) and torch.equal(pk["row0"].long(), row0)
    assert torch.equal(pk["len"].long().cpu(), lens)
    BL = B * Lt
    assert torch.equal(pk["gidx2"], torch.cat([rows, BL + torch.arange(BL, device="cuda")]))
    assert torch.equal(pk["gidx4"], torch.cat([rows, BL + rows]))
    inv = torch.full((2 * BL,), -1, dtype=torch.int64, device="cuda")
    inv[rows] = torch.arange(M, device="cuda"); inv[BL:] = M + torch.arange(BL, device="cuda")
    assert torch.equal(pk["inv"], inv)
    assert torch.equal(pk["idx_m"], torch.cat([row0, M + torch.arange(M, device="cuda")]))      # momentum text encoder's last layer: CLS | causal copy
    # a hint that contradicts the mask, a hole in a row, an empty row: the flag goes up and no index leaves the sized ranges
    for kind in ("short", "hole", "empty"):
        m2, M2 = mask.clone(), M
        if kind == "short":
            M2 = M - 3
        elif kind == "hole":
            m2[0, 0] = 0
        else:
            m2[1, :] = 0
        bad.zero_()
        p2 = ops.pack_plan(m2, M2, bad)
        assert int(bad) == 1, kind
        assert int(p2["rows"].min()) >= 0 and int(p2["rows"].max()) < BL and int(p2["gidx4"].max()) < 2 * BL and int(p2["inv"][:BL].max()) < M2
        assert int(p2["row0"].max()) < M2 and int((p2["row0"] + p2["len"]).max()) <= M2 and int(p2["len"].min()) >= 1
        assert int(p2["idx_m"].min()) >= 0 and int(p2["idx_m"].max()) < 2 * M2


@pytest.mark.parametrize("B,Lt,Lp", [(4, 16, 6), (128, 128, 54), (8, 37, 54)])
def test_fusion_plan_matches_tensor_bookkeeping(ops, B, Lt, Lp):
    """Every index array of the fusion batch against the torch.cat / index_select construction it replaces (the text negatives re-enter
    PACKED at the end of the batch: their row count lives on the device); the two shared key / value sources' inverse maps against
    KVSource.finalize()."""
    from spmm_amd.engine import KVSource
    g = torch.Generator().manual_seed(5 * B + Lt)
    lens = torch.randint(2, Lt + 1, (B,), generator=g); lens[0] = Lt
    mask = (torch.arange(Lt)[None, :] < lens[:, None]).int().cuda()
    M, H = int(lens.sum()), 64
    pk = ops.pack_plan(mask, M, torch.zeros(1, dtype=torch.int32, device="cuda"))
    neg = torch.randint(0, B, (2 * B,), generator=g).cuda()
    neg_p, neg_t = neg[:B], neg[B:]
    fp = ops.fusion_plan(neg, pk, Lp)
    y1, y2 = rnd(2 * B * Lp, H, seed=1), rnd(M + B * Lt, H, seed=2)
    X6 = ops.gather_rows2(torch.empty(fp["Rcap"], H, dtype=BF, device="cuda"), y1, fp["idx6"], y2)
    pe, pc, te, h10 = y1[:B * Lp].view(B, Lp * H), y1[B * Lp:], y2[:M], y2[M:]
    ar = torch.arange(B, device="cuda")
    len8 = pk["len"][neg_t].long()
    row8 = torch.cumsum(len8, 0) - len8
    Mn = int(len8.sum())
    src_rows = torch.cat([pk["row0_64"][neg_t[s]] + torch.arange(int(len8[s]), device="cuda") for s in range(B)])      # row of te behind every packed negative row
    ref = torch.cat([torch.cat([pe, pe[neg_p], pe], 0).view(-1, H), te, te, h10, pc, te[src_rows]])
    o_tp = 3 * B * Lp; o_lm = o_tp + 2 * M; o_12 = o_lm + B * Lt; o_8 = o_12 + B * Lp
    assert fp["Rcap"] == o_8 + B * Lt and int(fp["rows_dev"]) == o_8 + Mn and int(fp["mn_dev"]) == Mn
    assert torch.equal(X6[:o_8 + Mn], ref) and float(X6[o_8 + Mn:].float().abs().max() if Mn < B * Lt else 0.0) == 0.0
    assert torch.equal(fp["neg_rows"][:Mn], src_rows) and bool((fp["neg_rows"][Mn:] == -1).all())
    i32 = lambda t: t.to(torch.int32)
    assert torch.equal(fp["ar"], i32(ar)) and torch.equal(fp["kvidx_pv"], i32(torch.cat([ar, ar, neg_t]))) and torch.equal(fp["kvidx_tp"], i32(torch.cat([ar, neg_p])))
    assert torch.equal(fp["qrow0_tp"], torch.cat([pk["row0"], pk["row0"] + M])) and torch.equal(fp["qlen_tp"], torch.cat([pk["len"], pk["len"]]))
    assert torch.equal(fp["row0_8"], i32(row8)) and torch.equal(fp["len_8"], i32(len8))
    assert torch.equal(fp["skv_row0_pv"], i32(torch.arange(3 * B, device="cuda") * Lp)) and bool((fp["skv_len_pv"] == Lp).all())
    assert torch.equal(fp["skv_row0_tx"], torch.cat([o_tp + pk["row0"], o_tp + M + pk["row0"]])) and torch.equal(fp["skv_len_tx"], torch.cat([pk["len"], pk["len"]]))
    top = torch.cat([torch.arange(3 * B, device="cuda") * Lp, o_tp + pk["row0_64"], o_tp + M + pk["row0_64"], o_8 + row8,
                     o_lm + torch.arange(B * Lt + B * Lp, device="cuda")])
    assert torch.equal(fp["idx_top"], top)
    for nm, idx in (("t", torch.cat([ar, ar, neg_t, ar])), ("p", torch.cat([ar, neg_p, ar, ar]))):
        src = KVSource(None, B, 1)
        src.add(idx)
        src.finalize()
        assert torch.equal(fp["start_" + nm], src.start) and torch.equal(fp["list_" + nm], src.list), nm


@pytest.mark.parametrize("M,N,K,Md", [(20000, 768, 768, 100), (20000, 2304, 768, 255), (16384, 768, 3072, 1), (20000, 768, 768, 256), (20000, 768, 768, 257)])
def test_weight_gradient_with_few_device_side_rows(ops, M, N, K, Md):
    """The 8-phase weight-gradient kernel under a device-side row count BELOW its 256-row minimum slicing (the packed text negatives of a
    step can total fewer than 256 tokens while the batch is allocated for B x Lt): the rows past the count hold whatever the allocator
    left there -- NaN here, in BOTH operands -- and must contribute nothing (0 x NaN would poison the product: both operands' rows are
    zeroed in LDS, csrc/gemm_tn.hip TP_MASK_TAIL)."""
    assert ops.lib().cdll.spmm_gemm_tn_splits(M, N, K, 0) > 1       # (the shape takes the 8-phase kernel with several row slices)
    md = torch.tensor([Md], dtype=torch.int32, device="cuda")
    dY, X = rnd(M, N, seed=5), rnd(M, K, seed=6)
    dY[Md:] = float("nan"); X[Md:] = float("nan")
    g_d, g_s = torch.zeros(N, K, device="cuda"), torch.zeros(N, K, device="cuda")
    ops.gemm_tn(dY, X, g_d, M_dev=md)
    ops.gemm_tn(dY[:Md], X[:Md], g_s)
    assert bool(torch.isfinite(g_d).all())
    close(g_d, g_s, 2e-3 * Md ** 0.5, 1e-4, "weight gradient")
    want = dY[:Md].float().t() @ X[:Md].float()
    close(g_d, want, 2e-3 * Md ** 0.5, 1e-4, "weight gradient vs fp32")


@pytest.mark.parametrize("M,N,K,Md", [(9000, 768, 768, 8200), (9000, 768, 768, 9000), (700, 128, 128, 300), (20000, 2304, 768, 17123), (5000, 768, 3072, 4097)])
def test_device_side_row_counts(ops, M, N, K, Md):
    """The launches over a batch whose row count only the device knows (include/spmm_hip.h, "device-side row counts"): the NT GEMM, the
    weight-gradient GEMM + column sums and both LayerNorm kernels, sized for M rows and told Md <= M through device memory, give on rows
    [0, Md) exactly what the same launch on the first Md rows gives, touch no row past Md, and reduce nothing past it -- with NaN in the
    tail rows of every input."""
    md = torch.tensor([Md], dtype=torch.int32, device="cuda")
    A, W, R = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05), rnd(M, N, seed=3)
    A[Md:] = float("nan"); R[Md:] = float("nan")
    bias = torch.randn(N, device="cuda")
    for kw in (dict(), dict(R=R), dict(epi=ops.EPI_GELU_DERIV, C2=True), dict(epi=ops.EPI_MUL, G=R, colsum=True)):
        kw = dict(kw)
        two = kw.pop("C2", False)
        cs = kw.pop("colsum", False)
        outs = []
        for dyn in (True, False):
            rows = M if dyn else Md
            C = torch.full((M, N), 7.0, dtype=BF, device="cuda")
            C2 = torch.full((M, N), 7.0, dtype=BF, device="cuda") if two else None
            col = torch.zeros(N, device="cuda") if cs else None
            k2 = {k: (v[:rows] if torch.is_tensor(v) else v) for k, v in kw.items()}
            ops.gemm_nt(A[:rows], W, C[:rows], bias=None if "G" in kw else bias, C2=None if C2 is None else C2[:rows], colsum=col,
                        M_dev=md if dyn else None, **k2)
            outs.append((C, C2, col))
        (C_d, C2_d, col_d), (C_s, C2_s, col_s) = outs
        assert torch.equal(C_d[:Md], C_s[:Md]) and bool((C_d[Md:] == 7.0).all()), kw
        if two:
            assert torch.equal(C2_d[:Md], C2_s[:Md]) and bool((C2_d[Md:] == 7.0).all())
        if cs:
            close(col_d, col_s, 2e-2 * (Md ** 0.5) / 30, 1e-3, "fused column sums")
    # weight gradient + column sums
    dY, X = rnd(M, N, seed=5), rnd(M, K, seed=6)
    dY[Md:] = float("nan"); X[Md:] = float("nan")
    g_d, g_s = torch.zeros(N, K, device="cuda"), torch.zeros(N, K, device="cuda")
    b_d, b_s = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    ops.gemm_tn(dY, X, g_d, M_dev=md); ops.colsum_bf16(dY, b_d, R_dev=md)
    ops.gemm_tn(dY[:Md], X[:Md], g_s); ops.colsum_bf16(dY[:Md], b_s)
    assert bool(torch.isfinite(g_d).all()) and bool(torch.isfinite(b_d).all())
    close(g_d, g_s, 2e-3 * Md ** 0.5, 1e-4, "weight gradient")
    close(b_d, b_s, 1e-3 * Md ** 0.5, 1e-4, "bias gradient")
    # LayerNorm forward / backward
    if N in (128, 768):
        x, r = rnd(M, N, seed=7), rnd(M, N, seed=8)
        x[Md:] = float("nan")
        gamma, beta = torch.rand(N, device="cuda") + 0.5, torch.randn(N, device="cuda")
        seed = torch.full((1,), 99, dtype=torch.int64, device="cuda")
        res = []
        for dyn in (True, False):
            rows = M if dyn else Md
            y = torch.full((M, N), 7.0, dtype=BF, device="cuda"); z = torch.full((M, N), 7.0, dtype=BF, device="cuda")
            mean, rstd = torch.full((M,), 7.0, device="cuda"), torch.full((M,), 7.0, device="cuda")
            ops.ln_fwd(x[:rows], r[:rows], gamma, beta, y[:rows], zout=z[:rows], mean=mean[:rows], rstd=rstd[:rows], dropout_p=0.1, seed=seed, salt=5,
                       rows_dev=md if dyn else None)
            dz = torch.full((M, N), 7.0, dtype=BF, device="cuda"); dx = torch.full((M, N), 7.0, dtype=BF, device="cuda")
            dg, db, dxs = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
            dy = rnd(M, N, seed=9); dy[Md:] = float("nan")
            ops.ln_bwd(dy[:rows], z[:rows], mean[:rows], rstd[:rows], gamma, dz[:rows], dx=dx[:rows], dgamma=dg, dbeta=db, dropout_p=0.1, seed=seed, salt=5,
                       dxsum=dxs, rows_dev=md if dyn else None)
            res.append((y, z, mean, dz, dx, dg, db, dxs))
        for a_, b_ in zip(res[0][:5], res[1][:5]):
            assert torch.equal(a_[:Md], b_[:Md]) and bool((a_[Md:] == 7.0).all())
        for a_, b_, nm in zip(res[0][5:], res[1][5:], ("dgamma", "dbeta", "dxsum")):
            assert bool(torch.isfinite(a_).all())
            close(a_, b_, 2e-3 * Md ** 0.5, 1e-3, nm)


def test_row_helpers_gather2_add_zero_gelu(ops):
    H = 128
    a, b = rnd(50, H, seed=3), rnd(70, H, seed=4)
    g = torch.Generator().manual_seed(9)
    ia, ib = torch.randint(0, 50, (40,), generator=g), torch.randint(0, 70, (40,), generator=g)
    idx = torch.cat([ia, ib + ops.SRC_B, torch.full((7,), -1, dtype=torch.int64)]).cuda()
    out = ops.gather_rows2(torch.empty(87, H, dtype=BF, device="cuda"), a, idx, b)
    assert torch.equal(out, torch.cat([a[ia.cuda()], b[ib.cuda()], torch.zeros(7, H, dtype=BF, device="cuda")]))
    dst, src = rnd(60, H, seed=5), rnd(20, H, seed=6)
    perm = torch.randperm(60, generator=g)[:20].cuda()
    ref = dst.clone(); ref[perm] = (ref[perm].float() + src.float()).to(BF)
    assert torch.equal(ops.add_rows_bf16(dst, perm, src), ref)
    t = rnd(33, 3 * H, seed=7)
    keep = t.clone()
    ops.zero_(t[5:20, H:])
    keep[5:20, H:] = 0
    assert torch.equal(t, keep) and float(ops.zero_(rnd(1000, 8, seed=8)).abs().max()) == 0.0
    dz, pre = rnd(300, H, seed=10), rnd(300, H, seed=11, scale=2.0)
    x = pre.float()
    want = dz.float() * (0.5 * (1 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327)
    close(ops.gelu_bwd(dz, pre).float(), want, 2e-2, 1e-2, "gelu_bwd")


@pytest.mark.parametrize("nseq,nH,Lmax", [(6, 2, 54), (5, 12, 128), (4, 2, 200)])
def test_attention_of_position0_queries_over_full_sequences(ops, nseq, nH, Lmax):
    """The CLS-only top fusion layer's self-attention (engine.SelfKV): one query row per sequence (Lq = 1, dense) against the keys / values
    of the whole sequence, addressed by kv_row0 / kv_len in another tensor -- equal, bit for bit, to row 0 of the full-sequence launch."""
    H = nH * 64
    g = torch.Generator().manual_seed(nseq * Lmax)
    lens = torch.randint(3, Lmax + 1, (nseq,), generator=g); lens[0] = Lmax
    row0 = torch.cumsum(lens, 0) - lens
    M = int(lens.sum())
    qkv = rnd(M, 3 * H, seed=31)
    i32 = lambda t: t.to(torch.int32).cuda()
    lay = dict(q_row0=i32(row0), q_len=i32(lens), kv_row0=i32(row0), kv_len=i32(lens))
    O = torch.zeros(M, H, dtype=BF, device="cuda"); lse = torch.zeros(nseq, nH, Lmax, device="cuda")
    kw = dict(nseq=nseq, nH=nH, Lkv=Lmax, causal_from=nseq)
    ops.attn_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], O, lse, Lq=Lmax, **kw, **lay)
    q0 = qkv[row0.cuda(), :H].contiguous()
    O1 = torch.zeros(nseq, H, dtype=BF, device="cuda"); lse1 = torch.zeros(nseq, nH, 1, device="cuda")
    ops.attn_fwd(q0, qkv[:, H:2 * H], qkv[:, 2 * H:], O1, lse1, Lq=1, kv_row0=lay["kv_row0"], kv_len=lay["kv_len"], **kw)
    assert torch.equal(O1, O[row0.cuda()]) and torch.equal(lse1[:, :, 0], lse[:, :, 0])
    # backward: upstream gradient on position 0 only
    dO = torch.zeros(M, H, dtype=BF, device="cuda")
    dO1 = rnd(nseq, H, seed=32)
    dO[row0.cuda()] = dO1
    dQKV = torch.zeros(M, 3 * H, dtype=BF, device="cuda")
    ops.attn_bwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], O, lse, dO, dQKV[:, :H], dQKV[:, H:2 * H], dQKV[:, 2 * H:], Lq=Lmax, **kw, **lay)
    dQ1 = torch.zeros(nseq, H, dtype=BF, device="cuda"); dKV1 = torch.zeros(M, 2 * H, dtype=BF, device="cuda")
    ops.attn_bwd(q0, qkv[:, H:2 * H], qkv[:, 2 * H:], O1, lse1, dO1, dQ1, dKV1[:, :H], dKV1[:, H:], Lq=1, kv_row0=lay["kv_row0"], kv_len=lay["kv_len"], **kw)
    assert torch.equal(dQ1, dQKV[row0.cuda(), :H]) and torch.equal(dKV1, dQKV[:, H:])
    rest = torch.ones(M, dtype=torch.bool, device="cuda"); rest[row0.cuda()] = False
    assert float(dQKV[rest][:, :H].float().abs().max()) == 0.0        # rows without an upstream gradient get exactly zero

