"""Shape and edge coverage of the optimiser kernels (csrc/optim.hip: grad_sqnorm, adamw_step, ema_update, axpy_scalar) and of the small
kernels without a kernel-level test elsewhere (clamp_scalar, rows_linear, cast_transpose_multi, ln_fwd_r32) against float64 restatements
of the torch operations they replace, evaluated on the CPU.  Inputs come from a seeded CPU generator and are rounded to bf16 first where
the kernel reads bf16.

Tolerances (tests/helpers_gpu.py::check_ref) come from the reference, never from the kernel: E32 is the largest error of the same
formula in fp32 torch on the CPU against float64; an fp32 output may be max(8 * E32, 4 fp32 ulp of the output's magnitude) away, a bf16
output one bf16 ulp of the reference (relative 2^-7) more.  Casts, shadows, sentinels and skip paths are compared with torch.equal.
Every comparison prints `[tol] name: E32 kernel bound` (pytest -s).

Measured on an MI355X: per case the output with the least margin (kernel error / bound); for a bf16 output the kernel column is what
remains past one bf16 ulp of the reference.

| case | output | E32 | kernel | bound |
|---|---|---|---|---|
| grad_sqnorm[n=4] | out | 3.3e-05 | 3.3e-05 | 4.9e-04 |
| grad_sqnorm[n=1048580] | out | 1.8e-02 | 4.4e-02 | 2.5e-01 |
| grad_sqnorm[n=4194452] | out | 1.2e-01 | 1.2e-01 | 2.0e+00 |
| adamw[n=4 step 1] | m | 2.5e-08 | 2.5e-08 | 2.0e-07 |
| adamw[n=4 step 2] | v | 1.7e-09 | 1.7e-09 | 1.3e-08 |
| adamw[n=4 step 3] | v | 1.4e-09 | 1.5e-09 | 1.1e-08 |
| adamw[n=4 step 1 no shadow] | m | 2.5e-08 | 2.5e-08 | 2.0e-07 |
| adamw[n=4 step 2 no shadow] | v | 1.7e-09 | 1.7e-09 | 1.3e-08 |
| adamw[n=4 step 3 no shadow] | v | 1.4e-09 | 1.5e-09 | 1.1e-08 |
| adamw[n=1048580 step 1] | v | 6.9e-14 | 6.9e-14 | 5.5e-13 |
| adamw[n=1048580 step 2] | grad_norm | 6.6e-08 | 6.6e-08 | 5.3e-07 |
| adamw[n=1048580 step 3] | v | 8.8e-14 | 1.0e-13 | 7.0e-13 |
| adamw[n=1048580 step 1 no shadow] | v | 6.9e-14 | 6.9e-14 | 5.5e-13 |
| adamw[n=1048580 step 2 no shadow] | grad_norm | 6.6e-08 | 6.6e-08 | 5.3e-07 |
| adamw[n=1048580 step 3 no shadow] | v | 8.8e-14 | 1.0e-13 | 7.0e-13 |
| adamw[n=4194452 step 1] | v | 2.2e-14 | 2.2e-14 | 1.7e-13 |
| adamw[n=4194452 step 2] | v | 2.3e-14 | 2.5e-14 | 1.9e-13 |
| adamw[n=4194452 step 3] | v | 2.7e-14 | 2.7e-14 | 2.2e-13 |
| adamw[n=4194452 step 1 no shadow] | v | 2.2e-14 | 2.2e-14 | 1.7e-13 |
| adamw[n=4194452 step 2 no shadow] | v | 2.3e-14 | 2.5e-14 | 1.9e-13 |
| adamw[n=4194452 step 3 no shadow] | v | 2.7e-14 | 2.7e-14 | 2.2e-13 |
| ema[n=4 momentum=0.995] | twice, no shadow | 1.0e-07 | 1.0e-07 | 8.2e-07 |
| ema[n=4 momentum=0.0] | out | 0.0e+00 | 0.0e+00 | 4.8e-07 |
| ema[n=4 momentum=1.0] | out | 0.0e+00 | 0.0e+00 | 4.8e-07 |
| ema[n=1048580 momentum=0.995] | out | 3.8e-07 | 2.3e-07 | 3.0e-06 |
| ema[n=1048580 momentum=0.0] | out | 0.0e+00 | 0.0e+00 | 1.9e-06 |
| ema[n=1048580 momentum=1.0] | out | 0.0e+00 | 0.0e+00 | 1.9e-06 |
| ema[n=4194452 momentum=0.995] | twice, no shadow | 8.3e-07 | 4.6e-07 | 6.7e-06 |
| ema[n=4194452 momentum=0.0] | out | 0.0e+00 | 0.0e+00 | 1.9e-06 |
| ema[n=4194452 momentum=1.0] | out | 0.0e+00 | 0.0e+00 | 1.9e-06 |
| axpy_scalar[n=1 ptr=False] | out | 2.9e-09 | 2.9e-09 | 3.0e-08 |
| axpy_scalar[n=1 ptr=True] | out | 5.1e-09 | 5.1e-09 | 2.4e-07 |
| axpy_scalar[n=257 ptr=False] | out | 1.4e-07 | 1.4e-07 | 1.1e-06 |
| axpy_scalar[n=257 ptr=True] | out | 1.7e-07 | 1.7e-07 | 1.3e-06 |
| rows_linear[5x768x1 bf16 act=0] | out | 2.1e-07 | 2.1e-07 | 1.9e-06 |
| rows_linear[5x768x1 bf16 act=1] | out | 1.0e-06 | 5.0e-07 | 8.0e-06 |
| rows_linear[5x768x1 fp32 act=0] | out | 2.3e-07 | 2.3e-07 | 1.9e-06 |
| rows_linear[5x768x1 fp32 act=1] | out | 5.9e-07 | 3.2e-07 | 4.7e-06 |
| rows_linear[54x256x63 bf16 act=0] | out | 1.2e-06 | 2.3e-06 | 9.3e-06 |
| rows_linear[54x256x63 bf16 act=1] | out | 1.3e-06 | 1.5e-06 | 1.0e-05 |
| rows_linear[54x256x63 fp32 act=0] | out | 1.3e-06 | 1.8e-06 | 1.1e-05 |
| rows_linear[54x256x63 fp32 act=1] | out | 1.1e-06 | 1.6e-06 | 9.1e-06 |
| rows_linear[3x2x1536 bf16 act=0] | out | 2.2e-07 | 1.2e-07 | 1.8e-06 |
| rows_linear[3x2x1536 bf16 act=1] | out | 1.7e-07 | 6.8e-08 | 1.3e-06 |
| rows_linear[3x2x1536 fp32 act=0] | out | 3.8e-07 | 3.1e-07 | 3.0e-06 |
| rows_linear[3x2x1536 fp32 act=1] | out | 3.8e-07 | 2.4e-07 | 3.1e-06 |
| rows_linear[7x1x768 bf16 act=0] | out | 4.7e-07 | 1.7e-07 | 3.8e-06 |
| rows_linear[7x1x768 bf16 act=1] | out | 4.9e-07 | 1.4e-07 | 3.9e-06 |
| rows_linear[7x1x768 fp32 act=0] | out | 3.1e-07 | 3.1e-07 | 2.5e-06 |
| rows_linear[7x1x768 fp32 act=1] | out | 2.2e-07 | 1.2e-07 | 1.8e-06 |
| rows_linear[130x70x100 bf16 act=0] | out | 1.8e-06 | 4.5e-07 | 1.4e-05 |
| rows_linear[130x70x100 bf16 act=1] | out | 1.7e-06 | 5.9e-07 | 1.4e-05 |
| rows_linear[130x70x100 fp32 act=0] | out | 1.7e-06 | 4.4e-07 | 1.4e-05 |
| rows_linear[130x70x100 fp32 act=1] | out | 2.5e-06 | 6.1e-07 | 2.0e-05 |
| rows_linear[1x256x64 bf16 act=0] | out | 2.8e-07 | 2.2e-07 | 2.2e-06 |
| rows_linear[1x256x64 bf16 act=1] | out | 2.7e-07 | 2.9e-07 | 2.1e-06 |
| rows_linear[1x256x64 fp32 act=0] | out | 2.5e-07 | 2.5e-07 | 2.0e-06 |
| rows_linear[1x256x64 fp32 act=1] | out | 4.0e-07 | 2.5e-07 | 3.2e-06 |
| ln_fwd_r32[7x128 res32 p=0.0] | y32 | 3.0e-07 | 3.0e-07 | 2.4e-06 |
| ln_fwd_r32[7x128 res32 p=0.1] | y32 | 4.3e-07 | 3.0e-07 | 3.4e-06 |
| ln_fwd_r32[7x128 no res p=0.0] | rstd | 6.0e-08 | 6.0e-08 | 4.8e-07 |
| ln_fwd_r32[7x128 no res p=0.1] | mean | 1.9e-08 | 1.5e-08 | 1.5e-07 |
| ln_fwd_r32[1003x768 res32 p=0.0] | rstd | 7.0e-08 | 6.9e-08 | 5.6e-07 |
| ln_fwd_r32[1003x768 res32 p=0.1] | rstd | 7.2e-08 | 8.2e-08 | 5.7e-07 |
| ln_fwd_r32[1003x768 no res p=0.0] | mean | 7.5e-09 | 8.7e-09 | 6.0e-08 |
| ln_fwd_r32[1003x768 no res p=0.1] | rstd | 1.1e-07 | 1.3e-07 | 8.5e-07 |
| ln_fwd_r32[5x1000 res32 p=0.0] | rstd | 2.8e-08 | 5.7e-08 | 2.4e-07 |
| ln_fwd_r32[5x1000 res32 p=0.1] | rstd | 4.2e-08 | 5.1e-08 | 3.4e-07 |
| ln_fwd_r32[5x1000 no res p=0.0] | y32 | 4.4e-07 | 4.4e-07 | 3.5e-06 |
| ln_fwd_r32[5x1000 no res p=0.1] | mean | 3.9e-09 | 3.9e-09 | 3.2e-08 |
"""
import numpy as np

import pytest
import torch

from helpers_gpu import _host_dropout_keep, check_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32, F64 = torch.float32, torch.float64
SENT = 7.0


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
    """The value a kernel receives for the fp32 argument v, as a Python float."""
    return float(np.float32(v))


def dev_scalar(v, dtype=F32):
    return torch.tensor([v], dtype=dtype, device="cuda")


# n / 4 > 262 144 (grad_sqnorm) and > 1 048 576 (adamw_step, ema_update): the smallest sizes with a grid-stride iteration, plus one float4
SIZES = [4, 1048580, 4194452]


# ------------------------------------------------------------------------------------------------ grad_sqnorm
@pytest.mark.parametrize("n", SIZES)
def test_grad_sqnorm(ops, n):
    g = randn(n, seed=800 + n % 97)
    gd = g.cuda()
    out = dev_scalar(1024.0)
    ops.grad_sqnorm(gd, out)
    check_ref(f"grad_sqnorm[n={n}]", out, 1024.0 + (g.double() ** 2).sum().view(1), (1024.0 + (g ** 2).sum()).view(1))
    # fixed summation order: data-parallel replicas must derive the same clip coefficient bit for bit (csrc/optim.hip)
    a, b = dev_scalar(0.0), dev_scalar(0.0)
    ops.grad_sqnorm(gd, a)
    ops.grad_sqnorm(gd, b)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ adamw_step
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.02, max_norm=5.0)


def _adamw_ref(p, grads, dtype):
    """torch.optim.AdamW (decoupled decay, bias correction, eps outside the square root) after clip_grad_norm_(max_norm), restated on
    flat tensors; the hyper-parameters have the values the kernel receives as fp32.  -> [(p, m, v, grad_norm, clipped) after each step]"""
    lr, b1, b2, eps, wd, mx = (f32v(HP[k]) for k in ("lr", "beta1", "beta2", "eps", "wd", "max_norm"))
    p = p.to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t, g in enumerate(grads, 1):
        g = g.to(dtype)
        norm = (g * g).sum().sqrt()
        coef = torch.clamp(mx / (norm + 1e-6), max=1.0)
        g = g * coef
        p = p * (1 - lr * wd)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        denom = v.sqrt() / (bc2 ** 0.5) + eps
        p = p - (lr / bc1) * (m / denom)
        out.append((p.clone(), m.clone(), v.clone(), norm.view(1), bool(coef < 1)))
    return out


def _grads(n, seed):
    """Three gradients of norms 10, 1, 10: clipped, not clipped, clipped at max_norm = 5."""
    gs = []
    for i, target in enumerate((10.0, 1.0, 10.0)):
        g = randn(n, seed=seed + i)
        gs.append(g * (target / g.norm().item()))
    return gs


@pytest.mark.parametrize("with_shadow", [True, False], ids=["shadow", "no_shadow"])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_three_steps(ops, n, with_shadow):
    p0, grads = randn(n, seed=810), _grads(n, 811)
    r64, r32 = _adamw_ref(p0, grads, F64), _adamw_ref(p0, grads, F32)
    assert [r[4] for r in r64] == [True, False, True]
    p = p0.cuda()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    shadow = torch.full((n,), SENT, dtype=BF, device="cuda") if with_shadow else None
    lr, step = dev_scalar(HP["lr"]), torch.zeros(1, dtype=torch.int32, device="cuda")
    scal = torch.zeros(ops.adam_scalars_bytes() // 4, device="cuda")
    for it, g in enumerate(grads):
        nsq = dev_scalar(0.0)
        ops.grad_sqnorm(g.cuda(), nsq)
        ops.adamw_step(p, g.cuda(), m, v, shadow, lr=lr, normsq=nsq, step=step, scalars=scal)
        tag = f"adamw[n={n} step {it + 1}{'' if with_shadow else ' no shadow'}]"
        check_ref(f"{tag} p", p, r64[it][0], r32[it][0])
        check_ref(f"{tag} m", m, r64[it][1], r32[it][1])
        check_ref(f"{tag} v", v, r64[it][2], r32[it][2])
        check_ref(f"{tag} grad_norm", scal[4:5], r64[it][3], r32[it][3])
        assert step.item() == it + 1
        if with_shadow:
            assert torch.equal(shadow, p.to(BF)), "the bf16 shadow is the cast of the updated parameters, bit for bit"


@pytest.mark.parametrize("how", ["nan_in_g", "inf_in_g", "nan_flag"])
@pytest.mark.parametrize("n", [4, 1048580])
def test_adamw_skips_the_step(ops, n, how):
    p0, grads = randn(n, seed=810), _grads(n, 811)
    p = p0.cuda()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    shadow = torch.zeros(n, dtype=BF, device="cuda")
    lr, step = dev_scalar(HP["lr"]), torch.zeros(1, dtype=torch.int32, device="cuda")
    scal = torch.zeros(ops.adam_scalars_bytes() // 4, device="cuda")
    nsq = dev_scalar(0.0)
    ops.grad_sqnorm(grads[0].cuda(), nsq)
    ops.adamw_step(p, grads[0].cuda(), m, v, shadow, lr=lr, normsq=nsq, step=step, scalars=scal)        # one real step first
    before = [t.clone() for t in (p, m, v, shadow)]
    g = grads[1].clone()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    if how == "nan_in_g":
        g[n - 2] = float("nan")
    elif how == "inf_in_g":
        g[n - 2] = float("inf")
    else:
        flag.fill_(1)
    nsq = dev_scalar(0.0)
    ops.grad_sqnorm(g.cuda(), nsq)
    ops.adamw_step(p, g.cuda(), m, v, shadow, lr=lr, normsq=nsq, step=step, nan_flag=flag, scalars=scal)
    for name, t, b in zip("p m v shadow".split(), (p, m, v, shadow), before):
        assert torch.equal(t, b), f"{how}: {name} moved"
    assert step.item() == 1
    # ... and a clean step afterwards is taken again
    flag.zero_()
    nsq = dev_scalar(0.0)
    ops.grad_sqnorm(grads[1].cuda(), nsq)
    ops.adamw_step(p, grads[1].cuda(), m, v, shadow, lr=lr, normsq=nsq, step=step, nan_flag=flag, scalars=scal)
    assert step.item() == 2 and not torch.equal(p, before[0])


# ------------------------------------------------------------------------------------------------ ema_update
@pytest.mark.parametrize("momentum", [0.995, 0.0, 1.0])
@pytest.mark.parametrize("n", SIZES)
def test_ema_update(ops, n, momentum):
    pm0, p0 = randn(n, seed=820), randn(n, seed=821)
    pm, p = pm0.cuda(), p0.cuda()
    shadow = torch.full((n,), SENT, dtype=BF, device="cuda")
    ops.ema_update(pm, p, shadow, momentum)
    a = f32v(momentum)

    def ref(dtype):                                           # _momentum_update SPMM_models.py:266-269
        return pm0.to(dtype) * a + p0.to(dtype) * (1 - a)
    check_ref(f"ema[n={n} momentum={momentum}]", pm, ref(F64), ref(F32))
    assert torch.equal(shadow, pm.to(BF))
    assert torch.equal(p.cpu(), p0)
    ops.ema_update(pm, p, None, momentum)                     # without a shadow
    check_ref(f"ema[n={n} momentum={momentum}] twice, no shadow", pm, ref(F64) * a + p0.double() * (1 - a), ref(F32) * a + p0 * (1 - a))


# ------------------------------------------------------------------------------------------------ axpy_scalar / clamp_scalar
@pytest.mark.parametrize("with_ptr", [False, True])
@pytest.mark.parametrize("n", [1, 257])
def test_axpy_scalar(ops, n, with_ptr):
    d0, s0 = randn(n, seed=830), randn(n, seed=831)
    dst = d0.cuda()
    ops.axpy_scalar(dst, s0.cuda(), scale_ptr=dev_scalar(-1.75) if with_ptr else None, scale=0.3)
    k = f32v(0.3)

    def ref(dtype):
        return d0.to(dtype) + s0.to(dtype) * k * (-1.75 if with_ptr else 1.0)
    check_ref(f"axpy_scalar[n={n} ptr={with_ptr}]", dst, ref(F64), ref(F32))


@pytest.mark.parametrize("value,want", [(0.0001, 0.001), (0.07, 0.07), (0.75, 0.5)])
def test_clamp_scalar(ops, value, want):
    p = torch.tensor([SENT, value, SENT], device="cuda")
    ops.clamp_scalar(p[1:2], 0.001, 0.5)                      # temp.clamp_(0.001, 0.5), SPMM_models.py
    assert p.cpu().tolist() == [SENT, f32v(want), SENT]


# ------------------------------------------------------------------------------------------------ rows_linear
@pytest.mark.parametrize("act", [0, 1], ids=["linear", "gelu"])
@pytest.mark.parametrize("xdtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("rows,N,K", [(5, 768, 1), (54, 256, 63), (3, 2, 1536), (7, 1, 768), (130, 70, 100), (1, 256, 64)])
def test_rows_linear(ops, rows, N, K, xdtype, act):
    x = randn(rows, K, seed=840 + K).to(xdtype)
    W, bias = randn(N, K, seed=841, scale=K ** -0.5), randn(N, seed=842)
    xbuf = torch.full((rows, K + 8), SENT, dtype=xdtype)
    xbuf[:, :K] = x
    xd = xbuf.cuda()[:, :K]                                    # x and out are column slices: row strides K + 8 and N + 8
    for with_bias in (True, False):
        obuf = torch.full((rows, N + 8), SENT, device="cuda")
        ops.rows_linear(xd, W.cuda(), bias.cuda() if with_bias else None, obuf[:, :N], act=act)

        def ref(dtype):
            o = x.to(dtype) @ W.to(dtype).t()
            if with_bias:
                o = o + bias.to(dtype)
            return torch.nn.functional.gelu(o) if act else o          # erf-GELU
        check_ref(f"rows_linear[{rows}x{N}x{K} {'bf16' if xdtype == BF else 'fp32'} act={act} bias={with_bias}]", obuf[:, :N], ref(F64), ref(F32))
        assert (obuf[:, N:] == SENT).all(), "columns of out beyond N were written"


# ------------------------------------------------------------------------------------------------ cast_transpose_multi
def test_cast_transpose_multi_descriptor_table(ops):
    """One launch over five matrices; the table is packed by the function spmm_amd/params.py builds its own with."""
    from spmm_amd.params import ct_descriptor_table
    shapes = [(768, 768), (3072, 768), (70, 130), (1, 64), (64, 1)]
    gap = 37
    srcs = [randn(R, C, seed=850 + i).cuda() for i, (R, C) in enumerate(shapes)]
    buf = torch.full((sum(R * C for R, C in shapes) + gap * (len(shapes) + 1),), SENT, dtype=BF, device="cuda")
    dsts, gaps, o = [], [], 0
    for R, C in shapes:
        gaps.append(buf[o:o + gap])
        o += gap
        dsts.append(buf[o:o + R * C].view(C, R))
        o += R * C
    gaps.append(buf[o:])
    blob, tiles = ct_descriptor_table(list(zip(srcs, dsts)))
    assert tiles == sum(((R + 63) // 64) * ((C + 63) // 64) for R, C in shapes)
    desc = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    ops.cast_transpose_multi(desc, len(shapes), tiles)
    for (R, C), s, d in zip(shapes, srcs, dsts):
        assert torch.equal(d, s.to(BF).t()), f"dstT of the {R} x {C} matrix"
    for i, gp in enumerate(gaps):
        assert (gp == SENT).all(), f"the gap before destination {i} was written"


# ------------------------------------------------------------------------------------------------ ln_fwd_r32
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("with_res", [True, False], ids=["res32", "no_res"])
@pytest.mark.parametrize("rows,H", [(7, 128), (1003, 768), (5, 1000)])
def test_ln_fwd_r32(ops, rows, H, with_res, p):
    tag = f"ln_fwd_r32[{rows}x{H} {'res32' if with_res else 'no res'} p={p}]"
    seed_v, salt = 20260931, 4711
    x = randn(rows, H, seed=860 + H).to(BF)
    res = randn(rows, H, seed=861) if with_res else None
    gamma, beta = 1 + 0.1 * randn(H, seed=862), 0.1 * randn(H, seed=863)
    xd = x.cuda()
    y = torch.full((rows, H), SENT, dtype=BF, device="cuda")
    z = torch.full((rows, H), SENT, dtype=BF, device="cuda")
    y32 = torch.full((rows, H), SENT, device="cuda")
    mean, rstd = torch.full((rows,), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda")
    seed = torch.tensor([seed_v], dtype=torch.int64, device="cuda")
    ops.ln_fwd_r32(xd, None if res is None else res.cuda(), gamma.cuda(), beta.cuda(), y, y32=y32, zout=z, mean=mean, rstd=rstd, eps=1e-12,
                   dropout_p=p, seed=seed, salt=salt)
    keep = torch.from_numpy(_host_dropout_keep(seed_v, salt, np.arange(rows), H, p)) if p else torch.ones(rows, H, dtype=torch.bool)
    dscale = float(np.float32(1) / (np.float32(1) - np.float32(p)))               # the kernel's fp32 1 / (1 - p)

    def ref(dtype):
        zr = torch.where(keep, x.to(dtype) * dscale, torch.zeros((), dtype=dtype))
        if res is not None:
            zr = zr + res.to(dtype)
        mu = zr.mean(-1)
        var = zr.var(-1, unbiased=False)
        yr = torch.nn.functional.layer_norm(zr, (H,), gamma.to(dtype), beta.to(dtype), 1e-12)
        return zr, yr, mu, (var + 1e-12).rsqrt()
    (z64, y64, m64, r64), (z32, yr32, m32, r32) = ref(F64), ref(F32)
    check_ref(f"{tag} y32", y32, y64, yr32)
    check_ref(f"{tag} zout", z, z64, z32, bf16=True)
    check_ref(f"{tag} mean", mean, m64, m32)
    check_ref(f"{tag} rstd", rstd, r64, r32)
    assert torch.equal(y, y32.to(BF)), "the bf16 copy is the cast of the fp32 row, bit for bit"
    if p:                                                      # a dropped element leaves the residual alone, exactly
        assert not keep.all() and (z.cpu()[~keep] == (0 if res is None else res[~keep].to(BF))).all()
    if res is None:                                            # the backward regenerates the mask from the same hash: same zout as ln_fwd's
        y2, z2 = torch.empty_like(y), torch.full((rows, H), SENT, dtype=BF, device="cuda")
        ops.ln_fwd(xd, None, gamma.cuda(), beta.cuda(), y2, zout=z2, eps=1e-12, dropout_p=p, seed=seed, salt=salt)
        assert torch.equal(z, z2)
