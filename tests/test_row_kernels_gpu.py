"""Shape and edge coverage of the row kernels every training and decode step goes through: the embeddings with their LayerNorm (csrc/rowops.hip:
embed_ln_fwd in its three modes and with dropout, ln_bwd(drop_on_dy), embed_bwd on both launch shapes, embed_step_ln_fwd with a device-side
position), the column sums and the slab reduce of csrc/gemm_tn.hip (colsum_bf16, spmm_gemm_tn_reduce), and the layout / row helpers of
csrc/rowops.hip and csrc/plan.hip (transpose_bf16, cast_transpose, the casts, acc_rows, gather_rows, gather_rows2, add_rows_bf16, zero_,
gelu_bwd, segment_sum_bf16) -- against float64 restatements of the same operations in plain torch on the CPU.  Inputs come from a seeded CPU
generator and are rounded to bf16 first where the kernel reads bf16.

Tolerances (tests/helpers_gpu.py::check_ref) come from the reference, never from the kernel: E32 is the largest error of the same
formula in fp32 torch on the CPU against float64; an fp32 output may be max(8 * E32, 4 fp32 ulp of the output's magnitude) away, a bf16
output one bf16 ulp of the reference (relative 2^-7) more.  Column sums that reach the float64 value only through atomics (dpos, dtype0,
dword, d_w / d_b / d_cls / d_masktok, dgamma, dbeta, colsum) are held to the same rule.  Copies, casts, gathers, zero fills, sentinels and
masks are compared with torch.equal or as bit patterns.  Every comparison prints `[tol] name: E32 kernel bound` (pytest -s).

One comparison spans kernels: the chain embed_ln_fwd -> ln_bwd(drop_on_dy) -> embed_bwd against float64 autograd of the whole expression.
The chain stores the pre-LayerNorm sum and its gradient as bf16 between the launches, which the float64 expression does not; its fp32
restatement (the `ref32` of check_ref) therefore rounds those two tensors to bf16 where the chain stores them and is fp32 otherwise, so
that E32 holds the error of the number formats the chain is built from and the rule stays the one above.

Bad pointers and refused calls are tested on the CPU (tests/test_abi_cpu.py); nothing here passes a null or wrong pointer to a launch.

Measured on an MI355X: per case the output with the least margin (kernel error / bound); for a bf16 output the kernel column is what
remains past one bf16 ulp of the reference.

| case | output | E32 | kernel | bound |
|---|---|---|---|---|
| embed_fwd[m0 3x7x128] | mean | 2.6e-08 | 2.7e-08 | 2.1e-07 |
| embed_fwd[m0 5x24x768] | mean | 2.0e-08 | 1.9e-08 | 1.6e-07 |
| embed_fwd[m0 2x9x1000] | mean | 1.3e-08 | 1.3e-08 | 1.0e-07 |
| embed_fwd[m0 4x6x1024] | mean | 1.1e-08 | 1.0e-08 | 8.7e-08 |
| embed_fwd[m1 6x54x128 mod3] | mean | 4.8e-08 | 4.7e-08 | 3.9e-07 |
| embed_fwd[m1 6x54x768 mod3] | mean | 2.1e-08 | 1.9e-08 | 1.6e-07 |
| embed_fwd[m1 7x54x128 mod3] | mean | 4.3e-08 | 6.0e-08 | 3.4e-07 |
| embed_fwd[m2 3x12x768] | rstd | 6.5e-08 | 6.8e-08 | 5.2e-07 |
| embed_fwd[m2 2x5x1000] | rstd | 3.7e-08 | 3.7e-08 | 3.0e-07 |
| embed_fwd_dropout[H128] | mean | 2.2e-08 | 2.5e-08 | 1.8e-07 |
| embed_fwd_dropout[H768] | mean | 1.9e-08 | 2.2e-08 | 1.5e-07 |
| embed_fwd_dropout[H1000] | mean | 1.4e-08 | 9.5e-09 | 1.1e-07 |
| embed_step[1x256 pos_ptr] | y | 6.6e-07 | 0.0e+00 | 5.2e-06 |
| embed_step[1x256 pos_index] | y | 6.4e-07 | 0.0e+00 | 5.1e-06 |
| embed_step[1x768 pos_ptr] | y | 4.0e-07 | 0.0e+00 | 3.2e-06 |
| embed_step[1x768 pos_index] | y | 4.0e-07 | 0.0e+00 | 3.2e-06 |
| embed_step[1x1000 pos_ptr] | y | 4.4e-07 | 0.0e+00 | 3.5e-06 |
| embed_step[1x1000 pos_index] | y | 4.0e-07 | 0.0e+00 | 3.2e-06 |
| embed_step[9x256 pos_ptr] | y | 5.5e-07 | 0.0e+00 | 4.4e-06 |
| embed_step[9x256 pos_index] | y | 4.8e-07 | 0.0e+00 | 3.8e-06 |
| embed_step[9x768 pos_ptr] | y | 6.7e-07 | 0.0e+00 | 5.3e-06 |
| embed_step[9x768 pos_index] | y | 6.4e-07 | 0.0e+00 | 5.2e-06 |
| embed_step[9x1000 pos_ptr] | y | 6.2e-07 | 0.0e+00 | 5.0e-06 |
| embed_step[9x1000 pos_index] | y | 7.1e-07 | 0.0e+00 | 5.7e-06 |
| ln_bwd_drop_on_dy[21x128] | dgamma | 2.1e-06 | 2.5e-06 | 1.7e-05 |
| ln_bwd_drop_on_dy[21x128 dy2] | dbeta | 1.8e-06 | 1.2e-06 | 1.4e-05 |
| ln_bwd_drop_on_dy[21x128 no dgamma] | dz | 2.3e-07 | 0.0e+00 | 1.8e-06 |
| ln_bwd_drop_on_dy[333x768] | dbeta | 1.0e-05 | 1.6e-05 | 8.3e-05 |
| ln_bwd_drop_on_dy[333x768 dy2] | dbeta | 1.2e-05 | 1.9e-05 | 9.3e-05 |
| ln_bwd_drop_on_dy[333x768 no dgamma] | dz | 5.0e-07 | 0.0e+00 | 4.0e-06 |
| ln_bwd_drop_on_dy[5x1000] | dgamma | 1.2e-06 | 1.5e-06 | 9.8e-06 |
| ln_bwd_drop_on_dy[5x1000 dy2] | dbeta | 1.1e-06 | 1.1e-06 | 8.9e-06 |
| ln_bwd_drop_on_dy[5x1000 no dgamma] | dz | 3.1e-07 | 0.0e+00 | 2.5e-06 |
| ln_bwd_drop_on_dy[64x1024] | dbeta | 3.0e-06 | 3.6e-06 | 2.4e-05 |
| ln_bwd_drop_on_dy[64x1024 dy2] | dbeta | 4.5e-06 | 5.0e-06 | 3.6e-05 |
| ln_bwd_drop_on_dy[64x1024 no dgamma] | dz | 5.2e-07 | 0.0e+00 | 4.2e-06 |
| ln_bwd_drop_on_dy[1237x768] | dz | 1.2e-06 | 0.0e+00 | 9.7e-06 |
| ln_bwd_drop_on_dy[1237x768 dy2] | dz | 1.3e-06 | 0.0e+00 | 1.1e-05 |
| ln_bwd_drop_on_dy[1237x768 no dgamma] | dz | 1.2e-06 | 0.0e+00 | 9.7e-06 |
| embed_bwd[m0 6x7x128 mixed] | dtype0 | 7.2e-07 | 1.1e-06 | 7.6e-06 |
| embed_bwd[m0 32x7x768 mixed] | dpos | 9.0e-07 | 1.2e-06 | 7.6e-06 |
| embed_bwd[m0 33x7x1000 mixed] | dpos | 9.2e-07 | 1.3e-06 | 7.6e-06 |
| embed_bwd[m0 47x7x768 mixed] | dpos | 9.5e-07 | 1.3e-06 | 7.6e-06 |
| embed_bwd[m0 33x7x128 same] | dword | 1.1e-06 | 1.0e-06 | 8.6e-06 |
| embed_bwd[m0 47x7x1000 same] | dpos | 9.5e-07 | 1.3e-06 | 7.6e-06 |
| embed_bwd[m0 6x7x768 pad] | dtype0 | 9.5e-07 | 1.1e-06 | 7.6e-06 |
| embed_bwd[m0 33x7x768 pad] | dpos | 8.9e-07 | 1.3e-06 | 7.6e-06 |
| embed_bwd[m1 10x54x128 mod5] | d_w | 1.7e-06 | 3.1e-06 | 1.5e-05 |
| embed_bwd[m1 66x54x768 mod33] | d_cls | 9.5e-07 | 1.3e-06 | 7.6e-06 |
| embed_bwd[m1 7x54x128 mod3] | d_masktok | 1.2e-06 | 2.3e-06 | 9.3e-06 |
| embed_bwd[m1 66x54x1000 mod33] | d_cls | 9.5e-07 | 1.3e-06 | 7.6e-06 |
| embed_chain[33x7x768] | dbeta | 6.1e-06 | 1.5e-05 | 4.9e-05 |
| colsum[C8 ld8] | R600 R_dev=1 | 6.0e-08 | 6.0e-08 | 4.8e-07 |
| colsum[C128 ld128] | R600 R_dev=256 | 3.5e-06 | 3.5e-06 | 2.8e-05 |
| colsum[C300 ld304] | R1 R_dev=None | 2.4e-07 | 2.4e-07 | 1.9e-06 |
| colsum[C776 ld776] | R600 R_dev=None | 3.6e-06 | 5.1e-06 | 3.1e-05 |
| gemm_tn_reduce[ns1 3x4] | C | 0.0e+00 | 0.0e+00 | 1.9e-06 |
| gemm_tn_reduce[ns2 3x4] | C | 1.8e-07 | 1.8e-07 | 1.9e-06 |
| gemm_tn_reduce[ns7 3x4] | C | 1.9e-07 | 1.9e-07 | 1.9e-06 |
| gemm_tn_reduce[ns1 128x772] | C | 0.0e+00 | 0.0e+00 | 3.8e-06 |
| gemm_tn_reduce[ns2 128x772] | C | 4.8e-07 | 4.8e-07 | 3.8e-06 |
| gemm_tn_reduce[ns7 128x772] | C | 1.5e-06 | 1.5e-06 | 1.2e-05 |
| gemm_tn_reduce[ns2 1024x2052] | C | 7.2e-07 | 7.2e-07 | 5.7e-06 |
| transpose_bf16[60x40 Rpad192 ldo200] | colsum | 4.8e-07 | 4.8e-07 | 7.6e-06 |
| transpose_bf16[64x64 Rpad64 ldo64] | colsum | 9.2e-07 | 9.2e-07 | 7.6e-06 |
| transpose_bf16[216x300 Rpad256 ldo256] | colsum | 1.9e-06 | 2.4e-06 | 1.5e-05 |
| transpose_bf16[130x70 Rpad136 ldo136] | colsum | 1.2e-06 | 1.2e-06 | 1.5e-05 |
| acc_rows[atomic dup neg] | dst | 2.4e-07 | 2.4e-07 | 1.9e-06 |
| acc_rows[strided idx=yes] | dst | 2.4e-07 | 2.4e-07 | 1.9e-06 |
| acc_rows[strided idx=none] | dst | 2.4e-07 | 2.4e-07 | 1.9e-06 |
| acc_rows[2731x768 atomic=False] | dst | 2.4e-07 | 2.4e-07 | 1.9e-06 |
| acc_rows[2731x768 atomic=True] | dst | 2.4e-07 | 2.4e-07 | 1.9e-06 |
| gelu_bwd[n8] | out | 1.8e-09 | 2.6e-16 | 4.8e-07 |
| gelu_bwd[n4194312] | out | 5.7e-07 | 3.0e-08 | 4.6e-06 |
| segment_sum[W8] | out | 0.0e+00 | 0.0e+00 | 1.9e-06 |
| segment_sum[W2056] | out | 0.0e+00 | 0.0e+00 | 3.8e-06 |

The chain's E32 above holds the bf16 storage of z and dz.  The same comparison with a plain fp32 restatement, nothing rounded to bf16:
  embed_chain[33x7x768] dword: E32 of plain fp32 = 1.080e-06 (bound it would give 8.642e-06)
  embed_chain[33x7x768] dpos: E32 of plain fp32 = 2.775e-06 (bound it would give 2.220e-05)
  embed_chain[33x7x768] dtype0: E32 of plain fp32 = 4.356e-06 (bound it would give 3.485e-05)
  embed_chain[33x7x768] dgamma: E32 of plain fp32 = 8.392e-06 (bound it would give 6.714e-05)
  embed_chain[33x7x768] dbeta: E32 of plain fp32 = 6.110e-06 (bound it would give 4.888e-05)
"""
import copy

import numpy as np

import pytest
import torch

from helpers_gpu import _host_dropout_keep, check_ref, f32_bound

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32, F64 = torch.float32, torch.float64
SENT = 7.0
EPS = 1e-12
CAP = 2048 * 256            # work items of one pass of a grid-stride helper (grid_for / blocks_for cap at 2048 workgroups of 256)
SEED_V = 20261019


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops as o
    return o


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=gen(seed)) * scale


def rbf(*shape, seed, scale=1.0):
    """Random values a kernel reads as bf16 (CPU, bf16)."""
    return randn(*shape, seed=seed, scale=scale).to(BF)


def full(shape, dtype=F32, v=SENT):
    return torch.full(shape, v, dtype=dtype, device="cuda")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def is_sent(t):
    return bool((t == SENT).all())


def dscale(p):
    """1 / (1 - p) as the entry points form it, in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def dev_seed():
    return torch.tensor([SEED_V], dtype=torch.int64, device="cuda")


def host_keep(salt, rows, H, p):
    return torch.from_numpy(np.ascontiguousarray(_host_dropout_keep(SEED_V, salt, np.arange(rows), H, p)))


def keep_rate_in_band(keep, p):
    n, pt = keep.numel(), int(p * 65536 + 0.5) / 65536
    return abs((1 - keep.double().mean().item()) - pt) < 4 * (pt * (1 - pt) / n) ** 0.5


# ---------------------------------------------------------------------------------------------------------------------
# Embeddings: the references
# ---------------------------------------------------------------------------------------------------------------------
class EmbCase:
    """Inputs of one embed_ln_fwd launch (CPU tensors)."""

    def __init__(self, mode, nseq, L, H, *, src_mod=1, seed=0, V=50):
        self.mode, self.nseq, self.L, self.H, self.src_mod, self.V = mode, nseq, L, H, src_mod, V
        self.name = f"m{mode} {nseq}x{L}x{H}" + (f" mod{src_mod}" if mode == 1 else "")
        s = 1000 * seed + 7 * H + nseq
        self.pos, self.type0 = randn(L + 8, H, seed=s + 1), randn(H, seed=s + 2)
        self.gamma, self.beta = 1 + 0.2 * randn(H, seed=s + 3), 0.2 * randn(H, seed=s + 4)
        if mode == 0:
            self.word = randn(V, H, seed=s + 5)
            ids = torch.randint(1, V, (nseq, L), generator=gen(s + 6))
            ids[:, -2:] = 0                                  # PAD: an ordinary row in the forward, skipped in the backward
            ids[0, 0] = 0
            ids[-1, 1] = ids[0, 1]                           # a repeated id
            self.ids = ids.int()
        elif mode == 2:
            self.emb = randn(nseq * L, H, seed=s + 5)
        else:
            self.pv_x = randn(src_mod, L - 1, seed=s + 5)
            m = (torch.rand(src_mod, L - 1, generator=gen(s + 6)) < 0.5).float()
            m[0] = 0.0                                       # a source with nothing masked, one with everything masked, the rest mixed
            if src_mod > 1:
                m[1] = 1.0
            self.pv_mask = m
            self.pv_w, self.pv_b, self.pv_cls, self.pv_mt = (randn(H, seed=s + 7 + i) for i in range(4))

    def sources(self):
        d = lambda t: t.cuda()
        if self.mode == 0:
            return dict(ids=d(self.ids), word=d(self.word))
        if self.mode == 2:
            return dict(pv_x=d(self.emb))
        return dict(pv_x=d(self.pv_x), pv_mask=d(self.pv_mask), pv_w=d(self.pv_w), pv_b=d(self.pv_b), pv_cls=d(self.pv_cls),
                    pv_masktok=d(self.pv_mt), src_mod=self.src_mod)


def embed_sum(dt, c, pos0=0, word=None, pos=None, type0=None):
    """z = token + type0 + pos[pos0 + l] as [nseq * L, H] in dtype dt (word / pos / type0: autograd leaves in place of the case's own)."""
    nseq, L, H = c.nseq, c.L, c.H
    pos = (c.pos.to(dt) if pos is None else pos)[pos0:pos0 + L]
    base = pos[None] + (c.type0.to(dt) if type0 is None else type0)
    if c.mode == 0:
        t = (c.word.to(dt) if word is None else word)[c.ids.long()]
    elif c.mode == 2:
        t = c.emb.to(dt).view(nseq, L, H)
    else:
        src = torch.arange(nseq) % c.src_mod
        x, m = c.pv_x.to(dt)[src][:, :, None], c.pv_mask.to(dt)[src][:, :, None]
        body = (x * c.pv_w.to(dt) + c.pv_b.to(dt)) * (1 - m) + c.pv_mt.to(dt) * m
        t = torch.cat([c.pv_cls.to(dt).expand(nseq, 1, H), body], dim=1)
    return (base + t).reshape(nseq * L, H)


def ln_stats(z):
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + EPS)


def ln_ref(z, gamma, beta):
    """-> y, mean [rows], rstd [rows] in z's dtype."""
    mean, rstd = ln_stats(z)
    return (z - mean) * rstd * gamma.to(z.dtype) + beta.to(z.dtype), mean[:, 0], rstd[:, 0]


def run_embed_fwd(ops, c, *, p=0.0, salt=0, gamma=None, beta=None):
    """The launch, with one sentinel row behind every output.  -> y, zout (bf16), mean, rstd (fp32) on the CPU."""
    rows, H = c.nseq * c.L, c.H
    y, z = full((rows + 1, H), BF), full((rows + 1, H), BF)
    mean, rstd = full((rows + 1,)), full((rows + 1,))
    ops.embed_ln_fwd(c.mode, y[:rows], nseq=c.nseq, L=c.L, H=H, pos=c.pos.cuda(), type0=c.type0.cuda(),
                     gamma=(c.gamma if gamma is None else gamma).cuda(), beta=(c.beta if beta is None else beta).cuda(), zout=z[:rows],
                     mean=mean[:rows], rstd=rstd[:rows], eps=EPS, dropout_p=p, seed=dev_seed() if p > 0 else None, salt=salt, **c.sources())
    assert is_sent(y[rows]) and is_sent(z[rows]) and is_sent(mean[rows]) and is_sent(rstd[rows]), "a row past nseq * L was written"
    return y[:rows].cpu(), z[:rows].cpu(), mean[:rows].cpu(), rstd[:rows].cpu()


def check_embed_fwd(name, c, got, keep=None, p=0.0):
    y, z, mean, rstd = got
    z64, z32 = embed_sum(F64, c), embed_sum(F32, c)
    (y64, m64, r64), (y32, m32, r32) = ln_ref(z64, c.gamma, c.beta), ln_ref(z32, c.gamma, c.beta)
    if keep is not None:
        y64, y32 = y64 * keep.double() * dscale(p), y32 * keep.float() * dscale(p)
        assert torch.equal(y[~keep], torch.zeros_like(y[~keep]))
    check_ref(f"{name} y", y, y64, y32, bf16=True)
    check_ref(f"{name} zout", z, z64, z32, bf16=True)
    check_ref(f"{name} mean", mean, m64, m32)
    check_ref(f"{name} rstd", rstd, r64, r32)


# ------------------------------------------------------------------------------------------------ embed_ln_fwd
EMB_FWD = [EmbCase(0, 3, 7, 128), EmbCase(0, 5, 24, 768), EmbCase(0, 2, 9, 1000), EmbCase(0, 4, 6, 1024),          # rows 21, 120, 18, 24
           EmbCase(1, 6, 54, 128, src_mod=3), EmbCase(1, 6, 54, 768, src_mod=3), EmbCase(1, 7, 54, 128, src_mod=3),
           EmbCase(2, 3, 12, 768), EmbCase(2, 2, 5, 1000)]


@pytest.mark.parametrize("c", EMB_FWD, ids=[c.name for c in EMB_FWD])
def test_embed_ln_fwd(ops, c):
    """All four outputs of every mode: y, the stored sum, mean and rstd; row counts that leave the last workgroup partly empty; H with a
    tail chunk (1000); PV sources read by seq % src_mod (7 sequences over 3 sources tells it apart from seq / 2 or seq - B)."""
    check_embed_fwd(f"embed_fwd[{c.name}]", c, run_embed_fwd(ops, c))


@pytest.mark.parametrize("H", [128, 768, 1000])
def test_embed_ln_fwd_dropout(ops, H):
    """y = dropout(LN(z)): the mask is the host model's, element (row, col) by row counter `row`; the kept values are scaled by 1 / (1 - p);
    the stored sum and the statistics are those of the launch without dropout."""
    p, salt = 0.1, 300 + H
    c = EmbCase(0, 5, 7, H, seed=1)                                   # 35 rows: the last workgroup holds three
    rows = c.nseq * c.L
    keep = host_keep(salt, rows, H, p)
    assert keep_rate_in_band(keep, p)
    y1 = run_embed_fwd(ops, c, p=p, salt=salt, gamma=torch.zeros(H), beta=torch.ones(H))[0]          # every normalised value is exactly 1
    assert torch.equal(y1 != 0, keep), f"{int(((y1 != 0) != keep).sum())} of {keep.numel()} decisions differ from the host model"
    assert torch.equal(y1[keep], torch.full_like(y1[keep], dscale(p)))                                    # bf16(1 / (1 - p))
    assert keep_rate_in_band(y1 != 0, p)
    got = run_embed_fwd(ops, c, p=p, salt=salt)
    check_embed_fwd(f"embed_fwd_dropout[H{H}]", c, got, keep=keep, p=p)
    other = run_embed_fwd(ops, c, p=p, salt=salt + 1)[0]
    assert not torch.equal(other != 0, got[0] != 0)                                                       # the salt reaches the mask


# ------------------------------------------------------------------------------------------------ embed_step_ln_fwd
@pytest.mark.parametrize("H", [256, 768, 1000])
@pytest.mark.parametrize("rows", [1, 9])
def test_embed_step_with_device_side_position(ops, rows, H):
    """The position read from device memory (the graph-replayed decoders) wins over pos_index; the step's row is bit for bit the row
    the full embedding writes at that position, and agrees with float64."""
    L, t, t_host = 8, 5, 2
    c = EmbCase(0, rows, L, H, seed=2)
    full_y = run_embed_fwd(ops, c)[0].view(rows, L, H)
    src = c.sources()
    kw = dict(word=src["word"], pos=c.pos.cuda(), type0=c.type0.cuda(), gamma=c.gamma.cuda(), beta=c.beta.cuda(), eps=EPS)
    ids_t = src["ids"][:, t].contiguous()
    y = full((rows + 1, H), BF)
    ops.embed_step_ln_fwd(ids_t, t_host, y[:rows], pos_ptr=torch.tensor([t], dtype=torch.int32, device="cuda"), **kw)
    assert is_sent(y[rows])
    assert same_bits(y[:rows], full_y[:, t]), "pos_ptr did not select the position"
    y0 = full((rows + 1, H), BF)
    ops.embed_step_ln_fwd(ids_t, t_host, y0[:rows], **kw)                                    # without it: pos_index
    one = copy.copy(c)                                                                       # the same tables, the one token of position t
    one.L, one.ids = 1, c.ids[:, t:t + 1].contiguous()
    for got, pos0, nm in ((y, t, "pos_ptr"), (y0, t_host, "pos_index")):
        y64, y32 = ln_ref(embed_sum(F64, one, pos0=pos0), c.gamma, c.beta)[0], ln_ref(embed_sum(F32, one, pos0=pos0), c.gamma, c.beta)[0]
        check_ref(f"embed_step[{rows}x{H} {nm}] y", got[:rows], y64, y32, bf16=True)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward of y = dropout(LN(z))
# ---------------------------------------------------------------------------------------------------------------------
def ln_bwd_ref(dt, dy, dy2, zb, mean, rstd, gamma, keep, ds):
    """The formulas of csrc/rowops.hip::ln_bwd_kernel with drop_on_dy in dtype dt, from the STORED bf16 sum and the forward's statistics."""
    g = dy.to(dt) + (dy2.to(dt) if dy2 is not None else 0)
    g = g * keep.to(dt) * ds
    mean, rstd = mean.to(dt)[:, None], rstd.to(dt)[:, None]
    xh = (zb.to(dt) - mean) * rstd
    dg = g * gamma.to(dt)
    s1, s2 = dg.mean(-1, keepdim=True), (dg * xh).mean(-1, keepdim=True)
    return rstd * (dg - s1 - xh * s2), (g * xh).sum(0), g.sum(0)


def coarse(*shape, seed):
    """Multiples of 1/8 in [-4, 4]: six bits, exact in bf16."""
    return (randn(*shape, seed=seed) * 8).round().clamp(-32, 32) / 8


def unit_rows(rows, H, seed):
    """Rows with mean exactly 0 and variance exactly 1 in any summation order: H/8 values +-2, H/2 values +-0.5, 3H/8 values +-1, half of
    each positive, in a random order per row."""
    half = torch.cat([torch.full((H // 16,), 2.0), torch.full((H // 4,), 0.5), torch.full((3 * H // 16,), 1.0)])
    pat = torch.cat([half, -half])
    assert pat.numel() == H and pat.sum() == 0 and (pat * pat).sum() == H
    order = torch.rand(rows, H, generator=gen(seed)).argsort(dim=1)
    return pat[order]


# rows, H, as nseq x L of the forward, p.  Every column of dgamma and dbeta reaches memory through one fp32 atomic per workgroup; at 1237
# rows that is 256 atomics per column, in any order, and with ordinary inputs (24-bit terms g * xhat and g) the order alone moved the result
# between 0.4 and 0.7 of the bound for dbeta on the GPU (two runs at p = 0.1) and, in a CPU simulation of the launch's summation over 300 orders,
# past the bound for dgamma in a few per cent of them.  The inputs of that case are therefore chosen so that every partial sum is exact in
# fp32: p = 0.5 (1 / (1 - p) = 2), gradients and initial contents in multiples of 1/8, and rows of z with mean 0 and variance 1 exactly
# (unit_rows: xhat = z in {+-0.5, +-1, +-2} as long as rsqrt(1) = 1).  What the case is for -- more than one row-loop pass per wave, the
# prefetch of the next row, the mask per row -- does not depend on the values; the ordinary values are in the other four shapes.
LN_BWD = [(21, 128, 3, 7, 0.1), (333, 768, 9, 37, 0.1), (5, 1000, 5, 1, 0.1), (64, 1024, 4, 16, 0.1), (1237, 768, 1237, 1, 0.5)]


@pytest.mark.parametrize("rows,H,nseq,L,p", LN_BWD)
def test_ln_bwd_drop_on_dy(ops, rows, H, nseq, L, p):
    """ln_bwd(drop_on_dy) behind the forward that drew the mask (same seed, salt, rows): dz, dgamma, dbeta from the stored bf16 sum and the
    returned statistics; with a second incoming gradient; without dgamma / dbeta (the early return).  1237 rows: more than one row per
    wave at the 256-workgroup floor."""
    salt = 500 + H
    c = EmbCase(2, nseq, L, H, seed=3)
    exact = rows > 1024
    if exact:
        c.emb, c.pos, c.type0 = unit_rows(rows, H, seed=35), torch.zeros_like(c.pos), torch.zeros_like(c.type0)
    keep = host_keep(salt, rows, H, p)
    y, zb, mean, rstd = run_embed_fwd(ops, c, p=p, salt=salt)
    assert torch.equal(y == 0, ~keep) or int(((y == 0) != ~keep).sum()) <= 2          # (a normalised value that is itself 0 aside)
    mk = (lambda *sh, seed: coarse(*sh, seed=seed)) if exact else randn
    dy, dy2 = mk(rows, H, seed=31).to(BF), mk(rows, H, seed=32).to(BF)
    g0, b0 = mk(H, seed=33), mk(H, seed=34)                                           # the gradients accumulate onto these
    zd, md, rd, gd = zb.cuda(), mean.cuda(), rstd.cuda(), c.gamma.cuda()
    for nm, d2, stats in (("", None, True), (" dy2", dy2, True), (" no dgamma", None, False)):
        dz = full((rows + 1, H), BF)
        dg, db = (g0.cuda(), b0.cuda()) if stats else (None, None)
        ops.ln_bwd(dy.cuda(), zd, md, rd, gd, dz[:rows], dy2=None if d2 is None else d2.cuda(), dgamma=dg, dbeta=db, dropout_p=p,
                   seed=dev_seed(), salt=salt, drop_on_dy=True)
        assert is_sent(dz[rows])
        r64, r32 = (ln_bwd_ref(dt, dy, d2, zb, mean, rstd, c.gamma, keep, dscale(p)) for dt in (F64, F32))
        name = f"ln_bwd_drop_on_dy[{rows}x{H}{nm}]"
        check_ref(f"{name} dz", dz[:rows], r64[0], r32[0], bf16=True)
        if stats:
            check_ref(f"{name} dgamma", dg, g0.double() + r64[1], g0 + r32[1])
            check_ref(f"{name} dbeta", db, b0.double() + r64[2], b0 + r32[2])


# ---------------------------------------------------------------------------------------------------------------------
# Embedding backward
# ---------------------------------------------------------------------------------------------------------------------
def embed_bwd_ref(dt, c, dz, init):
    """-> dict of the accumulated gradients in dtype dt; dz [nseq * L, H] bf16, init: the buffers' contents before the launch."""
    nseq, L, H = c.nseq, c.L, c.H
    g = dz.to(dt).view(nseq, L, H)
    out = {k: v.to(dt).clone() for k, v in init.items()}
    out["dpos"][:L] += g.sum(0)
    out["dtype0"] += g.sum((0, 1))
    if c.mode == 0:
        ids = c.ids.long().reshape(-1)
        live = ids != 0
        out["dword"].index_add_(0, ids[live], g.reshape(-1, H)[live])
    else:
        src = torch.arange(nseq) % c.src_mod
        x, m = c.pv_x.to(dt)[src][:, :, None], c.pv_mask.to(dt)[src][:, :, None]
        gb = g[:, 1:]
        out["d_w"] += (gb * (1 - m) * x).sum((0, 1))
        out["d_b"] += (gb * (1 - m)).sum((0, 1))
        out["d_masktok"] += (gb * m).sum((0, 1))
        out["d_cls"] += g[:, 0].sum(0)
    return out


def run_embed_bwd(ops, c, dz, init):
    d = {k: v.cuda() for k, v in init.items()}
    kw = dict(ids=c.ids.cuda(), dword=d["dword"]) if c.mode == 0 else \
        dict(pv_x=c.pv_x.cuda(), pv_mask=c.pv_mask.cuda(), src_mod=c.src_mod, d_w=d["d_w"], d_b=d["d_b"], d_cls=d["d_cls"], d_masktok=d["d_masktok"])
    ops.embed_bwd(c.mode, dz.cuda(), nseq=c.nseq, L=c.L, H=c.H, dpos=d["dpos"], dtype0=d["dtype0"], **kw)
    return {k: v.cpu() for k, v in d.items()}


def embed_bwd_init(c, seed):
    init = dict(dpos=randn(c.L + 8, c.H, seed=seed), dtype0=randn(c.H, seed=seed + 1))
    if c.mode == 0:
        init["dword"] = randn(c.V, c.H, seed=seed + 2)
    else:
        init.update({k: randn(c.H, seed=seed + 3 + i) for i, k in enumerate(("d_w", "d_b", "d_cls", "d_masktok"))})
    return init


def check_embed_bwd(name, c, dz, init, got):
    r64, r32 = embed_bwd_ref(F64, c, dz, init), embed_bwd_ref(F32, c, dz, init)
    for k in init:
        check_ref(f"{name} {k}", got[k], r64[k], r32[k])
    assert same_bits(got["dpos"][c.L:], init["dpos"][c.L:]), "a position past L was written"


# nseq 6: one slice of sequences per position; 32: sixteen slices of two; 33: s_per = 3, slices 11..15 empty; 47: the last slice short
EMB_BWD0 = [(6, 128, "mixed"), (32, 768, "mixed"), (33, 1000, "mixed"), (47, 768, "mixed"), (33, 128, "same"), (47, 1000, "same"),
            (6, 768, "pad"), (33, 768, "pad")]


@pytest.mark.parametrize("nseq,H,kind", EMB_BWD0)
def test_embed_bwd_text(ops, nseq, H, kind):
    """Text embedding backward on both launch shapes, onto non-zero gradients: `same` = every sequence holds the same token at a
    position (all of a column's atomics land on one dword row), `pad` = every id is PAD (dword stays bit for bit what it was)."""
    c = EmbCase(0, nseq, 7, H, seed=4)
    if kind == "same":
        c.ids = torch.tensor([5, 9, 5, 0, 17, 1, 49], dtype=torch.int32).repeat(nseq, 1)
    elif kind == "pad":
        c.ids = torch.zeros(nseq, 7, dtype=torch.int32)
    dz, init = rbf(nseq * 7, H, seed=41), embed_bwd_init(c, 42)
    if kind == "pad":
        init["dword"] = torch.full((c.V, H), SENT)
    got = run_embed_bwd(ops, c, dz, init)
    check_embed_bwd(f"embed_bwd[m0 {nseq}x7x{H} {kind}]", c, dz, init, got)
    assert same_bits(got["dword"][0], init["dword"][0]), "the PAD row received a gradient"
    if kind == "pad":
        assert same_bits(got["dword"], init["dword"])


@pytest.mark.parametrize("nseq,src_mod,H", [(10, 5, 128), (66, 33, 768), (7, 3, 128), (66, 33, 1000)])
def test_embed_bwd_pv(ops, nseq, src_mod, H):
    """PV embedding backward on both launch shapes (10 sequences: one slice; 66: thirteen slices of five, one of one, two empty), sources by
    seq % src_mod.  The property values are multiples of 1/4 here: with dz in bf16 the products g * (1 - m) * x then have 13-bit mantissas
    and the fp32 partial sums of d_w stay as close to exact as those of the other column sums (terms of 8 bits).  With 24-bit values the 742
    atomics per column of the 66 x 54 launch come to 0.4 - 0.8 of the bound depending on their order in a CPU simulation of the launch's
    summation, 0.6 and 0.9 in the one run on the GPU: a case that would fail now and then without any fault in the kernel."""
    c = EmbCase(1, nseq, 54, H, src_mod=src_mod, seed=5)
    c.pv_x = (c.pv_x * 4).round().clamp(-16, 16) / 4
    dz, init = rbf(nseq * 54, H, seed=43), embed_bwd_init(c, 44)
    check_embed_bwd(f"embed_bwd[m1 {nseq}x54x{H} mod{src_mod}]", c, dz, init, run_embed_bwd(ops, c, dz, init))


def test_embedding_chain_against_autograd(ops):
    """The three launches the step chains -- embed_ln_fwd, ln_bwd(drop_on_dy), embed_bwd with one seed and salt -- against float64 autograd
    of sum(dy * dropout(LN(word[ids] + type0 + pos))) under the host mask.  ref32: fp32 with the two tensors the chain stores as bf16
    (the sum z and its gradient dz) rounded where it stores them (see the head of this file)."""
    nseq, L, H, p, salt = 33, 7, 768, 0.1, 77
    c = EmbCase(0, nseq, L, H, seed=6)
    rows, ds = nseq * L, dscale(p)
    keep = host_keep(salt, rows, H, p)
    dy = rbf(rows, H, seed=51)
    # ---- the chain
    y, zb, mean, rstd = run_embed_fwd(ops, c, p=p, salt=salt)
    dz = full((rows, H), BF)
    dg, db = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
    ops.ln_bwd(dy.cuda(), zb.cuda(), mean.cuda(), rstd.cuda(), c.gamma.cuda(), dz, dgamma=dg, dbeta=db, dropout_p=p, seed=dev_seed(), salt=salt,
               drop_on_dy=True)
    init = dict(dpos=torch.zeros(L + 8, H), dtype0=torch.zeros(H), dword=torch.zeros(c.V, H))
    got = run_embed_bwd(ops, c, dz.cpu(), init)
    got.update(dgamma=dg.cpu(), dbeta=db.cpu())
    # ---- float64 autograd of the whole expression
    leaf = {k: getattr(c, k).double().requires_grad_(True) for k in ("word", "pos", "type0", "gamma", "beta")}
    z = embed_sum(F64, c, word=leaf["word"], pos=leaf["pos"], type0=leaf["type0"])
    m_, r_ = ln_stats(z)
    out = ((z - m_) * r_ * leaf["gamma"] + leaf["beta"]) * keep.double() * ds
    (out * dy.double()).sum().backward()
    r64 = dict(dword=leaf["word"].grad.clone(), dpos=leaf["pos"].grad, dtype0=leaf["type0"].grad, dgamma=leaf["gamma"].grad, dbeta=leaf["beta"].grad)
    r64["dword"][0] = 0                                              # nn.Embedding(padding_idx=0): PAD takes no gradient
    # ---- fp32 with the chain's bf16 storage
    z32 = embed_sum(F32, c)
    m32, r32s = ln_stats(z32)
    dz32, dg32, db32 = ln_bwd_ref(F32, dy, None, z32.to(BF), m32[:, 0], r32s[:, 0], c.gamma, keep, ds)
    r32 = embed_bwd_ref(F32, c, dz32.to(BF), init)
    r32.update(dgamma=dg32, dbeta=db32)
    check_ref("embed_chain[33x7x768] y", y, out.detach(), ln_ref(z32, c.gamma, c.beta)[0] * keep.float() * ds, bf16=True)
    # ---- plain fp32, nothing rounded to bf16: printed next to the E32 in use, to show what the storage model adds to the bound
    dzp, dgp, dbp = ln_bwd_ref(F32, dy, None, z32, m32[:, 0], r32s[:, 0], c.gamma, keep, ds)
    g32 = dzp.view(nseq, L, H)
    ids = c.ids.long().reshape(-1)
    plain = dict(dpos=torch.zeros(L + 8, H), dtype0=g32.sum((0, 1)), dgamma=dgp, dbeta=dbp,
                 dword=torch.zeros(c.V, H).index_add_(0, ids[ids != 0], dzp[ids != 0]))
    plain["dpos"][:L] = g32.sum(0)
    for k in ("dword", "dpos", "dtype0", "dgamma", "dbeta"):
        print(f"[e32] embed_chain[33x7x768] {k}: E32 of plain fp32 = {f32_bound(r64[k], plain[k])[0]:.3e} (bound it would give {f32_bound(r64[k], plain[k])[1]:.3e})")
        check_ref(f"embed_chain[33x7x768] {k}", got[k], r64[k], r32[k])


# ---------------------------------------------------------------------------------------------------------------------
# Column sums, slab reduce
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,ld", [(8, 8), (128, 128), (300, 304), (776, 776)])
def test_colsum_bf16(ops, C, ld):
    """out[c] += sum over the first min(R, *R_dev) rows: one row, one short of / exactly / one past a 256-row strip, three strips; the scalar
    tail of a row whose length is no multiple of 8; rows past the device-side count and the row padding hold NaN; out starts non-zero and
    has sentinels behind column C."""
    nan = float("nan")
    for R in (1, 255, 256, 257, 600):
        x = torch.full((R, ld), nan, dtype=BF)
        x[:, :C] = rbf(R, C, seed=60 + R)
        init = torch.cat([randn(C, seed=61), torch.full((8,), SENT)])
        for Rd in (None, 0, 1, 256, 257, R):
            n = R if Rd is None else min(R, Rd)
            xd = x.clone()
            xd[n:] = nan
            out = init.cuda()
            ops.colsum_bf16(xd.cuda()[:, :C], out[:C], R_dev=None if Rd is None else torch.tensor([Rd], dtype=torch.int32, device="cuda"))
            assert is_sent(out[C:]), (R, Rd)
            if n == 0:
                assert same_bits(out, init)
            check_ref(f"colsum[C{C} ld{ld}] R{R} R_dev={Rd}", out[:C], init[:C].double() + x[:n, :C].double().sum(0),
                      init[:C] + x[:n, :C].float().sum(0))


@pytest.mark.parametrize("ns,N,K", [(1, 3, 4), (2, 3, 4), (7, 3, 4), (1, 128, 772), (2, 128, 772), (7, 128, 772), (2, 1024, 2052)])
def test_gemm_tn_reduce(ops, ns, N, K):
    """C[n, :K] += sum over the ns slabs, C at a row stride past K whose padding stays untouched; 1024 x 2052: N * K / 4 = 525 312 float4
    groups, past the 2048 x 256 one pass of the launch covers (gemm_tn.hip::tn_reduce_launch)."""
    from spmm_amd._lib import lib
    ldc = K + 4
    assert (N * K // 4 > CAP) == (N == 1024)
    ws = randn(ns, N, K, seed=70 + ns)
    init = torch.full((N + 1, ldc), SENT)
    init[:N, :K] = randn(N, K, seed=71)
    wd, Cd = ws.cuda(), init.cuda()
    lib().call("spmm_gemm_tn_reduce", ops._p(wd), ns, N, K, ops._p(Cd), ldc, ops._st())
    got = Cd.cpu()
    assert is_sent(got[:N, K:]) and is_sent(got[N])
    s32 = ws[0].clone()
    for z in range(1, ns):
        s32 += ws[z]
    check_ref(f"gemm_tn_reduce[ns{ns} {N}x{K}] C", got[:N, :K], init[:N, :K].double() + ws.double().sum(0), init[:N, :K] + s32)


# ---------------------------------------------------------------------------------------------------------------------
# Layout helpers
# ---------------------------------------------------------------------------------------------------------------------
# (60, 40): C < 64, tile rows 64.. and 128.. are pure padding, ldo past Rpad; (64, 64): one full tile, Rpad == R; (216, 300): a column slice
@pytest.mark.parametrize("R,C,Rpad,ldo,off", [(60, 40, 192, 200, 0), (64, 64, 64, 64, 0), (216, 300, 256, 256, 10), (130, 70, 136, 136, 0)])
def test_transpose_bf16(ops, R, C, Rpad, ldo, off):
    big = rbf(R, C + 2 * off, seed=80 + R)
    x = big[:, off:off + C]
    init = randn(C, seed=81)
    for with_sum in (True, False):
        out = full((C + 1, ldo), BF)
        cs = torch.cat([init, torch.full((8,), SENT)]).cuda()
        ops.transpose_bf16(big.cuda()[:, off:off + C], out[:C], Rpad=Rpad, colsum=cs[:C] if with_sum else None)
        o = out.cpu()
        assert same_bits(o[:C, :R], x.t().contiguous())
        assert same_bits(o[:C, R:Rpad], torch.zeros(C, Rpad - R, dtype=BF))
        assert is_sent(o[:C, Rpad:]) and is_sent(o[C]), "written past Rpad or past row C"
        assert is_sent(cs[C:])
        if with_sum:
            check_ref(f"transpose_bf16[{R}x{C} Rpad{Rpad} ldo{ldo}] colsum", cs[:C], init.double() + x.double().sum(0), init + x.float().sum(0))
        else:
            assert same_bits(cs[:C], init)


@pytest.mark.parametrize("R,C", [(130, 70), (64, 64), (1, 5)])
def test_cast_transpose(ops, R, C):
    w = randn(R, C, seed=82)
    wb = w.to(BF)
    for want_out, want_T in ((True, True), (False, True), (True, False)):
        o, oT = full((R * C + 8,), BF), full((R * C + 8,), BF)
        ops.cast_transpose(w.cuda(), o[:R * C].view(R, C) if want_out else None, oT[:R * C].view(C, R) if want_T else None)
        assert is_sent(o[R * C:]) and is_sent(oT[R * C:])
        assert same_bits(o[:R * C].view(R, C), wb) if want_out else is_sent(o)
        assert same_bits(oT[:R * C].view(C, R), wb.t().contiguous()) if want_T else is_sent(oT)


# fp32 words: ties to even in both directions (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6), their negatives, just past a tie, the largest
# finite value (rounds to inf), +-0, +-inf, NaN.  No subnormals: the project does not specify their treatment.
SPECIAL_WORDS = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000000, 0x80000000,
                 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7F8000, 0x00800000, 0x3F800000]


def special_f32():
    return torch.from_numpy(np.array(SPECIAL_WORDS, dtype=np.uint32).view(np.float32).copy())


@pytest.mark.parametrize("n", [4, 16, 4 * CAP + 20])
def test_cast_f32_bf16_and_back(ops, n):
    """Round to nearest even, bit for bit torch's conversion; n / 4 past the cap: a second grid-stride pass, with the special values at
    both ends.  The way back is exact."""
    x = randn(n, seed=83, scale=3.0)
    if n >= 16:
        x[:16] = special_f32()
    if n >= 32:
        x[-16:] = special_f32().flip(0)
    want = x.to(BF)
    o = full((n + 8,), BF)
    ops.cast_f32_bf16(x.cuda(), o[:n])
    got = o[:n].cpu()
    nanm = torch.isnan(want)
    assert is_sent(o[n:]) and torch.equal(torch.isnan(got), nanm)
    assert torch.equal(bits(got)[~nanm], bits(want)[~nanm])
    if n >= 16:
        assert torch.isinf(got[6]) and got[0] == 1.0 and bits(got)[1] == 0x3F82 and got[8:10].tolist() == [0.0, 0.0]      # the block is there
    back = full((n + 4,))
    ops.cast_bf16_f32(want.cuda(), back[:n])
    b, wf = back[:n].cpu(), want.float()
    assert is_sent(back[n:]) and torch.equal(torch.isnan(b), nanm)
    assert torch.equal(bits(b)[~nanm], bits(wf)[~nanm])


def test_acc_rows(ops):
    H = 128
    src = rbf(7, H, seed=84)
    # ---- atomic, duplicate and negative indices
    idx = torch.tensor([3, 3, -1, 0, 9, 3, -5])
    init = torch.cat([randn(10, H, seed=85), torch.full((1, H), SENT)])
    dst = init.cuda()
    ops.acc_rows(dst[:10], src.cuda(), idx=idx.cuda(), atomic=True)
    live = idx >= 0
    r64, r32 = (init[:10].to(dt).index_add_(0, idx[live], src.to(dt)[live]) for dt in (F64, F32))
    check_ref("acc_rows[atomic dup neg] dst", dst[:10], r64, r32)
    assert is_sent(dst[10]) and same_bits(dst[[1, 2, 4, 5, 6, 7, 8]], init[[1, 2, 4, 5, 6, 7, 8]])
    # ---- not atomic, dst and src at row strides past H, with unique indices and without indices
    sbig = torch.full((7, H + 12), float("nan"), dtype=BF)
    sbig[:, 4:4 + H] = src
    for idx2 in (torch.tensor([6, 0, -1, 2, 5, 1, 3]), None):
        init2 = torch.full((8, H + 8), SENT)
        init2[:7, :H] = randn(7, H, seed=86)
        d2 = init2.cuda()
        ops.acc_rows(d2[:7, :H], sbig.cuda()[:, 4:4 + H], idx=None if idx2 is None else idx2.cuda())
        ii = torch.arange(7) if idx2 is None else idx2
        r64, r32 = (init2[:7, :H].to(dt).index_add_(0, ii[ii >= 0], src.to(dt)[ii >= 0]) for dt in (F64, F32))
        check_ref(f"acc_rows[strided idx={'yes' if idx2 is not None else 'none'}] dst", d2[:7, :H], r64, r32)
        assert is_sent(d2[:, H:]) and is_sent(d2[7])
    # ---- rows * H / 4 past the cap
    rows, H = 2731, 768
    assert rows * (H // 4) > CAP >= (rows - 1) * (H // 4)
    src = rbf(rows, H, seed=87)
    perm = torch.randperm(rows, generator=gen(88))
    perm[5] = perm[rows - 3] = -1
    perm[rows - 1] = perm[0]                                       # one duplicate, in the second pass
    for idx3, atomic in ((None, False), (perm, True)):
        init3 = torch.cat([randn(rows, H, seed=89), torch.full((1, H), SENT)])
        d3 = init3.cuda()
        ops.acc_rows(d3[:rows], src.cuda(), idx=None if idx3 is None else idx3.cuda(), atomic=atomic)
        ii = torch.arange(rows) if idx3 is None else idx3
        r64, r32 = (init3[:rows].to(dt).index_add_(0, ii[ii >= 0], src.to(dt)[ii >= 0]) for dt in (F64, F32))
        check_ref(f"acc_rows[{rows}x{H} atomic={atomic}] dst", d3[:rows], r64, r32)
        assert is_sent(d3[rows])


@pytest.mark.parametrize("rows,H", [(5, 8), (5, 768), (CAP + 2, 8), (5462, 768)])
def test_gather_and_add_rows(ops, rows, H):
    """gather_rows, gather_rows2 (negative index: a zero row; SRC_B: the second source, or the first when there is none) and add_rows_bf16
    (unique indices); rows * H / 8 past the cap in the last two."""
    nsrc = rows + 3
    assert (rows * (H // 8) > CAP) == (rows > 5)
    A, B = rbf(nsrc, H, seed=90), rbf(nsrc, H, seed=91)
    idx = torch.randint(0, nsrc, (rows,), generator=gen(92))
    idx[0] = idx[rows - 1] = nsrc - 1
    Ad, Bd = A.cuda(), B.cuda()
    dst = full((rows + 1, H), BF)
    ops.gather_rows(dst[:rows], Ad, idx.cuda())
    assert same_bits(dst[:rows], A[idx]) and is_sent(dst[rows])
    # ---- two sources
    pick = torch.randint(0, 3, (rows,), generator=gen(93))              # 0: A, 1: B, 2: a zero row
    pick[0], pick[rows - 1] = 2, 1
    idx2 = torch.where(pick == 2, torch.full_like(idx, -1 - 7), idx + (pick == 1).long() * ops.SRC_B)
    for srcB, Bref in ((Bd, B), (None, A)):
        dst = full((rows + 1, H), BF)
        ops.gather_rows2(dst[:rows], Ad, idx2.cuda(), srcB)
        want = torch.where((pick == 1)[:, None], Bref[idx], A[idx])
        want[pick == 2] = 0
        assert same_bits(dst[:rows], want) and is_sent(dst[rows])
    # ---- dst[idx[r]] += src[r], every index once
    perm = torch.randperm(nsrc, generator=gen(94))[:rows]
    d0 = rbf(nsrc, H, seed=95)
    dd = torch.cat([d0, torch.full((1, H), SENT, dtype=BF)]).cuda()
    ops.add_rows_bf16(dd[:nsrc], perm.cuda(), Ad[:rows])
    want = d0.float()
    want[perm] += A[:rows].float()
    assert same_bits(dd[:nsrc], want.to(BF)) and is_sent(dd[nsrc])


def test_zero_fill(ops):
    """ops.zero_ on contiguous tensors (spmm_zero_bytes) and on column slices (spmm_zero_rows), 16-byte groups past the cap, sentinels
    on every side."""
    for n in (8, 8 * CAP + 8):                                    # bf16 elements: 1 and CAP + 1 groups of 16 bytes
        buf = full((n + 16,), BF)
        ops.zero_(buf[8:8 + n])
        assert is_sent(buf[:8]) and is_sent(buf[8 + n:]) and not buf[8:8 + n].any()
    for rows, W in ((3, 8), (5462, 768)):
        assert (rows * (W // 8) > CAP) == (rows > 3)
        big = full((rows + 1, W + 16), BF)
        t = big[:rows, 8:8 + W]
        assert not t.is_contiguous()
        ops.zero_(t)
        assert not t.any() and is_sent(big[:, :8]) and is_sent(big[:, 8 + W:]) and is_sent(big[rows])
    f = full((4, 12))                                             # fp32, four columns of a row: 16 bytes at a 48-byte stride
    ops.zero_(f[:, 4:8])
    assert not f[:, 4:8].any() and is_sent(f[:, :4]) and is_sent(f[:, 8:])


def _gelu_bwd_ref(dt, dz, pre):
    x = pre.to(dt)
    cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752))
    pdf = 0.3989422804014327 * torch.exp(-0.5 * x * x)
    return dz.to(dt) * (cdf + x * pdf)


@pytest.mark.parametrize("n", [8, 8 * CAP + 8])
def test_gelu_bwd(ops, n):
    """out = dz * gelu'(pre) at 0, +-0.5, +-8, +-12 and the largest finite bf16 (the density underflows; its product with x must be 0, not
    NaN); n / 8 past the cap."""
    big = float(torch.finfo(BF).max)
    special = torch.tensor([0.0, 0.5, -0.5, 8.0, -8.0, 12.0, -12.0, big, -big, -0.0, 1.0, -1.0, 3.0, -3.0, 0.125, -5.0])
    pre = rbf(n, seed=96, scale=2.0)
    if n == 8:
        pre = special[:8].to(BF)
    else:
        pre[:16] = special.to(BF)
        pre[-16:] = special.flip(0).to(BF)
    dz = rbf(n, seed=97)
    out = full((n + 8,), BF)
    ops.gelu_bwd(dz.cuda(), pre.cuda(), out[:n])
    assert is_sent(out[n:])
    check_ref(f"gelu_bwd[n{n}] out", out[:n], _gelu_bwd_ref(F64, dz, pre), _gelu_bwd_ref(F32, dz, pre), bf16=True)
    if n > 8:
        neg_big = out[:16].cpu()[8].item()
        assert neg_big == 0.0, neg_big


@pytest.mark.parametrize("W", [8, 2056])
def test_segment_sum_bf16(ops, W):
    """out[u] = sum of the listed rows in fp32: an empty segment is zeros, a single member a bit-equal copy; W / 8 = 257 vectors takes a
    second workgroup along x."""
    nsrc = 9
    src = rbf(nsrc, W, seed=98)
    segs = [[4], [], [0, 8, 3, 3, 7], [2, 1], []]
    start = torch.tensor([0] + list(np.cumsum([len(s) for s in segs])), dtype=torch.int32)
    lst = torch.tensor([k for s in segs for k in s], dtype=torch.int32)
    U = len(segs)
    out = full((U + 1, W), BF)
    ops.segment_sum_bf16(src.cuda(), start.cuda(), lst.cuda(), out[:U])
    o = out.cpu()
    assert is_sent(o[U])
    assert same_bits(o[0], src[4]) and same_bits(o[1], torch.zeros(W, dtype=BF)) and same_bits(o[4], torch.zeros(W, dtype=BF))
    r64 = torch.stack([src[s].double().sum(0) if s else torch.zeros(W, dtype=F64) for s in segs])
    r32 = torch.stack([src[s].float().sum(0) if s else torch.zeros(W) for s in segs])
    check_ref(f"segment_sum[W{W}] out", o[:U], r64, r32, bf16=True)
