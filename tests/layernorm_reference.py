"""The residual LayerNorm kernels of csrc/rowops.hip (spmm_ln_fwd, spmm_ln_bwd without drop_on_dy) restated in plain torch on the CPU, in a
dtype `dt` of the caller's choice: float64 is the reference, float32 the `ref32` of helpers_gpu.check_ref.  Nothing here touches a GPU;
tests/test_layernorm_reference_cpu.py checks this file, tests/test_layernorm_gpu.py holds the kernels to it.

Forward   z = x * keep / (1 - p) + res        keep: the host model of the dropout hash, row counter = row; 1 / (1 - p) formed in fp32
          mean = mean_H(z),  var = mean_H((z - mean)^2),  rstd = rsqrt(var + eps), and 0 where var + eps is not > 0
          y = (z - mean) * rstd * gamma + beta,  zout = z
Backward  from the STORED bf16 tensor and the statistics it is given (not from x):
          g = dy + dy2
          xhat = (z - mean) * rstd                         stored-sum form
               = (y - beta) * (1 / gamma), 0 at gamma == 0  from-output form (`beta_from_y`)
          dz = rstd * (g gamma - mean_H(g gamma) - xhat mean_H(g gamma xhat))
          dx = keep ? dz / (1 - p) : 0     the mask meets the unrounded dz; dx is rounded once
          dgamma += sum_rows g xhat,  dbeta += sum_rows g,  dxsum += sum_rows bf16(dx)    (of bf16(dz) when no dx is asked for)
dxsum is taken from the bf16 tensor the launch itself wrote (colsum_ref): that is what the kernel adds, and an ulp flip of one bf16
element belongs to the comparison of dx, not to the sum's.

exact_case() builds inputs on which every output of the backward is exact in its number format and every partial sum exact in fp32 in
any order, for the row counts at which the order of the launch's fp32 atomics alone could pass check_ref's bound (more than one pass
of the row loop: above 1024 rows)."""
import numpy as np
import torch

from helpers_gpu import _host_dropout_keep

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-12
XHAT = (0.5, 1.0, 2.0)                              # magnitudes of the normalised values and of gamma in the exact cases
ZERO_CH, SMALL_CH, NEG_CH = 1, 2, 3                 # channels of gamma == 0, gamma == -0.03 and a negative ordinary gamma


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def dscale(p):
    """1 / (1 - p) as the entry points form it, in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def host_keep(seed, salt, rows, H, p, row0=0):
    """bool [rows, H]: element (r, c) is kept; the row counter of row r is row0 + r.  None at p == 0 (the kernels draw nothing)."""
    if p == 0:
        return None
    return torch.from_numpy(np.ascontiguousarray(_host_dropout_keep(seed, salt, np.arange(row0, row0 + rows), H, p)))


# ---------------------------------------------------------------------------------------------------------------------
# The formulas
# ---------------------------------------------------------------------------------------------------------------------
def ln_fwd_ref(dt, x, res, gamma, beta, keep=None, p=0.0, eps=EPS):
    """-> dict y, zout [rows, H], mean, rstd [rows] in dtype dt.  x, res (or None): what the kernel reads (bf16); keep: host_keep()."""
    z = x.to(dt)
    if keep is not None:
        z = torch.where(keep, z * dscale(p), torch.zeros_like(z))
    if res is not None:
        z = z + res.to(dt)
    mean = z.mean(-1, keepdim=True)
    ve = ((z - mean) ** 2).mean(-1, keepdim=True) + torch.tensor(float(np.float32(eps)), dtype=dt)        # eps arrives as a float
    rstd = torch.where(ve > 0, torch.rsqrt(ve), torch.zeros_like(ve))
    y = (z - mean) * rstd * gamma.to(dt) + beta.to(dt)
    return dict(y=y, zout=z, mean=mean[:, 0], rstd=rstd[:, 0])


def xhat_ref(dt, zb, mean, rstd, gamma, beta=None):
    """The normalised values the backward works with: from the stored sum (beta None) or from the output."""
    if beta is None:
        return (zb.to(dt) - mean.to(dt)[:, None]) * rstd.to(dt)[:, None]
    gm = gamma.to(dt)
    ig = torch.where(gm != 0, 1.0 / gm, torch.zeros_like(gm))
    return (zb.to(dt) - beta.to(dt)) * ig


def ln_bwd_ref(dt, dy, dy2, zb, mean, rstd, gamma, beta=None, keep=None, p=0.0):
    """-> dict dz, dx [rows, H], dgamma, dbeta [H] (the launch's own sums, without the buffers' previous contents) in dtype dt, unrounded.
    zb: the stored bf16 tensor -- the sum z, or with `beta` the output y (mean is not read then and may be None)."""
    g = dy.to(dt) + (dy2.to(dt) if dy2 is not None else 0)
    xh = xhat_ref(dt, zb, mean, rstd, gamma, beta)
    dg = g * gamma.to(dt)
    s1, s2 = dg.mean(-1, keepdim=True), (dg * xh).mean(-1, keepdim=True)
    dz = rstd.to(dt)[:, None] * (dg - s1 - xh * s2)
    dx = dz if keep is None else torch.where(keep, dz * dscale(p), torch.zeros_like(dz))
    return dict(dz=dz, dx=dx, dgamma=(g * xh).sum(0), dbeta=g.sum(0))


def bwd_grid(rows):
    """Workgroups of a spmm_ln_bwd launch (4 waves, one row each per pass): rows / 4, capped at rows / 64 within [256, 512]."""
    return min((rows + 3) // 4, max(256, min(512, rows // 64)))


def bwd_passes(rows):
    """Passes of the row loop the busiest wave of the launch makes."""
    return -(-rows // (4 * bwd_grid(rows)))


def colsum_ref(dt, written):
    """dxsum's own sum: the column sums of the bf16 tensor the launch wrote."""
    return written.to(dt).sum(0)


def as_stored(r):
    """A float64 evaluation rounded the way the kernels store it: y / zout / dz / dx as bf16, everything else as fp32."""
    return {k: (v.to(BF) if k in ("y", "zout", "dz", "dx") else v.to(F32)) for k, v in r.items()}


# ---------------------------------------------------------------------------------------------------------------------
# Ordinary inputs
# ---------------------------------------------------------------------------------------------------------------------
def ordinary_case(rows, H, seed):
    """Seeded inputs of one forward + backward pair, rounded to bf16 where the kernels read bf16.  gamma holds a 0, a -0.03 and a negative
    ordinary channel; g0 / b0 / s0 are what dgamma / dbeta / dxsum hold before the launch.  x carries a common offset of 0.5 and the residual one of
    0.25: the row means are then of the size of the values they are means of, and check_ref's floor of 4 fp32 ulp of the output is what an fp32
    sum of such values can hold (a row mean that happens to fall at 1e-3 would be held to 1e-9 by one row's luck in E32)."""
    g = gen(seed * 7919 + 13 * H + rows)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    gamma = 1 + 0.2 * rn(H)
    gamma[ZERO_CH], gamma[SMALL_CH], gamma[NEG_CH] = 0.0, -0.03, -1.25
    return dict(x=(rn(rows, H) + 0.5).to(BF), res=(rn(rows, H) + 0.25).to(BF), gamma=gamma, beta=0.2 * rn(H), dy=rn(rows, H).to(BF),
                dy2=rn(rows, H).to(BF), g0=rn(H), b0=rn(H), s0=rn(H))


# ---------------------------------------------------------------------------------------------------------------------
# Exact-sum inputs
# ---------------------------------------------------------------------------------------------------------------------
def coarse(*shape, g, lim=2.0):
    """Multiples of 1/8 in [-lim, lim]."""
    return (torch.randn(*shape, generator=g) * 8).round().clamp(-8 * lim, 8 * lim) / 8


def unit_rows(rows, H, g):
    """Rows with mean exactly 0 and variance exactly 1 in any summation order, for any even H: n2 = H // 16 pairs +-2, 4 n2 pairs +-0.5
    (together 5 n2 pairs whose squares sum to 5 n2 as well) and H / 2 - 5 n2 pairs +-1, in a random order per row."""
    n2 = H // 16
    half = torch.cat([torch.full((n2,), 2.0), torch.full((4 * n2,), 0.5), torch.full((H // 2 - 5 * n2,), 1.0)])
    pat = torch.cat([half, -half])
    assert pat.numel() == H and pat.sum() == 0 and (pat * pat).sum() == H
    return pat[torch.rand(rows, H, generator=g).argsort(dim=1)]


def balanced(cls, g):
    """[rows, H] multiples of 1/8 in [-2, 2] that cancel within each row and each class of columns (cls [rows, H], classes at least 1 apart):
    the columns of a class are paired at random, a pair holds +v and -v, an odd leftover holds 0."""
    rows, H = cls.shape
    order = (cls.double() + 0.5 * torch.rand(rows, H, generator=g).double()).argsort(dim=1)
    ks = cls.gather(1, order)
    idx = torch.arange(H).expand(rows, H)
    new = torch.ones(rows, H, dtype=torch.bool)
    new[:, 1:] = ks[:, 1:] != ks[:, :-1]
    pos = idx - torch.where(new, idx, torch.zeros_like(idx)).cummax(dim=1).values           # place within the class
    first = (pos % 2 == 0)
    first[:, :-1] &= ~new[:, 1:]                                                            # ... with a partner behind it
    first[:, -1] = False
    v = coarse(rows, H, g=g)
    out = torch.where(first, v, torch.zeros_like(v))
    out[:, 1:] -= out[:, :-1].clone() * (pos[:, 1:] % 2 == 1)
    return torch.zeros(rows, H).scatter_(1, order, out)


def exact_case(rows, H, seed, varied=False):
    """Inputs of a backward launch whose outputs are exact (see the head of this file).  xhat in {+-0.5, +-1, +-2} with row mean 0 and row
    variance 1; gamma from the same six values and one channel at 0; beta and the buffers' contents multiples of 1/8; p = 0.5 (1 / (1 - p)
    = 2); dy and dy2 balanced per row and per class of columns sharing (xhat, gamma).  Then mean_H(g gamma) = mean_H(g gamma xhat) = 0
    exactly, dz = rstd g gamma is a bf16 number (g has six bits, the rest are powers of two), and every partial sum of g xhat, g and dx is a
    multiple of 1/32 below 2^17: exact in fp32.
    mean = 0 and rstd = 1 in every row; `varied`: rstd in {0.5, 1, 2} and mean in multiples of 1/4 per row, z = xhat / rstd + mean (still
    exact in bf16), so that a launch that takes the statistics of another row is seen."""
    g = gen(seed * 104729 + 31 * H + rows)
    xh = unit_rows(rows, H, g)
    mags = torch.tensor(XHAT)
    gamma = mags[torch.randint(0, 3, (H,), generator=g)] * (torch.randint(0, 2, (H,), generator=g) * 2 - 1)
    gamma[ZERO_CH] = 0.0
    beta = coarse(H, g=g)
    if varied:
        rstd = mags[torch.randint(0, 3, (rows,), generator=g)]
        mean = (torch.randn(rows, generator=g) * 4).round().clamp(-4, 4) / 4
    else:
        rstd, mean = torch.ones(rows), torch.zeros(rows)
    z, y = xh / rstd[:, None] + mean[:, None], xh * gamma + beta
    cls = (xh * 32 + gamma * 2).long()                                                       # +-{16, 32, 64} + {0, +-1, +-2, +-4}
    c = dict(xhat=xh, z=z.to(BF), y=y.to(BF), mean=mean, rstd=rstd, gamma=gamma, beta=beta, dy=balanced(cls, g).to(BF),
             dy2=balanced(cls, g).to(BF), g0=coarse(H, g=g), b0=coarse(H, g=g), s0=coarse(H, g=g), p=0.5)
    assert torch.equal(c["z"].float(), z) and torch.equal(c["y"].float(), y)
    return c
