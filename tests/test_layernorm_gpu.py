"""The residual LayerNorm kernels of csrc/rowops.hip -- spmm_ln_fwd and spmm_ln_bwd without drop_on_dy, the pair every sublayer of every
step runs -- against the float64 restatement in tests/layernorm_reference.py, on every launch path and at the shapes where each can go
wrong.  Inputs come from a seeded CPU generator and are rounded to bf16 where the kernel reads bf16; every output buffer is pre-filled
with the sentinel 7.0 and carries one spare row (eight spare columns for the column sums) that must stay untouched; dropout uses a device
seed tensor and a salt per case.

Tolerances (tests/helpers_gpu.py::check_ref) come from the reference, never from the kernel: E32 is the largest error of the same formula
in fp32 torch on the CPU against float64; mean, rstd, dgamma, dbeta, dxsum may be max(8 * E32, 4 fp32 ulp of the output's magnitude) away,
the bf16 outputs y, zout, dz, dx one bf16 ulp of the reference (relative 2^-7) more.  Masks are compared exactly: dx == 0 where the host
model of the hash drops, zout == res bit for bit where it drops x.  Every comparison prints `[tol] name: E32 kernel bound` (pytest -s);
profiles/layernorm_tol.txt holds one run's lines.

The backward starts from what the forward kernel stored (bf16 z or y, fp32 mean and rstd), as the product does; in the from-output form
the reference reads the same stored y, so the 1 / |gamma| amplification of y's rounding is in the reference too.  dxsum is compared with
the column sums of the bf16 dx (dz when no dx is asked for) that the same launch wrote.  Ordinary values stop at 333 rows: beyond that the
order of the launch's fp32 atomics alone can pass the bound (see above LN_BWD in tests/test_row_kernels_gpu.py).  The row loop -- more
than 1024 rows -- runs on layernorm_reference.exact_case, where every output and every partial sum is exact, and is compared bit for bit;
tests/test_layernorm_reference_cpu.py shows that those inputs are exact in any order and that check_ref rejects a wrong row, mask, scale,
row mean or column sum.  The from-output form is exact there because __builtin_amdgcn_rcpf is exact on +-0.5, +-1, +-2 (measured: the
exact cases pass with gamma drawn from those values).

Which case reaches which kernel (the choices of spmm_ln_fwd / spmm_ln_bwd):
  ln_fwd_kernel                       test_ln_fwd_generic_kernel, test_ln_fwd_options[260], test_ln_fwd_values[260], test_ln_fwd_device_row_count[260],
                                      the forward of every backward case at H not in {256, 512, 768, 1024}
  ln_fwd16_kernel<1 / 2 / 3 / 4>      test_ln_fwd_half_wave_kernels[256 / 512 / 768 / 1024]; <3> also the [768] cases of the options, values, device row
                                      count and consistency tests and the forward of the backward cases at 768, <4> at 1024
  ln_bwd_kernel<3, false, false, F>   H <= 768 unless HOT: ordinary values at 4, 260, 764, 768 (a second gradient is passed), options[260], every
                                      options[768] combination but one, row loop [260] and [768] with dy2 or without dxsum
  ln_bwd_kernel<4, false, false, F>   H > 768: ordinary values at 772, 1000, 1024, options[1024], row loop [1024]
  ln_bwd_kernel<3, true, true, F>     H == 768 with dx, dgamma, dbeta, dxsum, dropout and no second gradient: that combination of options[768] (its sibling
                                      with dy2 = zeros is forced onto the general path), row loop [768] without dy2, consistency [768]
  F = false: stored-sum form; F = true: from-output form (beta_from_y), the ids `stored-sum` / `from-output` of every backward test.

Measured on an MI355X: per test case the comparison with the least margin (kernel error / bound); for a bf16 output the kernel column is
what remains past one bf16 ulp of the reference (at most 0.09 of the bound, on y of the offset-100 rows).  The backward cases run the
forward first and check it too (`fwd`).  The row-loop cases print nothing: all 24, with their 2049-row variants, were bit-equal.

| case | comparison | output | E32 | kernel | bound |
|---|---|---|---|---|---|
| ln_fwd[H4] | 4 rows | rstd | 2.8e-07 | 2.8e-07 | 2.3e-06 |
| ln_fwd[H128] | 3 rows | rstd | 2.2e-08 | 4.1e-08 | 2.4e-07 |
| ln_fwd[H252] | 1 rows | mean | 4.7e-09 | 6.4e-08 | 2.4e-07 |
| ln_fwd[H260] | 5 rows | mean | 3.6e-08 | 5.3e-08 | 2.9e-07 |
| ln_fwd[H764] | 1 rows | mean | 6.5e-09 | 5.3e-08 | 2.4e-07 |
| ln_fwd[H1000] | 3 rows | rstd | 3.5e-08 | 6.8e-08 | 2.8e-07 |
| ln_fwd[H1020] | 4 rows | rstd | 4.1e-08 | 4.1e-08 | 3.3e-07 |
| ln_fwd16[H256] | 1 rows | mean | 9.8e-09 | 6.9e-08 | 2.4e-07 |
| ln_fwd16[H512] | 8 rows | rstd | 4.8e-08 | 7.3e-08 | 3.8e-07 |
| ln_fwd16[H768] | 7 rows | mean | 7.0e-08 | 8.1e-08 | 5.6e-07 |
| ln_fwd16[H1024] | 8 rows | rstd | 3.0e-08 | 4.8e-08 | 2.4e-07 |
| ln_fwd_options[H260] | res=0 zout=none stats=1 p=0.1 | mean | 2.8e-08 | 5.7e-08 | 2.4e-07 |
| ln_fwd_options[H768] | res=1 zout=alias stats=1 p=0.5 | rstd | 2.9e-08 | 6.0e-08 | 2.4e-07 |
| ln_fwd_values[H260] | offset 100 | rstd | 6.8e-07 | 4.8e-07 | 5.4e-06 |
| ln_fwd_values[H768] | offset 100 | mean | 1.1e-05 | 1.4e-05 | 8.4e-05 |
| ln_fwd_rows_dev[H260] | count 8 | mean | 4.9e-08 | 5.6e-08 | 3.9e-07 |
| ln_fwd_rows_dev[H768] | count 8 | mean | 5.1e-08 | 8.3e-08 | 4.1e-07 |
| ln_bwd[H4 z] | 333 rows | dxsum | 9.5e-07 | 1.3e-06 | 7.6e-06 |
| ln_bwd[H4 y] | 333 rows | dgamma | 3.2e-06 | 4.4e-06 | 2.6e-05 |
| ln_bwd[H260 z] | 333 rows | dgamma | 1.0e-05 | 3.5e-05 | 8.0e-05 |
| ln_bwd[H260 y] | 1 rows | dgamma | 4.3e-07 | 1.1e-06 | 3.8e-06 |
| ln_bwd[H764 z] | 333 rows | dgamma | 1.1e-05 | 2.2e-05 | 9.1e-05 |
| ln_bwd[H764 y] | 333 rows | dgamma | 1.2e-05 | 2.5e-05 | 9.4e-05 |
| ln_bwd[H768 z] | 333 rows | dgamma | 1.3e-05 | 2.3e-05 | 1.0e-04 |
| ln_bwd[H768 y] | 333 rows | dgamma | 1.2e-05 | 3.1e-05 | 9.6e-05 |
| ln_bwd[H772 z] | 333 rows | dgamma | 1.2e-05 | 3.4e-05 | 9.9e-05 |
| ln_bwd[H772 y] | 333 rows | dgamma | 1.2e-05 | 2.1e-05 | 9.4e-05 |
| ln_bwd[H1000 z] | 333 rows | dgamma | 1.2e-05 | 2.4e-05 | 9.8e-05 |
| ln_bwd[H1000 y] | 333 rows | dgamma | 1.2e-05 | 2.4e-05 | 9.6e-05 |
| ln_bwd[H1024 z] | 333 rows | dgamma | 1.3e-05 | 2.6e-05 | 1.1e-04 |
| ln_bwd[H1024 y] | 333 rows | dgamma | 1.5e-05 | 2.3e-05 | 1.2e-04 |
| ln_bwd_options[H260 z] | dy2=0 dx=1 dgb=1 dxsum=1 p=0.0 | dgamma | 2.0e-06 | 2.8e-06 | 1.6e-05 |
| ln_bwd_options[H260 y] | dy2=0 dx=0 dgb=1 dxsum=0 p=0.1 | dgamma | 2.1e-06 | 3.2e-06 | 1.7e-05 |
| ln_bwd_options[H768 z] | dy2=1 dx=0 dgb=1 dxsum=0 p=0.1 | dbeta | 9.5e-07 | 1.4e-06 | 7.6e-06 |
| ln_bwd_options[H768 y] | dy2=1 dx=0 dgb=1 dxsum=0 p=0.0 | dbeta | 9.5e-07 | 1.4e-06 | 7.6e-06 |
| ln_bwd_options[H1024 z] | dy2=0 dx=0 dgb=0 dxsum=1 p=0.1 | dxsum | 4.8e-07 | 6.6e-07 | 3.8e-06 |
| ln_bwd_options[H1024 y] | dy2=0 dx=1 dgb=1 dxsum=1 p=0.0 | dxsum | 4.8e-07 | 8.3e-07 | 3.8e-06 |
| ln_consistency[H260 seed 20261021] | fwd | rstd | 1.0e-07 | 9.4e-08 | 8.4e-07 |
| ln_consistency[H260 seed 20261021 z] |  | dbeta | 4.8e-07 | 6.6e-07 | 3.8e-06 |
| ln_consistency[H260 seed 20261021 y] |  | dbeta | 4.8e-07 | 6.3e-07 | 3.8e-06 |
| ln_consistency[H768 seed 20261021] | fwd | mean | 6.8e-08 | 8.2e-08 | 5.4e-07 |
| ln_consistency[H768 seed 20261021 z] |  | dxsum | 9.4e-07 | 1.2e-06 | 7.6e-06 |
| ln_consistency[H768 seed 20261021 y] |  | dxsum | 9.4e-07 | 1.1e-06 | 7.6e-06 |
| ln_consistency[H768 seed 1099511640121] | fwd | mean | 7.6e-08 | 7.9e-08 | 6.1e-07 |
| ln_consistency[H768 seed 1099511640121 z] |  | dgamma | 2.3e-06 | 3.1e-06 | 1.9e-05 |
| ln_consistency[H768 seed 1099511640121 y] |  | dxsum | 6.0e-07 | 1.2e-06 | 7.6e-06 |
| ln_consistency[H1024 seed 1099511640121] | fwd | mean | 6.0e-08 | 6.0e-08 | 4.8e-07 |
| ln_consistency[H1024 seed 1099511640121 z] |  | dxsum | 1.2e-06 | 2.6e-06 | 1.5e-05 |
| ln_consistency[H1024 seed 1099511640121 y] |  | dgamma | 3.0e-06 | 4.1e-06 | 2.4e-05 |

The least margin of the run is dgamma of ln_bwd[H260 z] at 333 rows, 0.44 of its bound.  Before ln_fwd16_kernel stopped clamping a
device-side count of 0 to 1, test_ln_fwd_device_row_count[768] failed at count 0 with `y: a row from row 0 on was written` (row 0 of
the NaN input, normalised); everything else here passed then as well.
"""
import itertools

import pytest
import torch

import layernorm_reference as R
from helpers_gpu import check_ref

pytestmark = pytest.mark.gpu

BF, F32, F64 = R.BF, R.F32, R.F64
SENT = 7.0
EPS = R.EPS
SEED_V = 20261021
SEED_HI = 2 ** 40 + 12345          # a seed whose high word is not zero
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops as o
    return o


def dev(t):
    return None if t is None else t.to(DEV)


def full(shape, dtype=F32, v=SENT):
    return torch.full(shape, v, dtype=dtype, device=DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def is_sent(t):
    return bool((t == SENT).all())


def dev_seed(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def dev_count(n):
    return torch.tensor([n], dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# Launch and compare
# ---------------------------------------------------------------------------------------------------------------------
def launch_fwd(ops, x, res, gamma, beta, *, zmode="given", stats=True, p=0.0, eps=EPS, seed_v=SEED_V, salt=0, count=None):
    """One spmm_ln_fwd launch on CPU inputs.  zmode: `given` / `none` / `alias` (zout is x's own buffer).  count: device-side row count.
    -> dict of the outputs asked for, the rows below the count, on the CPU; asserts that every row from the count on is still the sentinel."""
    rows, H = x.shape
    n = rows if count is None else min(count, rows)
    xd = full((rows + 1, H), BF)
    xd[:rows] = dev(x)
    y = full((rows + 1, H), BF)
    z = full((rows + 1, H), BF) if zmode == "given" else xd if zmode == "alias" else None
    mean, rstd = (full((rows + 1,)), full((rows + 1,))) if stats else (None, None)
    cut = lambda t: None if t is None else t[:rows]
    ops.ln_fwd(xd[:rows], dev(res), dev(gamma), dev(beta), y[:rows], zout=cut(z), mean=cut(mean), rstd=cut(rstd), eps=eps, dropout_p=p,
               seed=dev_seed(seed_v) if p > 0 else None, salt=salt, rows_dev=None if count is None else dev_count(count))
    got = {}
    for k, t in (("y", y), ("zout", z), ("mean", mean), ("rstd", rstd)):
        if t is not None:
            t = t.cpu()
            assert is_sent(t[n:]), f"{k}: a row from row {n} on was written"
            got[k] = t[:n]
    return got


def check_fwd(name, got, x, res, gamma, beta, *, p=0.0, eps=EPS, seed_v=SEED_V, salt=0):
    n, H = got["y"].shape
    if n == 0:
        return
    xs, rs = x[:n], None if res is None else res[:n]
    keep = R.host_keep(seed_v, salt, n, H, p)
    r64, r32 = (R.ln_fwd_ref(dt, xs, rs, gamma, beta, keep, p, eps) for dt in (F64, F32))
    for k in got:
        check_ref(f"{name} {k}", got[k], r64[k], r32[k], bf16=k in ("y", "zout"))
    if keep is not None and "zout" in got:
        want = torch.zeros(n, H, dtype=BF) if rs is None else rs
        assert same_bits(got["zout"][~keep], want[~keep]), f"{name}: zout differs from res where the host model drops x"


def launch_bwd(ops, c, zin, mean, rstd, *, from_y, dy2=True, dx=True, stats=True, xs=True, p=0.0, seed_v=SEED_V, salt=0, count=None):
    """One spmm_ln_bwd launch (drop_on_dy off) on the CPU inputs of case c.  zin: the stored sum, or with from_y the stored output (the row
    means are not passed then).  dy2: True / False / `zeros`.  -> dict of the outputs asked for on the CPU, the rows below the count."""
    rows, H = c["dy"].shape
    n = rows if count is None else min(count, rows)
    dz = full((rows + 1, H), BF)
    dxb = full((rows + 1, H), BF) if dx else None
    tail = lambda v: torch.cat([v, torch.full((8,), SENT)]).to(DEV)
    dg, db = (tail(c["g0"]), tail(c["b0"])) if stats else (None, None)
    sx = tail(c["s0"]) if xs else None
    d2 = dev(c["dy2"]) if dy2 is True else torch.zeros(rows, H, dtype=BF, device=DEV) if dy2 == "zeros" else None
    col = lambda t: None if t is None else t[:H]
    ops.ln_bwd(dev(c["dy"]), dev(zin), None if from_y else dev(mean), dev(rstd), dev(c["gamma"]), dz[:rows], dy2=d2,
               dx=None if dxb is None else dxb[:rows], dgamma=col(dg), dbeta=col(db), dropout_p=p, seed=dev_seed(seed_v) if p > 0 else None,
               salt=salt, dxsum=col(sx), rows_dev=None if count is None else dev_count(count), beta_from_y=dev(c["beta"]) if from_y else None)
    got = {}
    for k, t in (("dz", dz), ("dx", dxb)):
        if t is not None:
            t = t.cpu()
            assert is_sent(t[n:]), f"{k}: a row from row {n} on was written"
            got[k] = t[:n]
    for k, t in (("dgamma", dg), ("dbeta", db), ("dxsum", sx)):
        if t is not None:
            t = t.cpu()
            assert is_sent(t[H:]), f"{k}: a column past H was written"
            got[k] = t[:H]
    return got


def check_bwd(name, got, c, zin, mean, rstd, *, from_y, dy2=True, p=0.0, seed_v=SEED_V, salt=0, exact=False):
    n, H = got["dz"].shape
    keep = R.host_keep(seed_v, salt, n, H, p)
    d2 = c["dy2"][:n] if dy2 is True else None                                       # (a second gradient of zeros adds nothing)
    r64, r32 = (R.ln_bwd_ref(dt, c["dy"][:n], d2, zin[:n], None if from_y else mean[:n], rstd[:n], c["gamma"], c["beta"] if from_y else None,
                             keep, p) for dt in (F64, F32))
    written = got.get("dx", got["dz"])
    r64["dxsum"], r32["dxsum"] = R.colsum_ref(F64, written), R.colsum_ref(F32, written)
    for k, init in (("dgamma", "g0"), ("dbeta", "b0"), ("dxsum", "s0")):             # the sums land on the buffers' contents
        r64[k], r32[k] = c[init].double() + r64[k], c[init] + r32[k]
    for k in got:
        if exact:
            bad = got[k].double() != r64[k]
            assert not bad.any(), f"{name} {k}: {int(bad.sum())} of {bad.numel()} differ from float64, first at {bad.nonzero()[0].tolist()}"
        else:
            check_ref(f"{name} {k}", got[k], r64[k], r32[k], bf16=k in ("dz", "dx"))
    if keep is not None and "dx" in got:
        assert not got["dx"][~keep].any(), f"{name}: dx is not zero where the host model drops"


def fwd_then_bwd(ops, name, c, *, from_y, p, salt, seed_v=SEED_V, exact=False, **opts):
    """The forward kernel with every output, checked, then the backward from what it stored, with the same seed and salt."""
    f = launch_fwd(ops, c["x"], c["res"], c["gamma"], c["beta"], p=p, seed_v=seed_v, salt=salt)
    check_fwd(f"{name} fwd", f, c["x"], c["res"], c["gamma"], c["beta"], p=p, seed_v=seed_v, salt=salt)
    zin = f["y"] if from_y else f["zout"]
    got = launch_bwd(ops, c, zin, f["mean"], f["rstd"], from_y=from_y, p=p, seed_v=seed_v, salt=salt, **opts)
    check_bwd(name, got, c, zin, f["mean"], f["rstd"], from_y=from_y, dy2=opts.get("dy2", True), p=p, seed_v=seed_v, salt=salt, exact=exact)
    return f, got


FORMS = pytest.mark.parametrize("from_y", [False, True], ids=["stored-sum", "from-output"])


# ---------------------------------------------------------------------------------------------------------------------
# Forward
# ---------------------------------------------------------------------------------------------------------------------
# 4: one live lane; 252 / 764 / 1020: the last lane of a chunk has nothing; 260: one lane into the second chunk; 128, 1000: in between
@pytest.mark.parametrize("H", [4, 128, 252, 260, 764, 1000, 1020])
def test_ln_fwd_generic_kernel(ops, H):
    """ln_fwd_kernel, four rows per workgroup: one row, a workgroup one short, full, and one row into a second workgroup."""
    for rows in (1, 3, 4, 5):
        c, salt = R.ordinary_case(rows, H, seed=20), 1000 * rows + H
        got = launch_fwd(ops, c["x"], c["res"], c["gamma"], c["beta"], p=0.1, salt=salt)
        check_fwd(f"ln_fwd[H{H}] {rows} rows", got, c["x"], c["res"], c["gamma"], c["beta"], p=0.1, salt=salt)


@pytest.mark.parametrize("H", [256, 512, 768, 1024])
def test_ln_fwd_half_wave_kernels(ops, H):
    """ln_fwd16_kernel<H / 256>, eight rows per workgroup and two per wave: an odd count leaves a dead half-wave that borrows row rows - 1
    for the reductions and must write nothing."""
    for rows in (1, 7, 8, 9):
        c, salt = R.ordinary_case(rows, H, seed=21), 1000 * rows + H
        got = launch_fwd(ops, c["x"], c["res"], c["gamma"], c["beta"], p=0.1, salt=salt)
        check_fwd(f"ln_fwd16[H{H}] {rows} rows", got, c["x"], c["res"], c["gamma"], c["beta"], p=0.1, salt=salt)


@pytest.mark.parametrize("H,rows", [(260, 5), (768, 9)])
def test_ln_fwd_options(ops, H, rows):
    """With and without a residual, the stored sum (also written over x itself, which the header allows) and the statistics, at three
    dropout rates.  Outputs that are not asked for are null pointers to the launch."""
    c = R.ordinary_case(rows, H, seed=22)
    for i, (with_res, zmode, stats, p) in enumerate(itertools.product((True, False), ("given", "none", "alias"), (True, False), (0.0, 0.1, 0.5))):
        res, salt = c["res"] if with_res else None, 40 * H + i
        got = launch_fwd(ops, c["x"], res, c["gamma"], c["beta"], zmode=zmode, stats=stats, p=p, salt=salt)
        assert set(got) == {"y"} | ({"zout"} if zmode != "none" else set()) | ({"mean", "rstd"} if stats else set())
        check_fwd(f"ln_fwd_options[H{H}] res={int(with_res)} zout={zmode} stats={int(stats)} p={p}", got, c["x"], res, c["gamma"], c["beta"],
                  p=p, salt=salt)


@pytest.mark.parametrize("H,rows", [(260, 5), (768, 9)])
def test_ln_fwd_values(ops, H, rows):
    """Rows with a large common offset (mean near 100, spread 0.1: the variance must come from the centred values); constant rows, where
    y == beta and rstd == rsqrt(eps) at eps = 1e-12; and eps = 0, where the guard gives rstd == 0 and y == beta exactly (torch: NaN)."""
    c = R.ordinary_case(rows, H, seed=23)
    x = (0.1 * (c["x"].float() - 0.5)).to(BF)
    res = torch.full((rows, H), 100.0, dtype=BF)
    got = launch_fwd(ops, x, res, c["gamma"], c["beta"])
    assert (got["mean"] - 100).abs().max() < 0.05 and (got["rstd"] - 10).abs().max() < 2
    check_fwd(f"ln_fwd_values[H{H}] offset 100", got, x, res, c["gamma"], c["beta"])
    consts = torch.tensor([1.0, -2.0, 0.5, 4.0, -0.25, 2.0, -1.0, 0.25, -4.0])[:rows]          # H * c is exact in fp32 in any order
    xc = consts[:, None].expand(rows, H).to(BF).contiguous()
    got = launch_fwd(ops, xc, None, c["gamma"], c["beta"], eps=1e-12)
    check_fwd(f"ln_fwd_values[H{H}] constant rows", got, xc, None, c["gamma"], c["beta"], eps=1e-12)
    assert torch.equal(got["mean"], consts)
    got = launch_fwd(ops, xc, None, c["gamma"], c["beta"], eps=0.0)
    assert not got["rstd"].any(), got["rstd"]
    assert same_bits(got["y"], c["beta"].to(BF).expand(rows, H)) and torch.equal(got["mean"], consts) and same_bits(got["zout"], xc)


@pytest.mark.parametrize("H", [260, 768])
def test_ln_fwd_device_row_count(ops, H):
    """A launch sized for 9 rows with the count read from device memory: rows from the count on hold NaN in x and res and are neither
    read nor written (include/spmm_hip.h) -- at a count of 0 nothing at all is written."""
    rows = 9
    c = R.ordinary_case(rows, H, seed=24)
    for count in (0, 1, 8, 9):
        x, res, salt = c["x"].clone(), c["res"].clone(), 50 * H + count
        x[count:], res[count:] = float("nan"), float("nan")
        got = launch_fwd(ops, x, res, c["gamma"], c["beta"], p=0.1, salt=salt, count=count)
        assert got["y"].shape[0] == count
        check_fwd(f"ln_fwd_rows_dev[H{H}] count {count}", got, x, res, c["gamma"], c["beta"], p=0.1, salt=salt)


# ---------------------------------------------------------------------------------------------------------------------
# Backward
# ---------------------------------------------------------------------------------------------------------------------
# 4: one live lane; 260: the second chunk; 764 / 768: the last guarded lane and none; 772: the first H on NC = 4; 1000, 1024
@FORMS
@pytest.mark.parametrize("H", [4, 260, 764, 768, 772, 1000, 1024])
def test_ln_bwd_ordinary_values(ops, H, from_y):
    """Every output, two incoming gradients, p = 0.1, behind the forward that drew the mask: one row, a workgroup full, one row into the
    second, and 333 rows (84 workgroups' atomics per column)."""
    for rows in (1, 4, 5, 333):
        c = R.ordinary_case(rows, H, seed=30)
        fwd_then_bwd(ops, f"ln_bwd[H{H} {'y' if from_y else 'z'}] {rows} rows", c, from_y=from_y, p=0.1, salt=2000 * rows + H)


@FORMS
@pytest.mark.parametrize("H", [260, 768, 1024])
def test_ln_bwd_options(ops, H, from_y):
    """Every combination of a second gradient, dx, dgamma + dbeta, dxsum (of dx, or of dz when there is no dx) and dropout, at 37 rows.
    At 768, (no dy2, dx, dgamma + dbeta, dxsum, p = 0.1) is the HOT instantiation; the same with dy2 = zeros runs the general one."""
    rows = 37
    c = R.ordinary_case(rows, H, seed=31)
    fwd = {}
    combos = list(itertools.product((False, True), (False, True), (False, True), (False, True), (0.0, 0.1)))
    if H == 768:
        combos.append(("zeros", True, True, True, 0.1))
    for dy2, dx, stats, xs, p in combos:
        salt = 60 * H + int(p * 10)
        if p not in fwd:
            fwd[p] = launch_fwd(ops, c["x"], c["res"], c["gamma"], c["beta"], p=p, salt=salt)
        f = fwd[p]
        zin = f["y"] if from_y else f["zout"]
        got = launch_bwd(ops, c, zin, f["mean"], f["rstd"], from_y=from_y, dy2=dy2, dx=dx, stats=stats, xs=xs, p=p, salt=salt)
        assert set(got) == {"dz"} | ({"dx"} if dx else set()) | ({"dgamma", "dbeta"} if stats else set()) | ({"dxsum"} if xs else set())
        tag = f"dy2={dy2 if dy2 == 'zeros' else int(dy2)} dx={int(dx)} dgb={int(stats)} dxsum={int(xs)} p={p}"
        check_bwd(f"ln_bwd_options[H{H} {'y' if from_y else 'z'}] {tag}", got, c, zin, f["mean"], f["rstd"], from_y=from_y, dy2=dy2, p=p, salt=salt)


@FORMS
@pytest.mark.parametrize("H", [260, 768, 1024])
@pytest.mark.parametrize("rows", [1023, 1024, 1025, 2049])
def test_ln_bwd_row_loop_bit_for_bit(ops, rows, H, from_y):
    """The row loop and its prefetch of the next row on exact-sum inputs (p = 0.5): 1023 and 1024 rows are the last counts with one pass per
    wave, 1025 the first with a second (one wave), 2049 three passes for one wave and two for the rest.  dz, dx, dgamma, dbeta, dxsum
    equal float64 bit for bit.  At 768 the launch without dy2 is the HOT instantiation; with dy2, or without dxsum, the general one.
    At 2049 rows also with per-row statistics that differ (a prefetch of another row's mean or rstd is seen), and sized for 2049 rows
    with a device-side count of 1025 and NaN from row 1025 on."""
    assert R.bwd_passes(rows) == {1023: 1, 1024: 1, 1025: 2, 2049: 3}[rows]
    fy = "y" if from_y else "z"
    variants = [(False, True), (True, True)] + ([(False, False)] if H == 768 else [])            # (dy2, dxsum)
    cases = [("", R.exact_case(rows, H, seed=40))] + ([(" varied", R.exact_case(rows, H, seed=41, varied=True))] if rows == 2049 else [])
    for tag, c in cases:
        zin = c["y"] if from_y else c["z"]
        for i, (dy2, xs) in enumerate(variants):
            salt = 3 * rows + H + i
            got = launch_bwd(ops, c, zin, c["mean"], c["rstd"], from_y=from_y, dy2=dy2, xs=xs, p=c["p"], salt=salt)
            check_bwd(f"ln_bwd_exact[{rows}x{H} {fy}{tag}] dy2={int(dy2)} dxsum={int(xs)}", got, c, zin, c["mean"], c["rstd"], from_y=from_y,
                      dy2=dy2, p=c["p"], salt=salt, exact=True)
    if rows == 2049:
        count, c = 1025, dict(cases[0][1])
        for k in ("dy", "dy2", "z", "y"):
            c[k] = c[k].clone()
            c[k][count:] = float("nan")
        zin = c["y"] if from_y else c["z"]
        for i, (dy2, xs) in enumerate(variants):
            salt = 5 * rows + H + i
            got = launch_bwd(ops, c, zin, c["mean"], c["rstd"], from_y=from_y, dy2=dy2, xs=xs, p=c["p"], salt=salt, count=count)
            assert got["dz"].shape[0] == count
            check_bwd(f"ln_bwd_exact[{rows}x{H} {fy} count {count}] dy2={int(dy2)} dxsum={int(xs)}", got, c, zin, c["mean"], c["rstd"],
                      from_y=from_y, dy2=dy2, p=c["p"], salt=salt, exact=True)


@FORMS
@pytest.mark.parametrize("H,seed_v", [(260, SEED_V), (768, SEED_V), (768, SEED_HI), (1024, SEED_HI)])
def test_ln_fwd_and_bwd_drop_the_same_elements(ops, H, seed_v, from_y):
    """Same seed, salt and rows: the elements the forward dropped (read off its stored sum: no residual, no zero in x) are the host
    model's, and dx is zero exactly there.  No second gradient: the HOT instantiation at 768."""
    rows, p, salt = 37, 0.1, 7000 + H
    c = R.ordinary_case(rows, H, seed=32)
    x = torch.where(c["x"] == 0, torch.ones_like(c["x"]), c["x"])
    f = launch_fwd(ops, x, None, c["gamma"], c["beta"], p=p, seed_v=seed_v, salt=salt)
    check_fwd(f"ln_consistency[H{H} seed {seed_v}] fwd", f, x, None, c["gamma"], c["beta"], p=p, seed_v=seed_v, salt=salt)
    kept = f["zout"] != 0
    assert torch.equal(kept, R.host_keep(seed_v, salt, rows, H, p))
    if seed_v >> 32:
        assert not torch.equal(kept, R.host_keep(seed_v & 0xffffffff, salt, rows, H, p))         # the seed's high word reaches the mask
    zin = f["y"] if from_y else f["zout"]
    got = launch_bwd(ops, c, zin, f["mean"], f["rstd"], from_y=from_y, dy2=False, p=p, seed_v=seed_v, salt=salt)
    check_bwd(f"ln_consistency[H{H} seed {seed_v} {'y' if from_y else 'z'}]", got, c, zin, f["mean"], f["rstd"], from_y=from_y, dy2=False,
              p=p, seed_v=seed_v, salt=salt)
    assert not got["dx"][~kept].any() and (got["dx"][kept] != 0).float().mean() > 0.99
