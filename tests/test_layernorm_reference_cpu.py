"""tests/layernorm_reference.py checked on the CPU: the float64 formulas are those of torch's layer_norm under autograd, the from-output
form is the stored-sum form where the output determines the normalised values, the exact-sum inputs really are exact in any order of the
launch's fp32 additions, and helpers_gpu.check_ref -- the rule tests/test_layernorm_gpu.py holds the kernels to -- rejects a float64
evaluation with any one of six planted defects, rounded the way the kernels store their outputs."""
import pytest
import torch
import torch.nn.functional as F

import layernorm_reference as R
from helpers_gpu import check_ref

BF, F32, F64 = R.BF, R.F32, R.F64
SEED_V = 20261021
EXACT_SHAPES = [(rows, H) for rows in (1023, 1024, 1025, 2049) for H in (260, 768, 1024)]


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def stored_pair(rows, H, seed, salt, p):
    """Ordinary inputs, the host mask, and the forward's outputs as the kernel would store them (float64 formulas, rounded)."""
    c = R.ordinary_case(rows, H, seed)
    keep = R.host_keep(SEED_V, salt, rows, H, p)
    return c, keep, R.as_stored(R.ln_fwd_ref(F64, c["x"], c["res"], c["gamma"], c["beta"], keep, p))


def bwd_of(dt, c, f, keep, p, from_y, **over):
    a = dict(dy=c["dy"], dy2=c["dy2"], zb=f["y"] if from_y else f["zout"], mean=f["mean"], rstd=f["rstd"], keep=keep)
    a.update(over)
    return R.ln_bwd_ref(dt, a["dy"], a["dy2"], a["zb"], a["mean"], a["rstd"], c["gamma"], c["beta"] if from_y else None, a["keep"], p)


# ---------------------------------------------------------------------------------------------------------------------
# The formulas against autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,H,p", [(5, 260, 0.1), (9, 768, 0.5), (4, 1000, 0.0), (1, 4, 0.0)])
def test_float64_formulas_agree_with_layer_norm_autograd(rows, H, p):
    """Forward and stored-sum backward against float64 autograd of sum(g * layer_norm(x * keep / (1 - p) + res)), through the UNROUNDED sum
    and with the mask as a constant multiplier: 1e-12 relative."""
    c = R.ordinary_case(rows, H, seed=1)
    keep = R.host_keep(SEED_V, 3, rows, H, p)
    eps = 1e-5
    eps32 = float(torch.tensor(eps, dtype=F32))
    mult = torch.ones(rows, H, dtype=F64) if keep is None else keep.double() * R.dscale(p)
    x = c["x"].double().requires_grad_(True)
    gm, bt = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    z = x * mult + c["res"].double()
    z.retain_grad()
    y = F.layer_norm(z, (H,), gm, bt, eps32)
    g = c["dy"].double() + c["dy2"].double()
    (y * g).sum().backward()
    f = R.ln_fwd_ref(F64, c["x"], c["res"], c["gamma"], c["beta"], keep, p, eps)
    assert rel(f["y"], y.detach()) < 1e-12 and rel(f["zout"], z.detach()) < 1e-12
    assert rel(f["mean"], z.detach().mean(-1)) < 1e-12
    assert rel(f["rstd"], torch.rsqrt(z.detach().var(-1, unbiased=False) + eps32)) < 1e-12
    b = R.ln_bwd_ref(F64, c["dy"], c["dy2"], f["zout"], f["mean"], f["rstd"], c["gamma"], None, keep, p)
    for k, want in (("dz", z.grad), ("dx", x.grad), ("dgamma", gm.grad), ("dbeta", bt.grad)):
        assert rel(b[k], want) < 1e-12, (k, rel(b[k], want))


def test_constant_rows_and_the_rstd_guard():
    """A constant row: y == beta and rstd == rsqrt(eps) at eps = 1e-12; at eps = 0 the guard gives rstd == 0 and y == beta where torch's
    layer_norm gives NaN."""
    H = 260
    c = R.ordinary_case(3, H, seed=2)
    x = torch.tensor([1.0, -2.0, 0.5])[:, None].expand(3, H).to(BF)
    for dt in (F64, F32):
        f = R.ln_fwd_ref(dt, x, None, c["gamma"], c["beta"], None, 0.0, 1e-12)
        assert torch.equal(f["y"], c["beta"].to(dt).expand(3, H))
        assert torch.equal(f["rstd"], torch.rsqrt(torch.tensor(1e-12, dtype=F32).to(dt)).expand(3))
        f0 = R.ln_fwd_ref(dt, x, None, c["gamma"], c["beta"], None, 0.0, 0.0)
        assert torch.equal(f0["y"], c["beta"].to(dt).expand(3, H)) and not f0["rstd"].any() and torch.equal(f0["mean"], x[:, 0].to(dt))
    assert torch.isnan(F.layer_norm(x.float(), (H,), c["gamma"], c["beta"], 0.0)).all()


def test_from_output_form_equals_stored_sum_form():
    """In float64, from the unrounded output and with no gamma at 0, (y - beta) / gamma is the normalised value again; a channel with
    gamma == 0 reports dgamma == 0 and takes no part in the row means."""
    rows, H, p = 7, 260, 0.1
    c = R.ordinary_case(rows, H, seed=3)
    keep = R.host_keep(SEED_V, 4, rows, H, p)
    c0 = dict(c, gamma=c["gamma"].clone())
    c0["gamma"][R.ZERO_CH] = 0.7
    for case, with_zero in ((c0, False), (c, True)):
        f = R.ln_fwd_ref(F64, case["x"], case["res"], case["gamma"], case["beta"], keep, p)
        a = R.ln_bwd_ref(F64, case["dy"], case["dy2"], f["zout"], f["mean"], f["rstd"], case["gamma"], None, keep, p)
        b = R.ln_bwd_ref(F64, case["dy"], case["dy2"], f["y"], None, f["rstd"], case["gamma"], case["beta"], keep, p)
        if not with_zero:
            for k in a:
                assert rel(b[k], a[k]) < 1e-10, (k, rel(b[k], a[k]))                 # (1 / 0.03 times the rounding of y - beta)
        else:
            assert b["dgamma"][R.ZERO_CH] == 0 and a["dgamma"][R.ZERO_CH] != 0
            live = torch.arange(H) != R.ZERO_CH
            assert rel(b["dgamma"][live], a["dgamma"][live]) < 1e-10 and rel(b["dbeta"], a["dbeta"]) < 1e-10
            assert rel(b["dz"][:, live], a["dz"][:, live]) < 1e-10                  # g * gamma == 0 there: the channel is outside both means
            assert torch.equal(b["dz"][:, R.ZERO_CH], -f["rstd"] * (c["dy"].double() + c["dy2"].double()).mul(c["gamma"].double()).mean(-1))


def test_ordinary_case_holds_the_three_gamma_channels():
    c = R.ordinary_case(4, 4, seed=4)
    assert c["gamma"][R.ZERO_CH] == 0 and abs(c["gamma"][R.SMALL_CH] + 0.03) < 1e-6 and c["gamma"][R.NEG_CH] == -1.25
    assert c["x"].dtype == BF and c["dy2"].dtype == BF and c["gamma"].dtype == F32


def test_launch_geometry():
    """One pass up to 1024 rows, two from 1025, three for the first wave at 2049 (256 workgroups of 4 waves below 16448 rows)."""
    assert [R.bwd_passes(r) for r in (1, 333, 1023, 1024, 1025, 2048, 2049, 16384)] == [1, 1, 1, 1, 2, 2, 3, 16]
    assert [R.bwd_grid(r) for r in (1, 5, 1023, 1025, 2049, 20000, 85000)] == [1, 2, 256, 256, 256, 312, 512]


# ---------------------------------------------------------------------------------------------------------------------
# Exact-sum inputs
# ---------------------------------------------------------------------------------------------------------------------
def launch_sum32(T, init, g):
    """The fp32 sum of the rows of T [rows, H] onto init as an ln_bwd launch forms it: a wave adds its rows in turn, the four waves of a
    workgroup are added, the workgroups' partial sums reach memory one by one -- here in a random order."""
    rows, H = T.shape
    grid, passes = R.bwd_grid(rows), R.bwd_passes(rows)
    P = torch.zeros(passes * grid * 4, H)
    P[:rows] = T
    P = P.view(passes, grid, 4, H)
    w = P[0].clone()
    for k in range(1, passes):
        w += P[k]
    blk = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    out = init.clone()
    for b in torch.randperm(grid, generator=g).tolist():
        out += blk[b]
    return out


@pytest.mark.parametrize("varied", [False, True])
@pytest.mark.parametrize("rows,H", EXACT_SHAPES)
def test_exact_case_is_exact_in_any_order(rows, H, varied):
    c = R.exact_case(rows, H, seed=5, varied=varied)
    keep = R.host_keep(SEED_V, 6, rows, H, c["p"])
    # ---- the inputs are what the builder promises
    xh = c["xhat"]
    assert xh.sum(1).abs().max() == 0 and torch.equal((xh * xh).sum(1), torch.full((rows,), float(H)))
    assert set(xh.abs().unique().tolist()) == set(R.XHAT) and set(c["gamma"].abs().unique().tolist()) == {0.0, *R.XHAT}
    assert c["gamma"][R.ZERO_CH] == 0 and int((c["gamma"] == 0).sum()) == 1 and R.dscale(c["p"]) == 2.0
    for k in ("beta", "g0", "b0", "s0", "dy", "dy2"):
        assert torch.equal(c[k].float() * 8, (c[k].float() * 8).round()), k
    assert c["dy"].abs().max() > 0 and (c["dy"] != 0).float().mean() > 0.5
    if not varied:
        assert not c["mean"].any() and torch.equal(c["rstd"], torch.ones(rows)) and torch.equal(c["z"].float(), xh)
    for from_y in (False, True):
        r64 = R.ln_bwd_ref(F64, c["dy"], c["dy2"], c["y"] if from_y else c["z"], c["mean"], c["rstd"], c["gamma"],
                           c["beta"] if from_y else None, keep, c["p"])
        r32 = R.ln_bwd_ref(F32, c["dy"], c["dy2"], c["y"] if from_y else c["z"], c["mean"], c["rstd"], c["gamma"],
                           c["beta"] if from_y else None, keep, c["p"])
        g64 = c["dy"].double() + c["dy2"].double()
        assert torch.equal(r64["dz"], c["rstd"].double()[:, None] * g64 * c["gamma"].double())          # both row means vanish
        for k in r64:                                                                                   # exact in fp32, and dz / dx in bf16
            assert torch.equal(r32[k].double(), r64[k]), k
        assert torch.equal(r64["dz"].to(BF).double(), r64["dz"]) and torch.equal(r64["dx"].to(BF).double(), r64["dx"])
        # ---- every order of the launch's additions gives the float64 sums bit for bit
        xh64 = R.xhat_ref(F64, c["y"] if from_y else c["z"], c["mean"], c["rstd"], c["gamma"], c["beta"] if from_y else None)
        terms = dict(dgamma=(g64 * xh64, c["g0"]), dbeta=(g64, c["b0"]), dxsum=(r64["dx"], c["s0"]))
        g = R.gen(rows + H)
        for _ in range(10 if from_y else 20):
            perm = torch.randperm(rows, generator=g)
            for k, (T, init) in terms.items():
                got = launch_sum32(T.float()[perm], init, g)
                assert torch.equal(got.double(), init.double() + T.sum(0)), (k, from_y)


# ---------------------------------------------------------------------------------------------------------------------
# check_ref rejects planted defects
# ---------------------------------------------------------------------------------------------------------------------
def expect_rejected(name, wrong, r64, r32, keys):
    """check_ref passes the right evaluation as the kernel would store it, and refuses the wrong one on at least one of `keys`."""
    right = R.as_stored(r64)
    for k in r64:
        check_ref(f"{name} right {k}", right[k], r64[k], r32[k], bf16=k in ("dz", "dx"))
    w = R.as_stored(wrong)
    for k in keys:
        with pytest.raises(AssertionError):
            check_ref(f"{name} {k}", w[k], r64[k], r32[k], bf16=k in ("dz", "dx"))


def with_init(r, c):
    return dict(r, dgamma=c["g0"].to(r["dgamma"].dtype) + r["dgamma"], dbeta=c["b0"].to(r["dbeta"].dtype) + r["dbeta"])


@pytest.mark.parametrize("from_y", [False, True], ids=["stored-sum", "from-output"])
def test_row_loop_reading_a_row_of_the_next_pass_is_rejected(from_y):
    """2049 x 260, the smallest shape with a third pass: on its second pass the first wave reads row 2048 where it should read row 1024."""
    rows, H = 2049, 260
    c = R.exact_case(rows, H, seed=7)
    keep = R.host_keep(SEED_V, 8, rows, H, c["p"])
    idx = torch.arange(rows)
    idx[1024] = 2048
    f = dict(y=c["y"], zout=c["z"], mean=c["mean"], rstd=c["rstd"])
    r64, r32 = (with_init(bwd_of(dt, c, f, keep, c["p"], from_y), c) for dt in (F64, F32))
    wrong = with_init(bwd_of(F64, c, f, keep, c["p"], from_y, dy=c["dy"][idx], dy2=c["dy2"][idx], zb=(c["y"] if from_y else c["z"])[idx]), c)
    expect_rejected("defect[row + 1024]", wrong, r64, r32, ("dz", "dx", "dgamma", "dbeta"))


@pytest.mark.parametrize("from_y", [False, True], ids=["stored-sum", "from-output"])
def test_mask_and_scale_defects_are_rejected(from_y):
    p, salt = 0.1, 9
    c, keep, f = stored_pair(5, 260, 8, salt, p)
    r64, r32 = (with_init(bwd_of(dt, c, f, keep, p, from_y), c) for dt in (F64, F32))
    next_row = R.host_keep(SEED_V, salt, 5, 260, p, row0=1)
    assert not torch.equal(next_row, keep)
    expect_rejected("defect[mask of row + 1]", with_init(bwd_of(F64, c, f, next_row, p, from_y), c), r64, r32, ("dx",))
    c1, keep1, f1 = stored_pair(1, 260, 9, salt, p)                                  # one row is enough for the scale
    r64, r32 = (with_init(bwd_of(dt, c1, f1, keep1, p, from_y), c1) for dt in (F64, F32))
    unscaled = dict(r64, dx=torch.where(keep1, r64["dz"], torch.zeros_like(r64["dz"])))
    expect_rejected("defect[dx without 1 / (1 - p)]", unscaled, r64, r32, ("dx",))


@pytest.mark.parametrize("H,Hpad", [(260, 768), (764, 768), (772, 1024), (1000, 1024)])
@pytest.mark.parametrize("from_y", [False, True], ids=["stored-sum", "from-output"])
def test_row_means_over_the_padded_width_are_rejected(from_y, H, Hpad):
    """mean_H taken over the 768 / 1024 columns a lane's chunks span: at 764 of 768 both means are off by half a per cent only."""
    p, salt, rows = 0.1, 10, 5
    c, keep, f = stored_pair(rows, H, 10, salt, p)
    r64, r32 = (with_init(bwd_of(dt, c, f, keep, p, from_y), c) for dt in (F64, F32))
    g = c["dy"].double() + c["dy2"].double()
    xh = R.xhat_ref(F64, f["y"] if from_y else f["zout"], f["mean"], f["rstd"], c["gamma"], c["beta"] if from_y else None)
    dg = g * c["gamma"].double()
    dz = f["rstd"].double()[:, None] * (dg - dg.sum(-1, keepdim=True) / Hpad - xh * (dg * xh).sum(-1, keepdim=True) / Hpad)
    wrong = dict(r64, dz=dz, dx=torch.where(keep, dz * R.dscale(p), torch.zeros_like(dz)))
    expect_rejected(f"defect[mean over {Hpad} of H = {H}]", wrong, r64, r32, ("dz", "dx"))


@pytest.mark.parametrize("from_y", [False, True], ids=["stored-sum", "from-output"])
def test_column_sum_defects_are_rejected(from_y):
    p, salt = 0.1, 11
    c, keep, f = stored_pair(1, 4, 11, salt, p)                                      # the smallest launch there is
    r64, r32 = (with_init(bwd_of(dt, c, f, keep, p, from_y), c) for dt in (F64, F32))
    expect_rejected("defect[dgamma overwritten]", dict(r64, dgamma=bwd_of(F64, c, f, keep, p, from_y)["dgamma"]), r64, r32, ("dgamma",))
    rows, H = 333, 260                                                               # the most rows of ordinary values: the widest bound
    c, keep, f = stored_pair(rows, H, 12, salt, p)
    r64, r32 = (with_init(bwd_of(dt, c, f, keep, p, from_y), c) for dt in (F64, F32))
    g = c["dy"].double() + c["dy2"].double()
    for r in (0, 332):
        expect_rejected(f"defect[row {r} missing from dbeta]", dict(r64, dbeta=r64["dbeta"] - g[r]), r64, r32, ("dbeta",))
