"""spmm_s2p_append (csrc/heads.hip) against a float64 numpy restatement: the last Linear(H, 1) of property_mtr_head on the last-position
rows, then property_embed + BertEmbeddings (inputs_embeds branch: + position row + token type 0, LayerNorm) of the predicted value,
appended to the cache of embedded prefix rows.

Tolerances come from the number formats, never from the kernel:
  pred   fp32 dot of H bf16 x fp32 terms: |d| <= 1e-5 * (|b3| + sum |y w3|)  (a lane adds H/64 <= 16 products, the butterfly six
         more levels: (16 + 6) * 2^-24 = 1.3e-6 of the absolute sum; 1e-5 is the project's fp32-accumulation allowance).
  cache  the float64 LayerNorm of the kernel's OWN fp32 p (so that the prediction's error is not charged twice), within one bf16 ulp
         of that value (relative 2^-8: the rounding to bf16 is half an ulp, 2^-9, the other half covers a value that fp32 puts on the
         other side of a rounding boundary) plus what fp32 arithmetic itself may move the un-rounded value by:
           e = p w + b + pos + type0 is three fp32 operations on terms of size <= max|e| (4 roundings allowed), and the fp32 mean of H
           such values adds H/64 sequential roundings in a lane and six butterfly levels; an error of e or of the mean is divided by the
           row's standard deviation sigma -- the term that matters for a nearly constant row -- and variance / scale / shift are a
           handful more roundings of the O(1) normalised value:
           |d xhat| <= min((10 + H/64) * 2^-24 * max|e| / sigma, 2^-10) + 16 * 2^-24 * (1 + |xhat|);   |d out| <= |gamma| |d xhat| + 2^-23 * (|xhat gamma| + |beta|).
         The sigma term is a worst case (every rounding in the same direction) and is CAPPED at 2^-10, a quarter of a bf16 ulp of 1: on
         ordinary rows the whole allowance is ~1e-6 (it only keeps the relative bound meaningful for outputs near zero), on the nearly
         constant row it adds at most a quarter ulp to the one ulp the bound allows.
Buffers are canary-filled: every byte the launch must not write is compared bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = 1e-12
CANARY_BF, CANARY_F32 = -7.0, -12345.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops as o
    return o


def _inputs(rows, H, n_props, seed):
    """y rows bf16-rounded; row 0: y = 0, so p = b3 = 1e-2 and e is nearly constant (pe_b + pos + type0 is one constant per column);
    the last row: |p| ~ 30."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(rows, H, generator=g).to(BF)
    w3 = torch.randn(H, generator=g) * H ** -0.5
    b3 = torch.tensor([1e-2])
    y[0] = 0
    if rows > 1:
        y[rows - 1] = (30.0 * w3 / (w3 * w3).sum()).to(BF)
    pe_w = torch.randn(H, generator=g) * 0.1
    pos = torch.randn(n_props + 1, H, generator=g) * 0.05
    type0 = torch.randn(H, generator=g) * 0.05
    pe_b = torch.randn(H, generator=g) * 0.05
    gamma = 1.0 + 0.1 * torch.randn(H, generator=g)
    beta = 0.1 * torch.randn(H, generator=g)
    return dict(y=y, w3=w3, b3=b3, pe_w=pe_w, pe_b=pe_b, pos=pos, type0=type0, gamma=gamma, beta=beta)


def _run(ops, t, rows, H, n_props, i, ldy, ldp, const_row0=False, with_type0=True):
    dev = "cuda"
    t = {k: v.clone() for k, v in t.items()}
    if const_row0:      # pe_b + pos[j] + type0 == 1 in every column: the rows' e differ from a constant by p * pe_w only
        j = min(i + 1, n_props)
        t["pe_b"] = (1.0 - t["pos"][j].double() - (t["type0"].double() if with_type0 else 0)).float()
    ybuf = torch.full((rows, ldy), CANARY_BF, dtype=BF)
    ybuf[:, :H] = t["y"]
    yd = ybuf.to(dev)[:, :H]
    pred = torch.full((rows, ldp), CANARY_F32, dtype=torch.float32, device=dev)
    xc = torch.full((rows, n_props + 1, H), CANARY_BF, dtype=BF, device=dev)
    d = {k: v.to(dev).contiguous() for k, v in t.items() if k != "y"}
    ops.s2p_append(yd, d["w3"], d["b3"], pred, i, n_props=n_props, xcache=xc, pe_w=d["pe_w"], pe_b=d["pe_b"], pos=d["pos"],
                   type0=d["type0"] if with_type0 else None, gamma=d["gamma"], beta=d["beta"], eps=EPS)
    torch.cuda.synchronize()
    return t, pred.cpu(), xc.cpu()


def _check(t, pred, xc, rows, H, n_props, i, with_type0=True, tag=""):
    y64, w64 = t["y"].double().numpy(), t["w3"].double().numpy()
    want_p = float(t["b3"]) + (y64 * w64).sum(1)
    bound_p = 1e-5 * (abs(float(t["b3"])) + np.abs(y64 * w64).sum(1))
    got_p = pred[:, i].double().numpy()
    err_p = np.abs(got_p - want_p)
    print(f"[tol] s2p_append{tag} rows={rows} H={H} n_props={n_props} i={i}: pred max err {err_p.max():.3e} (bound {bound_p[err_p.argmax()]:.3e}), max |p| {np.abs(got_p).max():.3g}")
    assert (err_p <= bound_p).all(), (err_p.max(), bound_p.min())
    # every other column of pred is untouched
    others = torch.ones(pred.shape[1], dtype=torch.bool)
    others[i] = False
    assert (pred[:, others] == CANARY_F32).all()
    canary = torch.tensor(CANARY_BF, dtype=BF)
    if i == n_props - 1:
        assert (xc == canary).all(), "the last step must not write the cache"
        return
    j = i + 1
    keep = torch.ones(n_props + 1, dtype=torch.bool)
    keep[j] = False
    assert (xc[:, keep] == canary).all(), "a cache row other than j was written"
    p = got_p[:, None]                                              # the kernel's own fp32 p
    e = p * t["pe_w"].double().numpy() + t["pe_b"].double().numpy() + t["pos"][j].double().numpy()
    if with_type0:
        e = e + t["type0"].double().numpy()
    mean = e.mean(1, keepdims=True)
    sigma = np.sqrt(((e - mean) ** 2).mean(1, keepdims=True) + EPS)
    xhat = (e - mean) / sigma
    gm, bt = t["gamma"].double().numpy(), t["beta"].double().numpy()
    want = xhat * gm + bt
    u = 2.0 ** -24
    d_xhat = np.minimum((10 + H / 64) * u * np.abs(e).max(1, keepdims=True) / sigma, 2.0 ** -10) + 16 * u * (1 + np.abs(xhat))
    slack = np.abs(gm) * d_xhat + 2 * u * (np.abs(xhat * gm) + np.abs(bt))
    bound = 2.0 ** -8 * np.abs(want) + slack
    got = xc[:, j].double().numpy()
    err = np.abs(got - want)
    k = (err / bound).argmax()
    print(f"[tol] s2p_append{tag} cache row {j}: worst err/bound {(err / bound).max():.3f} (err {err.flat[k]:.3e}, bound {bound.flat[k]:.3e}, "
          f"of which fp32 slack {slack.flat[k]:.3e}); min sigma/max|e| {(sigma / np.abs(e).max(1, keepdims=True)).min():.2e}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (err.flat[k], bound.flat[k])


@pytest.mark.parametrize("n_props", [12, 53])
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("rows", [1, 5, 67])
def test_s2p_append_matches_float64(ops, rows, H, n_props):
    t = _inputs(rows, H, n_props, seed=1000 + rows + H + n_props)
    for i in sorted({0, 11, n_props - 2, n_props - 1}):
        wide = (i == 0)                                              # ldy > H and ldp > n_props at the first step of every shape
        tt, pred, xc = _run(ops, t, rows, H, n_props, i, ldy=H + 8 if wide else H, ldp=n_props + 3 if wide else n_props)
        _check(tt, pred, xc, rows, H, n_props, i)


@pytest.mark.parametrize("H", [64, 768])
def test_s2p_append_nearly_constant_row_and_large_value(ops, H):
    """Row 0's e differs from the constant 1 by 1e-2 * pe_w (sigma / max|e| ~ 1e-3: the small-variance case of the two-pass variance);
    the last row's |p| is ~30."""
    rows, n_props = 5, 53
    t = _inputs(rows, H, n_props, seed=77 + H)
    tt, pred, xc = _run(ops, t, rows, H, n_props, 7, ldy=H, ldp=n_props, const_row0=True)
    assert abs(float(pred[0, 7]) - 1e-2) < 1e-8 and 25 < abs(float(pred[rows - 1, 7])) < 35
    _check(tt, pred, xc, rows, H, n_props, 7, tag="[const]")


def test_s2p_append_without_the_token_type_row(ops):
    rows, H, n_props = 5, 128, 12
    t = _inputs(rows, H, n_props, seed=5)
    tt, pred, xc = _run(ops, t, rows, H, n_props, 3, ldy=H, ldp=n_props, with_type0=False)
    _check(tt, pred, xc, rows, H, n_props, 3, with_type0=False, tag="[no type0]")
