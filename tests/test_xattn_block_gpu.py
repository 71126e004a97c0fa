"""spmm_xattn_fwd (spmm_amd/csrc/xattn.hip: attention core + output projection + hidden dropout + residual + LayerNorm in one launch)
against the float64 reference of tests/xattn_reference.py, on every xattn_fwd_kernel<NT, NCT> the launcher can pick (dense at the upper
edge of the key-tile count, packed at the lower edge, dense with both dropouts), on 1 .. 5 row panels per sequence, with every subset of
the optional outputs, on strided operands, on the dropout counters' 64-bit range and on the LayerNorm's edge rows.

Tolerances come from the references, never from the kernel (xattn_reference.check_xattn): ctx, z, y, mean, rstd per block
||got - ref64|| <= 2 ||model - ref64|| + 2^-9 ||ref64|| with `model` the bf16 storage model of the kernel; lse by helpers_gpu.check_ref
(max(8 E32, 4 fp32 ulp)).  The dropout masks are those of the host model of the counter hash.  Every output is prefilled with NaN: rows
between packed sequences, columns beside a strided output and lse positions past a sequence's length must still hold it afterwards and
everything else must be finite.  On every case two launches are bit-identical, and ctx / lse are bit-equal to ops.attn_fwd on the same
inputs (ops.attn_fwd_long beyond 256 query rows, dense and without dropout -- the only form it takes there).
Every comparison prints `[tol] ...`, every case one `[tol-row]` line (pytest -s).

Measured on an MI355X: per case the output with the least margin; margin = ||got - ref64|| / bound (lse: |got - ref64| / bound), ratio =
||got - ref64|| / ||model - ref64|| of the worst block of that output.

| case | output | margin | ratio | lse: E32 | kernel | bound |
|---|---|---|---|---|---|---|
| nt1-nct1-dense | ctx | 0.331 | 1.000 | 4.8e-07 | 4.2e-07 | 3.9e-06 |
| nt1-nct1-packed | ctx | 0.335 | 1.000 | 5.1e-07 | 5.0e-07 | 4.1e-06 |
| nt1-nct1-drop | ctx | 0.333 | 1.000 | 5.5e-07 | 4.4e-07 | 4.4e-06 |
| nt2-nct1-dense | ctx | 0.336 | 1.000 | 5.3e-07 | 5.4e-07 | 4.2e-06 |
| nt2-nct1-packed | ctx | 0.333 | 1.000 | 4.0e-07 | 5.1e-07 | 3.2e-06 |
| nt2-nct1-drop | ctx | 0.335 | 1.000 | 5.9e-07 | 5.4e-07 | 4.8e-06 |
| nt3-nct1-dense | ctx | 0.339 | 1.001 | 4.9e-07 | 6.2e-07 | 3.9e-06 |
| nt3-nct1-packed | ctx | 0.336 | 1.000 | 5.1e-07 | 6.2e-07 | 4.1e-06 |
| nt3-nct1-drop | ctx | 0.338 | 1.000 | 5.6e-07 | 5.7e-07 | 4.5e-06 |
| nt4-nct1-dense | ctx | 0.337 | 1.000 | 5.3e-07 | 6.7e-07 | 4.2e-06 |
| nt4-nct1-packed | mean | 0.343 | 1.000 | 4.8e-07 | 6.4e-07 | 3.9e-06 |
| nt4-nct1-drop | ctx | 0.339 | 1.000 | 6.3e-07 | 6.3e-07 | 5.1e-06 |
| nt1-nct2-dense | ctx | 0.334 | 1.000 | 8.0e-07 | 5.7e-07 | 6.4e-06 |
| nt1-nct2-packed | ctx | 0.336 | 1.000 | 4.3e-07 | 5.2e-07 | 3.5e-06 |
| nt1-nct2-drop | ctx | 0.335 | 1.000 | 6.8e-07 | 6.4e-07 | 5.4e-06 |
| nt2-nct2-dense | ctx | 0.339 | 1.001 | 5.7e-07 | 5.4e-07 | 4.6e-06 |
| nt2-nct2-packed | z | 0.338 | 1.000 | 4.5e-07 | 5.9e-07 | 3.6e-06 |
| nt2-nct2-drop | ctx | 0.335 | 1.000 | 5.4e-07 | 6.0e-07 | 4.3e-06 |
| nt3-nct2-dense | ctx | 0.336 | 1.001 | 4.5e-07 | 6.0e-07 | 3.6e-06 |
| nt3-nct2-packed | ctx | 0.337 | 1.000 | 5.0e-07 | 5.9e-07 | 4.0e-06 |
| nt3-nct2-drop | ctx | 0.338 | 1.000 | 6.0e-07 | 6.6e-07 | 4.8e-06 |
| nt4-nct2-dense | ctx | 0.337 | 1.000 | 5.1e-07 | 6.4e-07 | 4.1e-06 |
| nt4-nct2-packed | ctx | 0.338 | 1.001 | 5.3e-07 | 6.6e-07 | 4.2e-06 |
| nt4-nct2-drop | ctx | 0.341 | 1.000 | 4.8e-07 | 6.1e-07 | 3.8e-06 |
| nt1-nct6-dense | z | 0.339 | 1.000 | 7.4e-07 | 6.0e-07 | 5.9e-06 |
| nt1-nct6-packed | z | 0.344 | 1.000 | 6.6e-07 | 6.1e-07 | 5.3e-06 |
| nt1-nct6-drop | y | 0.338 | 1.000 | 7.1e-07 | 9.0e-07 | 5.7e-06 |
| nt2-nct6-dense | ctx | 0.338 | 1.001 | 5.7e-07 | 6.9e-07 | 4.6e-06 |
| nt2-nct6-packed | z | 0.345 | 1.000 | 5.4e-07 | 5.7e-07 | 4.3e-06 |
| nt2-nct6-drop | ctx | 0.337 | 1.000 | 5.4e-07 | 6.3e-07 | 4.3e-06 |
| nt3-nct6-dense | ctx | 0.338 | 1.000 | 6.3e-07 | 7.3e-07 | 5.0e-06 |
| nt3-nct6-packed | z | 0.344 | 1.000 | 5.3e-07 | 5.9e-07 | 4.2e-06 |
| nt3-nct6-drop | ctx | 0.339 | 1.000 | 4.9e-07 | 6.5e-07 | 3.9e-06 |
| nt4-nct6-dense | ctx | 0.339 | 1.000 | 8.2e-07 | 7.4e-07 | 6.6e-06 |
| nt4-nct6-packed | z | 0.344 | 1.000 | 5.1e-07 | 6.6e-07 | 4.0e-06 |
| nt4-nct6-drop | ctx | 0.340 | 1.001 | 4.9e-07 | 6.7e-07 | 3.9e-06 |
| panels-h768-lq1 | mean | 0.466 | 1.000 | 2.2e-07 | 4.8e-07 | 1.9e-06 |
| panels-h768-lq32 | ctx | 0.337 | 1.000 | 5.1e-07 | 5.7e-07 | 4.1e-06 |
| panels-h768-lq33 | ctx | 0.340 | 1.001 | 5.7e-07 | 5.9e-07 | 4.6e-06 |
| panels-h768-lq63 | ctx | 0.337 | 1.000 | 6.6e-07 | 6.5e-07 | 5.3e-06 |
| panels-h768-lq64 | ctx | 0.339 | 1.000 | 8.3e-07 | 6.0e-07 | 6.7e-06 |
| panels-h768-lq65 | ctx | 0.338 | 1.000 | 6.3e-07 | 6.4e-07 | 5.0e-06 |
| panels-h768-lq128 | z | 0.335 | 1.000 | 6.6e-07 | 5.9e-07 | 5.3e-06 |
| panels-h768-lq129 | ctx | 0.337 | 1.000 | 5.5e-07 | 6.0e-07 | 4.4e-06 |
| panels-h768-lq192 | z | 0.335 | 1.000 | 6.2e-07 | 8.2e-07 | 5.0e-06 |
| panels-h768-lq256 | z | 0.335 | 1.000 | 7.8e-07 | 6.5e-07 | 6.2e-06 |
| panels-h768-lq257 | ctx | 0.336 | 1.000 | 1.1e-06 | 7.2e-07 | 8.7e-06 |
| panels-h768-lq300 | z | 0.336 | 1.000 | 6.2e-07 | 8.1e-07 | 5.0e-06 |
| panels-h768-packed | mean | 0.402 | 1.001 | 7.8e-07 | 6.1e-07 | 6.2e-06 |
| panels-h128-lq1 | ctx | 0.362 | 1.000 | 1.7e-07 | 3.0e-07 | 1.9e-06 |
| panels-h128-lq32 | ctx | 0.334 | 1.000 | 5.2e-07 | 5.2e-07 | 4.1e-06 |
| panels-h128-lq33 | ctx | 0.342 | 1.000 | 3.8e-07 | 4.4e-07 | 3.0e-06 |
| panels-h128-lq63 | ctx | 0.334 | 1.000 | 4.3e-07 | 5.3e-07 | 3.4e-06 |
| panels-h128-lq64 | ctx | 0.335 | 1.000 | 5.0e-07 | 5.4e-07 | 4.0e-06 |
| panels-h128-lq65 | ctx | 0.333 | 1.000 | 5.9e-07 | 4.6e-07 | 4.7e-06 |
| panels-h128-lq128 | ctx | 0.335 | 1.000 | 5.7e-07 | 5.5e-07 | 4.5e-06 |
| panels-h128-lq129 | ctx | 0.334 | 1.000 | 5.1e-07 | 5.6e-07 | 4.1e-06 |
| panels-h128-lq192 | ctx | 0.334 | 1.000 | 6.0e-07 | 5.6e-07 | 4.8e-06 |
| panels-h128-lq256 | ctx | 0.335 | 1.000 | 4.9e-07 | 6.1e-07 | 3.9e-06 |
| panels-h128-lq257 | ctx | 0.332 | 1.000 | 6.7e-07 | 6.7e-07 | 5.3e-06 |
| panels-h128-lq300 | ctx | 0.334 | 1.000 | 6.8e-07 | 5.8e-07 | 5.5e-06 |
| panels-h128-packed | ctx | 0.363 | 1.000 | 7.4e-07 | 5.9e-07 | 5.9e-06 |
| counter-base0 | ctx | 0.335 | 1.000 | 4.9e-07 | 5.3e-07 | 3.9e-06 |
| counter-base1000 | ctx | 0.333 | 1.000 | 8.7e-07 | 8.7e-07 | 7.0e-06 |
| counter-base2p33 | ctx | 0.334 | 1.000 | 4.6e-07 | 6.5e-07 | 3.7e-06 |
| counter-highwords | ctx | 0.333 | 1.000 | 4.8e-07 | 5.4e-07 | 3.8e-06 |
| counter-p05 | ctx | 0.339 | 1.000 | 5.2e-07 | 5.3e-07 | 4.2e-06 |
| ln-eps1e-5 | ctx | 0.337 | 1.000 | 5.8e-07 | 6.4e-07 | 4.6e-06 |
| ln-outlier | ctx | 0.337 | 1.000 | 6.0e-07 | 5.9e-07 | 4.8e-06 |
| ln-constant-h768 | ctx | 0.336 | 1.000 | 6.1e-07 | 5.8e-07 | 4.9e-06 |
| ln-constant-h128 | ctx | 0.335 | 1.000 | 4.3e-07 | 5.1e-07 | 3.4e-06 |
| ln-rounding-bias | z | 0.390 | 1.000 | 5.8e-07 | 6.2e-07 | 4.7e-06 |
| nt4-nct6-drop strided | ctx | 0.340 | 1.001 | 4.9e-07 | 6.7e-07 | 3.9e-06 |
| nt2-nct1-packed strided | ctx | 0.333 | 1.000 | 4.0e-07 | 5.1e-07 | 3.2e-06 |
| nt3-nct2-packed strided | ctx | 0.337 | 1.000 | 5.0e-07 | 5.9e-07 | 4.0e-06 |
"""
import pytest
import torch

import xattn_reference as X

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
PAD = 8                         # strided operands: a column block at offset PAD of a buffer PAD + H + PAD wide (16-byte aligned)
ALL = ("Z", "stats", "CTX", "LSE")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops as o
    return o


_dev_memo = {}


def _dev(ops, name, strided):
    """The device operands of a case.  strided: Q is the middle block of an [M, 3H] buffer, K / V the halves of [Mkv, 2H], R a column
    block of a wider buffer (the other columns hold values)."""
    if (name, strided) not in _dev_memo:
        c = X.CASES[name]
        Q, K, V, Wo, bo, R, gamma, beta = X.inputs(name)
        H = c["H"]
        i32 = lambda v: None if v is None else torch.as_tensor(v, dtype=torch.int32).cuda()
        d = dict(bo=bo.cuda(), gamma=gamma.cuda(), beta=beta.cuda(), seed=torch.tensor([c["seed"]], dtype=torch.int64, device="cuda"),
                 lay=dict(kmask=i32(c["kmask"]), kv_seq=i32(c["kv_seq"]), q_row0=i32(c["q_row0"]), q_len=i32(c["q_len"]),
                          kv_row0=i32(c["kv_row0"]), kv_len=i32(c["kv_len"])))
        if strided:
            g = torch.Generator().manual_seed(1)
            fill = lambda r, w: torch.randn(r, w, generator=g).to(BF).cuda()
            QKV, KV, Rw = fill(c["q_rows"], 3 * H), fill(c["kv_rows"], 2 * H), fill(c["q_rows"], H + 2 * PAD)
            QKV[:, H:2 * H], KV[:, :H], KV[:, H:], Rw[:, PAD:PAD + H] = Q.to(BF).cuda(), K.to(BF).cuda(), V.to(BF).cuda(), R.to(BF).cuda()
            d.update(Q=QKV[:, H:2 * H], K=KV[:, :H], V=KV[:, H:], R=Rw[:, PAD:PAD + H])
        else:
            d.update(Q=Q.to(BF).cuda(), K=K.to(BF).cuda(), V=V.to(BF).cuda(), R=R.to(BF).cuda())
        d["Wo"] = Wo.to(BF).cuda()
        d["WoF"] = ops.xattn_pack_wo(d["Wo"])
        _dev_memo[name, strided] = d
    return _dev_memo[name, strided]


def _own(c):
    own = torch.zeros(c["q_rows"], dtype=torch.bool)
    valid = torch.zeros(c["nseq"], c["nH"], c["Lq"], dtype=torch.bool)
    for s, (r0, n) in enumerate(X.seq_rows(c)):
        own[r0:r0 + n] = True
        valid[s, :, :n] = True
    return own.cuda(), valid.cuda()


def _launch(ops, name, keep=ALL, strided=False):
    """One launch into NaN-prefilled outputs.  -> {output: (whole buffer, the view the kernel was given)}; outputs not kept are absent."""
    c, d = X.CASES[name], _dev(ops, name, strided)
    H, M = c["H"], c["q_rows"]
    out = {}
    for k in ("y", "z", "ctx"):
        buf = torch.full((M, H + 2 * PAD if strided else H), NAN, dtype=BF, device="cuda")
        out[k] = (buf, buf[:, PAD:PAD + H] if strided else buf)
    for k in ("mean", "rstd"):
        out[k] = (torch.full((M,), NAN, device="cuda"),) * 2
    out["lse"] = (torch.full((c["nseq"], c["nH"], c["Lq"]), NAN, device="cuda"),) * 2
    for k, grp in (("z", "Z"), ("mean", "stats"), ("rstd", "stats"), ("ctx", "CTX"), ("lse", "LSE")):
        if grp not in keep:
            del out[k]
    view = lambda k: out[k][1] if k in out else None
    ops.xattn_fwd(d["Q"], d["K"], d["V"], d["WoF"], d["bo"], d["R"], d["gamma"], d["beta"], view("y"), nseq=c["nseq"], nH=c["nH"],
                  Lq=c["Lq"], Lkv=c["Lkv"], eps=c["eps"], Z=view("z"), mean=view("mean"), rstd=view("rstd"), CTX=view("ctx"), lse=view("lse"),
                  attn_dropout_p=c["pa"], salt_a=c["salt_a"], hidden_dropout_p=c["ph"], salt_h=c["salt_h"], seed=d["seed"],
                  row_base=c["row_base"], **d["lay"])
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b):
    """Whole buffers, the NaN prefill included."""
    return a.keys() == b.keys() and all(torch.equal(_bits(a[k][0]), _bits(b[k][0])) for k in a)


def _check_untouched(name, out, strided=False):
    """Finite exactly where the launch owns the element: the prefill everywhere else."""
    c = X.CASES[name]
    own, valid = _own(c)
    for k, (buf, _) in out.items():
        if k == "lse":
            want = valid
        elif buf.dim() == 1:
            want = own
        else:
            want = torch.zeros_like(buf, dtype=torch.bool)
            (want[:, PAD:PAD + c["H"]] if strided else want)[own] = True
        fin, nan = torch.isfinite(buf), torch.isnan(buf)
        assert torch.equal(fin, want) and torch.equal(nan, ~want), \
            f"{name} {k}: {int((fin != want).sum())} elements finite / not finite in the wrong place, {int((nan != ~want).sum())} prefill mismatches"


def _check_attn_fwd(ops, name, out, strided=False):
    """The project's invariant: ctx and lse bit-equal to the attention kernel of the composite."""
    c, d = X.CASES[name], _dev(ops, name, strided)
    if c["Lq"] > ops.ATTN_MAXL and (c["q_len"] is not None or c["pa"] > 0):
        return False                                # no launch of ops.attn_fwd / attn_fwd_long computes this one
    own, valid = _own(c)
    O = torch.full((c["q_rows"], c["H"]), NAN, dtype=BF, device="cuda")
    lse = torch.full((c["nseq"], c["nH"], c["Lq"]), NAN, device="cuda")
    ops.attn_fwd_long(d["Q"], d["K"], d["V"], O, lse, nseq=c["nseq"], nH=c["nH"], Lq=c["Lq"], Lkv=c["Lkv"], is_cross=True, dropout_p=c["pa"],
                      seed=d["seed"], salt=c["salt_a"], **d["lay"])
    torch.cuda.synchronize()
    assert torch.equal(_bits(out["ctx"][1][own]), _bits(O[own])), f"{name}: ctx differs from ops.attn_fwd"
    assert torch.equal(_bits(out["lse"][1][valid]), _bits(lse[valid])), f"{name}: lse differs from ops.attn_fwd"
    return True


def _run_case(ops, name, strided=False):
    """The checks every case gets: two launches bit-identical, untouched memory, the float64 reference, ops.attn_fwd."""
    c, _, ref, model, lse32 = X.reference(name)
    out, again = _launch(ops, name, strided=strided), _launch(ops, name, strided=strided)
    assert _same_bits(out, again), f"{name}: two launches differ"
    _check_untouched(name, out, strided)
    X.check_xattn(name + (" strided" if strided else ""), {k: v[1] for k, v in out.items()}, ref, model, c, lse32)
    _check_attn_fwd(ops, name, out, strided)
    return out


@pytest.mark.parametrize("name", X.INSTANTIATION_CASES)
def test_every_instantiation(ops, name):
    c = X.CASES[name]
    assert ops.xattn_supported(c["H"], c["nH"], c["Lq"], c["Lkv"])
    _run_case(ops, name)


@pytest.mark.parametrize("name", X.PANEL_CASES)
def test_one_to_five_row_panels(ops, name):
    _run_case(ops, name)


@pytest.mark.parametrize("name", X.COUNTER_CASES)
def test_dropout_counters(ops, name):
    _run_case(ops, name)


@pytest.mark.parametrize("name", X.LN_CASES)
def test_layernorm_edges(ops, name):
    out = _run_case(ops, name)
    if X.CASES[name]["special"] == "constant":      # z = 1.5 in every channel: y = beta to bf16 rounding, on every row
        beta = _dev(ops, name, False)["beta"]
        y = out["y"][1].float()
        assert ((y - beta).abs() <= 2.0 ** -8 * beta.abs()).all(), (y - beta).abs().max().item()


@pytest.mark.parametrize("name", ["nt4-nct6-drop", "nt2-nct1-drop"])
def test_optional_outputs_do_not_change_the_kept_ones(ops, name):
    """The engine's inference path keeps none of Z / mean, rstd / CTX / LSE; their branches sit inside the wait-counted loops."""
    full = _launch(ops, name)
    _check_untouched(name, full)
    for keep in ((), ("Z", "stats"), ("CTX",), ("LSE",), ALL):
        out = _launch(ops, name, keep=keep)
        _check_untouched(name, out)
        assert set(out) == {"y"} | {k for k, grp in (("z", "Z"), ("mean", "stats"), ("rstd", "stats"), ("ctx", "CTX"), ("lse", "LSE")) if grp in keep}
        for k in out:
            assert torch.equal(_bits(out[k][0]), _bits(full[k][0])), f"{name}: {k} changes when only {keep or 'y'} is kept"


@pytest.mark.parametrize("name", ["nt4-nct6-drop", "nt2-nct1-packed", "nt3-nct2-packed"])
def test_strided_operands(ops, name):
    """Q a column block of [M, 3H], K / V the halves of [Mkv, 2H], R / Y / Z / CTX column blocks of wider buffers: the same bits as
    the contiguous launch, and the columns beside the outputs untouched."""
    out = _run_case(ops, name, strided=True)
    plain = _launch(ops, name)
    for k in out:
        assert torch.equal(_bits(out[k][1].contiguous()), _bits(plain[k][1])), f"{name}: {k} depends on the strides"


@pytest.mark.parametrize("H", [128, 256, 768])
def test_pack_wo_reads_a_strided_weight(ops, H):
    g = torch.Generator().manual_seed(H)
    wide = torch.randn(H, H + 3 * PAD, generator=g).to(BF).cuda()
    view = wide[:, PAD:PAD + H]
    assert not view.is_contiguous()
    a, b = ops.xattn_pack_wo(view), ops.xattn_pack_wo(view.contiguous())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(a.float().sort().values, view.float().reshape(-1).sort().values)        # a permutation of the weight's elements
