"""tests/xattn_reference.py checked on the CPU: the float64 reference of the fused cross-attention block against an independent torch
evaluation, the coverage of the case tables (every xattn_fwd_kernel<NT, NCT>, dense and packed; every panel count), the precondition of
the inputs, and the checker of tests/test_xattn_block_gpu.py against the storage model itself (accepted) and against the storage model
with one known defect (rejected, each of xattn_reference.DEFECTS on every case the defect can show on)."""
import pytest
import torch

import xattn_reference as X
from helpers_gpu import attn_visible

F64 = torch.float64


def _independent(c, x):
    """The block in torch float64 with torch.softmax / layer_norm and per-sequence loops (dropout off); no helper of the reference."""
    Q, K, V, Wo, bo, R, gamma, beta = (t.double() for t in x)
    H, nH, Lq, Lkv = c["H"], c["nH"], c["Lq"], c["Lkv"]
    out = dict(ctx=torch.zeros(c["q_rows"], H, dtype=F64), z=torch.zeros(c["q_rows"], H, dtype=F64), y=torch.zeros(c["q_rows"], H, dtype=F64),
               mean=torch.zeros(c["q_rows"], dtype=F64), rstd=torch.zeros(c["q_rows"], dtype=F64), lse=torch.zeros(c["nseq"], nH, Lq, dtype=F64))
    for s in range(c["nseq"]):
        r0, n = (s * Lq, Lq) if c["q_len"] is None else (c["q_row0"][s], c["q_len"][s])
        u = c["kv_seq"][s]
        k0, nk = (u * Lkv, Lkv) if c["kv_len"] is None else (c["kv_row0"][u], c["kv_len"][u])
        q = Q[r0:r0 + n].view(n, nH, 64).transpose(0, 1)
        k, v = (t[k0:k0 + nk].view(nk, nH, 64).transpose(0, 1) for t in (K, V))
        sc = q @ k.transpose(1, 2) / 8.0
        if c["kmask"] is not None:
            sc = sc + (1.0 - c["kmask"][s, :nk].double())[None, None, :] * torch.finfo(torch.float32).min
        ctx = (torch.softmax(sc, -1) @ v).transpose(0, 1).reshape(n, H)
        z = ctx @ Wo.t() + bo + R[r0:r0 + n]
        out["ctx"][r0:r0 + n], out["z"][r0:r0 + n] = ctx, z
        out["y"][r0:r0 + n] = torch.nn.functional.layer_norm(z, (H,), gamma, beta, c["eps"])
        out["mean"][r0:r0 + n] = z.mean(-1)
        out["rstd"][r0:r0 + n] = 1.0 / torch.sqrt(z.var(-1, unbiased=False) + c["eps"])
        out["lse"][s, :, :n] = torch.logsumexp(sc, -1)
    return out


NO_DROPOUT = [n for n in X.ALL_CASES if X.CASES[n]["pa"] == 0 and X.CASES[n]["ph"] == 0]


@pytest.mark.parametrize("name", NO_DROPOUT)
def test_reference_agrees_with_an_independent_float64_evaluation(name):
    c, x, ref, _, _ = X.reference(name)
    ind = _independent(c, x)
    for k in ("ctx", "lse", "z", "mean", "rstd", "y"):
        err = (ind[k] - ref[k]).abs().max().item()
        # constant rows: rstd = 1 / sqrt(var + 1e-12) turns a variance of 1e-32 (the two evaluations' summation orders) into itself
        assert err <= 1e-11 * max(1.0, ref[k].abs().max().item()), (k, err)


def test_case_tables_cover_every_instantiation_dense_and_packed_and_every_panel_count():
    seen = {}
    for n in X.INSTANTIATION_CASES:
        c = X.CASES[n]
        seen.setdefault(X.instantiation(c["H"], c["Lkv"]), set()).add("packed" if c["kv_len"] is not None else "dense")
        assert c["Lq"] == 70 and c["nseq"] == 3 and c["nsrc"] == 2 and X.panels(c["Lq"]) == 2
        nt = X.instantiation(c["H"], c["Lkv"])[0]
        if c["kv_len"] is None:
            assert c["Lkv"] == 32 * nt and c["kmask"] is not None and not c["kmask"].all()
        else:
            assert c["Lkv"] == (31 if nt == 1 else 32 * (nt - 1) + 1) and 1 in c["kv_len"] and c["Lkv"] in c["kv_len"]
    want = {(nt, nct) for nt in (1, 2, 3, 4) for nct in (1, 2, 6)}
    print(f"instantiations covered: {len(seen)}/12")
    assert set(seen) == want and all(v == {"dense", "packed"} for v in seen.values()), seen
    for nt, nct in want:                                  # ... each with both dropouts on as well
        c = X.CASES[f"nt{nt}-nct{nct}-drop"]
        assert X.instantiation(c["H"], c["Lkv"]) == (nt, nct) and c["pa"] == 0.1 and c["ph"] == 0.1
    for H in (768, 128):
        counts = {X.panels(X.CASES[n]["Lq"]) for n in X.PANEL_CASES if X.CASES[n]["H"] == H}
        print(f"panel counts at H = {H}: {sorted(counts)}")
        assert {1, 2, 3, 4} <= counts and max(counts) >= 5
        assert {X.CASES[n]["Lq"] for n in X.PANEL_CASES if X.CASES[n]["H"] == H and X.CASES[n]["q_len"] is None} >= \
            {1, 32, 33, 63, 64, 65, 128, 129, 192, 257, 300}
        pk = X.CASES[f"panels-h{H}-packed"]
        assert pk["q_len"] == [300, 1, 64, 65] and all(b - (a + n) == X.GAP for a, n, b in zip(pk["q_row0"], pk["q_len"], pk["q_row0"][1:]))
    assert {X.CASES[n]["row_base"] for n in X.COUNTER_CASES} == {0, 1000, 2 ** 33 + 1000}
    hw = X.CASES["counter-highwords"]
    assert min(hw["seed"], hw["salt_a"], hw["salt_h"]) >= 2 ** 32 and X.CASES["counter-p05"]["pa"] == X.CASES["counter-p05"]["ph"] == 0.5


def test_instantiation_and_panels_restate_the_launcher():
    assert [X.instantiation(768, L)[0] for L in (1, 32, 33, 64, 65, 96, 97, 128)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [X.instantiation(H, 54)[1] for H in (128, 256, 768)] == [1, 2, 6]
    assert [X.panels(L) for L in (1, 64, 65, 128, 129, 256, 257, 300, 512)] == [1, 1, 2, 2, 3, 4, 5, 5, 8]


@pytest.mark.parametrize("name", X.ALL_CASES)
def test_every_query_row_keeps_a_visible_key(name):
    """Otherwise float64 and fp32 disagree about finfo.min absorption; no production batch has such a row."""
    c = X.CASES[name]
    vis = attn_visible(**X.layout_kw(c))
    for s, (_, n) in enumerate(X.seq_rows(c)):
        assert n >= 1 and vis[s, :n].any(-1).all(), (name, s)


@pytest.mark.parametrize("name", X.ALL_CASES)
def test_checker_accepts_the_storage_model(name):
    c, _, ref, model, lse32 = X.reference(name)
    margin = X.check_xattn(name, model, ref, model, c, lse32)
    assert all(v <= 0.5 + 1e-9 for k, v in margin.items() if k != "lse") and margin["lse"] == 0.0, margin


def _shows_on(defect, c):
    """Can the defect change an output of case c at all?"""
    nt = X.instantiation(c["H"], c["Lkv"])[0]
    return {"counter_q_len": c["pa"] > 0 and c["q_len"] is not None,
            "row_plus_one": c["ph"] > 0,
            "row_base_low_word": c["ph"] > 0 and c["row_base"] >= 2 ** 32,
            "last_key_tile": nt > 1,
            "kv_len_unmasked": c["kv_len"] is not None,
            "x_unrounded_stats_from_Z": c["special"] == "rounding_bias",
            "residual_before_mask": c["ph"] > 0,
            "neighbour_stats": c["special"] not in ("constant", "rounding_bias") and c["Lq"] > 1}[defect]      # (those: all rows alike)


CONTROLS = [(d, n) for d in X.DEFECTS for n in X.ALL_CASES if _shows_on(d, X.CASES[n])]


def test_every_negative_control_has_its_cases():
    for d in X.DEFECTS:
        assert any(dd == d for dd, _ in CONTROLS), d
    on = lambda d: {n for dd, n in CONTROLS if dd == d}
    assert on("last_key_tile") >= {n for n in X.INSTANTIATION_CASES if not n.startswith("nt1-")}
    assert on("kv_len_unmasked") >= {n for n in X.INSTANTIATION_CASES if n.endswith("-packed")}
    assert on("row_plus_one") >= {n for n in X.INSTANTIATION_CASES if n.endswith("-drop")} | set(X.COUNTER_CASES)
    assert on("counter_q_len") >= set(X.COUNTER_CASES) and on("row_base_low_word") == {"counter-base2p33"}


@pytest.mark.parametrize("defect,name", CONTROLS)
def test_checker_rejects_the_storage_model_with_one_defect(defect, name):
    c, x, ref, model, lse32 = X.reference(name)
    bad = X.xattn_ref64(*x, **X.ref_kw(c), storage_model=True, defect=defect)
    assert any(not torch.equal(bad[k], model[k]) for k in bad)
    with pytest.raises(AssertionError):
        X.check_xattn(f"{name} with {defect}", bad, ref, model, c, lse32)
