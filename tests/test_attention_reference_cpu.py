"""The float64 attention reference, its bf16 storage model and the mask probes of tests/helpers_gpu.py, checked on the CPU: the bound of
tests/test_attention_dropout_gpu.py accepts the storage model and rejects the defects it is there to catch, and the three probes return
the mask that was put in."""
import pytest
import torch

from helpers_gpu import (attention_dropout_case, attention_keep_mask, attention_layout_kw, attention_parity_blocks, attention_ref64,
                         attn_visible, check_attention_parity, probe_dq_mismatches, probe_masks)

NAMES = ("O", "dQ", "dK", "dV")
CASES = ["a", "f1", "f2"]


def _inputs(c):
    g = torch.Generator().manual_seed(11 + c["q_rows"])
    H = c["nH"] * 64
    r = lambda n: torch.randn(n, H, generator=g).to(torch.bfloat16).float()
    return r(c["q_rows"]), r(c["kv_rows"]), r(c["kv_rows"]), r(c["q_rows"])


_memo = {}


def _case(name):
    """(case, inputs, host mask, ref64 outputs, storage-model outputs), computed once and left unchanged."""
    if name not in _memo:
        c = attention_dropout_case(name)
        x = _inputs(c)
        keep = attention_keep_mask(c["seed"], c["salt"], c["nseq"], c["nH"], c["Lq"], c["Lkv"], c["p"])
        kw = dict(attention_layout_kw(c), p=c["p"], keep=keep)
        ref, model = attention_ref64(*x, **kw), attention_ref64(*x, **kw, storage_model=True)
        _memo[name] = c, x, keep, kw, ref, model
    return _memo[name]


def _tensors(out):
    return dict(zip(NAMES, (out[0], out[2], out[3], out[4])))


@pytest.mark.parametrize("name", CASES)
def test_reference_agrees_with_autograd_of_the_same_formula(name):
    c, (Q, K, V, dO), keep, kw, ref, _ = _case(name)
    assert c["kv_seq"] is None and c["q_row0"] is None
    nseq, nH, Lq, Lkv = c["nseq"], c["nH"], c["Lq"], c["Lkv"]
    hd = lambda t, L: t.double().view(nseq, L, nH, 64).permute(0, 2, 1, 3).clone().requires_grad_(True)
    q, k, v = hd(Q, Lq), hd(K, Lkv), hd(V, Lkv)
    vis = attn_visible(**attention_layout_kw(c))[:, None]
    m = torch.ones(nseq, 1, 1, Lkv, dtype=torch.float64) if c["kmask"] is None else c["kmask"].double()[:, None, None, :]
    if c["is_cross"]:
        add = (1 - m) * torch.finfo(torch.float32).min
    else:
        add = (1 - vis.double()) * -10000.0
    s = q @ k.transpose(-1, -2) / 8 + add
    o = (torch.softmax(s, -1) * keep.double() / (1 - c["p"])) @ v
    o.backward(hd(dO, Lq).detach())
    for nm, a, b in (("O", o.detach(), ref[0]), ("lse", torch.logsumexp(s, -1).detach(), ref[1]), ("dQ", q.grad, ref[2]), ("dK", k.grad, ref[3]),
                     ("dV", v.grad, ref[4])):
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item()), nm


@pytest.mark.parametrize("name", CASES)
def test_storage_model_sits_a_few_bf16_roundings_from_float64_and_passes_its_own_bound(name):
    _, _, _, _, ref, model = _case(name)
    for nm, r, m in ((n, _tensors(ref)[n], _tensors(model)[n]) for n in NAMES):
        rel = (m - r).flatten(2).norm(dim=-1) / r.flatten(2).norm(dim=-1)
        assert 5e-4 < rel.min().item() and rel.max().item() < 8e-3, (nm, rel)
        assert check_attention_parity(nm, m, r, m) == pytest.approx(1.0)
    assert torch.equal(ref[1], model[1])                                # lse stays unrounded


def _rejected(got, ref, model):
    """Per tensor: bool [n, nH], the blocks over the bound."""
    out = {}
    for nm in NAMES:
        eg, _, bound = attention_parity_blocks(_tensors(got)[nm], _tensors(ref)[nm], _tensors(model)[nm])
        out[nm] = eg > bound
    return out


@pytest.mark.parametrize("name", CASES)
def test_bound_rejects_one_flipped_16_key_tile_of_one_row_per_head(name):
    c, x, keep, kw, ref, model = _case(name)
    bad = keep.clone()
    q = c["Lq"] - 1                                                         # the last row sees keys 0..15 in every sequence of these cases
    assert attn_visible(**attention_layout_kw(c))[:, q, :16].all()
    bad[:, :, q, :16] ^= True
    rej = _rejected(attention_ref64(*x, **dict(kw, keep=bad), storage_model=True), ref, model)
    for nm in NAMES:
        assert rej[nm].all(), (nm, rej[nm])
        with pytest.raises(AssertionError):
            check_attention_parity(nm, _tensors(attention_ref64(*x, **dict(kw, keep=bad), storage_model=True))[nm], _tensors(ref)[nm],
                                   _tensors(model)[nm])


@pytest.mark.parametrize("name", CASES)
def test_bound_rejects_the_row_counter_of_a_wrong_Lq(name):
    """The packed length of a sequence in place of the launch's dense Lq (case a: the key mask's prefix lengths; f: one row less).  Blocks
    whose counter does not move -- (sequence 0, head 0) always; every head of a sequence whose length IS Lq -- keep their mask and pass."""
    c, x, keep, kw, ref, model = _case(name)
    wrong = [54, 40, 29] if name == "a" else [c["Lq"] - 1] * c["nseq"]
    bad = attention_keep_mask(c["seed"], c["salt"], c["nseq"], c["nH"], c["Lq"], c["Lkv"], c["p"], counter_Lq=wrong)
    moved = (bad != keep).flatten(2).any(-1)
    assert moved.sum() >= moved.numel() - c["nH"] and not moved[0, 0]
    rej = _rejected(attention_ref64(*x, **dict(kw, keep=bad), storage_model=True), ref, model)
    for nm in NAMES:
        assert torch.equal(rej[nm], moved), (nm, rej[nm], moved)


@pytest.mark.parametrize("name", CASES)
def test_bound_rejects_a_missing_dropout_scale_in_dP(name):
    c, x, keep, kw, ref, model = _case(name)
    rej = _rejected(attention_ref64(*x, **kw, storage_model=True, dp_scale=1.0), ref, model)
    assert rej["dQ"].all() and rej["dK"].all(), rej                       # dP reaches dQ and dK through dS
    assert not rej["O"].any() and not rej["dV"].any(), rej


@pytest.mark.parametrize("storage_model", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_probes_return_the_mask_that_was_put_in(name, storage_model):
    c, _, keep, kw, _, _ = _case(name)
    vis = attn_visible(**attention_layout_kw(c))
    want = keep & vis[:, None]

    def run(Q, K, V, dO, bwd):
        O, _, dQ, dK, dV = attention_ref64(Q, K, V, dO, **kw, storage_model=storage_model)
        return O, dQ, dK, dV

    fw, dv, (dq, flat, spread) = probe_masks(run, c)
    assert torch.equal(fw, want) and torch.equal(dv, want)
    assert probe_dq_mismatches(dq, flat, want, vis) == 0
    assert spread < 1 / 16, spread
    # the rows the dP probe cannot read are exactly those whose visible decisions are all alike (one-key rows of the causal sequences ...)
    kept, n = want.sum(-1), vis.sum(-1)[:, None].expand(-1, c["nH"], -1)
    assert torch.equal(flat, (kept == 0) | (kept == n))
    assert torch.equal(dq & ~flat[..., None], want & ~flat[..., None])
    # ... and a probe that read another mask is noticed
    other = attention_keep_mask(c["seed"] + 1, c["salt"], c["nseq"], c["nH"], c["Lq"], c["Lkv"], c["p"]) & vis[:, None]
    assert probe_dq_mismatches(dq, flat, other, vis) > 0.1 * int(vis.sum()) * c["nH"]
