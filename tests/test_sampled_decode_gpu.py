"""Seeded sampled PV -> SMILES search on the GPU: the counter-noise kernel against its host form, the SAMPLED instantiation of the
one-launch beam step against the tensor-op bookkeeping (every comparison exact: the noise is an explicit tensor), the search end to
end (fused = tensor-op form, compaction, reproducibility), generate_with_property and the pv2smiles.py driver."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_step_gpu import _mk, _peaky_lm          # tests/test_step_gpu.py: model construction helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from spmm_amd import ops as _ops
    return _ops


def _seed_tensor(seed):
    return torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------------------------------------ noise kernel
@pytest.mark.parametrize("N,k,V", [(37, 5, 300), (6, 3, 500), (20, 1, 70)])
def test_gumbel_noise_kernel_matches_the_host_form(ops, N, k, V):
    """csrc/decode.hip::gumbel_noise_kernel against decode.gumbel_noise_host (same integers, float64 transform): |g - g64| <= 1e-5
    everywhere (a wrong counter or hash gives unrelated values, O(1) apart); a molecule's rows are BIT-equal whether it is filled with
    the whole batch, with a part of it or alone; the position from device memory gives what the argument gives."""
    from spmm_amd import decode
    Lmax, t, salt, seed, base = 19, 4, decode.GUMBEL_SALT, (1 << 63) + 12345, 1000
    sd = _seed_tensor(seed)
    got = ops.gumbel_noise(sd, N, k, V, Lmax, salt=salt, t=t)
    want = decode.gumbel_noise_host(seed, salt, range(N), t, k, V, Lmax)
    assert tuple(got.shape) == (N * k, V) and bool(torch.isfinite(got).all())
    err = (got.double().cpu() - want).abs().max().item()
    print(f"gumbel noise N={N} k={k} V={V}: max |g - g64| = {err:.2e}")
    assert err <= 1e-5
    # through a permutation of the state indices and an offset of the global molecule index
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(N)).to(torch.int32)
    full = ops.gumbel_noise(sd, N, k, V, Lmax, salt=salt, t=t, mol=perm.cuda(), mol_base=base)
    want = decode.gumbel_noise_host(seed, salt, (base + perm.long()).tolist(), t, k, V, Lmax)
    assert (full.double().cpu() - want).abs().max().item() <= 1e-5
    a, b = N // 3, N // 3 + max(N // 4, 1)
    part = ops.gumbel_noise(sd, b - a, k, V, Lmax, salt=salt, t=t, mol=perm[a:b].contiguous().cuda(), mol_base=base)
    assert torch.equal(part, full[a * k:b * k])
    alone = ops.gumbel_noise(sd, 1, k, V, Lmax, salt=salt, t=t, mol_base=base + int(perm[a]))
    assert torch.equal(alone, full[a * k:(a + 1) * k])
    # the position from device memory; into a wider buffer (row stride > V)
    t_dev = torch.tensor([t - 1], dtype=torch.int32, device="cuda")
    wide = torch.full((N * k, V + 12), 7.0, device="cuda")
    ops.gumbel_noise(sd, N, k, V, Lmax, salt=salt, t=0, t_ptr=t_dev, t_off=1, out=wide)
    assert torch.equal(wide[:, :V], got) and bool((wide[:, V:] == 7.0).all())
    # another position, another salt, another seed: other noise
    for kw in (dict(t=t + 1), dict(salt=salt + 1)):
        other = ops.gumbel_noise(sd, N, k, V, Lmax, **{**dict(salt=salt, t=t), **kw})
        assert not torch.equal(other, got)
    assert not torch.equal(ops.gumbel_noise(_seed_tensor(seed + 1), N, k, V, Lmax, salt=salt, t=t), got)


def test_gumbel_noise_rejects_bad_shapes(ops):
    sd = _seed_tensor(1)
    for N, k, V, Lmax, t in ((4, 9, 30, 19, 1), (4, 2, 513, 19, 1), (4, 2, 30, 19, 19), (4, 2, 30, 300, 1), (4, 2, 30, 19, -1)):
        out = torch.full((N * k, V), 3.0, device="cuda")
        with pytest.raises(RuntimeError, match="spmm_gumbel_noise"):
            ops.gumbel_noise(sd, N, k, V, Lmax, t=t, out=out)
        assert bool((out == 3.0).all())                                  # refused before any launch
    with pytest.raises(RuntimeError, match="spmm_gumbel_noise"):
        ops.gumbel_noise(sd, 4, 2, 30, 19, t=1, mol_base=-1)


# ------------------------------------------------------------------------------------------------------------------ sampled beam step
def _beam_case(N, k, V, gseed, T=16):
    """Logits and noise of T positions (CPU, one generator) with [SEP] boosted as in test_beam_step_kernel_matches_tensor_bookkeeping, and
    the REFERENCE trajectory: BeamBook.update fed by _pick_seeded on the CPU, with the state after every position."""
    from spmm_amd import decode
    L, R = T + 3, N * k
    g = torch.Generator().manual_seed(gseed)
    v0, i0 = torch.randn(N, k, generator=g), torch.randint(4, V, (N, k), generator=g)
    ref = decode.BeamBook(N, k, T, "cpu")
    ref.first(v0, i0)
    rows = torch.arange(R, dtype=torch.int32)
    anc = rows[:, None].repeat(1, L).contiguous()
    steps = []
    for s in range(T):
        logits = torch.randn(R, V, generator=g) * 2.0
        boost = torch.rand(R, generator=g) < 0.12
        logits[:, decode.SEP_ID] += torch.where(boost, torch.full((R,), 6.0), torch.full((R,), -2.0))
        noise = -torch.log(-torch.log(torch.rand(R, V, generator=g).clamp(1e-7, 1 - 1e-7)))
        was_done, cur_p = ref.done.clone(), ref.cur_p.clone()
        values, indices = decode._pick_seeded(logits.view(N, k, V), noise, k)
        # ---- margins, from the reference alone: rows of molecules live BEFORE this position
        key = (logits + noise).view(N, k, V)
        top = torch.topk(key, min(k + 1, V), dim=-1).values
        key_ties = ((top[..., :-1] == top[..., 1:]).any(-1) & ~was_done[:, None]).any().item()
        k2 = (cur_p[:, :, None] + values).reshape(N, k * k)
        k2 = torch.where((indices.reshape(N, k * k) == decode.SEP_ID), torch.full_like(k2, -1e5), k2)          # struck out: never among the survivors of a live molecule
        c = torch.sort(k2, dim=1, descending=True).values[:, :min(k + 1, k * k)]
        gap = torch.where(c[:, 1:] > -9e4, c[:, :-1] - c[:, 1:], torch.full_like(c[:, 1:], float("inf")))
        parent, tok = ref.update(values, indices)
        live_after = ~ref.done
        min_gap = gap[live_after].min().item() if bool(live_after.any()) and gap.numel() else float("inf")
        anc = anc.view(N, k, L).gather(1, parent[:, :, None].expand(N, k, L)).reshape(R, L).contiguous()
        anc[:, s + 2:] = rows[:, None]
        steps.append(dict(logits=logits, noise=noise, key_ties=key_ties, min_gap=min_gap, tok=tok.reshape(R).clone(), anc=anc.clone(),
                          done=ref.done.clone(), fin_n=ref.fin_n.clone(), tokens=ref.tokens.clone(), cur_p=ref.cur_p.clone(),
                          fin_p=ref.fin_p.clone(), fin_len=ref.fin_len.clone(), fin_tok=ref.fin_tok.clone()))
        if bool(ref.done.all()):
            break
    return v0, i0, steps, ref


# generator seed of every case: the first one (counting up from 3) whose REFERENCE trajectory has the margins asserted below and finishes molecules
BEAM_CASES = [(37, 5, 300, False), (9, 8, 300, False), (20, 1, 70, False), (6, 3, 500, False), (5, 2, 320, False), (3, 2, 321, False),
              (11, 3, 300, True)]
BEAM_SEEDS = {(37, 5, 300): 6, (9, 8, 300): 3, (20, 1, 70): 3, (6, 3, 500): 3, (5, 2, 320): 3, (3, 2, 321): 4, (11, 3, 300): 3}


@pytest.mark.parametrize("N,k,V,compacted", BEAM_CASES)
def test_sampled_beam_step_matches_tensor_bookkeeping(N, k, V, compacted):
    """The SAMPLED instantiation of csrc/decode.hip::beam_step_kernel (spmm_beam_step_sampled) against decode._pick_seeded +
    BeamBook.update + the ancestry gather, position by position, from the same logits and the same explicit fp32 noise: tokens, finals and
    their slots, fin_n, done, the ancestry of live rows and the next ids bit-equal, scores within 2e-5.  (37, 5, 300): one wave in the last
    workgroup; (5, 2, 320) / (3, 2, 321): the two sides of the switch between the 5- and the 8-register instantiation.  compacted: the
    batch is a subset of a larger state (`mol`) whose rows own scattered K/V cache rows (`rowmap`), as after a compaction.
    The reference runs on the CPU; the test first asserts from it alone that the comparison is well posed: no two of a live row's top
    k + 1 keys are equal, and the top k + 1 candidate scores of every live molecule are pairwise more than 1e-4 apart (5 x the score
    tolerance), so neither side's rounding can change a decision."""
    from spmm_amd import decode
    T = 16
    L, R = T + 3, N * k
    v0, i0, steps, ref = _beam_case(N, k, V, BEAM_SEEDS[(N, k, V)], T)
    for s, st in enumerate(steps):
        assert not st["key_ties"], s
        assert st["min_gap"] > 1e-4, (s, st["min_gap"])
    if compacted:
        NS = N + 6                                                       # molecules of the state; the batch holds N of them, out of order
        keep = torch.randperm(NS, generator=torch.Generator().manual_seed(1))[:N]
        rowmap = (keep[:, None] * k + torch.arange(k)[None, :]).reshape(R).to(torch.int32)
    else:
        NS, keep, rowmap = N, torch.arange(N), torch.arange(R, dtype=torch.int32)
    fus = decode.BeamBook(NS, k, T, "cuda", fused=True)
    vf, idf = torch.zeros(NS, k), torch.full((NS, k), 5)
    vf[keep], idf[keep] = v0, i0
    fus.first(vf.cuda(), idf.cuda())
    if compacted:
        fus.mol = keep.to(torch.int32).cuda()
    untouched = torch.ones(NS, dtype=torch.bool)
    untouched[keep] = False
    tokens0 = fus.tokens.clone().cpu()
    anc_fus = rowmap[:, None].repeat(1, L).contiguous().cuda()
    rm = rowmap.long()
    F = ref.F
    for s, st in enumerate(steps):
        ids = fus.step_fused(st["logits"].cuda(), anc_fus, rowmap=rowmap.cuda() if compacted else None, noise=st["noise"].cuda())
        done, fin_n = fus.done.cpu()[keep], fus.fin_n.cpu().long()[keep]
        assert torch.equal(done, st["done"]) and int(fus.n_done) == int(st["done"].sum()), s
        assert torch.equal(fin_n, st["fin_n"]), s
        assert torch.equal(fus.tokens.cpu().long()[keep], st["tokens"]), s
        torch.testing.assert_close(fus.cur_p.cpu()[keep], st["cur_p"], rtol=0, atol=2e-5)
        fp_f, fp_r = fus.fin_p.cpu()[keep][:, :F], st["fin_p"][:, :F]
        assert torch.equal(torch.isinf(fp_f), torch.isinf(fp_r)), s
        torch.testing.assert_close(torch.where(torch.isinf(fp_f), torch.zeros_like(fp_f), fp_f), torch.where(torch.isinf(fp_r), torch.zeros_like(fp_r), fp_r),
                                   rtol=0, atol=2e-5)
        used = torch.arange(F)[None, :] < st["fin_n"][:, None]
        assert torch.equal(fus.fin_len.cpu()[keep][:, :F].long()[used], st["fin_len"][:, :F][used]), s
        assert torch.equal(fus.fin_tok.cpu()[keep][:, :F].long()[used], st["fin_tok"][:, :F][used]), s
        lr = (~st["done"])[:, None].expand(N, k).reshape(R)
        assert torch.equal(ids.cpu().long()[lr], st["tok"][lr]), s
        assert torch.equal(anc_fus.cpu().long()[lr], rm[st["anc"].long()][lr]), s              # (reference rows are batch rows: through the row map)
        af = anc_fus.cpu().view(N, k, L)
        assert torch.equal(af[st["done"]], af[st["done"]][:, :1].expand(-1, k, -1)), s            # finished molecules: beam 0's ancestry for all beams
    assert torch.equal(fus.tokens.cpu()[untouched], tokens0[untouched]) and not bool(fus.done.cpu()[untouched].any())
    n_fin = int(steps[-1]["fin_n"].sum())
    assert n_fin >= min(N, 8) and bool(steps[-1]["done"].any())
    got, want = fus.results(), ref.results()
    assert [[h[1] for h in got[int(n)]] for n in keep] == [[h[1] for h in m] for m in want]
    # the deterministic entry refuses nothing it accepted before, and the sampled one insists on its noise
    from spmm_amd import ops
    with pytest.raises(AssertionError):
        ops.beam_step(steps[0]["logits"].cuda(), fus, t=2, noise=steps[0]["noise"][:, :V - 1].contiguous().cuda())


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def peaky(env):
    O, SPMM, tiny_config, *_ = env
    sd = _peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), sep_gap=0.4)
    return _mk(SPMM, tiny_config(), sd).eval()


def _toks(res):
    return [[h[1] for h in mol] for mol in res]


def test_seeded_search_is_the_same_on_the_fused_and_the_tensor_op_path(peaky):
    """12 molecules x 4 beams, 14 positions, seed 7: the search on spmm_beam_step_sampled returns, token for token, what _pick_seeded +
    BeamBook.update return from the same counter noise; the same seed twice is identical, another seed is not; every hypothesis is
    [CLS] ... [SEP] and its score is the teacher-forced log-probability of the uncached forward (3e-2 per token, bf16 activations)."""
    from spmm_amd import decode
    m = peaky
    N, k, T = 12, 4, 14
    props = torch.randn(N, 53, generator=torch.Generator().manual_seed(4)) * 2
    fused = decode.beam_search_batched(m, props, k=k, max_steps=T, stochastic=True, seed=7)
    again = decode.beam_search_batched(m, props, k=k, max_steps=T, stochastic=True, seed=7)
    other = decode.beam_search_batched(m, props, k=k, max_steps=T, stochastic=True, seed=8)
    prev = decode.FUSED_BEAM_STEP
    decode.FUSED_BEAM_STEP = False
    try:
        plain = decode.beam_search_batched(m, props, k=k, max_steps=T, stochastic=True, seed=7)
    finally:
        decode.FUSED_BEAM_STEP = prev
    assert _toks(fused) == _toks(plain)
    for a, b in zip(fused, plain):
        for (pa, _), (pb, _) in zip(a, b):
            assert abs(pa - pb) < 1e-4
    assert _toks(again) == _toks(fused) and [[h[0] for h in mol] for mol in again] == [[h[0] for h in mol] for mol in fused]
    assert _toks(other) != _toks(fused)
    greedy = decode.beam_search_batched(m, props, k=k, max_steps=T)
    assert _toks(greedy) != _toks(fused)                                 # (it does sample)
    pe = decode.encode_properties(m, props)
    n_hyp = 0
    for n in range(N):
        assert len(fused[n]) <= k
        for p, seq in fused[n]:
            n_hyp += 1
            assert seq[0] == decode.CLS_ID and seq[-1] == decode.SEP_ID
            text = torch.tensor([seq], device="cuda")
            logits = m.text_encoder(text, attention_mask=torch.ones_like(text), encoder_hidden_states=pe[n:n + 1],
                                    encoder_attention_mask=torch.ones(1, pe.shape[1], dtype=torch.long, device="cuda"),
                                    return_dict=True, is_decoder=True, return_logits=True)
            lp = torch.log_softmax(logits.float(), -1)[0, :-1].gather(1, text[0, 1:, None]).sum().item()
            assert abs(lp - p) < 3e-2 * (len(seq) - 1), (n, seq, lp, p)
    print(f"seeded sampled search: {n_hyp} hypotheses for {N} molecules")
    assert n_hyp >= N
    # a molecule's draws do not depend on the batch it is decoded in: the last four alone, under their global indices
    tail = decode.beam_search_batched(m, props[8:], k=k, max_steps=T, stochastic=True, seed=7, mol_base=8)
    assert _toks(tail) == _toks(fused)[8:]


def test_seeded_search_with_compaction_equals_the_whole_batch(env):
    """Finished molecules leave the seeded search as they leave the deterministic one (sizes and sep_gap of
    test_batched_decode_drops_finished_molecules): same hypotheses with and without compaction, and the batch did shrink."""
    O, SPMM, tiny_config, *_ = env
    from spmm_amd import decode
    sd = _peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), seed=5, sep_gap=0.9)
    m = _mk(SPMM, tiny_config(), sd).eval()
    props = torch.randn(32, 53, generator=torch.Generator().manual_seed(12)) * 10.0
    whole = decode.beam_search_batched(m, props, k=5, max_steps=40, compact=False, stochastic=True, seed=7)
    assert decode.last_run["compactions"] == 0
    small = decode.beam_search_batched(m, props, k=5, max_steps=40, compact=True, stochastic=True, seed=7)
    run = dict(decode.last_run)
    print(f"seeded decode with compaction: {run}")
    assert run["compactions"] >= 1 and run["final_batch"] < 32
    assert _toks(small) == _toks(whole)
    for a, b in zip(small, whole):
        for (pa, _), (pb, _) in zip(a, b):
            assert abs(pa - pb) < 1e-4


def test_generate_with_property(peaky, monkeypatch):
    """24 samples from one PV with 33 properties masked, k = 2: sample i is molecule i of the seeded search on the repeated PV, one of its
    finals picked by random.Random(seed) in sample order; chunks of 10 give the same samples; the property encoder saw ONE row."""
    from spmm_amd import decode
    m = peaky
    g = torch.Generator().manual_seed(31)
    pv = torch.randn(53, generator=g) * 2
    mask = torch.zeros(53)
    mask[torch.randperm(53, generator=g)[:33]] = 1
    n, k, T, seed = 24, 2, 16, 5
    seen = []
    real = decode.encode_properties

    def spy(model, prop, prop_mask=None):
        seen.append(tuple(prop.shape))
        return real(model, prop, prop_mask)

    monkeypatch.setattr(decode, "encode_properties", spy)
    got = decode.generate_with_property(m, pv, n, mask, k=k, stochastic=True, seed=seed, max_steps=T)
    assert seen == [(1, 53)]
    assert decode.last_generate["samples"] == n and decode.last_generate["chunks"] == 1
    chunked = decode.generate_with_property(m, pv, n, mask, k=k, stochastic=True, seed=seed, max_steps=T, chunk=10)
    assert seen == [(1, 53), (1, 53)] and decode.last_generate["chunks"] == 3
    monkeypatch.undo()
    assert len(got) == n and chunked == got
    ref = decode.beam_search_batched(m, pv.repeat(n, 1), k=k, max_steps=T, prop_mask=mask, stochastic=True, seed=seed)
    rng = random.Random(seed)
    want = [finals[rng.randrange(len(finals))][1] if finals else [] for finals in ref]
    assert got == want
    assert decode.last_generate["no_final"] == sum(1 for s in got if not s)
    assert sum(1 for s in got if s) >= n // 2 and len({tuple(s) for s in got if s}) > 1
    for s in got:
        assert not s or (s[0] == decode.CLS_ID and s[-1] == decode.SEP_ID)
    # deterministic: every sample is the best final of the one beam search
    det = decode.generate_with_property(m, pv, 3, mask, k=k, stochastic=False, max_steps=T)
    best = decode.beam_search_batched(m, pv.reshape(1, -1), k=k, max_steps=T, prop_mask=mask)[0]
    assert det == [best[0][1] if best else []] * 3


def test_generation_driver_is_reproducible(tmp_path):
    """pv2smiles.py --synthetic --tiny --n_generate 8 --seed 1 in a fresh process, twice: 8 lines, the same 8 lines."""
    outs = []
    for i in range(2):
        out = tmp_path / f"gen{i}.txt"
        cmd = [sys.executable, os.path.join(ROOT, "pv2smiles.py"), "--synthetic", "--tiny", "--n_generate", "8", "--seed", "1", "--output", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "samples: 8" in r.stdout and "without a final hypothesis:" in r.stdout and "uniqueness" in r.stdout
        lines = out.read_text().split("\n")
        assert lines[-1] == "" and len(lines) == 9
        outs.append(lines[:-1])
    assert outs[0] == outs[1] and any(outs[0])
