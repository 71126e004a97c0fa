"""Guided and truncated PV -> SMILES decoding on the GPU: GuidedDecoder (both conditions as two halves of one set of launches, the mirror
ancestry, ops.logit_warp) against the whole-prefix forwards of its two conditions, against the plain searches it must reduce to, against
its tensor-op twin, and through generate_with_property and the driver.  Tiny configuration with the closed-form weights and the peaky
LM-head bias of tests/test_prefix_decode_gpu.py, V = 300."""
import os
import subprocess
import sys

import pytest
import torch

import warp_reference as WR
from prefix_reference import peaky_lm, prefixes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mk(SPMM, cfg, sd):
    m = SPMM(config=None, spmm_config=cfg)
    m.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    return m.eval()


@pytest.fixture(scope="module")
def peaky(env):
    O, SPMM, tiny_config, *_ = env
    return _mk(SPMM, tiny_config(), peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), sep_gap=0.4))


@pytest.fixture(scope="module")
def compacting(env):
    """Model and PVs of test_seeded_prompted_search_with_compaction_equals_the_whole_batch: molecules finish at different positions."""
    O, SPMM, tiny_config, *_ = env
    m = _mk(SPMM, tiny_config(), peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), seed=5, sep_gap=0.9))
    return m, torch.randn(32, 53, generator=torch.Generator().manual_seed(12)) * 10.0


def _toks(res):
    return [[h[1] for h in mol] for mol in res]


def _same_search(a, b, tol=1e-4):
    assert _toks(a) == _toks(b) and any(_toks(a))
    for x, y in zip(a, b):
        for (px, _), (py, _) in zip(x, y):
            assert abs(px - py) < tol, (px, py)


def _lsm(x):
    return torch.log_softmax(x.float(), -1)


def test_both_halves_follow_their_own_condition(peaky):
    """GuidedDecoder.step, N = 3, k = 4, guidance 1 and no truncation: the warped output is the conditioned half (to the rounding of
    lu + (lc - lu)), and through 6 positions of random tokens and random reorders both halves of the raw logits stay within 3e-2 (log
    softmax) of the whole-prefix forward of their own condition -- before and after a compaction that drops the middle molecule."""
    from spmm_amd import decode
    m, N, k, T = peaky, 3, 4, 6
    g = torch.Generator().manual_seed(21)
    props = torch.randn(N, 53, generator=g)
    pe, pe_u = decode.encode_properties(m, props), decode.encode_properties(m, props, torch.ones(53))
    base = decode._baseline_embeds(m, props[:1])
    assert base.shape == pe_u[:1].shape and (base.float() - pe_u.float()).abs().max().item() < 2e-2     # all-masked: the same encoding for every PV
    dec = decode.GuidedDecoder(m, pe, k, T + 6, base_embeds=base, guidance=1.0)
    assert dec.R == 2 * N * k and dec.R0 == N * k and dec.warp_info["baseline_rows"] == N * k
    for l, once in dec.xkv_once.items():                                   # projected once: N conditions + the baseline, which is never copied
        Lp = pe.shape[1]
        assert once.shape[0] == (N + 1) * Lp and dec.xkv[l].shape[0] == N * Lp and dec.xkv_base[l].shape[0] == Lp
        assert dec.xkv_base[l].data_ptr() == once[N * Lp:].data_ptr()
    full_c, full_u = decode.RecomputeDecoder(m, pe, k, T + 6), decode.RecomputeDecoder(m, pe_u, k, T + 6)
    raw = {}
    inner = decode.CachedDecoder._forward                                  # the step up to the raw logits of all 2R rows

    def spy(self, ids, t, t_dev=None):
        raw["logits"] = inner(self, ids, t, t_dev).clone()
        return raw["logits"].clone()

    worst = 0.0
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(decode.CachedDecoder, "_forward", spy)
        R, live = N * k, list(range(N))
        for t in range(T):
            if t == 3:                                                       # drop the middle molecule from all three decoders
                keep = torch.tensor([0, 2]).cuda()
                dec.compact(keep)
                rows = torch.cat([torch.arange(0, k), torch.arange(2 * k, 3 * k)])
                for f in (full_c, full_u):
                    f.kv, f.tok = f.kv[rows.cuda()], f.tok[rows.cuda()]
                R, live = 2 * k, [0, 2]
                anc, rowmap = dec.search_tables()
                assert anc.shape[0] == R and rowmap.tolist() == rows.tolist()
                assert dec.rowmap[R:].tolist() == (rows + N * k).tolist()
            ids = torch.randint(4, 300, (R,), generator=g).cuda()
            out = dec.step(ids, t)
            assert out.shape == (R, 300) and raw["logits"].shape == (2 * R, 300)
            lc, lu = raw["logits"][:R], raw["logits"][R:]
            bound = WR.value_bound(lc.cpu(), lu.cpu(), 1.0, 1.0).cuda()
            assert bool(((out.double() - lc.double()).abs() <= bound).all())
            assert bool((dec.anc[R:] == dec.anc[:R] + N * k).all())          # the mirror the step refreshed
            worst = max(worst, (_lsm(lc) - _lsm(full_c.step(ids, t))).abs().max().item(), (_lsm(lu) - _lsm(full_u.step(ids, t))).abs().max().item())
            assert worst < 3e-2, (t, worst)
            # what the beam step does to the search's half: a random reorder of rows [0, R) only
            parent = torch.randint(0, k, (len(live), k), generator=g).cuda()
            anc, _ = dec.search_tables()
            L = anc.shape[1]
            own = (dec.rows[:R] if dec.rowmap is None else dec.rowmap[:R])
            new = anc.view(len(live), k, L).gather(1, parent[:, :, None].expand(len(live), k, L)).reshape(R, L)
            anc.copy_(torch.where(dec.cols >= t + 1, own[:, None], new))
            full_c.reorder(parent, t + 1)
            full_u.reorder(parent, t + 1)
    print(f"guided decoder: worst |d log p| of either half over {T} positions, one compaction: {worst:.4f}")


@pytest.fixture(scope="module")
def compacting_runs(compacting):
    """The seeded sampled searches of the 32 molecules, computed once: conditioned, all-masked (both plain), and what compaction did."""
    from spmm_amd import decode
    m, props = compacting
    kw = dict(k=2, max_steps=40, stochastic=True, seed=7)
    cond = decode.beam_search_batched(m, props, **kw)
    run = dict(decode.last_run)
    masked = decode.beam_search_batched(m, props, prop_mask=torch.ones(53), **kw)
    return kw, cond, masked, run


def test_guidance_zero_is_the_all_masked_search(compacting, compacting_runs):
    """w = 0 leaves the baseline half's logits: the guided search must be the plain search with prop_mask = ones, token for token, scores to
    1e-4 (what the project allows between a compacted and a whole batch) -- through at least one compaction, which a wrong mirror, offset
    or row map of the baseline half does not survive."""
    from spmm_amd import decode
    m, props = compacting
    kw, _, masked, _ = compacting_runs
    got = decode.beam_search_batched(m, props, guidance=0.0, **kw)
    run = dict(decode.last_run)
    print(f"guidance 0, seeded, N = 32, k = 2: {run}")
    assert run["compactions"] >= 1 and run["final_batch"] < 32 and run["baseline_rows"] == 64 and run["guidance"] == 0.0
    _same_search(got, masked)


def test_a_guided_decoder_at_weight_one_is_the_conditioned_search(compacting, compacting_runs):
    """GuidedDecoder forced with w = 1 (the public functions never build the baseline for it): lu + (lc - lu) is lc to the last bits."""
    from spmm_amd import decode
    m, props = compacting
    kw, cond, _, plain_run = compacting_runs
    pe = decode.encode_properties(m, props)
    dec = decode.GuidedDecoder(m, pe, 2, 1 + 40 + 2, base_embeds=decode._baseline_embeds(m, props[:1]), guidance=1.0)
    got = decode._search(m, dec, 32, k=2, max_steps=40, stochastic=True, seed=7)
    run = dict(decode.last_run)
    assert run["compactions"] >= 1 and run["compactions"] == plain_run["compactions"] and run["baseline_rows"] == 64
    _same_search(got, cond)


@pytest.fixture(scope="module")
def twelve(env):
    O, SPMM, tiny_config, *_ = env
    sd = peaky_lm(O.closed_form_state_dict(O.tiny_cfg()), seed=11, sep_gap=0.5)
    return _mk(SPMM, tiny_config(), sd), torch.randn(12, 53, generator=torch.Generator().manual_seed(12)) * 2, prefixes(12, 5, seed=35)


@pytest.mark.parametrize("prompted", [False, True])
def test_the_fused_and_the_tensor_op_route_agree(twelve, monkeypatch, prompted):
    """guidance 2, temperature 0.8, top_p 0.9, seeded, N = 12, k = 3, 12 positions: the kernel route and the warp_logits route (tensor-op
    bookkeeping) agree as test_prefill_and_stepping_give_the_same_search requires of two routes -- identical hypotheses for at least
    0.9 N molecules, scores within 1e-4 where the tokens agree -- from [CLS] and from a 5-token prefix per molecule (prefill)."""
    from spmm_amd import decode, ops
    m, props, pre = twelve
    kw = dict(k=3, max_steps=12, stochastic=True, seed=9, guidance=2.0, temperature=0.8, top_p=0.9, prefix=pre if prompted else None)
    calls = []
    inner = ops.logit_warp
    monkeypatch.setattr(ops, "logit_warp", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    fused = decode.beam_search_batched(m, props, **kw)
    n_fused = len(calls)
    assert n_fused >= 2 and decode.last_run["baseline_rows"] == 36 and decode.last_run["prefill"] == prompted
    monkeypatch.setattr(decode, "FUSED_BEAM_STEP", False)
    plain = decode.beam_search_batched(m, props, **kw)
    assert len(calls) == n_fused                                             # the tensor-op route never launches the kernel
    same, worst = 0, 0.0
    for ha, hb in zip(fused, plain):
        same += int(bool(ha) and _toks([ha]) == _toks([hb]))
        for (pa, sa), (pb, sb) in zip(ha, hb):
            if sa == sb:
                worst = max(worst, abs(pa - pb))
    print(f"guided search, fused vs tensor-op route (prefix: {prompted}): identical for {same} / 12, worst score difference {worst:.2e}")
    assert same >= 0.9 * 12 and worst < 1e-4
    if prompted:
        assert all(s[:5] == pre[n].tolist() for n, mol in enumerate(fused) for _, s in mol)


def test_guided_generation_does_not_depend_on_the_chunking(peaky, monkeypatch):
    from spmm_amd import decode, ops
    m = peaky
    pv = torch.randn(53, generator=torch.Generator().manual_seed(31)) * 2
    kw = dict(k=2, max_steps=16, guidance=2.0, top_k=20)
    got = decode.generate_with_property(m, pv, 24, seed=3, **kw)
    assert decode.last_generate["chunks"] == 1 and decode.last_generate["baseline_rows"] == 48 and decode.last_generate["guidance"] == 2.0
    assert decode.last_generate["top_k"] == 20
    for chunk, chunks, rows in ((7, 4, 6), (1, 24, 2)):
        assert decode.generate_with_property(m, pv, 24, seed=3, chunk=chunk, **kw) == got
        assert decode.last_generate["chunks"] == chunks and decode.last_generate["baseline_rows"] == rows
    assert decode.generate_with_property(m, pv, 24, seed=4, **kw) != got
    done = [s for s in got if s]
    assert len(done) >= 12 and len({tuple(s) for s in done}) > 1 and all(s[-1] == decode.SEP_ID for s in done)
    # the defaults, spelled out: the call without them, and the kernel is never launched
    plain = decode.generate_with_property(m, pv, 24, k=2, seed=3, max_steps=16)
    assert plain != got

    def boom(*a, **k):
        raise AssertionError("ops.logit_warp called at the defaults")

    monkeypatch.setattr(ops, "logit_warp", boom)
    monkeypatch.setattr(decode.GuidedDecoder, "__init__", boom)
    assert decode.generate_with_property(m, pv, 24, k=2, seed=3, max_steps=16, guidance=1.0, temperature=1.0, top_k=0, top_p=1.0) == plain
    assert decode.last_generate["baseline_rows"] == 0 and decode.last_generate["guidance"] == 1.0
    props = pv[None].repeat(3, 1)
    a = decode.beam_search_batched(m, props, k=3, max_steps=10)
    assert decode.beam_search_batched(m, props, k=3, max_steps=10, guidance=1.0, temperature=1.0, top_k=0, top_p=1.0) == a


def test_truncation_alone_builds_no_baseline(peaky, monkeypatch):
    """guidance = 1 with a truncation: one half, the kernel with lu = null; top_k = k on the deterministic search keeps its choices."""
    from spmm_amd import decode, ops
    m = peaky
    props = torch.randn(5, 53, generator=torch.Generator().manual_seed(4)) * 2
    seen = []
    inner = ops.logit_warp
    monkeypatch.setattr(ops, "logit_warp", lambda lc, lu=None, **k: (seen.append((lc.shape[0], lu is None)), inner(lc, lu, **k))[1])
    decode.beam_search_batched(m, props, k=3, max_steps=6, stochastic=True, seed=2, temperature=0.7, top_p=0.8)
    assert decode.last_run["baseline_rows"] == 0 and decode.last_run["temperature"] == 0.7
    assert seen and all(rows == 15 and no_lu for rows, no_lu in seen)
    with pytest.raises(ValueError, match="top_k=2 is below the k=3"):
        decode.beam_search_batched(m, props, k=3, max_steps=6, top_k=2)
    with pytest.raises(ValueError, match="reaction prediction"):
        decode.GuidedDecoder(m, None, 3, 12, memory=dict(N=1, Lmax=4, xkv={}), guidance=2.0)


def _driver(tmp_path, name, *flags):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pv2smiles.py"), "--synthetic", "--tiny", "--n_generate", "8", "--seed", "1",
                        "--output", str(out), *flags], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return out.read_text(), r.stdout


def test_the_driver_takes_the_sampling_flags(tmp_path):
    flags = ("--guidance", "2", "--temperature", "0.8", "--top_p", "0.9")
    a, stdout = _driver(tmp_path, "a.txt", *flags)
    assert "sampling: guidance 2, temperature 0.8, top_k 0, top_p 0.9" in stdout
    b, _ = _driver(tmp_path, "b.txt", *flags)
    plain, stdout = _driver(tmp_path, "plain.txt")
    assert "sampling:" not in stdout
    spelled, _ = _driver(tmp_path, "spelled.txt", "--guidance", "1", "--temperature", "1", "--top_k", "0", "--top_p", "1")
    assert a == b and len(a.splitlines()) == 8
    assert a != plain
    assert spelled == plain
