"""spmm_sbs_step (csrc/sbs.hip) on the GPU against the float64 restatement tests/sbs_reference.py: one step on mixed states, ties, group
independence, nesting over six positions, and the sampling statistics of the toy model.

Selection against float64.  DELTA is 4 x the largest |kernel key - reference key| measured over CASES x POSITIONS below on an MI355X
(5.578e-6): every candidate whose reference key is above tau + DELTA must be selected and none below tau - DELTA,
tau = the reference's W-th key.  The seeds of CASES were picked on the CPU so that the float64 reference has at most 2 candidates inside
[tau - DELTA, tau + DELTA] per group; that is asserted on the reference before the kernel's output is looked at.  If DELTA moves, pick
new seeds (tests/sbs_reference.py and `band_count` below are all it takes); do not widen the cap."""
import numpy as np
import pytest
import torch

import sbs_reference as R

pytestmark = pytest.mark.gpu

DELTA = R.DELTA
BAND_CAP = 2
LMAX = 256
CASES = {                       # (G, W, V, pad of ldl / ldn): seed per position
    "1x1x4": ((1, 1, 4, 0), {0: 1, 1: 2, LMAX - 2: 11}),            # (the one slot: live at t = 1, finished at t = 254)
    "3x8x300": ((3, 8, 300, 0), {0: 1, 1: 2, LMAX - 2: 3}),
    "5x24x37 padded": ((5, 24, 37, 11), {0: 1, 1: 2, LMAX - 2: 3}),
    "2x64x300": ((2, 64, 300, 0), {0: 1, 1: 2, LMAX - 2: 3}),
    "1x1024x512": ((1, 1024, 512, 0), {0: 1, 1: 2, LMAX - 2: 3}),
}
POSITIONS = (0, 1, LMAX - 2)


def make_case(G, W, V, t, seed, L=LMAX, own_group_anc=False):
    """fp32 inputs and a state that mixes live, finished and empty slots, rows with -inf and -1e30 entries and (W > 1, t > 0) a live row
    with nothing allowed; t = 0: slot 0 alone.  |phi|, |gum| <= 64."""
    rs = np.random.RandomState(seed)
    logits = (rs.randn(G, W, V) * 3).astype(np.float32)
    logits[rs.rand(G, W, V) < 0.1] = -np.inf
    logits[rs.rand(G, W, V) < 0.1] = R.MASKED
    noise = rs.gumbel(size=(G, W, V)).astype(np.float32)
    state, _ = R.start_state(G, W, L)
    state["tokens"][:] = 0
    state["len"][:] = 0
    if t == 0:
        return logits, noise, state
    kind = rs.rand(G, W)
    empty, fin = kind < 0.15, (kind >= 0.15) & (kind < 0.4)
    if W > 1:
        empty[:, -1] = fin[:, -1] = False
        logits[:, -1, :] = R.MASKED
        logits[:, -1, ::2] = -np.inf
    phi = (-rs.rand(G, W) * 40).astype(np.float32)
    gum = np.clip(phi + rs.gumbel(size=(G, W)), -64, 0).astype(np.float32)
    state["phi"] = np.where(empty, R.NEG, phi).astype(np.float64)
    state["gum"] = np.where(empty, R.NEG, gum).astype(np.float64)
    state["fin"] = fin
    lo = min(4, V - 1)
    tok = rs.randint(lo, V, size=(G, W, L))
    tok[:, :, 0] = R.CLS
    ln = np.where(fin, rs.randint(1, t + 1, size=(G, W)), t)
    pos = np.arange(L)[None, None, :]
    tok = np.where(pos < ln[:, :, None], tok, 0)
    tok = np.where(fin[:, :, None] & (pos == ln[:, :, None] - 1), R.SEP, tok)
    state["tokens"] = np.where(empty[:, :, None], 0, tok)
    state["len"] = np.where(empty, 0, ln)
    rows = np.arange(G * W)
    if own_group_anc:
        anc = (rows // W * W)[:, None] + rs.randint(0, W, size=(G * W, L))
    else:
        anc = rs.randint(0, G * W, size=(G * W, L))
        anc[rs.rand(G * W, L) < 0.02] = G * W + 5                         # clamped by the kernel
        anc[rs.rand(G * W, L) < 0.02] = -3
    state["anc"] = np.where(pos[0] < t, anc, rows[:, None])
    return logits, noise, state


def run_kernel(logits, noise, state, t, pad=0, L=None):
    """The launch through ops.sbs_step on a DistinctBook -> the next state as numpy (the fields of sbs_reference.new_state_ref)."""
    from spmm_amd import decode, ops
    G, W, V = logits.shape
    L = state["tokens"].shape[-1] if L is None else L
    book = decode.DistinctBook(G, W, L - 3, "cuda", fused=True)
    assert book.Lmax == L
    c = book.cur
    c["phi"].copy_(torch.from_numpy(np.asarray(state["phi"], dtype=np.float32)))
    c["gum"].copy_(torch.from_numpy(np.asarray(state["gum"], dtype=np.float32)))
    c["fin"].copy_(torch.from_numpy(np.asarray(state["fin"]).astype(np.uint8)))
    c["len"].copy_(torch.from_numpy(np.asarray(state["len"]).astype(np.int32)))
    c["tokens"].copy_(torch.from_numpy(np.asarray(state["tokens"]).astype(np.int32)))
    c["anc"].copy_(torch.from_numpy(np.asarray(state["anc"]).astype(np.int32)))
    lg = torch.full((G * W, V + pad), float("nan"), dtype=torch.float32, device="cuda")
    nz = torch.full((G * W, V + pad), float("nan"), dtype=torch.float32, device="cuda")
    lg[:, :V] = torch.from_numpy(logits.reshape(G * W, V))
    nz[:, :V] = torch.from_numpy(noise.reshape(G * W, V))
    parent = torch.full((G * W,), -7, dtype=torch.int32, device="cuda")
    ids = ops.sbs_step(lg[:, :V], nz[:, :V], book, t=t, parent_out=parent)
    torch.cuda.synchronize()
    n = book.nxt
    out = {f: n[f].cpu().numpy() for f in ("phi", "gum", "len", "tokens", "anc")}
    out.update(fin=n["fin"].cpu().numpy().astype(bool), ids=ids.cpu().numpy(), parent=parent.cpu().numpy().reshape(G, W), open=book.open.cpu().numpy())
    have = out["gum"] > R.NEG
    tok_at = np.take_along_axis(out["tokens"], np.full((G, W, 1), t), axis=2)[:, :, 0]
    pfin = np.take_along_axis(np.asarray(state["fin"]).astype(bool), out["parent"].astype(np.int64), axis=1)
    out["tok"] = np.where(have, np.where(pfin, R.SEP, tok_at), 0)          # the token of the candidate: [SEP] for a finished slot's own
    return out


def band_count(ref_key, W, delta=DELTA):
    """Per group: tau (the reference's W-th key, -inf when there are fewer finite candidates) and the candidates inside [tau - delta, tau + delta]."""
    srt = -np.sort(-ref_key, axis=1)
    tau = srt[:, min(W, srt.shape[1]) - 1]
    fin = np.isfinite(tau)
    inside = (np.abs(ref_key - np.where(fin, tau, 0)[:, None]) <= delta) & fin[:, None]
    return tau, inside.sum(1)


def check_step(logits, noise, state, t, pad=0, name=""):
    """All checks of one launch -> largest |kernel key - reference key| over the selected candidates."""
    G, W, V = logits.shape
    ref = R.step_ref(logits.astype(np.float64), noise.astype(np.float64), state, t)
    tau, inside = band_count(ref["key"], W)
    assert inside.max() <= BAND_CAP, f"{name}: {inside.max()} reference candidates within DELTA of tau: pick another seed"
    got = run_kernel(logits, noise, state, t, pad)
    have = got["gum"] > R.NEG
    n_ref = np.isfinite(ref["key"]).sum(1)
    assert np.array_equal(have.sum(1), np.minimum(n_ref, W)), (have.sum(1), n_ref)
    assert all(have[g, : have[g].sum()].all() for g in range(G))                           # the empty slots are the trailing ones
    flat = got["parent"].astype(np.int64) * V + got["tok"]
    worst = 0.0
    for g in range(G):
        k = int(have[g].sum())
        keys = got["gum"][g, :k]
        assert np.all(np.diff(keys) <= 0), f"{name}: keys of group {g} increase"
        assert len(set(flat[g, :k].tolist())) == k, f"{name}: a (parent, token) pair twice in group {g}"
        rk = ref["key"][g, flat[g, :k]]
        assert np.all(np.isfinite(rk)), f"{name}: group {g} selected something that is no candidate"
        worst = max(worst, float(np.max(np.abs(keys.astype(np.float64) - rk))) if k else 0.0)
        sel = np.zeros(W * V, dtype=bool)
        sel[flat[g, :k]] = True
        if np.isfinite(tau[g]):
            assert sel[ref["key"][g] > tau[g] + DELTA].all(), f"{name}: group {g} misses a candidate above tau + DELTA"
            assert not sel[ref["key"][g] < tau[g] - DELTA].any(), f"{name}: group {g} selected a candidate below tau - DELTA"
        else:
            assert np.array_equal(sel, np.isfinite(ref["key"][g]))
        # equal keys in flat-index order
        same = np.diff(keys) == 0
        assert np.all(np.diff(flat[g, :k])[same] > 0), f"{name}: equal keys of group {g} not in flat-index order"
        # the arg-max child of a live parent carries the parent's key bit for bit
        T32 = np.asarray(state["gum"], dtype=np.float32)[g]
        par = got["parent"][g, :k]
        argmax_child = (rk == np.asarray(state["gum"])[g, par]) & ~np.asarray(state["fin"]).astype(bool)[g, par]
        assert np.array_equal(keys[argmax_child].view(np.uint32), T32[par][argmax_child].view(np.uint32)), f"{name}: arg-max child key != parent key"
    # everything else is an exact function of the kernel's own (parent, token)
    key64, cphi = R.candidates_ref(logits.astype(np.float64), noise.astype(np.float64), state["phi"], state["gum"], state["fin"])
    want = R.new_state_ref(flat, got["gum"].astype(np.float64), have, cphi, state["phi"], state["fin"], state["len"], state["tokens"], state["anc"], t, V)
    for f in ("fin", "len", "tokens", "anc", "ids", "open"):
        assert np.array_equal(np.asarray(got[f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)), f"{name}: {f}"
    assert np.array_equal(got["parent"][~have], np.broadcast_to(np.arange(W), (G, W))[~have])
    assert np.all(got["phi"][~have] == R.NEG)
    dphi = float(np.max(np.abs(got["phi"][have].astype(np.float64) - want["phi"][have]))) if have.any() else 0.0
    print(f"[sbs] {name} t={t}: selected {int(have.sum())}, max |key - ref| = {worst:.3e}, max |phi - ref| = {dphi:.3e}, band {inside.tolist()[:8]}")
    assert dphi <= DELTA and worst <= DELTA
    return worst


@pytest.mark.parametrize("t", POSITIONS)
@pytest.mark.parametrize("case", list(CASES))
def test_one_step_against_float64(case, t):
    (G, W, V, pad), seeds = CASES[case]
    logits, noise, state = make_case(G, W, V, t, seeds[t])
    check_step(logits, noise, state, t, pad, case)


def _kernel_step(logits, noise, state, t):
    return run_kernel(np.asarray(logits, dtype=np.float32), np.asarray(noise, dtype=np.float32), state, t)


def test_ties_go_to_the_lower_slot_and_missing_candidates_leave_empty_slots():
    R.check_tie_order(_kernel_step)


def test_a_group_alone_gives_what_it_gives_among_others():
    G, W, V, t = 3, 8, 300, 5
    logits, noise, state = make_case(G, W, V, t, 21, own_group_anc=True)
    full = run_kernel(logits, noise, state, t)
    for g in range(G):
        one = {f: (np.asarray(v)[g:g + 1] if f != "anc" else np.asarray(v)[g * W:(g + 1) * W] - g * W) for f, v in state.items()}
        alone = run_kernel(logits[g:g + 1], noise[g:g + 1], one, t)
        for f in ("phi", "gum", "fin", "len", "tokens", "parent", "open"):
            assert np.array_equal(np.asarray(full[f])[g:g + 1].view(np.uint8), np.asarray(alone[f]).view(np.uint8)), (g, f)
        assert np.array_equal(full["anc"][g * W:(g + 1) * W] - g * W, alone["anc"]) and np.array_equal(full["ids"][g * W:(g + 1) * W], alone["ids"])


def _device_search(table, W, G, steps, seed, V, L, forced_sep_at=None):
    """The search on the device with table-lookup logits: logits of a row = table[min(t - 1, len - 1)][last token], tokens 0-2 masked."""
    from spmm_amd import decode, ops
    book = decode.DistinctBook(G, W, L - 3, "cuda", fused=True)
    R8 = (W + 7) // 8
    seed_dev = torch.tensor([seed], dtype=torch.int64, device="cuda")
    mol = (torch.arange(G)[:, None] * 128 + torch.arange(R8)[None, :]).reshape(-1).to(torch.int32).cuda()
    tab = torch.from_numpy(table.astype(np.float32)).cuda()
    for _ in range(steps):
        t = book.t
        last = book.tokens[:, t - 1].long() % V
        logits = tab[min(t - 1, tab.shape[0] - 1)][last].clone()
        logits[:, :R.SEP] = R.MASKED
        if forced_sep_at is not None and t - 1 >= forced_sep_at:
            logits[:, R.SEP + 1:] = R.MASKED
        noise = ops.gumbel_noise(seed_dev, G * R8, 8, V, L, salt=decode.DISTINCT_SALT, t=t - 1, mol=mol)
        noise = noise.view(G, R8 * 8, V)[:, :W].reshape(G * W, V).contiguous()
        book.step_fused(logits, noise)
    return book


def test_the_first_8_slots_of_32_are_the_8_slot_search_bit_for_bit():
    """Six positions, history-dependent logits, the project's counter noise: nesting at kernel level."""
    V, L, G = 37, 12, 3
    table = np.random.RandomState(8).randn(6, V, V) * 2.0
    a, b = _device_search(table, 8, G, 6, 17, V, L), _device_search(table, 32, G, 6, 17, V, L)
    for f in ("tokens", "phi", "gum", "fin", "len"):
        x, y = a.cur[f].cpu().numpy(), b.cur[f][:, :8].cpu().numpy()
        assert np.array_equal(x.view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), f
    assert (a.cur["gum"] > -float("inf")).all() and int(a.cur["fin"].sum()) >= 1
    toks = a.cur["tokens"].cpu().numpy()
    assert all(len({tuple(r) for r in toks[g]}) == 8 for g in range(G))


def test_the_device_search_samples_the_toy_model_without_replacement():
    """4 096 independent groups at W = 2, four positions: first-slot and inclusion frequencies within 5 sigma of the exact probabilities."""
    n = 4096
    book = _device_search(R.TAB, 2, n, R.TOY_STEPS, 11, R.TOY_V, R.TOY_L, forced_sep_at=3)
    c = book.cur
    state = dict(gum=c["gum"].cpu().numpy(), fin=c["fin"].cpu().numpy().astype(bool), len=c["len"].cpu().numpy(), tokens=c["tokens"].cpu().numpy())
    seqs = R.sequences(state)
    assert all(len(s) == 2 and s[0] != s[1] for s in seqs)
    d1, d2 = R.toy_statistics([s[0] for s in seqs], seqs)
    print(f"[sbs] device, {n} groups at W = 2: first slot {d1:.2f} sigma, inclusion {d2:.2f} sigma")
    assert d1 <= R.SIGMA_BOUND and d2 <= R.SIGMA_BOUND
    ref = R.search_ref(R.toy_model, R.toy_noise(11), n, 2, R.TOY_STEPS, R.TOY_L)
    same = sum(a == b for a, b in zip(seqs, R.sequences(ref)))
    print(f"[sbs] device against the float64 search on the same noise: {same} / {n} groups identical")
    assert same >= 0.99 * n
