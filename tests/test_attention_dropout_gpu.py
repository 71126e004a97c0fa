"""Attention dropout in every layout the training step launches (engine.py::_self_attn_fwd, _xattn_* and their backwards): packed rows,
shared key/value sources, causal and non-causal sequences in one launch, key masks, the Lq = 1 queries of engine.SelfKV, the 256-key
kernels and the chunked path beyond 256 tokens.  csrc/attention.hip generates the mask in three separately written places (forward,
<= 128-key backward, 256-key backward) and each backward applies it twice (dP and P~); two layers pin them:

  * probes (Q = 0) read the mask each path applied, decision by decision: all of them must equal the host model of the hash on every
    visible (query, key) pair -- no mismatch tolerated;
  * with random data, O, dQ, dK, dV stay within 2 x the error of the bf16 storage model of the same formulas from the float64
    reference, per (sequence, head) block (helpers_gpu.py::attention_ref64, check_attention_parity).

tests/test_attention_reference_cpu.py shows on the CPU that both layers can fail."""
import pytest
import torch

from helpers_gpu import (attention_dropout_case, attention_keep_mask, attention_layout_kw, attention_ref64, attn_heads, attn_visible,
                         check_attention_parity, probe_dq_mismatches, probe_fwd_mask, probe_masks)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SINGLE = ["a", "b", "c", "d", "e", "f1", "f2", "h"]         # one launch each; g runs two launches, i the chunked path


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops as o
    return o


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def close(got, ref, atol, rtol, name=""):
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.numel()} off; max err {err.max().item():.4g}"


def _launch(ops, c, Q, K, V, dO, bwd=True, seed=None):
    """Case c through ops.attn_fwd_long / attn_bwd_long (the step's entry points) on CPU inputs in the launch's layout, Q | K | V and their
    gradients inside fused buffers as in the engine (row strides).  -> O, lse, dQ, dK, dV in the canonical form of helpers_gpu.py."""
    nseq, nH, Lq, Lkv = c["nseq"], c["nH"], c["Lq"], c["Lkv"]
    H = nH * 64
    dev = lambda x, dt=torch.int32: None if x is None else torch.as_tensor(x).to(dt).cuda()
    kw = dict(nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, kmask=dev(c["kmask"]), causal_from=c["causal_from"], is_cross=c["is_cross"],
              dropout_p=c["p"], seed=torch.tensor([c["seed"] if seed is None else seed], dtype=torch.int64, device="cuda"), salt=c["salt"],
              kv_seq=dev(c["kv_seq"]), q_row0=dev(c["q_row0"]), q_len=dev(c["q_len"]), kv_row0=dev(c["kv_row0"]), kv_len=dev(c["kv_len"]))
    qb = torch.cat([Q, dO], dim=1).to(BF).cuda()
    kvb = torch.cat([K, V], dim=1).to(BF).cuda()
    Qg, dOg, Kg, Vg = qb[:, :H], qb[:, H:], kvb[:, :H], kvb[:, H:]
    O = torch.zeros(c["q_rows"], H, dtype=BF, device="cuda")
    lse = torch.zeros(nseq, nH, Lq, device="cuda")
    ops.attn_fwd_long(Qg, Kg, Vg, O, lse, **kw)
    dkv_n = nseq if c["kv_seq"] is not None else c["nsrc"]
    dQ = torch.zeros(c["q_rows"], H, dtype=BF, device="cuda")
    dKV = torch.zeros(nseq * Lkv if c["kv_seq"] is not None else c["kv_rows"], 2 * H, dtype=BF, device="cuda")
    if bwd:
        ops.attn_bwd_long(Qg, Kg, Vg, O, lse, dOg, dQ, dKV[:, :H], dKV[:, H:], **kw)
    kv_lay = (None, None) if c["kv_seq"] is not None else (c["kv_row0"], c["kv_len"])     # shared sources: dense per query sequence
    if c["kv_seq"] is not None and c["kv_len"] is not None:                               # (rows past the source's length stay unwritten)
        kv_lay = (None, [c["kv_len"][u] for u in c["kv_seq"]])
    out = (attn_heads(O, nseq, Lq, nH, c["q_row0"], c["q_len"]), lse.cpu().double(), attn_heads(dQ, nseq, Lq, nH, c["q_row0"], c["q_len"]),
           attn_heads(dKV[:, :H], dkv_n, Lkv, nH, *kv_lay), attn_heads(dKV[:, H:], dkv_n, Lkv, nH, *kv_lay))
    return out, dKV


def _probe(ops, c, seed=None):
    def run(Q, K, V, dO, bwd):
        (O, _, dQ, dK, dV), _ = _launch(ops, c, Q, K, V, dO, bwd=bwd, seed=seed)
        return O, dQ, dK, dV
    return probe_masks(run, c)


def _check_probes(c, probes, want, vis):
    """All three recovered masks equal `want` on the visible pairs (and nothing but visible pairs ever shows); -> visible decisions."""
    fw, dv, (dq, flat, spread) = probes
    n_vis = int(vis.sum()) * c["nH"]
    want = want & vis[:, None]
    bad = dict(forward=int((fw != want).sum()), Ptilde=int((dv != want).sum()), dP=probe_dq_mismatches(dq, flat, want, vis))
    print(f"[probe] {n_vis} visible decisions, mismatches {bad}, dP rows that no output can read {int(flat.sum())}, level spread {spread:.3f} delta")
    assert bad == dict(forward=0, Ptilde=0, dP=0), bad
    assert spread < 1 / 16, f"the dP probe's dQ is not two-valued per row: {spread} of the level distance"
    return n_vis


def _enough(c, vis):
    per_seq = vis.flatten(1).sum(-1) * c["nH"]
    assert (per_seq >= 1).all(), per_seq
    return int(per_seq.sum())


def _host_mask(c, seed=None):
    return attention_keep_mask(c["seed"] if seed is None else seed, c["salt"], c["nseq"], c["nH"], c["Lq"], c["Lkv"], c["p"])


def _inputs(c, seed):
    H = c["nH"] * 64
    return rnd(c["q_rows"], H, seed=seed).float(), rnd(c["kv_rows"], H, seed=seed + 1).float(), rnd(c["kv_rows"], H, seed=seed + 2).float(), \
        rnd(c["q_rows"], H, seed=seed + 3).float()


def _parity(ops, c, keep, tag):
    """Layer 3 of one launch; -> (kernel outputs, reference, model, the kernel's fused dK | dV buffer)."""
    x = _inputs(c, seed=70)
    kw = dict(attention_layout_kw(c), p=c["p"], keep=keep)
    ref, model = attention_ref64(*x, **kw), attention_ref64(*x, **kw, storage_model=True)
    got, dKV = _launch(ops, c, *x)
    valid = attn_visible(**attention_layout_kw(c)).any(-1)[:, None].expand(-1, c["nH"], -1)
    close(got[1][valid], ref[1][valid], 2e-3, 1e-4, "lse")
    for i, nm in ((0, "O"), (2, "dQ"), (3, "dK"), (4, "dV")):
        check_attention_parity(f"{tag} {nm}", got[i], ref[i], model[i])
    return got, ref, model, dKV


# ------------------------------------------------------------------------------------------- single launches (a-f, h)
@pytest.mark.parametrize("name", SINGLE)
def test_every_path_applies_the_mask_of_the_host_model(ops, name):
    c = attention_dropout_case(name)
    vis = attn_visible(**attention_layout_kw(c))
    assert _enough(c, vis) >= 1000
    _check_probes(c, _probe(ops, c), _host_mask(c), vis)


@pytest.mark.parametrize("name", SINGLE)
def test_outputs_and_gradients_with_dropout_on(ops, name):
    """O, lse, dQ, dK, dV of one launch against attention_ref64 with the host model's mask.  (Case b's one-token sequence: dQ and dK are
    exactly zero in the reference and in the storage model -- the softmax gradient over a single key -- so the bound of those two blocks is
    zero and asks the kernel for an exact zero as well.)"""
    c = attention_dropout_case(name)
    got, ref, model, dKV = _parity(ops, c, _host_mask(c), name)
    if name != "c":
        return
    # the step folds the per-query-sequence dK | dV onto the shared sources (fp32 sum, one bf16 rounding): against the float64 sum over sharers
    nseq, nH, Lkv, U = c["nseq"], c["nH"], c["Lkv"], c["nsrc"]
    W = Lkv * 2 * nH * 64
    idx = torch.tensor(c["kv_seq"])
    order = torch.sort(idx, stable=True).indices.to(torch.int32).cuda()
    start = torch.zeros(U + 1, dtype=torch.int32)
    start[1:] = torch.cumsum(torch.bincount(idx, minlength=U), 0)
    folded = ops.segment_sum_bf16(dKV.view(nseq, W), start.cuda(), order, torch.zeros(U, W, dtype=BF, device="cuda")).view(U * Lkv, -1)
    fold64 = lambda t: torch.zeros(U, *t.shape[1:], dtype=torch.float64).index_add_(0, idx, t)
    for i, nm, cols in ((3, "dK", slice(0, nH * 64)), (4, "dV", slice(nH * 64, 2 * nH * 64))):
        g = attn_heads(folded[:, cols], U, Lkv, nH, None, c["kv_len"])
        check_attention_parity(f"c folded {nm}", g, fold64(ref[i]), fold64(model[i]).float().to(BF).double())


# ------------------------------------------------------------------------------------------- engine.SelfKV (g)
def test_position0_queries_over_sequences_of_another_tensor(ops):
    """Lq = 1: the row counter is (seq * nH + h) * 1.  Two launches (54 and 200 keys: the <= 128-key and the 256-key backward); the case's
    1 000 visible decisions are counted over both, 12 rows of 54 keys cannot hold them."""
    total = 0
    for name in ("g54", "g200"):
        c = attention_dropout_case(name)
        vis = attn_visible(**attention_layout_kw(c))
        total += _enough(c, vis)
        _check_probes(c, _probe(ops, c), _host_mask(c), vis)
        _parity(ops, c, _host_mask(c), name)
    assert total >= 1000, total


# ------------------------------------------------------------------------------------------- the chunked path (i)
_long = {}


def _long_case(ops):
    """Case i and the mask its forward applied, recovered once (the chunk salt rule of ops.py is not restated here)."""
    if not _long:
        c = attention_dropout_case("i")
        _long.update(c=c, vis=attn_visible(**attention_layout_kw(c)), probes=_probe(ops, c))
    return _long["c"], _long["vis"], _long["probes"]


def test_chunked_path_backward_regenerates_the_forward_mask(ops):
    c, vis, probes = _long_case(ops)
    assert _enough(c, vis) >= 1000
    keep = probes[0]
    n = _check_probes(c, probes, keep, vis)
    pt = int(c["p"] * 65536 + 0.5) / 65536
    rate = 1 - int(keep.sum()) / n
    assert abs(rate - pt) < 4 * (pt * (1 - pt) / n) ** 0.5, (rate, pt, n)
    # every (query-chunk, key-chunk) pair draws a mask of its own: two pairs disagree like independent draws on their common extent
    ch = [(o, min(128, c["Lq"] - o)) for o in range(0, c["Lq"], 128)]
    pairs = [(q0, ql, k0, kl) for q0, ql in ch for k0, kl in ch]
    v4 = vis[:, None].expand_as(keep)
    for i, (q0, ql, k0, kl) in enumerate(pairs):
        for (r0, rl, s0, sl) in pairs[i + 1:]:
            nq, nk = min(ql, rl), min(kl, sl)
            both = v4[:, :, q0:q0 + nq, k0:k0 + nk] & v4[:, :, r0:r0 + nq, s0:s0 + nk]
            assert int(both.sum()) >= 1000
            differ = (keep[:, :, q0:q0 + nq, k0:k0 + nk] != keep[:, :, r0:r0 + nq, s0:s0 + nk]) & both
            share = int(differ.sum()) / int(both.sum())
            assert abs(share - 2 * pt * (1 - pt)) <= 0.03, ((q0, k0), (r0, s0), share)


def test_chunked_path_outputs_and_gradients_with_dropout_on(ops):
    c, vis, probes = _long_case(ops)
    _parity(ops, c, probes[0] | ~vis[:, None], "i")              # (invisible pairs have probability 0: their keep bit reaches nothing)


@pytest.mark.parametrize("name", ["a", "i"])
def test_a_second_seed_draws_another_mask(ops, name):
    """Two seeds disagree like independent draws: on a share 2 p (1 - p) of the visible decisions, to four standard deviations."""
    c = attention_dropout_case(name)
    vis = attn_visible(**attention_layout_kw(c))
    n = int(vis.sum()) * c["nH"]

    def fwd_mask(seed):
        def run(Q, K, V, dO, bwd):
            (O, _, dQ, dK, dV), _ = _launch(ops, c, Q, K, V, dO, bwd=False, seed=seed)
            return O, dQ, dK, dV
        return probe_fwd_mask(run, c)

    first = _long_case(ops)[2][0] if name == "i" else fwd_mask(c["seed"])
    second = fwd_mask(c["seed"] + 1)
    pt = int(c["p"] * 65536 + 0.5) / 65536
    share, want = int((first != second).sum()) / n, 2 * pt * (1 - pt)
    assert abs(share - want) < 4 * (want * (1 - want) / n) ** 0.5, (share, want, n)
    if name == "a":
        assert torch.equal(second, _host_mask(c, c["seed"] + 1) & vis[:, None])
