"""spmm_amd.attribution on the GPU against the fp32 CPU restatement (tests/attn_map_reference.py: fusion_maps / reaction_maps), tiny
configuration, eval mode, seeded full-rank weights (oracle.init_state_dict; tests/test_retrieve_path_gpu.py says why: with the closed-form
weights all molecules look alike and a wrong row would pass) with the cross-attention query / key weights sharpened
(attn_map_reference.sharpen: the seeded weights alone give near-uniform maps, which any kernel would reproduce).

Path deviation, DESIGN.md section 5's rule.  No earlier path produces maps, so the trusted comparator is the eager fp32 softmax on the
TAPPED bf16 Q / K -- the engine's own hidden states, no new kernel.  cross_attention_maps / reaction_attention_maps may be at most 1.5 x as
far from the oracle as that comparator, measured in the same run; both deviations are printed.
Figures of an MI355X run (largest |map - oracle| over all pairs and heads; new path / comparator): one fusion layer pv2text 6.824e-3 /
6.823e-3, text2pv 4.348e-3 / 4.348e-3; two fusion layers 9.211e-3, 9.042e-3 (pv2text) and 3.817e-3, 5.753e-3 (text2pv), the same to four
digits on both sides; reactions 5.549e-3 / 5.549e-3.  The deviation is that of the bf16 hidden states, common to both.  Two molecules under
one PV are 8.0e-2 .. 3.5e-1 apart in the reference."""
import csv
import os
import subprocess
import sys
from dataclasses import replace

import pytest
import torch

import attn_map_reference as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = 1.5


def _mk(SPMM, cfg, sd):
    m = SPMM(config=None, spmm_config=cfg)
    m.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    return m.eval()


def _eager(tap, li, gi):
    """The comparator: softmax(Q K^T / 8) in fp32 torch on the tapped views, per sequence at its own lengths -> [per sequence [nH, nq, nk]]."""
    g, Q, K = tap.qk[(li, gi)]
    nH = tap.nH
    src = g.src
    q0 = g.q_row0.tolist() if g.q_row0 is not None else [s * g.L for s in range(g.nseq)]
    ql = g.q_len.tolist() if g.q_len is not None else [g.L] * g.nseq
    kv = g.kv_idx.tolist()
    k0 = src.row0.tolist() if src.row0 is not None else [u * src.Lkv for u in range(src.U)]
    kl = src.len.tolist() if src.len is not None else [src.Lkv] * src.U
    out = []
    for s in range(g.nseq):
        u = kv[s]
        q = Q[q0[s]:q0[s] + ql[s]].float().view(ql[s], nH, 64)
        k = K[k0[u]:k0[u] + kl[u]].float().view(kl[u], nH, 64)
        out.append(torch.softmax(torch.einsum("qhd,khd->hqk", q, k) / 8.0, dim=-1).cpu())
    return out


def _world(env, n_layers):
    import spmm_oracle as O
    _, SPMM, tiny_config, *_ = env
    cfg, oc = tiny_config(), O.tiny_cfg()
    cfg.text.num_hidden_layers = oc.text.num_hidden_layers = n_layers
    sd = A.path_state_dict(oc)
    m = _mk(SPMM, cfg, sd)
    ids, mask, pv, pm, pairs = A.path_case()
    ref = A.fusion_maps(sd, oc, pv, pm, ids, mask, pairs)
    return dict(m=m, oc=oc, sd=sd, ids=ids, mask=mask, pv=pv, pm=pm, pairs=pairs, ref=ref, lens=mask.sum(1).tolist())


@pytest.fixture(scope="module")
def world1(env):
    """The tiny configuration as it is: one fusion layer."""
    return _world(env, 2)


@pytest.fixture(scope="module")
def world2(env):
    """Three text layers, fusion_layer = 1: two fusion layers (as tests/test_retrieve_path_gpu.py builds them)."""
    return _world(env, 3)


def _check_paths(w, layers, tag):
    from spmm_amd import attribution
    taps = []

    def hook(t):
        t.keep_qk = True
        taps.append(t)
    maps = attribution.cross_attention_maps(w["m"], w["pv"], w["pm"], w["ids"], w["mask"], w["pairs"], layers=layers, heads="all", direction="both",
                                            _tap_hook=hook)
    mean = attribution.cross_attention_maps(w["m"], w["pv"], w["pm"], w["ids"], w["mask"], w["pairs"], layers=layers, heads="mean", direction="both")
    torch.cuda.synchronize()
    tap = taps[0]
    n_f = w["oc"].text.num_hidden_layers - w["oc"].text.fusion_layer
    assert maps.layers == (tuple(range(n_f)) if layers == "all" else (n_f - 1,))
    for d, gi in (("pv2text", 0), ("text2pv", 1)):
        for li in maps.layers:
            eager = _eager(tap, li, gi)
            dn = do = 0.0
            for p, (qi, mi) in enumerate(w["pairs"].tolist()):
                ref = w["ref"][p][(li, d)]
                got = maps.get(p, li, d).cpu()
                n = w["lens"][mi]
                assert tuple(got.shape) == ((2, 54, n) if d == "pv2text" else (2, n, 54)) == tuple(ref.shape), (got.shape, ref.shape)
                gm = mean.get(p, li, d).cpu()
                assert tuple(gm.shape) == tuple(got.shape[1:]) and (got.mean(0) - gm).abs().max().item() <= 1e-6
                assert (gm.double().sum(1) - 1).abs().max().item() <= 1e-5 and (got.double().sum(2) - 1).abs().max().item() <= 1e-5
                dn = max(dn, (got - ref).abs().max().item())
                do = max(do, (eager[p] - ref).abs().max().item())
            # vacuity guards, on the reference alone: molecules 2 and 4 under PV 0 (pairs 1 and 2) differ; the maps are not near-uniform
            a, b = w["ref"][1][(li, d)].mean(0), w["ref"][2][(li, d)].mean(0)
            apart = ((a[:, :20] - b[:, :20]) if d == "pv2text" else (a[:20] - b[:20])).abs().max().item()
            share = min(A.contrast_share(w["ref"][p][(li, d)]) for p in range(len(w["ref"])))
            print(f"[attention maps] {tag}, layer {li}, {d}: cross_attention_maps {dn:.3e}, eager softmax on the tapped Q / K {do:.3e} from the "
                  f"oracle (rule: {RULE} x); two molecules under one PV {apart:.3e} apart; rows with max / min > 1.5: at least {share:.2f}")
            assert apart > 10 * do, (apart, do)
            assert share >= 0.5, share
            assert dn <= RULE * do, (tag, li, d, dn, do)


def test_last_layer_maps_match_the_reference(world1):
    _check_paths(world1, (-1,), "one fusion layer")


def test_all_layers_maps_match_the_reference(world2):
    _check_paths(world2, "all", "two fusion layers")


def test_a_pair_alone_has_the_bits_it_has_among_the_seven(world2):
    """Packed rows, shared sources: the launch's other sequences do not reach a sequence's rows."""
    from spmm_amd import attribution
    w = world2
    allm = attribution.cross_attention_maps(w["m"], w["pv"], w["pm"], w["ids"], w["mask"], w["pairs"], layers="all", heads="all")
    for p in (0, 3, 6):
        one = attribution.cross_attention_maps(w["m"], w["pv"], w["pm"], w["ids"], w["mask"], w["pairs"][p:p + 1], layers="all", heads="all")
        for li in allm.layers:
            for d in allm.directions:
                assert torch.equal(one.get(0, li, d).view(torch.int32), allm.get(p, li, d).view(torch.int32)), (p, li, d)
    only = attribution.cross_attention_maps(w["m"], w["pv"], w["pm"], w["ids"], w["mask"], w["pairs"], layers=(0,), direction="text2pv")
    assert only.directions == ("text2pv",) and set(k[2] for k in only.maps) == {"text2pv"} and only.layers == (0,)
    assert (only.get(4) - allm.get(4, 0, "text2pv").mean(0)).abs().max().item() <= 1e-6


def test_refusals(world1):
    from spmm_amd import attribution, ops
    w = world1
    args = (w["m"], w["pv"], w["pm"], w["ids"], w["mask"])
    with pytest.raises(IndexError, match="not there"):
        attribution.cross_attention_maps(*args, torch.tensor([[3, 0]]))
    with pytest.raises(IndexError, match="not there"):
        attribution.cross_attention_maps(*args, torch.tensor([[0, 5]]))
    for kw, msg in ((dict(layers=(1,)), "unknown layer 1"), (dict(layers="every"), "layers='every'"), (dict(heads="max"), "heads='max'"),
                    (dict(direction="up"), "direction='up'")):
        with pytest.raises(ValueError, match=msg):
            attribution.cross_attention_maps(*args, w["pairs"], **kw)
    long_ids = torch.full((1, ops.ATTN_MAXL + 1), 5, dtype=torch.long)
    with pytest.raises(ValueError, match=f"exceeds the {ops.ATTN_MAXL}"):
        attribution.cross_attention_maps(w["m"], w["pv"][:1], None, long_ids, torch.ones_like(long_ids))
    empty = attribution.cross_attention_maps(*args, torch.zeros(0, 2, dtype=torch.long))
    assert empty.maps == {}


# ---------------------------------------------------------------------------------------------------------------- nothing existing changes
@pytest.mark.parametrize("fx", ["nograd", "off"])
def test_the_tap_leaves_the_stack_s_output_alone(env, fx):
    """eng.stack_fwd over the fusion batch with and without a tap, on the one-launch and on the composite cross-attention block."""
    import spmm_oracle as O
    from spmm_amd.engine import Batch, Group, KVSource
    _, SPMM, tiny_config, *_ = env
    cfg, oc = tiny_config(), O.tiny_cfg()
    cfg.text.num_hidden_layers = oc.text.num_hidden_layers = 3
    m = _mk(SPMM, cfg, A.path_state_dict(oc))
    eng = m.engine
    eng.train_mode = False
    old = eng.opt.fused_xattn
    eng.opt.fused_xattn = fx
    try:
        ct = cfg.text
        H = ct.hidden_size
        g = torch.Generator().manual_seed(3)
        BFL = torch.bfloat16
        X = torch.randn(3 * 54 + 40, H, generator=g).to(BFL).cuda()
        text = torch.randn(2 * 24, H, generator=g).to(BFL).cuda()
        pvh = torch.randn(2 * 54, H, generator=g).to(BFL).cuda()
        i32 = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")                                      # noqa: E731

        def run(tap):
            src_t = KVSource(text, 2, 24, row0=i32([0, 24]), length=i32([24, 9]))
            src_p = KVSource(pvh, 2, 54)
            b = Batch([Group(0, 3, 54, None, 3).bind(src_t, i32([0, 1, 1]), 0),
                       Group(162, 3, 24, None, 3, q_row0=i32([0, 24, 33]), q_len=i32([24, 9, 7]), nrows=40).bind(src_p, i32([1, 0, 0]), 0)])
            kw = {} if tap is None else {"xattn_tap": tap}
            y, _, _ = eng.stack_fwd("text_encoder.bert.", ct, range(ct.fusion_layer, ct.num_hidden_layers), True, X, b, False, **kw)
            torch.cuda.synchronize()
            return y
        seen = []
        y0 = run(None)
        y1 = run(lambda layer, gi, grp, Q, K: seen.append((layer, gi, tuple(Q.shape), tuple(K.shape), Q.data_ptr() % 16)))
        assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
        assert [(s[0], s[1]) for s in seen] == [(1, 0), (1, 1), (2, 0), (2, 1)], seen
        assert seen[0][2:4] == ((162, H), (48, H)) and seen[1][2:4] == ((40, H), (108, H))
    finally:
        eng.opt.fused_xattn = old


def test_the_existing_paths_return_the_same_bits_before_and_after(world1):
    from spmm_amd import attribution, retrieve
    w, m = world1, world1["m"]
    _, hid = retrieve.pv_features(m, w["pv"], w["pm"])
    before = retrieve.match_scores(m, hid, w["ids"], w["mask"], w["pairs"])
    attribution.cross_attention_maps(m, w["pv"], w["pm"], w["ids"], w["mask"], w["pairs"], layers="all", heads="all")
    after = retrieve.match_scores(m, hid, w["ids"], w["mask"], w["pairs"])
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- reactions
@pytest.fixture(scope="module")
def rxn_world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import spmm_oracle as O
    import rxn_reference as X
    from spmm_amd.config import tiny_config
    from spmm_amd.rxn import SPMMRxn
    o_dec = replace(O.tiny_cfg().text, num_hidden_layers=2)
    o_enc = X.encoder_cfg(o_dec)
    sd = A.rxn_state_dict(o_dec, o_enc)
    m = SPMMRxn(bert_config=replace(tiny_config().text, num_hidden_layers=2))
    res = m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    case = A.rxn_case()
    return dict(m=m.eval(), case=case, ref=A.reaction_maps(sd, o_dec, o_enc, *case))


def test_reaction_maps_match_the_reference(rxn_world):
    """Three reactions: sources of 3, 30 and 149 tokens, products of 2, 20 and 99.  Maps are [product tokens, source tokens]; columns past
    the source's length are absent.  score_products returns the same bits before and after."""
    from spmm_amd import attribution, score
    w, m = rxn_world, rxn_world["m"]
    sids, smask, pids, pmask, pairs = w["case"]
    before = score.score_products(m, sids, smask, pids, pmask, pairs)
    taps = []

    def hook(t):
        t.keep_qk = True
        taps.append(t)
    maps = attribution.reaction_attention_maps(m, sids, smask, pids, pmask, pairs, heads="all", _tap_hook=hook)
    mean = attribution.reaction_attention_maps(m, sids, smask, pids, pmask, pairs)
    after = score.score_products(m, sids, smask, pids, pmask, pairs)
    for a, b in ((before.logp, after.logp), (before.token_logp, after.token_logp)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(before.n_tokens, after.n_tokens)
    eager = _eager(taps[0], 0, 0)
    dn = do = 0.0
    for p, (ls, lc) in enumerate(((3, 2), (30, 20), (149, 99))):
        got, ref = maps.get(p).cpu(), w["ref"][p][0]
        assert tuple(got.shape) == (2, lc, ls) == tuple(ref.shape)
        gm = mean.get(p).cpu()
        assert (got.mean(0) - gm).abs().max().item() <= 1e-6 and (gm.double().sum(1) - 1).abs().max().item() <= 1e-5
        dn, do = max(dn, (got - ref).abs().max().item()), max(do, (eager[p] - ref).abs().max().item())
        assert A.contrast_share(ref) >= 0.5
    print(f"[attention maps] reactions: reaction_attention_maps {dn:.3e}, eager softmax on the tapped Q / K {do:.3e} from the oracle (rule: {RULE} x)")
    assert dn <= RULE * do, (dn, do)
    with pytest.raises(ValueError, match="unknown layer"):
        attribution.reaction_attention_maps(m, sids, smask, pids, pmask, pairs, layers=(3,))
    with pytest.raises(IndexError, match="not there"):
        attribution.reaction_attention_maps(m, sids, smask, pids, pmask, torch.tensor([[0, 4]]))


# ---------------------------------------------------------------------------------------------------------------- the driver
def _driver(tmp_path, *flags):
    out = tmp_path / "attention.csv"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "attend.py"), *flags, "--tiny", "--batch_size", "4", "--output", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = list(csv.reader(open(out)))
    assert rows[0] == ["line", "layer", "direction", "head", "query_index", "query_label", "key_index", "key_label", "weight"]
    return rows[1:], r.stdout


def _sums(rows):
    s = {}
    for x in rows:
        s[tuple(x[:5])] = s.get(tuple(x[:5]), 0.0) + float(x[8])
    return s


def test_driver_writes_maps_in_input_order(tmp_path):
    sys.path.insert(0, ROOT)
    from pv2smiles import synthetic_vocab
    from smiles2pv import synthetic_smiles
    rows, out = _driver(tmp_path, "--synthetic", "6")
    sums = _sums(rows)
    assert sums and all(abs(v - 1) <= 1e-4 for v in sums.values()), max(abs(v - 1) for v in sums.values())
    assert [int(x[0]) for x in rows] == sorted(int(x[0]) for x in rows) and {int(x[0]) for x in rows} == set(range(1, 7))
    assert {x[2] for x in rows} == {"pv2text", "text2pv"} and {x[3] for x in rows} == {"mean"}
    smiles = synthetic_smiles(synthetic_vocab(300), 6, 0)
    for line, s in enumerate(smiles, 1):            # the text-side labels of every line spell ITS molecule: the lines came back in input order
        labs = [x[7] for x in rows if int(x[0]) == line and x[2] == "pv2text" and x[4] == "0"]
        assert labs[0] == "[CLS]" and labs[-1] == "[SEP]"
        assert "".join(l[:l.rindex("[")] for l in labs[1:-1]) == s
        for l in labs[1:-1]:
            a, b = l[l.rindex("[") + 1:-1].split(":")
            assert s[int(a):int(b)] == l[:l.rindex("[")]
    assert out.count("entropy") == 18


def test_driver_writes_reaction_maps(tmp_path):
    rows, _ = _driver(tmp_path, "--rxn", "--synthetic", "4")
    sums = _sums(rows)
    assert sums and all(abs(v - 1) <= 1e-4 for v in sums.values())
    assert {x[2] for x in rows} == {"product2reactant"} and {int(x[0]) for x in rows} == {1, 2, 3, 4}
    assert [int(x[0]) for x in rows] == sorted(int(x[0]) for x in rows)
