"""spmm_amd.retrieve on the GPU against the fp32 CPU restatement (tests/retrieve_reference.py), tiny configuration, closed-form weights,
eval mode.

Tolerances.  None of these comparisons has an earlier tolerance, so DESIGN.md section 5's rule gives them: a new path may be 1.5 x as far from
the oracle as the path that is already trusted, measured in the same run -- here the facade composites (`text_encoder.bert(mode='text')[:, 0]`
-> `text_proj` -> F.normalize; `decode.encode_properties` -> `property_proj` -> F.normalize; `match_scores(engine=False)`).  Both deviations
are printed.  The oracle's runs are computed once per module and shared.

The end-to-end tests run on seeded full-rank weights (oracle.init_state_dict): with the closed-form weights the text features of all
molecules are nearly parallel (the oracle's own COSINE between two different molecules is 1 - 1e-7 .. 1 + 1e-7, their components differ by
at most 3.5e-4: rank-2 weight matrices and a position-0 token that is always [CLS]), so "the query molecule comes back first" would be
decided by rounding alone -- and a feature gathered from the wrong row or the wrong molecule would pass the closed-form comparison.
`test_features_on_seeded_weights_sit_at_their_own_molecule` therefore repeats the feature comparison on the seeded weights, where the
reference features of two molecules are further apart than the engine path is from the reference."""
import csv
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = 1.5


def _mk(SPMM, cfg, sd):
    m = SPMM(config=None, spmm_config=cfg)
    m.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    return m.eval()


def _facade_features(m, ids, mask, pv, pm):
    from spmm_amd import decode
    cls_t = m.text_encoder.bert(ids.cuda(), attention_mask=mask.cuda(), return_dict=True, mode="text").last_hidden_state[:, 0, :]
    hid = decode.encode_properties(m, pv.cuda(), pm.cuda())
    return F.normalize(m.text_proj(cls_t), dim=-1).cpu(), F.normalize(m.property_proj(hid[:, 0, :]), dim=-1).cpu()


@pytest.fixture(scope="module")
def world(env):
    import retrieve_reference as R
    from helpers_gpu import _tiny_train_model
    O = env[0]
    oc = O.tiny_cfg()
    sd = O.closed_form_state_dict(oc)
    m = _tiny_train_model(env, dropout=False).eval()
    ids, mask, pv, pm, pairs = R.path_case()
    ref_t = R.smiles_features(sd, oc, ids, mask)
    ref_p, ref_h = R.pv_features(sd, oc, pv, pm)
    ref_match = R.match_prob(sd, oc, ref_h, ids, mask, pairs)
    return dict(O=O, R=R, m=m, ids=ids, mask=mask, pv=pv, pm=pm, pairs=pairs, ref_t=ref_t, ref_p=ref_p, ref_match=ref_match)


def _dev(a, b):
    return (a.float().cpu() - b).abs().max().item()


def test_features_match_the_reference(world):
    """5 molecules of 2, 3, 20, Lt - 1, Lt tokens and 3 property vectors, one with 20 properties unknown."""
    from spmm_amd import retrieve
    w, m = world, world["m"]
    got_t = retrieve.smiles_features(m, w["ids"], w["mask"])
    got_p, hid = retrieve.pv_features(m, w["pv"], w["pm"])
    old_t, old_p = _facade_features(m, w["ids"], w["mask"], w["pv"], w["pm"])
    assert tuple(got_t.shape) == (5, 64) and got_t.dtype == torch.float32 and tuple(got_p.shape) == (3, 64) and tuple(hid.shape) == (3, 54, 128)
    for name, got, old, ref in (("text", got_t, old_t, w["ref_t"]), ("property", got_p, old_p, w["ref_p"])):
        dn, do = _dev(got, ref), _dev(old, ref)
        print(f"[retrieve] {name} features: engine path {dn:.3e}, facade composite {do:.3e} from the oracle (rule: {RULE} x)")
        assert dn <= RULE * do, (name, dn, do)
        assert (got.norm(dim=1).cpu() - 1).abs().max().item() < 1e-5
    # device inputs give the same features as host inputs (the packed batch is then sized by a device read)
    assert torch.equal(retrieve.smiles_features(m, w["ids"].cuda(), w["mask"].cuda()), got_t)


def _matching(m, O, R, oc, sd, tag):
    from spmm_amd import retrieve
    ids, mask, pv, pm, pairs = R.path_case()
    _, ref_h = R.pv_features(sd, oc, pv, pm)
    ref = R.match_prob(sd, oc, ref_h, ids, mask, pairs)
    spread = (ref.max() - ref.min()).item()
    assert spread > 1e-3, f"the oracle's seven probabilities are near-constant ({spread:.3e}): the comparison would be vacuous"
    _, hid = retrieve.pv_features(m, pv, pm)
    got = retrieve.match_scores(m, hid, ids, mask, pairs)
    old = retrieve.match_scores(m, hid, ids, mask, pairs, engine=False)
    assert tuple(got.shape) == (7,) and got.dtype == torch.float32 and got.device.type == "cuda"
    dn, do = _dev(got, ref), _dev(old, ref)
    print(f"[retrieve] matching probability, {tag}: engine path {dn:.3e}, engine=False {do:.3e} from the oracle (rule: {RULE} x); "
          f"oracle spread {spread:.3e}; engine {[round(x, 5) for x in got.tolist()]}")
    assert dn <= RULE * do, (tag, dn, do)
    return got, hid, (ids, mask, pairs)


def test_matching_probability_matches_the_reference(world):
    """P = 7 pairs over 3 queries and 5 molecules: molecule 2 is used by three queries, query 0 by three molecules, the 2-token molecule is
    in.  The tiny configuration has ONE fusion layer: the position-0 top layer alone."""
    w = world
    oc = w["O"].tiny_cfg()
    got, hid, (ids, mask, pairs) = _matching(w["m"], w["O"], w["R"], oc, w["O"].closed_form_state_dict(oc), "tiny")
    assert (got.cpu() - w["ref_match"]).abs().max().item() < 5e-2


def test_matching_probability_with_two_fusion_layers(env):
    """Three text layers with fusion_layer = 1 and two PV layers (as test_s2p_path_gpu.py builds them): a full fusion layer over the
    [P x 54 | packed text] batch below the position-0 top layer."""
    import retrieve_reference as R
    O, SPMM, tiny_config, *_ = env
    cfg, oc = tiny_config(), O.tiny_cfg()
    cfg.text.num_hidden_layers = oc.text.num_hidden_layers = 3
    cfg.prop.num_hidden_layers = oc.prop.num_hidden_layers = 2
    sd = O.closed_form_state_dict(oc)
    _matching(_mk(SPMM, cfg, sd), O, R, oc, sd, "two fusion layers")


def test_permuting_the_pairs_permutes_the_result_exactly(world):
    from spmm_amd import retrieve
    w, m = world, world["m"]
    _, hid = retrieve.pv_features(m, w["pv"], w["pm"])
    base = retrieve.match_scores(m, hid, w["ids"], w["mask"], w["pairs"])
    perm = torch.tensor([4, 0, 6, 2, 5, 1, 3])
    got = retrieve.match_scores(m, hid, w["ids"], w["mask"], w["pairs"][perm])
    assert torch.equal(got, base[perm.cuda()]), (got.tolist(), base.tolist())
    assert torch.equal(retrieve.match_scores(m, hid, w["ids"], w["mask"], w["pairs"]), base)          # and no state is carried between calls


@pytest.fixture(scope="module")
def library(env):
    import retrieve_reference as R
    from spmm_amd import retrieve
    O, SPMM, tiny_config, *_ = env
    m = _mk(SPMM, tiny_config(), O.init_state_dict(O.tiny_cfg(), seed=3))
    ids, mask, pv, pm = R.library_case(40)
    index = retrieve.MoleculeIndex.from_tokens(m, ids, mask, batch_size=16)
    return dict(m=m, ids=ids, mask=mask, pv=pv, pm=pm, index=index, retrieve=retrieve)


def test_features_on_seeded_weights_sit_at_their_own_molecule(library):
    """`smiles_features` (one padded batch of the 40 molecules) and the index built in length-sorted batches of 16, both against the fp32
    reference on the same seeded weights: section 5's rule against the facade composite of the same run, and every engine feature is
    nearer to ITS molecule's reference feature than to any other molecule's, so a feature of the wrong row or molecule does not pass.
    Figures of an MI355X run: engine path, index and facade composite all 1.212e-3 (largest component) = 2.5e-3 .. 3.9e-3 Euclidean from the
    reference, reference features of two molecules 4.5e-3 .. 2.4e-2 apart.  The stronger statement "within HALF the smallest distance between
    two reference features" is not asserted: 2.3e-3 is one bf16 ulp of a component of the position-0 hidden state the feature is projected
    from (2^-9 relative), which neither this path nor the trusted facade composite can meet; most of that deviation is common to all
    molecules, which is why the nearest reference is still the right one for every molecule."""
    import retrieve_reference as R
    import spmm_oracle as O
    L, rt, m = library, library["retrieve"], library["m"]
    oc = O.tiny_cfg()
    sd = O.init_state_dict(oc, seed=3)
    ref = R.smiles_features(sd, oc, L["ids"], L["mask"])
    got = rt.smiles_features(m, L["ids"], L["mask"]).cpu()
    cls_t = m.text_encoder.bert(L["ids"].cuda(), attention_mask=L["mask"].cuda(), return_dict=True, mode="text").last_hidden_state[:, 0, :]
    old = F.normalize(m.text_proj(cls_t), dim=-1).cpu()
    dn, do, di = (got - ref).abs().max().item(), (old - ref).abs().max().item(), (L["index"].feats.cpu() - ref).abs().max().item()
    apart = (torch.cdist(ref.double(), ref.double()) + 10 * torch.eye(40, dtype=torch.float64)).min().item()
    print(f"[retrieve] seeded weights, text features: engine path {dn:.3e}, index {di:.3e}, facade composite {do:.3e} from the oracle; "
          f"Euclidean: engine path at most {torch.cdist(got.double(), ref.double()).diagonal().max().item():.3e} from its own reference feature, "
          f"two reference features at least {apart:.3e} apart")
    assert dn <= RULE * do and di <= RULE * do, (dn, di, do)
    for name, x in (("smiles_features", got), ("index", L["index"].feats.cpu())):
        d = torch.cdist(x.double(), ref.double())
        assert torch.equal(d.argmin(dim=1), torch.arange(40)), name


BOUND = 2 * 64 * 2.0 ** -24          # the kernel's fp32 accumulation bound at E = 64 (tests/test_sim_topk_gpu.py)


def test_retrieve_end_to_end(library):
    """40 molecules, k = 8, rerank = 4: the shortlist is the top 8 of the float64 cosine matrix of the engine's own features (near-tie rule of
    the kernel's tests), its first four are ordered by the returned matching probability, and indices refer to INPUT order although the index
    was built in length-sorted batches of 16."""
    L, rt = library, library["retrieve"]
    m, index = L["m"], L["index"]
    assert tuple(index.feats.shape) == (40, 64) and len(index) == 40
    res = rt.retrieve(m, index, L["ids"], L["mask"], L["pv"], L["pm"], k=8, rerank=4)
    qf, hid = rt.pv_features(m, L["pv"], L["pm"])
    S64 = qf.cpu().double() @ index.feats.cpu().double().T
    idx, cos, match = res.index.cpu(), res.cosine.cpu(), res.match.cpu()
    assert tuple(idx.shape) == tuple(cos.shape) == tuple(match.shape) == (3, 8)
    true = S64.sort(dim=1, descending=True).values[:, :8]
    for q in range(3):
        assert idx[q].unique().numel() == 8 and int(idx[q].min()) >= 0 and int(idx[q].max()) < 40
    assert (cos.double() - S64.gather(1, idx)).abs().max().item() <= BOUND
    assert (true - cos.double().sort(dim=1, descending=True).values).max().item() <= BOUND
    assert bool((cos[:, 5:] <= cos[:, 4:7]).all())                                   # beyond the re-ranked head: still by cosine
    assert bool(torch.isnan(match[:, 4:]).all()) and bool(torch.isfinite(match[:, :4]).all())
    assert bool((match[:, 1:4] <= match[:, :3]).all()), match[:, :4]
    pairs = torch.stack([torch.arange(3).repeat_interleave(4), idx[:, :4].reshape(-1)], dim=1)
    direct = rt.match_scores(m, hid, L["ids"], L["mask"], pairs).cpu().reshape(3, 4)
    assert (direct - match[:, :4]).abs().max().item() < 1e-6
    # input order: the same library given in another order -- its 40 distinct lengths sort into the same batches -- gives the same features
    # at the permuted places and the same molecules at the permuted indices
    perm = torch.randperm(40, generator=torch.Generator().manual_seed(4))
    index_p = rt.MoleculeIndex.from_tokens(m, L["ids"][perm], L["mask"][perm], batch_size=16)
    assert torch.equal(index_p.feats, index.feats[perm.cuda()])
    assert not torch.equal(perm, torch.argsort(L["mask"].sum(1), stable=True))
    res_p = rt.retrieve(m, index_p, None, None, L["pv"], L["pm"], k=8, rerank=4)
    assert torch.equal(perm[res_p.index.cpu()], idx) and torch.equal(res_p.cosine.cpu(), cos)
    # a ranking longer than the kernel's 64 slots and than the library: two passes, then empty slots
    s100, i100 = index.search(qf, 100, chunk=16)
    assert torch.equal(i100[:, :8].cpu(), rt.MoleculeIndex(index.feats).search(qf, 8)[1].cpu())
    assert bool((i100[:, 40:] == -1).all()) and all(i100[q, :40].unique().numel() == 40 for q in range(3))
    assert (S64.sort(dim=1, descending=True).values - s100[:, :40].cpu().double()).abs().max().item() <= BOUND


def test_similar_returns_the_molecule_itself_first(library):
    """Queried with library molecules whose nearest other molecule is further than 2 x the kernel's bound away (float64 cosine of the
    engine's own features) -- for the others rounding could decide."""
    L, rt = library, library["retrieve"]
    feats64 = L["index"].feats.cpu().double()
    C = feats64 @ feats64.T - 2 * torch.eye(40, dtype=torch.float64)
    clear = torch.nonzero(1 - C.max(dim=1).values > 2 * BOUND).flatten()
    print(f"[retrieve] similar: {clear.numel()} of 40 molecules are more than {2 * BOUND:.2e} from their nearest neighbour")
    assert clear.numel() >= 3
    lens = L["mask"][clear].sum(1)
    Lq = int(lens.max())
    scores, idx = rt.similar(L["m"], L["index"], L["ids"][clear, :Lq], L["mask"][clear, :Lq], 5)
    assert torch.equal(idx[:, 0].cpu(), clear), (idx[:, 0].tolist(), clear.tolist())
    assert (scores[:, 0].cpu() - 1).abs().max().item() <= BOUND + 1e-6          # (+ the features' own distance from unit length)


def test_driver_writes_ranked_rows(tmp_path):
    out = tmp_path / "hits.csv"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "retrieve.py"), "--synthetic", "64", "--tiny", "--top_k", "5", "--rerank", "3",
                        "--output", str(out)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = list(csv.reader(open(out)))
    assert rows[0] == ["rank", "library_line", "smiles", "cosine", "match_probability"] and len(rows) == 6
    assert [int(x[0]) for x in rows[1:]] == [1, 2, 3, 4, 5]
    assert len({x[1] for x in rows[1:]}) == 5 and all(1 <= int(x[1]) <= 64 and x[2] for x in rows[1:])
    assert all(x[4] != "" for x in rows[1:4]) and all(x[4] == "" for x in rows[4:])
    assert [float(x[4]) for x in rows[1:4]] == sorted((float(x[4]) for x in rows[1:4]), reverse=True)
