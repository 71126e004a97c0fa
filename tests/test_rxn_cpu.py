"""CPU-side checks of the reaction-prediction path: the `need` rule of the beam bookkeeping against the sequential restatement of
`evaluate_beam`, the checkpoint mappings, the state-dict names, the argument validation of the two new entry points (no launch), the
driver's parsing / reader / accuracy / batching, and the whole-prefix baseline of predict_products on the CPU restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spmm_oracle as O
import rxn_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rxn_predict as D      # noqa: E402


# ------------------------------------------------------------------------------------------------------------------ bookkeeping
def _random_positions(N, k, V, T, seed, sep_rate):
    """Per position fp32 logits [N*k, V] in which [SEP] is among the k best of a beam with probability ~sep_rate."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(T):
        logits = torch.randn(N * k, V, generator=g) * 2.0
        boost = torch.rand(N * k, generator=g) < sep_rate
        logits[:, R.SEP_ID] += torch.where(boost, torch.full((N * k,), 6.0), torch.full((N * k,), -8.0))
        out.append(logits)
    return out


def _run_book(book, first, positions):
    from spmm_amd import decode
    N, k = book.N, book.k
    book.first(*first)
    for logits in positions:
        values, indices = decode._pick(torch.softmax(logits.view(N, k, -1), dim=-1), k, False)
        book.update(values, indices)
        if book.all_done():
            break
    return book.results()


def _run_sequential(N, k, need, first, positions):
    from spmm_amd import decode
    out = []
    for n in range(N):
        sb = R.SequentialBook(k, need)
        sb.first(first[0][n], first[1][n])
        for logits in positions:
            values, indices = decode._pick(torch.softmax(logits.view(N, k, -1)[n], dim=-1), k, False)
            if sb.update(values, indices):
                break
        out.append(sb.results())
    return out


@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("sep_rate", [0.6, 0.02])
def test_beam_book_with_need_matches_the_sequential_bookkeeping(k, sep_rate):
    """BeamBook(need=k*k).update (tensor ops, N molecules at once) against the sequential `evaluate_beam` bookkeeping, hypothesis for
    hypothesis, on random logits: V = 20, 12 positions.  sep_rate 0.02 reaches the position limit with fewer than k*k finals for most
    molecules (whatever ended is returned)."""
    from spmm_amd import decode
    N, V, T = 7, 20, 12
    g = torch.Generator().manual_seed(11 + k)
    first = (torch.randn(N, k, generator=g), torch.stack([torch.randperm(V - 4, generator=g)[:k] + 4 for _ in range(N)]))
    positions = _random_positions(N, k, V, T, seed=100 + k, sep_rate=sep_rate)
    book = decode.BeamBook(N, k, T, "cpu", need=k * k)
    assert book.F == k * k + k and book.need == k * k
    got = _run_book(book, first, positions)
    want = _run_sequential(N, k, k * k, first, positions)
    assert [[h[1] for h in m] for m in got] == [[h[1] for h in m] for m in want]
    for a, b in zip(got, want):
        for (pa, _), (pb, _) in zip(a, b):
            assert abs(pa - pb) < 1e-5
    n_fin = book.fin_n.tolist()
    if sep_rate < 0.1:
        assert any(n < k * k for n in n_fin) and not bool(book.done.all())          # the position limit, not the finals, ended these
    else:
        assert any(n >= k * k for n in n_fin)


@pytest.mark.parametrize("k", [1, 2, 5])
def test_beam_book_without_need_is_todays_rule(k):
    """need=None is need=k: F = 2k, done at k finals -- the sequential bookkeeping with need = k, and BeamBook(need=k) state for state."""
    from spmm_amd import decode
    N, V, T = 6, 20, 12
    g = torch.Generator().manual_seed(3 + k)
    first = (torch.randn(N, k, generator=g), torch.stack([torch.randperm(V - 4, generator=g)[:k] + 4 for _ in range(N)]))
    positions = _random_positions(N, k, V, T, seed=50 + k, sep_rate=0.25)
    a, b = decode.BeamBook(N, k, T, "cpu"), decode.BeamBook(N, k, T, "cpu", need=k)
    assert a.F == 2 * k == b.F and a.need == k
    got, same = _run_book(a, first, positions), _run_book(b, first, positions)
    assert got == same and torch.equal(a.tokens, b.tokens) and torch.equal(a.fin_tok, b.fin_tok) and torch.equal(a.done, b.done)
    want = _run_sequential(N, k, k, first, positions)
    assert [[h[1] for h in m] for m in got] == [[h[1] for h in m] for m in want]
    with pytest.raises(ValueError):
        decode.BeamBook(N, k, T, "cpu", need=k * k + 1)


# ------------------------------------------------------------------------------------------------------------ checkpoints, names
@pytest.fixture()
def dry_model():
    """SPMMRxn at the tiny configuration with every launch replaced by a prototype check (no GPU)."""
    from spmm_amd import ops
    from spmm_amd.config import tiny_config
    from spmm_amd.rxn import SPMMRxn
    old = ops._DRY_RUN
    ops._DRY_RUN = True
    try:
        yield SPMMRxn(bert_config=tiny_config().text, device="cpu")
    finally:
        ops._DRY_RUN = old


def test_rxn_spec_names_are_the_reference_models():
    """config.rxn_spec against the key list of SPMM_rxn.state_dict() derived from the two configs: `text_encoder` (BertForMaskedLM,
    cross-attention in the fusion layers) then `text_encoder2` (BertForMaskedLM on config_bert_smiles.json: num_hidden_layers =
    fusion_layer = 6, no cross-attention), names, shapes and order -- at the tiny and at the published size."""
    from spmm_amd.config import BertConfig, rxn_encoder_config, rxn_spec, tiny_config
    for c_dec, o_dec in ((tiny_config().text, O.tiny_cfg().text), (BertConfig(add_cross_attention=True), O.full_cfg().text)):
        c_enc = rxn_encoder_config(c_dec)
        assert c_enc.num_hidden_layers == c_enc.fusion_layer == c_dec.fusion_layer
        got = [(n, tuple(s)) for n, s, _ in rxn_spec(c_dec, c_enc)]
        want = [(n, tuple(s)) for n, s, _ in R.rxn_keys(o_dec, R.encoder_cfg(o_dec))]
        assert got == want
    names = [n for n, _ in got]
    assert len(names) == 2 * (6 + 7) + 12 * 16 + 6 * 10 + 6 * 16                   # embeddings + MLM head twice; 12 layers, 6 with cross; 6 encoder layers
    assert "text_encoder2.cls.predictions.decoder.weight" in names and not any("text_encoder2" in n and "crossattention" in n for n in names)
    assert "text_encoder.bert.encoder.layer.6.crossattention.self.key.weight" in names
    assert "text_encoder.bert.encoder.layer.5.crossattention.self.key.weight" not in names


def _pretraining_dict(cfg):
    """A pretraining checkpoint's state dict with distinct values, plus the legacy `_unk` key."""
    sd = O.closed_form_state_dict(cfg)
    sd["property_unk"] = sd.pop("property_mask")
    sd["text_encoder.legacy_unk"] = torch.ones(1)
    return sd


def test_pretraining_checkpoint_maps_onto_both_encoders(dry_model):
    from spmm_amd.rxn import map_checkpoint
    cfg = O.tiny_cfg()
    sd = _pretraining_dict(cfg)
    mapped = map_checkpoint(sd)
    assert not any(("queue" in k) or ("property" in k) or ("_m" in k.replace("_mask", "")) or ("_unk" in k) for k in mapped)      # dropped / renamed
    assert "text_encoder.legacy_mask" in mapped and "temp" in mapped and "text_proj.weight" in mapped       # kept (the load ignores them)
    res = dry_model.load_pretrained({"state_dict": sd})
    assert res.missing_keys == []
    assert set(res.unexpected_keys) >= {"temp", "text_proj.weight", "text_encoder.legacy_mask", "text_encoder2.legacy_mask"}
    assert all(not k.startswith("text_encoder.") or "legacy" in k for k in res.unexpected_keys)
    assert all("crossattention" in k or ".layer.1." in k or "legacy" in k for k in res.unexpected_keys if k.startswith("text_encoder2."))
    got = dry_model.state_dict()
    for name, t in got.items():
        src = name.replace("text_encoder2.", "text_encoder.")
        assert torch.equal(t.cpu(), sd[src].reshape(t.shape)), name                                          # decoder as is, encoder from the SMILES encoder
    # the 'model' key of legacy checkpoints and a bare dict load the same
    for ck in ({"model": sd}, sd):
        assert dry_model.load_pretrained(ck).missing_keys == []


def test_fine_tuned_checkpoint_round_trip(dry_model):
    """A fine-tuned checkpoint holds both prefixes under 'state_dict': its own text_encoder2.* wins over the copy of text_encoder.*."""
    c_dec = O.tiny_cfg().text
    sd = R.closed_form_state_dict(c_dec, R.encoder_cfg(c_dec))
    assert not torch.equal(sd["text_encoder2.bert.embeddings.word_embeddings.weight"], sd["text_encoder.bert.embeddings.word_embeddings.weight"])
    res = dry_model.load_pretrained({"state_dict": {k: v.clone() for k, v in sd.items()}})
    assert res.missing_keys == [] and all(k.startswith("text_encoder2.") for k in res.unexpected_keys)
    out = dry_model.state_dict()
    assert list(out) == list(sd)
    for k, v in sd.items():
        assert torch.equal(out[k].cpu(), v), k
    strict = dry_model.load_state_dict(out, strict=True)
    assert strict.missing_keys == [] and strict.unexpected_keys == []
    with pytest.raises(NotImplementedError, match="inference only"):
        dry_model(torch.zeros(1, 3, dtype=torch.long), torch.ones(1, 3, dtype=torch.long), torch.zeros(1, 3, dtype=torch.long), torch.ones(1, 3, dtype=torch.long))
    from spmm_amd.rxn import SPMM_rxn, SPMMRxn
    assert SPMM_rxn is SPMMRxn and dry_model.eval() is dry_model and dry_model.device == torch.device("cpu")


def test_engine_path_launch_sequence_matches_the_header(dry_model):
    """predict_products / greedy_products on the engine with launches replaced by prototype checks: every call matches include/spmm_hip.h, the
    memory's keys | values are projected once per fusion layer, every position reads them through spmm_decode_xattn and books through
    spmm_beam_step_until; masks that are not right-padded non-empty prefixes, and sources over 256 tokens, are refused."""
    from spmm_amd import decode, ops
    ids = torch.randint(4, 300, (3, 9))
    mask = torch.ones(3, 9, dtype=torch.long)
    mask[1, 4:] = 0
    mask[2, 1:] = 0
    ops._dry_log.clear()
    out = decode.predict_products(dry_model, ids, mask, k=3, max_steps=5)
    log = list(ops._dry_log)
    assert len(out) == 3
    assert log.count("spmm_decode_xattn") == 6 and log.count("spmm_beam_step_until") == 5 and "spmm_beam_step" not in log      # 1 fusion layer, positions 0..5
    assert log.count("spmm_pack_plan") == 1 and log.count("spmm_decode_attn") == 2 * 6
    ops._dry_log.clear()
    g = decode.greedy_products(dry_model, ids, mask, max_steps=5)
    assert len(g) == 3 and all(len(r) <= 6 and r[0] == R.CLS_ID for r in g) and ops._dry_log.count("spmm_decode_xattn") in (4, 5)      # (unlaunched logits: may "end" at the first host read)
    holes = mask.clone()
    holes[0, 2] = 0
    empty = mask.clone()
    empty[2] = 0
    for bad in (holes, empty):
        with pytest.raises(ValueError, match="right-padded"):
            decode.predict_products(dry_model, ids, bad, k=3, max_steps=5)
    with pytest.raises(ValueError, match="256"):
        decode.predict_products(dry_model, torch.ones(1, 257, dtype=torch.long), torch.ones(1, 257, dtype=torch.long), k=3, max_steps=5)
    with pytest.raises(ValueError, match="beams"):
        decode.predict_products(dry_model, ids, mask, k=9, max_steps=5)


# ----------------------------------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def built():
    so = os.path.join(ROOT, "spmm_amd", "libspmm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return so


def _xattn_args(**kw):
    a = dict(q=64, ldq=128, K=64, V=192, ldkv=256, kv_seq=None, kv_row0=64, kv_len=64, group=2, out=64, ldo=128, R=6, nH=2, Lkv_max=149, scale=0.125)
    a.update(kw)
    return tuple(a.values()) + (None,)


def test_decode_xattn_validates_its_arguments_without_touching_the_gpu(built):
    """Every refusal happens before the launch (the non-null pointers here are never dereferenced)."""
    from spmm_amd._lib import lib
    L = lib()
    for kw, msg in ((dict(group=0), "group=0"), (dict(group=9, R=9), "group=9"), (dict(R=7), "multiple of group"), (dict(Lkv_max=0), "Lkv_max=0"),
                    (dict(Lkv_max=257), "Lkv_max=257"), (dict(ldkv=260), "ldkv=260"), (dict(ldkv=64), "ldkv=64"), (dict(kv_len=None), "are required"),
                    (dict(kv_row0=None), "are required"), (dict(q=None), "are required"), (dict(ldq=100), "ldq=100"), (dict(ldo=64), "ldo=64"),
                    (dict(K=72), "misaligned"), (dict(R=0), "R=0")):
        with pytest.raises(RuntimeError, match=msg):
            L.call("spmm_decode_xattn", *_xattn_args(**kw))


def _beam_args(**kw):
    a = dict(logits=64, ldl=300, N=4, k=3, V=300, Lmax=103, F=11, t=2, t_ptr=None, t_off=0, tokens=64, cur_p=64, fin_p=64, fin_len=64, fin_tok=64,
             fin_n=64, done=64, anc=None, anc_ld=0, ids_out=64, parent_out=None, n_done=None, mol=None, rowmap=None, need=9)
    a.update(kw)
    return tuple(a.values()) + (None,)


def test_beam_step_until_validates_its_arguments_without_touching_the_gpu(built):
    from spmm_amd._lib import lib
    L = lib()
    for kw, msg in ((dict(need=2), "need=2"), (dict(need=10, F=12), "need=10"), (dict(F=10), "F=10"), (dict(k=9, need=81, F=90), "k=9"),
                    (dict(t=0), "t=0"), (dict(anc=64, anc_ld=50), "anc_ld=50")):
        with pytest.raises(RuntimeError, match=msg):
            L.call("spmm_beam_step_until", *_beam_args(**kw))


# -------------------------------------------------------------------------------------------------------------------- driver
def test_argument_parsing():
    a = D.parse_args([])
    assert (a.mode, a.n_beam, a.device, a.batch_size, a.max_steps) == ("forward", 5, "cuda", 32, 100) and not a.synthetic and not a.tiny
    a = D.parse_args(["--checkpoint", "c.pth", "--mode", "retro", "--n_beam", "1", "--device", "cpu", "--batch_size", "7", "--vocab_filename", "v.txt",
                      "--input", "i.txt", "--output", "o.csv", "--seed", "3", "--synthetic", "--tiny"])
    assert (a.checkpoint, a.mode, a.n_beam, a.device, a.batch_size, a.vocab_filename, a.input, a.output, a.seed) == \
        ("c.pth", "retro", 1, "cpu", 7, "v.txt", "i.txt", "o.csv", 3) and a.synthetic and a.tiny
    with pytest.raises(SystemExit):
        D.parse_args(["--mode", "sideways"])


def test_reaction_reader_and_accuracy(tmp_path):
    f = tmp_path / "r.txt"
    f.write_text("CCO.CC(=O)O\tCCOC(C)=O\n\nc1ccccc1\n  CC\tC  \nCN\t\n")
    src, tgt = D.read_reactions(str(f))
    assert src == ["CCO.CC(=O)O", "c1ccccc1", "CC", "CN"] and tgt == ["CCOC(C)=O", None, "C", None]
    # hand-made: reaction 0 right at rank 1, reaction 1 has no target (not counted), reaction 2 right at rank 3, reaction 3 wrong, 4 nothing returned
    targets = ["A", None, "B", "C", "D"]
    cands = [["A", "x"], ["q"], ["x", "y", "B"], ["x", "y", "z"], []]
    top1, topk = D.accuracy(targets, cands)
    assert top1 == 1 / 4 and topk == 2 / 4
    assert D.accuracy([None], [["a"]]) == (0.0, 0.0)
    top1, topk = D.accuracy(["a", "b"], [["A"], ["c", "B"]], canon=str.upper)        # a canonicaliser is applied to both sides
    assert (top1, topk) == (0.5, 1.0)
    out = tmp_path / "o.csv"
    D.write_csv(str(out), ["s1", "s2"], [["a", "b"], []], 3)
    assert out.read_text().splitlines() == ["source,candidate_1,candidate_2,candidate_3", "s1,a,b,", "s2,,,"]


def test_batches_are_restored_to_input_order_and_sources_truncated():
    class Tok:                                                                             # one token id per character after '[CLS]'
        pad_token_id = 0

        def encode(self, s, max_length=None):
            pieces = [2] + [10 + (ord(c) % 50) for c in s[5:]]                              # the text '[CLS]' is the first piece
            return [2] + pieces[: max_length - 2] + [3]

    lengths = [7, 3, 200, 3, 1, 12]
    sources = ["a" * n for n in lengths]
    seen = []

    def predict(model, ids, mask, k, max_steps):
        seen.append(tuple(ids.shape))
        assert torch.equal(mask, (ids != 0).long()) and int(mask[:, 0].min()) == 1 and bool((ids[:, 0] == 2).all())
        return [[(-float(j), [2, int(m.sum()), j, 3]) for j in range(k)] for m in mask]

    def greedy(model, ids, mask, max_steps):
        return [[2, int(m.sum()), 3] for m in mask]

    out = D.predict_all(None, Tok(), sources, 2, 4, predict=predict, greedy=greedy)
    ntok = [min(n + 2, D.MAX_SOURCE - 1) for n in lengths]                                 # '[CLS]' + pieces + [SEP]; max_length counts the dropped token
    assert [r[0][1] for r in out] == ntok and all(len(r) == 2 and r[1][2] == 1 for r in out)
    assert seen == [(4, 9), (2, 149)]
    out1 = D.predict_all(None, Tok(), sources, 1, 4, predict=predict, greedy=greedy)
    assert [r[0][1] for r in out1] == ntok and all(len(r) == 1 for r in out1)


def test_driver_refuses_the_cpu_with_the_products_message():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "rxn_predict.py"), "--synthetic", "--tiny", "--device", "cpu"], capture_output=True,
                       text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "no CPU / eager fallback" in r.stderr and "Traceback" not in r.stderr, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------------ baseline
def test_whole_prefix_baseline_on_the_cpu_restatement_equals_evaluate_beam():
    """predict_products(cached=False) -- the loop over `model.text_encoder2.bert` / `model.generate` -- on the CPU restatement's module API
    returns exactly what rxn_reference.evaluate_beam returns, scores included; greedy_products(cached=False) what evaluate returns."""
    from spmm_amd import decode
    c_dec = O.tiny_cfg().text
    c_enc = R.encoder_cfg(c_dec)
    sd = R.with_lm_bias(R.closed_form_state_dict(c_dec, c_enc), bias=R.ranked_lm_bias(c_dec.vocab_size, seed=23, k=3, margin=0.6))
    om = R.RxnModule(sd, c_dec, c_enc)
    g = torch.Generator().manual_seed(4)
    lens = [1, 5, 9]
    ids = torch.zeros(3, 9, dtype=torch.long)
    for n, L in enumerate(lens):
        ids[n, :L] = torch.randint(4, 300, (L,), generator=g)
    mask = (ids != 0).long()
    k, T = 3, 8
    got = decode.predict_products(om, ids, mask, k=k, max_steps=T)
    want = [R.evaluate_beam(sd, c_dec, c_enc, ids[n], mask[n], k, max_steps=T) for n in range(3)]
    assert got == want and any(len(h) > 0 for h in got)
    assert got != [R.evaluate_beam(sd, c_dec, c_enc, ids[n], mask[n], k, max_steps=T, need=k) for n in range(3)]
    greedy = decode.greedy_products(om, ids, mask, max_steps=T)
    assert greedy == [R.evaluate_oracle(sd, c_dec, c_enc, ids[n], mask[n], max_steps=T) for n in range(3)]
