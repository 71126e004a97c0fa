"""Seq2seq fine-tuning of the reaction model without a GPU: the oracle-side training loss (rxn_train_reference) against torch's
CrossEntropyLoss(ignore_index=0) and against the loss kernel's label rule restated in numpy, the new entry point in the header and its
wrapper, the launch sequence of a dry-run train_step (every call validated against the C ABI, none launched), the layout fall-backs, the
model API, the schedule cadence, the driver, and the kernel's argument refusals."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spmm_oracle as O
import rxn_reference as R
import rxn_train_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.fixture
def dry():
    from spmm_amd import ops
    old = ops._DRY_RUN
    ops._DRY_RUN = True
    yield ops
    ops._DRY_RUN = old


def _cfg(layers=2, f=1):
    from spmm_amd.config import BertConfig
    return BertConfig(hidden_size=128, num_attention_heads=2, intermediate_size=512, num_hidden_layers=layers, fusion_layer=f, encoder_width=128,
                      add_cross_attention=True)


def _trainable(c, **kw):
    from spmm_amd.rxn import SPMMRxn
    return SPMMRxn(bert_config=c, device="cpu", trainable=True, **kw)


# ------------------------------------------------------------------------------------------------------------------ the reference loss
def test_helper_loss_is_cross_entropy_ignoring_pad():
    oc = O.tiny_cfg().text
    oe = R.encoder_cfg(oc)
    sd = R.random_state_dict(oc, oe, seed=1)
    b = T.batch()
    with torch.no_grad():
        logits = T.logits(sd, oc, oe, *b)
        mine = T.ce_ignore0(logits, b[2])
        want = F.cross_entropy(logits[:, :-1].permute(0, 2, 1), b[2][:, 1:], ignore_index=0)       # SPMM_models_rxn.py:42-45
    assert abs(float(mine) - float(want)) <= 1e-6 * abs(float(want))
    lsd, names = T.leaves(sd, oc, oe)
    T.loss(lsd, oc, oe, *b).backward()
    assert sorted(n for n in names if lsd[n].grad is None) == sorted(n for n in T.UNTOUCHED if n in names)      # what no loss reaches


def _kernel_labels(ids, row_of, V):
    """The label rule of spmm_s2s_loss in numpy: row r is dense row d = row_of[r] (r when the rows are dense), t = d % L; the label is
    ids[d + 1] when t < L - 1; 0 and anything outside [0, V) is ignored (0)."""
    nseq, L = ids.shape
    flat = ids.reshape(-1)
    d = np.arange(nseq * L) if row_of is None else np.asarray(row_of)
    out = np.zeros(len(d), dtype=np.int64)
    for r, dr in enumerate(d):
        if dr % L < L - 1:
            lab = flat[dr + 1]
            out[r] = lab if 0 < lab < V else 0
    return out


def test_helper_label_rule_is_the_kernels_rule():
    _, _, prd, pmask = T.batch()
    ids = prd.numpy()
    want = T.labels(prd).numpy()                                                    # [B, L - 1]
    dense = _kernel_labels(ids, None, 300).reshape(ids.shape)
    assert (dense[:, :-1] == want).all() and not dense[:, -1].any()
    rows = np.flatnonzero(pmask.numpy().reshape(-1))                                # the pack plan's `rows`: dense row of every packed row
    packed = _kernel_labels(ids, rows, 300)
    assert len(rows) == 71 and int((packed != 0).sum()) == int((want != 0).sum()) == 63
    assert (packed == dense.reshape(-1)[rows]).all() and not dense.reshape(-1)[np.setdiff1d(np.arange(ids.size), rows)].any()
    assert not dense[0].any() and int(pmask[4].sum()) == int(pmask[7].sum()) == T.PROD_L      # a sequence without a label; two that end at L - 1


# ------------------------------------------------------------------------------------------------------------------ header, wrapper
def test_s2s_loss_is_declared_and_the_wrapper_matches(dry):
    from spmm_amd._lib import parse_header
    protos = parse_header()
    assert "spmm_s2s_loss" in protos and len(protos["spmm_s2s_loss"][1]) == 16
    ops = dry
    ops._dry_log.clear()
    logits = torch.zeros(71, 300)
    ids = torch.zeros(8 * 20, dtype=torch.int32)
    ws, losses = torch.zeros(4, dtype=torch.int32), torch.zeros(8)
    ops.s2s_loss(logits, ids, nseq=8, L=20, V=300, ws=ws, losses=losses, slot=0, row_of=torch.zeros(71, dtype=torch.int64),
                 dlogits=torch.zeros(71, 320, dtype=torch.bfloat16), gscale=torch.ones(1))
    ops.s2s_loss(torch.zeros(160, 300), ids, nseq=8, L=20, V=300, ws=ws, losses=losses, slot=0)
    assert ops._dry_log == ["spmm_s2s_loss", "spmm_s2s_loss"]
    with pytest.raises(AssertionError):
        ops.s2s_loss(logits, ids, nseq=8, L=20, V=300, ws=ws, losses=losses, slot=0)              # 71 rows are not the dense 160
    with pytest.raises(AssertionError):
        ops.s2s_loss(logits, ids, nseq=8, L=20, V=300, ws=ws, losses=losses, slot=0, row_of=torch.zeros(71, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the step, dry
@pytest.mark.parametrize("layers,f", [(2, 1), (4, 2)])
def test_train_step_launch_sequence_matches_the_header(dry, layers, f):
    ops = dry
    m = _trainable(_cfg(layers, f))
    b = T.batch()
    ops._dry_log.clear()
    loss = m.train_step(*b)
    n = collections.Counter(ops._dry_log)
    assert loss.shape == (1,)
    assert n["spmm_s2s_loss"] == 1 and n["spmm_lm_loss"] == 0                 # gscale is 1: the forward launch wrote dlogits
    assert n["spmm_attn_bwd"] == f + layers + (layers - f) == n["spmm_attn_fwd"]      # encoder layers + decoder layers + cross layers
    assert n["spmm_embed_bwd"] == 2 == n["spmm_embed_ln_fwd"] and n["spmm_adamw_step"] == 1 and n["spmm_pack_plan"] == 2
    assert n["spmm_segment_sum_bf16"] == layers - f                           # every cross layer folds its key/value gradient onto the source
    # the autograd path: the scale arrives with backward, which launches the loss kernel a second time
    ops._dry_log.clear()
    m(*b).backward()
    n = collections.Counter(ops._dry_log)
    assert n["spmm_s2s_loss"] == 2 and n["spmm_adamw_step"] == 0 and n["spmm_attn_bwd"] == 2 * layers
    assert all(m._parameters[k].grad is None for k in T.UNTOUCHED if k in m._parameters)
    assert m._parameters["text_encoder2.bert.embeddings.word_embeddings.weight"].grad is not None
    ops._dry_log.clear()
    with torch.no_grad():
        assert m(*b).shape == () and m.engine.tape is None and "spmm_attn_bwd" not in ops._dry_log


def test_layout_fallbacks_and_length_limit(dry):
    ops = dry
    m = _trainable(_cfg())
    src, sm, prd, pm = T.batch()

    def plans(*b):
        ops._dry_log.clear()
        m.train_step(*b)
        return ops._dry_log.count("spmm_pack_plan"), ops._dry_log.count("spmm_gather_rows2")
    assert plans(src, sm, prd, pm) == (2, 4)                                  # both packed: a gather in, a gather back, each
    holes = pm.clone()
    holes[3, 2] = 0
    assert plans(src, sm, prd, holes) == (1, 2)                               # a hole in a product mask: the product runs dense
    empty = sm.clone()
    empty[2] = 0
    assert plans(src, empty, prd, pm) == (1, 2)                               # an empty source row: the source runs dense
    full = T.batch(src_lens=(24,) * 8, prod_lens=(20,) * 8)
    assert plans(*full) == (0, 0)                                             # nothing to drop
    long_ids = torch.full((2, 257), 5)
    ones = torch.ones_like(long_ids)
    with pytest.raises(ValueError, match="256"):
        m.train_step(long_ids, ones, prd[:2], pm[:2])
    with pytest.raises(ValueError, match="256"):
        m(src[:2], sm[:2], long_ids, ones)


# ------------------------------------------------------------------------------------------------------------------ model API
def test_default_model_is_inference_only_and_trainable_has_the_arenas(dry):
    from spmm_amd.rxn import SPMMRxn
    c = _cfg()
    inf = SPMMRxn(bert_config=c, device="cpu")
    z = torch.zeros(1, 3, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="inference only"):
        inf(z, z + 1, z, z + 1)
    assert not hasattr(inf.store, "grad") and not any(p.requires_grad for p in inf.parameters())
    with pytest.raises(RuntimeError, match="trainable=True"):
        inf.configure_optimizers()
    m = _trainable(c)
    st = m.store
    assert st.grad.numel() == st.adam_m.numel() == st.adam_v.numel() == st.total and all(p.requires_grad for p in m.parameters())
    assert list(m.state_dict()) == list(inf.state_dict()) and [tuple(v.shape) for v in m.state_dict().values()] == [tuple(v.shape) for v in inf.state_dict().values()]
    assert m.options.ln_from_y is False and inf.options.ln_from_y is True
    # the fused AdamW steps the arena in front of the parameters no loss reaches
    n = m._stepped_numel()
    tail = [k for k in st.order if st.offset[k] >= n]
    assert sorted(tail) == sorted(k for k in T.UNTOUCHED if k in st.offset) and m.optimizers().numel == n < st.total
    assert m.optimizers().param_groups[0]["weight_decay"] == 0.02 and m.optimizers().max_norm == float("inf")
    s = m.lr_schedulers().s
    assert (s["lr"], s["min_lr"], s["warmup_lr"], s["warmup_epochs"]) == (1e-4, 5e-6, 1e-5, 1)      # d_rxn_prediction.py:276-278
    assert m.train() is m and m.engine.train_mode and m.eval() is m and not m.engine.train_mode
    assert inf.train() is inf and not inf._engine.train_mode


def test_training_step_schedule_over_two_epochs(dry):
    """d_rxn_prediction.py train(): scheduler.step(i // 100) every 100 iterations of epoch 0 through the warm-up, scheduler.step(epoch +
    warmup + 1) after every epoch -- against _CosineSchedule."""
    from spmm_amd.model import _CosineSchedule
    sched = {"sched": "cosine", "lr": 1e-3, "epochs": 5, "min_lr": 1e-5, "decay_rate": 1, "warmup_lr": 1e-4, "warmup_epochs": 2, "cooldown_epochs": 0}
    m = _trainable(_cfg(), config={"optimizer": {"lr": 1e-3, "weight_decay": 0.02}, "schedular": sched})
    sch = _CosineSchedule(sched)
    ids = torch.full((2, 6), 5)
    pair = (ids, torch.ones_like(ids))
    lr = lambda: m.optimizers().param_groups[0]["lr"]
    assert m.STEP_SIZE == 100 and lr() == pytest.approx(sch.lr_at(0))
    seen, n_batches = [], 210
    for epoch in range(2):
        for i in range(n_batches):
            m.training_step((pair, pair), i)
            seen.append(lr())
        m.on_train_epoch_end()
        assert lr() == pytest.approx(sch.lr_at(epoch + 2 + 1))
    expect, cur = [], sch.lr_at(0)
    for epoch in range(2):
        if epoch == 1:
            cur = sch.lr_at(0 + 2 + 1)
        for i in range(n_batches):
            if epoch == 0 and i % 100 == 0 and i <= 200:
                cur = sch.lr_at(i // 100)
            expect.append(cur)
    assert seen == pytest.approx(expect) and m.global_step == 2 * n_batches and m.current_epoch == 2


# ------------------------------------------------------------------------------------------------------------------ driver
def test_driver_help_lists_the_reference_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "rxn_finetune.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0
    for flag in ("--output_dir", "--checkpoint", "--mode", "--n_beam", "--device", "--lr", "--min_lr", "--epoch", "--batch_size", "--train", "--valid",
                 "--test", "--vocab_filename", "--seed", "--max_steps", "--synthetic", "--tiny"):
        assert flag in r.stdout
    import rxn_finetune as D
    a = D.parse_args([])
    assert (a.output_dir, a.mode, a.n_beam, a.device, a.lr, a.min_lr, a.epoch, a.batch_size) == ("./output/RXN", "forward", 5, "cuda", 1e-4, 5e-6, 300, 16)


def test_driver_synthetic_dry_run_writes_a_loadable_checkpoint(dry, tmp_path):
    import rxn_finetune as D
    from spmm_amd.rxn import SPMMRxn
    from spmm_amd.config import tiny_config
    out = str(tmp_path / "rxn")
    D.main(D.parse_args(["--synthetic", "8", "--tiny", "--epoch", "1", "--batch_size", "4", "--output_dir", out, "--device", "cpu"]))
    ck = torch.load(os.path.join(out, "checkpoint_best.pth"), map_location="cpu")
    assert {"state_dict", "config", "epoch"} <= set(ck) and ck["config"]["schedular"]["warmup_lr"] == 1e-5 and ck["global_step"] == 2
    inf = SPMMRxn(bert_config=tiny_config().text, device="cpu")
    res = inf.load_pretrained(os.path.join(out, "checkpoint_best.pth"))
    assert res.missing_keys == []
    assert list(ck["state_dict"]) == list(inf.state_dict())
    # batches: file order, the last incomplete one dropped, sources cut at 150 tokens and products at 100 with the leading token dropped
    class Tok:                                                                             # one token id per character after '[CLS]'
        pad_token_id = 0

        def encode(self, s, max_length=None):
            pieces = [2] + [10 + (ord(c) % 50) for c in s[5:]]                              # the text '[CLS]' is the first piece
            return [2] + pieces[: max_length - 2] + [3]

    src, tgt = ["a" * n for n in (3, 400, 5, 7, 9)], ["b" * n for n in (2, 3, 300, 4, 6)]
    got = list(D.train_batches(Tok(), src, tgt, 2))
    assert len(got) == 2 and got[0][0][0].shape == (2, 149) and got[1][1][0].shape == (2, 99)
    assert bool((got[0][0][0][:, 0] == R.CLS_ID).all()) and bool((got[1][1][0][:, 0] == R.CLS_ID).all())


# ------------------------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def built():
    so = os.path.join(ROOT, "spmm_amd", "libspmm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return so


def _s2s_args(**kw):
    a = dict(logits=64, ldl=300, ids=64, row_of=None, rows=160, nseq=8, L=20, V=300, ws=64, gscale=None, dlogits=64, ldd=320, Vpad=320, losses=64,
             slot=0)
    a.update(kw)
    return tuple(a.values()) + (None,)


def test_s2s_loss_validates_its_arguments_without_touching_the_gpu(built):
    """Every refusal happens before the launch (the non-null pointers here are never dereferenced) and names the entry point."""
    from spmm_amd._lib import lib
    L = lib()
    for kw, msg in ((dict(V=321), "V=321 Vpad=320"), (dict(L=1, rows=8), "L=1"), (dict(rows=0), "rows=0"), (dict(rows=161), "rows=161"),
                    (dict(ws=None), "workspace"), (dict(ws=68), "8-byte aligned"), (dict(ldl=299), "ldl=299"), (dict(ldd=300), "ldd=300"),
                    (dict(ids=None), "are required")):
        with pytest.raises(RuntimeError, match="spmm_s2s_loss.*" + msg):
            L.call("spmm_s2s_loss", *_s2s_args(**kw))
