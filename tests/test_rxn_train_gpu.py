"""Seq2seq fine-tuning of the reaction model (spmm_amd/rxn_step.py, SPMMRxn(trainable=True)) on the GPU: loss and whole gradient against the
oracle's autograd (rxn_train_reference: SPMM_rxn.forward on oracle.bert_model / mlm_head), the autograd path against train_step, training
runs against torch.optim.AdamW on the oracle, the parameters no loss reaches, dropout, a wrong token-count hint, the hand-off to the
searches, the published size and the two drivers end to end.

Configuration unless a test says otherwise: H = 128, 2 heads, I = 512, no dropout, weights from rxn_reference.random_state_dict; B = 8,
source lengths (1, 3, 7, 16, 17, 24, 9, 24) in L = 24, product lengths (1, 2, 5, 12, 20, 8, 3, 20) in L = 20."""
import math
import os
import subprocess
import sys

import pytest
import torch

import rxn_reference as R
import rxn_train_reference as T
from test_finetune_gpu import _assert_track, _grad_check, _trained_like_ln

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED = {"sched": "cosine", "lr": 2e-4, "epochs": 4, "min_lr": 1e-5, "decay_rate": 1, "warmup_lr": 5e-5, "warmup_epochs": 1, "cooldown_epochs": 0}


@pytest.fixture(scope="module")
def O():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import spmm_oracle
    return spmm_oracle


def _cfgs(O, layers=2, f=1, dropout=0.0, H=128, nH=2, I=512):
    from spmm_amd.config import BertConfig
    c = BertConfig(hidden_size=H, num_attention_heads=nH, intermediate_size=I, num_hidden_layers=layers, fusion_layer=f, encoder_width=H,
                   add_cross_attention=True, hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout)
    oc = O.BertCfg(hidden_size=H, num_attention_heads=nH, intermediate_size=I, num_hidden_layers=layers, fusion_layer=f, encoder_width=H,
                   hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    return c, oc, R.encoder_cfg(oc)


def _model(c, sd, trainable=True, **kw):
    from spmm_amd.rxn import SPMMRxn
    m = SPMMRxn(bert_config=c, trainable=trainable, **kw)
    m.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    return m


def _loss_gate(got, ref, tag=""):
    print(f"{tag}: loss hip {got:.6f} oracle {ref:.6f}")
    assert abs(got - ref) <= 1e-2 * abs(ref) + 1e-3, tag


# ------------------------------------------------------------------------------------------------ 1. loss and whole gradient
@pytest.mark.parametrize("variant", ["varied", "trained_ln", "full_length"])
@pytest.mark.parametrize("layers,f", [(2, 1), (4, 2)])
def test_loss_and_gradient_match_the_oracle(O, layers, f, variant):
    c, oc, oe = _cfgs(O, layers, f)
    sd = R.random_state_dict(oc, oe, seed=1)
    if variant == "trained_ln":
        sd = _trained_like_ln(sd)
    b = T.batch() if variant != "full_length" else T.batch(src_lens=(24,) * 8, prod_lens=(20,) * 8)
    m = _model(c, sd).train()
    loss = m(*b)
    loss.backward()
    assert (int(b[3].sum()) < b[3].numel()) == (variant != "full_length")        # varied lengths: the packed layout; full length: the dense one
    lsd, names = T.leaves(sd, oc, oe)
    ref = T.loss(lsd, oc, oe, *b)
    ref.backward()
    tag = f"{layers} layers f={f} {variant}"
    _loss_gate(float(loss), float(ref), tag)
    reached = [n for n in names if lsd[n].grad is not None]
    assert sorted(set(names) - set(reached)) == sorted(n for n in T.UNTOUCHED if n in names)
    _grad_check(m, lsd, reached, tag)
    for n in set(names) - set(reached):                  # what the loss does not reach: no gradient on either side
        assert not m.store.g(n).any() and m._parameters[n].grad is None, n


# ------------------------------------------------------------------------------------------------ 2. the reference's loop against train_step
def test_autograd_path_and_train_step_agree(O):
    c, oc, oe = _cfgs(O)
    sd = R.random_state_dict(oc, oe, seed=1)
    b = T.batch()
    lr, wd = 2e-4, 0.02
    m1 = _model(c, sd, config={"optimizer": {"lr": lr, "weight_decay": wd}, "schedular": dict(SCHED, warmup_lr=lr)}).train()
    a = [float(m1.train_step(*b)) for _ in range(2)]
    m2 = _model(c, sd).train()
    opt = torch.optim.AdamW(m2.parameters(), lr=lr, weight_decay=wd)
    bb = []
    for _ in range(2):
        loss = m2(*b)
        opt.zero_grad()
        loss.backward()
        opt.step()
        bb.append(float(loss))
    print("train_step", a, "autograd + torch.optim.AdamW", bb)
    assert a[0] == bb[0]                                 # the same forward launches
    assert abs(a[1] - bb[1]) <= 0.02 + 0.05 * abs(bb[1]) and a[1] < a[0] and bb[1] < bb[0]
    assert all(m2._parameters[n].grad is None for n in T.UNTOUCHED if n in m2._parameters)


# ------------------------------------------------------------------------------------------------ 3. twenty steps
def test_twenty_steps_track_torch_adamw(O):
    from spmm_amd.model import _CosineSchedule
    c, oc, oe = _cfgs(O)
    sd0 = R.random_state_dict(oc, oe, seed=1)
    batches, per_epoch = [T.batch(seed=s) for s in range(20)], 10
    lsd, names = T.leaves(sd0, oc, oe)
    opt = torch.optim.AdamW([lsd[n] for n in names if n not in T.UNTOUCHED], lr=SCHED["lr"], weight_decay=0.02)      # what the loss reaches
    sch = _CosineSchedule(SCHED)
    ref = []
    for i, b in enumerate(batches):
        epoch, bi = divmod(i, per_epoch)
        if bi == 0:
            for gp in opt.param_groups:
                gp["lr"] = sch.lr_at(0) if epoch == 0 else sch.lr_at(epoch + SCHED["warmup_epochs"])
        opt.zero_grad()
        loss = T.loss(lsd, oc, oe, *b)
        loss.backward()
        opt.step()
        ref.append(float(loss))
    m = _model(c, sd0, config={"optimizer": {"lr": SCHED["lr"], "weight_decay": 0.02}, "schedular": SCHED}).train()
    got = []
    for i, b in enumerate(batches):
        bi = i % per_epoch
        if i and bi == 0:
            m.on_train_epoch_end()
        got.append(float(m.training_step((b[:2], b[2:]), bi)))
    _assert_track(got, ref, "fused")
    assert m.optimizers().param_groups[0]["lr"] == pytest.approx(sch.lr_at(2))


# ------------------------------------------------------------------------------------------------ 4. parameters no loss reaches
def test_untouched_parameters_stay_bit_identical(O):
    c, oc, oe = _cfgs(O)
    sd = R.random_state_dict(oc, oe, seed=1)
    m = _model(c, sd).train()
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for s in range(3):
        m.train_step(*T.batch(seed=s))
    torch.cuda.synchronize()
    after = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for n in T.UNTOUCHED:
        assert torch.equal(after[n], before[n]) and torch.equal(after[n], sd[n]), n
        base = n.replace("decoder.bias", "bias")
        for arena in (m.store.adam_m, m.store.adam_v, m.store.grad):
            assert not m.store._view(arena, base).any(), n
    for n in ("text_encoder2.bert.encoder.layer.0.output.dense.weight", "text_encoder.cls.predictions.bias", "text_encoder.bert.embeddings.word_embeddings.weight"):
        assert not torch.equal(after[n], before[n]), n
    assert int(m.optimizers().step_count) == 3


# ------------------------------------------------------------------------------------------------ 5. dropout
def test_dropout_follows_mode_and_seed(O):
    c, oc, oe = _cfgs(O, dropout=0.1)
    sd = R.random_state_dict(oc, oe, seed=1)
    b = T.batch()
    m = _model(c, sd).train()
    seed0 = m.engine.seed.clone()
    with torch.no_grad():
        l1, l2 = float(m(*b)), float(m(*b))
        m.engine.seed.copy_(seed0)
        again = float(m(*b))
        m.eval()
        ev = [float(m(*b)) for _ in range(2)]
    c0, _, _ = _cfgs(O, dropout=0.0)
    with torch.no_grad():
        plain = float(_model(c0, sd).train()(*b))
    print("train", l1, l2, "again", again, "eval", ev, "no dropout", plain)
    assert l1 != l2 and again == l1 and ev[0] == ev[1] == plain


# ------------------------------------------------------------------------------------------------ 6. a wrong token-count hint
@pytest.mark.parametrize("delta", [-7, 9])
def test_wrong_product_token_hint_is_a_skipped_step(O, delta):
    from spmm_amd import ops
    c, oc, oe = _cfgs(O)
    b = T.batch()
    true, (B, L) = int(b[3].sum()), b[3].shape
    M = true + delta
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    pk = ops.pack_plan(b[3].to(torch.int32).cuda().contiguous(), M, bad)
    torch.cuda.synchronize()
    r0, ln = pk["row0"].long(), pk["len"].long()
    assert int(bad) == 1 and bool((r0 >= 0).all()) and bool((ln >= 1).all()) and bool((r0 + ln <= M).all())
    assert bool(((pk["rows"] >= 0) & (pk["rows"] < B * L)).all()) and bool(((pk["inv"][:B * L] >= -1) & (pk["inv"][:B * L] < M)).all())
    m = _model(c, R.random_state_dict(oc, oe, seed=1)).train()
    m.train_step(*b)                                     # a normal step first
    torch.cuda.synchronize()
    flat0, am0, av0, cnt0 = m.store.flat.clone(), m.store.adam_m.clone(), m.store.adam_v.clone(), int(m.optimizers().step_count)
    m.train_step(*b, n_prod_tokens=M)
    torch.cuda.synchronize()
    assert int(m.engine.nan_flag) != 0 and int(m.engine.hint_bad) == 1
    assert torch.equal(m.store.flat, flat0) and torch.equal(m.store.adam_m, am0) and torch.equal(m.store.adam_v, av0)
    assert int(m.optimizers().step_count) == cnt0
    loss = float(m.train_step(*b))                       # nothing sticky: the next step runs
    assert math.isfinite(loss) and int(m.engine.nan_flag) == 0 and not torch.equal(m.store.flat, flat0)


# ------------------------------------------------------------------------------------------------ 7. hand-off to inference
def test_trained_model_hands_its_weights_to_the_searches(O):
    from spmm_amd import decode
    c, oc, oe = _cfgs(O)
    m = _model(c, R.random_state_dict(oc, oe, seed=1)).train()
    b = T.batch()
    for s in range(5):
        m.train_step(*T.batch(seed=s))
    m.eval()
    with torch.no_grad():
        ev = float(m(*b))
    fresh = _model(c, m.state_dict(), trainable=False).eval()
    src, sm, prd, pm = b
    mine = decode.greedy_products(m, src, sm, max_steps=12)
    theirs = decode.greedy_products(fresh, src, sm, max_steps=12)
    assert mine == theirs and len(mine) == 8 and len({tuple(h) for h in mine}) > 1
    emb = fresh.text_encoder2.bert(src, attention_mask=sm, return_dict=True, mode="text").last_hidden_state
    logits = fresh.text_encoder(prd, attention_mask=pm, encoder_hidden_states=emb, encoder_attention_mask=sm, return_dict=True, is_decoder=True,
                                return_logits=True)
    _loss_gate(float(T.ce_ignore0(logits.float().cpu(), prd)), ev, "facades of the reloaded model vs the trainable model's eval loss")
    # a torch optimiser stepping the parameter views is seen by the next search too (the shadow refresh)
    opt = torch.optim.AdamW(m.parameters(), lr=5e-3)
    m.train()
    m(*b).backward()
    opt.step()
    m.eval()
    moved = _model(c, m.state_dict(), trainable=False).eval()
    assert decode.greedy_products(m, src, sm, max_steps=12) == decode.greedy_products(moved, src, sm, max_steps=12)


# ------------------------------------------------------------------------------------------------ 8. published size
def test_published_size_eval_loss_matches_the_fp32_oracle(O):
    c, oc, oe = _cfgs(O, layers=12, f=6, H=768, nH=12, I=3072)
    sd = R.random_state_dict(oc, oe, seed=11, std=0.05)
    b = T.batch(src_lens=(40, 150, 77, 113), prod_lens=(20, 100, 57, 81), src_L=150, prod_L=100)
    with torch.no_grad():
        ref = float(T.loss(sd, oc, oe, *b))
        with O.bf16_storage():                           # the oracle with the product's bf16 stores: the budget bf16 alone explains
            ref_bf = float(T.loss(sd, oc, oe, *b))
    dev = abs(ref_bf - ref)
    bound = max(2.0 * dev, 1e-3)
    m = _model(c, sd).eval()
    with torch.no_grad():
        got = float(m(*b))
    print(f"published size: oracle {ref:.6f}, bf16 storage model {ref_bf:.6f} (deviation {dev:.3g}), bound {bound:.3g}; hip {got:.6f} "
          f"(off by {abs(got - ref):.3g})")
    assert abs(got - ref) <= bound


# ------------------------------------------------------------------------------------------------ 9. the drivers
def test_drivers_end_to_end(O, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = str(tmp_path / "rxn")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "rxn_finetune.py"), "--synthetic", "16", "--tiny", "--epoch", "1", "--n_beam", "1",
                        "--output_dir", out], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    ck = os.path.join(out, "checkpoint_best.pth")
    assert os.path.exists(ck) and "SAVING" in r.stdout and "mean loss" in r.stdout, r.stdout
    saved = torch.load(ck, map_location="cpu")
    assert {"state_dict", "config", "epoch"} <= set(saved) and "text_encoder2.bert.embeddings.word_embeddings.weight" in saved["state_dict"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "rxn_predict.py"), "--checkpoint", ck, "--synthetic", "--tiny", "--n_beam", "3",
                        "--output", str(tmp_path / "c.csv")], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and f"load checkpoint from {ck} (missing 0" in r.stdout and "Candidates are saved" in r.stdout, r.stdout + r.stderr
