"""`SPMMRxn` -- drop-in for the reference's reaction-prediction model `SPMM_rxn` (SPMM_models_rxn.py): forward synthesis (USPTO-480k) and
retrosynthesis (USPTO-50k) by greedy or k-beam decoding of the product SMILES against the encoded reactant SMILES, and -- opt-in,
`SPMMRxn(..., trainable=True)` -- the seq2seq fine-tuning that produces such a model.

Same constructor (`cp=None, config=None`), same state_dict keys ([out,in] fp32 layout: config.rxn_spec), the sub-modules the evaluation
loops call -- `model.text_encoder2.bert(ids, attention_mask=, mode='text')`, `model.text_encoder(...)`, `model.generate(...)` -- as
facades on the engine.  The searches themselves are spmm_amd.decode.predict_products / greedy_products (K/V cache, masked-memory
cross-attention, one-launch beam step); the facades are their whole-prefix baseline.  The default model is inference only (no gradient or
Adam arenas; `forward` raises).  With `trainable=True` the engine is spmm_amd.rxn_step.RxnStep: `forward` returns the teacher-forced loss
behind an autograd boundary, so the training loop of d_rxn_prediction.py (`loss.backward()`, `torch.optim.AdamW(model.parameters())`) runs
unchanged, and `train_step` is the same step with the fused arena AdamW on the device.  There is no eager / CPU fallback."""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional

import torch
from torch import nn

from . import ops
from .config import BertConfig, SPMMConfig, is_buffer, rxn_encoder_config, rxn_spec
from .engine import Engine, host_token_count
from .model import _CosineSchedule, _FusedAdamW
from .options import EngineOptions
from .params import ParamStore
from .rxn_step import RxnStep

# d_rxn_prediction.py:276-278 at the script's default arguments (optimizer: AdamW(lr, weight_decay=0.02), no clipping)
DEFAULT_SCHED = {"sched": "cosine", "lr": 1e-4, "epochs": 300, "min_lr": 5e-6, "decay_rate": 1, "warmup_lr": 1e-5, "warmup_epochs": 1,
                 "cooldown_epochs": 0}
# What no loss reaches: the reactant encoder's MLM head is part of the state and never used (SPMM_models_rxn.py:34 calls text_encoder2.bert
# only), so autograd leaves these parameters with grad None and torch.optim.AdamW skips them, weight decay included.  They are the last
# entries of rxn_spec, i.e. the tail of the arena: the fused AdamW steps the range in front of them (`_FusedAdamW(numel=...)`).
UNTOUCHED_PREFIX = "text_encoder2.cls.predictions."

DROPPED = ("queue", "property", "_m")          # d_rxn_prediction.py:192-194: keys of a pretraining checkpoint the model has no use for


def map_checkpoint(sd: dict) -> "OrderedDict[str, torch.Tensor]":
    """A checkpoint's state dict as the reaction model loads it (SPMM_models_rxn.py:16-29, then d_rxn_prediction.py:192-200): keys that
    contain `queue`, `property` or `_m` are dropped and `_unk` is renamed `_mask`; every `text_encoder.*` tensor is offered to
    `text_encoder2.*` too (the reactant encoder starts as the pretrained SMILES encoder; what it has no slot for -- layers fusion_layer..,
    cross-attention -- is ignored by the non-strict load), unless the checkpoint holds that `text_encoder2.*` key itself (a fine-tuned one)."""
    kept = OrderedDict()
    for key, v in sd.items():
        if any(d in key for d in DROPPED):
            continue
        kept[key.replace("_unk", "_mask")] = v
    out = OrderedDict(kept)
    for key, v in kept.items():
        if key.startswith("text_encoder."):
            out.setdefault("text_encoder2." + key[len("text_encoder."):], v)
    return out


class _RxnStepFn(torch.autograd.Function):
    """Autograd boundary (as finetune._FinetuneStepFn): the loss is a function of every parameter; backward runs the engine's backward with
    the incoming loss gradient as the device-side scale and hands back views of a copy of the flat gradient arena."""

    @staticmethod
    def forward(ctx, model, sids, smask, pids, pmask, hints, *params):
        loss = model._engine.forward(sids, smask, pids, pmask, n_src_tokens=hints[0], n_prod_tokens=hints[1])
        ctx.model = model
        return loss.reshape(()).clone()

    @staticmethod
    def backward(ctx, g):
        m = ctx.model
        m._engine.gscale[0:1].copy_(g.reshape(1).to(torch.float32))
        ops.zero_(m.store.grad)
        m._engine.backward()
        # (a copy: autograd may keep a returned tensor as .grad, and the next backward rewrites the arena in place)
        g_all = m.store.grad.clone()
        return (None,) * 6 + tuple(None if n.startswith(UNTOUCHED_PREFIX) else m.store._view(g_all, n) for n in m._param_names)


class SPMMRxn(nn.Module):
    STEP_SIZE = 100           # warm-up schedule cadence of the script's train() (d_rxn_prediction.py:33)

    def __init__(self, cp=None, config=None, device=None, options: Optional[EngineOptions] = None, bert_config: Optional[BertConfig] = None,
                 bert_config_smiles: Optional[BertConfig] = None, trainable: bool = False, tokenizer=None):
        super().__init__()
        if not torch.cuda.is_available() and not ops._DRY_RUN:
            raise RuntimeError("spmm_amd.SPMMRxn needs an MI355X (HIP device); there is no CPU fallback")
        self.trainable, self.tokenizer = bool(trainable), tokenizer
        # a trainable model starts from trained LayerNorms: their backward reads the stored pre-norm sum (finetune.py)
        self.options = options if options is not None else (EngineOptions.from_env(ln_from_y=False) if trainable else EngineOptions.from_env())
        self.config = config
        if device is None:
            device = "cpu" if ops._DRY_RUN else f"cuda:{torch.cuda.current_device()}"
        self.device_ = torch.device(device)
        c_dec = bert_config if bert_config is not None else BertConfig.from_json_file(config["bert_config_text"])
        if bert_config_smiles is not None:
            c_enc = bert_config_smiles
        elif config is not None and config.get("bert_config_smiles"):
            c_enc = BertConfig.from_json_file(config["bert_config_smiles"])
        else:
            c_enc = rxn_encoder_config(c_dec)
        if c_enc.hidden_size != c_dec.encoder_width or c_enc.fusion_layer > c_enc.num_hidden_layers:
            raise ValueError("the reactant encoder's hidden size must be the decoder's encoder_width, its fusion_layer <= its layers")
        self.cfg, self.cfg_enc = SPMMConfig(text=c_dec), c_enc
        self.store = ParamStore(self.cfg, self.device_, train=self.trainable, spec=rxn_spec(c_dec, c_enc))
        if self.trainable:
            self._engine = RxnStep(self.cfg, self.store, self.device_, c_enc, self.options)
        else:
            self._engine = Engine(self.cfg, self.store, self.device_, self.options)
            self._engine.train_mode = False
        self._param_names = []
        for name, t in self.store.named_tensors():
            if is_buffer(name):
                self._buffers[name] = t
            elif self.store.kind[name] not in ("tied_w", "tied_b"):              # (aliases: part of state_dict() only)
                self._parameters[name] = nn.Parameter(t, requires_grad=self.trainable)
                self._param_names.append(name)
        self._shadow_version = None
        self.current_epoch = self.global_step = 0
        self._optimizer = self._scheduler = None
        self._init_weights()
        from .facade import BertFacade, MaskedLMFacade
        object.__setattr__(self, "text_encoder", MaskedLMFacade(self, "text_encoder.", c_dec))
        enc = MaskedLMFacade(self, "text_encoder2.", c_enc)
        enc.bert = BertFacade(self, "text_encoder2.bert.", c_enc, False)          # no cross-attention in the reactant encoder
        object.__setattr__(self, "text_encoder2", enc)
        if cp:
            self.load_pretrained(cp)

    # ---- init: BertForMaskedLM._init_weights (xbert.py:742-752) ----------------------------------------------------------------
    @torch.no_grad()
    def _init_weights(self):
        st = self.store
        g = torch.Generator(device="cpu").manual_seed(torch.initial_seed() % (2 ** 31))
        for name, shape, kind in st.spec:
            if is_buffer(name) or kind in ("tied_w", "tied_b"):
                continue
            t = st.w(name)
            if kind in ("emb", "lin_w"):
                t.copy_(torch.randn(shape, generator=g) * self.cfg.text.initializer_range)
            elif kind == "ln_w":
                t.fill_(1.0)
            else:
                t.zero_()
        self._refresh()

    # ---- shadows ---------------------------------------------------------------------------------------------------------------------
    def _refresh(self):
        """bf16 shadows <- fp32 masters; remembers the arena's version so that a later in-place update from outside (a torch optimiser
        stepping the parameter views) is seen by the next forward or search."""
        self._engine.pre_backward_wait()
        self.store.refresh_shadows()
        self.store.refresh_padded_shadows()
        self._shadow_version = self.store.flat._version

    def _sync_shadows(self):
        if self.store.flat._version != self._shadow_version:
            self._refresh()

    @property
    def engine(self):
        """The engine, with its bf16 shadows current: whatever runs on it -- the step, `generate`, the facades, the searches of
        spmm_amd.decode -- fetches it here and so sees the weights of the last optimiser step, a torch optimiser's included (the fused
        AdamW writes the shadows itself and leaves the version alone)."""
        if self.trainable:
            self._sync_shadows()
        return self._engine

    # ---- the reference's API -------------------------------------------------------------------------------------------------------
    def forward(self, text_input_ids=None, text_attention_mask=None, product_input_ids=None, product_attention_mask=None, *,
                n_src_tokens: Optional[int] = None, n_prod_tokens: Optional[int] = None):
        """trainable=True: SPMM_rxn.forward (SPMM_models_rxn.py:31-46), the mean next-token cross-entropy of the product with PAD targets
        ignored, as a 0-dim tensor; `loss.backward()` fills .grad of the parameters the loss reaches.  Under torch.no_grad(): the loss
        without a tape.  One deviation: a batch without a single target gives 0, not the reference's 0 / 0."""
        if not self.trainable:
            raise NotImplementedError("spmm_amd.SPMMRxn is inference only unless built with trainable=True: load a fine-tuned checkpoint and use "
                                      "generate / spmm_amd.decode.predict_products / greedy_products, or construct SPMMRxn(..., trainable=True) "
                                      "for seq2seq fine-tuning (SPMM_rxn.forward, the training loop of d_rxn_prediction.py)")
        eng = self.engine
        eng.train_mode = self.training
        if n_src_tokens is None:
            n_src_tokens = host_token_count(text_attention_mask)
        if n_prod_tokens is None:
            n_prod_tokens = host_token_count(product_attention_mask)
        t = [eng.to_device(x) for x in (text_input_ids, text_attention_mask, product_input_ids, product_attention_mask)]
        if torch.is_grad_enabled():
            return _RxnStepFn.apply(self, *t, (n_src_tokens, n_prod_tokens), *[self._parameters[n] for n in self._param_names])
        return eng.forward(*t, save=False, n_src_tokens=n_src_tokens, n_prod_tokens=n_prod_tokens).reshape(()).clone()

    # ---- optimiser and schedule (d_rxn_prediction.py:205-209: optim.AdamW(lr, weight_decay=0.02), no clipping, create_scheduler) -------
    def _stepped_numel(self) -> int:
        st = self.store
        n = min(st.offset[name] for name in st.order if name.startswith(UNTOUCHED_PREFIX))
        assert all(name.startswith(UNTOUCHED_PREFIX) == (st.offset[name] >= n) for name in st.order)      # they are the arena's tail
        return n

    def configure_optimizers(self):
        if not self.trainable:
            raise RuntimeError("SPMMRxn(..., trainable=True) has an optimiser; this model is inference only")
        cfg = self.config or {}
        o = cfg.get("optimizer", {})
        sched = dict(cfg.get("schedular", DEFAULT_SCHED))
        opt = _FusedAdamW(self.store, self._engine, lr=o.get("lr", sched["lr"]), weight_decay=o.get("weight_decay", 0.02), max_norm=math.inf,
                          numel=self._stepped_numel())
        sch = _CosineSchedule(sched)
        opt.param_groups[0]["lr"] = sch.lr_at(0)            # Scheduler.__init__ installs the warm-up start value
        self._optimizer, self._scheduler = opt, sch
        return [opt], [sch]

    def optimizers(self):
        if self._optimizer is None:
            self.configure_optimizers()
        return self._optimizer

    def lr_schedulers(self):
        if self._scheduler is None:
            self.configure_optimizers()
        return self._scheduler

    def train_step(self, text_input_ids, text_attention_mask, product_input_ids, product_attention_mask, *, n_src_tokens: Optional[int] = None,
                   n_prod_tokens: Optional[int] = None):
        """zero_grad -> forward -> backward -> AdamW, all on the device.  Returns the device loss [1].  Host tensors are copied through pinned
        memory without blocking and the packed row counts come from the host masks (or the hints), so the step reads nothing back from the
        device; with device masks and no hints each pack plan reads its count back once."""
        opt, eng = self.optimizers(), self.engine
        eng.train_mode = self.training
        eng.gscale.fill_(1.0)
        if n_src_tokens is None:
            n_src_tokens = host_token_count(text_attention_mask)
        if n_prod_tokens is None:
            n_prod_tokens = host_token_count(product_attention_mask)
        ops.zero_(self.store.grad)
        t = [eng.to_device(x) for x in (text_input_ids, text_attention_mask, product_input_ids, product_attention_mask)]
        loss = eng.forward(*t, n_src_tokens=n_src_tokens, n_prod_tokens=n_prod_tokens, grad_in_forward=True)
        eng.backward()
        opt.step()
        return loss

    def training_step(self, batch, batch_idx):
        """One iteration of the script's train() (d_rxn_prediction.py:38-51): `batch` = (reactants, products), each a SMILES list (needs
        `tokenizer`) or an (ids, mask) pair with the leading token already dropped.  The schedule steps every STEP_SIZE iterations through
        the warm-up of epoch 0; `on_train_epoch_end` steps it after each epoch."""
        pairs = []
        for text, max_len in zip(batch[:2], (150, 100)):
            if isinstance(text, (tuple, list)) and len(text) == 2 and torch.is_tensor(text[0]):
                pairs.append(tuple(text))
            else:
                ti = self.tokenizer(list(text), padding="longest", truncation=True, max_length=max_len, return_tensors="pt")
                pairs.append((ti.input_ids[:, 1:], ti.attention_mask[:, 1:]))
        loss = self.train_step(*pairs[0], *pairs[1])
        sch, opt = self.lr_schedulers(), self.optimizers()
        warm = sch.s["warmup_epochs"]
        if self.current_epoch == 0 and batch_idx % self.STEP_SIZE == 0 and batch_idx <= warm * self.STEP_SIZE:
            opt.param_groups[0]["lr"] = sch.lr_at(batch_idx // self.STEP_SIZE)
        self.global_step += 1
        return loss

    def on_train_epoch_end(self):
        """lr_scheduler.step(epoch + warmup_steps + 1) after each epoch (d_rxn_prediction.py:249)."""
        sch = self.lr_schedulers()
        self.optimizers().param_groups[0]["lr"] = sch.lr_at(self.current_epoch + sch.s["warmup_epochs"] + 1)
        self.current_epoch += 1

    @torch.no_grad()
    def generate(self, text_embeds, text_mask, product_input, stochastic=False, k=None):
        """SPMM_models_rxn.py:48-69 on the facades: the causal decoder on the whole prefix `product_input` [B, t] with cross-attention to
        `text_embeds` under `text_mask`; the last position's next-token distribution -> with k, (log-probs, ids) [B, k] of the k most
        probable tokens; else the sampled (stochastic) or most probable token [B, 1]."""
        atts = (product_input != 0).long()
        last = self.text_encoder(product_input, attention_mask=atts, encoder_hidden_states=text_embeds, encoder_attention_mask=text_mask,
                                 return_dict=True, is_decoder=True, return_logits=True)[:, -1, :]
        if k:
            top = torch.topk(torch.softmax(last, dim=-1), k=k, dim=-1)
            return torch.log(top.values), top.indices
        if stochastic:
            return torch.multinomial(torch.softmax(last, dim=-1), num_samples=1)
        return torch.argmax(last, dim=-1).unsqueeze(1)

    def train(self, mode: bool = True):
        self._engine.train_mode = bool(mode) and self.trainable          # dropout follows the mode
        return super().train(mode)

    @property
    def device(self):
        return self.device_

    # ---- state -------------------------------------------------------------------------------------------------------------------------
    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = OrderedDict() if destination is None else destination
        for name, t in self.store.named_tensors():
            out[prefix + name] = t if keep_vars else t.detach()
        return out

    def load_state_dict(self, state_dict, strict: bool = True):
        self._engine.pre_backward_wait()
        missing, unexpected = self.store.load_state_dict(state_dict, strict=strict)
        self._refresh()
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def load_pretrained(self, path_or_dict):
        """The script's checkpoint load: the 'model' or 'state_dict' of a pretraining or a fine-tuned reaction checkpoint (or a bare
        dict) through `map_checkpoint`, strict=False.  Returns the (missing, unexpected) keys."""
        ck = torch.load(path_or_dict, map_location="cpu") if isinstance(path_or_dict, str) else path_or_dict
        sd = ck.get("model", ck.get("state_dict", ck))
        return self.load_state_dict(map_checkpoint(sd), strict=False)

    def save_checkpoint(self, path: str, **extra):
        """The layout d_rxn_prediction.py:237-245 writes: 'state_dict' (what rxn_predict.py and load_pretrained read), 'config', 'epoch'."""
        ck = dict(state_dict={k: v.detach().cpu().clone() for k, v in self.state_dict().items()}, config=self.config,
                  epoch=int(self.current_epoch), global_step=int(self.global_step))
        ck.update(extra)
        torch.save(ck, path)


SPMM_rxn = SPMMRxn          # the reference's class name (a module swap: INTEGRATION.md)
