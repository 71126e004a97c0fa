"""`SPMMRegressor`, `SPMMClassifier`, `SPMMMultiLabelClassifier` -- drop-ins for the reference's downstream models
`SPMM_regressor` (d_regression.py:24-49), `SPMM_classifier` (d_classification.py:26-50) and the multi-label `SPMM_classifier`
(d_classification_multilabel.py:26-47).

Same constructor (`tokenizer=None, config=None, n_output=2`), same `forward(text_input_ids, text_attention_mask, value, eval=False)`,
same state_dict keys ([out,in] fp32 layout: config.finetune_spec).  The reference loop -- its own `optim.AdamW(model.parameters())`,
`loss.backward()`, `optimizer.step()` -- runs unchanged; `train_step` is the same step with the fused arena AdamW on the device.
All arithmetic runs in the HIP kernels of libspmm_hip.so (spmm_amd/finetune_step.py); there is no eager / CPU fallback."""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional

import torch
from torch import nn

from . import ops
from .config import BertConfig, SPMMConfig, finetune_spec, is_buffer
from .engine import host_token_count
from .finetune_step import FinetuneStep
from .model import _CosineSchedule, _FusedAdamW
from .options import EngineOptions
from .params import ParamStore

# the fine-tuning scripts' inline config (d_regression.py:215-223 and its two siblings) minus the paths
DEFAULT_SCHED = {"sched": "cosine", "lr": 5e-5, "epochs": 15, "min_lr": 5e-6, "decay_rate": 1, "warmup_lr": 0.5e-5, "warmup_epochs": 1,
                 "cooldown_epochs": 0}


class _FinetuneStepFn(torch.autograd.Function):
    """Autograd boundary: the loss is a function of every parameter; backward runs the engine's backward with the incoming loss
    gradient as the device-side scale and hands back views of the flat gradient arena."""

    @staticmethod
    def forward(ctx, model, ids, mask, target, n_tokens, *params):
        loss, _ = model.engine.forward(ids, mask, target, n_tokens=n_tokens)
        ctx.model = model
        return loss.reshape(()).clone()

    @staticmethod
    def backward(ctx, g):
        m = ctx.model
        m.engine.gscale[0:1].copy_(g.reshape(1).to(torch.float32))
        ops.zero_(m.store.grad)
        m.engine.backward()
        # (a copy: autograd may keep a returned tensor as .grad, and the next backward rewrites the arena in place)
        g_all = m.store.grad.clone()
        return (None,) * 5 + tuple(m.store._view(g_all, n) for n in m._param_names)


class _FinetuneModel(nn.Module):
    TASK = ""
    STEP_SIZE = 50            # warm-up schedule cadence of the script's train() (d_classification.py:58; d_regression.py:57 uses 100)

    def __init__(self, tokenizer=None, config=None, n_output: int = 2, device=None, options: Optional[EngineOptions] = None,
                 bert_config: Optional[BertConfig] = None):
        super().__init__()
        if not torch.cuda.is_available() and not ops._DRY_RUN:
            raise RuntimeError(f"spmm_amd.{type(self).__name__} needs an MI355X (HIP device); there is no CPU fallback")
        # the LayerNorm backward from the stored pre-norm sum: a fine-tuned model starts from trained LayerNorms, where recovering the
        # normalised values from the output, (y - beta) / gamma, loses accuracy once |beta / gamma| >> 1
        self.options = options if options is not None else EngineOptions.from_env(ln_from_y=False)
        self.tokenizer, self.config = tokenizer, config
        if device is None:
            device = "cpu" if ops._DRY_RUN else f"cuda:{torch.cuda.current_device()}"
        self.device_ = torch.device(device)
        self.bert_cfg = bert_config if bert_config is not None else BertConfig.from_json_file(config["bert_config_text"])
        self.n_output = 1 if self.TASK == "regression" else int(n_output)
        self.store = ParamStore(SPMMConfig(text=self.bert_cfg), self.device_, train=True,
                                spec=finetune_spec(self.bert_cfg, self.TASK, self.n_output))
        self.engine = FinetuneStep(SPMMConfig(text=self.bert_cfg), self.store, self.device_, self.TASK, self.options)
        self._param_names = []
        for name, t in self.store.named_tensors():
            if is_buffer(name):
                self._buffers[name] = t
            else:
                self._parameters[name] = nn.Parameter(t)
                self._param_names.append(name)
        self._init_weights()
        self.current_epoch = 0
        self.global_step = 0
        self._optimizer = self._scheduler = None

    # ---- init: BertForMaskedLM._init_weights (xbert.py:742-752) for the encoder, nn.Linear's default for reg_head -------------------
    @torch.no_grad()
    def _init_weights(self):
        st, c = self.store, self.bert_cfg
        g = torch.Generator(device="cpu").manual_seed(torch.initial_seed() % (2 ** 31))
        for name, shape, kind in st.spec:
            if is_buffer(name):
                continue
            t = st.w(name)
            if name.startswith("reg_head."):
                fan_in = st.shape[name[:-len("bias")] + "weight"][1] if kind == "lin_b" else shape[1]
                t.copy_((torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in))
            elif kind in ("emb", "lin_w"):
                t.copy_(torch.randn(shape, generator=g) * c.initializer_range)
            elif kind == "ln_w":
                t.fill_(1.0)
            else:
                t.zero_()
        self._refresh()

    def _refresh(self):
        """bf16 shadows <- fp32 masters; remembers the arena's version so that a later in-place update from outside (a torch optimiser
        stepping the parameter views, load_state_dict) is seen by the next forward."""
        self.engine.pre_backward_wait()
        self.store.refresh_shadows()
        self._shadow_version = self.store.flat._version

    def _sync_shadows(self):
        if self.store.flat._version != self._shadow_version:
            self._refresh()

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def forward(self, text_input_ids, text_attention_mask, value=None, eval=False, *, n_tokens: Optional[int] = None):
        """Training: the mean loss (0-dim tensor; `loss.backward()` fills .grad of the parameters).  eval=True: the predictions,
        [B] for the regressor and [B, C] logits for the classifiers -- no tape, no dropout.  Host tensors are copied through pinned memory
        without blocking (FinetuneStep.to_device)."""
        eng = self.engine
        self._sync_shadows()
        ids, mask = eng.to_device(text_input_ids), eng.to_device(text_attention_mask)
        if eval:
            eng.train_mode = False
            _, logits = eng.forward(ids, mask, None, save=False)
            return logits[:, 0].clone() if self.TASK == "regression" else logits.clone()
        eng.train_mode = self.training
        if n_tokens is None:
            n_tokens = host_token_count(text_attention_mask)
        if torch.is_grad_enabled():
            return _FinetuneStepFn.apply(self, ids, mask, value, n_tokens, *[self._parameters[n] for n in self._param_names])
        loss, _ = eng.forward(ids, mask, value, save=False, n_tokens=n_tokens)
        return loss.reshape(()).clone()

    # ---- optimiser and schedule (the scripts' optim.AdamW(lr, weight_decay=0.02), no clipping, and create_scheduler) ---------------
    def configure_optimizers(self):
        cfg = self.config or {}
        o = cfg.get("optimizer", {})
        sched = dict(cfg.get("schedular", DEFAULT_SCHED))
        opt = _FusedAdamW(self.store, self.engine, lr=o.get("lr", sched["lr"]), weight_decay=o.get("weight_decay", 0.02), max_norm=math.inf)
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

    def train_step(self, ids, mask, value, n_tokens: Optional[int] = None):
        """zero_grad -> forward -> backward -> AdamW, all on the device.  Returns the device loss.  Host tensors (ids, mask, value) are
        copied through pinned memory without blocking; the packed row count comes from a host mask or `n_tokens`, so the step reads
        nothing back from the device (with a device mask and no `n_tokens` the pack plan reads the count back once)."""
        eng, opt = self.engine, self.optimizers()
        self._sync_shadows()
        eng.train_mode = self.training
        eng.gscale.fill_(1.0)
        if n_tokens is None:
            n_tokens = host_token_count(mask)
        ops.zero_(self.store.grad)
        loss, _ = eng.forward(eng.to_device(ids), eng.to_device(mask), value, n_tokens=n_tokens)
        eng.backward()
        opt.step()
        return loss

    def training_step(self, batch, batch_idx):
        """One iteration of the scripts' train(): `batch` = (SMILES list or (ids, mask), targets).  The schedule steps every STEP_SIZE
        iterations through the warm-up of epoch 0; `on_train_epoch_end` steps it after each epoch."""
        text, value = batch[0], batch[1]
        if isinstance(text, (tuple, list)) and torch.is_tensor(text[0]):
            ids, mask = text
        else:
            ti = self.tokenizer(text, padding="longest", truncation=True, max_length=100, return_tensors="pt")
            ids, mask = ti.input_ids[:, 1:], ti.attention_mask[:, 1:]
        loss = self.train_step(ids, mask, value)
        sch, opt = self.lr_schedulers(), self.optimizers()
        warm = sch.s["warmup_epochs"]
        if self.current_epoch == 0 and batch_idx % self.STEP_SIZE == 0 and batch_idx <= warm * self.STEP_SIZE:
            opt.param_groups[0]["lr"] = sch.lr_at(batch_idx // self.STEP_SIZE)
        self.global_step += 1
        return loss

    def on_train_epoch_end(self):
        """lr_scheduler.step(epoch + warmup_steps + 1) after each epoch (d_regression.py:190)."""
        sch = self.lr_schedulers()
        self.optimizers().param_groups[0]["lr"] = sch.lr_at(self.current_epoch + sch.s["warmup_epochs"] + 1)
        self.current_epoch += 1

    # ---- state ------------------------------------------------------------------------------------------------------------------
    @property
    def device(self):
        return self.device_

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = OrderedDict() if destination is None else destination
        for name, t in self.store.named_tensors():
            out[prefix + name] = t if keep_vars else t.detach()
        return out

    def load_state_dict(self, state_dict, strict: bool = True):
        self.engine.pre_backward_wait()
        missing, unexpected = self.store.load_state_dict(state_dict, strict=strict)
        self._refresh()
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def load_pretrained(self, path_or_dict):
        """The scripts' checkpoint load (d_regression.py:153-162): the 'state_dict' of a pretraining checkpoint (or 'model', or a bare
        dict), `_unk` -> `_mask`, strict=False.  Returns (missing, unexpected) keys; reg_head keeps its initial values."""
        ck = torch.load(path_or_dict, map_location="cpu") if isinstance(path_or_dict, str) else path_or_dict
        sd = ck.get("state_dict", ck.get("model", ck))
        sd = {k.replace("_unk", "_mask"): v for k, v in sd.items()}
        return self.load_state_dict(sd, strict=False)

    def save_checkpoint(self, path: str, **extra):
        ck = dict(state_dict={k: v.detach().cpu().clone() for k, v in self.state_dict().items()}, epoch=int(self.current_epoch),
                  global_step=int(self.global_step))
        ck.update(extra)
        torch.save(ck, path)


class SPMMRegressor(_FinetuneModel):
    """SPMM_regressor, d_regression.py:24-49: reg_head Linear(H, 2H), GELU, Linear(2H, 1); MSE."""
    TASK = "regression"
    STEP_SIZE = 100


class SPMMClassifier(_FinetuneModel):
    """SPMM_classifier, d_classification.py:26-50: reg_head Linear(H, H), GELU, Linear(H, n_output); cross entropy."""
    TASK = "classification"


class SPMMMultiLabelClassifier(_FinetuneModel):
    """SPMM_classifier, d_classification_multilabel.py:26-47: reg_head Linear(H, H), GELU, Linear(H, n_output); BCE on sigmoid."""
    TASK = "multilabel"


# the reference's class names (a module swap: INTEGRATION.md)
SPMM_regressor = SPMMRegressor
SPMM_classifier = SPMMClassifier
SPMM_multilabel_classifier = SPMMMultiLabelClassifier
