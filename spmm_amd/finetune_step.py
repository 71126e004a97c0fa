"""One fine-tuning step on the engine: the reference's downstream models (d_regression.py:24-49, d_classification.py:26-50,
d_classification_multilabel.py:26-47) -- text_encoder.bert(ids, mask, mode='text').last_hidden_state[:, 0, :] -> reg_head -> loss --
and its backward.

  embed_text -> [pack plan: padding rows dropped] -> text layers 0..f-1 -> position-0 rows -> Linear + GELU (gemm_nt, EPI_GELU)
  -> spmm_task_head (second Linear + loss, csrc/heads.hip)

Only position 0 of the last layer reaches the loss and a padding token is never attended as a key, so the layers run on the packed
valid rows (Engine._pack_plan), as the pretraining step's text passes do.  The gradients land in the parameter arena."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .engine import Engine

PFX = "text_encoder.bert."
TASK_KIND = {"regression": ops.TASK_MSE, "classification": ops.TASK_CE, "multilabel": ops.TASK_BCE}


class FinetuneStep(Engine):
    def __init__(self, cfg, params, device, task: str, options=None):
        super().__init__(cfg, params, device, options)
        self.task, self.kind = task, TASK_KIND[task]
        self.loss = self.losses[0:1]                       # (zeroed with the rest of step_zero at the head of every forward)

    def forward(self, ids: torch.Tensor, mask: torch.Tensor, target: Optional[torch.Tensor] = None, *, save: bool = True,
                n_tokens: Optional[int] = None):
        """-> (device loss [1] or None without targets, fp32 logits [B, C]).  `n_tokens`: the host's count of valid tokens (every mask
        row a non-empty prefix), which spares the pack plan its one device read."""
        c, P = self.cfg.text, self.P
        H = c.hidden_size
        B, L = ids.shape
        if save and L > ops.ATTN_MAXL:
            raise ValueError(f"fine-tuning sequences are limited to {ops.ATTN_MAXL} tokens (got {L}); the reference truncates at 100")
        self._salt = 0
        if self.train_mode:
            self.seed.add_(1)                              # new dropout masks every step; the backward re-reads the same value
        ops.zero_(self.step_zero)
        ids32 = ids.to(torch.int32).contiguous()
        mask32 = mask.to(torch.int32).contiguous()
        t = self.text_rows_of(PFX, c, ids32, mask32, n_tokens=n_tokens, save=save)
        if n_tokens is not None:
            self.nan_flag.bitwise_or_(self.hint_bad)       # a wrong hint: the optimiser step becomes a no-op (step.py)
        t.y, t.tape, _ = self.stack_fwd(PFX, c, range(0, c.fusion_layer), False, t.x, t.groups, save)
        cls = ops.gather_rows2(self._new(B, H), t.y, t.cls_rows)
        W2 = P.w("reg_head.2.weight")
        Wd, C = W2.shape[1], W2.shape[0]
        act, pre = self._new(B, Wd), self._new(B, Wd)
        ops.gemm_nt(cls, P.wb("reg_head.0.weight"), act, bias=P.w("reg_head.0.bias"), epi=ops.EPI_GELU, C2=pre)
        logits = self._new(B, C, dtype=torch.float32)
        tgt = None if target is None else self._target(target, B, C)
        ops.task_head(act, W2, P.w("reg_head.2.bias"), logits, kind=self.kind, target=tgt, loss=None if tgt is None else self.loss)
        self.tape = dict(B=B, L=L, pk=t.pk, M=t.y.shape[0], ids32=ids32, esv=t.esv, groups=t.groups, tape=t.tape, cls=cls, cls_idx=t.cls_rows, act=act,
                         pre=pre, logits=logits, target=tgt) if save else None
        return (None if tgt is None else self.loss), logits

    def to_device(self, t: torch.Tensor) -> torch.Tensor:
        """A host tensor is staged in pinned memory and copied without blocking: a copy from pageable memory waits for the stream, i.e.
        for the previous step's GPU work, before the host may enqueue this one."""
        if t.device.type == "cpu" and self.dev.type == "cuda":
            return t.pin_memory().to(self.dev, non_blocking=True)
        return t.to(self.dev)

    def _target(self, t: torch.Tensor, B: int, C: int) -> torch.Tensor:
        t = self.to_device(t)
        if self.kind == ops.TASK_CE:
            return t.reshape(B).to(torch.int32).contiguous()
        return t.reshape((B,) if self.kind == ops.TASK_MSE else (B, C)).to(torch.float32).contiguous()

    def backward(self):
        """Accumulates gscale[0] * d(loss)/d(param) into the gradient arena (self.P.grad)."""
        T = self.tape
        if T is None or T["target"] is None:
            raise RuntimeError("backward() without a taped forward() on targets")
        self.pre_backward_wait()
        c, P = self.cfg.text, self.P
        H, f, B, L = c.hidden_size, c.fusion_layer, T["B"], T["L"]
        dact = self._new(*T["act"].shape)
        ops.task_head(T["act"], P.w("reg_head.2.weight"), P.w("reg_head.2.bias"), T["logits"], kind=self.kind, target=T["target"],
                      gscale=self.gscale[0:1], dA=dact, dW2=P.g("reg_head.2.weight"), db2=P.g("reg_head.2.bias"))
        dpre = self._gelu_bwd(dact, T["pre"])
        self._wgrad(dpre, T["cls"], P.g("reg_head.0.weight"), P.g("reg_head.0.bias"))
        dcls = self._new(B, H)
        ops.gemm_nt(dpre, self._wT("reg_head.0", P.w("reg_head.0.weight")), dcls)
        dY = ops.add_rows_bf16(self._zeros(T["M"], H), T["cls_idx"], dcls)
        dX = self.stack_bwd(PFX, c, range(0, f), T["tape"], dY, T["groups"])
        pk = T["pk"]
        if pk:                                             # back to the dense layout of the embedding kernels (padding rows: zero)
            dX = ops.gather_rows2(self._new(B * L, H), dX, pk["inv"])
        dz = self._embed_ln_bwd(PFX, c, T["esv"], dX)
        ep = PFX + "embeddings."
        ops.embed_bwd(0, dz, nseq=B, L=L, H=H, dpos=P.g(ep + "position_embeddings.weight"), dtype0=P.g(ep + "token_type_embeddings.weight"),
                      ids=T["ids32"], dword=P.g(ep + "word_embeddings.weight"))
        self.end_backward()
