"""One seq2seq fine-tuning step of the reaction model on the engine: `SPMM_rxn.forward` (SPMM_models_rxn.py:31-46) and its backward.

  reactants: embed (text_encoder2.bert.) -> [pack plan: padding rows dropped] -> encoder layers 0..f_enc-1 -> KVSource
  product:   embed (text_encoder.bert.)  -> [pack plan] -> every decoder layer, causal, sequence s cross-attending source s in the fusion
             layers -> tied LM head -> spmm_s2s_loss (CrossEntropyLoss(ignore_index=0) on the shifted product, csrc/losses.hip)

A padding token is never attended as a key and the row of a padding token has no label (its target is PAD or it is the last position), so
both stacks run on the packed valid rows (Engine._pack_plan) whenever the masks are non-empty prefixes; the loss kernel finds a packed
row's label through the pack plan's `rows`.  The backward folds the decoder's cross-attention key/value gradients of all fusion layers
into one fp32 source gradient (`dkv_acc`), which enters the encoder's backward in bf16.  The gradients land in the parameter arena."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .engine import Engine, _ceil
from .finetune_step import FinetuneStep

DEC, ENC = "text_encoder.", "text_encoder2."


class RxnStep(Engine):
    def __init__(self, cfg, params, device, c_enc, options=None):
        super().__init__(cfg, params, device, options)
        self.c_enc = c_enc
        self.loss = self.losses[0:1]                       # (zeroed with the rest of step_zero at the head of every forward)

    to_device = FinetuneStep.to_device

    def forward(self, src_ids: torch.Tensor, src_mask: torch.Tensor, prod_ids: torch.Tensor, prod_mask: torch.Tensor, *, save: bool = True,
                n_src_tokens: Optional[int] = None, n_prod_tokens: Optional[int] = None, grad_in_forward: bool = False):
        """-> device loss [1].  `n_src_tokens` / `n_prod_tokens`: the host's counts of valid tokens (every mask row a non-empty prefix),
        which spare the pack plans their device reads.  grad_in_forward (train_step: the loss-gradient scale is already on the device): the
        loss launch writes d(loss)/d(logits) too, so `backward` launches no second one."""
        cd, ce = self.cfg.text, self.c_enc
        B, Ls = src_ids.shape
        Lp = prod_ids.shape[1]
        if save and max(Ls, Lp) > ops.ATTN_MAXL:
            raise ValueError(f"seq2seq fine-tuning sequences are limited to {ops.ATTN_MAXL} tokens (got {Ls} source / {Lp} product); "
                             "the reference truncates at 150 / 100")
        if Lp < 2:
            raise ValueError("the product needs at least two positions: position t predicts token t + 1")
        self._salt = 0
        if self.train_mode:
            self.seed.add_(1)                              # new dropout masks every step; the backward re-reads the same value
        ops.zero_(self.step_zero)
        sids32, smask32 = src_ids.to(torch.int32).contiguous(), src_mask.to(torch.int32).contiguous()
        pids32, pmask32 = prod_ids.to(torch.int32).contiguous(), prod_mask.to(torch.int32).contiguous()
        # ---- reactants (SPMM_models_rxn.py:34)
        ts = self.encode_text(ENC + "bert.", ce, sids32, smask32, n_tokens=n_src_tokens, save=save)
        src = ts.source()
        # ---- product (:35-42): one group of B sequences, causal from sequence 0, sequence s attending source s
        tp = self.text_rows_of(DEC + "bert.", cd, pids32, pmask32, n_tokens=n_prod_tokens, save=save, causal=True)
        if n_src_tokens is not None or n_prod_tokens is not None:
            self.nan_flag.bitwise_or_(self.hint_bad)       # a wrong hint: the optimiser step becomes a no-op (step.py)
        gp, pkp = tp.groups, tp.pk
        g = gp.groups[0]
        g.kv_mask = ts.kv_mask
        g.attend(src, torch.arange(B, dtype=torch.int64, device=self.dev))
        src.finalize()
        yp, tape_p, _ = self.stack_fwd(DEC + "bert.", cd, range(0, cd.num_hidden_layers), True, tp.x, gp, save)
        logits, lmsv = self.lm_head_fwd(DEC, cd, yp, save)
        # ---- CrossEntropyLoss(ignore_index=0) on the shifted product (:44-45)
        row_of = pkp["rows"] if pkp else None
        dlogits = self._new(yp.shape[0], _ceil(cd.vocab_size, 64)) if (save and grad_in_forward) else None
        ops.s2s_loss(logits, pids32.view(-1), nseq=B, L=Lp, V=cd.vocab_size, ws=self.icount[0:4], losses=self.losses, slot=0, row_of=row_of,
                     dlogits=dlogits, gscale=self.gscale[0:1] if dlogits is not None else None)
        self.tape = dict(B=B, Ls=Ls, Lp=Lp, pks=ts.pk, pkp=pkp, sids32=sids32, pids32=pids32, esv_s=ts.esv, esv_p=tp.esv, gs=ts.groups, gp=gp, src=src,
                         tape_s=ts.tape, tape_p=tape_p, logits=logits, lmsv=lmsv, row_of=row_of, dlogits=dlogits) if save else None
        return self.loss

    def backward(self):
        """Accumulates gscale[0] * d(loss)/d(param) into the gradient arena (self.P.grad)."""
        T = self.tape
        if T is None:
            raise RuntimeError("backward() without a taped forward()")
        self.pre_backward_wait()
        cd, ce, P = self.cfg.text, self.c_enc, self.P
        H, B, Ls, Lp, V = cd.hidden_size, T["B"], T["Ls"], T["Lp"], cd.vocab_size
        dlogits = T["dlogits"]
        if dlogits is None:                                # the scale arrived after the forward (the autograd path)
            dlogits = self._new(T["logits"].shape[0], _ceil(V, 64))
            ops.s2s_loss(T["logits"], T["pids32"].view(-1), nseq=B, L=Lp, V=V, ws=self.icount[0:4], losses=self.loss_scratch, slot=0,
                         row_of=T["row_of"], dlogits=dlogits, gscale=self.gscale[0:1])
        dY = self.lm_head_bwd(DEC, cd, T["lmsv"], dlogits)
        # ---- decoder; the cross-attention key/value data gradients of every fusion layer land on the source's rows, in fp32
        src = T["src"]
        d_src = self._zeros(src.kv.shape[0], H, dtype=torch.float32)
        dXp = self.stack_bwd(DEC + "bert.", cd, range(0, cd.num_hidden_layers), T["tape_p"], dY, T["gp"], dkv_acc={id(src): d_src})
        self._embed_bwd(DEC + "bert.", cd, T["esv_p"], dXp, T["pkp"], T["pids32"], B, Lp)
        # ---- encoder
        dYs = ops.cast_f32_bf16(d_src.view(-1), self._new(d_src.numel())).view(-1, H)
        dXs = self.stack_bwd(ENC + "bert.", ce, range(0, ce.fusion_layer), T["tape_s"], dYs, T["gs"])
        self._embed_bwd(ENC + "bert.", ce, T["esv_s"], dXs, T["pks"], T["sids32"], B, Ls)
        self.end_backward()

    def _embed_bwd(self, pfx, c, esv, dX, pk, ids32, B, L):
        P, H = self.P, c.hidden_size
        if pk:                                             # back to the dense layout of the embedding kernels (padding rows: zero)
            dX = ops.gather_rows2(self._new(B * L, H), dX, pk["inv"])
        dz = self._embed_ln_bwd(pfx, c, esv, dX)
        ep = pfx + "embeddings."
        ops.embed_bwd(0, dz, nseq=B, L=L, H=H, dpos=P.g(ep + "position_embeddings.weight"), dtype0=P.g(ep + "token_type_embeddings.weight"),
                      ids=ids32, dword=P.g(ep + "word_embeddings.weight"))
