"""`SPMMRxn` -- drop-in for the reference's reaction-prediction model `SPMM_rxn` (SPMM_models_rxn.py), INFERENCE only: forward synthesis
(USPTO-480k) and retrosynthesis (USPTO-50k) by greedy or k-beam decoding of the product SMILES against the encoded reactant SMILES.

Same constructor (`cp=None, config=None`), same state_dict keys ([out,in] fp32 layout: config.rxn_spec), the sub-modules the evaluation
loops call -- `model.text_encoder2.bert(ids, attention_mask=, mode='text')`, `model.text_encoder(...)`, `model.generate(...)` -- as
facades on the engine.  The searches themselves are spmm_amd.decode.predict_products / greedy_products (K/V cache, masked-memory
cross-attention, one-launch beam step); the facades are their whole-prefix baseline.  Fine-tuning (`SPMM_rxn.forward`, the training
loop of d_rxn_prediction.py) is not built: `forward` raises.  There is no eager / CPU fallback."""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch
from torch import nn

from . import ops
from .config import BertConfig, SPMMConfig, is_buffer, rxn_encoder_config, rxn_spec
from .engine import Engine
from .options import EngineOptions
from .params import ParamStore

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


class SPMMRxn(nn.Module):
    def __init__(self, cp=None, config=None, device=None, options: Optional[EngineOptions] = None, bert_config: Optional[BertConfig] = None,
                 bert_config_smiles: Optional[BertConfig] = None):
        super().__init__()
        if not torch.cuda.is_available() and not ops._DRY_RUN:
            raise RuntimeError("spmm_amd.SPMMRxn needs an MI355X (HIP device); there is no CPU fallback")
        self.options = options if options is not None else EngineOptions.from_env()
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
        self.store = ParamStore(self.cfg, self.device_, train=False, spec=rxn_spec(c_dec, c_enc))
        self.engine = Engine(self.cfg, self.store, self.device_, self.options)
        self.engine.train_mode = False
        for name, t in self.store.named_tensors():
            if is_buffer(name):
                self._buffers[name] = t
            elif self.store.kind[name] not in ("tied_w", "tied_b"):              # (aliases: part of state_dict() only)
                self._parameters[name] = nn.Parameter(t, requires_grad=False)
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
        st.refresh_shadows()

    # ---- the reference's API -------------------------------------------------------------------------------------------------------
    def forward(self, *args, **kwargs):
        raise NotImplementedError("spmm_amd.SPMMRxn is inference only: seq2seq fine-tuning (SPMM_rxn.forward, the training loop of "
                                  "d_rxn_prediction.py) is not built -- load a fine-tuned checkpoint and use generate / "
                                  "spmm_amd.decode.predict_products / greedy_products")

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

    def eval(self):
        self.engine.train_mode = False
        return super().eval()

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
        missing, unexpected = self.store.load_state_dict(state_dict, strict=strict)
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def load_pretrained(self, path_or_dict):
        """The script's checkpoint load: the 'model' or 'state_dict' of a pretraining or a fine-tuned reaction checkpoint (or a bare
        dict) through `map_checkpoint`, strict=False.  Returns the (missing, unexpected) keys."""
        ck = torch.load(path_or_dict, map_location="cpu") if isinstance(path_or_dict, str) else path_or_dict
        sd = ck.get("model", ck.get("state_dict", ck))
        return self.load_state_dict(map_checkpoint(sd), strict=False)


SPMM_rxn = SPMMRxn          # the reference's class name (a module swap: INTEGRATION.md)
