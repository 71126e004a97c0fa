"""Teacher-forced likelihood on the engine: how probable is a given molecule under a given condition?

  score_smiles    log p(SMILES | property vector), as the pretraining's LM pass computes its logits (SPMM_models.py:224-231): the property
                  states of `decode.encode_properties`, `text_encoder` run causally over the SMILES with its fusion layers cross-attending
                  them, the tied LM head.
  score_products  log p(product | reactants) on `spmm_amd.rxn.SPMMRxn`, as SPMM_models_rxn.py:31-46 computes its logits: the reactants
                  through `text_encoder2`, the candidate decoded causally against them.

Both score P (condition, sequence) pairs.  engine=True: every distinct condition is encoded once and its cross-attention keys | values are
projected once per fusion layer (engine.KVSource, bound per pair); the unimodal layers 0 .. fusion_layer-1 are causal and see no condition,
so they run once per distinct sequence, on packed rows; the P query sequences of the fusion layers are gathered from those rows; the
transform head is followed by `ops.lm_score` (csrc/score.hip: vocabulary projection, log_softmax and the label gather in one launch, no
logits tensor) or -- fused=False -- by `lm_head_fwd`, log_softmax and a gather in torch.  engine=False: the dense module call
`text_encoder(..., is_decoder=True, return_logits=True)` on the P pairs as a padded batch, every condition and sequence encoded once per
pair: the yard-stick, written against the module API, so it runs on any object that has it (the CPU oracle included).

A sequence [CLS] t1 .. tn [SEP] PAD.. is scored over t1 .. tn and [SEP] -- position t predicts token t + 1, a PAD target is ignored -- which
is what the beam searches accumulate.  Inference only: no tape, dropout off."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops
from .engine import BF, KVSource, Group, Batch, host_lens, host_token_count      # noqa: F401  (host_lens: importable from here too)

TP, EP = "text_encoder.bert.", "text_encoder2.bert."


@dataclass
class Scores:
    """Per pair: logp = sum of the labelled positions' log-probabilities, n_tokens = their number, token_logp[:, t] = log p(token t + 1 |
    tokens 0 .. t, condition), 0 beyond the sequence's labels."""
    logp: torch.Tensor          # fp32 [P]
    n_tokens: torch.Tensor      # int64 [P]
    token_logp: torch.Tensor    # fp32 [P, L - 1]

    def per_token(self) -> torch.Tensor:
        return self.logp / self.n_tokens.clamp(min=1).to(self.logp.dtype)


def _engine(model):
    eng = getattr(model, "engine", None)
    if eng is None:
        raise TypeError(f"spmm_amd.score needs a model with an engine (spmm_amd.model.SPMM / spmm_amd.rxn.SPMMRxn); {type(model).__name__} has "
                        "none -- the engine path is HIP kernels and has no CPU / eager fallback (engine=False runs on the module API)")
    eng.train_mode = False
    return eng


def check_pairs(pairs: Optional[torch.Tensor], n_cond: int, n_seq: int, what: str) -> torch.Tensor:
    """pairs int64 [P, 2] = (row of the conditions, row of the sequences) on the host; None: row i with row i."""
    if pairs is None:
        if n_cond != n_seq:
            raise ValueError(f"{what}: without `pairs` row i is paired with row i, but there are {n_cond} conditions and {n_seq} sequences")
        i = torch.arange(n_seq, dtype=torch.int64)
        return torch.stack([i, i], dim=1)
    pairs_h = pairs.detach().cpu().to(torch.int64).reshape(-1, 2)
    if pairs_h.shape[0] and (int(pairs_h[:, 0].min()) < 0 or int(pairs_h[:, 0].max()) >= n_cond or int(pairs_h[:, 1].min()) < 0
                             or int(pairs_h[:, 1].max()) >= n_seq):
        raise IndexError(f"{what}: a pair names a condition or a sequence that is not there")
    return pairs_h


def _empty(L: int, dev) -> Scores:
    return Scores(torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                  torch.empty(0, max(L - 1, 0), dtype=torch.float32, device=dev))


def _from_logits(logits: torch.Tensor, ids: torch.Tensor, L_out: int) -> Scores:
    """The composite ending on dense logits [P, L, V] and the ids [P, L] (PAD = 0): log_softmax, gather, sums.  Float32 throughout."""
    P, L = ids.shape
    tok = torch.zeros(P, max(L_out - 1, 0), dtype=torch.float32, device=logits.device)
    if L > 1:
        lab = ids[:, 1:].to(logits.device).long()
        lp = torch.log_softmax(logits[:, :-1].float(), dim=-1).gather(2, lab[..., None])[..., 0]
        tok[:, :L - 1] = torch.where(lab > 0, lp, torch.zeros_like(lp))
        n = (lab > 0).sum(1)
    else:
        n = torch.zeros(P, dtype=torch.int64, device=logits.device)
    return Scores(tok.sum(1), n, tok)


def _decode_scores(eng, ct, ids_h, lens_all, pairs_h, src: KVSource, fused: bool, L_out: int, what: str, xattn_tap=None) -> Scores:
    """The shared engine path: the causal decoder `text_encoder` over the sequences ids_h (host, PAD = 0 beyond lens_all) of the pairs,
    pair p cross-attending sequence pairs_h[p, 0] of `src` in the fusion layers -> Scores.  xattn_tap: Engine.stack_fwd's, on the fusion
    layers (attribution.reaction_attention_maps; pair p owns lens_all[pairs_h[p, 1]] packed query rows, in pair order)."""
    dev = eng.dev
    P = pairs_h.shape[0]
    f, n = ct.fusion_layer, ct.num_hidden_layers
    ms, inv_m = torch.unique(pairs_h[:, 1], return_inverse=True)
    lens_u = lens_all[ms.numpy()]
    Lt = int(lens_u.max())
    if Lt > ops.ATTN_MAXL:
        raise ValueError(f"{what}: a sequence of {Lt} tokens exceeds the {ops.ATTN_MAXL} the packed attention layouts hold")
    if Lt < 2:                                             # nothing but [CLS]: no position has a target
        return Scores(torch.zeros(P, dtype=torch.float32, device=dev), torch.zeros(P, dtype=torch.int64, device=dev),
                      torch.zeros(P, max(L_out - 1, 0), dtype=torch.float32, device=dev))
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)                        # noqa: E731
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)                        # noqa: E731
    # ---- the unimodal layers, causal, once per distinct sequence, on packed rows
    ids_u = ids_h[ms, :Lt].contiguous()
    mask_u = (torch.arange(Lt)[None, :] < torch.from_numpy(lens_u)[:, None]).to(torch.int32)
    ids32 = ids_u.to(dev).to(torch.int32).contiguous()
    t = eng.encode_text(TP, ct, ids32, mask_u.to(dev).contiguous(), n_tokens=int(lens_u.sum()), causal=True, what=what + ": ")
    # ---- the fusion layers: P query sequences gathered from those rows, packed, causal, pair p bound to its condition
    im, iq = inv_m.numpy(), pairs_h[:, 0].numpy()
    len_p, qrow0, Mt, pos, seq, gat = t.pair_layout(lens_u, im)
    X = t.y.index_select(0, i64(gat))
    qrow0_d, qlen_d = i32(qrow0), i32(len_p)
    gq = Batch([Group(0, P, Lt, None, 0, q_row0=qrow0_d, q_len=qlen_d, nrows=Mt).bind(src, i32(iq), 0)])
    y, _, _ = eng.stack_fwd(TP, ct, range(f, n), True, X, gq, False, **({} if xattn_tap is None else {"xattn_tap": xattn_tap}))
    # ---- the tied LM head on the Mt rows; row r = position pos[r] of pair seq[r] = dense row seq[r] * Lt + pos[r] of the [P, Lt] ids
    W = max(L_out, Lt)
    lay = dict(P=P, Lt=Lt, W=W, row_of=i64(seq * Lt + pos), pos=i64(pos), dest=i64(seq * W + pos), seq_row0=qrow0_d, seq_len=qlen_d,
               ids=ids32.index_select(0, i64(im)).contiguous())                                              # ids: [P, Lt]
    logp, n_tok, tok = lm_ending(eng, ct, y, lay, fused)
    return Scores(logp, n_tok, tok[:, :max(L_out - 1, 0)].contiguous())


def lm_ending(eng, ct, y, lay, fused: bool):
    """The ending of both paths on the decoder's output rows y [Mt, H] -> (logp fp32 [P], n_tokens int64 [P], token log-probabilities fp32
    [P, W] scattered to (pair, position)).  fused: the transform head, then ops.lm_score.  Composite: lm_head_fwd (fp32 logits [Mt, V]),
    log_softmax, the label gather and the sums in torch."""
    P, Lt, W, row_of = lay["P"], lay["Lt"], lay["W"], lay["row_of"]
    tok = torch.zeros(P, W, dtype=torch.float32, device=y.device)
    if fused:
        tf = "text_encoder.cls.predictions.transform."
        yt, _ = eng._transform_fwd(tf + "dense", tf + "LayerNorm", y, False, eps=ct.layer_norm_eps, pre=False)
        tok_lp, seq_lp, seq_n = ops.lm_score(yt, eng.P.wb("text_encoder.cls.predictions.decoder.weight"), eng.P.w("text_encoder.cls.predictions.bias"),
                                             lay["ids"].view(-1), nseq=P, L=Lt, row_of=row_of, seq_row0=lay["seq_row0"], seq_len=lay["seq_len"])
        tok.view(-1)[lay["dest"]] = tok_lp
        return seq_lp, seq_n.to(torch.int64), tok
    logits, _ = eng.lm_head_fwd("text_encoder.", ct, y, False)
    flat = lay["ids"].view(-1).long()
    lab = torch.where(lay["pos"] < Lt - 1, flat[(row_of + 1).clamp(max=P * Lt - 1)], torch.zeros_like(row_of))
    lp = torch.log_softmax(logits, dim=-1).gather(1, lab[:, None])[:, 0]
    tok.view(-1)[lay["dest"]] = torch.where(lab > 0, lp, torch.zeros_like(lp))
    n_lab = torch.zeros(P, W, dtype=torch.int64, device=y.device)
    n_lab.view(-1)[lay["dest"]] = (lab > 0).to(torch.int64)
    return tok.sum(1), n_lab.sum(1), tok


def _inputs(ids, mask, what):
    ids_h, mask_h = ids.detach().cpu().long(), mask.detach().cpu()
    if ids_h.dim() != 2 or tuple(ids_h.shape) != tuple(mask_h.shape):
        raise ValueError(f"{what}: ids and mask must both be [n, L]")
    lens = host_lens(mask_h, what)
    return ids_h * (mask_h != 0).long(), mask_h, lens                  # (a token under a zero mask is PAD: it is no target)


@torch.no_grad()
def score_smiles(model, pv: torch.Tensor, ids: torch.Tensor, mask: torch.Tensor, pairs: Optional[torch.Tensor] = None,
                 prop_mask: Optional[torch.Tensor] = None, engine: bool = True, fused: bool = True) -> Scores:
    """log p(SMILES | PV) of P pairs.  pv [Q, n_props] (normalised values); prop_mask ([n_props] or [Q, n_props], 1 = property unknown:
    the learned mask token stands there, decode.encode_properties); ids / mask [N, L]: token ids with '[CLS]' at position 0 and their
    attention masks (non-empty prefixes); pairs int64 [P, 2] = (row of pv, row of ids), None: row i with row i.
    Raises ValueError for a mask that is not a non-empty prefix or a sequence longer than ops.ATTN_MAXL, IndexError for a pair out of range."""
    from .decode import encode_properties
    what = "score_smiles"
    ids_h, mask_h, lens = _inputs(ids, mask, what)
    pv = pv.reshape(-1, pv.shape[-1])
    pairs_h = check_pairs(pairs, pv.shape[0], ids_h.shape[0], what)
    P, L = pairs_h.shape[0], ids_h.shape[1]
    if prop_mask is not None:
        prop_mask = prop_mask.reshape(-1, pv.shape[1]).expand(pv.shape[0], pv.shape[1])
    if not engine:
        dev = pv.device
        if P == 0:
            return _empty(L, dev)
        q_sel, m_sel = pairs_h[:, 0], pairs_h[:, 1]
        Lt = int(lens[m_sel.numpy()].max())
        pe = encode_properties(model, pv[q_sel.to(dev)], None if prop_mask is None else prop_mask[q_sel.to(prop_mask.device)])
        ones = torch.ones(pe.shape[:2], dtype=torch.long, device=pe.device)
        ids_p, mask_p = ids_h[m_sel, :Lt].to(pe.device), mask_h[m_sel, :Lt].to(pe.device).long()
        logits = model.text_encoder(ids_p, attention_mask=mask_p, encoder_hidden_states=pe, encoder_attention_mask=ones, return_dict=True,
                                    is_decoder=True, return_logits=True)
        return _from_logits(logits, ids_p, L)
    eng = _engine(model)
    if P == 0:
        return _empty(L, eng.dev)
    cfg, dev = model.cfg, eng.dev
    qs, inv_q = torch.unique(pairs_h[:, 0], return_inverse=True)
    pv_d = pv.to(dev).to(torch.float32)[qs.to(dev)]
    pe = encode_properties(model, pv_d, None if prop_mask is None else prop_mask.to(dev)[qs.to(dev)])        # [Up, Lp, H]
    eng.train_mode = False
    Up, Lp, H = pe.shape
    src = KVSource(pe.to(BF).reshape(Up * Lp, H).contiguous(), Up, Lp)
    return _decode_scores(eng, cfg.text, ids_h, lens, torch.stack([inv_q, pairs_h[:, 1]], dim=1), src, fused, L, what)


@torch.no_grad()
def score_products(model, src_ids: torch.Tensor, src_mask: torch.Tensor, prod_ids: torch.Tensor, prod_mask: torch.Tensor,
                   pairs: Optional[torch.Tensor] = None, engine: bool = True, fused: bool = True) -> Scores:
    """log p(product | reactants) of P pairs on the reaction model.  src_ids / src_mask [S, Ls]: the reactant tokens as the encoder sees
    them; prod_ids / prod_mask [C, L]: candidate products with '[CLS]' at position 0; pairs int64 [P, 2] = (row of the sources, row of the
    candidates), None: row i with row i.  The length limits are those of decode.predict_products; errors as `score_smiles`."""
    what = "score_products"
    sids_h, smask_h, slens = _inputs(src_ids, src_mask, what + " (sources)")
    pids_h, pmask_h, plens = _inputs(prod_ids, prod_mask, what + " (candidates)")
    pairs_h = check_pairs(pairs, sids_h.shape[0], pids_h.shape[0], what)
    P, L = pairs_h.shape[0], pids_h.shape[1]
    if not engine:
        dev = getattr(model, "device_", src_ids.device)
        if P == 0:
            return _empty(L, dev)
        s_sel, c_sel = pairs_h[:, 0], pairs_h[:, 1]
        Ls, Lt = int(slens[s_sel.numpy()].max()), int(plens[c_sel.numpy()].max())
        sid, smk = sids_h[s_sel, :Ls].to(dev), smask_h[s_sel, :Ls].to(dev).long()
        pid, pmk = pids_h[c_sel, :Lt].to(dev), pmask_h[c_sel, :Lt].to(dev).long()
        enc = model.text_encoder2.bert(sid, attention_mask=smk, return_dict=True, mode="text").last_hidden_state
        logits = model.text_encoder(pid, attention_mask=pmk, encoder_hidden_states=enc, encoder_attention_mask=smk, return_dict=True,
                                    is_decoder=True, return_logits=True)
        return _from_logits(logits, pid, L)
    eng = _engine(model)
    if P == 0:
        return _empty(L, eng.dev)
    src, inv_s = _rxn_memory(model, eng, sids_h, slens, pairs_h, what)
    return _decode_scores(eng, model.cfg.text, pids_h, plens, torch.stack([inv_s, pairs_h[:, 1]], dim=1), src, fused, L, what)


def _rxn_memory(model, eng, sids_h, slens, pairs_h, what: str):
    """-> (the encoded reactants of the pairs' distinct sources as a shared cross-attention source, source of every pair in it)."""
    ce, dev = model.cfg_enc, eng.dev
    ss, inv_s = torch.unique(pairs_h[:, 0], return_inverse=True)
    lens_s = slens[ss.numpy()]
    Ls = int(lens_s.max())
    if Ls > ops.ATTN_MAXL:
        raise ValueError(f"{what}: reactant sequences are limited to {ops.ATTN_MAXL} tokens (got {Ls}); the reference truncates at 150")
    # ---- every distinct source, once, through text_encoder2 on packed rows (as decode.RxnDecoder encodes its memory)
    mask_s = (torch.arange(Ls)[None, :] < torch.from_numpy(lens_s)[:, None]).to(torch.int32)
    mem = eng.encode_text(EP, ce, sids_h[ss, :Ls].to(dev).to(torch.int32).contiguous(), mask_s.to(dev).contiguous(),
                          n_tokens=host_token_count(mask_s), what=what + ": ")
    return mem.source(tables=True), inv_s
