"""Property-to-molecule retrieval on the engine: which molecules of a library have these properties?

Two stages, as ALBEF (whose fusion passes the reference's xbert.py carries) retrieves:

  1. shortlist by the contrastive similarity the pretraining aligns (SPMM_models.py:92-131): `pv_features` / `smiles_features` are
     F.normalize(property_proj / text_proj (position 0 of the unimodal encoder)), and `MoleculeIndex.search` is a streaming top-k of the
     query features against the library's on csrc/retrieve.hip -- the [Q, N] similarity matrix is never formed;
  2. re-rank the head of the shortlist with the matching head (SPMM_models.py:137-152, 199-202): `match_scores` runs the two fusion passes
     of every (query, molecule) pair -- every distinct molecule's text encoded once on packed rows, the cross-attention keys | values of
     both directions projected once per distinct source per fusion layer, the last fusion layer on the position-0 rows only -- and returns
     softmax(itm_head(cat(cls_p, cls_t)))[:, 1].

Inference only: no tape, dropout off.  `similar` is the same search with text features as queries (the t2t similarity of :111)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .engine import BF, Batch, Group, KVSource, SelfKV, host_lens, host_token_count
from .tokenizer import MAX_LENGTH, encode_smiles, length_sorted_batches, pad_rows      # noqa: F401  (the library's batching helpers)

TP = "text_encoder.bert."


def _engine(model):
    eng = getattr(model, "engine", None)
    if eng is None:
        raise TypeError(f"spmm_amd.retrieve needs a model with an engine (spmm_amd.model.SPMM); {type(model).__name__} has none -- the retrieval "
                        "paths are HIP kernels and have no CPU / eager fallback")
    eng.train_mode = False
    return eng


def _normalized(eng, proj: str, X: torch.Tensor, L: int, B: int, cls_rows=None) -> torch.Tensor:
    """F.normalize(proj(position 0)) of B sequences of X.  The projection reads the fp32 master weights (spmm_rows_linear, as the module
    facades `text_proj` / `property_proj` do): the training step's bf16 weight shadow put the features 2.6 x further from the fp32
    reference than the facade composite (1.0e-4 against 4.0e-5 on the tiny configuration), and a feature is computed once per molecule."""
    H, E = X.shape[1], eng.cfg.embed_dim
    cls = X.index_select(0, cls_rows) if cls_rows is not None else X.view(-1, L * H)[:B, :H]
    raw = ops.rows_linear(cls, eng.P.w(proj + ".weight"), eng.P.w(proj + ".bias"), torch.empty(B, E, dtype=torch.float32, device=X.device))
    feat = torch.empty(B, E, dtype=torch.float32, device=X.device)
    ops.l2norm_fwd(raw, feat, torch.empty(B, dtype=torch.float32, device=X.device))
    return feat


@torch.no_grad()
def smiles_features(model, ids: torch.Tensor, mask: torch.Tensor, n_tokens: Optional[int] = None) -> torch.Tensor:
    """text_feat of SPMM_models.py:93-95 for a batch of token ids [B, Lt] (position 0 = the '[CLS]' token) -> fp32 [B, E], unit rows.
    n_tokens: the host's count of the mask's ones, for a mask that lives on the device (wordpiece_device.TokenLibrary.batches): sizes the
    packed rows without a device read.  Absent, a host mask is counted here, as before."""
    eng = _engine(model)
    t = eng.encode_text(TP, model.cfg.text, ids.to(eng.dev).to(torch.int32).contiguous(), mask.to(eng.dev).to(torch.int32).contiguous(),
                        n_tokens=host_token_count(mask) if n_tokens is None else int(n_tokens))
    return _normalized(eng, "text_proj", t.y, t.L, t.B, cls_rows=t.cls_rows)


@torch.no_grad()
def pv_features(model, pv: torch.Tensor, prop_mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """prop_feat of SPMM_models.py:82-92 without the MPM draw: pv [Q, n_props] (normalised values); prop_mask ([n_props] or [Q, n_props],
    1 = property unknown) puts the learned `property_mask` token at those entries, as conditional generation does
    (decode.encode_properties).  -> (fp32 [Q, E] unit rows, the PV encoder's hidden states bf16 [Q, n_props + 1, H] for `match_scores`)."""
    eng = _engine(model)
    cfg, dev = model.cfg, eng.dev
    cp, Lp = cfg.prop, cfg.n_props + 1
    pv = pv.to(dev).to(torch.float32).reshape(-1, cfg.n_props).contiguous()
    Q = pv.shape[0]
    if prop_mask is None:
        pm = torch.zeros(Q, cfg.n_props, dtype=torch.float32, device=dev)
    else:
        pm = prop_mask.to(dev).to(torch.float32).reshape(-1, cfg.n_props).expand(Q, cfg.n_props).contiguous()
    x, _ = eng.embed_pv("property_encoder.", cp, pv, pm, Q, Q, False)
    y, _, _ = eng.stack_fwd("property_encoder.", cp, range(cp.num_hidden_layers), False, x, Batch([Group(0, Q, Lp, None, Q)]), False)
    return _normalized(eng, "property_proj", y, Lp, Q), y.view(Q, Lp, cp.hidden_size)


# ------------------------------------------------------------------------------------------------------------------ stage one
def topk_reference(q: torch.Tensor, feats: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The tensor-library pair the kernel replaces: torch.topk(q @ feats.T, k) -- forms the [Q, N] matrix.  Yard-stick of the bench."""
    v, i = torch.topk(q @ feats.T, min(k, feats.shape[0]), dim=1)
    return v, i


class MoleculeIndex:
    """The text features of a library, fp32 [N, E] on the device in INPUT order, and -- when built from tokens -- the padded token ids the
    re-ranking stage needs (host tensors)."""

    def __init__(self, feats: torch.Tensor, ids: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                 smiles: Optional[List[str]] = None):
        assert feats.dim() == 2 and feats.dtype == torch.float32
        self.feats, self.ids, self.mask, self.smiles = feats.contiguous(), ids, mask, smiles

    def __len__(self):
        return self.feats.shape[0]

    @classmethod
    @torch.no_grad()
    def from_tokens(cls, model, ids: torch.Tensor, mask: torch.Tensor, batch_size: int = 256, smiles=None) -> "MoleculeIndex":
        """ids / mask [N, L] (host or device; zero padded prefixes): batches in order of token length, each cut to its longest molecule,
        features written back in input order."""
        eng = _engine(model)
        ids_h, mask_h = ids.cpu(), mask.cpu()
        N = ids_h.shape[0]
        feats = torch.empty(N, model.cfg.embed_dim, dtype=torch.float32, device=eng.dev)
        lens = mask_h.sum(1)
        for idx in length_sorted_batches(lens.numpy(), batch_size):
            sel = torch.from_numpy(idx)
            L = max(1, int(lens[sel].max()))
            feats[sel.to(eng.dev)] = smiles_features(model, ids_h[sel, :L], mask_h[sel, :L])
        return cls(feats, ids_h, mask_h, smiles)

    @classmethod
    @torch.no_grad()
    def from_library(cls, model, library, batch_size: int = 256, smiles=None) -> "MoleculeIndex":
        """The index of a wordpiece_device.TokenLibrary (host or device rows): its length-sorted batches through `smiles_features`, the
        features written back in input order; the host ids / mask the re-ranking stage and `save` keep are made once, for the library."""
        eng = _engine(model)
        feats = torch.empty(len(library), model.cfg.embed_dim, dtype=torch.float32, device=eng.dev)
        for idx, ids, mask, n_tokens in library.batches(batch_size):
            feats[torch.from_numpy(idx).to(eng.dev)] = smiles_features(model, ids, mask, n_tokens=n_tokens)
        ids_h, mask_h = library.padded_host()
        return cls(feats, ids_h, mask_h, smiles)

    @classmethod
    def build(cls, model, tokenizer, smiles: Sequence[str], batch_size: int = 256, tokenizer_device=None) -> "MoleculeIndex":
        """tokenizer_device: the GPU that tokenises the library (wordpiece_device.encode_smiles_device: one launch, the ids stay on the
        device); None: SmilesWordPiece on the host, as before.  The index is the same either way."""
        if tokenizer_device is not None:
            from .wordpiece_device import TokenLibrary
            return cls.from_library(model, TokenLibrary.from_strings(tokenizer, smiles, MAX_LENGTH, tokenizer_device), batch_size, smiles=list(smiles))
        rows = encode_smiles(tokenizer, smiles)
        ids, mask = pad_rows(rows, tokenizer.pad_token_id)
        return cls.from_tokens(model, ids, mask, batch_size, smiles=list(smiles))

    def save(self, path: str) -> None:
        torch.save({"format": "spmm_amd.MoleculeIndex/1", "feats": self.feats.cpu(), "ids": self.ids, "mask": self.mask, "smiles": self.smiles}, path)

    @classmethod
    def load(cls, path: str, device="cuda") -> "MoleculeIndex":
        d = torch.load(path, map_location="cpu", weights_only=True)
        if d.get("format") != "spmm_amd.MoleculeIndex/1":
            raise ValueError(f"{path}: not a saved MoleculeIndex")
        return cls(d["feats"].to(device), d["ids"], d["mask"], d["smiles"])

    @torch.no_grad()
    def search(self, query_feats: torch.Tensor, k: int, chunk: int = 1 << 20) -> Tuple[torch.Tensor, torch.Tensor]:
        """The k most similar library rows of every query -> (scores fp32 [Q, k], index int64 [Q, k]): largest first, equal scores by
        ascending index, (-inf, -1) beyond the library's size.  The library is streamed `chunk` rows at a time through spmm_sim_topk
        (any chunking gives the same bits); a ranking longer than the kernel's 64 slots takes one more pass over the library per further
        64, each cut at the last entry of the pass before."""
        q = query_feats.to(self.feats.device).to(torch.float32)
        if q.dim() != 2 or q.shape[1] != self.feats.shape[1]:
            raise ValueError(f"query features {tuple(q.shape)} do not match the library's {tuple(self.feats.shape)}")
        if k < 1 or chunk < 1:
            raise ValueError(f"k={k} chunk={chunk}")
        if q.stride(1) != 1 or q.stride(0) % 4 or q.data_ptr() % 16:
            q = q.contiguous()
        Q, N, dev = q.shape[0], self.feats.shape[0], q.device
        K = ops.SIM_TOPK_MAXK
        # one workspace for the launches of THIS search (they are ordered on the current stream; sized for its largest chunk and pass):
        # nothing is shared between two searches, so an index may be searched from several streams at once
        ws = ops.sim_topk_workspace(Q, min(N, chunk), min(k, K), dev)
        out_s, out_i, cut = [], [], None
        for k0 in range(0, k, K):
            kk = min(K, k - k0)
            s = torch.empty(Q, kk, dtype=torch.float32, device=dev)
            i = torch.empty(Q, kk, dtype=torch.int64, device=dev)
            ops.sim_topk(q, self.feats[:min(N, chunk)], s, i, base=0, merge=False, cut=cut, ws=ws if N > 0 else None)
            for r0 in range(chunk, N, chunk):
                ops.sim_topk(q, self.feats[r0:r0 + chunk], s, i, base=r0, merge=True, cut=cut, ws=ws)
            out_s.append(s)
            out_i.append(i)
            cut = (s[:, kk - 1].contiguous(), i[:, kk - 1].contiguous())
        return (out_s[0], out_i[0]) if len(out_s) == 1 else (torch.cat(out_s, 1), torch.cat(out_i, 1))


# ------------------------------------------------------------------------------------------------------------------ stage two
@torch.no_grad()
def match_scores(model, pv_hidden: torch.Tensor, ids: torch.Tensor, mask: torch.Tensor, pairs: torch.Tensor, engine: bool = True) -> torch.Tensor:
    """Matching probability of P (query, molecule) pairs: pairs int64 [P, 2] = (row of pv_hidden, row of ids / mask) -> fp32 [P] =
    softmax(itm_head(cat(cls_p, cls_t)))[:, 1] (SPMM_models.py:137-152, 199-202), cls_p = position 0 of the fusion layers over the PV
    states cross-attending the molecule's text, cls_t = position 0 of the fusion layers over the text cross-attending the PV states.

    engine=True: the text of every distinct molecule is encoded once on packed rows; the keys | values of both cross-attention directions
    are projected once per distinct source per fusion layer (engine.KVSource: the P PV-query sequences are bound to their molecule's text,
    the P text-query sequences to their query's PV states); the last fusion layer runs on the 2 P position-0 rows, its self-attention
    keys / values projected from the full sequences of the layer below (engine.SelfKV); the head is spmm_rows_linear.
    engine=False: the same arithmetic the way the reference runs it -- the dense module calls `text_encoder.bert(mode='text')` and the two
    `text_encoder.bert(mode='fusion')` on the P pairs as a padded batch, every molecule encoded once per pair it occurs in: the yard-stick."""
    pairs_h = pairs.cpu().to(torch.int64).reshape(-1, 2)
    P = pairs_h.shape[0]
    ids_h, mask_h = ids.cpu(), mask.cpu()
    if P == 0:
        return torch.empty(0, dtype=torch.float32, device=pv_hidden.device)
    if int(pairs_h[:, 0].min()) < 0 or int(pairs_h[:, 0].max()) >= pv_hidden.shape[0] or int(pairs_h[:, 1].min()) < 0 or int(pairs_h[:, 1].max()) >= ids_h.shape[0]:
        raise IndexError("match_scores: a pair names a query or a molecule that is not there")
    if not engine:
        return _match_dense(model, pv_hidden, ids_h, mask_h, pairs_h)
    eng = _engine(model)
    cfg, dev = model.cfg, eng.dev
    ct = cfg.text
    H, Lp, f, n = ct.hidden_size, cfg.n_props + 1, ct.fusion_layer, ct.num_hidden_layers
    qs, inv_q = torch.unique(pairs_h[:, 0], return_inverse=True)
    ms, inv_m = torch.unique(pairs_h[:, 1], return_inverse=True)
    Up = qs.numel()
    # ---- every distinct molecule's text, once, on packed rows (cut to the longest of them)
    lens_u = host_lens(mask_h[ms], "match_scores")
    Lt = int(lens_u.max())
    if Lt > ops.ATTN_MAXL:
        raise ValueError(f"match_scores: a molecule of {Lt} tokens exceeds the {ops.ATTN_MAXL} the packed attention layouts hold")
    mask_u = mask_h[ms, :Lt]
    t = eng.encode_text(TP, ct, ids_h[ms, :Lt].to(dev).to(torch.int32).contiguous(), mask_u.to(dev).to(torch.int32).contiguous(),
                        n_tokens=host_token_count(mask_u))
    text = t.y
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)                        # noqa: E731
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)                        # noqa: E731
    src_text = t.source(tables=True)                                              # (dense: every molecule is Lt long)
    pvh = pv_hidden.to(dev).to(BF)[qs.to(dev)].reshape(Up * Lp, H).contiguous()
    src_pv = KVSource(pvh, Up, Lp)
    # ---- the fusion batch: [P PV-query sequences, dense | P text-query sequences, packed]
    iq, im = inv_q.numpy(), inv_m.numpy()
    len_p, qrow0, Mt, _, _, gat_tx = t.pair_layout(lens_u, im)
    o_t = P * Lp
    gat_pv = (iq[:, None] * Lp + np.arange(Lp)[None, :]).reshape(-1)
    X = torch.cat([pvh.index_select(0, i64(gat_pv)), text.index_select(0, i64(gat_tx))])
    kv_m, kv_q = i32(im), i32(iq)
    qrow0_d, qlen_d = i32(qrow0), i32(len_p)
    g_lo = Batch([Group(0, P, Lp, None, P).bind(src_text, kv_m, 0),
                  Group(o_t, P, Lt, None, P, q_row0=qrow0_d, q_len=qlen_d, nrows=Mt).bind(src_pv, kv_q, 0)])
    y, _, _ = eng.stack_fwd(TP, ct, range(f, n - 1), True, X, g_lo, False)
    # ---- the last fusion layer on the 2 P position-0 rows; self-attention keys / values from every row of the layer below
    top_rows = np.concatenate([np.arange(P, dtype=np.int64) * Lp, o_t + qrow0])
    xt = y.index_select(0, i64(top_rows))
    skv = SelfKV(y)
    g_top = Batch([Group(0, P, 1, None, P, self_src=skv, skv_row0=i32(np.arange(P) * Lp), skv_len=i32(np.full(P, Lp)), skv_L=Lp).bind(src_text, kv_m, 0),
                   Group(P, P, 1, None, P, self_src=skv, skv_row0=i32(o_t + qrow0), skv_len=qlen_d, skv_L=Lt).bind(src_pv, kv_q, 0)])
    yt, _, _ = eng._layer_fwd(f"{TP}encoder.layer.{n - 1}.", ct, True, xt, g_top, False)
    vl = torch.cat([yt[:P], yt[P:]], dim=1)                                       # [P, 2H]: cat(cls_p, cls_t) of :201
    logits = ops.rows_linear(vl, eng.P.w("itm_head.weight"), eng.P.w("itm_head.bias"), torch.empty(P, 2, dtype=torch.float32, device=dev))
    return torch.softmax(logits, dim=1)[:, 1]


def _match_dense(model, pv_hidden, ids_h, mask_h, pairs_h) -> torch.Tensor:
    """`match_scores(engine=False)`: written against the module API (text_encoder.bert, itm_head), so it runs on any object that has it."""
    dev = pv_hidden.device
    m_sel = pairs_h[:, 1]
    L = max(1, int(mask_h[m_sel].sum(1).max()))
    ids, mask = ids_h[m_sel, :L].to(dev), mask_h[m_sel, :L].to(dev)
    pv = pv_hidden[pairs_h[:, 0].to(dev)].float()
    ones = torch.ones(pv.shape[:2], dtype=torch.long, device=dev)
    bert = model.text_encoder.bert
    text = bert(ids, attention_mask=mask, return_dict=True, mode="text").last_hidden_state
    cls_p = bert(encoder_embeds=pv, attention_mask=ones, encoder_hidden_states=text, encoder_attention_mask=mask, return_dict=True,
                 mode="fusion").last_hidden_state[:, 0, :]
    cls_t = bert(encoder_embeds=text, attention_mask=mask, encoder_hidden_states=pv, encoder_attention_mask=ones, return_dict=True,
                 mode="fusion").last_hidden_state[:, 0, :]
    logits = model.itm_head(torch.cat([cls_p, cls_t], dim=-1))
    return torch.softmax(logits.float(), dim=-1)[:, 1]


# ------------------------------------------------------------------------------------------------------------------ both stages
@dataclass
class Retrieved:
    """Per query: the k shortlisted library indices (input order of the library; -1 beyond its size) with their cosine similarity; the
    first `rerank` of them are ordered by matching probability (`match`, NaN for the rest) or -- rerank_by='likelihood' -- by the
    teacher-forced log-likelihood per token under the query (`logp_per_token`, NaN for the rest; `match` is then all NaN)."""
    index: torch.Tensor        # int64 [Q, k]
    cosine: torch.Tensor       # fp32 [Q, k]
    match: torch.Tensor        # fp32 [Q, k]
    logp_per_token: Optional[torch.Tensor] = None      # fp32 [Q, k], rerank_by='likelihood' only


def _as_index(index_or_feats) -> MoleculeIndex:
    return index_or_feats if isinstance(index_or_feats, MoleculeIndex) else MoleculeIndex(index_or_feats)


@torch.no_grad()
def retrieve(model, index_or_feats, library_ids, library_mask, pv, prop_mask=None, k: int = 100, rerank: int = 16, chunk: int = 1 << 20,
             rerank_by: str = "match") -> Retrieved:
    """Molecules of the library whose properties match `pv` ([Q, n_props] normalised; prop_mask: 1 = unspecified).  library_ids /
    library_mask: the library's padded tokens in the index's order (None: the index's own).  rerank_by: 'match' orders the head of the
    shortlist by the matching head's probability, 'likelihood' by log p(SMILES | PV) per token (spmm_amd.score.score_smiles)."""
    if rerank_by not in ("match", "likelihood"):
        raise ValueError(f"rerank_by={rerank_by!r}: 'match' or 'likelihood'")
    index = _as_index(index_or_feats)
    library_ids = index.ids if library_ids is None else library_ids
    library_mask = index.mask if library_mask is None else library_mask
    qf, hidden = pv_features(model, pv, prop_mask)
    scores, idx = index.search(qf, k, chunk=chunk)
    if rerank_by == "likelihood":
        return _rerank_likelihood(model, pv, prop_mask, library_ids, library_mask, scores, idx, rerank)
    return _rerank(model, hidden, library_ids, library_mask, scores, idx, rerank)


def _rerank_likelihood(model, pv, prop_mask, library_ids, library_mask, scores, idx, rerank) -> Retrieved:
    from .score import score_smiles
    Q, k = idx.shape
    nan = torch.full((Q, k), float("nan"), dtype=torch.float32, device=idx.device)
    per = nan.clone()
    r = min(int(rerank), k)
    if r > 0:
        if library_ids is None or library_mask is None:
            raise ValueError("re-ranking needs the library's token ids and mask (or rerank=0)")
        head = idx[:, :r].cpu()
        qq, jj = torch.nonzero(head >= 0, as_tuple=True)
        if qq.numel():
            sc = score_smiles(model, pv.reshape(Q, -1), library_ids, library_mask, pairs=torch.stack([qq, head[qq, jj]], dim=1), prop_mask=prop_mask)
            per[qq.to(idx.device), jj.to(idx.device)] = sc.per_token().to(idx.device)
            # log-likelihood per token, largest first; equal values keep the shortlist's order; empty slots stay last
            order = torch.sort(torch.nan_to_num(per[:, :r], nan=-float("inf")), dim=1, descending=True, stable=True).indices
            idx, scores = idx.clone(), scores.clone()
            idx[:, :r] = idx[:, :r].gather(1, order)
            scores[:, :r] = scores[:, :r].gather(1, order)
            per[:, :r] = per[:, :r].gather(1, order)
    return Retrieved(idx, scores, nan, per)


def _rerank(model, hidden, library_ids, library_mask, scores, idx, rerank) -> Retrieved:
    Q, k = idx.shape
    match = torch.full((Q, k), float("nan"), dtype=torch.float32, device=idx.device)
    r = min(int(rerank), k)
    if r > 0:
        if library_ids is None or library_mask is None:
            raise ValueError("re-ranking needs the library's token ids and mask (or rerank=0)")
        head = idx[:, :r].cpu()
        qq, jj = torch.nonzero(head >= 0, as_tuple=True)
        if qq.numel():
            prob = match_scores(model, hidden, library_ids, library_mask, torch.stack([qq, head[qq, jj]], dim=1))
            match[qq.to(idx.device), jj.to(idx.device)] = prob
            # matching probability, largest first; equal probabilities keep the shortlist's order; empty slots stay last
            order = torch.sort(torch.nan_to_num(match[:, :r], nan=-1.0), dim=1, descending=True, stable=True).indices
            idx, scores, match = idx.clone(), scores.clone(), match.clone()
            idx[:, :r] = idx[:, :r].gather(1, order)
            scores[:, :r] = scores[:, :r].gather(1, order)
            match[:, :r] = match[:, :r].gather(1, order)
    return Retrieved(idx, scores, match)


@torch.no_grad()
def similar(model, index_or_feats, ids: torch.Tensor, mask: torch.Tensor, k: int, chunk: int = 1 << 20) -> Tuple[torch.Tensor, torch.Tensor]:
    """Molecule-to-molecule neighbours on the t2t similarity (SPMM_models.py:111): the search with text features as queries."""
    return _as_index(index_or_feats).search(smiles_features(model, ids, mask), k, chunk=chunk)
