"""TEST INFRASTRUCTURE (never imported by spmm_amd/): cross-attention probabilities as the reference computes them
(BertSelfAttention.forward xbert.py:305-340 up to `attention_probs`, encoder mask of invert_attention_mask :1038-1043), restated on the CPU.

  probs            the kernel's contract (spmm_attn_probs) in float64 on given Q / K and layout arrays, written sequence by sequence and
                   head by head; `defect` seeds one of six mistakes a kernel could make (tests/test_attention_maps_cpu.py shows the
                   comparison of tests/test_attn_probs_gpu.py rejects each of them)
  kernel_cases     the fixed inputs of the kernel tests (bf16-representable values, seeded)
  attention_probs / attention_from_probs
                   oracle.spmm_oracle.attention split at `pr`, the tensor it computes and discards
  fusion_maps / reaction_maps
                   the fusion and decoder passes restated on the oracle's own pieces (`_lin`, `attention`, bert_layer's structure,
                   `inverted_enc_mask`), one pair at a time at its own lengths, returning that `pr` per layer
  path_case / rxn_case   the fixed small inputs of the path tests"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

import spmm_oracle as O

TP = "text_encoder.bert."
DEFECTS = ("scale", "mean_before_softmax", "self_mask", "kv_len_off_by_one", "kv_seq_ignored", "next_head_k")

# Largest |kernel - float64| on a probability over every case of tests/test_attn_probs_gpu.py, measured on an MI355X, and the
# absolute tolerance derived from it (4 x: other seeds, another compiler's instruction order).  The issue's condition: below 1e-4.
KERNEL_DEV_MEASURED = 1.2e-7          # 1.197e-7, per head, at dense-2x12x54x128
KERNEL_TOL = 4 * KERNEL_DEV_MEASURED
TOL_CEILING = 1e-4


# ---------------------------------------------------------------------------------------------------------------- the kernel's contract
def probs(Q: torch.Tensor, K: torch.Tensor, *, nseq: int, nH: int, Lq: int, Lkv: int, kmask=None, kv_seq=None, q_row0=None, q_len=None,
          kv_row0=None, kv_len=None, defect: Optional[str] = None) -> dict:
    """Q [query rows, >= nH*64], K [source rows, >= nH*64] (any float dtype; read as float64).  -> dict(mean float64 [rows, Lkv], heads
    float64 [nH, rows, Lkv], owned bool [rows]: the row belongs to a sequence, keys bool [rows, Lkv]: the key is not masked).  Entries of
    rows that belong to no sequence are 0 and not to be compared."""
    assert defect is None or defect in DEFECTS
    Q64, K64 = Q.double(), K.double()
    rows = Q.shape[0]
    heads = torch.zeros(nH, rows, Lkv, dtype=torch.float64)
    owned = torch.zeros(rows, dtype=torch.bool)
    keys = torch.zeros(rows, Lkv, dtype=torch.bool)
    d = 32 if defect == "scale" else 64
    for s in range(nseq):
        u = int(kv_seq[s]) if (kv_seq is not None and defect != "kv_seq_ignored") else s
        if defect == "kv_seq_ignored" and kv_len is not None:
            u = s % len(kv_len)                                           # (fewer sources than query sequences: stay inside them)
        nq = int(q_len[s]) if q_len is not None else Lq
        r0 = int(q_row0[s]) if q_row0 is not None else s * Lq
        nk = int(kv_len[u]) if kv_len is not None else Lkv
        k0 = int(kv_row0[u]) if kv_row0 is not None else u * Lkv
        ok = torch.zeros(Lkv, dtype=torch.bool)
        ok[:nk] = True
        if kmask is not None:
            ok &= kmask[s, :Lkv] != 0
        if defect == "kv_len_off_by_one" and bool(ok.any()):
            ok[int(torch.nonzero(ok).max())] = False                     # the last valid key is lost
        owned[r0:r0 + nq] = True
        keys[r0:r0 + nq] = ok
        if nk == 0:
            continue
        sc = []
        for h in range(nH):
            hk = (h + 1) % nH if defect == "next_head_k" else h
            q = Q64[r0:r0 + nq, h * 64:(h + 1) * 64]
            k = K64[k0:k0 + nk, hk * 64:(hk + 1) * 64]
            x = torch.full((nq, Lkv), -math.inf, dtype=torch.float64)
            x[:, :nk] = q @ k.T / math.sqrt(d)
            if defect == "self_mask":                                     # additive -10000 on the keys kmask strikes (-inf past the source stays)
                x = x + torch.where(ok, 0.0, -10000.0).to(torch.float64)[None, :]
            else:
                x = torch.where(ok[None, :], x, torch.full_like(x, -math.inf))
            sc.append(x)
        if defect == "mean_before_softmax":
            m = torch.stack(sc).mean(0)
            sc = [m for _ in range(nH)]
        for h in range(nH):
            x = sc[h]
            alive = torch.isfinite(x).any(dim=1, keepdim=True)            # a row with every key masked: zeros
            p = torch.softmax(torch.where(alive, x, torch.zeros_like(x)), dim=1)
            heads[h, r0:r0 + nq] = torch.where(alive & torch.isfinite(x), p, torch.zeros_like(p))
    return dict(mean=heads.mean(0), heads=heads, owned=owned, keys=keys)


def _bf(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(torch.float32)


DENSE = [(1, 1, 1, 1), (2, 2, 16, 16), (2, 2, 17, 15), (3, 2, 54, 77), (2, 3, 100, 54), (2, 12, 54, 128), (2, 2, 256, 54), (2, 2, 54, 256),
         (2, 2, 130, 129), (1, 16, 33, 65)]
AGREE_CASES = ("dense-2x2x17x15", "dense-3x2x54x77", "packed-shared", "packed-text")     # cases also compared with ops.attn_fwd


def _dense_case(name, nseq, nH, Lq, Lkv, lens, g):
    H = nH * 64
    kmask = (torch.arange(Lkv)[None, :] < torch.tensor(lens)[:, None]).to(torch.int32)
    return dict(name=name, nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, Qbuf=_bf((nseq * Lq, H), g), qcol=0, Kbuf=_bf((nseq * Lkv, H), g), kcol=0,
                V=_bf((nseq * Lkv, H), g), kmask=kmask, kv_seq=None, q_row0=None, q_len=None, kv_row0=None, kv_len=None, ldp=Lkv)


def kernel_cases() -> List[dict]:
    """Every case: Qbuf / Kbuf (fp32 holding bf16 values; Q = Qbuf[:, qcol : qcol + nH*64], the same for K), V [source rows, nH*64], the
    layout arrays (int32 or None) and ldp.  Dense cases: kmask prefixes of lengths drawn in [1, Lkv], the first sequence at full length
    and the last at length 1 (a case of ONE sequence runs twice: full length, length 1)."""
    g = torch.Generator().manual_seed(20)
    out = []
    for nseq, nH, Lq, Lkv in DENSE:
        name = f"dense-{nseq}x{nH}x{Lq}x{Lkv}"
        if nseq == 1:
            out.append(_dense_case(name + ("" if Lkv == 1 else "-full"), 1, nH, Lq, Lkv, [Lkv], g))
            if Lkv > 1:
                out.append(_dense_case(name + "-len1", 1, nH, Lq, Lkv, [1], g))
            continue
        lens = [Lkv] + [int(torch.randint(1, Lkv + 1, (1,), generator=g)) for _ in range(nseq - 2)] + [1]
        out.append(_dense_case(name, nseq, nH, Lq, Lkv, lens, g))
    # a row with every key masked: sequence 1 of the 17 x 15 case
    c = _dense_case("dense-allmasked", 2, 2, 17, 15, [9, 0], g)
    out.append(c)
    # packed, shared sources: 5 query sequences over 3 sources; Q / K are column blocks of fused [M, 3H] / [M, 2H] buffers; ldp > Lkv
    nH, H = 2, 128
    ql, kl, kvs = [1, 2, 31, 64, 65], [1, 54, 200], [0, 1, 2, 1, 2]
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)                                                          # noqa: E731
    cum = lambda a: [sum(a[:i]) for i in range(len(a))]                                                           # noqa: E731
    out.append(dict(name="packed-shared", nseq=5, nH=nH, Lq=65, Lkv=200, Qbuf=_bf((sum(ql), 3 * H), g), qcol=0, Kbuf=_bf((sum(kl), 2 * H), g),
                    kcol=0, V=None, kmask=None, kv_seq=i32(kvs), q_row0=i32(cum(ql)), q_len=i32(ql), kv_row0=i32(cum(kl)), kv_len=i32(kl),
                    ldp=203))
    # packed, the text-query direction: query lengths 2 .. Lt over dense sources of 54 rows
    ql = [2, 3, 20, 23, 24]
    out.append(dict(name="packed-text", nseq=5, nH=nH, Lq=24, Lkv=54, Qbuf=_bf((sum(ql), 3 * H), g), qcol=H, Kbuf=_bf((3 * 54, 2 * H), g),
                    kcol=H, V=None, kmask=None, kv_seq=i32([0, 0, 1, 2, 2]), q_row0=i32(cum(ql)), q_len=i32(ql), kv_row0=i32([0, 54, 108]),
                    kv_len=i32([54, 54, 54]), ldp=54))
    for c in out:
        if c["V"] is None:
            c["V"] = _bf((c["Kbuf"].shape[0], c["nH"] * 64), g)
    return out


def case_qk(c) -> Tuple[torch.Tensor, torch.Tensor]:
    H = c["nH"] * 64
    return c["Qbuf"][:, c["qcol"]:c["qcol"] + H], c["Kbuf"][:, c["kcol"]:c["kcol"] + H]


def case_layout(c) -> dict:
    return {k: c[k] for k in ("nseq", "nH", "Lq", "Lkv", "kmask", "kv_seq", "q_row0", "q_len", "kv_row0", "kv_len")}


def defect_applies(c, defect: str) -> bool:
    """Where a seeded defect changes the arithmetic at all.  A row with ONE key is 1.0 under any score; one head has no other head; a case
    without kv_seq has nothing to ignore; -10000 in place of the cross mask's -inf / finfo.min changes nothing unless EVERY key of a row is
    masked (exp(-10000 - max) underflows to 0 in float32 and float64 alike): that defect shows at the all-masked case alone."""
    single_key = c["Lkv"] == 1 or (c["kmask"] is not None and int(c["kmask"].sum(1).max()) <= 1)
    if defect == "scale":
        return not single_key
    if defect in ("mean_before_softmax", "next_head_k"):
        return c["nH"] > 1 and not single_key
    if defect == "self_mask":
        return c["name"] == "dense-allmasked"
    if defect == "kv_seq_ignored":
        return c["kv_seq"] is not None
    return True


def compare(got: dict, ref: dict) -> float:
    """Largest |difference| of head mean and per-head values over the rows that belong to a sequence (the kernel test's comparison)."""
    o = ref["owned"]
    return max((got["mean"][o] - ref["mean"][o]).abs().max().item(), (got["heads"][:, o] - ref["heads"][:, o]).abs().max().item())


# ---------------------------------------------------------------------------------------------------------------- the oracle, split at pr
def attention_probs(sd, p: str, c, hidden: torch.Tensor, add_mask: torch.Tensor, enc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The `pr` of oracle.attention (eval mode): [B, nH, L, Lkv]."""
    B, L, H = hidden.shape
    nh, d = c.num_attention_heads, H // c.num_attention_heads
    kv_src = hidden if enc is None else enc
    q = O._lin(sd, p + ".self.query", hidden).view(B, L, nh, d).permute(0, 2, 1, 3)
    k = O._lin(sd, p + ".self.key", kv_src).view(B, -1, nh, d).permute(0, 2, 1, 3)
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(d) + add_mask
    return torch.softmax(s, dim=-1)


def attention_from_probs(sd, p: str, c, hidden: torch.Tensor, pr: torch.Tensor, enc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What oracle.attention makes of `pr`: context, output projection, residual LayerNorm."""
    B, L, H = hidden.shape
    nh, d = c.num_attention_heads, H // c.num_attention_heads
    kv_src = hidden if enc is None else enc
    v = O._lin(sd, p + ".self.value", kv_src).view(B, -1, nh, d).permute(0, 2, 1, 3)
    ctx = torch.matmul(pr, v).permute(0, 2, 1, 3).reshape(B, L, H)
    return O._ln(sd, p + ".output.LayerNorm", O._lin(sd, p + ".output.dense", ctx) + hidden, c.layer_norm_eps)


def _cross_layers(sd, p: str, c, x: torch.Tensor, self_mask: torch.Tensor, enc: torch.Tensor, lo: int) -> Dict[int, torch.Tensor]:
    """Layers lo .. n - 1 of bert_layer's structure on one sequence x [1, L, H] cross-attending enc [1, Lkv, H] (no padding: masks of
    ones) -> {index among the cross-attending layers: pr [nH, L, Lkv]}."""
    emask = O.inverted_enc_mask(torch.ones(enc.shape[:2]))
    out = {}
    for i in range(lo, c.num_hidden_layers):
        lp = f"{p}encoder.layer.{i}."
        a = O.attention(sd, lp + "attention", c, x, self_mask)
        if i >= c.fusion_layer:
            out[i - c.fusion_layer] = attention_probs(sd, lp + "crossattention", c, a, emask, enc)[0]
            a = O.attention(sd, lp + "crossattention", c, a, emask, enc)
        h = O._lin(sd, lp + "intermediate.dense", a, act=F.gelu)
        x = O._ln(sd, lp + "output.LayerNorm", O._lin(sd, lp + "output.dense", h) + a, c.layer_norm_eps)
    return out


@torch.no_grad()
def fusion_maps(sd, cfg, pv, prop_mask, ids, mask, pairs) -> List[Dict[Tuple[int, str], torch.Tensor]]:
    """Per pair {(fusion layer index, direction): pr fp32 [nH, Lq, Lkv]}: 'pv2text' [nH, n_props + 1, tokens], 'text2pv' the other way."""
    import retrieve_reference as R
    tc = cfg.text
    pv_h = R.pv_hidden(sd, cfg, pv, prop_mask)
    rows = R._rows(ids, mask)
    out = []
    for qi, mi in pairs.tolist():
        pvx, text = pv_h[qi:qi + 1], R.text_hidden(sd, cfg, rows[mi])
        sm_p = O.extended_self_mask(torch.ones(pvx.shape[:2]), False)
        sm_t = O.extended_self_mask(torch.ones(text.shape[:2]), False)
        d = {}
        for li, pr in _cross_layers(sd, TP, tc, pvx, sm_p, text, tc.fusion_layer).items():
            d[(li, "pv2text")] = pr
        for li, pr in _cross_layers(sd, TP, tc, text, sm_t, pvx, tc.fusion_layer).items():
            d[(li, "text2pv")] = pr
        out.append(d)
    return out


@torch.no_grad()
def reaction_maps(sd, c_dec, c_enc, sids, smask, pids, pmask, pairs) -> List[Dict[int, torch.Tensor]]:
    """Per pair {decoder cross-attention layer index: pr fp32 [nH, product tokens, reactant tokens]} of the teacher-forced decoder pass."""
    import rxn_reference as X
    out = []
    for si, ci in pairs.tolist():
        ls, lc = int(smask[si].sum()), int(pmask[ci].sum())
        enc = X.encode(sd, c_enc, sids[si:si + 1, :ls], torch.ones(1, ls, dtype=torch.long))
        x = O.embeddings(sd, X.DEC + "bert.", c_dec, input_ids=pids[ci:ci + 1, :lc])
        sm = O.extended_self_mask(torch.ones(1, lc), True)
        out.append(_cross_layers(sd, X.DEC + "bert.", c_dec, x, sm, enc, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------- the path cases
WEIGHT_SEED = 3


def path_case():
    """tests/retrieve_reference.path_case: molecules of 2, 3, 20, Lt - 1 and Lt tokens, 3 PVs (the third with 20 properties masked), 7
    pairs with repeats on both sides."""
    import retrieve_reference as R
    return R.path_case()


def rxn_case():
    """Three reactions: sources of 3, 30 and 149 tokens, products of 2, 20 and 99 ([CLS] first, [SEP] last), paired in order."""
    g = torch.Generator().manual_seed(77)

    def rows(lens, cls):
        ids = torch.zeros(len(lens), max(lens), dtype=torch.long)
        for b, n in enumerate(lens):
            ids[b, :n] = torch.randint(4, 300, (n,), generator=g)
            if cls:
                ids[b, 0], ids[b, n - 1] = 2, 3
        return ids, (ids != 0).long()
    sids, smask = rows([3, 30, 149], False)
    pids, pmask = rows([2, 20, 99], True)
    return sids, smask, pids, pmask, torch.tensor([[0, 0], [1, 1], [2, 2]], dtype=torch.long)


SHARPEN = 6.0


def sharpen(sd, scale: float = SHARPEN):
    """A copy of the state dict with every cross-attention query and key weight times `scale`.  The seeded initialisers draw weights small
    enough that every cross-attention score is near 0 and every map near uniform (largest / smallest weight of a row below 1.5 in every
    row): any kernel, a wrong one included, would reproduce a uniform map.  Scores grow with scale^2; at 6 at least 80 % of the rows of
    every map of `path_case` have a ratio above 1.5 and the largest weight is 0.996."""
    sd = dict(sd)
    for k in list(sd):
        if k.endswith(("crossattention.self.query.weight", "crossattention.self.key.weight")):
            sd[k] = sd[k] * scale
    return sd


def path_state_dict(oc):
    return sharpen(O.init_state_dict(oc, seed=WEIGHT_SEED))


def rxn_state_dict(o_dec, o_enc):
    import rxn_reference as X
    return sharpen(X.random_state_dict(o_dec, o_enc, seed=1), 1.5)      # (these weights are drawn 4 x as large as init_state_dict's)


def contrast_share(m: torch.Tensor) -> float:
    """Share of the rows of a map [.., Lq, Lkv] (head mean of a 3-D one) whose largest weight is more than 1.5 x its smallest."""
    mm = m.mean(0) if m.dim() == 3 else m
    return (mm.max(1).values > 1.5 * mm.min(1).values).float().mean().item()
