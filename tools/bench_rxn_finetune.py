"""Times seq2seq fine-tuning steps of the reaction model at the published size (H = 768, 6 encoder layers, 12 decoder layers with
cross-attention in the upper 6) on one GPU: the HIP step (spmm_amd.rxn.SPMMRxn(trainable=True).train_step: forward, backward and the fused
AdamW, padding rows packed away) against an eager PyTorch encoder-decoder of the same shape (nn.TransformerEncoderLayer /
nn.TransformerDecoderLayer, bf16 autocast, torch.optim.AdamW, padded batches as the reference runs them), alternating the two in one
process.  Sources of 30..149 tokens, products of 20..99.  Per step: device time, host enqueue time and GPU-busy time as
tools/bench_finetune.py defines them.  When device time tracks enqueue time and the GPU-busy time is smaller, the step is host-bound.
Prints ONE JSON line.

  python tools/bench_rxn_finetune.py [--steps 20] [--warmup 6] [--rounds 3] [--batches 16 64]"""
import argparse
import json
import os
import sys

import torch
from torch import nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_finetune import gpu_busy, host_syncs, timed      # noqa: E402


class _SelfOnlyLayer(nn.Module):
    """A decoder layer of the lower half: self-attention and FFN only (BertLayer below fusion_layer), post-LN."""

    def __init__(self, H, nH, I, p):
        super().__init__()
        self.layer = nn.TransformerEncoderLayer(H, nH, I, p, activation="gelu", batch_first=True, norm_first=False, layer_norm_eps=1e-12)

    def forward(self, x, causal, pad):
        return self.layer(x, src_mask=causal, src_key_padding_mask=pad)


class EagerSeq2Seq(nn.Module):
    """SPMM_rxn as torch.nn modules: a 6-layer encoder, a 12-layer causal decoder whose upper 6 layers cross-attend the encoder output,
    BertOnlyMLMHead with the tied decoder, CrossEntropyLoss(ignore_index=0) on the shifted product."""

    def __init__(self, V=300, H=768, nH=12, I=3072, enc_layers=6, dec_layers=12, fusion=6, p=0.1):
        super().__init__()
        def emb():
            return nn.ModuleDict(dict(word=nn.Embedding(V, H, padding_idx=0), pos=nn.Embedding(512, H), typ=nn.Embedding(2, H), ln=nn.LayerNorm(H, eps=1e-12)))
        self.e_src, self.e_prd, self.drop = emb(), emb(), nn.Dropout(p)
        self.enc = nn.ModuleList([nn.TransformerEncoderLayer(H, nH, I, p, activation="gelu", batch_first=True, norm_first=False,
                                                             layer_norm_eps=1e-12) for _ in range(enc_layers)])
        self.dec_lo = nn.ModuleList([_SelfOnlyLayer(H, nH, I, p) for _ in range(fusion)])
        self.dec_hi = nn.ModuleList([nn.TransformerDecoderLayer(H, nH, I, p, activation="gelu", batch_first=True, norm_first=False,
                                                                layer_norm_eps=1e-12) for _ in range(dec_layers - fusion)])
        self.tf, self.tf_ln, self.bias = nn.Linear(H, H), nn.LayerNorm(H, eps=1e-12), nn.Parameter(torch.zeros(V))

    def _embed(self, e, ids):
        return self.drop(e["ln"](e["word"](ids) + e["pos"].weight[:ids.shape[1]] + e["typ"].weight[0]))

    def forward(self, src, smask, prd, pmask):
        spad, ppad = smask == 0, pmask == 0
        mem = self._embed(self.e_src, src)
        for layer in self.enc:
            mem = layer(mem, src_key_padding_mask=spad)
        L = prd.shape[1]
        causal = torch.triu(torch.ones(L, L, dtype=torch.bool, device=prd.device), 1)
        x = self._embed(self.e_prd, prd)
        for layer in self.dec_lo:
            x = layer(x, causal, ppad)
        for layer in self.dec_hi:
            x = layer(x, mem, tgt_mask=causal, tgt_key_padding_mask=ppad, memory_key_padding_mask=spad)
        h = self.tf_ln(F.gelu(self.tf(x)))
        logits = F.linear(h, self.e_prd["word"].weight, self.bias)[:, :-1]
        return F.cross_entropy(logits.float().permute(0, 2, 1), prd[:, 1:], ignore_index=0)


def _seqs(g, B, lo, hi, V):
    lens = torch.randint(lo, hi + 1, (B,), generator=g)
    ids = torch.zeros(B, int(lens.max()), dtype=torch.long)
    for i in range(B):
        n = int(lens[i])
        ids[i, 0] = 2
        ids[i, 1:n - 1] = torch.randint(4, V, (n - 2,), generator=g)
        ids[i, n - 1] = 3
    return ids


def make_batches(n, B, seed, V=300):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        src, prd = _seqs(g, B, 30, 149, V), _seqs(g, B, 20, 99, V)
        sm, pm = (src != 0).long(), (prd != 0).long()
        out.append((src.cuda(), sm.cuda(), prd.cuda(), pm.cuda(), int(sm.sum()), int(pm.sum()), src.numel() + prd.numel()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rxn_finetune.py needs a GPU")
    from spmm_amd.config import BertConfig
    from spmm_amd.rxn import SPMMRxn
    torch.manual_seed(0)
    cfg = BertConfig.from_json_file(os.path.join(ROOT, "configs", "config_bert.json"))
    hip = SPMMRxn(bert_config=cfg, trainable=True).train()
    eager = EagerSeq2Seq(enc_layers=cfg.fusion_layer, dec_layers=cfg.num_hidden_layers, fusion=cfg.fusion_layer).cuda().train()
    opt = torch.optim.AdamW(eager.parameters(), lr=1e-4, weight_decay=0.02)

    def hip_step(b):                                 # (device masks + the host's token counts: nothing in the step waits for the GPU)
        hip.train_step(b[0], b[1], b[2], b[3], n_src_tokens=b[4], n_prod_tokens=b[5])

    def eager_step(b):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = eager(b[0], b[1], b[2], b[3])
        loss.backward()
        opt.step()

    results = []
    for B in a.batches:
        batches = make_batches(a.warmup + a.steps, B, seed=B)
        rows = {"hip": [], "eager": []}
        for _ in range(a.rounds):                        # alternating, so that neither side always runs on the warmer clocks
            rows["hip"].append(timed(hip_step, batches, a.warmup, a.steps))
            rows["eager"].append(timed(eager_step, batches, a.warmup, a.steps))
        med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
        busy_hip, cov_hip = gpu_busy(hip_step, batches, 6)
        busy_eager, cov_eager = gpu_busy(eager_step, batches, 6)
        hip_host_bound = bool(med["hip"][1] >= 0.9 * med["hip"][0] and busy_hip < 0.9 * med["hip"][0])
        results.append({"B": B, "mean_tokens": round(sum(b[4] + b[5] for b in batches) / len(batches), 1),
                        "mean_padded_tokens": round(sum(b[6] for b in batches) / len(batches), 1),
                        "hip_device_ms": round(med["hip"][0], 3), "hip_enqueue_ms": round(med["hip"][1], 3),
                        "eager_device_ms": round(med["eager"][0], 3), "eager_enqueue_ms": round(med["eager"][1], 3),
                        "eager_over_hip": round(med["eager"][0] / med["hip"][0], 3),
                        "hip_gpu_busy_ms": round(busy_hip, 3), "eager_gpu_busy_ms": round(busy_eager, 3),
                        "gpu_busy_window_covered": bool(cov_hip and cov_eager), "hip_host_bound": hip_host_bound,
                        "hip_step_host_syncs": host_syncs(hip_step, batches[0]),
                        "hip_device_ms_all": [round(r[0], 3) for r in rows["hip"]], "eager_device_ms_all": [round(r[0], 3) for r in rows["eager"]]})
    print(json.dumps({"tool": "bench_rxn_finetune", "H": cfg.hidden_size, "encoder_layers": cfg.fusion_layer, "decoder_layers": cfg.num_hidden_layers,
                      "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "source_lengths": "U[30,149]", "product_lengths": "U[20,99]",
                      "results": results, "graph_captured_step": "not measured", "device": torch.cuda.get_device_name()}))


if __name__ == "__main__":
    main()
