"""Likelihood scoring on one MI355X at the published size (H = 768, 12 text layers, fusion from layer 6, 6 property layers), seeded random
weights, molecules of 30 .. 100 tokens, in one process:

  workloads   one property vector against 4 096 molecules;  64 vectors x 64 molecules each (4 096 pairs, 4 096 distinct molecules)
  variants    score_smiles(engine=True, fused=True)   the engine path ending in spmm_lm_score (csrc/score.hip)
              score_smiles(engine=True, fused=False)  the same path ending in lm_head_fwd, log_softmax and a gather in torch
              score_smiles(engine=False)              the dense module-facade call on the pairs as a padded batch (--dense_chunk pairs at a time)
  and, on the rows of each workload alone, the two endings from the decoder's output on (`score.lm_ending`: transform head included in both).

Every timed window is bracketed by device events; the variants alternate inside each of the `--pairs` rounds; the figure is the median
window, the spread (max - min over median) is reported beside it.  Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from spmm_amd import score as S
from spmm_amd.config import BertConfig, SPMMConfig
from spmm_amd.model import SPMM

ap = argparse.ArgumentParser()
ap.add_argument("--molecules", type=int, default=4096, help="workload 1: molecules under one vector")
ap.add_argument("--vectors", type=int, default=64, help="workload 2: vectors ...")
ap.add_argument("--each", type=int, default=64, help="... and molecules under each")
ap.add_argument("--pairs", type=int, default=5, help="rounds of alternating windows")
ap.add_argument("--dense_chunk", type=int, default=1024, help="pairs per engine=False call (the padded batch's activations are chunked)")
ap.add_argument("--ending_reps", type=int, default=10)
ap.add_argument("--tiny", type=int, default=0, help="1: the 2-layer / 128-d configuration (a rehearsal of the tool, not a measurement)")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_score.py measures on the GPU: no device found (spmm_amd has no CPU / eager fallback)")
dev = torch.device("cuda")
torch.manual_seed(0)


def window(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def alternate(fns, reps=1):
    """fns: {name: callable} -> ({name: (median ms, spread)}, {name: last output}): one warm-up of each, then alternating windows."""
    outs, times = {}, {k: [] for k in fns}
    for k, fn in fns.items():
        window(fn)
    for _ in range(a.pairs):
        for k, fn in fns.items():
            t, outs[k] = window(fn, reps)
            times[k].append(t)
    return {k: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for k, t in times.items()}, outs


if a.tiny:
    from spmm_amd.config import tiny_config
    cfg = tiny_config()
else:
    cfg = SPMMConfig(text=BertConfig(num_hidden_layers=12, fusion_layer=6, add_cross_attention=True),
                     prop=BertConfig(num_hidden_layers=6, fusion_layer=6, vocab_size=1), embed_dim=256, queue_size=36864)
m = SPMM(spmm_config=cfg, no_train=True).eval()
m.store.refresh_shadows()
eng = m.engine
gh = torch.Generator().manual_seed(2)


def molecules(n):
    lens = torch.randint(30, 101, (n,), generator=gh)
    ids = torch.zeros(n, 100, dtype=torch.long)
    for b, ln in enumerate(lens.tolist()):
        ids[b, 0] = 2
        ids[b, 1:ln - 1] = torch.randint(4, cfg.text.vocab_size, (ln - 2,), generator=gh)
        ids[b, ln - 1] = 3
    return ids, (ids != 0).long()


def dense(pv, ids, mask, pairs):
    parts = [S.score_smiles(m, pv, ids, mask, pairs[i:i + a.dense_chunk], engine=False) for i in range(0, pairs.shape[0], a.dense_chunk)]
    return S.Scores(torch.cat([p.logp for p in parts]), torch.cat([p.n_tokens for p in parts]), torch.cat([p.token_logp for p in parts]))


def workload(name, n_vec, n_each):
    n = n_vec * n_each
    ids, mask = molecules(n)
    pv = torch.randn(n_vec, cfg.n_props, generator=gh).to(dev)
    pairs = torch.stack([torch.arange(n_vec).repeat_interleave(n_each), torch.arange(n)], dim=1)
    t, o = alternate({"engine_fused": lambda: S.score_smiles(m, pv, ids, mask, pairs),
                      "engine_composite": lambda: S.score_smiles(m, pv, ids, mask, pairs, fused=False),
                      "dense": lambda: dense(pv, ids, mask, pairs)})
    rows = int(mask.sum())
    entry = {"vectors": n_vec, "molecules_per_vector": n_each, "pairs": n, "rows": rows, "tokens": "30..100"}
    for k, (ms, spread) in t.items():
        entry[k + "_ms"], entry[k + "_spread"] = round(ms, 2), round(spread, 4)
    entry["fused_over_composite"] = round(t["engine_composite"][0] / t["engine_fused"][0], 4)
    entry["engine_fused_over_dense"] = round(t["dense"][0] / t["engine_fused"][0], 3)
    entry["max_abs_logp_per_token_fused_vs_composite"] = float((o["engine_fused"].per_token() - o["engine_composite"].per_token()).abs().max())
    entry["max_abs_logp_per_token_fused_vs_dense"] = float((o["engine_fused"].per_token() - o["dense"].per_token()).abs().max())
    # ---- the two endings alone, on this workload's rows (random decoder output)
    lens = mask.sum(1)
    H, Lt = cfg.text.hidden_size, int(lens.max())
    seq = torch.arange(n).repeat_interleave(lens)
    pos = torch.cat([torch.arange(int(ln)) for ln in lens])
    row0 = torch.cumsum(lens, 0) - lens
    lay = dict(P=n, Lt=Lt, W=Lt, row_of=(seq * Lt + pos).to(dev), pos=pos.to(dev), dest=(seq * Lt + pos).to(dev), seq_row0=row0.to(torch.int32).to(dev),
               seq_len=lens.to(torch.int32).to(dev), ids=ids[:, :Lt].to(torch.int32).to(dev).contiguous())
    y = torch.randn(rows, H, device=dev).to(torch.bfloat16)
    te, _ = alternate({"fused": lambda: S.lm_ending(eng, cfg.text, y, lay, True), "composite": lambda: S.lm_ending(eng, cfg.text, y, lay, False)}, a.ending_reps)
    entry["ending_only"] = {"rows": rows, "fused_ms": round(te["fused"][0], 4), "composite_ms": round(te["composite"][0], 4),
                            "fused_spread": round(te["fused"][1], 4), "composite_spread": round(te["composite"][1], 4),
                            "composite_over_fused": round(te["composite"][0] / te["fused"][0], 3),
                            "logits_bytes_not_written": rows * cfg.text.vocab_size * 4}
    res[name] = entry


res = {"device": torch.cuda.get_device_name(0), "pairs_rounds": a.pairs, "dense_chunk": a.dense_chunk, "tiny": a.tiny,
       "H": cfg.text.hidden_size, "V": cfg.text.vocab_size}
workload("one_vector", 1, a.molecules)
workload("many_vectors", a.vectors, a.each)
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
