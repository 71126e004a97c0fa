"""Reaction-prediction search throughput: the engine path (decode.predict_products / greedy_products with cached=True: reactants encoded once
on packed rows, K/V cache, masked-memory cross-attention through spmm_decode_xattn, one-launch beam step) against the reference's loop over
the module facades (cached=False: the whole prefix re-run and the memory re-projected at every position; the beam search one reaction at a
time) on the same model and the same reactions, in reactions/s, for k-beam (`--k`) and greedy search.

One model at the published size (12-layer decoder, fusion from layer 6, 6-layer reactant encoder, H = 768) with seeded random weights (no
[SEP] to speak of: both paths decode `--max_steps` positions); `--reactions` synthetic sources of 30 .. 149 tokens in length-sorted
batches of `--batch`.  Per setting: one untimed pass of both paths (warm-up), then `--pairs` alternating A/B pairs, each pass -- all its
searches -- timed with device events; the figure is the median pass, the spread of the passes and the per-pair ratios are reported beside
it.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from spmm_amd import decode
from spmm_amd.config import BertConfig
from spmm_amd.rxn import SPMMRxn

ap = argparse.ArgumentParser()
ap.add_argument("--reactions", type=int, default=256)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--k", type=int, default=5)
ap.add_argument("--max_steps", type=int, default=100)
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--tiny", type=int, default=0, help="1: the 2-layer / 128-d configuration (a rehearsal of the tool, not a measurement)")
ap.add_argument("--searches", nargs="+", default=["beam", "greedy"], choices=["beam", "greedy"], help="which searches to time")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_rxn.py measures on the GPU: no device found (spmm_amd has no CPU / eager fallback)")

torch.manual_seed(0)
if a.tiny:
    from spmm_amd.config import tiny_config
    c_dec = tiny_config().text
else:
    c_dec = BertConfig(num_hidden_layers=12, fusion_layer=6, add_cross_attention=True)
m = SPMMRxn(bert_config=c_dec).eval()

g = torch.Generator().manual_seed(1)
lens = torch.randint(30, 150, (a.reactions,), generator=g)
rows = [[2] + torch.randint(4, c_dec.vocab_size, (n - 2,), generator=g).tolist() + [3] for n in lens.tolist()]
order = np.argsort(lens.numpy(), kind="stable")
batches = []
for i in range(0, len(order), a.batch):
    idx = order[i:i + a.batch]
    ids = torch.zeros(len(idx), max(len(rows[j]) for j in idx), dtype=torch.long)
    for r, j in enumerate(idx):
        ids[r, :len(rows[j])] = torch.tensor(rows[j])
    batches.append((ids, (ids != 0).long()))


def one_pass(greedy: bool, cached: bool):
    """-> (milliseconds by device events for every search of the run, results of the first batch)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    first = None
    e0.record()
    for ids, mask in batches:
        if not cached:
            ids, mask = ids.cuda(), mask.cuda()
        out = decode.greedy_products(m, ids, mask, max_steps=a.max_steps, cached=cached) if greedy else \
            decode.predict_products(m, ids, mask, k=a.k, max_steps=a.max_steps, cached=cached)
        first = out if first is None else first
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), first


res = {"reactions": a.reactions, "batch": a.batch, "k": a.k, "max_steps": a.max_steps, "pairs": a.pairs, "tiny": a.tiny,
       "source_tokens": [int(lens.min()), int(lens.max())], "device": torch.cuda.get_device_name(0)}
for name, greedy in ((f"beam_k{a.k}", False), ("greedy", True)):
    if ("greedy" if greedy else "beam") not in a.searches:
        continue
    _, ra = one_pass(greedy, True)             # warm-up, both paths
    _, rb = one_pass(greedy, False)
    ta, tb = [], []
    for _ in range(a.pairs):
        ta.append(one_pass(greedy, True)[0])
        tb.append(one_pass(greedy, False)[0])
    ma, mb = statistics.median(ta), statistics.median(tb)
    best = (lambda r: r) if greedy else (lambda r: r[0][1] if r else None)
    res[name] = {"engine_reactions_per_s": round(a.reactions / ma * 1e3, 2), "facade_loop_reactions_per_s": round(a.reactions / mb * 1e3, 2),
                 "engine_ms": [round(t, 1) for t in ta], "facade_loop_ms": [round(t, 1) for t in tb], "speedup": round(mb / ma, 2),
                 "speedup_of_pairs_min_max": [round(min(y / x for x, y in zip(ta, tb)), 2), round(max(y / x for x, y in zip(ta, tb)), 2)],
                 "spread_engine": round((max(ta) - min(ta)) / ma, 4), "spread_facade_loop": round((max(tb) - min(tb)) / mb, 4),
                 "engine_last_run": dict(decode.last_run),
                 "first_batch_identical_best": sum(int(best(x) == best(y)) for x, y in zip(ra, rb)), "first_batch": len(ra)}
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
