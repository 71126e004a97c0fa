"""Retrieval on one MI355X at the published size (H = 768, E = 256), seeded random weights, alternating A/B pairs in one process:

  (a) MoleculeIndex.search (spmm_sim_topk, csrc/retrieve.hip) against torch.topk(q @ feats.T, k) on the same fp32 features: N library rows,
      k = 100 (two passes of the 64-slot kernel) and k = 64 (one pass), Q = 1 and Q = 64; the peak device memory each needs on top of the
      features; the kernel's rate over ALL its passes against its roofline (N E 4 bytes per pass below the ridge Q ~ 40, 2 Q N E FLOP above it);
  (b) match_scores on the engine against engine=False (the dense module calls) for 64 queries x 16 candidates, library molecules of
      30 .. 100 tokens;
  (c) index build in molecules / s.

Every timed window is bracketed by device events and repeated `--pairs` times, A and B alternating; the figure is the median window, the
spread (max - min over median) is reported beside it.  Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from spmm_amd import retrieve as R
from spmm_amd.config import BertConfig, SPMMConfig
from spmm_amd.model import SPMM

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=1_000_000)
ap.add_argument("--E", type=int, default=256)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--Q", type=int, nargs="+", default=[1, 64])
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--reps", type=int, default=10, help="searches per timed window")
ap.add_argument("--queries", type=int, default=64)
ap.add_argument("--candidates", type=int, default=16)
ap.add_argument("--library", type=int, default=4096, help="molecules of the matching / build benchmark's library")
ap.add_argument("--build", type=int, default=20000, help="molecules of the index-build benchmark")
ap.add_argument("--batch_size", type=int, default=256)
ap.add_argument("--tiny", type=int, default=0, help="1: the 2-layer / 128-d configuration (a rehearsal of the tool, not a measurement)")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_retrieve.py measures on the GPU: no device found (spmm_amd has no CPU / eager fallback)")
dev = torch.device("cuda")
torch.manual_seed(0)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def ab(fa, fb, reps):
    """-> (median ms of A, of B, spreads, last outputs): one warm-up of each, then alternating windows."""
    window(fa, 1), window(fb, 1)
    ta, tb = [], []
    for _ in range(a.pairs):
        t, oa = window(fa, reps)
        ta.append(t)
        t, ob = window(fb, reps)
        tb.append(t)
    ma, mb = statistics.median(ta), statistics.median(tb)
    return ma, mb, (max(ta) - min(ta)) / ma, (max(tb) - min(tb)) / mb, oa, ob


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


res = {"device": torch.cuda.get_device_name(0), "N": a.N, "E": a.E, "k": a.k, "pairs": a.pairs, "reps": a.reps, "tiny": a.tiny}

# ---------------------------------------------------------------------------------------------------------------- (a) search
g = torch.Generator(device=dev).manual_seed(1)
feats = torch.nn.functional.normalize(torch.randn(a.N, a.E, generator=g, device=dev), dim=1)
index = R.MoleculeIndex(feats)
for Q in a.Q:
    q = torch.nn.functional.normalize(torch.randn(Q, a.E, generator=g, device=dev), dim=1)
    entry = {}
    for k in sorted({a.k, min(a.k, 64)}):
        ma, mb, sa, sb, (s1, i1), (s2, i2) = ab(lambda: index.search(q, k), lambda: R.topk_reference(q, feats, k), a.reps)
        passes = (k + 63) // 64
        entry[f"k{k}"] = {
            "search_ms": round(ma, 4), "torch_matmul_topk_ms": round(mb, 4), "speedup": round(mb / ma, 3), "spread_search": round(sa, 4),
            "spread_torch": round(sb, 4), "passes_over_the_library": passes,
            "search_GBps_of_library_bytes_all_passes": round(passes * a.N * a.E * 4 / (ma * 1e-3) / 1e9, 1),
            "search_TFLOPs_all_passes": round(passes * 2.0 * Q * a.N * a.E / (ma * 1e-3) / 1e12, 2),
            "same_index_fraction": round(float((i1 == i2).float().mean()), 6), "max_abs_score_diff": float((s1 - s2).abs().max()),
            # (the search allocates its workspace -- the per-workgroup partial lists -- per call: it is part of this peak)
            "peak_extra_bytes_search": peak_extra(lambda: index.search(q, k)),
            "peak_extra_bytes_torch": peak_extra(lambda: R.topk_reference(q, feats, k))}
    res[f"search_Q{Q}"] = entry
del index, feats
torch.cuda.empty_cache()

# ------------------------------------------------------------------------------------------------ (b) matching, (c) index build
if a.tiny:
    from spmm_amd.config import tiny_config
    cfg = tiny_config()
else:
    cfg = SPMMConfig(text=BertConfig(num_hidden_layers=12, fusion_layer=6, add_cross_attention=True),
                     prop=BertConfig(num_hidden_layers=6, fusion_layer=6, vocab_size=1), embed_dim=256, queue_size=36864)
m = SPMM(spmm_config=cfg, no_train=True).eval()
m.store.refresh_shadows()
gh = torch.Generator().manual_seed(2)


def molecules(n):
    lens = torch.randint(30, 101, (n,), generator=gh)
    ids = torch.zeros(n, 100, dtype=torch.long)
    for b, ln in enumerate(lens.tolist()):
        ids[b, 0] = 2
        ids[b, 1:ln - 1] = torch.randint(4, cfg.text.vocab_size, (ln - 2,), generator=gh)
        ids[b, ln - 1] = 3
    return ids, (ids != 0).long()


ids, mask = molecules(a.library)
pv = torch.randn(a.queries, cfg.n_props, generator=gh)
_, hidden = R.pv_features(m, pv)
cand = torch.stack([torch.randperm(a.library, generator=gh)[:a.candidates] for _ in range(a.queries)])
pairs = torch.stack([torch.arange(a.queries).repeat_interleave(a.candidates), cand.reshape(-1)], dim=1)
ma, mb, sa, sb, pa, pb = ab(lambda: R.match_scores(m, hidden, ids, mask, pairs), lambda: R.match_scores(m, hidden, ids, mask, pairs, engine=False), 2)
res["match_scores"] = {"queries": a.queries, "candidates": a.candidates, "pairs": int(pairs.shape[0]), "distinct_molecules": int(pairs[:, 1].unique().numel()),
                       "tokens": "30..100", "engine_ms": round(ma, 2), "dense_ms": round(mb, 2), "speedup": round(mb / ma, 3),
                       "spread_engine": round(sa, 4), "spread_dense": round(sb, 4), "max_abs_diff": float((pa - pb).abs().max()),
                       "prob_min_max": [float(pb.min()), float(pb.max())]}

bids, bmask = molecules(a.build)
R.MoleculeIndex.from_tokens(m, bids[:2 * a.batch_size], bmask[:2 * a.batch_size], a.batch_size)          # warm-up
R.MoleculeIndex.from_tokens(m, bids[-2 * a.batch_size:], bmask[-2 * a.batch_size:], a.batch_size)
tb = [window(lambda: R.MoleculeIndex.from_tokens(m, bids, bmask, a.batch_size), 1)[0] for _ in range(3)]
res["index_build"] = {"molecules": a.build, "batch_size": a.batch_size, "tokens": "30..100", "ms": [round(t, 1) for t in tb],
                      "molecules_per_s": round(a.build / statistics.median(tb) * 1e3, 1)}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
