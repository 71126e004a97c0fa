"""SMILES -> PV throughput: decode.predict_properties (engine path: text encoded once on packed rows, cross-attention keys / values projected
once, cache of embedded prefix rows, last fusion layer on the last rows only) against decode.smiles_to_pv (the loop over the module facades)
on the same model, the same molecules and the same length-sorted batches, in molecules/s at two batch sizes.

One model at the published size (12 text layers, fusion from layer 6, 6 PV layers, H = 768) with seeded random weights; `--molecules` synthetic
token sequences, lengths uniform in [Lt/2, Lt] (SURVEY.md section 8d's recipe for text, Lt = 100 as the reference truncates).  Per batch
size: one untimed pass of both paths over every batch shape (warm-up), then `--pairs` alternating A/B pairs, each pass timed with device events
around all its batches; the figure is the median pass, and the spread of the passes and of the per-pair ratios is reported beside it.  Also reported: the largest difference between the two paths' predictions
(random weights: the values are O(1)) and the launches a step of each path makes.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from spmm_amd import decode
from spmm_amd.config import BertConfig, SPMMConfig
from spmm_amd.model import SPMM

ap = argparse.ArgumentParser()
ap.add_argument("--molecules", type=int, default=1000)
ap.add_argument("--Lt", type=int, default=100)
ap.add_argument("--batches", type=int, nargs="+", default=[64, 1000])
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--n_props", type=int, default=53)
ap.add_argument("--tiny", type=int, default=0, help="1: the 2-layer / 128-d configuration (a rehearsal of the tool, not a measurement)")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_smiles2pv.py measures on the GPU: no device found (spmm_amd has no CPU / eager fallback)")

torch.manual_seed(0)
if a.tiny:
    from spmm_amd.config import tiny_config
    cfg = tiny_config()
else:
    cfg = SPMMConfig(text=BertConfig(num_hidden_layers=12, fusion_layer=6, add_cross_attention=True),
                     prop=BertConfig(num_hidden_layers=6, fusion_layer=6, vocab_size=1), embed_dim=256, queue_size=36864)
m = SPMM(spmm_config=cfg, no_train=True).eval()
m.store.refresh_shadows()

g = torch.Generator().manual_seed(1)
lens = torch.randint(max(a.Lt // 2, 3), a.Lt + 1, (a.molecules,), generator=g)
rows = []
for n in lens.tolist():
    rows.append([2] + torch.randint(4, cfg.text.vocab_size, (n - 2,), generator=g).tolist() + [3])
order = np.argsort(lens.numpy(), kind="stable")


def batches_of(bs):
    out = []
    for i in range(0, len(order), bs):
        idx = order[i:i + bs]
        L = max(len(rows[j]) for j in idx)
        ids = torch.zeros(len(idx), L, dtype=torch.long)
        for r, j in enumerate(idx):
            ids[r, :len(rows[j])] = torch.tensor(rows[j])
        out.append((ids, (ids != 0).long()))
    return out


def one_pass(fn, batches, host_mask):
    """-> (milliseconds by device events, predictions of the first batch)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    first = None
    e0.record()
    for ids, mask in batches:
        out = fn(m, ids if host_mask else ids.cuda(), mask if host_mask else mask.cuda(), a.n_props)
        first = out if first is None else first
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), first


from spmm_amd import ops as _ops


def launches_per_step(fn):
    """Library launches of a 3-step run minus those of a 2-step run (counted with the prototype checker: nothing is launched)."""
    ids, mask = batches_of(4)[0]
    n = []
    _ops._DRY_RUN = True
    try:
        for steps in (2, 3):
            _ops._dry_log.clear()
            fn(m, ids.cuda(), mask.cuda(), steps)
            n.append(len(_ops._dry_log))
    finally:
        _ops._DRY_RUN = False
    return n[1] - n[0]


res = {"molecules": a.molecules, "Lt": a.Lt, "n_props": a.n_props, "pairs": a.pairs, "tiny": a.tiny, "device": torch.cuda.get_device_name(0)}
for bs in a.batches:
    B = batches_of(bs)
    _, pa = one_pass(decode.predict_properties, B, True)        # warm-up of every batch shape, both paths
    _, pb = one_pass(decode.smiles_to_pv, B, False)
    ta, tb = [], []
    for _ in range(a.pairs):
        ta.append(one_pass(decode.predict_properties, B, True)[0])
        tb.append(one_pass(decode.smiles_to_pv, B, False)[0])
    ma, mb = statistics.median(ta), statistics.median(tb)
    res[f"batch_{bs}"] = {"predict_properties_molecules_per_s": round(a.molecules / ma * 1e3, 1), "smiles_to_pv_molecules_per_s": round(a.molecules / mb * 1e3, 1),
                          "predict_properties_ms": [round(t, 1) for t in ta], "smiles_to_pv_ms": [round(t, 1) for t in tb],
                          "speedup": round(mb / ma, 3), "speedup_of_pairs_min_max": [round(min(y / x for x, y in zip(ta, tb)), 3), round(max(y / x for x, y in zip(ta, tb)), 3)],
                          "spread_predict_properties": round((max(ta) - min(ta)) / ma, 4), "spread_smiles_to_pv": round((max(tb) - min(tb)) / mb, 4), "ms_per_step_predict_properties": round(ma / (len(B) * a.n_props), 3),
                          "ms_per_step_smiles_to_pv": round(mb / (len(B) * a.n_props), 3),
                          "max_abs_diff_first_batch": float((pa.float() - pb.float()).abs().max()), "pred_abs_max": float(pb.float().abs().max())}
torch.cuda.synchronize()
try:
    res["launches_per_step"] = {"predict_properties": launches_per_step(decode.predict_properties), "smiles_to_pv": launches_per_step(decode.smiles_to_pv)}
except Exception as e:      # noqa: BLE001  (the count is a side figure: the timings above are not lost with it)
    res["launches_per_step"] = f"not counted: {type(e).__name__}: {e}"
print(json.dumps(res))
