"""Guided generation: one PV x --samples samples x k = 2, seeded sampled search, --positions positions; published model size, random-init
weights (with them [SEP] rarely wins: nearly every sample runs all the positions).  Times, --rounds alternating rounds in one process,
medians:
  plain       generate_with_property at the defaults (R = samples * k beam rows);
  guided      generate_with_property(guidance=w): GuidedDecoder, both conditions as the two halves of one set of launches (2R rows);
  two_plain   the plain search twice, once with the PV and once with every property masked: what the two conditions cost as two searches
              (their logits are never combined: a lower bound of guidance without the merged rows);
  warp        ops.logit_warp alone at R = --warp_rows, V = the vocabulary, with and without truncation (hipEvents around --warp_iters
              back-to-back launches, per launch).
Not measured: a trained checkpoint (searches end early and compaction shrinks the batch), and what w does to property adherence.
Prints one JSON line and writes it to --out."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from spmm_amd import decode, ops
from spmm_amd.config import BertConfig, SPMMConfig
from spmm_amd.model import SPMM

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=1000)
ap.add_argument("--k", type=int, default=2)
ap.add_argument("--positions", type=int, default=40)
ap.add_argument("--guidance", type=float, default=2.0)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warp_rows", type=int, default=2000)
ap.add_argument("--warp_iters", type=int, default=200)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default="")
a = ap.parse_args()
torch.manual_seed(0)
cfg = SPMMConfig(text=BertConfig(num_hidden_layers=12, fusion_layer=6, add_cross_attention=True),
                 prop=BertConfig(num_hidden_layers=6, fusion_layer=6, vocab_size=1), embed_dim=256, queue_size=36864)
m = SPMM(spmm_config=cfg, no_train=True).eval()
m.store.refresh_shadows()
pv = torch.randn(53).cuda()
ones = torch.ones(53).cuda()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def search(mask=None, **kw):
    return decode.generate_with_property(m, pv, a.samples, mask, k=a.k, stochastic=True, seed=a.seed, max_steps=a.positions - 1, **kw)


def plain():
    search()


def guided():
    search(guidance=a.guidance)


def two_plain():
    search()
    search(ones)


def warp_us(**kw):
    V = cfg.text.vocab_size
    g = torch.Generator().manual_seed(1)
    both = (torch.randn(2 * a.warp_rows, V, generator=g) * 2).cuda()
    out = torch.empty(a.warp_rows, V, device="cuda")
    run = lambda: ops.logit_warp(both[:a.warp_rows], both[a.warp_rows:], out=out, min_keep=a.k, **kw)      # noqa: E731
    for _ in range(10):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.warp_iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / a.warp_iters, 2)


plain(), guided(), two_plain()                                             # warm-up
t = {"plain": [], "guided": [], "two_plain": []}
info = {}
for _ in range(a.rounds):
    t["plain"].append(timed(plain))
    info["plain"] = dict(decode.last_run)
    t["guided"].append(timed(guided))
    info["guided"] = dict(decode.last_run)
    t["two_plain"].append(timed(two_plain))
med = {k_: statistics.median(v) for k_, v in t.items()}
out = {"samples": a.samples, "k": a.k, "positions": a.positions, "guidance": a.guidance, "rounds": a.rounds, "seed": a.seed,
       "model": "published size, random-init weights",
       **{k_ + "_ms_median": round(v, 3) for k_, v in med.items()}, **{k_ + "_ms_all": [round(x, 3) for x in v] for k_, v in t.items()},
       "guided_over_plain": round(med["guided"] / med["plain"], 3), "two_plain_over_plain": round(med["two_plain"] / med["plain"], 3),
       "guided_over_two_plain": round(med["guided"] / med["two_plain"], 3),
       "last_run_plain": info["plain"], "last_run_guided": info["guided"],
       "warp_rows": a.warp_rows, "warp_vocab": cfg.text.vocab_size,
       "warp_us_per_launch": {"guidance_only": warp_us(w=a.guidance), "guidance_temperature_top_p": warp_us(w=a.guidance, temperature=0.8, top_p=0.9),
                              "guidance_top_k_top_p": warp_us(w=a.guidance, top_k=40, top_p=0.9)},
       "not_measured": "a trained checkpoint; the effect of the guidance weight on property adherence"}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
