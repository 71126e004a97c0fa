"""Prefix-constrained generation: one PV x --samples samples x k = 2, seeded sampled search started from a prefix of P random non-special
tokens, --free positions after it; published model size, random-init weights (with them [SEP] rarely wins: nearly every sample runs all
the positions).  Times, per P:
  search   generate_with_property(prefix=..., prefill=True) against prefill=False (the prefix stepped through on every beam row):
           --pairs alternating pairs in one process, medians;
  prefill  CachedDecoder.prefill alone -- the packed pass over the P positions, the cache fills and the LM head on one row -- against its
           by_steps twin, P positions of `step` on all samples * k rows; same alternation, medians.
Prints one JSON line and writes it to --out."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from spmm_amd import decode
from spmm_amd.config import BertConfig, SPMMConfig
from spmm_amd.model import SPMM

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=1000)
ap.add_argument("--k", type=int, default=2)
ap.add_argument("--free", type=int, default=40, help="positions decoded after the prefix")
ap.add_argument("--prefix_lengths", type=int, nargs="+", default=[8, 32], help="prefix tokens, [CLS] not counted")
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default="")
a = ap.parse_args()
torch.manual_seed(0)
cfg = SPMMConfig(text=BertConfig(num_hidden_layers=12, fusion_layer=6, add_cross_attention=True),
                 prop=BertConfig(num_hidden_layers=6, fusion_layer=6, vocab_size=1), embed_dim=256, queue_size=36864)
m = SPMM(spmm_config=cfg, no_train=True).eval()
m.store.refresh_shadows()
pv = torch.randn(53).cuda()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


out = {"samples": a.samples, "k": a.k, "free_positions": a.free, "pairs": a.pairs, "seed": a.seed, "model": "published size, random-init weights",
       "by_prefix_length": {}}
for n_tok in a.prefix_lengths:
    P = n_tok + 1
    prefix = [decode.CLS_ID] + torch.randint(4, cfg.text.vocab_size, (n_tok,), generator=torch.Generator().manual_seed(n_tok)).tolist()
    pre_t = torch.tensor([prefix])

    def search(prefill):
        return decode.generate_with_property(m, pv, a.samples, None, k=a.k, stochastic=True, seed=a.seed, max_steps=a.free - 1, prefix=prefix,
                                             prefill=prefill)

    pe = decode.encode_properties(m, pv.reshape(1, -1))
    xkv = decode.CachedDecoder(m, pe, a.k, P + a.free + 1, repeat=1).xkv_once

    def prefill_only(by_steps):
        dec = decode.CachedDecoder(m, pe, a.k, P + a.free + 1, repeat=a.samples, xkv=xkv)
        dec.prefill(pre_t, [0] * a.samples, by_steps=by_steps)

    search(True), search(False), prefill_only(False), prefill_only(True)                   # warm-up
    t = {"search_prefill": [], "search_stepped": [], "prefill_packed": [], "prefill_stepped": []}
    for _ in range(a.pairs):
        t["search_prefill"].append(timed(lambda: search(True)))
        t["search_stepped"].append(timed(lambda: search(False)))
        t["prefill_packed"].append(timed(lambda: prefill_only(False)))
        t["prefill_stepped"].append(timed(lambda: prefill_only(True)))
    same = sum(x == y for x, y in zip(search(True), search(False)))
    out["by_prefix_length"][str(n_tok)] = dict({k_ + "_ms_median": round(statistics.median(v), 3) for k_, v in t.items()},
                                               **{k_ + "_ms_all": [round(x, 3) for x in v] for k_, v in t.items()},
                                               positions=decode.last_run.get("positions"), samples_identical_between_the_two_paths=same)
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
