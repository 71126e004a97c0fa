"""Syntax-constrained generation: one PV x --samples samples x k = 2, seeded sampled search, --positions positions; published model size,
random-init weights, the published 300-piece vocabulary (tests/golden/tokenizer_vocab300.npz; the driver's synthetic one if it is missing).
Times, --rounds alternating rounds in one process, medians:
  plain         generate_with_property at the defaults (R = samples * k beam rows): the search without the constraint, launch for launch;
  constrained   generate_with_property(syntax=True): one ops.smiles_mask launch for the first pick and one per position;
  mask          ops.smiles_mask alone at R = --mask_rows, V = the vocabulary, histories of t = 8 and t = 100 tokens (seeded random walks of
                the grammar, 64 distinct ones tiled), hipEvents around --mask_iters back-to-back launches, per launch.
  results       the host part at the end of a search (BeamBook.results: every final hypothesis copied out and turned into lists), timed
                apart after a device synchronisation: it grows with the number of samples that finished, and with random weights the
                constrained search finishes all of them while the plain one finishes fewer than half -- `loop` = total - results is what the
                positions themselves cost.
Also reported: the share of well-formed strings (smiles_syntax.well_formed) among the finished samples of both searches, and how many
samples finished at all.
Not measured: a trained checkpoint -- there searches end early, compaction shrinks the batch, and whether the constraint changes the
well-formed share of a model that has learnt the syntax cannot be told from random weights.
Prints one JSON line and writes it to --out."""
import argparse, json, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from spmm_amd import decode, ops, smiles_syntax as SS
from spmm_amd.config import BertConfig, SPMMConfig
from spmm_amd.model import SPMM
from spmm_amd.tokenizer import SmilesWordPiece

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=1000)
ap.add_argument("--k", type=int, default=2)
ap.add_argument("--positions", type=int, default=40)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--mask_rows", type=int, default=2000)
ap.add_argument("--mask_iters", type=int, default=200)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default="")
a = ap.parse_args()
torch.manual_seed(0)
cfg = SPMMConfig(text=BertConfig(num_hidden_layers=12, fusion_layer=6, add_cross_attention=True),
                 prop=BertConfig(num_hidden_layers=6, fusion_layer=6, vocab_size=1), embed_dim=256, queue_size=36864)
m = SPMM(spmm_config=cfg, no_train=True).eval()
m.store.refresh_shadows()
golden = os.path.join(ROOT, "tests", "golden", "tokenizer_vocab300.npz")
if os.path.exists(golden):
    vocab, vocab_name = [str(x) for x in np.load(golden)["vocab"]], "published 300 pieces"
else:
    import pv2smiles
    vocab, vocab_name = pv2smiles.synthetic_vocab(cfg.text.vocab_size), "synthetic"
tok = m.tokenizer = SmilesWordPiece(vocab)
table = decode.syntax_table(m, True)
pv = torch.randn(53).cuda()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


spent = {"results": 0.0}
_results = decode.BeamBook.results


def _timed_results(self):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = _results(self)
    spent["results"] += (time.perf_counter() - t0) * 1e3
    return out


decode.BeamBook.results = _timed_results


def search(**kw):
    return decode.generate_with_property(m, pv, a.samples, None, k=a.k, stochastic=True, seed=a.seed, max_steps=a.positions - 1, **kw)


def plain():
    return search()


def constrained():
    return search(syntax=table)


def shares(samples):
    done = [tok.decode(s) for s in samples if s]
    return {"finished": len(done), "well_formed": sum(1 for s in done if SS.well_formed(s))}


def walks(n_tokens, n=64):
    rng, live, out = random.Random(n_tokens), [v for v in range(table.V) if table.text[v]], []
    for _ in range(n):
        hist, state = [decode.CLS_ID], SS.INITIAL
        while len(hist) < n_tokens:
            v = rng.choice(live)
            nxt = table.step_token(state, v)
            if nxt[0] != SS.REJECT and SS.cost(nxt) <= 200 - len(hist):
                hist.append(v)
                state = nxt
        out.append(hist)
    return out


def mask_us(t):
    R, V = a.mask_rows // a.k * a.k, table.V
    hist = torch.tensor(walks(t), dtype=torch.int32)
    tokens = torch.zeros(R, 256, dtype=torch.int32)
    tokens[:, :t] = hist[torch.arange(R) % hist.shape[0]]
    tokens, dev_table = tokens.view(R // a.k, a.k, 256).cuda(), torch.from_numpy(table.packed).cuda()
    logits = (torch.randn(R, V, generator=torch.Generator().manual_seed(1)) * 2).cuda()
    run = lambda: ops.smiles_mask(logits, tokens, dev_table, t=t, t_last=254, k=a.k)      # noqa: E731
    for _ in range(10):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.mask_iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / a.mask_iters, 2)


plain(), constrained()                                                     # warm-up
t = {"plain": [], "constrained": []}
t_res = {"plain": [], "constrained": []}
info, res = {}, {}
for _ in range(a.rounds):
    for name, fn in (("plain", plain), ("constrained", constrained)):
        spent["results"] = 0.0
        ms, res[name] = timed(fn)
        t[name].append(ms)
        t_res[name].append(spent["results"])
        info[name] = dict(decode.last_run)
med = {k_: statistics.median(v) for k_, v in t.items()}
med_loop = {k_: statistics.median([x - r for x, r in zip(t[k_], t_res[k_])]) for k_ in t}
positions = max(info["constrained"]["positions"], 1)
mask = {"t8": mask_us(8), "t100": mask_us(100)}
out = {"samples": a.samples, "k": a.k, "positions": a.positions, "rounds": a.rounds, "seed": a.seed,
       "model": "published size, random-init weights", "vocabulary": vocab_name,
       **{k_ + "_ms_median": round(v, 3) for k_, v in med.items()}, **{k_ + "_ms_all": [round(x, 3) for x in v] for k_, v in t.items()},
       "constrained_over_plain": round(med["constrained"] / med["plain"], 3),
       "results_ms_median": {k_: round(statistics.median(v), 3) for k_, v in t_res.items()},
       "loop_ms_median": {k_: round(v, 3) for k_, v in med_loop.items()},
       "constrained_over_plain_loop": round(med_loop["constrained"] / med_loop["plain"], 3),
       "loop_ms_per_position": {k_: round(v / max(info[k_]["positions"], 1), 4) for k_, v in med_loop.items()},
       "last_run_plain": info["plain"], "last_run_constrained": info["constrained"],
       "outputs_plain": shares(res["plain"]), "outputs_constrained": shares(res["constrained"]),
       "mask_rows": a.mask_rows // a.k * a.k, "mask_vocab": table.V, "mask_us_per_launch": mask,
       "mask_t100_share_of_a_constrained_position": round(mask["t100"] * 1e-3 / (med_loop["constrained"] / positions), 4),
       "fold": "sequential (every lane walks the row's history from LDS); not parallelised",
       "not_measured": "a trained checkpoint (early ends, compaction); whether the constraint changes the well-formed share of a trained model"}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
