"""Distinct PV -> SMILES samples: sample_distinct (one stochastic beam search, sampling without replacement) against generate_with_property
(--samples independent seeded searches, k = 2, one final per sample).  One PV, published model size, random-init weights, the published
300-piece vocabulary (tests/golden/tokenizer_vocab300.npz; the driver's synthetic one if it is missing), --syntax on both sides so that the
searches of an untrained model finish, --positions positions, seeded, --rounds alternating rounds in one process, medians.
  independent   generate_with_property(n_sample = --samples, k = 2, syntax=True): time, finished samples, DISTINCT finished token sequences;
  distinct      sample_distinct(n_distinct = --samples, syntax=True): the same three -- finished and distinct coincide by construction;
  per second    distinct finished token sequences per second of each;
  step          ops.sbs_step alone at W = --samples rounded up to a multiple of 8, V = the vocabulary, on the logits and the state of a
                mid-search position (half the positions in), hipEvents around --iters back-to-back launches, per launch; and the same
                launch stopped after its first, second and third phase (SPMM_SBS_PHASES), whose differences say where its time goes;
  position      CachedDecoder.step alone at the same rows and position (k = 8, repeat = W / 8), the same way;
  self_group    the self-attention launch of one layer (ops.decode_attn with the ancestry table of that mid-search position: slot order
                follows the keys, so the eight rows of a group are mostly unrelated hypotheses) with group = 8 against group = 1.
Not measured: a trained checkpoint (searches end early and the share of duplicates among independent samples is what a trained model
makes it; with random weights and the grammar mask the independent samples are nearly all different already, so the gain in distinct
molecules per second shown here is a floor, not the figure of a trained model); more than one PV per call; prefixes; the tensor-op form.
Prints one JSON line and writes it to --out."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from spmm_amd import decode, ops
from spmm_amd.config import BertConfig, SPMMConfig
from spmm_amd.model import SPMM
from spmm_amd.tokenizer import SmilesWordPiece

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=1000)
ap.add_argument("--positions", type=int, default=40)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=50)
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
m.tokenizer = SmilesWordPiece(vocab)
pv = torch.randn(53).cuda()
N, T = a.samples, a.positions


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def independent():
    return [tuple(s) for s in decode.generate_with_property(m, pv, N, k=2, seed=a.seed, max_steps=T, syntax=True) if s]


def distinct():
    return [tuple(s) for _, s in decode.sample_distinct(m, pv, N, seed=a.seed, max_steps=T, syntax=True)[0]]


independent(), distinct()                                              # warm-up: kernel attributes, the grammar table, allocator
ms = {"independent": [], "distinct": []}
for _ in range(a.rounds):
    for name, fn in (("independent", independent), ("distinct", distinct)):
        t, out = timed(fn)
        ms[name].append(t)
        if name == "independent":
            ind = out
        else:
            dis = out
run = dict(decode.last_distinct)
res = {"bench": "distinct", "samples": N, "positions": T, "rounds": a.rounds, "vocabulary": vocab_name, "W": run["W"]}
for name, out in (("independent", ind), ("distinct", dis)):
    med = statistics.median(ms[name])
    res[name] = {"ms": round(med, 1), "ms_min_max": [round(min(ms[name]), 1), round(max(ms[name]), 1)], "finished": len(out), "distinct_finished": len(set(out)),
                 "distinct_per_second": round(len(set(out)) / (med * 1e-3), 1)}
res["distinct"]["unfinished"] = run["unfinished"][0]

# ---- one mid-search position: the step launch, the decoder position and the self-attention group widths, each alone
W, t_mid = run["W"], max(T // 2, 2)
V, L = cfg.text.vocab_size, 1 + T + 2
pe = decode.encode_properties(m, pv.reshape(1, -1))
dec = decode.CachedDecoder(m, pe, 8, L, repeat=W // 8)
book = decode.DistinctBook(1, W, T, "cuda", fused=True)
seed_dev = torch.tensor([a.seed], dtype=torch.int64, device="cuda")
mol = torch.arange(W // 8, dtype=torch.int32, device="cuda")
ids = torch.full((W,), decode.CLS_ID, dtype=torch.long, device="cuda")
for t in range(t_mid):                                                 # an unconstrained search up to the position that is timed
    logits = dec.step(ids, t)
    noise = ops.gumbel_noise(seed_dev, W // 8, 8, V, L, salt=decode.DISTINCT_SALT, t=t, mol=mol)
    logits[:, decode.SEP_ID] = -float("inf")                           # (nothing ends: every row stays live, the widest step there is)
    ids = book.step_fused(logits, noise)
    dec.anc = book.anc
logits = dec.step(ids, t_mid)
noise = ops.gumbel_noise(seed_dev, W // 8, 8, V, L, salt=decode.DISTINCT_SALT, t=t_mid, mol=mol)


def per_launch(fn, iters=a.iters):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                           # microseconds


res["step_us"] = round(per_launch(lambda: ops.sbs_step(logits, noise, book, t=book.t)), 1)      # (reads cur, writes nxt: repeatable)
upto = []                                                              # the launch stopped after phase A, B, C (SPMM_SBS_PHASES, csrc/sbs.hip)
for ph in ("1", "2", "3"):
    os.environ["SPMM_SBS_PHASES"] = ph
    upto.append(per_launch(lambda: ops.sbs_step(logits, noise, book, t=book.t)))
del os.environ["SPMM_SBS_PHASES"]
upto.append(res["step_us"])
res["step_phases_us"] = {name: round(b - a, 1) for name, a, b in zip(("keys", "select", "sort", "gather"), [0.0] + upto[:-1], upto)}
res["position_us"] = round(per_launch(lambda: dec.step(ids, t_mid), max(a.iters // 5, 5)), 1)
res["step_share_of_position"] = round(res["step_us"] / res["position_us"], 3)
H, nH = cfg.text.hidden_size, cfg.text.num_attention_heads
QKV = torch.randn(W, 3 * H, device="cuda").to(torch.bfloat16)
ctx = torch.empty(W, H, dtype=torch.bfloat16, device="cuda")
for g in (8, 1):
    rounds = []
    for _ in range(a.rounds):
        rounds.append(per_launch(lambda: ops.decode_attn(QKV[:, :H], dec.kc[0], dec.vc[0], ctx, nH=nH, Lkv=t_mid + 1, seq_stride=L * H, tok_stride=64,
                                                         head_stride=L * 64, anc=dec.anc, group=g, knew=QKV[:, H:2 * H], vnew=QKV[:, 2 * H:])))
    res[f"self_attn_group{g}_us"] = {"median": round(statistics.median(rounds), 1), "min_max": [round(min(rounds), 1), round(max(rounds), 1)]}
res["not_measured"] = ["a trained checkpoint (duplicates among independent samples; early ends)", "more than one PV per call", "prefixes",
                       "the tensor-op form of the step", "self_group inside a whole search (the launch alone is timed)"]
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
