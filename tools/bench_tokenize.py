"""Tokenising a library of SMILES strings: tokenizer.encode_smiles + pad_rows (Python, one string at a time) against
wordpiece_device.encode_smiles_device (csrc/tokenize.hip, one launch).  One MI355X, the published 300-piece vocabulary
(tests/golden/tokenizer_vocab300.npz), published model size with random-init weights, --rounds alternating rounds in one process, medians.

The library is synthetic and seeded: for every string a piece count n uniform in 30..100 is drawn, n - 2 pieces are sampled from the
vocabulary's '##' entries and their contents are joined ("decoded"); strings longer than 245 characters are drawn again.  Greedy matching
may merge neighbours, so the rows are a little shorter than n; the mean row length is reported.  The large library is --distinct strings
tiled up to --n_large (1 000 000 = 100 000 x 10): building a million Python strings is not what is timed.

  tokens     strings -> padded ids on the device.  host: encode_smiles + pad_rows + one H2D copy; device: encode_smiles_device (packing the
             strings, the H2D copy of the bytes, the launch, the copy of lens | status back).  At --n_small and --n_large; at --n_large the
             host side is timed on --host_subset of the strings and scaled by n_large / host_subset (stated in the output).
  kernel     spmm_wordpiece alone, hipEvents around --kernel_iters back-to-back launches on a blob that is already on the device.
  index      MoleculeIndex.build from strings with each path, at --n_small and --n_e2e (--rounds_e2e_large rounds there: the host path
             takes minutes per round at a million strings).
  score      score.py's batch loop (score_all over a TokenLibrary, score_smiles per batch) from strings with each path, at --n_small.

Not measured: the chain walk's share of the kernel (it is not separable without a second kernel); the score loop beyond --n_small; a
trained checkpoint (the text pass does not depend on the weights' values); real SMILES files (ChEMBL / PubChem strings
average ~45 characters, shorter than these).
Prints one JSON line and writes it to --out."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import score as score_driver
from spmm_amd import ops, score as S, wordpiece_device as W
from spmm_amd.config import BertConfig, SPMMConfig
from spmm_amd.model import SPMM
from spmm_amd.retrieve import MoleculeIndex
from spmm_amd.tokenizer import MAX_LENGTH, SmilesWordPiece, encode_smiles, pad_rows

ap = argparse.ArgumentParser()
ap.add_argument("--n_small", type=int, default=4096)
ap.add_argument("--n_large", type=int, default=1000000)
ap.add_argument("--distinct", type=int, default=100000, help="distinct strings of the large library")
ap.add_argument("--host_subset", type=int, default=20000, help="the host side of `tokens` at n_large is timed on this many strings and scaled")
ap.add_argument("--n_e2e", type=int, default=1000000, help="the larger end-to-end size (index build)")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--rounds_e2e_large", type=int, default=1, help="rounds of the index build at n_e2e (the host path takes minutes there)")
ap.add_argument("--kernel_iters", type=int, default=20)
ap.add_argument("--batch_size", type=int, default=256)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_tokenize.py measures on a GPU; there is none")
dev = torch.device("cuda:0")
tok = SmilesWordPiece([str(x) for x in np.load(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab300.npz"))["vocab"]])
table = W.table_of(tok)


def library(n, seed):
    rng = np.random.default_rng(seed)
    pieces = [p[2:] for p in tok.itos if p.startswith("##")]
    out = []
    while len(out) < n:
        s = "".join(pieces[j] for j in rng.integers(0, len(pieces), size=int(rng.integers(30, 101)) - 2))
        if len(s) <= 245:
            out.append(s)
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def alternate(what, fns, rounds, warm=True):
    """{name: median seconds} over `rounds` alternating rounds (after one warm-up round unless the shapes are warm), and the last outputs."""
    t, out = {k: [] for k in fns}, {}
    for r in range(0 if warm else 1, rounds + 1):
        for k, fn in fns.items():
            s, out[k] = timed(fn)
            print(f"[{what}] round {r} {k}: {s:.4f} s", file=sys.stderr, flush=True)
            if r:
                t[k].append(s)
    return {k: statistics.median(v) for k, v in t.items()}, t, out


def host_tokens(strings):
    ids, mask = pad_rows(encode_smiles(tok, strings), tok.pad_token_id)
    return ids.to(dev), mask


def device_tokens(strings):
    return W.encode_smiles_device(tok, strings, MAX_LENGTH, dev, table=table)


def kernel_us(strings, iters):
    blob, offsets = W.pack_strings(strings)
    words, head = table.on(dev)
    blob_d, off_d = torch.from_numpy(blob).to(dev), torch.from_numpy(offsets).to(dev)
    N = len(strings)
    ids = torch.empty(N, MAX_LENGTH - 1, dtype=torch.int32, device=dev)
    lens, status = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    run = lambda: ops.wordpiece(blob_d, off_d, words, head, ids, lens, status, gap=1, max_chars=table.max_chars, max_pieces=MAX_LENGTH - 2,      # noqa: E731
                                unk_id=table.unk_id, sep_id=table.sep_id, pad_id=table.pad_id)
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters, int(blob.size)


def rate(n, seconds):
    return round(n / seconds, 1)


distinct = library(max(a.distinct, a.n_small), a.seed)
small, subset = distinct[:a.n_small], distinct[:a.host_subset]
reps = -(-a.n_large // len(distinct))
large = (distinct * reps)[:a.n_large]
rows_small = encode_smiles(tok, small)
out = {"vocabulary": "published 300 pieces", "model": "published size, random-init weights", "rounds": a.rounds, "seed": a.seed,
       "library": f"synthetic: 28..98 sampled '##' pieces joined per string; n_large = {len(distinct)} distinct strings tiled x{reps}",
       "mean_tokens_per_row": round(float(np.mean([len(r) for r in rows_small])), 2),
       "mean_bytes_per_string": round(float(np.mean([len(s) for s in small])), 2), "table_words": int(table.words.size)}

# ---- (a) tokens only
med, allt, res = alternate("tokens_small", {"host": lambda: host_tokens(small), "device": lambda: device_tokens(small)}, a.rounds)
assert torch.equal(res["host"][0].to(torch.int32), res["device"][0][:, :res["host"][0].shape[1]])          # same ids, or the timing means nothing
out["tokens_small"] = {"n": a.n_small, "host_s": round(med["host"], 5), "device_s": round(med["device"], 5),
                       "host_strings_per_s": rate(a.n_small, med["host"]), "device_strings_per_s": rate(a.n_small, med["device"]),
                       "host_over_device": round(med["host"] / med["device"], 2), "device_s_all": [round(x, 5) for x in allt["device"]]}
med, allt, res = alternate("tokens_large", {"host": lambda: host_tokens(subset), "device": lambda: device_tokens(large)}, a.rounds)
scale = a.n_large / len(subset)
out["tokens_large"] = {"n": a.n_large, "host_timed_on": len(subset), "host_scaled_by": round(scale, 3), "host_s": round(med["host"] * scale, 4),
                       "device_s": round(med["device"], 4), "host_strings_per_s": rate(len(subset), med["host"]),
                       "device_strings_per_s": rate(a.n_large, med["device"]), "host_over_device": round(med["host"] * scale / med["device"], 2),
                       "device_s_all": [round(x, 4) for x in allt["device"]]}
del res
# ---- (b) the kernel alone
out["kernel"] = {}
for name, strings, iters in (("small", small, a.kernel_iters * 10), ("large", large, a.kernel_iters)):
    us, nbytes = kernel_us(strings, iters)
    out["kernel"][name] = {"n": len(strings), "us_per_launch": round(us, 2), "strings_per_s": rate(len(strings), us * 1e-6),
                           "blob_bytes": nbytes, "chain_walk_share": "not measured"}

# ---- (c) end to end from strings
torch.manual_seed(0)
cfg = SPMMConfig(text=BertConfig(num_hidden_layers=12, fusion_layer=6, add_cross_attention=True),
                 prop=BertConfig(num_hidden_layers=6, fusion_layer=6, vocab_size=1), embed_dim=256, queue_size=36864)
m = SPMM(spmm_config=cfg, no_train=True).eval()
m.store.refresh_shadows()
pv = torch.randn(1, 53, generator=torch.Generator().manual_seed(1))


def build(strings, device_path):
    return MoleculeIndex.build(m, tok, strings, batch_size=a.batch_size, tokenizer_device=dev if device_path else None).feats


def score(strings, device_path):
    def score_batch(idx, ids, mask):
        pairs = torch.stack([torch.zeros(len(idx), dtype=torch.int64), torch.arange(len(idx))], dim=1)
        r = S.score_smiles(m, pv, ids, mask, pairs=pairs)
        return r.logp.cpu(), r.n_tokens.cpu()
    lib = W.TokenLibrary.from_strings(tok, strings, MAX_LENGTH, dev if device_path else None)
    return score_driver.score_all(lib, a.batch_size, score_batch, tok.pad_token_id)


def e2e(name, fn, strings, rounds, warm=True):
    med, allt, res = alternate(f"{name} n={len(strings)}", {"host": lambda: fn(strings, False), "device": lambda: fn(strings, True)}, rounds, warm)
    same = torch.equal(res["host"], res["device"]) if torch.is_tensor(res["host"]) else res["host"] == res["device"]
    return {"n": len(strings), "rounds": rounds, "host_s": round(med["host"], 4), "device_s": round(med["device"], 4),
            "host_strings_per_s": rate(len(strings), med["host"]), "device_strings_per_s": rate(len(strings), med["device"]),
            "host_over_device": round(med["host"] / med["device"], 2), "identical_outputs": bool(same),
            "host_s_all": [round(x, 4) for x in allt["host"]], "device_s_all": [round(x, 4) for x in allt["device"]]}


out["index_small"] = e2e("index", build, small, a.rounds)
out["score_small"] = e2e("score", score, small, a.rounds)
if a.n_e2e > a.n_small:
    out["index_large"] = e2e("index", build, (distinct * (-(-a.n_e2e // len(distinct))))[:a.n_e2e], a.rounds_e2e_large, warm=False)      # (same batch shapes as index_small: warm)
out["not_measured"] = ("the chain walk's share of the kernel; the score loop beyond n_small strings; a trained checkpoint; real SMILES files "
                       "(shorter strings than these)")
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
