"""Reaction prediction driver -- the counterpart of the reference's `d_rxn_prediction.py --evaluate True` (forward synthesis on USPTO-480k,
retrosynthesis on USPTO-50k): the product SMILES of every reactant SMILES of a file, by k-beam or greedy search, from a fine-tuned
reaction checkpoint (or a pretraining checkpoint mapped the way the reference maps it):

  python rxn_predict.py --checkpoint ./output/RXN/checkpoint_best.pth --vocab_filename ./vocab_bpe_300.txt --input test_parsed.txt \
                        --mode forward --n_beam 5 --output rxn_candidates.csv
  python rxn_predict.py --synthetic --tiny --n_beam 3                        (no data files: seeded weights, reactions and vocabulary)

--input holds one reaction per line, `source<TAB>target` (the reference's *_parsed.txt; the target is optional).  --mode says which
direction the checkpoint was fine-tuned for: `forward` reads the line as reactants<TAB>product, `retro` as product<TAB>reactants -- the
source is always the first column.  What differs from the reference, on purpose: the reactions are sorted by source length into batches
(and written back in input order), and every batch is decoded together on the engine (spmm_amd.decode.predict_products /
greedy_products: reactants encoded once on packed rows, K/V cache, masked-memory cross-attention) -- the reference's beam search takes
one reaction at a time.  Accuracy is the share of exact string matches; the strings are RDKit-canonical only if `rdkit` can be imported.
Fine-tuning is rxn_finetune.py; with --synthetic an explicitly named --checkpoint (e.g. one rxn_finetune.py --synthetic wrote) replaces the seeded weights."""
import argparse
import csv
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from pv2smiles import synthetic_vocab                                # noqa: E402
from smiles2pv import add_tokenizer_flags, encode, length_sorted_batches, library_of, pad_batch      # noqa: E402,F401  ('[CLS]' prefix, the tokenizer's own first token dropped)

MAX_SOURCE = 150          # d_rxn_prediction.py:63,92 (tokenizer(text, padding='longest', max_length=150))
MAX_STEPS = 100           # positions of evaluate / evaluate_beam (:67, :100)
DEFAULT_CHECKPOINT = "./output/RXN/checkpoint_best.pth"


# --------------------------------------------------------------------------------------------------------------------- input
def read_reactions(path: str):
    """-> (sources, targets): one `source<TAB>target` per line (SMILESDataset_USPTO's format); blank lines are skipped, a line without a
    tab has no target (None)."""
    src, tgt = [], []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            parts = line.split("\t")
            src.append(parts[0])
            tgt.append(parts[1] if len(parts) > 1 and parts[1] else None)
    return src, tgt


def predict_all(model, tokenizer, sources, n_beam: int, batch_size: int, max_steps: int = MAX_STEPS, predict=None, greedy=None,
                host_tokenizer=False):
    """Candidate id lists of every reaction in INPUT order: result[i] = up to n_beam id lists, best first (one for n_beam == 1).
    host_tokenizer: --host_tokenizer (the sources go through the Python tokenizer also where the GPU could tokenise them in one launch)."""
    if predict is None or greedy is None:
        from spmm_amd import decode
        predict, greedy = predict or decode.predict_products, greedy or decode.greedy_products
    lib = library_of(tokenizer, sources, MAX_SOURCE, model, host_tokenizer)
    out = [None] * len(lib)
    for idx, ids, mask, _ in lib.batches(batch_size):
        if n_beam == 1:
            res = [[seq] for seq in greedy(model, ids, mask, max_steps=max_steps)]
        else:
            res = [[seq for _, seq in hyps] for hyps in predict(model, ids, mask, k=n_beam, max_steps=max_steps)]
        for i, r in zip(idx.tolist(), res):
            out[i] = r
    return out


# ------------------------------------------------------------------------------------------------------------------- metrics
def _canonical():
    """RDKit's canonical, non-isomeric SMILES (metric_eval, d_rxn_prediction.py:127-145) when rdkit is there; the string itself otherwise."""
    try:
        from rdkit import Chem, RDLogger
    except ImportError:
        return lambda s: s
    RDLogger.DisableLog("rdApp.*")

    def canon(s):
        mol = Chem.MolFromSmiles(s)
        return None if mol is None else Chem.MolToSmiles(mol, isomericSmiles=False, canonical=True)
    return canon


def accuracy(targets, candidates, canon=None):
    """-> (top-1, top-k) accuracy over the reactions that have a target: exact match of the (canonical) strings."""
    canon = canon or (lambda s: s)
    n = top1 = topk = 0
    for t, cands in zip(targets, candidates):
        if t is None:
            continue
        n += 1
        want = canon(t)
        got = [canon(c) for c in cands]
        if want is None:
            continue
        top1 += int(bool(got) and got[0] == want)
        topk += int(want in got)
    return (top1 / n, topk / n) if n else (0.0, 0.0)


def write_csv(path: str, sources, candidates, k: int):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["source"] + [f"candidate_{i + 1}" for i in range(k)])
        for s, cands in zip(sources, candidates):
            w.writerow([s] + list(cands) + [""] * (k - len(cands)))


def synthetic_reactions(vocab, n: int, seed: int):
    """n made-up reactions: sources of 1 .. 40 vocabulary pieces, targets of 1 .. 10."""
    g = np.random.default_rng(seed)
    pieces = [p[2:] for p in vocab if p.startswith("##")]

    def word(lo, hi):
        return "".join(pieces[j] for j in g.integers(0, len(pieces), size=int(g.integers(lo, hi))))
    return [word(1, 41) for _ in range(n)], [word(1, 11) for _ in range(n)]


# ---------------------------------------------------------------------------------------------------------------------- main
def main(args):
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"rxn_predict.py: --device {args.device}: spmm_amd has no CPU / eager fallback -- its layers are HIP kernels for "
                         "gfx950 and need a GPU (the fp32 CPU restatement under tests/ is test infrastructure, not a product path)")
    if not 1 <= args.n_beam <= 8:
        raise SystemExit(f"--n_beam {args.n_beam}: the masked-memory decode kernels serve 1..8 beams")
    torch.manual_seed(args.seed)
    from spmm_amd.rxn import SPMMRxn
    from spmm_amd.tokenizer import SmilesWordPiece

    config = {"bert_config_text": os.path.join(ROOT, "configs", f"config_bert{'_tiny' if args.tiny else ''}.json")}
    if os.path.exists(args.vocab_filename):
        tokenizer = SmilesWordPiece(args.vocab_filename)
    elif args.synthetic:
        tokenizer = None
    else:
        raise SystemExit(f"--vocab_filename {args.vocab_filename} not found")
    print("Creating model")
    model = SPMMRxn(config=config, device=device)
    if tokenizer is None:
        tokenizer = SmilesWordPiece(synthetic_vocab(model.cfg.text.vocab_size))
    if args.checkpoint and (not args.synthetic or args.checkpoint != DEFAULT_CHECKPOINT):      # (--synthetic: seeded weights unless one is named)
        res = model.load_pretrained(args.checkpoint)
        print(f"load checkpoint from {args.checkpoint} (missing {len(res.missing_keys)}, unexpected {len(res.unexpected_keys)})")
    if args.synthetic:
        sources, targets = synthetic_reactions(tokenizer.itos, 8, args.seed)
    else:
        sources, targets = read_reactions(args.input)
    model.eval()
    print("=" * 50)
    print(f"{args.mode} reaction prediction, {'greedy' if args.n_beam == 1 else f'{args.n_beam} beams'}, {len(sources)} reactions...")
    ids = predict_all(model, tokenizer, sources, args.n_beam, args.batch_size, args.max_steps, host_tokenizer=args.host_tokenizer)
    candidates = [[tokenizer.decode(seq) for seq in cands] for cands in ids]
    write_csv(args.output, sources, candidates, args.n_beam)
    print(f"Candidates are saved in '{args.output}'")
    if any(t is not None for t in targets):
        top1, topk = accuracy(targets, candidates, _canonical())
        print("Accuracy (top-1):", top1)
        print(f"Accuracy (top-{args.n_beam}):", topk)
    print("=" * 50)
    return candidates


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Predict the products (or reactants) of every reaction of a file (the reference's d_rxn_prediction.py --evaluate True).")
    # the reference's flags (d_rxn_prediction.py:259-268)
    p.add_argument("--checkpoint", default=DEFAULT_CHECKPOINT)
    p.add_argument("--mode", default="forward", choices=("forward", "retro"))
    p.add_argument("--n_beam", default=5, type=int, help="beams per reaction; 1 runs the greedy search")
    p.add_argument("--device", default="cuda")
    p.add_argument("--batch_size", default=32, type=int, help="reactions decoded together")
    # additions
    p.add_argument("--vocab_filename", default="./vocab_bpe_300.txt")
    p.add_argument("--input", default="./test_parsed.txt", help="one reaction per line: source<TAB>target (the target is optional)")
    p.add_argument("--output", default="rxn_candidates.csv", help="CSV: source, then the n_beam candidates, best first")
    p.add_argument("--max_steps", default=MAX_STEPS, type=int, help="positions decoded at most (the reference's 100)")
    p.add_argument("--seed", default=0, type=int, help="seed of --synthetic's weights and reactions")
    p.add_argument("--synthetic", action="store_true", help="no data files: seeded weights, reactions and vocabulary")
    p.add_argument("--tiny", action="store_true", help="2-layer / 128-d decoder (configs/config_bert_tiny.json)")
    add_tokenizer_flags(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
