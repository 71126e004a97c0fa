"""Likelihood scoring driver: how probable is each molecule of a file under a condition?  The reference has no such script; the query is given
as pv2smiles.py takes it, the molecules as smiles2pv.py takes its input, a reaction checkpoint as rxn_predict.py loads it:

  python score.py --checkpoint ./Pretrain/checkpoint_SPMM.ckpt --vocab_filename ./vocab_bpe_300.txt --input p2s_input.csv \
                  --property_names property_name.txt --normalize normalize.pkl --library candidates.txt --output scores.csv
  python score.py --rxn --checkpoint ./output/RXN/checkpoint_best.pth --vocab_filename ./vocab_bpe_300.txt --library pairs.txt
  python score.py --synthetic 8 --tiny            python score.py --rxn --synthetic 8 --tiny         (no data files: seeded weights and input)

PV mode scores log p(SMILES | property vector) of every line of --library (one SMILES per line) under the one query of --input
(spmm_amd.score.score_smiles: the query encoded once per batch, every molecule's unimodal layers on packed rows, the fused LM-head
scoring kernel).  --rxn reads `source<TAB>candidate` lines and scores log p(candidate | source) on the reaction model
(spmm_amd.score.score_products).  Molecules are sorted by token length into batches and written back in input order.  The CSV has one
row per input line: line, smiles, logp, tokens, logp_per_token, perplexity = exp(-logp / tokens); the scored tokens are the molecule's
pieces and the closing [SEP], which is what the beam searches accumulate."""
import argparse
import csv
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from pv2smiles import read_condition, read_normalize, synthetic_vocab      # noqa: E402  (the query is read exactly as pv2smiles.py reads it)
from rxn_predict import MAX_SOURCE, synthetic_reactions                     # noqa: E402
from smiles2pv import TokenLibrary, add_tokenizer_flags, encode, length_sorted_batches, library_of, pad_batch, read_smiles, synthetic_smiles      # noqa: E402,F401

N_PROPS = 53
MAX_LENGTH = 100          # tokens per scored molecule, as the reference's inference scripts truncate
COLUMNS = ["line", "smiles", "logp", "tokens", "logp_per_token", "perplexity"]


def read_pairs(path: str):
    """-> (sources, candidates): one `source<TAB>candidate` per line; blank lines are skipped, a line without a candidate is refused."""
    src, cand = [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.split("\t")
            if len(parts) < 2 or not parts[0] or not parts[1]:
                raise SystemExit(f"{path}:{no}: expected source<TAB>candidate")
            src.append(parts[0])
            cand.append(parts[1])
    return src, cand


def score_rows(smiles, logp, tokens):
    """The CSV's rows from the per-line sums: logp per token and perplexity = exp(-logp / tokens); a line without a scored token has neither."""
    rows = []
    for i, (s, lp, n) in enumerate(zip(smiles, logp, tokens)):
        lp, n = float(lp), int(n)
        per = lp / n if n else float("nan")
        rows.append((i + 1, s, repr(lp), n, repr(per) if n else "", repr(math.exp(-per)) if n else ""))
    return rows


def write_csv(path: str, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(COLUMNS)
        w.writerows(rows)


def score_all(token_rows, batch_size: int, score_batch, pad_id: int = 0):
    """(logp, tokens) of every sequence in INPUT order: the sequences -- token rows, or a TokenLibrary that holds them on the host or the
    device -- go to `score_batch(index array, ids, mask)` in batches sorted by token length; it returns the batch's (logp, n_tokens)."""
    lib = token_rows if isinstance(token_rows, TokenLibrary) else TokenLibrary.from_host(token_rows, pad_id)
    logp, tokens = [0.0] * len(lib), [0] * len(lib)
    for idx, ids, mask, _ in lib.batches(batch_size):
        lp, n = score_batch(idx, ids, mask)
        for i, a, b in zip(idx.tolist(), lp.tolist(), n.tolist()):
            logp[i], tokens[i] = float(a), int(b)
    return logp, tokens


def check_args(args):
    """What can be refused before a model is built."""
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be at least 1")
    if args.synthetic < 0:
        raise SystemExit("--synthetic must not be negative")
    if not args.synthetic and not args.library:
        raise SystemExit("give the molecules: --library FILE (one SMILES per line; with --rxn one source<TAB>candidate per line)")
    if args.rxn and (args.input or args.property_names or args.normalize):
        raise SystemExit("--rxn scores candidates against their sources: --input / --property_names / --normalize belong to the property query")
    if args.input and not args.property_names:
        raise SystemExit("--input needs --property_names (one property name per line)")
    return args


def main(args):
    check_args(args)
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"score.py: --device {args.device}: spmm_amd has no CPU / eager fallback -- its layers are HIP kernels for gfx950 and "
                         "need a GPU")
    torch.manual_seed(args.seed)
    from spmm_amd import score as S
    from spmm_amd.tokenizer import SmilesWordPiece

    cfg_dir = os.path.join(ROOT, "configs")
    tiny = "_tiny" if args.tiny else ""
    if os.path.exists(args.vocab_filename):
        tokenizer = SmilesWordPiece(args.vocab_filename)
    elif args.synthetic:
        tokenizer = None
    else:
        raise SystemExit(f"--vocab_filename {args.vocab_filename} not found")
    print("Creating model")
    if args.rxn:
        from spmm_amd.rxn import SPMMRxn
        model = SPMMRxn(config={"bert_config_text": os.path.join(cfg_dir, f"config_bert{tiny}.json")}, device=device)
    else:
        from spmm_amd.model import SPMM
        config = {"embed_dim": 64 if args.tiny else 256, "queue_size": 16 if args.tiny else 36864,
                  "bert_config_text": os.path.join(cfg_dir, f"config_bert{tiny}.json"),
                  "bert_config_property": os.path.join(cfg_dir, f"config_bert_property{tiny}.json")}
        model = SPMM(config=config, tokenizer=tokenizer, no_train=True, device=device)
    if tokenizer is None:
        tokenizer = SmilesWordPiece(synthetic_vocab(model.cfg.text.vocab_size))
    if args.checkpoint and not args.synthetic:
        print("LOADING PRETRAINED MODEL..")
        res = model.load_pretrained(args.checkpoint) if args.rxn else model.load_checkpoint(args.checkpoint, weights_only=True)
        print(f"load checkpoint from {args.checkpoint} (missing {len(res.missing_keys)}, unexpected {len(res.unexpected_keys)})")
    model.eval()
    pad = tokenizer.pad_token_id
    if args.rxn:
        sources, smiles = synthetic_reactions(tokenizer.itos, args.synthetic, args.seed) if args.synthetic else read_pairs(args.library)
        src_lib = library_of(tokenizer, sources, MAX_SOURCE, model, args.host_tokenizer)

        def score_batch(idx, ids, mask):
            sid, smask, _ = src_lib.take(idx)
            r = S.score_products(model, sid, smask, ids, mask)
            return r.logp.cpu(), r.n_tokens.cpu()
    else:
        if args.synthetic:
            g = torch.Generator().manual_seed(args.seed)
            smiles = synthetic_smiles(tokenizer.itos, args.synthetic, args.seed)
            prop_input, prop_mask = torch.randn(N_PROPS, generator=g), (torch.arange(N_PROPS) % 3 == 0).float()
        else:
            smiles = read_smiles(args.library)
            if args.input:
                prop_input, prop_mask = read_condition(args.input, args.property_names)
            else:                                              # nothing specified: every property unknown
                prop_input, prop_mask = torch.zeros(N_PROPS), torch.ones(N_PROPS)
        norm = read_normalize(args.normalize) if args.normalize else None
        pv = (prop_input if norm is None or args.synthetic else (prop_input - norm[0]) / norm[1]).reshape(1, -1)

        def score_batch(idx, ids, mask):
            pairs = torch.stack([torch.zeros(len(idx), dtype=torch.int64), torch.arange(len(idx))], dim=1)
            r = S.score_smiles(model, pv, ids, mask, pairs=pairs, prop_mask=prop_mask)
            return r.logp.cpu(), r.n_tokens.cpu()
    print("=" * 50)
    print(f"Scoring {len(smiles)} {'candidates against their sources' if args.rxn else 'molecules under the query'}...")
    logp, tokens = score_all(library_of(tokenizer, smiles, MAX_LENGTH, model, args.host_tokenizer), args.batch_size, score_batch, pad)
    rows = score_rows(smiles, logp, tokens)
    write_csv(args.output, rows)
    for r in rows[:10]:
        print("line %-6d logp %-12s tokens %-4d per token %-10s %s" % (r[0], r[2][:11], r[3], r[4][:9] or "-", r[1]))
    total = sum(tokens)
    if total:
        print(f"corpus perplexity: {math.exp(-sum(logp) / total):.4f} over {total} tokens")
    print(f"{len(rows)} scores are saved in '{args.output}'")
    print("=" * 50)
    return rows


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Score molecules by teacher-forced likelihood under a property query (or, --rxn, candidates under their sources).")
    # the query, as pv2smiles.py takes it
    p.add_argument("--checkpoint", default="", help="a pretraining checkpoint (with --rxn: a reaction checkpoint, loaded as rxn_predict.py does)")
    p.add_argument("--vocab_filename", default="./vocab_bpe_300.txt")
    p.add_argument("--input", default="", help="CSV with the columns property,input_value: the properties asked for (the others are masked)")
    p.add_argument("--property_names", default="", help="one property name per line; line i names property i")
    p.add_argument("--normalize", default="", help="mean / std of the properties: the reference's normalize.pkl, or an .npz with mean and std")
    p.add_argument("--device", default="cuda")
    # what is scored
    p.add_argument("--library", default="", help="one SMILES per line; with --rxn one source<TAB>candidate per line")
    p.add_argument("--rxn", action="store_true", help="score log p(candidate | source) on the reaction model")
    p.add_argument("--batch_size", default=256, type=int, help="molecules scored together")
    p.add_argument("--output", default="scores.csv", help="CSV: line, smiles, logp, tokens, logp_per_token, perplexity")
    p.add_argument("--seed", default=0, type=int, help="seed of --synthetic's weights and input")
    p.add_argument("--synthetic", default=0, type=int, metavar="N", help="no data files: seeded weights, N made-up molecules (or reactions), a made-up query")
    p.add_argument("--tiny", action="store_true", help="2-layer / 128-d encoders (configs/config_bert_tiny.json)")
    add_tokenizer_flags(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
