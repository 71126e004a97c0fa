"""Property-to-molecule retrieval driver: which molecules of a library have these properties?  The reference has no such script; the
query is given as pv2smiles.py takes it and the library as smiles2pv.py takes its input:

  python retrieve.py --checkpoint ./Pretrain/checkpoint_SPMM.ckpt --vocab_filename ./vocab_bpe_300.txt --input p2s_input.csv \
                     --property_names property_name.txt --normalize normalize.pkl --library library.txt --top_k 100 --rerank 16
  python retrieve.py ... --library library.txt --save_index library.idx          (encode the library once ...)
  python retrieve.py ... --index library.idx --input p2s_input.csv                (... and query it many times)
  python retrieve.py ... --index library.idx --query_smiles 'CCO' --top_k 10     (neighbours of a molecule instead of a property query)
  python retrieve.py --synthetic 64 --tiny --top_k 5 --rerank 3                  (no data files: seeded weights, library, query, vocabulary)

Stage one shortlists --top_k molecules by the contrastive similarity of the pretraining (spmm_amd.retrieve.MoleculeIndex.search, a streaming
top-k kernel); stage two re-orders the first --rerank of them by the matching head's probability (spmm_amd.retrieve.match_scores) or, with --rerank_by likelihood, by log p(SMILES | query) per token (spmm_amd.score.score_smiles; the
CSV then ends with a logp_per_token column).  The CSV
has one row per shortlisted molecule: rank, line number in the library (1-based), SMILES, cosine, matching probability (empty beyond
--rerank and for --query_smiles)."""
import argparse
import csv
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from pv2smiles import read_condition, read_normalize, synthetic_vocab      # noqa: E402  (the query is read exactly as pv2smiles.py reads it)
from smiles2pv import add_tokenizer_flags, read_smiles, synthetic_smiles   # noqa: E402  (the library as smiles2pv.py reads its input)

N_PROPS = 53


def ranked_rows(index_row, cosine_row, match_row, smiles, logp_row=None):
    """One query's result -> [(rank, library line number, SMILES, cosine, matching probability or '')], empty slots dropped; with
    logp_row (--rerank_by likelihood) every row ends with the log-likelihood per token or ''."""
    rows = []
    extra = [None] * len(index_row) if logp_row is None else logp_row.tolist()
    for i, c, m, lp in zip(index_row.tolist(), cosine_row.tolist(), match_row.tolist(), extra):
        if i < 0:
            continue
        row = (len(rows) + 1, i + 1, smiles[i] if smiles is not None else "", repr(float(c)), "" if m != m else repr(float(m)))
        rows.append(row if logp_row is None else row + ("" if lp != lp else repr(float(lp)),))
    return rows


def write_csv(path: str, rows, likelihood: bool = False):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["rank", "library_line", "smiles", "cosine", "match_probability"] + (["logp_per_token"] if likelihood else []))
        w.writerows(rows)


def check_args(args):
    """What can be refused before a model is built."""
    if args.top_k < 1:
        raise SystemExit("--top_k must be at least 1")
    if args.rerank < 0:
        raise SystemExit("--rerank must not be negative")
    if not args.synthetic and not (args.library or args.index):
        raise SystemExit("give the library: --library FILE (one SMILES per line) or --index FILE (saved by --save_index)")
    if args.library and args.index:
        raise SystemExit("--library and --index are alternatives")
    if args.query_smiles and args.input:
        raise SystemExit("--query_smiles and --input are alternatives")
    if args.input and not args.property_names:
        raise SystemExit("--input needs --property_names (one property name per line)")
    return args


def main(args):
    check_args(args)
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"retrieve.py: --device {args.device}: spmm_amd has no CPU / eager fallback -- its layers are HIP kernels for gfx950 "
                         "and need a GPU")
    torch.manual_seed(args.seed)
    from spmm_amd import retrieve as R
    from spmm_amd.model import SPMM
    from spmm_amd.tokenizer import SmilesWordPiece

    cfg_dir = os.path.join(ROOT, "configs")
    tiny = "_tiny" if args.tiny else ""
    config = {"embed_dim": 64 if args.tiny else 256, "queue_size": 16 if args.tiny else 36864,
              "bert_config_text": os.path.join(cfg_dir, f"config_bert{tiny}.json"),
              "bert_config_property": os.path.join(cfg_dir, f"config_bert_property{tiny}.json")}
    if os.path.exists(args.vocab_filename):
        tokenizer = SmilesWordPiece(args.vocab_filename)
    elif args.synthetic:
        tokenizer = None
    else:
        raise SystemExit(f"--vocab_filename {args.vocab_filename} not found")
    print("Creating model")
    model = SPMM(config=config, tokenizer=tokenizer, no_train=True, device=device)
    if tokenizer is None:
        tokenizer = model.tokenizer = SmilesWordPiece(synthetic_vocab(model.cfg.text.vocab_size))
    norm = read_normalize(args.normalize) if args.normalize else None
    if args.synthetic:
        g = torch.Generator().manual_seed(args.seed)
        library = synthetic_smiles(tokenizer.itos, args.synthetic, args.seed)
        prop_input = torch.randn(N_PROPS, generator=g)
        prop_mask = (torch.arange(N_PROPS) % 3 == 0).float()
    else:
        if args.checkpoint:
            print("LOADING PRETRAINED MODEL..")
            res = model.load_checkpoint(args.checkpoint, weights_only=True)
            print(f"load checkpoint from {args.checkpoint} (missing {len(res.missing_keys)}, unexpected {len(res.unexpected_keys)})")
        library = read_smiles(args.library) if args.library else None
        if args.input:
            prop_input, prop_mask = read_condition(args.input, args.property_names)
        else:                                              # nothing specified: every property unknown
            prop_input, prop_mask = torch.zeros(N_PROPS), torch.ones(N_PROPS)
    model.eval()
    if library is not None:
        print(f"Encoding {len(library)} molecules...")
        from spmm_amd.wordpiece_device import device_tokenizer_for
        index = R.MoleculeIndex.build(model, tokenizer, library, batch_size=args.batch_size,
                                      tokenizer_device=device_tokenizer_for(tokenizer, device, args.host_tokenizer))
    else:
        index = R.MoleculeIndex.load(args.index, device=device)
        print(f"Loaded {len(index)} molecules from '{args.index}'")
    if args.save_index:
        index.save(args.save_index)
        print(f"Index saved in '{args.save_index}'")
    print("=" * 50)
    if args.query_smiles:
        ids, mask = R.pad_rows(R.encode_smiles(tokenizer, [args.query_smiles]), tokenizer.pad_token_id)
        cosine, idx = R.similar(model, index, ids, mask, args.top_k)
        match, logp = torch.full_like(cosine, float("nan")), None
    else:
        pv = prop_input if norm is None or args.synthetic else (prop_input - norm[0]) / norm[1]
        res = R.retrieve(model, index, None, None, pv.reshape(1, -1), prop_mask, k=args.top_k, rerank=args.rerank, rerank_by=args.rerank_by)
        idx, cosine, match, logp = res.index, res.cosine, res.match, res.logp_per_token
    rows = ranked_rows(idx[0].cpu(), cosine[0].cpu(), match[0].cpu(), index.smiles, None if logp is None else logp[0].cpu())
    write_csv(args.output, rows, likelihood=logp is not None)
    for r in rows[:10]:
        print("%4d  line %-8d cosine %s  match %s  %s" % (r[0], r[1], r[3][:9], r[4][:9] or "-", r[2]))
    print(f"{len(rows)} molecules are saved in '{args.output}'")
    print("=" * 50)
    return rows


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Retrieve the molecules of a library that match a property query (or resemble a molecule).")
    # the query, as pv2smiles.py takes it
    p.add_argument("--checkpoint", default="./Pretrain/checkpoint_SPMM.ckpt")
    p.add_argument("--vocab_filename", default="./vocab_bpe_300.txt")
    p.add_argument("--input", default="", help="CSV with the columns property,input_value: the properties asked for (the others are masked)")
    p.add_argument("--property_names", default="", help="one property name per line; line i names property i")
    p.add_argument("--normalize", default="", help="mean / std of the properties: the reference's normalize.pkl, or an .npz with mean and std")
    p.add_argument("--device", default="cuda")
    p.add_argument("--query_smiles", default="", help="a molecule instead of a property query: its nearest neighbours in the library")
    # the library
    p.add_argument("--library", default="", help="one SMILES per line")
    p.add_argument("--index", default="", help="a library saved by --save_index")
    p.add_argument("--save_index", default="", help="write the encoded library here")
    # the search
    p.add_argument("--top_k", default=100, type=int, help="molecules shortlisted by contrastive similarity")
    p.add_argument("--rerank", default=16, type=int, help="head of the shortlist re-ordered by matching probability (0: none)")
    p.add_argument("--rerank_by", default="match", choices=("match", "likelihood"),
                   help="what orders the head of the shortlist: the matching head's probability, or log p(SMILES | query) per token "
                        "(spmm_amd.score.score_smiles; the CSV gains a logp_per_token column)")
    p.add_argument("--batch_size", default=256, type=int, help="molecules encoded together when the index is built")
    p.add_argument("--output", default="retrieved_molecules.csv", help="CSV: rank, library line number, SMILES, cosine, matching probability")
    p.add_argument("--seed", default=0, type=int, help="seed of --synthetic's weights, library and query")
    p.add_argument("--synthetic", default=0, type=int, metavar="N", help="no data files: seeded weights, N made-up molecules, a made-up query")
    p.add_argument("--tiny", action="store_true", help="2-layer / 128-d encoders (configs/config_bert_tiny.json)")
    add_tokenizer_flags(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
