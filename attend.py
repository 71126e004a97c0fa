"""Cross-attention map driver: which SMILES tokens does each property attend to, and which properties each token?  The reference has no
such script; the SPMM paper reads the model's chemistry from exactly these maps.  Molecules are given as smiles2pv.py takes its input, a
reaction checkpoint as rxn_predict.py loads it:

  python attend.py --checkpoint ./Pretrain/checkpoint_SPMM.ckpt --vocab_filename ./vocab_bpe_300.txt --input_file molecules.txt \
                   --pv_csv pv.csv --property_names property_name.txt --normalize normalize.pkl --output attention.csv --npz attention.npz
  python attend.py --rxn --checkpoint ./output/RXN/checkpoint_best.pth --vocab_filename ./vocab_bpe_300.txt --input_file pairs.txt
  python attend.py --synthetic 6 --tiny          python attend.py --rxn --synthetic 4 --tiny          (no data files: seeded weights and input)

Every line of --input_file is one SMILES; its property vector is row i of --pv_csv (53 values per row, raw values normalised with
--normalize) or, without --pv_csv, the model's own prediction (spmm_amd.decode.predict_properties: RDKit is not needed).
--mask_properties NAME,... puts the learned mask token at those properties.  --rxn reads `source<TAB>product` lines and writes
product-token -> reactant-token maps (spmm_amd.attribution.reaction_attention_maps).  Molecules are sorted by token length into batches
and written back in input order.  The CSV is long format, one row per (line, layer, direction, head, query, key): labels are the
property name or [CLS] on the PV side and the WordPiece piece with its character span in the input SMILES, `piece[start:end]`, on the
text side.  For each molecule the report names the three properties whose row is most concentrated (lowest entropy) and the tokens they
attend to."""
import argparse
import csv
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from pv2smiles import read_normalize, synthetic_vocab                       # noqa: E402
from rxn_predict import MAX_SOURCE, synthetic_reactions                     # noqa: E402
from score import read_pairs                                                # noqa: E402
from smiles2pv import add_tokenizer_flags, encode, length_sorted_batches, library_of, pad_batch, read_smiles, synthetic_smiles      # noqa: E402,F401

N_PROPS = 53
MAX_LENGTH = 100
COLUMNS = ["line", "layer", "direction", "head", "query_index", "query_label", "key_index", "key_label", "weight"]
SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]")


# --------------------------------------------------------------------------------------------------------------------- labels
def property_labels(names):
    return ["[CLS]"] + list(names)


def token_labels(itos, ids_row):
    """Labels of a token row: `piece[start:end]` with the character span of the piece in the input SMILES (pieces are laid end to end from
    character 0; the '##' marker is not part of the text), the bare name for [CLS] / [SEP]; a row that holds [UNK] has no spans (one
    unmatched position makes the whole molecule one [UNK])."""
    toks = [itos[int(i)] for i in ids_row]
    spans = "[UNK]" not in toks
    out, at = [], 0
    for t in toks:
        if t in SPECIALS:
            out.append(t)
            continue
        text = t[2:] if t.startswith("##") else t
        out.append(f"{text}[{at}:{at + len(text)}]" if spans else text)
        at += len(text)
    return out


def read_property_names(path: str):
    if not path:
        return [f"property_{i}" for i in range(N_PROPS)]
    with open(path) as f:
        names = [line.strip() for line in f if line.strip()]
    if len(names) != N_PROPS:
        raise SystemExit(f"{path}: {len(names)} property names, {N_PROPS} expected")
    return names


def read_pv_csv(path: str, n: int):
    """n rows of 53 values (a first row that is not numeric is a header)."""
    rows = []
    with open(path, newline="") as f:
        for no, row in enumerate(csv.reader(f), 1):
            if not row or not "".join(row).strip():
                continue
            try:
                vals = [float(x) for x in row]
            except ValueError:
                if not rows and no == 1:
                    continue
                raise SystemExit(f"{path}:{no}: not a row of numbers")
            if len(vals) != N_PROPS:
                raise SystemExit(f"{path}:{no}: {len(vals)} values, {N_PROPS} expected")
            rows.append(vals)
    if len(rows) != n:
        raise SystemExit(f"{path}: {len(rows)} property vectors for {n} molecules")
    return torch.tensor(rows, dtype=torch.float32)


def mask_from_names(spec: str, names):
    """--mask_properties NAME,... -> prop_mask [53] (1 = the learned mask token stands there)."""
    mask = torch.zeros(len(names))
    for name in [s.strip() for s in spec.split(",") if s.strip()]:
        if name not in names:
            raise SystemExit(f"--mask_properties: unknown property {name!r}")
        mask[names.index(name)] = 1
    return mask


# --------------------------------------------------------------------------------------------------------------------- output
def map_rows(line: int, layer: int, direction: str, m, qlabels, klabels):
    """CSV rows of one map: m [Lq, Lkv] (head 'mean') or [nH, Lq, Lkv] (head index), queries outer, keys inner."""
    a = np.asarray(m, dtype=np.float64)
    heads = [("mean", a)] if a.ndim == 2 else [(str(h), a[h]) for h in range(a.shape[0])]
    assert heads[0][1].shape == (len(qlabels), len(klabels)), (heads[0][1].shape, len(qlabels), len(klabels))
    rows = []
    for hname, x in heads:
        for qi, ql in enumerate(qlabels):
            for ki, kl in enumerate(klabels):
                rows.append((line, layer, direction, hname, qi, ql, ki, kl, repr(float(x[qi, ki]))))
    return rows


def row_entropy(m):
    p = np.clip(np.asarray(m, dtype=np.float64), 0.0, None)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -(np.where(p > 0, p * np.log(p), 0.0)).sum(axis=-1)


def entropy_ranking(m, qlabels, klabels, k: int = 3, top: int = 3):
    """The k queries other than [CLS] with the most concentrated (lowest-entropy) row of m [Lq, Lkv] (ties by index), each with its `top`
    largest keys -> [(query label, entropy, [(key label, weight), ..]), ..]."""
    a = np.asarray(m, dtype=np.float64)
    if a.ndim == 3:
        a = a.mean(0)
    ent = row_entropy(a)
    cand = [i for i, l in enumerate(qlabels) if l != "[CLS]"]
    order = sorted(cand, key=lambda i: (ent[i], i))[:k]
    out = []
    for i in order:
        keys = sorted(range(a.shape[1]), key=lambda j: (-a[i, j], j))[:top]
        out.append((qlabels[i], float(ent[i]), [(klabels[j], float(a[i, j])) for j in keys]))
    return out


def attend_all(lengths, batch_size: int, run_batch):
    """Results in INPUT order: the lines go to `run_batch(index array)` in batches sorted by token length; it returns one result per line
    of the batch."""
    out = [None] * len(lengths)
    for idx in length_sorted_batches(lengths, batch_size):
        for i, r in zip(idx.tolist(), run_batch(idx)):
            out[i] = r
    return out


def write_csv(path: str, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(COLUMNS)
        w.writerows(rows)


def parse_layer(spec: str):
    if spec == "all":
        return "all"
    try:
        return tuple(int(s) for s in spec.split(","))
    except ValueError:
        raise SystemExit(f"--layer {spec!r}: indices among the fusion layers (negative from the last), comma separated, or 'all'")


def check_args(args):
    """What can be refused before a model is built."""
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be at least 1")
    if args.synthetic < 0:
        raise SystemExit("--synthetic must not be negative")
    if not args.synthetic and not args.input_file:
        raise SystemExit("give the molecules: --input_file FILE (one SMILES per line; with --rxn one source<TAB>product per line)")
    if args.rxn and (args.pv_csv or args.property_names or args.normalize or args.mask_properties):
        raise SystemExit("--rxn maps products onto their reactants: --pv_csv / --property_names / --normalize / --mask_properties belong to the property side")
    if args.rxn and args.direction != "both":
        raise SystemExit("--rxn has one direction (product2reactant): leave --direction out")
    if args.mask_properties and not args.property_names:
        raise SystemExit("--mask_properties needs --property_names (one property name per line)")
    args.layers = parse_layer(args.layer)
    return args


# ---------------------------------------------------------------------------------------------------------------------- main
def main(args):
    check_args(args)
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"attend.py: --device {args.device}: spmm_amd has no CPU / eager fallback -- its layers are HIP kernels for gfx950 and "
                         "need a GPU")
    torch.manual_seed(args.seed)
    from spmm_amd import attribution as AT
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
    pad, itos = tokenizer.pad_token_id, tokenizer.itos
    kw = dict(layers=args.layers, heads=args.heads)
    if args.rxn:
        sources, smiles = synthetic_reactions(itos, args.synthetic, args.seed) if args.synthetic else read_pairs(args.input_file)
        src_lib = library_of(tokenizer, sources, MAX_SOURCE, model, args.host_tokenizer)
        lib_t = library_of(tokenizer, smiles, MAX_LENGTH, model, args.host_tokenizer)
        src_rows, rows_t = src_lib.host_rows(), lib_t.host_rows()                      # (the token labels of the CSV)

        def run_batch(idx):
            sid, smask, _ = src_lib.take(idx)
            ids, mask, _ = lib_t.take(idx)
            maps = AT.reaction_attention_maps(model, sid, smask, ids, mask, **kw)
            return [{(l, d): maps.get(p, l, d).cpu().numpy() for l in maps.layers for d in maps.directions} for p in range(len(idx))]
        qlab = [token_labels(itos, r) for r in rows_t]
        klab = {AT.RXN_DIRECTION: [token_labels(itos, r) for r in src_rows]}
    else:
        names = read_property_names(args.property_names)
        smiles = synthetic_smiles(itos, args.synthetic, args.seed) if args.synthetic else read_smiles(args.input_file)
        lib_t = library_of(tokenizer, smiles, MAX_LENGTH, model, args.host_tokenizer)
        rows_t = lib_t.host_rows()                                                     # (the token labels of the CSV)
        prop_mask = mask_from_names(args.mask_properties, names) if args.mask_properties else None
        pv_all = None
        if args.pv_csv:
            pv_all = read_pv_csv(args.pv_csv, len(smiles))
            if args.normalize:
                mean, std = read_normalize(args.normalize)
                pv_all = (pv_all - mean) / std
        else:
            print("no --pv_csv: every molecule's property vector is the model's own prediction")

        def run_batch(idx):
            from spmm_amd.decode import predict_properties
            ids, mask, n_tokens = lib_t.take(idx)
            pv = pv_all[torch.from_numpy(idx)] if pv_all is not None else predict_properties(model, ids, mask, N_PROPS, n_tokens=n_tokens).float()
            maps = AT.cross_attention_maps(model, pv, prop_mask, ids, mask, direction=args.direction, **kw)
            return [{(l, d): maps.get(p, l, d).cpu().numpy() for l in maps.layers for d in maps.directions} for p in range(len(idx))]
        plab = property_labels(names)
        tlab = [token_labels(itos, r) for r in rows_t]
        qlab, klab = None, None
    print("=" * 50)
    print(f"Reading the attention of {len(smiles)} {'reactions' if args.rxn else 'molecules'}...")
    results = attend_all([len(r) for r in rows_t], args.batch_size, run_batch)
    rows, arrays = [], {}
    for i, res in enumerate(results):
        for (l, d), m in sorted(res.items()):
            if args.rxn:
                ql, kl = qlab[i], klab[d][i]
            else:
                ql, kl = (plab, tlab[i]) if d == "pv2text" else (tlab[i], plab)
            rows += map_rows(i + 1, l, d, m, ql, kl)
            arrays[f"line{i + 1}_layer{l}_{d}"] = m
        l_last = max(l for l, _ in res)                    # the report: the last requested layer, properties as queries where they are
        d0 = "pv2text" if (l_last, "pv2text") in res else min(d for l, d in res if l == l_last)
        m = res[(l_last, d0)]
        ql, kl = (qlab[i], klab[d0][i]) if args.rxn else ((plab, tlab[i]) if d0 == "pv2text" else (tlab[i], plab))
        print(f"line {i + 1}: {smiles[i]}   (layer {l_last}, {d0})")
        for name, ent, keys in entropy_ranking(m, ql, kl):
            print("    %-28s entropy %.3f -> %s" % (name, ent, ", ".join(f"{k} {w:.3f}" for k, w in keys)))
    write_csv(args.output, rows)
    if args.npz:
        np.savez(args.npz, **arrays)
        print(f"{len(arrays)} maps are saved in '{args.npz}'")
    print(f"{len(rows)} weights of {len(results)} lines are saved in '{args.output}'")
    print("=" * 50)
    return rows


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Write the cross-attention maps between properties and SMILES tokens (or, --rxn, products and reactants).")
    p.add_argument("--checkpoint", default="", help="a pretraining checkpoint (with --rxn: a reaction checkpoint, loaded as rxn_predict.py does)")
    p.add_argument("--vocab_filename", default="./vocab_bpe_300.txt")
    p.add_argument("--device", default="cuda")
    p.add_argument("--batch_size", default=256, type=int, help="molecules read together")
    p.add_argument("--input_file", default="", help="one SMILES per line; with --rxn one source<TAB>product per line")
    p.add_argument("--pv_csv", default="", help="one row of 53 property values per molecule (default: the model's own prediction)")
    p.add_argument("--property_names", default="", help="one property name per line; line i names property i")
    p.add_argument("--normalize", default="", help="mean / std of the properties: the reference's normalize.pkl, or an .npz with mean and std")
    p.add_argument("--mask_properties", default="", help="NAME,...: properties replaced by the learned mask token")
    p.add_argument("--layer", default="-1", help="indices among the fusion layers (negative from the last), comma separated, or 'all'")
    p.add_argument("--heads", default="mean", choices=["mean", "all"])
    p.add_argument("--direction", default="both", choices=["pv2text", "text2pv", "both"])
    p.add_argument("--output", default="attention.csv", help="CSV, long format: " + ", ".join(COLUMNS))
    p.add_argument("--npz", default="", help="also write the raw arrays")
    p.add_argument("--rxn", action="store_true", help="product-token -> reactant-token maps on the reaction model")
    p.add_argument("--seed", default=0, type=int, help="seed of --synthetic's weights and input")
    p.add_argument("--synthetic", default=0, type=int, metavar="N", help="no data files: seeded weights, N made-up molecules (or reactions)")
    p.add_argument("--tiny", action="store_true", help="2-layer / 128-d encoders (configs/config_bert_tiny.json)")
    add_tokenizer_flags(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
