"""PV -> SMILES generation driver -- the counterpart of the reference's d_pv2smiles_single.py (flags, one property vector, n samples,
stochastic k-beam search with k = 2, any subset of the 53 properties left unspecified):

  python pv2smiles.py --checkpoint ./Pretrain/checkpoint_SPMM.ckpt --vocab_filename ./vocab_bpe_300.txt --input p2s_input.csv \
                      --property_names property_name.txt --normalize normalize.pkl --n_generate 1000 --k 2 --seed 7
  python pv2smiles.py --synthetic --tiny --n_generate 8 --seed 1                          (no data files: seeded weights, PV and vocabulary)
  python pv2smiles.py ... --prefix c1ccccc1                                               (every molecule starts with this SMILES fragment)
  python pv2smiles.py ... --guidance 2 --temperature 0.8 --top_k 40 --top_p 0.95          (the distribution the samples are drawn from)
  python pv2smiles.py ... --syntax                                                        (only well-formed SMILES strings are generated)
  python pv2smiles.py ... --distinct --n_generate 1000                                    (1000 DIFFERENT token sequences: sampling without replacement)

--guidance w is classifier-free guidance between the requested condition and the same decoder with every property masked,
log p~ = log p_u + w (log p_c - log p_u): 1 (default) is the conditioned model alone, w > 1 pushes the samples towards the requested
properties, 0 is the unconditional model.  --temperature divides the guided logits, --top_k keeps the K most probable tokens (0: all; at
least --k), --top_p the smallest set of them whose probability reaches p (1: all).  Order: guidance, temperature, top-k, then top-p on
the renormalised distribution; at least --k tokens always stay.  With all four at their defaults the run is the one without them.

--syntax constrains every position to the tokens that can follow the beam's own history in a well-formed SMILES string that still ends
inside --max_steps (spmm_amd/smiles_syntax.py): balanced parentheses, paired ring-bond digits, closed bracket atoms, no trailing bond or
dot, a non-empty molecule.  Syntax only: element symbols, valence and aromaticity are not checked, two-digit ring labels (%nn) are never
generated, and a ring closed on the atom that opened it (C11) passes.  Off by default; with a --prefix that is not the beginning of such a
string, or cannot be closed in --max_steps tokens, the run stops before anything is decoded.  `well-formed: n / N` (the same automaton
over the N strings written, without RDKit) is reported with and without the flag.

--distinct replaces the n independent k-beam searches by ONE stochastic beam search (Kool, van Hoof, Welling 2019;
spmm_amd.decode.sample_distinct): --n_generate (<= 1024) token sequences drawn WITHOUT replacement from the model's distribution, so no
two of them are equal, in sampling order; the same --seed with a larger --n_generate extends the list.  It composes with --seed, --prefix,
--temperature, --top_k, --top_p, --syntax and --max_steps; --guidance other than 1 and --stochastic False are refused, --k and --chunk are
ignored.  Sequences still open after --max_steps positions are dropped and counted, so fewer than --n_generate lines may be written.  Two
token sequences can spell the same string (WordPiece splits a string in more than one way): the count of distinct strings is printed, and
nothing is filtered.

What differs from the reference, on purpose: the seed is a flag (the reference draws one at random) and the same seed gives the same
molecules whatever `--chunk` is; all samples of a chunk are decoded together against a K/V cache (spmm_amd.decode.generate_with_property);
the conditions come from `--input` / `--property_names` instead of files next to the script; the CSV is read with the csv module; validity
and the normalised RMSE of the controlled properties are reported only where RDKit is installed."""
import argparse
import csv
import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_PROPS = 53


def str2bool(s) -> bool:
    return str(s).lower() in ("1", "true", "yes", "y")


# ------------------------------------------------------------------------------------------------------------------- conditions
def read_condition(input_csv: str, property_names: str):
    """d_pv2smiles_single.py:186-195: `property,input_value` rows -> (prop_input [53], prop_mask [53]); a property that the file does not
    name is masked (1) and its input is 0.  property_names: one name per line, the line number is the property's index."""
    with open(property_names) as f:
        index = {line.strip(): i for i, line in enumerate(f) if line.strip()}
    prop_input, prop_mask = torch.zeros(len(index)), torch.ones(len(index))
    with open(input_csv, newline="") as f:
        for row in csv.DictReader(f):
            name = row["property"].strip()
            if name not in index:
                raise SystemExit(f"{input_csv}: unknown property {name!r} (not in {property_names})")
            prop_input[index[name]] = float(row["input_value"])
            prop_mask[index[name]] = 0
    return prop_input, prop_mask


def read_normalize(path: str):
    """(mean [53], std [53]) from the reference's normalize.pkl (a pickled pair) or an .npz with `mean` and `std`."""
    if path.endswith(".npz"):
        z = np.load(path)
        mean, std = z["mean"], z["std"]
    else:
        with open(path, "rb") as f:
            mean, std = pickle.load(f)
    return torch.as_tensor(np.asarray(mean), dtype=torch.float32), torch.as_tensor(np.asarray(std), dtype=torch.float32)


def synthetic_vocab(size: int):
    """Specials at the reference's ids, then `size - 4` made-up continuation pieces (decoding needs names, nothing else)."""
    atoms = ["C", "c", "N", "n", "O", "o", "S", "s", "F", "Cl", "Br", "(", ")", "=", "#", "1", "2", "3", "4", "[nH]"]
    pieces = ["##" + a for a in atoms] + ["##" + a + b for a in atoms for b in atoms]
    return ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + pieces[: size - 4]


def prefix_ids(tokenizer, fragment: str):
    """--prefix: the SMILES fragment every molecule starts with -> token ids [CLS] piece_1 .. piece_n, tokenised as the model's text is
    ('[CLS]' + fragment is one word: the literal [CLS] piece, then the fragment's pieces in their '##' form).  The fragment is tokenised
    greedily on its own, so its last piece may differ from how a whole molecule would split there."""
    if not fragment or fragment != "".join(fragment.split()):
        raise SystemExit(f"--prefix {fragment!r}: a SMILES fragment without white space is needed")
    ids = tokenizer.encode("[CLS]" + fragment)[1:-1]
    if tokenizer.unk_token_id in ids or ids[0] != tokenizer.cls_token_id:
        raise SystemExit(f"--prefix {fragment!r}: the vocabulary cannot spell this fragment ([UNK])")
    return ids


# ------------------------------------------------------------------------------------------------------------------- metrics
def report(samples, smiles, prop_input, prop_mask, norm, names):
    n = len(samples)
    none = sum(1 for s in samples if not s)
    done = [s for s in smiles if s]
    print(f"samples: {n}")
    print(f"without a final hypothesis: {none}")
    print(f"uniqueness (strings): {len(set(done)) / max(len(done), 1):.4f}")
    from spmm_amd.smiles_syntax import well_formed
    print(f"well-formed: {sum(1 for s in done if well_formed(s))} / {len(done)}")           # (syntax only; of the molecules that were finished)
    try:
        from rdkit import Chem
        from rdkit.Chem import Descriptors
    except ImportError:
        print("validity / normalised RMSE: not computed (RDKit is not installed)")
        return
    mols = [(s, Chem.MolFromSmiles(s)) for s in done]
    valid = [(s, m) for s, m in mols if m is not None]
    print(f"validity: {len(valid) / max(n, 1):.4f}")
    canon = {Chem.MolToSmiles(m, isomericSmiles=False) for _, m in valid}
    print(f"uniqueness (canonical, among valid): {len(canon) / max(len(valid), 1):.4f}")
    if norm is None or names is None or not valid:
        return
    mean, std = norm
    ctrl = [i for i in range(len(names)) if prop_mask[i] == 0 and hasattr(Descriptors, names[i])]
    if not ctrl:
        return
    err = []
    for _, m in valid:
        got = torch.tensor([float(getattr(Descriptors, names[i])(m)) for i in ctrl])
        err.append(((got - mean[ctrl]) / std[ctrl] - (prop_input[ctrl] - mean[ctrl]) / std[ctrl]) ** 2)
    rmse = torch.sqrt(torch.stack(err).mean(0))
    print(f"mean of controlled properties' normalized RMSE: {rmse.mean().item():.4f}")


DISTINCT_MAX = 1024       # spmm_amd.decode.DISTINCT_MAX: the slots of one stochastic beam search


def distinct_args(args):
    """--distinct against the other flags, before anything is built: SystemExit for what it cannot do, else the lines to print."""
    if args.n_generate < 1 or args.n_generate > DISTINCT_MAX:
        raise SystemExit(f"pv2smiles.py --distinct: --n_generate {args.n_generate} outside [1, {DISTINCT_MAX}]: one search draws at most {DISTINCT_MAX} "
                         "distinct sequences per property vector")
    if float(args.guidance) != 1.0:
        raise SystemExit(f"pv2smiles.py --distinct: --guidance {args.guidance:g} is not available with --distinct (guidance 1 only)")
    if not args.stochastic:
        raise SystemExit("pv2smiles.py --distinct: --stochastic False asks for the deterministic beam search; --distinct is a sampling method")
    return [f"distinct: one stochastic beam search of {args.n_generate} slots; --k {args.k} and --chunk {args.chunk} are ignored"]


# ------------------------------------------------------------------------------------------------------------------- main
def main(args):
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    from spmm_amd import decode
    distinct_lines = distinct_args(args) if args.distinct else None
    try:
        warp = decode.check_warp(args.guidance, args.temperature, args.top_k, args.top_p, 1 if args.distinct else args.k)       # (before the model is built)
    except ValueError as e:
        raise SystemExit(f"pv2smiles.py: {e}")
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
        tokenizer = None                                   # (made below, once the model's vocabulary size is known)
    else:
        raise SystemExit(f"--vocab_filename {args.vocab_filename} not found (needed to decode the generated ids)")
    print("Creating model")
    model = SPMM(config=config, tokenizer=tokenizer, no_train=True, device=device)
    if tokenizer is None:
        tokenizer = model.tokenizer = SmilesWordPiece(synthetic_vocab(model.cfg.text.vocab_size))
    names = None
    if args.property_names:
        with open(args.property_names) as f:
            names = [line.strip() for line in f if line.strip()]
    norm = read_normalize(args.normalize) if args.normalize else None
    if args.synthetic:
        # seeded weights (torch.manual_seed above) with [SEP] made a likely token, so that the searches of an untrained model end;
        # a seeded PV with every third property left unspecified
        sd = model.state_dict()
        g = torch.Generator().manual_seed(args.seed)
        bias = torch.randn(sd["text_encoder.cls.predictions.bias"].shape, generator=g) * 1.5
        bias[decode.SEP_ID] = bias.max() - 0.5
        model.load_state_dict({"text_encoder.cls.predictions.bias": bias, "text_encoder.cls.predictions.decoder.bias": bias}, strict=False)
        prop_input = torch.randn(N_PROPS, generator=g)
        prop_mask = (torch.arange(N_PROPS) % 3 == 0).float()
    else:
        if args.checkpoint:
            print("LOADING PRETRAINED MODEL..")
            res = model.load_checkpoint(args.checkpoint, weights_only=True)
            print(f"load checkpoint from {args.checkpoint} (missing {len(res.missing_keys)}, unexpected {len(res.unexpected_keys)})")
        if args.input:
            if not args.property_names:
                raise SystemExit("--input needs --property_names (one property name per line)")
            prop_input, prop_mask = read_condition(args.input, args.property_names)
        else:                                              # nothing specified: unconditional generation (every property masked)
            prop_input, prop_mask = torch.zeros(N_PROPS), torch.ones(N_PROPS)
    model.eval()
    pv = prop_input if norm is None or args.synthetic else (prop_input - norm[0]) / norm[1]
    syntax = None
    if args.syntax:
        try:
            syntax = decode.syntax_table(model, True)      # (the vocabulary check, with a clear message, before anything is decoded)
        except ValueError as e:
            raise SystemExit(f"pv2smiles.py --syntax: {str(e).removeprefix('syntax: ')}")
        print("syntax: every position is constrained to well-formed SMILES (syntax only: no elements, valence, aromaticity, %nn)")
    if args.distinct:
        print("\n".join(distinct_lines))
        print(f"PV-to-SMILES generation of {args.n_generate} distinct token sequences (sampling without replacement), seed {args.seed}...")
    else:
        print(f"PV-to-SMILES generation in {'stochastic' if args.stochastic else 'deterministic'} manner with k={args.k}, seed {args.seed}...")
    prefix = prefix_ids(tokenizer, args.prefix) if args.prefix else None
    if warp is not None:
        print(f"sampling: guidance {warp['guidance']:g}, temperature {warp['temperature']:g}, top_k {warp['top_k']}, top_p {warp['top_p']:g}")
    if prefix is not None:
        print(f"prefix: {args.prefix!r} ({len(prefix)} tokens with [CLS]); every molecule starts with it")
    try:
        if args.distinct:
            found = decode.sample_distinct(model, pv.to(device), args.n_generate, prop_mask.to(device), seed=args.seed, max_steps=args.max_steps,
                                           prefix=prefix, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, syntax=syntax)[0]
            samples = [ids for _, ids in found]
        else:
            samples = decode.generate_with_property(model, pv.to(device), args.n_generate, prop_mask.to(device), k=args.k, stochastic=args.stochastic,
                                                    seed=args.seed, max_steps=args.max_steps, chunk=args.chunk or None, prefix=prefix,
                                                    guidance=args.guidance, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
                                                    syntax=syntax)
    except ValueError as e:
        if syntax is None or not str(e).startswith("syntax:"):
            raise
        raise SystemExit(f"pv2smiles.py --syntax: {str(e).removeprefix('syntax: ')}")
    smiles = [tokenizer.decode(s) for s in samples]
    with open(args.output, "w") as f:
        for s in smiles:
            f.write(s + "\n")
    print("=" * 50)
    if prefix is not None:
        print(f"prefix: {args.prefix} ({len(prefix)} tokens)")
    report(samples, smiles, prop_input, prop_mask, norm, names)
    if args.distinct:
        run = decode.last_distinct
        print(f"distinct: {len({tuple(s) for s in samples})} token sequences, {len(set(smiles))} strings / {args.n_generate} requested")
        print(f"finished: {run['finished'][0]}, unfinished after {args.max_steps} positions (dropped): {run['unfinished'][0]}, empty slots: {run['empty'][0]}")
    print(f"Generated molecules are saved in '{args.output}'")
    print("=" * 50)
    return smiles


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    # the reference's flags (d_pv2smiles_single.py:227-233)
    p.add_argument("--checkpoint", default="./Pretrain/checkpoint_SPMM.ckpt")
    p.add_argument("--vocab_filename", default="./vocab_bpe_300.txt")
    p.add_argument("--device", default="cuda")
    p.add_argument("--n_generate", default=1000, type=int)
    p.add_argument("--k", default=2, type=int)
    p.add_argument("--stochastic", default=True, type=str2bool)
    # additions
    p.add_argument("--seed", default=0, type=int, help="seed of the draws (and of --synthetic's weights and PV): same seed, same molecules")
    p.add_argument("--input", default="", help="CSV with the columns property,input_value: the properties to control (the others are masked)")
    p.add_argument("--property_names", default="", help="one property name per line; line i names property i")
    p.add_argument("--normalize", default="", help="mean / std of the properties: the reference's normalize.pkl, or an .npz with mean and std")
    p.add_argument("--output", default="generated_molecules.txt")
    p.add_argument("--max_steps", default=100, type=int, help="positions decoded at most")
    p.add_argument("--chunk", default=0, type=int, help="samples decoded together (0: all)")
    p.add_argument("--prefix", default="", help="SMILES fragment every generated molecule starts with (tokenised as '[CLS]' + fragment)")
    p.add_argument("--guidance", default=1.0, type=float, help="classifier-free guidance weight w between the condition and the all-masked PV: "
                   "1 = the conditioned model alone (default), > 1 towards the requested properties, 0 = unconditional")
    p.add_argument("--temperature", default=1.0, type=float, help="divides the (guided) logits; > 0")
    p.add_argument("--top_k", default=0, type=int, help="keep the K most probable tokens (0: all; not below --k, which are always kept)")
    p.add_argument("--top_p", default=1.0, type=float, help="nucleus: keep the most probable tokens until their probability reaches p, in (0, 1] (1: all)")
    p.add_argument("--syntax", action="store_true", help="generate well-formed SMILES strings only (syntax: parentheses, ring bonds, bracket atoms, "
                   "bonds; not elements, valence or aromaticity)")
    p.add_argument("--distinct", action="store_true", help="--n_generate (<= 1024) DIFFERENT token sequences by one stochastic beam search (sampling "
                   "without replacement) instead of independent searches; ignores --k and --chunk")
    p.add_argument("--synthetic", action="store_true", help="no data files: seeded weights, property vector and vocabulary")
    p.add_argument("--tiny", action="store_true", help="2-layer / 128-d encoders (configs/config_bert_tiny.json)")
    return p.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
