"""SMILES -> PV prediction driver -- the counterpart of the reference's d_smiles2pv.py (same flags; all 53 properties of every SMILES of
a file, one property per autoregressive step, straight from the pretraining checkpoint):

  python smiles2pv.py --checkpoint ./Pretrain/checkpoint_SPMM.ckpt --vocab_filename ./vocab_bpe_300.txt --input_file s2p_input.txt \
                      --normalize normalize.pkl --property_names property_name.txt --output predicted_properties.csv
  python smiles2pv.py --synthetic --tiny                                    (no data files: seeded weights, SMILES and vocabulary)

What differs from the reference, on purpose: the molecules are sorted by token length into batches (and written back in input order), every
batch runs on the engine path (spmm_amd.decode.predict_properties: text encoded once on packed rows, cross-attention keys / values
projected once, an append-only cache of embedded prefix rows); the reference values its dataset computes with RDKit come from
`--reference_csv` instead (one 53-vector per line, in the order of --input_file), and r^2 is computed here (1 - SS_res / SS_tot per
property, scikit-learn's definition) -- neither RDKit nor scikit-learn is needed.  With reference values the driver prints what
`metric_eval` prints; without, it writes one de-normalised 53-vector per molecule."""
import argparse
import csv
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from pv2smiles import read_normalize, synthetic_vocab      # noqa: E402  (the mean / std file is read exactly as pv2smiles.py reads it)
# the package's batching helpers, under the names the drivers import
from spmm_amd.tokenizer import MAX_LENGTH, encode_smiles as encode, length_sorted_batches, pad_rows as pad_batch, with_cls      # noqa: E402,F401
from spmm_amd.wordpiece_device import TokenLibrary, add_tokenizer_flags, library_of      # noqa: E402,F401  (a file's molecules: host or device rows)

N_PROPS = 53


# --------------------------------------------------------------------------------------------------------------------- input
def read_smiles(path: str):
    """One SMILES per line (s2p_input.txt); blank lines are skipped."""
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def predict_all(model, tokenizer, smiles, batch_size: int, n_props: int = N_PROPS, predict=None, host_tokenizer=False) -> torch.Tensor:
    """Normalised predictions [len(smiles), n_props] in INPUT order.  host_tokenizer: --host_tokenizer (the Python tokenizer also where
    the GPU could tokenise the file in one launch)."""
    if predict is None:
        from spmm_amd.decode import predict_properties as predict
    lib = library_of(tokenizer, smiles, MAX_LENGTH, model, host_tokenizer)
    out = torch.empty(len(lib), n_props, dtype=torch.float32)
    for idx, ids, mask, n_tokens in lib.batches(batch_size):
        kw = {"n_tokens": n_tokens} if lib.on_device else {}      # (host mask: counted there; device mask: the host's count goes along)
        out[torch.from_numpy(idx)] = predict(model, ids, mask, n_props, **kw).float().cpu()
    return out


# ------------------------------------------------------------------------------------------------------------------- metrics
def denormalize(x, mean, std):
    """d_smiles2pv.py:56: normalised -> raw property values."""
    return x * std + mean


def r2_score(y_true: np.ndarray, y_pred: np.ndarray) -> float:
    """1 - SS_res / SS_tot (scikit-learn's r2_score for one output; a constant y_true gives 1 for a perfect prediction, else 0)."""
    y_true, y_pred = np.asarray(y_true, dtype=np.float64), np.asarray(y_pred, dtype=np.float64)
    ss_res = ((y_true - y_pred) ** 2).sum()
    ss_tot = ((y_true - y_true.mean()) ** 2).sum()
    if ss_tot == 0.0:
        return 1.0 if ss_res == 0.0 else 0.0
    return float(1.0 - ss_res / ss_tot)


def metric_eval(ref: torch.Tensor, cand: torch.Tensor, mean: torch.Tensor, std: torch.Tensor):
    """d_smiles2pv.py:81-107 on normalised [N, P] tensors -> (mean over properties of the normalised RMSE, mean r^2 of the raw values)."""
    n_rmse = torch.sqrt(((ref - cand) ** 2).mean(0))
    rs, cs = denormalize(ref, mean, std).double().numpy(), denormalize(cand, mean, std).double().numpy()
    r2 = np.array([r2_score(rs[:, i], cs[:, i]) for i in range(rs.shape[1])])
    return float(n_rmse.mean()), float(r2.mean())


def read_reference(path: str, n: int, n_props: int = N_PROPS) -> torch.Tensor:
    """One property vector per line (comma separated; a first line that does not parse as numbers is a header)."""
    rows = []
    with open(path, newline="") as f:
        for k, row in enumerate(csv.reader(f)):
            if not row:
                continue
            try:
                rows.append([float(v) for v in row])
            except ValueError:
                if k == 0:
                    continue
                raise SystemExit(f"{path}: line {k + 1} is not a row of numbers")
    ref = torch.tensor(rows, dtype=torch.float32)
    if tuple(ref.shape) != (n, n_props):
        raise SystemExit(f"{path}: {tuple(ref.shape)} values, expected {n} molecules x {n_props} properties")
    return ref


def write_csv(path: str, smiles, values: torch.Tensor, names=None):
    names = names if names else [f"p{i}" for i in range(values.shape[1])]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["smiles"] + list(names))
        for s, v in zip(smiles, values.tolist()):
            w.writerow([s] + [repr(float(x)) for x in v])


def synthetic_smiles(vocab, n: int, seed: int):
    """n made-up strings of 1 .. 30 vocabulary pieces (they tokenise back into pieces of the same vocabulary)."""
    g = np.random.default_rng(seed)
    pieces = [p[2:] for p in vocab if p.startswith("##")]
    return ["".join(pieces[j] for j in g.integers(0, len(pieces), size=int(g.integers(1, 31)))) for _ in range(n)]


# ---------------------------------------------------------------------------------------------------------------------- main
def main(args):
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"smiles2pv.py: --device {args.device}: spmm_amd has no CPU / eager fallback -- its layers are HIP kernels for "
                         "gfx950 and need a GPU (the fp32 CPU restatement under oracle/ is test infrastructure, not a product path)")
    torch.manual_seed(args.seed)
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
    names = None
    if args.property_names:
        with open(args.property_names) as f:
            names = [line.strip() for line in f if line.strip()]
    mean, std = read_normalize(args.normalize) if args.normalize else (torch.zeros(N_PROPS), torch.ones(N_PROPS))
    if args.synthetic:
        smiles = synthetic_smiles(tokenizer.itos, 8, args.seed)
    else:
        if args.checkpoint:
            print("LOADING PRETRAINED MODEL..")
            res = model.load_checkpoint(args.checkpoint, weights_only=True)
            print(f"load checkpoint from {args.checkpoint} (missing {len(res.missing_keys)}, unexpected {len(res.unexpected_keys)})")
        smiles = read_smiles(args.input_file)
    model.eval()
    print("=" * 50)
    print("SMILES-to-PV generation...")
    cand = predict_all(model, tokenizer, smiles, args.batch_size, host_tokenizer=args.host_tokenizer)
    print("SMILES-to-PV generation done")
    if args.reference_csv:
        ref = read_reference(args.reference_csv, len(smiles))
        if args.reference_space == "raw":
            ref = (ref - mean) / std
        n_rmse, r2 = metric_eval(ref, cand, mean, std)
        print("mean of 53 properties' normalized RMSE:", n_rmse)
        print("mean r^2 coefficient of determination:", r2)
    else:
        write_csv(args.output, smiles, denormalize(cand, mean, std), names)
        print(f"Predicted properties are saved in '{args.output}'" + ("" if args.normalize else " (normalised: no --normalize given)"))
    print("=" * 50)
    return cand


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Predict the 53 properties of every SMILES of a file (the reference's d_smiles2pv.py).")
    # the reference's flags (d_smiles2pv.py:154-157)
    p.add_argument("--checkpoint", default="./Pretrain/checkpoint_SPMM.ckpt")
    p.add_argument("--vocab_filename", default="./vocab_bpe_300.txt")
    p.add_argument("--input_file", default="./s2p_input.txt", help="one SMILES per line")
    p.add_argument("--device", default="cuda")
    # additions
    p.add_argument("--batch_size", default=64, type=int, help="molecules per batch (the reference's batch_size_test)")
    p.add_argument("--normalize", default="", help="mean / std of the properties: the reference's normalize.pkl, or an .npz with mean and std")
    p.add_argument("--property_names", default="", help="one property name per line: the header of --output")
    p.add_argument("--output", default="predicted_properties.csv", help="CSV: smiles, then the de-normalised properties")
    p.add_argument("--reference_csv", default="", help="reference property vectors, one comma-separated line per molecule: prints the metrics")
    p.add_argument("--reference_space", default="normalized", choices=("normalized", "raw"), help="whether --reference_csv holds normalised or raw values")
    p.add_argument("--seed", default=0, type=int, help="seed of --synthetic's weights and SMILES")
    p.add_argument("--synthetic", action="store_true", help="no data files: seeded weights, SMILES and vocabulary")
    p.add_argument("--tiny", action="store_true", help="2-layer / 128-d encoders (configs/config_bert_tiny.json)")
    add_tokenizer_flags(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
