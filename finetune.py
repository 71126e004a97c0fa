"""SPMM fine-tuning driver -- the counterpart of the reference's d_regression.py, d_classification.py and
d_classification_multilabel.py (flags, inline config, train / evaluate loop, best-validation test metric):

  python finetune.py --task regression --train LIPO_train.csv --valid LIPO_valid.csv --test LIPO_test.csv --target_cols exp \
                     --checkpoint ./Pretrain/checkpoint_SPMM.ckpt
  python finetune.py --task classification --train BBBP_train.csv ... --target_cols p_np
  python finetune.py --task multilabel --train clintox_train.csv ... --target_cols FDA_APPROVED CT_TOX
  python finetune.py --task classification --synthetic 256 --tiny            (no data: seeded token ids and targets)

What differs from the reference, on purpose: the CSVs are read with the csv module (the SMILES are used as written: RDKit is not on
the target image), regression targets are normalised with the training split's own mean and std (the reference hard-codes those of
each MoleculeNet split, dataset.py), and ROC-AUC is computed here in numpy (sklearn may be missing)."""
import argparse
import csv
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


# ------------------------------------------------------------------------------------------------------------------- metrics
def roc_auc(y_true, score) -> float:
    """Area under the ROC curve of binary labels: the Mann-Whitney statistic on average ranks (ties count one half), which is what
    sklearn.metrics.roc_auc_score computes.  NaN when only one class is present."""
    y = np.asarray(y_true).astype(bool).ravel()
    s = np.asarray(score, dtype=np.float64).ravel()
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    order = np.argsort(s, kind="mergesort")
    ss = s[order]
    ranks = np.empty(len(s), dtype=np.float64)
    i = 0
    while i < len(s):                                  # average rank over each run of equal scores
        j = i
        while j + 1 < len(s) and ss[j + 1] == ss[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return float((ranks[y].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def macro_roc_auc(y_true, score) -> float:
    """roc_auc_score on [N, C] label / score matrices: the mean over the columns (average='macro')."""
    y, s = np.asarray(y_true), np.asarray(score)
    return float(np.mean([roc_auc(y[:, c], s[:, c]) for c in range(y.shape[1])]))


# ------------------------------------------------------------------------------------------------------------------- data
class CsvData:
    """SMILES column + target columns of a CSV (the reference's SMILESDataset_* minus RDKit canonicalisation): '[CLS]' + SMILES as
    the text, like dataset.py."""

    def __init__(self, path, smiles_col, target_cols, task):
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        self.text = ["[CLS]" + r[smiles_col] for r in rows]
        y = np.array([[float(r[c]) for c in target_cols] for r in rows], dtype=np.float32)
        self.y = torch.from_numpy(y[:, 0].astype(np.int64) if task == "classification" else (y[:, 0] if task == "regression" else y))

    def __len__(self):
        return len(self.text)


class SyntheticData:
    """N seeded token-id rows ([CLS] pieces [SEP], length U{Lt/2..Lt}, already sliced [:, 1:] like the scripts do) and targets that
    depend on the ids, so that a model can learn them."""

    def __init__(self, n, seq_len, task, n_output, seed, vocab_size=300):
        g = torch.Generator().manual_seed(seed)
        ids = torch.zeros(n, seq_len, dtype=torch.long)
        lens = torch.randint(max(seq_len // 2, 3), seq_len + 1, (n,), generator=g)
        for i in range(n):
            L = int(lens[i])
            ids[i, 0] = 2
            ids[i, 1:L - 1] = torch.randint(4, vocab_size, (L - 2,), generator=g)
            ids[i, L - 1] = 3
        self.text = ids
        feat = (ids[:, 1:6].float() / vocab_size).mean(1) + lens.float() / seq_len
        if task == "regression":
            self.y = feat + 0.1 * torch.randn(n, generator=g)
        elif task == "classification":
            self.y = (feat > feat.median()).long()
        else:
            self.y = torch.stack([(feat + 0.2 * torch.randn(n, generator=g) > feat.median()).float() for _ in range(n_output)], 1)

    def __len__(self):
        return self.text.shape[0]


def batches(data, batch_size, tokenizer, device, drop_last):
    """(ids, mask) on the device with the host's valid-token count, and targets, in order (the scripts' DataLoader: shuffle=False)."""
    n = len(data)
    stop = n - n % batch_size if drop_last else n
    for b in range(0, stop, batch_size):
        if torch.is_tensor(data.text):
            ids = data.text[b:b + batch_size]
            ids = ids[:, :int((ids != 0).any(0).nonzero().max()) + 1]         # padding='longest'
            mask = (ids != 0).long()
        else:
            ti = tokenizer(data.text[b:b + batch_size], padding="longest", truncation=True, max_length=100, return_tensors="pt")
            ids, mask = ti.input_ids[:, 1:], ti.attention_mask[:, 1:]
        yield ids.to(device), mask, data.y[b:b + batch_size]


# ------------------------------------------------------------------------------------------------------------------- loop
def evaluate(model, data, tokenizer, device, task, norm):
    model.eval()
    preds, ys = [], []
    with torch.no_grad():
        for ids, mask, y in batches(data, 16, tokenizer, device, False):
            preds.append(model(ids, mask, None, eval=True).float().cpu())
            ys.append(y)
    model.train()
    p, y = torch.cat(preds), torch.cat(ys)
    if task == "regression":                          # RMSE on the de-normalised values (d_regression.py:95-104)
        mean, std = norm
        return float(torch.sqrt(torch.mean(((p * std + mean) - (y * std + mean)) ** 2))), {}
    if task == "classification":                      # softmax score of class 1 (d_classification.py:90-103)
        score = torch.softmax(p, -1)
        pred = score.argmax(-1)
        extra = {"acc": float((pred == y).float().mean()),
                 "SE": float(((pred == 1) & (y == 1)).sum() / max(int((y == 1).sum()), 1)),
                 "SP": float(((pred == 0) & (y == 0)).sum() / max(int((y == 0).sum()), 1))}
        return roc_auc(y.numpy(), score[:, 1].numpy()), extra
    return macro_roc_auc(y.numpy(), torch.sigmoid(p).numpy()), {}


def main(args):
    if args.dry_run:                                 # CPU plumbing check: every launch validated against the C ABI, none executed
        from spmm_amd import ops
        ops._DRY_RUN = True
        device = torch.device("cpu")
    else:
        device = torch.device("cuda")
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    from spmm_amd.finetune import SPMMClassifier, SPMMMultiLabelClassifier, SPMMRegressor
    from spmm_amd.tokenizer import SmilesWordPiece

    task = args.task
    n_output = 1 if task == "regression" else (len(args.target_cols) if task == "multilabel" else args.n_output)
    tokenizer = SmilesWordPiece(args.vocab_filename) if os.path.exists(args.vocab_filename) else None
    if args.synthetic:
        n = args.synthetic
        full = SyntheticData(n, args.seq_len, task, n_output, args.seed)
        splits = []
        for lo, hi in ((0, int(0.8 * n)), (int(0.8 * n), int(0.9 * n)), (int(0.9 * n), n)):
            d = SyntheticData.__new__(SyntheticData)
            d.text, d.y = full.text[lo:hi], full.y[lo:hi]
            splits.append(d)
        d_train, d_val, d_test = splits
    else:
        if tokenizer is None:
            raise SystemExit(f"--vocab_filename {args.vocab_filename} not found (needed to tokenise the CSVs)")
        d_train, d_val, d_test = (CsvData(p, args.smiles_col, args.target_cols, task) for p in (args.train, args.valid, args.test))
    norm = (0.0, 1.0)
    if task == "regression":                         # the training split's mean / std normalise every split (dataset.py)
        mean, std = float(d_train.y.mean()), float(d_train.y.std())
        for d in (d_train, d_val, d_test):
            d.y = (d.y - mean) / std
        norm = (mean, std)
    print(len(d_train), len(d_val), len(d_test))

    cfg_path = os.path.join(ROOT, "configs", "config_bert_tiny.json" if args.tiny else "config_bert.json")
    config = {"batch_size_train": args.batch_size, "bert_config_text": cfg_path,
              "schedular": {"sched": "cosine", "lr": args.lr, "epochs": args.epoch, "min_lr": args.min_lr, "decay_rate": 1,
                            "warmup_lr": 0.5e-5, "warmup_epochs": 1, "cooldown_epochs": 0},
              "optimizer": {"opt": "adamW", "lr": args.lr, "weight_decay": 0.02}}
    cls = {"regression": SPMMRegressor, "classification": SPMMClassifier, "multilabel": SPMMMultiLabelClassifier}[task]
    model = cls(tokenizer=tokenizer, config=config, n_output=n_output, device=device).train()
    print("#parameters:", sum(p.numel() for p in model.parameters()))
    if args.checkpoint:
        missing, unexpected = model.load_pretrained(args.checkpoint)
        print(f"load checkpoint from {args.checkpoint} (missing {len(missing)}, unexpected {len(unexpected)})")

    higher = task != "regression"
    best_valid, best_test = None, None
    for epoch in range(args.epoch):
        print("TRAIN", epoch)
        loss = None
        for i, (ids, mask, y) in enumerate(batches(d_train, args.batch_size, tokenizer, device, task != "multilabel")):
            loss = model.training_step(((ids, mask), y), i)
        if loss is not None:
            print(f"loss={float(loss):.4f}, lr={model.optimizers().param_groups[0]['lr']:.6f}")
        val, vx = evaluate(model, d_val, tokenizer, device, task, norm)
        test, tx = evaluate(model, d_test, tokenizer, device, task, norm)
        name = "RMSE" if task == "regression" else "AUROC"
        print(f"VALID {name}: {val:.4f} {vx or ''}")
        print(f"TEST {name}: {test:.4f} {tx or ''}")
        if best_valid is None or (val > best_valid if higher else val < best_valid):
            best_valid, best_test = val, test
        model.on_train_epoch_end()
    print(f"Test set {'AUROC' if higher else 'RMSE'} of the checkpoint with best validation: {best_test}")
    return best_test


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--task", choices=("regression", "classification", "multilabel"), default="classification")
    p.add_argument("--train", default="")
    p.add_argument("--valid", default="")
    p.add_argument("--test", default="")
    p.add_argument("--smiles_col", default="smiles")
    p.add_argument("--target_cols", nargs="+", default=["label"], help="target column(s); several for --task multilabel")
    p.add_argument("--n_output", type=int, default=2, help="classes of --task classification")
    p.add_argument("--checkpoint", default="")
    p.add_argument("--vocab_filename", default="./vocab_bpe_300.txt")
    p.add_argument("--seed", default=42, type=int)
    p.add_argument("--lr", default=5e-5, type=float)
    p.add_argument("--min_lr", default=5e-6, type=float)
    p.add_argument("--epoch", default=15, type=int)
    p.add_argument("--batch_size", default=16, type=int)
    p.add_argument("--synthetic", type=int, default=0, help="train on N seeded synthetic samples (80/10/10 split) instead of the CSVs")
    p.add_argument("--seq_len", type=int, default=64, help="longest synthetic sequence")
    p.add_argument("--tiny", action="store_true", help="2-layer / 128-d encoder (configs/config_bert_tiny.json)")
    p.add_argument("--dry_run", action="store_true", help="no GPU: validate every kernel call against the C ABI without launching")
    return p.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
