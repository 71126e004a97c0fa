"""Reaction prediction fine-tuning driver -- the counterpart of the reference's `d_rxn_prediction.py` without `--evaluate` (forward synthesis
on USPTO-480k, retrosynthesis on USPTO-50k): seq2seq fine-tuning of the reactant encoder and the product decoder from a pretraining
checkpoint, validation and test by greedy or k-beam search after every epoch, `checkpoint_best.pth` at the best validation accuracy:

  python rxn_finetune.py --checkpoint ./Pretrain/checkpoint_SPMM_20m.ckpt --vocab_filename ./vocab_bpe_300.txt --mode forward \
                         --train train_parsed.txt --valid valid_parsed.txt --test test_parsed.txt --output_dir ./output/RXN
  python rxn_finetune.py --synthetic 16 --tiny --epoch 1 --n_beam 1          (no data files: seeded weights, reactions and vocabulary)

The files hold one reaction per line, `source<TAB>target` (rxn_predict.read_reactions; for --mode retro the source column is the product).
Per epoch, as the script: the training reactions in file order in batches of --batch_size (the last incomplete batch dropped), sources cut
at 150 tokens and products at 100 with the tokenizer's own first token dropped; validation and test by spmm_amd.decode.greedy_products
(--n_beam 1) or predict_products with rxn_predict's exact-match accuracy; the checkpoint is saved when the validation accuracy is >= the best
so far; the schedule steps with epoch + warmup + 1.  The step is SPMMRxn.train_step (spmm_amd/rxn_step.py and the fused arena AdamW).  The
reference's random-SMILES augmentation of the training pairs needs `rdkit`; without it the augmentation is off and the driver says so once.
`rxn_predict.py --checkpoint <output_dir>/checkpoint_best.pth` decodes with the result."""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from pv2smiles import synthetic_vocab                                # noqa: E402
from rxn_predict import MAX_SOURCE, MAX_STEPS, _canonical, accuracy, predict_all, read_reactions, synthetic_reactions      # noqa: E402
from smiles2pv import encode, pad_batch                              # noqa: E402  ('[CLS]' prefix, the tokenizer's own first token dropped)

MAX_PRODUCT = 100         # d_rxn_prediction.py:40 (tokenizer(product, padding='longest', max_length=100))
PRINT_FREQ = 50


# ------------------------------------------------------------------------------------------------------------------- augmentation
def augmenter():
    """The training set's augmentation (dataset.py:259-265: with probability 1/2 both sides of a pair are rewritten as non-canonical SMILES
    of the same molecules, atoms renumbered at random) -- or None without rdkit."""
    try:
        from rdkit import Chem, RDLogger
    except ImportError:
        return None
    RDLogger.DisableLog("rdApp.*")

    def shuffled(s):
        mol = Chem.MolFromSmiles(s)
        if mol is None:
            return s
        order = list(range(mol.GetNumAtoms()))
        random.shuffle(order)
        return Chem.MolToSmiles(Chem.RenumberAtoms(mol, order), canonical=False, isomericSmiles=False)

    def aug(source, target):
        return (shuffled(source), shuffled(target)) if random.random() > 0.5 else (source, target)
    return aug


# ----------------------------------------------------------------------------------------------------------------------- epochs
def train_batches(tokenizer, sources, targets, batch_size: int, aug=None):
    """((src_ids, src_mask), (prod_ids, prod_mask)) host tensors of every full batch, in file order (DataLoader(drop_last=True))."""
    for i in range(0, len(sources) - batch_size + 1, batch_size):
        pairs = list(zip(sources[i:i + batch_size], targets[i:i + batch_size]))
        if aug is not None:
            pairs = [aug(s, t) for s, t in pairs]
        src = pad_batch(encode(tokenizer, [s for s, _ in pairs], MAX_SOURCE), tokenizer.pad_token_id)
        prod = pad_batch(encode(tokenizer, [t for _, t in pairs], MAX_PRODUCT), tokenizer.pad_token_id)
        yield src, prod


def train_epoch(model, tokenizer, sources, targets, batch_size: int, epoch: int, aug=None, max_steps: int = 0):
    """train() of d_rxn_prediction.py:27-52 -> (steps run, running mean of the loss as the script prints it)."""
    model.train()
    running, losses, n = 0.0, [], 0
    for i, batch in enumerate(train_batches(tokenizer, sources, targets, batch_size, aug)):
        if max_steps and model.global_step >= max_steps:
            break
        losses.append(model.training_step(batch, i))               # (device tensors: read back at the print cadence only)
        n += 1
        if n % PRINT_FREQ == 0:
            for l in losses:
                running = running * 0.99 + 0.01 * float(l)
            losses = []
            print(f"Train Epoch: [{epoch}] step {n}: loss={float(l):.4f}, lr={model.optimizers().param_groups[0]['lr']:.6f}", flush=True)
    for l in losses:
        running = running * 0.99 + 0.01 * float(l)
    print("mean loss:", [running])
    return n, running


@torch.no_grad()
def evaluate(model, tokenizer, sources, targets, n_beam: int, batch_size: int, max_steps: int = MAX_STEPS, canon=None):
    """evaluate / evaluate_beam + metric_eval (d_rxn_prediction.py:55-145) on the engine's batched searches -> top-n_beam accuracy."""
    model.eval()
    if not sources:
        return 0.0
    ids = predict_all(model, tokenizer, sources, n_beam, batch_size, max_steps)
    candidates = [[tokenizer.decode(seq) for seq in cands] for cands in ids]
    _, topk = accuracy(targets, candidates, canon)
    print("Accuracy:", topk)
    return topk


# ---------------------------------------------------------------------------------------------------------------------- main
def main(args):
    device = torch.device(args.device)
    from spmm_amd import ops
    if args.dry_run:
        ops._DRY_RUN = True
    if not ops._DRY_RUN and (device.type != "cuda" or not torch.cuda.is_available()):
        raise SystemExit(f"rxn_finetune.py: --device {args.device}: spmm_amd has no CPU / eager fallback -- its layers are HIP kernels for "
                         "gfx950 and need a GPU (the fp32 CPU restatement under tests/ is test infrastructure, not a product path)")
    if not 1 <= args.n_beam <= 8:
        raise SystemExit(f"--n_beam {args.n_beam}: the masked-memory decode kernels serve 1..8 beams")
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    from spmm_amd.rxn import SPMMRxn
    from spmm_amd.tokenizer import SmilesWordPiece

    # d_rxn_prediction.py:271-279
    config = {"batch_size_train": args.batch_size, "batch_size_test": 32,
              "bert_config_text": os.path.join(ROOT, "configs", f"config_bert{'_tiny' if args.tiny else ''}.json"),
              "schedular": {"sched": "cosine", "lr": args.lr, "epochs": args.epoch, "min_lr": args.min_lr, "decay_rate": 1, "warmup_lr": 1e-5,
                            "warmup_epochs": 1, "cooldown_epochs": 0},
              "optimizer": {"opt": "adamW", "lr": args.lr, "weight_decay": 0.02}}
    if os.path.exists(args.vocab_filename):
        tokenizer = SmilesWordPiece(args.vocab_filename)
    elif args.synthetic:
        tokenizer = None
    else:
        raise SystemExit(f"--vocab_filename {args.vocab_filename} not found")
    print("Creating model")
    model = SPMMRxn(config=config, device="cpu" if ops._DRY_RUN else device, trainable=True)
    print("#parameters:", sum(p.numel() for p in model.parameters() if p.requires_grad))
    if tokenizer is None:
        tokenizer = SmilesWordPiece(synthetic_vocab(model.cfg.text.vocab_size))
    model.tokenizer = tokenizer
    print("Creating dataset")
    if args.synthetic:
        src, tgt = synthetic_reactions(tokenizer.itos, args.synthetic, args.seed)
        data = {"train": (src, tgt), "valid": (src[:8], tgt[:8]), "test": (src[-8:], tgt[-8:])}
    else:
        if args.checkpoint:
            res = model.load_pretrained(args.checkpoint)
            print(f"load checkpoint from {args.checkpoint} (missing {len(res.missing_keys)}, unexpected {len(res.unexpected_keys)})")
        data = {k: read_reactions(getattr(args, k)) for k in ("train", "valid", "test")}
        for k, (s, t) in data.items():
            if any(x is None for x in t):
                raise SystemExit(f"--{k}: every line needs a target (source<TAB>target)")
    print(len(data["train"][0]), len(data["valid"][0]), len(data["test"][0]))
    aug = None if args.synthetic else augmenter()
    if aug is None and not args.synthetic:
        print("rdkit is not installed: the random-SMILES augmentation of the training pairs is off")
    canon = _canonical()
    os.makedirs(args.output_dir, exist_ok=True)
    best_valid = best_test = 0.0
    start = time.time()
    for epoch in range(args.epoch):
        print("TRAIN", epoch)
        train_epoch(model, tokenizer, *data["train"], args.batch_size, epoch, aug, args.max_steps)
        print("VALIDATION")
        val = evaluate(model, tokenizer, *data["valid"], args.n_beam, config["batch_size_test"], args.decode_steps, canon)
        print("TEST")
        test = evaluate(model, tokenizer, *data["test"], args.n_beam, config["batch_size_test"], args.decode_steps, canon)
        if val >= best_valid:
            print("SAVING...", test)
            model.save_checkpoint(os.path.join(args.output_dir, "checkpoint_best.pth"), lr_scheduler=dict(model.lr_schedulers().s), mode=args.mode)
            best_valid, best_test = val, test
        model.on_train_epoch_end()                                   # lr_scheduler.step(epoch + warmup_steps + 1)
        if args.max_steps and model.global_step >= args.max_steps:
            break
    print(f"Training time {int(time.time() - start)} s")
    print("test ACC of checkpoint with best val ACC:", best_test)
    return best_test


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Fine-tune the reaction-prediction model (the reference's d_rxn_prediction.py without --evaluate).")
    # the reference's flags (d_rxn_prediction.py:259-268)
    p.add_argument("--output_dir", default="./output/RXN")
    p.add_argument("--checkpoint", default="./Pretrain/checkpoint_SPMM_20m.ckpt")
    p.add_argument("--mode", default="forward", choices=("forward", "retro"))
    p.add_argument("--n_beam", default=5, type=int, help="beams of the validation / test search; 1 runs the greedy search")
    p.add_argument("--device", default="cuda")
    p.add_argument("--lr", default=1e-4, type=float)
    p.add_argument("--min_lr", default=5e-6, type=float)
    p.add_argument("--epoch", default=300, type=int)
    p.add_argument("--batch_size", default=16, type=int)
    # additions
    p.add_argument("--train", default="./data/6_RXNprediction/USPTO-480k/train_parsed.txt", help="one reaction per line: source<TAB>target")
    p.add_argument("--valid", default="./data/6_RXNprediction/USPTO-480k/valid_parsed.txt")
    p.add_argument("--test", default="./data/6_RXNprediction/USPTO-480k/test_parsed.txt")
    p.add_argument("--vocab_filename", default="./vocab_bpe_300.txt")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--max_steps", default=0, type=int, help="stop after this many training steps (0: no limit)")
    p.add_argument("--decode_steps", default=MAX_STEPS, type=int, help="positions decoded at most in validation / test (the reference's 100)")
    p.add_argument("--synthetic", default=0, type=int, metavar="N", help="no data files: N seeded reactions, seeded weights and vocabulary")
    p.add_argument("--tiny", action="store_true", help="2-layer / 128-d decoder (configs/config_bert_tiny.json)")
    p.add_argument("--dry_run", action="store_true", help="validate every kernel call against the C header without launching (no GPU needed)")
    return p.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
