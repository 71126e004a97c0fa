"""Library clustering driver: organise an encoded library.  The reference has no such script; the model and the library are given as
retrieve.py takes them:

  python cluster.py --checkpoint ./Pretrain/checkpoint_SPMM.ckpt --vocab_filename ./vocab_bpe_300.txt --library library.txt --k 1000 \
                    --output clusters.csv --medoids medoids.txt
  python cluster.py ... --library library.txt --save_index library.idx     (encode the library once ...)
  python cluster.py --index library.idx --pick 500 --output picks.csv      (... and organise it many times; no model is needed then)
  python cluster.py --synthetic 300 --tiny --k 5                           (no data files: seeded weights, library, vocabulary)
  python cluster.py --index library.idx --threshold 0.8 --output clusters.csv --medoids leaders.txt      (Butina: the threshold gives K)
  python cluster.py --index library.idx --dedup 0.98 --output unique.csv                                   (drop near-duplicates)

--k K clusters the library by spherical k-means on the text features (spmm_amd.cluster.kmeans): the CSV has one row per molecule --
library line (1-based), SMILES, cluster, cosine to the cluster's centre, whether it is the cluster's medoid; --medoids FILE lists one
representative per cluster.  --pick N picks N molecules as unlike each other as possible (MaxMin picking, spmm_amd.cluster.pick_diverse):
the CSV has one row per pick in picking order with its largest cosine to the earlier picks.  --threshold T clusters by leaders instead
(spmm_amd.cluster.leaders: Taylor-Butina with --order count, first-come leaders with --order row): every molecule within T of its cluster's
leader, no two leaders within T of each other; the same CSV with the leader in the medoid's place and a column n_neighbours.  --dedup T
writes the molecules that are not within T of an earlier kept one."""
import argparse
import csv
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from pv2smiles import synthetic_vocab                                       # noqa: E402
from smiles2pv import add_tokenizer_flags, read_smiles, synthetic_smiles    # noqa: E402  (the library as smiles2pv.py reads its input)

MAX_K = 65536


def cluster_rows(assign, best, medoid, smiles):
    """A clustering -> [(library line, SMILES, cluster, cosine to its centre, 1 if the cluster's medoid else 0)], one per molecule."""
    med = set(m for m in medoid.tolist() if m >= 0)
    return [(i + 1, smiles[i] if smiles is not None else "", int(a), repr(float(b)), int(i in med))
            for i, (a, b) in enumerate(zip(assign.tolist(), best.tolist()))]


def pick_rows(rows, similarity, smiles):
    """Picks in order -> [(pick order, library line, SMILES, largest cosine to the earlier picks; empty for the first)]."""
    return [(j + 1, r + 1, smiles[r] if smiles is not None else "", "" if s == float("-inf") else repr(float(s)))
            for j, (r, s) in enumerate(zip(rows.tolist(), similarity.tolist()))]


def medoid_rows(counts, medoid, smiles):
    """[(cluster, size, library line of its medoid or '', SMILES)], one per cluster."""
    return [(c, int(n), "" if m < 0 else m + 1, "" if m < 0 or smiles is None else smiles[m])
            for c, (n, m) in enumerate(zip(counts.tolist(), medoid.tolist()))]


def leader_rows(cluster, cosine, leader, n_neighbours, smiles):
    """A leader clustering -> cluster_rows' columns (the cosine is to the leader, is_medoid marks the leader) and the neighbour count."""
    return [(i + 1, smiles[i] if smiles is not None else "", int(c), repr(float(b)), int(l == i), int(d))
            for i, (c, b, l, d) in enumerate(zip(cluster.tolist(), cosine.tolist(), leader.tolist(), n_neighbours.tolist()))]


def dedup_rows(leader, smiles):
    """-> (kept [(library line, SMILES)], dropped [(library line, the line it was folded into)])."""
    kept, dropped = [], []
    for i, l in enumerate(leader.tolist()):
        if l == i:
            kept.append((i + 1, smiles[i] if smiles is not None else ""))
        else:
            dropped.append((i + 1, l + 1))
    return kept, dropped


def write_csv(path: str, header, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        w.writerows(rows)


CLUSTER_HEADER = ["library_line", "smiles", "cluster", "cosine_to_centre", "is_medoid"]
PICK_HEADER = ["pick_order", "library_line", "smiles", "max_cosine_to_earlier_picks"]
MEDOID_HEADER = ["cluster", "size", "library_line", "smiles"]
LEADER_HEADER = CLUSTER_HEADER + ["n_neighbours"]
DEDUP_HEADER = ["library_line", "smiles"]


def check_size(args, N: int):
    """--k / --pick against the library's size."""
    if args.k and not 1 <= args.k <= N:
        raise SystemExit(f"--k {args.k} outside [1, {N}] (the library has {N} molecules)")
    if args.pick and not 1 <= args.pick <= N:
        raise SystemExit(f"--pick {args.pick} outside [1, {N}] (the library has {N} molecules)")


def check_args(args):
    """What can be refused before a model is built -> the library's SMILES when they are read here (None for --index)."""
    by_threshold, by_dedup = args.threshold is not None, args.dedup is not None
    if by_threshold and args.k:
        raise SystemExit("--threshold and --k are alternatives: the threshold decides the number of clusters")
    if (by_threshold or by_dedup) and (args.k or args.pick or (by_threshold and by_dedup)):
        raise SystemExit("--k, --pick, --threshold and --dedup are alternatives")
    for name, t in (("--threshold", args.threshold), ("--dedup", args.dedup)):
        if t is not None and not -1.0 <= t <= 1.0:
            raise SystemExit(f"{name} {t} is not a cosine in [-1, 1]")
    if args.max_pairs < 0:
        raise SystemExit("--max_pairs must be at least 0")
    if args.k and args.pick:
        raise SystemExit("--k and --pick are alternatives: cluster the library, or pick a diverse subset of it")
    if not args.k and not args.pick and not by_threshold and not by_dedup:
        raise SystemExit("give --k K (cluster the library) or --pick N (pick a diverse subset)")
    if args.k < 0 or args.k > MAX_K:
        raise SystemExit(f"--k {args.k} outside [1, {MAX_K}]")
    if args.pick < 0:
        raise SystemExit(f"--pick {args.pick} must be at least 1")
    if args.iters < 1:
        raise SystemExit("--iters must be at least 1")
    if args.medoids and not (args.k or by_threshold):
        raise SystemExit("--medoids goes with --k or --threshold")
    if not args.synthetic and not (args.library or args.index):
        raise SystemExit("give the library: --library FILE (one SMILES per line) or --index FILE (saved by --save_index)")
    if args.library and args.index:
        raise SystemExit("--library and --index are alternatives")
    if args.synthetic:
        check_size(args, args.synthetic)
        return None
    if args.library:
        library = read_smiles(args.library)
        check_size(args, len(library))
        return library
    return None


def size_summary(counts):
    s = sorted(counts.tolist())
    return s[0], s[len(s) // 2], s[-1]


def main_leaders(args, index, C):
    """--threshold / --dedup on an encoded library."""
    dedup = args.dedup is not None
    try:
        res = C.leaders(index, args.dedup if dedup else args.threshold, order="row" if dedup else args.order, max_pairs=args.max_pairs)
    except ValueError as e:
        raise SystemExit(f"cluster.py: {e}")
    N = len(index)
    degree = res.n_neighbours.cpu()
    print(f"{res.pairs // 2} pairs at or above {res.threshold!r}: mean degree {res.pairs / max(N, 1):.2f}, max degree "
          f"{int(degree.max()) if N else 0}; {res.rounds} rounds")
    if dedup:
        kept, dropped = dedup_rows(res.leader.cpu(), index.smiles)
        write_csv(args.output, DEDUP_HEADER, kept)
        for line, into in dropped:
            print("line %-8d dropped: a duplicate of line %d" % (line, into))
        print(f"{len(dropped)} of {N} lines dropped; {len(kept)} molecules are saved in '{args.output}'")
        return kept
    counts, lead = res.counts.cpu(), res.leaders.cpu()
    print(f"{counts.numel()} clusters (order {res.order}), {int((counts == 1).sum())} singletons")
    if counts.numel():
        print("cluster sizes: min %d, median %d, max %d" % size_summary(counts))
    meds = medoid_rows(counts, lead, index.smiles)
    for c, n, line, smi in sorted(meds, key=lambda r: (-r[1], r[0]))[:10]:
        print("cluster %-6d size %-8d leader line %-8s %s" % (c, n, line, smi))
    out = leader_rows(res.cluster.cpu(), res.cosine_to_leader.cpu(), res.leader.cpu(), degree, index.smiles)
    write_csv(args.output, LEADER_HEADER, out)
    print(f"{len(out)} molecules are saved in '{args.output}'")
    if args.medoids:
        write_csv(args.medoids, MEDOID_HEADER, meds)
        print(f"{len(meds)} clusters are saved in '{args.medoids}'")
    return out


def main(args):
    library = check_args(args)
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"cluster.py: --device {args.device}: spmm_amd has no CPU / eager fallback -- its layers are HIP kernels for gfx950 "
                         "and need a GPU")
    torch.manual_seed(args.seed)
    from spmm_amd import cluster as C
    from spmm_amd import retrieve as R

    if args.index:
        index = R.MoleculeIndex.load(args.index, device=device)
        print(f"Loaded {len(index)} molecules from '{args.index}'")
        check_size(args, len(index))
    else:
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
        if args.synthetic:
            library = synthetic_smiles(tokenizer.itos, args.synthetic, args.seed)
        elif args.checkpoint:
            print("LOADING PRETRAINED MODEL..")
            res = model.load_checkpoint(args.checkpoint, weights_only=True)
            print(f"load checkpoint from {args.checkpoint} (missing {len(res.missing_keys)}, unexpected {len(res.unexpected_keys)})")
        model.eval()
        print(f"Encoding {len(library)} molecules...")
        from spmm_amd.wordpiece_device import device_tokenizer_for
        index = R.MoleculeIndex.build(model, tokenizer, library, batch_size=args.batch_size,
                                      tokenizer_device=device_tokenizer_for(tokenizer, device, args.host_tokenizer))
    if args.save_index:
        index.save(args.save_index)
        print(f"Index saved in '{args.save_index}'")
    print("=" * 50)
    if args.threshold is not None or args.dedup is not None:
        out = main_leaders(args, index, C)
    elif args.pick:
        rows, sim = C.pick_diverse(index, args.pick, seed=args.seed)
        out = pick_rows(rows.cpu(), sim.cpu(), index.smiles)
        write_csv(args.output, PICK_HEADER, out)
        for r in out[:10]:
            print("%4d  line %-8d max cosine to earlier picks %s  %s" % (r[0], r[1], r[3][:9] or "-", r[2]))
        print(f"{len(out)} picks are saved in '{args.output}'")
    else:
        res = C.kmeans(index, args.k, iters=args.iters, init=args.init, seed=args.seed)
        for it, obj in enumerate(res.objective):
            print(f"iteration {it + 1:3d}  objective {obj:.6f}  (mean cosine to centre {obj / len(index):.6f})")
        print(f"{res.iterations} iterations ({'converged' if res.changed == 0 else f'{res.changed} rows still moving'}), "
              f"{res.reseeded} clusters re-seeded")
        counts, medoid = res.counts.cpu(), res.medoid.cpu()
        print("cluster sizes: min %d, median %d, max %d" % size_summary(counts))
        meds = medoid_rows(counts, medoid, index.smiles)
        for c, n, line, smi in sorted(meds, key=lambda r: (-r[1], r[0]))[:10]:
            print("cluster %-6d size %-8d medoid line %-8s %s" % (c, n, line, smi))
        out = cluster_rows(res.assign.cpu(), res.best.cpu(), medoid, index.smiles)
        write_csv(args.output, CLUSTER_HEADER, out)
        print(f"{len(out)} molecules are saved in '{args.output}'")
        if args.medoids:
            write_csv(args.medoids, MEDOID_HEADER, meds)
            print(f"{len(meds)} clusters are saved in '{args.medoids}'")
    print("=" * 50)
    return out


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Cluster an encoded library, or pick a diverse subset of it.")
    p.add_argument("--checkpoint", default="./Pretrain/checkpoint_SPMM.ckpt")
    p.add_argument("--vocab_filename", default="./vocab_bpe_300.txt")
    p.add_argument("--device", default="cuda")
    # the library
    p.add_argument("--library", default="", help="one SMILES per line")
    p.add_argument("--index", default="", help="a library saved by --save_index")
    p.add_argument("--save_index", default="", help="write the encoded library here")
    p.add_argument("--batch_size", default=256, type=int, help="molecules encoded together when the index is built")
    # what to do with it
    p.add_argument("--k", default=0, type=int, help="cluster the library into K clusters (spherical k-means)")
    p.add_argument("--iters", default=20, type=int, help="k-means iterations at the most")
    p.add_argument("--init", default="farthest", choices=("farthest", "random"), help="initial centres: farthest-first traversal, or random rows")
    p.add_argument("--pick", default=0, type=int, metavar="N", help="pick N molecules as unlike each other as possible instead of clustering")
    p.add_argument("--threshold", default=None, type=float, metavar="T",
                   help="cluster by leaders instead: every molecule within cosine T of its cluster's leader (the number of clusters is a result)")
    p.add_argument("--order", default="count", choices=("count", "row"),
                   help="with --threshold: 'count' = Taylor-Butina (the most neighbours lead first, ties to the lower line), 'row' = first come")
    p.add_argument("--dedup", default=None, type=float, metavar="T",
                   help="write the molecules that are not within cosine T of an earlier kept one (library_line, smiles)")
    p.add_argument("--max_pairs", default=1 << 30, type=int, help="refuse a neighbour list with more entries than this (4 bytes each)")
    p.add_argument("--output", default="clustered_molecules.csv",
                   help="CSV: library line, SMILES, cluster, cosine to its centre, is_medoid (--pick: pick order, library line, SMILES, "
                        "largest cosine to the earlier picks)")
    p.add_argument("--medoids", default="", help="with --k: one line per cluster -- cluster, size, library line and SMILES of its medoid "
                                                 "(with --threshold: of its leader)")
    p.add_argument("--seed", default=0, type=int, help="seed of the first pick / the random centres, and of --synthetic's weights and library")
    p.add_argument("--synthetic", default=0, type=int, metavar="N", help="no data files: seeded weights and N made-up molecules")
    p.add_argument("--tiny", action="store_true", help="2-layer / 128-d encoders (configs/config_bert_tiny.json)")
    add_tokenizer_flags(p)
    return p.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
