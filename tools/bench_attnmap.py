"""Cross-attention maps on one MI355X at the published size (H = 768, 12 heads, 6 fusion layers), seeded random weights: `--molecules`
molecules of 30 .. 100 tokens x their PVs, last fusion layer, both directions, head mean, in batches of `--batch_size`; alternating A/B
windows in one process, `--pairs` rounds, medians (spread = (max - min) / median beside them).

  (a) the kernel: ops.attn_probs (spmm_attn_probs, csrc/attnmap.hip) against the eager composite on the SAME tapped Q / K of one batch:
      einsum -> mask -> softmax -> mean(heads) in fp32 torch on Q / K already gathered into padded [P, L, nH, 64] tensors (the gather is
      NOT timed: the composite starts from the layout it likes best); the peak device memory each needs on top of its inputs;
  (b) the path: attribution.cross_attention_maps against the dense module route -- what a user had to write before: the padded batch,
      every molecule encoded once per pair (`text_encoder.bert(mode='text')`), the two fusion passes as the facade runs them (dense
      groups, a private key/value source per pair), and the eager composite on the last layer's Q / K.

What this does NOT measure: a trained checkpoint (random weights give near-uniform maps; the arithmetic does not depend on the values),
reactions at the published size, heads='all'.  Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from spmm_amd import attribution as AT, decode, ops
from spmm_amd.config import BertConfig, SPMMConfig
from spmm_amd.engine import BF, Batch, Group
from spmm_amd.model import SPMM

ap = argparse.ArgumentParser()
ap.add_argument("--molecules", type=int, default=4096)
ap.add_argument("--batch_size", type=int, default=512)
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--reps", type=int, default=10, help="kernel / composite launches per timed window")
ap.add_argument("--tiny", type=int, default=0, help="1: the 2-layer / 128-d configuration (a rehearsal of the tool, not a measurement)")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_attnmap.py measures on the GPU: no device found (spmm_amd has no CPU / eager fallback)")
dev = torch.device("cuda")
torch.manual_seed(0)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def ab(fa, fb, reps):
    window(fa, 1), window(fb, 1)
    ta, tb = [], []
    for _ in range(a.pairs):
        t, oa = window(fa, reps)
        ta.append(t)
        t, ob = window(fb, reps)
        tb.append(t)
    ma, mb = statistics.median(ta), statistics.median(tb)
    return ma, mb, (max(ta) - min(ta)) / ma, (max(tb) - min(tb)) / mb, oa, ob


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


if a.tiny:
    from spmm_amd.config import tiny_config
    cfg = tiny_config()
else:
    cfg = SPMMConfig(text=BertConfig(num_hidden_layers=12, fusion_layer=6, add_cross_attention=True),
                     prop=BertConfig(num_hidden_layers=6, fusion_layer=6, vocab_size=1), embed_dim=256, queue_size=36864)
m = SPMM(spmm_config=cfg, no_train=True).eval()
m.store.refresh_shadows()
eng, ct = m.engine, cfg.text
H, nH, Lp, f, n = ct.hidden_size, ct.num_attention_heads, cfg.n_props + 1, ct.fusion_layer, ct.num_hidden_layers
gh = torch.Generator().manual_seed(2)
N = a.molecules
lens = torch.randint(30, 101, (N,), generator=gh)
ids = torch.zeros(N, 100, dtype=torch.long)
for b, ln in enumerate(lens.tolist()):
    ids[b, 0] = 2
    ids[b, 1:ln - 1] = torch.randint(4, ct.vocab_size, (ln - 2,), generator=gh)
    ids[b, ln - 1] = 3
mask = (ids != 0).long()
pv = torch.randn(N, cfg.n_props, generator=gh)
batches = [slice(i, min(i + a.batch_size, N)) for i in range(0, N, a.batch_size)]
res = {"device": torch.cuda.get_device_name(0), "molecules": N, "tokens": "30..100", "batch_size": a.batch_size, "pairs": a.pairs, "tiny": a.tiny,
       "H": H, "heads": nH, "fusion_layers": n - f}


def composite(Qp, Kp, km):
    """Qp [P, Lq, nH, 64], Kp [P, Lkv, nH, 64] bf16, km bool [P, Lkv] -> head-mean probabilities [P, Lq, Lkv] (forms [P, nH, Lq, Lkv])."""
    s = torch.einsum("pqhd,pkhd->phqk", Qp.float(), Kp.float()) / 8.0
    s = s.masked_fill(~km[:, None, None, :], float("-inf"))
    return torch.softmax(s, dim=-1).mean(1)


# ---------------------------------------------------------------------------------------------------------------- (a) the kernel
taps = []


def hook(t):
    t.keep_qk = True
    taps.append(t)


b0 = batches[0]
AT.cross_attention_maps(m, pv[b0], None, ids[b0], mask[b0], layers=(-1,), _tap_hook=hook)
tap = taps[0]
res["kernel"] = {}
for d, gi in (("pv2text", 0), ("text2pv", 1)):
    g, Q, K = tap.qk[(n - f - 1, gi)]
    src, P = g.src, g.nseq
    q0 = g.q_row0.tolist() if g.q_row0 is not None else [s * g.L for s in range(P)]
    ql = g.q_len.tolist() if g.q_len is not None else [g.L] * P
    kv = g.kv_idx.tolist()
    k0 = src.row0.tolist() if src.row0 is not None else [u * src.Lkv for u in range(src.U)]
    kl = src.len.tolist() if src.len is not None else [src.Lkv] * src.U
    Qp, Kp = torch.zeros(P, g.L, nH, 64, dtype=BF, device=dev), torch.zeros(P, g.Lkv, nH, 64, dtype=BF, device=dev)
    km = torch.zeros(P, g.Lkv, dtype=torch.bool, device=dev)
    for s in range(P):
        u = kv[s]
        Qp[s, :ql[s]] = Q[q0[s]:q0[s] + ql[s]].view(ql[s], nH, 64)
        Kp[s, :kl[u]] = K[k0[u]:k0[u] + kl[u]].view(kl[u], nH, 64)
        km[s, :kl[u]] = True
    kern = lambda: ops.attn_probs(Q, K, nseq=P, nH=nH, Lq=g.L, Lkv=g.Lkv, **g.cross_layout())[0]                 # noqa: E731
    comp = lambda: composite(Qp, Kp, km)                                                                              # noqa: E731
    ma, mb, sa, sb, pk, pc = ab(kern, comp, a.reps)
    dmax = max((pk[q0[s]:q0[s] + ql[s], :kl[kv[s]]] - pc[s, :ql[s], :kl[kv[s]]]).abs().max().item() for s in range(0, P, max(1, P // 16)))
    rows = sum(ql)
    res["kernel"][d] = {"sequences": P, "Lq": g.L, "Lkv": g.Lkv, "query_rows": rows, "kernel_ms": round(ma, 4), "composite_ms": round(mb, 4),
                        "speedup": round(mb / ma, 3), "spread_kernel": round(sa, 4), "spread_composite": round(sb, 4),
                        "kernel_GBps_of_bytes_written": round(rows * g.Lkv * 4 / (ma * 1e-3) / 1e9, 1), "max_abs_diff_sampled": dmax,
                        "peak_extra_bytes_kernel": peak_extra(kern), "peak_extra_bytes_composite": peak_extra(comp)}
    del Qp, Kp, km
del tap, taps[:]
torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- (b) the path
def engine_route():
    out = None
    for b in batches:
        out = AT.cross_attention_maps(m, pv[b], None, ids[b], mask[b], layers=(-1,), heads="mean", direction="both")
    return out


def dense_route():
    """The padded batch, every molecule encoded per pair, the fusion passes as facade.BertFacade runs them, the eager composite last."""
    out = None
    for b in batches:
        L = int(mask[b].sum(1).max())
        idb, mkb = ids[b, :L].to(dev), mask[b, :L].to(dev)
        P = idb.shape[0]
        text = m.text_encoder.bert(idb, attention_mask=mkb, return_dict=True, mode="text").last_hidden_state
        pe = decode.encode_properties(m, pv[b].to(dev))
        eng.train_mode = False
        tx, px = text.to(BF).reshape(P * L, H).contiguous(), pe.to(BF).reshape(P * Lp, H).contiguous()
        mk32, ones = mkb.to(torch.int32).contiguous(), torch.ones(P, Lp, dtype=torch.int32, device=dev)
        got = {}

        def keep(name, Lq, Lkv, km, layer, gi, g, Q, K):
            if layer == n - 1:
                got[name] = composite(Q.reshape(P, Lq, nH, 64), K.reshape(P, Lkv, nH, 64), km != 0)
        import functools
        eng.stack_fwd("text_encoder.bert.", ct, range(f, n), True, px, Batch([Group(0, P, Lp, ones, P, kv=tx, Lkv=L, kv_mask=mk32)]), False,
                      xattn_tap=functools.partial(keep, "pv2text", Lp, L, mk32))
        eng.stack_fwd("text_encoder.bert.", ct, range(f, n), True, tx, Batch([Group(0, P, L, mk32, P, kv=px, Lkv=Lp, kv_mask=ones)]), False,
                      xattn_tap=functools.partial(keep, "text2pv", L, Lp, ones))
        out = got
    return out


ma, mb, sa, sb, em, dm = ab(engine_route, dense_route, 1)
last = batches[-1]
nb = last.stop - last.start
d_pt = max((em.get(p, n - f - 1, "pv2text") - dm["pv2text"][p, :, :int(lens[last][p])]).abs().max().item() for p in range(0, nb, max(1, nb // 16)))
res["path"] = {"engine_ms": round(ma, 2), "dense_ms": round(mb, 2), "speedup": round(mb / ma, 3), "spread_engine": round(sa, 4),
               "spread_dense": round(sb, 4), "molecules_per_s_engine": round(N / ma * 1e3, 1), "molecules_per_s_dense": round(N / mb * 1e3, 1),
               "max_abs_diff_pv2text_sampled": d_pt}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write(json.dumps(res, indent=1) + "\n")
