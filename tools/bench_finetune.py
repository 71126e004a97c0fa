"""Times eager fine-tuning steps at the published width (H = 768, 6 text layers, the classifier head of d_classification.py) on one GPU:
the HIP step (spmm_amd.finetune: forward, backward and the fused AdamW, padding rows packed away) against an eager PyTorch model of
the same shape (torch.nn modules, bf16 autocast, torch.optim.AdamW, padded batches as the reference runs them), alternating the two
in one process.  Lengths ~ U[50, 100].  Per step: device time from events around `--steps` steps, host enqueue time (the host clock
around the same calls, which return before the GPU finishes -- `hip_step_host_syncs` checks that no call in the step waits for the GPU),
and the GPU's own time with the host out of the way (`gpu_busy`: the steps queued behind a spin kernel, then run back to back).  When
device time tracks enqueue time and the GPU-busy time is smaller, the step is host-bound: the gap is what graph capture could remove.
Prints ONE JSON line.

  python tools/bench_finetune.py [--steps 30] [--warmup 10] [--rounds 3] [--batches 16 64]"""
import argparse
import json
import os
import sys
import time

import torch
from torch import nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class EagerClassifier(nn.Module):
    """BertForMaskedLM's text layers 0..5 + reg_head as torch.nn modules: post-LN encoder layers (BERT's order), erf-GELU."""

    def __init__(self, V=300, H=768, nH=12, I=3072, layers=6, C=2, p=0.1):
        super().__init__()
        self.word, self.pos, self.tok_type = nn.Embedding(V, H, padding_idx=0), nn.Embedding(512, H), nn.Embedding(2, H)
        self.ln, self.drop = nn.LayerNorm(H, eps=1e-12), nn.Dropout(p)
        self.layers = nn.ModuleList([nn.TransformerEncoderLayer(H, nH, I, p, activation="gelu", batch_first=True, norm_first=False,
                                                                layer_norm_eps=1e-12) for _ in range(layers)])
        self.head = nn.Sequential(nn.Linear(H, H), nn.GELU(), nn.Linear(H, C))

    def forward(self, ids, mask, y):
        L = ids.shape[1]
        x = self.drop(self.ln(self.word(ids) + self.pos.weight[:L] + self.tok_type.weight[0]))
        pad = mask == 0
        for layer in self.layers:
            x = layer(x, src_key_padding_mask=pad)
        return F.cross_entropy(self.head(x[:, 0]).float(), y)


def make_batches(n, B, seed, V=300):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        lens = torch.randint(50, 101, (B,), generator=g)
        L = int(lens.max())
        ids = torch.zeros(B, L, dtype=torch.long)
        for i in range(B):
            ids[i, 0] = 2
            ids[i, 1:int(lens[i]) - 1] = torch.randint(4, V, (int(lens[i]) - 2,), generator=g)
            ids[i, int(lens[i]) - 1] = 3
        mask = (ids != 0).long()
        out.append((ids.cuda(), mask, mask.cuda(), torch.randint(0, 2, (B,), generator=g).cuda(), int(mask.sum())))
    return out


def timed(step, batches, warmup, steps):
    """-> (device ms per step, host enqueue ms per step)."""
    for b in batches[:warmup]:
        step(b)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    host = 0.0
    e0.record()
    for b in batches[warmup:warmup + steps]:
        t = time.perf_counter()
        step(b)
        host += time.perf_counter() - t
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps, 1e3 * host / steps


def gpu_busy(step, batches, n):
    """GPU time per step with the host out of the way: the n steps are enqueued while the stream is held by a spin kernel
    (torch.cuda._sleep), so the GPU then runs them back to back.  -> (ms per step, whether the hold outlasted the enqueue).  When it did
    not, host gaps entered the window and the figure is an upper bound of the GPU's own time per step."""
    torch.cuda.synchronize()
    cal0, cal1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cal0.record()
    torch.cuda._sleep(10_000_000)
    cal1.record()
    cal1.synchronize()
    t = time.perf_counter()
    for b in batches[:2]:                       # host cost of a step, to size the hold
        step(b)
    host_ms = 1e3 * (time.perf_counter() - t) / 2
    torch.cuda.synchronize()
    hold_ms = 3.0 * host_ms * n + 20.0
    cycles = int(10_000_000 * hold_ms / cal0.elapsed_time(cal1))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(cycles)
    e0.record()
    t = time.perf_counter()
    for b in batches[:n]:
        step(b)
    enq_ms = 1e3 * (time.perf_counter() - t)
    e1.record()
    covered = not e0.query()                    # the hold still running after the last enqueue: no host gap entered the window
    e1.synchronize()
    return e0.elapsed_time(e1) / n, covered


def host_syncs(step, b):
    """Whether one step makes a synchronising tensor-library call (torch's sync debug mode; the package's own launches never wait)."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step(b)
        return "none"
    except RuntimeError as e:
        return str(e).splitlines()[0][:160]
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune.py needs a GPU")
    from spmm_amd.config import BertConfig
    from spmm_amd.finetune import SPMMClassifier
    torch.manual_seed(0)
    cfg = BertConfig.from_json_file(os.path.join(ROOT, "configs", "config_bert.json"))
    sched = {"sched": "cosine", "lr": 5e-5, "epochs": 15, "min_lr": 5e-6, "decay_rate": 1, "warmup_lr": 0.5e-5, "warmup_epochs": 1,
             "cooldown_epochs": 0}
    hip = SPMMClassifier(bert_config=cfg, config={"optimizer": {"lr": 5e-5, "weight_decay": 0.02}, "schedular": sched}).train()
    eager = EagerClassifier().cuda().train()
    opt = torch.optim.AdamW(eager.parameters(), lr=5e-5, weight_decay=0.02)

    def hip_step(b):
        ids, _, mask_d, y, n_tok = b                 # (device mask + the host's token count: nothing in the step waits for the GPU)
        hip.train_step(ids, mask_d, y, n_tokens=n_tok)

    def eager_step(b):
        ids, _, mask_d, y, _ = b
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = eager(ids, mask_d, y)
        loss.backward()
        opt.step()

    results = []
    for B in a.batches:
        batches = make_batches(a.warmup + a.steps, B, seed=B)
        tok = sum(b[4] for b in batches) / len(batches)
        rows = {"hip": [], "eager": []}
        for _ in range(a.rounds):                        # alternating, so that neither side always runs on the warmer clocks
            rows["hip"].append(timed(hip_step, batches, a.warmup, a.steps))
            rows["eager"].append(timed(eager_step, batches, a.warmup, a.steps))
        med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
        busy_hip, cov_hip = gpu_busy(hip_step, batches, 6)
        busy_eager, cov_eager = gpu_busy(eager_step, batches, 6)
        results.append({"B": B, "mean_tokens": round(tok, 1), "mean_padded_tokens": round(sum(b[0].numel() for b in batches) / len(batches), 1),
                        "hip_device_ms": round(med["hip"][0], 3), "hip_enqueue_ms": round(med["hip"][1], 3),
                        "eager_device_ms": round(med["eager"][0], 3), "eager_enqueue_ms": round(med["eager"][1], 3),
                        "eager_over_hip": round(med["eager"][0] / med["hip"][0], 3),
                        "hip_gpu_busy_ms": round(busy_hip, 3), "eager_gpu_busy_ms": round(busy_eager, 3),
                        "gpu_busy_window_covered": bool(cov_hip and cov_eager), "hip_step_host_syncs": host_syncs(hip_step, batches[0]),
                        "hip_device_ms_all": [round(r[0], 3) for r in rows["hip"]], "eager_device_ms_all": [round(r[0], 3) for r in rows["eager"]]})
    print(json.dumps({"tool": "bench_finetune", "H": 768, "layers": cfg.fusion_layer, "task": "classification", "steps": a.steps,
                      "warmup": a.warmup, "rounds": a.rounds, "lengths": "U[50,100]", "results": results,
                      "graph_captured_step": "not measured", "device": torch.cuda.get_device_name()}))


if __name__ == "__main__":
    main()
