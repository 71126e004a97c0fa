"""Helpers shared by the GPU test modules."""
import math

import numpy as np


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _tiny_train_model(env, dropout=True):
    O, SPMM, tiny_config, *_ = env
    cfg = tiny_config()
    if not dropout:
        for c in (cfg.text, cfg.prop):
            c.hidden_dropout_prob = c.attention_probs_dropout_prob = 0.0
    sched = {'sched': 'cosine', 'lr': 1e-3, 'epochs': 4, 'min_lr': 1e-5, 'decay_rate': 1, 'warmup_lr': 1e-4,
             'warmup_epochs': 2, 'cooldown_epochs': 0}
    tc = {'embed_dim': 64, 'temp': 0.07, 'queue_size': 16, 'momentum': 0.995, 'alpha': 0.4, 'schedular': sched,
          'optimizer': {'opt': 'adamW', 'lr': 1e-3, 'weight_decay': 0.02}}
    m = SPMM(config=tc, spmm_config=cfg, loader_len=10)
    m.load_state_dict(O.closed_form_state_dict(O.tiny_cfg()))
    return m.train()


# ---------------------------------------------------------------------------------------------------------------------
# Host model of csrc/common.h's counter-based generator: the ONE model of it in the tests.
# ---------------------------------------------------------------------------------------------------------------------
_M64, _M32 = (1 << 64) - 1, np.uint64(0xffffffff)


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _host_seed_mix(seed, salt):
    """seed_mix: two splitmix64 rounds over the per-step seed and the per-call-site salt."""
    return _splitmix64((_splitmix64(seed & _M64) + salt) & _M64)


def _mix32(x):                                      # "lowbias32" on uint64 arrays holding 32-bit values
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x21f0aaad)) & _M32
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x735a2d97)) & _M32
    return x ^ (x >> np.uint64(15))


def _host_dropout_keep(seed, salt, rows, ncols, p):
    """Host model of csrc/common.h's dropout counter hash: keep[row, col] for `rows` (uint64 row counters) x ncols elements.
    seed_mix (two splitmix64 rounds over seed and salt) -> drop_rowkey (lowbias32 of the row) -> drop_pair (Weyl step + two 24-bit
    multiply rounds) -> one 16-bit half per element against round(p * 65536).  The statistics of THIS function were checked against
    lowbias32 when it was adopted (EXPERIMENTS.md 1.7); test_kernels_gpu.py::test_dropout_masks_equal_the_host_model_of_the_hash pins
    the kernels to it bit for bit."""
    def mix24(x):
        x = x ^ (x >> np.uint64(16)); x = ((x & np.uint64(0xffffff)) * np.uint64(0xda8f81)) & _M32
        x = x ^ (x >> np.uint64(16)); x = ((x & np.uint64(0xffffff)) * np.uint64(0x76dfb5)) & _M32
        return x ^ (x >> np.uint64(16))

    s64 = _host_seed_mix(seed, salt)
    s_lo, s_hi = np.uint64(s64 & 0xffffffff), np.uint64(s64 >> 32)
    rows = np.asarray(rows, dtype=np.uint64)
    rowkey = _mix32((rows & _M32) ^ s_lo) ^ s_hi ^ (((rows >> np.uint64(32)) * np.uint64(0x9E3779B1)) & _M32)
    pair = np.arange(ncols // 2, dtype=np.uint64)
    r = mix24((rowkey[:, None] + pair[None, :] * np.uint64(0x9E3779B1)) & _M32)
    u = np.stack([r & np.uint64(0xffff), r >> np.uint64(16)], axis=2).reshape(len(rows), ncols)
    return u >= np.uint64(int(p * 65536 + 0.5))


def _host_rng_uniform(seed, salt, idx):
    """Host model of rng_uniform(seed_mix(seed, salt), idx) = (rng_pair(...) >> 8) / 2^24, exact in float64, for an array of indices.
    rng_pair = lowbias32((idx_lo ^ seed_lo) + (idx_hi ^ seed_hi) * 0x9E3779B1)."""
    s64 = _host_seed_mix(seed, salt)
    s_lo, s_hi = np.uint64(s64 & 0xffffffff), np.uint64(s64 >> 32)
    idx = np.asarray(idx, dtype=np.uint64)
    lo, hi = idx & _M32, idx >> np.uint64(32)
    r = _mix32(((lo ^ s_lo) + (((hi ^ s_hi) * np.uint64(0x9E3779B1)) & _M32)) & _M32)
    return (r >> np.uint64(8)).astype(np.float64) / 16777216.0


# ---------------------------------------------------------------------------------------------------------------------
# Tolerances of the per-kernel tests that compare with a float64 reference (test_loss_kernels_gpu.py,
# test_optim_and_small_kernels_gpu.py).  The bound is derived from the reference alone:
#   E32   = largest error of the SAME formula evaluated in fp32 torch on the CPU against its float64 evaluation
#   bound = max(8 * E32, 4 fp32 ulp of the output's largest magnitude)        (8: __expf against expf, another summation order)
#   a bf16 output may additionally be one bf16 ulp of the reference (relative 2^-7) away, element by element.
# ---------------------------------------------------------------------------------------------------------------------
def f32_bound(ref64, ref32):
    E32 = (ref32.double() - ref64).abs().max().item()
    mag = ref64.abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(mag)) - 23) if mag > 0 else 0.0
    return E32, max(8 * E32, 4 * ulp)


def check_ref(name, got, ref64, ref32, bf16=False):
    """Assert |got - ref64| <= bound (see above) element by element; prints E32, the kernel's error and the bound."""
    got = got.detach().cpu().double().reshape(ref64.shape)
    ref32 = ref32.detach().reshape(ref64.shape)
    E32, bound = f32_bound(ref64, ref32)
    err = (got - ref64).abs()
    allow = bound + (2.0 ** -7) * ref64.abs() if bf16 else bound + 0 * ref64
    over = (err - ((2.0 ** -7) * ref64.abs() if bf16 else 0)).max().item()      # what the fp32 part of the bound has to cover
    print(f"[tol] {name}: E32={E32:.3e} kernel={err.max().item():.3e}{f' (past 1 bf16 ulp: {max(over, 0):.3e})' if bf16 else ''} "
          f"bound={bound:.3e}{' + 2^-7|ref|' if bf16 else ''}")
    ok = err <= allow                                                         # (NaN compares false)
    assert ok.all(), f"{name}: {int((~ok).sum())}/{ok.numel()} off; max err {err.max().item():.4g} (E32 {E32:.3g}, bound {bound:.3g}, " \
                     f"ref max {ref64.abs().max().item():.4g}) first bad idx {(~ok).nonzero()[0].tolist()}"
