"""TEST INFRASTRUCTURE (not collected): the logit warp of the PV -> SMILES search (include/spmm_hip.h, spmm_logit_warp) restated by brute
force in float64 -- an explicit stable sort per row and a sequential cumulative sum, nothing shared with spmm_amd.decode.warp_logits -- the
distance of a row's cut from the boundary (`cut_margin`), and the cases the kernel test runs with their seeded inputs, so that the CPU
suite can assert that no committed row sits within fp32 rounding of its cut."""
from __future__ import annotations

import math
from typing import List, Tuple

import torch

NEG = -float("inf")


def warped_z(lc: torch.Tensor, lu: torch.Tensor | None, w: float, temperature: float) -> torch.Tensor:
    """Rules 1 and 2 in float64 on the fp32 inputs' values: z = (lu + w (lc - lu)) / temperature; lu=None: lc / temperature."""
    g = lc.double() if lu is None else lu.double() + float(w) * (lc.double() - lu.double())
    return g if temperature == 1 else g / float(temperature)


def _ranked(z_row: List[float]) -> List[int]:
    return sorted(range(len(z_row)), key=lambda j: (-z_row[j], j))          # z descending, index ascending


def _row(z_row: List[float], top_k: int, top_p: float, min_keep: int) -> Tuple[List[int], List[float], int]:
    """One row -> (order, cum, K): the ranking, cum[r] = the q-mass of the ranks < r (r < K), and K."""
    V = len(z_row)
    order = _ranked(z_row)
    K = top_k if 0 < top_k < V else V
    top = [z_row[j] for j in order[:K]]
    ex = [math.exp(v - top[0]) for v in top]
    tot = math.fsum(ex)
    cum, run = [], 0.0
    for r in range(K):
        cum.append(run)
        run += ex[r] / tot
    return order, cum, K


def brute_force(lc, lu=None, *, w=1.0, temperature=1.0, top_k=0, top_p=1.0, min_keep=1) -> torch.Tensor:
    """Rules 1-5 on [R, V] inputs -> float64 [R, V]: z where the token is kept, -inf where it is dropped."""
    z = warped_z(lc, lu, w, temperature)
    out = torch.full_like(z, NEG)
    for i, z_row in enumerate(z.tolist()):
        order, cum, K = _row(z_row, top_k, top_p, min_keep)
        for r, j in enumerate(order):
            if r < min_keep or (r < K and cum[r] < top_p):
                out[i, j] = z[i, j]
    return out


def cut_margin(lc, lu=None, *, w=1.0, temperature=1.0, top_k=0, top_p=1.0, min_keep=1) -> torch.Tensor:
    """Per row, how far the cut is from flipping under rounding -- the smaller of
      * the distance of the nearest cumulative mass (of the ranks the nucleus rule decides: min_keep <= r < K) to top_p; top_p = 1 cuts
        nothing (every partial sum of a softmax is below 1) and contributes no distance;
      * the relative gap in z between the last kept and the first dropped rank (the top-k cut, the nucleus cut and the min_keep floor
        alike: a rank swap there changes the kept set).
    A row that keeps everything has margin inf."""
    z = warped_z(lc, lu, w, temperature)
    out = []
    for z_row in z.tolist():
        V = len(z_row)
        order, cum, K = _row(z_row, top_k, top_p, min_keep)
        m = float("inf")
        if top_p < 1:
            for r in range(min_keep, K):
                m = min(m, abs(cum[r] - top_p))
        kept = sum(1 for r in range(V) if r < min_keep or (r < K and cum[r] < top_p))
        if kept < V:
            a, b = z_row[order[kept - 1]], z_row[order[kept]]
            m = min(m, (a - b) / max(abs(a), abs(b), 1e-30))
        out.append(m)
    return torch.tensor(out, dtype=torch.float64)


def value_bound(lc, lu, w: float, temperature: float) -> torch.Tensor:
    """Elementwise bound on |kernel z - float64 z|: the kernel forms z in four fp32 roundings (lc - lu, w * that, + lu, / temperature), each
    at most 2^-24 relative to a quantity no larger than |w| |lc - lu| + |lu| + |g|; a factor 2 on top: 8 * 2^-24 * (...) / temperature.
    Derived, not measured.  (Without lu and at temperature 1 the kernel passes the bits of lc through; the bound is then just not tight.)"""
    lcd = lc.double()
    lud = torch.zeros_like(lcd) if lu is None else lu.double()
    g = lcd if lu is None else lud + float(w) * (lcd - lud)
    return 8.0 * 2.0 ** -24 * (abs(float(w)) * (lcd - lud).abs() + lud.abs() + g.abs()) / float(temperature)


# ------------------------------------------------------------------------------------------------------------------ the kernel test's cases
VS = (8, 64, 65, 300, 320, 321, 512)          # lane-count (64 | 65) and registers-per-lane (320 | 321, 512) boundaries
RS = (1, 4, 5, 9)                             # the workgroup of four waves and one past it
WS = (0.0, 1.0, 1.5, 3.0)
TEMPS = (1.0, 0.7, 1.5)
TOPKS = ("0", "min_keep", "17", "V-1", "V", "V+5")
TOPPS = (1.0, 0.9, 0.5, 1e-6)
KEEPS = (1, 2, 8)
# seed of case i is SEED0 + i + 1000 * BUMP.get(i, 0): a case one of whose rows sat within 1e-4 of its cut got another seed, never a
# narrower bound (tests/test_logit_warp_cpu.py::test_no_committed_row_sits_on_its_cut)
SEED0 = 4100
BUMP: dict = {17: 1, 18: 1, 27: 1}


def _top_k(spec: str, V: int, min_keep: int) -> int:
    return {"0": 0, "min_keep": min_keep, "17": 17, "V-1": V - 1, "V": V, "V+5": V + 5}[spec]


def cases() -> List[dict]:
    """A pruned product of the factors: five cases per V, the other factors cycling at strides coprime to their counts, so every value
    of every factor appears -- 35 cases (tests/test_logit_warp_cpu.py checks the coverage).  A top_k at or above V (17 at V = 8, V, V + 5)
    is "no top-k cut"; the kernel itself also takes a top_k below min_keep -- min_keep wins -- which only the searches refuse."""
    out = []
    i = 0
    for vi, V in enumerate(VS):
        for u in range(5):
            min_keep = KEEPS[(i + vi) % 3]
            c = dict(V=V, R=RS[i % 4], pad_in=(0, 3, 20)[i % 3], pad_out=(0, 5, 12)[(i + 1) % 3], has_lu=i % 5 != 0, alias=i % 4 == 1,
                     w=WS[(i // 2) % 4], temperature=TEMPS[i % 3], top_k=_top_k(TOPKS[i % 6], V, min_keep), top_p=TOPPS[(i + i // 4) % 4],
                     min_keep=min_keep, seed=SEED0 + i + 1000 * BUMP.get(i, 0))
            if c["alias"]:
                c["pad_out"] = c["pad_in"]
            out.append(c)
            i += 1
    return out


def case_id(c: dict) -> str:
    return (f"V{c['V']}-R{c['R']}-{'lu' if c['has_lu'] else 'nolu'}{'-alias' if c['alias'] else ''}-w{c['w']:g}-T{c['temperature']:g}"
            f"-k{c['top_k']}-p{c['top_p']:g}-m{c['min_keep']}")


def case_inputs(c: dict) -> Tuple[torch.Tensor, torch.Tensor | None]:
    """(lc, lu) fp32 [R, ld] on the host, logits ~ N(0, 2^2) in the first V columns and NaN in the padding; lu None when the case has none."""
    g = torch.Generator().manual_seed(c["seed"])
    ld = c["V"] + c["pad_in"]

    def one():
        x = torch.full((c["R"], ld), float("nan"))
        x[:, :c["V"]] = torch.randn(c["R"], c["V"], generator=g) * 2
        return x

    lc = one()
    return lc, (one() if c["has_lu"] else None)


def case_kwargs(c: dict) -> dict:
    return dict(w=c["w"] if c["has_lu"] else 1.0, temperature=c["temperature"], top_k=c["top_k"], top_p=c["top_p"], min_keep=c["min_keep"])


def ties_case() -> Tuple[torch.Tensor, dict]:
    """lc fp32 [5, 300], no lu, temperature 1: blocks of exactly equal logits straddling the top-k cut (rows 0-1), the nucleus cut (rows 2-3)
    and both at once (row 4, all equal).  Small dyadic values: exact in every format, so the index rule alone decides."""
    V = 300
    lc = torch.full((5, V), -6.0)
    j = torch.arange(V)
    lc[0] = -4.0 - (j % 7).float() * 0.25
    lc[0, 10:40] = 2.0                                   # 30 equal best values: top_k = 17 cuts inside the block
    lc[1] = -3.0
    lc[1, 250:300] = 1.5                                 # the block at the end of the row
    lc[1, 3] = 4.0
    lc[2] = -8.0 + (j % 5).float() * 0.5
    lc[2, 100:108] = 3.0                                 # 8 equal values hold nearly all the mass: top_p = 0.5 cuts after the 4th
    lc[3] = -9.0
    lc[3, 0:300:50] = 2.5                                # 6 equal values spread over the row
    lc[4] = 0.5                                          # all equal
    return lc, dict(w=1.0, temperature=1.0, top_k=17, top_p=0.5, min_keep=2)
