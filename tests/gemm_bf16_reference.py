"""Reference, kernel-arithmetic model, per-element bound, case list and seeded defects for the bf16-output epilogues of spmm_gemm_nt
(SPMM_EPI_BF16, _GELU, _GELU_DERIV, _GELU_GRAD, _MUL; include/spmm_hip.h) on every tile kernel that builds them.  Plain torch, any device;
tests/test_gemm_bf16_epilogues_gpu.py runs the kernels on these cases, tests/test_gemm_bf16_reference_cpu.py checks this module itself.

    acc = A[M,K] . W[N,K]^T          pre = alpha * acc / (*div) + bias          (bias under EVERY epilogue, the two multiplying ones too)
    SPMM_EPI_BF16        C = pre + R
    SPMM_EPI_GELU        C = gelu(pre)            C2 = pre            gelu(x) = x/2 (1 + erf(x / sqrt 2)), exact erf here
    SPMM_EPI_GELU_DERIV  C = gelu(pre)            C2 = gelu'(pre)
    SPMM_EPI_GELU_GRAD   C = pre * gelu'(G)
    SPMM_EPI_MUL         C = pre * G
    colsum[n] += sum over the rows computed of the C the kernel stored (the rounded values)

ref() evaluates that in float64 and in float32.  model() is the kernels' own arithmetic in float32 (used by the CPU test only): `pre` is
rounded to bf16 where epi_convert / p8_epilogue_blocks write it into the LDS tile, the second operand (+ R, * G, * gelu'(G)) is applied to
the rounded value in fp32 and the result is rounded again; the GELU forms use the Abramowitz-Stegun 7.1.26 erf of csrc/common.h.

The bound is per element and holds no fixed tolerance.  With U = 2^-8 (half a bf16 ulp, relative: what round-to-nearest guarantees) and
b(q) = max(8 E32, 4 fp32 ulp of max |q|) (helpers_gpu.f32_bound; E32 = largest error of the float32 evaluation of q against float64):

    BF16          b(pre) + U |C|                                              one rounding
    BF16 + R      b(pre) + U |pre| + U |C|                                    the first rounding passes through `+ R` with factor 1
    MUL           (b(pre) + U |pre|) |G| + U |C|                              ... through `* G` with factor |G|
    GELU_GRAD     (b(pre) + U |pre|) |g| + (b(g) + 1.5e-7) |pre| + U |C|      g = gelu'(G); 1.5e-7: the stated error of 7.1.26 on erf, which
                                                                              bounds the error of gelu' too (the density shares the exponential)
    GELU, _DERIV  C:  b(gelu(pre)) + 0.75e-7 |pre| + U |C|                    one rounding (gelu is taken of the unrounded pre)
                  C2: b(pre) + U |pre|   (GELU)         b(gelu'(pre)) + 1.5e-7 + U |C2|   (GELU_DERIV)
    colsum        b(s) alone, s = colsum_after - colsum_before against the float64 column sums of the stored C; its float32 evaluation adds
                  the rows to the initial (random, non-zero) colsum 64 at a time in fp32, as a wave adds its partial sums with atomics.

The bound is first order: the second half ulp is taken at the exact value, not at the once-rounded one the kernel rounds (a difference of at
most 2^-16 |pre|, and only where the two straddle a power of two).  No term had to be widened: model() stays inside this bound at every case
below (the CPU test asserts it; worst error / bound 0.996).

Every output is a view of a larger buffer full of SENTINEL (PAD_ROWS more rows; row stride N + 8 for C and N + 16 for C2, N rounded up to
a multiple of 8 first: the entry point refuses bf16 rows that are not 16-B aligned); R and G are views of wider matrices with strides of
their own.  check_output() asserts the bound on the views and that every element outside them keeps SENTINEL's bits.  Under a device-side
row count (M_launch) the rows [M, M_launch) of A, R and G hold NaN: the rows of C / C2 past M keep the sentinel and colsum stays finite.
defective() returns the buffers as a kernel with ONE known defect would leave them; the CPU test asserts that check_output() rejects every
one of them at every problem where it applies."""
import functools
from dataclasses import dataclass
from typing import Optional

import torch

from helpers_gpu import f32_bound

BF = torch.bfloat16
EPI_BF16, EPI_GELU, EPI_GELU_GRAD, EPI_GELU_DERIV, EPI_MUL = 0, 1, 4, 6, 7          # spmm_amd.ops.EPI_* (pinned by the CPU test)
K128, K256x128, K256, K128PC, K256P8, K256P8_TILES = 1, 2, 3, 5, 8, 9              # SPMM_GEMM_* kernel selectors (pinned too)
SHARED_KERNELS, P8_KERNELS = (K128, K256x128, K256, K128PC), (K256P8, K256P8_TILES)  # epi_convert / epi_store; p8_epilogue_blocks
SENTINEL = -1232.0                                                                  # exact in bf16
PAD_ROWS = 3
DIV = 0.07                                                                          # the step's temperature
U = 2.0 ** -8
ERF_ERR = 1.5e-7                                                                    # Abramowitz-Stegun 7.1.26: |erf error| <= 1.5e-7
SQRT1_2, INV_SQRT_2PI = 0.70710678118654752, 0.3989422804014327
CLS_L, CLS_SPARE, WROWS_OFF, C_OFF = 5, 2, 64, 32
# One-row problems have as few as 8 outputs, and truncation is outside the bound only on an element whose dropped bits are large: the seed of
# A at these (M, rows, N, K) is moved until truncated_store is rejected in every form the shape runs in (inputs chosen, never the bound).
SEED_BUMP = {(1, 1, 8, 64): 98, (1, 1, 8, 128): 35, (1, 700, 136, 128): 7}


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    """test_kernels_gpu.py::rnd, left on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def ceil8(n):
    return (n + 7) // 8 * 8


# the epilogue forms of the issue's group (b) (+ GELU_GRAD with a bias: the header's statement about it)
FORMS = {
    "bf16": dict(epi=EPI_BF16),
    "bf16-bias-R": dict(epi=EPI_BF16, bias=True, R=True),
    "bf16-full": dict(epi=EPI_BF16, bias=True, alpha=0.5, div=DIV, R=True, colsum=True),
    "bf16-R-cs": dict(epi=EPI_BF16, R=True, colsum=True),
    "bf16-R": dict(epi=EPI_BF16, R=True),
    "gelu-c2": dict(epi=EPI_GELU, bias=True, C2=True),
    "gelu": dict(epi=EPI_GELU, bias=True),
    "deriv": dict(epi=EPI_GELU_DERIV, bias=True, C2=True),
    "grad": dict(epi=EPI_GELU_GRAD),
    "grad-cs": dict(epi=EPI_GELU_GRAD, colsum=True),
    "grad-bias": dict(epi=EPI_GELU_GRAD, bias=True),
    "mul-cs": dict(epi=EPI_MUL, colsum=True),
    "mul-alpha-cs": dict(epi=EPI_MUL, alpha=0.5, colsum=True),
    "mul-bias": dict(epi=EPI_MUL, bias=True),
}
FORM_DEFAULTS = dict(epi=None, bias=False, alpha=1.0, div=None, R=False, C2=False, colsum=False)
FORMS_B = ("bf16", "bf16-full", "gelu-c2", "gelu", "deriv", "grad-cs", "mul-alpha-cs", "mul-bias", "grad-bias")


@dataclass(frozen=True)
class Problem:
    M: int                              # rows computed (the device-side row count where M_launch is set)
    N: int
    K: int
    form: str
    layout: str = "dense"               # dense | cls | wslice | wrows | knarrow | cslice (group c)
    M_launch: Optional[int] = None      # the launch is sized for M_launch rows, *M_dev = M; A, R, G hold NaN in rows [M, M_launch)
    launches: int = 1                   # launches (operands of their own, outputs of their own) that add into ONE colsum

    def __getattr__(self, k):           # epi, bias, alpha, div, R, C2, colsum: the form's
        if k not in FORM_DEFAULTS:
            raise AttributeError(k)
        return FORMS[self.form].get(k, FORM_DEFAULTS[k])

    @property
    def rows(self):
        return self.M if self.M_launch is None else self.M_launch

    @property
    def has_G(self):
        return self.epi in (EPI_GELU_GRAD, EPI_MUL)

    @property
    def c_off(self):
        return C_OFF if self.layout == "cslice" else 0

    @property
    def name(self):
        s = f"{self.M}x{self.N}x{self.K}-{self.form}" + (f"-{self.layout}" if self.layout != "dense" else "")
        return s + (f"-x{self.launches}" if self.launches > 1 else "") + (f"-of{self.M_launch}" if self.M_launch else "")


# ---------------------------------------------------------------------------------------------------------------------
# operands and buffers
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bases(M, rows, N, K, layout, launches, device):
    nan = float("nan")
    A, W = [], []
    for l in range(launches):
        if layout == "cls":
            a = rnd((rows + CLS_SPARE) * CLS_L, K, seed=100 + l)
        else:
            a = rnd(rows, 2 * K if layout == "knarrow" else K, seed=100 + l + SEED_BUMP.get((M, rows, N, K), 0))
            a[M:] = nan
        A.append(a)
        wshape = {"wslice": (N, 2 * K), "wrows": (N + WROWS_OFF, K), "knarrow": (N, K + 64)}.get(layout, (N, K))
        W.append(rnd(*wshape, scale=0.05, seed=200 + l))
    Rw, Gw = rnd(rows, ceil8(N) + 24, seed=400), rnd(rows, ceil8(N) + 48, seed=450)
    Rw[M:] = nan
    Gw[M:] = nan
    x = dict(A=A, W=W, bias=rnd(N, seed=300, dtype=torch.float32), R=Rw, G=Gw, colsum0=3.0 * rnd(N, seed=600, dtype=torch.float32),
             div=torch.tensor([DIV], dtype=torch.float32))
    return {k: [t.to(device) for t in v] if isinstance(v, list) else v.to(device) for k, v in x.items()}


def bases(p, device="cpu"):
    """Base tensors the operands are views of: the same for every epilogue form and kernel of a shape.  Shared: never modified."""
    return _bases(p.M, p.rows, p.N, p.K, p.layout, p.launches, str(device))


def operands(p, x, l=0):
    """The tensors of launch l as ops.gemm_nt takes them (views of x = bases(p, device)): A, W, keyword arguments."""
    A, W = x["A"][l], x["W"][l]
    if p.layout == "cls":
        A = A.view(-1, CLS_L * p.K)[:p.rows, :p.K]                  # position 0 of each sequence: row stride L * H
    elif p.layout == "wslice":
        W = W[:, p.K:]                                             # WT[:, H:]
    elif p.layout == "wrows":
        W = W[WROWS_OFF:]                                          # Wqkv[H:]
    kw = dict(bias=x["bias"] if p.bias else None, alpha=p.alpha, div=x["div"] if p.div is not None else None,
              R=x["R"][:, :p.N] if p.R else None, G=x["G"][:, :p.N] if p.has_G else None, epi=p.epi)
    if p.layout == "knarrow":
        kw["K"] = p.K
    return A, W, kw


def initial_buffers(p, device="cpu"):
    """{'C': one [rows + PAD_ROWS, c_off + ceil8(N) + 8] bf16 buffer of SENTINEL per launch, 'C2': the same with + 16 (or None),
    'colsum': the random initial vector (or None)}."""
    full = lambda w: torch.full((p.rows + PAD_ROWS, w), SENTINEL, dtype=BF, device=device)
    return dict(C=[full(p.c_off + ceil8(p.N) + 8) for _ in range(p.launches)],
                C2=[full(ceil8(p.N) + 16) for _ in range(p.launches)] if p.C2 else None,
                colsum=bases(p, device)["colsum0"].clone() if p.colsum else None)


def c_view(buf, p):
    return buf[:p.rows, p.c_off:p.c_off + p.N]


def c2_view(buf, p):
    return buf[:p.rows, :p.N]


# ---------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------
def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * SQRT1_2))


def dgelu(x):
    return 0.5 * (1.0 + torch.erf(x * SQRT1_2)) + x * (INV_SQRT_2PI * torch.exp(-0.5 * x * x))


@functools.lru_cache(maxsize=None)
def _acc(M, rows, N, K, layout, launches, l, device, dtype):
    p = Problem(M, N, K, "bf16", layout=layout, M_launch=None if rows == M else rows, launches=launches)
    A, W, _ = operands(p, bases(p, device), l)
    return A[:M, :K].to(dtype) @ W[:, :K].to(dtype).t()


def ref(p, dtype, l=0, device="cpu"):
    """The documented formula of launch l, every operation in `dtype` (float64 or float32), over the M rows computed.
    -> {'pre', 'C', 'C2' (or None), 'g' (the factor of the multiplying epilogues, or None), 'colsum' (the increment, or None)}."""
    x = bases(p, device)
    _, _, kw = operands(p, x, l)
    v = p.alpha * _acc(p.M, p.rows, p.N, p.K, p.layout, p.launches, l, str(device), dtype)
    if kw["div"] is not None:
        v = v / kw["div"].to(dtype)
    if kw["bias"] is not None:
        v = v + kw["bias"].to(dtype)
    C2 = g = None
    if p.epi == EPI_BF16:
        C = v + kw["R"][:p.M].to(dtype) if p.R else v
    elif p.epi == EPI_MUL:
        g = kw["G"][:p.M].to(dtype)
        C = v * g
    elif p.epi == EPI_GELU_GRAD:
        g = dgelu(kw["G"][:p.M].to(dtype))
        C = v * g
    else:
        C, C2 = gelu(v), (v if p.epi == EPI_GELU else dgelu(v))
    return dict(pre=v, C=C, C2=C2, g=g, colsum=C.sum(0) if p.colsum else None)


def bound(p, r64, r32):
    """-> {'C': (E32, fp32 part, rounding allowance), 'C2': ...}: the per-element bound of the module docstring is fp32 part + rounding
    allowance (tensors shaped like the output, or scalars)."""
    E, b = f32_bound(r64["pre"], r32["pre"].double())
    pre, C = r64["pre"].abs(), r64["C"].abs()
    out = {}
    if p.epi == EPI_BF16:
        out["C"] = (E, b + 0 * C, (U * pre if p.R else 0) + U * C)
    elif p.epi == EPI_MUL:
        g = r64["g"].abs()
        out["C"] = (E, b * g, U * pre * g + U * C)
    elif p.epi == EPI_GELU_GRAD:
        g = r64["g"].abs()
        _, bg = f32_bound(r64["g"], r32["g"].double())
        out["C"] = (E, b * g + (bg + ERF_ERR) * pre, U * pre * g + U * C)
    else:
        Ec, bc = f32_bound(r64["C"], r32["C"].double())
        out["C"] = (Ec, bc + 0.5 * ERF_ERR * pre, U * C)
        if p.epi == EPI_GELU:
            out["C2"] = (E, b + 0 * pre, U * pre)
        else:
            E2, b2 = f32_bound(r64["C2"], r32["C2"].double())
            out["C2"] = (E2, b2 + ERF_ERR + 0 * pre, U * r64["C2"].abs())
    return out


def _check_view(name, buf, r0, c0, M, N, ref64, E32, fp, rounding):
    """buf[r0:r0+M, c0:c0+N] within fp + rounding of ref64, every other element of buf SENTINEL's bits.  Prints the `[tol]` line.
    -> worst error / bound."""
    got = buf[r0:r0 + M, c0:c0 + N].double()
    err = (got - ref64).abs()
    allow = fp + rounding
    ok = err <= allow                                                         # (NaN compares false)
    ratio = (err / allow.clamp_min(1e-300)).max().item()
    print(f"[tol] {name}: E32={E32:.3e} kernel={err.max().item():.3e} past_rounding={max((err - rounding).max().item(), 0.0):.3e} "
          f"bound={fp.max().item():.3e}+rounding ratio={ratio:.3f}")
    assert ok.all(), f"{name}: {int((~ok).sum())}/{ok.numel()} off; max err {err.max().item():.4g}, worst err/bound {ratio:.3f} " \
                     f"(E32 {E32:.3g}, ref max {ref64.abs().max().item():.4g}) first bad idx {(~ok).nonzero()[0].tolist()}"
    outside = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    outside[r0:r0 + M, c0:c0 + N] = False
    touched = outside & (buf.view(torch.int16) != torch.tensor(SENTINEL, dtype=BF).view(torch.int16).item())
    assert not touched.any(), f"{name}: {int(touched.sum())} elements outside the view written; first {touched.nonzero()[0].tolist()}"
    return ratio


def colsum_bound(p, stored, colsum0):
    """stored: the [:M, :N] views of C the launches left (bf16).  -> (float64 increment, E32, bound): the float32 evaluation adds the rows
    to colsum0 64 at a time, launch after launch."""
    s64 = sum(c.double().sum(0) for c in stored)
    run = colsum0.clone()
    for c in stored:
        for r in range(0, p.M, 64):
            run = run + c[r:r + 64].float().sum(0)
    E32, b = f32_bound(s64, run.double() - colsum0.double())
    return s64, E32, b


def check_output(name, out, p, device="cpu"):
    """out: the buffers of initial_buffers(p) after the launches, on `device`.  Asserts the module's bound on every view, SENTINEL's bits
    everywhere else, and the column-sum rule.  -> the worst error / bound ratio over the outputs."""
    worst = 0.0
    stored = []
    for l in range(p.launches):
        r64, r32 = ref(p, torch.float64, l, device), ref(p, torch.float32, l, device)
        bd = bound(p, r64, r32)
        tag = f"{name}{f' launch {l}' if p.launches > 1 else ''}"
        buf = out["C"][l]
        assert buf.dtype == BF and tuple(buf.shape) == (p.rows + PAD_ROWS, p.c_off + ceil8(p.N) + 8) and buf.is_contiguous()
        worst = max(worst, _check_view(f"{tag} C", buf, 0, p.c_off, p.M, p.N, r64["C"], *bd["C"]))
        stored.append(buf[:p.M, p.c_off:p.c_off + p.N])
        if p.C2:
            buf2 = out["C2"][l]
            assert buf2.dtype == BF and tuple(buf2.shape) == (p.rows + PAD_ROWS, ceil8(p.N) + 16) and buf2.is_contiguous()
            worst = max(worst, _check_view(f"{tag} C2", buf2, 0, 0, p.M, p.N, r64["C2"], *bd["C2"]))
    if p.colsum:
        cs, cs0 = out["colsum"], bases(p, device)["colsum0"]
        assert cs.dtype == torch.float32 and tuple(cs.shape) == (p.N,)
        assert bool(torch.isfinite(cs).all()), f"{name} colsum: not finite"
        s64, E32, b = colsum_bound(p, stored, cs0)
        err = (cs.double() - cs0.double() - s64).abs()
        ratio = err.max().item() / b
        print(f"[tol] {name} colsum: E32={E32:.3e} kernel={err.max().item():.3e} past_rounding={err.max().item():.3e} bound={b:.3e} "
              f"ratio={ratio:.3f}")
        assert bool((err <= b).all()), f"{name} colsum: max err {err.max().item():.4g} over the bound {b:.4g} (E32 {E32:.3g}); " \
                                       f"first bad column {(err > b).nonzero()[0].tolist()}"
        worst = max(worst, ratio)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in float32 (CPU), with or without one seeded defect
# ---------------------------------------------------------------------------------------------------------------------
def fast_erf(z):
    """csrc/common.h::fast_erf -- Abramowitz-Stegun 7.1.26 in float32."""
    az = z.abs()
    t = 1.0 / (1.0 + 0.3275911 * az)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    return torch.copysign(1.0 - poly * torch.exp(-az * az), z)


def fast_gelu_both(x):
    """csrc/common.h::gelu_erf_both -- gelu and gelu' from one exponential."""
    az = x.abs() * SQRT1_2
    t = 1.0 / (1.0 + 0.3275911 * az)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    e = torch.exp(-0.5 * x * x)
    cdf = 0.5 * (1.0 + torch.copysign(1.0 - poly * e, x))
    return x * cdf, cdf + x * (INV_SQRT_2PI * e)


def fast_gelu(x):
    return 0.5 * x * (1.0 + fast_erf(x * SQRT1_2))


def fast_dgelu(x):                      # csrc/common.h::gelu_erf_grad
    return 0.5 * (1.0 + fast_erf(x * SQRT1_2)) + x * (INV_SQRT_2PI * torch.exp(-0.5 * x * x))


def truncate_bf16(x):
    """float32 -> bf16 by dropping the low 16 bits (the defect; the kernels round to nearest even)."""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


DEFECTS = ("truncated_store", "k_tile_missing", "bias_4_columns_off", "alpha_after_bias", "div_ignored", "operand_row_off",
           "operand_row_clamped", "R_skips_last_chunk", "C_and_C2_exchanged", "C2_is_gelu", "stale_accumulators", "tiles_exchanged",
           "chunk_past_N", "row_past_M", "colsum_past_M_dev", "colsum_misses_second_half", "colsum_unrounded")


def _last_tile(p):
    return (p.M - 1) // 128 * 128, (p.N - 1) // 128 * 128


def applicable_defects(p):
    second = p.R or p.has_G                                  # an R or G operand is read
    tiles = _last_tile(p) != (0, 0)
    return [d for d in DEFECTS if {
        "bias_4_columns_off": p.bias, "alpha_after_bias": p.bias and p.alpha != 1.0, "div_ignored": p.div is not None,
        "operand_row_off": second and p.M > 1, "operand_row_clamped": second and p.M > 1, "R_skips_last_chunk": p.R,
        "C_and_C2_exchanged": p.C2, "C2_is_gelu": p.C2, "stale_accumulators": tiles, "tiles_exchanged": tiles,
        "colsum_past_M_dev": p.colsum and p.M_launch is not None, "colsum_misses_second_half": p.colsum and p.M > 64,
        "colsum_unrounded": p.colsum}.get(d, True)]


def model(p):
    """The buffers as the kernels' documented arithmetic leaves them: float32 matmul, pre rounded to bf16, the second operand applied in
    fp32 and rounded again, the 7.1.26 erf, column sums of the rounded outputs."""
    return _emulate(p, None)


def defective(p, name):
    """The buffers as a kernel with ONE defect would leave them:
      truncated_store            the final conversion to bf16 drops the low bits instead of rounding to nearest
      k_tile_missing             the last 64-wide K-tile is never multiplied
      bias_4_columns_off         column n adds bias[n + 4]              alpha_after_bias: alpha * (acc / div + bias)
      div_ignored                *div is not applied
      operand_row_off            row m reads row m + 1 of R / G         operand_row_clamped: the final 8 rows all read row M - 1 of R / G
      R_skips_last_chunk         the last 8- (or 4-) column chunk of every row is stored without R
      C_and_C2_exchanged         each output lands in the other's buffer          C2_is_gelu: C2 receives gelu(pre) as well
      stale_accumulators         the last tile still holds the first tile's product (added to its own)
      tiles_exchanged            the first and the last 128 x 128 tile store each other's results (the part they share)
      chunk_past_N               row 0 writes one 16-B chunk right of column N    row_past_M: row M (or *M_dev) receives a row of results
      colsum_past_M_dev          the column sums run over the rows the launch is sized for (NaN operands past *M_dev)
      colsum_misses_second_half  rows 64 .. 127 of every 128-row wave tile are not summed
      colsum_unrounded           the column sums add the fp32 values before the final rounding"""
    assert name in DEFECTS
    return _emulate(p, name)


def _emulate(p, defect):
    x, out, f32 = bases(p), initial_buffers(p), torch.float32
    M, N = p.M, p.N
    for l in range(p.launches):
        A, W, kw = operands(p, x, l)
        A, W = A[:M, :p.K].float(), W[:, :p.K].float()
        kend = p.K - 64 if defect == "k_tile_missing" else p.K
        acc = A[:, :kend] @ W[:, :kend].t() if kend > 0 else torch.zeros(M, N)
        r0, c0 = _last_tile(p)
        if defect == "stale_accumulators":
            acc[r0:, c0:] += acc[:M - r0, :N - c0].clone()
        scale = torch.tensor(p.alpha, dtype=f32)
        if kw["div"] is not None and defect != "div_ignored":
            scale = scale / kw["div"]
        bias = kw["bias"]
        if bias is not None and defect == "bias_4_columns_off":
            bias = torch.roll(bias, -4)
        if defect == "alpha_after_bias":
            v = (acc * (scale / p.alpha) + bias) * p.alpha
        else:
            v = acc * scale if bias is None else acc * scale + bias
        S = None
        if p.R or p.has_G:
            S = (kw["R"] if p.R else kw["G"])[:M].float()
            if defect == "operand_row_off":
                S = torch.roll(S, -1, 0)
            if defect == "operand_row_clamped":
                S = S.clone()
                S[max(M - 8, 0):] = S[M - 1]
        C2 = None
        if p.epi == EPI_BF16:
            y = v.to(BF).float() + S if p.R else v
            if defect == "R_skips_last_chunk":
                n0 = N - (8 if N % 8 == 0 else 4)
                y[:, n0:] = v.to(BF).float()[:, n0:]
        elif p.epi == EPI_MUL:
            y = v.to(BF).float() * S
        elif p.epi == EPI_GELU_GRAD:
            y = v.to(BF).float() * fast_dgelu(S)
        elif p.epi == EPI_GELU:
            y, C2 = fast_gelu(v), v
        else:
            y, C2 = fast_gelu_both(v)
        to_bf = truncate_bf16 if defect == "truncated_store" else (lambda t: t.to(BF))
        C = to_bf(y)
        if defect == "tiles_exchanged":
            a, b = C[r0:, c0:].clone(), C[:M - r0, :N - c0].clone()
            C[r0:, c0:], C[:M - r0, :N - c0] = b, a
        if p.C2:
            C2 = C.clone() if defect == "C2_is_gelu" else to_bf(C2)
            if defect == "C_and_C2_exchanged":
                C, C2 = C2, C
            c2_view(out["C2"][l], p)[:M] = C2
        buf = out["C"][l]
        c_view(buf, p)[:M] = C
        if defect == "chunk_past_N":
            buf[0, p.c_off + N:p.c_off + N + 8] = C[0, N - 8:N]
        if defect == "row_past_M":
            buf[M, p.c_off:p.c_off + N] = C[M - 1]
        if p.colsum:
            add = y if defect == "colsum_unrounded" else C.float()
            if defect == "colsum_misses_second_half":
                add = add[(torch.arange(M) % 128) < 64]
            out["colsum"] += add.sum(0)
            if defect == "colsum_past_M_dev":
                out["colsum"] += float("nan")                # what NaN operands in the rows past *M_dev sum to
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gemm_bf16_epilogues_gpu.py: (problem, kernel selector); selector 0 = the automatic choice
# ---------------------------------------------------------------------------------------------------------------------
def _with_auto(cases):
    """+ every problem of `cases` once on selector 0."""
    return cases + [(p, 0) for p in dict.fromkeys(p for p, _ in cases)]


# a. ragged edges on every selector: M = 1, the 8-row store predicate of the 8-phase blocks (72, 264 = 16 k + 8), one row past each tile
#    height (129, 257), more than two tiles (520); N = one chunk (8), one chunk past a tile (72, 136, 264), the half chunk of epi_store
#    (12, 132, 260); K = ring exactly full / first restage (64, 192, 320), one to three K-tile pairs of the 8-phase kernel (128, 256, 384)
RAGGED_SHARED = [(1, 8, 64), (72, 12, 192), (129, 72, 320), (257, 132, 64), (264, 136, 192), (520, 264, 64), (520, 260, 192),
                 (520, 264, 320), (1, 260, 320)]
RAGGED_P8 = [(1, 8, 128), (72, 72, 256), (129, 136, 384), (257, 8, 256), (264, 72, 128), (520, 264, 128), (520, 264, 256),
             (520, 264, 384), (1, 136, 384)]
FORMS_A = ("bf16-bias-R", "mul-cs")
CASES_RAGGED = _with_auto([(Problem(M, N, K, f), k) for ks, shapes in ((SHARED_KERNELS, RAGGED_SHARED), (P8_KERNELS, RAGGED_P8))
                           for (M, N, K) in shapes for f in FORMS_A for k in ks])

# b. every epilogue form on every selector, ragged both ways and several tiles
CASES_FORMS = _with_auto([(Problem(520, 264, 256, f), k) for f in FORMS_B for k in SHARED_KERNELS + P8_KERNELS]
                         + [(Problem(520, 260, 256, f), k) for f in FORMS_B for k in SHARED_KERNELS])

# c. operand layouts the engine uses (B = 70 sequences, H = 128)
LAYOUTS = ("cls", "wslice", "wrows", "knarrow", "cslice")
CASES_LAYOUTS = _with_auto([(Problem(70, 136, 128, "bf16-bias-R", layout=lay), k) for lay in LAYOUTS for k in SHARED_KERNELS + P8_KERNELS])

# d. device-side row count: sized for 700 rows, *M_dev = 1, 300, 700; 264 of 520; NaN tails
CASES_MDEV = _with_auto([(Problem(Md, 136, 128, f, M_launch=700), k) for f in FORMS_B for Md in (1, 300, 700) for k in SHARED_KERNELS + P8_KERNELS]
                        + [(Problem(264, 136, 128, "bf16-full", M_launch=520), k) for k in SHARED_KERNELS + P8_KERNELS])

# f. two launches with operands of their own into one colsum vector
CASES_ACCUM = [(Problem(264, 136, 128, f, launches=2), k) for f in ("bf16-full", "mul-alpha-cs") for k in (K256, K256P8)]


# e. the persistent walk of the 8-phase kernel
def persistent_shape(ncu):
    """-> (s, M = N): s the smallest odd number with s * s > the grid (the CU count rounded down to a multiple of 8); s x s tiles of 256 with a
    ragged last tile row and column."""
    grid = ncu // 8 * 8
    s = 1
    while s * s <= grid:
        s += 2
    return s, 256 * (s - 1) + 8


PERSISTENT_FORMS = [("bf16-R-cs", 128), ("deriv", 128), ("grad", 128), ("mul-cs", 128), ("bf16-R", 1152)]


def persistent_cases(ncu):
    """The problems of group e on a device with `ncu` CUs: the full s x s walk in every form (K = 128: tile order 2; K = 1152: order 0), and two
    device-side row counts: tile rows r with r * s < grid (some workgroups exit at once) and grid < r * s < 2 grid."""
    s, MN = persistent_shape(ncu)
    grid = ncu // 8 * 8
    cases = [Problem(MN, MN, K, f) for f, K in PERSISTENT_FORMS]
    r_below = (grid - 1) // s
    r_between = next(r for r in range(1, s + 1) if r * s > grid)
    for r in (r_below, r_between):
        if 1 <= r < s:
            assert r * s < grid if r == r_below else grid < r * s < 2 * grid
            cases.append(Problem(256 * (r - 1) + 8, MN, 128, "bf16-R-cs", M_launch=MN))
    return cases


ALL_CASES = CASES_RAGGED + CASES_FORMS + CASES_LAYOUTS + CASES_MDEV + CASES_ACCUM
PROBLEMS = list(dict.fromkeys(p for p, _ in ALL_CASES))                   # distinct, in order


def case_id(case):
    p, k = case
    return f"k{k}-{p.name}"
