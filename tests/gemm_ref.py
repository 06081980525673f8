"""Float64 reference of every epilogue of the bf16 MFMA GEMM, operand builders that keep its f32 accumulator
exact, and a per-element gate.

A helper module, not a test file (the kernel tests import it as `gemm_ref`); plain torch, so it runs on CPU and
GPU tensors alike.

Operands as the kernel takes them (include/vit_hip.h, vit_gemm_args): bf16 A and B, each K-contiguous or
M/N-contiguous with its leading dimension and batch stride, f32 bias (+ batch stride), the aux matrix (bf16 GELU
input / multiplier, f32 residual or position table) with its leading dimension, aux2 (the cls row) and tokens of
the PATCH epilogue, and the dropout multipliers as ops.dropout_mask gives them. Everything the reference returns
is logical: [batch, M, N] (column partials [tile rows, N]).

Exact operands. A is integers in [-4, 4]; B is integers in [-4, 4] (linear epilogues) or those / 64 (GELU
epilogues, so that u = acc + bias is of order 1); bias, aux, pos and cls are integers (GELU: eighths). Every
partial sum of the accumulator is then a multiple of 2^-6 below 2^18 in magnitude: exact in f32 in any summation
order (assert_exact), so whatever tile config, pipeline or split-K produced it, the accumulator the epilogue
sees is THE product and any difference from the reference is the epilogue's or the addressing's.

The gate, per element, never a norm:

    linear outputs (F32, BF16, BIAS_BF16, BIAS_RESID_F32, MUL_BF16, PATCH, SPLITK, their dropout forms with
    p = 0.5, the bf16 `u` of BIAS_GELU, and their column partials): equal to the float64 value rounded once to
    the output type (the integer sums pass 256, so the bf16 rounding, ties included, really happens; the column
    partials are sums of the f32 values before that rounding, as gemm_kernels.h says, hence exact too)

    GELU outputs:   |got - ref| <= U |ref| + c s        U = 2^-8, the bf16 unit roundoff
        s = d max(1, |u|)          gelu and gelu' of BIAS_GELU (c = C_PHI) and BIAS_GELU_DGELU (c = C_DGELU);
                                   d: the dropout multiplier (where it is 0 the output must be 0)
        s = |acc| max(1, |aux|)    GELU_BWD (c = C_PHI)
    column partials of GELU_BWD:  c sum_rows(s) + 2^-16 sum_rows |ref|   (no U: the f32 values are summed)

c is the error each erf formula documents in the source: C_PHI = 1e-6 where only phi_and_pdf runs (Abramowitz &
Stegun 7.1.26, 1.5e-7 on erf, common.h), C_DGELU = 2.5e-5 for the packed gelu_dgelu2 of BIAS_GELU_DGELU (7.1.25,
2.5e-5 on erf, i.e. 1.25e-5 on the cdf: the gate is twice the documented error). Both formulas are ported to
torch below (phi_and_pdf, gelu_dgelu2) for the CPU test of the gate; no kernel is ever compared with them.
"""
import math

import torch

U = 2.0 ** -8
F = 2.0 ** -16
C_PHI = 1e-6
C_DGELU = 2.5e-5

# enum vit_epilogue / vit_layout of include/vit_hip.h (the GPU sweep asserts they match vitmi._lib)
(F32, BF16, BIAS_BF16, BIAS_GELU, BIAS_RESID_F32, GELU_BWD, PATCH, SPLITK, BIAS_GELU_DGELU, MUL_BF16) = range(10)
K_CONTIG, MN_CONTIG = 0, 1
NAMES = ["F32", "BF16", "BIAS_BF16", "BIAS_GELU", "BIAS_RESID_F32", "GELU_BWD", "PATCH", "SPLITK", "BIAS_GELU_DGELU",
         "MUL_BF16"]
LAYOUTS = [(K_CONTIG, K_CONTIG), (K_CONTIG, MN_CONTIG), (MN_CONTIG, MN_CONTIG), (MN_CONTIG, K_CONTIG)]
GELU_EPIS = (BIAS_GELU, GELU_BWD, BIAS_GELU_DGELU)
HAS_BIAS = (BIAS_BF16, BIAS_GELU, BIAS_RESID_F32, PATCH, BIAS_GELU_DGELU)
HAS_AUX = (BIAS_RESID_F32, GELU_BWD, PATCH, MUL_BF16)
HAS_C2 = (BIAS_GELU, BIAS_GELU_DGELU)
HAS_DROPOUT = (BIAS_RESID_F32, PATCH, BIAS_GELU_DGELU)
HAS_COL_PARTIAL = (F32, BF16, BIAS_BF16, BIAS_RESID_F32, GELU_BWD, MUL_BF16)


def out_dtype(epi):
    return torch.float32 if epi in (F32, BIAS_RESID_F32, PATCH, SPLITK) else torch.bfloat16


def aux_dtype(epi):
    return torch.float32 if epi in (BIAS_RESID_F32, PATCH) else torch.bfloat16


# ---- operands in memory ------------------------------------------------------------------------------------------
def strided(buf, rows, cols, ld, batch=1, bs=0, transposed=False):
    """the logical [batch, rows, cols] view of a packed (contiguous) buffer: element (z, r, c) at
    z bs + r ld + c, or at z bs + c ld + r when transposed"""
    st = (bs, 1, ld) if transposed else (bs, ld, 1)
    return buf.reshape(-1).as_strided((batch, rows, cols), st)


def logical_a(A, M, K, layout, lda, batch=1, bs=0):
    """[batch, M, K] view of A ([M][lda] K-contiguous, [K][lda] M-contiguous)"""
    return strided(A, M, K, lda, batch, bs, layout == MN_CONTIG)


def logical_b(B, K, N, layout, ldb, batch=1, bs=0):
    """[batch, K, N] view of B ([N][ldb] K-contiguous, [K][ldb] N-contiguous)"""
    return strided(B, K, N, ldb, batch, bs, layout == K_CONTIG)


def pack(A, B, al, bl):
    """bf16 A [M, K] and B [K, N] as the kernel reads them in layouts (al, bl): Am, Bm, lda, ldb. M/N-contiguous
    operands get their rows zero-padded to a multiple of 8 elements (16 B)."""
    (M, K), N = A.shape, B.shape[1]
    pad = lambda n: (n + 7) // 8 * 8
    if al == K_CONTIG:
        Am, lda = A.contiguous(), K                                            # [M][K]
    else:
        lda = pad(M)
        Am = torch.zeros(K, lda, device=A.device, dtype=torch.bfloat16)        # [K][lda]
        Am[:, :M] = A.t()
    if bl == K_CONTIG:
        Bm, ldb = B.t().contiguous(), K                                        # [N][K]
    else:
        ldb = pad(N)
        Bm = torch.zeros(K, ldb, device=B.device, dtype=torch.bfloat16)        # [K][ldb]
        Bm[:, :N] = B
    return Am, Bm, lda, ldb


def mats(M, N, K, al, bl, ints=False, gen=None, device="cuda"):
    """random bf16 A [M, K] and B [K, N] (ints: integers in [-4, 4]) and their packed forms:
    A, B, Am, Bm, lda, ldb"""
    if ints:
        A = torch.randint(-4, 5, (M, K), device=device).float()
        B = torch.randint(-4, 5, (K, N), device=device).float()
    else:
        A = torch.randn(M, K, device=device)
        B = torch.randn(K, N, device=device)
    A = A.bfloat16()
    B = B.bfloat16()
    return (A, B) + pack(A, B, al, bl)


# ---- exact operand builders --------------------------------------------------------------------------------------
def exact_ab(epi, M, N, K, gen, batch=1):
    """bf16 A [batch, M, K], integers in [-4, 4], and B [batch, K, N], integers in [-4, 4] (/ 64 for the GELU
    epilogues); gen: a CPU torch.Generator"""
    A = torch.randint(-4, 5, (batch, M, K), generator=gen).float()
    B = torch.randint(-4, 5, (batch, K, N), generator=gen).float()
    if epi in GELU_EPIS:
        B = B / 64
    return A.bfloat16(), B.bfloat16()


def exact_bias(epi, N, batch=1):
    """f32 bias [batch, N]: ((n mod 17) - 8) (+ 3 z), in eighths for the GELU epilogues; differs from itself
    shifted by 8 columns everywhere"""
    n = torch.arange(N)
    b = ((n % 17) - 8)[None, :] + 3 * torch.arange(batch)[:, None]
    return (b / 8 if epi in GELU_EPIS else b).float()


def exact_aux(epi, rows, N):
    """the aux matrix [rows, N] in its dtype, a function of (m, n) constant along no row and no column: the f32
    residual / position table and the bf16 multiplier are integers, the bf16 GELU input is eighths in [-2, 2]"""
    m, n = torch.arange(rows)[:, None], torch.arange(N)[None, :]
    if epi == GELU_BWD:
        return ((((3 * m + 5 * n) % 33) - 16) / 8).bfloat16()
    if epi == MUL_BF16:
        return (((3 * m + 5 * n) % 17) - 8).float().bfloat16()
    return (((3 * m + 5 * n) % 23) - 11).float()


def exact_cls(N):
    return ((torch.arange(N) % 13) - 6).float()


def assert_exact(epi, K, rows=256):
    """the condition under which every value the kernel handles is exact in f32, in any summation order: with
    |a| <= 4 and |b| <= 4 (/ 64) every partial sum of the accumulator is an integer (/ 64) of magnitude at most
    16 K, so |acc| 64 < 2^24 suffices for the GELU epilogues; a linear epilogue's value ((acc + bias) mult + aux
    with |bias| <= 14, mult <= 2, |aux| <= 11, or acc aux with |aux| <= 8) is an integer, and so is a column
    partial over at most `rows` of them: rows |value| < 2^24. Returns the largest |value|."""
    assert 16 * K * 64 < 2 ** 24, K
    if epi in GELU_EPIS:
        return 16 * K + 2
    value = 16 * K * 8 if epi == MUL_BF16 else (16 * K + 14) * 2 + 11
    assert rows * value < 2 ** 24, (K, rows, value)
    return value


# ---- float64 reference -------------------------------------------------------------------------------------------
def gelu64(u):
    """erf GELU and its derivative in float64"""
    cdf = 0.5 * (1.0 + torch.special.erf(u / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return u * cdf, cdf + u * pdf


class Ref:
    """out: name -> float64 reference (C, C2, partial); bound: name -> per-element bound, None where the output
    is exact; acc, u, aux, mult, bias: what the outputs were made of (the CPU emulation reuses them)"""


def reference(epi, A, B, M, N, K, *, a_layout, b_layout, lda, ldb, bias=None, aux=None, ldaux=0, aux2=None,
              tokens=0, batch=1, a_bs=0, b_bs=0, bias_bs=0, mult=None, rows_per_tile=None):
    """every output of epilogue epi for these operands. mult: the [M, N] dropout multipliers (None: no dropout).
    rows_per_tile: also the column partials, one row per tile row of that many rows. A SPLITK output is the sum
    of its slabs."""
    r = Ref()
    r.epi = epi
    a = logical_a(A, M, K, a_layout, lda, batch, a_bs).double()
    b = logical_b(B, K, N, b_layout, ldb, batch, b_bs).double()
    acc = r.acc = a @ b
    r.bias = bv = strided(bias, 1, N, 0, batch, bias_bs).double() if bias is not None else torch.zeros_like(acc[:, :1])
    r.mult = dm = mult.double()[None] if mult is not None else torch.ones_like(acc[:1])
    r.aux = ax = (strided(aux, tokens if epi == PATCH else M, N, ldaux).double() if aux is not None else None)
    r.u = u = acc + bv
    r.out, r.bound = {}, {"C": None, "C2": None, "partial": None}
    if epi in (F32, BF16, SPLITK):
        r.out["C"] = acc
    elif epi == BIAS_BF16:
        r.out["C"] = u
    elif epi == BIAS_GELU:
        g, _ = gelu64(u)
        r.out["C"], r.out["C2"] = u, g
        r.bound["C2"] = U * g.abs() + C_PHI * u.abs().clamp_min(1.0)
    elif epi == BIAS_RESID_F32:
        r.out["C"] = u * dm + ax
    elif epi == GELU_BWD:
        _, d = gelu64(ax)
        r.out["C"] = acc * d
        r.scale = acc.abs() * ax.abs().clamp_min(1.0)
        r.bound["C"] = U * r.out["C"].abs() + C_PHI * r.scale
    elif epi == BIAS_GELU_DGELU:
        g, d = gelu64(u)
        r.out["C"], r.out["C2"] = d * dm, g * dm
        s = dm * u.abs().clamp_min(1.0)
        r.bound["C"] = U * r.out["C"].abs() + C_DGELU * s
        r.bound["C2"] = U * r.out["C2"].abs() + C_DGELU * s
    elif epi == MUL_BF16:
        r.out["C"] = acc * ax
    elif epi == PATCH:
        t = torch.arange(M, device=acc.device) % tokens
        body = u + ax[0][t]
        cls = (aux2.double()[:N] + ax[0, 0])[None, None, :].expand_as(body)
        r.out["C"] = torch.where((t == 0)[None, :, None], cls, body) * dm
    else:
        raise ValueError(f"epilogue {epi}")
    r.rows_per_tile = rows_per_tile
    if rows_per_tile:
        v = r.out["C"][0]
        tiles = (M + rows_per_tile - 1) // rows_per_tile
        tsum = lambda x: torch.stack([x[k * rows_per_tile:(k + 1) * rows_per_tile].sum(0) for k in range(tiles)])
        r.out["partial"] = tsum(v)
        if epi == GELU_BWD:
            r.bound["partial"] = C_PHI * tsum(r.scale[0]) + F * tsum(v.abs())
    return r


# ---- the gate ----------------------------------------------------------------------------------------------------
def worst(got, ref, bound):
    """the largest |got - ref| / bound and where: (ratio, index tuple). An element whose bound is 0 must be exact;
    a NaN counts as infinite."""
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err),
                                                            torch.full_like(err, float("inf"))))
    ratio = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf"))
    at = int(ratio.argmax())
    value, idx = float(ratio.reshape(-1)[at]), []
    for n in reversed(ratio.shape):
        idx.append(at % n)
        at //= n
    return value, tuple(reversed(idx))


def expected(ref, dtype):
    """the float64 value rounded once to the output type (bf16: round to nearest even)"""
    return ref.float().to(dtype)


def check(r, **got):
    """got: any of C, C2 ([batch, M, N], in the output's own dtype) and partial ([tile rows, N] f32). Returns
    name -> (worst ratio, (batch, row, column)); partial reports (tile row, column). An exact output's ratio is 0
    or infinite."""
    res = {}
    for name, t in got.items():
        ref, bound = r.out[name], r.bound[name]
        if bound is None:
            ref, bound = expected(ref, t.dtype).double(), torch.zeros_like(ref)
        res[name] = worst(t, ref, bound)
    return res


def failures(res, tag=""):
    """the entries of check()'s result past the gate, as readable strings"""
    return [f"{tag}{name}: {ratio:.3g} x gate at (batch, row, col) {loc}" for name, (ratio, loc) in res.items()
            if not ratio <= 1.0]


# ---- the kernels' two erf formulas, ported (the CPU test of the gate only) ----------------------------------------
def phi_and_pdf(u):
    """common.h phi_and_pdf in f32 torch: the normal cdf from Abramowitz & Stegun 7.1.26, and the pdf"""
    u = u.float()
    e = torch.exp(-0.5 * u * u)
    t = 1.0 / (1.0 + (0.3275911 * 0.70710678118654752) * u.abs())
    p = 1.061405429 * t - 1.453152027
    p = p * t + 1.421413741
    p = p * t - 0.284496736
    p = p * t + 0.254829592
    erfa = 1.0 - p * t * e
    return 0.5 + 0.5 * torch.copysign(erfa, u), 0.39894228040143268 * e


def gelu_dgelu2(u):
    """gemm_kernels.h gelu_dgelu2 in f32 torch: gelu and gelu' with erf from Abramowitz & Stegun 7.1.25"""
    u = u.float()
    e = torch.exp2(u * u * -0.72134752044448170)
    t = 1.0 / (u.abs() * (0.47047 * 0.70710678118654752) + 1.0)
    q = t * 0.7478556 - 0.0958798
    q = q * t + 0.3480242
    q = q * t
    erfa = 1.0 - q * e
    cdf = torch.copysign(erfa, u) * 0.5 + 0.5
    pdf = e * 0.39894228040143268
    return u * cdf, u * pdf + cdf


def emulate(r, dgelu_vector=True):
    """The epilogue of r.epi in f32 torch on the exact accumulator, rounded to the output type: what a correct
    kernel writes (dgelu_vector: BIAS_GELU_DGELU by gelu_dgelu2, as the 8-column paths, else by phi_and_pdf, as
    the scalar path). Only the CPU test of the gate uses it."""
    epi, dt = r.epi, out_dtype(r.epi)
    acc, u, dm = r.acc.float(), r.u.float(), r.mult.float()
    if epi == BIAS_GELU:
        cdf, _ = phi_and_pdf(u)
        out = {"C": u, "C2": u * cdf}
    elif epi == GELU_BWD:
        ax = r.aux.float()
        cdf, pdf = phi_and_pdf(ax)
        out = {"C": acc * (cdf + ax * pdf)}
        if "partial" in r.out:
            rpt = r.rows_per_tile
            out["partial"] = torch.stack([out["C"][0][k:k + rpt].sum(0) for k in range(0, acc.shape[1], rpt)])
    elif epi == BIAS_GELU_DGELU:
        if dgelu_vector:
            g, d = gelu_dgelu2(u)
        else:
            cdf, pdf = phi_and_pdf(u)
            g, d = u * cdf, cdf + u * pdf
        out = {"C": d * dm, "C2": g * dm}
    else:
        out = {k: v.float() for k, v in r.out.items()}
    return {k: (v if k == "partial" else v.to(dt)) for k, v in out.items()}
