"""Float64 references, per-element gates and f32 emulations for LayerNorm (csrc/layernorm.hip).

A helper module like glue_ref.py (whose embed / first_touched / first_diff / worst / ints / ulp32 it builds on); plain
torch, so it runs on CPU and GPU tensors alike. The references are float64 evaluations of the definition on the f32
inputs as the kernel sees them (a bf16 dy after its exact widening; the backward takes mean and rstd as the f32 inputs
they are). Every gate is per element and is a sum of terms, each a counted number of roundings times the magnitude it
acts on, u = 2^-24 per rounding; SLACK = 1 + 2^-9 covers the second-order products of those terms (the largest
first-order relative term, the rstd error of a row with mean 1000 and sigma 1, is below 2^-10). None is fitted.

The kernels. One wave per row; lane l holds the float4 chunks k = 0..NV-1 at columns (64 k + l) 4 .. + 3,
NV = ceil(D / 256); FULL (D == 256 NV) only drops the per-chunk guards. A row sum is: per lane and chunk
((a + b) + c) + d added to the lane's running sum (4 additions per chunk, so 4 NV deep), the 6-level xor butterfly,
one division by D: a sum of positives t has relative error (4 NV + 7) u, a general sum absolute error
(4 NV + 7) u mean|t|. hipcc may contract a product and a sum into one fma: that removes roundings, never adds one.

Forward, with a = x - mu, var = mean(a^2), rs = 1 / sqrt(var + eps), xh = a rs, y = xh gamma + beta:
    dmu  = (4 NV + 7) u mean|x|                                                         |mean - mu| <= dmu
    theta = (4 NV + 10) u      the centred value's rounding twice (it is squared), the square, the sum as above
    tau  = (dmu^2 + theta (var + dmu^2)) / (var + eps)     since mean((x - mu')^2) = var + (mu' - mu)^2 exactly
    rho  = tau (1 + tau) / 2 + 2.5 u      the addition of eps (u / 2 after the square root) and rsqrtf's 1 ulp = 2 u
                                                                                        |rstd - rs| <= rs rho
    |y - ref| <= |gamma| (rs dmu + |xh| rho) + 3 u |xh gamma| + u |y|
the last two terms: x - mu, (.) rs and (.) gamma, each u relative to xh gamma, and the addition of beta. A bf16 output
adds half a bf16 ulp of the reference (rigorous: if the f32 value lies in the binade above the reference's it is
within the f32 bound of that power of two and rounds to it).

Backward, with xh = (x - mean) rstd, g = dy gamma, m1 = mean(g), m2 = mean(g xh), I = g - m1 - xh m2,
dx = rstd I (+ dres):
    e_xh = 2 u |xh|  (the subtraction, the product);   e_g = u |g|
    dm1  = (4 NV + 8) u mean|g|         (g's rounding, the sum)
    dm2  = (4 NV + 11) u mean|g xh|     (g u + xh 2 u + the product u, the sum)
    e_I  = e_g + dm1 + |xh| dm2 + |m2| e_xh + u |xh m2| + u |g - m1| + u |I|
    |dx - ref| <= rstd e_I + u |rstd I| + u |dx|
The bf16 copy is the dropout-masked dx m (m = 0 or 1 / (1 - p)): m times that bound, u |dx m| for the product, half a
bf16 ulp. The three column sums add, per column, a term from each row: dy xh (3 u relative: e_xh and the product), dy
(exact) and dx m (its own bound, summed over the rows). A term passes through at most
    n_acc(rows) = rows-per-wave + 3 + (per + chunks + 16) + 1
additions: the wave's running sums over the rows it walks, the 4 waves of a block, vit_colsum over the nblk block
partials (chunks of `per` rows, summed in row order or as 8 row lanes of per / 8 and a sum of 8: at most per + 8,
then the chunks the same way: at most chunks + 8), and the accumulation onto the prior value:
    |sum - ref| <= (term count + n_acc) u (sum_rows |term| + |prior|)  + sum_rows (the term's own bound)
dbeta on integer-valued dy has only exact partial sums and is compared for equality.
"""
import math

import torch

import glue_ref as G

UF = G.UF
SLACK = 1.0 + 2.0 ** -9
LN_BWD_MAX_BLOCKS = 512

# every instantiation: D -> (NV, FULL), both sides of each FULL width
SWEEP_D = (4, 252, 256, 260, 508, 512, 516, 768, 772, 1024, 1028, 1280, 1284, 1536, 1540, 1792, 1796, 2044, 2048)
FAMILIES = ("wide", "bigmean", "tight")


def kernel_of(D):
    """(NV, FULL) of the kernel vit_layernorm_fwd / vit_layernorm_bwd launch for width D"""
    nv = (D + 255) // 256
    return nv, D == nv * 256


def bwd_blocks(rows):
    """workgroups of ln_bwd_kernel (4 rows each, capped): vit_layernorm_bwd_blocks"""
    return min(max((rows + 3) // 4, 1), LN_BWD_MAX_BLOCKS)


def n_acc(rows):
    """additions a row's term passes through on its way into a column sum (module docstring)"""
    nblk = bwd_blocks(rows)
    chunks, per = G.colsum_chunks(nblk)
    return -(-rows // (4 * nblk)) + 3 + (per + chunks + 16) + 1


def family(kind, rows, D, gen):
    """f32 [rows, D] inputs: wide = 3 N(0,1) + 1; bigmean = 1000 + N(0,1) (a one-pass variance cancels);
    tight = 5 + 1e-3 N(0,1) (variance 1e-6: eps = 1e-5 dominates rstd)"""
    z = torch.randn(rows, D, generator=gen)
    return {"wide": z * 3 + 1, "bigmean": z + 1000, "tight": z * 1e-3 + 5}[kind]


def half_ulp_bf16(ref):
    """half the bf16 spacing at |ref| (float64 in)"""
    return G.ulp32(ref) * 2.0 ** 15


def bf16_trunc(x):
    """f32 -> bf16 by dropping the low half (the planted fault), returned as f32"""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


class R:
    """a bag of float64 references and bounds"""


# ---- forward ---------------------------------------------------------------------------------------------------------
def fwd(x, gamma, beta, eps=1e-5):
    """mean, rstd [rows], xh, y [rows, D] and the gates b_mean, b_rstd [rows], b_y (f32 output), b_y16 (bf16 output)"""
    r = R()
    D = x.shape[1]
    nv, _ = kernel_of(D)
    eps = G.f32(eps)
    x, gm, bt = x.double(), gamma.double()[None, :], beta.double()[None, :]
    mu = x.mean(1, keepdim=True)
    a = x - mu
    var = (a * a).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    r.xh = a * rs
    r.y = r.xh * gm + bt
    dmu = (4 * nv + 7) * UF * x.abs().mean(1, keepdim=True)
    theta = (4 * nv + 10) * UF
    tau = (dmu * dmu + theta * (var + dmu * dmu)) / (var + eps)
    rho = tau * (1 + tau) / 2 + 2.5 * UF
    r.mean, r.rstd = mu[:, 0], rs[:, 0]
    r.b_mean, r.b_rstd = SLACK * dmu[:, 0], SLACK * (rs * rho)[:, 0]
    r.b_y = SLACK * (gm.abs() * (rs * dmu + r.xh.abs() * rho) + 3 * UF * (r.xh * gm).abs() + UF * r.y.abs())
    r.b_y16 = r.b_y + half_ulp_bf16(r.y)
    return r


def _lanes(t, nv, fill=0.0):
    """[rows, D] -> [rows, nv, 64, 4] in the kernels' chunk / lane order, columns past D holding `fill`"""
    rows, D = t.shape
    p = torch.full((rows, nv * 256), fill, dtype=t.dtype)
    p[:, :D] = t
    return p.view(rows, nv, 64, 4)


def _wave_sum(s):
    """the 6-level xor butterfly over [rows, 64] (every lane ends with the same bits): [rows, 1]"""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, idx ^ o]
    return s[:, :1]


def _row_sum(v):
    """a row sum of [rows, nv, 64, 4] in the kernels' order, before the division: [rows, 1]"""
    s = torch.zeros(v.shape[0], 64)
    for k in range(v.shape[1]):
        s = s + (((v[:, k, :, 0] + v[:, k, :, 1]) + v[:, k, :, 2]) + v[:, k, :, 3])
    return _wave_sum(s)


def fwd_emulate(x, gamma, beta, eps=1e-5, var_div=None, one_pass=False):
    """ln_fwd_kernel in f32 torch, in its own summation order and unfused: (y f32 before any pack, mean, rstd).
    Planted faults: var_div (the variance's divisor, D - 1), one_pass (E[x^2] - mu^2)"""
    rows, D = x.shape
    nv, _ = kernel_of(D)
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    v = _lanes(x, nv)
    live = _lanes(torch.ones_like(x), nv)
    mu = _row_sum(v) / t(D)
    if one_pass:
        var = _row_sum(v * v) / t(D) - mu * mu
    else:
        a = (v - mu[:, :, None, None]) * live
        var = _row_sum(a * a) / t(D if var_div is None else var_div)
    rs = torch.rsqrt(var + t(eps))
    y = ((x - mu) * rs) * gamma[None, :] + beta[None, :]
    return y, mu[:, 0], rs[:, 0]


# ---- backward --------------------------------------------------------------------------------------------------------
def bwd(dy, x, mean, rstd, gamma, dres=None, mult=None):
    """dx and its gate b_dx; dxm = dx mult (the bf16 copy's source) with b_dxm (as f32) and b_dx16 (after the pack);
    the per-row column-sum terms t_g = dy xh, t_b = dy, t_s = dxm"""
    r = R()
    D = x.shape[1]
    nv, _ = kernel_of(D)
    dy, x, gm = dy.double(), x.double(), gamma.double()[None, :]
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (x - mu) * rs
    g = dy * gm
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    inner = g - m1 - xh * m2
    r.dx = rs * inner if dres is None else rs * inner + dres.double()
    dm1 = (4 * nv + 8) * UF * g.abs().mean(1, keepdim=True)
    dm2 = (4 * nv + 11) * UF * (g * xh).abs().mean(1, keepdim=True)
    e_i = (UF * g.abs() + dm1 + xh.abs() * dm2 + 3 * UF * (xh * m2).abs() + UF * (g - m1).abs() + UF * inner.abs())
    r.b_dx = SLACK * (rs.abs() * e_i + UF * (rs * inner).abs() + UF * r.dx.abs())
    m = torch.ones_like(r.dx) if mult is None else mult.double()
    r.dxm = r.dx * m
    r.b_dxm = m * r.b_dx + SLACK * UF * r.dxm.abs()
    r.b_dx16 = r.b_dxm + half_ulp_bf16(r.dxm)
    r.t_g, r.t_b, r.t_s = dy * xh, dy, r.dxm
    return r


def colsums(r, rows, prior=None):
    """(dgamma, dbeta, dx_colsum) float64 [D] and their gates from bwd()'s terms; prior: the [3, D] values accumulated
    onto (dgamma, dbeta, dx_colsum)"""
    n = n_acc(rows)
    out, bounds = [], []
    for k, (t, own, cnt) in enumerate(((r.t_g, None, 3), (r.t_b, None, 0), (r.t_s, r.b_dxm, 0))):
        s, mag = t.sum(0), t.abs().sum(0)
        if prior is not None:
            s, mag = s + prior[k].double(), mag + prior[k].double().abs()
        b = SLACK * (cnt + n) * UF * mag
        out.append(s)
        bounds.append(b if own is None else b + own.sum(0))
    return out, bounds


def bwd_emulate(dy, x, mean, rstd, gamma, dres=None, mult=None, no_rs_chunk=None, m2_skip_last=False):
    """ln_bwd_kernel's row math in f32 torch, its own summation order, unfused: (dx, dxm = dx mult, dy xh).
    Planted faults: no_rs_chunk = k (chunk k's dx without the factor rstd), m2_skip_last (m2 without the last chunk)"""
    rows, D = x.shape
    nv, _ = kernel_of(D)
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    mu, rs = mean[:, None], rstd[:, None]
    xh = (x - mu) * rs
    g = dy * gamma[None, :]
    gx = g * xh
    if m2_skip_last:
        gx = gx.clone()
        gx[:, (nv - 1) * 256:] = 0.0
    m1 = _row_sum(_lanes(g, nv)) / t(D)
    m2 = _row_sum(_lanes(gx, nv)) / t(D)
    inner = (g - m1) - xh * m2
    o = rs * inner
    if no_rs_chunk is not None:
        c0 = no_rs_chunk * 256
        o[:, c0:c0 + 256] = inner[:, c0:c0 + 256]
    if dres is not None:
        o = o + dres
    return o, (o if mult is None else o * mult), dy * xh


def colsum_emulate(term, drop=None):
    """one column-sum of the backward in f32: each of the nblk x 4 waves adds its rows in turn, a block adds its
    4 waves, vit_colsum adds the block rows chunk by chunk. drop = (row, col): that row is left out of that column"""
    rows, D = term.shape
    if drop is not None:
        term = term.clone()
        term[drop[0], drop[1]] = 0.0
    nblk = bwd_blocks(rows)
    stride = nblk * 4
    acc = torch.zeros(stride, D)
    for r0 in range(0, rows, stride):
        n = min(stride, rows - r0)
        acc[:n] = acc[:n] + term[r0:r0 + n]
    w = acc.view(nblk, 4, D)
    blk = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    chunks, per = G.colsum_chunks(nblk)
    total = torch.zeros(D)
    for c in range(chunks):
        s = torch.zeros(D)
        for r in range(c * per, min((c + 1) * per, nblk)):
            s = s + blk[r]
        total = total + s
    return total
