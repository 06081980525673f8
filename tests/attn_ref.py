"""Float64 reference of the attention kernels, the condition scales of every output, and a per-element gate.

A helper module, not a test file (the kernel tests import it as `attn_ref`); plain torch, so it runs on CPU
and GPU tensors alike.

Operands as the kernels take them: bf16 qkv [B*N, 3, H, hd] (q | k | v), bf16 dout [B*N, H, hd], scale.
Everything the reference returns is per (image, head): [B, H, rows, hd] (lse: [B, H, rows]; bias: [B, 3, H, hd]).

The gate (u = 2^-8, the bf16 unit roundoff; f = 2^-16, 256 f32 eps of slack), per element, never a norm:

    |o   - ref| <= 3u A_o                  A_o  = P |v|
    |dv  - ref| <= 3u A_dv                 A_dv = P^T |dO|
    |dq  - ref| <= 3u A_dq + f C_dq        A_dq = scale |dS| |k|,    C_dq = scale c |k|
    |dk  - ref| <= 3u A_dk + f C_dk        A_dk = scale |dS|^T |q|,  C_dk = scale c^T |q|,  c = P (|dP| + |delta|)
    |lse - ref| <= f max(1, S_abs)         S_abs[i] = max_j scale |q_i| . |k_j|
    |bias - ref| <= 2u sum_rows(A) + f sum_rows(C)   (the kernels sum the f32 values before the bf16 rounding)

3u is the worst-case forward error at the kernels' rounding points: P (or dS) rounded to bf16 gives u A, the
output rounded to bf16 u |out| <= u A, and one more u A covers the normaliser of o (the rounded P against the
unrounded row sum); the f terms cover f32 accumulation over at most 96 products per MFMA chain and the
cancellation in dP - delta. The bias partials skip the output rounding, hence 2u.
"""
import torch

U = 2.0 ** -8
F = 2.0 ** -16


def split_qkv(qkv, B, N, H, hd):
    """[B*N, 3, H, hd] (any dtype, any view of it) -> q, k, v as [B, H, N, hd]"""
    return qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)


def split_heads(x, B, N, H, hd):
    """[B*N, H, hd] -> [B, H, N, hd]"""
    return x.reshape(B, N, H, hd).permute(0, 2, 1, 3)


def split_bias(bias, B, H, hd):
    """per-image column sums [B, 3*H*hd] -> [B, 3, H, hd]"""
    return bias.reshape(B, 3, H, hd)


class Ref:
    """float64 outputs (o, lse, dq, dk, dv, bias) and the scales of their gates (A_*, C_*, S_abs)"""


def forward_reference(q, k, v, scale):
    """o, lse and their scales for queries q [..., R, hd] against keys / values k, v [..., N, hd] (the ragged
    forward: a sample's own queries against all its keys); returns the Ref and P"""
    q, k, v = q.double(), k.double(), v.double()
    r = Ref()
    s = scale * (q @ k.transpose(-1, -2))
    r.lse = torch.logsumexp(s, -1)
    P = torch.exp(s - r.lse[..., None])
    r.o = P @ v
    r.A_o = P @ v.abs()
    r.S_abs = scale * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1)
    return r, P


def reference(qkv, dout, B, N, H, hd, scale, q_rows=None):
    """q_rows: only queries [0, q_rows) exist (o / lse have q_rows rows; dq keeps N rows, zero past them, and
    the rows of dout past them are not read). dout None: forward only."""
    q, k, v = (t.double() for t in split_qkv(qkv, B, N, H, hd))
    R = N if q_rows is None else q_rows
    q = q[:, :, :R]
    r, P = forward_reference(q, k, v, scale)
    if dout is None:
        return r
    dO = split_heads(dout, B, N, H, hd).double()[:, :, :R]
    dP = dO @ v.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    c = P * (dP.abs() + delta.abs())
    pad = lambda t: torch.cat([t, t.new_zeros(B, H, N - R, hd)], 2) if R < N else t
    r.dq = pad(scale * (dS @ k))
    r.dk = scale * (dS.transpose(-1, -2) @ q)
    r.dv = P.transpose(-1, -2) @ dO
    r.A_dq = pad(scale * (dS.abs() @ k.abs()))
    r.A_dk = scale * (dS.abs().transpose(-1, -2) @ q.abs())
    r.A_dv = P.transpose(-1, -2) @ dO.abs()
    r.C_dq = pad(scale * (c @ k.abs()))
    r.C_dk = scale * (c.transpose(-1, -2) @ q.abs())
    r.bias = torch.stack([r.dq.sum(2), r.dk.sum(2), r.dv.sum(2)], 1)
    zero = torch.zeros_like(r.A_dv).sum(2)
    r.A_bias = torch.stack([r.A_dq.sum(2), r.A_dk.sum(2), r.A_dv.sum(2)], 1)
    r.C_bias = torch.stack([r.C_dq.sum(2), r.C_dk.sum(2), zero], 1)
    return r


def bounds(r, o_factor=3 * U):
    """name -> the per-element bound of the gate (o_factor: f for the f32-operand forward, which rounds nothing)"""
    b = {"o": o_factor * r.A_o, "lse": F * r.S_abs.clamp_min(1.0)}
    if hasattr(r, "dq"):
        b.update(dq=3 * U * r.A_dq + F * r.C_dq, dk=3 * U * r.A_dk + F * r.C_dk, dv=3 * U * r.A_dv,
                 bias=2 * U * r.A_bias + F * r.C_bias)
    return b


def worst(got, ref, bound):
    """the largest |got - ref| / bound and where: (ratio, index tuple). An element whose bound is 0 must be
    exact; a NaN counts as infinite."""
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


def check(r, o_factor=3 * U, **got):
    """got: any of o, lse, dq, dk, dv ([B, H, rows, hd]; lse [B, H, rows]) and bias ([B, 3, H, hd]), rows cut to
    the reference's. Returns name -> (worst ratio, (image, head, row, column)); lse has no column, and bias
    reports (image, dq | dk | dv, head, column)."""
    bd = bounds(r, o_factor)
    return {name: worst(t, getattr(r, name), bd[name]) for name, t in got.items()}


def failures(res, tag=""):
    """the entries of check()'s result past the gate, as readable strings"""
    return [f"{tag}{name}: {ratio:.3g} x gate at (image, head, row, col) {loc}" for name, (ratio, loc) in res.items()
            if not ratio <= 1.0]


def emulate_bf16(qkv, dout, B, N, H, hd, scale):
    """The kernels' arithmetic in f32 torch with their rounding points: P to bf16 (against the f32 row max, the
    row sum taken of the unrounded values), dS to bf16, outputs to bf16, bias sums of the unrounded f32 values.
    Only the CPU test of the gate uses it; no kernel is ever compared with it."""
    bf = lambda t: t.bfloat16().float()
    q, k, v = (t.float() for t in split_qkv(qkv, B, N, H, hd))
    dO = split_heads(dout, B, N, H, hd).float()
    s = scale * (q @ k.transpose(-1, -2))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    e = Ref()
    e.lse = (m + torch.log(l))[..., 0]
    e.o = bf((bf(p) @ v) / l)
    P = torch.exp(s - e.lse[..., None])
    dP = dO @ v.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = bf(P * (dP - delta))
    dq = scale * (dS @ k)
    dk = scale * (dS.transpose(-1, -2) @ q)
    dv = bf(P).transpose(-1, -2) @ dO
    e.bias = torch.stack([dq.sum(2), dk.sum(2), dv.sum(2)], 1)
    e.dq, e.dk, e.dv = bf(dq), bf(dk), bf(dv)
    return e
