"""Every 16-key tile count of the attention kernels, and every q_rows form, against the float64 reference of
attn_ref.py under its per-element gate (GPU only)."""
import math

import pytest
import torch

import attn_ref
from vitmi import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H = 2, 2  # image and head offsets both non-trivial
NAN = float("nan")


def _tokens(path):
    ns = sorted({n for t in range(1, 21) for n in (16 * t - 15, 16 * t)})
    return ns + [321, 385] if path == ops.ATTN_TILED else ns


def _inputs(g, N, hd):
    qkv = (torch.randn(B * N, 3, H, hd, device=DEV, generator=g) * 1.5).bfloat16()
    dout = torch.randn(B * N, H, hd, device=DEV, generator=g).bfloat16()
    return qkv, dout


def _forward(qkv, N, hd, path, q_rows=None):
    o = torch.full((B * N, H, hd), NAN, device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B, H, N), NAN, device=DEV)
    ops.attention_fwd(qkv, o, lse, B, N, H, hd, 1.0 / math.sqrt(hd), q_rows=q_rows, path=path)
    return o, lse


def _backward(qkv, o, dout, lse, N, hd, path, q_rows=None):
    dqkv = torch.full((B * N, 3, H, hd), NAN, device=DEV, dtype=torch.bfloat16)
    bpart = torch.full((B * ops.attention_bias_rows(N, hd, path), 3 * H * hd), NAN, device=DEV)
    ops.attention_bwd(qkv, o, dout, lse, dqkv, B, N, H, hd, 1.0 / math.sqrt(hd), bias_partial=bpart, q_rows=q_rows,
                      path=path)
    return dqkv, bpart


def _gate(r, o, lse, dqkv, bpart, N, hd, rows=None):
    """check()'s result for the kernels' buffers (o / lse cut to the reference's `rows`)"""
    dq, dk, dv = attn_ref.split_qkv(dqkv, B, N, H, hd)
    bias = attn_ref.split_bias(bpart.view(B, -1, 3 * H * hd).double().sum(1), B, H, hd)
    return attn_ref.check(r, o=attn_ref.split_heads(o, B, N, H, hd)[:, :, :rows], lse=lse[:, :, :rows], dq=dq, dk=dk,
                          dv=dv, bias=bias)


@pytest.mark.parametrize("path", [ops.ATTN_AUTO, ops.ATTN_ONESHOT, ops.ATTN_TILED], ids=["auto", "oneshot", "tiled"])
@pytest.mark.parametrize("hd", [16, 32, 48, 64, 80, 96])
def test_attention_tile_count_sweep(hd, path):
    """The first and the last token count of every 16-key tile count 1..20 (N = 16 t - 15 and 16 t; the tiled
    path also 321 and 385): every instantiation of the persistent kernels (tile counts 1..20 at width 32, 1..13
    at width 64), of the two-stage kernels (even counts 2..20 and their NKT - 1 forms) and every dispatch boundary
    between them (N = 208 / 209 at hd 64, 256 / 257 at hd 32, 320 / 321), on B = 2 x H = 2 items. Per N:
    forward, then backward from the kernel's own o / lse, into NaN-filled buffers; o, lse, dq, dk, dv and the
    summed bias partials under the per-element float64 gate, no NaN left, and a second backward bit-identical.
    Every failing (N, output) is collected and reported together; an error raised by a launch ends the test at
    once.

    LDS: the largest dynamic request of the swept shapes is the two-stage backward at hd 96, N = 305..320
    (2 x 20 x 16 x 96 x 2 + 2 x 20 x 16 x 4 + 4 x 3 x 96 x 4 = 130 048 B); the largest of all is the persistent
    backward's static 162 624 B at hd 64, N = 193..208 (6 images of 208 x 64 bf16 + 2 lse slots + delta), under
    the 160 KiB (163 840 B) of a CU."""
    g = torch.Generator(device=DEV).manual_seed(1000 * hd + path)
    sc = 1.0 / math.sqrt(hd)
    bad, top = [], {}
    for N in _tokens(path):
        qkv, dout = _inputs(g, N, hd)
        o, lse = _forward(qkv, N, hd, path)
        dqkv, bpart = _backward(qkv, o, dout, lse, N, hd, path)
        dqkv2, bpart2 = _backward(qkv, o, dout, lse, N, hd, path)
        torch.cuda.synchronize()
        res = _gate(attn_ref.reference(qkv, dout, B, N, H, hd, sc), o, lse, dqkv, bpart, N, hd)
        bad += attn_ref.failures(res, f"N={N} ")
        for name, (ratio, _) in res.items():
            top[name] = max(top.get(name, 0.0), ratio)
        for name, t in (("o", o), ("lse", lse), ("dqkv", dqkv), ("bias partials", bpart)):
            if torch.isnan(t.float()).any():
                bad.append(f"N={N} {name}: NaN left")
        # (bit patterns: NaN == NaN there)
        if not (torch.equal(dqkv.view(torch.int16), dqkv2.view(torch.int16))
                and torch.equal(bpart.view(torch.int32), bpart2.view(torch.int32))):
            bad.append(f"N={N}: the backward differs run to run")
    print(f"\nattention sweep hd={hd} path={path}: worst ratio to the gate "
          + " ".join(f"{k}={v:.3f}" for k, v in top.items()))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("N,hd,path", [(99, 64, ops.ATTN_AUTO), (197, 64, ops.ATTN_AUTO), (257, 80, ops.ATTN_AUTO),
                                       (300, 32, ops.ATTN_AUTO), (337, 64, ops.ATTN_AUTO), (197, 64, ops.ATTN_TILED)])
def test_attention_query_rows_sweep(N, hd, path):
    """q_rows in {1, 16, 17, 32, 33, 64, 65, N - 1, N} (below, at and past the 16-row strips, the 32-row pairs
    and the tiled path's 64-row blocks). Forward: rows [0, q_rows) of o / lse bit-identical to the full run's
    and inside the gate (nothing is promised of the rows past them). Backward with dO zero on rows >= q_rows:
    dq, dk, dv and the bias partials bit-identical to the full backward's on the same dO and inside the gate,
    and the dQ rows >= q_rows exactly 0 (the buffers start as NaN); the same bits again when the backward is fed
    by the q_rows forward's own o / lse (NaN in every row that forward left alone), as the engine's last layer
    pairs the two."""
    g = torch.Generator(device=DEV).manual_seed(7000 + N)
    sc = 1.0 / math.sqrt(hd)
    qkv, dout_all = _inputs(g, N, hd)
    o_f, l_f = _forward(qkv, N, hd, path)
    bad = []
    for qr in sorted({1, 16, 17, 32, 33, 64, 65, N - 1, N}):
        o_r, l_r = _forward(qkv, N, hd, path, q_rows=qr)
        dout = dout_all.clone().view(B, N, H, hd)
        dout[:, qr:] = 0
        dout = dout.view(B * N, H, hd)
        g_f, b_f = _backward(qkv, o_f, dout, l_f, N, hd, path)
        g_r, b_r = _backward(qkv, o_f, dout, l_f, N, hd, path, q_rows=qr)
        # as the engine pairs them: fed by the q_rows forward's own o / lse, NaN wherever that wrote nothing
        g_o, b_o = _backward(qkv, o_r, dout, l_r, N, hd, path, q_rows=qr)
        torch.cuda.synchronize()
        if not (torch.equal(g_o, g_r) and torch.equal(b_o, b_r)):
            bad.append(f"q_rows={qr}: the backward reads o / lse rows that the q_rows forward does not write")
        if not (torch.equal(o_f.view(B, N, -1)[:, :qr], o_r.view(B, N, -1)[:, :qr])
                and torch.equal(l_f[:, :, :qr], l_r[:, :, :qr])):
            bad.append(f"q_rows={qr}: o / lse differ from the full forward's")
        if not torch.equal(g_f, g_r):  # (a NaN anywhere fails this too)
            bad.append(f"q_rows={qr}: dqkv differs from the full backward's")
        if not torch.equal(b_f, b_r):
            bad.append(f"q_rows={qr}: bias partials differ from the full backward's")
        if not (attn_ref.split_qkv(g_r, B, N, H, hd)[0][:, :, qr:].float() == 0).all():
            bad.append(f"q_rows={qr}: dQ rows past q_rows are not 0")
        r = attn_ref.reference(qkv, dout, B, N, H, hd, sc, q_rows=qr)
        bad += attn_ref.failures(_gate(r, o_r, l_r, g_r, b_r, N, hd, rows=qr), f"q_rows={qr} ")
    assert not bad, "\n".join(bad)
