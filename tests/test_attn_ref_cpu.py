"""The per-element attention gate of attn_ref.py, proved without a GPU: sound (the kernels' arithmetic, emulated
in f32 torch with their bf16 rounding points, passes it) and sharp (small planted faults that a whole-tensor
norm ratio lets through are flagged, and the flag names the item and row)."""
import math

import pytest
import torch

import attn_ref


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _inputs(B, N, H, hd, in_scale, seed=0, zero_q=False):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * N, 3, H, hd, generator=g) * in_scale).bfloat16()
    if zero_q:
        qkv[:, 0] = 0
    dout = torch.randn(B * N, H, hd, generator=g).bfloat16()
    return qkv, dout


def _all(e):
    return dict(o=e.o, lse=e.lse, dq=e.dq, dk=e.dk, dv=e.dv, bias=e.bias)


@pytest.mark.parametrize("B,N,H,hd,in_scale,zero_q", [
    (2, 1, 2, 16, 1.5, False), (2, 2, 2, 64, 1.5, False), (2, 197, 2, 64, 1.5, False), (2, 197, 2, 64, 8.0, False),
    (1, 320, 2, 96, 4.0, False), (1, 577, 2, 64, 3.0, False), (2, 50, 2, 48, 1.5, True)])
def test_gate_is_sound(B, N, H, hd, in_scale, zero_q):
    """the emulated kernel arithmetic stays inside the gate on every output, saturated scores (input scale 8)
    and q = 0 (uniform softmax, dk = 0 exactly) included"""
    sc = 1.0 / math.sqrt(hd)
    qkv, dout = _inputs(B, N, H, hd, in_scale, zero_q=zero_q)
    r = attn_ref.reference(qkv, dout, B, N, H, hd, sc)
    res = attn_ref.check(r, **_all(attn_ref.emulate_bf16(qkv, dout, B, N, H, hd, sc)))
    print({k: round(v[0], 3) for k, v in res.items()})
    assert not attn_ref.failures(res), attn_ref.failures(res)


def test_reference_matches_autograd():
    """the float64 reference is the softmax attention torch differentiates, q_rows form included"""
    B, N, H, hd, R = 2, 37, 2, 32, 17
    sc = 1.0 / math.sqrt(hd)
    qkv, dout = _inputs(B, N, H, hd, 1.5)
    for rows in (None, R):
        x = qkv.double().requires_grad_(True)
        q, k, v = attn_ref.split_qkv(x, B, N, H, hd)
        o = torch.softmax(sc * (q @ k.transpose(-1, -2)), -1) @ v
        dO = attn_ref.split_heads(dout, B, N, H, hd).double().clone()
        if rows:
            dO[:, :, rows:] = 0
        gq, gk, gv = attn_ref.split_qkv(torch.autograd.grad(o, x, dO)[0], B, N, H, hd)
        r = attn_ref.reference(qkv, dout, B, N, H, hd, sc, q_rows=rows)
        assert torch.allclose(r.o, o.detach()[:, :, :rows], rtol=1e-12, atol=1e-12)
        for got, ref in ((r.dq, gq), (r.dk, gk), (r.dv, gv)):
            assert torch.allclose(got, ref, rtol=1e-10, atol=1e-12)
        assert torch.allclose(r.bias[:, 0], gq.sum(2), rtol=1e-10, atol=1e-12)
        if rows:
            assert (r.dq[:, :, rows:] == 0).all() and r.o.shape[2] == rows and r.lse.shape[2] == rows


@pytest.fixture(scope="module")
def clean():
    B, N, H, hd = 4, 197, 4, 64
    sc = 1.0 / math.sqrt(hd)
    qkv, dout = _inputs(B, N, H, hd, 1.5, seed=1)
    r = attn_ref.reference(qkv, dout, B, N, H, hd, sc)
    e = attn_ref.emulate_bf16(qkv, dout, B, N, H, hd, sc)
    assert not attn_ref.failures(attn_ref.check(r, **_all(e)))
    return qkv, sc, r, e


def test_fault_dropped_key(clean):
    """one key left out of one item's softmax: o and lse of that item are flagged"""
    qkv, sc, r, e = clean
    B, N, H, hd = 4, 197, 4, 64
    b, h, key = 2, 1, 100
    q, k, v = (t.double() for t in attn_ref.split_qkv(qkv, B, N, H, hd))
    s = sc * (q[b, h] @ k[b, h].t())
    s[:, key] = -float("inf")
    o, lse = e.o.clone(), e.lse.clone()
    o[b, h] = (torch.softmax(s, -1) @ v[b, h]).bfloat16().float()
    lse[b, h] = torch.logsumexp(s, -1).float()
    res = attn_ref.check(r, o=o, lse=lse)
    for name in ("o", "lse"):
        ratio, loc = res[name]
        assert ratio > 1.0 and loc[:2] == (b, h), (name, ratio, loc)


def test_fault_last_keys_dv_zeroed(clean):
    """the dV rows of the last 5 keys of one item zeroed (a dropped tail of the last key tile)"""
    _, _, r, e = clean
    b, h = 1, 3
    dv = e.dv.clone()
    dv[b, h, -5:] = 0
    ratio, loc = attn_ref.check(r, dv=dv)["dv"]
    assert ratio > 1.0 and loc[:2] == (b, h) and loc[2] >= 197 - 5, (ratio, loc)


def test_fault_dq_row_zeroed(clean):
    """one dQ row zeroed (a typical one: the item's row of median norm; row norms spread by 2x either way):
    named by the per-element gate, invisible to the whole-tensor ratio at its 2e-2"""
    _, _, r, e = clean
    b, h = 3, 0
    row = int(r.dq[b, h].norm(dim=-1).argsort()[197 // 2])
    dq = e.dq.clone()
    dq[b, h, row] = 0
    ratio, loc = attn_ref.check(r, dq=dq)["dq"]
    assert ratio > 1.0 and loc[:3] == (b, h, row), (ratio, loc)
    assert rel(dq, r.dq) < 2e-2


def test_fault_o_rows_exchanged(clean):
    _, _, r, e = clean
    b, h, r0, r1 = 0, 2, 30, 31
    o = e.o.clone()
    o[b, h, r0], o[b, h, r1] = e.o[b, h, r1], e.o[b, h, r0]
    ratio, loc = attn_ref.check(r, o=o)["o"]
    assert ratio > 1.0 and loc[:2] == (b, h) and loc[2] in (r0, r1), (ratio, loc)


def test_fault_dv_item_scaled(clean):
    """one item's dV times 1.05: flagged per element, 1.3e-2 as a whole-tensor ratio"""
    _, _, r, e = clean
    b, h = 2, 2
    dv = e.dv.clone()
    dv[b, h] = (dv[b, h] * 1.05).bfloat16().float()
    ratio, loc = attn_ref.check(r, dv=dv)["dv"]
    assert ratio > 1.0 and loc[:2] == (b, h), (ratio, loc)
    assert rel(dv, r.dv) < 2e-2
