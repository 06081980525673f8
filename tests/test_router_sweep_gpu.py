"""The Res-ViT router kernels (csrc/elementwise.hip from segment_colsum_kernel on) through vitmi.ops against
glue_ref.py's references, at the edges of their loops: segment sums on exact integers (equal), the gated data
gradient as bit patterns with exact 32-row partials, the routing masks (equal), the router head forward and backward
per element against float64 within bounds counted from their roundings ("RATIO name value", visible with pytest -s).

Inputs sit in NaN-padded buffers, outputs (where the caller allocates them) in NaN-filled ones whose padding must
stay NaN."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import glue_ref as G
from vitmi import ops

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _same(name, got, want, fails, tag="", **kw):
    d = G.first_diff(got, want.to(got.device), **kw)
    if d is not None:
        fails.append(f"{name}{tag}: at {d[0]} got {d[1]!r}, want {d[2]!r}")


def _guards(name, flat, views, fails, tag=""):
    at = G.first_touched(flat, *views)
    if at is not None:
        fails.append(f"{name}{tag}: guard element {at} of the buffer was written")


def _nan_out(rows, cols, ld, dtype=F32):
    return G.embed(torch.full((rows, cols), G.NAN, device=DEV, dtype=dtype), ld, extra_rows=1)


# ---- vit_segment_colsum / _bcast: exact integers -----------------------------------------------------------------------
SEG_ROWS = [0, 1, 3, 4, 5, 12, 13, 15, 16, 17, 29, 33]      # both sides of `r + 12 < seg_rows` for every row lane
SEG_COLS = [1, 2, 3, 127, 128, 129, 255]                    # the half-empty last pair, the second column block


@pytest.mark.parametrize("seg_rows", SEG_ROWS)
def test_segment_colsum(seg_rows):
    G.assert_exact_sum(seg_rows, 8)
    fails = []
    row0, scale = 2, 0.25
    seg_stride = row0 + seg_rows + 3
    for cols in SEG_COLS:
        ld = cols + (cols % 2) + 2
        for segs in (1, 3):
            x = G.ints((segs * seg_stride, cols), _gen(seg_rows * 1000 + cols + segs))
            want = G.segment_colsum(x, segs, seg_rows, seg_stride, row0, scale).float()
            for dt in (F32, BF16):
                # rows outside [row0, row0 + seg_rows) of every segment are never read: NaN
                xin = x.clone()
                for s in range(segs):
                    xin[s * seg_stride:s * seg_stride + row0] = G.NAN
                    xin[s * seg_stride + row0 + seg_rows:(s + 1) * seg_stride] = G.NAN
                _, view = G.embed(xin.to(DEV).to(dt), ld)
                tag = f" [cols {cols} segs {segs} {dt}]"
                oflat, out = _nan_out(segs, cols, cols + 3)
                ops.segment_colsum(view, ld, segs, seg_rows, cols, out, cols + 3, seg_stride=seg_stride, row0=row0,
                                   scale=scale)
                _same("segment_colsum", out, want, fails, tag)
                _guards("segment_colsum out", oflat, [out], fails, tag)
                for bc_rows in (0, 1, 3, 4, 5, seg_stride):
                    # bc is the right half of a shared buffer: the left half, the rows past bc_rows and the columns past
                    # cols keep every bit
                    ldbc = 2 * cols + (2 * cols) % 2 + 2
                    left = cols + cols % 2
                    shared = G.ints((segs * seg_stride, ldbc), _gen(bc_rows)).to(DEV).to(BF16)
                    before = shared.clone()
                    oflat, out = _nan_out(segs, cols, cols + 3)
                    bc = shared[:, left:]
                    ops.segment_colsum_bcast(view, ld, segs, seg_rows, cols, out, cols + 3, bc, ldbc, bc_rows,
                                             seg_stride=seg_stride, row0=row0, scale=scale)
                    btag = tag + f" bc_rows {bc_rows}"
                    _same("segment_colsum_bcast out", out, want, fails, btag)
                    _guards("segment_colsum_bcast out", oflat, [out], fails, btag)
                    expect = before.clone()
                    for s in range(segs):
                        expect[s * seg_stride:s * seg_stride + bc_rows, left:left + cols] = want[s].to(DEV).to(BF16)
                    _same("segment_colsum_bcast bc", shared, expect, fails, btag, bits=True)
    assert not fails, fails[:8]


# ---- vit_router_dx_gate ------------------------------------------------------------------------------------------------
# (cols, cols_pad): odd -> the generic kernel; even with cols_pad > cols -> the generic kernel; even and equal -> the
# pair kernel; 514 -> a second column block (both kernels)
RDG_COLS = [(5, 6), (6, 8), (8, 8), (514, 514), (513, 514)]


def _rows_pads(T):
    up = -(-T // 32) * 32
    return sorted({T, T + 3, up, up + 32})


@pytest.mark.parametrize("T", [1, 7, 8, 9, 31, 32, 33, 65])
def test_router_dx_gate(T):
    fails = []
    for N in (1, 3, 5, 50):
        for cols, cols_pad in RDG_COLS:
            if cols > 500 and N != 3:
                continue
            imgs = -(-T // N)
            for kind in ("real", "ints"):
                g0 = _gen(T * 100 + N * 10 + cols)
                if kind == "ints":       # every value a multiple of 1/2 below 64: bf16 holds it, the partials are exact
                    dx, g = G.ints((T, cols), g0), G.ints((imgs, cols), g0)
                    gp, scale = G.ints((T, cols_pad), g0, -4, 4).to(BF16), 0.5
                    G.assert_exact_sum(32, 2 * 48)
                else:
                    dx, g = torch.randn(T, cols, generator=g0), torch.randn(imgs, cols, generator=g0)
                    gp, scale = torch.randn(T, cols_pad, generator=g0).to(BF16), 0.3
                gp[:, cols:] = G.NAN          # gp is as wide as the padded output; its padding is not used
                ldx, ldg = cols + cols % 2 + 2, cols + cols % 2 + 4
                _, dxv = G.embed(dx.to(DEV), ldx)
                _, gv = G.embed(g.to(DEV), ldg)
                _, gpv = G.embed(gp.to(DEV), cols_pad + 2)
                for rows_pad in _rows_pads(T):
                    for reserve in sorted({0, 1, N}):
                        for with_partial in (True, False) if reserve == 0 else (True,):
                            tag = f" [N {N} cols {cols}/{cols_pad} {kind} rows_pad {rows_pad} reserve {reserve}]"
                            want, wpart = G.router_dx_gate(dx, g, scale, gp[:, :cols], T, N, reserve, rows_pad, cols_pad)
                            oflat, out = _nan_out(rows_pad, cols_pad, cols_pad + 2, BF16)
                            nblk = ops.router_dx_gate_partial_rows(rows_pad)
                            assert nblk == wpart.shape[0]
                            pflat, part = _nan_out(nblk, cols, cols + 3)
                            ops.router_dx_gate(dxv, ldx, gv, ldg, scale, gpv, cols_pad + 2, T, N, reserve, cols, out,
                                               cols_pad + 2, col_partial=part if with_partial else None, ldp=cols + 3)
                            _same("router_dx_gate out", out, want, fails, tag, bits=True)
                            _guards("router_dx_gate out", oflat, [out], fails, tag)
                            if with_partial and kind == "ints":
                                _same("router_dx_gate partial", part, wpart.float(), fails, tag)
                            _guards("router_dx_gate partial", pflat, [part] if with_partial else [part[:, :0]], fails,
                                    tag)
    assert not fails, fails[:8]


# ---- vit_router_select -------------------------------------------------------------------------------------------------
SETS8 = [{0, 3, 31}, {1}, set(), {5, 7, 13}, set(range(32)), {30, 31}, {12}, {0}]


@pytest.mark.parametrize("T", [1, 3, 4, 5, 4096, 4100, 4101])
def test_router_select(T):
    fails = []
    idx = G.router_select_case(T, _gen(T))
    assert int((idx == 13.0).sum()) == 1 and float(idx[-1]) == 13.0       # a key present only in the last token
    for offset in (0, 1):            # one element off 16-B alignment: the 4-token vector path must fall back
        flat = torch.full((T + offset + 8,), G.NAN, device=DEV)
        view = flat[offset:offset + T]
        view.copy_(idx)
        for sets, nkeys in ((SETS8, 32), (SETS8[:2], 0), ([], 14)):
            tag = f" [offset {offset} npos {len(sets)} nkeys {nkeys}]"
            active, sel, anyf = ops.router_select(view, sets, nkeys)
            want = G.router_select(idx, sets, nkeys)
            for name, got, w in zip(("active", "sel", "any"), (active, sel, anyf), want):
                if got.numel() or w.numel():
                    assert got.shape == w.shape, (name, got.shape, w.shape)
                    if not torch.equal(got.cpu(), w):
                        at = (got.cpu() != w).nonzero()[0].tolist()
                        fails.append(f"router_select {name}{tag}: first difference at {at}")
            if nkeys > 13:
                assert bool(want[2][13]) and (T == 1 or not bool(want[1][13, :-1].any()))
    assert not fails, fails[:8]


# ---- vit_router_head_fwd / _bwd: per element against float64 -----------------------------------------------------------
# (noise_mode, training, y_hard given)
HEAD_FORMS = [(0, False, False), (0, False, True), (0, True, False), (1, True, False), (2, True, False), (1, True, True)]


def _dev(t):
    """a dense device copy with NaN behind it (None stays None)"""
    if t is None:
        return None
    flat = torch.full((t.numel() + 8,), G.NAN, device=DEV)
    v = flat[:t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("bs", [1, 2, 8])
@pytest.mark.parametrize("T", [1, 255, 256, 257, 513])
def test_router_head(T, bs):
    fails, worst = [], {}
    norm = 100.0

    def gate(name, got, ref, bound, tag):
        ratio, at = G.worst(got.cpu(), ref, bound)
        worst[name] = max(worst.get(name, 0.0), ratio)
        if not ratio <= 1.0:
            fails.append(f"{name}{tag}: {ratio:.4g} x gate at {at}")

    N = min(5, T)
    for reserve in sorted({0, 1, N}):
        for mode, training, yh in HEAD_FORMS:
            g = _gen(T * 1000 + bs * 10 + mode + reserve)
            tag = f" [reserve {reserve} mode {mode} training {training} y_hard {yh}]"
            x = G.router_head_logits(T, bs, g)
            noise = G.router_head_noise(T, bs, mode, g) if mode else None
            yhard = None
            if yh:
                h1 = torch.randint(0, 2, (T, bs), generator=g).float()
                yhard = torch.stack([1 - h1, h1], -1)
            r = G.router_head_fwd(x, noise, mode, yhard, N, reserve, training, norm)
            assert float((~r.decided).double().mean()) <= 0.01
            soft, ysoft, hard, idx, ent = ops.router_head_fwd(_dev(x), _dev(noise), mode, _dev(yhard), N, reserve,
                                                              training, norm)
            gate("soft", soft, r.soft, r.b_soft, tag)
            if training:
                gate("ysoft", ysoft, r.ysoft, r.b_ysoft, tag)
            else:
                assert ysoft is None
            hard_c = torch.where(r.decided[..., None], hard.cpu().double(), r.hard)
            idx_c = torch.where(r.idx_decided, idx.cpu().double(), r.indices)
            gate("hard", hard_c, r.hard, r.b_hard, tag)
            gate("indices", idx_c, r.indices, r.b_idx, tag)
            gate("entropy", ent.reshape(1), r.ent.reshape(1), r.b_ent.reshape(1), tag)
            # the backward reads the f32 soft / ysoft the forward wrote
            grads = [torch.randn(T, bs, 2, generator=g), torch.randn(T, bs, 2, generator=g),
                     torch.randn(T, generator=g), torch.randn((), generator=g)]
            for drop in range(5):
                a = [None if k == drop else t for k, t in enumerate(grads)]
                ref, bound = G.router_head_bwd(soft.cpu(), None if ysoft is None else ysoft.cpu(), *a, N, reserve,
                                               training, norm)
                dl = ops.router_head_bwd(soft, ysoft, *[_dev(t) for t in a], N, reserve, training, norm)
                gate("dlogits", dl, ref, bound, tag + f" gradient {drop} absent")
    for name, v in worst.items():
        print(f"RATIO router_head_{name}_T{T}_bs{bs} {v:.4g}")
    assert not fails, fails[:8]
