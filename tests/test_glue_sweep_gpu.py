"""The step's glue kernels (csrc/elementwise.hip, csrc/optim.hip) through vitmi.ops, every output element against
glue_ref.py's float64 references: reductions and the f32 GEMM on exact integers (equal), casts and moves (bit
patterns), GELU / cross entropy / cls-MSE backward / SGD / AdamW within bounds counted from their roundings.

Inputs sit in NaN-padded buffers (padding must never be read: a NaN would reach the output), outputs in NaN-filled
ones (guard columns, alignment gaps and rows past the end must stay NaN). Bounded gates print their worst ratio
("RATIO name value", visible with pytest -s)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import glue_ref as G
from vitmi import ops

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
GUARD = 8


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _nan(n, dtype=F32):
    return torch.full((n,), G.NAN, device=DEV, dtype=dtype)


def _out(n, prior=None, dtype=F32):
    """an n-element output inside a NaN-filled buffer with a guard behind it (prior: the values to accumulate onto;
    without them the output itself is NaN, so a kernel that reads instead of overwriting shows): (flat, view)"""
    flat = _nan(n + GUARD, dtype)
    if prior is not None:
        flat[:n] = prior.to(DEV)
    return flat, flat[:n]


def _dense(t, dtype=None, offset=0):
    """a contiguous tensor inside a NaN-filled buffer: NaN before (offset) and behind it"""
    t = t.to(DEV) if dtype is None else t.to(DEV).to(dtype)
    flat = _nan(offset + t.numel() + GUARD, t.dtype)
    v = flat[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    return flat, v


def _report(name, ratio):
    print(f"RATIO {name} {ratio:.4g}")


def _bounded(name, got, ref, bound, fails, tag=""):
    ratio, at = G.worst(got, ref.to(got.device), bound.to(got.device))
    if not ratio <= 1.0:
        fails.append(f"{name}{tag}: {ratio:.3g} x gate at {at}")
    return ratio


def _same(name, got, want, fails, tag="", **kw):
    d = G.first_diff(got, want.to(got.device), **kw)
    if d is not None:
        fails.append(f"{name}{tag}: at {d[0]} got {d[1]!r}, want {d[2]!r}")


def _guards(name, flat, views, fails, tag=""):
    at = G.first_touched(flat, *views)
    if at is not None:
        fails.append(f"{name}{tag}: guard element {at} of the buffer was written")


# ---- 1. reductions: exact integers ----------------------------------------------------------------------------------
COLSUM_ROWS = [1, 63, 64, 127, 128, 129, 200, 4225]
# (cols, ld, offset): the vector path (8-column groups: one block of 32 groups at 256, a second block with one group
# at 264), the scalar path (across a 256-thread block at 257), and two vector-eligible widths that must fall back to
# the scalar path: the input one element off its alignment, and ld % 8 == 4
COLSUM_COLS = [(8, 16, 0), (256, 264, 0), (264, 272, 0), (1000, 1008, 0),
               (1, 4, 0), (10, 13, 0), (100, 103, 0), (257, 260, 0),
               (264, 272, 1), (264, 268, 0)]


@pytest.mark.parametrize("rows", COLSUM_ROWS)
def test_colsum(rows):
    G.assert_exact_sum(rows, 8, start=8)
    fails = []
    chunks = ops.colsum_partial_rows(rows)
    assert chunks == G.colsum_chunks(rows)[0]
    for cols, ld, offset in COLSUM_COLS:
        x = G.ints((rows, cols), _gen(rows * 1000 + cols))
        prior = G.ints((cols,), _gen(cols))
        for dt in (F32, BF16):
            flat, view = G.embed(x.to(DEV).to(dt), ld, offset=offset)
            for acc in (False, True):
                tag = f" [cols {cols} ld {ld} offset {offset} {dt} acc {acc}]"
                pflat, _ = _out(chunks * cols)
                oflat, out = _out(cols, prior if acc else None)
                ops.colsum(view, rows, cols, ld, pflat, out, accumulate=acc)
                _same("colsum", out, G.colsum(x, prior if acc else None).float(), fails, tag)
                _guards("colsum out", oflat, [out], fails, tag)
                _guards("colsum partial", pflat, [pflat[:chunks * cols]], fails, tag)
    assert not fails, fails[:8]


@pytest.mark.parametrize("rows", [40, 200])
@pytest.mark.parametrize("seg", [8, 104])
def test_colsum3(rows, seg):
    cols, ld = 3 * seg, 3 * seg + 8
    G.assert_exact_sum(rows, 8, start=8)
    chunks = ops.colsum_partial_rows(rows)
    x = G.ints((rows, cols), _gen(rows + seg))
    prior = G.ints((3, seg), _gen(1))
    fails = []
    for dt in (F32, BF16):
        _, view = G.embed(x.to(DEV).to(dt), ld)
        for acc in (False, True):
            for drop1 in (False, True):
                tag = f" [{dt} acc {acc} out1 dropped {drop1}]"
                pflat, _ = _out(chunks * cols)
                bufs = [_out(seg, prior[k] if acc else None) for k in range(3)]
                outs = [b[1] for b in bufs]
                ops.colsum3(view, rows, seg, ld, pflat, outs[0], None if drop1 else outs[1], outs[2], accumulate=acc)
                for k in range(3):
                    if k == 1 and drop1:
                        want = prior[1] if acc else torch.full((seg,), G.NAN)            # untouched
                    else:
                        want = G.colsum(x[:, k * seg:(k + 1) * seg], prior[k] if acc else None).float()
                    _same(f"colsum3 out{k}", outs[k], want, fails, tag)
                    _guards(f"colsum3 out{k}", bufs[k][0], [outs[k]], fails, tag)
                _guards("colsum3 partial", pflat, [pflat[:chunks * cols]], fails, tag)
    assert not fails, fails[:8]


COLSUM_BATCH_ROWS = [1, 15, 16, 17, 113, 128, 129, 241]   # the unrolled `r + 112 < rows` loop: 0, 1, 2 passes, +- a rest


@pytest.mark.parametrize("cols,ld", [(4, 8), (63, 66), (64, 68), (65, 68)])
def test_colsum_batch_row_loops(cols, ld):
    """one launch of eight jobs, one per row count; (4, 8) and (64, 68) take the 16-B loads, the others scalar loads"""
    fails, jobs, keep = [], [], []
    for k, rows in enumerate(COLSUM_BATCH_ROWS):
        x = G.ints((rows, cols), _gen(rows * 100 + cols))
        prior = G.ints((cols,), _gen(rows))
        acc = k % 2 == 1
        _, view = G.embed(x.to(DEV), ld)
        oflat, out = _out(cols, prior if acc else None)
        jobs.append((view, rows, cols, ld, 0, (out,), acc))
        keep.append((rows, x, prior if acc else None, oflat, out))
    ops.colsum_batch(jobs)
    for rows, x, prior, oflat, out in keep:
        _same("colsum_batch", out, G.colsum(x, prior).float(), fails, f" [rows {rows}]")
        _guards("colsum_batch out", oflat, [out], fails, f" [rows {rows}]")
    assert not fails, fails[:8]


# (B, N, D, offset of dh0 in elements, dropout). D picks the launch: 4 one float4 column, 8, 388 = 4 x 97 (prime: 97
# slices of 8 threads), 768 (768-thread blocks), 772 = 4 x 193, 1280; 6 and 300 the scalar kernel (300 across a
# 256-thread block); D = 8 one element off its alignment falls back to it. B against the 8 image groups; N = 1 is the
# cls row alone, N >= 256 changes the slice rule. Every value of B, N runs on both kernels.
EMBED_GRAD_CASES = [(1, 1, 4, 0, False), (7, 2, 8, 0, False), (8, 17, 388, 0, True), (9, 257, 768, 0, False),
                    (17, 17, 772, 0, False), (8, 2, 1280, 0, False), (9, 257, 8, 0, False), (17, 1, 768, 0, False),
                    (1, 1, 6, 0, False), (7, 2, 300, 0, True), (8, 17, 6, 0, False), (9, 257, 6, 0, False),
                    (17, 17, 300, 0, False), (17, 2, 8, 1, False)]


@pytest.mark.parametrize("B,N,D,offset,drop", EMBED_GRAD_CASES)
def test_embed_grad(B, N, D, offset, drop):
    G.assert_exact_sum(B * N, 16)
    x = G.ints((B * N, D), _gen(B * N + D))
    _, dh0 = _dense(x, offset=offset)
    desc, mult = None, None
    if drop:
        desc = ops.dropout_desc(0.5, 0, 1234, 77)
        mult = torch.empty(B * N, D, device=DEV)
        ops.dropout_mask(desc, 0, B * N, D, mult, D)
        assert set(mult.unique().tolist()) == {0.0, 2.0}
        mult = mult.cpu()
    bufs = [_out(N * D), _out(D), _out(D)]
    ops.embed_grad(dh0, B, N, D, bufs[0][1], bufs[1][1], bufs[2][1], dropout=desc)
    refs = G.embed_grad(x, B, N, D, mult)
    fails = []
    for name, (flat, out), ref in zip(("dpos", "dcls", "dconv_bias"), bufs, refs):
        _same(name, out, ref.float().reshape(-1), fails)
        _guards(name, flat, [out], fails)
    if N == 1:
        assert float(bufs[2][1].abs().max()) == 0.0
    assert not fails, fails[:8]


@pytest.mark.parametrize("nparts", [1, 7, 64])
def test_sqnorm_partial(nparts):
    fails = []
    for n in (1, 3, 4, 5, 1027, 3074):
        G.assert_exact_sum(n, 64)
        g = G.ints((n,), _gen(n))
        _, gv = _dense(g)
        pflat, part = _out(nparts, dtype=torch.float64)
        ops.sqnorm_partial(gv, n, part)
        # workgroup i owns the float4s q with (q mod (256 nparts)) // 256 == i, workgroup 0 also the n % 4 tail
        sq = g.double() ** 2
        n4 = n // 4
        own = (torch.arange(n4) % (256 * nparts)) // 256
        want = torch.zeros(nparts, dtype=torch.float64).index_add_(0, own, sq[:n4 * 4].reshape(n4, 4).sum(1))
        want[0] += sq[n4 * 4:].sum()
        _same("sqnorm partial", part, want, fails, f" [n {n}]")                      # idle workgroups: exactly 0.0
        if float(part.sum()) != float(sq.sum()):
            fails.append(f"sqnorm total [n {n}]: {float(part.sum())} != {float(sq.sum())}")
        _guards("sqnorm partial", pflat, [part], fails, f" [n {n}]")
    assert not fails, fails[:8]


@pytest.mark.parametrize("B,D", [(1, 1), (1, 768), (3, 1), (3, 255), (3, 256), (3, 257), (3, 768), (257, 1),
                                 (257, 255)])
def test_cls_mse(B, D):
    assert B * D * 256 < 2 ** 24
    x, t = G.ints((B, D), _gen(B + D)), G.ints((B, D), _gen(B * D))
    _, xv = G.embed(x.to(DEV), D + 3)
    _, tv = G.embed(t.to(DEV), D + 5)
    loss, e, part = ops.cls_mse(xv, D + 3, tv, D + 5, B, D, return_part=True)
    re, rpart, rloss = G.cls_mse(x, t)
    fails = []
    _same("e", e, re.float(), fails)
    _same("part", part, rpart.float(), fails)
    _same("loss", loss.reshape(1), rloss.float().reshape(1), fails)
    assert not fails, fails


# ---- 2. vit_gemm_f32: exact integers -------------------------------------------------------------------------------
GEMM_MN = [1, 31, 32, 33, 70]
GEMM_K = [0, 1, 15, 16, 17, 48, 64, 65, 150]    # 48: three k-tiles, the fourth wave idle; 17: a second tile of one column


@pytest.mark.parametrize("at,bt", [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_f32_exact(at, bt):
    G.assert_exact_sum(150, 16, start=16)
    Af, Bf = G.ints((70, 150), _gen(1), -4, 4), G.ints((150, 70), _gen(2), -4, 4)
    biasf, C0f = G.ints((70,), _gen(3)), G.ints((70, 70), _gen(4))
    fails, n = [], 0
    for K in GEMM_K:
        for M in GEMM_MN:
            for N in GEMM_MN:
                use_bias, acc = bool(n & 1), bool(n & 2)
                n += 1
                A, B = Af[:M, :K], Bf[:K, :N]
                lda, ldb, ldc = (M if at else K) + 3, (K if bt else N) + 5, N + 7
                aflat, Av = G.embed((A.t() if at else A).contiguous().to(DEV), lda)
                bflat, Bv = G.embed((B.t() if bt else B).contiguous().to(DEV), ldb)
                if K == 0:      # an empty view has no address: the (all-NaN, never read) buffers themselves
                    Av, Bv = aflat, bflat
                bias = _dense(biasf[:N])[1] if use_bias else None
                cflat, Cv = G.embed(C0f[:M, :N].to(DEV) if acc else torch.full((M, N), G.NAN, device=DEV), ldc,
                                    extra_rows=1)
                ops.gemm_f32(M, N, K, Av, lda, at, Bv, ldb, bt, Cv, ldc, bias, accumulate=acc)
                want = G.gemm_f32(A, B, biasf[:N] if use_bias else None, C0f[:M, :N] if acc else None).float()
                tag = f" [M {M} N {N} K {K} bias {use_bias} acc {acc}]"
                _same("C", Cv, want, fails, tag)
                _guards("C", cflat, [Cv], fails, tag)
    assert n % 4 == 1 and not fails, fails[:8]          # 225 cases: the four bias / accumulate forms rotate through all


# ---- 3. casts and moves: bit-identical ------------------------------------------------------------------------------
def test_cast_f32_bf16_every_rounding():
    x = G.cast_patterns()
    nan = x.isnan()
    assert x.numel() == 393216 and int(nan.sum()) == G.CAST_NAN_COUNT == 1534
    fails = []
    _, xv = _dense(x)
    oflat, out = _out(x.numel(), dtype=BF16)
    ops.cast_bf16(xv, out, x.numel())
    _same("cast", out, x.bfloat16(), fails, bits=True, nan_by_kind=nan.to(DEV))
    _guards("cast", oflat, [out], fails)
    r = torch.randn(8192 * 256 + 5, generator=_gen(5))
    for n in (1, 255, 256, 257, 8192 * 256 + 5):        # the last: past the grid cap, a second stride pass
        _, xv = _dense(r[:n])
        oflat, out = _out(n, dtype=BF16)
        ops.cast_bf16(xv, out, n)
        _same("cast", out, r[:n].bfloat16(), fails, f" [n {n}]", bits=True)
        _guards("cast", oflat, [out], fails, f" [n {n}]")
    assert not fails, fails[:8]


@pytest.mark.parametrize("cols", [1, 37])
def test_unpack_bf16_f32_every_pattern(cols):
    rows = -(-65536 // cols)
    b = G.all_bf16()
    b = torch.cat([b, b[:rows * cols - 65536]]).reshape(rows, cols)
    want = (b.view(torch.int16).to(torch.int32) << 16).view(F32)
    _, bv = G.embed(b.to(DEV), cols + 2)
    oflat, ov = G.embed(torch.full((rows, cols), G.NAN, device=DEV), cols + 1, extra_rows=1)
    ops.unpack_bf16_f32(bv, cols + 2, rows, cols, ov, cols + 1)
    fails = []
    _same("unpack", ov, want, fails, bits=True)
    _guards("unpack", oflat, [ov], fails)
    assert not fails, fails


@pytest.mark.parametrize("rows,cols,ldo", [(1, 1, 1), (3, 5, 8), (7, 64, 64), (300, 70, 128)])
def test_cast_pad_rows(rows, cols, ldo):
    x = torch.randn(rows, cols, generator=_gen(rows))
    _, xv = _dense(x)
    oflat, ov = G.embed(torch.full((rows, ldo), G.NAN, device=DEV, dtype=BF16), ldo, extra_rows=2)
    ops.cast_pad_rows(xv, rows, cols, ov, ldo)
    want = torch.zeros(rows, ldo, dtype=BF16)
    want[:, :cols] = x.bfloat16()
    fails = []
    _same("cast_pad_rows", ov, want, fails, bits=True)      # columns past cols: +0
    _guards("cast_pad_rows", oflat, [ov], fails)             # rows past the end untouched
    assert not fails, fails


def _pack_case(rows, cols, Z, batch, out_dtype, negative):
    ldi, ldo = cols + 2, Z * cols + 3
    zstride = rows * ldi + 4
    set_in, set_out = Z * zstride + 5, rows * ldo + 6
    x = torch.randn(batch, Z, rows, cols, generator=_gen(rows + cols))
    iflat = _nan(batch * set_in + GUARD)
    for b in range(batch):
        for z in range(Z):
            iflat[b * set_in + z * zstride:].as_strided((rows, cols), (ldi, 1)).copy_(x[b, z])
    oflat = _nan(batch * set_out + GUARD, out_dtype)
    oviews = [oflat[b * set_out:].as_strided((rows, Z * cols), (ldo, 1)) for b in range(batch)]
    want = x.permute(0, 2, 1, 3).reshape(batch, rows, Z * cols).to(out_dtype)
    if negative:        # set z of the call = set batch - 1 - z of the buffer
        first, in_bs = iflat[(batch - 1) * set_in:], -set_in
        want = want.flip(0)
    else:
        first, in_bs = iflat, set_in
    return first, in_bs, zstride, ldi, oflat, oviews, set_out, ldo, want


@pytest.mark.parametrize("out_dtype", [BF16, F32])
def test_pack_cols(out_dtype):
    fails = []
    rows, cols, Z = 5, 7, 3
    first, _, zstride, ldi, oflat, oviews, _, ldo, want = _pack_case(rows, cols, Z, 1, out_dtype, False)
    ops.pack_cols(first, zstride, ldi, rows, cols, Z, oviews[0], ldo)
    _same("pack_cols", oviews[0], want[0], fails, bits=True)
    _guards("pack_cols", oflat, oviews, fails)
    # batch 3 read backwards; 96 x 3 x 1000 = 288,000 elements: past the 1024-block cap, the stride loop repeats
    for rows, cols, batch, negative in ((5, 7, 3, True), (96, 1000, 2, False)):
        first, in_bs, zstride, ldi, oflat, oviews, out_bs, ldo, want = _pack_case(rows, cols, Z, batch, out_dtype,
                                                                                  negative)
        ops.pack_cols_batched(first, in_bs, zstride, ldi, rows, cols, Z, oflat, out_bs, ldo, batch)
        for b in range(batch):
            _same("pack_cols_batched", oviews[b], want[b], fails, f" [rows {rows} set {b}]", bits=True)
        _guards("pack_cols_batched", oflat, oviews, fails, f" [rows {rows}]")
    assert not fails, fails[:8]


# (rows, cols, ldo, batch, negative strides). ldo % 8 == 0 takes the 16-B stores: (40, 16, 40) has whole 16-element
# store segments at rows 0 and 16 and a partial one at 32
TRANSPOSE_CASES = [(1, 1, 4, 1, False), (63, 65, 66, 1, False), (64, 64, 67, 1, False), (65, 63, 68, 1, False),
                   (1, 1, 8, 1, False), (63, 65, 64, 1, False), (64, 64, 64, 1, False), (65, 63, 72, 1, False),
                   (40, 16, 40, 1, False), (40, 16, 40, 3, True), (63, 65, 66, 3, True)]


@pytest.mark.parametrize("rows,cols,ldo,batch,negative", TRANSPOSE_CASES)
def test_transpose_f32_bf16(rows, cols, ldo, batch, negative):
    ldi = cols + 3
    set_in, set_out = rows * ldi + 5, cols * ldo + 8
    x = torch.randn(batch, rows, cols, generator=_gen(rows * cols))
    iflat = _nan(batch * set_in + GUARD)
    for b in range(batch):
        iflat[b * set_in:].as_strided((rows, cols), (ldi, 1)).copy_(x[b])
    oflat = _nan(batch * set_out + GUARD, BF16)
    oviews = [oflat[b * set_out:].as_strided((cols, rows), (ldo, 1)) for b in range(batch)]
    want = x.transpose(1, 2).bfloat16()
    if negative:        # matrix z of the call = matrix batch - 1 - z of both buffers
        ops.transpose_bf16(iflat[(batch - 1) * set_in:], rows, cols, ldi, oflat[(batch - 1) * set_out:], ldo, batch,
                           -set_in, -set_out)
    else:
        ops.transpose_bf16(iflat, rows, cols, ldi, oflat, ldo, batch, set_in, set_out)
    fails = []
    for b in range(batch):
        _same("transpose", oviews[b], want[b], fails, f" [matrix {b}]", bits=True)
    _guards("transpose", oflat, oviews, fails)
    assert not fails, fails[:8]


@pytest.mark.parametrize("n", [1, 255, 257])
def test_axpby(n):
    fails = []
    x = torch.randn(n, generator=_gen(n))
    _, xv = _dense(x)
    yflat, yv = _out(n)                                             # y holds NaN: b == 0 must not read it
    ops.axpby(xv, yv, n, 0.75, 0.0)
    _same("axpby b=0", yv, x * 0.75, fails, bits=True)
    _guards("axpby b=0", yflat, [yv], fails)
    # b != 0 on small integers with a = 2, b = -0.5: exact whether or not the multiply-add fuses
    xi, yi = G.ints((n,), _gen(n + 1)), G.ints((n,), _gen(n + 2))
    _, xv = _dense(xi)
    yflat, yv = _out(n, yi)
    ops.axpby(xv, yv, n, 2.0, -0.5)
    _same("axpby", yv, 2.0 * xi - 0.5 * yi, fails)
    _guards("axpby", yflat, [yv], fails)
    yflat, yv = _out(n, yi)                                         # in place: y = 2 y - 0.5 y
    ops.axpby(yv, yv, n, 2.0, -0.5)
    _same("axpby in place", yv, 1.5 * yi, fails)
    _guards("axpby in place", yflat, [yv], fails)
    assert not fails, fails


def test_one_rounding_elementwise_ops():
    """embed_fwd_f32, add_bcast_f32, dropout_apply_f32, scale_by_coef: one f32 add or multiply per element, so the
    bits of the same torch expression"""
    fails = []
    for B, N, D in ((1, 1, 1), (3, 5, 7), (2, 197, 65)):
        g = _gen(B * N * D)
        h, pos, cls = torch.randn(B * N, D, generator=g), torch.randn(N, D, generator=g), torch.randn(D, generator=g)
        hflat, hv = _dense(h)
        ops.embed_fwd_f32(hv, B, N, D, _dense(pos)[1], _dense(cls)[1])
        want = h.reshape(B, N, D).clone()
        want[:, 0] = cls
        _same("embed_fwd", hv, (want + pos[None]).reshape(B * N, D), fails, f" [{B} {N} {D}]", bits=True)
        _guards("embed_fwd", hflat, [hv], fails)
    for outer, inner in ((1, 1), (5, 33), (300, 257)):
        g = _gen(outer + inner)
        x, y = torch.randn(outer, inner, generator=g), torch.randn(inner, generator=g)
        oflat, ov = _out(outer * inner)
        ops.add_bcast_f32(_dense(x)[1], _dense(y)[1], ov, outer, inner)
        _same("add_bcast", ov.view(outer, inner), x + y[None], fails, f" [{outer} {inner}]", bits=True)
        _guards("add_bcast", oflat, [ov], fails)
    rows, cols = 37, 13                                             # a width that is no multiple of 8; in == out
    desc = ops.dropout_desc(0.1, 3, 99, 5)
    mult = torch.empty(rows, cols, device=DEV)
    ops.dropout_mask(desc, 0, rows, cols, mult, cols)
    assert 0 < int((mult == 0).sum()) < rows * cols // 2
    x = torch.randn(rows, cols, generator=_gen(6))
    xflat, xv = _dense(x)
    ops.dropout_apply_f32(desc, xv, xv, rows, cols)
    _same("dropout_apply", xv, x.to(DEV) * mult, fails, bits=True)
    _guards("dropout_apply", xflat, [xv], fails)
    coef = torch.tensor([0.37], device=DEV)
    r = torch.randn(4096 * 256 * 4 + 7, generator=_gen(7))
    for n in (1, 3, 4, 5, 4096 * 256 * 4 + 7):                     # the last: a second stride pass plus the tail
        gflat, gv = _dense(r[:n])
        ops.scale_by_coef(gv, n, coef)
        _same("scale_by_coef", gv, r[:n].to(DEV) * coef, fails, f" [n {n}]", bits=True)
        _guards("scale_by_coef", gflat, [gv], fails, f" [n {n}]")
    assert not fails, fails[:8]


# ---- 4. bounded per element against float64 --------------------------------------------------------------------------
def test_gelu_f32_and_bwd():
    fails = []
    u = G.gelu_inputs()
    n = u.numel()
    _, uv = _dense(u)
    oflat, out = _out(n)
    ops.gelu_f32(uv, out, n)
    _report("gelu_f32", _bounded("gelu", out, *G.gelu(u), fails))
    _guards("gelu", oflat, [out], fails)
    dy = torch.randn(n, generator=_gen(8))
    oflat, out = _out(n)
    ops.gelu_bwd_f32(uv, _dense(dy)[1], out, n)
    _report("gelu_bwd_f32", _bounded("gelu_bwd", out, *G.gelu_bwd(u, dy), fails))
    _guards("gelu_bwd", oflat, [out], fails)
    assert not fails, fails


@pytest.mark.parametrize("B,D", [(1, 1), (3, 257), (257, 255)])
def test_cls_mse_bwd(B, D):
    dx0, e, g = G.cls_mse_bwd_case(B, D, _gen(B + D))
    dflat, dv = G.embed(dx0.to(DEV), D + 3, extra_rows=1)
    ops.cls_mse_bwd(dv, D + 3, _dense(e)[1], g.to(DEV))
    fails = []
    _report(f"cls_mse_bwd[{B},{D}]", _bounded("cls_mse_bwd", dv, *G.cls_mse_bwd(dx0, e, g), fails))
    _guards("cls_mse_bwd", dflat, [dv], fails)
    assert not fails, fails


@pytest.mark.parametrize("first", [True, False])
def test_sgd_step(first):
    lr, mom, wd = 0.1, 0.9, 1e-2
    big = 8192 * 256 * 4 + 1024 + 3                                # a second stride pass plus the tail
    g_ = _gen(9)
    P, Gr, Bu = (torch.randn(big, generator=g_) for _ in range(3))
    fails, worst = [], 0.0
    for n in (1, 2, 3, 4, 5, big):
        p, g, buf = P[:n], Gr[:n], Bu[:n]
        pflat, pv = _dense(p)
        _, gv = _dense(g)
        bflat, bv = _out(n, None if first else buf)                # first: garbage (NaN) that must not be read
        mflat, mv = _out(n, dtype=BF16)
        ops.sgd_step(pv, gv, bv, mv, n, lr, mom, wd, first)
        pn, bn, bp, bb = G.sgd(p, g, buf, lr, mom, wd, first)
        tag = f" [n {n}]"
        worst = max(worst, _bounded("p", pv, pn, bp, fails, tag), _bounded("buf", bv, bn, bb, fails, tag))
        _same("mirror", mv, pv.bfloat16(), fails, tag, bits=True)
        for name, flat, v in (("p", pflat, pv), ("buf", bflat, bv), ("mirror", mflat, mv)):
            _guards(name, flat, [v], fails, tag)
    _report(f"sgd_step[first={first}]", worst)
    assert not fails, fails[:8]


@pytest.mark.parametrize("nseg,nparts,seed,clip", G.ADAMW_PREP_CASES)
def test_adamw_prep(nseg, nparts, seed, clip):
    lr, b1, b2 = 1e-3, 0.9, 0.999
    partial, used, steps, max_norm = G.adamw_prep_case(nseg, nparts, seed, clip)
    table, st, norm, coef = G.adamw_prep(partial, used, steps, lr, b1, b2, max_norm)
    assert (coef == 1.0) == (not clip or nparts == 0)
    pv = _dense(partial)[1] if nparts else None
    sflat, sv = _out(nseg, steps)
    tflat, tv = _out(nseg * 4)
    nflat, nv = _out(2)
    ops.adamw_prep(pv, _dense(used)[1], sv, lr, b1, b2, max_norm, tv, nv)
    fails = []
    _same("steps", sv, st.float(), fails)
    r = _bounded("table", tv.view(nseg, 4), table, G.ulp32(table) * (table != 0), fails)    # zeros exact
    want = torch.tensor([norm, coef], dtype=torch.float64)
    r = max(r, _bounded("norm_out", nv, want, G.ulp32(want) * (want != 0), fails))
    _report(f"adamw_prep[{nseg},{nparts}] (ulps)", r)
    for name, flat, v in (("steps", sflat, sv), ("table", tflat, tv), ("norm_out", nflat, nv)):
        _guards(name, flat, [v], fails)
    assert not fails, fails[:8]


@pytest.mark.parametrize("write_grad", [False, True])
@pytest.mark.parametrize("mirror", [True, False])
def test_adamw_update(write_grad, mirror):
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 0.05
    assert ops.adamw_chunk_elems() == 8192
    starts, total, chunks, active = G.adamw_layout()
    coef = G.f32(0.37)
    g_ = _gen(10)
    seg = {name: [] for name in "pgmv"}
    flat = {name: _nan(total + GUARD) for name in "pgmv"}
    mflat = _nan(total + GUARD, BF16)
    table = torch.zeros(len(starts), 4)
    for s, (at, n) in enumerate(zip(starts, G.ADAMW_LENGTHS)):
        vals = dict(p=torch.randn(n, generator=g_), g=torch.randn(n, generator=g_), m=torch.randn(n, generator=g_),
                    v=torch.rand(n, generator=g_) + 1e-4)
        for name in "pgmv":
            seg[name].append(vals[name])
            flat[name][at:at + n] = vals[name].to(DEV)
        mflat[at:at + n] = 7.0                                     # what an inactive segment's mirror must keep
        step = s + 1
        table[s] = torch.tensor([G.f32(lr) / (1 - G.f32(b1) ** step), math.sqrt(1 - G.f32(b2) ** step), 1.0, coef]) \
            if active[s] else torch.tensor([0.0, 0.0, 0.0, coef])
    ops.adamw_update(flat["p"], flat["g"], flat["m"], flat["v"], mflat if mirror else None, chunks.to(DEV),
                     table.to(DEV), lr, b1, b2, eps, wd, write_grad)
    fails, worst = [], 0.0
    views = lambda f: [f[at:at + n] for at, n in zip(starts, G.ADAMW_LENGTHS)]
    for s, (at, n) in enumerate(zip(starts, G.ADAMW_LENGTHS)):
        tag = f" [segment {s} length {n}]"
        got = {name: flat[name][at:at + n] for name in "pgmv"}
        if not active[s]:                                          # torch skips it: every bit stays
            for name in "pgmv":
                _same(name, got[name], seg[name][s], fails, tag, bits=True)
            _same("mirror", mflat[at:at + n], torch.full((n,), 7.0, dtype=BF16), fails, tag, bits=True)
            continue
        refs, bounds = G.adamw(seg["p"][s], seg["g"][s], seg["m"][s], seg["v"][s], float(table[s, 0]),
                               float(table[s, 1]), coef, lr, b1, b2, eps, wd)
        for name, ref, bound in zip("pgmv", refs, bounds):
            if name == "g" and not write_grad:
                _same("g", got["g"], seg["g"][s], fails, tag, bits=True)
            else:
                worst = max(worst, _bounded(name, got[name], ref, bound, fails, tag))
        want_m = got["p"].bfloat16() if mirror else torch.full((n,), 7.0, dtype=BF16)
        _same("mirror", mflat[at:at + n], want_m, fails, tag, bits=True)
    for name in "pgmv":
        _guards(name, flat[name], views(flat[name]), fails)        # the alignment gaps stay NaN
    _guards("mirror", mflat, views(mflat), fails)
    _report(f"adamw_update[write_grad={write_grad},mirror={mirror}]", worst)
    assert not fails, fails[:8]


# ---- 5. cross entropy ------------------------------------------------------------------------------------------------
def _ce(x, y, gs, dlogits=True, stats=True):
    B, C = x.shape
    _, xv = _dense(x)
    dflat, dv = _out(B * C) if dlogits else (None, None)
    sflat, sv = _out(B * 3) if stats else (None, None)
    ops.cross_entropy(xv, y.to(DEV), dv.view(B, C) if dlogits else None, gs, sv.view(B, 3) if stats else None)
    return dflat, (dv.view(B, C) if dlogits else None), sflat, (sv.view(B, 3) if stats else None)


def _ce_check(x, y, gs, fails, tag, dlogits=True, stats=True):
    """every row's loss, hits and gradient against glue_ref.cross_entropy: (loss ratio, dlogits ratio)"""
    r = G.cross_entropy(x, y, gs)
    dflat, dv, sflat, sv = _ce(x, y, gs, dlogits, stats)
    rl = rd = 0.0
    if stats:
        rl = _bounded("loss", sv[:, 0], r.loss, r.bound_loss, fails, tag)
        _same("top1", sv[:, 1], r.top1.float(), fails, tag)
        _same("top5", sv[:, 2], r.top5.float(), fails, tag)
        _guards("row_stats", sflat, [sv], fails, tag)
    if dlogits:
        rd = _bounded("dlogits", dv, r.dlogits, r.bound_d, fails, tag)
        _guards("dlogits", dflat, [dv], fails, tag)
    return rl, rd


@pytest.mark.parametrize("C", [2, 5, 6, 10, 100, 255, 256, 257, 1000, 1023])
def test_cross_entropy_sweep(C):
    fails, rl, rd = [], 0.0, 0.0
    for B in (1, 3, 65):
        g = _gen(B * 10000 + C)
        x = G.ce_logits(B, C, g)
        y = torch.randint(0, C, (B,), generator=g)
        for gs in (1.0, 1.0 / B):
            a, b = _ce_check(x, y, gs, fails, f" [B {B} grad_scale {gs:.3g}]")
            rl, rd = max(rl, a), max(rd, b)
    if C == 5:      # every finite row is a top-5 hit
        _, _, _, sv = _ce(x, y, 1.0)
        assert bool((sv[:, 2] == 1).all())
    _report(f"cross_entropy loss[C={C}]", rl)
    _report(f"cross_entropy dlogits[C={C}]", rd)
    assert not fails, fails[:8]


def test_cross_entropy_nan_rows_are_misses():
    """a NaN logit ranks above every number (torch.topk): a diverged row is a miss, not a hit"""
    nan = G.NAN
    x = torch.tensor([[1.0, nan, 3.0, 2.0, 0.0, -1.0, 5.0],     # label 6 is the largest number: top-1 is the NaN
                      [nan] * 7,                                 # all NaN
                      [nan, nan, nan, nan, nan, 1.0, 0.0],       # five NaN above the label: no top-5 hit either
                      [nan, nan, nan, nan, 0.5, 1.0, 0.0],       # four: a top-5 hit
                      [0.0, 1.0, 2.0, nan, 3.0, 4.0, 5.0],       # the label's own logit the only NaN: a hit, as in torch
                      [0.0, 1.0, 2.0, 6.0, 3.0, 4.0, 5.0]])      # a finite neighbour
    y = torch.tensor([6, 2, 5, 5, 3, 3])
    _, dv, _, sv = _ce(x, y, 1.0)
    assert sv[:, 1].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0], sv[:, 1].tolist()
    assert sv[:, 2].tolist() == [1.0, 0.0, 0.0, 1.0, 1.0, 1.0], sv[:, 2].tolist()
    assert sv[:, 0].isnan().tolist() == [True] * 5 + [False]
    assert dv.isnan().all(1).tolist() == [True] * 5 + [False]
    fails = []
    _ce_check(x, y, 1.0, fails, "")
    assert not fails, fails


def test_cross_entropy_ties_and_top5_edges():
    fails = []
    g = _gen(11)
    # exact ties at the label's value count for the label, wherever the label sits among them
    x = G.ce_logits(65, 100, g)
    y = torch.randint(0, 100, (65,), generator=g)
    xy = x.gather(1, y[:, None])
    x = torch.where(torch.rand(65, 100, generator=g) < 0.2, xy.expand(-1, 100), x)
    _ce_check(x, y, 1.0 / 65, fails, " [ties]")
    # the label tied for fifth place (a hit) and just below five larger ones (a miss)
    x = torch.tensor([[9.0, 8.0, 7.0, 6.0, 3.0, 3.0, 3.0, 0.0],
                      [9.0, 8.0, 7.0, 6.0, 5.0, 3.0, 3.0, 0.0],
                      [2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])
    y = torch.tensor([6, 6, 7])
    _ce_check(x, y, 1.0, fails, " [fifth place]")
    _, _, _, sv = _ce(x, y, 1.0)
    assert sv[:, 1].tolist() == [0.0, 0.0, 1.0] and sv[:, 2].tolist() == [1.0, 0.0, 1.0]
    assert not fails, fails[:8]


def test_cross_entropy_bad_labels_and_null_outputs():
    fails = []
    g = _gen(12)
    for C in (6, 257):
        x = G.ce_logits(5, C, g)
        y = torch.tensor([1, -1, C, 2, C - 1])                   # -1 and C: NaN loss, a NaN gradient row, a miss
        _ce_check(x, y, 0.2, fails, f" [C {C} bad labels]")      # the neighbours within their gates
        _, dv, _, sv = _ce(x, y, 0.2)
        assert sv[:, 0].isnan().tolist() == [False, True, True, False, False]
        assert dv.isnan().all(1).tolist() == [False, True, True, False, False]
        assert not bool(dv[[0, 3, 4]].isnan().any())
        y = torch.randint(0, C, (5,), generator=g)
        _ce_check(x, y, 0.2, fails, f" [C {C} dlogits NULL]", dlogits=False)
        _ce_check(x, y, 0.2, fails, f" [C {C} row_stats NULL]", stats=False)
    assert not fails, fails[:8]
