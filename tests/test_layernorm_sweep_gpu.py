"""LayerNorm (csrc/layernorm.hip) through vitmi.ops, every output element against norm_ref.py's float64 references
and counted gates: all sixteen instantiations NV 1..8 x FULL of each direction (norm_ref.SWEEP_D, both sides of every
FULL width), three input families (variance 9, mean 1000, variance 1e-6), the row counts around the backward's
512-block cap, and every form of the ABI.

Inputs sit in NaN-padded buffers of their own strides (padding must never be read), outputs in NaN-filled ones
(padding and guards must stay NaN). Each backward runs twice and must repeat bit for bit. Gates print their worst
ratio ("RATIO name value", visible with pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import glue_ref as G
import norm_ref as N
from oracle.dropout import dropout_mult
from vitmi import ops
from vitmi._lib import VitHipError

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SEED, OFF = 0x1234_5678_9ABC_DEF1, 0x2_0000_0007


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _inp(t, ld, dtype=F32):
    """the logical tensor inside a NaN-padded device buffer of row stride ld: the view"""
    return G.embed(t.to(DEV).to(dtype), ld)[1]


def _outbuf(rows, cols, ld, dtype=F32, prior=None):
    """a NaN-filled output (or the values to accumulate onto) in a NaN buffer: (flat, view)"""
    t = torch.full((rows, cols), G.NAN, dtype=dtype) if prior is None else prior.reshape(rows, cols)
    return G.embed(t.to(DEV).to(dtype), ld, extra_rows=1)


class Worst(dict):
    """worst ratio per gate name, and the failures"""

    def __init__(self):
        super().__init__()
        self.fails = []

    def gate(self, name, got, ref, bound, tag):
        ratio, at = G.worst(got, ref, bound)
        self[name] = max(self.get(name, 0.0), ratio)
        if not ratio <= 1.0:
            self.fails.append(f"{name}{tag}: {ratio:.4g} x gate at {at}")

    def same(self, name, got, want, tag, bits=True):
        d = G.first_diff(got, want, bits=bits)
        if d is not None:
            self.fails.append(f"{name}{tag}: at {d[0]} got {d[1]!r}, want {d[2]!r}")

    def guards(self, name, flat, view, tag):
        at = G.first_touched(flat, view)
        if at is not None:
            self.fails.append(f"{name}{tag}: guard element {at} of the buffer was written")

    def done(self, prefix):
        for name, r in self.items():
            print(f"RATIO {prefix}_{name} {r:.4g}")
        assert not self.fails, self.fails[:8]


def _forward(w, x, gamma, beta, D, y_dtype, tag, pad=True):
    """vit_layernorm_fwd on the logical x [rows, D]: gates mean, rstd and y; returns (x view, mean, rstd) as the
    backward receives them"""
    rows = x.shape[0]
    ldx, ldy = (D + 4, D + 8) if pad else (D, D)
    xv = _inp(x, ldx)
    yflat, y = _outbuf(rows, D, ldy, y_dtype)
    mflat, mean = _outbuf(1, rows, rows)
    rflat, rstd = _outbuf(1, rows, rows)
    ops.layernorm_fwd(xv, ldx, gamma, beta, y, ldy, mean, rstd, rows, D)
    ref = N.fwd(xv, gamma, beta)
    w.gate("mean", mean[0], ref.mean, ref.b_mean, tag)
    w.gate("rstd", rstd[0], ref.rstd, ref.b_rstd, tag)
    if y_dtype == F32:
        w.gate("y_f32", y, ref.y, ref.b_y, tag)
    else:
        w.gate("y_bf16", y, ref.y, ref.b_y16, tag)
    for name, flat, view in (("y", yflat, y), ("mean", mflat, mean), ("rstd", rflat, rstd)):
        w.guards(name, flat, view, tag)
    return xv, ldx, mean[0], rstd[0]


def _backward(w, xv, ldx, mean, rstd, gamma, dy, D, tag, *, dy_dtype=BF16, dres=None, dxb=True, sums=True, acc=False,
              drop_stride=0, pad=True, int_dy=False):
    """vit_layernorm_bwd twice (bit-identical), every output gated; dy / dres: logical CPU tensors. sums False: the
    partials-only call, whose block partials are gated as column sums. drop_stride > 0: dropout p = 0.1 with that
    row_stride."""
    rows = xv.shape[0]
    lddy, lddres, lddx, lddxb = ((D + 12, D + 16, D + 20, D + 24) if pad else (D,) * 4)
    dyv = _inp(dy, lddy, dy_dtype)
    dresv = None if dres is None else _inp(dres, lddres)
    desc, mult = None, None
    if drop_stride:
        desc = ops.dropout_desc(0.1, 9, SEED, OFF, row_stride=drop_stride)
        mult = torch.from_numpy(dropout_mult(0.1, 9, SEED, OFF, rows, D, 0, drop_stride)).to(DEV)
    prior = torch.randn(3, D, generator=_gen(D)) if acc else None
    if acc and int_dy:
        prior = G.ints((3, D), _gen(D))
    nblk = ops.layernorm_bwd_blocks(rows)
    assert nblk == N.bwd_blocks(rows)
    prow = ops.layernorm_bwd_partial_rows(rows)
    runs = []
    for _ in range(2):
        dxflat, dx = _outbuf(rows, D, lddx)
        bflat, dxbv = _outbuf(rows, D, lddxb, BF16) if dxb else (None, None)
        pflat, part = _outbuf(prow, 3 * D, 3 * D)
        gflat, dgb = _outbuf(1, 2 * D, 2 * D, prior=None if prior is None else prior[:2])
        sflat, dsum = _outbuf(1, D, D, prior=None if prior is None else prior[2])
        ops.layernorm_bwd(dyv, lddy, xv, ldx, mean, rstd, gamma, dx, lddx, part, rows, D, dres=dresv,
                          lddres=lddres if dres is not None else 0, dx_bf16=dxbv, lddxb=lddxb if dxb else 0,
                          dgamma_dbeta=dgb[0] if sums else None, dx_colsum=dsum[0] if sums else None, accumulate=acc,
                          dx_dropout=desc)
        runs.append((dx, dxbv, part[:nblk], dgb, dsum))
        w.guards("dx", dxflat, dx, tag)
        if dxb:
            w.guards("dx_bf16", bflat, dxbv, tag)
        w.guards("partial", pflat, part if sums else part[:nblk], tag)
        w.guards("dgamma_dbeta", gflat, dgb if sums else dgb[:, :0], tag)
        w.guards("dx_colsum", sflat, dsum if sums else dsum[:, :0], tag)
    for name, a, b in zip(("dx", "dx_bf16", "partial", "dgamma_dbeta", "dx_colsum"), *runs):
        if a is not None and (sums or name in ("dx", "dx_bf16", "partial")):
            w.same(name + " (second run)", b, a, tag)
    dx, dxbv, part, dgb, dsum = runs[0]
    ref = N.bwd(dyv, xv, mean, rstd, gamma, dresv, mult)
    w.gate("dx" if dres is not None else "dx_nodres", dx, ref.dx, ref.b_dx, tag)
    if dxb:
        w.gate("dx_bf16_dropout" if drop_stride else "dx_bf16", dxbv, ref.dxm, ref.b_dx16, tag)
    (dg, db, ds), (b_dg, b_db, b_ds) = N.colsums(ref, rows, None if prior is None else prior.to(DEV))
    if sums:
        got = (dgb[0, :D], dgb[0, D:], dsum[0])
    else:       # the block partials, summed in float64: the rounding of the final reduction is not in them
        got = tuple(part[:, k * D:(k + 1) * D].double().sum(0) for k in range(3))
    sfx = ("" if sums else "_partials") + ("_dropout" if drop_stride else "")
    w.gate("dgamma" + sfx, got[0], dg, b_dg, tag)
    if int_dy:
        G.assert_exact_sum(rows, 8, start=8)
        w.same("dbeta (integers)", got[1].float(), db.float(), tag, bits=False)
    else:
        w.gate("dbeta" + sfx, got[1], db, b_db, tag)
    w.gate("dx_colsum" + sfx, got[2], ds, b_ds, tag)


def _params(D, g):
    return torch.randn(D, generator=g).to(DEV), torch.randn(D, generator=g).to(DEV)


@pytest.mark.parametrize("D", N.SWEEP_D)
def test_every_instantiation(D):
    """D -> (NV, FULL) = norm_ref.kernel_of(D): SWEEP_D covers all sixteen of each direction (asserted by
    test_norm_ref_cpu.test_table_covers_all_32_kernels)"""
    w = Worst()
    for rows in (5, 2053):
        for k, kind in enumerate(N.FAMILIES):
            g = _gen(D * 10 + k)
            tag = f" [D {D} rows {rows} {kind}]"
            x = N.family(kind, rows, D, g)
            gamma, beta = _params(D, g)
            _forward(w, x, gamma, beta, D, F32, tag)
            xv, ldx, mean, rstd = _forward(w, x, gamma, beta, D, BF16, tag)
            dy, dres = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
            _backward(w, xv, ldx, mean, rstd, gamma, dy, D, tag, dy_dtype=BF16 if k != 1 else F32, dres=dres)
    nv, full = N.kernel_of(D)
    w.done(f"ln_NV{nv}_{'full' if full else 'guarded'}_D{D}")


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 2047, 2048, 2049, 4101])
@pytest.mark.parametrize("D", [64, 768])
def test_row_edges(D, rows):
    """fewer rows than a block's waves; 2048 = 512 blocks x 4 waves, the last count with no second row per wave;
    2049: exactly one wave prefetches; 4101: five waves walk a third row. The second backward has integer dy, so
    dbeta must be exact."""
    w = Worst()
    g = _gen(rows * 3 + D)
    tag = f" [D {D} rows {rows}]"
    x = N.family("wide", rows, D, g)
    gamma, beta = _params(D, g)
    xv, ldx, mean, rstd = _forward(w, x, gamma, beta, D, BF16, tag)
    dy, dres = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    _backward(w, xv, ldx, mean, rstd, gamma, dy, D, tag, dres=dres)
    _backward(w, xv, ldx, mean, rstd, gamma, G.ints((rows, D), g), D, tag + " integer dy", dres=dres, acc=True,
              int_dy=True)
    w.done(f"ln_rows{rows}_D{D}")


# (name, keyword arguments of _backward); every case at D = 100 (D % 8 == 4: dgamma | dbeta and the dx column sum by
# two vit_colsum, scalar path), 260 (the same with NV 2) and 768, at 517 rows (130 blocks: two column-sum chunks)
FORMS = [("dy_f32", dict(dy_dtype=F32, dres=True)),
         ("no_dres", dict()),
         ("no_dx_bf16", dict(dres=True, dxb=False)),
         ("accumulate", dict(dres=True, acc=True)),
         ("partials_only", dict(dres=True, sums=False)),
         ("dense_strides", dict(dres=True, pad=False)),
         ("dropout_stride_1", dict(dres=True, drop_stride=1)),
         ("dropout_stride_7", dict(dres=True, drop_stride=7, acc=True)),
         ("dropout_partials_no_dres", dict(drop_stride=1, sums=False))]


@pytest.mark.parametrize("D", [100, 260, 768])
@pytest.mark.parametrize("name,kw", FORMS, ids=[f[0] for f in FORMS])
def test_forms(name, kw, D):
    rows = 517
    w = Worst()
    g = _gen(D + len(name))
    tag = f" [{name} D {D}]"
    x = N.family("wide", rows, D, g)
    gamma, beta = _params(D, g)
    kw = dict(kw)
    pad = kw.get("pad", True)
    xv, ldx, mean, rstd = _forward(w, x, gamma, beta, D, F32 if "f32" in name else BF16, tag, pad=pad)
    dy = torch.randn(rows, D, generator=g)
    if kw.pop("dres", False):
        kw["dres"] = torch.randn(rows, D, generator=g)
    _backward(w, xv, ldx, mean, rstd, gamma, dy, D, tag, **kw)
    w.done(f"ln_form_{name}_D{D}")


@pytest.mark.parametrize("D", [64, 768, 1284])
def test_constant_row(D):
    """variance 0 (3.0: every partial sum is exact, so mean = 3 and x - mean = 0): y = beta bit for bit in both output
    types, rstd within its gate of 1 / sqrt(eps)"""
    rows = 6
    w = Worst()
    g = _gen(D)
    x = N.family("wide", rows, D, g)
    x[1], x[4] = 3.0, 3.0
    gamma, beta = _params(D, g)
    for dt in (F32, BF16):
        ldy = D + 8
        xv = _inp(x, D + 4)
        _, y = _outbuf(rows, D, ldy, dt)
        mean, rstd = torch.full((rows,), G.NAN, device=DEV), torch.full((rows,), G.NAN, device=DEV)
        ops.layernorm_fwd(xv, D + 4, gamma, beta, y, ldy, mean, rstd, rows, D)
        ref = N.fwd(xv, gamma, beta)
        for r in (1, 4):
            w.same("y of a constant row", y[r], beta.to(dt), f" [D {D} {dt} row {r}]")
            assert float(mean[r]) == 3.0
        w.gate("rstd_constant_row", rstd, ref.rstd, ref.b_rstd, f" [D {D}]")
        assert abs(float(ref.rstd[1]) - G.f32(1e-5) ** -0.5) < 1e-9
    w.done(f"ln_D{D}")


@pytest.mark.parametrize("bad", ["lddy", "ldx", "lddx", "lddres", "lddxb", "fwd_ldx", "fwd_ldy"])
def test_misaligned_strides_are_rejected(bad):
    """a stride that is not a multiple of 4 would misalign the 16-B / 8-B vector accesses of every odd row: both
    directions return the bad-argument status before any launch, and no output is written"""
    rows, D = 9, 64
    g = _gen(1)
    ld = {k: D + 4 for k in ("lddy", "ldx", "lddx", "lddres", "lddxb", "fwd_ldx", "fwd_ldy")}
    ld[bad] = D + 2
    gamma, beta = _params(D, g)
    x = torch.randn(rows, D + 4, generator=g).to(DEV)
    nan = lambda *s, dt=F32: torch.full(s, G.NAN, device=DEV, dtype=dt)
    if bad.startswith("fwd"):
        y, mean, rstd = nan(rows, D + 4, dt=BF16), nan(rows), nan(rows)
        with pytest.raises(VitHipError, match="multiples of 4"):
            ops.layernorm_fwd(x, ld["fwd_ldx"], gamma, beta, y, ld["fwd_ldy"], mean, rstd, rows, D)
        torch.cuda.synchronize()
        assert bool(y.float().isnan().all()) and bool(mean.isnan().all()) and bool(rstd.isnan().all())
        return
    dy = torch.randn(rows, D + 4, generator=g).to(DEV).to(BF16)
    dres = torch.randn(rows, D + 4, generator=g).to(DEV)
    mean, rstd = x[:, :D].mean(1), torch.rsqrt(x[:, :D].var(1, unbiased=False) + 1e-5)
    dx, dxb = nan(rows, D + 4), nan(rows, D + 4, dt=BF16)
    part, dgb, dsum = nan(ops.layernorm_bwd_partial_rows(rows), 3 * D), nan(2 * D), nan(D)
    with pytest.raises(VitHipError, match="multiples of 4"):
        ops.layernorm_bwd(dy, ld["lddy"], x, ld["ldx"], mean, rstd, gamma, dx, ld["lddx"], part, rows, D, dres=dres,
                          lddres=ld["lddres"], dx_bf16=dxb, lddxb=ld["lddxb"], dgamma_dbeta=dgb, dx_colsum=dsum)
    torch.cuda.synchronize()
    for t in (dx, dxb, part, dgb, dsum):
        assert bool(t.float().isnan().all())
    # the strides of absent operands are not looked at
    if bad in ("lddres", "lddxb"):
        ops.layernorm_bwd(dy, D + 4, x, D + 4, mean, rstd, gamma, dx, D + 4, part, rows, D, lddres=D + 2, lddxb=D + 2,
                          dgamma_dbeta=dgb, dx_colsum=dsum)
        torch.cuda.synchronize()
        assert not bool(dx[:, :D].isnan().any()) and bool(dx[:, D:].isnan().all())
