"""The per-element GEMM gate of gemm_ref.py, proved without a GPU: the float64 reference is the operation torch
computes, the kernels' two erf formulas leave it half of the gate's absolute term, correct (emulated) outputs pass,
and small planted faults that a whole-matrix norm lets through are flagged at their location."""
import math

import pytest
import torch
import torch.nn.functional as Fn

import gemm_ref as G

EPIS = list(range(10))
M, N, K, TOKENS = 40, 48, 320, 5      # 2.5 blocks of 16 rows, 6 chunks of 8 columns; K = 320 is the sweep's largest
RPT = 16                               # rows per "tile" of the column partials: M = 40 leaves a partial tile


def _case(epi, drop=False, exact=True, seed=0, batch=1):
    """operands of one small GEMM (packed K-contiguous / N-contiguous, padded leading dimensions) and the
    reference() keywords"""
    g = torch.Generator().manual_seed(seed)
    if exact:
        A, B = G.exact_ab(epi, M, N, K, g, batch)
        bias = G.exact_bias(epi, N, batch) if epi in G.HAS_BIAS else None
        aux = G.exact_aux(epi, TOKENS if epi == G.PATCH else M, N) if epi in G.HAS_AUX else None
        cls = G.exact_cls(N) if epi == G.PATCH else None
    else:
        A, B = torch.randn(batch, M, K, generator=g).bfloat16(), (torch.randn(batch, K, N, generator=g) / 8).bfloat16()
        bias = torch.randn(batch, N, generator=g) if epi in G.HAS_BIAS else None
        aux = (torch.randn(TOKENS if epi == G.PATCH else M, N, generator=g).to(G.aux_dtype(epi))
               if epi in G.HAS_AUX else None)
        cls = torch.randn(N, generator=g) if epi == G.PATCH else None
    lda, ldb, ldaux = K + 8, N + 16, N + 24
    Am = torch.zeros(batch, M, lda, dtype=torch.bfloat16)
    Am[:, :, :K] = A
    Bm = torch.zeros(batch, K, ldb, dtype=torch.bfloat16)
    Bm[:, :, :N] = B
    auxm = None
    if aux is not None:
        auxm = torch.full((aux.shape[0], ldaux), float("nan"), dtype=aux.dtype)
        auxm[:, :N] = aux
    mult = (torch.randint(0, 2, (M, N), generator=g) * 2).float() if drop else None
    kw = dict(a_layout=G.K_CONTIG, b_layout=G.MN_CONTIG, lda=lda, ldb=ldb, bias=bias, aux=auxm, ldaux=ldaux, aux2=cls,
              tokens=TOKENS if epi == G.PATCH else 0, batch=batch, a_bs=M * lda, b_bs=K * ldb, bias_bs=N, mult=mult,
              rows_per_tile=RPT if epi in G.HAS_COL_PARTIAL and batch == 1 else None)
    return A, B, bias, aux, cls, mult, Am, Bm, kw


def _ref(epi, drop=False, **over):
    A, B, bias, aux, cls, mult, Am, Bm, kw = _case(epi, drop)
    kw.update(over)
    return G.reference(epi, Am, Bm, M, N, K, **kw)


CASES = [(e, False) for e in EPIS] + [(e, True) for e in G.HAS_DROPOUT]
IDS = [G.NAMES[e] + ("+DROP" if d else "") for e, d in CASES]


@pytest.mark.parametrize("epi", EPIS, ids=G.NAMES)
def test_reference_matches_torch(epi):
    """random, non-exact operands: the reference is what F.linear / F.gelu / autograd compute in float64, through
    the packed layouts, leading dimensions and batch strides"""
    batch = 1 if epi == G.PATCH or epi in G.HAS_AUX else 3
    A, B, bias, aux, cls, mult, Am, Bm, kw = _case(epi, exact=False, batch=batch)
    r = G.reference(epi, Am, Bm, M, N, K, **kw)
    a, b = A.double(), B.double()
    want = {}
    if epi in (G.F32, G.BF16, G.SPLITK):
        want["C"] = a @ b
    elif epi in (G.BIAS_BF16, G.BIAS_GELU, G.BIAS_GELU_DGELU):
        u = torch.stack([Fn.linear(a[z], b[z].t(), bias[z].double()) for z in range(batch)]).requires_grad_(True)
        g = Fn.gelu(u)
        d, = torch.autograd.grad(g.sum(), u)
        want = {G.BIAS_BF16: {"C": u}, G.BIAS_GELU: {"C": u, "C2": g}, G.BIAS_GELU_DGELU: {"C": d, "C2": g}}[epi]
    elif epi == G.BIAS_RESID_F32:
        want["C"] = Fn.linear(a[0], b[0].t(), bias[0].double())[None] + aux.double()
    elif epi == G.GELU_BWD:
        x = aux.double().requires_grad_(True)
        want["C"], = torch.autograd.grad(Fn.gelu(x), x, (a @ b)[0])
        want["C"] = want["C"][None]
    elif epi == G.MUL_BF16:
        want["C"] = (a @ b) * aux.double()
    elif epi == G.PATCH:
        c = Fn.linear(a[0], b[0].t(), bias[0].double()) + aux.double().repeat(M // TOKENS, 1)
        c[::TOKENS] = cls.double() + aux[0].double()
        want["C"] = c[None]
    want = {name: w.detach() for name, w in want.items()}
    for name, w in want.items():
        err = float((r.out[name] - w).abs().max())
        assert err <= 1e-12 * max(1.0, float(w.abs().max())), (name, err)
    if kw["rows_per_tile"]:
        w = torch.stack([want["C"][0][k:k + RPT].sum(0) for k in range(0, M, RPT)]).detach()
        assert float((r.out["partial"] - w).abs().max()) <= 1e-11 * float(w.abs().max())


def test_operands_are_exact():
    """every partial sum the kernel can form is exact in f32 (assert_exact), u of the GELU epilogues is of order 1
    and not saturated, and the linear sums pass 256, so bf16 rounding (ties included) happens"""
    for epi in EPIS:
        for k in (64, 320):
            G.assert_exact(epi, k)
    r = _ref(G.BIAS_GELU)
    u = r.u
    assert float((u * 64 - (u * 64).round()).abs().max()) == 0 and float(u.abs().max()) * 64 < 2 ** 24
    assert 0.5 < float(u.std()) < 4 and float((u.abs() < 3).double().mean()) > 0.8
    c = _ref(G.BF16).out["C"]
    assert float((c - c.round()).abs().max()) == 0
    odd = (c.abs() > 256) & (c.abs() < 512) & (c % 2 != 0)             # bf16 ties
    assert int(odd.sum()) > 0
    assert not torch.equal(G.expected(c, torch.bfloat16).double(), c)


def _grid():
    g = torch.Generator().manual_seed(1)
    return torch.cat([torch.linspace(-14, 14, 2_800_001, dtype=torch.float64),
                      torch.randn(1_000_000, generator=g, dtype=torch.float64)])


def test_formula_headroom():
    """the kernels' erf formulas, evaluated in float32 and rounded to bf16, use less than half of the absolute
    term c s of their gate (the rest is for the device's rcp / exp2 and the f32 accumulator-side arithmetic):
    |bf16(f(u)) - ref| - U |ref| <= c max(1, |u|) / 2 over a dense grid on [-14, 14] and 10^6 normal samples"""
    u = _grid()
    u = u.float().double()                       # the values the formulas see
    s = u.abs().clamp_min(1.0)
    g64, d64 = G.gelu64(u)
    cdf, pdf = G.phi_and_pdf(u)
    u32 = u.float()
    forms = {"phi_and_pdf": (G.C_PHI, u32 * cdf, cdf + u32 * pdf), "gelu_dgelu2": (G.C_DGELU,) + G.gelu_dgelu2(u)}
    for name, (c, g, d) in forms.items():
        raw = max(float(((g.double() - g64).abs() / s).max()), float(((d.double() - d64).abs() / s).max()))
        worst = excess = 0.0
        for got, ref in ((g, g64), (d, d64)):
            err = (got.bfloat16().double() - ref).abs()
            excess = max(excess, float(((err - G.U * ref.abs()).clamp_min(0) / s).max()))
            worst = max(worst, float((err / (G.U * ref.abs() + c * s)).max()))
        print(f"{name}: f32 error {raw:.3g} max(1,|u|), past the bf16 term {excess:.3g} (c/2 = {c / 2:.3g}), "
              f"worst gate ratio after rounding {worst:.3f}")
        assert raw <= c / 2 and excess <= c / 2 and worst <= 1.0, (name, raw, excess, worst)


@pytest.mark.parametrize("epi,drop", CASES, ids=IDS)
def test_emulated_outputs_pass(epi, drop):
    """an f32 emulation of the epilogue on the exact accumulator passes the gate (BIAS_GELU_DGELU by both of its
    formulas)"""
    r = _ref(epi, drop)
    for vec in (True, False):
        res = G.check(r, **G.emulate(r, vec))
        print({k: round(v[0], 3) for k, v in res.items()})
        assert not G.failures(res), G.failures(res)


# ---- planted faults ----------------------------------------------------------------------------------------------
ROWS, COLS = slice(16, 32), slice(8, 16)      # one 16-row block, one 8-column chunk


def _flagged(r, got, rows=slice(0, M), cols=slice(0, N), names=None):
    """the gate fails, and every failing output's location lies inside the planted region"""
    res = G.check(r, **got)
    bad = {k: v for k, v in res.items() if not v[0] <= 1.0}
    assert bad, res
    assert names is None or set(bad) <= set(names), bad
    for name, (ratio, loc) in bad.items():
        if name == "partial":
            assert rows.start // RPT <= loc[0] <= (rows.stop - 1) // RPT and cols.start <= loc[1] < cols.stop, bad
        else:
            assert rows.start <= loc[1] < rows.stop and cols.start <= loc[2] < cols.stop, (name, loc)
    assert G.failures(res)


def _splice(good, bad, rows, cols, names=("C", "C2")):
    out = {k: v.clone() for k, v in good.items()}
    for k in names:
        if k in out:
            out[k][:, rows, cols] = bad[k][:, rows, cols]
    return out


def _bump(t, loc, ulps):
    """t[loc] moved `ulps` units in the last place away from zero"""
    it = t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    it[loc] += ulps


@pytest.mark.parametrize("epi,drop", CASES, ids=IDS)
def test_one_element_changed(epi, drop):
    """one element off by one unit in the last place (exact outputs), or by 2 bf16 ulps where the gate is a bound"""
    r = _ref(epi, drop)
    for name in [k for k in r.out if k != "partial"]:
        got = G.emulate(r)
        if r.bound[name] is None:
            loc, ulps = (0, 21, 13), 1
            if float(got[name][loc]) == 0:
                loc = (0, 22, 13)
        else:
            # 2 ulps exceed U |ref| + c s once U |ref| / 2 > c s: the element where |ref| / s is largest
            ratio = r.out[name].abs() / (r.bound[name] - G.U * r.out[name].abs()).clamp_min(1e-30)
            loc, ulps = G.worst(ratio, torch.zeros_like(ratio), torch.ones_like(ratio))[1], 2
            got[name][loc] = G.expected(r.out[name], got[name].dtype)[loc]
        _bump(got[name], loc, ulps)
        _flagged(r, got, slice(loc[1], loc[1] + 1), slice(loc[2], loc[2] + 1), names=[name])


@pytest.mark.parametrize("epi,drop", CASES, ids=IDS)
def test_chunk_swapped_with_neighbour(epi, drop):
    r = _ref(epi, drop)
    got = G.emulate(r)
    for name in [k for k in got if k != "partial"]:
        t = got[name]
        a, b = t[0, 21, 8:16].clone(), t[0, 21, 16:24].clone()
        t[0, 21, 8:16], t[0, 21, 16:24] = b, a
    _flagged(r, got, slice(21, 22), slice(8, 24))


@pytest.mark.parametrize("epi,drop", [c for c in CASES if c[0] in G.HAS_BIAS],
                         ids=[i for c, i in zip(CASES, IDS) if c[0] in G.HAS_BIAS])
def test_bias_shifted_by_8_columns(epi, drop):
    """one chunk of one 16-row block computed with bias[n + 8]"""
    A, B, bias, aux, cls, mult, Am, Bm, kw = _case(epi, drop)
    r = G.reference(epi, Am, Bm, M, N, K, **kw)
    shifted = G.reference(epi, Am, Bm, M, N, K, **dict(kw, bias=torch.roll(bias, -8, 1)))
    _flagged(r, _splice(G.emulate(r), G.emulate(shifted), ROWS, COLS), ROWS, COLS)


@pytest.mark.parametrize("epi,drop", [c for c in CASES if c[0] in G.HAS_AUX],
                         ids=[i for c, i in zip(CASES, IDS) if c[0] in G.HAS_AUX])
def test_aux_from_next_row(epi, drop):
    """one 16-row block (a staging pass) computed with aux row m + 1 (PATCH: the position row of token t + 1)"""
    A, B, bias, aux, cls, mult, Am, Bm, kw = _case(epi, drop)
    r = G.reference(epi, Am, Bm, M, N, K, **kw)
    auxm = kw["aux"]
    moved = G.reference(epi, Am, Bm, M, N, K, **dict(kw, aux=torch.roll(auxm, -1, 0)))
    _flagged(r, _splice(G.emulate(r), G.emulate(moved), ROWS, slice(0, N)), ROWS)


@pytest.mark.parametrize("epi,drop", [c for c in CASES if c[0] in G.HAS_C2],
                         ids=[i for c, i in zip(CASES, IDS) if c[0] in G.HAS_C2])
def test_c_and_c2_exchanged(epi, drop):
    r = _ref(epi, drop)
    got = G.emulate(r)
    _flagged(r, {"C": got["C2"], "C2": got["C"]})
    # ... and on one chunk of one block only
    _flagged(r, _splice(got, {"C": got["C2"], "C2": got["C"]}, ROWS, COLS), ROWS, COLS)


@pytest.mark.parametrize("epi,drop", CASES, ids=IDS)
def test_row_of_partial_tile_unwritten(epi, drop):
    """the last row of the partial block keeps its NaN prefill"""
    r = _ref(epi, drop)
    got = G.emulate(r)
    for name in [k for k in got if k != "partial"]:
        got[name][0, M - 1, :] = float("nan")
    _flagged(r, got, slice(M - 1, M))


def test_splitk_slab_duplicated():
    """split-K over 3 k-ranges: the slabs sum to the product exactly; slab 0 written in slab 1's place does not"""
    A, B, bias, aux, cls, mult, Am, Bm, kw = _case(G.SPLITK)
    r = G.reference(G.SPLITK, Am, Bm, M, N, K, **kw)
    a, b = A.float(), B.float()
    cut = [0, 64, 192, K]
    slabs = torch.stack([a[:, :, k0:k1] @ b[:, k0:k1] for k0, k1 in zip(cut, cut[1:])], 1)     # [1, 3, M, N]
    assert not G.failures(G.check(r, C=slabs.sum(1)))
    slabs[:, 1] = slabs[:, 0]
    _flagged(r, {"C": slabs.sum(1)})
