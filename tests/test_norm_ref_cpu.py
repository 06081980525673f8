"""The per-element LayerNorm gates of norm_ref.py, proved without a GPU: the float64 references are what torch
computes, an f32 evaluation in the kernels' own summation order stays inside every gate (ratio <= 1) on the three
input families and at the widths 4, 100, 768 and 2048, and each planted fault that the row-norm tests let through
exceeds its gate (ratio > 1). Each ratio is printed ("RATIO name value", visible with pytest -s)."""
import pytest
import torch
import torch.nn.functional as Fn

import glue_ref as G
import norm_ref as N

WIDTHS = (4, 100, 768, 2048)
ROWS = 37
D_MID = 384


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _report(name, ratio):
    print(f"RATIO {name} {ratio:.4g}")
    return ratio


def _case(kind, D, rows=ROWS, seed=0):
    g = _gen(seed * 7919 + D)
    x = N.family(kind, rows, D, g)
    return x, torch.randn(D, generator=g), torch.randn(D, generator=g), g


def _fwd_ratios(x, gamma, beta, ref=None, eps_kernel=1e-5, **fault):
    """worst ratios (mean, rstd, y f32, y bf16) of the emulation against the gates (of eps 1e-5)"""
    ref = ref or N.fwd(x, gamma, beta)
    y, mean, rstd = N.fwd_emulate(x, gamma, beta, eps_kernel, **fault)
    return (G.worst(mean, ref.mean, ref.b_mean)[0], G.worst(rstd, ref.rstd, ref.b_rstd)[0],
            G.worst(y, ref.y, ref.b_y)[0], G.worst(y.bfloat16(), ref.y, ref.b_y16)[0])


def test_table_covers_all_32_kernels():
    seen = {N.kernel_of(D) for D in N.SWEEP_D}
    assert seen == {(nv, full) for nv in range(1, 9) for full in (False, True)}
    assert N.kernel_of(4) == (1, False) and N.kernel_of(256) == (1, True) and N.kernel_of(2044) == (8, False)
    # the row counts of the sweep: one block's waves, the 512-block cap, one wave prefetching, a third row for 5 waves
    assert N.bwd_blocks(1) == 1 and N.bwd_blocks(5) == 2 and N.bwd_blocks(2048) == 512 == N.bwd_blocks(4101)
    assert 4101 - 2 * 4 * 512 == 5 and 2049 - 4 * 512 == 1


@pytest.mark.parametrize("D", WIDTHS)
def test_references_are_torchs_layernorm(D):
    x, gamma, beta, g = _case("wide", D)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = Fn.layer_norm(x64, (D,), g64, b64, G.f32(1e-5))
    f = N.fwd(x, gamma, beta)
    assert float((f.y - y.detach()).abs().max()) < 1e-12
    dy, dres = torch.randn(ROWS, D, generator=g).bfloat16(), torch.randn(ROWS, D, generator=g)
    gx, gg, gb = torch.autograd.grad(y, (x64, g64, b64), dy.double())
    # the backward reference takes the f32 mean / rstd it is given: here the float64 ones, so it is torch's backward
    b = N.bwd(dy, x, f.mean, f.rstd, gamma, dres)
    assert float((b.dx - (gx + dres.double())).abs().max()) < 1e-11
    (dg, db, ds), _ = N.colsums(b, ROWS)
    assert float((dg - gg).abs().max()) < 1e-11 and float((db - gb).abs().max()) < 1e-12
    assert float((ds - (gx + dres.double()).sum(0)).abs().max()) < 1e-10


@pytest.mark.parametrize("D", WIDTHS)
def test_forward_gates_hold_and_catch_the_faults(D):
    worst = [0.0] * 4
    for kind in N.FAMILIES:
        x, gamma, beta, _ = _case(kind, D)
        worst = [max(a, b) for a, b in zip(worst, _fwd_ratios(x, gamma, beta))]
    for name, r in zip(("mean", "rstd", "y_f32", "y_bf16"), worst):
        assert _report(f"ln_fwd_emulated_{name}_D{D}", r) <= 1.0

    # a pack that truncates instead of rounding to nearest even
    x, gamma, beta, _ = _case("wide", D)
    ref = N.fwd(x, gamma, beta)
    y, _, _ = N.fwd_emulate(x, gamma, beta)
    assert _report(f"fault_truncating_pack_y_D{D}", G.worst(N.bf16_trunc(y), ref.y, ref.b_y16)[0]) > 1.0

    # eps = 1e-6: invisible on the wide family, far outside on rows of variance 1e-6
    x, gamma, beta, _ = _case("tight", D)
    r = _fwd_ratios(x, gamma, beta, eps_kernel=1e-6)
    assert _report(f"fault_eps_1e-6_rstd_D{D}", r[1]) > 1.0 and _report(f"fault_eps_1e-6_y_D{D}", r[2]) > 1.0

    # D - 1 in the variance
    x, gamma, beta, _ = _case("wide", D)
    r = _fwd_ratios(x, gamma, beta, var_div=D - 1)
    assert _report(f"fault_var_D-1_rstd_D{D}", r[1]) > 1.0 and _report(f"fault_var_D-1_y_D{D}", r[2]) > 1.0

    # a one-pass variance E[x^2] - mu^2 on rows of mean 1000
    x, gamma, beta, _ = _case("bigmean", D)
    r = _fwd_ratios(x, gamma, beta, one_pass=True)
    assert _report(f"fault_one_pass_rstd_D{D}", r[1]) > 1.0 and _report(f"fault_one_pass_y_D{D}", r[2]) > 1.0


def test_forward_one_wrong_element_is_caught():
    """10 % on one element of a 768-wide row moves the row-norm ratio by 3.6e-3 (under the old 5e-3 gate)"""
    x, gamma, beta, _ = _case("wide", 768)
    ref = N.fwd(x, gamma, beta)
    y = N.fwd_emulate(x, gamma, beta)[0].bfloat16().float()
    col = int(ref.y[3].abs().argsort()[D_MID])           # an element of median size
    y[3, col] = y[3, col] * 1.1
    assert float((y[3].double() - ref.y[3]).norm() / ref.y[3].norm()) < 5e-3       # what the row gate saw
    assert G.worst(y.bfloat16(), ref.y, ref.b_y16)[1] == (3, col)
    assert _report("fault_one_element_10pct_y_D768", G.worst(y.bfloat16(), ref.y, ref.b_y16)[0]) > 1.0


def test_constant_row_is_beta_and_rsqrt_eps():
    D = 768
    x = torch.full((3, D), 3.0)
    gamma, beta = torch.randn(D, generator=_gen(1)), torch.randn(D, generator=_gen(2))
    ref = N.fwd(x, gamma, beta)
    y, mean, rstd = N.fwd_emulate(x, gamma, beta)
    assert G.first_diff(y, beta[None, :].expand(3, D).contiguous(), bits=True) is None
    assert float(ref.b_mean.max()) > 0 and torch.equal(mean, torch.full((3,), 3.0))
    assert G.worst(rstd, ref.rstd, ref.b_rstd)[0] <= 1.0
    assert abs(float(ref.rstd[0]) - G.f32(1e-5) ** -0.5) < 1e-9
    assert _report("fault_eps_1e-6_rstd_constant_row", G.worst(N.fwd_emulate(x, gamma, beta, 1e-6)[2], ref.rstd,
                                                               ref.b_rstd)[0]) > 1.0


def _bwd_inputs(kind, D, rows=ROWS, p=0.0):
    x, gamma, beta, g = _case(kind, D, rows, seed=1)
    _, mean, rstd = N.fwd_emulate(x, gamma, beta)
    dy = torch.randn(rows, D, generator=g).bfloat16().float()
    dres = torch.randn(rows, D, generator=g)
    mult = None
    if p:
        mult = (torch.rand(rows, D, generator=g) >= p).float() * torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
    return x, gamma, mean, rstd, dy, dres, mult


@pytest.mark.parametrize("D", WIDTHS)
def test_backward_gates_hold_and_catch_the_faults(D):
    nv, _ = N.kernel_of(D)
    worst = {"dx": 0.0, "dx_nodres": 0.0, "dx_bf16": 0.0, "dx_bf16_dropout": 0.0}
    for kind in N.FAMILIES:
        x, gamma, mean, rstd, dy, dres, mult = _bwd_inputs(kind, D, p=0.25)
        for name, dr, mk in (("dx", dres, None), ("dx_nodres", None, None), ("dx_bf16_dropout", dres, mult)):
            ref = N.bwd(dy, x, mean, rstd, gamma, dr, mk)
            o, om, _ = N.bwd_emulate(dy, x, mean, rstd, gamma, dr, mk)
            if mk is None:
                worst[name] = max(worst[name], G.worst(o, ref.dx, ref.b_dx)[0])
                worst["dx_bf16"] = max(worst["dx_bf16"], G.worst(om.bfloat16(), ref.dxm, ref.b_dx16)[0])
            else:
                worst[name] = max(worst[name], G.worst(om.bfloat16(), ref.dxm, ref.b_dx16)[0])
    for name, r in worst.items():
        assert _report(f"ln_bwd_emulated_{name}_D{D}", r) <= 1.0

    x, gamma, mean, rstd, dy, dres, mult = _bwd_inputs("wide", D, p=0.25)
    ref = N.bwd(dy, x, mean, rstd, gamma, dres)
    o, _, _ = N.bwd_emulate(dy, x, mean, rstd, gamma, dres)
    assert _report(f"fault_truncating_pack_dx_bf16_D{D}", G.worst(N.bf16_trunc(o), ref.dxm, ref.b_dx16)[0]) > 1.0
    # rstd ~ 1/3 on this family: a chunk without it is three times too large
    o, _, _ = N.bwd_emulate(dy, x, mean, rstd, gamma, dres, no_rs_chunk=nv - 1)
    assert _report(f"fault_no_rs_in_one_chunk_dx_D{D}", G.worst(o, ref.dx, ref.b_dx)[0]) > 1.0
    if D > 256:     # with one chunk per lane the last chunk is the whole row
        o, _, _ = N.bwd_emulate(dy, x, mean, rstd, gamma, dres, m2_skip_last=True)
        assert _report(f"fault_m2_without_last_chunk_dx_D{D}", G.worst(o, ref.dx, ref.b_dx)[0]) > 1.0

    # dres read at dx's stride: another element (or the NaN padding) reaches dx
    flat, view = G.embed(dres, D + 8)
    wrong = flat.as_strided((ROWS, D), (D + 4, 1))
    o, _, _ = N.bwd_emulate(dy, x, mean, rstd, gamma, wrong)
    assert _report(f"fault_dres_at_lddx_dx_D{D}", G.worst(o, ref.dx, ref.b_dx)[0]) > 1.0


@pytest.mark.parametrize("rows,D", [(5, 100), (333, 768), (4101, 64), (4101, 768)])
def test_column_sum_gates_hold_and_catch_the_faults(rows, D):
    x, gamma, mean, rstd, dy, dres, mult = _bwd_inputs("wide", D, rows, p=0.25)
    prior = torch.randn(3, D, generator=_gen(5))
    for mk, pr, tag in ((None, None, ""), (mult, prior, "_dropout_acc")):
        ref = N.bwd(dy, x, mean, rstd, gamma, dres, mk)
        (dg, db, ds), (b_dg, b_db, b_ds) = N.colsums(ref, rows, pr)
        o, om, tg = N.bwd_emulate(dy, x, mean, rstd, gamma, dres, mk)
        add = (lambda k, v: v) if pr is None else (lambda k, v: pr[k] + v)
        got = [add(0, N.colsum_emulate(tg)), add(1, N.colsum_emulate(dy)), add(2, N.colsum_emulate(om))]
        for name, gt, rf, bd in zip(("dgamma", "dbeta", "dx_colsum"), got, (dg, db, ds), (b_dg, b_db, b_ds)):
            assert _report(f"ln_bwd_emulated_{name}{tag}_rows{rows}_D{D}", G.worst(gt, rf, bd)[0]) <= 1.0
        if mk is None:
            # one row missing from one column, a row whose term is at the 20th percentile of the column's sizes
            row = int(ref.t_g[:, D // 2].abs().argsort()[rows // 5])
            bad = N.colsum_emulate(tg, drop=(row, D // 2))
            assert _report(f"fault_row_dropped_dgamma_rows{rows}_D{D}", G.worst(bad, dg, b_dg)[0]) > 1.0
            assert G.worst(bad, dg, b_dg)[1] == (D // 2,)
            if (rows, D) == (4101, 768):
                assert float((bad.double() - dg).norm() / dg.norm()) < 1e-4        # what the vector gate saw
        else:
            bad = add(2, N.colsum_emulate(o))      # the unmasked dx summed under dropout
            assert _report(f"fault_unmasked_dx_colsum_rows{rows}_D{D}", G.worst(bad, ds, b_ds)[0]) > 1.0


def test_dbeta_on_integers_is_exact():
    rows, D = 4101, 64
    G.assert_exact_sum(rows, 8, start=8)
    dy = G.ints((rows, D), _gen(3))
    dy[4100, 63] = 3.0
    prior = G.ints((D,), _gen(4))
    want = (dy.double().sum(0) + prior.double()).float()
    assert G.first_diff(prior + N.colsum_emulate(dy), want) is None
    assert G.first_diff(prior + N.colsum_emulate(dy, drop=(4100, 63)), want)[0] == (63,)      # the last row dropped
