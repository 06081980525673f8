"""The per-element gates of glue_ref.py, proved without a GPU: each float64 reference is the operation torch
computes, a correctly rounded f32 evaluation of each kernel's formula passes its gate, and the small planted faults
that a whole-tensor norm lets through (one wrong tail element, a dropped last chunk, a row shifted by one, a segment
written to the wrong output, a touched guard column, a NaN-logit row counted as a hit; for the router kernels an unrolled
loop entered one group early, a truncating pack, reserve off by one, a late image index, ties taking index 1, the entropy
over reserved tokens or with the wrong sign, reserved tokens taking the hard gradient) are rejected."""
import math

import pytest
import torch
import torch.nn.functional as Fn

import glue_ref as G


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---- memory --------------------------------------------------------------------------------------------------------
def test_embed_and_touched_guard_column():
    t = G.ints((5, 7), _gen())
    flat, view = G.embed(t, 12, extra_rows=2, offset=3)
    assert torch.equal(view, t) and flat.numel() == 3 + 7 * 12 + 8
    assert int(flat.isnan().sum()) == flat.numel() - 35
    assert G.first_touched(flat, view) is None
    for at in (3 + 7, 2, 3 + 5 * 12, flat.numel() - 1):     # a guard column, the gap before, a row past the end, the end
        bad = flat.clone()
        bad[at] = 0.0
        assert G.first_touched(bad, bad[3:].as_strided((5, 7), (12, 1))) == at
    # a transposed (column-major) view is handled by its strides
    vt = flat[3:].as_strided((7, 5), (1, 12))
    assert G.first_touched(flat, vt) is None


def test_first_diff_values_bits_and_nans():
    a = torch.tensor([1.0, 0.0, G.NAN, 3.0])
    assert G.first_diff(a, a.clone()) is None
    assert G.first_diff(a, torch.tensor([1.0, -0.0, G.NAN, 3.0])) is None
    assert G.first_diff(a, torch.tensor([1.0, -0.0, G.NAN, 3.0]), bits=True)[0] == (1,)
    assert G.first_diff(a, torch.tensor([1.0, 0.0, G.NAN, 3.0000002]))[0] == (3,)
    assert G.first_diff(a, torch.tensor([1.0, 0.0, 2.0, 3.0]))[0] == (2,)
    other = (a.view(torch.int32) | torch.tensor([0, 0, 1, 0], dtype=torch.int32)).view(torch.float32)   # another NaN
    assert G.first_diff(a, other, bits=True)[0] == (2,)
    assert G.first_diff(a, other, bits=True, nan_by_kind=a.isnan()) is None


def test_worst_is_nan_aware():
    ref = torch.tensor([1.0, G.NAN, 2.0], dtype=torch.float64)
    bound = torch.tensor([0.5, 0.5, 0.0], dtype=torch.float64)
    assert G.worst(torch.tensor([1.25, G.NAN, 2.0]), ref, bound) == (0.5, (0,))
    assert G.worst(torch.tensor([1.0, 7.0, 2.0]), ref, bound) == (float("inf"), (1,))     # a NaN row written finite
    assert G.worst(torch.tensor([G.NAN, G.NAN, 2.0]), ref, bound) == (float("inf"), (0,))
    assert G.worst(torch.tensor([1.0, G.NAN, 2.0000002]), ref, bound) == (float("inf"), (2,))   # bound 0: exact


# ---- column sums ---------------------------------------------------------------------------------------------------
def _chunked_sum_f32(x, drop_last=False):
    """vit_colsum's two passes in f32: per-chunk partial rows, then their sum"""
    rows = x.shape[0]
    chunks, per = G.colsum_chunks(rows)
    parts = [x[k * per:min((k + 1) * per, rows)].sum(0) for k in range(chunks)]
    if drop_last:
        last = max(k for k in range(chunks) if k * per < rows)
        parts[last] = torch.zeros_like(parts[last])
    return torch.stack(parts).sum(0)


def test_colsum_chunk_geometry():
    assert G.colsum_chunks(1) == (1, 1) and G.colsum_chunks(127) == (1, 127)
    assert G.colsum_chunks(129) == (2, 65) and G.colsum_chunks(200) == (3, 67)
    assert G.colsum_chunks(4225) == (66, 65) and 65 * 65 == 4225            # the 66th chunk covers nothing
    empty = lambda r: (lambda c, per: (c - 1) * per >= r)(*G.colsum_chunks(r))
    assert not any(empty(r) for r in range(1, 4225)) and empty(4225)        # and it is the smallest such row count
    assert G.colsum_chunks(10 ** 6)[0] == 256


@pytest.mark.parametrize("rows", [1, 63, 129, 200, 4225])
def test_colsum_gate_exact_and_dropped_chunk(rows):
    G.assert_exact_sum(rows, 8, start=8)
    x = G.ints((rows, 16), _gen(rows))
    prior = G.ints((16,), _gen(1))
    want = G.colsum(x, prior).float()
    assert G.first_diff(_chunked_sum_f32(x) + prior, want) is None
    assert G.first_diff(_chunked_sum_f32(x.bfloat16().float()) + prior, want) is None      # bf16 holds the integers
    assert G.first_diff(_chunked_sum_f32(x, drop_last=True) + prior, want) is not None
    assert G.first_diff(_chunked_sum_f32(x), want) is not None                              # accumulate ignored
    if rows == 4225:
        assert _rel(_chunked_sum_f32(x, drop_last=True), G.colsum(x)) < 0.2   # a norm at 1e-2 on random data is no help


def test_colsum3_segment_to_wrong_output():
    seg = 8
    x = G.ints((40, 3 * seg), _gen(3))
    s = G.colsum(x).float()
    outs = [s[k * seg:(k + 1) * seg] for k in range(3)]
    for k in range(3):
        assert G.first_diff(outs[k], G.colsum(x[:, k * seg:(k + 1) * seg]).float()) is None
    assert G.first_diff(outs[2], G.colsum(x[:, seg:2 * seg]).float()) is not None           # out2 got segment 1's


def test_embed_grad_gate_and_shifted_row():
    B, N, D = 9, 17, 8
    G.assert_exact_sum(B * N, 16)
    dh0 = G.ints((B * N, D), _gen(4))
    mult = torch.randint(0, 2, (B * N, D), generator=_gen(5)).float() * 2
    for m in (None, mult):
        dpos, dcls, dcb = (t.float() for t in G.embed_grad(dh0, B, N, D, m))
        x = dh0 if m is None else dh0 * m
        got = x.reshape(B, N, D).sum(0)
        assert G.first_diff(got, dpos) is None and G.first_diff(got[0], dcls) is None
        assert G.first_diff(got[1:].sum(0), dcb) is None
        shifted = torch.roll(x, 1, 0).reshape(B, N, D).sum(0)                               # every row one too low
        assert G.first_diff(shifted, dpos) is not None
        assert G.first_diff(got.sum(0), dcb) is not None                                    # the cls row counted in
    dpos, _, dcb = G.embed_grad(dh0[:B], B, 1, D)
    assert float(dcb.abs().max()) == 0.0                                                    # N = 1: no patch rows


def test_sqnorm_and_cls_mse_exact():
    g = G.ints((1027,), _gen(6))
    G.assert_exact_sum(1027, 64)
    assert float((g.double() ** 2).sum()) == float((g * g).sum())
    B, D = 3, 257
    assert B * D * 256 < 2 ** 24
    x, t = G.ints((B, D), _gen(7)), G.ints((B, D), _gen(8))
    e, part, loss = G.cls_mse(x, t)
    assert G.first_diff(x - t, e.float()) is None
    assert G.first_diff(((x - t) ** 2).sum(1), part.float()) is None
    assert float(((x - t) ** 2).sum() / (B * D)) == float(loss.float())                    # the one division
    assert abs(float(loss) - float(Fn.mse_loss(x.double(), t.double()))) < 1e-12
    bad = ((x - t) ** 2)[:, :256].sum(1)                                                    # the loop's second pass lost
    assert G.first_diff(bad, part.float()) is not None


def test_cls_mse_bwd_gate():
    for B, D in ((1, 1), (3, 257)):
        dx0, e, g = G.cls_mse_bwd_case(B, D, _gen(9))
        ref, bound = G.cls_mse_bwd(dx0, e, g)
        x = e.double().requires_grad_(True)
        (Fn.mse_loss(x, torch.zeros_like(x)) * float(g)).backward()
        assert float((ref - dx0.double() - x.grad).abs().max()) < 1e-15
        norm = torch.tensor(2.0 / (B * D), dtype=torch.float32)
        unfused = dx0 + (norm * e) * g
        fused = (dx0.double() + (norm * e).double() * g.double()).float()                   # one rounding: an fma
        for got in (unfused, fused):
            assert G.worst(got, ref, bound)[0] <= 0.75
        bad = unfused.clone()
        bad[-1, -1] += 4 * float(bound[-1, -1])
        assert G.worst(bad, ref, bound) == (pytest.approx(4, rel=0.3), (B - 1, D - 1))


# ---- f32 GEMM --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 17, 150])
def test_gemm_f32_gate(K):
    M, N = 33, 31
    G.assert_exact_sum(K, 16, start=16)
    A, B = G.ints((M, K), _gen(K), -4, 4), G.ints((K, N), _gen(K + 1), -4, 4)
    bias, C0 = G.ints((N,), _gen(2)), G.ints((M, N), _gen(3))
    want = G.gemm_f32(A, B, bias, C0).float()
    got = A @ B + bias + C0
    assert G.first_diff(got, want) is None
    if K == 0:
        assert G.first_diff(want, bias + C0) is None
    bad = got.clone()
    bad[M - 1, N - 1] += 1                                                                  # one tail element
    assert G.first_diff(bad, want)[0] == (M - 1, N - 1)
    if K > 1:
        assert G.first_diff(A[:, :K - 1] @ B[:K - 1] + bias + C0, want) is not None         # the last k column dropped
        assert _rel(bad, want) < 1e-2


# ---- casts -----------------------------------------------------------------------------------------------------------
def test_cast_patterns_and_rounding_reference():
    x = G.cast_patterns()
    assert x.numel() == 393216 == 65536 * len(G.CAST_LOW_HALVES)
    nan = x.isnan()
    assert int(nan.sum()) == G.CAST_NAN_COUNT
    want = x.bfloat16()
    assert bool(want[nan].isnan().all())
    # torch's cast is round to nearest even on every non-NaN pattern (an independent integer formula)
    mine = G.bf16_rne_bits(x[~nan])
    theirs = want[~nan].view(torch.int16).to(torch.int64) & 0xffff
    assert torch.equal(mine, theirs)
    trunc = (x.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)                # a truncating cast
    assert G.first_diff(trunc, want, bits=True, nan_by_kind=nan) is not None
    assert G.first_diff(want.clone(), want, bits=True, nan_by_kind=nan) is None
    b = G.all_bf16()
    assert b.numel() == 65536 and torch.unique(b.view(torch.int16)).numel() == 65536
    up = b.float()
    assert torch.equal((up.view(torch.int32) >> 16).to(torch.int16), b.view(torch.int16))


def test_moves_row_shift_and_wrong_tail():
    x = torch.randn(7, 5, generator=_gen(10))
    want = x.bfloat16()
    assert G.first_diff(torch.roll(x, 1, 0).bfloat16(), want, bits=True) is not None
    bad = want.clone()
    bad[6, 4] = bad[6, 3]
    assert G.first_diff(bad, want, bits=True)[0] == (6, 4)


# ---- GELU ------------------------------------------------------------------------------------------------------------
def test_gelu_gates():
    u = G.gelu_inputs()
    assert u.numel() == 1291 and float(u.min()) == -40.0
    ref, bound = G.gelu(u)
    ur = u.double().requires_grad_(True)
    Fn.gelu(ur).sum().backward()
    assert float((ref - Fn.gelu(u.double())).abs().max()) < 1e-15
    got = 0.5 * u * (1.0 + torch.erf(u * 0.70710678118654752))
    assert G.worst(got, ref, bound)[0] <= 0.5
    bad = got.clone()
    bad[700] += 2 * float(bound[700])
    assert G.worst(bad, ref, bound)[1] == (700,)
    dy = torch.randn(u.numel(), generator=_gen(11))
    refb, boundb = G.gelu_bwd(u, dy)
    assert float((refb - dy.double() * ur.grad).abs().max()) < 1e-15
    cdf = 0.5 * (1.0 + torch.erf(u * 0.70710678118654752))
    gotb = dy * (cdf + u * (0.39894228040143268 * torch.exp(-0.5 * u * u)))
    assert G.worst(gotb, refb, boundb)[0] <= 0.5
    badb = gotb.clone()
    badb[-1] = 1.0                                                                          # dx of a denormal u
    assert not G.worst(badb, refb, boundb)[0] <= 1.0


# ---- cross entropy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C", [(3, 2), (65, 10), (3, 257), (65, 1000), (1, 1023)])
def test_cross_entropy_reference_and_gate(B, C):
    g = _gen(C)
    x = G.ce_logits(B, C, g)
    y = torch.randint(0, C, (B,), generator=g)
    for gs in (1.0, 1.0 / B):
        r = G.cross_entropy(x, y, gs)
        xr = x.double().requires_grad_(True)
        loss = Fn.cross_entropy(xr, y, reduction="none")
        (loss.sum() * G.f32(gs)).backward()
        assert float((r.loss - loss.detach()).abs().max()) < 1e-12
        assert float((r.dlogits - xr.grad).abs().max()) < 1e-15
        el, ed = G.ce_emulate(x, y, gs)
        assert G.worst(el, r.loss, r.bound_loss)[0] <= 0.5                                  # within E / 2
        assert G.worst(ed, r.dlogits, r.bound_d)[0] <= 0.5
        bad = el.double().clone()
        bad[B - 1] = r.loss[B - 1] + 2 * r.bound_loss[B - 1]                                # a planted 2 E
        assert G.worst(bad, r.loss, r.bound_loss)[1] == (B - 1,)
        badd = ed.double().clone()
        badd[B - 1, C - 1] = r.dlogits[B - 1, C - 1] + 2 * r.bound_d[B - 1, C - 1]          # one tail element
        ratio, at = G.worst(badd, r.dlogits, r.bound_d)
        assert at == (B - 1, C - 1) and ratio == pytest.approx(2, rel=1e-6)
        assert _rel(badd, r.dlogits) < 1e-5                                                 # invisible to a norm gate
    # a row shifted by one: every row gets its neighbour's gradient
    r = G.cross_entropy(x, y, 1.0)
    if B > 1:
        assert not G.worst(torch.roll(G.ce_emulate(x, y, 1.0)[1], 1, 0), r.dlogits, r.bound_d)[0] <= 1.0


def _topk_hits(x, y):
    top = x.topk(min(5, x.shape[1]), 1).indices
    return (top[:, 0] == y).double(), (top == y[:, None]).any(1).double()


def test_cross_entropy_hits_rule():
    nan = G.NAN
    # the issue's row: torch's top-1 is the NaN at index 1, a miss; counting x > x_y alone calls it a hit
    x = torch.tensor([[1.0, nan, 3.0, 2.0, 0.0, -1.0, 5.0]])
    y = torch.tensor([6])
    assert x.topk(1, 1).indices[0, 0] == 1
    t1, t5 = G.ce_hits(x, y)
    assert (float(t1), float(t5)) == (0.0, 1.0) == tuple(float(v[0]) for v in _topk_hits(x, y))
    old_top1 = ((x > x[:, 6:7]).sum(1) < 1).double()                                        # the parent's count
    assert float(old_top1) == 1.0 and G.first_diff(old_top1, t1) is not None               # rejected by the gate
    # all NaN: a miss; five NaN above a finite label: a top-5 miss; the label's own logit the only NaN: a hit
    rows = torch.tensor([[nan] * 7,
                         [nan, nan, nan, nan, nan, 1.0, 0.0],
                         [nan, nan, nan, nan, 0.5, 1.0, 0.0],
                         [0.0, 1.0, 2.0, nan, 3.0, 4.0, 5.0]])
    labels = torch.tensor([2, 5, 5, 3])
    t1, t5 = G.ce_hits(rows, labels)
    assert t1.tolist() == [0.0, 0.0, 0.0, 1.0] and t5.tolist() == [0.0, 0.0, 1.0, 1.0]
    k1, k5 = _topk_hits(rows[1:], labels[1:])                                               # determinate in torch
    assert k1.tolist() == t1[1:].tolist() and k5.tolist() == t5[1:].tolist()
    # random rows without ties: torch's order exactly
    g = _gen(12)
    for C in (2, 5, 6, 100):
        x = G.ce_logits(65, C, g)
        y = torch.randint(0, C, (65,), generator=g)
        t1, t5 = G.ce_hits(x, y)
        k1, k5 = _topk_hits(x, y)
        assert torch.equal(t1, k1) and torch.equal(t5, k5)
        if C == 5:
            assert bool(t5.all())
    # ties count for the label: tied for first with four others, tied for fifth place, six tied (label in any place)
    x = torch.tensor([[2.0, 2.0, 2.0, 2.0, 2.0, 1.0, 0.0],
                      [9.0, 8.0, 7.0, 6.0, 3.0, 3.0, 3.0],
                      [9.0, 8.0, 7.0, 6.0, 5.0, 3.0, 3.0]])
    t1, t5 = G.ce_hits(x, torch.tensor([4, 6, 6]))
    assert t1.tolist() == [1.0, 0.0, 0.0] and t5.tolist() == [1.0, 1.0, 0.0]
    # labels outside [0, C): NaN loss and gradient row, a miss, the neighbours untouched
    x = G.ce_logits(4, 6, g)
    y = torch.tensor([1, -1, 6, 2])
    r = G.cross_entropy(x, y, 0.25)
    assert r.loss.isnan().tolist() == [False, True, True, False]
    assert r.dlogits.isnan().all(1).tolist() == [False, True, True, False]
    assert r.top1[1:3].tolist() == [0.0, 0.0] and r.top5[1:3].tolist() == [0.0, 0.0]
    good = G.cross_entropy(x[[0, 3]], y[[0, 3]], 0.25)
    assert torch.equal(good.dlogits, r.dlogits[[0, 3]])


# ---- SGD -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [True, False])
def test_sgd_gate(first):
    n, lr, mom, wd = 1027, 0.1, 0.9, 1e-2
    g_ = _gen(13)
    p, g = torch.randn(n, generator=g_), torch.randn(n, generator=g_)
    buf = torch.full((n,), G.NAN) if first else torch.randn(n, generator=g_)
    pn, bn, bp, bb = G.sgd(p, g, buf, lr, mom, wd, first)
    # the reference is torch.optim.SGD's step in float64 (with the f32 hyper-parameters)
    w = p.double().clone().requires_grad_(True)
    opt = torch.optim.SGD([w], lr=G.f32(lr), momentum=G.f32(mom), weight_decay=G.f32(wd))
    if not first:
        opt.state[w]["momentum_buffer"] = buf.double().clone()
    w.grad = g.double().clone()
    opt.step()
    assert float((w.detach() - pn).abs().max()) < 1e-15
    assert float((opt.state[w]["momentum_buffer"] - bn).abs().max()) < 1e-15
    ep, eb = G.sgd_emulate(p, g, buf, lr, mom, wd, first)
    assert G.worst(ep, pn, bp)[0] <= 0.5 and G.worst(eb, bn, bb)[0] <= 0.5
    assert not bool(ep.isnan().any())                                                       # first: NaN buf never read
    bad = ep.clone()
    bad[n - 1] = p[n - 1]                                                                   # a tail element not stepped
    assert G.worst(bad, pn, bp)[1] == (n - 1,) and not G.worst(bad, pn, bp)[0] <= 1.0
    assert _rel(bad, pn) < 1e-2
    if not first:                                                                           # `first` taken when it is off
        assert not G.worst(G.sgd_emulate(p, g, buf, lr, mom, wd, True)[1], bn, bb)[0] <= 1.0


# ---- AdamW -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,nparts,seed,clip", G.ADAMW_PREP_CASES)
def test_adamw_prep_reference_and_ulp_gate(nseg, nparts, seed, clip):
    lr, b1, b2 = 1e-3, 0.9, 0.999
    partial, used, steps, max_norm = G.adamw_prep_case(nseg, nparts, seed, clip)
    table, st, norm, coef = G.adamw_prep(partial, used, steps, lr, b1, b2, max_norm)
    assert torch.equal(st, steps.double() + (used > 0).double())
    assert (coef < 1.0) == (clip and nparts > 0)
    if nparts:
        # the f32 chain of the kernel stays within one ulp of the float64 value for this case
        en, ec = G.adamw_prep_emulate(partial, max_norm)
        assert abs(en - norm) <= float(G.ulp32(torch.tensor(norm, dtype=torch.float64)))
        assert abs(ec - coef) <= float(G.ulp32(torch.tensor(coef, dtype=torch.float64)))
        # clip_grad_norm_'s coefficient
        gr = torch.zeros(nparts, dtype=torch.float64, requires_grad=True)
        gr.grad = partial.sqrt()
        tn = torch.nn.utils.clip_grad_norm_([gr], max_norm)
        assert abs(float(tn) - norm) < 1e-12 * max(norm, 1)
    act = used > 0
    assert bool((table[~act][:, :3] == 0).all()) and bool((table[:, 3] == coef).all())
    k = int(act.nonzero()[-1])
    s = float(st[k])
    assert float(table[k, 0]) == pytest.approx(G.f32(lr) / (1 - G.f32(b1) ** s), rel=1e-14)
    assert float(table[k, 1]) == pytest.approx(math.sqrt(1 - G.f32(b2) ** s), rel=1e-14)
    got = table.float()
    assert G.worst(got, table, G.ulp32(table) * (table != 0))[0] <= 0.5
    bad = got.clone()
    bad[nseg - 1] = torch.tensor([1.0, 1.0, 1.0, 1.0]) - bad[nseg - 1]                      # the last row's activity flipped
    assert G.worst(bad, table, G.ulp32(table) * (table != 0))[1][0] == nseg - 1


def test_adamw_reference_is_torch_and_gate():
    # hyper-parameters exact in f32, so the reference's f32 rounding of them is the identity and torch.optim.AdamW in
    # float64 is the same computation
    lr, b1, b2, eps, wd = 2.0 ** -10, 0.875, 0.984375, 2.0 ** -27, 0.25
    n, step = 1027, 3
    g_ = _gen(14)
    p, g, m = (torch.randn(n, generator=g_) for _ in range(3))
    v = torch.rand(n, generator=g_) + 1e-4
    step_size, bc2s, coef = lr / (1 - b1 ** step), math.sqrt(1 - b2 ** step), 1.0
    (pn, gn, mn, vn), bounds = G.adamw(p, g, m, v, step_size, bc2s, coef, lr, b1, b2, eps, wd)
    w = p.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([w], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[w] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.double().clone(),
                    "exp_avg_sq": v.double().clone()}
    w.grad = g.double().clone()
    opt.step()
    assert float((w.detach() - pn).abs().max()) < 1e-14
    assert float((opt.state[w]["exp_avg"] - mn).abs().max()) < 1e-15
    assert float((opt.state[w]["exp_avg_sq"] - vn).abs().max()) < 1e-15
    # the f32 update passes with its f32 table, clipped or not; planted faults do not
    for coef in (1.0, G.f32(0.37)):
        args = (G.f32(step_size), G.f32(bc2s), coef, lr, b1, b2, eps, wd)
        refs, bounds = G.adamw(p, g, m, v, *args)
        emu = G.adamw_emulate(p, g, m, v, *args)
        for got, ref, bound in zip(emu, refs, bounds):
            assert G.worst(got, ref, bound)[0] <= 0.5
        bad = emu[0].clone()
        bad[n - 1] = p[n - 1] * G.f32(1.0 - lr * wd)                                        # a tail element: decay only
        assert G.worst(bad, refs[0], bounds[0])[1] == (n - 1,)
        assert not G.worst(emu[2] * (1 + 2.0 ** -20), refs[2], bounds[2])[0] <= 1.0         # 16 ulp on every moment
        assert _rel(bad, refs[0]) < 1e-2


def test_adamw_layout_by_hand():
    starts, total, chunks, active = G.adamw_layout()
    assert starts == [0, 64, 128, 192, 256, 320, 1344, 9536] and total == 9536 + 8256
    assert all(s % 64 == 0 for s in starts) and active.count(False) == 1
    assert chunks.tolist()[-2:] == [[7, 9536, 8192], [7, 9536 + 8192, 3]]
    assert chunks.shape == (9, 3) and int(chunks[:, 2].max()) == 8192
    for s, n in enumerate(G.ADAMW_LENGTHS):
        assert int(chunks[chunks[:, 0] == s][:, 2].sum()) == n


# ---- Res-ViT router kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_rows", [0, 1, 3, 4, 5, 12, 13, 15, 16, 17, 29, 33])
def test_segment_colsum_gate_and_unroll_bound(seg_rows):
    G.assert_exact_sum(seg_rows + 12, 8)
    segs, row0, scale, cols = 3, 2, 0.25, 5
    stride = row0 + seg_rows + 3
    x = G.ints((segs * stride + 16, cols), _gen(seg_rows), 1, 8)             # (positive: a row read too many shows)
    want = G.segment_colsum(x, segs, seg_rows, stride, row0, scale).float()
    assert G.first_diff(G.segment_colsum_emulate(x, segs, seg_rows, stride, row0, scale), want) is None
    assert G.first_diff(G.segment_colsum_emulate(x.bfloat16(), segs, seg_rows, stride, row0, scale), want) is None
    # the unrolled loop entered at r + 8 < seg_rows reads row r + 12 past the segment for some row lane
    bad = G.segment_colsum_emulate(x, segs, seg_rows, stride, row0, scale, unroll_bound=8)
    reads_past = any(l + 8 < seg_rows <= l + 12 for l in range(4)) or any(
        l + 16 + 8 < seg_rows <= l + 16 + 12 for l in range(4))
    assert (G.first_diff(bad, want) is not None) == reads_past
    if seg_rows:
        assert G.first_diff(G.segment_colsum_emulate(x, segs, seg_rows, stride, row0 + 1, scale), want) is not None


@pytest.mark.parametrize("T,N,reserve", [(9, 3, 1), (33, 5, 0), (65, 50, 50), (7, 1, 1)])
def test_router_dx_gate_reference(T, N, reserve):
    cols, rows_pad, cols_pad = 6, T + 35, 8
    imgs = -(-T // N)
    g0 = _gen(T)
    dx, g = torch.randn(T, cols, generator=g0), torch.randn(imgs, cols, generator=g0)
    gp = torch.randn(T, cols, generator=g0).bfloat16()
    out, part = G.router_dx_gate(dx, g, 0.3, gp, T, N, reserve, rows_pad, cols_pad)
    assert out.shape == (rows_pad, cols_pad) and part.shape == (-(-rows_pad // 32), cols)
    assert float(out[T:].float().abs().max()) == 0.0 and float(out[:, cols:].float().abs().max()) == 0.0
    # element by element: three f32 roundings, then the independent integer round-to-nearest-even
    s = torch.tensor(0.3, dtype=torch.float32)
    loop = torch.empty(T, cols)
    for t in range(T):
        v = dx[t] + s * g[t // N] if t % N >= reserve else dx[t]
        loop[t] = v * gp[t].float()
    bits = out[:T, :cols].contiguous().view(torch.int16).to(torch.int64) & 0xffff
    assert torch.equal(bits, G.bf16_rne_bits(loop).reshape(T, cols))
    # planted: one rounding of the exact value (a fused evaluation), a truncating pack, reserve off by one, the image
    # index advanced one row late
    t = torch.arange(T)
    live = ((t % N) >= reserve)[:, None]
    trunc = (loop.view(torch.int32) >> 16).to(torch.int64) & 0xffff
    assert not torch.equal(trunc, bits)
    if N > 1 or reserve == 0:
        other = G.router_dx_gate(dx, g, 0.3, gp, T, N, (reserve + 1) % (N + 1), rows_pad, cols_pad)[0]
        assert G.first_diff(other, out, bits=True) is not None
    if imgs > 1 and reserve == 0:       # (with N = 1 every row names its own row of g)
        late = G.router_dx_gate(dx, g[((t - 1).clamp(min=0)) // N], 0.3, gp, T, 1, 0, rows_pad, cols_pad)[0]
        assert G.first_diff(late, out, bits=True) is not None
    # integer operands: the partials are exact, and a block's sum that skips its last data row is not
    G.assert_exact_sum(32, 96)
    dxi, gi = G.ints((T, cols), g0), G.ints((imgs, cols), g0)
    gpi = G.ints((T, cols), g0, 1, 4).bfloat16()
    outi, parti = G.router_dx_gate(dxi, gi, 0.5, gpi, T, N, reserve, rows_pad, cols_pad)
    seq = torch.zeros(parti.shape[0], cols)
    for r in range(T):
        seq[r // 32] = seq[r // 32] + outi[r, :cols].float()
    assert G.first_diff(seq, parti.float()) is None
    assert float(parti[-1].abs().max()) == 0.0                                   # a whole padding block
    assert torch.equal(outi[:T, :cols].float().double(), ((dxi.double() + torch.where(
        live, 0.5 * gi.double()[t // N], torch.zeros(T, cols, dtype=torch.float64))) * gpi.double()))


def test_router_select_reference():
    idx = G.router_select_case(4101, _gen(1))
    sets = [{0, 3, 31}, {1}, set(), set(range(32))]
    active, sel, anyf = G.router_select(idx, sets, 32)
    defined = ~idx.isnan() & (idx.abs() < 1e6)          # where torch's .long() is defined
    for j, st in enumerate(sets):
        want = torch.isin(idx[defined].long(), torch.tensor(sorted(st), dtype=torch.int64))
        assert torch.equal(active[j][defined], want)
        assert not bool(active[j][~defined].any())
    at = {float(v): int((idx == v).nonzero()[0]) for v in (-0.5, -1.0, 3.5, 31.0, 32.0)}
    assert bool(active[0][at[-0.5]]) and not bool(active[3][at[-1.0]]) and bool(active[0][at[3.5]])
    assert bool(active[0][at[31.0]]) and not bool(active[3][at[32.0]])
    assert not bool(sel[:, idx.isnan()].any()) and not bool(sel[3][at[3.5]])
    assert bool(anyf[13]) and int(sel[13].sum()) == 1 and bool(sel[13][-1])
    assert torch.equal(sel[0], idx == 0) and bool(sel[0][(idx == 0) & (torch.signbit(idx))].all())    # -0.0 == 0
    assert G.router_select(idx, [], 0)[1].shape == (0, 4101)


# (T, bs, N, reserve, noise_mode, training, y_hard given)
HEAD_CASES = [(513, 8, 57, 1, 1, True, False), (257, 2, 3, 0, 2, True, False), (255, 1, 5, 5, 0, True, True),
              (513, 8, 57, 1, 0, False, False), (256, 2, 4, 1, 0, False, True), (1, 8, 1, 0, 0, True, False)]


def _head_inputs(T, bs, mode, yh, seed):
    g = _gen(seed)
    x = G.router_head_logits(T, bs, g)
    noise = G.router_head_noise(T, bs, mode, g) if mode else None
    yhard = None
    if yh:
        h1 = torch.randint(0, 2, (T, bs), generator=g).float()
        yhard = torch.stack([1 - h1, h1], -1)
    return x, noise, yhard, g


@pytest.mark.parametrize("T,bs,N,reserve,mode,training,yh", HEAD_CASES)
def test_router_head_gates(T, bs, N, reserve, mode, training, yh):
    x, noise, yhard, g = _head_inputs(T, bs, mode, yh, T + bs)
    r = G.router_head_fwd(x, noise, mode, yhard, N, reserve, training, 100.0)
    soft, ysoft, hard, idx, ent = G.router_head_fwd_emulate(x, noise, mode, yhard, N, reserve, training, 100.0)
    assert float((r.soft - torch.softmax(x.double(), -1)).abs().max()) < 1e-15
    assert G.worst(soft, r.soft, r.b_soft)[0] <= 1.0
    if training:
        assert G.worst(ysoft, r.ysoft, r.b_ysoft)[0] <= 1.0
    # the 1 % cap on undecided one-hots holds on the reference alone (and the Gumbel grid leaves none)
    skipped = float((~r.decided).double().mean())
    assert skipped <= 0.01 and (mode == 2 or skipped == 0.0)
    sel = lambda got, ref, m: torch.where(m, got.double(), ref)
    assert G.worst(sel(hard, r.hard, r.decided[..., None]), r.hard, r.b_hard)[0] <= 1.0
    assert G.worst(sel(idx, r.indices, r.idx_decided), r.indices, r.b_idx)[0] <= 1.0
    if not training:
        assert float(r.b_hard.max()) == 0.0 and float(r.b_idx.max()) == 0.0                  # evaluation: equal
    assert G.worst(ent.reshape(1), r.ent.reshape(1), r.b_ent.reshape(1))[0] <= 1.0
    res = (torch.arange(T) % N) < reserve
    assert torch.equal(r.hard[res], torch.tensor([0.0, 1.0], dtype=torch.float64).expand(int(res.sum()), bs, 2))
    if not yh:
        tie = (x[..., 0] == x[..., 1]) & ~res[:, None] if mode == 0 else torch.zeros(T, bs, dtype=torch.bool)
        assert bool((r.hard[tie][:, 0] == 1.0).all()) and bool(r.decided[tie].all())         # exact ties: index 0
        if mode == 0 and bool(tie.any()):
            bad = hard.clone()
            bad[tie] = torch.tensor([0.0, 1.0])                                               # ties taking index 1
            assert not G.worst(sel(bad, r.hard, r.decided[..., None]), r.hard, r.b_hard)[0] <= 1.0
    if reserve and reserve < N:
        # the entropy summed over the reserved tokens too
        bad = G.router_head_fwd_emulate(x, noise, mode, yhard, N, 0, training, 100.0)[4]
        assert G.worst(bad.reshape(1), r.ent.reshape(1), r.b_ent.reshape(1))[0] > 1.0
    # backward, from the f32 soft / ysoft, with each gradient absent in turn
    grads = [torch.randn(T, bs, 2, generator=g), torch.randn(T, bs, 2, generator=g), torch.randn(T, generator=g),
             torch.randn((), generator=g)]
    for drop in range(5):
        a = [None if k == drop else t for k, t in enumerate(grads)]
        ref, bound = G.router_head_bwd(soft, ysoft, *a, N, reserve, training, 100.0)
        assert G.worst(G.router_head_bwd_emulate(soft, ysoft, *a, N, reserve, training, 100.0), ref, bound)[0] <= 1.0
        if a[3] is not None and reserve < N:
            bad = G.router_head_bwd_emulate(soft, ysoft, *a, N, reserve, training, 100.0, ent_sign=1.0)
            assert G.worst(bad, ref, bound)[0] > 1.0
        if training and reserve and (a[1] is not None or a[2] is not None):
            bad = G.router_head_bwd_emulate(soft, ysoft, *a, N, reserve, training, 100.0, reserved_take_hard=True)
            assert G.worst(bad, ref, bound)[0] > 1.0
    # the reference is autograd's gradient of the same function
    if training and not yh and mode != 2:
        xr = x.double().requires_grad_(True)
        p = torch.softmax(xr, -1)
        y = torch.softmax(xr + (noise.double() if mode else 0), -1)
        live = (~res)[:, None, None].double()
        entv = -(p * torch.log(p + G.f32(G.RH_C)) * live).sum() / 100.0
        w = 2.0 ** torch.arange(bs - 1, -1, -1, dtype=torch.float64)
        hardv = torch.where(res[:, None, None], torch.tensor([0.0, 1.0], dtype=torch.float64), (r.hard - y.detach()) + y)
        loss = (p * grads[0].double()).sum() + (hardv * grads[1].double()).sum() + \
            ((hardv[..., 1] * w).sum(1) * grads[2].double()).sum() + entv * grads[3].double()
        gx, = torch.autograd.grad(loss, xr)
        ref, _ = G.router_head_bwd(p.detach().float(), y.detach().float(), *grads, N, reserve, training, 100.0)
        assert float((ref - gx).abs().max()) < 1e-5
