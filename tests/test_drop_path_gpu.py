"""Stochastic depth (drop-path) on the GPU: the multiplier table, the GEMM epilogue and LayerNorm-backward variants per
element, a whole training step against the oracle, "off means off", accumulation, and the standalone module.

Gates. The GEMM cases use gemm_ref's exact operands (integer A, B, bias, residual; power-of-two multipliers), so its
gate for BIAS_RESID_F32 holds unchanged: every element equals the float64 value rounded once to f32. The one case the
exact operands cannot cover is dropout at p = 0.1, whose multiplier 1/0.9 is not a power of two: there the branch
u * dm * ps (u an exact integer, dm the f32 multiplier the reference also uses, ps a power of two) takes one f32
rounding and the residual add (fused or not) one more, so |got - ref| <= 2^-24 |u dm ps| + 2^-24 |ref|, doubled for the
comparison against a float64 reference rounded to f32. The LayerNorm cases use norm_ref's gates as they are, with
mult = dropout multiplier x sample scale (products of a power of two with the dropout multiplier: exact).
"""
import functools
import math

import numpy as np
import pytest
import torch

import gemm_ref as G
import norm_ref as NR
from oracle.dropout import dropout_mult
from oracle.vit_oracle import ViTConfig, init_params, loss_and_grads, tame_params
from vitmi import ops
from vitmi._lib import EPI_BIAS_RESID_F32, K_CONTIG, MN_CONTIG

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED, OFF = 0x1234_5678_9ABC_DEF1, 0x2_0000_0007  # tests/test_dropout_gpu.py's
RESID = EPI_BIAS_RESID_F32


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def scales_ref(rates, B, seed, off):
    """the CPU restatement: [sites, B] from the numpy oracle's dropout multipliers of (row b, col 0)"""
    return torch.from_numpy(np.stack([dropout_mult(p, 0x80000000 | s, seed, off, B, 1)[:, 0]
                                      for s, p in enumerate(rates)]))


# ---- 1. the table ----------------------------------------------------------------------------------------------------
def test_scale_table_matches_the_oracle_and_the_dropout_mask_kernel():
    rates, B = [0.0, 0.25, 0.25, 0.5], 8
    out = torch.full((4, B), -1.0, device=DEV)
    ops.drop_path_scales(rates, B, SEED, OFF, out)
    want = scales_ref(rates, B, SEED, OFF)
    assert torch.equal(out.cpu(), want)
    assert torch.equal(out[0].cpu(), torch.ones(B))
    assert not torch.equal(out[1], out[2])  # same rate, independent sites
    for s, p in enumerate(rates):
        vals = set(out[s].tolist())
        assert vals <= {0.0, float(np.float32(1.0 / (1.0 - p)))}, (s, vals)
        m = torch.empty(B, 1, device=DEV)
        ops.dropout_mask(ops.dropout_desc(p, 0x80000000 | s, SEED, OFF) if p else None, 0, B, 1, m, 1)
        assert torch.equal(m[:, 0], out[s]), s


# ---- 2. the GEMM epilogue --------------------------------------------------------------------------------------------
RPS = 197


def sample_scales(n, gen):
    """zeros, ones and other powers of two, every value present"""
    v = torch.tensor([0.0, 2.0, 1.0, 4.0])[torch.randint(0, 4, (n,), generator=gen)]
    assert n >= 4
    v[:4] = torch.tensor([2.0, 0.0, 4.0, 1.0])
    return v


def run_gemm_case(M, N, K, bl, p_drop, inplace, tile=0, null_check=False):
    gen = torch.Generator().manual_seed(1000 + M + N + 7 * bl + tile)
    G.assert_exact(RESID, K)
    A, B = G.exact_ab(RESID, M, N, K, gen)
    Am, Bm, lda, ldb = G.pack(A[0].to(DEV), B[0].to(DEV), K_CONTIG, bl)
    bias = G.exact_bias(RESID, N)[0].to(DEV)
    R = G.exact_aux(RESID, M, N).to(DEV)
    nsamp = -(-M // RPS)
    scale = sample_scales(nsamp, gen).to(DEV)
    rows = scale[torch.arange(M, device=DEV) // RPS]
    dm = torch.ones(M, N, device=DEV)
    d = None
    if p_drop:
        d = ops.dropout_desc(p_drop, 3, SEED, OFF)
        ops.dropout_mask(d, 0, M, N, dm, N)
    kw = dict(a_layout=K_CONTIG, b_layout=bl, lda=lda, ldb=ldb, ldc=N, epilogue=RESID, bias=bias, ldaux=N, dropout=d,
              tile=tile)
    C = R.clone() if inplace else torch.full((M, N), float("nan"), device=DEV)
    ops.gemm_drop_path(Am, Bm, C, M, N, K, ops.drop_path_desc(scale, RPS), aux=C if inplace else R, **kw)
    r = G.reference(RESID, Am, Bm, M, N, K, a_layout=K_CONTIG, b_layout=bl, lda=lda, ldb=ldb, bias=bias, aux=R, ldaux=N,
                    mult=dm * rows[:, None])
    if p_drop and p_drop != 0.5:  # the derived gate of the module docstring
        branch = (r.u * r.mult).abs()
        r.bound["C"] = 2.0 * 2.0 ** -24 * (branch + r.out["C"].abs())
    res = G.check(r, C=C[None])
    print(f"M{M} N{N} K{K} bl{bl} p{p_drop} inplace{inplace} tile{tile}: {res}")
    assert not G.failures(res), G.failures(res)
    dropped = rows == 0
    assert bool(dropped.any()) and bool((rows > 1).any())
    assert torch.equal(C[dropped], R[dropped])  # a dropped sample's rows are the residual, exactly
    if null_check:  # a NULL descriptor is vit_gemm_bf16
        C0, C1 = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
        ops.gemm(Am, Bm, C0, M, N, K, aux=R, **kw)
        ops.gemm_drop_path(Am, Bm, C1, M, N, K, None, aux=R, **kw)
        assert torch.equal(C0, C1)
    return Am, Bm, C, kw, R


@pytest.mark.parametrize("bl", [K_CONTIG, MN_CONTIG], ids=["b_k", "b_mn"])
@pytest.mark.parametrize("p_drop,inplace", [(0.0, False), (0.0, True), (0.5, False), (0.1, True)],
                         ids=["plain", "inplace", "drop0.5", "drop0.1-inplace"])
def test_gemm_epilogue_straddled_tiles(bl, p_drop, inplace):
    """985 x 256 x 64, 5 samples of 197 rows: tiles straddle samples and the last one is partial"""
    run_gemm_case(985, 256, 64, bl, p_drop, inplace, null_check=not p_drop and not inplace)


@pytest.mark.parametrize("tile", [3, 5, 9], ids=["256x128", "pingpong", "halftile"])
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
def test_gemm_epilogue_on_every_256_row_kernel(tile, p_drop):
    """the same case forced onto the 256-row kernels the large shapes pick (whole tiles: the register-resident
    epilogue with the multipliers prefetched; the last tile: the generic path)"""
    run_gemm_case(985, 256, 64, MN_CONTIG if tile != 3 else K_CONTIG, p_drop, False, tile=tile)


@pytest.mark.parametrize("p_drop", [0.0, 0.5])
def test_gemm_epilogue_scalar_store_path(p_drop):
    """N = ldc = ldaux = 100: no 8-wide store anywhere"""
    run_gemm_case(985, 100, 64, K_CONTIG, p_drop, False)


def test_gemm_epilogue_wave_split():
    """50432 x 768 x 64 (256 samples): the whole-wave rows on the half-tile kernel, the remainder on 128-row tiles
    indexed by the absolute row"""
    M, N, K = 50432, 768, 64
    Am, Bm, C, kw, R = run_gemm_case(M, N, K, K_CONTIG, 0.5, True)
    assert ops.gemm_split_rows(Am, Bm, C, M, N, K, aux=R, **kw) > 0


def test_gemm_drop_path_refuses_other_epilogues():
    from vitmi._lib import EPI_BF16, VitHipError
    A = torch.zeros(128, 64, device=DEV, dtype=torch.bfloat16)
    C = torch.zeros(128, 128, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(VitHipError):
        ops.gemm_drop_path(A, A, C, 128, 128, 64, ops.drop_path_desc(torch.ones(1, device=DEV), 128),
                           a_layout=K_CONTIG, b_layout=K_CONTIG, lda=64, ldb=64, ldc=128, epilogue=EPI_BF16)


# ---- 3. LayerNorm backward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [None, 1, 7], ids=["nodrop", "stride1", "stride7"])
@pytest.mark.parametrize("D", [768, 200])
def test_layernorm_bwd_drop_path(D, stride):
    rows, rps = 333, 37
    gen = torch.Generator().manual_seed(D + (stride or 0))
    x = (torch.randn(rows, D, generator=gen) * 2 + 1).to(DEV)
    gam = torch.randn(D, generator=gen).to(DEV)
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)
    dy = torch.randn(rows, D, generator=gen).to(DEV).bfloat16()
    dres = torch.randn(rows, D, generator=gen).to(DEV)
    rs = stride or 1
    nsamp = -(-(rows * rs) // rps)
    scale = sample_scales(nsamp, gen).to(DEV)
    srow = scale[(torch.arange(rows, device=DEV) * rs) // rps]
    d = ops.dropout_desc(0.1, 9, SEED, OFF, row_stride=stride) if stride else None
    dm = torch.ones(rows, D, device=DEV)
    if d is not None:
        dm = torch.from_numpy(dropout_mult(0.1, 9, SEED, OFF, rows, D, 0, stride)).to(DEV)
    nparts = ops.layernorm_bwd_partial_rows(rows)

    def run(path):
        dx = torch.empty(rows, D, device=DEV)
        dxb = torch.full((rows, D), float("nan"), device=DEV, dtype=torch.bfloat16)
        part = torch.empty(nparts, 3 * D, device=DEV)
        dgb, dsum = torch.empty(2 * D, device=DEV), torch.empty(D, device=DEV)
        ops.layernorm_bwd(dy, D, x, D, mean, rstd, gam, dx, D, part, rows, D, dres=dres, lddres=D, dx_bf16=dxb, lddxb=D,
                          dgamma_dbeta=dgb, dx_colsum=dsum, dx_dropout=d, dx_path=path)
        return dx, dxb, dgb, dsum

    dx0, _, dgb0, _ = run(None)
    dx, dxb, dgb, dsum = run(ops.drop_path_desc(scale, rps))
    assert torch.equal(dx, dx0) and torch.equal(dgb, dgb0)  # the residual gradient and dgamma | dbeta are untouched
    r = NR.bwd(dy.float(), x, mean, rstd, gam, dres=dres, mult=dm * srow[:, None])
    w16 = G.worst(dxb.float(), r.dxm, r.b_dx16)
    (_, _, cs), (_, _, bs) = NR.colsums(r, rows)
    wcs = G.worst(dsum, cs, bs)
    print(f"D{D} stride{stride}: bf16 copy {w16}, colsum {wcs}")
    assert w16[0] <= 1.0 and wcs[0] <= 1.0
    dropped = srow == 0
    assert bool(dropped.any()) and bool((srow > 1).any())
    assert bool((dxb[dropped].float() == 0).all())


# ---- 4. the whole step against the oracle ----------------------------------------------------------------------------
CFG = ViTConfig(image_size=32, patch_size=8, emb_dim=64, mlp_dim=128, num_heads=2, num_layers=3, num_classes=10)
BS = 8


@functools.lru_cache(maxsize=None)
def step_problem():
    params = tame_params(init_params(CFG, seed=42))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(BS, 3, 32, 32, generator=g)
    y = torch.randint(0, 10, (BS,), generator=g)
    return params, x, y, loss_and_grads(params, x, y, CFG)[0]


def build(dropout_rate=0.0, **kw):
    from vitmi.model import VisionTransformer
    torch.manual_seed(42)
    m = VisionTransformer(image_size=(32, 32), patch_size=(8, 8), emb_dim=64, mlp_dim=128, num_heads=2, num_layers=3,
                          num_classes=10, attn_dropout_rate=0.0, dropout_rate=dropout_rate, **kw)
    m.load_state_dict(step_problem()[0])
    return m.cuda().train()


@pytest.mark.parametrize("dropout_rate", [0.0, 0.1])
def test_train_step_with_drop_path_matches_oracle(dropout_rate):
    from vitmi.model import CrossEntropyLoss
    params, x, y, ref_eval = step_problem()
    m = build(dropout_rate, drop_path_rate=0.5)
    logits = m(x.cuda())
    loss = CrossEntropyLoss()(logits, y.cuda())
    loss.backward()
    eng = m.engine()
    L, N, D, M = CFG.num_layers, CFG.num_tokens, CFG.emb_dim, CFG.mlp_dim
    seed, off = eng.drop_seed, eng._drop_offset
    assert off == 1 and eng._path == [0.0, 0.0, 0.25, 0.25, 0.5, 0.5] and not eng._pruned
    assert (eng._drop is None) == (dropout_rate == 0.0)
    sc = scales_ref(eng._path, BS, seed, off)
    assert torch.equal(eng.acts(BS).path_scale.cpu(), sc)
    for s, p in enumerate(eng._path):  # the condition: every active site keeps and drops at least one sample
        if p > 0:
            assert bool((sc[s] == 0).any()) and bool((sc[s] > 0).any()), (s, sc[s])
    # the draw of torch.manual_seed(42), offset 1, as the numpy oracle gives it
    assert seed == (42 * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & (2**64 - 1)
    dropped = [set(torch.nonzero(sc[s] == 0).flatten().tolist()) for s in range(2, 6)]
    assert dropped == [{6}, {3, 4, 6}, {0, 1, 2, 4, 5}, {0, 2, 4}], dropped
    T = BS * N
    if dropout_rate:
        mk = lambda site, cols: torch.from_numpy(dropout_mult(dropout_rate, site, seed, off, T, cols)).view(BS, N, cols)
    else:
        mk = lambda site, cols: torch.ones(BS, N, cols)
    drop = {"pos": mk(0, D)}
    for i in range(L):
        drop[("attn", i)] = mk(1 + 3 * i, D) * sc[2 * i][:, None, None]
        drop[("d1", i)] = mk(2 + 3 * i, M)
        drop[("d2", i)] = mk(3 + 3 * i, D) * sc[2 * i + 1][:, None, None]
    ref_logits, ref_loss, ref_grads = loss_and_grads(params, x, y, CFG, drop=drop)
    print("logits", rel(logits, ref_logits), "loss", float(loss.detach()), float(ref_loss))
    assert rel(logits, ref_logits) < 1e-2
    assert abs(float(loss.detach()) - float(ref_loss)) <= 1e-3 * abs(float(ref_loss))
    tot = math.sqrt(sum(float(v.double().norm()) ** 2 for v in ref_grads.values()))
    named = dict(m.named_parameters())
    for k, gr in ref_grads.items():
        mine = named[k].grad
        if k.endswith("attn.key.bias") or float(gr.double().norm()) < 1e-4 * tot:
            assert float((mine.double().cpu() - gr.double()).norm()) <= 1e-3 * tot, k
        else:
            assert rel(mine, gr) < 3e-2, (k, rel(mine, gr))
    m.eval()
    with torch.no_grad():
        ev = m(x.cuda())
    assert rel(ev, ref_eval) < 1e-2


# ---- 5. off means off; accumulation ----------------------------------------------------------------------------------
def test_rate_zero_is_bit_identical_to_a_model_without_the_keyword():
    from vitmi.model import CrossEntropyLoss
    _, x, y, _ = step_problem()
    outs = []
    for kw in ({}, {"drop_path_rate": 0.0}):
        m = build(**kw)
        logits = m(x.cuda())
        CrossEntropyLoss()(logits, y.cuda()).backward()
        assert m.engine()._path is None and m.engine()._drop_offset == 0 and m.engine()._pruned
        outs.append((logits.detach().clone(), m.engine().grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_accumulation_draws_a_table_per_micro_step_and_sums_bit_for_bit(monkeypatch):
    from test_accum_step_gpu import CFG as ACFG, BS as ABS, force_split_1, problem
    from test_parity_gpu import make_model
    force_split_1(monkeypatch)
    params, x, y, _ = problem()
    eng = make_model(ACFG, params)
    eng(x[:1])
    eng = eng._engine
    tables = []

    def step(sl, accumulate):
        eng.forward(x[sl], drop_path_rate=0.5)
        tables.append(eng.acts(4).path_scale.clone())
        dl, _ = eng.cross_entropy(y[sl], grad_scale=1.0 / ABS)
        if accumulate:
            eng.backward(dl, eng.grad, accumulate=True)
        else:
            eng.backward(dl)
        torch.cuda.synchronize()
        return eng.grad.detach().clone()

    a, b = slice(0, 4), slice(4, 8)
    eng._drop_offset = 0
    parts = [step(a, False), step(b, False)]  # offsets 1 and 2
    assert eng._drop_offset == 2 and not torch.equal(tables[0], tables[1])
    eng._drop_offset = 0
    step(a, False)
    got = step(b, True)
    assert torch.equal(tables[2], tables[0]) and torch.equal(tables[3], tables[1])
    want = parts[0] + parts[1]
    assert torch.equal(got, want), (int((got != want).sum()), float((got - want).abs().max()))


# ---- 6. the standalone module ----------------------------------------------------------------------------------------
def test_functional_drop_path_forward_and_backward():
    import vitmi.functional as HF
    x = torch.randn(4, 17, 64, device=DEV, requires_grad=True)
    y = HF.drop_path(x, 0.5, True)
    sc = scales_ref([0.5], 4, HF._DROP_SEED, HF._DROP_OFFSET[0])[0].to(DEV)
    assert torch.equal(y, x.detach() * sc[:, None, None])
    dy = torch.randn_like(x)
    y.backward(dy)
    assert torch.equal(x.grad, dy * sc[:, None, None])
    assert HF.drop_path(x, 0.5, False) is x and HF.drop_path(x, 0.0, True) is x


def test_encoder_block_train_differs_from_eval():
    from vitmi.model import DropPath, EncoderBlock
    torch.manual_seed(3)
    blk = EncoderBlock(64, 128, 2, dropout_rate=0.0, attn_dropout_rate=0.0, drop_path_rate=0.5).cuda()
    x = torch.randn(8, 17, 64, device=DEV)
    with torch.no_grad():
        ev = blk.eval()(x)
        outs = [blk.train()(x) for _ in range(3)]  # (three draws: 2^-48 that every one keeps every sample)
    assert any(not torch.equal(o, ev) for o in outs)
    assert torch.equal(blk.eval()(x), ev)
    dp = DropPath(0.5).cuda()
    assert dp.eval()(x) is x
