"""Direct members of the weight-gradient table launch that add into their destination (vit_gemm_group_prepare's
direct[i] == 2), through the C ABI, exact.

Operands are gemm_ref's exact integers in [-4, 4], both M/N-contiguous; destinations are pre-filled with integers of
magnitude up to 1000, a function of (z, m, n) that is constant along no row and no column. Every value is then exact
in f32 (|prefill + 2 A^T B| <= 1000 + 2 * 16 * 192), so the gate is equality, element by element, with
prefill + A^T B computed in float64. Everything outside a member's [M, N] windows (the ldo padding, the gap of out_bs,
a guard band on both sides) holds a canary and is compared too: the whole buffer must equal the expected one.

Members, the smallest that reach every store path of the 256 x 256 tile:
    whole    (256, 256), ldo 256                 whole tile: the register-resident path, old values prefetched
    scalar   (256, 256), ldo 260                 ldo no multiple of 8 (vec = 0): the scalar path
    edge     (300, 264), ldo 272                 edge tiles in both directions: the generic 8-column path    
    qkv      (256, 320), batch 3, out_bs + 64    the q|k|v form: a B batch stride, a padded output batch stride
    tail     (264, 260), ldo 264                 N no multiple of 8: the last chunk of the 8-column path stores 4 scalars
K = 64 (one k-tile) and 192."""
import functools

import pytest
import torch

import gemm_ref as G
from vitmi import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
MN = G.MN_CONTIG
CANARY = -12345.5  # no integer: never a prefill value or a sum
GUARD = 64
KS = (64, 192)

# name -> (M, N, ldo, batch, out_bs)
MEMBERS = {
    "whole": (256, 256, 256, 1, 0),
    "scalar": (256, 256, 260, 1, 0),
    "edge": (300, 264, 272, 1, 0),
    "qkv": (256, 320, 320, 3, 256 * 320 + 64),
    "tail": (264, 260, 264, 1, 0),
}
ORDER = list(MEMBERS)


@functools.lru_cache(maxsize=None)
def operands(name, K):
    """(Am, Bm, gemm keywords, float64 A^T B [batch, M, N]) of a member: built once, shared, never written"""
    M, N, _, batch, _ = MEMBERS[name]
    G.assert_exact(G.SPLITK, K)
    gen = torch.Generator().manual_seed(2000 + 10 * ORDER.index(name) + K)
    A, B = G.exact_ab(G.SPLITK, M, N, K, gen, batch)            # [batch, M, K], [batch, K, N]
    lda = (M + 7) // 8 * 8
    Am = torch.zeros(batch, K, lda, dtype=torch.bfloat16)
    Am[:, :, :M] = A.transpose(1, 2)
    Am = Am.to(DEV)                                              # [batch][K][lda]
    ldb = (batch * N + 7) // 8 * 8                               # (rows of both operands start 16-B aligned)
    Bm = torch.zeros(K, ldb, dtype=torch.bfloat16)
    Bm[:, :batch * N] = torch.cat(list(B), dim=1)                # [K][ldb]: batch z in columns z N ...
    Bm = Bm.to(DEV)
    kw = dict(a_layout=MN, b_layout=MN, lda=lda, ldb=ldb, batch=batch, a_bs=K * lda if batch > 1 else 0,
              b_bs=N if batch > 1 else 0)
    r = G.reference(G.SPLITK, Am, Bm, M, N, K, **kw)
    return Am, Bm, kw, r.out["C"].cpu()


def prefill(batch, M, N):
    """integers in [-1000, 1000], constant along no row and no column, different per z (float64 [batch, M, N])"""
    z, m, n = torch.arange(batch)[:, None, None], torch.arange(M)[None, :, None], torch.arange(N)[None, None, :]
    return (((7 * m + 13 * n + 101 * z) % 2001) - 1000).double()


def window(buf, name, off):
    """the [batch, M, N] view of member `name` placed at element `off` of the flat buffer"""
    M, N, ldo, batch, out_bs = MEMBERS[name]
    return G.strided(buf[off:], M, N, ldo, batch, out_bs)


def span(name):
    M, N, ldo, batch, out_bs = MEMBERS[name]
    return (batch - 1) * out_bs + M * ldo


class Layout:
    """members side by side in one flat f32 buffer, a guard band around each"""

    def __init__(self, names):
        self.names, self.offs, o = names, [], GUARD
        for nm in names:
            assert o % 8 == 0
            self.offs.append(o)
            o += span(nm) + GUARD
        o = (o + 7) // 8 * 8
        self.numel = o

    def initial(self, fill=None):
        """float64 host buffer: the canary everywhere, each window its prefill (or `fill`)"""
        buf = torch.full((self.numel,), CANARY, dtype=torch.float64)
        for nm, off in zip(self.names, self.offs):
            M, N, _, batch, _ = MEMBERS[nm]
            window(buf, nm, off).copy_(prefill(batch, M, N) if fill is None else torch.full((batch, M, N), fill))
        return buf

    def members(self, dev_buf, K, direct):
        out = []
        for nm, off in zip(self.names, self.offs):
            M, N, ldo, batch, out_bs = MEMBERS[nm]
            Am, Bm, kw, _ = operands(nm, K)
            out.append((Am, Bm, dev_buf[off:], M, N, K,
                        dict(kw, ldc=ldo, c_bs=out_bs, epilogue=_lib.EPI_SPLITK, split_k=1), direct))
        return out

    def add(self, host64, K, times=1):
        for nm, off in zip(self.names, self.offs):
            window(host64, nm, off).add_(operands(nm, K)[3] * times)
        return host64


def assert_same(got, want64, what):
    got = got.cpu()
    want = want64.float()
    assert float((want.double() - want64).abs().max()) == 0.0  # the expectation itself is exact in f32
    same = got == want
    assert bool(same.all()), (f"{what}: {int((~same).sum())} elements differ, the first at {int((~same).nonzero()[0])}: "
                              f"got {float(got[~same][0])}, want {float(want[~same][0])}")


def run_accumulating(names, K):
    lay = Layout(names)
    # (every window starts 32-B aligned in the buffer, so `vec` is what the member's own strides say)
    dev = lay.initial().float().to(DEV)
    assert dev.data_ptr() % 32 == 0
    t = ops.GemmGroupTable(lay.members(dev, K, 2))
    t.launch()
    torch.cuda.synchronize()
    assert_same(dev, lay.add(lay.initial(), K), f"{names} K={K}, first launch")
    t.launch()
    torch.cuda.synchronize()
    assert_same(dev, lay.add(lay.initial(), K, 2), f"{names} K={K}, second launch")


def test_enums_match():
    assert (G.SPLITK, G.MN_CONTIG) == (_lib.EPI_SPLITK, _lib.MN_CONTIG)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ORDER)
def test_one_accumulating_member(name, K):
    run_accumulating([name], K)


@pytest.mark.parametrize("K", KS)
def test_all_members_in_one_table(K):
    run_accumulating(ORDER, K)


@pytest.mark.parametrize("K", KS)
def test_mixed_table(K):
    """an accumulating member, a plain direct member over a NaN-filled destination (finite, = A^T B afterwards) and a
    slab member at split 2 (exact slabs; the tensor it would later be reduced into is not part of the launch)"""
    acc, plain = Layout(["edge", "qkv"]), Layout(["whole", "scalar"])
    dacc = acc.initial().float().to(DEV)
    dplain = plain.initial(fill=float("nan")).float().to(DEV)
    M, N = MEMBERS["whole"][:2]
    slabs = torch.full((2 * M * N + 2 * GUARD,), CANARY, device=DEV)
    final = torch.full((M * N,), CANARY, device=DEV)
    Am, Bm, kw, ref = operands("whole", K)
    slab_member = (Am, Bm, slabs[GUARD:], M, N, K, dict(kw, ldc=N, epilogue=_lib.EPI_SPLITK, split_k=2), 0)
    t = ops.GemmGroupTable(acc.members(dacc, K, 2)[:1] + plain.members(dplain, K, 1) + [slab_member] +
                           acc.members(dacc, K, 2)[1:])
    for times in (1, 2):
        t.launch()
        torch.cuda.synchronize()
        assert_same(dacc, acc.add(acc.initial(), K, times), f"accumulating members, launch {times}")
        assert_same(dplain, plain.add(plain.initial(fill=0.0), K), f"plain direct members, launch {times}")
        s = slabs.cpu()
        assert bool((s[:GUARD] == CANARY).all()) and bool((s[GUARD + 2 * M * N:] == CANARY).all())
        assert torch.equal(s[GUARD:GUARD + 2 * M * N].view(2, M, N).double().sum(0), ref[0])
        assert bool((final == CANARY).all())


def test_accumulating_member_needs_split_1():
    K = 192
    Am, Bm, kw, _ = operands("whole", K)
    out = torch.zeros(256 * 256, device=DEV)
    with pytest.raises(_lib.VitHipError, match=rf"status {_lib_invalid_arg()}\)"):
        ops.GemmGroupTable([(Am, Bm, out, 256, 256, K, dict(kw, ldc=256, epilogue=_lib.EPI_SPLITK, split_k=2), 2)])
    assert float(out.abs().max()) == 0.0


def _lib_invalid_arg():
    return 1  # VIT_ERR_INVALID_ARG (include/vit_hip.h)
