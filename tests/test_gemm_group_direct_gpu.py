"""The table form of the weight-gradient group (vit_gemm_group_prepare / vit_gemm_group_launch, ops.GemmGroupTable)
and its direct-output members, through the C ABI.

Operands are gemm_ref's exact integers, both M/N-contiguous (the only layout pair the group accepts). Every member's
expected result is the existing single call (vit_gemm_bf16, VIT_EPI_SPLITK) with the same split: a slab member's
slabs as they are, a direct member's split-1 slab reduced by vit_splitk_reduce into the same leading dimension and
batch stride. Same kernel body, same accumulation order: the comparison is bit for bit, over the whole output
buffers, which are filled with a canary first, so it also shows that nothing outside a member's M x N region (or its
slabs) was written. Each result also passes gemm_ref's per-element float64 gate.
"""
import functools

import pytest
import torch

import gemm_ref as G
from vitmi import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
MN = G.MN_CONTIG
CANARY = -12345.5  # no integer: never a product of the exact operands
GUARD = 64

# kind -> (M, N, K, batch, direct ldc - N, valid K rows, split when the member writes slabs)
KINDS = {
    "one_ktile": (256, 256, 64, 1, 0, None, 1),      # one k-tile; ldc = N
    "two_tiles": (512, 256, 192, 1, 8, None, 3),
    "batch3": (256, 256, 256, 3, 8, None, 4),        # stacked A, column blocks of B, c_bs > M ldc
    "ragged": (320, 264, 512, 1, 4, None, 8),        # partial tiles; ldc = 268 is no multiple of 8: scalar stores
    "zero_tail": (256, 256, 128, 1, 8, 65, 2),       # 65 valid token rows, zero rows after them
}
ORDER = list(KINDS)


@functools.lru_cache(maxsize=None)
def operands(kind):
    """(Am, Bm, call arguments, float64 reference) of a kind: built once, shared by every case, never written"""
    M, N, K, batch, _, valid, _ = KINDS[kind]
    G.assert_exact(G.SPLITK, K)
    gen = torch.Generator().manual_seed(1000 + ORDER.index(kind))
    A, B = G.exact_ab(G.SPLITK, M, N, K, gen, batch)           # [batch, M, K], [batch, K, N]
    if valid:
        A[:, :, valid:] = 0
        B[:, valid:, :] = 0
    lda = M
    Am = A.transpose(1, 2).contiguous().to(DEV)                 # [batch][K][lda]
    Bm = torch.cat(list(B), dim=1).contiguous().to(DEV)         # [K][batch N]: batch z in columns z N ...
    kw = dict(a_layout=MN, b_layout=MN, lda=lda, ldb=batch * N, batch=batch, a_bs=K * lda if batch > 1 else 0,
              b_bs=N if batch > 1 else 0)
    r = G.reference(G.SPLITK, Am, Bm, M, N, K, **kw)
    return Am, Bm, kw, r


class Plan:
    """members [(kind, direct)] laid out in one direct-output buffer and one slab buffer"""

    def __init__(self, members):
        self.members, self.place = members, []
        nd = ns = 0
        for kind, direct in members:
            M, N, K, batch, dld, _, split = KINDS[kind]
            if direct:
                ldc = N + dld
                c_bs = M * ldc + 64 if batch > 1 else 0
                self.place.append((nd, ldc, c_bs, 1))
                nd += (batch - 1) * c_bs + M * ldc + GUARD
            else:
                self.place.append((ns, N, 0, split))
                ns += batch * split * M * N + GUARD
        self.nd, self.ns = nd + GUARD, ns + GUARD

    def buffers(self):
        return (torch.full((self.nd,), CANARY, device=DEV), torch.full((self.ns,), CANARY, device=DEV))

    def workgroups(self):
        return sum(-(-KINDS[k][0] // 256) * -(-KINDS[k][1] // 256) * KINDS[k][3] * pl[3]
                   for (k, _), pl in zip(self.members, self.place))

    def run_group(self):
        out, slabs = self.buffers()
        table = []
        for (kind, direct), (off, ldc, c_bs, split) in zip(self.members, self.place):
            M, N, K = KINDS[kind][:3]
            Am, Bm, kw, _ = operands(kind)
            C = (out if direct else slabs)[off:]
            table.append((Am, Bm, C, M, N, K, dict(kw, ldc=ldc, c_bs=c_bs, epilogue=_lib.EPI_SPLITK, split_k=split),
                          direct))
        t = ops.GemmGroupTable(table)
        assert t.total == self.workgroups()
        t.launch()
        return out, slabs

    def run_separately(self):
        out, slabs = self.buffers()
        for (kind, direct), (off, ldc, c_bs, split) in zip(self.members, self.place):
            M, N, K, batch = KINDS[kind][:4]
            Am, Bm, kw, _ = operands(kind)
            skw = dict(kw, ldc=N, epilogue=_lib.EPI_SPLITK, split_k=split)
            if direct:
                ws = torch.full((batch * M * N,), CANARY, device=DEV)
                ops.gemm(Am, Bm, ws, M, N, K, **skw)
                ops.splitk_reduce(ws, batch, 1, M, N, out[off:], ldc, c_bs)
            else:
                ops.gemm(Am, Bm, slabs[off:], M, N, K, **skw)
        return out, slabs

    def check(self):
        got, want = self.run_group(), self.run_separately()
        torch.cuda.synchronize()
        for name, g, w in zip(("direct outputs", "slabs"), got, want):
            same = g == w
            assert bool(same.all()), f"{name}: {int((~same).sum())} elements differ, the first at {int((~same).nonzero()[0])}"
        fails = []
        for i, ((kind, direct), (off, ldc, c_bs, split)) in enumerate(zip(self.members, self.place)):
            M, N, K, batch = KINDS[kind][:4]
            r = operands(kind)[3]
            if direct:
                C = G.strided(got[0][off:off + (batch - 1) * c_bs + M * ldc], M, N, ldc, batch, c_bs)
            else:
                C = got[1][off:off + batch * split * M * N].view(batch, split, M, N).double().sum(1).float()
            fails += G.failures(G.check(r, C=C), f"member {i} ({kind}, {'direct' if direct else f'split {split}'}) ")
        assert not fails, "\n".join(fails[:8])


def test_enums_match():
    assert (G.SPLITK, G.MN_CONTIG) == (_lib.EPI_SPLITK, _lib.MN_CONTIG)
    assert ops.GEMM_TABLE_MAX >= 64


@pytest.mark.parametrize("kind", ORDER)
def test_one_direct_member(kind):
    Plan([(kind, True)]).check()


def test_five_direct_members():
    Plan([(k, True) for k in ORDER]).check()


def test_46_direct_members():
    p = Plan([(ORDER[i % 5], True) for i in range(46)])
    assert p.workgroups() == 100
    p.check()


def test_46_mixed_members_over_256_workgroups():
    """every other round of the five kinds writes slabs at its split, the rest directly"""
    p = Plan([(ORDER[i % 5], (i // 5) % 2 == 0) for i in range(46)])
    assert p.workgroups() > 256
    p.check()


def test_five_mixed_members():
    Plan([(k, i % 2 == 1) for i, k in enumerate(ORDER)]).check()


def test_direct_member_needs_split_1():
    Am, Bm, kw, _ = operands("two_tiles")
    out = torch.zeros(512 * 256, device=DEV)
    with pytest.raises(_lib.VitHipError):
        ops.GemmGroupTable([(Am, Bm, out, 512, 256, 192, dict(kw, ldc=256, epilogue=_lib.EPI_SPLITK, split_k=3), True)])
