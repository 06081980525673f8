"""Every epilogue of the bf16 MFMA GEMM on every tile config, store path and operand layout, against the float64
reference of gemm_ref.py with its per-element gate (bit equality for the linear epilogues, U |ref| + c s for the
GELU ones).

One pytest case per (tile config, epilogue); inside, the rest of the matrix as a few dozen tiny launches, counted
and the count asserted, so that no part of it can drop out silently.

Shapes: M = 293 = 256 + 37 and N = 296 / 300 put a whole tile, a row-partial, a column-partial and the corner tile
into one launch for 256- and 128-wide tiles alike (PATCH: M = 295 = 59 x 5 tokens, so cls rows fall into whole and
partial tiles). The three forms of N reach the three store paths:
    N = 296, ldc = 296   d.vec set, no ragged chunk: whole tiles on the register-resident path, the rest on the
                         8-column path (also the col_partial form)
    N = 300, ldc = 304   d.vec set, every row ends in a 4-column scalar tail next to its vector chunks
    N = 300, ldc = 301   d.vec clear: every element on the scalar path, whole tiles included
K = 64 is one 64-deep k-tile (two 32-deep ones), fewer than any pipeline depth; K = 320 is five (ten), an odd count
for the half-tile schedule. C, C2 and aux have three different leading dimensions; C / C2 are prefilled with NaN
and the padding of aux is NaN: inside [M, N] no NaN may appear and outside it every NaN must survive.

Empty split (K = 64, split_k = 3: a split without a k-tile). Read before it was first run: with nk = 0 all three
kernel bodies issue no LDS-DMA, wait vmcnt(0) on nothing, and both wave groups meet exactly one workgroup barrier
(the prologue's) before the epilogue: gemm_bf16_kernel's k loop is empty for every wave; gemm_pp_kernel's group 0
loop is empty and group 1's slots are behind `else if (nk > 0)`; pp2_tile the same. With nk > 0 both groups of
gemm_pp_kernel pass 1 + 2 nk barriers and of pp2_tile 1 + 2 nk. The epilogue then writes the zero accumulator.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref as G
from vitmi import _lib, ops

DEV = "cuda"
NAN = float("nan")
DROP = 16                                     # dropout variant of an epilogue (p = 0.5: multipliers 0 and 2)
SEED, OFF = 0x1234ABCD5678, 3 << 20
K_CONTIG, MN_CONTIG = G.K_CONTIG, G.MN_CONTIG
KK, KM = (K_CONTIG, K_CONTIG), (K_CONTIG, MN_CONTIG)

EPILOGUES = list(range(10)) + [G.BIAS_RESID_F32 | DROP, G.PATCH | DROP, G.BIAS_GELU_DGELU | DROP]
EPI_IDS = [G.NAMES[e & 15] + ("+DROP" if e & DROP else "") for e in EPILOGUES]
TILE_ROWS = {0: 128, 1: 256, 2: 256, 3: 256, 4: 128, 5: 256, 6: 256, 7: 256, 8: 256, 9: 256}
# (N, ldc, ldc2, ldaux)
N_FORMS = [(296, 296, 304, 312), (300, 304, 312, 320), (300, 301, 312, 320)]
KS = (64, 320)
# launches per case: 3 forms of N x 2 K x 4 layouts = 24 (the dropout variants: x 1 layout, BIAS_RESID_F32 x 2);
# BIAS_RESID_F32 twice (out of place, in place); + 8 with col_partial (2 K x 4 layouts); + 6 batched (4 layouts of
# stacked batches, 2 of strided column blocks); SPLITK: 2 N x 2 K x 4 layouts unsplit + 2 splits x 2 N x 4 layouts
# + 2 N x 4 layouts of the empty split
LAUNCHES = {G.F32: 32, G.BF16: 38, G.BIAS_BF16: 38, G.BIAS_GELU: 24, G.BIAS_RESID_F32: 56, G.GELU_BWD: 32, G.PATCH: 24,
            G.SPLITK: 40, G.BIAS_GELU_DGELU: 24, G.MUL_BF16: 32, G.BIAS_RESID_F32 | DROP: 24, G.PATCH | DROP: 6,
            G.BIAS_GELU_DGELU | DROP: 6}


def test_enums_match_the_library():
    assert [getattr(_lib, "EPI_" + n) for n in G.NAMES] == list(range(10))
    assert (_lib.K_CONTIG, _lib.MN_CONTIG) == (G.K_CONTIG, G.MN_CONTIG)


@functools.lru_cache(maxsize=None)
def _operands(gelu, M, N, K, al, bl, batch):
    """exact A [batch, M, K], B [batch, K, N] on the device, packed per batch and stacked: Am, Bm, lda, ldb (shared by
    every case and never written)"""
    g = torch.Generator().manual_seed(1000 * K + M + N)
    A, B = G.exact_ab(G.BIAS_GELU if gelu else G.F32, M, N, K, g, batch)
    A, B = A.to(DEV), B.to(DEV)
    packed = [G.pack(A[z], B[z], al, bl) for z in range(batch)]
    Am, Bm = torch.stack([p[0] for p in packed]), torch.stack([p[1] for p in packed])
    return Am, Bm, packed[0][2], packed[0][3]


def _padded(t, ld, fill=NAN):
    """[rows, cols] -> a [rows, ld] buffer, the padding columns filled"""
    buf = torch.full((t.shape[0], ld), fill, device=DEV, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf


class Sweep:
    """the launches of one (tile config, epilogue) case, their failures and worst gate ratios"""

    def __init__(self, cfg, epi):
        self.cfg, self.epi, self.drop = cfg, epi & 15, bool(epi & DROP)
        self.launches, self.fails, self.worst, self.abs_c = 0, [], {}, {}

    def _gate(self, tag, r, **got):
        res = G.check(r, **got)
        self.fails += G.failures(res, tag + " ")
        for name, t in got.items():
            if r.bound[name] is None:
                continue
            self.worst[name] = max(self.worst.get(name, 0.0), res[name][0])
            if name != "partial":
                # the absolute term alone, to hold against c: the largest (|err| - U |ref|) / s
                ref, c = r.out[name], (G.C_DGELU if self.epi == G.BIAS_GELU_DGELU else G.C_PHI)
                s = (r.bound[name] - G.U * ref.abs()) / c
                ex = ((t.double() - ref).abs() - G.U * ref.abs()).clamp_min(0)[s > 0] / s[s > 0]
                self.abs_c[name] = max(self.abs_c.get(name, 0.0), float(torch.nan_to_num(ex, nan=0.0).max()))

    def _untouched(self, tag, buf, M, N, ld, batch=1, bs=0):
        """inside the logical [batch, M, N] of buf no NaN, outside it nothing but the NaN prefill"""
        inside = torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
        G.strided(inside, M, N, ld, batch, bs)[:] = True
        nan = torch.isnan(buf.reshape(-1))
        if bool((nan & inside).any()):
            self.fails.append(f"{tag}: NaN inside [M, N]")
        if not bool(nan[~inside].all()):
            at = int((~nan & ~inside).nonzero()[0])
            self.fails.append(f"{tag}: padding overwritten at flat element {at} (row {at // ld}, col {at % ld})")

    def run(self, M, N, K, al, bl, ldc, ldc2=0, ldaux=0, inplace=False, col_partial=False, batch=1, blocks=False,
            split_k=1):
        cfg, epi, drop = self.cfg, self.epi, self.drop
        tag = (f"cfg {cfg} {G.NAMES[epi]}{'+DROP' if drop else ''} M={M} N={N} K={K} layouts=({al},{bl}) ldc={ldc}"
               f"{' inplace' if inplace else ''}{' col_partial' if col_partial else ''}"
               f"{f' batch={batch}' if batch > 1 else ''}{' blocks' if blocks else ''}"
               f"{f' split_k={split_k}' if split_k > 1 else ''}:")
        G.assert_exact(epi, K)
        odt = G.out_dtype(epi)
        Am, Bm, lda, ldb = _operands(epi in G.GELU_EPIS, M, N, K, al, bl, batch)
        a_bs, b_bs = (Am[0].numel(), Bm[0].numel()) if batch > 1 else (0, 0)
        c_bs, bias_bs, c_rows = (M * ldc if batch > 1 else 0), 0, batch * M
        if blocks:
            # batches as strided column blocks of shared rows (the LoRA data gradient of resvit_fused.py):
            # A [M][batch K], batch z its columns z K ..; C [M][ldc], batch z its columns z c_bs ..
            assert al == K_CONTIG and batch > 1
            Am, lda, a_bs = Am.permute(1, 0, 2).reshape(M, batch * K).contiguous(), batch * K, K
            c_bs, c_rows = (N + 7) // 8 * 8, M
            assert ldc >= batch * c_bs
        kw = dict(a_layout=al, b_layout=bl, lda=lda, ldb=ldb, batch=batch, a_bs=a_bs, b_bs=b_bs)
        rkw = dict(kw)
        if epi in G.HAS_BIAS:
            bias_bs = 0 if batch == 1 else (N + 7) // 8 * 8 + 24         # distinct from a_bs, b_bs and c_bs
            bias = _padded(G.exact_bias(epi, N, batch).to(DEV), max(N, bias_bs))
            kw.update(bias=bias, bias_bs=bias_bs)
            rkw.update(bias=bias, bias_bs=bias_bs)
        C = torch.full((c_rows, ldc), NAN, device=DEV, dtype=odt)
        if epi in G.HAS_AUX:
            tokens = 5 if epi == G.PATCH else 0
            aux = G.exact_aux(epi, tokens or M, N).to(DEV)
            if inplace:
                assert epi == G.BIAS_RESID_F32 and ldaux == ldc
                C[:, :N] = aux
                auxm = C
            else:
                auxm = _padded(aux, ldaux)
            kw.update(aux=auxm, ldaux=ldaux, tokens=tokens)
            rkw.update(aux=auxm, ldaux=ldaux, tokens=tokens)
            if epi == G.PATCH:
                cls = G.exact_cls(N).to(DEV)
                kw.update(aux2=cls)
                rkw.update(aux2=cls)
        C2 = None
        if epi in G.HAS_C2:
            C2 = torch.full((M, ldc2), NAN, device=DEV, dtype=odt)
            kw.update(C2=C2, ldc2=ldc2)
        if drop:
            d = ops.dropout_desc(0.5, 3, SEED, OFF)
            mult = torch.empty(M, N, device=DEV)
            ops.dropout_mask(d, 0, M, N, mult, N)
            assert sorted(mult.unique().tolist()) == [0.0, 2.0]
            kw.update(dropout=d)
            rkw.update(mult=mult)
        kw.update(ldc=ldc, c_bs=c_bs, epilogue=epi, tile=cfg, split_k=split_k)
        rows = ops.gemm_tile_rows(Am, Bm, C, M, N, K, **kw)
        assert rows == TILE_ROWS[cfg], (tag, rows)           # the config the case is about is the one that runs
        part = None
        if col_partial:
            tiles = (M + rows - 1) // rows
            part = torch.full((tiles + 1, N), NAN, device=DEV)          # one guard row
            kw.update(col_partial=part)
            rkw.update(rows_per_tile=rows)
        r = G.reference(epi, Am, Bm, M, N, K, **rkw)          # before the launch: in place, C is an operand
        if epi == G.SPLITK:
            ws = torch.full((split_k * M * N + 64,), NAN, device=DEV)   # slabs [split][M][N] and a guard
            ops.gemm(Am, Bm, ws, M, N, K, **kw)
            self.launches += 1
            slabs = ws[:split_k * M * N].view(split_k, M, N)
            if not bool(torch.isfinite(slabs).all()):
                self.fails.append(f"{tag} a slab holds a NaN or an infinity")
            if not bool(torch.isnan(ws[split_k * M * N:]).all()):
                self.fails.append(f"{tag} wrote past the last slab")
            self._gate(tag, r, C=slabs.double().sum(0)[None])
            return
        ops.gemm(Am, Bm, C, M, N, K, **kw)
        self.launches += 1
        got = dict(C=G.strided(C, M, N, ldc, batch, c_bs))
        self._untouched(tag + " C", C, M, N, ldc, batch, c_bs)
        if C2 is not None:
            got["C2"] = G.strided(C2, M, N, ldc2)
            self._untouched(tag + " C2", C2, M, N, ldc2)
        if part is not None:
            got["partial"] = part[:-1]
            if not bool(torch.isnan(part[-1]).all()):
                self.fails.append(f"{tag} col_partial guard row overwritten")
        self._gate(tag, r, **got)


@pytest.mark.parametrize("epi", EPILOGUES, ids=EPI_IDS)
@pytest.mark.parametrize("cfg", range(10))
def test_gemm_epilogue_sweep(cfg, epi):
    sw = Sweep(cfg, epi)
    e, drop = epi & 15, bool(epi & DROP)
    M = 295 if e == G.PATCH else 293
    layouts = G.LAYOUTS if not drop else [KK, KM] if e == G.BIAS_RESID_F32 else [KK]
    if e == G.SPLITK:
        # tile = 0 picks the half-tile kernel for a split-K GEMM from 256 x 256 up: M = 165 = 128 + 37 keeps config 0
        M = 165 if cfg == 0 else 293
        for N in (296, 300):                      # d.vec set / clear (slab rows are N long)
            for al, bl in layouts:
                for K, split in ((64, 1), (320, 1), (320, 2), (320, 3), (64, 3)):
                    sw.run(M, N, K, al, bl, ldc=N, split_k=split)
    else:
        for N, ldc, ldc2, ldaux in N_FORMS:
            for K in KS:
                for al, bl in layouts:
                    sw.run(M, N, K, al, bl, ldc, ldc2, ldaux)
                    if e == G.BIAS_RESID_F32:
                        sw.run(M, N, K, al, bl, ldc, ldc2, ldc, inplace=True)
        if e in G.HAS_COL_PARTIAL and not drop:
            N, ldc, ldc2, ldaux = N_FORMS[0]
            for K in KS:
                for al, bl in layouts:
                    sw.run(M, N, K, al, bl, ldc, ldc2, ldaux, col_partial=True)
        if e in (G.BF16, G.BIAS_BF16):
            for al, bl in layouts:
                sw.run(M, 300, 64, al, bl, ldc=304, batch=3)
            for al, bl in (KK, KM):
                sw.run(M, 44, 64, al, bl, ldc=152, batch=3, blocks=True)
    print(f"GATE cfg={cfg} epi={EPI_IDS[EPILOGUES.index(epi)]} launches={sw.launches} "
          f"worst={ {k: round(v, 4) for k, v in sw.worst.items()} } abs_term={ {k: f'{v:.3g}' for k, v in sw.abs_c.items()} }")
    assert sw.launches == LAUNCHES[epi], (sw.launches, LAUNCHES[epi])
    assert not sw.fails, f"{len(sw.fails)} failures, the first: " + "\n".join(sw.fails[:8])
