"""The weight-gradient scheduler: every trainable weight's gradient is out[z] (+)= A[z]^T B[z] over K token rows, one
Spec each. A launch runs its specs over a common K as split-K f32 slabs plus the fixed-order, deterministic
vit_splitk_reduce, or directly at split 1 in the table form. plan() alone lays the slabs out and assembles what the
kernel wrappers take; three launch forms run it:
    single  one spec: ops.gemm (EPI_SPLITK) + ops.splitk_reduce (ops.wgrad; the engine's per-GEMM path)
    group   up to 4 specs at their own or a common split: one ops.gemm_splitk_group + one ops.splitk_reduce_group
    table   any number of specs with M, N >= 256 at a common split, ops.GEMM_TABLE_MAX per prepared launch
The workspace is the caller's (`alloc`: numel -> an f32 tensor of at least that size; default a fresh one); the split
factors are ops.splitk_factor / ops.splitk_factor_group, looked up on `ops` at call time."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import ops
from ._lib import EPI_SPLITK, MN_CONTIG


class Spec(NamedTuple):
    """out[z] ([M][N] f32, row stride ldo, z < batch at stride out_bs) (+)= sum_t A[z][t][m] B[z][t][n]: bf16 operands,
    token-major (M/N-contiguous, row strides lda / ldb, z at strides a_bs / b_bs), K a multiple of 64, rows past the
    data zero. `out` may be a sequence of `batch` tensors, one destination per z (`accumulate` then a flag or a
    matching sequence of flags; out_bs unused)."""
    A: torch.Tensor
    lda: int
    B: torch.Tensor
    ldb: int
    M: int
    N: int
    out: object
    ldo: int
    batch: int = 1
    a_bs: int = 0
    b_bs: int = 0
    out_bs: int = 0
    accumulate: object = False


# a table member's `direct` value for "direct, adding into its destination" (vit_gemm_group_prepare's direct[i] == 2);
# plain direct members carry True, slab members False
DIRECT_ACCUMULATE = 2


def timed(probe, tail, fn, *args, **kw):
    """fn(*args, **kw); when `probe` is a list, between two timing events on the current stream, and
    (start, end, *tail) appended to it"""
    if probe is None:
        return fn(*args, **kw)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    fn(*args, **kw)
    ev1.record()
    probe.append((ev0, ev1, *tail))


def _tail(probe, specs, K, grouped):
    """the (flop, K, grouped) of a probe entry; nothing is computed while no probe list is set"""
    return None if probe is None else (sum(2.0 * sp.M * sp.N * K * sp.batch for sp in specs), K, grouped)


def _slabs(specs, splits):
    return sum(sp.batch * s * sp.M * sp.N for sp, s in zip(specs, splits))


def _alloc(alloc, sp, numel):
    return alloc(numel) if alloc else torch.empty(numel, device=sp.A.device, dtype=torch.float32)


def _gemm_kw(sp, s, ldc, c_bs=0):
    """ops.gemm's keywords for spec sp at split s (slabs: ldc = N, the kernel packs the z and split slabs itself)"""
    return dict(a_layout=MN_CONTIG, b_layout=MN_CONTIG, lda=sp.lda, ldb=sp.ldb, ldc=ldc, epilogue=EPI_SPLITK,
                batch=sp.batch, a_bs=sp.a_bs, b_bs=sp.b_bs, c_bs=c_bs, split_k=s)


def _reduce_jobs(sp, s, w):
    """ops.splitk_reduce_group jobs of spec sp's slabs w: one, or one per z for per-batch destinations"""
    if isinstance(sp.out, torch.Tensor):
        return [(w, sp.batch, s, sp.M, sp.N, sp.out, sp.ldo, sp.out_bs, sp.accumulate)]
    if len(sp.out) != sp.batch:
        raise ValueError(f"Spec.out: {len(sp.out)} destinations for batch {sp.batch}")
    acc = sp.accumulate if isinstance(sp.accumulate, (tuple, list)) else (sp.accumulate,) * sp.batch
    n = s * sp.M * sp.N
    return [(w[z * n:(z + 1) * n], 1, s, sp.M, sp.N, o, sp.ldo, 0, a) for z, (o, a) in enumerate(zip(sp.out, acc))]


def plan(specs, K, splits, ws, table=False):
    """Lay out one launch (pure: no library call). splits: one factor per spec; ws: the f32 workspace, the slabs packed
    into it in spec order, batch * s * M * N floats each. Returns
      views    each spec's slab view of ws (None for a direct member),
      members  as ops.gemm_splitk_group takes them, (A, B, C, M, N, K, kwargs); with table=True as ops.GemmGroupTable
               does, (..., kwargs, direct): a spec at split 1 is direct, writing out[z*out_bs + m*ldo + n] itself
               (direct = DIRECT_ACCUMULATE when the spec accumulates: the launch's epilogue adds into it),
      jobs     as ops.splitk_reduce_group takes them, (ws, batch, split, M, N, out, ldo, out_bs, accumulate)."""
    views, members, jobs, o = [], [], [], 0
    for sp, s in zip(specs, splits):
        if table and s == 1:
            if not isinstance(sp.out, torch.Tensor):
                raise ValueError("a direct member writes one strided destination, not a list of per-z destinations")
            if not isinstance(sp.accumulate, (bool, int)):
                raise ValueError("a direct member takes one accumulate flag")
            views.append(None)
            members.append((sp.A, sp.B, sp.out, sp.M, sp.N, K, _gemm_kw(sp, 1, sp.ldo, sp.out_bs),
                            DIRECT_ACCUMULATE if sp.accumulate else True))
            continue
        n = _slabs([sp], [s])
        w = ws[o:o + n]
        o += n
        views.append(w)
        members.append((sp.A, sp.B, w, sp.M, sp.N, K, _gemm_kw(sp, s, sp.N)) + ((False,) if table else ()))
        jobs += _reduce_jobs(sp, s, w)
    return views, members, jobs


def single(sp, K, alloc=None, target=256, probe=None):
    """one spec at its own split: vit_gemm_bf16 into slabs, then their reduction"""
    s = ops.splitk_factor(sp.M, sp.N, K, sp.batch, target)
    ws = _alloc(alloc, sp, _slabs([sp], [s]))
    timed(probe, _tail(probe, [sp], K, False), ops.gemm, sp.A, sp.B, ws, sp.M, sp.N, K, **_gemm_kw(sp, s, sp.N))
    for job in _reduce_jobs(sp, s, ws):
        ops.splitk_reduce(*job)


def group(specs, K, common, alloc=None, target=256, probe=None):
    """up to 4 specs as one vit_gemm_splitk_group launch and one grouped reduction. common: all at the split of their
    summed grid; else each at the split single() gives it, so its sums are bit-identical to single()'s"""
    if common:
        splits = [ops.splitk_factor_group([(sp.M, sp.N, sp.batch) for sp in specs], K, target)] * len(specs)
    else:
        splits = [ops.splitk_factor(sp.M, sp.N, K, sp.batch, target) for sp in specs]
    _, members, jobs = plan(specs, K, splits, _alloc(alloc, specs[0], _slabs(specs, splits)))
    timed(probe, _tail(probe, specs, K, True), ops.gemm_splitk_group, members)
    ops.splitk_reduce_group(jobs)


def table(specs, K, tables, slot, alloc=None, target=256, probe=None):
    """specs (M, N >= 256) at their common split, one prepared launch per ops.GEMM_TABLE_MAX: direct at split 1 (the
    usual case: a backward's worth of tiles covers the CUs several times), else slabs and one grouped reduction after
    the last launch. tables: the caller's dict, (slot, first member) -> (key, ops.GemmGroupTable, reduce jobs); an
    entry is rebuilt (which synchronises the stream) only when its key changes: the split, K, the workspace and every
    member's pointers, strides, shapes and accumulate flag."""
    s = ops.splitk_factor_group([(sp.M, sp.N, sp.batch) for sp in specs], K, target)
    ws = _alloc(alloc, specs[0], _slabs(specs, [s] * len(specs))) if s > 1 else None
    jobs, o = [], 0
    for c0 in range(0, len(specs), ops.GEMM_TABLE_MAX):
        part = specs[c0:c0 + ops.GEMM_TABLE_MAX]
        key = (s, K, o, ws.data_ptr() if s > 1 else 0) + tuple(
            (sp.A.data_ptr(), sp.lda, sp.B.data_ptr(), sp.ldb, sp.M, sp.N, sp.out.data_ptr(), sp.ldo, sp.batch, sp.a_bs,
             sp.b_bs, sp.out_bs, bool(sp.accumulate)) for sp in part)
        ent = tables.get((slot, c0))
        if ent is None or ent[0] != key:
            _, members, red = plan(part, K, [s] * len(part), ws[o:] if s > 1 else None, table=True)
            ent = tables[(slot, c0)] = (key, ops.GemmGroupTable(members), red)
        timed(probe, _tail(probe, part, K, True), ent[1].launch)
        jobs += ent[2]
        o += _slabs(part, [s] * len(part)) if s > 1 else 0
    if jobs:
        ops.splitk_reduce_group(jobs)
