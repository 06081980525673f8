"""ops.embed_grad(..., accumulate=True) (vit_embed_grad_accum): dpos, dcls and dconv_bias each become old + s, with s
bit for bit what the overwriting vit_embed_grad writes (the same summation order, one f32 add at the end). Random f32
inputs, so any other order of the sums would show. Cases: the vector position-gradient kernel's shapes (D % 4 == 0,
one and several column slices, B against its 8 image groups, N against the 16 row lanes of the bias sum), the scalar
kernel's (D % 4 != 0, or dh0 off its 16-B alignment), D no multiple of the 16-column workgroup, the cls row alone,
and the position-embedding dropout with an inexact multiplier (p = 0.1)."""
import pytest
import torch

from vitmi import ops

pytestmark = pytest.mark.gpu

GUARD = 32
CANARY = -12345.5

# (B, N, D, offset of dh0 in elements, dropout p)
CASES = [(1, 1, 4, 0, 0.0), (7, 2, 8, 0, 0.0), (8, 17, 388, 0, 0.1), (9, 33, 768, 0, 0.0), (17, 18, 772, 0, 0.0),
         (5, 50, 256, 0, 0.1), (7, 2, 300, 0, 0.1), (8, 17, 6, 0, 0.0), (17, 35, 50, 0, 0.0), (17, 2, 8, 1, 0.0)]


def guarded(n, gen=None):
    flat = torch.full((n + 2 * GUARD,), CANARY)
    if gen is not None:
        flat[GUARD:GUARD + n] = torch.randn(n, generator=gen)
    else:
        flat[GUARD:GUARD + n] = 0.0
    flat = flat.cuda()
    return flat, flat[GUARD:GUARD + n]


@pytest.mark.parametrize("B,N,D,offset,p", CASES)
def test_accumulate_adds_the_overwriting_result_once(B, N, D, offset, p):
    gen = torch.Generator().manual_seed(B * 1000 + N * 10 + D)
    store = torch.randn(B * N * D + 8, generator=gen).cuda()
    dh0 = store[offset:offset + B * N * D]
    desc = ops.dropout_desc(p, 0, 1234, 77)
    fresh = [guarded(N * D), guarded(D), guarded(D)]
    ops.embed_grad(dh0, B, N, D, *(v for _, v in fresh), dropout=desc)
    acc = [guarded(N * D, gen), guarded(D, gen), guarded(D, gen)]
    want = [flat.clone() for flat, _ in acc]
    for w, (_, s) in zip(want, fresh):
        w[GUARD:GUARD + s.numel()] += s
    for times in (1, 2):
        ops.embed_grad(dh0, B, N, D, *(v for _, v in acc), dropout=desc, accumulate=True)
        torch.cuda.synchronize()
        for name, (flat, _), w in zip(("dpos", "dcls", "dconv_bias"), acc, want):
            assert torch.equal(flat, w), (name, times, float((flat - w).abs().max()))
        for w, (_, s) in zip(want, fresh):
            w[GUARD:GUARD + s.numel()] += s
    assert float(fresh[0][1].abs().max()) > 0
