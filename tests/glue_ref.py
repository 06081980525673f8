"""Float64 references, exact operand builders and per-element gates for the step's glue kernels
(csrc/elementwise.hip, csrc/optim.hip): column sums, embedding gradients, the f32 GEMM, casts / packs / transposes,
GELU, cross entropy, the cls MSE, SGD and AdamW, and the Res-ViT router kernels (segment sums, the gated data gradient,
the router head, the routing masks).

A helper module, not a test file (the tests import it as `glue_ref`); plain torch, so it runs on CPU and GPU
tensors alike.

Memory. Operands sit in buffers wider than their logical width wherever the ABI has a leading dimension
(embed()): input padding is NaN, so a kernel that reads it poisons its output; output padding and the rows past
the end are NaN sentinels that must stay NaN (first_touched()).

Three kinds of gate, all per element, never a norm:

    exact     reductions and the f32 GEMM on integer operands (ints(): every partial sum is an integer below 2^24,
              exact in f32 in any order, assert_exact_sum()): the output equals the float64 sum, first_diff()
    bits      casts and moves, and ops that are one f32 rounding of a torch expression: the output's bit pattern
              equals torch's, first_diff(bits=True); NaN inputs of a cast compare by NaN-ness only
    bounded   |got - ref| <= bound against float64, the bound counted from the roundings the formula performs
              (one unit roundoff UF = 2^-24 each, at most a factor 2 on top); each reference below derives its own.
              worst() gives the largest ratio to the bound and where.
"""
import math

import torch

from gemm_ref import C_PHI, gelu64

UF = 2.0 ** -24          # unit roundoff of f32
NAN = float("nan")


# ---- memory: padded buffers and sentinels --------------------------------------------------------------------------
def embed(t, ld, extra_rows=0, fill=NAN, offset=0):
    """the 2-D tensor t inside a flat buffer of row stride ld >= t.shape[1], `offset` elements in, with `extra_rows`
    more rows and 8 guard elements after it (so an empty t still has an address); everything that is not t holds
    `fill`. Returns (flat buffer, view of t's place)."""
    rows, cols = t.shape
    assert ld >= cols
    flat = torch.full((offset + (rows + extra_rows) * ld + 8,), fill, dtype=t.dtype, device=t.device)
    view = flat[offset:].as_strided((rows, cols), (ld, 1))
    view.copy_(t)
    return flat, view


def first_touched(flat, *views):
    """index of the first element of the flat NaN-filled buffer outside every view (views of `flat` the kernel may
    write) that is no longer NaN, or None: guard columns, alignment gaps and rows past the end must stay NaN"""
    mask = torch.zeros(flat.shape, dtype=torch.bool, device=flat.device)
    base = flat.data_ptr()
    for v in views:
        off = (v.data_ptr() - base) // flat.element_size()
        idx = off + sum((torch.arange(n, device=flat.device) * s).reshape([-1 if k == d else 1 for k in range(v.dim())])
                        for d, (n, s) in enumerate(zip(v.shape, v.stride())))
        mask[idx.reshape(-1)] = True
    bad = (~mask) & ~flat.float().isnan()
    return int(bad.nonzero()[0]) if bool(bad.any()) else None


# ---- gates ---------------------------------------------------------------------------------------------------------
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}


def first_diff(got, want, bits=False, nan_by_kind=None):
    """None when got equals want at every element, else (index tuple, got, want) of the first difference.
    bits: compare bit patterns (tells -0.0 from 0.0); otherwise values, a NaN equal to a NaN. nan_by_kind: a bool
    mask of elements compared by NaN-ness alone (both NaN) instead."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if bits:
        ne = got.contiguous().view(_INT[got.dtype]) != want.contiguous().view(_INT[want.dtype])
    else:
        ne = ~((got == want) | (got.isnan() & want.isnan()))
    if nan_by_kind is not None:
        ne = torch.where(nan_by_kind, ~(got.isnan() & want.isnan()), ne)
    if not bool(ne.any()):
        return None
    at = tuple(int(i) for i in ne.nonzero()[0])
    return at, float(got[at]), float(want[at])


def worst(got, ref, bound):
    """the largest |got - ref| / bound and where: (ratio, index tuple). An element whose bound is 0 must be exact;
    where the reference is NaN the output must be NaN (ratio 0) and any other NaN counts as infinite."""
    g = got.double()
    err = (g - ref).abs()
    inf = torch.full_like(err, float("inf"))
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), inf))
    ratio = torch.where(ref.isnan(), torch.where(g.isnan(), torch.zeros_like(err), inf), ratio)
    ratio = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf"))
    at = int(ratio.argmax())
    value, idx = float(ratio.reshape(-1)[at]), []
    for n in reversed(ratio.shape):
        idx.append(at % n)
        at //= n
    return value, tuple(reversed(idx))


def ulp32(x):
    """spacing of f32 at |x| (float64 tensor in), 2^-149 at 0"""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


# ---- exact integer operands ----------------------------------------------------------------------------------------
def ints(shape, gen, lo=-8, hi=8):
    """f32 integers in [lo, hi] (bf16 holds them exactly); gen: a CPU torch.Generator"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).float()


def assert_exact_sum(terms, max_abs, start=0):
    """`terms` addends of magnitude <= max_abs onto a start value: every partial sum, in any order, is an integer
    below 2^24 and so exact in f32"""
    assert terms * max_abs + start < 2 ** 24, (terms, max_abs, start)


# ---- casts ---------------------------------------------------------------------------------------------------------
CAST_LOW_HALVES = (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)
CAST_NAN_COUNT = 1534     # of the 393,216 patterns: 2 signs x (127 NaN upper halves x 6 + the Inf upper half x 5 non-zero lows)


def cast_patterns():
    """f32 [393216]: all 65,536 upper halves x the lower halves that decide a bf16 rounding (exact, just above,
    just below the tie, the tie, just above it, all ones)"""
    hi = torch.arange(65536, dtype=torch.int64)[:, None] << 16
    bits = (hi | torch.tensor(CAST_LOW_HALVES, dtype=torch.int64)[None, :]).reshape(-1)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits)
    return bits.to(torch.int32).view(torch.float32)


def all_bf16():
    """bf16 [65536]: every bit pattern"""
    return (torch.arange(65536, dtype=torch.int32) - 32768).to(torch.int16).view(torch.bfloat16)


def bf16_rne_bits(x):
    """round-to-nearest-even f32 -> bf16 on the integer bit patterns (int64 [n] of the 16 result bits), written
    out independently of torch's cast; NaN inputs are not defined here. Only the CPU test uses it."""
    b = x.view(torch.int32).to(torch.int64) & 0xffffffff
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16) & 0xffff


# ---- column sums ---------------------------------------------------------------------------------------------------
def colsum_chunks(rows):
    """(chunks, rows per chunk) of vit_colsum / vit_colsum3: rows // 64 clamped to 1..256 chunks of
    ceil(rows / chunks) rows; the last chunk may be short or (4225 rows: 66 chunks of 65) empty"""
    c = min(max(rows // 64, 1), 256)
    return c, -(-rows // c)


def colsum(x, prior=None):
    """float64 column sums of the logical [rows, cols] input (+ the accumulated-onto values)"""
    s = x.double().sum(0)
    return s if prior is None else s + prior.double()


def embed_grad(dh0, B, N, D, mult=None):
    """float64 (dpos [N, D], dcls [D], dconv_bias [D]) of vit_embed_grad from dh0 [B N, D] (mult: the position
    dropout's multipliers, same shape)"""
    x = dh0.double()
    if mult is not None:
        x = x * mult.double()
    dpos = x.reshape(B, N, D).sum(0)
    return dpos, dpos[0].clone(), dpos[1:].sum(0)


def cls_mse(x, t):
    """float64 (e [B, D], part [B], loss) of vit_cls_mse. With integer x and t and B D 256 < 2^24 (|e| <= 16) e and
    part are exact in f32 and loss is the one division sum / (B D), correctly rounded."""
    e = x.double() - t.double()
    part = (e * e).sum(1)
    return e, part, part.sum() / e.numel()


def cls_mse_bwd(dx0, e, g):
    """vit_cls_mse_bwd, dx = dx0 + ((2 / (B D)) e) g: float64 (ref, bound).
    Roundings: the f32 constant 2 / (B D), its product with e, the product with g, the sum (the last two may fuse):
    at most 3 UF |term| + UF (|dx0| + |term|). The gate is 2^-23 (|dx0| + |term|) = UF (2 |dx0| + 2 |term|), which
    covers that wherever |term| <= |dx0|; cls_mse_bwd_case() builds such operands."""
    term = (2.0 / e.numel()) * e.double() * float(g)
    return dx0.double() + term, 2.0 ** -23 * (dx0.double().abs() + term.abs())


def cls_mse_bwd_case(B, D, gen):
    """dx0 with 1 <= |dx0| <= 2, |e| <= 0.5, g = 0.75: |term| = (2 / (B D)) |e| g <= 0.75 <= |dx0|"""
    sign = torch.randint(0, 2, (B, D), generator=gen).float() * 2 - 1
    dx0 = sign * (1 + torch.rand(B, D, generator=gen))
    e = torch.rand(B, D, generator=gen) - 0.5
    return dx0, e, torch.tensor(0.75)


# ---- f32 GEMM --------------------------------------------------------------------------------------------------------
def gemm_f32(A, B, bias=None, C0=None):
    """float64 C = A [M, K] @ B [K, N] (+ bias [N]) (+ C0): at K = 0 the product is 0"""
    C = A.double() @ B.double()
    if bias is not None:
        C = C + bias.double()[None, :]
    return C if C0 is None else C + C0.double()


# ---- GELU ------------------------------------------------------------------------------------------------------------
def gelu_inputs():
    """a grid over [-10, 10] (step 1/64, every binade of the erf argument down to 2^-6), 0, -0.0, +-40 (erf
    saturated, exp(-800) = 0) and f32 denormals"""
    grid = torch.arange(-640, 641).float() / 64
    edge = torch.tensor([0.0, -0.0, 40.0, -40.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -127, -2.0 ** -130, 1e-30, -1e-30])
    return torch.cat([grid, edge])


def gelu(u):
    """vit_gelu_f32: float64 (ref, bound), gemm_ref's GELU gate without its bf16 term, c = C_PHI:
    |got - ref| <= C_PHI max(1, |u|). 0.5 u (1 + erf(u / sqrt 2)) is four f32 roundings on a value of at most |u|
    and erff's few-ulp absolute error on (1 + erf) <= 2 times 0.5 |u|: below 8 UF max(1, |u|) = 4.8e-7 max(1, |u|)"""
    g, _ = gelu64(u.double())
    return g, C_PHI * u.double().abs().clamp_min(1.0)


def gelu_bwd(u, dy):
    """vit_gelu_bwd_f32, dx = dy gelu'(u): float64 (ref, bound), gemm_ref's GELU_BWD gate without the bf16 term:
    |got - ref| <= C_PHI |dy| max(1, |u|)"""
    _, d = gelu64(u.double())
    return dy.double() * d, C_PHI * dy.double().abs() * u.double().abs().clamp_min(1.0)


# ---- cross entropy ---------------------------------------------------------------------------------------------------
class CE:
    """loss [B], dlogits [B, C], lse, p, E [B], bound_loss [B], bound_d [B, C], top1 / top5 [B] (0. / 1.)"""


def ce_hits(logits, labels):
    """The hit rule of vit_cross_entropy (include/vit_hip.h): above = #{c != y : x[c] > x[y] or x[c] is NaN};
    top-1 = above < 1, top-5 = above < 5. Ties count for the label; a NaN logit ranks above every number (torch.topk's
    order), so an all-NaN row is a miss, and a row whose only NaN is the label's own logit a hit. A label outside
    [0, C) is a miss. Returns (top1, top5) as float64 0 / 1."""
    x = logits.double()
    B, C = x.shape
    ok = (labels >= 0) & (labels < C)
    y = labels.clamp(0, C - 1)
    xy = x.gather(1, y[:, None])
    other = torch.arange(C, device=x.device)[None, :] != y[:, None]
    above = (((x > xy) | x.isnan()) & other).sum(1)
    return ((above < 1) & ok).double(), ((above < 5) & ok).double()


def cross_entropy(logits, labels, grad_scale):
    """float64 reference and per-row gates of vit_cross_entropy. With R = max - min of the row and
    E = 2^-21 (4 + R + |lse|):
        |loss - ref|          <= E max(1, |lse| + |x_y|)
        |dlogits - ref|       <= grad_scale (E p + 2^-23)      per element
    E counts, in units of 2^-24: the rounding of x - max / x - lse (an argument of size up to R, so R UF absolute on
    the exponent, i.e. relative on p), the fast exp's argument scaling by log2 e (another R UF) and its unit error
    (2 UF), the f32 sum of the exponentials (each addition UF relative on a sum of positives: the wave tree keeps it
    to a few UF) and the log, whose error and the final max + log rounding are relative to |lse|; 8 (4 + R + |lse|)
    UF is that count with the factor 2 on top. The loss is lse - x_y, one more rounding at the size |lse| + |x_y|;
    the gradient (p - onehot) grad_scale adds two roundings of a value below 1: 2^-23.
    A label outside [0, C): loss and the dlogits row are NaN. A NaN logit makes its row's loss and dlogits NaN."""
    r = CE()
    grad_scale = f32(grad_scale)        # as the ABI's `float` argument receives it
    x = logits.double()
    B, C = x.shape
    ok = (labels >= 0) & (labels < C)
    y = labels.clamp(0, C - 1)
    r.lse = torch.logsumexp(x, 1)
    xy = x.gather(1, y[:, None])[:, 0]
    nan = torch.full_like(r.lse, NAN)
    r.loss = torch.where(ok, r.lse - xy, nan)
    r.p = torch.exp(x - r.lse[:, None])
    onehot = (torch.arange(C, device=x.device)[None, :] == y[:, None]).double()
    r.dlogits = torch.where(ok[:, None], (r.p - onehot) * grad_scale, nan[:, None])
    R = x.max(1).values - x.min(1).values
    r.E = 2.0 ** -21 * (4 + R + r.lse.abs())
    r.bound_loss = r.E * (r.lse.abs() + xy.abs()).clamp_min(1.0)
    r.bound_d = grad_scale * (r.E[:, None] * r.p + 2.0 ** -23)
    r.top1, r.top5 = ce_hits(logits, labels)
    return r


def ce_logits(B, C, gen):
    """3 N(0, 1), clamped to |x| <= 16"""
    return (3 * torch.randn(B, C, generator=gen)).clamp(-16, 16)


def ce_emulate(logits, labels, grad_scale):
    """the kernel's formula in f32 torch (exp as exp2(x log2 e) in f32): (loss, dlogits) a correct kernel writes up
    to the order of its sum. Only the CPU test of the gate uses it."""
    x = logits.float()
    l2e = torch.tensor(1.4426950408889634, dtype=torch.float32)
    mx = x.max(1, keepdim=True).values
    s = torch.exp2((x - mx) * l2e).sum(1, keepdim=True)
    lse = mx + torch.log(s)
    p = torch.exp2((x - lse) * l2e)
    onehot = (torch.arange(x.shape[1])[None, :] == labels[:, None]).float()
    return (lse - x.gather(1, labels[:, None]))[:, 0], (p - onehot) * torch.tensor(grad_scale, dtype=torch.float32)


# ---- SGD -------------------------------------------------------------------------------------------------------------
def f32(v):
    """the Python float as the C ABI's `float` argument receives it"""
    return float(torch.tensor(v, dtype=torch.float32))


def sgd(p, g, buf, lr, momentum, wd, first):
    """vit_sgd_step in float64 with the f32 hyper-parameters: (p', buf', bound_p, bound_buf).
        d = g + wd p                 wd p and the sum (or one fused rounding):      e_d   = UF (|g| + 2 |wd p|)
        buf' = d  |  mom buf + d     the product and the sum:                        e_buf = e_d + UF (2 |mom buf| + |d|)
        p' = p - lr buf'             the product and the sum:                        e_p   = lr e_buf + UF (2 |lr buf'| + |p|)
    each with the factor 2 on top. With first set buf is never read (it may hold NaN)."""
    lr, momentum, wd = f32(lr), f32(momentum), f32(wd)
    p, g = p.double(), g.double()
    d = g + wd * p
    e = UF * (g.abs() + 2 * (wd * p).abs())
    if not first:
        mb = momentum * buf.double()
        e = e + UF * (2 * mb.abs() + d.abs())
        d = mb + d
    pn = p - lr * d
    ep = lr * e + UF * (2 * (lr * d).abs() + p.abs())
    return pn, d, 2 * ep, 2 * e


def sgd_emulate(p, g, buf, lr, momentum, wd, first):
    """the same step in f32 torch, unfused: what a correct kernel may write"""
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    d = g + t(wd) * p
    if not first:
        d = t(momentum) * buf + d
    return p - t(lr) * d, d


# ---- AdamW -----------------------------------------------------------------------------------------------------------
def adamw_prep(partial, used, steps, lr, beta1, beta2, max_norm):
    """float64 (table [nseg, 4], steps', norm, coef) of vit_adamw_prep with the f32 hyper-parameters: steps advance
    where used > 0; an active row is {lr / (1 - beta1^step), sqrt(1 - beta2^step), 1, coef}, an inactive one
    {0, 0, 0, coef}; coef = min(1, max_norm / (norm + 1e-6)) with norm = sqrt(sum partial), 1 without partials or
    with max_norm <= 0.
    Gate: one f32 ulp of the float64 value (ulp32). The first two columns are computed in double on the device and
    rounded once, so they can differ from the rounded reference only by a double-precision difference of pow that
    flips the rounding. norm and coef go through f32 roundings (the sqrt's result, + 1e-6f, the division), each
    half an ulp: adamw_prep_emulate() is that chain, and the CPU test proves it stays within one ulp for the cases
    adamw_prep_case() builds, which are the cases the GPU sweep runs."""
    lr, beta1, beta2, max_norm = f32(lr), f32(beta1), f32(beta2), f32(max_norm)
    norm = math.sqrt(float(partial.double().sum())) if partial is not None else 0.0
    coef = 1.0
    if partial is not None and max_norm > 0:
        coef = min(max_norm / (norm + f32(1e-6)), 1.0)
    act = used > 0
    st = steps.double() + act.double()
    table = torch.zeros(steps.numel(), 4, dtype=torch.float64)
    table[:, 0] = torch.where(act, lr / (1 - beta1 ** st), torch.zeros_like(st))
    table[:, 1] = torch.where(act, torch.sqrt(1 - beta2 ** st), torch.zeros_like(st))
    table[:, 2] = act.double()
    table[:, 3] = coef
    return table, st, norm, coef


def adamw_prep_emulate(partial, max_norm):
    """(norm, coef) through the kernel's f32 chain: f32(sqrt(sum)), + 1e-6f, the division, min with 1"""
    norm = torch.tensor(math.sqrt(float(partial.double().sum())), dtype=torch.float32)
    coef = torch.minimum(torch.tensor(max_norm, dtype=torch.float32) / (norm + torch.tensor(1e-6, dtype=torch.float32)),
                         torch.tensor(1.0))
    return float(norm), float(coef)


def adamw_prep_case(nseg, nparts, seed, clip=True):
    """(partial f64 [nparts] or None for nparts 0, used [nseg], steps [nseg], max_norm): every third segment unused,
    steps 0..9; clip: the norm is above max_norm = 1 (coef < 1), otherwise below it (coef = 1)"""
    g = torch.Generator().manual_seed(seed)
    used = (torch.arange(nseg) % 3 != 1).float()
    steps = (torch.arange(nseg) % 10).float()
    partial = None
    if nparts:
        partial = torch.rand(nparts, generator=g, dtype=torch.float64) * ((40.0 if clip else 0.25) / nparts)
        if nparts > 2:
            partial[nparts // 2] = 0.0          # a workgroup that had no elements
    return partial, used, steps, 1.0


# (nseg, nparts, seed, clip): nseg across the 256-thread loop, nparts across the 256-thread sum, no partials at all
# (coef 1), a norm below max_norm (coef 1)
ADAMW_PREP_CASES = [(1, 1, 0, True), (256, 255, 1, True), (257, 257, 2, True), (300, 1, 3, True), (300, 257, 4, False),
                    (257, 0, 5, True), (256, 255, 6, False)]


def adamw(p, g, m, v, step_size, bc2s, coef, lr, beta1, beta2, eps, wd):
    """One active segment of vit_adamw_update in float64: torch's single-tensor AdamW (decoupled decay) on the clipped
    gradient, with the constants the kernel receives (decay = f32(1 - lr wd), f32 betas and (1 - beta)s, the table's
    f32 step_size / sqrt(bc2) / coef). Returns (p', g', m', v') and their bounds, counted per line:
        g' = g coef                                  e_g = UF |g'|
        m' = m + omb1 (g' - m)                       e_m = omb1 e_g + 2 UF omb1 |g' - m| + UF |m'|
        v' = v beta2 + (omb2 g') g'                  e_v = UF (|v beta2| + 4 omb2 g'^2 + |v'|)
        den = sqrt(v') / bc2s + eps                  e_den = (sqrt(v') / bc2s) (e_v / (2 v') + 2 UF) + UF den
        q = m' / den                                 e_q = e_m / den + |q| e_den / den + UF |q|
        p' = p decay - step_size q                   e_p = UF |p decay| + step_size (e_q + UF |q|) + UF |p'|
    each with the factor 2 on top. v >= 1e-4 keeps den far above eps, so no term is eps-dominated."""
    decay, b1, b2 = f32(1.0 - lr * wd), f32(beta1), f32(beta2)
    omb1, omb2, eps = f32(1.0 - beta1), f32(1.0 - beta2), f32(eps)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gn = g * coef
    e_g = UF * gn.abs()
    mn = m + omb1 * (gn - m)
    e_m = omb1 * e_g + 2 * UF * omb1 * (gn - m).abs() + UF * mn.abs()
    vn = v * b2 + omb2 * gn * gn
    e_v = UF * ((v * b2).abs() + 4 * omb2 * gn * gn + vn)
    s = vn.sqrt() / bc2s
    den = s + eps
    e_den = s * (e_v / (2 * vn) + 2 * UF) + UF * den
    q = mn / den
    e_q = e_m / den + q.abs() * e_den / den + UF * q.abs()
    pn = p * decay - step_size * q
    e_p = UF * (p * decay).abs() + step_size * (e_q + UF * q.abs()) + UF * pn.abs()
    return (pn, gn, mn, vn), (2 * e_p, 2 * e_g, 2 * e_m, 2 * e_v)


def adamw_emulate(p, g, m, v, step_size, bc2s, coef, lr, beta1, beta2, eps, wd):
    """the kernel's update in f32 torch, unfused"""
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    gn = g * t(coef)
    pn = p * t(1.0 - lr * wd)
    mn = m + t(1.0 - beta1) * (gn - m)
    vn = v * t(beta2) + t(1.0 - beta2) * gn * gn
    den = vn.sqrt() / t(bc2s) + t(eps)
    return pn - t(step_size) * (mn / den), gn, mn, vn


ADAMW_LENGTHS = (1, 2, 3, 4, 5, 1023, 8192, 8195)


def adamw_layout(lengths=ADAMW_LENGTHS, chunk=8192, inactive=2):
    """64-aligned segments of the given lengths in one flat buffer and their chunk list, by hand:
    (starts, total, chunks int64 [nchunks, 3] = {segment, start, length <= chunk}, active bool list). Length 8195
    splits into chunks of 8192 and 3; segment `inactive` has no gradient."""
    starts, chunks, at = [], [], 0
    for s, n in enumerate(lengths):
        starts.append(at)
        for c0 in range(0, n, chunk):
            chunks.append([s, at + c0, min(chunk, n - c0)])
        at += (n + 63) // 64 * 64
    return starts, at, torch.tensor(chunks, dtype=torch.int64), [s != inactive for s in range(len(lengths))]


# ---- Res-ViT router kernels --------------------------------------------------------------------------------------------
def segment_colsum(x, segs, seg_rows, seg_stride, row0, scale):
    """float64 [segs, cols] of vit_segment_colsum: scale times the sum of rows [s seg_stride + row0, + seg_rows) of x.
    On integer operands (assert_exact_sum) and a power-of-two scale every partial sum and the product are exact."""
    out = torch.zeros(segs, x.shape[1], dtype=torch.float64, device=x.device)
    for s in range(segs):
        r0 = s * seg_stride + row0
        out[s] = x[r0:r0 + seg_rows].double().sum(0) * scale
    return out


def segment_colsum_emulate(x, segs, seg_rows, seg_stride, row0, scale, unroll_bound=12):
    """the kernel's order in f32: four row lanes, lane l adds rows l, l + 4, ... (four at a time while
    r + 12 < seg_rows, then one at a time), then lanes 0..3 in turn, then the scale. unroll_bound: the planted
    fault (r + 8 < seg_rows reads three rows past the segment)"""
    out = torch.zeros(segs, x.shape[1])
    for s in range(segs):
        base = s * seg_stride + row0
        lanes = []
        for l in range(4):
            acc, r = torch.zeros(x.shape[1]), l
            while r + unroll_bound < seg_rows:
                for k in (0, 4, 8, 12):
                    acc = acc + x[base + r + k].float()
                r += 16
            while r < seg_rows:
                acc = acc + x[base + r].float()
                r += 4
            lanes.append(acc)
        out[s] = (((lanes[0] + lanes[1]) + lanes[2]) + lanes[3]) * torch.tensor(scale, dtype=torch.float32)
    return out


RDG_RB = 32     # rows per column-partial block of vit_router_dx_gate


def router_dx_gate(dx, g, g_scale, gp, T, N, reserve, rows_pad, cols_pad):
    """vit_router_dx_gate from CPU f32 operands dx [T, cols], g [ceil(T / N), cols], gp bf16 [T, cols]:
    (out bf16 [rows_pad, cols_pad], col_partial float64 [ceil(rows_pad / 32), cols]).
    out = bf16((dx + s g[t // N]) gp), s = g_scale where t % N >= reserve, else the term is absent; the product s g,
    the sum and the product with gp each rounded to f32 (torch's CPU f32 operators, which never fuse), then one
    round-to-nearest-even to bf16: compared as bit patterns. Zeros in the padding. col_partial: per 32-row block, the
    column sums of the rounded values; exact in f32 when they are small integers or halves."""
    cols = dx.shape[1]
    t = torch.arange(T)
    term = torch.tensor(g_scale, dtype=torch.float32) * g.float()[t // N]
    term = torch.where(((t % N) >= reserve)[:, None], term, torch.zeros_like(term))
    val = ((dx.float() + term) * gp.float()).bfloat16()
    out = torch.zeros(rows_pad, cols_pad, dtype=torch.bfloat16)
    out[:T, :cols] = val
    nblk = -(-rows_pad // RDG_RB)
    full = torch.zeros(nblk * RDG_RB, cols, dtype=torch.float64)
    full[:T] = val.double()
    return out, full.reshape(nblk, RDG_RB, cols).sum(1)


def router_select(idx, sets, nkeys):
    """vit_router_select: (active bool [npos, T], sel bool [nkeys, T], any bool [nkeys]); active[j] = isin(trunc(idx),
    sets[j]) with the truncation toward zero of torch's .long() (so -0.5 -> 0); NaN and values whose truncation is
    outside [0, 32) are in no set (their conversion is not performed: it is undefined for NaN and 1e9 alike);
    sel[k] = idx == k"""
    T = idx.numel()
    ok = (idx > -1) & (idx < 32)
    lv = torch.where(ok, idx, torch.zeros_like(idx)).long()
    active = torch.zeros(len(sets), T, dtype=torch.bool)
    for j, st in enumerate(sets):
        active[j] = ok & torch.isin(lv, torch.tensor(sorted(st), dtype=torch.int64))
    sel = torch.stack([idx == float(k) for k in range(nkeys)]) if nkeys else torch.zeros(0, T, dtype=torch.bool)
    return active, sel, sel.any(1)


ROUTER_SELECT_VALUES = (-0.5, -1.0, 3.5, 31.0, 32.0, 1e9, NAN, 0.0, -0.0, 5.0, 7.0)


def router_select_case(T, gen):
    """pattern indices f32 [T]: integers 0..31 with the edge values strewn in; key 13 appears in the last token only"""
    idx = torch.randint(0, 32, (T,), generator=gen).float()
    idx[idx == 13.0] = 12.0
    edge = torch.tensor(ROUTER_SELECT_VALUES)
    n = min(T - 1, edge.numel())
    if n > 0:
        at = torch.randperm(T - 1, generator=gen)[:n]
        idx[at] = edge[:n]
    idx[T - 1] = 13.0
    return idx


# ---- Res-ViT router head ---------------------------------------------------------------------------------------------
RH_THREADS = 256
RH_SLACK = 1.0 + 2.0 ** -9      # second-order products of the counted terms
RH_C = 1e-8                     # the entropy's p + 1e-8 (as f32)


def _softmax2(a, b, darg):
    """float64 two-element softmax of the arguments a, b and its gate. The kernel's softmax2 is max, two expf, one
    addition, two divisions. With d = |a - b|: the larger argument gives expf(0) = 1 exactly; the other's argument
    a - max is rounded (u d absolute, so u d relative on the exponential) and expf is good to 1 ulp (2 u):
    eps_e = (d + 2) u. The sum 1 + e adds u, each division 1 ulp (2 u): rel(p) <= eps_e + (u + eps_e) + 2 u
    = (2 d + 7) u. darg: the absolute error of a - b already in the arguments (noise added in f32); it moves either
    probability by at most p darg (dp/dd = p0 p1)."""
    m = torch.maximum(a, b)
    e0, e1 = torch.exp(a - m), torch.exp(b - m)
    p0, p1 = e0 / (e0 + e1), e1 / (e0 + e1)
    rel = RH_SLACK * ((2 * (a - b).abs() + 7) * UF + darg)
    return p0, p1, rel * p0, rel * p1


def router_head_fwd(logits, noise, noise_mode, yhard, N, reserve, training, norm):
    """float64 reference and gates of vit_router_head_fwd (logits [T, bs, 2] CPU f32). Returns an object with
    soft / b_soft; ysoft / b_ysoft (training); hard (the expected values: the one-hot, the caller's y_hard, (0, 1) on
    reserved tokens) with b_hard (0 in evaluation: equal; 2 u in training, the two roundings of (y_hard - y) + y) and
    `decided` [T, bs], false where the float64 margin |y1 - y0| is within the softmax gates (the one-hot may
    legitimately differ there; an exact tie of equal arguments is decided: index 0); indices [T] with b_idx and
    idx_decided [T]; ent with b_ent.
    Entropy: each term t = p log(p + 1e-8) carries |t| (rel(p) + 3 u) + p (rel(p) + u) (the probability, the
    addition, logf's 1 ulp, the product); the sum of the two terms, the bs positions, the 8-level tree of a block,
    the strided sum over ceil(blocks / 256) partials, another 8-level tree and the division by norm are
    n = bs + 19 + ceil(blocks / 256) roundings of a sum of same-signed terms: n u sum|t|."""
    r = CE()
    T, bs, _ = logits.shape
    x = logits.double()
    zero = torch.zeros(T, bs, dtype=torch.float64)
    r.soft0, r.soft1, r.b_soft0, r.b_soft1 = _softmax2(x[..., 0], x[..., 1], zero)
    r.soft = torch.stack([r.soft0, r.soft1], -1)
    r.b_soft = torch.stack([r.b_soft0, r.b_soft1], -1)
    res = ((torch.arange(T) % N) < reserve)[:, None].expand(T, bs)
    c = f32(RH_C)
    t = r.soft * torch.log(r.soft + c)
    relp = r.b_soft / r.soft.clamp_min(1e-300)
    dt = t.abs() * (relp + 3 * UF) + r.soft * (relp + UF)
    live = (~res)[..., None]
    nb = -(-T // RH_THREADS)
    n = bs + 19 + -(-nb // RH_THREADS)
    norm = f32(norm)
    r.ent = -(t * live).sum() / norm
    r.b_ent = RH_SLACK * ((dt * live).sum() + n * UF * (t.abs() * live).sum()) / norm
    if training:
        g = torch.zeros_like(x)
        darg = zero
        if noise_mode == 1:
            g = noise.double()
        elif noise_mode == 2:
            g = -torch.log(noise.double())
        a = x + g
        if noise_mode:      # the f32 sum's rounding, and logf's 1 ulp on the noise
            darg = (UF * a.abs() + (2 * UF * g.abs() if noise_mode == 2 else 0)).sum(-1)
        y0, y1, b0, b1 = _softmax2(a[..., 0], a[..., 1], darg)
        r.ysoft, r.b_ysoft = torch.stack([y0, y1], -1), torch.stack([b0, b1], -1)
        q0, q1, m0, m1 = y0, y1, b0, b1
        if noise_mode == 1:     # the kernel's own f32 sums logits + noise (one addition: torch's is the same one)
            a32 = logits + noise
            equal_args = a32[..., 0] == a32[..., 1]
        else:
            equal_args = (logits[..., 0] == logits[..., 1]) & (
                True if not noise_mode else (noise[..., 0] == noise[..., 1]))
    else:
        q0, q1, m0, m1 = r.soft0, r.soft1, r.b_soft0, r.b_soft1
        equal_args = logits[..., 0] == logits[..., 1]
    if yhard is not None:
        hard = yhard.double().clone()
        r.decided = torch.ones(T, bs, dtype=torch.bool)
    else:
        h1 = (q1 > q0).double()
        hard = torch.stack([1 - h1, h1], -1)
        r.decided = ((q1 - q0).abs() > m0 + m1) | equal_args
        hard = torch.where(equal_args[..., None], torch.tensor([1.0, 0.0], dtype=torch.float64), hard)
    hard = torch.where(res[..., None], torch.tensor([0.0, 1.0], dtype=torch.float64), hard)
    r.decided = r.decided | res
    r.hard = hard
    straight = training & ~res      # (y_hard - y) + y: two roundings of values of size at most 1 + |y_hard|
    r.b_hard = torch.where(straight[..., None], 2 * UF * RH_SLACK * hard.abs().clamp_min(1.0), torch.zeros_like(hard))
    w = 2.0 ** torch.arange(bs - 1, -1, -1, dtype=torch.float64)
    r.indices = (hard[..., 1] * w).sum(1)
    # the fma chain: bs roundings of a partial index below 2^bs max|hard|, plus the hard values' own error
    r.b_idx = (r.b_hard[..., 1] * w).sum(1) + torch.where(
        straight.any(1), RH_SLACK * bs * UF * (hard[..., 1].abs() * w).sum(1), torch.zeros(T, dtype=torch.float64))
    r.idx_decided = r.decided.all(1)
    return r


def router_head_fwd_emulate(logits, noise, noise_mode, yhard, N, reserve, training, norm):
    """the kernel's formulas in f32 torch, unfused: (soft, ysoft or None, hard, indices, entropy)"""
    def sm(a, b):
        m = torch.maximum(a, b)
        e0, e1 = torch.exp(a - m), torch.exp(b - m)
        s = e0 + e1
        return e0 / s, e1 / s
    T, bs, _ = logits.shape
    t32 = lambda v: torch.tensor(v, dtype=torch.float32)
    l0, l1 = logits[..., 0], logits[..., 1]
    p0, p1 = sm(l0, l1)
    res = ((torch.arange(T) % N) < reserve)[:, None].expand(T, bs)
    term = p0 * torch.log(p0 + t32(RH_C)) + p1 * torch.log(p1 + t32(RH_C))
    ent = -(torch.where(res, torch.zeros_like(term), term).sum()) / t32(norm)
    ysoft = None
    if training:
        g0 = g1 = torch.zeros_like(l0)
        if noise_mode == 1:
            g0, g1 = noise[..., 0], noise[..., 1]
        elif noise_mode == 2:
            g0, g1 = -torch.log(noise[..., 0]), -torch.log(noise[..., 1])
        y0, y1 = sm(l0 + g0, l1 + g1)
        ysoft = torch.stack([y0, y1], -1)
        if yhard is not None:
            yh0, yh1 = yhard[..., 0], yhard[..., 1]
        else:
            yh1 = (y1 > y0).float()
            yh0 = 1 - yh1
        h0, h1 = (yh0 - y0) + y0, (yh1 - y1) + y1
    elif yhard is not None:
        h0, h1 = yhard[..., 0], yhard[..., 1]
    else:
        h1 = (p1 > p0).float()
        h0 = 1 - h1
    h0 = torch.where(res, torch.zeros_like(h0), h0)
    h1 = torch.where(res, torch.ones_like(h1), h1)
    idx = torch.zeros(T)
    for i in range(bs):
        idx = h1[:, i] * t32(float(1 << (bs - 1 - i))) + idx
    return torch.stack([p0, p1], -1), ysoft, torch.stack([h0, h1], -1), idx, ent


def router_head_bwd(soft, ysoft, dsoft, dhard, dind, dent, N, reserve, training, norm):
    """float64 dlogits [T, bs, 2] of vit_router_head_bwd from the f32 soft / ysoft it is given, and its gate. With
    c = 1e-8, L = log(p + c), q = p / (p + c), ge = -dent / norm on non-reserved tokens (else the term is absent):
        A = L + q                   e_A  = u + 2 u |L| + 3 u q + u |A|   (p + c; logf's 1 ulp; the division; the sum)
        d = dsoft + ge A            e_d  = |ge| e_A + 3 u |ge A| + u |d|  (ge's division 2 u, the product, the sum)
        sd = d0 p0 + d1 p1          e_sd = sum p e_d + 2 u sum |d p|      (the two products, the sum)
        o = p (d - sd)              e_o  = p (e_d + e_sd + u |d - sd|) + u |o|
    and in training on non-reserved tokens with dhard or dind, h = dhard, h1 += dind 2^(bs-1-i) (e_h1 = u |h1|),
    sy = h0 y0 + h1 y1, o += y (h - sy) with the same three-product count, and u |o| for the final sum."""
    T, bs, _ = soft.shape
    p = soft.double()
    res = ((torch.arange(T) % N) < reserve)[:, None, None]
    norm = f32(norm)
    c = f32(RH_C)
    d = torch.zeros_like(p) if dsoft is None else dsoft.double()
    e_d = torch.zeros_like(p)
    if dent is not None:
        ge = torch.where(res, torch.zeros(1, dtype=torch.float64), -dent.double() / norm)
        L, q = torch.log(p + c), p / (p + c)
        A = L + q
        e_A = UF * (1 + 2 * L.abs() + 3 * q + A.abs())
        d = d + ge * A
        e_d = torch.where(ge != 0, ge.abs() * e_A + 3 * UF * (ge * A).abs() + UF * d.abs(), e_d)
    sd = (d * p).sum(-1, keepdim=True)
    e_sd = (p * e_d).sum(-1, keepdim=True) + 2 * UF * (d * p).abs().sum(-1, keepdim=True)
    o = p * (d - sd)
    e_o = p * (e_d + e_sd + UF * (d - sd).abs()) + UF * o.abs()
    if training and ysoft is not None and (dhard is not None or dind is not None):
        y = ysoft.double()
        h = torch.zeros_like(p) if dhard is None else dhard.double().clone()
        e_h = torch.zeros_like(p)
        if dind is not None:
            w = 2.0 ** torch.arange(bs - 1, -1, -1, dtype=torch.float64)
            h[..., 1] = h[..., 1] + dind.double()[:, None] * w[None, :]
            e_h[..., 1] = UF * h[..., 1].abs()
        sy = (h * y).sum(-1, keepdim=True)
        e_sy = (y * e_h).sum(-1, keepdim=True) + 2 * UF * (h * y).abs().sum(-1, keepdim=True)
        t2 = y * (h - sy)
        e_t2 = y * (e_h + e_sy + UF * (h - sy).abs()) + UF * t2.abs()
        o = torch.where(res, o, o + t2)
        e_o = torch.where(res, e_o, e_o + e_t2 + UF * o.abs())
    return o, RH_SLACK * e_o


def router_head_bwd_emulate(soft, ysoft, dsoft, dhard, dind, dent, N, reserve, training, norm, reserved_take_hard=False,
                            ent_sign=-1.0):
    """the kernel's formulas in f32 torch, unfused. Planted faults: reserved tokens take the hard gradient; the
    entropy gradient with the wrong sign (ent_sign 1)"""
    T, bs, _ = soft.shape
    t32 = lambda v: torch.tensor(v, dtype=torch.float32)
    res = ((torch.arange(T) % N) < reserve)[:, None, None]
    p = soft
    d = torch.zeros_like(p) if dsoft is None else dsoft.clone()
    if dent is not None:
        ge = torch.where(res, torch.zeros(1), ent_sign * dent / t32(norm))
        A = torch.log(p + t32(RH_C)) + p / (p + t32(RH_C))
        d = torch.where(ge != 0, d + ge * A, d)
    sd = d[..., :1] * p[..., :1] + d[..., 1:] * p[..., 1:]
    o = p * (d - sd)
    if training and ysoft is not None and (dhard is not None or dind is not None):
        h = torch.zeros_like(p) if dhard is None else dhard.clone()
        if dind is not None:
            w = torch.tensor([float(1 << (bs - 1 - i)) for i in range(bs)])
            h[..., 1] = h[..., 1] + dind[:, None] * w[None, :]
        sy = h[..., :1] * ysoft[..., :1] + h[..., 1:] * ysoft[..., 1:]
        o2 = o + ysoft * (h - sy)
        o = o2 if reserved_take_hard else torch.where(res, o, o2)
    return o


def router_head_logits(T, bs, gen, ties=True):
    """logits: multiples of 1/8 in [-4, 4]; with Gumbel noise in multiples of 1/4 every argument difference is 0 (a
    tie, decided: index 0) or at least 1/8 (|y1 - y0| >= tanh(1/16) = 0.06, far above the softmax gate), so the
    reference alone never has to skip a decision. ties: a few exact ties planted."""
    x = torch.randint(-32, 33, (T, bs, 2), generator=gen).float() / 8
    if ties:
        x[::7, 0, 1] = x[::7, 0, 0]
    return x


def router_head_noise(T, bs, mode, gen):
    """mode 1: Gumbel-like noise in multiples of 1/4 in [-2, 2]; mode 2: exponential draws in [2^-20, 1]"""
    if mode == 1:
        return torch.randint(-8, 9, (T, bs, 2), generator=gen).float() / 4
    return torch.rand(T, bs, 2, generator=gen).clamp_min(2.0 ** -20)
