"""Float64 references, exact operand builders and per-element gates for the step's glue kernels
(csrc/elementwise.hip, csrc/optim.hip): column sums, embedding gradients, the f32 GEMM, casts / packs / transposes,
GELU, cross entropy, the cls MSE, SGD and AdamW.

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
