"""Float64 reference, bounds and cases for vit_adamw_ema_update (csrc/optim.hip): glue_ref.adamw's update extended
with the undecayed case and the weight-EMA line, and the SGD path's EMA (one vit_axpby).

A helper module, not a test file (imported as `adamw_ema_ref`); plain torch on the CPU.

    decayed chunk       glue_ref.adamw as it stands (decay = f32(1 - lr wd))
    undecayed chunk     glue_ref.adamw with wd = 0: decay is exactly 1, so the reference is the unmultiplied p; its
                        bound keeps the UF |p| of a product the kernel does not make (never tighter than needed)
    ema' = ema + omd (p' - ema), omd = f32(1 - ema_decay):
                        e_ema = omd e_p + 2 UF omd |p' - ema| + UF |ema'|
                        (p' carries e_p; the difference and the product round once each, relative to omd |p' - ema|;
                        the sum rounds once), with the factor 2 on top as elsewhere
    SGD's EMA, vit_axpby(p, ema, a, b) with a = f32(1 - d), b = f32(d): ema' = a p + b ema on the kernel's own p:
                        e = UF (|a p| + |b ema| + |ema'|), two products and a sum, with the factor 2 on top
"""
import math

import torch

import glue_ref as G

UF = G.UF
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05)
EMA_DECAY = 0.99
COEFS = (0.37, 1.0)    # a clipped step and an unclipped one


def omd_of(ema_decay):
    return G.f32(1.0 - ema_decay)


def ema_lerp(p_new, e_p, ema, ema_decay):
    """(ema', bound): p_new float64 carrying the (already doubled) bound e_p; ema f32 or f64"""
    omd = omd_of(ema_decay)
    ema = ema.double()
    d = p_new - ema
    out = ema + omd * d
    return out, omd * e_p + 2 * (2 * UF * omd * d.abs() + UF * out.abs())


def adamw_ema(p, g, m, v, ema, step_size, bc2s, coef, decayed, ema_decay=EMA_DECAY, **hyper):
    """one chunk in float64: ((p', g', m', v', ema'), bounds). ema None: no EMA (4-tuples)"""
    h = dict(HYPER, **hyper)
    refs, bounds = G.adamw(p, g, m, v, step_size, bc2s, coef, h["lr"], h["beta1"], h["beta2"], h["eps"],
                           h["wd"] if decayed else 0.0)
    if ema is None:
        return refs, bounds
    e, be = ema_lerp(refs[0], bounds[0], ema, ema_decay)
    return refs + (e,), bounds + (be,)


def adamw_ema_emulate(p, g, m, v, ema, step_size, bc2s, coef, decayed, ema_decay=EMA_DECAY, **hyper):
    """the kernel's chunk in f32 torch, unfused; an undecayed p is not multiplied"""
    h = dict(HYPER, **hyper)
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    gn = g * t(coef)
    pn = p * t(1.0 - h["lr"] * h["wd"]) if decayed else p
    mn = m + t(1.0 - h["beta1"]) * (gn - m)
    vn = v * t(h["beta2"]) + t(1.0 - h["beta2"]) * gn * gn
    den = vn.sqrt() / t(bc2s) + t(h["eps"])
    pn = pn - t(step_size) * (mn / den)
    out = (pn, gn, mn, vn)
    if ema is not None:
        out += (ema + t(1.0 - ema_decay) * (pn - ema),)
    return out


def ema_chain(ps, ema0, ema_decay):
    """the EMA after the steps that left the f32 parameters ps[0], ps[1], ... (taken as given: e_p = 0), from ema0:
    (float64 ema, bound). A step's inherited error shrinks by (1 - omd)."""
    omd = omd_of(ema_decay)
    ema, bound = ema0.double(), torch.zeros_like(ema0, dtype=torch.float64)
    for p in ps:
        ema, b = ema_lerp(p.double(), 0.0, ema, ema_decay)
        bound = (1 - omd) * bound + b
    return ema, bound


def ema_axpby(p, ema, ema_decay):
    """(ema', bound) of SGD's vit_axpby(p, ema, f32(1 - d), f32(d)) on the given f32 p"""
    a, b = G.f32(1.0 - ema_decay), G.f32(ema_decay)
    x, y = a * p.double(), b * ema.double()
    out = x + y
    return out, 2 * UF * (x.abs() + y.abs() + out.abs())


def ema_axpby_chain(ps, ema0, ema_decay):
    ema, bound = ema0.double(), torch.zeros_like(ema0, dtype=torch.float64)
    b_ = G.f32(ema_decay)
    for p in ps:
        ema, b = ema_axpby(p, ema, ema_decay)
        bound = b_ * bound + b
    return ema, bound


# ---- the sweep's layout and inputs (shared by the CPU proof and the GPU gate) ----------------------------------------
def sweep_layout(lengths=G.ADAMW_LENGTHS, chunk=8192):
    """64-aligned segments with alternating decay flags (segment 0 decayed) and their chunk list, by hand:
    (starts, total, chunks int64 [nchunks, 3] = {flags, start, length}, decayed bool list). 8195 splits into 8192 + 3"""
    starts, chunks, at = [], [], 0
    for s, n in enumerate(lengths):
        starts.append(at)
        for c0 in range(0, n, chunk):
            chunks.append([1 - s % 2, at + c0, min(chunk, n - c0)])
        at += (n + 63) // 64 * 64
    return starts, at, torch.tensor(chunks, dtype=torch.int64), [s % 2 == 0 for s in range(len(lengths))]


def sweep_inputs(seed=10, lengths=G.ADAMW_LENGTHS):
    """per segment {p, g, m, v, ema} as test_glue_sweep_gpu.py draws them for AdamW (v >= 1e-4), ema ~ N(0, 1)"""
    gen = torch.Generator().manual_seed(seed)
    segs = []
    for n in lengths:
        segs.append(dict(p=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen),
                         m=torch.randn(n, generator=gen), v=torch.rand(n, generator=gen) + 1e-4,
                         ema=torch.randn(n, generator=gen)))
    return segs


def sweep_table(step, coef):
    """the float4 vit_adamw_prep writes at this step count: {lr / (1 - beta1^step), sqrt(1 - beta2^step), 1, coef}"""
    return torch.tensor([G.f32(HYPER["lr"]) / (1 - G.f32(HYPER["beta1"]) ** step),
                         math.sqrt(1 - G.f32(HYPER["beta2"]) ** step), 1.0, G.f32(coef)], dtype=torch.float32)
