"""A stage-local audit of one training step of the ViT engine (vitmi/engine.py, vitmi/wgrad.py).

A helper module like attn_ref / gemm_ref / norm_ref / glue_ref (the tests import it as `step_ref`); plain torch, so it
runs on CPU and GPU tensors alike. The kernel sweeps hold every kernel to a float64 reference with arguments the tests
choose, and the parity tests hold the whole step to norms. This module checks what lies between: which buffer, leading
dimension, dropout site, drop-path row and bf16 weight copy each launch of the real step gets.

The trace. Recorder wraps every public function of vitmi.ops (engine.py and wgrad.py look them up on the module at call
time). Every argument that is a tensor of the step's activation workspace (_Acts), or a view anywhere into one (matched
by address range), is copied before and after the call;
OUTPUTS says which parameters of which function are outputs. An argument that is not an output must be unchanged by its
call. The cross-entropy launch runs on autograd's own tensors, so all its tensors are copied under "ce.*" names. The
parameter and gradient buffers are never copied per call: they are read once after the step.

The walk. Walk.run() follows the step's data flow stage by stage. A stage is found by the buffer it writes, counted per
buffer (the rotating dhb / dg / dqkv / partial rings count as one buffer each), never by the launch index, so independent
launches may be reordered. The inputs of a stage are the engine's own outputs of the stages that feed it, as copied;
its parameters are read by name from the fp32 master weights (each bf16 weight is master.bfloat16(), never the engine's
mirror); the stage is recomputed in float64 and every output element held to the stage's own gate, so an error shows at
the stage that made it and only there. A write that no stage claims, an input changed by its launch and a missing
write fail the audit. With `sim` set the same walk generates a trace instead: every stage's float64 value rounded once
to its storage type (the CPU self-test's clean trace, and, through `sim`'s fault entries, its planted errors).

Gates, all per element (u = 2^-24 the f32 unit roundoff; half a bf16 ulp is norm_ref.half_ulp_bf16: 2^-9 of the top of
the value's binade, so between 2^-9 |ref| and 2^-8 |ref|; a flat 2^-9 |ref| is below what round-to-nearest does at the
low end of a binade and a correct kernel would miss it):

  LayerNorm forward / backward and their three column sums: norm_ref.fwd / bwd / colsums unchanged.
  Attention forward / backward and its bias partials: attn_ref.bounds unchanged (the backward from the engine's own o /
  lse, compared with the reference from qkv alone, as the attention sweep does).
  Cross entropy: glue_ref.cross_entropy unchanged.
  im2col, copies, zero fills, the drop-path table: equal.

  GEMM with general bf16 operands (mm()). A product of two bf16 values is exact in f32. K - 1 additions rounded to
  nearest, in any order and over any split, are off by at most (K - 1) u (|A| |B|)_ij to first order. The gate takes
      E = K 2^-23 (|A| |B|)_ij,
  twice that: the doubling covers the MFMA's internal sums, whose rounding the ISA does not document. Split-K slabs and
  their fixed-order reduction, the direct table members and the f32 classifier GEMMs (K products rounded once each and
  K - 1 sums: at most 2 K - 1 roundings of u, below K 2^-23) fall under the same E. E is carried through the epilogue:
      qkv            bf16(acc + b):       E + u |ref| (the bias addition), then the bf16 rounding
      hm, h[i+1]     res + s d (acc + b): |s d| E + u |branch| (the bias addition) + 2^-23 (|branch| + |ref|) (the
                                          product with s d and the residual addition, doubled as in
                                          test_drop_path_gpu's derivation)
      h[0]           PATCH:               d E + 2^-23 (d (|acc + b| + |pos|) + |ref|)
      gp, g          fc1:                 with E' = E + u |u|: d sup|gelu''| E' resp. d sup|gelu'| E' (SUP_D2GELU,
                                          SUP_DGELU; the CPU test checks both suprema on a grid), plus gemm_ref's
                                          U |ref| + C_DGELU d max(1, |u|) for the erf approximation and the rounding
      dg             bf16(acc gp):        |gp| E + u |ref|, then the bf16 rounding; its column partials the row sums of
                                          that without the rounding
      dyln, dO       bf16(acc):           E, then the bf16 rounding
      logits, dlncls f32:                 E + 2^-23 |ref|
  "then the bf16 rounding" is b16(): (1 + 2^-8) e + half a bf16 ulp of ref (a value within e of ref is rounded).
  Weight gradients A^T B over the T token rows: E (K = T) + 2^-23 (|ref| + |prior|) for the store and, in an
  accumulating backward, the addition to the prior value.

  Column sums over R rows (the bias gradients from their partial buffers, the classifier bias, the embedding
  gradients): every term passes at most R additions (the accumulation onto the prior included):
  SLACK R u (sum |x| + |prior|). A partial buffer is checked at the stage that writes it: the sum of its valid rows
  against the float64 column sums of the stage's reference, with the rows' own bounds summed and R u sum|x| for the
  additions inside the kernel (R = the stage's rows) and the partial rows' own sum.

Invariants: after an overwriting backward into a NaN-filled gradient buffer every parameter element is finite (no
gradient launch dropped) and every alignment gap still NaN; rows T..Tp of every bf16 operand buffer (K rows of the
weight gradients) are 0 after the step.
"""
import inspect
import re

import torch

import attn_ref as AR
import gemm_ref as GR
import glue_ref as G
import norm_ref as NR
from oracle.dropout import dropout_mult

UF = G.UF
SLACK = NR.SLACK
SUP_DGELU = 1.13      # sup |gelu'|  = 1.1290 at u = sqrt 2
SUP_D2GELU = 0.8      # sup |gelu''| = 2 pdf(0) = 0.7979 at u = 0
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
ROTATING = ("dhb", "dg", "dqkv", "lnparts", "gelu_parts", "qkv_bparts")
SCRATCH = ("attn_ws",)
# bf16 operand buffers whose rows past the data are K rows of weight gradients: (name, True: rows T..Tp, False: b..bp)
PAD_BUFFERS = (("patches", True), ("ln1", True), ("ln2", True), ("o", True), ("g", True), ("dhb", True), ("dg", True),
               ("dqkv", True), ("c_o", False), ("c_ln2", False), ("c_dh", False), ("c_dh2", False), ("c_dyln", False),
               ("c_g", False), ("c_gp", False), ("c_dg", False))

# per vitmi.ops function: the parameters that are outputs (others are inputs); functions that take no workspace tensor
# need no entry. A function missing here that is handed a workspace tensor makes an unrecognised write.
OUTPUTS = {
    "gemm": ("C", "C2", "col_partial"), "gemm_drop_path": ("C", "C2", "col_partial"), "gemm_f32": ("C",),
    "layernorm_fwd": ("y", "mean", "rstd"),
    "layernorm_bwd": ("dx", "dx_bf16", "partial", "dgamma_dbeta", "dx_colsum"),
    "attention_fwd": ("o", "lse"), "attention_bwd": ("dqkv", "bias_partial", "workspace"),
    "im2col_hw": ("out",), "copy2d": ("dst",), "zero_": ("t",), "drop_path_scales": ("out",),
    "cross_entropy": ("dlogits", "row_stats"), "cross_entropy_soft": ("dlogits", "row_stats"),
    "embed_grad": ("dpos", "dcls", "dconv_bias"), "colsum_batch": (), "splitk_reduce": ("out",),
    "splitk_reduce_group": (), "gemm_splitk_group": (), "drop_path_desc": (),
}
QUERIES = ("gemm_partial_rows", "gemm_tile_rows", "gemm_split_rows")   # host-side questions: nothing is launched
CE = ("cross_entropy", "cross_entropy_soft")


def _rup(x, m):
    return (x + m - 1) // m * m


class Dims:
    def __init__(self, image_hw, patch_hw, D, M, H, L, C, b):
        (ih, iw), (fh, fw) = image_hw, patch_hw
        self.image_hw, self.patch_hw = (ih, iw), (fh, fw)
        self.D, self.M, self.H, self.L, self.C, self.b = D, M, H, L, C, b
        self.hd = D // H
        self.N = (ih // fh) * (iw // fw) + 1
        self.T = b * self.N
        self.Tp, self.bp = _rup(self.T, 64), _rup(b, 64)
        self.pk = 3 * fh * fw
        self.kpad = _rup(self.pk, 64)

    def shape(self, buf):
        """(shape, dtype) of a workspace buffer by its name (the simulated trace allocates from it)"""
        n = re.sub(r"\[\d+\]", "", buf)
        D, M, T, Tp, b, bp = self.D, self.M, self.T, self.Tp, self.b, self.bp
        table = {"patches": ((Tp, self.kpad), BF16), "h": ((Tp, D), F32), "hm": ((Tp, D), F32), "ln1": ((Tp, D), BF16),
                 "ln2": ((Tp, D), BF16), "o": ((Tp, D), BF16), "qkv": ((Tp, 3 * D), BF16), "gp": ((Tp, M), BF16),
                 "g": ((Tp, M), BF16), "lse": ((b, self.H, self.N), F32), "lncls": ((b, D), F32),
                 "logits": ((b, self.C), F32), "dh": ((Tp, D), F32), "dhb": ((Tp, D), BF16), "dg": ((Tp, M), BF16),
                 "dyln": ((Tp, D), BF16), "dO": ((Tp, D), BF16), "dqkv": ((Tp, 3 * D), BF16), "dlncls": ((b, D), F32),
                 "path_scale": ((2 * self.L, b), F32), "ce.dlogits": ((b, self.C), F32), "ce.row_stats": ((b, 3), F32),
                 "c_o": ((bp, D), BF16), "c_ln2": ((bp, D), BF16), "c_dh": ((bp, D), BF16), "c_dh2": ((bp, D), BF16),
                 "c_dyln": ((bp, D), BF16), "c_g": ((bp, M), BF16), "c_gp": ((bp, M), BF16), "c_dg": ((bp, M), BF16)}
        if n in ("mu1", "rs1", "mu2", "rs2"):
            return (T,), F32
        if n in ("muf", "rsf", "c_mu2", "c_rs2"):
            return (b,), F32
        return table[n]


class Layout:
    """the flat parameter / gradient layout: offsets and shapes by name (vitmi.engine.FlatLayout's, or made here)"""

    def __init__(self, offsets, shapes, numel):
        self.offsets, self.shapes, self.numel = offsets, shapes, numel

    def view(self, buf, name):
        n = 1
        for s in self.shapes[name]:
            n *= s
        return buf[self.offsets[name]:self.offsets[name] + n].view(self.shapes[name])

    def gap_mask(self, device):
        m = torch.ones(self.numel, dtype=torch.bool, device=device)
        for name in self.offsets:
            self.view(m, name).fill_(False)
        return m


class Event:
    def __init__(self, fn, pre, post, writes, info=None):
        self.fn, self.pre, self.post, self.writes, self.info = fn, pre, post, set(writes), info or {}


class Trace:
    """dims, x, labels; p_drop, path (per-site rates or None), seed, offset; pruned, accumulate; events; after the
    step: master {name: f32}, layout, grad_before / grad_after (flat), nan_filled, pads {buffer: copy}; mirror {name:
    bf16} in a simulated trace"""

    def __init__(self, dims, x, labels, p_drop=0.0, path=None, seed=0, offset=0, pruned=True, accumulate=False):
        self.dims, self.x, self.labels = dims, x, labels
        self.p_drop, self.path, self.seed, self.offset = float(p_drop or 0.0), path, seed, offset
        self.pruned, self.accumulate = pruned, accumulate
        self.events, self.master, self.layout, self.mirror = [], None, None, None
        self.grad_before = self.grad_after = None
        self.nan_filled, self.pads = False, {}


class AuditError(AssertionError):
    pass


# ---- the recorder ----------------------------------------------------------------------------------------------------
def _tensors(value, path):
    """(path, tensor) of every tensor inside an argument (lists, tuples and dicts are walked)"""
    if isinstance(value, torch.Tensor):
        yield path, value
    elif isinstance(value, (list, tuple)):
        for k, v in enumerate(value):
            yield from _tensors(v, f"{path}.{k}")
    elif isinstance(value, dict):
        for k, v in value.items():
            yield from _tensors(v, f"{path}.{k}" if path else str(k))


class Recorder:
    """Wraps vitmi.ops for one step of `eng` at batch size b. pre_hooks / post_hooks: {function name: callable(recorder,
    arguments dict)} run before / after the real call (before the copies after it are taken): the planted wiring
    errors. `arguments` holds the call's parameters by name, ops.gemm's keywords flattened into it; a pre-hook may
    change entries."""

    def __init__(self, eng, b):
        self.eng, self.b = eng, b
        self.events, self.depth, self.active = [], 0, False
        self.pre_hooks, self.post_hooks = {}, {}
        self.calls = {}

    def names(self):
        a = self.eng._acts.get(self.b)      # (never allocates: the allocation itself asks wrapped functions)
        out = {}
        if a is None:
            return out
        for k, v in vars(a).items():
            if k in ("dhb", "dg", "dqkv") and getattr(a, k + "_l") is not None:
                continue
            k = k[:-2] if k.endswith("_l") else k
            if isinstance(v, torch.Tensor):
                out[v.data_ptr()] = (k, v)
            elif isinstance(v, (list, tuple)):
                for i, t in enumerate(v):
                    if isinstance(t, torch.Tensor):
                        out[t.data_ptr()] = (f"{k}[{i}]", t)
        return out

    @staticmethod
    def find(names, t):
        """(buffer name, tensor to copy) of a launch argument, or (None, None) for a tensor outside the workspace. A
        view that starts inside a buffer is named "<buffer>+<byte offset>" and the whole buffer is copied, so a write
        through it is a write no stage claims."""
        p = t.data_ptr()
        hit = names.get(p)
        if hit is not None:
            return hit
        for start, (name, base) in names.items():
            if start < p < start + base.numel() * base.element_size():
                return f"{name}+{p - start}", base
        return None, None

    def buffer(self, name):
        """the workspace tensor of that name"""
        a = self.eng.acts(self.b)
        m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
        if not m:
            return getattr(a, name)
        lst = getattr(a, m.group(1) + "_l", None) or getattr(a, m.group(1))
        return lst[int(m.group(2))]

    def install(self, monkeypatch, ops):
        for name, fn in list(vars(ops).items()):
            if inspect.isfunction(fn) and not name.startswith("_") and fn.__module__ == ops.__name__:
                monkeypatch.setattr(ops, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)
        kwname = next((p.name for p in sig.parameters.values() if p.kind == p.VAR_KEYWORD), None)

        def wrapped(*args, **kw):
            if not self.active or self.depth:      # (ops.gemm calls ops.gemm_drop_path: one launch, one event)
                return fn(*args, **kw)
            ba = sig.bind(*args, **kw)
            ba.apply_defaults()
            arg = dict(ba.arguments)
            if kwname:
                arg.update(arg.pop(kwname))
            n = self.calls[name] = self.calls.get(name, 0) + 1
            arg["_call"] = n
            hook = self.pre_hooks.get(name)
            if hook:
                hook(self, arg)
            call = {k: v for k, v in arg.items() if k != "_call"}
            names = self.names()
            ws = {}
            for path, t in _tensors(call, ""):
                buf, t = self.find(names, t) if name not in CE else ("ce." + path, t)
                if buf is not None and buf not in SCRATCH:
                    ws[path] = (buf, t)
            if name in QUERIES:
                r = fn(**call)
                if "col_partial" in ws:      # the rows the launch just issued wrote: kept with that launch's event
                    for ev in reversed(self.events):
                        if ws["col_partial"][0] in ev.writes:
                            ev.info["partial_rows"] = r
                            break
                return r
            pre = {buf: t.detach().clone() for buf, t in ws.values()}
            self.depth += 1
            try:
                r = fn(**call)
            finally:
                self.depth -= 1
            hook = self.post_hooks.get(name)
            if hook:
                hook(self, arg)
            if ws:
                post = {buf: t.detach().clone() for buf, t in ws.values()}
                outs = OUTPUTS.get(name)
                writes = [buf for path, (buf, _) in ws.items() if outs is None or path.split(".")[0] in outs]
                self.events.append(Event(name, pre, post, writes, {"unknown": outs is None}))
            return r
        return wrapped

    def trace(self, x, labels, accumulate=False, grad_before=None, nan_filled=False):
        """the Trace of the recorded step; call after the backward (reads the master weights and the gradient)"""
        eng, cfg = self.eng, self.eng.cfg
        a = eng.acts(self.b)
        d = Dims(cfg.image_hw, cfg.patch_hw, cfg.emb_dim, cfg.mlp_dim, cfg.num_heads, cfg.num_layers, cfg.num_classes,
                 self.b)
        seed, off = eng.drop_seed, eng._drop_offset
        tr = Trace(d, x.detach().clone(), labels.detach().clone(), eng._drop[0] if eng._drop else 0.0,
                   list(eng._path) if eng._path else None, seed, off, eng._pruned, accumulate)
        tr.events = self.events
        tr.layout = Layout(dict(eng.layout.offsets), dict(eng.layout.shapes), eng.layout.numel)
        tr.master = {k: eng.pv(k).detach().clone() for k in eng.layout.offsets}
        tr.grad_before, tr.grad_after, tr.nan_filled = grad_before, eng.grad.detach().clone(), nan_filled
        for name, _ in PAD_BUFFERS:
            v = getattr(a, name + "_l", None) or getattr(a, name)
            for i, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
                tr.pads[f"{name}[{i}]" if isinstance(v, (list, tuple)) else name] = t.detach().clone()
        return tr


# ---- references ------------------------------------------------------------------------------------------------------
def mm(A, B):
    """float64 A [m, k] @ B [k, n] and the accumulation gate E = k 2^-23 |A| |B| (module docstring)"""
    A, B = A.double(), B.double()
    return A @ B, A.shape[1] * 2.0 ** -23 * (A.abs() @ B.abs())


def b16(ref, e):
    """the gate of bf16(value) for a value within e of ref"""
    return (1.0 + 2.0 ** -8) * e + NR.half_ulp_bf16(ref.double())


def im2col(x, Ph, Pw, kpad):
    """f32 [b N, kpad]: torch's unfold in the kernel's (channel, row, column) order, a zero cls row per image"""
    B, _, Hh, Ww = x.shape
    gh, gw = Hh // Ph, Ww // Pw
    cols = x[:, :, :gh * Ph, :gw * Pw].unfold(2, Ph, Ph).unfold(3, Pw, Pw).permute(0, 2, 3, 1, 4, 5)
    ref = torch.zeros(B, gh * gw + 1, kpad, device=x.device)
    ref[:, 1:, :3 * Ph * Pw] = cols.reshape(B, gh * gw, 3 * Ph * Pw)
    return ref.reshape(B * (gh * gw + 1), kpad)


def kind_of(stage):
    return re.sub(r"\[\d+\]", "", stage)


def family(buf):
    n = re.sub(r"\[\d+\]", "", buf)
    return n if n in ROTATING else buf


class Walk:
    """Walk(trace).run(): the audit. Walk(trace, sim={...}).run(): fill the trace with the references' own values.
    After the audit: stages (names in order), failed (names of stages past their gate, in order), ratios {stage kind:
    worst ratio}, problems (unclaimed writes, changed inputs, broken invariants)."""

    def __init__(self, tr, sim=None):
        self.tr, self.d, self.sim = tr, tr.dims, sim
        self.stages, self.failed, self.ratios, self.problems, self.detail = [], [], {}, [], {}
        self.pos, self.by_family, self.claimed = {}, {}, set()
        self.rot = {}
        self.dev = tr.x.device
        if sim is None:
            for k, ev in enumerate(tr.events):
                for buf in ev.post:
                    if buf in ev.writes:
                        self.by_family.setdefault(family(buf), []).append((k, ev, buf))
        else:
            self.state = {}
        self.wg, self.bias_src = {}, {}

    # -- bookkeeping
    def _stage(self, stage):
        if stage not in self.stages:
            self.stages.append(stage)

    def _fail(self, stage, why):
        if stage not in self.failed:
            self.failed.append(stage)
        self.detail.setdefault(stage, []).append(why)

    def _cmp(self, stage, label, got, ref, bound):
        ref = ref.double()
        bound = bound if isinstance(bound, torch.Tensor) else torch.full_like(ref, float(bound))
        ratio, at = G.worst(got, ref, bound.double().expand_as(ref))
        k = kind_of(stage)
        self.ratios[k] = max(self.ratios.get(k, 0.0), ratio)
        if not ratio <= 1.0:
            self._fail(stage, f"{label}: {ratio:.3g} x gate at {at}")

    def _take(self, stage, fam):
        lst, i = self.by_family.get(fam, []), self.pos.get(fam, 0)
        if i >= len(lst):
            raise AuditError(f"stage {stage}: no launch wrote {fam} (write {i} of that buffer)")
        self.pos[fam] = i + 1
        k, ev, buf = lst[i]
        self.claimed.add((k, buf))
        return ev, buf

    def _sim_buf(self, fam):
        if fam in ROTATING:
            i = self.rot[fam] = self.rot.get(fam, -1) + 1
            return f"{fam}[{i % 2}]"
        return fam

    def out(self, stage, fam, ref, bound, sel=None, outside=None):
        """one output of a stage: the region sel(buffer) against ref / bound (audit) or written from ref (sim);
        outside: the buffer's expected content everywhere else (compared for equality). Returns the whole buffer."""
        self._stage(stage)
        sel = sel or (lambda t: t)
        if self.sim is None:
            ev, buf = self._take(stage, fam)
            got = ev.post[buf]
            self._cmp(stage, buf, sel(got), ref, bound)
            if outside is not None:
                rest = got.clone()
                sel(rest).copy_(sel(outside))
                if G.first_diff(rest, outside) is not None:
                    self._fail(stage, f"{buf}: changed outside the stage's rows at {G.first_diff(rest, outside)}")
            return got
        buf = self._sim_buf(fam)
        shape, dt = self.d.shape(buf)
        base = outside.clone() if outside is not None else self.state.get(buf, torch.zeros(shape, dtype=dt)).clone()
        sel(base).copy_(ref.to(dt))
        fault = self.sim.get("post", {}).get(stage)
        if fault:
            fault(buf, base)
        self.state[buf] = base
        self.tr.events.append(Event("sim", {}, {buf: base}, [buf]))
        return base

    def partial(self, stage, fam, rows, ref, bound, terms):
        """a partial-sum buffer: the sum of its `rows` valid rows (None: as the launch reported) against the float64
        column sums `ref`; terms = the stage's rows (additions inside the kernel). Returns the valid rows."""
        self._stage(stage)
        n = ref.numel()
        if self.sim is not None:
            buf = self._sim_buf(fam)
            t = torch.zeros(2, n)
            t[0] = ref.float()
            self.tr.events.append(Event("sim", {}, {buf: t}, [buf], {"partial_rows": 1}))
            return t[:1]
        ev, buf = self._take(stage, fam)
        rows = ev.info.get("partial_rows") if rows is None else ev.post[buf].shape[0] if rows == "all" else rows
        if rows is None:
            raise AuditError(f"stage {stage}: the launch that wrote {buf} never said how many partial rows it wrote")
        got = ev.post[buf][:rows, :n]
        mag = got.double().abs().sum(0)
        self._cmp(stage, buf, got.double().sum(0), ref, bound + SLACK * (terms + rows) * UF * mag)
        return got

    def grad(self, name, ref, bound, stage=None):
        """a parameter's gradient in the flat buffer after the step (+ the prior value when accumulating)"""
        stage = stage or "grad." + name.replace("transformer.encoder_layers.", "").replace("transformer.", "")
        stage = re.sub(r"^grad\.(\d+)\.(.*)$", r"grad.\2[\1]", stage)
        self._stage(stage)
        tr = self.tr
        ref = ref.double().reshape(tr.layout.shapes[name])
        bound = bound.double().reshape(ref.shape)
        prior = tr.layout.view(tr.grad_before, name).double() if tr.accumulate else None
        if self.sim is not None:
            if prior is not None and name not in self.sim.get("no_prior", ()):
                ref = ref + prior
            tr.layout.view(tr.grad_after, name).copy_(ref.float())
            return
        if prior is not None:
            ref, bound = ref + prior, bound + 2.0 ** -23 * (ref + prior).abs() + UF * prior.abs()
        self._cmp(stage, name, tr.layout.view(tr.grad_after, name), ref, bound)

    # -- parameters
    def P(self, name):
        return self.tr.master[name].double()

    def W(self, name):
        """a bf16 GEMM weight: bf16(master), by name (the simulated engine reads its mirror)"""
        if self.sim is not None:
            return self.tr.mirror[name].double()
        return self.tr.master[name].bfloat16().double()

    def lp(self, i, s):
        return f"transformer.encoder_layers.{i}.{s}"

    # -- masks
    def dm(self, stage, site, rows, cols, stride=1):
        """dropout multipliers [rows, cols] of `site` (mask row = row * stride)"""
        tr = self.tr
        if not tr.p_drop:
            return torch.ones(rows, cols, dtype=F64, device=self.dev)
        if self.sim is not None:
            site += self.sim.get("site", {}).get(stage, 0)
        m = dropout_mult(tr.p_drop, site, tr.seed, tr.offset, rows, cols, row_stride=stride)
        return torch.from_numpy(m).to(self.dev).double()

    def ps(self, table, site, rows, rows_per_sample):
        """drop-path multipliers [rows, 1] of branch `site` from the table the forward wrote"""
        tr = self.tr
        if not tr.path or site < 0 or not tr.path[site] > 0.0:
            return torch.ones(rows, 1, dtype=F64, device=self.dev)
        idx = torch.arange(rows, device=self.dev) // rows_per_sample
        return table[site].double()[idx][:, None]

    # -- the walk
    def run(self):
        self.forward()
        self.loss()
        self.backward()
        self.grads()
        if self.sim is None:
            self.finish()
        return self

    def forward(self):
        tr, d = self.tr, self.d
        D, M, H, hd, L, N, b, T = d.D, d.M, d.H, d.hd, d.L, d.N, d.b, d.T
        rows = lambda t: t[:T]
        cls = lambda t: t[:T].view(b, N, -1)[:, 0]
        self.ps_tab = None
        if tr.path:
            ref = torch.stack([torch.from_numpy(dropout_mult(p, 0x80000000 | s, tr.seed, tr.offset, b, 1)[:, 0])
                               for s, p in enumerate(tr.path)]).to(self.dev)
            self.ps_tab = self.out("fwd.path_scale", "path_scale", ref, 0.0)
        self.ps_bwd = self.ps_tab
        if self.sim is not None and tr.path and self.sim.get("path_bwd"):
            self.ps_bwd = self.sim["path_bwd"](self.ps_tab.clone())
        # patch embedding
        pat = torch.zeros(d.Tp, d.kpad, device=self.dev)
        pat[:T] = im2col(tr.x.float(), *d.patch_hw, d.kpad)
        self.patches = self.out("fwd.patches", "patches", pat.bfloat16(), 0.0)
        acc, E = mm(self.patches[:T, :d.pk], self.W("embedding.weight").reshape(D, d.pk).t())
        u = acc + self.P("embedding.bias")[None]
        pos = self.P("transformer.pos_embedding.pos_embedding").reshape(N, D)
        t = torch.arange(T, device=self.dev) % N
        first = (t == 0)[:, None]
        body, mag = u + pos[t], u.abs() + pos[t].abs()
        c = (self.P("cls_token").reshape(D) + pos[0])[None].expand_as(body)
        cmag = (self.P("cls_token").reshape(D).abs() + pos[0].abs())[None].expand_as(body)
        d0 = self.dm("fwd.h[0]", 0, T, D)
        ref = torch.where(first, c, body) * d0
        bound = torch.where(first, torch.zeros_like(E), d0 * E) + 2.0 ** -23 * (d0 * torch.where(first, cmag, mag)
                                                                               + ref.abs())
        h = [self.out("fwd.h[0]", "h[0]", ref, bound, rows)]
        self.hm, self.ln1, self.mu1, self.rs1, self.qkv, self.o, self.lse = [], [], [], [], [], [], []
        self.ln2, self.mu2, self.rs2, self.gp, self.g = [], [], [], [], []
        scale = 1.0 / hd ** 0.5
        for i in range(L):
            last = tr.pruned and i == L - 1
            lp = lambda s: self.lp(i, s)
            st = f"fwd.ln1[{i}]"
            r = NR.fwd(h[i][:T], self.P(lp("norm1.weight")), self.P(lp("norm1.bias")))
            self.ln1.append(self.out(st, f"ln1[{i}]", r.y, r.b_y16, rows))
            self.mu1.append(self.out(st, f"mu1[{i}]", r.mean, r.b_mean))
            self.rs1.append(self.out(st, f"rs1[{i}]", r.rstd, r.b_rstd))
            w = torch.cat([self.W(lp(f"attn.{z}.weight")).reshape(D, D) for z in ("query", "key", "value")], 1)
            bq = torch.cat([self.P(lp(f"attn.{z}.bias")).reshape(D) for z in ("query", "key", "value")])
            acc, E = mm(self.ln1[i][:T], w)
            ref = acc + bq[None]
            self.qkv.append(self.out(f"fwd.qkv[{i}]", f"qkv[{i}]", ref, b16(ref, E + UF * ref.abs()), rows))
            R = 1 if last else N
            st = f"fwd.attn[{i}]"
            ar = AR.reference(self.qkv[i][:T], None, b, N, H, hd, scale, q_rows=1 if last else None)
            bd = AR.bounds(ar)
            tok = lambda x: x.permute(0, 2, 1, 3).reshape(b, R, D)
            self.o.append(self.out(st, f"o[{i}]", tok(ar.o), tok(bd["o"]), lambda t: t[:T].view(b, N, D)[:, :R]))
            self.lse.append(self.out(st, f"lse[{i}]", ar.lse, bd["lse"], lambda t: t[:, :, :R]))
            part = cls if last else rows            # the pruned last layer: the cls rows only (row stride N D)
            nr = b if last else T
            # out-projection + residual
            st = f"fwd.hm[{i}]"
            acc, E = mm(part(self.o[i]), self.W(lp("attn.out.weight")).reshape(D, D))
            sd = self.dm(st, 1 + 3 * i, T, D) * self.ps(self.ps_tab, 2 * i, T, N) if not last else torch.ones_like(acc)
            u = acc + self.P(lp("attn.out.bias"))[None]
            ref = part(h[i]).double() + u * sd
            bound = sd * E + UF * (u * sd).abs() + 2.0 ** -23 * ((u * sd).abs() + ref.abs())
            self.hm.append(self.out(st, f"hm[{i}]", ref, bound, part))
            if last:
                self.c_o = self.out("fwd.c_o", "c_o", cls(self.o[i]), 0.0, lambda t: t[:b])
            # LayerNorm 2
            st = f"fwd.ln2[{i}]"
            r = NR.fwd(part(self.hm[i]), self.P(lp("norm2.weight")), self.P(lp("norm2.bias")))
            pre = "c_" if last else ""
            idx = "" if last else f"[{i}]"
            top = (lambda t: t[:b]) if last else rows
            self.ln2.append(self.out(st, f"{pre}ln2{idx}", r.y, r.b_y16, top))
            self.mu2.append(self.out(st, f"{pre}mu2{idx}", r.mean, r.b_mean))
            self.rs2.append(self.out(st, f"{pre}rs2{idx}", r.rstd, r.b_rstd))
            # fc1: gelu' and gelu, each times the dropout multiplier
            st = f"fwd.fc1[{i}]"
            acc, E = mm(top(self.ln2[i]), self.W(lp("mlp.fc1.weight")).t())
            u = acc + self.P(lp("mlp.fc1.bias"))[None]
            E = E + UF * u.abs()
            gl, dg = GR.gelu64(u)
            dmul = self.dm(st, 2 + 3 * i, nr, M)
            erf = GR.C_DGELU * dmul * u.abs().clamp_min(1.0)
            self.gp.append(self.out(st, f"{pre}gp{idx}", dg * dmul, dmul * SUP_D2GELU * E + GR.U * (dg * dmul).abs() + erf,
                                    top))
            self.g.append(self.out(st, f"{pre}g{idx}", gl * dmul, dmul * SUP_DGELU * E + GR.U * (gl * dmul).abs() + erf,
                                   top))
            # fc2 + residual
            st = f"fwd.h[{i + 1}]"
            acc, E = mm(top(self.g[i]), self.W(lp("mlp.fc2.weight")).t())
            sd = self.dm(st, 3 + 3 * i, T, D) * self.ps(self.ps_tab, 2 * i + 1, T, N) if not last else torch.ones_like(acc)
            u = acc + self.P(lp("mlp.fc2.bias"))[None]
            ref = part(self.hm[i]).double() + u * sd
            bound = sd * E + UF * (u * sd).abs() + 2.0 ** -23 * ((u * sd).abs() + ref.abs())
            h.append(self.out(st, f"h[{i + 1}]", ref, bound, part))
        self.h = h
        r = NR.fwd(cls(h[L]), self.P("transformer.norm.weight"), self.P("transformer.norm.bias"))
        self.lncls = self.out("fwd.lncls", "lncls", r.y, r.b_y)
        self.muf = self.out("fwd.lncls", "muf", r.mean, r.b_mean)
        self.rsf = self.out("fwd.lncls", "rsf", r.rstd, r.b_rstd)
        acc, E = mm(self.lncls, self.P("classifier.weight").t())
        ref = acc + self.P("classifier.bias")[None]
        self.logits = self.out("fwd.logits", "logits", ref, E + 2.0 ** -23 * ref.abs())

    def loss(self):
        tr, b = self.tr, self.d.b
        r = G.cross_entropy(self.logits, tr.labels, 1.0 / b)
        if self.sim is None:
            ev = next((e for e in tr.events if "ce.logits" in e.pre), None)
            if ev is not None and G.first_diff(ev.pre["ce.logits"], self.logits) is not None:
                self._stage("loss")
                self._fail("loss", "the cross entropy did not read the forward's logits")
        self.dl = self.out("loss", "ce.dlogits", r.dlogits, r.bound_d)
        st = torch.stack([r.loss, r.top1, r.top5], 1)
        self.out("loss", "ce.row_stats", st, torch.stack([r.bound_loss, 0 * r.top1, 0 * r.top5], 1))

    def ln_bwd(self, stage, dy, x, mean, rstd, gamma, dres, mult, names):
        """NR.bwd of one LayerNorm backward and its three column sums; names: the parameters the sums belong to"""
        r = NR.bwd(dy, x, mean, rstd, self.P(gamma), dres=dres, mult=mult)
        nrows = x.shape[0]
        refs, bnds = NR.colsums(r, nrows)
        part = self.partial(stage, "lnparts", NR.bwd_blocks(nrows), torch.cat(refs), torch.cat(bnds), nrows)
        D = self.d.D
        for k, name in enumerate(names):
            if name is not None:
                self.bias_src[name] = part[:, k * D:(k + 1) * D]
        return r

    def backward(self):
        tr, d = self.tr, self.d
        D, M, H, hd, L, N, b, T, C = d.D, d.M, d.H, d.hd, d.L, d.N, d.b, d.T, d.C
        rows = lambda t: t[:T]
        top = lambda t: t[:b]
        cls = lambda t: t[:T].view(b, N, -1)[:, 0]
        pruned = tr.pruned
        dl = self.dl
        acc, E = mm(dl, self.P("classifier.weight"))
        self.dlncls = self.out("bwd.dlncls", "dlncls", acc, E + 2.0 ** -23 * acc.abs())
        zD = torch.zeros(d.Tp, D, device=self.dev)
        dh = self.out("bwd.zero_dh", "dh", zD, 0.0)
        if not pruned:
            self.out("bwd.zero_dhb", "dhb", zD.bfloat16(), 0.0)
        # final LayerNorm, on the cls rows
        st = "bwd.lnf"
        mult = self.dm(st, 3 + 3 * (L - 1), b, D, N) * self.ps(self.ps_bwd, 2 * (L - 1) + 1, b, 1)
        r = self.ln_bwd(st, self.dlncls, cls(self.h[L]), self.muf, self.rsf, "transformer.norm.weight", None, mult,
                        ("transformer.norm.weight", "transformer.norm.bias", self.lp(L - 1, "mlp.fc2.bias")))
        dh = self.out(st, "dh", r.dx, r.b_dx, cls, outside=dh)
        if pruned:
            dhb = self.out(st, "c_dh", r.dxm, r.b_dx16, top)
        else:
            dhb = self.out(st, "dhb", r.dxm, r.b_dx16, cls, outside=zD.bfloat16())
        scale = 1.0 / hd ** 0.5
        for i in reversed(range(L)):
            lp = lambda s: self.lp(i, s)
            last = pruned and i == L - 1
            part, nr = (top, b) if last else (rows, T)
            pre, idx = ("c_", "") if last else ("", f"[{i}]")
            # MLP
            self.wg[lp("mlp.fc2.weight")] = (part(dhb), part(self.g[i]))
            st = f"bwd.dg[{i}]"
            gp = part(self.gp[i]).double()
            acc, E = mm(part(dhb), self.W(lp("mlp.fc2.weight")))
            ref, e = acc * gp, gp.abs() * E + UF * (acc * gp).abs()
            dg = self.out(st, "c_dg" if last else "dg", ref, b16(ref, e), part)
            self.bias_src[lp("mlp.fc1.bias")] = self.partial(st, "gelu_parts", None, ref.sum(0), e.sum(0), nr)
            self.wg[lp("mlp.fc1.weight")] = (part(dg), part(self.ln2[i]))
            acc, E = mm(part(dg), self.W(lp("mlp.fc1.weight")))
            dyln = self.out(f"bwd.dyln_mlp[{i}]", "c_dyln" if last else "dyln", acc, b16(acc, E), part)
            # LayerNorm 2: dh in place (dres), the bf16 copy times the attention branch's multipliers
            st = f"bwd.ln2[{i}]"
            sel = cls if last else rows
            mult = torch.ones(nr, D, dtype=F64, device=self.dev) if last else \
                self.dm(st, 1 + 3 * i, T, D) * self.ps(self.ps_bwd, 2 * i, T, N)
            r = self.ln_bwd(st, part(dyln), sel(self.hm[i]), self.mu2[i], self.rs2[i], lp("norm2.weight"), sel(dh), mult,
                            (lp("norm2.weight"), lp("norm2.bias"), lp("attn.out.bias")))
            dh = self.out(st, "dh", r.dx, r.b_dx, sel, outside=dh if last else None)
            dhb = self.out(st, "c_dh2" if last else "dhb", r.dxm, r.b_dx16, part)
            # attention: out-projection weight and data gradient
            self.wg[lp("attn.out.weight")] = (part(self.c_o if last else self.o[i]), part(dhb))
            acc, E = mm(part(dhb), self.W(lp("attn.out.weight")).reshape(D, D).t())
            if last:
                self.out("bwd.zero_dO", "dO", zD.bfloat16(), 0.0)
            dO = self.out(f"bwd.dO[{i}]", "dO", acc, b16(acc, E), sel, outside=zD.bfloat16() if last else None)
            st = f"bwd.attn[{i}]"
            ar = AR.reference(self.qkv[i][:T], dO[:T], b, N, H, hd, scale, q_rows=1 if last else None)
            bd = AR.bounds(ar)
            tok = lambda q, k, v: torch.stack([x.permute(0, 2, 1, 3) for x in (q, k, v)], 2).reshape(T, 3 * D)
            dqkv = self.out(st, "dqkv", tok(ar.dq, ar.dk, ar.dv), tok(bd["dq"], bd["dk"], bd["dv"]), rows)
            bias = self.partial(st, "qkv_bparts", "all", ar.bias.reshape(b, 3 * D).sum(0),
                                bd["bias"].reshape(b, 3 * D).sum(0), N)
            for z, name in enumerate(("query", "key", "value")):
                self.bias_src[lp(f"attn.{name}.bias")] = bias[:, z * D:(z + 1) * D]
                self.wg[lp(f"attn.{name}.weight")] = (self.ln1[i][:T], dqkv[:T, z * D:(z + 1) * D])
            w = torch.cat([self.W(lp(f"attn.{z}.weight")).reshape(D, D) for z in ("query", "key", "value")], 1)
            acc, E = mm(dqkv[:T], w.t())
            dyln = self.out(f"bwd.dyln_qkv[{i}]", "dyln", acc, b16(acc, E), rows)
            # LayerNorm 1: the bf16 copy times the multipliers of the branch below (the position dropout at layer 0)
            st = f"bwd.ln1[{i}]"
            mult = self.dm(st, 3 + 3 * (i - 1), T, D) * self.ps(self.ps_bwd, 2 * (i - 1) + 1, T, N) if i > 0 else \
                self.dm(st, 0, T, D)
            r = self.ln_bwd(st, dyln[:T], self.h[i][:T], self.mu1[i], self.rs1[i], lp("norm1.weight"), dh[:T], mult,
                            (lp("norm1.weight"), lp("norm1.bias"), self.lp(i - 1, "mlp.fc2.bias") if i > 0 else None))
            dh = self.out(st, "dh", r.dx, r.b_dx, rows)
            dhb = self.out(st, "dhb", r.dxm, r.b_dx16, rows)
        self.wg["embedding.weight"] = (dhb[:T], self.patches[:T, :d.pk])
        self.dh0 = dh

    def grads(self):
        tr, d = self.tr, self.d
        D, N, b, T = d.D, d.N, d.b, d.T
        # classifier (f32 operands)
        acc, E = mm(self.dl.t(), self.lncls)
        self.grad("classifier.weight", acc, E + 2.0 ** -23 * acc.abs())
        self.bias_src["classifier.bias"] = self.dl
        for name, (A, B) in self.wg.items():
            rows_k = A.shape[0]
            if self.sim is not None:
                rows_k = self.sim.get("wgrad_rows", {}).get(name, rows_k)
            acc, E = mm(A[:rows_k].t(), B[:rows_k])
            if rows_k != A.shape[0]:
                E = mm(A.t(), B)[1]
            self.grad(name, acc, E + 2.0 ** -23 * acc.abs())
        for name, part in self.bias_src.items():
            x = part.double()
            prior = tr.layout.view(tr.grad_before, name).double().reshape(-1).abs() if tr.accumulate else 0.0
            self.grad(name, x.sum(0), SLACK * (x.shape[0] + 1) * UF * (x.abs().sum(0) + prior))
        # embedding: position table, cls token, conv bias from dh of layer 0 times the position dropout
        mult = self.dm("grad.embed", 0, T, D)
        dpos, dcls, dcb = G.embed_grad(self.dh0[:T], b, N, D, mult)
        mag = (self.dh0[:T].double() * mult).abs().reshape(b, N, D)
        for name, ref, m, n in (("transformer.pos_embedding.pos_embedding", dpos, mag.sum(0), b),
                                ("cls_token", dcls, mag.sum(0)[0], b),
                                ("embedding.bias", dcb, mag.sum(0)[1:].sum(0), b * (N - 1))):
            prior = tr.layout.view(tr.grad_before, name).double().reshape(m.shape).abs() if tr.accumulate else 0.0
            self.grad(name, ref, SLACK * (n + 2) * UF * (m + prior), stage="grad.embed." + name.split(".")[-1])

    def finish(self):
        """unclaimed writes, inputs changed by their launch, and the invariants"""
        tr, d = self.tr, self.d
        for k, ev in enumerate(tr.events):
            for buf in ev.post:
                if buf in ev.writes:
                    if (k, buf) not in self.claimed and ev.fn not in CE:
                        self.problems.append(f"unrecognised write: launch {k} ({ev.fn}) wrote {buf}")
                elif buf in ev.pre and not torch.equal(ev.pre[buf].contiguous().view(torch.uint8),
                                                       ev.post[buf].contiguous().view(torch.uint8)):
                    self.problems.append(f"launch {k} ({ev.fn}) changed its input {buf}")
        if tr.nan_filled:
            gaps = tr.layout.gap_mask(tr.grad_after.device)
            if not bool(tr.grad_after[~gaps].isfinite().all()):
                names = [n for n in tr.layout.offsets if not bool(tr.layout.view(tr.grad_after, n).isfinite().all())]
                self.problems.append(f"gradient elements not written (still NaN): {names[:4]}")
            if not bool(tr.grad_after[gaps].isnan().all()):
                self.problems.append("an alignment gap of the gradient buffer was written")
        for buf, t in tr.pads.items():
            n0 = d.T if dict(PAD_BUFFERS)[re.sub(r"\[\d+\]", "", buf)] else d.b
            if bool((t[n0:].float() != 0).any()):
                self.problems.append(f"rows past the data of {buf} are no longer zero")

    def report(self):
        lines = [f"RATIO {k} {v:.3g}" for k, v in self.ratios.items()]
        lines += [f"FAILED {s}: {'; '.join(self.detail[s])}" for s in self.failed]
        lines += [f"PROBLEM {p}" for p in self.problems]
        return "\n".join(lines)


def audit(tr):
    return Walk(tr).run()


# ---- a simulated step (the CPU self-test) ------------------------------------------------------------------------------
def make_layout(dims):
    """the engine's flat layout (vitmi.engine.flat_param_specs / FlatLayout), restated: 64-element alignment"""
    D, M, H, hd, L, C, N = dims.D, dims.M, dims.H, dims.hd, dims.L, dims.C, dims.N
    specs = [("classifier.weight", (C, D)), ("classifier.bias", (C,)), ("transformer.norm.weight", (D,)),
             ("transformer.norm.bias", (D,))]
    for i in reversed(range(L)):
        p = f"transformer.encoder_layers.{i}."
        specs += [(p + "norm1.weight", (D,)), (p + "norm1.bias", (D,))]
        for w in ("query", "key", "value"):
            specs += [(p + f"attn.{w}.weight", (D, H, hd)), (p + f"attn.{w}.bias", (H, hd))]
        specs += [(p + "attn.out.weight", (H, hd, D)), (p + "attn.out.bias", (D,)), (p + "norm2.weight", (D,)),
                  (p + "norm2.bias", (D,)), (p + "mlp.fc1.weight", (M, D)), (p + "mlp.fc1.bias", (M,)),
                  (p + "mlp.fc2.weight", (D, M)), (p + "mlp.fc2.bias", (D,))]
    specs += [("embedding.weight", (D, 3, *dims.patch_hw)), ("embedding.bias", (D,)),
              ("transformer.pos_embedding.pos_embedding", (1, N, D)), ("cls_token", (1, 1, D))]
    offsets, shapes, off = {}, {}, 0
    for name, shape in specs:
        n = 1
        for s in shape:
            n *= s
        offsets[name], shapes[name] = off, shape
        off = _rup(off + n, 64)
    return Layout(offsets, shapes, off)


def simulate(dims, params, x, labels, p_drop=0.0, path_rate=0.0, seed=1234, offset=1, pruned=True, grad_before=None,
             faults=None):
    """a trace made of the stage references' own values, each rounded once to its storage type. faults: post {stage:
    fn(buffer name, tensor)}, site {stage: dropout-site shift}, path_bwd fn(table) -> the table the backward reads,
    wgrad_rows {parameter: token rows its weight gradient sums}, no_prior (parameters whose accumulation overwrites)"""
    L = dims.L
    path = None
    if path_rate and L > 1:
        path = [float(path_rate) * i / (L - 1) for i in range(L) for _ in range(2)]
    tr = Trace(dims, x, labels, p_drop, path, seed, offset, pruned and not p_drop and not path,
               grad_before is not None)
    tr.layout = make_layout(dims)
    tr.master = {k: v.detach().clone().float().reshape(tr.layout.shapes[k]) for k, v in params.items()}
    tr.mirror = {k: v.bfloat16() for k, v in tr.master.items()}
    tr.grad_before = grad_before
    tr.grad_after = torch.full((tr.layout.numel,), float("nan"))
    tr.nan_filled = grad_before is None
    Walk(tr, sim=faults or {}).run()
    return tr
