"""The engine's AdamW + EMA step on the GPU: vit_adamw_ema_update gated per element against adamw_ema_ref.py's float64
reference, vitmi.optim.EngineAdamW against torch.optim.AdamW on a small ViT's own gradients, the weight EMA and
VisionTransformer.swapped_weights, the state-dict round trip, and vitmi.train / vitmi.eval end to end.

Bounded gates print their worst ratio ("RATIO name value", visible with pytest -s)."""
import functools
import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

import adamw_ema_ref as R
import glue_ref as G
from oracle.vit_oracle import init_params, tame_params
from test_parity_gpu import SMALL, TINY, make_model, rel

DEV = "cuda"
BF16 = torch.bfloat16
GUARD = 8
NAMES = ("p", "g", "m", "v", "ema")
STEP = 3


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------
def _sweep_buffers():
    """flat f32 {p, g, m, v, ema} with the sweep's inputs, zero alignment padding and a NaN guard behind; the mirror
    holds 7 everywhere the kernel must not write"""
    starts, total, chunks, decayed = R.sweep_layout()
    segs = R.sweep_inputs()
    flat = {}
    for name in NAMES:
        buf = torch.zeros(total + GUARD)
        buf[total:] = G.NAN
        for at, seg in zip(starts, segs):
            buf[at:at + seg[name].numel()] = seg[name]
        flat[name] = buf.to(DEV)
    mirror = torch.full((total + GUARD,), 7.0, dtype=BF16, device=DEV)
    return starts, total, chunks.pin_memory(), decayed, segs, flat, mirror


def _update(flat, mirror, chunks, table, ema, write_grad, ema_buf=None):
    from vitmi import ops
    h = R.HYPER
    ops.adamw_ema_update(flat["p"], flat["g"], flat["m"], flat["v"], mirror,
                         (flat["ema"] if ema_buf is None else ema_buf) if ema else None, chunks, table.to(DEV), h["lr"],
                         h["beta1"], h["beta2"], h["eps"], h["wd"], R.EMA_DECAY if ema else None, write_grad)
    torch.cuda.synchronize()


@pytest.mark.parametrize("write_grad", [0, 1])
@pytest.mark.parametrize("mirror", [True, False])
@pytest.mark.parametrize("ema", [True, False])
def test_kernel_sweep(ema, mirror, write_grad):
    from vitmi import ops
    assert ops.adamw_chunk_elems() == 8192
    fails, worst = [], 0.0
    for coef in R.COEFS:
        starts, total, chunks, decayed, segs, flat, mflat = _sweep_buffers()
        before = {name: flat[name].clone() for name in NAMES}
        table = R.sweep_table(STEP, coef)
        _update(flat, mflat if mirror else None, chunks, table, ema, write_grad)
        inside = torch.zeros(total + GUARD, dtype=torch.bool, device=DEV)
        for s, (at, seg) in enumerate(zip(starts, segs)):
            n = seg["p"].numel()
            inside[at:at + n] = True
            tag = f" [coef {coef} segment {s} length {n} decayed {decayed[s]}]"
            # (an undecayed chunk: the reference with decay = 1)
            refs, bounds = R.adamw_ema(seg["p"], seg["g"], seg["m"], seg["v"], seg["ema"] if ema else None,
                                       float(table[0]), float(table[1]), float(table[3]), decayed=decayed[s])
            for name, ref, bound in zip(NAMES, refs, bounds):
                got = flat[name][at:at + n]
                if name == "g" and not write_grad:
                    d = G.first_diff(got, seg["g"].to(DEV), bits=True)
                    if d is not None:
                        fails.append(f"g{tag}: rewritten at {d[0]}")
                    continue
                ratio, where = G.worst(got, ref.to(DEV), bound.to(DEV))
                worst = max(worst, ratio)
                if not ratio <= 1.0:
                    fails.append(f"{name}{tag}: {ratio:.3g} x gate at {where}")
            want_m = flat["p"][at:at + n].bfloat16() if mirror else torch.full((n,), 7.0, dtype=BF16, device=DEV)
            d = G.first_diff(mflat[at:at + n], want_m, bits=True)       # RNE of the kernel's own p'
            if d is not None:
                fails.append(f"mirror{tag}: at {d[0]} got {d[1]!r}, want {d[2]!r}")
        for name in NAMES:   # alignment padding stays zero, the guard NaN; without an EMA its buffer keeps every bit
            keep = ~inside if (ema or name != "ema") else torch.ones_like(inside)
            d = G.first_diff(torch.where(keep, flat[name], before[name]), before[name], bits=True)
            if d is not None:
                fails.append(f"{name} [coef {coef}]: element {d[0]} outside the chunks changed to {d[1]!r}")
        d = G.first_diff(mflat[~inside], torch.full_like(mflat[~inside], 7.0), bits=True)
        if d is not None:
            fails.append(f"mirror [coef {coef}]: element outside the chunks written")
    print(f"RATIO adamw_ema_update[ema={ema},mirror={mirror},write_grad={write_grad}] {worst:.4g}")
    assert not fails, fails[:8]


def test_kernel_takes_padding_inside_a_chunk_and_keeps_it_zero():
    """the engine's chunks run over the alignment padding: one decayed chunk over segments 3 and 4 (lengths 4 and 5,
    64-aligned) and everything between and behind them"""
    starts, total, _, _, segs, flat, mflat = _sweep_buffers()
    at, end = starts[3], starts[5]
    chunks = torch.tensor([[1, at, end - at]], dtype=torch.int64).pin_memory()
    table = R.sweep_table(STEP, 0.37)
    _update(flat, mflat, chunks, table, True, 1)
    pad = torch.ones(end - at, dtype=torch.bool, device=DEV)
    for s in (3, 4):
        n = segs[s]["p"].numel()
        pad[starts[s] - at:starts[s] - at + n] = False
        refs, bounds = R.adamw_ema(*(segs[s][k] for k in NAMES), float(table[0]), float(table[1]), float(table[3]),
                                   decayed=True)
        for name, ref, bound in zip(NAMES, refs, bounds):
            assert G.worst(flat[name][starts[s]:starts[s] + n], ref.to(DEV), bound.to(DEV))[0] <= 1.0, (name, s)
    for name in NAMES:
        assert float(flat[name][at:end][pad].abs().max()) == 0.0, name
    assert float(mflat[at:end][pad].float().abs().max()) == 0.0


def test_kernel_refuses_bad_flags_a_misaligned_ema_and_unpinned_chunks():
    from vitmi import _lib
    starts, total, chunks, _, _, flat, mflat = _sweep_buffers()
    table = R.sweep_table(STEP, 1.0)
    before = {name: flat[name].clone() for name in NAMES}
    bad = chunks.clone()
    bad[5, 0] = 3                                                   # bit 1 set on one chunk in the middle
    with pytest.raises(_lib.VitHipError, match="flags"):
        _update(flat, mflat, bad.pin_memory(), table, True, 1)
    with pytest.raises(_lib.VitHipError, match="16-B aligned"):
        _update(flat, mflat, chunks, table, True, 1, ema_buf=flat["ema"][1:])
    with pytest.raises(ValueError, match="pinned"):
        _update(flat, mflat, torch.tensor(chunks.tolist()), table, True, 1)
    torch.cuda.synchronize()
    for name in NAMES:                                              # nothing was launched: every bit as it was
        assert G.first_diff(flat[name], before[name], bits=True) is None, name
    assert G.first_diff(mflat, torch.full_like(mflat, 7.0), bits=True) is None


# ---- 2.-4. the optimizer on a small ViT ------------------------------------------------------------------------------
BS = 4
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)


CFGS = {"tiny": TINY, "small": SMALL}


@functools.lru_cache(maxsize=None)
def problem(which):
    """tamed parameters and one batch of the named configuration: computed once, never written"""
    cfg = CFGS[which]
    params = tame_params(init_params(cfg, seed=42))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(BS, 3, cfg.image_size, cfg.image_size, generator=g)
    y = torch.randint(0, cfg.num_classes, (BS,), generator=g)
    return params, x.cuda(), y.cuda()


def backward(m, opt, which):
    """one real backward of the engine: .grad become views of its flat gradient"""
    from vitmi.model import CrossEntropyLoss
    _, x, y = problem(which)
    opt.zero_grad()
    loss = CrossEntropyLoss()(m(x), y)
    loss.backward()
    return float(loss.detach())


def torch_twin(m, decay_all=False):
    """torch.optim.AdamW over CPU copies of the model's parameters in the groups EngineAdamW.state_dict() names"""
    from vitmi.optim import no_decay_names
    skip = set() if decay_all else set(no_decay_names(m.engine().layout))
    cpu = {n: p.detach().cpu().clone().requires_grad_() for n, p in m.named_parameters()}
    groups = [dict(params=[t for n, t in cpu.items() if n not in skip])]
    if skip:
        groups.append(dict(params=[t for n, t in cpu.items() if n in skip], weight_decay=0.0))
    return cpu, torch.optim.AdamW(groups, **HP)


def feed(m, cpu):
    for n, p in m.named_parameters():
        cpu[n].grad = p.grad.detach().cpu().clone()


def mirror_is_a_full_refresh(eng):
    got = [t.clone() for t in (eng.mirror, eng.wqkv, eng.bqkv, eng.wconv) if t is not None]
    eng.refresh_mirror(full=True)
    want = [t for t in (eng.mirror, eng.wqkv, eng.bqkv, eng.wconv) if t is not None]
    return all(G.first_diff(a, b, bits=True) is None for a, b in zip(got, want))


def agree(m, opt, cpu, topt, tol=1e-5):
    bad = []
    for n, p in m.named_parameters():
        st, tst = opt.state[p], topt.state[cpu[n]]
        for what, a, b in (("p", p, cpu[n]), ("exp_avg", st["exp_avg"], tst["exp_avg"]),
                           ("exp_avg_sq", st["exp_avg_sq"], tst["exp_avg_sq"])):
            if rel(a, b.detach()) > tol:
                bad.append((n, what, rel(a, b.detach())))
        assert float(st["step"]) == float(tst["step"])
    return bad


@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip1"])
@pytest.mark.parametrize("cfg", ["tiny", "small"])
def test_engine_adamw_matches_torch_adamw(cfg, clip):
    """tiny: the ctor_tiny.json model; small: 4-px patches, so the padded conv operand (wconv) exists"""
    from vitmi.optim import EngineAdamW
    m = make_model(CFGS[cfg], problem(cfg)[0])
    opt = EngineAdamW(m.parameters(), model=m, max_grad_norm=clip, **HP)
    eng = m.engine()
    assert (eng.wconv is not None) == (cfg == "small")
    cpu, topt = torch_twin(m)
    for step in range(3):
        backward(m, opt, cfg)
        feed(m, cpu)
        if clip is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(list(cpu.values()), clip))
        opt.step()
        topt.step()
        torch.cuda.synchronize()
        if clip is not None:
            got = opt.last_norm.cpu()
            print(f"step {step}: norm {norm:.6g} coef {float(got[1]):.6g}")
            assert abs(float(got[0]) - norm) <= 1e-5 * norm
            for n, p in m.named_parameters():                       # .grad is left clipped
                assert rel(p.grad, cpu[n].grad) <= 1e-5, n
        assert mirror_is_a_full_refresh(eng), step
        assert not agree(m, opt, cpu, topt), step
    # the groups did their work: an undecayed and a decayed parameter both moved, by different rules
    assert float(opt.steps[0]) == 3.0


def test_engine_adamw_needs_the_flat_engine():
    from vitmi.optim import EngineAdamW
    m = make_model(TINY, problem("tiny")[0])
    with pytest.raises(NotImplementedError, match="model="):
        EngineAdamW(m.parameters(), **HP)
    with pytest.raises(NotImplementedError, match="flat"):
        EngineAdamW(list(m.parameters())[:-1], model=m, **HP)
    opt = EngineAdamW(m.parameters(), model=m, **HP)
    with pytest.raises(NotImplementedError, match="flat"):          # no backward yet: .grad is not the flat gradient
        opt.step()


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_ema_and_swapped_weights(kind):
    from vitmi.optim import SGD, EngineAdamW
    cfg, d = "tiny", 0.9
    m = make_model(TINY, problem(cfg)[0])
    if kind == "adamw":
        opt = EngineAdamW(m.parameters(), model=m, ema_decay=d, **HP)
    else:
        m(problem(cfg)[1])
        opt = SGD(m.parameters(), lr=0.03, momentum=0.9, weight_decay=1e-4, model=m, ema_decay=d)
    eng = m.engine()
    ema0, ps = eng.flat.detach().cpu().clone(), []
    assert G.first_diff(opt.ema.cpu(), ema0, bits=True) is None     # a copy of the weights at construction
    for _ in range(3):
        backward(m, opt, cfg)
        opt.step()
        ps.append(eng.flat.detach().cpu().clone())
    ref, bound = (R.ema_chain if kind == "adamw" else R.ema_axpby_chain)(ps, ema0, d)
    sd = opt.ema_state_dict()
    assert list(sd.keys()) == list(m.state_dict().keys())
    worst = 0.0
    for name, t in sd.items():
        off, n = eng.layout.offsets[name], t.numel()
        assert t.shape == m.state_dict()[name].shape
        ratio, at = G.worst(t.cpu().reshape(-1), ref[off:off + n], bound[off:off + n])
        assert ratio <= 1.0, (name, at, ratio)
        worst = max(worst, ratio)
    print(f"RATIO ema_chain[{kind}] {worst:.4g}")
    assert float((opt.ema.cpu() - ps[-1]).abs().max()) > 0          # (it is not the weights)
    # the swap: same engine, same activations, bit-equal logits
    x = problem(cfg)[1]
    m.eval()
    with torch.no_grad():
        before = m(x).clone()
        acts = dict(eng._acts)
        with m.swapped_weights(opt.ema) as sm:
            assert sm is m and m.engine() is eng and eng.flat.data_ptr() == opt.ema.data_ptr()
            inside = m(x).clone()
        after = m(x).clone()
        assert eng.flat.data_ptr() != opt.ema.data_ptr() and m._bound()
        assert all(eng._acts[k] is v for k, v in acts.items())
        fresh = make_model(TINY, sd).eval()
        want = fresh(x).clone()
    assert G.first_diff(inside, want, bits=True) is None
    assert G.first_diff(after, before, bits=True) is None
    assert G.first_diff(inside, before, bits=True) is not None
    # ... and training goes on from the trained weights
    m.train()
    backward(m, opt, cfg)
    opt.step()


def _recorded_step(monkeypatch, opt):
    """the names of the vitmi.ops functions one opt.step() calls, in order"""
    import types
    from vitmi import ops
    calls = []
    for name, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_") and \
                name != "lib":
            def wrapper(*a, _fn=fn, _name=name, **k):
                calls.append(_name)
                return _fn(*a, **k)
            monkeypatch.setattr(ops, name, wrapper)
    opt.step()
    monkeypatch.undo()
    return calls


PARENT_SGD_STEP = ["sgd_step", "pack_cols_batched", "pack_cols_batched"]
PARENT_SGD_CLIP = ["sqnorm_partial", "adamw_prep", "scale_by_coef"] + PARENT_SGD_STEP


@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip1"])
def test_sgd_without_ema_calls_what_it_called(monkeypatch, clip):
    """the sequences are vitmi.optim.SGD.step's fast path as it was before ema_decay existed (TINY has no wconv)"""
    from vitmi.optim import SGD, EngineAdamW
    cfg = "tiny"
    m = make_model(TINY, problem(cfg)[0])
    m(problem(cfg)[1])
    opt = SGD(m.parameters(), lr=0.03, momentum=0.9, model=m, max_grad_norm=clip)
    assert opt.ema is None
    backward(m, opt, cfg)
    assert _recorded_step(monkeypatch, opt) == (PARENT_SGD_STEP if clip is None else PARENT_SGD_CLIP)
    opt = SGD(m.parameters(), lr=0.03, momentum=0.9, model=m, max_grad_norm=clip, ema_decay=0.9)
    backward(m, opt, cfg)
    want = PARENT_SGD_STEP[:1] + ["axpby"] + PARENT_SGD_STEP[1:]
    assert _recorded_step(monkeypatch, opt) == (want if clip is None else PARENT_SGD_CLIP[:3] + want)
    opt = EngineAdamW(m.parameters(), model=m, max_grad_norm=clip, ema_decay=0.9, **HP)
    backward(m, opt, cfg)
    want = ["adamw_prep", "adamw_ema_update", "pack_cols_batched", "pack_cols_batched"]   # one update launch
    assert _recorded_step(monkeypatch, opt) == (want if clip is None else ["sqnorm_partial"] + want)


@pytest.mark.parametrize("decay_all", [False, True], ids=["groups", "decay_all"])
def test_state_dict_round_trip_through_torch_adamw(decay_all):
    from vitmi.optim import EngineAdamW
    cfg = "tiny"
    m = make_model(TINY, problem(cfg)[0])
    opt = EngineAdamW(m.parameters(), model=m, decay_all=decay_all, **HP)
    assert opt.state_dict()["state"] == {}                          # torch's: no state before the first step
    for _ in range(2):
        backward(m, opt, cfg)
        opt.step()
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == (1 if decay_all else 2)
    cpu, topt = torch_twin(m, decay_all)                            # the weights as they are now
    topt.load_state_dict(sd)
    assert [g["weight_decay"] for g in topt.param_groups] == ([0.05] if decay_all else [0.05, 0.0])
    # back: into a new optimizer over a model with the same weights
    m2 = make_model(TINY, {k: v.detach().cpu() for k, v in m.state_dict().items()})
    opt2 = EngineAdamW(m2.parameters(), model=m2, decay_all=decay_all, lr=1.0, weight_decay=0.5)
    opt2.load_state_dict(topt.state_dict())
    assert opt2.param_groups[0]["lr"] == HP["lr"] and opt2.param_groups[0]["weight_decay"] == HP["weight_decay"]
    assert float(opt2.steps[0]) == 2.0
    assert G.first_diff(opt2.exp_avg, opt.exp_avg, bits=True) is None
    assert G.first_diff(opt2.exp_avg_sq, opt.exp_avg_sq, bits=True) is None
    # one more step on both sides
    backward(m2, opt2, cfg)
    feed(m2, cpu)
    opt2.step()
    topt.step()
    assert not agree(m2, opt2, cpu, topt)
    with pytest.raises(ValueError, match="groups"):
        opt2.load_state_dict({"state": {}, "param_groups": [dict(params=[0])]})


# ---- 5. end to end ---------------------------------------------------------------------------------------------------
def test_train_adamw_ema_end_to_end_and_eval_use_ema(tmp_path, monkeypatch, capsys):
    from vitmi import eval as veval
    from vitmi import train
    from vitmi.engine import ArchConfig, FlatLayout
    from vitmi.optim import no_decay_names
    monkeypatch.chdir(tmp_path)
    train.main(["--synthetic", "--model-arch", "b16", "--any-image-size", "--image-size", "32", "--batch-size", "8",
                "--steps-per-epoch", "2", "--train-steps", "4", "--optimizer", "adamw", "--wd", "0.05", "--ema-decay",
                "0.9", "--accum-steps", "2", "--clip-grad-norm", "1", "--checkpoint-path", ""])
    out = capsys.readouterr().out
    logged = {k: [float(v) for v in re.findall(rf"^\s+{k}\s*: (\S+)$", out, re.M)]
              for k in ("loss", "val_loss", "val_ema_loss", "val_ema_acc1", "val_ema_acc5")}
    assert all(len(v) == 4 for v in logged.values()), logged        # 4 epochs of one optimizer step each
    assert all(math.isfinite(x) for v in logged.values() for x in v), logged
    paths = list(tmp_path.glob("experiments/save/*/checkpoints/current.pth"))
    assert len(paths) == 1
    ckpt = torch.load(str(paths[0]), map_location="cpu", weights_only=True)
    assert ckpt["state_dict_ema"].keys() == ckpt["state_dict"].keys()
    assert any(float((ckpt["state_dict_ema"][k] - ckpt["state_dict"][k]).abs().max()) > 0 for k in ckpt["state_dict"])
    # the optimizer state loads into torch's AdamW over the same two groups
    skip = set(no_decay_names(FlatLayout(ArchConfig(image_size=32, num_classes=100))))
    shapes = {k: v.shape for k, v in ckpt["state_dict"].items()}
    order = [k for k in shapes if k not in skip] + [k for k in shapes if k in skip]
    sizes = [len(g["params"]) for g in ckpt["optimizer"]["param_groups"]]
    assert sizes == [len(shapes) - len(skip), len(skip)]
    zeros = [torch.zeros(shapes[k]) for k in order]
    topt = torch.optim.AdamW([dict(params=zeros[:sizes[0]]), dict(params=zeros[sizes[0]:], weight_decay=0.0)])
    topt.load_state_dict(ckpt["optimizer"])
    assert float(topt.state[zeros[0]]["step"]) == 4.0 and topt.param_groups[0]["weight_decay"] == 0.05
    del ckpt, topt, zeros
    # vitmi.eval --use-ema: the run's validation split (its loader's batch, seed and length), the EMA weights
    acc1, acc5 = veval.main(["--synthetic", "--model-arch", "b16", "--any-image-size", "--image-size", "32",
                             "--batch-size", "4", "--steps-per-epoch", "1", "--seed", "10042", "--num-classes", "100",
                             "--use-ema", "--checkpoint-path", str(paths[0])])
    capsys.readouterr()
    assert acc1 == pytest.approx(logged["val_ema_acc1"][-1], abs=1e-6)
    assert acc5 == pytest.approx(logged["val_ema_acc5"][-1], abs=1e-6)
