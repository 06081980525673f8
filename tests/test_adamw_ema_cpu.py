"""CPU side of the engine's AdamW + EMA step: the float64 reference (adamw_ema_ref.py) against torch.optim.AdamW with
two parameter groups and against timm's EMA rule, the unfused f32 emulation inside the reference's bounds for the cases
the GPU sweep runs, the chunk-table builder on the tiny configuration, the new flags, and the library's exports."""
import json
import math
import os

import pytest
import torch

import adamw_ema_ref as R
import glue_ref as G


# ---- the reference ---------------------------------------------------------------------------------------------------
# hyper-parameters that f32 holds exactly (glue_ref.adamw rounds them as the C ABI does), so torch in float64 gets the
# very same numbers: lr 2^-10, wd 2^-4 (lr wd = 2^-14), beta1 7/8, beta2 1 - 2^-8, eps 2^-27
EXACT = dict(lr=2.0 ** -10, beta1=0.875, beta2=1 - 2.0 ** -8, eps=2.0 ** -27, wd=0.0625)


def test_reference_is_torch_adamw_with_two_groups():
    gen = torch.Generator().manual_seed(1)
    n = 257
    dec = torch.randn(n, generator=gen, dtype=torch.float64).requires_grad_()
    nod = torch.randn(n, generator=gen, dtype=torch.float64).requires_grad_()
    opt = torch.optim.AdamW([dict(params=[dec]), dict(params=[nod], weight_decay=0.0)], lr=EXACT["lr"],
                            betas=(EXACT["beta1"], EXACT["beta2"]), eps=EXACT["eps"], weight_decay=EXACT["wd"])
    mine = {k: dict(p=t.detach().clone(), m=torch.zeros(n, dtype=torch.float64), v=torch.zeros(n, dtype=torch.float64))
            for k, t in (("dec", dec), ("nod", nod))}
    for step in range(1, 4):
        grads = dict(dec=torch.randn(n, generator=gen, dtype=torch.float64),
                     nod=torch.randn(n, generator=gen, dtype=torch.float64))
        dec.grad, nod.grad = grads["dec"].clone(), grads["nod"].clone()
        opt.step()
        step_size = EXACT["lr"] / (1 - EXACT["beta1"] ** step)
        bc2s = math.sqrt(1 - EXACT["beta2"] ** step)
        for k, t in (("dec", dec), ("nod", nod)):
            s = mine[k]
            (s["p"], _, s["m"], s["v"]), _ = R.adamw_ema(s["p"], grads[k], s["m"], s["v"], None, step_size, bc2s, 1.0,
                                                         decayed=k == "dec", **EXACT)
            st = opt.state[t]
            for got, want in ((s["p"], t.detach()), (s["m"], st["exp_avg"]), (s["v"], st["exp_avg_sq"])):
                assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max()), (k, step)
    assert float((mine["dec"]["p"] - mine["nod"]["p"]).abs().max()) > 0     # (the groups do differ)


def test_reference_ema_is_timms_rule():
    gen = torch.Generator().manual_seed(2)
    d = 1.0 - R.omd_of(0.9999)                       # the decay the f32 (1 - d) stands for
    ema = torch.randn(300, generator=gen, dtype=torch.float64)
    timm, ps = ema.clone(), []
    for _ in range(3):
        p = torch.randn(300, generator=gen)
        ps.append(p)
        timm = d * timm + (1 - d) * p.double()       # timm.utils.ModelEmaV2: ema = decay * ema + (1 - decay) * model
    got, bound = R.ema_chain(ps, ema, 0.9999)
    assert float((got - timm).abs().max()) <= 1e-14
    assert float(bound.min()) > 0


@pytest.mark.parametrize("coef", R.COEFS)
@pytest.mark.parametrize("step", [1, 3])
def test_f32_emulation_stays_inside_the_bounds(coef, step):
    """the cases the GPU sweep runs: its layout, its inputs, its table"""
    starts, total, chunks, decayed = R.sweep_layout()
    table = R.sweep_table(step, coef)
    worst = 0.0
    for s, seg in enumerate(R.sweep_inputs()):
        args = (seg["p"], seg["g"], seg["m"], seg["v"], seg["ema"], float(table[0]), float(table[1]), float(table[3]))
        refs, bounds = R.adamw_ema(*args, decayed=decayed[s])
        for name, got, ref, bound in zip(("p", "g", "m", "v", "ema"), R.adamw_ema_emulate(*args, decayed=decayed[s]),
                                         refs, bounds):
            ratio, at = G.worst(got, ref, bound)
            assert ratio <= 1.0, (name, s, at, ratio)
            worst = max(worst, ratio)
    print(f"RATIO adamw_ema_emulate[coef={coef},step={step}] {worst:.4g}")
    assert worst > 0.01                               # the bounds are not vacuous


def test_axpby_ema_reference_is_timms_rule_and_bounds_its_emulation():
    gen = torch.Generator().manual_seed(3)
    p, ema = torch.randn(4096, generator=gen), torch.randn(4096, generator=gen)
    ref, bound = R.ema_axpby(p, ema, 0.99)
    a, b = G.f32(1 - 0.99), G.f32(0.99)
    assert float((ref - (b * ema.double() + a * p.double())).abs().max()) == 0
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    assert G.worst(t(a) * p + t(b) * ema, ref, bound)[0] <= 1.0


# ---- the chunk table -------------------------------------------------------------------------------------------------
def _tiny_layout(golden_dir):
    from vitmi.engine import ArchConfig, FlatLayout
    with open(os.path.join(golden_dir, "ctor_tiny.json")) as f:
        shapes = {k: tuple(v["shape"]) for k, v in json.load(f).items()}
    lay = FlatLayout(ArchConfig(image_size=32, patch_size=8, emb_dim=64, mlp_dim=128, num_heads=2, num_layers=2,
                                num_classes=10))
    assert {k: tuple(v) for k, v in lay.shapes.items()} == shapes          # the fixture's model
    return lay


# by hand, from the constructor fixture's names: per layer 2 LayerNorms x (weight, bias), q/k/v/out/fc1/fc2 biases
TINY_UNDECAYED = sorted(
    [f"transformer.encoder_layers.{i}.{s}" for i in range(2)
     for s in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "attn.query.bias", "attn.key.bias",
               "attn.value.bias", "attn.out.bias", "mlp.fc1.bias", "mlp.fc2.bias")] +
    ["transformer.norm.weight", "transformer.norm.bias", "classifier.bias", "embedding.bias",
     "transformer.pos_embedding.pos_embedding", "cls_token"])


@pytest.mark.parametrize("chunk", [8192, 1024])
def test_chunk_table_of_the_tiny_model(golden_dir, chunk):
    from vitmi.optim import ADAMW_CHUNK, adamw_chunk_table, no_decay_names
    assert ADAMW_CHUNK == 8192
    lay = _tiny_layout(golden_dir)
    assert sorted(no_decay_names(lay)) == TINY_UNDECAYED
    table = adamw_chunk_table(lay, chunk=chunk)
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 3 and not table.is_cuda
    flags, start, length = table.unbind(1)
    assert set(flags.tolist()) == {0, 1}
    assert int(length.min()) >= 1 and int(length.max()) <= chunk
    assert bool((start % 4 == 0).all())
    hits = torch.zeros(lay.numel, dtype=torch.int64)
    flag_of = torch.full((lay.numel,), -1, dtype=torch.int64)
    for f, s, n in table.tolist():
        assert 0 <= s and s + n <= lay.numel
        hits[s:s + n] += 1
        flag_of[s:s + n] = f
    assert int(hits.max()) == 1                                              # nothing twice
    for name, off in lay.offsets.items():
        n = math.prod(lay.shapes[name])
        assert bool((hits[off:off + n] == 1).all()), name                    # every parameter element once
        want = 0 if name in TINY_UNDECAYED else 1
        assert bool((flag_of[off:off + n] == want).all()), name              # and no chunk across a decay boundary
    all_ = adamw_chunk_table(lay, decay_all=True, chunk=chunk)
    assert bool((all_[:, 0] == 1).all()) and int(all_[:, 2].sum()) == lay.numel
    assert int(all_[:, 2].max()) <= chunk


# ---- flags -----------------------------------------------------------------------------------------------------------
BASE = ["--no-save", "--synthetic"]


def test_defaults_keep_sgd_and_no_ema(capsys):
    from vitmi.config import get_train_config
    c = get_train_config(BASE)
    assert c.optimizer == "sgd" and c.ema_decay == 0.0 and c.lr_schedule == "onecycle" and not c.decay_all
    assert (c.beta1, c.beta2, c.adam_eps) == (0.9, 0.999, 1e-8)
    c = get_train_config(BASE + ["--optimizer", "adamw", "--ema-decay", "0.9999"])
    assert c.optimizer == "adamw" and c.lr_schedule == "cosine" and c.ema_decay == 0.9999
    assert get_train_config(BASE + ["--lr-schedule", "cosine"]).lr_schedule == "cosine"          # sgd may take it
    capsys.readouterr()


@pytest.mark.parametrize("args", [["--optimizer", "adamw", "--lr-schedule", "onecycle"], ["--ema-decay", "1"],
                                  ["--ema-decay", "-0.1"], ["--ema-decay", "nan"]])
def test_bad_optimizer_flags_exit_with_one_line(args, capsys):
    from vitmi.config import get_train_config
    with pytest.raises(SystemExit) as e:
        get_train_config(BASE + args)
    assert isinstance(e.value.code, str) and "\n" not in e.value.code and args[0] in e.value.code
    capsys.readouterr()


def test_use_ema_names_a_checkpoint_without_the_key(tmp_path, capsys):
    from vitmi import eval as veval
    from vitmi.checkpoint import EMA_KEY, load_checkpoint, load_checkpoint_ema
    plain, with_ema = str(tmp_path / "plain.pth"), str(tmp_path / "ema.pth")
    torch.save({"state_dict": {"w": torch.zeros(2)}}, plain)
    torch.save({"state_dict": {"w": torch.zeros(2)}, EMA_KEY: {"w": torch.ones(2)}}, with_ema)
    assert float(load_checkpoint_ema(with_ema)["w"].sum()) == 2.0
    assert float(load_checkpoint(with_ema)["w"].sum()) == 0.0                 # the default still reads state_dict
    with pytest.raises(SystemExit) as e:
        veval.main(["--synthetic", "--use-ema", "--checkpoint-path", plain])
    assert isinstance(e.value.code, str) and "\n" not in e.value.code and plain in e.value.code
    assert EMA_KEY in e.value.code
    capsys.readouterr()


# ---- exports ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_and_the_abi_numbers_agree():
    """(the number itself stays 24: the entry is an addition, nothing that existed changed its meaning, and the
    build id already refuses a library built from other sources)"""
    from vitmi import _lib
    lib = _lib.load()
    assert lib.vit_abi_version() == _lib.ABI_VERSION
    assert "vit_adamw_ema_update" in _lib._SIGS
    assert hasattr(lib, "vit_adamw_ema_update") and lib.vit_adamw_chunk_elems() == 8192
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "vit_hip.h")).read()
    assert "int vit_adamw_ema_update(" in header
