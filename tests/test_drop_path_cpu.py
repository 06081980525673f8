"""Stochastic depth (drop-path), the parts that need no GPU: the C ABI additions, the constructor keyword, the linear
depth rule and the --drop-path-rate flag."""
import ctypes
import os
import re

import pytest
import torch

from vitmi import _lib
from vitmi.model import Encoder, VisionTransformer, drop_path_rates

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vit_drop_path_scales", "vit_gemm_bf16_drop_path", "vit_layernorm_bwd_drop_path", "vit_row_scale_f32")


def test_abi_additions_only():
    assert _lib.ABI_VERSION == 24
    header = open(os.path.join(REPO, "include", "vit_hip.h")).read()
    assert re.search(r"typedef struct vit_drop_path \{\s*const float\* scale;[^}]*int64_t rows_per_sample;[^}]*\} vit_drop_path;",
                     header)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib._SIGS, name
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
    assert lib.vit_abi_version() == 24
    # struct vit_drop_path: a pointer and an int64
    assert ctypes.sizeof(_lib.DropPath) == 16 and [f[0] for f in _lib.DropPath._fields_] == ["scale", "rows_per_sample"]


KW = dict(image_size=(32, 32), patch_size=(8, 8), emb_dim=64, mlp_dim=128, num_heads=2, num_layers=3, num_classes=10)


def test_no_new_parameters_and_the_same_initial_tensors():
    torch.manual_seed(42)
    a = VisionTransformer(**KW)
    torch.manual_seed(42)
    b = VisionTransformer(**KW, drop_path_rate=0.2)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert b.drop_path_rate == 0.2 and a.drop_path_rate == 0.0
    assert [n for n, _ in b.named_buffers()] == [n for n, _ in a.named_buffers()]


@pytest.mark.parametrize("L", [1, 2, 12])
def test_linear_depth_rule(L):
    r = 0.3
    want = torch.linspace(0, r, L) if L > 1 else torch.zeros(1)
    assert torch.allclose(torch.tensor(drop_path_rates(r, L)), want, rtol=0, atol=1e-7)
    enc = Encoder(num_patches=16, emb_dim=64, mlp_dim=128, num_layers=L, num_heads=2, dropout_rate=0.0,
                  drop_path_rate=r)
    got = [blk.drop_path_rate for blk in enc.encoder_layers]
    assert torch.allclose(torch.tensor(got), want, rtol=0, atol=1e-7)
    assert got[0] == 0.0


def test_rate_out_of_range_is_refused():
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            VisionTransformer(**KW, drop_path_rate=bad)


BASE = ["--synthetic", "--no-save", "--model-arch", "b16", "--batch-size", "8"]


def _config(extra):
    from vitmi.config import get_train_config
    return get_train_config(BASE + extra)


def test_flag_parses_and_defaults_to_zero(capsys):
    assert _config([]).drop_path_rate == 0.0
    assert _config(["--drop-path-rate", "0.1"]).drop_path_rate == 0.1
    assert "drop_path_rate" in capsys.readouterr().out  # printed with the run's configuration


@pytest.mark.parametrize("bad", ["1.0", "-0.1"])
def test_flag_rejects_out_of_range(bad):
    with pytest.raises(SystemExit) as e:
        _config(["--drop-path-rate", bad])
    assert "--drop-path-rate" in str(e.value)


def test_resvit_train_has_no_flag():
    from vitmi.resvit_train import get_train_config
    with pytest.raises(SystemExit):
        get_train_config(["--drop-path-rate", "0.1"])
