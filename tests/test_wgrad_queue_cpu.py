"""The engine's weight-gradient queue (vitmi.engine._WgradQueue): which launch form every gradient of a backward goes
to, in which order, per mode. The three launch forms are replaced by recorders and a backward's pushes are replayed
as ViTEngine.backward issues them, so no library and no GPU is needed. D = 256, MLP 512, three layers."""
from types import SimpleNamespace

import pytest

from vitmi import wgrad
from vitmi.engine import _WgradQueue
from vitmi.wgrad import Spec

D, M, L, TP, BP = 256, 512, 3, 192, 64
FC2, FC1, OUT, QKV = (D, M), (M, D), (D, D), (D, D, 3)


def spec(M_, N_, batch=1):
    return Spec(None, 0, None, 0, M_, N_, None, N_, batch=batch)


@pytest.fixture
def log(monkeypatch):
    """launches as (form, K, [(M, N) or (M, N, batch), ...]) and done callbacks as ("done", name), in issue order"""
    out = []

    def shapes(specs):
        return [(sp.M, sp.N) if sp.batch == 1 else (sp.M, sp.N, sp.batch) for sp in specs]

    monkeypatch.setattr(wgrad, "single", lambda sp, K, **kw: out.append(("single", K, shapes([sp]))))
    monkeypatch.setattr(wgrad, "group", lambda sps, K, common, **kw: out.append(("group", K, shapes(sps))) or
                        (common is True or pytest.fail("the engine's group launch runs at the common split")))
    monkeypatch.setattr(wgrad, "table", lambda sps, K, tables, slot, **kw: out.append(("table", K, shapes(sps), slot)))
    return out


def replay(log, defer, group, patch_k, pruned=False):
    """the pushes of ViTEngine.backward for L layers and the patch embedding (N = patch_k)"""
    eng = SimpleNamespace(_workspace=None, probe_wgrad=None, _wgrad_tables={}, _last_b=8)
    wq = _WgradQueue(eng, TP, lambda fn: fn(), defer, group)
    done = lambda name: (lambda: log.append(("done", name)))
    for i in reversed(range(L)):
        if pruned and i == L - 1:
            for shape in (FC2, FC1, OUT):
                wq.single(spec(*shape), K=BP)
        else:
            wq.push(spec(*FC2), done=done(f"fc2.{i}"))
            wq.push(spec(*FC1), done=done(f"fc1.{i}"))
            wq.push(spec(*OUT), done=done(f"out.{i}"), hold=True)
        wq.push(spec(*QKV), done=done(f"qkv.{i}"))
        wq.end_layer(i)
    wq.push(spec(D, patch_k))
    wq.finish()
    return [e for e in log if e[0] != "done"], log


LAYER = [FC2, FC1, OUT, QKV]


@pytest.mark.parametrize("patch_k", [192, 768])
def test_single_mode_launches_every_spec_at_once(log, patch_k):
    launches, events = replay(log, 0, False, patch_k)
    assert launches == [("single", TP, [s]) for s in LAYER * L + [(D, patch_k)]]
    # each release right after its own launch
    assert events[:4] == [("single", TP, [FC2]), ("done", "fc2.2"), ("single", TP, [FC1]), ("done", "fc1.2")]


@pytest.mark.parametrize("patch_k", [192, 768])
def test_group_mode_pairs_the_out_projection_with_qkv(log, patch_k):
    launches, events = replay(log, 0, True, patch_k)
    layer = [("single", TP, [FC2]), ("single", TP, [FC1]), ("group", TP, [OUT, QKV])]
    assert launches == layer * L + [("single", TP, [(D, patch_k)])]
    i = events.index(("group", TP, [OUT, QKV]))
    assert ("done", "out.2") not in events[:i] and set(events[i + 1:i + 3]) == {("done", "out.2"), ("done", "qkv.2")}


def test_group_mode_pruned_last_layer_runs_qkv_alone(log):
    launches, _ = replay(log, 0, True, 768, pruned=True)
    assert launches[:4] == [("single", BP, [FC2]), ("single", BP, [FC1]), ("single", BP, [OUT]), ("single", TP, [QKV])]
    assert launches[4:7] == [("single", TP, [FC2]), ("single", TP, [FC1]), ("group", TP, [OUT, QKV])]


@pytest.mark.parametrize("group", [False, True])
def test_deferred_all_is_one_table_launch_after_the_last_push(log, group):
    launches, events = replay(log, L, group, 768)
    assert launches == [("table", TP, LAYER * L + [(D, 768)], (8, 0))]
    assert events[0][0] == "table" and len(events) == 1 + 4 * L  # every release after the launch


@pytest.mark.parametrize("group", [False, True])
@pytest.mark.parametrize("defer", [1, 2, L])
def test_deferred_keeps_a_sub_256_spec_on_the_single_form(log, group, defer):
    """the 192-column patch-embedding gradient is not a table member: its own launch, before the last table launch,
    whatever group_wgrad says"""
    launches, _ = replay(log, defer, group, 192)
    per = {1: [1, 1, 1], 2: [2, 1], L: [L]}[defer]
    tables = [("table", TP, LAYER * n, (8, k)) for k, n in enumerate(per)]
    assert launches == tables[:-1] + [("single", TP, [(D, 192)]), tables[-1]]


@pytest.mark.parametrize("group", [False, True])
def test_deferred_pruned_last_layer(log, group):
    """the cls-row gradients run at once at their own K; the layer still counts towards `defer`"""
    launches, _ = replay(log, 1, group, 768, pruned=True)
    assert launches == [("single", BP, [FC2]), ("single", BP, [FC1]), ("single", BP, [OUT]),
                        ("table", TP, [QKV], (8, 0)), ("table", TP, LAYER, (8, 1)),
                        ("table", TP, LAYER + [(D, 768)], (8, 2))]
