"""Engine option dw_pipe (the fused data + weight gradient's pipelined window loop,
conv_dw.hip PIPE): on by default, and the headline plan with it off or on differs in
nothing but the fused launches' fw_pipe field (no GPU: dry-run plans)."""

from unet_distributed_amd.runtime import native_engine as ne
from unet_distributed_amd.runtime import plan_check
from unet_distributed_amd.runtime.plan_check import check_engine

from test_plan_check import _engine


def test_dw_pipe_is_on_by_default():
    assert ne.engine_options()["dw_pipe"] == 1
    assert ne.engine_options(dict(dw_pipe=0))["dw_pipe"] == 0


def _conv_dicts(monkeypatch, dw_pipe):
    """The validated headline engine with option dw_pipe and the conv dicts of its training
    and evaluation plans, in order."""
    dicts = []
    add = plan_check.RecordingPlan.add_conv_fwd

    def record(self, d):
        dicts.append(dict(d))
        return add(self, d)

    monkeypatch.setattr(plan_check.RecordingPlan, "add_conv_fwd", record)
    e = _engine("none", False, 2, 128, opts=dict(dw_pipe=dw_pipe))
    monkeypatch.setattr(plan_check.RecordingPlan, "add_conv_fwd", add)
    assert check_engine(e) == {"train": [], "eval": []}
    return e, dicts


def test_dw_pipe_changes_only_fw_pipe(monkeypatch):
    e0, d0 = _conv_dicts(monkeypatch, 0)
    e1, d1 = _conv_dicts(monkeypatch, 1)
    assert e0.plan.names() == e1.plan.names() and e0.fusions == e1.fusions
    assert sorted(e1.fusions["dw_fused"]) == ["conv1b", "conv9b"]
    assert len(d0) == len(d1)
    fused = 0
    for a, b in zip(d0, d1):
        assert set(a) == set(b), a.get("name")
        # (two dry-run engines allocate their own buffers: compare everything but pointers
        # by value, pointers by presence)
        for k in a:
            if k == "fw_pipe":
                assert (a[k], b[k]) == (0, 1), a.get("name")
            elif isinstance(a[k], int) and (a[k] > 1 << 20 or b[k] > 1 << 20):
                assert bool(a[k]) == bool(b[k]), (a.get("name"), k)
            else:
                assert a[k] == b[k], (a.get("name"), k)
        fused += "fw_pipe" in a
        assert ("fw_pipe" in a) == bool(a.get("fw_x")), a.get("name")
    assert fused == 3          # conv9b's launch and the two batch halves of conv1b's
