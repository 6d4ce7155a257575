"""Engine option win_bm2 (512-pixel windows of the 64-channel row-window tile, conv_win.h
win_b512_eligible) on dry-run plans, no GPU: with it on, the norm-free 128^2 plan validates
(every launch has a built kernel) and its level-2 / level-3 forward and data-gradient
launches run half the workgroups; the normalised and 3D plans do not change."""
import pytest

from unet_distributed_amd import native
from unet_distributed_amd.runtime import native_engine as ne
from unet_distributed_amd.runtime import plan_check
from unet_distributed_amd.runtime.plan_check import check_engine

from test_plan_check import _engine


def test_win_bm2_is_an_engine_option():
    assert ne.engine_options()["win_bm2"] == ne.ENGINE_DEFAULTS["win_bm2"]
    assert ne.engine_options(dict(win_bm2=3))["win_bm2"] == 3


def _conv_dicts(monkeypatch, cfg, win_bm2):
    """The engine of config `cfg` with option win_bm2 and the conv dicts of its plans, in order."""
    dicts = []
    add = plan_check.RecordingPlan.add_conv_fwd

    def record(self, d):
        dicts.append(dict(d))
        return add(self, d)

    monkeypatch.setattr(plan_check.RecordingPlan, "add_conv_fwd", record)
    e = _engine(*cfg, opts=dict(win_bm2=win_bm2))
    monkeypatch.setattr(plan_check.RecordingPlan, "add_conv_fwd", add)
    return e, dicts


def test_headline_plan_halves_the_level_2_3_grids(monkeypatch):
    grid = native.require().conv_fwd_grid
    e0, d0 = _conv_dicts(monkeypatch, ("none", False, 2, 128), 0)
    e1, d1 = _conv_dicts(monkeypatch, ("none", False, 2, 128), 3)
    assert check_engine(e1) == {"train": [], "eval": []}
    assert e0.plan.names() == e1.plan.names() and e0.fusions == e1.fusions
    assert len(d0) == len(d1)
    halved = set()
    for a, b in zip(d0, d1):
        name, g0, g1 = a.get("name", ""), grid(a), grid(b)
        assert name == b.get("name", "")
        lvl23 = name.split(":")[0] in ("fwd", "dgrad", "dgrad_skip") and a["OW"] in (32, 64) and g0 > 0
        # (dgrad:conv2a writes 32 channels: the 32-channel tile, whose window is 512 pixels already)
        if lvl23 and name != "dgrad:conv2a":
            assert g0 == 2 * g1, (name, g0, g1)
            halved.add(name)
        else:
            assert g0 == g1, (name, g0, g1)
    convs = ("conv2a", "conv2b", "conv3a", "conv3b", "conv7a", "conv7b", "conv8a", "conv8b")
    want = {"fwd:" + c for c in convs} | {"dgrad:" + c for c in convs if c != "conv2a"}
    want |= {"dgrad_skip:conv7a", "dgrad_skip:conv8a", "dgrad:conv9a"}     # (conv9a's: the composite, 64-wide s2d form)
    assert halved == want


@pytest.mark.parametrize("cfg", [("batch", False, 2, 128), ("group", False, 2, 128), ("none", False, 3, 128)])
def test_normalised_and_3d_plans_are_unchanged(monkeypatch, cfg):
    grid = native.require().conv_fwd_grid
    e0, d0 = _conv_dicts(monkeypatch, cfg, 0)
    e1, d1 = _conv_dicts(monkeypatch, cfg, 3)
    assert check_engine(e1) == {"train": [], "eval": []}
    assert e0.plan.names() == e1.plan.names() and len(d0) == len(d1)
    for a, b in zip(d0, d1):
        assert not b.get("win_bm2") and grid(a) == grid(b), a.get("name")
