"""Engine option win_bm2 bit 2 (two-image 512-pixel windows of the 64-channel row-window tile
on 16-wide rows, conv_win.h win_b512_eligible) on dry-run plans, no GPU: with win_bm2 = 7 the
norm-free 128^2 plan validates (every launch has a built kernel) and exactly its nine level-4
forward and data-gradient launches run half the workgroups of win_bm2 = 3; win_bm2 = 3 is
what it was without the bit; the normalised and 3D plans ignore it."""
import pytest

from unet_distributed_amd import native
from unet_distributed_amd.runtime import plan_check
from unet_distributed_amd.runtime.plan_check import check_engine

from test_plan_check import _engine

BATCH = 1024           # the headline batch: the training forward runs as two chunks of 512 images
LEVEL4 = {"fwd:conv4a", "fwd:conv4b", "fwd:conv6a", "fwd:conv6b", "dgrad:conv6b", "dgrad:conv6a",
          "dgrad_skip:conv6a", "dgrad:conv4b", "dgrad:conv4a"}


def _conv_dicts(monkeypatch, cfg, win_bm2, batch=BATCH):
    """The engine of config `cfg` with option win_bm2 and the conv dicts of its plans, in order."""
    dicts = []
    add = plan_check.RecordingPlan.add_conv_fwd

    def record(self, d):
        dicts.append(dict(d))
        return add(self, d)

    monkeypatch.setattr(plan_check.RecordingPlan, "add_conv_fwd", record)
    e = _engine(*cfg, batch=batch, opts=dict(win_bm2=win_bm2))
    monkeypatch.setattr(plan_check.RecordingPlan, "add_conv_fwd", add)
    return e, dicts


def test_headline_plan_halves_the_nine_level_4_grids(monkeypatch):
    grid = native.require().conv_fwd_grid
    e3, d3 = _conv_dicts(monkeypatch, ("none", False, 2, 128), 3)
    e7, d7 = _conv_dicts(monkeypatch, ("none", False, 2, 128), 7)
    assert check_engine(e7) == {"train": [], "eval": []}
    assert e3.plan.names() == e7.plan.names() and e3.fusions == e7.fusions
    assert len(d3) == len(d7)
    halved = set()
    for a, b in zip(d3, d7):
        name, g3, g7 = a.get("name", ""), grid(a), grid(b)
        assert name == b.get("name", "")
        if name in LEVEL4 and a["OW"] == 16 and g3 > 0:
            assert a["OH"] == 16 and a["N"] % 2 == 0, (name, a["N"])
            if name.startswith("fwd:") and a["N"] < BATCH:
                assert a["N"] == BATCH // 2                       # a half-batch forward chunk
            assert g3 == a["N"] * (a["Cout"] // 64) and g3 == 2 * g7, (name, g3, g7)
            halved.add(name)
        else:
            assert g3 == g7, (name, g3, g7)
    assert halved == LEVEL4


def test_bits_0_and_1_alone_launch_what_they_did(monkeypatch):
    """win_bm2 = 3 leaves every 16-wide launch at one 256-pixel window per image and 64 channels
    (the grid of win_bm2 = 0), and bit 2 alone moves nothing but the 16-wide launches."""
    grid = native.require().conv_fwd_grid
    _, d0 = _conv_dicts(monkeypatch, ("none", False, 2, 128), 0)
    _, d3 = _conv_dicts(monkeypatch, ("none", False, 2, 128), 3)
    _, d4 = _conv_dicts(monkeypatch, ("none", False, 2, 128), 4)
    assert len(d0) == len(d3) == len(d4)
    for a, b, c in zip(d0, d3, d4):
        if a["OW"] == 16:
            assert grid(a) == grid(b), a.get("name")
        else:
            assert grid(a) == grid(c), a.get("name")


def test_odd_image_count_keeps_256(monkeypatch):
    """Batch 2: the training forward's chunks hold one image each and keep the 256-pixel window;
    the whole-batch backward launches (two images) take the two-image window."""
    grid = native.require().conv_fwd_grid
    e3, d3 = _conv_dicts(monkeypatch, ("none", False, 2, 128), 3, batch=2)
    e7, d7 = _conv_dicts(monkeypatch, ("none", False, 2, 128), 7, batch=2)
    assert check_engine(e7) == {"train": [], "eval": []}
    for a, b in zip(d3, d7):
        if a["OW"] == 16 and a.get("name", "") in LEVEL4 and a["N"] % 2 == 0:
            assert grid(a) == 2 * grid(b), a.get("name")
        else:
            assert grid(a) == grid(b), a.get("name")


@pytest.mark.parametrize("cfg", [("batch", False, 2, 128), ("group", False, 2, 128), ("none", False, 3, 128)])
def test_normalised_and_3d_plans_ignore_the_bit(monkeypatch, cfg):
    grid = native.require().conv_fwd_grid
    e3, d3 = _conv_dicts(monkeypatch, cfg, 3, batch=4)
    e7, d7 = _conv_dicts(monkeypatch, cfg, 7, batch=4)
    assert check_engine(e7) == {"train": [], "eval": []}
    assert e3.plan.names() == e7.plan.names() and len(d3) == len(d7)
    for a, b in zip(d3, d7):
        assert not b.get("win_bm2") and grid(a) == grid(b), a.get("name")
