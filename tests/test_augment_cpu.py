"""Training-time augmentation off the GPU: the --augment flags, the counter-based parameter
draw (data/augment.py), the torch transform against numpy, plan-time validation of the
gather_batch_aug ops on the CPU dry run, the feeder, and the trainer on the ATen backend
(evaluation untouched, resume and data-parallel runs see the same augmented batches)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from unet_distributed_amd.data import augment as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ flags
def test_augment_flags_default_off_and_validated():
    from unet_distributed_amd.config import Config, parse_args, parse_augment, validate
    assert Config().augment == "" and Config().augment_intensity == 0.1
    assert parse_args([]).augment == ""
    cfg = parse_args(["--augment", "rot90,flip", "--augment_intensity", "0.25"])
    assert parse_augment(cfg.augment) == ("rot90", "flip") and cfg.augment_intensity == 0.25
    assert parse_augment("") == () and parse_augment("flip, intensity") == ("flip", "intensity")
    for bad, item in (("flip,rot", "rot"), ("flip,flip", "flip"), ("flip,,rot90", "''"), ("Flip", "Flip")):
        with pytest.raises(SystemExit) as e:
            parse_args(["--augment", bad])
        assert item in str(e.value)
    for a in (-0.01, 1.0, 2.0, float("nan")):
        with pytest.raises(SystemExit):
            validate(Config(augment="intensity", augment_intensity=a))
    validate(Config(augment="intensity", augment_intensity=0.0))
    validate(Config(augment_intensity=0.999))


# ------------------------------------------------------------------ draw
ALL = "flip,rot90,intensity"


def test_draw_depends_only_on_seed_step_and_sample_index():
    idx = np.arange(100, 164)
    code, aff = A.draw(816, 7, idx, ALL, 4, 2, 0.1)
    assert code.dtype == np.int32 and code.shape == (64,) and aff.dtype == np.float32 and aff.shape == (64, 4, 2)
    perm = np.random.default_rng(0).permutation(64)
    c2, a2 = A.draw(816, 7, idx[perm], ALL, 4, 2, 0.1)
    assert np.array_equal(c2, code[perm]) and np.array_equal(a2, aff[perm])
    sub = np.array([5, 40, 41, 3])
    c3, a3 = A.draw(816, 7, idx[sub], ALL, 4, 2, 0.1)
    assert np.array_equal(c3, code[sub]) and np.array_equal(a3, aff[sub])
    one = A.draw(816, 7, [idx[9]], ALL, 4, 2, 0.1)
    assert one[0][0] == code[9] and np.array_equal(one[1][0], aff[9])
    # another step, another seed: other parameters
    for other in (A.draw(816, 8, idx, ALL, 4, 2, 0.1), A.draw(817, 7, idx, ALL, 4, 2, 0.1)):
        assert (other[0] != code).mean() > 0.5 and (other[1] != aff).mean() > 0.9
    # a repeated index repeats its parameters
    rep = A.draw(816, 7, [3, 9, 3], ALL, 4, 2, 0.1)
    assert rep[0][0] == rep[0][2] and np.array_equal(rep[1][0], rep[1][2])


def test_draw_sets_only_enabled_bits_and_covers_every_code():
    idx = np.arange(1024)
    hist = lambda spec, dims: np.bincount(A.draw(1, 3, idx, spec, 4, dims)[0], minlength=16)  # noqa: E731
    h = hist("flip", 2)
    assert (h[:4] > 0).all() and h[4:].sum() == 0
    h = hist("flip", 3)
    assert all(h[c] > 0 for c in (0, 1, 2, 3, 8, 9, 10, 11)) and h[4:8].sum() == 0 and h[12:].sum() == 0
    for dims in (2, 3):
        h = hist("rot90", dims)
        assert sorted(np.nonzero(h)[0]) == sorted(A.ROT90_CODES) == [0, 3, 5, 6]
    h = hist("flip,rot90", 2)
    assert (h[:8] > 0).all() and h[8:].sum() == 0
    h = hist("rot90,flip", 3)
    assert (h > 0).all()
    # uniform within a loose 6-sigma band (1024 draws over 8 codes: 128 +- 64)
    assert np.abs(hist("flip,rot90", 2)[:8] - 128).max() < 64
    assert hist("intensity", 3)[1:].sum() == 0 and hist("", 2)[1:].sum() == 0
    assert A.draw(1, 3, idx, "flip", 4, 2)[1] is None


@pytest.mark.parametrize("a", [0.0, 0.1, 0.25, 0.999])
def test_draw_intensity_ranges(a):
    _, aff = A.draw(5, 0, np.arange(4096), "intensity", 3, 2, a)
    s, t = aff[..., 0].astype(np.float64), aff[..., 1].astype(np.float64)
    assert s.min() >= 1.0 - a and s.max() <= 1.0 + a and t.min() >= -a and t.max() <= a
    if a > 0:
        # the ranges are used: both ends within 1 % of the width, channels drawn independently
        assert s.min() < 1 - 0.98 * a and s.max() > 1 + 0.98 * a and t.min() < -0.98 * a and t.max() > 0.98 * a
        assert abs(np.corrcoef(s[:, 0], s[:, 1])[0, 1]) < 0.1 and abs(np.corrcoef(s[:, 0], t[:, 0])[0, 1]) < 0.1
    else:
        assert (s == 1).all() and (t == 0).all()


# ------------------------------------------------------------------ apply_torch against numpy
def _np_by_definition(src, code):
    """out[d, h, w] = src[d', h', w'] read off the issue's definition with index arrays."""
    vol = src if src.ndim == 4 else src[None]
    Dn, H, W = vol.shape[:3]
    d, h, w = np.meshgrid(np.arange(Dn), np.arange(H), np.arange(W), indexing="ij")
    dd = Dn - 1 - d if code & 8 else d
    hh, ww = (w, h) if code & 4 else (h, w)
    hh = H - 1 - hh if code & 2 else hh
    ww = W - 1 - ww if code & 1 else ww
    out = vol[dd, hh, ww]
    return out if src.ndim == 4 else out[0]


def _np_by_flips(src, code):
    hd, wd = src.ndim - 3, src.ndim - 2
    a = src
    if code & 2:
        a = np.flip(a, hd)
    if code & 1:
        a = np.flip(a, wd)
    if code & 8:
        a = np.flip(a, 0)
    if code & 4:
        a = np.swapaxes(a, hd, wd)
    return a


@pytest.mark.parametrize("dims,K", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_apply_torch_matches_numpy_for_every_code(dims, K):
    rng = np.random.default_rng(dims * 10 + K)
    ncode = 8 if dims == 2 else 16
    shape = (ncode, 16, 16) if dims == 2 else (ncode, 4, 16, 16)
    x = rng.standard_normal(shape + (4,)).astype(np.float32)
    y = (rng.random(shape + (K,)) < 0.3).astype(np.float32)
    code = rng.permutation(ncode).astype(np.int32)
    xo, yo = A.apply_torch(torch.from_numpy(x), torch.from_numpy(y), code)
    assert xo.is_contiguous() and xo.shape == x.shape and yo.shape == y.shape
    for i, c in enumerate(code):
        for got, src in ((xo, x), (yo, y)):
            assert np.array_equal(got[i].numpy(), _np_by_definition(src[i], int(c))), (c, "definition")
            assert np.array_equal(got[i].numpy(), _np_by_flips(src[i], int(c))), (c, "flips")
    # the inverse code restores the input; the inputs were not written
    inv = np.array([A.inverse_code(int(c)) for c in code], dtype=np.int32)
    xr, yr = A.apply_torch(xo, yo, torch.from_numpy(inv))
    assert np.array_equal(xr.numpy(), x) and np.array_equal(yr.numpy(), y)
    assert set(inv) == set(code) and sum(i != c for i, c in zip(inv, code)) == (2 if dims == 2 else 4)


def test_rot90_codes_are_numpy_rot90():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 16, 16, 4)).astype(np.float32)
    y = rng.standard_normal((4, 16, 16, 3)).astype(np.float32)
    xo, yo = A.apply_torch(torch.from_numpy(x), torch.from_numpy(y), np.array(A.ROT90_CODES, dtype=np.int32))
    for k in range(4):
        assert np.array_equal(xo[k].numpy(), np.rot90(x[k], k, axes=(0, 1)))
        assert np.array_equal(yo[k].numpy(), np.rot90(y[k], k, axes=(0, 1)))
    v = rng.standard_normal((4, 4, 16, 16, 1)).astype(np.float32)
    vo, _ = A.apply_torch(torch.from_numpy(v), torch.from_numpy(v), np.array(A.ROT90_CODES, dtype=np.int32))
    for k in range(4):
        assert np.array_equal(vo[k].numpy(), np.rot90(v[k], k, axes=(1, 2)))


def test_apply_torch_intensity_and_refusals():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((8, 16, 16, 4)).astype(np.float32)
    y = (rng.random((8, 16, 16, 1)) < 0.5).astype(np.float32)
    code, aff = A.draw(3, 1, np.arange(8), ALL, 4, 2, 0.25)
    xo, yo = A.apply_torch(torch.from_numpy(x), torch.from_numpy(y), code, aff)
    xg, yg = A.apply_torch(torch.from_numpy(x), torch.from_numpy(y), code)
    assert torch.equal(yo, yg)                         # targets: geometry only
    want = (xg.numpy().astype(np.float64) * aff[:, None, None, :, 0].astype(np.float64)
            + aff[:, None, None, :, 1].astype(np.float64)).astype(np.float32)
    assert np.array_equal(xo.numpy(), want)
    with pytest.raises(ValueError):
        A.apply_torch(torch.zeros(2, 8, 16, 1), torch.zeros(2, 8, 16, 1), np.array([4, 0]))    # T, not square
    with pytest.raises(ValueError):
        A.apply_torch(torch.zeros(2, 8, 8, 1), torch.zeros(2, 8, 8, 1), np.array([8, 0]))      # FD in 2D
    with pytest.raises(ValueError):
        A.apply_torch(torch.zeros(2, 8, 8, 1), torch.zeros(2, 8, 8, 1), np.array([0]))


# ------------------------------------------------------------------ plan-time validation
def _C():
    from unet_distributed_amd import native
    return native.require()


@pytest.mark.parametrize("kind", ["gather_batch_aug", "f32_gather_batch_aug"])
def test_gather_batch_aug_plan_time_validation(kind):
    C = _C()
    for dt in ((0, 1) if kind == "gather_batch_aug" else (0,)):
        plan = C.Plan(dt)
        ptrs = [4096 * (i + 1) for i in range(7)]
        # ints: B, D, H, W, Cin, Cpad, K -- tiled (Cpad 4, 8) and per-pixel kernels, null affine
        for ints in ([8, 1, 48, 48, 4, 4, 3], [16, 16, 16, 16, 4, 4, 2], [2, 1, 16, 16, 1, 4, 1], [4, 1, 32, 32, 8, 8, 4],
                     [2, 1, 16, 16, 1, 1, 1], [2, 1, 16, 16, 3, 32, 1], [1024, 1, 128, 128, 4, 4, 1],
                     [8, 128, 128, 128, 4, 4, 1]):
            i = plan.add_generic(kind, ptrs, ints, [], "gather")
            assert plan.check_dispatch(i, i + 1) == []
            i = plan.add_generic(kind, ptrs[:4] + [0] + ptrs[5:], ints, [], "gather")
            assert plan.check_dispatch(i, i + 1) == []
        n0 = plan.size()
        bad = ([2, 1, 32, 16, 4, 4, 1],            # H != W
               [2, 1, 32, 32, 4, 4, 5], [2, 1, 32, 32, 4, 4, 0],        # K outside 1..4
               [2, 1, 32, 32, 8, 4, 1], [2, 1, 32, 32, 4, 128, 1], [2, 1, 32, 32, 0, 4, 1],   # Cin <= Cpad <= 64
               [2, 0, 32, 32, 4, 4, 1], [0, 1, 32, 32, 4, 4, 1],        # D, B >= 1
               [1024, 1, 512, 512, 8, 8, 1], [2048, 1, 512, 512, 1, 1, 4], [1 << 40, 1 << 40, 1, 1, 1, 1, 1])  # >= 2^31
        for ints in bad:
            with pytest.raises(ValueError):
                plan.add_generic(kind, ptrs, ints, [], "gather")
            with pytest.raises(ValueError):
                C.generic(kind, ptrs, ints, [], 0, dt)                   # (immediate style: nothing launched)
        good = [2, 1, 32, 32, 4, 4, 1]
        for missing in (0, 1, 2, 3, 5, 6):          # every pointer but the affine is required
            with pytest.raises(ValueError):
                plan.add_generic(kind, [0 if j == missing else p for j, p in enumerate(ptrs)], good, [], "")
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs[:6], good, [], "")
        with pytest.raises(ValueError):
            plan.add_generic(kind, ptrs, good[:6], [], "")
        assert plan.size() == n0


def test_plan_check_knows_the_extents_of_the_new_ops():
    from unet_distributed_amd.runtime.plan_check import _generic_rw, _generic_write_spans
    p = [4096 * (i + 1) for i in range(7)]
    ints = [8, 2, 16, 16, 3, 4, 2]
    px = 8 * 2 * 16 * 16
    assert _generic_write_spans("gather_batch_aug", p, ints) == [(p[5], px * 4 * 2), (p[6], px * 2 * 2)]
    assert _generic_write_spans("f32_gather_batch_aug", p, ints) == [(p[5], px * 4 * 4), (p[6], px * 2 * 4)]
    assert _generic_rw("gather_batch_aug", p[:4] + [0] + p[5:], ints) == (p[:4], p[5:])


# ------------------------------------------------------------------ feeder
def test_feeder_without_aug_is_unchanged_and_with_aug_feeds_the_sorted_batch():
    from unet_distributed_amd.data.loader import DeviceFeeder, ResidentBatch
    rng = np.random.default_rng(4)
    x = rng.standard_normal((11, 16, 16, 4)).astype(np.float32)
    y = (rng.random((11, 16, 16, 3)) < 0.5).astype(np.float32)
    idx = np.array([9, 2, 7, 2])
    f = DeviceFeeder(x, y, 4, "cpu")
    si = np.sort(idx)
    for got in (f.get(idx), f.get(idx, lazy=False), f.get(idx, False, None)):
        assert np.array_equal(got[0].numpy(), x[si]) and np.array_equal(got[1].numpy(), y[si])
    seen = []

    def aug(sorted_idx):
        seen.append(np.array(sorted_idx))
        return A.draw(1, 2, sorted_idx, ALL, 4, 2, 0.2)

    gx, gy = f.get(idx, aug=aug)
    assert len(seen) == 1 and np.array_equal(seen[0], si)
    wx, wy = A.apply_torch(torch.from_numpy(x[si]), torch.from_numpy(y[si]), *A.draw(1, 2, si, ALL, 4, 2, 0.2))
    assert torch.equal(gx, wx) and torch.equal(gy, wy)
    assert gx[0].equal(gx[1]) and not gx[1].equal(gx[2])    # the repeated sample: same parameters, same pixels
    # a ResidentBatch hands out the augmented tensors too
    code, aff = A.draw(1, 2, si, ALL, 4, 2, 0.2)
    rb = ResidentBatch(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(si),
                       (torch.from_numpy(code), torch.from_numpy(aff)))
    tx, ty = rb.tensors()
    assert torch.equal(tx, wx) and torch.equal(ty, wy) and rb.npix == 4 * 16 * 16 * 3
    px, py = ResidentBatch(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(si)).tensors()
    assert np.array_equal(px.numpy(), x[si]) and np.array_equal(py.numpy(), y[si])


# ------------------------------------------------------------------ trainer on the ATen backend
def _trainer_cfg(tmp, **kw):
    from unet_distributed_amd.config import Config
    base = dict(synthetic=True, synthetic_train=16, synthetic_test=8, batch_size=4, img_size=32, in_channels=4,
                out_channels=1, device="cpu", backend="torch", dtype="fp32", dropout=0.0, checkpoint_dir=str(tmp),
                no_checkpoint=True, tensorboard=False, export=False, resume=False, progress=False, steps=3,
                log_every=1000)
    return Config(**dict(base, **kw))


def _record(tr):
    """Every batch the trainer feeds its backend, by step."""
    fed = {}
    inner = tr.backend.fwd_bwd

    def fwd_bwd(x, y, seed, **kw):
        fed[tr.flat.global_step] = (x.clone(), y.clone())
        return inner(x, y, seed, **kw)

    tr.backend.fwd_bwd = fwd_bwd
    return fed


def test_cpu_trainer_augments_training_batches_only(tmp_path, capsys):
    from unet_distributed_amd.runtime.trainer import Trainer
    plain = Trainer(_trainer_cfg(tmp_path / "a"))
    capsys.readouterr()
    tr = Trainer(_trainer_cfg(tmp_path / "b", augment="flip,rot90"))
    assert "Training augmentation: flip, rot90\n" in capsys.readouterr().out
    # evaluation: the same parameters score the same with and without the flag
    assert torch.equal(plain.flat.master, tr.flat.master)
    assert tr.evaluate() == plain.evaluate()
    fed_plain, fed = _record(plain), _record(tr)
    out = tr.run()
    plain.run()
    assert out["global_step"] == 3 and np.isfinite(out["train"]["loss"]) and sorted(fed) == [0, 1, 2]
    epoch = tr.sampler.epoch_indices(0)
    for step in range(3):
        si = np.sort(epoch[step])
        x0, y0 = fed_plain[step]
        assert np.array_equal(x0.numpy(), tr.x_train[si])           # (the plain run: the dataset's pixels)
        code, aff = A.draw(tr.cfg.seed, step, si, "flip,rot90", 4, 2)
        assert aff is None
        wx, wy = A.apply_torch(x0, y0, code)
        assert torch.equal(fed[step][0], wx) and torch.equal(fed[step][1], wy)
    assert any(not torch.equal(fed[s][0], fed_plain[s][0]) for s in range(3))


def test_resumed_run_feeds_the_batches_of_the_uninterrupted_run(tmp_path):
    from unet_distributed_amd.runtime.trainer import Trainer
    kw = dict(augment="flip,rot90,intensity", augment_intensity=0.2)
    whole = Trainer(_trainer_cfg(tmp_path / "whole", **kw))
    fed_whole = _record(whole)
    whole.run()
    ck = dict(no_checkpoint=False, resume=True, save_model_secs=1e9)
    Trainer(_trainer_cfg(tmp_path / "ck", steps=2, **ck, **kw)).run()
    again = Trainer(_trainer_cfg(tmp_path / "ck", steps=3, **ck, **kw))
    assert again.restored and again.flat.global_step == 2
    fed = _record(again)
    again.run()
    assert sorted(fed) == [2]
    assert torch.equal(fed[2][0], fed_whole[2][0]) and torch.equal(fed[2][1], fed_whole[2][1])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
    torch.set_num_threads(2)
    from unet_distributed_amd.parallel import dist as D
    from unet_distributed_amd.runtime.trainer import Trainer
    cfg = _trainer_cfg(os.path.join(out, "r%d" % rank), batch_size=8, dist_backend="gloo", dist_timeout_s=120.0,
                       augment="flip,rot90,intensity")
    tr = Trainer(cfg)
    idx = tr.sampler.epoch_indices(0)[1]             # this rank's shard of global batch 1
    x, y = tr._batch(idx, 1)
    np.savez(os.path.join(out, "r%d.npz" % rank), idx=np.sort(idx), x=x.numpy(), y=y.numpy())
    D.destroy()


def test_two_ranks_see_the_augmented_global_batch_of_one(tmp_path):
    from unet_distributed_amd.runtime.trainer import Trainer
    mp.spawn(_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    tr = Trainer(_trainer_cfg(tmp_path / "w1", batch_size=8, augment="flip,rot90,intensity"))
    gidx = tr.sampler.epoch_indices(0)[1]
    gx, gy = tr._batch(gidx, 1)
    pos = {int(s): i for i, s in enumerate(np.sort(gidx))}
    seen = []
    for r in range(2):
        z = np.load(tmp_path / ("r%d.npz" % r))
        assert len(z["idx"]) == 4
        code, aff = A.draw(tr.cfg.seed, 1, z["idx"], "flip,rot90,intensity", 4, 2, tr.cfg.augment_intensity)
        gcode, gaff = A.draw(tr.cfg.seed, 1, np.sort(gidx), "flip,rot90,intensity", 4, 2, tr.cfg.augment_intensity)
        for j, s in enumerate(z["idx"]):
            i = pos[int(s)]
            assert code[j] == gcode[i] and np.array_equal(aff[j], gaff[i])
            assert np.array_equal(z["x"][j], gx[i].numpy()) and np.array_equal(z["y"][j], gy[i].numpy())
            seen.append(int(s))
    assert sorted(seen) == sorted(pos)
