"""Label maps on the GPU: the labelmap op (csrc/kernels/labelmap.h) against its torch definition
(ops/labelmap.py) by torch.equal -- the outputs are bytes and integer counts, so there is no
tolerance anywhere -- its refusals, `executor_base.sliding_labels` with its fallback,
`Predictor.segment` on the native backend and predict.py on the device."""
import os
import re

import numpy as np
import pytest
import torch

from unet_distributed_amd.ops import labelmap as lm

pytestmark = pytest.mark.gpu

PAD = 64
GUARD = 0x5A5A5A5A
GUARD8 = 0x5A
UNWRITTEN = 0xEE


def _piece():
    """Labels of a destination row per unit: LM_PIECE of the kernel's text."""
    import unet_distributed_amd
    path = os.path.join(os.path.dirname(unet_distributed_amd.__file__), "csrc", "kernels", "labelmap.h")
    return int(re.search(r"constexpr int LM_PIECE = (\d+);", open(path).read()).group(1))


PIECE = _piece()
# (source (N, D, H, W), destination (Do, Ho, Wo) or None, offset): a sample boundary inside a wave |
# odd Wo: the byte path, an unaligned source | aligned destination, source offset no multiple of 4 |
# whole padded planes | a row of more than one piece (word path) | the same on the byte path |
# identity volume | the real paste | more units than waves (4 x LM_MAX_WGS = 8192): a wave walks two
# rows, one wave's pair straddles the images 0 | 1 and another's ends with image 1
SHAPES = [((3, 1, 8, 8), None, (0, 0, 0)),
          ((2, 1, 16, 24), (1, 20, 31), (0, 3, 5)),
          ((2, 3, 5, 65), (3, 7, 68), (0, 1, 2)),
          ((2, 4, 8, 8), (6, 8, 8), (1, 0, 0)),
          ((1, 1, 3, 4 * PIECE + 520), None, (0, 0, 0)),
          ((1, 1, 2, 2 * PIECE + 3), None, (0, 0, 0)),
          ((1, 16, 24, 24), None, (0, 0, 0)),
          ((1, 1, 128, 128), (1, 240, 240), (0, 56, 56)),
          ((3, 1, 3001, 8), (1, 3003, 12), (0, 1, 4))]
CONTENTS = ["random", "all off", "all on", "at the threshold", "one ulp below", "NaN", "tied maxima", "non-nested"]


def C():
    from unet_distributed_amd import native
    return native.require()


def ptr(t):
    return int(t.data_ptr())


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _probs(shape, K, thr, seed, only=None):
    """fp32 [N, D, H, W, K]: voxel i holds content CONTENTS[(i + i // 7) % 8] (so every content
    meets every lane, row end and box edge), or `only` everywhere."""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    t32 = np.float32(thr)
    below = np.nextafter(t32, np.float32(0))
    p = rng.uniform(0, 1, (n, K)).astype(np.float32)
    i = np.arange(n)
    kind = (i + i // 7) % 8 if only is None else np.full(n, CONTENTS.index(only))
    lo = np.minimum(rng.uniform(0, thr, (n, K)).astype(np.float32), below)
    hi = np.maximum(rng.uniform(thr, 1, (n, K)).astype(np.float32), t32)
    p = np.where((kind == 1)[:, None], lo, p)
    p = np.where((kind == 2)[:, None], hi, p)
    p = np.where((kind == 3)[:, None], t32, p)
    p = np.where((kind == 4)[:, None], below, p)
    p = np.where((kind == 5)[:, None], np.float32("nan"), p)
    p = np.where((kind == 6)[:, None], np.float32(0.75), p)
    nn = hi.copy()
    nn[:, 0] = below                                  # channel 0 off under channels that are on
    p = np.where((kind == 7)[:, None], nn, p)
    return p.reshape(tuple(shape) + (K,)).astype(np.float32)


def _launch(prob, thr, rule, values, dst, off, out_off=0):
    """(labels, counts int32 [N][5], guards intact) of one launch between guard words; `out_off`:
    bytes by which `out` is moved off its 4-byte alignment."""
    N, D, H, W, K = prob.shape
    dev = prob.device
    n_out = N * dst[0] * dst[1] * dst[2]
    obig = torch.full((n_out + 2 * PAD + 4,), GUARD8, dtype=torch.uint8, device=dev)[out_off:]
    out = obig[PAD:PAD + n_out]
    out.fill_(UNWRITTEN)
    cbig = torch.full((N * 5 + 2 * PAD,), GUARD, dtype=torch.int32, device=dev)
    counts = cbig[PAD:PAD + N * 5]
    before = prob.clone()
    ints = [N, D, H, W, K] + list(dst) + list(off) + [lm.RULES.index(rule), lm.pack_values(values)]
    assert C().labelmap_check(*ints, thr) is None
    C().generic("labelmap", [ptr(prob), ptr(out), ptr(counts)], ints, [thr], stream())
    torch.cuda.synchronize()
    ok = bool((obig[:PAD] == GUARD8).all() and (obig[PAD + n_out:] == GUARD8).all() and
              (cbig[:PAD] == GUARD).all() and (cbig[PAD + N * 5:] == GUARD).all() and
              torch.equal(before.view(torch.int32), prob.view(torch.int32)))
    return out.view((N,) + tuple(dst)).clone(), counts.view(N, 5).clone(), ok


def _check(prob, thr, rule, values, dst, off, tag, out_off=0):
    K = prob.shape[-1]
    dst = tuple(prob.shape[1:4]) if dst is None else tuple(dst)
    want, wc = lm.labelmap_torch(prob, thr, rule, values, dst, off)
    got, gc, ok = _launch(prob, thr, rule, values, dst, off, out_off)
    assert ok, tag + ": a guard word or the input changed"
    assert torch.equal(got, want), tag + ": %d labels differ" % int((got != want).sum())
    assert torch.equal(gc[:, :K + 1].long(), wc) and not gc[:, K + 1:].any(), tag + ": counts"
    assert (gc.sum(1) == prob[0].numel() // K).all(), tag
    got2, gc2, ok2 = _launch(prob, thr, rule, values, dst, off, out_off)
    assert ok2 and torch.equal(got2, got) and torch.equal(gc2, gc), tag + ": two launches differ"
    return got


@pytest.mark.parametrize("shape,dst,off", SHAPES, ids=lambda v: "x".join(map(str, v)) if v else "same")
def test_labelmap_matches_labelmap_torch(cuda_dev, shape, dst, off):
    seen = set()
    for K in (1, 2, 3, 4):
        for rule in lm.RULES:
            for thr in (0.5, 0.3):
                values = tuple(range(1, K + 1)) if rule == "nested" else (255, 3, 17, 200)[:K]
                prob = torch.from_numpy(_probs(shape, K, thr, 31 * K + len(rule))).to(cuda_dev)
                tag = "%r -> %r at %r K %d %s thr %g" % (shape, dst, off, K, rule, thr)
                got = _check(prob, thr, rule, values, dst, off, tag)
                seen |= set(got.unique().tolist())
    assert {1, 2, 3, 4, 255, 17, 200} <= seen
    # every content alone (all off: nothing but zeros; all on: the last slot everywhere in the box)
    for only in CONTENTS[1:]:
        prob = torch.from_numpy(_probs(shape, 3, 0.5, 5, only)).to(cuda_dev)
        for rule in lm.RULES:
            got = _check(prob, 0.5, rule, (2, 1, 4), dst, off, "%r %s %s" % (shape, only, rule))
            if only in ("all off", "one ulp below", "NaN"):
                assert not got.any()
            if only in ("at the threshold", "tied maxima"):
                assert set(got.unique().tolist()) <= {0, 4 if rule == "nested" else 2}


def test_labelmap_unaligned_bases(cuda_dev):
    """`out` 1..3 bytes off a word: the byte path; `prob` 4 bytes off a vector: float loads."""
    shape, dst, off = SHAPES[2]
    for K in (1, 3, 4):
        base = torch.from_numpy(_probs(shape, K, 0.5, 77 + K)).to(cuda_dev)
        for out_off in (1, 2, 3):
            _check(base, 0.5, "nested", tuple(range(1, K + 1)), dst, off, "out + %d K %d" % (out_off, K), out_off)
        moved = torch.cat([base.new_zeros(1), base.reshape(-1)])[1:].view(base.shape)
        assert moved.data_ptr() % 16 == 4
        _check(moved, 0.5, "argmax", tuple(range(1, K + 1)), (3, 7, 68), (0, 1, 0), "prob + 4 bytes K %d" % K)
        _check(moved, 0.5, "argmax", tuple(range(1, K + 1)), (3, 7, 68), (0, 1, 0), "both K %d" % K, 2)


def test_labelmap_refusals(cuda_dev):
    """Every refusal of labelmap_check raises ValueError through C.generic with its reason; no
    refused launch is submitted (the pointers are those of tiny buffers)."""
    prob = torch.zeros(64, dtype=torch.float32, device=cuda_dev)
    out = torch.zeros(64, dtype=torch.uint8, device=cuda_dev)
    counts = torch.zeros(8, dtype=torch.int32, device=cuda_dev)
    good = dict(N=1, D=1, H=2, W=2, K=1, Do=1, Ho=2, Wo=2, od=0, oh=0, ow=0, rule=0, values=1, threshold=0.5)
    keys = list(good)[:13]
    assert C().labelmap_check(**good) is None
    big = 1 << 16
    cases = [(dict(K=0), "1..4 classes"), (dict(K=5, values=0x0101010101), "1..4 classes"),
             (dict(N=0), ">= 1"), (dict(D=0), ">= 1"), (dict(H=0), ">= 1"), (dict(W=0), ">= 1"),
             (dict(Do=0), ">= 1"), (dict(Ho=0), ">= 1"), (dict(Wo=0), ">= 1"), (dict(W=1 << 31), "< 2^31"),
             (dict(Wo=(1 << 31) - 256), "Wo < 2^31 - 256"),
             (dict(N=2, D=big, H=big, W=1, Do=big, Ho=big, Wo=1), "N D H W >= 2^31"),
             (dict(N=1 << 15, Do=big, Ho=1, Wo=2, D=1, H=1, W=1), "N Do Ho Wo >= 2^31"),
             (dict(od=1), "outside the destination"), (dict(oh=-1), "outside the destination"),
             (dict(Wo=3, ow=2), "outside the destination"), (dict(Ho=1), "outside the destination"),
             (dict(rule=2), "rule 0 (nested) or 1 (argmax)"),
             (dict(threshold=0.0), "threshold in (0, 1)"), (dict(threshold=1.0), "threshold in (0, 1)"),
             (dict(threshold=float("nan")), "threshold in (0, 1)"), (dict(threshold=1e-60), "threshold in (0, 1)"),
             (dict(values=0), "values byte of 0"), (dict(K=3, values=0x040001), "values byte of 0"),
             (dict(values=-1), "packed in 32 bits"), (dict(values=1 << 32), "packed in 32 bits")]
    for change, reason in cases:
        args = dict(good, **change)
        msg = C().labelmap_check(**args)
        assert msg is not None and reason in msg and msg.startswith("labelmap:"), (change, msg)
        with pytest.raises(ValueError) as e:
            C().generic("labelmap", [ptr(prob), ptr(out), ptr(counts)], [args[k] for k in keys], [args["threshold"]],
                        stream())
        assert msg in str(e.value), (change, str(e.value))
    ints = [good[k] for k in keys]
    for ptrs, reason in (([0, ptr(out), ptr(counts)], "required"), ([ptr(prob), 0, ptr(counts)], "required"),
                         ([ptr(prob), ptr(out), 0], "required"), ([ptr(prob) + 2, ptr(out), ptr(counts)], "aligned"),
                         ([ptr(prob), ptr(out), ptr(counts) + 1], "aligned")):
        with pytest.raises(ValueError, match=reason):
            C().generic("labelmap", ptrs, ints, [0.5], stream())
    with pytest.raises(ValueError, match="argument count"):
        C().generic("labelmap", [ptr(prob), ptr(out), ptr(counts)], ints[:12], [0.5], stream())
    torch.cuda.synchronize()
    assert not out.any() and not counts.any()


class _Refusing:
    """The extension with a labelmap op that refuses everything and must then not be launched."""

    def __init__(self, real):
        self._real, self.asked = real, 0

    def labelmap_check(self, *a, **k):
        self.asked += 1
        return "labelmap: refused by the test"

    def generic(self, kind, *a, **k):
        assert kind != "labelmap", "a refused launch was submitted"
        return self._real.generic(kind, *a, **k)

    def __getattr__(self, name):
        return getattr(self._real, name)


def test_sliding_labels_and_its_fallback(cuda_dev):
    from unet_distributed_amd.runtime.executor_base import sliding_labels
    prob = torch.from_numpy(_probs((2, 3, 9, 20), 3, 0.5, 9)).to(cuda_dev)
    for p, dst, off in ((prob, (5, 9, 24), (1, 0, 4)), (prob[:, 0], (12, 21), (3, 1)), (prob, None, (0, 0, 0))):
        want, wc = lm.labelmap_torch(p, 0.5, "nested", (2, 1, 4), dst, off)
        got, gc = sliding_labels(C(), p, 0.5, "nested", (2, 1, 4), dst, off)
        assert got.dtype == torch.uint8 and gc.dtype == torch.int32 and got.is_cuda
        assert torch.equal(got, want) and torch.equal(gc.long(), wc)
        refusing = _Refusing(C())
        fb, fc = sliding_labels(refusing, p, 0.5, "nested", (2, 1, 4), dst, off)
        assert refusing.asked == 1, "the fallback asks the op's check"
        assert fb.dtype == torch.uint8 and fc.dtype == torch.int32 and fb.is_cuda
        assert torch.equal(fb, got) and torch.equal(fc, gc)
    with pytest.raises(ValueError, match="does not fit"):
        sliding_labels(C(), prob, 0.5, "nested", (2, 1, 4), (3, 9, 19), (0, 0, 0))


# ------------------------------------------------------------------ public paths
def _export(tmp_path, **kw):
    from test_labelmap_cpu import _export as export
    return export(tmp_path, **kw)


@pytest.mark.parametrize("components", ["", "largest"])
@pytest.mark.parametrize("size", [(40, 56), (37, 45)], ids=lambda s: "%dx%d" % s)
def test_predictor_segment_native(cuda_dev, tmp_path, size, components):
    """5 images under a byte cap that holds two (chunks (0, 2), (2, 4), (4, 5)): segment is the
    definition applied to the backend's own filtered sliding-window probabilities."""
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    K = 3
    model = load_saved_model(_export(tmp_path, out_channels=K), device=cuda_dev, batch=4, components=components)
    assert model.name == "native"
    x, _ = synthetic_brats(5, 64, 4, seed=2, out_channels=K)
    x = np.ascontiguousarray(x[:, :size[0], :size[1]])
    cap = 2 * size[0] * size[1] * (4 + K) * 4
    chunks = model.sliding_chunks(x.shape, cap)
    assert chunks == [(0, 2), (2, 4), (4, 5)]
    be = model.backend
    raw = [be.predict_sliding(torch.from_numpy(x[s:t]).to(cuda_dev), post=False).clone() for s, t in chunks]
    rule, values = lm.parse_labels("", K, 5)
    dst, off = (1, size[0] + 5, size[1] + 3), (0, 2, 3)
    want = [lm.labelmap_torch(be.sliding_filter(p, 0.5).clone(), 0.5, rule, values, dst, off) for p in raw]
    labels, counts = model.segment(x, max_bytes=cap, mode=5, out_shape=dst[1:], offset=off[1:])
    assert labels.dtype == np.uint8 and labels.shape == (5,) + dst[1:] and counts.shape == (5, K + 1)
    assert np.array_equal(labels, torch.cat([w[0] for w in want]).cpu().numpy())
    assert np.array_equal(counts, torch.cat([w[1] for w in want]).cpu().numpy())
    assert len(np.unique(labels)) > 1, "a constant map tests nothing"
    case = be.sliding_filter(torch.cat(raw).unsqueeze(0), 0.5).clone()
    wv, wc = lm.labelmap_torch(case, 0.5, rule, values, (5,) + dst[1:], off)
    vol, vc = model.segment(x, max_bytes=cap, mode=5, volume=True, out_shape=dst[1:], offset=off[1:])
    assert vol.shape == (5,) + dst[1:] and np.array_equal(vol, wv[0].cpu().numpy())
    assert np.array_equal(vc, wc.cpu().numpy()) and vc.shape == (1, K + 1)
    if not components:                                  # (no filter: the case is its slices)
        assert np.array_equal(vol, labels)


def test_cli_case_on_the_device(cuda_dev, tmp_path):
    from test_labelmap_cpu import check_cli_case
    check_cli_case(tmp_path, "native", str(cuda_dev))


def test_segment_moves_nothing_else(cuda_dev, tmp_path):
    """predict, predict_sliding, stats_sliding and components_sliding return the same values
    before and after segment, and segment leaves the kept full-size filter result (_sw_pp)
    alone; _pp_thr is invalidated, as after any predict_sliding (the tiles' forwards overwrite
    the executor's probabilities)."""
    from unet_distributed_amd.data.datasets import synthetic_brats
    from unet_distributed_amd.inference import load_saved_model
    K = 3
    model = load_saved_model(_export(tmp_path, out_channels=K), device=cuda_dev, batch=4, components="largest")
    x, y = synthetic_brats(4, 64, 4, seed=6, out_channels=K)
    xs, ys = np.ascontiguousarray(x[:3, :40, :56]), np.ascontiguousarray(y[:3, :40, :56]).astype(np.float32)
    x32 = np.ascontiguousarray(x[:, :32, :32])

    def everything():
        return [model.predict_sliding(xs), model.stats_sliding(xs, ys), model.components_sliding(xs),
                model.predict(x32)]

    before = everything()
    kept, thr = model.backend._sw_pp, model.backend._pp_thr
    assert kept is not None and thr == 0.5
    a, _ = model.segment(xs)
    b, _ = model.segment(xs, volume=True, labels="argmax:7,8,9", threshold=0.3)
    assert a.shape == b.shape == (3, 40, 56)
    assert model.backend._sw_pp is kept and model.backend._pp_thr is None
    after = everything()
    for u, v in zip(before, after):
        assert u.dtype == v.dtype and np.array_equal(u, v, equal_nan=True)
