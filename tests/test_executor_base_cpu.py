"""The executors' shared base (runtime/executor_base.py): the op-name prefix and the one builder
of the gather_batch_aug / _crop / _warp arguments, on dry-run executors with a recording `C`.
The expected (ptrs, ints) are those of bindings.cpp, written out by hand."""
import types

import pytest
import torch

from test_tta_cpu import _dry_engine

B, IMG, CIN = 2, 16, 4
STREAM = types.SimpleNamespace(cuda_stream=0)      # (no GPU: native.stream_handle reads this field only)


class _Recorder:
    """The extension module with `generic` recording its arguments and launching nothing."""

    def __init__(self, C):
        self._C = C
        self.calls = []

    def generic(self, kind, ptrs, ints, floats, stream=0, dt=0):
        self.calls.append((kind, list(ptrs), list(ints), list(floats), dt))

    def __getattr__(self, k):
        return getattr(self._C, k)


def _engine(dtype, K):
    from unet_distributed_amd.config import Config
    e = _dry_engine(Config(out_channels=K, batch_size=B, img_size=IMG, in_channels=CIN, dtype=dtype))
    e.C = _Recorder(e.C)
    return e


def _dataset(stored, K):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, stored, stored, CIN, generator=g)
    y = (torch.rand(5, stored, stored, K, generator=g) > 0.5).float()
    return x, y, torch.tensor([3, 1])


def p(t):
    return int(t.data_ptr())


CASES = [("bf16", 1, ""), ("bf16", 3, ""), ("fp32", 1, "f32_")]


@pytest.mark.parametrize("dtype,K,prefix", CASES, ids=["bf16-K1", "bf16-K3", "fp32"])
def test_load_indexed_issues_the_documented_launch(dtype, K, prefix):
    e = _engine(dtype, K)
    assert (e.OP_PREFIX, e.K, e.dt_id, e.cpad) == (prefix, K, 0, 4)
    assert e._op("seg_stats") == prefix + "seg_stats" and e._op("gather_batch_warp") == prefix + "gather_batch_warp"
    for bare in ("tta_acc", "sw_extract", "sw_blend", "sw_finish", "components"):
        assert e._op(bare) == bare
    xb, tb = p(e.bufs["x"]), p(e.target)
    x, y, idx = _dataset(IMG, K)
    code = torch.tensor([1, 6], dtype=torch.int32)
    affine = torch.rand(B, CIN, 2)

    # plain: gather_batch (ptrs x_all, y_all, idx, xb, tb; ints B, P, Cin, Cpad [, K]); the fp32
    # executor has no such kernel and copies
    e.load_indexed(x, y, idx, STREAM)
    if dtype == "fp32":
        assert e.C.calls == []
        assert torch.equal(e.bufs["x"], x.index_select(0, idx))
        assert torch.equal(e.target, y.index_select(0, idx).reshape(-1))
    else:
        assert e.C.calls == [("gather_batch", [p(x), p(y), p(idx), xb, tb],
                              [2, 256, 4, 4] + ([] if K == 1 else [K]), [], 0)]
    e.C.calls.clear()

    # aug: ptrs x_all, y_all, idx, code, affine or 0, xb, tb; ints B, D, H, W, Cin, Cpad, K
    e.load_indexed(x, y, idx, STREAM, aug=(code, affine))
    assert e.C.calls == [(prefix + "gather_batch_aug", [p(x), p(y), p(idx), p(code), p(affine), xb, tb],
                          [2, 1, 16, 16, 4, 4, K], [], 0)]
    e.C.calls.clear()
    e.load_indexed(x, y, idx, STREAM, aug=(code, None))
    assert e.C.calls == [(prefix + "gather_batch_aug", [p(x), p(y), p(idx), p(code), 0, xb, tb],
                          [2, 1, 16, 16, 4, 4, K], [], 0)]
    e.C.calls.clear()

    # crop: ptrs x_all, y_all, idx, origin, code or 0, affine or 0, xb, tb;
    # ints B, Ds, Hs, Ws, D, H, W, Cin, Cpad, K
    xs, ys, _ = _dataset(24, K)
    origin = torch.tensor([[0, 3, 8], [0, 0, 5]], dtype=torch.int32)
    crop = (origin, (1, 16, 16))
    e.load_indexed(xs, ys, idx, STREAM, crop=crop)
    assert e.C.calls == [(prefix + "gather_batch_crop", [p(xs), p(ys), p(idx), p(origin), 0, 0, xb, tb],
                          [2, 1, 24, 24, 1, 16, 16, 4, 4, K], [], 0)]
    e.C.calls.clear()
    e.load_indexed(xs, ys, idx, STREAM, aug=(code, affine), crop=crop)
    assert e.C.calls == [(prefix + "gather_batch_crop", [p(xs), p(ys), p(idx), p(origin), p(code), p(affine), xb, tb],
                          [2, 1, 24, 24, 1, 16, 16, 4, 4, K], [], 0)]
    e.C.calls.clear()

    # warp: ptrs x_all, y_all, idx, origin or 0, code or 0, mat, affine or 0, xb, tb; ints as the crop's
    mat = torch.tensor([[65536, 0, 0, 65536], [0, -65536, 65536, 0]], dtype=torch.int32)
    e.load_indexed(xs, ys, idx, STREAM, aug=(code, None, mat), crop=crop)
    assert e.C.calls == [(prefix + "gather_batch_warp", [p(xs), p(ys), p(idx), p(origin), p(code), p(mat), 0, xb, tb],
                          [2, 1, 24, 24, 1, 16, 16, 4, 4, K], [], 0)]
    e.C.calls.clear()
    e.load_indexed(xs, ys, idx, STREAM, aug=(None, affine, mat))        # (no crop: the input at origin 0)
    assert e.C.calls == [(prefix + "gather_batch_warp", [p(xs), p(ys), p(idx), 0, 0, p(mat), p(affine), xb, tb],
                          [2, 1, 24, 24, 1, 16, 16, 4, 4, K], [], 0)]
    e.C.calls.clear()
    # a third item that is None is no warp
    e.load_indexed(xs, ys, idx, STREAM, aug=(code, None, None), crop=crop)
    assert [c[0] for c in e.C.calls] == [prefix + "gather_batch_crop"]


@pytest.mark.parametrize("dtype,K,prefix", CASES, ids=["bf16-K1", "bf16-K3", "fp32"])
def test_load_indexed_refuses_malformed_tensors(dtype, K, prefix):
    e = _engine(dtype, K)
    x, y, idx = _dataset(IMG, K)
    xs, ys, _ = _dataset(24, K)
    code = torch.tensor([1, 6], dtype=torch.int32)
    affine = torch.rand(B, CIN, 2)
    origin = torch.zeros(B, 3, dtype=torch.int32)
    mat = torch.tensor([[65536, 0, 0, 65536]] * B, dtype=torch.int32)
    crop = (origin, (1, 16, 16))
    codes = "augmentation codes: a contiguous int32 [2] tensor on cpu"
    affines = "augmentation affine: a contiguous float32 [2][4][2] tensor on cpu"
    origins = "crop origins: a contiguous int32 [2][3] tensor on cpu"
    mats = "warp matrices: a contiguous int32 [2][4] tensor on cpu"
    bad = [
        (codes, (x, y), dict(aug=(code.long(), affine))),
        (codes, (xs, ys), dict(aug=(code.long(), None), crop=crop)),
        (codes, (xs, ys), dict(aug=(code.long(), None, mat), crop=crop)),
        (affines, (x, y), dict(aug=(code, affine[:, :3]))),
        (affines, (xs, ys), dict(aug=(None, affine[:, :3].contiguous()), crop=crop)),
        (affines, (xs, ys), dict(aug=(None, torch.rand(B, CIN, 3), mat), crop=crop)),
        (origins, (xs, ys), dict(crop=(origin[:1], (1, 16, 16)))),
        (origins, (xs, ys), dict(aug=(None, None, mat), crop=(torch.zeros(B, 2, dtype=torch.int32), (1, 16, 16)))),
        (mats, (xs, ys), dict(aug=(code, None, mat[:, :3].contiguous()), crop=crop)),
        (mats, (xs, ys), dict(aug=(None, None, torch.zeros(B, 2, 2, dtype=torch.int32)))),
        ("crop patch (1, 8, 8): the executor's input is (1, 16, 16)", (xs, ys), dict(crop=(origin, (1, 8, 8)))),
        ("the executor's input (1, 16, 16) exceeds the stored sample (1, 8, 8)",
         (x[:, :8, :8].contiguous(), y[:, :8, :8].contiguous()), dict(aug=(None, None, mat))),
    ]
    for message, (xa, ya), kw in bad:
        with pytest.raises(ValueError) as err:
            e.load_indexed(xa, ya, idx, STREAM, **kw)
        assert str(err.value) == message, kw
    assert e.C.calls == []
