"""Host batch loader: gathers a per-rank shard's samples into a (pinned) staging
buffer with the native multi-threaded row gather (``_C.gather_rows``), falling
back to numpy fancy indexing when the extension is unavailable.

Replaces the reference's full in-memory epoch materialisation (`data.py:29-54`
builds the whole shuffled epoch array every epoch): only the current batch is
copied, straight from the memory-mapped ``.npy`` arrays, with index order sorted
for sequential reads.  ``--num_threads`` (README.md:63) sizes the gather pool.
"""

import numpy as np
import torch

from .augment import apply_torch


class BatchLoader:
    def __init__(self, x: np.ndarray, y: np.ndarray, per_rank: int, threads: int = 8, pin: bool = False):
        self.x, self.y = x, y
        self.threads = max(1, int(threads))
        self.bx = torch.empty((per_rank,) + tuple(x.shape[1:]), dtype=torch.float32, pin_memory=pin)
        self.by = torch.empty((per_rank,) + tuple(y.shape[1:]), dtype=torch.float32, pin_memory=pin)
        self._native = None
        try:
            from .. import native
            if native.available():
                self._native = native.lib()
        except Exception:
            self._native = None

    def _gather(self, src: np.ndarray, idx: np.ndarray, dst: torch.Tensor):
        n = len(idx)
        if (self._native is not None and src.dtype == np.float32 and src.flags.c_contiguous
                and dst.is_contiguous()):
            row = int(np.prod(src.shape[1:])) * 4
            ii = np.ascontiguousarray(idx, dtype=np.int64)
            self._native.gather_rows(src.ctypes.data, ii.ctypes.data, n, row, dst.data_ptr(), self.threads)
        else:
            dst.numpy()[:n] = src[idx]

    def gather(self, idx: np.ndarray):
        idx = np.sort(np.asarray(idx))
        self._gather(self.x, idx, self.bx)
        self._gather(self.y, idx, self.by)
        return self.bx, self.by


class ResidentBatch:
    """A batch of the HBM-resident dataset named by sample index: the native backend
    gathers and casts it into its input buffers in one kernel; anything else asks
    for the tensors.  `aug`: optional augmentation parameters of the batch on the
    device, (code int32 [n], affine float32 [n][Cin][2] or None) (data/augment.py)."""

    def __init__(self, x_all: torch.Tensor, y_all: torch.Tensor, idx: torch.Tensor, aug=None):
        self.x_all, self.y_all, self.idx = x_all, y_all, idx
        self.aug = aug

    def tensors(self):
        x, y = self.x_all.index_select(0, self.idx), self.y_all.index_select(0, self.idx)
        if self.aug is not None:
            x, y = apply_torch(x, y, *self.aug)
        return x, y

    @property
    def npix(self) -> int:
        return int(self.idx.numel()) * int(self.y_all[0].numel())


class DeviceFeeder:
    """Per-step batches on the training device.

    * ``resident`` (MI355X default): the whole training set is uploaded to HBM
      once (a BraTS 2016 slice set is a few GB against 288 GB per GPU) and each
      step's shard is one on-device ``index_select`` -- no host gather, no PCIe
      traffic on the hot path.
    * ``streamed``: :class:`BatchLoader` gathers into one of two pinned staging
      buffers and copies asynchronously; a HIP event per buffer keeps the host
      from overwriting a buffer whose copy has not executed yet (the host runs
      ahead of the GPU by several steps when nothing synchronises).
    """

    def __init__(self, x: np.ndarray, y: np.ndarray, per_rank: int, device, threads: int = 8,
                 mode: str = "auto", budget_frac: float = 0.25):
        self.device = torch.device(device)
        self.per_rank = per_rank
        nbytes = (x.size + y.size) * 4
        resident = False
        if self.device.type == "cuda":
            if mode == "on":
                resident = True
            elif mode == "auto":
                total = torch.cuda.get_device_properties(self.device).total_memory
                resident = nbytes <= budget_frac * total
        self.resident = resident
        if resident:
            self.x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
            self.y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(self.device)
            return
        pin = self.device.type == "cuda"
        self.loaders = [BatchLoader(x, y, per_rank, threads, pin) for _ in range(2 if pin else 1)]
        self.events = [None] * len(self.loaders)
        self.k = 0

    def _upload(self, sorted_idx: np.ndarray, code: np.ndarray, affine):
        """Index tensor and augmentation parameters in one small non-blocking copy:
        [idx int64 | affine fp32 | code int32] -> (idx, (code, affine)) device views."""
        n = len(sorted_idx)
        af = np.ascontiguousarray(affine, dtype=np.float32) if affine is not None else np.empty(0, np.float32)
        parts = [sorted_idx.view(np.uint8), af.reshape(-1).view(np.uint8),
                 np.ascontiguousarray(code, dtype=np.int32).view(np.uint8)]
        buf = torch.from_numpy(np.concatenate(parts)).to(self.device, non_blocking=True)
        na = parts[1].size
        ii = buf[:8 * n].view(torch.int64)
        af = buf[8 * n:8 * n + na].view(torch.float32).view(affine.shape) if affine is not None else None
        return ii, (buf[8 * n + na:].view(torch.int32), af)

    def get(self, idx: np.ndarray, lazy: bool = False, aug=None):
        """(x, y) of the samples `idx`; lazy (resident data only): a ResidentBatch
        for a backend that gathers it itself.  `aug`: optional callable, sorted dataset
        sample indices -> (code, affine) (data/augment.py): the batch is augmented with
        them (a ResidentBatch carries them for the backend's gather kernel)."""
        if aug is None:
            return self._get(idx, lazy)
        si = np.sort(np.asarray(idx, dtype=np.int64))       # (the order every path below feeds)
        code, affine = aug(si)
        if self.resident:
            ii, dev = self._upload(si, code, affine)
            if lazy:
                return ResidentBatch(self.x, self.y, ii, dev), None
            return apply_torch(self.x.index_select(0, ii), self.y.index_select(0, ii), code, affine)
        return apply_torch(*self._get(idx, False), code, affine)

    def _get(self, idx: np.ndarray, lazy: bool):
        if self.resident:
            ii = torch.from_numpy(np.sort(np.asarray(idx, dtype=np.int64))).to(self.device, non_blocking=True)
            if lazy:
                return ResidentBatch(self.x, self.y, ii), None
            return self.x.index_select(0, ii), self.y.index_select(0, ii)
        k = self.k
        self.k = (self.k + 1) % len(self.loaders)
        if self.events[k] is not None:
            self.events[k].synchronize()        # the copy that last read this buffer is done
        bx, by = self.loaders[k].gather(idx)
        if self.device.type != "cuda":
            return bx.clone(), by.clone()
        gx = bx.to(self.device, non_blocking=True)
        gy = by.to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k] = ev
        return gx, gy
