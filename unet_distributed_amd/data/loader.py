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

from .augment import apply_torch, crop_torch, elastic_torch, warp3_torch, warp_torch


class BatchLoader:
    def __init__(self, x: np.ndarray, y: np.ndarray, per_rank: int, threads: int = 8, pin: bool = False,
                 patch=None):
        """`patch`: optional (D, H, W) of the training patches (--crop): the staging buffers
        are patch-sized and `gather` takes the patch origins."""
        self.x, self.y = x, y
        self.threads = max(1, int(threads))
        self.patch = None if patch is None else tuple(int(v) for v in patch)
        sp = tuple(x.shape[1:-1]) if patch is None else self.patch[3 - (x.ndim - 2):]
        self.bx = torch.empty((per_rank,) + sp + (x.shape[-1],), dtype=torch.float32, pin_memory=pin)
        self.by = torch.empty((per_rank,) + sp + (y.shape[-1],), dtype=torch.float32, pin_memory=pin)
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

    def _gather_patches(self, src: np.ndarray, idx: np.ndarray, origin: np.ndarray, dst: torch.Tensor):
        """dst[i] = the patch of sample idx[i] at origin[i]: only the slice is read and copied."""
        out = dst.numpy()
        D, H, W = self.patch
        for i, (n, (d, h, w)) in enumerate(zip(idx, origin)):
            out[i] = src[n, d:d + D, h:h + H, w:w + W] if src.ndim == 5 else src[n, h:h + H, w:w + W]

    def gather(self, idx: np.ndarray, origin=None):
        """`origin` (a patch loader): int [n][3] patch origins of the samples `idx`, which are
        taken in the order given (the feeder's sorted order)."""
        if self.patch is not None:
            if origin is None or len(origin) != len(idx):
                raise ValueError("patch loader: one origin per sample")
            idx, origin = np.asarray(idx), np.asarray(origin).reshape(-1, 3)
            self._gather_patches(self.x, idx, origin, self.bx)
            self._gather_patches(self.y, idx, origin, self.by)
            return self.bx, self.by
        idx = np.sort(np.asarray(idx))
        self._gather(self.x, idx, self.bx)
        self._gather(self.y, idx, self.by)
        return self.bx, self.by


class ResidentBatch:
    """A batch of the HBM-resident dataset named by sample index: the native backend
    gathers and casts it into its input buffers in one kernel; anything else asks
    for the tensors.  `aug`: optional augmentation parameters of the batch on the
    device, (code int32 [n], affine float32 [n][Cin][2] or None) (data/augment.py).  `crop`:
    optional (origin int32 [n][3] on the device, patch dims (D, H, W)): the batch is the patch
    of each stored sample at its origin (--crop), cropped before it is augmented.  An `aug` of three
    items ends in the warp matrices (mat int32 [n][4], --augment rotate / scale): the patch, or the
    whole sample without `crop`, is resampled through them straight from the stored sample (mat int32
    [n][9], --augment rotate3d / scale3d: trilinearly, through the 3 x 3 matrices).  An `aug`
    of four items (code, affine, mat or None, field int32 [n][N][N][2], --augment elastic) adds the
    elastic displacement of each sample's field, a lattice of `elastic_cell` patch pixels per cell."""

    def __init__(self, x_all: torch.Tensor, y_all: torch.Tensor, idx: torch.Tensor, aug=None, crop=None,
                 elastic_cell: int = 32):
        self.x_all, self.y_all, self.idx = x_all, y_all, idx
        self.aug = aug
        self.crop = crop
        self.elastic_cell = int(elastic_cell)

    def tensors(self):
        x, y = self.x_all.index_select(0, self.idx), self.y_all.index_select(0, self.idx)
        if self.aug is not None and len(self.aug) > 3:
            return elastic_batch(x, y, self.crop, *self.aug, S=self.elastic_cell)
        if self.aug is not None and len(self.aug) > 2 and self.aug[2] is not None:
            return warp_batch(x, y, self.crop, *self.aug)
        if self.crop is not None:
            x, y = crop_torch(x, y, *self.crop)
        if self.aug is not None:
            x, y = apply_torch(x, y, *self.aug)
        return x, y

    @property
    def npix(self) -> int:
        if self.crop is not None:
            d, h, w = self.crop[1]
            return int(self.idx.numel()) * d * h * w * int(self.y_all.shape[-1])
        return int(self.idx.numel()) * int(self.y_all[0].numel())


def is_mat3(mat) -> bool:
    """Whether `mat` holds draw_spatial3's 3 x 3 matrices, [n][9], not the in-plane [n][4] ones."""
    return mat is not None and len(mat.shape) == 2 and int(mat.shape[1]) == 9


def warp_batch(x, y, crop, code, affine, mat):
    """The training transform with warp matrices on the samples x [n, (Ds,) Hs, Ws, C] and y of a
    batch: `crop` = (origin [n][3], patch dims) or None (the whole sample at origin 0), then
    warp_torch -- warp3_torch for matrices of 9 entries (--augment rotate3d / scale3d) -- then
    apply_torch(code or the identity, affine)."""
    origin, patch = crop if crop is not None else (None, tuple(x.shape[1:-1]))
    x, y = warp3_torch(x, y, origin, patch, mat) if is_mat3(mat) else warp_torch(x, y, origin, patch, mat)
    return apply_torch(x, y, code if code is not None else np.zeros(x.shape[0], dtype=np.int32), affine)


def elastic_batch(x, y, crop, code, affine, mat, field, S: int = 32):
    """warp_batch with an elastic field (cells of S patch pixels): elastic_torch, whose `mat` may be
    None (the identity) -- warp3_torch with the field for matrices of 9 entries -- then
    apply_torch(code or the identity, affine)."""
    origin, patch = crop if crop is not None else (None, tuple(x.shape[1:-1]))
    if is_mat3(mat):
        x, y = warp3_torch(x, y, origin, patch, mat, (field, S))
    else:
        x, y = elastic_torch(x, y, origin, patch, mat, field, S)
    return apply_torch(x, y, code if code is not None else np.zeros(x.shape[0], dtype=np.int32), affine)


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
                 mode: str = "auto", budget_frac: float = 0.25, patch=None, elastic_cell: int = 32):
        """`patch`: optional (D, H, W) of the training patches (--crop): every batch is then
        cut out of the stored samples at the origins its `aug` callable returns.  `elastic_cell`:
        the cell side of the fields an `aug` callable may return (--augment_elastic_cell)."""
        self.device = torch.device(device)
        self.elastic_cell = int(elastic_cell)
        self.per_rank = per_rank
        self.patch = None if patch is None else tuple(int(v) for v in patch)
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
        self.loaders = [BatchLoader(x, y, per_rank, threads, pin, self.patch) for _ in range(2 if pin else 1)]
        self.events = [None] * len(self.loaders)
        self.k = 0

    def _upload(self, sorted_idx: np.ndarray, code: np.ndarray, affine, origin=None, mat=None, field=None):
        """Index tensor and augmentation parameters in one small non-blocking copy:
        [idx int64 | affine fp32 | code int32 | origin int32 | mat int32 | field int32] ->
        (idx, (code, affine)) device views, and with `origin` (int [n][3], --crop) the origin view
        as a third item.  With `mat` (int [n][4], --augment rotate / scale, or [n][9], rotate3d /
        scale3d: the rows keep their width) the second item is
        (code, affine, mat); with `field` (int [n][N][N][2], --augment elastic) it is (code, affine,
        mat or None, field): the field rides at the end, every other view keeps its offset."""
        n = len(sorted_idx)
        af = np.ascontiguousarray(affine, dtype=np.float32) if affine is not None else np.empty(0, np.float32)
        parts = [sorted_idx.view(np.uint8), af.reshape(-1).view(np.uint8),
                 np.ascontiguousarray(code, dtype=np.int32).view(np.uint8)]
        if origin is not None:
            parts.append(np.ascontiguousarray(origin, dtype=np.int32).reshape(-1).view(np.uint8))
        if mat is not None:
            mat = np.ascontiguousarray(mat, dtype=np.int32).reshape(n, -1)
            parts.append(mat.reshape(-1).view(np.uint8))
        if field is not None:
            field = np.ascontiguousarray(field, dtype=np.int32)
            parts.append(field.reshape(-1).view(np.uint8))
        buf = torch.from_numpy(np.concatenate(parts)).to(self.device, non_blocking=True)
        na = parts[1].size
        ii = buf[:8 * n].view(torch.int64)
        af = buf[8 * n:8 * n + na].view(torch.float32).view(affine.shape) if affine is not None else None
        cd = buf[8 * n + na:8 * n + na + 4 * n].view(torch.int32)
        at = 8 * n + na + 4 * n
        no = 12 * n if origin is not None else 0
        nm = mat.nbytes if mat is not None else 0
        dev = (cd, af) if mat is None else (cd, af, buf[at + no:at + no + nm].view(torch.int32).view(mat.shape))
        if field is not None:
            dev = dev[:2] + (dev[2] if mat is not None else None,
                             buf[at + no + nm:at + no + nm + field.nbytes].view(torch.int32).view(field.shape))
        if origin is None:
            return ii, dev
        return ii, dev, buf[at:at + no].view(torch.int32).view(n, 3)

    def get(self, idx: np.ndarray, lazy: bool = False, aug=None):
        """(x, y) of the samples `idx`; lazy (resident data only): a ResidentBatch
        for a backend that gathers it itself.  `aug`: optional callable, sorted dataset
        sample indices -> (code, affine) (data/augment.py): the batch is augmented with
        them (a ResidentBatch carries them for the backend's gather kernel).  A feeder with
        `patch` needs `aug` to return (code, affine, origin) (augment.make_crop_aug): the batch
        is the patches at the origins, cropped first and then augmented.  Either tuple may end in
        the warp matrices `mat` (--augment rotate / scale): the batch is then resampled through
        them straight from the stored samples (augment.warp_torch; the backend's gather kernel
        for a ResidentBatch).  With --augment elastic the tuples are (code, affine, mat or None,
        field) and (code, affine, origin, mat or None, field) (augment.elastic_torch)."""
        if aug is None:
            if self.patch is not None:
                raise ValueError("a cropping feeder needs the per-step origins (aug)")
            return self._get(idx, lazy)
        si = np.sort(np.asarray(idx, dtype=np.int64))       # (the order every path below feeds)
        drawn = aug(si)
        if self.patch is not None:
            return self._get_crop(si, lazy, *drawn)
        code, affine, mat, field = (tuple(drawn) + (None, None))[:4]
        if self.resident:
            ii, dev = self._upload(si, code, affine, mat=mat, field=field)
            if lazy:
                return ResidentBatch(self.x, self.y, ii, dev, elastic_cell=self.elastic_cell), None
            x, y = self.x.index_select(0, ii), self.y.index_select(0, ii)
        else:
            x, y = self._get(idx, False)
        if field is not None:
            return elastic_batch(x, y, None, code, affine, mat, field, self.elastic_cell)
        return apply_torch(x, y, code, affine) if mat is None else warp_batch(x, y, None, code, affine, mat)

    def _get_crop(self, si: np.ndarray, lazy: bool, code, affine, origin, mat=None, field=None):
        origin = np.ascontiguousarray(origin, dtype=np.int32).reshape(len(si), 3)
        if self.resident:
            ii, dev, org = self._upload(si, code, affine, origin, mat, field)
            if lazy:
                return ResidentBatch(self.x, self.y, ii, dev, (org, self.patch), self.elastic_cell), None
            x, y = self.x.index_select(0, ii), self.y.index_select(0, ii)
            if field is not None:
                return elastic_batch(x, y, (origin, self.patch), code, affine, mat, field, self.elastic_cell)
            if mat is not None:
                return warp_batch(x, y, (origin, self.patch), code, affine, mat)
            return apply_torch(*crop_torch(x, y, origin, self.patch), code, affine)
        if mat is not None or field is not None:
            # streamed and warped: the taps leave the patch rectangle, so the host resamples the
            # whole stored samples and only the patches are copied to the device
            ld = self.loaders[0]
            x = torch.from_numpy(np.ascontiguousarray(ld.x[si], dtype=np.float32))
            y = torch.from_numpy(np.ascontiguousarray(ld.y[si], dtype=np.float32))
            if field is not None:
                x, y = elastic_batch(x, y, (origin, self.patch), code, affine, mat, field, self.elastic_cell)
            else:
                x, y = warp_batch(x, y, (origin, self.patch), code, affine, mat)
            return x.to(self.device), y.to(self.device)
        # streamed: the host copies each sample's patch into the patch-sized staging buffers
        return apply_torch(*self._get(si, False, origin), code, affine)

    def _get(self, idx: np.ndarray, lazy: bool, origin=None):
        if self.resident:
            ii = torch.from_numpy(np.sort(np.asarray(idx, dtype=np.int64))).to(self.device, non_blocking=True)
            if lazy:
                return ResidentBatch(self.x, self.y, ii), None
            return self.x.index_select(0, ii), self.y.index_select(0, ii)
        k = self.k
        self.k = (self.k + 1) % len(self.loaders)
        if self.events[k] is not None:
            self.events[k].synchronize()        # the copy that last read this buffer is done
        bx, by = self.loaders[k].gather(idx, origin) if origin is not None else self.loaders[k].gather(idx)
        if self.device.type != "cuda":
            return bx.clone(), by.clone()
        gx = bx.to(self.device, non_blocking=True)
        gy = by.to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k] = ev
        return gx, gy
