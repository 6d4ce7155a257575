"""CLI flag surface.

Accepts every flag the reference trainer defines with ``tf.app.flags``
(`test_dist.py:64-85`) with the same names, types and defaults, plus the
README-only spellings (`README.md:63-71`) as aliases, plus the extensions the
MI355X framework adds (dtype, norm, dims, synthetic data, ...).

Boolean flags follow absl/``tf.app.flags`` conventions so that reference
command lines keep working: ``--use_upsampling``, ``--use_upsampling=True``,
``--use_upsampling=false`` and ``--nouse_upsampling`` are all accepted.
"""

import argparse
import dataclasses
import socket
from typing import List, Optional

from . import settings


def _str2bool(v):
    if isinstance(v, bool):
        return v
    s = str(v).strip().lower()
    if s in ("1", "true", "t", "yes", "y", "on"):
        return True
    if s in ("0", "false", "f", "no", "n", "off"):
        return False
    raise argparse.ArgumentTypeError("expected a boolean, got %r" % v)


def _default_ip():
    try:
        return socket.gethostbyname(socket.gethostname())
    except OSError:
        return "127.0.0.1"


@dataclasses.dataclass
class Config:
    # --- reference flags (test_dist.py:64-85) ---
    const_learningrate: bool = settings.CONST_LEARNINGRATE
    learning_rate: float = settings.LEARNINGRATE
    lr_fraction: float = settings.LR_FRACTION
    decay_steps: int = settings.DECAY_STEPS
    is_sync: int = 1
    ip: str = "127.0.0.1"
    batch_size: int = settings.BATCH_SIZE          # GLOBAL batch, split over ranks
    epochs: int = settings.EPOCHS
    use_upsampling: bool = settings.USE_UPSAMPLING
    # --- README-only flags (README.md:63-66): host loader threads on GPU ---
    num_threads: int = settings.NUM_INTRA_THREADS
    num_inter_threads: int = settings.NUM_INTER_THREADS
    blocktime: int = settings.BLOCKTIME
    # --- extensions ---
    dtype: str = "bf16"              # fp32 | bf16 | fp16 (compute dtype)
    norm: str = "none"               # none | batch | group
    groups: int = 8                  # GroupNorm groups
    dims: int = 2                    # 2 | 3
    in_channels: int = settings.IN_CHANNEL_NO
    out_channels: int = settings.OUT_CHANNEL_NO
    img_size: int = settings.IMG_ROWS
    base_filters: int = 32
    depth: int = 4
    dropout: float = 0.2
    eval_dropout: bool = False       # reference keeps dropout on at eval (Q9)
    loss: str = "dice"               # dice | dice_bce
    bce_weight: float = 1.0
    mode: int = settings.MODE
    synthetic: bool = False
    synthetic_train: int = 2048
    synthetic_test: int = 256
    synthetic_difficulty: str = "easy"   # easy | hard (datasets.synthetic_brats)
    synthetic_size: int = 0          # stored side of the synthetic train / test images (0: img_size)
    data_on_device: str = "auto"     # auto | on | off: keep the train set resident in HBM
    data_path: str = settings.OUT_PATH
    steps: int = 0                   # >0 overrides epochs*num_batches
    seed: int = 816
    checkpoint_dir: str = settings.CHECKPOINT_DIRECTORY
    save_model_secs: float = 60.0
    no_checkpoint: bool = False
    resume: bool = True
    bucket_mb: float = 8.0
    overlap_comm: bool = True
    backend: str = "auto"            # auto | native | torch
    device: str = "auto"             # auto | cuda | cpu
    dist_backend: str = "auto"       # auto | nccl | gloo
    dist_timeout_s: float = 300.0
    profile: bool = False
    profile_steps: str = "5,10"
    log_every: int = 10
    log_jsonl: str = ""
    tensorboard: bool = True
    export: bool = True
    fault_inject_step: int = -1
    fault_inject_rank: int = -1
    fault_inject_overflow_step: int = -1   # fp16 test hook: poison this step's gradient
    check_sync_every: int = 0        # cross-rank parameter checksum every K steps
    deterministic: bool = False      # torch path: deterministic algorithms (native path always is)
    serialize_kernels: bool = False  # debug: AMD_SERIALIZE_KERNEL=3 + HIP_LAUNCH_BLOCKING=1
    launch_tensorboard: bool = False # start `tensorboard --logdir` on the chief if installed
    hip_graph: bool = True           # native: replay the forward / Adam as HIP graphs (the bench default)
    progress: bool = True
    loss_scale: float = 0.0          # fp16 static loss scale (0 = dynamic)
    eval_threshold: float = 0.5      # probability threshold of the per-case (hard) evaluation metrics
    eval_hd95: bool = False          # evaluation also reports the per-case 95th-percentile Hausdorff distance
    augment: str = ""                # training batches only: comma-separated subset of flip, rot90, intensity, rotate, scale, elastic, rotate3d, scale3d
    augment_intensity: float = 0.1   # intensity: scale in [1-a, 1+a], shift in [-a, a] per (sample, channel)
    augment_rotate: float = 30.0     # rotate: angle uniform in [-r, r] degrees per sample, r in (0, 180]
    augment_scale: float = 0.25      # scale: zoom log-uniform in [1/(1+a), 1+a] per sample, a in (0, 1]
    augment_rotate3d: float = 15.0   # rotate3d: the two out-of-plane angles uniform in [-r, r] degrees, r in (0, 180]
    augment_elastic: float = 4.0     # elastic: standard deviation of a control node's displacement, stored-image pixels
    augment_elastic_cell: int = 32   # elastic: side of a control-lattice cell in patch pixels, 8, 16, 32 or 64
    eval_tta: str = ""               # evaluation only: mean prediction over flip and / or rot90 (comma-separated)
    eval_components: str = ""        # evaluation only: connected-component filter, comma list of largest, min:V
    crop: str = ""                   # training patches of img_size from larger stored images: random | foreground[:P]
    eval_overlap: float = 0.5        # sliding-window evaluation (test images not of the model's size): window overlap
    eval_blend: str = "gaussian"     # ... and window weighting: constant | gaussian

    @property
    def method_up(self):
        return "upsample2D" if self.use_upsampling else "conv2DTranspose"


_BOOL_FLAGS = [f.name for f in dataclasses.fields(Config) if f.type in (bool, "bool")]

_ALIASES = {
    "learningrate": "learning_rate",   # README.md:68
}

_CHOICES = {
    "dtype": ("fp32", "bf16", "fp16"),
    "norm": ("none", "batch", "group"),
    "loss": ("dice", "dice_bce"),
    "backend": ("auto", "native", "torch"),
    "device": ("auto", "cuda", "cpu"),
    "dist_backend": ("auto", "nccl", "gloo"),
    "data_on_device": ("auto", "on", "off"),
    "synthetic_difficulty": ("easy", "hard"),
    "eval_blend": ("constant", "gaussian"),
}


AUGMENT_NAMES = ("flip", "rot90", "intensity", "rotate", "scale", "elastic", "rotate3d", "scale3d")
SPATIAL_NAMES = ("rotate", "scale")  # the transforms that resample the image (data/augment.py draw_spatial)
SPATIAL3_NAMES = ("rotate3d", "scale3d")  # ... through a 3 x 3 matrix over (d, h, w), --dims 3 (draw_spatial3)
ELASTIC_CELLS = (8, 16, 32, 64)      # --augment_elastic_cell (data/augment.py draw_elastic)


def parse_augment(s: str) -> tuple:
    """The --augment string as a tuple of transform names; an unknown or repeated name
    is a SystemExit that names it."""
    names = [t.strip() for t in str(s).split(",")] if str(s).strip() else []
    for i, t in enumerate(names):
        if t not in AUGMENT_NAMES:
            raise SystemExit("--augment: unknown transform %r (choose from %s)" % (t, ", ".join(AUGMENT_NAMES)))
        if t in names[:i]:
            raise SystemExit("--augment: %r is listed twice" % t)
    return tuple(names)


TTA_NAMES = ("flip", "rot90")


def parse_tta(s: str) -> tuple:
    """The --eval_tta string as a tuple of transform names (the geometric ones of --augment);
    an unknown or repeated name is a SystemExit that names it."""
    names = [t.strip() for t in str(s).split(",")] if str(s).strip() else []
    for i, t in enumerate(names):
        if t not in TTA_NAMES:
            raise SystemExit("--eval_tta: unknown transform %r (choose from %s)" % (t, ", ".join(TTA_NAMES)))
        if t in names[:i]:
            raise SystemExit("--eval_tta: %r is listed twice" % t)
    return tuple(names)


def parse_components(s: str) -> tuple:
    """The --eval_components string as the policy (keep_largest, min_size): a comma list of
    `largest` and / or `min:V` (V >= 1 voxels); "" is (False, 0), the filter off.  An unknown,
    malformed or repeated item is a SystemExit that names it."""
    items = [t.strip() for t in str(s).split(",")] if str(s).strip() else []
    largest, min_size, seen = False, 0, []
    for t in items:
        name = t.split(":", 1)[0]
        if t == "largest":
            largest = True
        elif name == "min" and ":" in t:
            v = t.split(":", 1)[1].strip()
            if not v.isdigit() or int(v) < 1:
                raise SystemExit("--eval_components: min:V takes a voxel count V >= 1, got %r" % t)
            if int(v) >= 1 << 31:
                raise SystemExit("--eval_components: min:V below 2^31, got %r" % t)
            min_size = int(v)
        else:
            raise SystemExit("--eval_components: unknown item %r (choose from largest, min:V)" % t)
        if name in seen:
            raise SystemExit("--eval_components: %r is listed twice" % name)
        seen.append(name)
    return largest, min_size


CROP_MODES = ("random", "foreground")
CROP_P_FG = 1.0 / 3.0                # plain `foreground`: the share of patches forced to hold foreground


def parse_crop(s: str) -> tuple:
    """The --crop string as (mode, p_fg): "" is ("", 0.0), cropping off; `random` is
    ("random", 0.0); `foreground` or `foreground:P` (P in (0, 1], default 1/3) is
    ("foreground", P).  An unknown, malformed or repeated item is a SystemExit that names it."""
    items = [t.strip() for t in str(s).split(",")] if str(s).strip() else []
    if not items:
        return "", 0.0
    if len(items) > 1:
        raise SystemExit("--crop: one mode, %r is listed after %r" % (items[1], items[0]))
    t = items[0]
    name, _, v = t.partition(":")
    if name not in CROP_MODES or (":" in t and name != "foreground"):
        raise SystemExit("--crop: unknown item %r (choose from random, foreground, foreground:P)" % t)
    if name == "random":
        return "random", 0.0
    if ":" not in t:
        return "foreground", CROP_P_FG
    try:
        p = float(v)
    except ValueError:
        p = float("nan")
    if not 0.0 < p <= 1.0:
        raise SystemExit("--crop: foreground:P takes a probability P in (0, 1], got %r" % t)
    return "foreground", p


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        description="MI355X-native distributed UNet trainer "
                    "(flag-compatible with the reference test_dist.py)")
    defaults = Config()
    for f in dataclasses.fields(Config):
        name = f.name
        default = getattr(defaults, name)
        if name in _BOOL_FLAGS:
            p.add_argument("--" + name, dest=name, nargs="?", const=True,
                           default=default, type=_str2bool)
            p.add_argument("--no" + name, dest=name, action="store_false")
        else:
            kw = dict(dest=name, default=default, type=type(default))
            if name in _CHOICES:
                kw["choices"] = _CHOICES[name]
            p.add_argument("--" + name, **kw)
    for alias, target in _ALIASES.items():
        p.add_argument("--" + alias, dest=target, type=float,
                       default=argparse.SUPPRESS)
    return p


def parse_args(argv: Optional[List[str]] = None) -> Config:
    ns, unknown = build_parser().parse_known_args(argv)
    if unknown:
        raise SystemExit("unrecognised flags: %s" % " ".join(unknown))
    cfg = Config(**vars(ns))
    validate(cfg)
    return cfg


def validate(cfg: Config) -> None:
    if cfg.dims not in (2, 3):
        raise SystemExit("--dims must be 2 or 3")
    if cfg.img_size % (1 << cfg.depth) != 0:
        raise SystemExit("--img_size must be divisible by 2**depth")
    if cfg.batch_size <= 0:
        raise SystemExit("--batch_size must be positive")
    if not 0.0 <= cfg.dropout < 1.0:
        raise SystemExit("--dropout must be in [0, 1)")
    if not 1 <= cfg.out_channels <= 4:
        raise SystemExit("--out_channels must be 1..4")
    if not 0.0 < cfg.eval_threshold < 1.0:
        raise SystemExit("--eval_threshold must lie strictly inside (0, 1)")
    parse_augment(cfg.augment)
    parse_tta(cfg.eval_tta)
    parse_components(cfg.eval_components)
    parse_crop(cfg.crop)
    if cfg.synthetic_size < 0:
        raise SystemExit("--synthetic_size must be >= 0 (0: --img_size)")
    from .ops.sliding import check_overlap
    try:
        check_overlap(cfg.eval_overlap)
    except ValueError as e:
        raise SystemExit("--eval_overlap: %s" % e)
    if cfg.eval_blend not in _CHOICES["eval_blend"]:
        raise SystemExit("--eval_blend must be constant or gaussian")
    if not 0.0 <= cfg.augment_intensity < 1.0:
        raise SystemExit("--augment_intensity must be in [0, 1)")
    if not 0.0 < cfg.augment_rotate <= 180.0:
        raise SystemExit("--augment_rotate must be in (0, 180]: the largest angle in degrees, got %r"
                         % (cfg.augment_rotate,))
    if not 0.0 < cfg.augment_scale <= 1.0:
        raise SystemExit("--augment_scale must be in (0, 1]: the zoom is drawn from [1/(1+a), 1+a], got %r"
                         % (cfg.augment_scale,))
    if not 0.0 < cfg.augment_rotate3d <= 180.0:
        raise SystemExit("--augment_rotate3d must be in (0, 180]: the largest out-of-plane angle in degrees, got %r"
                         % (cfg.augment_rotate3d,))
    names = parse_augment(cfg.augment)
    for t in SPATIAL3_NAMES:
        if t in names and cfg.dims != 3:
            raise SystemExit("--augment %s needs --dims 3 (it resamples along depth), got --dims %d" % (t, cfg.dims))
    if "rotate" in names and "rotate3d" in names:
        raise SystemExit("--augment: rotate together with rotate3d (rotate3d includes the in-plane rotation)")
    if "scale" in names and "scale3d" in names:
        raise SystemExit("--augment: scale together with scale3d (scale3d includes the in-plane zoom)")
    if "elastic" in names:
        # node values are truncated at +-2a, so neighbouring nodes differ by at most 4a and the
        # quadratic B-spline's derivative is at most 4a / S: a <= S / 8 keeps it within 1/2
        S, a = cfg.augment_elastic_cell, cfg.augment_elastic
        if S not in ELASTIC_CELLS:
            raise SystemExit("--augment_elastic_cell must be one of %s, got %r" % (", ".join(map(str, ELASTIC_CELLS)), S))
        if not a > 0.0:
            raise SystemExit("--augment_elastic must be positive: the nodes' standard deviation in pixels, got %r" % (a,))
        if not a <= S / 8.0:
            raise SystemExit("--augment_elastic must be at most --augment_elastic_cell / 8 = %g (the displacement's "
                             "gradient stays within 1/2), got %r" % (S / 8.0, a))
    if cfg.mode == 5 and cfg.out_channels > 3:
        raise SystemExit("--mode 5 has three nested regions: --out_channels must be 1..3")
