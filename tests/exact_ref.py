"""Exact integer-operand references for the conv / data-gradient / weight-gradient kernels.

Every GEMM in those kernels is products of 16-bit operands (fp32 x fp32 in the fp32
executor) accumulated in fp32.  With small integer operands and sum |x||w| + |b| < 2^24
every partial sum is an integer fp32 holds exactly, whatever the order of MFMAs, waves,
LDS reductions and split-K slabs: the fp32 result is the mathematical result and the
stored value its round-to-nearest-even image in the storage type.  A float64 CPU reference
then predicts every output bit.

Plain helper module (imported like ``test_gpu_kernels``): operand generators, the guards
that keep a case inside the exact regime, float64 references of the linear ops, and the
operand / reference builders of every case tests/test_gpu_exact.py launches (so that
tests/test_exact_ref_cpu.py checks their input conditions without a GPU).
"""

import functools
import zlib

import torch
import torch.nn.functional as F

EXACT = float(2 ** 24)
FP16_MAX = 65504.0
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_DROP = {torch.bfloat16: 16, torch.float16: 13, torch.float32: 0}     # fp32 mantissa bits the store drops


def _dt(dtype):
    return DTYPES[dtype] if isinstance(dtype, str) else dtype


def _gen(seed):
    return torch.Generator().manual_seed(int(seed) & 0x7FFFFFFF)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


# ----------------------------------------------------------------------------- operands
def ints(seed, shape, lo, hi, density=1.0):
    """Uniform integers in [lo, hi] (closed), float64 on the CPU; `density` < 1 forces the
    other share of the entries to zero (ReLU-like inputs, masks)."""
    g = _gen(seed)
    t = torch.randint(int(lo), int(hi) + 1, tuple(shape), generator=g, dtype=torch.int64).double()
    if density < 1.0:
        t = t * (torch.rand(tuple(shape), generator=g, dtype=torch.float64) < density)
    return t


def nonneg(seed, shape, hi, density=0.5):
    """Post-ReLU activation: integers in [1, hi] on a `density` share of the entries, else 0."""
    return ints(seed, shape, 1, hi, density)


def to_storage(t, dtype, device="cuda"):
    """Lossless cast of a float64 operand (channels-last, as the kernels read it) to the
    storage type, on `device`."""
    dtype = _dt(dtype)
    s = t.to(dtype)
    assert torch.equal(s.double(), t.double()), "operand not representable in %s: max |t| = %g" % (
        dtype, t.abs().max().item())
    return s.contiguous().to(device)


def require_exact(abs_bound, ref64=None, dtype=None):
    """`abs_bound`: the reference routine on absolute values (sum |x||w| + |b| per output).
    Asserts the exact regime; for fp16 outputs also that nothing overflows the format."""
    b = float(torch.as_tensor(abs_bound).abs().max())
    assert b < EXACT, "case leaves the exact regime: sum of |products| up to %.4g >= 2^24" % b
    if dtype is not None and _dt(dtype) == torch.float16:
        assert ref64 is not None
        m = float(ref64.abs().max())
        assert m < FP16_MAX, "fp16 output overflows: max |reference| = %.4g" % m
    return b


def rne(ref64, dtype):
    """Round-to-nearest-even image of an (fp32-exact) float64 reference in `dtype`."""
    r32 = ref64.float()
    assert torch.equal(r32.double(), ref64), "reference is not exact in fp32"
    return r32.to(_dt(dtype))


def _dropped_bits(ref64, dtype):
    r32 = ref64.float()
    assert torch.equal(r32.double(), ref64), "reference is not exact in fp32"
    drop = _DROP[_dt(dtype)]
    low = r32.contiguous().view(torch.int32) & ((1 << drop) - 1)
    return low, drop


def needs_rounding(ref64, dtype):
    """Per element: the value is not representable in `dtype` (normal range)."""
    low, drop = _dropped_bits(ref64, dtype)
    return low != 0


def rounding_share(ref64, dtype):
    """(share not representable in dtype, share that are exact ties) over the non-zero
    reference outputs."""
    low, drop = _dropped_bits(ref64, dtype)
    nz = ref64 != 0
    n = max(int(nz.sum()), 1)
    if drop == 0:
        return 0.0, 0.0
    return float(((low != 0) & nz).sum()) / n, float(((low == (1 << (drop - 1))) & nz).sum()) / n


class BitsMismatch(AssertionError):
    def __init__(self, msg, coords):
        super().__init__(msg)
        self.coords = coords


def assert_bits_equal(out, ref, what, ref64=None, dtype=None, show=8):
    """torch.equal on the values; on failure names the wrong elements: count, the first few
    coordinates (n, [d,] h, w, c) with both values, the float64 value, whether it needed
    rounding and whether the pixel lies on an image border."""
    out, ref = out.detach().cpu(), ref.detach().cpu()
    assert out.shape == ref.shape and out.dtype == ref.dtype, (what, out.shape, ref.shape, out.dtype, ref.dtype)
    if torch.equal(out, ref):
        return
    bad = (out != ref) | (out != out)
    coords = bad.nonzero()
    dtype = _dt(dtype) if dtype is not None else out.dtype
    lines = ["%s: %d of %d elements differ" % (what, coords.shape[0], out.numel())]
    for c in coords[:show].tolist():
        i = tuple(c)
        line = "  %s: kernel %r, reference %r" % (i, out[i].item(), ref[i].item())
        if ref64 is not None and ref64.shape == out.shape:
            v = ref64[i].reshape(1)
            line += ", float64 %r" % v.item()
            if dtype in _DROP and _DROP[dtype]:
                line += ", needs rounding" if bool(needs_rounding(v, dtype)[0]) else ", representable"
        if out.dim() >= 4:
            sp = i[1:-1]
            border = any(k == 0 or k == s - 1 for k, s in zip(sp, out.shape[1:-1]))
            line += ", border pixel" if border else ", interior pixel"
        lines.append(line)
    raise BitsMismatch("\n".join(lines), coords)


# --------------------------------------------------------------------------- references
# float64 on the CPU; activations channels-last [N, (D,) H, W, C], conv weights HWIO
# [(kd,) kh, kw, ci, co], transposed-conv weights in the Keras layout [(kd,) kh, kw, co, ci].
def cfirst(x):
    return x.movedim(-1, 1)


def clast(x):
    return x.movedim(1, -1)


def oihw(w_hwio):
    """[(kd,) kh, kw, ci, co] -> [co, ci, (kd,) kh, kw]"""
    return w_hwio.movedim(-1, 0).movedim(-1, 1)


def hwio(w_oihw):
    """[co, ci, (kd,) kh, kw] -> [(kd,) kh, kw, ci, co]"""
    return w_oihw.movedim(0, -1).movedim(0, -2)


def _conv(nd):
    return F.conv3d if nd == 3 else F.conv2d


def _tconv(nd):
    return F.conv_transpose3d if nd == 3 else F.conv_transpose2d


def _cat(srcs):
    return torch.cat([s for s in srcs if s is not None], -1)


def conv_ref(srcs, w, bias=None, relu=False):
    """3x3 (3x3x3) 'same' conv of the channel concat of `srcs`, + bias, ReLU."""
    x = _cat(srcs).double()
    y = _conv(x.dim() - 2)(cfirst(x), oihw(w.double()), None if bias is None else bias.double(), padding=1)
    return clast(F.relu(y) if relu else y).contiguous()


def conv_dgrad_ref(dy, w):
    """Data gradient of conv_ref: [.., co] -> [.., ci] (autograd, float64)."""
    nd = dy.dim() - 2
    x = torch.zeros((dy.shape[0], w.shape[-2]) + tuple(dy.shape[1:-1]), dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(_conv(nd)(x, oihw(w.double()), padding=1), x, cfirst(dy.double()))
    return clast(g).contiguous()


def conv_wgrad_ref(srcs, dy):
    """Weight (HWIO) and bias gradients of conv_ref (autograd, float64)."""
    x = _cat(srcs).double()
    nd = x.dim() - 2
    w = torch.zeros((dy.shape[-1], x.shape[-1]) + (3,) * nd, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(dy.shape[-1], dtype=torch.float64, requires_grad=True)
    gw, gb = torch.autograd.grad(_conv(nd)(cfirst(x), w, b, padding=1), [w, b], cfirst(dy.double()))
    return hwio(gw).contiguous(), gb


def _tw(k):
    """Keras [(kd,) kh, kw, co, ci] -> torch conv_transpose weight [ci, co, (kd,) kh, kw]"""
    return k.movedim(-1, 0).movedim(-1, 1)


def tconv_ref(x, k, bias=None):
    """2x2 (2x2x2) stride-2 transposed conv with its pixel shuffle: [.., ci] -> fine [.., co]."""
    nd = x.dim() - 2
    y = _tconv(nd)(cfirst(x.double()), _tw(k.double()), None if bias is None else bias.double(), stride=2)
    return clast(y).contiguous()


def tconv_dgrad_ref(dout, k):
    """Data gradient of tconv_ref: fine [.., co] -> coarse [.., ci]."""
    nd = dout.dim() - 2
    x = torch.zeros((dout.shape[0], k.shape[-1]) + tuple(s // 2 for s in dout.shape[1:-1]), dtype=torch.float64,
                    requires_grad=True)
    (g,) = torch.autograd.grad(_tconv(nd)(x, _tw(k.double()), stride=2), x, cfirst(dout.double()))
    return clast(g).contiguous()


def tconv_wgrad_ref(x, dout):
    """Weight ([(kd,) kh, kw, co, ci]) and bias gradients of tconv_ref."""
    nd = x.dim() - 2
    k = torch.zeros((x.shape[-1], dout.shape[-1]) + (2,) * nd, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(dout.shape[-1], dtype=torch.float64, requires_grad=True)
    gk, gb = torch.autograd.grad(_tconv(nd)(cfirst(x.double()), k, b, stride=2), [k, b], cfirst(dout.double()))
    return gk.movedim(0, -1).movedim(0, -2).contiguous(), gb


def pack_bits(y):
    """[..., C] -> [..., C / 8] uint8, bit e of byte b = channel 8 b + e > 0."""
    pos = (y > 0).to(torch.int32).reshape(*y.shape[:-1], y.shape[-1] // 8, 8)
    return (pos << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)


def pool_ref(y):
    """2x2 max-pool of [N, H, W, C] with the kernels' codes: per 8 channels one int32, bits
    [2e, 2e + 2) the FIRST argmax (dy * 2 + dx) of channel e, bit 24 + e: its maximum > 0."""
    N, H, W, Cc = y.shape
    win = y.reshape(N, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, Cc, 4)
    m = win.max(-1).values
    arg = (win == m.unsqueeze(-1)).to(torch.int64).argmax(-1)          # first index of the maximum
    e = torch.arange(8, dtype=torch.int64)
    code = ((arg.reshape(-1, 8) << (2 * e)) | ((m.reshape(-1, 8) > 0).to(torch.int64) << (24 + e))).sum(-1)
    return m.contiguous(), code.to(torch.int32)


def pool_route_ref(gy, code_src):
    """Pool backward routing: gy lands on the first argmax of each 2x2 window of `code_src`
    (the pooled activation's source), nothing where the maximum is not positive."""
    N, H, W, Cc = code_src.shape
    win = code_src.reshape(N, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, Cc, 4)
    m = win.max(-1).values
    arg = (win == m.unsqueeze(-1)).to(torch.int64).argmax(-1)
    hot = F.one_hot(arg, 4).double() * (m > 0).unsqueeze(-1) * gy.unsqueeze(-1)
    return hot.reshape(N, H // 2, W // 2, Cc, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, Cc).contiguous()


# -------------------------------------------------------------------------------- cases
class Case(dict):
    """ops: float64 operands; ref: float64 pre-rounding references by output name; bound:
    the reference on absolute values; dtype: storage type; rounds: outputs stored in 16 bits."""
    __getattr__ = dict.__getitem__


def ranges(dtype, first=False):
    """(|x| max, |w| max, |bias| max); tests/test_exact_ref_cpu.py asserts the rounding
    shares they give.  fp16 keeps 11 bits, so it needs wider operands than bf16 and fp32."""
    if dtype == "fp16":
        return 15, 15, 0
    return (64, 16, 8) if first else (8, 4, 8)


@functools.lru_cache(maxsize=None)
def fwd_case(N, D, H, W, C1, C2, Cout, dtype="bf16", relu=True, small=False):
    """Forward conv + bias (+ ReLU).  small: the statistics cases' |z| <= 64 ranges."""
    key = ("fwd", N, D, H, W, C1, C2, Cout, dtype, small)
    first = C1 <= 8
    xm, wm, bm = ranges(dtype, first)
    sp = (N, D, H, W) if D > 1 else (N, H, W)
    kk = (3, 3, 3) if D > 1 else (3, 3)
    if small:
        a = ints(seed_of(key, "a"), sp + (C1,), -2, 2, 0.5)
        b2 = ints(seed_of(key, "b"), sp + (C2,), -2, 2, 0.5) if C2 else None
        w = ints(seed_of(key, "w"), kk + (C1 + C2, Cout), -1, 1, 16.0 / (C1 + C2) if C1 > 8 else 1.0)
        bias = ints(seed_of(key, "bias"), (Cout,), -2, 2)
    else:
        a = ints(seed_of(key, "a"), sp + (C1,), -xm, xm)
        b2 = ints(seed_of(key, "b"), sp + (C2,), -xm, xm) if C2 else None
        w = ints(seed_of(key, "w"), kk + (C1 + C2, Cout), -wm, wm)
        bias = ints(seed_of(key, "bias"), (Cout,), -bm, bm)
    ref = conv_ref([a, b2], w, bias, relu)
    bound = conv_ref([a.abs(), None if b2 is None else b2.abs()], w.abs(), bias.abs()).max().item()
    return Case(ops=dict(a=a, b2=b2, w=w, bias=bias), ref=dict(y=ref), bound=bound, dtype=dtype,
                rounds=dtype != "fp32" and not small)


@functools.lru_cache(maxsize=None)
def dgrad_case(N, D, H, W, C1, C2, Co, dtype="bf16"):
    """Data gradient of a concat conv into two destinations.  2D: dst1 = g[..., :C1] x (mask1
    > 0), dst2 = g[..., C1:] x (mask2 > 0) x 1.25.  3D (the launch of test_conv3d_row_window):
    dst1 unmasked, dst2 masked, no rescale."""
    key = ("dgrad", N, D, H, W, C1, C2, Co, dtype)
    scale2 = 1.25 if D == 1 else 1.0
    xm, wm, _ = ranges(dtype)
    sp = (N, D, H, W) if D > 1 else (N, H, W)
    kk = (3, 3, 3) if D > 1 else (3, 3)
    dy = ints(seed_of(key, "dy"), sp + (Co,), -xm, xm)
    w = ints(seed_of(key, "w"), kk + (C1 + C2, Co), -wm, wm)
    m1 = ints(seed_of(key, "m1"), sp + (C1,), -8, 8, 0.7)
    m2 = nonneg(seed_of(key, "m2"), sp + (C2,), 8, 0.6)
    g = conv_dgrad_ref(dy, w)
    bound = conv_dgrad_ref(dy.abs(), w.abs()).max().item() * scale2
    r1 = g[..., :C1] * (m1 > 0) if D == 1 else g[..., :C1]
    ref = dict(d1=r1.contiguous(), d2=(g[..., C1:] * (m2 > 0) * scale2).contiguous())
    return Case(ops=dict(dy=dy, w=w, m1=m1, m2=m2), ref=ref, bound=bound, dtype=dtype, rounds=dtype != "fp32")


@functools.lru_cache(maxsize=None)
def wgrad_case(N, D, H, W, C1, C2, Cout, dtype="bf16", creal=0):
    """Weight + bias gradient.  creal > 0: first layer, C1 padded channels of which creal
    are real (the rest zero, dropped by the slab reduction's row remap)."""
    key = ("wgrad", N, D, H, W, C1, C2, Cout, dtype, creal)
    sp = (N, D, H, W) if D > 1 else (N, H, W)
    xm = 15 if dtype == "fp16" and N * D * H * W <= 8192 else 8
    if creal:
        a = torch.zeros(sp + (C1,), dtype=torch.float64)
        a[..., :creal] = ints(seed_of(key, "a"), sp + (creal,), -xm, xm)
    else:
        a = nonneg(seed_of(key, "a"), sp + (C1,), xm, 0.6)
    b2 = nonneg(seed_of(key, "b"), sp + (C2,), xm, 0.6) if C2 else None
    dy = ints(seed_of(key, "dy"), sp + (Cout,), -xm, xm)
    srcs = [a[..., :creal] if creal else a, b2]
    gw, gb = conv_wgrad_ref(srcs, dy)
    bw, bb = conv_wgrad_ref([s.abs() if s is not None else None for s in srcs], dy.abs())
    return Case(ops=dict(a=a, b2=b2, dy=dy), ref=dict(gw=gw, gb=gb), bound=max(bw.max().item(), bb.max().item()),
                dtype=dtype, rounds=False)


@functools.lru_cache(maxsize=None)
def tconv_case(N, D, H, Ci, Co, dtype="bf16"):
    """Transposed conv: forward (+ bias), its data gradient masked by x > 0, its weight and
    bias gradients.  D = 1: 2D on H x H coarse pixels; D > 1: 3D on D x H x H."""
    key = ("tconv", N, D, H, Ci, Co, dtype)
    # (one tap of Ci products per output, 4 taps x Co per data-gradient element: wider
    # ranges than the 9-tap convs so that the sums leave bf16's exact integers)
    sp = (N, D, H, H) if D > 1 else (N, H, H)
    fine = (N,) + tuple(2 * s for s in sp[1:])
    kk = (2, 2, 2) if D > 1 else (2, 2)
    x = nonneg(seed_of(key, "x"), sp + (Ci,), 32, 0.6)
    k = ints(seed_of(key, "k"), kk + (Co, Ci), -16, 16)
    bias = ints(seed_of(key, "bias"), (Co,), -8, 8)
    dout = ints(seed_of(key, "dout"), fine + (Co,), -8, 8)
    y = tconv_ref(x, k, bias)
    dxu = tconv_dgrad_ref(dout, k)
    dx = dxu * (x > 0)
    gk, gb = tconv_wgrad_ref(x, dout)
    bk, bb = tconv_wgrad_ref(x.abs(), dout.abs())
    return Case(ops=dict(x=x, k=k, bias=bias, dout=dout), ref=dict(y=y, dx=dx, dxu=dxu, gk=gk, gb=gb),
                bound=max(tconv_ref(x, k.abs(), bias.abs()).max().item(),
                          tconv_dgrad_ref(dout.abs(), k.abs()).max().item(), bk.max().item(), bb.max().item()),
                dtype=dtype, rounds=dtype != "fp32")


@functools.lru_cache(maxsize=None)
def pool_route_case(N, H, C1, C2, Co):
    """Skip half of a decoder data gradient with the max-pool backward in its epilogue.
    Reference RNE(RNE(masked conv) + routed gy): conv_epilogue.h documents the sum as "the
    (masked, 16-bit rounded) skip gradient plus the routed pool gradient"."""
    key = ("route", N, H, C1, C2, Co)
    dy = ints(seed_of(key, "dy"), (N, H, H, Co), -8, 8)
    w = ints(seed_of(key, "w"), (3, 3, C1 + C2, Co), -4, 4)
    y = nonneg(seed_of(key, "y"), (N, H, H, C2), 8, 0.6)               # the skip source (pooled)
    gy = ints(seed_of(key, "gy"), (N, H // 2, H // 2, C2), -64, 64)
    g = conv_dgrad_ref(dy, w)
    bound = conv_dgrad_ref(dy.abs(), w.abs()).max().item() + 64
    skip = (g[..., C1:] * (y > 0)).contiguous()
    routed = pool_route_ref(gy, y)
    return Case(ops=dict(dy=dy, w=w, y=y, gy=gy), ref=dict(up=g[..., :C1].contiguous(), skip=skip, routed=routed),
                bound=bound, dtype="bf16", rounds=True)


def route_final(case):
    """RNE(RNE(masked conv) + routed gy) as float64 (still to be rounded by the caller)."""
    return rne(case.ref["skip"], "bf16").double() + case.ref["routed"]


@functools.lru_cache(maxsize=None)
def conv_dw_case(N, nsplit):
    """Fused data + weight gradient on 128 x 128 x 32: dx masked by act > 0; slab rows sum to
    the weight / bias gradient of the conv whose input is x."""
    key = ("conv_dw", N, nsplit)
    sp = (N, 128, 128)
    dy = ints(seed_of(key, "dy"), sp + (32,), -8, 8)
    x = nonneg(seed_of(key, "x"), sp + (32,), 8, 0.6)
    act = nonneg(seed_of(key, "act"), sp + (32,), 8, 0.6)
    w = ints(seed_of(key, "w"), (3, 3, 32, 32), -4, 4)
    dx = conv_dgrad_ref(dy, w) * (act > 0)
    gw, gb = conv_wgrad_ref([x], dy)
    bw, bb = conv_wgrad_ref([x], dy.abs())
    bound = max(conv_dgrad_ref(dy.abs(), w.abs()).max().item(), bw.max().item(), bb.max().item())
    return Case(ops=dict(dy=dy, x=x, act=act, w=w), ref=dict(dx=dx.contiguous(), gw=gw, gb=gb), bound=bound,
                dtype="bf16", rounds=True)


@functools.lru_cache(maxsize=None)
def f32_bwd_case(C1, C2, Co, N=2, H=32):
    """fp32 executor: data gradient masked by the producer's ReLU, weight gradient slabs."""
    key = ("f32_bwd", C1, C2, Co, N, H)
    xa = nonneg(seed_of(key, "xa"), (N, H, H, C1), 8, 0.6)
    xb = nonneg(seed_of(key, "xb"), (N, H, H, C2), 8, 0.6)
    w = ints(seed_of(key, "w"), (3, 3, C1 + C2, Co), -4, 4)
    dy = ints(seed_of(key, "dy"), (N, H, H, Co), -8, 8)
    mask = torch.cat([xa, xb], -1)
    dx = conv_dgrad_ref(dy, w) * (mask > 0)
    gw, _ = conv_wgrad_ref([mask], dy)
    bw, _ = conv_wgrad_ref([mask], dy.abs())
    return Case(ops=dict(xa=xa, xb=xb, w=w, dy=dy), ref=dict(dx=dx.contiguous(), gw=gw),
                bound=max(conv_dgrad_ref(dy.abs(), w.abs()).max().item(), bw.max().item()), dtype="fp32", rounds=False)


def _per_sample(c, gn, N):
    """Coefficient rows [N or 1, C] -> broadcastable over [N, H, W, C]"""
    return c.reshape(N if gn else 1, 1, 1, -1)


@functools.lru_cache(maxsize=None)
def norm_onload_case(N, H, Cin, Cout, gn):
    """Normalise-on-load forward (xform 1): the conv reads the pre-norm z and forms
    y = relu(a z + b) in LDS, in 16 bits by design (conv_win.h XF 1: "normalises it in LDS";
    xout holds that activation) -- integer coefficients keep y an exact small integer."""
    key = ("norm_onload", N, H, Cin, Cout, gn)
    rows = N if gn else 1
    z = ints(seed_of(key, "z"), (N, H, H, Cin), -8, 8)
    a = ints(seed_of(key, "a"), (rows, Cin), 1, 3)
    b = ints(seed_of(key, "b"), (rows, Cin), -4, 4)
    w = ints(seed_of(key, "w"), (3, 3, Cin, Cout), -4, 4)
    bias = ints(seed_of(key, "bias"), (Cout,), -8, 8)
    y = torch.clamp(_per_sample(a, gn, N) * z + _per_sample(b, gn, N), min=0)
    return Case(ops=dict(z=z, a=a, b=b, w=w, bias=bias), ref=dict(_y=y, out=conv_ref([y], w, bias)),
                bound=conv_ref([y], w.abs(), bias.abs()).max().item(), dtype="bf16", rounds=True)


@functools.lru_cache(maxsize=None)
def dz_onload_case(N, W, Co, Ci, gn):
    """dz-on-load data gradient (xform 2): the halo is dz = ca g + cb z + cc formed in LDS."""
    key = ("dz_onload", N, W, Co, Ci, gn)
    rows = N if gn else 1
    g = ints(seed_of(key, "g"), (N, W, W, Co), -4, 4)
    z = ints(seed_of(key, "z"), (N, W, W, Co), -4, 4)
    ca = ints(seed_of(key, "ca"), (rows, Co), 1, 2)
    cb = ints(seed_of(key, "cb"), (rows, Co), -1, 1)
    cc = ints(seed_of(key, "cc"), (rows, Co), -2, 2)
    w = ints(seed_of(key, "w"), (3, 3, Ci, Co), -4, 4)
    act = nonneg(seed_of(key, "act"), (N, W, W, Ci), 8, 0.6)
    dz = _per_sample(ca, gn, N) * g + _per_sample(cb, gn, N) * z + _per_sample(cc, gn, N)
    dx = conv_dgrad_ref(dz, w) * (act > 0)
    return Case(ops=dict(g=g, z=z, ca=ca, cb=cb, cc=cc, w=w, act=act), ref=dict(_dz=dz, dx=dx.contiguous()),
                bound=conv_dgrad_ref(dz.abs(), w.abs()).max().item(), dtype="bf16", rounds=True)


@functools.lru_cache(maxsize=None)
def tconv_onload_case(N, H, K, Cc, Cs, O):
    """Decoder forward z = relu(conv3x3([tconv(b) + bt, skip]) + ba) with u formed on load.
    The reference forms u = RNE(tconv(b) + bt) first: u lives in LDS in 16 bits by design
    (conv_win.h XF 5; bit-identical to the materialised 16-bit tconv output)."""
    key = ("tconv_onload", N, H, K, Cc, Cs, O)
    b = nonneg(seed_of(key, "b"), (N, H, H, K), 16, 0.6)
    skip = ints(seed_of(key, "skip"), (N, 2 * H, 2 * H, Cs), -8, 8)
    wt = ints(seed_of(key, "wt"), (2, 2, Cc, K), -8, 8)
    bt = ints(seed_of(key, "bt"), (Cc,), -8, 8)
    wa = ints(seed_of(key, "wa"), (3, 3, Cc + Cs, O), -1, 1, 0.5)     # (small: z keeps >= 5 % ties)
    ba = ints(seed_of(key, "ba"), (O,), -8, 8)
    u64 = tconv_ref(b, wt, bt)
    u = rne(u64, "bf16").double()
    z = conv_ref([u, skip], wa, ba, relu=True)
    bound = max(tconv_ref(b, wt.abs(), bt.abs()).max().item(),
                conv_ref([u.abs(), skip.abs()], wa.abs(), ba.abs()).max().item())
    return Case(ops=dict(b=b, skip=skip, wt=wt, bt=bt, wa=wa, ba=ba), ref=dict(u=u64, z=z), bound=bound, dtype="bf16",
                rounds=True)


@functools.lru_cache(maxsize=None)
def s2d_case(N, H, K, Cc, Cs, O):
    """Composite transposed-conv data gradient: db through u = tconv(b), z = conv3x3([u, skip])
    as one coarse conv over the space-to-depth image of dz with composed weights.  |wt|, |wa|
    <= 1 keep the composed weights (16-bit by design: tconv_fused.hip tconv_compose writes
    them in the storage type) small exact integers; the reference is the true chain-rule
    gradient, rounded once."""
    key = ("s2d", N, H, K, Cc, Cs, O)
    b = nonneg(seed_of(key, "b"), (N, H, H, K), 8, 0.6)
    wt = ints(seed_of(key, "wt"), (2, 2, Cc, K), -1, 1)
    wa = ints(seed_of(key, "wa"), (3, 3, Cc + Cs, O), -1, 1)
    dz = ints(seed_of(key, "dz"), (N, 2 * H, 2 * H, O), -8, 8)
    db = tconv_dgrad_ref(conv_dgrad_ref(dz, wa)[..., :Cc].contiguous(), wt) * (b > 0)
    bound = tconv_dgrad_ref(conv_dgrad_ref(dz.abs(), wa.abs())[..., :Cc].contiguous(), wt.abs()).max().item()
    return Case(ops=dict(b=b, wt=wt, wa=wa, dz=dz), ref=dict(db=db.contiguous()), bound=bound, dtype="bf16", rounds=True)


@functools.lru_cache(maxsize=None)
def tconv_chain_case(N, H, K, Cc, Cs, O):
    """Composite transposed-conv weight gradients: the 4x4-tap stride-2 slab sums
    Hs[sh][sw][o][k] = sum dz[2h + sh - 1][2w + sw - 1][o] b[h][w][k] (and the per-tap sums Bs
    of dz), and through the chain rule dWt, dbt and the consumer conv's dWa -- against float64
    autograd of u = tconv(b) + bt; z = conv3x3([u, skip])."""
    key = ("tconv_chain", N, H, K, Cc, Cs, O)
    b = nonneg(seed_of(key, "b"), (N, H, H, K), 2, 0.5)
    skip = ints(seed_of(key, "skip"), (N, 2 * H, 2 * H, Cs), -2, 2)
    wt = ints(seed_of(key, "wt"), (2, 2, Cc, K), -1, 1)
    bt = ints(seed_of(key, "bt"), (Cc,), -2, 2)
    wa = ints(seed_of(key, "wa"), (3, 3, Cc + Cs, O), -1, 1, 0.5)
    dz = ints(seed_of(key, "dz"), (N, 2 * H, 2 * H, O), -2, 2)

    def chain(b, skip, wt, bt, wa, dz):
        wtr, btr, war = [t.clone().requires_grad_(True) for t in (wt, bt, wa)]
        u = F.conv_transpose2d(cfirst(b), _tw(wtr), btr, stride=2)
        z = F.conv2d(torch.cat([u, cfirst(skip)], 1), oihw(war), padding=1)
        gwt, gbt, gwa = torch.autograd.grad(z, (wtr, btr, war), cfirst(dz))
        dzp = F.pad(dz, (0, 0, 1, 3, 1, 3))                  # fine rows / cols -1 .. 2H + 1
        sl = [dzp[:, sh:sh + 2 * H:2, sw:sw + 2 * H:2, :] for sh in range(4) for sw in range(4)]
        Hs = torch.stack([torch.einsum("nhwo,nhwk->ok", t, b) for t in sl])
        Bs = torch.stack([t.sum((0, 1, 2)) for t in sl])
        return dict(Hs=Hs, Bs=Bs, dwt=gwt.reshape(4, Cc, K), dbt=gbt, dwa=gwa)
    ref = chain(b, skip, wt, bt, wa, dz)
    ab = chain(b, skip.abs(), wt.abs(), bt.abs(), wa.abs(), dz.abs())
    return Case(ops=dict(b=b, skip=skip, wt=wt, bt=bt, wa=wa, dz=dz), ref=ref,
                bound=max(v.max().item() for v in ab.values()), dtype="bf16", rounds=False)


# The shapes tests/test_gpu_exact.py launches (taken from the existing parametrisations).
# forward: (N, D, H, W, C1, C2, Cout, tile, expected conv_fwd_pick id)
FWD_BF16 = [
    (2, 1, 16, 16, 32, 0, 32, 8, 4), (2, 1, 8, 8, 64, 0, 128, 8, 2), (2, 1, 8, 8, 64, 0, 128, 1, 1),
    (2, 1, 8, 8, 64, 0, 128, 2, 2), (2, 1, 16, 16, 32, 0, 32, 4, 4),
    (3, 1, 128, 128, 32, 32, 32, 6, 6), (3, 1, 16, 16, 32, 0, 32, 6, 6), (5, 1, 16, 16, 64, 0, 64, 6, 6),
    (3, 1, 64, 64, 64, 64, 64, 12, 12), (5, 1, 16, 16, 64, 0, 128, 12, 12),
    (3, 1, 128, 128, 32, 0, 32, 0, 6), (3, 1, 64, 64, 64, 0, 64, 0, 6),
    (1, 1, 4, 384, 32, 32, 32, 6, 6),
    (5, 1, 8, 8, 64, 64, 128, 0, 13),
    (5, 1, 16, 16, 4, 0, 64, 9, 9), (3, 1, 128, 128, 4, 0, 32, 9, 9), (2, 1, 32, 32, 8, 0, 64, 8, 2),
    (2, 3, 64, 64, 32, 32, 32, 6, 6), (2, 3, 64, 64, 4, 0, 64, 9, 9),
]
FWD_FP16 = [(2, 1, 64, 64, 32, 0, 32, 6, 6), (2, 1, 16, 16, 64, 0, 64, 12, 12), (2, 1, 16, 16, 64, 0, 64, 0, 6),
            (2, 1, 8, 8, 64, 0, 128, 8, 2)]
# statistics rows: |z| <= 64, <= 4096 pixels per sample (sum z^2 <= 2^24); (..., tile, expected id)
STATS = [(4, 1, 16, 16, 64, 0, 64, 0, 6), (2, 1, 32, 32, 32, 32, 64, 12, 12), (2, 1, 64, 64, 4, 0, 32, 0, 9),
         (8, 1, 8, 8, 128, 0, 256, 0, 13), (2, 1, 16, 16, 32, 0, 32, 0, 6)]
# dual-destination data gradient: (N, D, H, C1, C2, Co, dtype)
DGRAD = [(2, 1, 16, 32, 32, 32, "bf16"), (2, 1, 128, 32, 32, 32, "bf16"), (6, 1, 8, 256, 256, 512, "bf16"),
         (2, 3, 64, 32, 32, 32, "bf16"), (2, 1, 16, 32, 32, 32, "fp16")]
ROUTE = [(2, 128, 32, 32, 32), (2, 64, 64, 64, 64)]
TCONV = [(2, 1, 8, 64, 32), (3, 1, 64, 64, 32)]
# weight gradients: (N, D, H, W, C1, C2, Cout, splits, win, creal, dtype, expected wgrad_pick tuple
# (BM, BN, taps per group, small-C)).  win = -1 on the two tiled shapes of test_conv_wgrad_and_bias
# (which launches them without the key, i.e. on the window kernel) forces the tiled kernel the
# issue lists them under, as the win = -1 cases of test_wgrad_row_window do.
WGRAD = [
    (4, 1, 16, 16, 32, 0, 32, 3, -1, 0, "bf16", (32, 32, 9, 0)), (2, 1, 8, 8, 256, 0, 512, 2, -1, 0, "bf16", (128, 128, 1, 0)),
    (3, 1, 128, 128, 32, 0, 32, 5, 0, 0, "bf16", (32, 32, 9, 0)), (2, 1, 128, 128, 32, 32, 32, 7, 0, 0, "bf16", (32, 32, 9, 0)),
    (3, 1, 32, 32, 32, 0, 32, 40, 0, 0, "bf16", (32, 32, 9, 0)), (4, 1, 16, 16, 64, 0, 64, 3, 0, 0, "bf16", (32, 64, 9, 0)),
    (3, 1, 8, 8, 32, 0, 32, 7, 0, 0, "bf16", (32, 32, 9, 0)),
    (1, 1, 6, 384, 32, 32, 32, 4, 0, 0, "bf16", (32, 32, 9, 0)), (2, 3, 64, 64, 32, 32, 32, 5, 0, 0, "bf16", (32, 32, 9, 0)),
    (2, 1, 32, 32, 4, 0, 32, 3, 0, 1, "bf16", (48, 32, 1, 1)), (2, 1, 32, 32, 4, 0, 32, 3, -1, 1, "bf16", (64, 32, 1, 1)),
    (3, 1, 128, 128, 4, 0, 32, 7, 0, 4, "bf16", (48, 32, 1, 1)), (2, 3, 64, 64, 4, 0, 32, 5, 0, 1, "bf16", (112, 32, 1, 1)),
    (3, 1, 64, 64, 32, 0, 32, 5, 0, 0, "fp16", (32, 32, 9, 0)), (2, 1, 16, 16, 64, 0, 128, 2, -1, 0, "fp16", (64, 64, 3, 0)),
]
WGRAD_PF = (2, 1, 128, 128, 32, 0, 32, 7, (32, 32, 9, 0))
TCONV_WGRAD = [(2, 8, 64, 32, 2, (32, 32, 4, 0)), (3, 64, 64, 32, 40, (32, 64, 4, 0))]     # (..., splits, pick)
CONV_DW = [(2, 7, "act"), (3, 64, "bits")]
DROPOUT_PICK = 13
DROPOUT = (2, 1, 8, 8, 32, 0, 64)          # rate 0.5: the rescale 2 is exact however 1 / (1 - rate) is formed
# on-load transforms: (N, H, Cin, Cout, gn, tile, stats) / (N, W, Co, Ci, gn) / (N, H, K, Cc, Cs, O)
NORM_ONLOAD = [(2, 128, 32, 32, True, 6, False), (4, 16, 32, 32, True, 0, False), (2, 64, 64, 64, True, 0, True)]
DZ_ONLOAD = [(2, 64, 64, 64, False), (2, 32, 128, 128, True), (3, 16, 256, 128, False)]
TCONV_ONLOAD = [(2, 64, 64, 32, 32, 32), (3, 16, 64, 32, 32, 64)]
TCONV_ONLOAD_PF = [(3, 64, 64, 32, 32, 32, 5, 1), (2, 64, 32, 32, 32, 32, 8, 1)]      # (..., win_pf, rev)
S2D = [(2, 64, 64, 32, 32, 32), (3, 16, 64, 32, 32, 32)]
TCONV_CHAIN = [(2, 64, 64, 32, 32, 32, 8, 0), (3, 16, 64, 32, 32, 32, 3, -1)]          # (..., splits, win)
SPLIT_RANGES = dict(first=(4, 1, 32, 32, 4, 0, 32, "bf16", 4), win=(4, 1, 32, 32, 64, 0, 64, "bf16", 0),
                    tconv=(4, 1, 32, 64, 32))
SPLIT_PICKS = dict(first=(48, 32, 1, 1), win=(32, 64, 9, 0), tconv=(32, 64, 4, 0))
F32_TCONV = [(2, 1, 8, 64, 32), (2, 8, 8, 64, 32)]
F32_FWD = [(2, 16, 32, 32, 64), (3, 16, 64, 0, 48), (2, 8, 1, 0, 32)]
F32_BWD = [(32, 32, 32), (64, 0, 64), (4, 0, 32)]


def rounding_cases():
    """(name, builder) of every 16-bit forward / data-gradient case of the GPU tests."""
    out = []
    for dt, table in (("bf16", FWD_BF16), ("fp16", FWD_FP16)):
        for k in table:
            out.append(("fwd %s %s" % (dt, k[:7]), functools.partial(fwd_case, *k[:7], dt)))
    out.append(("fwd bf16 dropout %s" % (DROPOUT,), functools.partial(fwd_case, *DROPOUT)))
    for (N, D, H, C1, C2, Co, dt) in DGRAD:
        out.append(("dgrad %s %s" % (dt, (N, D, H, C1, C2, Co)), functools.partial(dgrad_case, N, D, H, H, C1, C2, Co, dt)))
    for k in ROUTE:
        out.append(("route %s" % (k,), functools.partial(pool_route_case, *k)))
    for (N, D, H, Ci, Co) in TCONV:
        out.append(("tconv %s" % ((N, D, H, Ci, Co),), functools.partial(tconv_case, N, D, H, Ci, Co)))
    for k in CONV_DW:
        out.append(("conv_dw %s" % (k[:2],), functools.partial(conv_dw_case, *k[:2])))
    for k in NORM_ONLOAD:
        out.append(("norm on load %s" % (k[:5],), functools.partial(norm_onload_case, *k[:5])))
    for k in DZ_ONLOAD:
        out.append(("dz on load %s" % (k,), functools.partial(dz_onload_case, *k)))
    for k in TCONV_ONLOAD + [p[:6] for p in TCONV_ONLOAD_PF]:
        out.append(("tconv on load %s" % (k,), functools.partial(tconv_onload_case, *k)))
    for k in S2D:
        out.append(("s2d %s" % (k,), functools.partial(s2d_case, *k)))
    return out


def exact_only_cases():
    """(name, builder) of the cases with fp32 outputs or |z| <= 64 (no store rounding)."""
    out = []
    for k in STATS:
        out.append(("stats %s" % (k[:7],), functools.partial(fwd_case, *k[:7], "bf16", False, True)))
    for k in WGRAD:
        out.append(("wgrad %s %s" % (k[10], k[:7] + (k[9],)), functools.partial(wgrad_case, *k[:7], k[10], k[9])))
    out.append(("wgrad pf128", functools.partial(wgrad_case, *WGRAD_PF[:7])))
    for (N, H, C1, C2, Co) in F32_FWD:
        out.append(("f32 fwd %s" % ((N, H, C1, C2, Co),), functools.partial(fwd_case, N, 1, H, H, C1, C2, Co, "fp32")))
    for kind, k in SPLIT_RANGES.items():
        out.append(("wgrad split ranges %s" % kind, functools.partial(tconv_case if kind == "tconv" else wgrad_case, *k)))
    for k in TCONV_CHAIN:
        out.append(("tconv chain %s" % (k[:6],), functools.partial(tconv_chain_case, *k[:6])))
    for k in F32_BWD:
        out.append(("f32 bwd %s" % (k,), functools.partial(f32_bwd_case, *k)))
    for k in F32_TCONV:
        out.append(("f32 tconv %s" % (k,), functools.partial(tconv_case, *k, "fp32")))
    return out
