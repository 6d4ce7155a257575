"""The exact-reference helpers (tests/exact_ref.py) on the CPU: the float64 references against
brute-force loops, the weight packers, the sensitivity of the bit comparison, the guards,
and the input conditions of every case tests/test_gpu_exact.py launches."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
from test_gpu_kernels import pack_dgrad, pack_fwd


def _brute_conv(x, w, b):
    """x [N, H, W, ci], w [3, 3, ci, co] -> [N, H, W, co], 'same' zero padding; plain loops."""
    N, H, W, Ci = x.shape
    Co = w.shape[-1]
    y = np.zeros((N, H, W, Co))
    for n in range(N):
        for h in range(H):
            for ww in range(W):
                acc = b.copy()
                for kh in range(3):
                    for kw in range(3):
                        ih, iw = h + kh - 1, ww + kw - 1
                        if 0 <= ih < H and 0 <= iw < W:
                            acc = acc + x[n, ih, iw, :] @ w[kh, kw]
                y[n, h, ww] = acc
    return y


def test_references_match_brute_force():
    x = X.ints(1, (1, 5, 5, 2), -8, 8)
    x2 = X.ints(2, (1, 5, 5, 1), -8, 8)
    w = X.ints(3, (3, 3, 3, 3), -4, 4)
    b = X.ints(4, (3,), -8, 8)
    ref = _brute_conv(torch.cat([x, x2], -1).numpy(), w.numpy(), b.numpy())
    assert np.array_equal(X.conv_ref([x, x2], w, b).numpy(), ref)
    assert np.array_equal(X.conv_ref([x, x2], w, b, relu=True).numpy(), np.maximum(ref, 0))
    # data gradient: dx[n, p, ci] = sum over (tap, co) of dy[n, p - tap + 1, co] w[tap, ci, co]
    dy = X.ints(5, (1, 5, 5, 3), -8, 8)
    wf = np.flip(w.numpy(), (0, 1)).transpose(0, 1, 3, 2).copy()
    assert np.array_equal(X.conv_dgrad_ref(dy, w).numpy(), _brute_conv(dy.numpy(), wf, np.zeros(3)))
    # weight / bias gradient
    gw, gb = X.conv_wgrad_ref([x, x2], dy)
    xin, dyn = np.pad(torch.cat([x, x2], -1).numpy(), ((0, 0), (1, 1), (1, 1), (0, 0))), dy.numpy()
    bw = np.zeros((3, 3, 3, 3))
    for kh in range(3):
        for kw in range(3):
            bw[kh, kw] = np.einsum("nhwi,nhwo->io", xin[:, kh:kh + 5, kw:kw + 5], dyn)
    assert np.array_equal(gw.numpy(), bw) and np.array_equal(gb.numpy(), dyn.sum((0, 1, 2)))


def test_tconv_references_match_brute_force():
    x = X.ints(6, (1, 3, 3, 2), -8, 8)
    k = X.ints(7, (2, 2, 3, 2), -4, 4)            # (kh, kw, co, ci)
    b = X.ints(8, (3,), -8, 8)
    y = np.zeros((1, 6, 6, 3))
    for h in range(3):
        for w in range(3):
            for th in range(2):
                for tw in range(2):
                    y[0, 2 * h + th, 2 * w + tw] = k[th, tw].numpy() @ x[0, h, w].numpy() + b.numpy()
    assert np.array_equal(X.tconv_ref(x, k, b).numpy(), y)
    dout = X.ints(9, (1, 6, 6, 3), -8, 8)
    dx, gk = np.zeros((1, 3, 3, 2)), np.zeros((2, 2, 3, 2))
    for h in range(3):
        for w in range(3):
            for th in range(2):
                for tw in range(2):
                    g = dout[0, 2 * h + th, 2 * w + tw].numpy()
                    dx[0, h, w] += g @ k[th, tw].numpy()
                    gk[th, tw] += np.outer(g, x[0, h, w].numpy())
    assert np.array_equal(X.tconv_dgrad_ref(dout, k).numpy(), dx)
    rk, rb = X.tconv_wgrad_ref(x, dout)
    assert np.array_equal(rk.numpy(), gk) and np.array_equal(rb.numpy(), dout.numpy().sum((0, 1, 2)))
    # 3D: against the 2D reference applied per depth tap
    x3 = X.ints(10, (1, 2, 3, 3, 2), -8, 8)
    k3 = X.ints(11, (2, 2, 2, 3, 2), -4, 4)
    y3 = X.tconv_ref(x3, k3, b)
    for d in range(2):
        for td in range(2):
            assert torch.equal(y3[:, 2 * d + td], X.tconv_ref(x3[:, d], k3[td], b))


def _im2col(x):
    """[N, H, W, C] -> [N H W, 9 C]: column (kh * 3 + kw) * C + c, the kernels' K order."""
    N, H, W, Cc = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    cols = [xp[:, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)]
    return torch.stack(cols, 3).reshape(N * H * W, 9 * Cc)


@pytest.mark.parametrize("kh,kw,ci,co", [(0, 0, 0, 0), (2, 1, 3, 5), (1, 2, 7, 0), (0, 2, 31, 31)])
def test_packers_place_a_one_hot_weight(kh, kw, ci, co):
    """pack_fwd / pack_dgrad rows are the GEMM's B operand over K = (tap, channel): a one-hot
    weight lands where the float64 conv / data gradient puts it; HWIO <-> OIHW round-trips."""
    Ci, Co = 32, 32
    w = torch.zeros(3, 3, Ci, Co, dtype=torch.float64)
    w[kh, kw, ci, co] = 3.0
    x = X.ints(12, (2, 4, 5, Ci), -8, 8)
    wp = pack_fwd(w)
    assert wp.shape == (Co, 320) and wp.count_nonzero() == 1 and wp[co, (kh * 3 + kw) * Ci + ci] == 3.0
    y = (_im2col(x) @ wp[:, :9 * Ci].t()).reshape(2, 4, 5, Co)
    assert torch.equal(y, X.conv_ref([x], w))
    dy = X.ints(13, (2, 4, 5, Co), -8, 8)
    wd = pack_dgrad(w)
    assert wd.shape == (Ci, 320) and wd.count_nonzero() == 1
    assert wd[ci, ((2 - kh) * 3 + (2 - kw)) * Co + co] == 3.0
    dx = (_im2col(dy) @ wd[:, :9 * Co].t()).reshape(2, 4, 5, Ci)
    assert torch.equal(dx, X.conv_dgrad_ref(dy, w))
    o = X.oihw(w)
    assert o.shape == (Co, Ci, 3, 3) and o[co, ci, kh, kw] == 3.0 and torch.equal(X.hwio(o), w)
    w3 = torch.zeros(3, 3, 3, 4, 8, dtype=torch.float64)
    w3[2, kh, kw, 1, 5] = 1.0
    assert X.oihw(w3)[5, 1, 2, kh, kw] == 1.0 and torch.equal(X.hwio(X.oihw(w3)), w3)


def test_pool_reference_matches_max_pool_and_routes_to_first_argmax():
    y = X.nonneg(14, (2, 6, 8, 16), 3, 0.5)         # many ties and all-zero windows
    m, code = X.pool_ref(y)
    assert torch.equal(m, X.clast(F.max_pool2d(X.cfirst(y), 2)))
    gy = X.ints(15, (2, 3, 4, 16), 1, 9)
    r = X.pool_route_ref(gy, y)
    assert torch.equal(r.reshape(2, 3, 2, 4, 2, 16).sum((2, 4)), gy * (m > 0))      # each window routes once
    assert ((r != 0) <= (y == m.repeat_interleave(2, 1).repeat_interleave(2, 2))).all()
    c = code.reshape(2, 3, 4, 2).to(torch.int64)
    for (n, h, w, ch) in [(0, 0, 0, 0), (1, 2, 3, 15), (0, 1, 2, 9)]:
        word, e = c[n, h, w, ch // 8].item(), ch % 8
        arg = (word >> (2 * e)) & 3
        win = y[n, 2 * h:2 * h + 2, 2 * w:2 * w + 2, ch].reshape(-1)
        assert arg == int((win == win.max()).to(torch.int64).argmax()) and ((word >> (24 + e)) & 1) == int(win.max() > 0)


def test_sensitivity_one_input_element_and_one_output_bit():
    """+1 on one corner input element changes exactly its 3x3 neighbourhood (clipped at the
    border) in the channels whose weight there is non-zero, and the comparison reports exactly
    those coordinates; one flipped mantissa bit of a stored output is one mismatch."""
    c = X.fwd_case(2, 1, 8, 8, 32, 0, 32, "bf16", False)
    a, w, bias = c.ops["a"], c.ops["w"].clone(), c.ops["bias"]
    w[1, 1, 5, 7] = 0
    w[0, 0, 5, 3] = 0
    ref64 = X.conv_ref([a], w, bias)
    a2 = a.clone()
    a2[1, 0, 7, 5] += 1                             # top-right corner of image 1, channel 5
    out64 = X.conv_ref([a2], w, bias)
    expect = set()
    for h in range(0, 2):
        for ww in range(6, 8):
            kh, kw = 0 - h + 1, 7 - ww + 1          # the tap that reads (0, 7) from output (h, ww)
            for co in range(32):
                if w[kh, kw, 5, co] != 0:
                    expect.add((1, h, ww, co))
    assert (1, 0, 7, 7) not in expect and len(expect) < 4 * 32
    # compared before rounding (fp32 holds both exactly): every changed sum is reported
    with pytest.raises(X.BitsMismatch) as e:
        X.assert_bits_equal(out64.float(), ref64.float(), "perturbed input", ref64, "bf16")
    assert set(map(tuple, e.value.coords.tolist())) == expect
    assert "border pixel" in str(e.value) and "float64" in str(e.value)
    # after rounding a +1 below half an ulp can vanish, never appear elsewhere
    with pytest.raises(X.BitsMismatch) as e:
        X.assert_bits_equal(X.rne(out64, "bf16"), X.rne(ref64, "bf16"), "perturbed input, stored", ref64, "bf16")
    got = set(map(tuple, e.value.coords.tolist()))
    assert got and got <= expect
    for dt in ("bf16", "fp16"):
        r = X.rne(ref64, dt)
        o = r.clone()
        o.view(torch.int16)[0, 3, 4, 9] ^= 1
        with pytest.raises(X.BitsMismatch) as e:
            X.assert_bits_equal(o, r, "one ulp", ref64, dt)
        assert e.value.coords.tolist() == [[0, 3, 4, 9]] and "interior pixel" in str(e.value)
    X.assert_bits_equal(X.rne(ref64, "bf16"), X.rne(ref64, "bf16"), "equal")
    nan = X.rne(ref64, "bf16")
    nan[0, 0, 0, 0] = float("nan")
    with pytest.raises(X.BitsMismatch):
        X.assert_bits_equal(nan, nan.clone(), "NaN never equals")


def test_rounding_share_counts_ties_and_inexact_values():
    v = torch.tensor([0.0, 1.0, 255.0, 256.0, 257.0, 258.0, 259.0, 260.0, 513.0, 514.0, 2049.0, 2050.0, 4098.0],
                     dtype=torch.float64)
    # bf16 (8 bits): 257 tie, 258 ok, 259 tie, 513 inexact, 514 tie, 2049 inexact, 2050 inexact, 4098 inexact
    nr, tie = X.rounding_share(v, "bf16")
    assert nr == pytest.approx(7 / 12) and tie == pytest.approx(3 / 12)
    # fp16 (11 bits): 2049 tie, 2050 ok, 4098 tie
    nr, tie = X.rounding_share(v, "fp16")
    assert nr == pytest.approx(2 / 12) and tie == pytest.approx(2 / 12)
    assert X.rounding_share(v, "fp32") == (0.0, 0.0)
    # RNE: ties go to the even neighbour
    assert X.rne(torch.tensor([257.0, 259.0, 514.0], dtype=torch.float64), "bf16").tolist() == [256.0, 260.0, 512.0]
    assert X.rne(torch.tensor([2049.0, 2051.0], dtype=torch.float64), "fp16").tolist() == [2048.0, 2052.0]


def test_guards_reject_cases_outside_the_exact_regime():
    with pytest.raises(AssertionError, match="exact regime"):
        X.require_exact(torch.tensor([2.0 ** 24]))
    assert X.require_exact(torch.tensor([2.0 ** 24 - 1])) == 2.0 ** 24 - 1
    x = torch.full((1, 64, 64, 64), 255.0, dtype=torch.float64)
    w = torch.full((3, 3, 64, 32), 127.0, dtype=torch.float64)
    with pytest.raises(AssertionError, match="exact regime"):
        X.require_exact(X.conv_ref([x.abs()], w.abs()))
    with pytest.raises(AssertionError, match="fp16 output overflows"):
        X.require_exact(1e5, torch.tensor([65504.0], dtype=torch.float64), "fp16")
    with pytest.raises(AssertionError, match="not representable"):
        X.to_storage(torch.tensor([257.0], dtype=torch.float64), "bf16", "cpu")
    with pytest.raises(AssertionError, match="not representable"):
        X.to_storage(torch.tensor([2049.0], dtype=torch.float64), "fp16", "cpu")
    assert X.to_storage(torch.tensor([256.0, -3.0]), "bf16", "cpu").dtype == torch.bfloat16
    with pytest.raises(AssertionError, match="not exact in fp32"):
        X.rne(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64), "bf16")
    # generators: closed range, density, non-negative variant
    t = X.ints(3, (4000,), -8, 8)
    assert t.min() == -8 and t.max() == 8 and t.dtype == torch.float64 and torch.equal(t, X.ints(3, (4000,), -8, 8))
    z = X.ints(3, (4000,), 1, 8, 0.25)
    assert 0.2 < (z != 0).double().mean() < 0.3
    p = X.nonneg(4, (4000,), 8)
    assert p.min() == 0 and p.max() == 8 and 0.45 < (p > 0).double().mean() < 0.55


_ROUNDING = X.rounding_cases()
_EXACT_ONLY = X.exact_only_cases()


@pytest.mark.parametrize("name,make", _ROUNDING, ids=[n for n, _ in _ROUNDING])
def test_input_conditions_of_16bit_cases(name, make):
    """Every 16-bit forward / data-gradient case: exact regime; bf16 >= 10 % of the non-zero
    reference outputs not representable and >= 5 % exact ties; fp16 >= 5 % / >= 5 % and no
    overflow.  Measured on the reference alone."""
    case = make()
    for k, r in case.ref.items():
        if k in ("gw", "gb", "gk", "routed", "dxu") or k[0] == "_":      # fp32 slabs / exact operands
            continue
        X.require_exact(case.bound, r, case.dtype)
        nr, tie = X.rounding_share(r, case.dtype)
        print("%s %s: bound %.3g, not representable %.1f %%, ties %.1f %%" % (name, k, case.bound, 100 * nr, 100 * tie))
        assert nr >= (0.05 if case.dtype == "fp16" else 0.10), (name, k, nr)
        assert tie >= 0.05, (name, k, tie)
    if "routed" in case.ref:
        f = X.route_final(case)
        X.require_exact(case.bound, f, case.dtype)
        # (the second rounding acts where a pool gradient was routed: at most one pixel in four)
        nr, tie = X.rounding_share(f * (case.ref["routed"] != 0), case.dtype)
        print("%s final, routed elements: not representable %.1f %%, ties %.1f %%" % (name, 100 * nr, 100 * tie))
        assert nr >= 0.10 and tie >= 0.05, (name, nr, tie)


@pytest.mark.parametrize("name,make", _EXACT_ONLY, ids=[n for n, _ in _EXACT_ONLY])
def test_input_conditions_of_fp32_and_statistics_cases(name, make):
    case = make()
    X.require_exact(case.bound)
    for r in case.ref.values():
        assert torch.equal(r.float().double(), r)
    if name.startswith("stats"):
        z = case.ref["y"]
        assert z.abs().max() <= 64 and z[0].numel() // z.shape[-1] <= 4096
        X.require_exact((z * z).reshape(z.shape[0], -1, z.shape[-1]).sum(1))
        X.to_storage(z, "bf16", "cpu")              # |z| <= 64: stored without rounding
