"""Bank-conflict model for gfx950 LDS (MI355X_MICROARCH.md §LDS) used to
check the swizzles of the conv kernels before they run on hardware.

Each instruction is serviced in lane groups; within a group every extra
distinct address on a busy bank costs one cycle.  Returns the max ways."""

B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
               list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
               list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
               list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
HALVES = [list(range(0, 32)), list(range(32, 64))]


def ways(addrs, nbytes, groups, nbanks):
    worst = 1
    for g in groups:
        banks = {}
        for l in g:
            a = addrs[l]
            for d in range(nbytes // 4):
                b = (a // 4 + d) % nbanks
                banks.setdefault(b, set()).add(a // 4 + d)
        worst = max(worst, max(len(v) for v in banks.values()))
    return worst


def read_b128(addrs):
    return ways(addrs, 16, B128_GROUPS, 64)


def read_tr_b64(addrs):
    return ways(addrs, 8, HALVES, 64)


def write_b128(addrs):
    return ways(addrs, 16, [list(range(i, i + 8)) for i in range(0, 64, 8)], 32)


def write_b64(addrs):
    return ways(addrs, 8, [list(range(i, i + 16)) for i in range(0, 64, 16)], 32)


# ---------------------------------------------------------------- conv fwd
# LDS tile [row][32 bf16] = 64 B rows; 16x16x32 fragment: lane l reads row
# (r0 + l&15), 16-byte chunk (l>>4).  Physical chunk = c ^ G[(row>>2)&3].
G = [0, 2, 3, 1]


def fwd_addr(row, c):
    return row * 64 + 16 * (c ^ G[(row >> 2) & 3])


def check_fwd():
    worst = 1
    for r0 in range(0, 256, 16):
        worst = max(worst, read_b128([fwd_addr(r0 + (l & 15), l >> 4) for l in range(64)]))
    # writes: thread t writes row t>>2 chunk t&3
    for base in range(0, 256, 64):
        worst = max(worst, write_b128([fwd_addr(base // 4 * 0 + (base + l) >> 2, (base + l) & 3) for l in range(64)]))
    return worst


# ---------------------------------------------------------------- wgrad tr-read
# LDS image [k][m] (m contiguous), row bytes RB = BM*2; 32-byte blocks
# (16 m) XOR-swizzled by s(k).
def tr_swz(k, nb):
    if nb == 2:
        return (k >> 3) & 1
    if nb == 4:
        return ((k >> 1) & 1) | (((k >> 3) & 1) << 1)
    if nb >= 8:
        return (k & 3) | (((k >> 3) & 1) << 2)
    return 0


def tr_addr(k, m, BM):
    nb = BM // 16
    blk = (m // 16) ^ tr_swz(k, nb)
    return k * BM * 2 + blk * 32 + (m % 16) * 2


def check_tr(BM):
    worst = 1
    for k0 in range(0, 64, 32):
        for mb in range(BM // 16):
            for half in range(2):     # first / second 4-row read
                addrs = []
                for l in range(64):
                    g, i = l >> 4, l & 15
                    q, p = i >> 2, i & 3
                    k = k0 + 8 * g + 4 * half + q
                    addrs.append(tr_addr(k, mb * 16 + 4 * p, BM))
                worst = max(worst, read_tr_b64(addrs))
    # writes: thread writes 8 consecutive m of one k; chunks row-major
    wworst = 1
    cpr = BM // 8
    for base in range(0, 32 * cpr, 64):
        addrs = []
        for l in range(64):
            t = base + l
            k, c = t // cpr, t % cpr
            addrs.append(tr_addr(k, c * 8, BM))
        wworst = max(wworst, write_b128(addrs))
    return worst, wworst


# ---------------------------------------------------------------- conv_win XF 5 u stores
# tconv-on-load (conv_win.h ut_chunk): lane (fr = l & 15, fsub = l >> 4) holds u channels
# 8 fsub .. + 7 of coarse pixel 16 pb + fr for both column phases tw; fine halo column
# hc = 2 (16 pb + fr) + tw + 1, 64-byte slots, physical chunk fsub ^ ((hc >> 1) & 3).
def check_ut_store():
    """(ways of the old 8-byte per-tile stores, ways of one phase per 16-byte store,
    ways of the phase-interleaved 16-byte stores)."""
    def a16(fr, fsub, tw, pb):
        hc = 2 * (16 * pb + fr) + tw + 1
        return hc * 64 + 16 * (fsub ^ ((hc >> 1) & 3))
    old = one = inter = 1
    for pb in range(4):
        for tw in range(2):
            for j in range(2):        # old: chunk 2 j + (fsub >> 1), half fsub & 1
                addrs = []
                for l in range(64):
                    fr, fsub = l & 15, l >> 4
                    hc = 2 * (16 * pb + fr) + tw + 1
                    ch = 2 * j + (fsub >> 1)
                    addrs.append(hc * 64 + 16 * (ch ^ ((hc >> 1) & 3)) + 8 * (fsub & 1))
                old = max(old, write_b64(addrs))
            one = max(one, write_b128([a16(l & 15, l >> 4, tw, pb) for l in range(64)]))
        for s in range(2):
            inter = max(inter, write_b128([a16(l & 15, l >> 4, s ^ (((l & 15) >> 2) & 1), pb) for l in range(64)]))
    return old, one, inter


# ---------------------------------------------------------------- conv epilogue staging (BN = 32)
# conv_epilogue.h: 64-byte pixel rows, chunk c of pixel ml at c ^ ((ml >> 2) & 3); the
# register phase writes 8-byte halves (lane: pixel base + (l & 15), channels 16 j + 4 (l >> 4)),
# the coalesced phase reads 16-byte chunks (thread t: pixel t >> 2, chunk t & 3).
def check_epi(half_swap=True):
    """(write ways, read ways) of the staging tile."""
    def eoff(ml, ch):
        return ml * 64 + 16 * (ch ^ ((ml >> 2) & 3))
    w = r = 1
    for base in range(0, 512, 16):
        for j in range(2):
            addrs = []
            for l in range(64):
                ml, nl = base + (l & 15), 16 * j + 4 * (l >> 4)
                h = (2 * (nl & 7)) ^ (8 * ((ml >> 1) & 1) if half_swap else 0)
                addrs.append(eoff(ml, nl >> 3) + h)
            w = max(w, write_b64(addrs))
    for base in range(0, 2048, 64):
        r = max(r, read_b128([eoff((base + l) >> 2, (base + l) & 3) for l in range(64)]))
    return w, r


# ---------------------------------------------------------------- generic wgrad_kernel stores
# conv_wgrad.hip wgrad_kernel: 4 threads per pixel row k (tid >> 2), thread's chunk group c
# (chunks sub + 4 c of the row) -> [k][W] transposed-read image; SWP: odd rows take c ^ 1.
def check_wgrad_store(W, swap=True):
    worst = 1
    for wave in range(4):
        for c in range(W // 32):
            addrs = []
            for l in range(64):
                tid = 64 * wave + l
                k, sub = tid >> 2, tid & 3
                cc = c ^ (k & 1) if swap else c
                addrs.append(tr_addr(k, 8 * (sub + 4 * cc), W))
            worst = max(worst, write_b128(addrs))
    return worst


# ---------------------------------------------------------------- tconv_fwd epilogue staging
# conv_fwd.hip tconv_fwd_kernel: register phase, wave = tap (th, tw), lane: coarse pixel
# 16 i + (l & 15) -> fine pixel fp (2 apart along a fine row), 8-byte half h of chunk c of
# channels 16 j + 4 (l >> 4); coalesced phase: thread t -> fine pixel t >> 2, chunk t & 3.
# 64-byte rows: fine pixel fp in row fp ^ ((fp >> 1) & 1), chunk c ^ ((fp >> 2) & 3), half
# h ^ ((fp >> 4) ^ (fp >> 5)) & 1; `padded`: the previous 72-byte rows (half ^ (fp >> 4) & 1).
def check_tconv_epi(W, padded=False):
    def off(fp, c, h):
        if padded:
            return fp * 72 + 16 * c + 8 * (h ^ ((fp >> 4) & 1))
        return (fp ^ ((fp >> 1) & 1)) * 64 + 16 * (c ^ ((fp >> 2) & 3)) + 8 * (h ^ (((fp >> 4) ^ (fp >> 5)) & 1))
    w = 1
    for wave in range(4):
        th, tw = wave >> 1, wave & 1
        for i in range(8):
            for j in range(2):
                addrs = []
                for l in range(64):
                    pl = 16 * i + (l & 15)
                    rr, x = divmod(pl, W)
                    fp = (2 * rr + th) * (2 * W) + 2 * x + tw
                    nl = 16 * j + 4 * (l >> 4)
                    addrs.append(off(fp, nl >> 3, (nl >> 2) & 1))
                w = max(w, write_b64(addrs))
    r = 1
    for base in range(0, 2048, 64):
        if padded:      # two 8-byte reads per chunk (72-byte rows are not 16-byte aligned)
            for hh in range(2):
                addrs = [off((base + l) >> 2, (base + l) & 3, hh) for l in range(64)]
                r = max(r, ways(addrs, 8, HALVES, 64))
        else:
            r = max(r, read_b128([off((base + l) >> 2, (base + l) & 3, 0) for l in range(64)]))
    return w, r


# ---------------------------------------------------------------- gather_aug tile transpose
# gather.h gather_copy_tile_kernel: 32 x 32 pixel tile, a pixel is nw dwords (2: Cpad 4 in
# 16 bits; 4: Cpad 8 in 16 bits or Cpad 4 in fp32; 8: Cpad 8 in fp32), rows of 32 nw + pad
# dwords.  Lane (r, c) = (tid >> 5, tid & 31) writes pixel [r + 8 i][c] and reads back
# [c][r + 8 i]; 8-byte accesses for nw = 2, 16-byte pieces otherwise.  The target planes are
# fp32 [32][33]: 4-byte accesses, same lane map.
def read_b64(addrs):
    return ways(addrs, 8, HALVES, 64)


def check_gather_aug(nw, pad=None):
    """(write ways, transposed-read ways) of the image tile."""
    pitch = 32 * nw + ((2 if nw == 2 else 4) if pad is None else pad)
    wr, rd = (write_b64, read_b64) if nw == 2 else (write_b128, read_b128)
    w = r = 1
    for wave in range(4):
        for i in range(4):
            lanes = [((64 * wave + l) >> 5) + 8 * i for l in range(64)]
            for q in range(0, nw, 4 if nw > 2 else 2):
                w = max(w, wr([4 * (lanes[l] * pitch + (l & 31) * nw + q) for l in range(64)]))
                r = max(r, rd([4 * ((l & 31) * pitch + lanes[l] * nw + q) for l in range(64)]))
    return w, r


def check_gather_aug_target(pitch=33):
    """(write ways, transposed-read ways) of one fp32 target plane."""
    w = r = 1
    for wave in range(4):
        for i in range(4):
            rows = [((64 * wave + l) >> 5) + 8 * i for l in range(64)]
            w = max(w, ways([4 * (rows[l] * pitch + (l & 31)) for l in range(64)], 4, HALVES, 32))
            r = max(r, ways([4 * ((l & 31) * pitch + rows[l]) for l in range(64)], 4, HALVES, 32))
    return w, r


# ---------------------------------------------------------------- tta_acc tile transpose
# tta.h tta_acc_kernel: 32 x 32 pixel tile of K fp32 per pixel, rows of 33 K floats.  Lane
# tid's float f = tid + 256 i (i < 4 K) is pixel q = f // K, class k = f % K: written at
# [q >> 5][(q & 31) K + k] (a row of the source) and read back from [q & 31][(q >> 5) K + k]
# (a row of the output); 4-byte accesses, serviced in 32-lane halves over 32 banks.
def check_tta_tile(K, pitch=None):
    """(write ways, transposed-read ways) of the probability tile."""
    pitch = 33 * K if pitch is None else pitch
    w = r = 1
    for wave in range(4):
        for i in range(4 * K):
            f = [64 * wave + l + 256 * i for l in range(64)]
            q = [v // K for v in f]
            k = [v % K for v in f]
            w = max(w, ways([4 * ((q[l] >> 5) * pitch + (q[l] & 31) * K + k[l]) for l in range(64)], 4, HALVES, 32))
            r = max(r, ways([4 * ((q[l] & 31) * pitch + (q[l] >> 5) * K + k[l]) for l in range(64)], 4, HALVES, 32))
    return w, r


if __name__ == "__main__":
    print("tta_acc tile (write, transposed read) ways K=1..4, unpadded:",
          [check_tta_tile(K) for K in (1, 2, 3, 4)], [check_tta_tile(K, 32 * K) for K in (1, 2, 3, 4)])
    print("gather_aug tile (write, transposed read) ways nw=2/4/8, unpadded nw=2/4:",
          [check_gather_aug(n) for n in (2, 4, 8)], [check_gather_aug(n, 0) for n in (2, 4)],
          "target plane:", check_gather_aug_target(), check_gather_aug_target(32))
    print("fwd b128 read/write worst ways:", check_fwd())
    for BM in (32, 64, 128, 256):
        print("tr BM=%d read/write ways:" % BM, check_tr(BM))
    print("epilogue staging (write, read) ways, half swap / none:", check_epi(), check_epi(False))
    print("wgrad_kernel stores W=64/128/256 (swap, none):",
          [(check_wgrad_store(w), check_wgrad_store(w, False)) for w in (64, 128, 256)])
    print("tconv_fwd staging W=8..64 (new, padded):",
          [(check_tconv_epi(w), check_tconv_epi(w, True)) for w in (8, 16, 32, 64)])
    print("XF 5 u stores (old b64, one-phase b128, interleaved b128) ways:", check_ut_store())


# ---------------------------------------------------------------- 128-byte rows (BK = 64)
def find_swz128():
    """Search XOR swizzles chunk' = chunk ^ (A . bits(row & 15)) over GF(2) for
    conflict-free ds_read_b128 16x16x32 fragment reads on [row][64 bf16] tiles."""
    import itertools
    best = None
    for cols in itertools.product(range(8), repeat=4):     # images of row bits 0..3
        def f(r):
            v = 0
            for b in range(4):
                if (r >> b) & 1:
                    v ^= cols[b]
            return v
        worst = 1
        for kh2 in range(2):
            addrs = [(l & 15) * 128 + 16 * (((l >> 4) + 4 * kh2) ^ f(l & 15)) for l in range(64)]
            worst = max(worst, read_b128(addrs))
        if worst == 1:
            return cols
        if best is None or worst < best[0]:
            best = (worst, cols)
    return best
