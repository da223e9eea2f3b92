"""CPU: Python model of the fused CRC32 + CRC32C scan (crc_dual_kernels.hip), checked
against the oracle.  It restates, independently of the C++:

  * the LDS image as dual_build_tables lays it out: lo tables per polynomial (entry e's 256-byte row:
    polynomial p at 128 p, table 7 - q at 32 (3 - q), copy c at 4 c) and the hi tables as 8-byte pairs
    (CRC32 entry, CRC32C entry; table 3 - q at 64 (3 - q), copy c at 8 c);
  * the per-lane slot schedule of DualBraid::init (byte q = (k + j) & 3, j = (lane >> 3) & 3, copy
    lane & 7) with the addresses the v_perm produces, and the banks they meet;
  * the row walk of dual_rows (x_p = u_p ^ lo(w_r); hi(w_r)'s pairs join one step later), the lane
    shares u * x^(-64 l) and the wave XOR;
  * the finish pass: tiles joined by Horner in x^(8 TILE) (and the kernel's tree form of it), the seed
    and head bytes entering times x^(8 mainlen), the tail bytes;
  * the host's geometry (tiles of 1 to 256 groups, front pad, the static split) and the kernel's
    prefetch cursor with its buffer resources: every tile once, every real word once, every address
    inside its buffer's main region.

A failure here is a design bug, not a kernel bug.
"""
import random

import pytest

from oracle import oracle

POLYS = (("crc32", 0xEDB88320), ("crc32c", 0x82F63B78))
M32 = 0xFFFFFFFF
ROW = 512
LO_OFF, HI_OFF = 0, 65536
GROUP = 4096


def mulx(v, P):
    return (v >> 1) ^ (P if v & 1 else 0)


def inv_mulx(t, P):
    return ((((t ^ P) << 1) | 1) & M32) if t & 0x80000000 else (t << 1) & M32


def mulmod(a, b, P):
    m, p = 0x80000000, 0
    while m:
        if a & m:
            p ^= b
        m >>= 1
        b = mulx(b, P)
    return p


def xpow8n(n, P):
    r, sq = 0x80000000, 0x00800000  # x^0, x^8
    while n:
        if n & 1:
            r = mulmod(r, sq, P)
        sq = mulmod(sq, sq, P)
        n >>= 1
    return r


def table_entry(e, k, P):
    c = e
    for _ in range(8 * (k + 1)):
        c = mulx(c, P)
    return c


class DualLds:
    """the 128 KiB of tables exactly as the 1024 threads of dual_build_tables store them"""

    def __init__(self):
        self.mem = bytearray(131072)
        self.written = bytearray(131072)
        Tp = []
        for _, P in POLYS:
            skip = xpow8n(ROW - 8, P)
            Tp.append([[mulmod(table_entry(e, t, P), skip, P) for e in range(256)] for t in range(8)])
        self.Tp = Tp
        for tid in range(1024):
            e, s = tid >> 2, tid & 3
            lo0, lo1 = Tp[0][4 + s][e], Tp[1][4 + s][e]
            hi0, hi1 = Tp[0][s][e], Tp[1][s][e]
            lo = LO_OFF + (e << 8) + (s << 5)
            self._store16(lo, [lo0] * 4)
            self._store16(lo + 16, [lo0] * 4)
            self._store16(lo + 128, [lo1] * 4)
            self._store16(lo + 144, [lo1] * 4)
            hi = HI_OFF + (e << 8) + (s << 6)
            for c in range(4):
                self._store16(hi + 16 * c, [hi0, hi1, hi0, hi1])
        self.K = []
        for _, P in POLYS:
            ks, kl = [], 0x80000000
            for _ in range(64):
                ks.append(kl)
                for _ in range(64):
                    kl = inv_mulx(kl, P)
            self.K.append(ks)

    def _store16(self, a, words):
        assert a % 16 == 0 and not any(self.written[a:a + 16]), a  # every byte stored once
        for i, w in enumerate(words):
            self.mem[a + 4 * i:a + 4 * i + 4] = w.to_bytes(4, "little")
        self.written[a:a + 16] = b"\x01" * 16

    def rd32(self, a):
        assert a % 4 == 0
        return int.from_bytes(self.mem[a:a + 4], "little")

    def rd64(self, a):
        assert a % 8 == 0
        return int.from_bytes(self.mem[a:a + 8], "little")


def lane_consts(lane):
    """DualBraid::init: per slot k the byte q it takes, and the row offsets of the lo and hi reads"""
    j, c = (lane >> 3) & 3, lane & 7
    out = []
    for k in range(4):
        q = (k + j) & 3
        out.append((q, ((3 - q) << 5) | (c << 2), ((3 - q) << 6) | (c << 3)))
    return out


def perm_addr(cst, a, q):
    """v_perm with selector 0x0c0c0004 | q << 8: byte 0 <- the row offset, byte 1 <- byte q of a"""
    return (cst & 255) | (((a >> (8 * q)) & 255) << 8)


@pytest.fixture(scope="module")
def lds():
    return DualLds()


def test_tables_fill_the_regions(lds):
    assert all(lds.written)


def look_hi(lds, lane, hi):
    return [lds.rd64(HI_OFF + perm_addr(chi, hi, q)) for q, _, chi in lane_consts(lane)]


def look_lo(lds, lane, x0, x1, h, wn):
    o0 = o1 = wn
    for (q, clo, _), hv in zip(lane_consts(lane), h):
        o0 ^= lds.rd32(LO_OFF + perm_addr(clo, x0, q)) ^ (hv & M32)
        o1 ^= lds.rd32(LO_OFF + 128 + perm_addr(clo, x1, q)) ^ (hv >> 32)
    return o0, o1


def tile_pair(lds, words_of_lane, rows):
    """one tile: every lane walks its rows as dual_rows does, shares times K_l, wave XOR"""
    r = [0, 0]
    for lane in range(64):
        w = words_of_lane(lane)
        x0 = x1 = w[0] & M32
        h = look_hi(lds, lane, w[0] >> 32)
        for c in range(1, rows):
            x0, x1 = look_lo(lds, lane, x0, x1, h, w[c] & M32)
            h = look_hi(lds, lane, w[c] >> 32)
        u0, u1 = look_lo(lds, lane, x0, x1, h, 0)
        r[0] ^= mulmod(u0, lds.K[0][lane], POLYS[0][1])
        r[1] ^= mulmod(u1, lds.K[1][lane], POLYS[1][1])
    return r


def dual_model(lds, data, addr, seeds, rows):
    """one buffer through both passes, tiles of `rows` rows"""
    n = len(data)
    H, Ea = (addr + 15) & ~15, (addr + n) & ~15
    assert Ea > H
    hoff, mainlen = H - addr, Ea - H
    tile = ROW * rows
    T = -(-mainlen // tile)
    pad = T * tile - mainlen
    acc = [0, 0]
    for k in range(T):
        def words(lane, k=k):
            out = []
            for c in range(rows):
                v = k * tile + ROW * c + 8 * lane  # virtual offset in the padded main region
                out.append(0 if v < pad else int.from_bytes(data[hoff + v - pad: hoff + v - pad + 8], "little"))
            return out

        pair = tile_pair(lds, words, rows)
        for p, (_, P) in enumerate(POLYS):
            acc[p] = mulmod(acc[p], xpow8n(tile, P), P) ^ pair[p]
    out = []
    for p, (_, P) in enumerate(POLYS):
        T0 = [table_entry(e, 0, P) for e in range(256)]
        s = ~seeds[p] & M32
        for b in data[:hoff]:
            s = (s >> 8) ^ T0[(s ^ b) & 255]
        s = mulmod(s, xpow8n(mainlen, P), P) ^ acc[p]
        for b in data[hoff + mainlen:]:
            s = (s >> 8) ^ T0[(s ^ b) & 255]
        out.append(~s & M32)
    return out


@pytest.mark.parametrize("rows", [1, 2, 3, 9])
def test_dual_row_walk_vs_oracle(lds, rows):
    rnd = random.Random(7000 + rows)
    tile = ROW * rows
    for n, addr in ((tile, 0), (tile + 16, 16), (2 * tile + 21, 5), (3 * tile - 16 + 7, 9), (tile // 2 + 48, 15)):
        data = bytes(rnd.getrandbits(8) for _ in range(n))
        for seeds in ((0, 0), (rnd.getrandbits(32), rnd.getrandbits(32)), (0xFFFFFFFF, 0)):
            got = dual_model(lds, data, addr, seeds, rows)
            want = [oracle.crc(name, data, seeds[p]) for p, (name, _) in enumerate(POLYS)]
            assert got == want, (rows, n, addr, seeds)


def test_dual_lds_schedule_conflict_free_and_complete(lds):
    rnd = random.Random(11)
    for half in (range(0, 32), range(32, 64)):
        for k in range(4):
            for _ in range(8):  # whatever bytes the lanes index
                a = {l: rnd.getrandbits(32) for l in half}
                for poly_off in (0, 128):
                    banks = [((LO_OFF + poly_off + perm_addr(lane_consts(l)[k][1], a[l], lane_consts(l)[k][0])) // 4) % 32
                             for l in half]
                    assert len(set(banks)) == 32, ("b32", k)
                pairs = []
                for l in half:
                    ad = HI_OFF + perm_addr(lane_consts(l)[k][2], a[l], lane_consts(l)[k][0])
                    assert ad % 8 == 0
                    pairs += [(ad // 4) % 64, (ad // 4 + 1) % 64]
                assert len(set(pairs)) == 64, ("b64", k)
    # every lane reads every byte of both dwords once, from the table of that byte
    for lane in range(64):
        assert sorted(q for q, _, _ in lane_consts(lane)) == [0, 1, 2, 3]
        for q, clo, chi in lane_consts(lane):
            for e in (0, 1, 0x5A, 255):
                a = e << (8 * q)
                for p in range(2):
                    assert lds.rd32(LO_OFF + 128 * p + perm_addr(clo, a, q)) == lds.Tp[p][7 - q][e]
                v = lds.rd64(HI_OFF + perm_addr(chi, a, q))
                assert (v & M32, v >> 32) == (lds.Tp[0][3 - q][e], lds.Tp[1][3 - q][e])
    # every table and copy is read by some lane and slot, in both regions
    lo_cells = {(clo >> 5, (clo >> 2) & 7) for lane in range(64) for _, clo, _ in lane_consts(lane)}
    hi_cells = {(chi >> 6, (chi >> 3) & 7) for lane in range(64) for _, _, chi in lane_consts(lane)}
    assert lo_cells == hi_cells == {(t, c) for t in range(4) for c in range(8)}


# ---- geometry: engine.cpp dual_impl and the kernel's cursors
WAVES = 16
U32 = 1 << 32


def dual_plan(base, stride, length, count, cus):
    H, Ea = (base + 15) & ~15, (base + length) & ~15
    ml = Ea - H if Ea > H else 0
    if ml < GROUP:
        return None  # the two single scans
    G = 1  # the largest tile of 256, 64, 16 or 4 groups that still gives every wave slot a tile
    for g in (256, 64, 16, 4):
        if g * GROUP <= ml and count * -(-ml // (g * GROUP)) >= cus * WAVES:
            G = g
            break
    tile = G * GROUP
    T = -(-ml // tile)
    ntiles = T * count
    blocks = min(cus, -(-ntiles // WAVES))
    nw = blocks * WAVES
    fth = 64
    while fth < 1024 and fth < T:
        fth <<= 1
    return dict(base=base, stride=stride, hoff=H - base, ml=ml, G=G, tile=tile, T=T, ntiles=ntiles, pad=T * tile - ml,
                blocks=blocks, q=ntiles // nw, r=ntiles % nw, count=count, fth=fth)


def wave_walk(pl, gw):
    """crc32_dual_stream_kernel for wave gw: (tile stored, buffer, addresses loaded) per tile.  Every group
    is read through a buffer resource over its real bytes: lane offsets past the records load zeros."""
    t0 = gw * pl["q"] + min(gw, pl["r"])
    ntw = pl["q"] + (1 if gw < pl["r"] else 0) if t0 < pl["ntiles"] else 0
    G, T, tile, pad = pl["G"], pl["T"], pl["tile"], pl["pad"]
    nq = ntw * G
    if nq == 0:
        return []
    fb, fk = divmod(t0, T)
    fg = fq = 0
    fmain = pl["base"] + fb * pl["stride"] + pl["hoff"]
    groups = []
    steps = -(-nq // 3) * 3  # whole rotations: up to two placeholder groups after the last
    for _ in range(steps + 2):  # the two groups issued ahead included
        v = fk * tile + fg * GROUP
        adj = 0 if v >= pad else min(pad - v, GROUP)
        real = fq < nq
        rec = GROUP - adj if real else 0
        rs_base = fmain + v - pad + adj if real else None
        loads = []
        for lane in range(64 if adj or not real else 0):
            o0 = (8 * lane - adj) % U32 if real else 8 * lane
            for R in range(8):
                o = min((o0 + ROW * R) % U32, rec)
                if o + 8 <= rec:  # the resource's range check; otherwise the lane word is zero
                    loads.append((R, lane, rs_base + o))
        loads.sort()
        addrs = [a for _, _, a in loads]
        if real and not adj:  # no lane is clamped: the 512 words of the group (the loop above, in closed form)
            addrs = list(range(rs_base, rs_base + GROUP, 8))
        groups.append((fb if real else None, addrs))
        fq += 1  # f_next
        if fq < nq:
            fg += 1
            if fg == G:
                fg = 0
                fk += 1
                if fk == T:
                    fk, fb = 0, fb + 1
                    fmain += pl["stride"]
    assert all(not ld for _, ld in groups[nq:])  # placeholders read nothing
    out, st, tend = [], t0, t0 + ntw
    for i in range(0, steps, G):  # the scan cursor (step): one finish per G groups, stored below tend only
        if st < tend:
            out.append((st, groups[i][0], [a for _, lds_ in groups[i:i + G] for a in lds_]))
        st += 1
    return out


@pytest.mark.parametrize("length,offset,count,cus", [
    (4096, 0, 1, 256), (4096, 0, 5, 256), (3 * 4096 + 21, 5, 300, 256), (8192, 0, 4096, 256),
    (4096 + 15, 1, 3, 4), (65536, 0, 3, 2), (65536 - 16, 16, 2, 256), (300 * 1024 + 3, 13, 7, 8),
    (1048576 + 5, 7, 1, 256), (4 << 20, 0, 2, 16), ((4 << 20) + 4096 + 33, 3, 2, 4), (5000, 9, 17, 1),
    ((16 << 20) + 48, 11, 1, 1), ((2 << 20) - 4096 + 7, 2, 3, 2), ((1 << 20) - 64 + 9, 5, 8, 1),
])
def test_tile_and_wave_walk(length, offset, count, cus):
    for stride in ((length + 15) & ~15, 0) if count > 1 else (length,):
        base = 0x7F0000100000 + offset
        pl = dual_plan(base, stride, length, count, cus)
        assert pl is not None and pl["pad"] < pl["tile"]
        assert pl["G"] == {(16 << 20) + 48: 256, (1 << 20) - 64 + 9: 64, (4 << 20) + 4096 + 33: 16}.get(length, pl["G"])
        seen = {}
        for gw in range(pl["blocks"] * WAVES):
            for st, b, loads in wave_walk(pl, gw):
                assert st not in seen
                seen[st] = (b, loads)
        assert sorted(seen) == list(range(pl["ntiles"]))  # every tile exactly once
        T = pl["T"]
        for st, (b, loads) in seen.items():
            assert b == st // T
            lo = pl["base"] + b * stride + pl["hoff"]
            k = st % T
            want0 = lo if k == 0 else lo + k * pl["tile"] - pl["pad"]
            want1 = lo + (k + 1) * pl["tile"] - pl["pad"]
            assert lo <= want0 < want1 <= lo + pl["ml"]             # inside the main region
            assert sorted(loads) == list(range(want0, want1, 8))   # each real word exactly once


def test_tile_sizes_follow_the_wave_slots():
    big = dual_plan(0x1000, 256 << 20, 256 << 20, 16, 256)
    assert (big["G"], big["T"], big["ntiles"], big["fth"]) == (256, 256, 4096, 256)
    mid = dual_plan(0x1000, 64 << 20, 64 << 20, 16, 256)
    assert (mid["G"], mid["T"], mid["fth"]) == (64, 256, 256)
    two = dual_plan(0x1000, 64 << 20, 64 << 20, 2, 256)
    assert (two["G"], two["T"], two["fth"]) == (4, 4096, 1024)
    assert dual_plan(0x1000, 8192, 8192, 4096, 256)["G"] == 1
    assert dual_plan(0x1007, 0, (1 << 20) + 5, 1, 256)["T"] == 256  # G = 1: 1 MiB - 16 of main + the pad


def finish_tree(pairs, nth, xlev):
    """crc32_dual_finish_kernel's join of one buffer's T tile pairs with nth threads (one polynomial's
    values; xlev[l] = x^(8 TILE 2^l))"""
    T = len(pairs)
    P = xlev["P"]
    lp = 0
    while (nth << lp) < T:
        lp += 1
    per = 1 << lp
    parts = (T + per - 1) >> lp
    ne = 1
    while ne < parts:
        ne <<= 1
    assert ne <= nth
    zero = per * ne - T
    v = [0] * nth
    for tid in range(ne):
        a = 0
        for j in range(tid * per, (tid + 1) * per):
            if j < zero:
                continue
            a = mulmod(a, xlev[0], P) ^ pairs[j - zero]
        v[tid] = a
    s, lev = 1, lp
    while s < ne:
        for tid in range(0, ne, 2 * s):
            v[tid] = mulmod(v[tid], xlev[lev], P) ^ v[tid + s]
        s, lev = s << 1, lev + 1
    return v[0]


@pytest.mark.parametrize("name,P", POLYS)
def test_finish_tree_is_horner(name, P):
    rnd = random.Random(99)
    tile = 4096
    xlev = {"P": P, 0: xpow8n(tile, P)}
    for l in range(1, 32):
        xlev[l] = mulmod(xlev[l - 1], xlev[l - 1], P)
    assert xlev[5] == xpow8n(tile * 32, P)
    for T in (1, 2, 3, 5, 63, 64, 65, 100, 257, 1024, 1025, 3000, 4096):
        fth = 64
        while fth < 1024 and fth < T:
            fth <<= 1
        pairs = [rnd.getrandbits(32) for _ in range(T)]
        want = 0
        for r in pairs:
            want = mulmod(want, xlev[0], P) ^ r
        assert finish_tree(pairs, fth, xlev) == want, T


def test_short_buffers_take_the_single_scans():
    for length, offset in ((0, 0), (1, 0), (17, 0), (1000, 0), (4095, 0), (4096 + 14, 1), (4096 + 13, 2)):
        assert dual_plan(0x1000 + offset, 0, length, 1, 256) is None, (length, offset)
    for length, offset in ((4096, 0), (4096 + 15, 1), (4112, 0)):
        assert dual_plan(0x1000 + offset, 0, length, 1, 256) is not None, (length, offset)
