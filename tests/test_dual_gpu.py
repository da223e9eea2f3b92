"""GPU: aws_crt_amd_crc32_dual_strided (CRC32 and CRC32C of the same bytes from one read) against the
oracle, bit-exact in both columns.  The fused kernel's smallest tile is 4 KiB: buffers whose
16-byte-aligned main region holds one take the fused kernel (dual_fused_launches rises), shorter ones
the two single scans and the pairing kernel.  One random device buffer and its host copy serve every
test; seeds are random 32-bit values unless a test says otherwise."""
import random

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

TILE = 4096
POOL = (128 << 20) + 4096
CRC32, CRC32C = 0, 1


@pytest.fixture(scope="module")
def pool(engine):
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(707)
    d = torch.randint(0, 256, (POOL,), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    return d, d.cpu().numpy()


def seed_pairs(rng, count):
    return [(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(count)]


def seeds_tensor(pairs):
    import torch

    a = np.array(pairs, dtype=np.uint32).reshape(-1, 2).view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def pairs_of(out):
    a = out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    return [(int(x), int(y)) for x, y in a]


def want_pairs(h, off, stride, L, count, seeds=None):
    out = []
    for i in range(count):
        b = h[off + i * stride: off + i * stride + L]
        s = seeds[i] if seeds else (0, 0)
        out.append((oracle.crc("crc32", b, s[0]), oracle.crc("crc32c", b, s[1])))
    return out


def run(engine, d, L, off, count, stride, seeds=None, stream=None):
    import torch

    st = seeds_tensor(seeds) if seeds else None
    out = engine.checksum_dual_strided(d, stride, L, count, seeds=st, stream=stream, base_offset=off)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (count, 2) and out.dtype == torch.int32
    return pairs_of(out)


@pytest.mark.parametrize("L,off,count,fused", [
    (0, 0, 5, False),                  # empty buffers: the results are the seeds
    (1, 0, 33, False),                 # the two single scans and the pairing kernel
    (17, 0, 64, False),
    (1000, 0, 257, False),
    (TILE, 0, 1, True),                # one tile
    (TILE, 0, 5, True),                # fewer tiles than waves
    (3 * TILE + 21, 5, 300, True),     # head and tail around whole tiles, several tiles per buffer
    (8192, 0, 4096, True),             # more buffers than waves (8 KiB >= tile)
    ((1 << 20) + 5, 7, 1, True),       # 256 tiles in one buffer (the last 16 bytes short: a front pad)
    (64 << 20, 0, 2, True),            # long buffers, all CUs, 4096 tiles of 16 KiB each: 1024 finish threads, 4 tiles per thread
])
def test_strided_shapes(engine, pool, L, off, count, fused):
    d, h = pool
    stride = (L + 15) & ~15
    rng = random.Random(L * 31 + count)
    seeds = seed_pairs(rng, count)
    before = engine.dual_fused_launches()
    got = run(engine, d, L, off, count, stride, seeds)
    rose = engine.dual_fused_launches() - before
    assert rose == (1 if fused else 0), (L, off, count, rose)
    assert got == want_pairs(h, off, stride, L, count, seeds)
    if L == 0:
        assert got == seeds


@pytest.mark.parametrize("mib,groups", [(4, 16), (16, 64), (64, 256)])
def test_large_tiles(engine, pool, mib, groups):
    """tiles of 64 KiB, 256 KiB and 1 MiB: taken once a call has a tile of that size for each of the
    device's 4096 wave slots -- here 64 seed pairs over one buffer (stride 0), with a front pad"""
    import torch

    assert torch.cuda.get_device_properties(0).multi_processor_count * 16 == 64 * (mib << 20) // (groups * 4096)
    d, h = pool
    L, off, count = (mib << 20) + 5, 3, 64  # main region 16 bytes short of whole tiles: a front pad
    seeds = seed_pairs(random.Random(mib), count)
    got = run(engine, d, L, off, count, 0, seeds)
    b = h[off: off + L]
    # one oracle pass per polynomial: a seed enters a CRC as crc(b, s) = crc(b, 0) ^ (crc(z, s) ^ crc(z, 0)), z = zeros
    z = np.zeros(L, dtype=np.uint8)
    for col, name in ((0, "crc32"), (1, "crc32c")):
        c0, z0 = oracle.crc(name, b), oracle.crc(name, z)
        for i in (0, 1, 31, 63):
            assert got[i][col] == oracle.crc(name, b, seeds[i][col]), (name, i)
        for i in range(count):  # crc(z, s) = combine(s, crc(z, 0), |z|)
            assert got[i][col] == c0 ^ oracle.combine(name, seeds[i][col], z0, L) ^ z0, (name, i)


@pytest.mark.parametrize("off", range(16))
def test_every_head_alignment(engine, pool, off):
    d, h = pool
    L = 2 * TILE + 3
    seeds = seed_pairs(random.Random(off), 1)
    assert run(engine, d, L, off, 1, L, seeds) == want_pairs(h, off, L, L, 1, seeds)


def test_seeds(engine, pool):
    d, h = pool
    L, off, count = 2 * TILE + 40, 3, 4
    stride = (L + 15) & ~15
    # NULL seeds are zero seeds
    assert run(engine, d, L, off, count, stride) == run(engine, d, L, off, count, stride, [(0, 0)] * count) \
        == want_pairs(h, off, stride, L, count)
    # the columns keep their own seeds
    for pair in ((0xFFFFFFFF, 0), (0, 0xFFFFFFFF)):
        for n in (L, 100):  # the fused kernel and the single scans
            got = run(engine, d, n, off, 1, n, [pair])
            assert got == want_pairs(h, off, n, n, 1, [pair]), (pair, n)
            assert got != want_pairs(h, off, n, n, 1, [pair[::-1]])
    # stride 0: one buffer under four seed pairs
    seeds = seed_pairs(random.Random(5), 4)
    for n in (L, 100):
        assert run(engine, d, n, off, 4, 0, seeds) == want_pairs(h, off, 0, n, 4, seeds), n


def test_running_crc(engine, pool):
    """a 4 MiB buffer in 4 chunks, each call seeded with the previous results, equals the one-shot
    result, the oracle, and combine_batch of the unseeded chunk results per column"""
    import torch

    d, h = pool
    L, off, parts = 4 << 20, 16, 4
    n = L // parts
    one = run(engine, d, L, off, 1, L)
    assert one == want_pairs(h, off, L, L, 1)
    st = None
    for i in range(parts):
        st = engine.checksum_dual_strided(d, n, n, 1, seeds=st, base_offset=off + i * n)
    torch.cuda.synchronize()
    assert pairs_of(st) == one
    chunks = engine.checksum_dual_strided(d, n, n, parts, base_offset=off)  # unseeded, one call
    torch.cuda.synchronize()
    for col, alg in ((0, CRC32), (1, CRC32C)):
        acc = chunks[0:1, col].contiguous()
        for i in range(1, parts):
            acc = engine.combine_batch(alg, acc, chunks[i:i + 1, col].contiguous(), [n])
        torch.cuda.synchronize()
        assert int(acc.cpu().numpy().view(np.uint32)[0]) == one[0][col], col


def test_two_streams(engine, pool):
    import torch

    d, h = pool
    L, count = 3 * TILE + 21, 40
    stride = (L + 15) & ~15
    offs = (5, 5 + (1 << 20))
    s = (torch.cuda.Stream(), torch.cuda.Stream())
    torch.cuda.synchronize()
    outs = []
    for rnd in range(3):
        for k in (0, 1):
            outs.append((k, engine.checksum_dual_strided(d, stride, L, count, stream=s[k], base_offset=offs[k])))
    torch.cuda.synchronize()
    want = [want_pairs(h, o, stride, L, count) for o in offs]
    for k, o in outs:
        assert pairs_of(o) == want[k]
    for st in s:
        engine.stream_release(st)


def test_graph_capture_replay(engine):
    """captured on one stream after a warm-up call of the same shape (no forked branches), replayed on
    changed data, as tests/test_gpu_parity.py::test_graph_capture_replay does for the single scans"""
    import torch

    L, count = 5 * TILE + 16 + 9, 24
    stride = (L + 15) & ~15
    g0 = torch.Generator(device="cuda")

    def fill(t, seed):
        g0.manual_seed(seed)
        t.copy_(torch.randint(0, 256, t.shape, dtype=torch.uint8, device="cuda", generator=g0))

    d = torch.empty(count * stride + 16, dtype=torch.uint8, device="cuda")
    fill(d, 51)
    s = torch.cuda.Stream()
    out = torch.empty((count, 2), dtype=torch.int32, device="cuda")
    with torch.cuda.stream(s):
        engine.checksum_dual_strided(d, stride, L, count, out=out, stream=s, base_offset=1)  # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        engine.checksum_dual_strided(d, stride, L, count, out=out, stream=s, base_offset=1)
    for it in range(3):
        if it:
            fill(d, 60 + it)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        assert pairs_of(out) == want_pairs(d.cpu().numpy(), 1, stride, L, count), it


def test_fuzz(engine, pool):
    d, h = pool
    rng = random.Random(20261)
    for case in range(40):
        L = rng.choice([rng.randrange(0, 300 << 10), rng.randrange(0, 20000), rng.randrange(4000, 4200)])
        off, count = rng.randrange(16), rng.randrange(1, 41)
        stride = (L + 15) & ~15 if count > 1 else L
        seeds = seed_pairs(rng, count) if rng.random() < 0.7 else None
        got = run(engine, d, L, off, count, stride, seeds)
        assert got == want_pairs(h, off, stride, L, count, seeds), (case, L, off, count)
