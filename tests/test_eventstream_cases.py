"""The event-stream test inputs reach what they are meant to reach (CPU only).

tests/test_eventstream.py's GPU tests compare eventstream_flat_kernel's results with zlib and cannot
see which path a wave took.  This file checks the other half on the CPU, from the inputs alone: that
tests/eventstream_cases.py's predictor puts each named stream in the class it was built for, that
the named and fuzz streams together cover the kernel's branches (all four hex digits of a join
distance, four end words in one block, the smallest and largest chunk, the exact region bound, ...),
and that the predictor's geometry is the geometry of the model the kernel was written from
(test_eventstream_flat_model.flat_wave_patched), which is checked against zlib on the same waves.
"""
import zlib

import pytest

from tests.eventstream_cases import (ES_MAX_REGION, ES_WAVE, NAMED, NAMED_IDS, fuzz_streams, named_stream, packed,
                                     wave_classes)
from tests.test_eventstream_flat_model import flat_wave_patched


def _offsets(lens, lead):
    offs, pos = [], lead
    for t in lens:
        offs.append(pos)
        pos += t
    return offs, pos


def _classes(name, base=0):
    _, lens, lead = NAMED[NAMED_IDS.index(name)]
    offs, end = _offsets(lens, lead)
    return wave_classes(base, offs, end + 64)


def _flat(name):
    return [c for c in _classes(name) if c["flat"]]


def test_packed_offsets_are_the_running_sum():
    """the predictor is fed offsets computed from the lengths; packed() places the frames there"""
    for name, lens, lead in NAMED:
        blob, offs, want = named_stream(name)
        assert offs == _offsets(lens, lead)[0] and len(blob) == offs[-1] + lens[-1] + 64
        assert len(want) == len(lens)


def test_named_long_frames():
    (c,) = _flat("one_long")
    assert c["C"] == 3168 and c["s0"] == 5 and c["digits"] == {0, 1, 2, 3} and c["span"] == 63
    assert 24000 < c["max_m"] < 25500
    (c,) = _flat("two_long")
    assert c["digits"] == {0, 1, 2, 3} and c["span"] == 33 and c["s0"] == 13
    (c,) = _flat("long_last")
    assert c["digits"] == {0, 1, 2, 3} and c["span"] == 63 and 30500 < c["max_m"] < 32768


def test_named_region_bound():
    """a region of exactly kEsMaxRegion is flat (C 4096, or 4112 when message 0 starts 5 bytes into
    its 16: one more block step of two words); 16 bytes more is not"""
    (c,) = _flat("bound_exact_lead0")
    assert (c["C"], c["nb"], c["wl"], c["s0"]) == (4096, 64, 8, 0)
    (c,) = _flat("bound_exact_lead5")
    assert (c["C"], c["nb"], c["wl"], c["s0"]) == (4112, 65, 2, 5)
    _, lens, _ = NAMED[NAMED_IDS.index("bound_exact_lead0")]
    assert sum(lens[:ES_WAVE]) == ES_MAX_REGION
    w = _classes("bound_over")
    assert w[0] == {"flat": False, "why": "region over the bound"}
    _, lens, _ = NAMED[NAMED_IDS.index("bound_over")]
    assert sum(lens[:ES_WAVE]) == ES_MAX_REGION + 16


def test_named_smallest_chunks():
    for name in ("min_chunk_lead0", "min_chunk_lead16", "min_chunk_lead48", "min_chunk_17"):
        (c,) = _flat(name)
        assert (c["C"], c["nb"], c["wl"], c["s0"]) == (16, 1, 2, 0), name
    (c,) = _flat("min_chunk_lead8")
    assert (c["C"], c["nb"], c["wl"], c["s0"]) == (32, 1, 4, 8)


def test_named_mixes():
    mixed = _flat("mixed")
    assert len(mixed) == 4
    assert any(4 in c["ends"] for c in mixed) and all(2 in c["digits"] for c in mixed)
    assert all(7 <= c["span"] <= 13 for c in mixed)
    mid = _flat("mid")
    assert len(mid) == 4
    assert all(2700 <= c["C"] <= 3200 and 2 in c["digits"] for c in mid)
    _, lens, lead = NAMED[NAMED_IDS.index("mid")]
    offs, _ = _offsets(lens, lead)
    a = set()
    for w0 in range(0, 256, ES_WAVE):  # every a_i = e_i - P_i (the end word's fill) within the flat waves
        rs = offs[w0] & ~15
        a |= {(e - ((e - 1) & ~7)) for e in (offs[i] - rs + lens[i] - 4 for i in range(w0, w0 + ES_WAVE))}
    assert a == set(range(1, 9))
    # four ends in a block whose a classes differ pairwise somewhere: a wrong pw[] select shows
    tiny = _flat("tiny_runs")
    assert len(tiny) == 4 and all(c["nb"] > 1 for c in tiny)
    assert set().union(*(c["sel"] for c in tiny)) == {(j, k) for k in range(4) for j in range(k)}


def test_every_wave_without_a_next_offset_is_left_to_the_lane_path():
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 512, 513, 577):
        offs, end = _offsets([16] * n, 0)
        w = wave_classes(0, offs, end)
        assert len(w) == (n + ES_WAVE - 1) // ES_WAVE
        assert [c["flat"] for c in w] == [True] * ((n - 1) // ES_WAVE) + [False], n


def test_limit_inside_a_wave_sends_it_to_the_lane_path():
    offs, end = _offsets([40] * 129, 0)
    assert [c["flat"] for c in wave_classes(0, offs, end)] == [True, True, False]
    assert [c["flat"] for c in wave_classes(0, offs, offs[128])] == [True, True, False]
    assert [c["flat"] for c in wave_classes(0, offs, offs[128] - 1)] == [True, False, False]
    assert [c["flat"] for c in wave_classes(0, offs, offs[30])] == [False, False, False]


def test_union_of_named_and_fuzz_streams_covers_the_kernel():
    """conditions on the inputs (from the predictor alone), not measurements of the kernel"""
    waves = [c for name in NAMED_IDS for c in _flat(name)]
    streams = fuzz_streams()
    assert len(streams) == 40
    leads, corrupted = set(), 0
    for lens, lead, corrupt, _ in streams:
        assert 65 <= len(lens) <= 321 and min(lens) >= 16
        offs, end = _offsets(lens, lead)
        assert end + 64 <= (1 << 20) + (1 << 12)  # about 1 MiB per stream at the most
        w = wave_classes(0, offs, end + 64)
        assert all(c["flat"] for c in w[:-1]) and not w[-1]["flat"]  # the grammar keeps whole waves under the bound
        waves += [c for c in w if c["flat"]]
        leads.add(lead)
        corrupted += corrupt
    assert leads == set(range(16)) and 12 <= corrupted <= 28
    assert len(waves) >= 60
    assert set().union(*(c["digits"] for c in waves)) == {0, 1, 2, 3}
    assert set().union(*(c["ends"] for c in waves)) == {1, 2, 3, 4}
    assert set().union(*(c["sel"] for c in waves)) == {(j, k) for k in range(4) for j in range(k)}
    assert min(c["C"] for c in waves) == 16 and max(c["C"] for c in waves) >= 4096
    assert max(c["span"] for c in waves) >= 32
    assert set().union(*(c["edge_a"] for c in waves)) == {(edge, a) for edge in (0, 1) for a in range(1, 9)}
    assert {c["wl"] for c in waves} == {2, 4, 6, 8}
    assert any(c["straddle"] for c in waves)
    assert {c["s0"] for c in waves} == set(range(16))
    # the global-memory image branches with more than the few values the named cases give them
    assert max(c["max_m"] for c in waves) >= 0x7000


@pytest.mark.parametrize("name", NAMED_IDS)
def test_named_flat_waves_model_equals_zlib(name):
    """every flat wave of the named cases through the model the kernel was written from: the same
    chunk size as the predictor's, and zlib's CRCs (clean and corrupted bytes alike)"""
    _, lens, lead = NAMED[NAMED_IDS.index(name)]
    for corrupt in (False, True):
        blob, offs, want = named_stream(name, corrupt)
        blob = bytes(blob)
        for w, c in enumerate(wave_classes(0, offs, len(blob))):
            if not c["flat"]:
                continue
            sl = slice(ES_WAVE * w, ES_WAVE * w + ES_WAVE)
            got, C = flat_wave_patched(blob, 0, offs[sl], lens[sl])
            assert C == c["C"]
            assert got == [zlib.crc32(blob[o:o + t - 4]) for o, t in zip(offs[sl], lens[sl])]
            assert got == [x[1] for x in want[sl]]


def test_fuzz_flat_waves_model_equals_zlib():
    """the same for every fourth fuzz stream (the bytes the GPU test uses)"""
    for lens, lead, corrupt, seed in fuzz_streams()[::4]:
        blob, offs, want = packed(lens, seed, lead, corrupt)
        blob = bytes(blob)
        for w, c in enumerate(wave_classes(0, offs, len(blob))):
            if c["flat"]:
                sl = slice(ES_WAVE * w, ES_WAVE * w + ES_WAVE)
                got, C = flat_wave_patched(blob, 0, offs[sl], lens[sl])
                assert C == c["C"] and got == [x[1] for x in want[sl]]


@pytest.mark.parametrize("shift", [1, 3, 8])
def test_unaligned_base_model_equals_zlib(shift):
    """a base that is not 16-aligned moves the region start: predictor and model agree there too"""
    lens = [16 + (7 * i) % 50 for i in range(65)]
    blob, offs, want = packed(lens, 77 + shift, 4)
    mem = bytes(shift) + bytes(blob)
    (c, _) = wave_classes(shift, offs, len(blob))
    assert c["flat"] and c["s0"] == (shift + 4) & 15
    got, C = flat_wave_patched(mem, shift, offs[:ES_WAVE], lens[:ES_WAVE])
    assert C == c["C"] and got == [x[1] for x in want[:ES_WAVE]]
