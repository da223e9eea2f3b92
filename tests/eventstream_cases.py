"""Inputs for the event-stream framing tests (tests/test_eventstream.py, tests/test_eventstream_cases.py):
a packed-stream builder, a predictor of what eventstream_flat_kernel does with each wave of 64 offsets,
and the streams -- a named list and a seeded fuzz grammar -- chosen with that predictor so that the
kernel's rarely taken branches are reached.  Plain helpers, no fixtures.

The GPU tests cannot observe which path a wave took (the result is the same either way, that is the
point); which wave is flat, with what chunk size and which join distances, is predicted here on the CPU
from the offsets, and tests/test_eventstream_cases.py asserts that the predicted classes cover the
kernel's branches and that the geometry agrees with the model the kernel was written from.
"""
import random
import struct
import zlib

# wave_classes mirrors these constants of aws-crt-cpp_amd/csrc/crc_kernels.hip; whoever changes them
# there changes them here:
#   kEsMaxRegion = 256 KiB   the largest off_next[63] - off[0] a flat wave may span
#   a wave = 64 frames       lane l owns frame 64 w + l and chunk l of the wave's region
#   kEsBlock = 512 threads   8 waves per workgroup: a multiple of 64, so wave w of the launch is
#                            offsets[64 w .. 64 w + 63] whatever the workgroup
#   16-byte region start and end alignment, chunk size C a multiple of 16, 64-byte block steps,
#   8-byte words, four hex digits of a join distance (digits 0, 1 from LDS images, 2, 3 from global)
ES_MAX_REGION = 256 << 10
ES_WAVE = 64
ES_BLOCK = 512

MALFORMED = (0, 0, 4)


def packed(lens, seed, lead=0, corrupt=False):
    """messages packed back to back after `lead` bytes (a stream of frames, eventstream_flat_kernel's
    shape), with correct stored CRCs unless corrupted; returns blob, offsets, expected (pre, msg, st)"""
    rng = random.Random(seed)
    blob = bytearray(rng.randbytes(lead))
    offs, want = [], []
    for i, total in enumerate(lens):
        offs.append(len(blob))
        m = bytearray(struct.pack(">II", total, rng.randint(0, total - 16)) + bytes(4) + rng.randbytes(total - 12))
        pre = zlib.crc32(bytes(m[:8]))
        m[8:12] = struct.pack(">I", pre)
        msg = zlib.crc32(bytes(m[:total - 4]))
        m[total - 4:] = struct.pack(">I", msg)
        st = 3
        if corrupt and i % 5 == 1:  # stored prelude CRC wrong
            m[9] ^= 0x10
            msg = zlib.crc32(bytes(m[:total - 4]))
            m[total - 4:] = struct.pack(">I", msg)
            st = 2
        elif corrupt and i % 5 == 2:  # body flipped after the message CRC was stored
            m[rng.randrange(12, total - 4) if total > 16 else 12] ^= 0x04
            msg = zlib.crc32(bytes(m[:total - 4]))
            st = 1
        elif corrupt and i % 5 == 3:  # stored message CRC wrong
            m[total - 1] ^= 0x80
            st = 1
        blob += m
        want.append((pre, msg, st))
    blob += rng.randbytes(64)
    return blob, offs, want


def wave_classes(base_addr, offsets, limit):
    """What each wave of 64 offsets does in eventstream_flat_kernel, from the offsets alone: one dict
    per wave.  {"flat": False, "why": ...} for a wave the kernel leaves to its one-lane-per-message
    path; for a flat wave (the preludes must then still agree with the offsets, which is theirs to do)

      s0, C, nb, wl   message 0's start in the region, chunk bytes, block steps, words of the last step
      digits          the hex digits d with a non-zero nibble in some join distance m (es_shift_words)
      max_m, span     the largest join distance in words; the most chunks one frame's join covers
      ends            the set of end-word counts met in one 64-byte block of one lane's chunk
      sel             the pairs (j, k), j < k, of ends in one such block whose a_i differ in class (a <= 4
                      keeps the next frame's head in the register, a >= 5 restarts it at 0): only then
                      does taking end j's window entry for end k (fold_words' pw[] select) change a result
      edge_a          the (edge, a_i) pairs with an end word first (0) or last (1) in its chunk
      straddle        an end patch (bytes e_i .. e_i + 7) lies across a chunk boundary
    """
    n = len(offsets)
    out = []
    for w0 in range(0, n, ES_WAVE):
        if w0 + ES_WAVE > n:
            out.append({"flat": False, "why": "partial wave"})
            continue
        if w0 + ES_WAVE >= n:
            out.append({"flat": False, "why": "no next offset"})
            continue
        off = offsets[w0:w0 + ES_WAVE + 1]
        if any(off[i + 1] < off[i] + 16 for i in range(ES_WAVE)):
            out.append({"flat": False, "why": "not 16 apart"})
            continue
        if off[ES_WAVE] > limit:
            out.append({"flat": False, "why": "past the limit"})
            continue
        if off[ES_WAVE] - off[0] > ES_MAX_REGION:
            out.append({"flat": False, "why": "region over the bound"})
            continue
        rs = (base_addr + off[0]) & ~15
        s = [base_addr + o - rs for o in off[:ES_WAVE]]
        e = [s[i] + (off[i + 1] - off[i]) - 4 for i in range(ES_WAVE)]
        P = [(x - 1) & ~7 for x in e]
        a = [e[i] - P[i] for i in range(ES_WAVE)]
        re = (e[-1] + 4 + 15) & ~15
        C = (((re + 63) >> 6) + 15) & ~15
        digits, ends_in, edge_a = set(), {}, set()
        max_m = span = 0
        straddle = False
        for i in range(ES_WAVE):
            B = P[i - 1] if i else 0
            span = max(span, P[i] // C - B // C)
            for k in range(B // C, P[i] // C):
                m = (P[i] + 8 - (k + 1) * C) >> 3
                max_m = max(max_m, m)
                digits |= {d for d in range(4) if (m >> (4 * d)) & 15}
                assert m < 1 << 16
            ends_in.setdefault((P[i] // C, (P[i] % C) >> 6), []).append(a[i] >= 5)
            if P[i] % C == 0:
                edge_a.add((0, a[i]))
            if P[i] % C == C - 8:
                edge_a.add((1, a[i]))
            if e[i] // C != (e[i] + 7) // C and (e[i] + 7) // C < ES_WAVE:
                straddle = True
        assert P[-1] // C < ES_WAVE and 64 * C >= re
        sel = {(j, k) for a5 in ends_in.values() for k in range(len(a5)) for j in range(k) if a5[j] != a5[k]}
        out.append({"flat": True, "s0": s[0], "C": C, "nb": (C + 63) >> 6, "wl": (C & 63) >> 3 if C & 63 else 8,
                    "digits": digits, "max_m": max_m, "span": span, "ends": {len(a5) for a5 in ends_in.values()},
                    "sel": sel, "edge_a": edge_a, "straddle": straddle})
    return out


def _short(rng, n, lo=16, hi=64):
    return [rng.randint(lo, hi) for _ in range(n)]


def _named():
    rng = random.Random(0xE5CA5E)
    cases = []

    def add(name, lens, lead):
        cases.append((name, lens, lead))

    lens = _short(rng, 65)
    lens[17] = 200000
    add("one_long", lens, 5)
    lens = _short(rng, 65)
    lens[0], lens[40] = 120000, 130000
    add("two_long", lens, 13)
    lens = _short(rng, 65)
    lens[63] = 250000
    add("long_last", lens, 0)
    add("bound_exact_lead0", [4096] * 65, 0)
    add("bound_exact_lead5", [4096] * 65, 5)
    add("bound_over", [4096] * 63 + [4112, 16], 0)
    add("min_chunk_lead0", [16] * 65, 0)
    add("min_chunk_lead16", [16] * 65, 16)
    add("min_chunk_lead48", [16] * 65, 48)
    add("min_chunk_17", [16] * 64 + [17], 0)
    add("min_chunk_lead8", [16] * 65, 8)
    add("mixed", [rng.choice([16, 17, 23, 24, 25, 100, 4000, 20000]) for _ in range(257)], 3)
    add("mid", _short(rng, 257, 16, 6000), 7)
    # 16..19-byte frames between a few long ones (which widen the chunk past one block): 3 and 4 ends
    # per block with every mix of a <= 4 and a >= 5
    add("tiny_runs", [3000 if i % 16 == 9 else rng.randint(16, 19) for i in range(257)], 0)
    return cases


NAMED = _named()  # (name, lens, lead); the stream's bytes are packed(lens, seed, lead, corrupt)
NAMED_IDS = [c[0] for c in NAMED]


def named_stream(name, corrupt=False, seed=None):
    """blob, offsets, expected results of a named case (seed: the bytes' seed, by default the case's own)"""
    i = NAMED_IDS.index(name)
    _, lens, lead = NAMED[i]
    return packed(lens, 0xCA5E00 + i if seed is None else seed, lead, corrupt)


FUZZ_SEED = 0xF1A7F022
FUZZ_STREAMS = 40


def _fuzz_wave(rng):
    """64 frame lengths whose sum stays under the flat kernel's bound: runs of 16..24, 16..64 and
    16..6000-byte frames and zero to two giants that take up part of what the bound leaves"""
    giants = rng.choice([0, 0, 1, 1, 2])
    lens = []
    while len(lens) < ES_WAVE - giants:
        lo, hi = rng.choice([(16, 24), (16, 24), (16, 64), (16, 6000)])
        lens += _short(rng, rng.randint(1, 24), lo, hi)
    del lens[ES_WAVE - giants:]
    budget = ES_MAX_REGION - rng.choice([0, 0, 16, 1000, 50000])
    while sum(lens) > (budget * 5 // 8 if giants else budget):
        lens[lens.index(max(lens))] = rng.randint(16, 24)
    if giants:
        room = budget - sum(lens)
        room = room if rng.random() < 0.3 else int(room * rng.uniform(0.2, 1.0))
        cut = rng.randint(room // 4, room - room // 4) if giants == 2 else room
        for g in ([cut, room - cut] if giants == 2 else [room]):
            lens.insert(rng.randint(0, len(lens)), max(16, g))
    assert len(lens) == ES_WAVE and sum(lens) <= ES_MAX_REGION
    return lens


def fuzz_streams(seed=FUZZ_SEED, count=FUZZ_STREAMS):
    """`count` streams of 65..321 frames as (lens, lead, corrupt, bytes seed): whole waves from
    _fuzz_wave, then 1..65 short frames (the last wave has no next offset: the lane path); every lead
    0..15 in turn, corruption on roughly half of the streams"""
    rng = random.Random(seed)
    streams = []
    for i in range(count):
        lens = []
        for _ in range(rng.randint(1, 4)):
            lens += _fuzz_wave(rng)
        lens += _short(rng, rng.randint(1, 65), 16, rng.choice([24, 64, 300]))
        streams.append((lens, i % 16, rng.random() < 0.5, rng.getrandbits(32)))
    return streams
