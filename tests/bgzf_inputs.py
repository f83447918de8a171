"""Input builder for the BGZF encoder's edge tests (a plain helper module, like edge_inputs.py).

Every builder returns a Case: the bytes (whole 65280-byte blocks unless said otherwise) and the
counters of oracle.bgzf_block_stats (oracle/bgzf_ref.h bgzf_ref_stats) that the block must reach,
as {counter: (op, value)} with op one of "==", ">=", "<=".  tests/test_bgzf_inputs.py checks the
promises on the CPU, so an input holds its edge whatever the kernel does; tests/test_gpu_bgzf_edges.py
then compares the kernel's bytes with the restatement's on the same inputs.  Seeded numpy only.

Facts of the encoder the cases rest on: a match is found through the fixed probes at distances
1, 2 and 4 (3 bytes suffice) or through the hash chain (the 4 bytes at the position must recur, or
collide in the 2048-slot table); a match never leaves its 255-byte segment, so the longest is 255
(length code 27, symbol 284, hlit 285: hlit 286 would need length 258 and cannot occur); the
chain holds 8 positions, which in random bytes (one position per slot every ~2048 bytes) reach
about 16 KB back, so the far-distance cases keep the table slots of the planted bytes free of
other positions (_quiet).

Huffman length-limit retries.  The literal/length retry (limit 15) is reached by litlen_retry and
by the sweep's skewed blocks.  The distance retry (limit 15, 30 symbols) is reached by dist_retry:
18 distance codes with match counts growing by 1.65 per code, found by the bounded search
search_dist_retry (seeds 0..).  The code-length retry (limit 7) is reached by codelen_retry: byte values
in classes of frequency ~ 2^-L with ~1.618^L values per class, so the counts of the code lengths
are Fibonacci-like (search_codelen_retry, seeds 0..); the sweep reaches it too.  All three retry
paths are therefore run by block inputs.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

import numpy as np

BLOCK, SEG, ROUND = 65280, 255, 256
SIZES = (1, 2, 3, 4, 5, 254, 255, 256, 257, 511, 65279, 65281)
EDGE_LENGTHS = (3, 4, 31, 32, 33, 63, 64, 65, 254, 255, 300)
EDGE_DISTANCES = (1, 2, 3, 4, 5, 255, 256, 257, 32767, 32768, 32769)
ROUND_OFFSETS = (0, 1, 63, 64, 65, 127, 128, 191, 192, 255)


@dataclass
class Case:
    name: str
    data: bytes
    want: Dict[str, Tuple[str, int]] = field(default_factory=dict)


def check_want(case: Case, stats: Dict[str, int]):
    for k, (op, v) in case.want.items():
        got = stats[k]
        ok = got == v if op == "==" else got >= v if op == ">=" else got <= v
        assert ok, "%s: %s = %d, wanted %s %d (%s)" % (case.name, k, got, op, v, stats)


def hash4(v):
    """the encoder's hash of a 4-byte little-endian value (or an array of them)."""
    return ((np.asarray(v, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(21)


def _grams(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.uint32)
    return a[:-3] | a[1:-2] << 8 | a[2:-1] << 16 | a[3:] << 24


def _quiet(rng, n: int, fixed: Sequence[Tuple[int, bytes]]) -> bytes:
    """n random bytes with the pieces `fixed` (position, bytes) in place, redrawn until no position
    outside the pieces hashes into a table slot of a piece's 4 bytes: a planted position's
    candidate is then the planted position before it, however far."""
    a = rng.integers(0, 256, n, dtype=np.uint8)
    frozen = np.zeros(n, bool)
    reserved = np.zeros(2048, bool)
    for pos, b in fixed:
        assert 0 <= pos and pos + len(b) <= n, (pos, len(b))
        a[pos:pos + len(b)] = np.frombuffer(b, np.uint8)
        frozen[pos:pos + len(b)] = True
        if len(b) >= 4:
            reserved[hash4(_grams(np.frombuffer(b, np.uint8))).astype(np.int64)] = True
    inside = frozen[:-3] & frozen[1:-2] & frozen[2:-1] & frozen[3:]
    for _ in range(200):
        bad = np.nonzero(reserved[hash4(_grams(a)).astype(np.int64)] & ~inside)[0]
        if not bad.size:
            return a.tobytes()
        for p in bad:
            j = max(k for k in range(4) if not frozen[p + k])
            a[p + j] = rng.integers(0, 256)
    raise AssertionError("no quiet filler")


def _distinct(rng, n: int) -> bytes:
    """n random bytes, neighbours and next-but-one neighbours different (no run, no period 2)."""
    out = []
    while len(out) < n:
        b = int(rng.integers(0, 256))
        if b not in out[-3:]:
            out.append(b)
    return bytes(out)


# ---- Huffman retries ----------------------------------------------------------------------------
def litlen_multiset(k: int, total: int = BLOCK) -> np.ndarray:
    """byte 0 once, bytes 1..k-1 with counts 2, 3, 5, 8, ... (with the end-of-block symbol the
    Fibonacci series 1, 1, 2, 3, 5, ...), the rest of `total` bytes spread evenly over the 232 bytes
    24..255."""
    fib = [2, 3]
    while len(fib) < k - 1:
        fib.append(fib[-1] + fib[-2])
    parts = [np.zeros(1, np.uint8)] + [np.full(c, 1 + i, np.uint8) for i, c in enumerate(fib[:k - 1])]
    rest = total - sum(len(p) for p in parts)
    parts.append((24 + np.arange(rest) % 232).astype(np.uint8))
    return np.concatenate(parts)


def litlen_retry(k: int = 10, seed: int = 1) -> Case:
    a = litlen_multiset(k)
    np.random.default_rng([71, k, seed]).shuffle(a)
    return Case("litlen_retry_k%d" % k, a.tobytes(), {"retries_litlen": (">=", 1), "matches": ("<=", 4)})


def dist_retry_block(seed: int, n_codes: int = 18, ratio: float = 1.65) -> bytes:
    """Copies of 4 bytes (then one fresh byte) whose distances fall into n_codes distance codes
    (codes 4 .., distances 5 ..), code 4 + j used ~ratio^(n_codes - 1 - j) times: frequencies that
    grow faster than the golden ratio make the Huffman tree one code deeper per symbol, 17 and
    more over the limit of 15.  No copy within 5 bytes of a segment end."""
    rng = np.random.default_rng([72, seed])
    counts = [max(1, int(round(ratio ** (n_codes - 1 - j)))) for j in range(n_codes)]
    codes = np.concatenate([np.full(c, 4 + j) for j, c in enumerate(counts)])
    rng.shuffle(codes)
    base = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
            4097, 6145, 8193, 12289, 16385, 24577, 32769]
    out = bytearray(_distinct(rng, 4200))
    for c in codes:
        while len(out) % SEG > SEG - 6:
            out.append(int(rng.integers(0, 256)))
        if len(out) + 5 > BLOCK:
            break
        d = int(rng.integers(base[c], base[c + 1]))
        src = len(out) - d
        out += out[src:src + 4] if d >= 4 else (out[src:src + d] * 4)[:4]
        b = int(rng.integers(0, 256))
        while b == out[src + 4]:
            b = int(rng.integers(0, 256))
        out.append(b)
    out += bytes(rng.integers(0, 256, max(0, BLOCK - len(out)), dtype=np.uint8))
    return bytes(out[:BLOCK])


def codelen_retry_block(seed: int) -> bytes:
    """A candidate for the code-length (limit 7) retry: n_L ~ 1.618^L byte values of frequency
    ~ 2^-L, L from 2 or 3 up, drawn independently; odd seeds put a run region behind."""
    rng = np.random.default_rng([73, seed])
    l0 = 2 + seed % 2
    vals = rng.permutation(256)
    w, sym, used = [], [], 0
    for L in range(l0, 13):
        n = max(1, int(round(0.3 * 1.618 ** L * (0.8 + 0.4 * rng.random()))))
        n = min(n, 256 - used)
        sym += list(vals[used:used + n])
        w += [2.0 ** -L] * n
        used += n
        if used >= 256:
            break
    w = np.asarray(w) / np.sum(w)
    n_lit = BLOCK if seed % 4 < 2 else int(rng.integers(2000, 30000))
    a = rng.choice(np.asarray(sym, np.uint8), size=n_lit, p=w)
    return (a.tobytes() + bytes([int(vals[-1])]) * (BLOCK - n_lit))[:BLOCK]


def search_dist_retry(stats_of, seeds=range(200)):
    """the bounded search behind dist_retry: the first seed whose block has a distance retry."""
    for s in seeds:
        if stats_of(dist_retry_block(s))["retries_dist"] >= 1:
            return s
    return None


def search_codelen_retry(stats_of, seeds=range(300)):
    for s in seeds:
        if stats_of(codelen_retry_block(s))["retries_codelen"] >= 1:
            return s
    return None


DIST_RETRY_SEED = 0     # search_dist_retry's result
CODELEN_RETRY_SEED = 0  # search_codelen_retry's result


def dist_retry() -> Case:
    return Case("dist_retry", dist_retry_block(DIST_RETRY_SEED), {"retries_dist": (">=", 1)})


def codelen_retry() -> Case:
    return Case("codelen_retry", codelen_retry_block(CODELEN_RETRY_SEED), {"retries_codelen": (">=", 1)})


# ---- distances ----------------------------------------------------------------------------------
def far_copy(dist: int, seed: int = 0) -> Case:
    """random bytes, 40 of them (from position 100) again `dist` later.  32767 and 32768: taken,
    distance code 29; 32769: beyond kMaxDist, the chain is cut and the block has no match."""
    rng = np.random.default_rng([74, dist, seed])
    p = _distinct(rng, 40)
    data = _quiet(rng, BLOCK, [(100, p), (100 + dist, p)])
    if dist <= 32768:
        want = {"max_dist": ("==", dist), "min_dist": ("==", dist), "matches": (">=", 1), "hdist": ("==", 30),
                "dist_used": ("==", 1), "dist_single": ("==", 1)}
    else:
        want = {"matches": ("==", 0), "chain_cut_maxdist": (">=", 1), "dist_used": ("==", 0), "hlit": ("==", 257),
                "hdist": ("==", 1)}
    return Case("far_copy_%d" % dist, data, want)


def near_copy(dist: int, seed: int = 0) -> Case:
    """random bytes with a stretch of period `dist`, 40 bytes, inside one segment: 1, 2 and 4 are
    the fixed probes, 3 and 5 come from the chain alone."""
    rng = np.random.default_rng([75, dist, seed])
    unit = _distinct(rng, 5)[:dist]
    p = (unit * 40)[:40]
    data = _quiet(rng, BLOCK, [(20 * SEG + 30, p)])
    return Case("near_copy_%d" % dist, data, {"max_dist": ("==", dist), "min_dist": ("==", dist), "matches": ("==", 1),
                                              "max_len": ("==", 40 - dist)})


# ---- lengths ------------------------------------------------------------------------------------
def match_length(length: int, seed: int = 0) -> Case:
    """One string of `length` bytes early in the block and copies of it: inside a segment (at its
    start when it would not fit otherwise), 1, 2 and 3 bytes before a segment end (the match is
    clipped there, or too short and literals), 2 bytes before a round end, and 3 bytes before a
    segment end that lies inside a round.  A copy's neighbours differ
    from the string's, so a match is `length` long at most.  Length 3 is only found by a probe:
    its copies lie 4 bytes after a string of their own."""
    rng = np.random.default_rng([76, length, seed])
    w = _distinct(rng, length)
    starts = [100 * SEG + (0 if length > SEG - 10 else 10), 110 * SEG - 1, 120 * SEG - 2, 130 * SEG - 3,
              140 * ROUND - 2, 150 * SEG + 252]
    fixed = []
    if length == 3:
        for k, s in enumerate(starts):
            fixed.append((s - 4, w + bytes([(w[0] + 1 + k) & 255]) + w + bytes([(w[0] + 7 + k) & 255])))
    else:
        fixed.append((5 * SEG + 3, b"\x01" + w + b"\x01"))
        for k, s in enumerate(starts):
            fixed.append((s - 1, bytes([2 + k]) + w + bytes([2 + k])))
    data = _quiet(rng, BLOCK, fixed)
    top = min(length, SEG)
    want = {"max_len": ("==", top), "matches": (">=", 3), "clipped": (">=", 1),
            "lazy_skipped": (">=", 1) if top >= 32 else ("==", 0), "nice_stops": (">=", 1) if top >= 64 else ("==", 0)}
    if top == SEG:
        want["hlit"] = ("==", 285)
    return Case("match_length_%d" % length, data, want)


def lazy_deferral(seed: int = 0) -> Case:
    """y W z where "y W[:30]" stands elsewhere (a match of 31 at y) and W[:32] elsewhere (a match
    of 32 one byte on): 31 is below kLazy, the next position is looked at, and y becomes a literal."""
    rng = np.random.default_rng([77, seed])
    w = _distinct(rng, 40)
    y = bytes([(w[0] + 100) & 255])
    fixed = [(3 * SEG + 10, b"\x05" + w[:32] + b"\x05"), (6 * SEG + 10, b"\x06" + y + w[:30] + b"\x06"),
             (9 * SEG + 10, b"\x07" + y + w[:32] + b"\x08")]
    return Case("lazy_deferral", _quiet(rng, BLOCK, fixed), {"lazy_deferrals": (">=", 1), "max_len": ("==", 32),
                                                              "lazy_skipped": (">=", 1)})


def nice_stop(near: int, seed: int = 0) -> Case:
    """A string of 100 bytes, then its first `near` bytes, then the whole again: at the last, the
    chain reaches the short copy first.  near = 64 ends the search there (a match of 64, then the
    rest); near = 63 goes on to the whole string (one match of 100)."""
    rng = np.random.default_rng([78, near, seed])
    w = _distinct(rng, 100)
    fixed = [(3 * SEG + 10, b"\x05" + w + b"\x05"), (6 * SEG + 10, b"\x06" + w[:near] + b"\x06"),
             (9 * SEG + 10, b"\x07" + w + b"\x08")]
    want = ({"max_len": ("==", 64), "nice_stops": (">=", 2)} if near >= 64 else
            {"max_len": ("==", 100), "nice_stops": (">=", 1)})
    return Case("nice_stop_%d" % near, _quiet(rng, BLOCK, fixed), want)


# ---- candidates ---------------------------------------------------------------------------------
def round_offsets(two_rounds: bool, seed: int = 0) -> Case:
    """Runs of one byte value that put the same 4 bytes at the round offsets ROUND_OFFSETS and
    nowhere else, in round 20 (and in round 21): lane 0 of a wave takes its candidate from the last
    lane of the wave before, lane 63 from its own wave, offset 0 from the table.  The runs differ in
    length, so which earlier run a search reaches first decides the match."""
    rng = np.random.default_rng([79, int(two_rounds), seed])
    g = 0xA7
    fixed = []
    for r in (20, 21) if two_rounds else (20,):
        for o, n in ((0, 5), (63, 6), (127, 5), (191, 5), (255, 4)):
            fixed.append((r * ROUND + o - 1, bytes([3]) + bytes([g]) * n + bytes([4])))
    a = np.frombuffer(_quiet(rng, BLOCK, fixed), np.uint8).copy()
    frozen = np.zeros(BLOCK, bool)
    for pos, b in fixed:
        frozen[pos:pos + len(b)] = True
    a[(a == g) & ~frozen] = g ^ 1
    n = len(ROUND_OFFSETS) * (2 if two_rounds else 1)
    return Case("round_offsets_%d" % (2 if two_rounds else 1), a.tobytes(),
                {"cand_round": (">=", n - (2 if two_rounds else 1)), "cand_table": (">=", 1)})


def chain_cut(seed: int = 0) -> Case:
    """The same 8 bytes 12 times, 300 apart: the last ones' chains are cut after kChain = 8."""
    rng = np.random.default_rng([80, seed])
    w = _distinct(rng, 8)
    fixed = [(7 * SEG + 20 + 300 * k, bytes([k]) + w + bytes([k])) for k in range(12)]
    return Case("chain_cut", _quiet(rng, BLOCK, fixed), {"chain_cut_kchain": (">=", 1), "matches": (">=", 11)})


def colliding_pair(rng):
    """two different 4-byte values with the same hash, by enumeration from a random start."""
    v = int(rng.integers(1 << 24, 1 << 32))
    h = int(hash4(v))
    u = v
    while True:
        u = (u + 1) & 0xFFFFFFFF
        if int(hash4(u)) == h:
            return v, u


def hash_collision(seed: int = 0) -> Case:
    """Pairs of different 4-byte values with equal hashes, the second 300 bytes after the first,
    the table slot otherwise untouched: the second's candidate is the first."""
    rng = np.random.default_rng([81, seed])
    fixed = []
    for k in range(4):
        v, u = colliding_pair(rng)
        fixed.append((10 * SEG + 700 * k, int(v).to_bytes(4, "little")))
        fixed.append((10 * SEG + 700 * k + 300, int(u).to_bytes(4, "little")))
    a = _quiet(rng, BLOCK, fixed)
    return Case("hash_collision", a, {"collisions": (">=", 4)})


# ---- degenerate alphabets ----------------------------------------------------------------------
def one_value() -> Case:
    return Case("one_value", b"\x07" * BLOCK, {"literals": ("==", 1), "min_dist": ("==", 1), "max_dist": ("==", 1),
                                              "dist_single": ("==", 1), "hlit": ("==", 285), "max_len": ("==", 255),
                                              "clipped": (">=", 255), "hdist": ("==", 1)})


def two_values() -> Case:
    return Case("two_values", b"\x07\x70" * (BLOCK // 2), {"literals": ("==", 2), "min_dist": ("==", 2),
                                                          "max_dist": ("==", 2), "dist_single": ("==", 1)})


def no_match(seed: int = 0) -> Case:
    rng = np.random.default_rng([82, seed])
    return Case("no_match", _quiet(rng, BLOCK, []), {"matches": ("==", 0), "dist_used": ("==", 0), "hlit": ("==", 257),
                                                      "hdist": ("==", 1), "literals": ("==", BLOCK)})


def edge_cases() -> List[Case]:
    """every full-block edge case."""
    out = [litlen_retry(10), litlen_retry(12), litlen_retry(14), dist_retry(), codelen_retry()]
    out += [far_copy(d) for d in (32767, 32768, 32769)]
    out += [near_copy(d, seed=1 if d == 2 else 0) for d in (1, 2, 3, 4, 5)]
    out += [match_length(n) for n in EDGE_LENGTHS]
    out += [lazy_deferral(), nice_stop(63), nice_stop(64), round_offsets(False), round_offsets(True), chain_cut(),
            hash_collision(), one_value(), two_values(), no_match()]
    return out


# ---- sizes --------------------------------------------------------------------------------------
def sized(n: int) -> bytes:
    """n bytes of a 4-value alphabet with repeats: partial blocks still find matches."""
    rng = np.random.default_rng([83, n])
    return rng.integers(0, 4, n, dtype=np.uint8).tobytes()


# ---- random sweep -------------------------------------------------------------------------------
SWEEP_BLOCKS = 48


def sweep_block(k: int, seed: int = 0) -> bytes:
    """Block k of the sweep: LZ-style, literal runs interleaved with copies.  The alphabet size is
    drawn from {2, 4, 16, 64, 256}; copy distances and lengths are drawn half from the edge values,
    half uniformly.  Now and then a literal run comes from all 256 byte values ("foreign", in a
    small alphabet the only bytes whose table slots stay quiet) and is scheduled to come again
    32767, 32768 or 32769 bytes later.  k % 8 selects the block's kind: 0 no copies at all
    (alphabet 256), 1 copies at one distance only, 2 all the literals of litlen_multiset (the skewed
    histogram of the literal/length retry) with 24 copies between them, the rest as drawn."""
    rng = np.random.default_rng([84, seed, k])
    kind = k % 8
    asz = 256 if kind in (0, 2) else int(rng.choice([2, 4, 16, 64, 256]))
    alpha = rng.permutation(256)[:asz].astype(np.uint8)
    pool, preset = None, []
    if kind == 2:  # a few copies of preset lengths; the literals are the whole multiset
        preset = [int(rng.choice(EDGE_LENGTHS)) for _ in range(24)]
        pool = litlen_multiset(10 + 2 * (k // 8 % 3), BLOCK - sum(preset))
        rng.shuffle(pool)
    one_dist = int(rng.choice(EDGE_DISTANCES[:8])) if kind == 1 else 0
    out = bytearray()
    echoes = []  # (position, source, length), by position
    used = 0

    def literals(n, foreign):
        nonlocal used
        if pool is not None:
            b = pool[used:used + n].tobytes()
            used += n
            return b
        return (rng.integers(0, 256, n, dtype=np.uint8) if foreign else alpha[rng.integers(0, asz, n)]).tobytes()

    while len(out) < BLOCK:
        pos = len(out)
        room = (echoes[0][0] if echoes else BLOCK) - pos
        if echoes and room == 0:
            _, src, n = echoes.pop(0)
            out += out[src:src + n]
            continue
        foreign = kind >= 3 and rng.random() < 0.08
        n = min(room, int(rng.integers(1, 24 if asz > 16 else 6)) + (12 if foreign else 0))
        if pool is not None:
            n = min(int(rng.integers(1000, 4000)), len(pool) - used)
        out += literals(n, foreign)
        if foreign and n >= 8 and len(echoes) < 4:
            d = int(rng.choice(EDGE_DISTANCES[8:]))
            if pos + d + n <= BLOCK and all(abs(pos + d - e[0]) > 400 for e in echoes):
                echoes.append((pos + d, pos, n))
                echoes.sort()
        if kind == 0 or (pool is not None and not preset):
            continue
        pos = len(out)
        room = (echoes[0][0] if echoes else BLOCK) - pos
        if room <= 0:
            continue
        d = one_dist or (int(rng.choice(EDGE_DISTANCES)) if rng.random() < 0.5 else int(rng.integers(1, 40000)))
        if d > pos:
            d = int(rng.integers(1, pos + 1))
        n = int(rng.choice(EDGE_LENGTHS)) if rng.random() < 0.5 else int(rng.integers(3, 100))
        n = preset.pop() if preset else min(n, room)
        for _ in range(n):
            out.append(out[len(out) - d])
    return bytes(out[:BLOCK])


def sweep() -> List[bytes]:
    return [sweep_block(k) for k in range(SWEEP_BLOCKS)]


# ---- many blocks --------------------------------------------------------------------------------
MANY_BLOCKS = 260


def many_contents() -> List[bytes]:
    """the 4 distinct contents the 260-block input cycles through (sizes that differ)."""
    return [sweep_block(3), sweep_block(5), one_value().data, no_match().data]
