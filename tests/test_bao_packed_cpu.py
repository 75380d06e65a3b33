"""The packed layout of the sparse bao calls without a GPU (b3w_bao_packed_layout, bao.packed_layout, bao.pack_ranges): where the chunks
that an update, a ranged verification or a range-slice call over files that are not resident reads lie in the packed buffer.  The
oracle is a restatement written here that shares nothing with the library's interval arithmetic: it builds the SET of listed chunks of
every file chunk by chunk, sorts (file, chunk) and gives each its rank.  Files: the 51 lengths of tests/test_bao_range_cpu.py, each
alone and all in one call (the small ones between the large), at g in {0, 1, 4, 6}.  Then the three device twins' names, and the
refusals that need no context."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import b3w_testlib as T
from test_bao_range_cpu import ALL_LENGTHS

GS = (0, 1, 4, 6)
BAD = 100
FILL = 0xEEEEEEEEEEEEEEEE
NAMES = {"b3w_bao_packed_layout": 12, "b3w_bao_outboard_update_packed_device": 16, "b3w_bao_verify_ranges_packed_device": 20,
         "b3w_bao_range_slice_packed_device": 13}
# the lengths with a file of at most 64 chunks between every two larger ones, and the two largest not at an end
WORLD = sorted(ALL_LENGTHS)[-5:-3] + [x for pair in zip(sorted(ALL_LENGTHS)[:3], sorted(ALL_LENGTHS)[-3:]) for x in pair] + sorted(ALL_LENGTHS)[3:-5]


def _n(length):
    return max(1, (length + 1023) // 1024)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _listed_of(length, g, a, c):
    """the chunks range (a, c) of a file of this length lists"""
    n = _n(length)
    if c == 0:
        return []
    if n <= 64:
        return list(range(n))
    return [ch for ch in range(n) if (a >> g) <= (ch >> g) <= ((a + c - 1) >> g)]


def _restated(lens, g, ranges):
    """-> (range_slot, range_first, range_chunks, total_slots, total_bytes) from the sets of listed chunks, sorted and ranked"""
    listed = set()
    for f, a, c in ranges:
        listed.update((f, ch) for ch in _listed_of(lens[f], g, a, c))
    order = sorted(listed)
    rank = {fc: i for i, fc in enumerate(order)}
    slot, first, count = [], [], []
    for f, a, c in ranges:
        mine = _listed_of(lens[f], g, a, c)
        assert mine == list(range(mine[0], mine[0] + len(mine))) if mine else True
        if mine:                                                             # a range's chunks are consecutive slots
            assert [rank[(f, ch)] for ch in mine] == list(range(rank[(f, mine[0])], rank[(f, mine[0])] + len(mine))), (f, a, c)
        slot.append(rank[(f, mine[0])] if mine else 0)
        first.append(mine[0] if mine else 0)
        count.append(len(mine))
    total_bytes = 0
    if order:
        f, ch = order[-1]
        total_bytes = 1024 * (len(order) - 1) + min(1024, lens[f] - 1024 * ch)
    return slot, first, count, len(order), total_bytes


def _layout(L, lens, g, ranges, n_files=None, outs=(True, True, True)):
    """b3w_bao_packed_layout over prefilled outputs -> (rc, slot, first, count, total_slots, total_bytes)"""
    ln = np.array(lens, dtype=np.uint64)
    fi = np.array([f for f, _, _ in ranges], dtype=np.uint32)
    fc = np.array([a for _, a, _ in ranges], dtype=np.uint64)
    nc = np.array([c for _, _, c in ranges], dtype=np.uint64)
    arr = [np.full(len(ranges), FILL, dtype=np.uint64) for _ in range(3)]
    tot = np.full(2, FILL, dtype=np.uint64)
    rc = L.b3w_bao_packed_layout(ln.ctypes.data, len(lens) if n_files is None else n_files, g, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, len(ranges),
                                 *[a.ctypes.data if on else None for a, on in zip(arr, outs)], tot.ctypes.data, tot.ctypes.data + 8)
    return (rc, *[a.tolist() for a in arr], int(tot[0]), int(tot[1]))


def _kinds(length, g):
    """name -> the ranges (first chunk, chunks) of that kind that exist in a file of this length"""
    n, G = _n(length), 1 << g
    out = {"one chunk": [[(c, 1)] for c in sorted({0, n // 2, n - 1, min(n - 1, 64), min(n - 1, 1023), min(n - 1, 1024)})],
           "the last chunk": [[(n - 1, 1)]], "the whole file": [[(0, n)]], "an empty range": [[(0, 0)], [(n, 0)], [(n // 2, 0)]]}
    b = G * max(1, n // 2 // G)                                               # a unit boundary (any chunk at g = 0) inside the file
    if b + 1 <= n:
        out["across a unit boundary, unaligned at both ends"] = [[(b - 1, 2)]] + ([[(b - 1, G + 2)]] if b + G + 1 <= n else [])
    if n > 1024:
        out["across a tile boundary"] = [[(1022, min(4, n - 1022))], [(1000 - G, min(n - 1000 + G, 40 + 2 * G))]]
    for t0 in (0, 1024):                                                      # two ranges of one tile with a gap of whole units between them
        if n >= t0 + 5 * G + 4:
            out.setdefault("two ranges of one tile with a gap", []).append([(t0 + 1, 2), (t0 + 3 * G + 1, min(n - t0 - 3 * G - 1, G + 1))])
    if n >= 3:
        out["repeated, overlapping and unsorted"] = [[(n - 2, 2), (0, 2), (1, n - 2), (0, 2), (n - 1, 1), (n // 2, 0), (0, 1)],
                                                     [(n // 2, 1), (n // 2 - 1, 2), (n // 2, 1)]]
    return out


def _check(L, lens, g, ranges, why):
    want = _restated(lens, g, ranges)
    got = _layout(L, lens, g, ranges)
    assert got[0] == 0, why
    assert got[1:] == want, why
    return got


def test_the_51_lengths_are_those_of_the_range_test_and_hold_64_and_65_chunks():
    assert len(ALL_LENGTHS) == 51 and sorted(WORLD) == sorted(ALL_LENGTHS)
    assert {64, 65, 1025, 2049} <= {_n(x) for x in ALL_LENGTHS}
    big = [i for i, x in enumerate(WORLD) if _n(x) > 64]
    assert len(big) == 3 and all(b - a > 1 for a, b in zip(big, big[1:])) and big[0] > 0 and big[-1] < len(WORLD) - 1


@pytest.mark.parametrize("g", GS)
def test_every_kind_of_range_on_every_length_alone(g):
    L = T.pkg().lib()
    seen = set()
    for length in ALL_LENGTHS:
        for name, cases in _kinds(length, g).items():
            seen.add(name)
            for case in cases:
                _check(L, [length], g, [(0, a, c) for a, c in case], (length, g, name, case))
    assert len(seen) == 8, seen


@pytest.mark.parametrize("g", GS)
def test_all_lengths_in_one_call_with_small_files_between_large_ones(g):
    L = T.pkg().lib()
    every = [(f, a, c) for f, length in enumerate(WORLD) for cases in _kinds(length, g).values() for case in cases for a, c in case]
    rng = random.Random(g)
    rng.shuffle(every)
    slot, first, count, slots, nbytes = _check(L, WORLD, g, every, g)[1:]
    assert slots == sum(_n(x) for x in WORLD)                                  # (the whole file is among every file's ranges)
    # one kind at a time across the files: what the large files list now depends on the kind
    for name in ("one chunk", "the last chunk", "two ranges of one tile with a gap", "across a tile boundary", "repeated, overlapping and unsorted"):
        some = [(f, a, c) for f, length in enumerate(WORLD) for case in _kinds(length, g).get(name, [])[:1] for a, c in case]
        rng.shuffle(some)
        _check(L, WORLD, g, some, (g, name))
    # a small file between two large ones, and nothing else listed
    big = [i for i, x in enumerate(WORLD) if _n(x) > 64]
    mid = big[0] + 1
    assert _n(WORLD[mid]) <= 64
    got = _check(L, WORLD, g, [(big[1], 70, 3), (mid, 0, 1), (big[0], 64, 1)], g)
    assert got[1][2] == 0 and got[1][1] == got[3][2] and got[1][0] == got[1][1] + _n(WORLD[mid])   # large | the small one whole | large


@pytest.mark.parametrize("g", GS)
def test_ranges_that_share_a_chunk_name_the_same_slot_for_it(g):
    L = T.pkg().lib()
    K = 1024
    lens = [2049 * K, 40 * K + 3, 1025 * K]
    ranges = [(0, 100, 50), (0, 120, 100), (0, 149, 1), (2, 1020, 5), (2, 1024, 1), (1, 3, 2), (1, 30, 1), (0, 120, 100)]
    _, slot, first, count, _, _ = _check(L, lens, g, ranges, g)
    place = {}
    for (f, a, c), s, lo, k in zip(ranges, slot, first, count):
        assert lo <= a and a + c <= lo + k
        for ch in range(lo, lo + k):
            assert place.setdefault((f, ch), s + ch - lo) == s + ch - lo, (g, f, ch)
    assert slot[1] == slot[7] and slot[5] == slot[6] and first[5] == 0 and count[5] == 41


def test_total_bytes_ends_with_the_chunk_in_the_last_slot():
    L = T.pkg().lib()
    K = 1024
    lens = [100 * K + 5, 100 * K, 3 * K + 1, 0]
    for g in GS:
        G = 1 << g
        assert _layout(L, lens, g, [(0, 100, 1)])[4:] == (min(G, 101 - 100 // G * G), K * (min(G, 101 - 100 // G * G) - 1) + 5)   # a short last chunk
        assert _layout(L, lens, g, [(0, 100, 1), (1, 99, 1)])[5] == K * (min(G, 101 - 100 // G * G) + min(G, 100 - 99 // G * G))   # a whole one
        assert _layout(L, lens, g, [(0, 0, 1)])[4:] == (G, K * G)                                                                  # inside the file
        assert _layout(L, lens, g, [(2, 1, 1)])[4:] == (4, 3 * K + 1)                                                              # a small file, whole
        assert _layout(L, lens, g, [(3, 0, 1)])[4:] == (1, 0)                                                                      # a file of no bytes: a slot of none
        assert _layout(L, lens, g, [(1, 5, 1), (3, 0, 1)])[4:] == (G + 1, K * G)
        assert _layout(L, lens, g, [(0, 7, 0), (3, 1, 0)])[1:] == ([0, 0], [0, 0], [0, 0], 0, 0)                                   # nothing listed
        assert _layout(L, lens, g, [])[4:] == (0, 0)


def test_the_range_outputs_may_be_null():
    L = T.pkg().lib()
    lens, ranges = [70 * 1024, 5], [(0, 3, 9), (1, 0, 1), (0, 66, 4)]
    full = _layout(L, lens, 1, ranges)
    for outs in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = _layout(L, lens, 1, ranges, outs=outs)
        assert got[0] == 0 and got[4:] == full[4:]
        for k, on in enumerate(outs):
            assert got[1 + k] == (full[1 + k] if on else [FILL] * 3)


def test_every_refusal_of_the_layout_writes_nothing():
    m = T.pkg()
    L = m.lib()
    assert m.B3W_E_BAD_ARGUMENT == BAD
    K = 1024
    lens = [70 * K, 5 * K]
    untouched = ([FILL], [FILL], [FILL], FILL, FILL)
    assert _layout(L, lens, 7, [(0, 0, 1)]) == (BAD, *untouched)               # group_log above the maximum
    assert _layout(L, lens, 0, [(2, 0, 1)]) == (BAD, *untouched)               # a file index >= n_files
    assert _layout(L, lens, 0, [(1, 0, 1)], n_files=1) == (BAD, *untouched)
    for a, c in ((70, 1), (69, 2), (0, 71), (71, 0), (1 << 63, 1 << 63)):      # past the file's 70 chunks
        assert _layout(L, lens, 0, [(0, a, c)]) == (BAD, *untouched), (a, c)
    assert _layout(L, [(1 << 40) + 1], 0, [(0, 0, 1)]) == (BAD, *untouched)    # more than 2^30 chunks
    assert _layout(L, [1 << 40], 0, [(0, (1 << 30) - 1, 1)])[4:] == (1, 1024)
    got = _layout(L, lens, 0, [(0, 0, 1), (1, 0, 1), (0, 70, 1)])              # a bad range behind good ones
    assert got == (BAD, [FILL] * 3, [FILL] * 3, [FILL] * 3, FILL, FILL)
    ln, one, u32 = np.array(lens, dtype=np.uint64), np.array([1], dtype=np.uint64), np.array([0], dtype=np.uint32)
    tot = np.full(2, FILL, dtype=np.uint64)
    args = [ln.ctypes.data, 2, 0, u32.ctypes.data, one.ctypes.data, one.ctypes.data, 1, None, None, None, tot.ctypes.data, tot.ctypes.data + 8]
    assert L.b3w_bao_packed_layout(*args) == 0 and tot.tolist() == [1, 1024]
    for k in (0, 3, 4, 5, 10, 11):                                             # a null pointer
        tot[:] = FILL
        assert L.b3w_bao_packed_layout(*[None if i == k else a for i, a in enumerate(args)]) == BAD, k
        assert tot.tolist() == [FILL, FILL]
    assert L.b3w_bao_packed_layout(None, 0, 0, None, None, None, 0, None, None, None, tot.ctypes.data, tot.ctypes.data + 8) == 0 and tot.tolist() == [0, 0]


def test_the_cost_does_not_grow_with_the_file_count():
    """host_lens is read at listed files alone: a table of 2^32 - 1 files of which the array holds the first three"""
    L = T.pkg().lib()
    got = _layout(L, [5, 70 * 1024, 9], 0, [(1, 69, 1), (2, 0, 1)], n_files=(1 << 32) - 1)
    assert got == (0, [0, 1], [69, 0], [1, 1], 2, 1024 + 9)


def test_the_python_calls():
    m = T.pkg()
    K = 1024
    lens = [70 * K + 7, 3 * K, 0]
    files, firsts, counts = [0, 1, 0, 2, 0], [68, 1, 2, 0, 70], [3, 1, 1, 1, 0]
    for g in (0, 4):
        lay = m.bao.packed_layout(lens, files, firsts, counts, g)
        want = _restated(lens, g, list(zip(files, firsts, counts)))
        assert ([lay[k].tolist() for k in ("range_slot", "range_first", "range_chunks")] + [lay["total_slots"], lay["total_bytes"]]) == list(want)
        # the gather, from host bytes and from numpy: every listed chunk in its slot, zero behind a short last chunk
        data = np.random.default_rng(g).integers(0, 256, sum(lens) + 11, dtype=np.uint8)
        offsets = [11, 11 + lens[0], 11 + lens[0] + lens[1]]
        for src in (data, data.tobytes()):
            packed = m.bao.pack_ranges(src, offsets, lens, files, firsts, counts, g, device="cpu").numpy()
            assert packed.shape == (lay["total_slots"], 1024)
            seen = np.zeros(lay["total_slots"], dtype=bool)
            for f, s, lo, k in zip(files, lay["range_slot"], lay["range_first"], lay["range_chunks"]):
                for ch in range(int(lo), int(lo + k)):
                    nb = min(1024, lens[f] - ch * 1024)
                    row = packed[int(s) + ch - int(lo)]
                    assert (row[:nb] == data[offsets[f] + ch * 1024:offsets[f] + ch * 1024 + nb]).all() and not row[nb:].any(), (g, f, ch)
                    seen[int(s) + ch - int(lo)] = True
            assert seen.all()
    assert m.bao.pack_ranges(b"", [0], [0], [0], [0], [0], device="cpu").shape == (0, 1024)
    for g in (-1, 7):
        for call in (lambda: m.bao.packed_layout(lens, [0], [0], [1], g), lambda: m.bao.pack_ranges(b"", [0, 0, 0], lens, [0], [0], [1], g, device="cpu"),
                     lambda: m.bao.outboard_update_packed(None, None, lens, None, None, [0], [0], [1], group_log=g),
                     lambda: m.bao.verify_ranges_packed(None, None, lens, None, None, [0], [0], [1], group_log=g),
                     lambda: m.bao.range_slices_packed(None, None, lens, None, [0], [0], [1], group_log=g)):
            with pytest.raises(m.B3WError, match="group_log"):
                call()
    with pytest.raises(m.B3WError, match="b3w_bao_packed_layout"):
        m.bao.packed_layout(lens, [3], [0], [1])
    with pytest.raises(m.B3WError, match="b3w_bao_packed_layout"):
        m.bao.packed_layout(lens, [1], [3], [1])
    with pytest.raises(m.B3WError, match="2 first chunks and 1 chunk counts"):
        m.bao.packed_layout(lens, [0, 0], [0, 1], [1])
    with pytest.raises(m.B3WError, match="1 files and 2 ranges"):
        m.bao.packed_layout(lens, [0], [0, 1], [1, 1])


def test_the_names_are_declared_exported_and_bound():
    m = T.pkg()
    L = m.lib()
    hdr = open(os.path.join(T.ROOT, "include", "b3wit.h")).read()
    declared = set(re.findall(r"\b(b3w_[a-z0-9_]+)\s*\(", hdr))
    for name, n_args in NAMES.items():
        assert name in declared and name in m.EXPORTED_SYMBOLS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int32 and fn.argtypes is not None and len(fn.argtypes) == n_args, name
    assert L.b3w_abi_version() == (1 << 16) + 4                                # new names only: the number stays
    for name in ("packed_layout", "pack_ranges", "outboard_update_packed", "verify_ranges_packed", "range_slices_packed"):
        assert callable(getattr(m.bao, name)), name
    # each twin takes its arena counterpart's arguments with (d_packed, packed_bytes) for (d_arena, arena_bytes, host_offsets)
    for packed, arena in (("b3w_bao_outboard_update_packed_device", "b3w_bao_outboard_update_batch_device"),
                          ("b3w_bao_verify_ranges_packed_device", "b3w_bao_verify_ranges_batch_device"),
                          ("b3w_bao_range_slice_packed_device", "b3w_bao_range_slice_arena_device")):
        a = getattr(L, arena).argtypes
        assert list(getattr(L, packed).argtypes) == list(a[:3]) + list(a[4:]), packed


def test_the_device_twins_refuse_a_null_context_and_touch_nothing():
    L = T.pkg().lib()
    one = (ctypes.c_uint64 * 1)(0)
    for name, n_args in list(NAMES.items())[1:]:
        fn = getattr(L, name)
        ints = [i for i, t in enumerate(fn.argtypes) if t is not ctypes.c_void_p]
        assert fn(*[0 if i in ints else None for i in range(n_args)]) == BAD, name
        assert fn(*[(8 if i == 2 else 1) if i in ints else (None if i == 0 else one) for i in range(n_args)]) == BAD, name
    assert one[0] == 0
