"""The arrival bitmap without a GPU (b3w_bao_have_layout, b3w_bao_have_runs, b3w_bao_have_from_status; bao.have_layout, have_runs_host,
have_from_status_host, runs_chunks) against the restatement in tests/bao_have_ref.py: files of every length of test_bao_cpu.LENGTHS and
of exactly 1, 63, 64, 65, 127, 128 and 129 chunks, unit sizes g in {0, 1, 4, 6}, both kinds, every pattern of _patterns().  The host
round trip: a shuffled half of a file's chunks taken in through ingest_slice_host into buffers of 0xEE, verify_host over them, and the
bitmap made from those statuses is the set of chunks taken in (g = 0) or its collapse into whole units (g > 0)."""
import ctypes

import numpy as np
import pytest

import b3w_testlib as T
import bao_have_ref as H
import bao_ref as R
from test_bao_cpu import LENGTHS
from test_bao_ingest_cpu import _fresh
from test_bao_slices_cpu import _made

BAD = 100
GS = [0, 1, 4, 6]
KINDS = ["missing", "present"]
ALL_LENGTHS = LENGTHS + [n * 1024 for n in (63, 64, 65, 127, 128, 129)] + [128 * 1024 + 1]


def _patterns(n, seed):
    """-> [(name, bits of the n chunks, the caller's pad bits set)]"""
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    out = [("all clear", np.zeros(n, bool), False), ("all set", np.ones(n, bool), False),
           ("alternating bits", idx % 2 == 0, False), ("alternating bits, odd", idx % 2 == 1, False)]
    for g in GS[1:]:
        out.append((f"alternating units of {1 << g}", (idx >> g) % 2 == 0, False))
        out.append((f"alternating units of {1 << g}, odd", (idx >> g) % 2 == 1, False))
    for c in sorted({0, 63, 64, n - 1}):
        if c < n:
            out.append((f"only chunk {c}", idx == c, False))
            out.append((f"all but chunk {c}", idx != c, False))
    out.append(("a run across the word boundary", (idx >= 60) & (idx < 70), False))
    out.append(("a hole across the word boundary", ~((idx >= 60) & (idx < 70)), False))
    out.append(("a run that ends on the last chunk", idx >= n - min(n, 10), False))
    out.append(("a hole that ends on the last chunk", idx < n - min(n, 10), False))
    out.append(("pad bits set, all clear", np.zeros(n, bool), True))
    out.append(("pad bits set, random", rng.random(n) < 0.5, True))
    for density in (0.01, 0.5, 0.99):
        out.append((f"random {density}", rng.random(n) < density, False))
    return out


def test_the_restatement_agrees_with_itself():
    """the vectorised runs() against the definition read aloud, and the alternating pattern reaches the ceil(u / 2) bound"""
    for n in (1, 2, 63, 64, 65, 129, 200):
        for name, bits, _ in _patterns(n, n):
            for g in GS:
                for kind in (H.MISSING, H.PRESENT):
                    assert H.runs(bits, g, kind) == H.runs_slow(bits, g, kind), (n, name, g, kind)
        assert len(H.runs(np.arange(n) % 2 == 0, 0, H.PRESENT)[0]) == (n + 1) // 2
        assert (H.unpack(H.pack(np.arange(n) % 3 == 0, pad=True), n) == (np.arange(n) % 3 == 0)).all()


def test_the_layout():
    m = T.pkg()
    assert [int(x) for x in m.bao.have_layout(ALL_LENGTHS)] == H.layout(ALL_LENGTHS)
    assert [int(x) for x in m.bao.have_layout([])] == [0]
    assert [int(x) for x in m.bao.have_layout([0])] == [0, 1]                          # an empty file has one chunk and one bit
    assert [int(x) for x in m.bao.have_layout([64 * 1024, 64 * 1024 + 1, 1])] == [0, 1, 3, 4]
    assert m.lib().b3w_bao_have_layout(None, 0, None) == 0


@pytest.mark.parametrize("length", ALL_LENGTHS)
def test_runs_equal_the_restatement_row_for_row(length):
    m = T.pkg()
    n = H.num_chunks(length)
    for name, bits, pad in _patterns(n, length):
        have = H.pack(bits, pad)
        for g in GS:
            covered = np.zeros((n + (1 << g) - 1) >> g, dtype=np.int32)
            for kind in KINDS:
                want_rows, want_have = H.runs(bits, g, H.KINDS[kind])
                first, count, n_runs, n_have = m.bao.have_runs_host(have, length, kind, g)
                assert n_runs == len(want_rows) and n_have == want_have, (name, g, kind)
                assert list(zip(first.tolist(), count.tolist())) == want_rows, (name, g, kind)
                assert n_runs <= m.bao.have_runs_bound([length], g)
                for a, k in want_rows:
                    assert a % (1 << g) == 0 and a + k <= n and (k % (1 << g) == 0 or a + k == n)
                    covered[a >> g:(a + k + (1 << g) - 1) >> g] += 1
                if n_runs > 1:                                                       # a capacity below the total: the first rows, the total
                    cap = n_runs // 2
                    f2, c2, n2, h2 = m.bao.have_runs_host(have, length, kind, g, capacity=cap)
                    assert (n2, h2) == (n_runs, n_have) and list(zip(f2.tolist(), c2.tolist())) == want_rows[:cap]
                f0, c0, n0, h0 = m.bao.have_runs_host(have, length, kind, g, capacity=0)     # count only
                assert f0.size == 0 and (n0, h0) == (n_runs, n_have)
            assert (covered == 1).all(), (name, g, "PRESENT and MISSING do not partition the units")
    if n > 1:
        assert m.bao.have_runs_host(H.pack(np.arange(n) % 2 == 0), length, "present")[2] == m.bao.have_runs_bound([length]) == (n + 1) // 2


def test_a_capacity_below_the_total_leaves_what_lies_behind_it():
    m = T.pkg()
    L = m.lib()
    n = 129
    have = H.pack(np.arange(n) % 2 == 0)
    first, count = np.full(80, 0xEEEE, dtype=np.uint64), np.full(80, 0xEEEE, dtype=np.uint64)
    n_runs = ctypes.c_uint64()
    assert L.b3w_bao_have_runs(have.ctypes.data, n * 1024, 0, H.MISSING, 10, first.ctypes.data, count.ctypes.data, ctypes.byref(n_runs), None) == 0
    assert n_runs.value == 64 and first[:10].tolist() == list(range(1, 21, 2)) and count[:10].tolist() == [1] * 10
    assert (first[10:] == 0xEEEE).all() and (count[10:] == 0xEEEE).all()


@pytest.mark.parametrize("length", ALL_LENGTHS)
def test_from_status_equals_the_restatement(length):
    m = T.pkg()
    n = H.num_chunks(length)
    for g in GS:
        units = (n + (1 << g) - 1) >> g
        rng = np.random.default_rng(length + g)
        for status in (np.zeros(units, np.uint8), np.full(units, 0xFF, np.uint8), rng.choice(np.array([0, 0, 0, 1, 2, 3, 0xFF], dtype=np.uint8), units)):
            got = m.bao.have_from_status_host(status, length, g)
            assert got.dtype == np.uint64 and (got == H.from_status(status, n, g)).all(), (g, status)
            assert (H.unpack(got, n) == np.repeat(status == 0, 1 << g)[:n]).all()
            if n % 64:
                assert int(got[-1]) >> (n % 64) == 0, "a pad bit is set"


@pytest.mark.parametrize("length", LENGTHS + [65 * 1024 + 1])
def test_the_host_round_trip(length):
    """a shuffled half of the chunks taken in, verified where they lie, and the bitmap made from the statuses"""
    m = T.pkg()
    data, ob, root = _made(length)
    n = R.num_chunks(length)
    for g in GS:
        got_data, got_ob = _fresh(length, g)
        taken = np.random.default_rng(7 * length + g).permutation(n)[:(n + 1) // 2]
        for c in taken.tolist():
            assert m.bao.ingest_slice_host(got_data, got_ob, length, c, root, R.slice_chunk(ob, data, c), g) == 0
        status, _, _ = m.bao.verify_host(bytes(got_data), bytes(got_ob), root, g)
        have = m.bao.have_from_status_host(status, length, g)
        bits = np.zeros(n, bool)
        bits[taken] = True
        assert (H.unpack(have, n) == H.collapse(bits, g)).all(), (length, g)
        if g == 0:
            first, count, n_runs, n_have = m.bao.have_runs_host(have, length, "missing")
            fi, ch = m.bao.runs_chunks(np.zeros(first.size, np.uint32), first, count)
            assert n_have == taken.size and sorted(ch.tolist() + taken.tolist()) == list(range(n)) and not fi.any()


def test_runs_chunks():
    m = T.pkg()
    fi, ch = m.bao.runs_chunks([2, 2, 5], [0, 7, 64], [3, 1, 2])
    assert fi.dtype == np.uint32 and ch.dtype == np.uint64
    assert fi.tolist() == [2, 2, 2, 2, 5, 5] and ch.tolist() == [0, 1, 2, 7, 64, 65]
    fi, ch = m.bao.runs_chunks([], [], [])
    assert fi.size == 0 and ch.size == 0
    fi, ch = m.bao.runs_chunks([1, 3], [4, 9], [0, 2])                                # (a row of no chunks gives no sample)
    assert fi.tolist() == [3, 3] and ch.tolist() == [9, 10]
    with pytest.raises(m.B3WError):
        m.bao.runs_chunks([1], [1, 2], [1, 1])


def test_names_are_exported_and_the_abi_number_stands():
    m = T.pkg()
    L = m.lib()
    assert L.b3w_abi_version() == (1 << 16) | 4                                      # new names only
    hdr = open(__import__("os").path.join(T.ROOT, "include", "b3wit.h")).read()
    for name in ("b3w_bao_have_layout", "b3w_bao_slice_ingest_have_device", "b3w_bao_have_runs_scratch_bytes", "b3w_bao_have_runs_device",
                 "b3w_bao_have_from_status_device", "b3w_bao_have_runs", "b3w_bao_have_from_status"):
        assert name in m.EXPORTED_SYMBOLS and hasattr(L, name) and name + "(" in hdr, name
    for name in ("have_layout", "have_new", "have_runs", "have_from_status", "have_runs_host", "have_from_status_host", "runs_chunks", "have_runs_bound"):
        assert callable(getattr(m.bao, name)), name
    assert "#define B3W_BAO_HAVE_MISSING 0" in hdr and "#define B3W_BAO_HAVE_PRESENT 1" in hdr
    assert m.bao.HAVE_KINDS == {"missing": 0, "present": 1}
    import inspect
    assert inspect.signature(m.bao.ingest_slices).parameters["d_have"].default is None
    lens = np.array([1 << 20, 0, 1025], dtype=np.uint64)
    assert L.b3w_bao_have_runs_scratch_bytes(lens.ctypes.data, 3) >= 16 and L.b3w_bao_have_runs_scratch_bytes(None, 3) == 0


def test_refusals():
    m = T.pkg()
    L = m.lib()
    n = 70
    have = H.pack(np.arange(n) % 2 == 0)
    first, count = np.full(40, 0xEEEE, dtype=np.uint64), np.full(40, 0xEEEE, dtype=np.uint64)
    n_runs, n_have = ctypes.c_uint64(77), ctypes.c_uint64(77)

    def call(have_p=have.ctypes.data, g=0, kind=0, cap=40, first_p=first.ctypes.data, count_p=count.ctypes.data, n_runs_p=ctypes.byref(n_runs)):
        return L.b3w_bao_have_runs(have_p, n * 1024, g, kind, cap, first_p, count_p, n_runs_p, ctypes.byref(n_have))
    for change in (dict(have_p=None), dict(g=7), dict(kind=2), dict(first_p=None), dict(count_p=None), dict(n_runs_p=None)):
        assert call(**change) == BAD, change
        assert n_runs.value == 77 and n_have.value == 77 and (first == 0xEEEE).all() and (count == 0xEEEE).all(), change
    assert call(cap=0, first_p=None, count_p=None) == 0 and n_runs.value == 35 and n_have.value == 35
    assert call() == 0 and first[:35].tolist() == list(range(1, 70, 2))
    status = np.zeros(n, dtype=np.uint8)
    out = np.full(2, 0xEEEE, dtype=np.uint64)
    assert L.b3w_bao_have_from_status(None, n * 1024, 0, out.ctypes.data) == BAD
    assert L.b3w_bao_have_from_status(status.ctypes.data, n * 1024, 0, None) == BAD
    assert L.b3w_bao_have_from_status(status.ctypes.data, n * 1024, 7, out.ctypes.data) == BAD
    assert (out == 0xEEEE).all()
    assert L.b3w_bao_have_from_status(status.ctypes.data, n * 1024, 0, out.ctypes.data) == 0 and out.tolist() == [(1 << 64) - 1, (1 << 6) - 1]
    for bad in (lambda: m.bao.have_runs_host(have, n * 1024, "absent"), lambda: m.bao.have_runs_host(have, n * 1024, "missing", 7),
                lambda: m.bao.have_runs_host(have[:1], n * 1024), lambda: m.bao.have_from_status_host(status, n * 1024, 7),
                lambda: m.bao.have_from_status_host(status[:5], n * 1024)):
        with pytest.raises(m.B3WError):
            bad()
