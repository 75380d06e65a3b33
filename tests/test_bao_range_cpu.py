"""Range slices without a GPU (b3w_bao_range_slice_size, _batch_layout, b3w_bao_range_slice, _decode, _ingest; bao.range_slice_size,
range_slice_layout, range_slice_host, decode_range_slice, ingest_range_slice_host) on three independent legs: the restatement in
tests/bao_range_ref.py (the recursive encoder from the data alone, the sequential decoder), the identity of a range of one chunk with
bao_ref.slice_chunk / b3w_bao_slice, and the PROJECTION of a range slice onto each of its chunks fed to the existing, tested one-chunk
calls (decode_slice, ingest_slice_host), which define the receiver's statuses and writes.  Files: test_bao_cpu.LENGTHS plus exactly 63,
64, 65, 1 025 and 2 049 chunks, at g in {0, 1, 4, 6}."""
import ctypes
import struct

import numpy as np
import pytest

import b3w_testlib as T
import bao_range_ref as RR
import bao_ref as R
from test_bao_cpu import LENGTHS, _data, _flip
from test_bao_ingest_cpu import _fresh, _want_outboard
from test_bao_slices_cpu import _made

BAD = 100
GS = [0, 1, 4, 6]
EXTRA = [n * 1024 for n in (63, 64, 65, 1025, 2049)]
ALL_LENGTHS = LENGTHS + EXTRA
CROSS = [x for x in LENGTHS if x <= 6 * 1024] + [17 * 1024 + 300, 40 * 1024]   # where bao_ref / bao_groups_ref restate the outboards too
REF_DECODE = 70                                          # the restatement's decoder hashes in plain Python: the ranges up to this many chunks
_FILES = {}


def _file(length):
    """-> dict(data, n, root, obs: {g: outboard}): the outboards read off the restatement's whole-file slice (a group outboard is the
    pre-order of the nodes over more than a group); held against bao_ref / bao_groups_ref where those are cheap"""
    if length not in _FILES:
        data = _data(length)
        n = R.num_chunks(length)
        RR.seed(data, length)
        whole, places = RR.encode(data, 0, n, key=length)
        nodes = sorted((at, key[2]) for key, at in places.items() if key[0] == "node")
        obs = {g: whole[:8] + b"".join(whole[at:at + 64] for at, size in nodes if size > (1 << g)) for g in GS}
        root = RR._subtree_cv(data, length, 0, n, True)
        if length in CROSS:
            assert (data, obs[0], root) == _made(length)
            for g in GS[1:]:
                assert obs[g] == _want_outboard(length, g), (length, g)
        _FILES[length] = dict(data=data, n=n, root=root, obs=obs)
    return _FILES[length]


def _split_ranges(n):
    """both sides of and across the splits of the tree's top three levels"""
    out = set()

    def walk(lo, m, depth):
        if m > 1 and depth:
            k = R._split(m)
            out.update([(lo, k), (lo + k, m - k), (lo + k - 1, 2)])
            walk(lo, k, depth - 1)
            walk(lo + k, m - k, depth - 1)
    walk(0, n, 3)
    return out


def _long_ranges(n):
    """every kind but the single chunks: the whole file, the splits, the ragged end, the group boundaries, the tile boundary"""
    out = {(0, n), (n - 1, 1)} | _split_ranges(n)
    if n >= 2:
        out.add((n - 2, 2))
    for g in GS[1:]:
        G = 1 << g
        for gs in {0, ((n - 1) // G) * G, ((n - 1) // G // 2) * G}:
            inside = min(G, n - gs) - 2
            if inside >= 1:
                out.add((gs + 1, inside))                                 # inside one group
            if gs + G + 1 <= n:
                out.add((gs, G + 1))                                      # ends one chunk into the next group
                out.add((gs + G - 1, 2))                                  # starts one chunk before a boundary
    if n > 1024:
        out.add((1022, min(4, n - 1022)))                                 # (the 1 025-chunk file ends before 1 022 + 4 and 1 023 + 1 026)
        out.add((1023, min(1026, n - 1023)))
    return sorted(out)


def _group_bytes(f, length, a, k, g):
    g0 = (a >> g) << g
    g1 = min(f["n"], (((a + k - 1) >> g) + 1) << g)
    return f["data"][g0 * 1024:min(length, g1 * 1024)]


def _on_path_at_or_below(c, n, lo, size):
    return sum(1 for x, m in RR.path_spans(c, n) if x >= lo and x + m <= lo + size)


@pytest.mark.parametrize("length", ALL_LENGTHS)
def test_size_places_extractors_and_decoder(length):
    m = T.pkg()
    f = _file(length)
    data, n, root = f["data"], f["n"], f["root"]
    singles = [(c, 1) for c in range(n)]
    for a, k in singles + _long_ranges(n):
        sl, places = RR.encode(data, a, k, key=length)
        payload = min(length, (a + k) * 1024) - a * 1024
        assert len(sl) == 8 + 64 * RR.union_nodes(n, a, a + k - 1) + payload == m.bao.range_slice_size(length, a, k), (length, a, k)
        for g in GS:
            assert m.bao.range_slice_host(f["obs"][g], length, a, k, _group_bytes(f, length, a, k, g), g) == sl, (length, a, k, g)
        if k == 1:
            assert sl == R.slice_chunk(f["obs"][0], data, a) == m.bao.slice_chunk(f["obs"][0], length, a, data[a * 1024:(a + 1) * 1024]), (length, a)
            continue
        parts = sorted(places.items(), key=lambda x: x[1])
        if len(parts) > 300:                                              # the long ranges: the ends and every so-manieth part
            parts = parts[:40] + parts[40:-40:len(parts) // 60] + parts[-40:]
        for key, at in parts:                                             # the two formulas
            if key[0] == "chunk":
                assert at == 8 + 64 * RR.union_nodes(n, a, key[1]) + 1024 * (key[1] - a), (length, a, k, key)
            else:
                c0 = max(key[1], a)
                assert at == places[("chunk", c0)] - 64 * _on_path_at_or_below(c0, n, key[1], key[2]), (length, a, k, key)
        in_slice = {key[1:] for key in places if key[0] == "node"}            # the union of the one-chunk slices' path nodes
        assert in_slice == {s for c in range(a, a + k) for s in RR.path_spans(c, n)}, (length, a, k)
        assert m.bao.decode_range_slice(sl, length, a, k, root) == (0, None, data[a * 1024:a * 1024 + payload]), (length, a, k)
        if k <= REF_DECODE:
            status, got = RR.decode(sl, length, a, k, root)
            assert status == [0] * k and b"".join(got[c] for c in range(a, a + k)) == data[a * 1024:a * 1024 + payload]


def _have(n):
    return np.zeros((n + 63) // 64, dtype=np.uint64)


def _bits(have, n):
    return [bool((int(have[c >> 6]) >> (c & 63)) & 1) for c in range(n)]


@pytest.mark.parametrize("length", ALL_LENGTHS)
def test_every_range_in_shuffled_order_gives_the_file_and_the_providers_outboard(length):
    m = T.pkg()
    f = _file(length)
    n = f["n"]
    ranges = [(c, 1) for c in range(n)] + _long_ranges(n)
    for g in GS:
        got_data, got_ob = _fresh(length, g)
        have = _have(n)
        for i in np.random.default_rng(77 * g + length).permutation(len(ranges)):
            a, k = ranges[i]
            sl = RR.encode(f["data"], a, k, key=length)[0]
            assert m.bao.ingest_range_slice_host(got_data, got_ob, length, a, k, f["root"], sl, g, have) == (0, None), (length, g, a, k)
        assert bytes(got_data) == f["data"] and bytes(got_ob) == f["obs"][g], (length, g)
        assert all(_bits(have, n)) and int(have[-1]) >> ((n - 1) % 64 + 1) == 0, (length, g)


def _by_projection(m, f, length, g, sl, places, a, k, root):
    """what the projections through the one-chunk calls give: (statuses, data, outboard, bits)"""
    exp_data, exp_ob = _fresh(length, g)
    status = []
    for c in range(a, a + k):
        p = RR.project(sl, places, length, c)
        st = m.bao.ingest_slice_host(exp_data, exp_ob, length, c, root, p, g)
        assert st == m.bao.decode_slice(p, length, c, root)[0]
        status.append(st)
    bits = [a <= c < a + k and status[c - a] == 0 for c in range(f["n"])]
    return status, exp_data, exp_ob, bits


def _check_against_projection(m, f, length, g, sl, places, a, k, root, what):
    status, exp_data, exp_ob, bits = _by_projection(m, f, length, g, sl, places, a, k, root)
    got_data, got_ob = _fresh(length, g)
    have = _have(f["n"])
    bad = [a + i for i, s in enumerate(status) if s]
    want = (max(status), bad[0] if bad else None)
    assert m.bao.ingest_range_slice_host(got_data, got_ob, length, a, k, root, sl, g, have) == want, (length, g, a, k, what)
    assert got_data == exp_data and got_ob == exp_ob and _bits(have, f["n"]) == bits, (length, g, a, k, what)
    if g == 0:
        st, fb, out = m.bao.decode_range_slice(sl, length, a, k, root)
        assert (st, fb) == want, (length, a, k, what)
        for c in range(a, a + k):
            lo, hi = (c - a) * 1024, min(length, (c + 1) * 1024) - a * 1024
            assert out[lo:hi] == (f["data"][c * 1024:c * 1024 + hi - lo] if status[c - a] == 0 else bytes(hi - lo)), (length, a, k, what, c)
        if k <= REF_DECODE:
            assert RR.decode(sl, length, a, k, root)[0] == status, (length, a, k, what)
    return status


@pytest.mark.parametrize("length", ALL_LENGTHS)
def test_one_range_writes_what_its_projections_write(length):
    m = T.pkg()
    f = _file(length)
    for a, k in _long_ranges(f["n"]):
        sl, places = RR.encode(f["data"], a, k, key=length)
        for g in GS:
            assert not any(_check_against_projection(m, f, length, g, sl, places, a, k, f["root"], "clean"))


def _tampers(sl, places, a, k, length, root):
    """-> [(what, slice, root, the tampered node's (lo, size) or None)]"""
    wrong_root = list(root)
    wrong_root[3] ^= 0x10000
    out = [("header", _flip(sl, a % 8), root, None), ("root", sl, wrong_root, None)]
    nodes = sorted((at, key[1], key[2]) for key, at in places.items() if key[0] == "node")
    if nodes:
        out.append(("first node", _flip(sl, nodes[0][0] + (a + 13) % 64), root, nodes[0][1:]))
        out.append(("last node", _flip(sl, nodes[-1][0] + (a + 5) % 64), root, nodes[-1][1:]))
        late = [x for x in nodes if x[1] >= a + (k + 1) // 2]               # a subtree that covers only the second half of the range
        if late:
            at, lo, size = max(late, key=lambda x: x[2])
            out.append(("a node over the second half", _flip(sl, at + 7), root, (lo, size)))
            out.append(("a node over the second half, other side", _flip(sl, at + 39), root, (lo, size)))
    for name, c in (("first", a), ("middle", a + k // 2), ("last", a + k - 1)):
        size = min(length, (c + 1) * 1024) - c * 1024
        if size:
            out.append((f"a byte of the {name} chunk", _flip(sl, places[("chunk", c)] + (c * 7) % size), root, None))
    return out


def _tamper_ranges(n):
    out = {(0, n)} if n <= 65 else set()
    out |= {r for r in _split_ranges(n) if r[1] <= 70}
    if n > 1024:
        out |= {(1022, min(4, n - 1022)), (1023, min(1026, n - 1023))}
    return sorted(out)


@pytest.mark.parametrize("length", ALL_LENGTHS)
def test_tampers_have_the_projections_statuses_and_buffers(length):
    m = T.pkg()
    f = _file(length)
    for a, k in _tamper_ranges(f["n"]):
        sl, places = RR.encode(f["data"], a, k, key=length)
        for g in (GS if k <= 70 else [0, 4]):
            for what, bad_sl, rt, node in _tampers(sl, places, a, k, length, f["root"]):
                status = _check_against_projection(m, f, length, g, bad_sl, places, a, k, rt, what)
                assert any(status), (length, g, a, k, what)
                if node:                                                    # a bad node keeps out the chunks below it and no other
                    below = [node[0] <= c < node[0] + node[1] for c in range(a, a + k)]
                    assert status == [2 if b else 0 for b in below], (length, g, a, k, what, status)
                    assert not what.startswith("a node over the second half") or status[0] == 0      # the chunks before it still come in


def test_layout_names_abi_refusals_and_the_empty_file():
    m = T.pkg()
    L = m.lib()
    assert L.b3w_abi_version() == (1 << 16) | 4                            # new names only
    names = ("b3w_bao_range_slice_size", "b3w_bao_range_slice_batch_layout", "b3w_bao_range_slice", "b3w_bao_range_slice_decode",
             "b3w_bao_range_slice_ingest", "b3w_bao_range_slice_arena_device", "b3w_bao_range_slice_ingest_scratch_bytes",
             "b3w_bao_range_slice_ingest_device")
    header = open(T.ROOT + "/include/b3wit.h").read() if hasattr(T, "ROOT") else None
    for name in names:
        assert name in m.EXPORTED_SYMBOLS and hasattr(L, name)
        assert header is None or name + "(" in header
    for name in ("range_slice_size", "range_slice_layout", "range_slices_arena", "ingest_range_slices", "range_slice_host", "decode_range_slice",
                 "ingest_range_slice_host"):
        assert callable(getattr(m.bao, name))
    # the layout: every start 8 modulo 16, a k = 1 range the size of the one-chunk slice
    lens = [5 * 1024 + 7, 0, 70 * 1024]
    files, first, count = [0, 2, 1, 2, 0], [1, 3, 0, 69, 5], [3, 64, 1, 1, 1]
    sf = m.bao.range_slice_layout(lens, files, first, count)
    at = 8
    for i in range(5):
        assert int(sf[i]) == at and at % 16 == 8
        at = ((at + m.bao.range_slice_size(lens[files[i]], first[i], count[i]) + 7) & ~15) + 8
    assert int(sf[5]) == at
    assert m.bao.range_slice_size(lens[2], 69, 1) == m.bao.slice_size(lens[2], 69) and m.bao.range_slice_size(0, 0, 1) == 8
    for bad in ((0, 0, 0), (0, 6, 1), (0, 5, 2), (1, 1, 1), (3, 0, 1)):
        with pytest.raises(m.B3WError):
            m.bao.range_slice_layout(lens, [bad[0]], [bad[1]], [bad[2]])
    assert L.b3w_bao_range_slice_size(lens[0], 0, 0) == 0 and L.b3w_bao_range_slice_size(lens[0], 2, 2 ** 64 - 1) == 0
    assert L.b3w_bao_range_slice_ingest_scratch_bytes(None, 0, None, None, None, 0) == 0
    # refusals leave the outputs untouched
    length = lens[0]
    data = _data(length)
    ob, root = R.outboard(data)
    sl = RR.encode(data, 1, 3)[0]
    rw = np.array(root, dtype=np.uint32)
    got_data, got_ob = _fresh(length, 0)
    have = np.full(1, 0x5555, dtype=np.uint64)
    clean = bytes(got_data), bytes(got_ob)
    d = (ctypes.c_uint8 * length).from_buffer(got_data)
    o = (ctypes.c_uint8 * len(got_ob)).from_buffer(got_ob)
    st, fb = ctypes.c_int32(-7), ctypes.c_uint64(77)

    def ingest(sl=sl, slice_len=len(sl), a=1, k=3, root=rw.ctypes.data, g=0, data=d, ob=o, status=ctypes.byref(st)):
        return L.b3w_bao_range_slice_ingest(sl, slice_len, length, a, k, root, g, data, ob, have.ctypes.data, status, ctypes.byref(fb))
    for kw in (dict(sl=None), dict(root=None), dict(status=None), dict(data=None), dict(ob=None), dict(k=0), dict(a=6), dict(a=4, k=3), dict(g=7),
               dict(slice_len=len(sl) - 1), dict(sl=sl + b"\0", slice_len=len(sl) + 1), dict(k=2)):
        assert ingest(**kw) == BAD, kw
        assert (bytes(got_data), bytes(got_ob), int(have[0]), st.value, fb.value) == clean + (0x5555, -7, 77), kw
    out = (ctypes.c_uint8 * 4096)(*([0xEE] * 4096))
    for args in ((None, len(sl), length, 1, 3, rw.ctypes.data), (sl, len(sl), length, 1, 3, None), (sl, len(sl) + 1, length, 1, 3, rw.ctypes.data),
                 (sl, len(sl), length, 1, 0, rw.ctypes.data), (sl, len(sl), length, 5, 2, rw.ctypes.data)):
        assert L.b3w_bao_range_slice_decode(*args, out, ctypes.byref(st), ctypes.byref(fb)) == BAD
        assert bytes(out) == bytes([0xEE]) * 4096 and (st.value, fb.value) == (-7, 77)
    assert L.b3w_bao_range_slice_decode(sl, len(sl), length, 1, 3, rw.ctypes.data, out, None, None) == BAD
    small = (ctypes.c_uint8 * 16)(*([0xEE] * 16))
    assert L.b3w_bao_range_slice(ob, length, 0, 1, 3, data[1024:4096], None, 0) == len(sl)       # out == NULL asks for the size
    for args in ((ob, length, 0, 1, 3, data[1024:4096], small, 16), (None, length, 0, 1, 3, data[1024:4096], small, 16),
                 (ob, length, 0, 1, 3, None, small, 16), (ob, length, 7, 1, 3, data[1024:4096], small, 16), (ob, length, 0, 1, 0, data[1024:4096], small, 16),
                 (ob, length, 0, 4, 3, data[1024:4096], small, 16)):
        assert L.b3w_bao_range_slice(*args) == -BAD and bytes(small) == bytes([0xEE]) * 16
    assert ingest() == 0 and (st.value, fb.value) == (0, 2 ** 64 - 1) and int(have[0]) == 0x5555 | 0b1110
    with pytest.raises(m.B3WError):
        m.bao.ingest_range_slice_host(got_data, got_ob, length, 1, 3, root, sl, group_log=7)
    with pytest.raises(m.B3WError):
        m.bao.ingest_range_slice_host(got_data, bytearray(8), length, 1, 3, root, sl)
    with pytest.raises(m.B3WError):
        m.bao.range_slice_host(ob, length, 1, 3, data[1024:4095])
    # the empty file: one chunk, the slice is the header
    e_ob, e_root = R.outboard(b"")
    e_sl = RR.encode(b"", 0, 1)[0]
    assert e_sl == bytes(8) == m.bao.range_slice_host(e_ob, 0, 0, 1, b"")
    assert m.bao.decode_range_slice(e_sl, 0, 0, 1, e_root) == (0, None, b"")
    target, e_have = bytearray([0xEE]) * 8, _have(1)
    assert m.bao.ingest_range_slice_host(bytearray(), target, 0, 0, 1, e_root, e_sl, 0, e_have) == (0, None)
    assert bytes(target) == e_ob and int(e_have[0]) == 1
    wrong = list(e_root)
    wrong[0] ^= 1
    target, e_have = bytearray([0xEE]) * 8, _have(1)
    assert m.bao.ingest_range_slice_host(bytearray(), target, 0, 0, 1, wrong, e_sl, 0, e_have) == (1, 0)      # a one-chunk file's wrong root is 1
    assert bytes(target) == bytes([0xEE]) * 8 and int(e_have[0]) == 0
    assert struct.unpack("<Q", e_sl)[0] == 0
