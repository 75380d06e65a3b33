"""Set slices without a GPU (b3w_bao_set_slice_size, _batch_layout, b3w_bao_set_slice, _decode, _ingest; bao.set_slice_size,
set_slice_layout, set_slice_host, decode_set_slice, ingest_set_slice_host) on three independent legs: the restatement in
tests/bao_set_ref.py (the recursive encoder from the data alone with its places, the sequential decoder), the identities with the range
slice (one run: the range slice byte for byte; every chunk: the whole-file range slice), and the PROJECTION of a set slice onto each of
its chunks fed to the one-chunk calls (decode_slice, ingest_slice_host), which define the receiver's statuses and writes.  Files and
group_logs: test_bao_range_cpu's 51 lengths at g in {0, 1, 4, 6}."""
import ctypes
import os

import numpy as np
import pytest

import b3w_testlib as T
import bao_range_ref as RR
import bao_ref as R
import bao_set_ref as RS
from test_bao_cpu import _data, _flip
from test_bao_ingest_cpu import _fresh
from test_bao_range_cpu import ALL_LENGTHS, GS, _bits, _file, _have, _on_path_at_or_below

BAD = 100
REF_DECODE = 70                                          # the restatement's decoder hashes in plain Python: the sets up to this many chunks


def set_shapes(n):
    """-> {name: runs}: the shapes that fit a file of n chunks"""
    out = {"one run": [(n // 3, max(1, n // 4))], "the whole file": [(0, n)]}
    for a, b in ((0, 2), (63, 65), (1023, 1025)):
        if b < n:
            out[f"{{{a}, {b}}}"] = [(a, 1), (b, 1)]
    if n >= 2:
        out["first and last chunk"] = [(0, 1), (n - 1, 1)]
        out["every second chunk"] = [(c, 1) for c in range(0, n, 2)]
        out["the odd chunks"] = [(c, 1) for c in range(1, n, 2)]
    if n >= 4:
        out["a run ending on the last chunk"] = [(0, 1), (n - 2, 2)]
        out["touching runs"] = [(1, 1), (2, 1), (3, 1)] if n < 8 else [(1, 2), (3, 1), (4, 3), (n - 1, 1)]
    if n > 70:
        out["runs across the 64-chunk blocks"] = [(60, 3), (63, 2), (66, 1), (n - 3, 2)]
    return out


def _wanted(runs):
    return RS.chunks_of(runs)


def _fc(runs):
    return [a for a, _ in runs], [k for _, k in runs]


@pytest.mark.parametrize("length", ALL_LENGTHS)
def test_size_places_encoder_identities_and_decoder(length):
    m = T.pkg()
    f = _file(length)
    data, n, root = f["data"], f["n"], f["root"]
    for name, runs in set_shapes(n).items():
        first, count = _fc(runs)
        wanted = _wanted(runs)
        sl, places = RS.encode(data, runs, key=length)
        payload = sum(min(length, (c + 1) * 1024) - c * 1024 for c in wanted)
        assert len(sl) == 8 + 64 * RS.union_nodes(n, wanted, wanted[-1]) + payload == m.bao.set_slice_size(length, first, count), (length, name)
        for g in GS:
            assert m.bao.set_slice_host(f["obs"][g], length, first, count, data, g) == sl, (length, name, g)
        # the identities: one run is the range slice, every chunk the whole-file range slice
        if len(runs) == 1:
            a, k = runs[0]
            assert sl == RR.encode(data, a, k, key=length)[0], (length, name)
            assert sl == m.bao.range_slice_host(f["obs"][0], length, a, k, data[a * 1024:(a + k) * 1024]), (length, name)
        # the size against the runs' range slices
        apart = sum(m.bao.range_slice_size(length, a, k) for a, k in runs)
        assert len(sl) <= apart and (len(sl) < apart or len(runs) == 1 or n == 1), (length, name)
        # the place formulas
        parts = sorted(places.items(), key=lambda x: x[1])
        if len(parts) > 300:
            parts = parts[:40] + parts[40:-40:len(parts) // 60] + parts[-40:]
        rank = {c: i for i, c in enumerate(wanted)}
        for key, at in parts:
            if key[0] == "chunk":
                assert at == 8 + 64 * RS.union_nodes(n, wanted, key[1]) + 1024 * rank[key[1]], (length, name, key)
            else:
                c0 = min(c for c in wanted if key[1] <= c < key[1] + key[2]) if len(wanted) < 200 else next(c for c in wanted if c >= key[1])
                assert at == places[("chunk", c0)] - 64 * _on_path_at_or_below(c0, n, key[1], key[2]), (length, name, key)
        assert {key[1:] for key in places if key[0] == "node"} == {s for c in wanted for s in RR.path_spans(c, n)}, (length, name)
        # the decoder on the clean slice
        st, fb, cs, out = m.bao.decode_set_slice(sl, length, first, count, root)
        assert (st, fb) == (0, None) and not cs.any() and cs.size == len(wanted), (length, name)
        assert out == b"".join(data[c * 1024:(c + 1) * 1024] for c in wanted), (length, name)
        if len(wanted) <= REF_DECODE:
            status, got = RS.decode(sl, length, runs, root)
            assert status == [0] * len(wanted) and all(got[c] == data[c * 1024:(c + 1) * 1024] for c in wanted)
    whole = RS.encode(data, [(0, n)], key=length)[0]
    assert whole == RR.encode(data, 0, n, key=length)[0]
    assert whole == RS.encode(data, [(c, 1) for c in range(n)], key=length)[0]                     # (however S is cut into runs)
    assert m.bao.set_slice_size(length, list(range(n)), [1] * n) == len(whole)


def _by_projection(m, f, length, g, sl, places, wanted, root):
    """what the projections through the one-chunk calls give: (statuses, data, outboard, bits)"""
    exp_data, exp_ob = _fresh(length, g)
    status = []
    for c in wanted:
        p = RS.project(sl, places, length, c)
        st = m.bao.ingest_slice_host(exp_data, exp_ob, length, c, root, p, g)
        assert st == m.bao.decode_slice(p, length, c, root)[0]
        status.append(st)
    ok = {c for c, s in zip(wanted, status) if s == 0}
    return status, exp_data, exp_ob, [c in ok for c in range(f["n"])]


def _check_against_projection(m, f, length, g, sl, places, runs, root, what):
    first, count = _fc(runs)
    wanted = _wanted(runs)
    status, exp_data, exp_ob, bits = _by_projection(m, f, length, g, sl, places, wanted, root)
    got_data, got_ob = _fresh(length, g)
    have = _have(f["n"])
    bad = [c for c, s in zip(wanted, status) if s]
    st, fb, cs = m.bao.ingest_set_slice_host(got_data, got_ob, length, first, count, root, sl, g, have)
    assert (st, fb, cs.tolist()) == (max(status), bad[0] if bad else None, status), (length, g, what)
    assert got_data == exp_data and got_ob == exp_ob and _bits(have, f["n"]) == bits, (length, g, what)
    if g == 0:
        st, fb, cs, out = m.bao.decode_set_slice(sl, length, first, count, root)
        assert (st, fb, cs.tolist()) == (max(status), bad[0] if bad else None, status), (length, what)
        for r, c in enumerate(wanted):
            size = min(length, (c + 1) * 1024) - c * 1024
            assert out[r * 1024:r * 1024 + size] == (f["data"][c * 1024:c * 1024 + size] if status[r] == 0 else bytes(size)), (length, what, c)
        if len(wanted) <= REF_DECODE:
            assert RS.decode(sl, length, runs, root)[0] == status, (length, what)
    return status


@pytest.mark.parametrize("length", ALL_LENGTHS)
def test_a_set_writes_what_its_projections_write(length):
    m = T.pkg()
    f = _file(length)
    for name, runs in set_shapes(f["n"]).items():
        sl, places = RS.encode(f["data"], runs, key=length)
        for g in GS:
            assert not any(_check_against_projection(m, f, length, g, sl, places, runs, f["root"], name))


def tampers(sl, places, wanted, length, root):
    """-> [(what, slice, root, the tampered node's (lo, size) or None)]: one tamper each, beside good chunks where the set has any"""
    wrong_root = list(root)
    wrong_root[3] ^= 0x10000
    out = [("header", _flip(sl, wanted[0] % 8), root, None), ("wrong root", sl, wrong_root, None)]
    nodes = sorted((at, key[1], key[2]) for key, at in places.items() if key[0] == "node")
    if nodes:
        out.append(("the root node", _flip(sl, nodes[0][0] + (wanted[0] + 13) % 64), root, nodes[0][1:]))
        out.append(("the last node", _flip(sl, nodes[-1][0] + (wanted[0] + 5) % 64), root, nodes[-1][1:]))
        one_sided = [(at, lo, size) for at, lo, size in nodes
                     if RS._meets(wanted, lo, lo + R._split(size)) != RS._meets(wanted, lo + R._split(size), lo + size)]
        if one_sided:
            at, lo, size = max(one_sided, key=lambda x: (x[2], x[1]))
            out.append(("a node with wanted chunks on one side only", _flip(sl, at + 7), root, (lo, size)))
            out.append(("a node with wanted chunks on one side only, other half", _flip(sl, at + 39), root, (lo, size)))
    for name, c in (("first", wanted[0]), ("middle", wanted[len(wanted) // 2]), ("last", wanted[-1])):
        size = min(length, (c + 1) * 1024) - c * 1024
        if size:
            out.append((f"a byte of the {name} wanted chunk", _flip(sl, places[("chunk", c)] + (c * 7) % size), root, None))
    return out


@pytest.mark.parametrize("length", ALL_LENGTHS)
def test_tampers_have_the_projections_statuses_and_buffers(length):
    m = T.pkg()
    f = _file(length)
    for name, runs in set_shapes(f["n"]).items():
        wanted = _wanted(runs)
        sl, places = RS.encode(f["data"], runs, key=length)
        for g in (GS if len(wanted) <= REF_DECODE else [0, 4]):
            for what, bad_sl, rt, node in tampers(sl, places, wanted, length, f["root"]):
                status = _check_against_projection(m, f, length, g, bad_sl, places, runs, rt, (name, what))
                assert any(status), (length, g, name, what)
                if what == "wrong root":
                    assert set(status) == {1 if f["n"] == 1 else 2}, (length, g, name)            # a one-chunk file's wrong root is 1
                if node:                                                    # a bad node keeps out the chunks below it and no other
                    assert status == [2 if node[0] <= c < node[0] + node[1] else 0 for c in wanted], (length, g, name, what, status)
                if what.startswith("a byte of"):
                    assert sorted(status) == [0] * (len(wanted) - 1) + [1], (length, g, name, what)


def test_layout_names_abi_null_outputs_and_refusals():
    m = T.pkg()
    L = m.lib()
    assert L.b3w_abi_version() == (1 << 16) | 4                            # new names only
    names = ("b3w_bao_set_slice_size", "b3w_bao_set_slice_batch_layout", "b3w_bao_set_slice", "b3w_bao_set_slice_decode", "b3w_bao_set_slice_ingest",
             "b3w_bao_set_slice_arena_device", "b3w_bao_set_slice_ingest_scratch_bytes", "b3w_bao_set_slice_ingest_device")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "b3wit.h")).read()
    for name in names:
        assert name in m.EXPORTED_SYMBOLS and hasattr(L, name)
        assert name + "(" in header, name
    for name in ("set_slice_size", "set_slice_layout", "set_slices_arena", "ingest_set_slices", "set_slice_host", "decode_set_slice", "ingest_set_slice_host"):
        assert callable(getattr(m.bao, name))
    # the layout: sets are the stretches of one file, every start 8 modulo 16, chunk firsts the running sum
    lens = [5 * 1024 + 7, 0, 70 * 1024, 3000 * 1024]
    files, first, count = [0, 0, 1, 2, 2, 2, 3, 3], [1, 4, 0, 0, 3, 64, 5, 2999], [2, 2, 1, 3, 1, 6, 1, 1]
    lay = m.bao.set_slice_layout(lens, files, first, count)
    assert lay["set_file"].tolist() == [0, 1, 2, 3] and lay["set_range_first"].tolist() == [0, 2, 3, 6, 8]
    assert lay["set_chunk_first"].tolist() == [0, 4, 5, 15, 17]
    at = 8
    for s in range(4):
        lo, hi = lay["set_range_first"][s], lay["set_range_first"][s + 1]
        assert int(lay["slice_first"][s]) == at and at % 16 == 8
        at = ((at + m.bao.set_slice_size(lens[s], first[lo:hi], count[lo:hi]) + 7) & ~15) + 8
    assert int(lay["slice_first"][4]) == at
    u64 = lambda x: np.array(x, dtype=np.uint64)
    args = (u64(lens), np.array(files, dtype=np.uint32), u64(first), u64(count))
    raw = lambda *outs: L.b3w_bao_set_slice_batch_layout(args[0].ctypes.data, 4, args[1].ctypes.data, args[2].ctypes.data, args[3].ctypes.data, 8, *outs)
    assert raw(None, None, None, None, None) == at                         # every output may be NULL
    assert L.b3w_bao_set_slice_batch_layout(None, 0, None, None, None, 0, None, None, None, None, None) == 8
    # a row per set and touched block: sets 0 .. 2 are short (one, one and two rows of 64), set 3 touches two tiles
    assert L.b3w_bao_set_slice_ingest_scratch_bytes(*(a.ctypes.data for a in args[:1]), 4, *(a.ctypes.data for a in args[1:]), 8) == 16 * (1 + 1 + 2 + 2)
    assert L.b3w_bao_set_slice_ingest_scratch_bytes(None, 0, None, None, None, 0) == 0
    assert m.bao.set_slice_size(0, [0], [1]) == 8
    # refused lists: unsorted, overlapping, empty, past the file, a file that comes back, a file index past the count; nothing is written
    guard = np.full(16, 0xEEEEEEEE, dtype=np.uint32)
    g64 = np.full(16, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    k = ctypes.c_uint32(77)
    for fi, fc, nc in (([0, 0], [4, 1], [1, 1]), ([0, 0], [1, 2], [2, 1]), ([0], [1], [0]), ([0], [5], [2]), ([0], [6], [1]), ([0, 2, 0], [0, 0, 3], [1, 1, 1]),
                       ([2, 0], [0, 0], [1, 1]), ([4], [0], [1]), ([2, 2], [3, 3], [1, 1])):
        with pytest.raises(m.B3WError):
            m.bao.set_slice_layout(lens, fi, fc, nc)
        a = (u64(lens), np.array(fi, dtype=np.uint32), u64(fc), u64(nc))
        assert L.b3w_bao_set_slice_batch_layout(a[0].ctypes.data, 4, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, len(fi), guard.ctypes.data,
                                                guard.ctypes.data, g64.ctypes.data, g64.ctypes.data, ctypes.byref(k)) == -BAD, (fi, fc, nc)
        assert (guard == 0xEEEEEEEE).all() and (g64 == 0xEEEEEEEEEEEEEEEE).all() and k.value == 77
        assert L.b3w_bao_set_slice_ingest_scratch_bytes(a[0].ctypes.data, 4, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, len(fi)) == 0
        if len(set(fi)) == 1 and fi[0] < 4:
            assert L.b3w_bao_set_slice_size(lens[fi[0]], a[2].ctypes.data, a[3].ctypes.data, len(fi)) == 0
    assert L.b3w_bao_set_slice_size(lens[0], None, None, 0) == 0 and L.b3w_bao_set_slice_size(lens[0], None, None, 1) == 0
    # the one-file calls: refusals leave the outputs untouched
    length = lens[0]
    data = _data(length)
    ob, root = R.outboard(data)
    runs = [(1, 2), (4, 2)]
    sl = RS.encode(data, runs)[0]
    rw = np.array(root, dtype=np.uint32)
    got_data, got_ob = _fresh(length, 0)
    have = np.full(1, 0x40, dtype=np.uint64)
    clean = bytes(got_data), bytes(got_ob)
    d = (ctypes.c_uint8 * length).from_buffer(got_data)
    o = (ctypes.c_uint8 * len(got_ob)).from_buffer(got_ob)
    st, fb = ctypes.c_int32(-7), ctypes.c_uint64(77)
    cs = np.full(4, -9, dtype=np.int32)
    good = (u64([1, 4]), u64([2, 2]))

    def ingest(sl=sl, slice_len=len(sl), fc=good[0], nc=good[1], k=2, root=rw.ctypes.data, g=0, data=d, ob=o, status=ctypes.byref(st), chunk=cs.ctypes.data):
        return L.b3w_bao_set_slice_ingest(sl, slice_len, length, fc.ctypes.data if fc is not None else None, nc.ctypes.data if nc is not None else None, k, root, g,
                                          data, ob, have.ctypes.data, chunk, status, ctypes.byref(fb))
    for kw in (dict(sl=None), dict(root=None), dict(status=None), dict(data=None), dict(ob=None), dict(k=0), dict(fc=None), dict(nc=None), dict(g=7),
               dict(fc=u64([4, 1])), dict(fc=u64([1, 2])), dict(nc=u64([2, 0])), dict(nc=u64([2, 3])), dict(fc=u64([1, 6])),
               dict(slice_len=len(sl) - 1), dict(sl=sl + b"\0", slice_len=len(sl) + 1), dict(k=1)):
        assert ingest(**kw) == BAD, kw
        assert (bytes(got_data), bytes(got_ob), int(have[0]), st.value, fb.value, cs.tolist()) == clean + (0x40, -7, 77, [-9] * 4), kw
    out = (ctypes.c_uint8 * 4096)(*([0xEE] * 4096))
    for a in ((None, len(sl), length, good[0].ctypes.data, good[1].ctypes.data, 2, rw.ctypes.data), (sl, len(sl), length, good[0].ctypes.data, good[1].ctypes.data, 2, None),
              (sl, len(sl) + 1, length, good[0].ctypes.data, good[1].ctypes.data, 2, rw.ctypes.data), (sl, len(sl), length, good[0].ctypes.data, good[1].ctypes.data, 0, rw.ctypes.data),
              (sl, len(sl), length, good[1].ctypes.data, good[0].ctypes.data, 2, rw.ctypes.data)):
        assert L.b3w_bao_set_slice_decode(*a, out, cs.ctypes.data, ctypes.byref(st), ctypes.byref(fb)) == BAD
        assert bytes(out) == bytes([0xEE]) * 4096 and (st.value, fb.value, cs.tolist()) == (-7, 77, [-9] * 4)
    assert L.b3w_bao_set_slice_decode(sl, len(sl), length, good[0].ctypes.data, good[1].ctypes.data, 2, rw.ctypes.data, out, None, None, None) == BAD
    # NULL outputs: no bytes, no chunk statuses, no first bad
    assert L.b3w_bao_set_slice_decode(sl, len(sl), length, good[0].ctypes.data, good[1].ctypes.data, 2, rw.ctypes.data, None, None, ctypes.byref(st), None) == 0
    assert st.value == 0 and bytes(out) == bytes([0xEE]) * 4096
    st.value = -7
    small = (ctypes.c_uint8 * 16)(*([0xEE] * 16))
    enc = lambda *a: L.b3w_bao_set_slice(*a)
    assert enc(ob, length, 0, good[0].ctypes.data, good[1].ctypes.data, 2, data, None, 0) == len(sl)         # out == NULL asks for the size
    for a in ((ob, length, 0, good[0].ctypes.data, good[1].ctypes.data, 2, data, small, 16), (None, length, 0, good[0].ctypes.data, good[1].ctypes.data, 2, data, small, 16),
              (ob, length, 0, good[0].ctypes.data, good[1].ctypes.data, 2, None, small, 16), (ob, length, 7, good[0].ctypes.data, good[1].ctypes.data, 2, data, small, 16),
              (ob, length, 0, good[1].ctypes.data, good[0].ctypes.data, 2, data, small, 16), (ob, length, 0, good[0].ctypes.data, good[1].ctypes.data, 0, data, small, 16)):
        assert enc(*a) == -BAD and bytes(small) == bytes([0xEE]) * 16
    assert ingest(chunk=None) == 0 and (st.value, fb.value) == (0, 2 ** 64 - 1) and int(have[0]) == 0x40 | 0b110110 and cs.tolist() == [-9] * 4
    assert ingest() == 0 and cs.tolist() == [0] * 4
    with pytest.raises(m.B3WError):
        m.bao.ingest_set_slice_host(got_data, got_ob, length, [1, 4], [2, 2], root, sl, group_log=7)
    with pytest.raises(m.B3WError):
        m.bao.ingest_set_slice_host(got_data, bytearray(8), length, [1, 4], [2, 2], root, sl)
    with pytest.raises(m.B3WError):
        m.bao.set_slice_host(ob, length, [1, 4], [2, 2], data[:-1])
    # the empty file: one chunk, the slice is the header
    e_ob, e_root = R.outboard(b"")
    e_sl = RS.encode(b"", [(0, 1)])[0]
    assert e_sl == bytes(8) == m.bao.set_slice_host(e_ob, 0, [0], [1], b"")
    assert m.bao.decode_set_slice(e_sl, 0, [0], [1], e_root)[:2] == (0, None)
    target, e_have = bytearray([0xEE]) * 8, _have(1)
    assert m.bao.ingest_set_slice_host(bytearray(), target, 0, [0], [1], e_root, e_sl, 0, e_have)[:2] == (0, None)
    assert bytes(target) == e_ob and int(e_have[0]) == 1
    wrong = list(e_root)
    wrong[0] ^= 1
    target, e_have = bytearray([0xEE]) * 8, _have(1)
    assert m.bao.ingest_set_slice_host(bytearray(), target, 0, [0], [1], wrong, e_sl, 0, e_have)[:2] == (1, 0)   # a one-chunk file's wrong root is 1
    assert bytes(target) == bytes([0xEE]) * 8 and int(e_have[0]) == 0
