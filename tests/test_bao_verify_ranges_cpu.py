"""Listed chunk ranges verified against an outboard, without a GPU: the library's host walk (b3w_bao_verify_ranges,
bao.verify_ranges_host) against the whole-file decoders (bao.verify_host everywhere, tests/bao_verify_ref.py on one tamper per length
and g), read at the listed units.  What the ranged walk may not write keeps a 0xEE prefill; what it may not read is shown by poison
(the arena outside the listed units and every stored node with no listed unit below it are 0xEE and the result is unchanged); the
per-range outputs against the same reduction in numpy; b3w_bao_verify_ranges_scratch_bytes against counts made here; the names, the
ABI number and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
import bao_ref as R
import bao_update_ref as U
import bao_verify_ref as V
import test_bao_cpu as C
from test_bao_update_cpu import _dirty_sets, _made, _ranges

GS = (0, 1, 4, 6)
NAMES = {"b3w_bao_verify_ranges_batch_device": 21, "b3w_bao_verify_ranges_scratch_bytes": 5, "b3w_bao_verify_ranges": 11}
NONE = (1 << 64) - 1
FILL = 0xEE


def _flip(b, i, bit=0x10):
    out = bytearray(b)
    out[i] ^= bit
    return bytes(out)


def _host(L, data, ob, root, ranges, g):
    """b3w_bao_verify_ranges over a 0xEE prefill -> (unit bytes, range statuses, range first bad units)"""
    nu = GR.num_groups(R.num_chunks(len(data)), g)
    st = np.full(nu, FILL, dtype=np.uint8)
    rw = np.array(root, dtype=np.uint32)
    fc = np.array([a for a, _ in ranges], dtype=np.uint64)
    nc = np.array([c for _, c in ranges], dtype=np.uint64)
    rs, rf = np.full(len(ranges), -7, dtype=np.int32), np.full(len(ranges), 7, dtype=np.uint64)
    assert L.b3w_bao_verify_ranges(data, len(data), ob, g, rw.ctypes.data, fc.ctypes.data, nc.ctypes.data, len(ranges), st.ctypes.data, rs.ctypes.data,
                                   rf.ctypes.data) == 0
    return st, rs.tolist(), rf.tolist()


def _reduced(want, ranges, g):
    """the per-range outputs from a whole-file decoder's unit bytes"""
    rs, rf = [], []
    for a, c in ranges:
        units = range(a >> g, ((a + c - 1) >> g) + 1) if c else []
        bad = [u for u in units if want[u]]
        rs.append(max((int(want[u]) for u in units), default=0))
        rf.append(bad[0] if bad else NONE)
    return rs, rf


def _tampers(data, ob, root, n, g, units):
    """name -> (data, outboard, root) with one tamper each; a place that does not exist in this file is left out"""
    nu = GR.num_groups(n, g)
    listed = set(units)
    keep = set(U.dirty_nodes(nu, units))
    out = {"clean": (data, ob, root)}
    for name, want_listed in (("a byte in a listed chunk", True), ("a byte in an unlisted chunk", False)):
        for c in range(n):
            a, b = R.chunk_range(len(data), c)
            if ((c >> g) in listed) == want_listed and b > a:
                out[name] = (_flip(data, a + (c * 7) % (b - a)), ob, root)
                break
    for name, want_listed in (("a node on a listed path", True), ("a node on no listed path", False)):
        for i in reversed(range(nu - 1)):                                  # (the deepest such node first: it is not the root node where another one is)
            if (i in keep) == want_listed:
                out[name] = (data, _flip(ob, 8 + 64 * i + (i * 5) % 64), root)
                break
    out["the root"] = (data, ob, [root[0] ^ 1] + list(root[1:]))
    out["the header"] = (data, _flip(ob, 3), root)
    return out


def test_the_names_are_declared_exported_and_bound():
    m = T.pkg()
    L = m.lib()
    hdr = open(os.path.join(T.ROOT, "include", "b3wit.h")).read()
    declared = set(re.findall(r"\b(b3w_[a-z0-9_]+)\s*\(", hdr))
    for name, n_args in NAMES.items():
        assert name in declared and name in m.EXPORTED_SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, name
    assert L.b3w_bao_verify_ranges_batch_device.restype is ctypes.c_int32 and L.b3w_bao_verify_ranges_scratch_bytes.restype is ctypes.c_uint64
    assert L.b3w_abi_version() == (1 << 16) + 4                                # new names only: the number stays
    for name in ("verify_ranges_batch", "verify_ranges_host", "chunk_ranges"):
        assert callable(getattr(m.bao, name)), name


@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("length", C.LENGTHS)
def test_listed_units_get_the_whole_file_decoders_bytes_and_nothing_else_is_written(length, g):
    m = T.pkg()
    L = m.lib()
    data, ob, root = _made(length, g)
    n = R.num_chunks(length)
    nu = GR.num_groups(n, g)
    seen = set()
    for name, chunks in _dirty_sets(n).items():
        ranges = _ranges(chunks)
        units = U.dirty_units(ranges, n, g)
        is_listed = np.zeros(nu, dtype=bool)
        is_listed[units] = True
        for tamper, (d, o, r) in _tampers(data, ob, root, n, g, units).items():
            seen.add(tamper)
            want, _, _ = m.bao.verify_host(d, o, r, g)
            if tamper == "a node on a listed path" and name == "middle":
                assert V.verify(d, o, r, length, g) == want.tolist(), (length, g)  # (the two oracles agree)
            st, rs, rf = _host(L, d, o, r, ranges, g)
            assert (st[is_listed] == want[is_listed]).all(), (length, g, name, tamper)
            assert (st[~is_listed] == FILL).all(), (length, g, name, tamper)
            assert (rs, rf) == _reduced(want, ranges, g), (length, g, name, tamper)
            if tamper in ("a byte in an unlisted chunk", "a node on no listed path"):
                assert not st[is_listed].any() and not any(rs), (length, g, name, tamper)
            elif tamper != "clean" and units:
                assert st[is_listed].any(), (length, g, name, tamper)
            # the Python call: the same bytes over its own prefill
            if tamper in ("clean", "a node on a listed path"):
                p_st, p_rs, p_rf = m.bao.verify_ranges_host(d, o, r, [a for a, _ in ranges], [c for _, c in ranges], g)
                assert (p_st[is_listed] == want[is_listed]).all() and (p_st[~is_listed] == 0xFF).all(), (length, g, name, tamper)
                assert (p_rs.tolist(), p_rf.tolist()) == (rs, rf), (length, g, name, tamper)
            # poison: what the contract says is not read is 0xEE, and the outputs are those of the untouched inputs
            if tamper in ("clean", "a byte in a listed chunk", "a node on a listed path"):
                pd = bytearray(b"\xEE" * length)
                for u in units:
                    a, b = (u << g) * 1024, min(length, ((u + 1) << g) * 1024)
                    pd[a:b] = d[a:b]
                po, _ = U.poison(o, nu, units)
                if not units:
                    po = b"\xEE" * len(o)                                  # (nothing listed: not even the header is read)
                assert [x.tolist() if isinstance(x, np.ndarray) else x for x in _host(L, bytes(pd), po, r, ranges, g)] == [st.tolist(), rs, rf], \
                    (length, g, name, tamper)
        # the same ranges many times over, reversed and overlapping: the same unit bytes, and each range its own outputs
        if chunks:
            messy = [(c, 1) for c in reversed(chunks)] + ranges + [(chunks[0], min(3, n - chunks[0])), (chunks[-1], 0), (n, 0)]
            d, o, r = _tampers(data, ob, root, n, g, units).get("a node on a listed path", (data, ob, root))
            want, _, _ = m.bao.verify_host(d, o, r, g)
            also = np.zeros(nu, dtype=bool)
            also[U.dirty_units(messy, n, g)] = True
            st, rs, rf = _host(L, d, o, r, messy, g)
            assert (st[also] == want[also]).all() and (st[~also] == FILL).all(), (length, g, name)
            assert (rs, rf) == _reduced(want, messy, g), (length, g, name)
    assert {"clean", "the root", "the header"} <= seen
    if nu >= 4:
        assert len(seen) == 7, (length, g, seen)


def _scratch(L, lens, files, firsts, counts):
    ln, fi = np.array(lens, dtype=np.uint64), np.array(files, dtype=np.uint32)
    fc, nc = np.array(firsts, dtype=np.uint64), np.array(counts, dtype=np.uint64)
    return L.b3w_bao_verify_ranges_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)


def test_scratch_sizes_equal_counts_made_here():
    L = T.pkg().lib()
    K = 1024
    #       0     1        2          3             4                5                  6 (1 026 tiles)
    lens = [0, 5 * K, 64 * K, 65 * K + 3, (1 << 20) + 1, 2051 * K - 300, (1 << 30) + (1 << 20) + 5]
    cases = [
        ([0, 1, 2, 3], [0, 2, 0, 7], [1, 3, 64, 50]),                          # files of one tile: none
        ([4], [0], [1]), ([4], [1024], [1]), ([4], [1023], [2]), ([4, 4, 4], [5, 5, 1000], [1, 1, 30]),
        ([5, 5, 5], [2050, 0, 1020], [1, 1, 11]),                              # three tiles, out of order
        ([5, 5, 5, 5], [100, 90, 100, 1500], [2000, 20, 2000, 1]),             # overlapping and duplicated
        ([6], [0], [1]), ([6, 6, 6, 6], [0, 1023 * K, 1024 * K, 1025 * K], [1, 1, 1, 1]),
        ([6, 5, 6, 1, 4], [1024 * K - 1, 2047, 1024 * K - 1, 0, 1000], [2, 2, 2, 5, 25]),
        ([6], [0], [1025 * K + 1025]),                                          # all of it: 1 026 tiles and 2 spans
        ([5, 6], [3, 3], [0, 0]),                                               # empty ranges
    ]
    want = [0, 1, 1, 2, 2, 3, 3, 1 + 1, 4 + 2, (2 + 2) + 2 + 0 + 2, 1026 + 2, 0]
    for (files, firsts, counts), w in zip(cases, want):
        assert U.scratch_items(lens, files, firsts, counts) == w, (files, firsts, counts)
        assert _scratch(L, lens, files, firsts, counts) == (36 * w + 15) // 16 * 16, (files, firsts, counts)
    assert L.b3w_bao_verify_ranges_scratch_bytes(None, None, None, None, 0) == 0
    one = (ctypes.c_uint64 * 1)(5 << 20)
    assert L.b3w_bao_verify_ranges_scratch_bytes(one, None, one, one, 1) == 0 and L.b3w_bao_verify_ranges_scratch_bytes(None, one, one, one, 1) == 0


def test_refusals_that_need_no_device():
    m = T.pkg()
    L = m.lib()
    bad = m.B3W_E_BAD_ARGUMENT
    one = (ctypes.c_uint64 * 1)(0)
    nul = [None] * 21
    nul[2] = nul[5] = nul[6] = nul[13] = nul[19] = 0
    assert L.b3w_bao_verify_ranges_batch_device(*nul) == bad
    assert L.b3w_bao_verify_ranges_batch_device(None, one, 8, one, one, 1, 0, one, one, one, one, one, one, 1, one, one, one, one, None, 0, None) == bad
    assert one[0] == 0
    data, ob, root = _made(5 * 1024, 1)
    rw = np.array(root, dtype=np.uint32)
    st = np.full(3, FILL, dtype=np.uint8)
    rs, rf = np.full(2, -7, dtype=np.int32), np.full(2, 7, dtype=np.uint64)
    fc, nc = np.array([1, 4], dtype=np.uint64), np.array([2, 1], dtype=np.uint64)

    def call(d=data, o=ob, g=1, r=rw.ctypes.data, a=fc.ctypes.data, c=nc.ctypes.data, k=2, s=st.ctypes.data, x=rs.ctypes.data, y=rf.ctypes.data):
        return L.b3w_bao_verify_ranges(d, len(data), o, g, r, a, c, k, s, x, y)
    assert call(d=None) == bad and call(o=None) == bad and call(r=None) == bad and call(a=None) == bad and call(c=None) == bad and call(g=7) == bad
    assert call(s=None) == bad
    for first, count in ((5, 1), (4, 2), (0, 6), (6, 0), (1 << 63, 1 << 63)):  # past the file's 5 chunks
        fc[1], nc[1] = first, count
        assert call() == bad, (first, count)
    assert (st == FILL).all() and (rs == -7).all() and (rf == 7).all()         # a refused call writes nothing
    fc[1], nc[1] = 5, 0                                                        # an empty range at the end: 0 and none
    assert call() == 0
    assert st.tolist() == [0, 0, FILL] and rs.tolist() == [0, 0] and rf.tolist() == [NONE, NONE]
    st[:] = FILL
    assert call(x=None, y=None) == 0 and st.tolist() == [0, 0, FILL]           # (the per-range outputs are optional on the host)
    st[:] = FILL
    assert call(a=None, c=None, k=0) == 0 and (st == FILL).all()
    # a file of no bytes has one chunk
    e_ob, e_root = GR.group_outboard(b"", 0)
    e_rw, e_st = np.array(e_root, dtype=np.uint32), np.full(1, FILL, dtype=np.uint8)
    z, o1 = np.array([0], dtype=np.uint64), np.array([1], dtype=np.uint64)
    assert L.b3w_bao_verify_ranges(None, 0, e_ob, 0, e_rw.ctypes.data, z.ctypes.data, o1.ctypes.data, 1, e_st.ctypes.data, None, None) == 0 and e_st[0] == 0
    assert L.b3w_bao_verify_ranges(None, 0, e_ob, 0, e_rw.ctypes.data, o1.ctypes.data, o1.ctypes.data, 1, e_st.ctypes.data, None, None) == bad
    # the Python calls, before they touch a device
    for g in (-1, 7):
        with pytest.raises(m.B3WError, match="group_log"):
            m.bao.verify_ranges_host(data, ob, root, [0], [1], g)
        with pytest.raises(m.B3WError, match="group_log"):
            m.bao.verify_ranges_batch(None, None, [0], [10], None, None, [0], [0], [1], group_log=g)
    with pytest.raises(m.B3WError, match="size"):
        m.bao.verify_ranges_host(data, ob + bytes(64), root, [0], [1], 1)
    with pytest.raises(m.B3WError, match="2 first chunks and 1 chunk counts"):
        m.bao.verify_ranges_host(data, ob, root, [0, 1], [1], 1)
    with pytest.raises(m.B3WError):
        m.bao.verify_ranges_host(data, ob, root, [5], [1], 1)
