"""Whole-file verification without a GPU: the library's host calls (b3w_bao_verify_layout, b3w_bao_verify_scratch_bytes,
b3w_bao_verify) against the plain-Python restatement (tests/bao_verify_ref.py) on untouched and tampered files, outboards and
roots; the locality claims asserted by counting (a bad chunk marks its unit alone, a bad node exactly the units below it, a wrong
root every unit); and the restatement tied to bao_ref.decode_slice, which is pinned to the reference-made transcripts."""
import ctypes
import struct

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
import bao_ref as R
import bao_verify_ref as V
import test_bao_cpu as C
import test_bao_groups_cpu as CG
from test_bao_slices_cpu import _ref_accepts

GS = (0, 1, 4, 6)
NONE = (1 << 64) - 1
_CACHE = {}


def _made(length, g):
    """-> (data, group outboard of g, root words) of the test file of this length"""
    if (length, g) not in _CACHE:
        data = C._data(length)
        _CACHE[(length, g)] = (data,) + GR.group_outboard(data, g)
    return _CACHE[(length, g)]


def _host(L, data, ob, root, g):
    """b3w_bao_verify -> (statuses, file status, first bad)"""
    n_units = V.num_units(len(data), g)
    rw = np.array(root, dtype=np.uint32)
    st = np.full(n_units + 1, 0xEE, dtype=np.uint8)                        # (one past the end: must stay untouched)
    fs, fb = ctypes.c_int32(-7), ctypes.c_uint64(5)
    assert L.b3w_bao_verify(data, len(data), ob, g, rw.ctypes.data, st.ctypes.data, ctypes.byref(fs), ctypes.byref(fb)) == 0
    assert st[n_units] == 0xEE
    return [int(x) for x in st[:n_units]], fs.value, fb.value


def _between(n_units):
    """a stored node that is neither the root nor a lowest one, or None"""
    for i, (_, m) in enumerate(GR.node_spans(n_units)):
        if i and m > 2:
            return i
    return None


def _cases(length, g):
    """(name, data, outboard, root, the status every unit must have: {unit: status} over a default of 0) for one file"""
    data, ob, root = _made(length, g)
    n, nu = R.num_chunks(length), V.num_units(length, g)
    out = [("untouched", data, ob, root, {})]
    if length:                                                             # a byte of the first, the last and a middle chunk, in one go
        bad, hit = data, {}
        for c in sorted({0, n // 2, n - 1}):
            a, b = R.chunk_range(length, c)
            bad = C._flip(bad, a + (c * 7) % (b - a))
            hit[c >> g] = 1
        out.append(("chunks", bad, ob, root, hit))
    spans = GR.node_spans(nu)
    for name, i in (("root node", 0 if nu > 1 else None), ("lowest node", nu - 2 if nu > 1 else None), ("node between", _between(nu))):
        if i is None:
            continue
        first, m = spans[i]
        if name == "lowest node":
            assert m == 2
        for half in (0, 1):                                                # either half: exactly the units below the node
            out.append((f"{name} half {half}", data, C._flip(ob, 8 + 64 * i + 32 * half + (5 * i + length) % 32), root,
                        {u: 2 for u in range(first, first + m)}))
    wrong = list(root)
    wrong[3] ^= 0x10000
    out.append(("wrong root", data, ob, wrong, {u: 2 if nu > 1 else 1 for u in range(nu)}))
    out.append(("header", data, struct.pack("<Q", length + 1) + ob[8:], root, {u: 3 for u in range(nu)}))
    return out


def test_layout_and_scratch_equal_the_restatement():
    m = T.pkg()
    L = m.lib()
    lens = np.array(CG.LENGTHS, dtype=np.uint64)
    for g in range(7):
        uf = np.full(lens.size + 1, 77, dtype=np.uint64)
        total = L.b3w_bao_verify_layout(lens.ctypes.data, lens.size, g, uf.ctypes.data)
        want = V.layout(lens, g)
        assert list(uf) == want and total == want[-1], g
        assert list(m.bao.verify_layout(lens, g)) == want
        for length in CG.LENGTHS:
            assert V.num_units(length, g) == max(1, -(-R.num_chunks(length) // (1 << g)))
    assert list(m.bao.verify_layout(lens)) == V.layout(lens, 0)
    # the scratch: nothing for files of one tile, a CV and a flag per tile (and per 1 024 tiles) beyond
    assert L.b3w_bao_verify_scratch_bytes(lens.ctypes.data, lens.size) == 0
    big = np.array([0, 4096, 1 << 20, (1 << 20) + 1, 5 << 20, (1 << 30) + 5, 1 << 30, 70000, (3 << 30) + 12345], dtype=np.uint64)
    assert V.scratch_items(big) == 2 + 5 + (1025 + 2) + 1024 + (3073 + 4)
    for k in range(1, big.size + 1):
        items = V.scratch_items(big[:k])
        assert L.b3w_bao_verify_scratch_bytes(big.ctypes.data, k) == (36 * items + 15) // 16 * 16, k
    none = np.zeros(1, dtype=np.uint64)
    assert L.b3w_bao_verify_layout(None, 0, 3, none.ctypes.data) == 0 == int(none[0])


def test_refusals():
    m = T.pkg()
    L = m.lib()
    bad = m.B3W_E_BAD_ARGUMENT
    lens = np.array([5000, 70000], dtype=np.uint64)
    uf = np.zeros(3, dtype=np.uint64)
    assert L.b3w_bao_verify_layout(lens.ctypes.data, 2, 7, uf.ctypes.data) == 0                # a group_log above B3W_BAO_MAX_GROUP_LOG
    assert L.b3w_bao_verify_layout(lens.ctypes.data, 2, 2, None) == 0
    assert L.b3w_bao_verify_layout(None, 2, 2, uf.ctypes.data) == 0
    assert L.b3w_bao_verify_scratch_bytes(None, 2) == 0
    with pytest.raises(m.B3WError):
        m.bao.verify_layout(lens, 7)
    data, ob, root = _made(5 * 1024, 1)
    rw = np.array(root, dtype=np.uint32)
    st = np.zeros(8, dtype=np.uint8)
    assert L.b3w_bao_verify(data, len(data), ob, 7, rw.ctypes.data, st.ctypes.data, None, None) == bad
    assert L.b3w_bao_verify(None, len(data), ob, 1, rw.ctypes.data, st.ctypes.data, None, None) == bad
    assert L.b3w_bao_verify(data, len(data), None, 1, rw.ctypes.data, st.ctypes.data, None, None) == bad
    assert L.b3w_bao_verify(data, len(data), ob, 1, None, st.ctypes.data, None, None) == bad
    assert L.b3w_bao_verify(data, len(data), ob, 1, rw.ctypes.data, None, None, None) == bad
    assert L.b3w_bao_verify(data, len(data), ob, 1, rw.ctypes.data, st.ctypes.data, None, None) == 0 and not st.any()   # (the summaries are optional)
    with pytest.raises(m.B3WError):
        m.bao.verify_host(data, ob, root, 7)
    with pytest.raises(m.B3WError):
        m.bao.verify_host(data, ob + bytes(64), root, 1)
    # the device call refuses without a context, before it looks at anything else
    assert L.b3w_bao_verify_batch_device(None, None, None, None, 0, 0, None, None, None, None, None, None, 0, None) == bad


@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("length", C.LENGTHS)
def test_host_verify_equals_the_restatement_and_tampering_stays_local(length, g):
    m = T.pkg()
    L = m.lib()
    nu = V.num_units(length, g)
    for name, data, ob, root, hit in _cases(length, g):
        want = [hit.get(u, 0) for u in range(nu)]
        got, fs, fb = _host(L, data, ob, root, g)
        assert got == V.verify(data, ob, root, length, g), (length, g, name)
        # locality, by counting: the units the tampering names have its status and no other unit has any
        assert got == want, (length, g, name)
        for code in (1, 2, 3):
            assert got.count(code) == sum(1 for s in hit.values() if s == code), (length, g, name, code)
        assert (fs, fb) == V.summary(want) == (max(want), min(hit) if hit else NONE), (length, g, name)
        st, fs2, fb2 = m.bao.verify_host(data, ob, root, g)
        assert (list(st), fs2, fb2) == (want, fs, fb)


@pytest.mark.parametrize("length", C.LENGTHS)
def test_precedence_header_then_node_then_bytes(length):
    L = T.pkg().lib()
    for g in GS:
        data, ob, root = _made(length, g)
        nu = V.num_units(length, g)
        if nu < 2:
            continue
        bad_data = C._flip(data, 0)
        bad_ob = C._flip(ob, 8 + 64 * (nu - 2) + 40)                       # a lowest node: two units; where unit 0 is one of them 2 wins
        first, _ = GR.node_spans(nu)[nu - 2]
        want = [1] + [0] * (nu - 1)
        want[first:first + 2] = [2, 2]
        got = _host(L, bad_data, bad_ob, root, g)
        assert got[0] == want == V.verify(bad_data, bad_ob, root, length, g), (length, g)
        assert got[1:] == (2, 0)
        worst = struct.pack("<Q", length ^ 1) + bad_ob[8:]
        assert _host(L, bad_data, worst, root, g) == ([3] * nu, 3, 0)


def _slice(ob, data, c, length):
    """the slice of chunk c cut from a (maybe tampered) full outboard by a caller who knows the file's length"""
    a, b = R.chunk_range(length, c)
    return ob[:8] + b"".join(ob[8 + 64 * i:8 + 64 * i + 64] for i in R.path_nodes(c, R.num_chunks(length))) + bytes(data[a:b])


@pytest.mark.parametrize("length", C.LENGTHS)
def test_restatement_accepts_exactly_the_chunks_the_slice_decoder_accepts(length):
    """g = 0: a chunk's status is 0 exactly where bao_ref.decode_slice (with the header comparison of a caller who knows the length)
    accepts the slice of that chunk cut from the same tampered file, outboard and root"""
    for name, data, ob, root, _ in _cases(length, 0):
        st = V.verify(data, ob, root, length, 0)
        for c in range(R.num_chunks(length)):
            assert (st[c] == 0) == _ref_accepts(_slice(ob, data, c, length), c, root, length), (length, name, c)
