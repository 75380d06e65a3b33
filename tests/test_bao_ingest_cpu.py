"""Taking verified slices in without a GPU (b3w_bao_slice_ingest, bao.ingest_slice_host): the receiver's side of bao slices.  A slice that
verifies against the root puts the chunk's bytes at their place in the file, the stored nodes of its path at their pre-order places in
the outboard (all of them at g = 0, the part above the group at g > 0) and the header in front; one that does not writes nothing.  Held
against the restatements (tests/bao_ref.py, tests/bao_groups_ref.py) on every length of test_bao_cpu.LENGTHS at g in {0, 1, 4, 6}:
every chunk in shuffled order gives the file and the provider's outboard byte for byte, a subset writes exactly its own extents, nodes
and header, and every tampered slice has b3w_bao_slice_decode's status and leaves both buffers bit for bit as they were."""
import ctypes

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
import bao_ref as R
from test_bao_cpu import LENGTHS, _flip
from test_bao_slices_cpu import _made

BAD = 100
GS = [0, 1, 4, 6]
FILL = 0xEE
_GROUP_OBS = {}


def _want_outboard(length, g):
    """the provider's outboard of the test file of this length: the full one (g = 0) or the one over groups of 2^g chunks"""
    data, ob, root = _made(length)
    if g == 0:
        return ob
    if (length, g) not in _GROUP_OBS:
        got, group_root = GR.group_outboard(data, g)
        assert group_root == root
        _GROUP_OBS[(length, g)] = got
    return _GROUP_OBS[(length, g)]


def _stored_nodes(c, n, g):
    return R.path_nodes(c, n) if g == 0 else GR.group_path_nodes(c, n, g)


def _listed(n):
    """chunk 0, the last chunk and both sides of every split of the tree's top three levels"""
    out = {0, n - 1}

    def splits(lo, m, depth):
        if m > 1 and depth:
            k = R._split(m)
            out.update((lo + k - 1, lo + k))
            splits(lo, k, depth - 1)
            splits(lo + k, m - k, depth - 1)
    splits(0, n, 3)
    return sorted(out)


def _fresh(length, g):
    return bytearray([FILL]) * length, bytearray([FILL]) * GR.group_outboard_size(length, g)


@pytest.mark.parametrize("length", LENGTHS)
def test_every_chunk_in_shuffled_order_gives_the_file_and_the_providers_outboard(length):
    m = T.pkg()
    data, ob, root = _made(length)
    n = R.num_chunks(length)
    for g in GS:
        got_data, got_ob = _fresh(length, g)
        for c in np.random.default_rng(1000 * g + length).permutation(n):
            assert m.bao.ingest_slice_host(got_data, got_ob, length, int(c), root, R.slice_chunk(ob, data, int(c)), g) == 0, (length, g, c)
        assert bytes(got_data) == data, (length, g)
        assert bytes(got_ob) == _want_outboard(length, g), (length, g)


@pytest.mark.parametrize("length", LENGTHS)
def test_a_subset_writes_its_own_extents_nodes_and_header_and_nothing_else(length):
    m = T.pkg()
    data, ob, root = _made(length)
    n = R.num_chunks(length)
    chunks = _listed(n)
    for g in GS:
        want_ob = _want_outboard(length, g)
        got_data, got_ob = _fresh(length, g)
        exp_data, exp_ob = _fresh(length, g)
        exp_ob[:8] = want_ob[:8]
        for c in chunks:
            a, b = R.chunk_range(length, c)
            exp_data[a:b] = data[a:b]
            for i in _stored_nodes(c, n, g):
                exp_ob[8 + 64 * i:8 + 64 * i + 64] = want_ob[8 + 64 * i:8 + 64 * i + 64]
        for c in reversed(chunks):
            assert m.bao.ingest_slice_host(got_data, got_ob, length, c, root, R.slice_chunk(ob, data, c), g) == 0, (length, g, c)
        assert got_data == exp_data, (length, g)
        assert got_ob == exp_ob, (length, g)
        if len(chunks) < n:                                              # (what was not listed is still the fill)
            assert got_data != bytearray(data) and FILL in got_data


def _tampers(sl, c, n, length, root):
    """-> [(what, slice, root, the status the contract names)]: the header, the first and the last path node, a chunk byte, the root"""
    P = len(R.path_nodes(c, n))
    a, b = R.chunk_range(length, c)
    wrong_root = list(root)
    wrong_root[3] ^= 0x10000
    out = [("header", _flip(sl, c % 8), root, 3)]
    if P:
        out.append(("first node", _flip(sl, 8 + (c + 13) % 64), root, 2))
        out.append(("last node", _flip(sl, 8 + 64 * (P - 1) + (c + 5) % 64), root, 2))
    if b > a:
        out.append(("chunk byte", _flip(sl, 8 + 64 * P + (c * 7) % (b - a)), root, 1))
    out.append(("root", sl, wrong_root, 2 if P else 1))                   # one chunk: its ROOT-flagged output is what meets the root
    return out


@pytest.mark.parametrize("length", LENGTHS)
def test_a_tampered_slice_has_the_decoders_status_and_writes_nothing(length):
    m = T.pkg()
    data, ob, root = _made(length)
    n = R.num_chunks(length)
    for g in GS:
        got_data, got_ob = _fresh(length, g)
        first = _listed(n)[0]
        assert m.bao.ingest_slice_host(got_data, got_ob, length, first, root, R.slice_chunk(ob, data, first), g) == 0      # (buffers that are not all fill)
        before = bytes(got_data), bytes(got_ob)
        for c in _listed(n):
            for what, sl, rt, want in _tampers(R.slice_chunk(ob, data, c), c, n, length, root):
                st = m.bao.ingest_slice_host(got_data, got_ob, length, c, rt, sl, g)
                assert st == want == m.bao.decode_slice(sl, length, c, rt)[0], (length, g, c, what, st)
                assert (bytes(got_data), bytes(got_ob)) == before, (length, g, c, what)
    # precedence: the header over a node over the bytes
    c = n - 1
    P = len(R.path_nodes(c, n))
    a, b = R.chunk_range(length, c)
    if P and b > a:
        sl = R.slice_chunk(ob, data, c)
        got_data, got_ob = _fresh(length, 0)
        node_and_byte = _flip(_flip(sl, 8 + 64 * (P - 1) + 40), 8 + 64 * P)
        assert m.bao.ingest_slice_host(got_data, got_ob, length, c, root, _flip(node_and_byte, 0)) == 3
        assert m.bao.ingest_slice_host(got_data, got_ob, length, c, root, node_and_byte) == 2
        assert got_data == _fresh(length, 0)[0] and got_ob == _fresh(length, 0)[1]


def _call(L, sl, slice_len, length, chunk, root, g, data, ob, with_status=True):
    rw = np.array(root, dtype=np.uint32) if root is not None else None
    st = ctypes.c_int32(-7)
    d = (ctypes.c_uint8 * len(data)).from_buffer(data) if data is not None and len(data) else None
    o = (ctypes.c_uint8 * len(ob)).from_buffer(ob) if ob is not None else None
    rc = L.b3w_bao_slice_ingest(sl, slice_len, length, chunk, rw.ctypes.data if rw is not None else None, g, d, o, ctypes.byref(st) if with_status else None)
    return rc, st.value


def test_names_abi_and_refusals():
    m = T.pkg()
    L = m.lib()
    assert L.b3w_abi_version() == (1 << 16) | 4                            # new names only
    for name in ("b3w_bao_slice_ingest", "b3w_bao_slice_ingest_device"):
        assert name in m.EXPORTED_SYMBOLS and hasattr(L, name)
    assert callable(m.bao.ingest_slices) and callable(m.bao.ingest_slice_host)
    length = 5 * 1024 + 7
    data = _made(5 * 1024)[0] + bytes(range(7))
    ob, root = R.outboard(data)
    n = R.num_chunks(length)
    sl = R.slice_chunk(ob, data, 2)
    got_data, got_ob = _fresh(length, 0)
    clean = bytes(got_data), bytes(got_ob)
    assert _call(L, None, len(sl), length, 2, root, 0, got_data, got_ob)[0] == BAD
    assert _call(L, sl, len(sl), length, 2, None, 0, got_data, got_ob)[0] == BAD
    assert _call(L, sl, len(sl), length, 2, root, 0, got_data, got_ob, with_status=False)[0] == BAD
    assert _call(L, sl, len(sl), length, 2, root, 0, None, got_ob)[0] == BAD          # no place for the bytes of a file that has some
    assert _call(L, sl, len(sl), length, 2, root, 0, got_data, None)[0] == BAD
    assert _call(L, sl, len(sl), length, n, root, 0, got_data, got_ob)[0] == BAD      # no such chunk
    assert _call(L, sl, len(sl) - 1, length, 2, root, 0, got_data, got_ob)[0] == BAD  # a slice one byte short or long
    assert _call(L, sl + b"\0", len(sl) + 1, length, 2, root, 0, got_data, got_ob)[0] == BAD
    assert _call(L, sl, len(sl), length, 2, root, 7, got_data, got_ob)[0] == BAD      # group_log above the maximum
    assert (bytes(got_data), bytes(got_ob)) == clean
    assert _call(L, sl, len(sl), length, 2, root, 6, got_data, got_ob) == (0, 0)
    with pytest.raises(m.B3WError):
        m.bao.ingest_slice_host(got_data, got_ob, length, 2, root, sl, group_log=7)
    with pytest.raises(m.B3WError):
        m.bao.ingest_slice_host(got_data, got_ob, length, n, root, sl)
    with pytest.raises(m.B3WError):
        m.bao.ingest_slice_host(got_data, bytearray(8), length, 2, root, sl)          # an outboard of another size
    with pytest.raises(m.B3WError):
        m.bao.ingest_slice_host(bytes(got_data), got_ob, length, 2, root, sl)         # a buffer that cannot be written
    # an empty file: its slice is its header, and there is no place for bytes to give
    e_ob, e_root = R.outboard(b"")
    e_sl = R.slice_chunk(e_ob, b"", 0)
    assert e_sl == bytes(8)
    target = bytearray([FILL]) * 8
    assert _call(L, e_sl, 8, 0, 0, e_root, 0, None, target) == (0, 0) and bytes(target) == e_ob
    target = bytearray([FILL]) * 8
    wrong = list(e_root)
    wrong[0] ^= 1
    assert _call(L, e_sl, 8, 0, 0, wrong, 0, None, target) == (0, 1) and bytes(target) == bytes([FILL]) * 8
    # numpy buffers are taken as bytearrays are
    np_data, np_ob = np.full(length, FILL, dtype=np.uint8), np.full(len(ob), FILL, dtype=np.uint8)
    assert m.bao.ingest_slice_host(np_data, np_ob, length, 2, root, sl) == 0
    assert np_data[2048:3072].tobytes() == data[2048:3072] and (np_data[:2048] == FILL).all() and (np_data[3072:] == FILL).all()
    assert np_ob[:8].tobytes() == ob[:8]
