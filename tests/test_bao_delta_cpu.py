"""Outboard deltas without a GPU (b3w_bao_outboard_delta / _apply; bao.delta_host / apply_delta_host) against the restatement in
tests/bao_delta_ref.py.  The delta reads no file byte, so most outboards here are FABRICATED from made-up unit CVs (consistent with
their roots node by node, bao_delta_ref.fabricate); a last test takes real bytes and the restatement of the outboards.
Unit counts 1, 2, 3, 4, 5, 64, 65, 66, 129 (the bitmap's word edges are U - 1 = 64 and 65), 1 025 and 2 049; last chunks of 1 and
1 024 bytes; group_log 0, 4, 6; version b with no unit, the first, a middle, the last and every unit edited; b grown and shrunk across
one unit, a power of two and the tile, with a whole and with a ragged last unit; and the replica that holds nothing."""
import functools
import struct

import numpy as np
import pytest

import b3w_testlib as T
import bao_delta_ref as D
import bao_groups_ref as GR

K = 1024
BAD = 100
GS = [0, 4, 6]
COUNTS = [1, 2, 3, 4, 5, 64, 65, 66, 129, 1025, 2049]
RESIZED = [(1, 2), (2, 1), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (7, 6), (64, 65), (65, 64), (65, 66), (64, 128), (129, 65), (1024, 1025), (1025, 1024),
           (1025, 2049), (2049, 1025)]
WALL, FILL = 0xA5, 0xEE


def length(U, g, last, ragged=False):
    """bytes of a file of U units whose last chunk has `last` bytes; ragged: its last unit has one chunk"""
    n = ((U - 1) << g) + (1 if ragged else 1 << g)
    return (n - 1) * K + last


def _side(seeds, ln, g):
    ob, root = D.version(seeds, ln, g)
    return ob, ln, root


@functools.lru_cache(maxsize=None)
def cases(g):
    """-> [(name, side a or None, side b)], a side = (outboard bytes, length, root bytes)"""
    out = []
    for U in COUNTS:
        for last in (1, K):
            ln = length(U, g, last)
            a = _side(np.zeros(U, int), ln, g)
            for what, units in (("no unit", []), ("the first unit", [0]), ("a middle unit", [U // 2]), ("the last unit", [U - 1]), ("every unit", range(U))):
                seeds = np.zeros(U, int)
                seeds[list(units)] = 1
                out.append((f"{U} units, last of {last}: {what} edited", a, _side(seeds, ln, g)))
        out.append((f"{U} units against nothing", None, _side(np.zeros(U, int), length(U, g, K), g)))
    for i, (ua, ub) in enumerate(RESIZED):
        for ragged_a, ragged_b in ((False, False), (True, False), (False, True)) if g else ((False, False),):
            la, lb = length(ua, g, 1 if i % 2 else K, ragged_a), length(ub, g, K if i % 2 else 1, ragged_b)
            a = _side(np.zeros(ua, int), la, g)
            out.append((f"{ua} -> {ub} units (ragged {ragged_a}, {ragged_b})", a, _side(np.zeros(ub, int), lb, g)))
            if min(ua, ub) > 2:
                seeds = np.zeros(ub, int)
                seeds[1] = 1
                out.append((f"{ua} -> {ub} units (ragged {ragged_a}, {ragged_b}), unit 1 edited", a, _side(seeds, lb, g)))
    return out


def _root(root):
    return np.frombuffer(bytes(root), dtype=np.uint32).copy()


def delta_c(m, a, b, g, capacity=None):
    """the C provider into a walled blob of `capacity` bytes -> (the blob, k as found)"""
    cap = D.bound(b[1], g) if capacity is None else capacity
    buf = np.full(cap + 32, WALL, dtype=np.uint8)
    buf[16:16 + cap] = FILL
    k = np.zeros(1, dtype=np.uint64)
    ra, rb = (_root(a[2]) if a else None), _root(b[2])
    rc = m.lib().b3w_bao_outboard_delta(a[0] if a else None, a[1] if a else 0, ra.ctypes.data if a else None, b[0], b[1], rb.ctypes.data, g, buf[16:].ctypes.data, cap,
                                        k.ctypes.data)
    assert rc == 0
    assert (buf[:16] == WALL).all() and (buf[16 + cap:] == WALL).all(), "a byte outside the blob's extent was written"
    return buf[16:16 + cap].tobytes(), int(k[0])


def apply_c(m, a, len_b, root_b, g, blob, into=None):
    """the C replica into a walled outboard (into: the bytes that lie there before, else 0xEE) -> (status, first bad node, the bytes after)"""
    size = GR.group_outboard_size(len_b, g)
    buf = np.full(size + 32, WALL, dtype=np.uint8)
    buf[16:16 + size] = FILL if into is None else np.frombuffer(into, dtype=np.uint8)
    status, bad = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint64)
    ra, rb = (_root(a[2]) if a else None), _root(root_b)
    src = np.frombuffer(blob, dtype=np.uint8).copy()                             # (an exact-size heap copy)
    rc = m.lib().b3w_bao_outboard_delta_apply(a[0] if a else None, a[1] if a else 0, ra.ctypes.data if a else None, len_b, rb.ctypes.data, g, src.ctypes.data, src.size,
                                              buf[16:].ctypes.data, status.ctypes.data, bad.ctypes.data)
    assert rc == 0
    assert (buf[:16] == WALL).all() and (buf[16 + size:] == WALL).all(), "a byte outside the output outboard was written"
    return int(status[0]), -1 if bad[0] == np.uint64(2 ** 64 - 1) else int(bad[0]), buf[16:16 + size].tobytes()


@pytest.mark.parametrize("g", GS)
def test_the_host_mirrors_are_the_restatement_and_the_round_trip_gives_bs_outboard(g):
    m = T.pkg()
    seen = {"nothing sent": 0, "everything sent": 0, "some nodes sent": 0, "copied across positions": 0, "a ragged unit decides": 0}
    for name, a, b in cases(g):
        want = D.make_blob(*(a or (None, 0, None)), *b, g)
        got, k = delta_c(m, a, b, g)
        assert k == struct.unpack("<Q", want[8:16])[0], name
        assert got[:len(want)] == want, (name, "not the restatement's blob")
        assert got[len(want):] == bytes([FILL]) * (len(got) - len(want)), (name, "written behind the last node")
        assert len(got) == m.bao.delta_bound(b[1], g) == D.bound(b[1], g)
        status, bad, out = apply_c(m, a, b[1], b[2], g, want)
        assert (status, bad) == (0, -1) and out == b[0], (name, status, bad)
        assert D.apply_blob(*(a or (None, 0, None)), b[1], b[2], g, want) == (0, -1, b[0]), name
        U = D.units(b[1], g)
        seen["nothing sent"] += k == 0
        seen["everything sent"] += U > 1 and k == U - 1
        seen["some nodes sent"] += 0 < k < U - 1
        if a and 0 < k < U - 1 and D.units(a[1], g) != U:
            seen["copied across positions"] += 1
        seen["a ragged unit decides"] += g == 0 or "ragged True" in name
    assert all(seen.values()), seen
    # the wrappers: one case of each kind
    for name, a, b in cases(g)[3::41]:
        blob, k = m.bao.delta_host(*(a or (None, 0, None)), *b, g)
        used = 16 + 8 * D.words(D.units(b[1], g)) + 64 * k
        assert (blob[:used], k) == (D.make_blob(*(a or (None, 0, None)), *b, g), k) and blob[used:] == bytes(len(blob) - used), name
        assert m.bao.apply_delta_host(*(a or (None, 0, None)), b[1], b[2], blob[:used], g) == (0, -1, b[0]), name


@pytest.mark.parametrize("g", [0, 4])
def test_equal_lengths_in_place(g):
    """the output may BE a's outboard where U_a = U_b: only present nodes are written"""
    m = T.pkg()
    for name, a, b in cases(g):
        if a and D.units(a[1], g) == D.units(b[1], g) and a[1] == b[1]:
            blob = D.make_blob(*a, *b, g)
            buf = np.frombuffer(a[0], dtype=np.uint8).copy()
            status, bad = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint64)
            ra, rb = _root(a[2]), _root(b[2])
            assert m.lib().b3w_bao_outboard_delta_apply(buf.ctypes.data, a[1], ra.ctypes.data, b[1], rb.ctypes.data, g, blob, len(blob), buf.ctypes.data,
                                                        status.ctypes.data, bad.ctypes.data) == 0
            assert status[0] == 0 and buf.tobytes() == b[0], name


# ---- tampering ----------------------------------------------------------------------------------------------------------------------
def tamper_base(g):
    """66 units (65 nodes: two bitmap words, 63 pad bits), units 0, 20 and 65 edited -> (a, b, the blob, {span: node index})"""
    U = 66
    ln = length(U, g, 500)
    seeds = np.zeros(U, int)
    seeds[[0, 20, 65]] = 1
    a, b = _side(np.zeros(U, int), ln, g), _side(seeds, ln, g)
    return a, b, D.make_blob(*a, *b, g), D.tree(U)[1]


def _bits(blob, W):
    return np.unpackbits(np.frombuffer(blob[16:16 + 8 * W], np.uint8), bitorder="little").astype(bool)


def _rebuild(len_b, bits, nodes):
    """a blob from a bitmap (bools, pad included) and {node index: 64 bytes}"""
    return struct.pack("<QQ", len_b, len(nodes)) + np.packbits(bits.astype(np.uint8), bitorder="little").tobytes() + b"".join(nodes[p] for p in sorted(nodes))


@functools.lru_cache(maxsize=None)
def tampers(g):
    """-> [(name, side a, blob, status, first bad node)]: ordinary inputs that must end in that status (0: b's outboard)"""
    a, b, blob, at = tamper_base(g)
    U, W = 66, 2
    bits = _bits(blob, W)
    k = int(bits.sum())
    nodes = {int(p): blob[16 + 8 * W + 64 * r:16 + 8 * W + 64 * r + 64] for r, p in enumerate(np.flatnonzero(bits))}
    mid, leafp, absent, spare = at[(16, 16)], at[(20, 2)], at[(32, 32)], at[(40, 8)]
    assert bits[[0, mid, leafp]].all() and not bits[absent] and not bits[spare] and k == 12
    out = []

    def flip(data, where):
        return data[:where] + bytes([data[where] ^ 0x10]) + data[where + 1:]

    def node_at(p):
        return 16 + 8 * W + 64 * sorted(nodes).index(p)
    out.append(("the header's length", a, struct.pack("<Q", b[1] + 1) + blob[8:], D.MALFORMED, 0))
    out.append(("the header's k one more", a, blob[:8] + struct.pack("<Q", k + 1) + blob[16:], D.MALFORMED, 0))
    out.append(("the header's k one less", a, blob[:8] + struct.pack("<Q", k - 1) + blob[16:], D.MALFORMED, 0))
    out.append(("the header's k huge", a, blob[:8] + struct.pack("<Q", 2 ** 63) + blob[16:], D.MALFORMED, 0))
    padded, more = bits.copy(), dict(nodes)
    padded[U - 1 + 3] = True
    more[U - 1 + 3] = bytes(64)
    out.append(("a pad bit, counted and with a node", a, _rebuild(b[1], padded, more), D.MALFORMED, U - 1 + 3))
    out.append(("a bitmap bit cleared", a, blob[:16 + mid // 8] + bytes([blob[16 + mid // 8] & ~(1 << (mid % 8)) & 0xFF]) + blob[17 + mid // 8:], D.MALFORMED, 0))
    out.append(("a bitmap bit set", a, blob[:16 + absent // 8] + bytes([blob[16 + absent // 8] | 1 << (absent % 8)]) + blob[17 + absent // 8:], D.MALFORMED, 0))
    extra, garbage = bits.copy(), dict(nodes)
    extra[absent] = True
    garbage[absent] = bytes(range(64))
    out.append(("a bit set and a made-up node put in", a, _rebuild(b[1], extra, garbage), D.BAD_HASH, absent))
    true = dict(nodes)
    true[absent] = D.node(a[0], absent)
    out.append(("a bit set and a's own node put in: a larger delta, still b's", a, _rebuild(b[1], extra, true), 0, -1))
    out.append(("a byte of the root node", a, flip(blob, node_at(0) + 40), D.BAD_HASH, 0))
    out.append(("a byte of a middle node", a, flip(blob, node_at(mid) + 3), D.BAD_HASH, mid))
    out.append(("a byte of a leaf parent", a, flip(blob, node_at(leafp) + 63), D.BAD_HASH, leafp))
    for name, p in (("a middle node dropped", mid), ("a leaf parent dropped", leafp)):
        fewer, rest = bits.copy(), dict(nodes)
        fewer[p] = False
        del rest[p]
        out.append((name, a, _rebuild(b[1], fewer, rest), D.NOT_HELD, p))
    none, root_only = bits.copy(), {}
    none[:] = False
    out.append(("the root dropped with everything below", a, _rebuild(b[1], none, root_only), D.MALFORMED, 0))
    orphan = bits.copy()
    orphan[0] = False
    out.append(("the root dropped alone", a, _rebuild(b[1], orphan, {p: n for p, n in nodes.items() if p}), D.MALFORMED, 0))
    out.append(("the last node cut off", a, blob[:-64], D.MALFORMED, 0))
    out.append(("the last eight bytes cut off", a, blob[:-8], D.MALFORMED, 0))
    seeds = np.zeros(U, int)
    seeds[40] = 2
    out.append(("an absent subtree that a holds otherwise", _side(seeds, a[1], g), blob, D.NOT_HELD, absent))
    shorter = _side(np.zeros(40, int), length(40, g, 500), g)                     # (a of 40 units holds (0, 32) and below, nothing to the right)
    out.append(("an absent subtree that a does not have", shorter, blob, D.NOT_HELD, absent))
    out.append(("a replica that holds nothing", None, blob, D.NOT_HELD, at[(2, 2)]))
    return out


@pytest.mark.parametrize("g", GS)
def test_every_tampered_blob_ends_in_its_status_and_an_untouched_output(g):
    m = T.pkg()
    _, b, blob, _ = tamper_base(g)
    assert apply_c(m, tamper_base(g)[0], b[1], b[2], g, blob)[:2] == (0, -1)
    for name, a, bad_blob, status, bad in tampers(g):
        ref = D.apply_blob(*(a or (None, 0, None)), b[1], b[2], g, bad_blob)
        assert ref[:2] == (status, bad), (name, "the restatement", ref[:2])
        got = apply_c(m, a, b[1], b[2], g, bad_blob)
        assert got[:2] == (status, bad), (name, got[:2])
        assert got[2] == (b[0] if status == 0 else bytes([FILL]) * len(b[0])), (name, "the output")
        assert m.bao.apply_delta_host(*(a or (None, 0, None)), b[1], b[2], bad_blob, g)[:2] == (status, bad), name


def test_a_wrong_root_and_a_one_unit_file():
    m = T.pkg()
    a, b, blob, _ = tamper_base(0)
    other = bytes(x ^ 1 for x in b[2])
    assert apply_c(m, a, b[1], other, 0, blob)[:2] == D.apply_blob(*a, b[1], other, 0, blob)[:2] == (D.BAD_HASH, 0)
    one = _side(np.zeros(1, int), 700, 0)
    assert delta_c(m, None, one, 0) == (struct.pack("<QQ", 700, 0), 0)
    assert apply_c(m, None, 700, one[2], 0, struct.pack("<QQ", 700, 0)) == (0, -1, struct.pack("<Q", 700))
    for bad_blob in (struct.pack("<QQ", 701, 0), struct.pack("<QQ", 700, 1), struct.pack("<QQ", 700, 1) + bytes(64)):      # (the root present although U_b = 1)
        assert apply_c(m, None, 700, one[2], 0, bad_blob)[:2] == D.apply_blob(None, 0, None, 700, one[2], 0, bad_blob)[:2] == (D.MALFORMED, 0)


@pytest.mark.parametrize("g", [0, 6])
def test_the_capacity_rule(g):
    """k is reported above the capacity, the nodes that fit are written and nothing beyond the extent"""
    m = T.pkg()
    a, b, blob, _ = tamper_base(g)
    head, k = 16 + 8 * 2, 12
    for cap in (head, head + 64, head + 64 * (k - 1), head + 64 * (k - 1) + 56, head + 64 * k, head + 64 * k + 8):
        got, found = delta_c(m, a, b, g, cap)
        fit = min(k, (cap - head) // 64)
        assert found == k and got[:head + 64 * fit] == blob[:head + 64 * fit] and got[head + 64 * fit:] == bytes([FILL]) * (cap - head - 64 * fit), cap
        want = (0, -1) if fit == k else (D.MALFORMED, 0)
        assert apply_c(m, a, b[1], b[2], g, got)[:2] == want, cap


def test_refusals():
    m = T.pkg()
    L = m.lib()
    a, b, blob, _ = tamper_base(0)
    ra, rb = _root(a[2]), _root(b[2])
    buf, k = np.full(len(blob) + 8, FILL, dtype=np.uint8), np.zeros(1, dtype=np.uint64)
    out, status, bad = np.full(len(b[0]), FILL, dtype=np.uint8), np.full(1, 77, dtype=np.int32), np.full(1, 77, dtype=np.uint64)
    good = (a[0], a[1], ra.ctypes.data, b[0], b[1], rb.ctypes.data, 0, buf.ctypes.data, len(blob), k.ctypes.data)
    assert L.b3w_bao_outboard_delta(*good) == 0 and buf[:len(blob)].tobytes() == blob
    buf[:] = FILL
    huge = ((1 << 30) + 1) * K
    for i, v in ((2, None), (3, None), (5, None), (6, 7), (7, None), (8, 16 + 8 * 2 - 8), (9, None), (1, huge), (4, huge)):
        args = list(good)
        args[i] = v
        assert L.b3w_bao_outboard_delta(*args) == BAD, i
        assert (buf == FILL).all()
    good = (a[0], a[1], ra.ctypes.data, b[1], rb.ctypes.data, 0, blob, len(blob), out.ctypes.data, status.ctypes.data, bad.ctypes.data)
    for i, v in ((2, None), (4, None), (5, 7), (6, None), (7, 16 + 8 * 2 - 1), (8, None), (9, None), (10, None), (1, huge), (3, huge)):
        args = list(good)
        args[i] = v
        assert L.b3w_bao_outboard_delta_apply(*args) == BAD, i
        assert (out == FILL).all() and status[0] == 77 and bad[0] == 77
    assert L.b3w_bao_outboard_delta_apply(*good) == 0 and out.tobytes() == b[0] and status[0] == 0
    assert L.b3w_bao_outboard_delta_bound(1, 7) == 0 and m.bao.delta_bound(1) == 16
    with pytest.raises(m.B3WError):
        m.bao.delta_host(*a, *b, 7)
    with pytest.raises(m.B3WError):
        m.bao.delta_host(a[0], a[1] + K, a[2], *b)                                # (an outboard that is not of that length)
    with pytest.raises(m.B3WError):
        m.bao.apply_delta_host(*a, b[1], b[2][:28], blob)
    first = m.bao.delta_layout([b[1], 700, a[1]], 0, [2, 1, 1, 0])
    assert first.tolist() == np.cumsum([0, D.bound(a[1], 0), 16, 16, D.bound(b[1], 0)]).tolist()
    for name in ("b3w_bao_outboard_delta_bound", "b3w_bao_outboard_delta_layout", "b3w_bao_outboard_delta_scratch_bytes", "b3w_bao_outboard_delta_device",
                 "b3w_bao_outboard_delta_apply_device", "b3w_bao_outboard_delta", "b3w_bao_outboard_delta_apply"):
        assert name in m.EXPORTED_SYMBOLS and hasattr(L, name)


def test_the_numpy_restatement_is_the_plain_one():
    """nodes_np / same_np (the GPU test's yardstick at 2^20 units) against the walk over node_spans"""
    rng = np.random.default_rng(7)
    for U in (2, 3, 5, 64, 65, 66, 129, 1025, 1029):
        lo, cnt, parent, side = D.nodes_np(U)
        spans, _, up, _ = D.tree(U)
        assert list(zip(lo.tolist(), cnt.tolist())) == spans
        assert [(int(p), int(s)) for p, s in zip(parent[1:], side[1:])] == up[1:]
    for na, nb, g in ((1025, 1025, 0), (1025, 2049, 0), (2049, 1025, 0), (70, 200, 0), (1029 * 16 - 3, 1029 * 16, 4), (129 * 64, 129 * 64 - 70, 6)):
        Ua, Ub = GR.num_groups(na, g), GR.num_groups(nb, g)
        ob_a = rng.integers(0, 256, 8 + 64 * (Ua - 1), dtype=np.uint8)
        ob_b = rng.integers(0, 256, 8 + 64 * (Ub - 1), dtype=np.uint8)
        index_a, up_a, up_b = D.tree(Ua)[1], D.tree(Ua)[2], D.tree(Ub)[2]
        for p, span in enumerate(D.tree(Ub)[0]):                                 # six stored halves in ten are a's wherever a has the span
            pa = index_a.get(span)
            if p and pa and rng.random() < 0.6:
                (qa, sa), (qb, sb) = up_a[pa], up_b[p]
                ob_b[8 + 64 * qb + 32 * sb:8 + 64 * qb + 32 * sb + 32] = ob_a[8 + 64 * qa + 32 * sa:8 + 64 * qa + 32 * sa + 32]
        want = D.same_nodes(ob_a.tobytes(), na * K, bytes(32), ob_b.tobytes(), nb * K, bytes(32), g)
        got = D.same_np(ob_a, na, ob_b, nb, g, roots_equal=True)
        assert (got == want).all(), (na, nb, g)
        assert want.any() and not want.all()


def test_real_bytes_against_the_restatement_of_the_outboards():
    """apply(delta(a, b)) onto a's outboard is bao_groups_ref.group_outboard(b) byte for byte, from bytes this time"""
    m = T.pkg()
    rng = np.random.default_rng(11)
    for g, n_a, n_b, last in ((0, 5, 5, 1), (0, 5, 5, K), (0, 3, 5, 17), (0, 5, 2, K), (0, 1, 1, 1), (4, 48, 48, 9), (4, 33, 48, K)):
        data_a = rng.integers(0, 256, (n_a - 1) * K + last, dtype=np.uint8)
        data_b = rng.integers(0, 256, (n_b - 1) * K + last, dtype=np.uint8)
        keep = min(data_a.size, data_b.size)
        data_b[:keep] = data_a[:keep]
        data_b[min(K + 5, data_b.size - 1)] ^= 4                                    # (chunk 1, or the only chunk)
        sides = []
        for data in (data_a, data_b):
            ob, root = GR.group_outboard(data.tobytes(), g)
            sides.append((ob, data.size, D.R._cv_bytes(root)))
        a, b = sides
        blob, k = delta_c(m, a, b, g)
        want = D.make_blob(*a, *b, g)
        assert blob[:len(want)] == want
        assert apply_c(m, a, b[1], b[2], g, want) == (0, -1, b[0]), (g, n_a, n_b)
        assert (k >= 1) == (D.units(b[1], g) > 1)
