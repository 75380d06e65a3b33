"""The outboard diff without a GPU (b3w_bao_outboard_diff; bao.diff_host) against the restatement in tests/bao_diff_ref.py and against
what the bytes say.  Files of 1, 2, 3, 63, 64, 65, 1 023, 1 024, 1 025 and 2 049 chunks, each with a last chunk of 1 byte and of 1 024
bytes (and the empty file); version b with no edit and with an edit in the first, a middle and the last chunk; b grown and b shrunk,
to and from one chunk, across a unit boundary of every unit size and across the tile of 1 024 chunks; (group_log_a, group_log_b) over
{0, 1, 4, 6}^2, which makes the files of at most 2^G chunks the root case and 64 against 65 chunks a whole file on one side only.  The
outboards are the host's own (resize_host from nothing), which test_bao_resize_cpu holds against the restatement of the outboards."""
import functools

import numpy as np
import pytest

import b3w_testlib as T
import bao_diff_ref as D
import bao_have_ref as H

K = 1024
BAD = 100
GS = [0, 1, 4, 6]
COUNTS = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049]
GUARD = 0xA5A5A5A5A5A5A5A5
# (chunks of a, chunks of b): b = a's bytes cut off or continued
RESIZED = [(1, 2), (2, 1), (1, 3), (3, 1), (1, 65), (65, 1), (2, 3), (3, 2), (16, 17), (17, 16), (17, 18), (18, 17), (32, 33), (63, 64), (64, 65), (65, 64),
           (64, 128), (129, 65), (1023, 1025), (1025, 1023), (1024, 1025), (1025, 1024), (1025, 2049), (2049, 1025), (1023, 2049)]


def _bytes(n, last, seed):
    """a file of n chunks whose last chunk has `last` bytes"""
    return np.random.default_rng(seed).integers(0, 256, (n - 1) * K + last, dtype=np.uint8)


def _edited(data, chunk):
    out = data.copy()
    at = min(chunk * K + 7, out.size - 1)
    out[at] ^= 0x20
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """-> [(name, a's bytes, b's bytes)], numpy uint8; a version that takes part in several pairs is one object"""
    out = []
    for n in COUNTS:
        for last in (1, K):
            a = _bytes(n, last, [n, last])
            out.append((f"{n} chunks, last of {last}: no edit", a, a.copy()))
            for what, c in (("first", 0), ("middle", n // 2), ("last", n - 1)):
                out.append((f"{n} chunks, last of {last}: the {what} chunk edited", a, _edited(a, c)))
    empty = np.zeros(0, dtype=np.uint8)
    out.append(("empty against empty", empty, empty.copy()))
    out.append(("empty against one byte", empty, _bytes(1, 1, 5)))
    out.append(("one byte against empty", _bytes(1, 1, 5), empty))
    for i, (na, nb) in enumerate(RESIZED):
        for last in (1, K):
            longer = _bytes(max(na, nb), last, [1000 + i, last])
            shorter = longer[:min(na, nb) * K - (K - last if i % 2 else 0)]       # (in every second pair the shorter one ends on a chunk boundary)
            a, b = (longer, shorter) if na > nb else (shorter, longer)
            out.append((f"{na} -> {nb} chunks, last of {last}", a, b))
            if min(na, nb) > 1:
                out.append((f"{na} -> {nb} chunks, last of {last}, chunk 1 edited", a, _edited(b, 1)))
    return out


_OBS, _TRUTH = {}, {}


def outboard_of(m, data, g):
    """the host's outboard and root of these bytes at group_log g, made once per version"""
    key = (id(data), g)
    if key not in _OBS:
        ob, root = m.bao.resize_host(data.tobytes(), bytes(8), 0, g)
        _OBS[key] = (data, ob, root.copy())
    return _OBS[key][1:]


def diff_c(m, ob_a, len_a, root_a, ga, ob_b, len_b, root_b, gb):
    """the C call into guarded words -> the pair's words after the guards were checked"""
    words = H.words(H.num_chunks(len_b))
    buf = np.full(words + 4, GUARD, dtype=np.uint64)
    ra, rb = np.ascontiguousarray(root_a, dtype=np.uint32), np.ascontiguousarray(root_b, dtype=np.uint32)
    rc = m.lib().b3w_bao_outboard_diff(ob_a, len_a, ra.ctypes.data, ga, ob_b, len_b, rb.ctypes.data, gb, buf[2:].ctypes.data)
    assert rc == 0
    assert (buf[:2] == GUARD).all() and (buf[2 + words:] == GUARD).all(), "a word outside the pair was written"
    return buf[2:2 + words].copy()


@pytest.mark.parametrize("ga", GS)
@pytest.mark.parametrize("gb", GS)
def test_the_host_call_is_the_restatement_and_what_the_bytes_say(ga, gb):
    m = T.pkg()
    G = max(ga, gb)
    seen = {"root case": 0, "whole on one side": 0, "ragged last unit": 0, "some same, some not": 0}
    for name, a, b in cases():
        ob_a, root_a = outboard_of(m, a, ga)
        ob_b, root_b = outboard_of(m, b, gb)
        nb = H.num_chunks(b.size)
        got = diff_c(m, ob_a, a.size, root_a, ga, ob_b, b.size, root_b, gb)
        bits = H.unpack(got, nb)
        assert (got == H.pack(bits)).all(), (name, "pad bits set")
        want = D.same_chunks(ob_a, a.size, root_a.tobytes(), ga, ob_b, b.size, root_b.tobytes(), gb)
        assert (bits == want).all(), (name, "not the restatement", np.flatnonzero(bits != want)[:8])
        if (name, G) not in _TRUTH:
            _TRUTH[(name, G)] = D.truth(a, b, G)
        true = _TRUTH[(name, G)]
        assert (bits == true).all(), (name, "not what the bytes say", np.flatnonzero(bits != true)[:8])
        assert (m.bao.diff_host(ob_a, a.size, root_a, ob_b, b.size, root_b, ga, gb) == got).all(), name
        na = H.num_chunks(a.size)
        seen["root case"] += na <= 1 << G and nb <= 1 << G
        seen["whole on one side"] += (na <= 1 << G) != (nb <= 1 << G)
        seen["ragged last unit"] += G == 0 or (nb > 1 << G and nb % (1 << G) != 0)
        seen["some same, some not"] += bool(bits.any()) and not bool(bits.all())
    assert all(seen.values()), seen


def test_the_numpy_restatement_is_the_plain_one():
    """places_np / same_chunks_np (the GPU test's yardstick at 2^20 chunks) against the walk over node_spans, on fabricated outboards"""
    rng = np.random.default_rng(3)
    for na, nb in ((1025, 1025), (1025, 2049), (2049, 1025), (70, 200), (129, 129), (1029, 1029)):
        for ga, gb in ((0, 0), (0, 6), (6, 0), (1, 4), (4, 4), (6, 6)):
            G = max(ga, gb)
            ob_a = rng.integers(0, 256, 8 + 64 * (D.GR.num_groups(na, ga) - 1), dtype=np.uint8)
            ob_b = rng.integers(0, 256, 8 + 64 * (D.GR.num_groups(nb, gb) - 1), dtype=np.uint8)
            pa, pb = D.places_np(na, ga, G), D.places_np(nb, gb, G)
            for u in range(0, min(pa.size, pb.size), 3):                        # every third unit shares its CV
                ob_b[pb[u]:pb[u] + 32] = ob_a[pa[u]:pa[u] + 32]
            want = D.same_chunks(ob_a.tobytes(), na * K, bytes(32), ga, ob_b.tobytes(), nb * K, bytes(32), gb)
            assert (D.same_chunks_np(ob_a, na, ga, ob_b, nb, gb) == want).all(), (na, nb, ga, gb)
            assert want.any() and not want.all()


def test_refusals():
    m = T.pkg()
    L = m.lib()
    ob, root, same = bytes(8), np.zeros(8, dtype=np.uint32), np.full(3, GUARD, dtype=np.uint64)
    r, s = root.ctypes.data, same[1:].ctypes.data
    assert L.b3w_bao_outboard_diff(ob, 1, r, 0, ob, 1, r, 0, s) == 0 and same.tolist() == [GUARD, 1, GUARD]
    same[1] = GUARD
    huge = ((1 << 30) + 1) * K
    for args in ((None, 1, r, 0, ob, 1, r, 0, s), (ob, 1, None, 0, ob, 1, r, 0, s), (ob, 1, r, 0, None, 1, r, 0, s), (ob, 1, r, 0, ob, 1, None, 0, s),
                 (ob, 1, r, 0, ob, 1, r, 0, None), (ob, 1, r, 7, ob, 1, r, 0, s), (ob, 1, r, 0, ob, 1, r, 7, s), (ob, huge, r, 0, ob, 1, r, 0, s),
                 (ob, 1, r, 0, ob, huge, r, 0, s)):
        assert L.b3w_bao_outboard_diff(*args) == BAD, args
        assert (same == GUARD).all()
    with pytest.raises(m.B3WError):
        m.bao.diff_host(ob, 1, root, ob, 1, root, 7, 0)
    with pytest.raises(m.B3WError):
        m.bao.diff_host(ob, 2 * K, root, ob, 1, root)                            # (an outboard that is not of that length)
    with pytest.raises(m.B3WError):
        m.bao.diff_host(ob, 1, root[:7], ob, 1, root)
