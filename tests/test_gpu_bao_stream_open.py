"""Outboards of streamed files whose length is not known up front (bao.StreamOutboardOpen / outboard_stream_open,
b3w_bao_stream_open_*): whatever the window size, the order of the pushes, the streams they come on and the capacity given, an open
session leaves byte for byte what the batch calls leave for the same bytes as a batch of one, and writes nothing behind the outboard;
files past 1 GiB take the second storey; push_many takes open sessions and no mixture; a refused call launches nothing and leaves the
session usable; repeated sessions agree; the helper streams from a reader of unknown length through a ring whose device memory does
not grow with the file."""
import ctypes
import io

import numpy as np
import pytest

import b3w_testlib as T
from test_gpu_bao_batch import _arena

pytestmark = pytest.mark.gpu

GS = [0, 1, 4, 6]
K = 1024
MIB = 1 << 20
LENS = [0, 1, MIB - 1, MIB, MIB + 1, 2 * MIB, 2049 * K + 3, 3 * MIB, 3 * MIB + 5, 5 * MIB + 5]
ORDERS = ["ascending", "descending", "two streams"]
CANARY = 64

_state = {}


def _setup():
    """one context, one arena of every length on the device and, per group_log, the batch calls' outboard and root of every file as a
    batch of one: made once, shared, never written to"""
    if not _state:
        import torch
        m = T.pkg()
        arena, offsets = _arena(LENS, seed=15)
        _state.update(m=m, ctx=m.Context("nova_vesta", 0), arena=arena, offsets=offsets, d_arena=torch.from_numpy(arena).cuda(), ref={})
    return _state


def _data(s, f):
    a = int(s["offsets"][f])
    return s["d_arena"][a:a + LENS[f]]


def _host(s, f):
    a = int(s["offsets"][f])
    return s["arena"][a:a + LENS[f]]


def _batch_outboard(m, ctx, d_file, g):
    n = d_file.numel()
    return m.bao.outboard_batch(ctx, d_file, [0], [n]) if g == 0 else m.bao.outboard_groups_batch(ctx, d_file, [0], [n], g)


def _ref(s, f, g):
    if (f, g) not in s["ref"]:
        s["ref"][f, g] = _batch_outboard(s["m"], s["ctx"], _data(s, f), g)
    return s["ref"][f, g]


def _push_tiles(session, d_file, window, order):
    """the whole MiB of the file in windows of `window` (the last one maybe shorter, still whole MiB) in `order`; leaves the current
    stream behind all of them"""
    import torch
    whole = d_file.numel() // MIB * MIB
    wins = [(off, min(window, whole - off)) for off in range(0, whole, window)]
    if order == "ascending":
        for off, nb in wins:
            session.push(off, d_file[off:off + nb])
    elif order == "descending":
        for off, nb in reversed(wins):
            session.push(off, d_file[off:off + nb])
    else:
        cur = torch.cuda.current_stream()
        sides = [torch.cuda.Stream(), torch.cuda.Stream()]
        for st in sides:
            st.wait_stream(cur)
        for i, (off, nb) in enumerate(wins):
            session.push(off, d_file[off:off + nb], stream=sides[i & 1].cuda_stream)
        for st in sides:
            ev = torch.cuda.Event()
            ev.record(st)
            cur.wait_event(ev)                                                 # the event before finish


def _finish_into(m, session, d_file, size, fill=0xA5):
    """b3w_bao_stream_open_finish into a buffer of the caller's: `size` bytes filled with 0xA5 and CANARY bytes behind them
    -> rc, the buffer, the root, the length"""
    import torch
    buf = torch.full((size + CANARY,), fill, dtype=torch.uint8, device="cuda")
    root = torch.full((1, 8), -1, dtype=torch.int32, device="cuda")
    tail = d_file[d_file.numel() // MIB * MIB:]
    n = ctypes.c_uint64(0)
    rc = m.lib().b3w_bao_stream_open_finish(session._h, tail.data_ptr() if tail.numel() else None, tail.numel(), buf.data_ptr(), size, root.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream, ctypes.byref(n))
    return rc, buf, root, n.value


def _check(m, session, d_file, want, g, what):
    import torch
    size = want["outboards"].numel()
    assert size == m.bao.group_outboard_size(d_file.numel(), g)
    rc, buf, root, n = _finish_into(m, session, d_file, size)
    assert rc == m.B3W_OK, (what, session.ctx.last_error())
    assert n == d_file.numel(), what
    assert torch.equal(buf[:size], want["outboards"]), what
    assert torch.equal(root, want["roots"]), what
    assert bool((buf[size:] == 0xA5).all().item()), (what, "the canary")


@pytest.mark.parametrize("g", GS)
def test_outboards_equal_the_batch_calls(g):
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    for f, ln in enumerate(LENS):
        want = _ref(s, f, g)
        for capacity in ((ln + MIB - 1) // MIB * MIB, 64 * MIB):
            for window in (MIB, 2 * MIB):
                for order in ORDERS:
                    so = m.bao.StreamOutboardOpen(ctx, capacity, g)
                    so.staging.fill_(0x5A)
                    _push_tiles(so, _data(s, f), window, order)
                    _check(m, so, _data(s, f), want, g, (g, ln, capacity, window, order))
                    so.close()


@pytest.mark.parametrize("g", [0, 4])
def test_the_python_finish_and_an_outboard_off_the_16_byte_boundary(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    for f, ln in enumerate(LENS):
        want = _ref(s, f, g)
        so = m.bao.StreamOutboardOpen(ctx, ln, g)                              # (a capacity of exactly the length)
        _push_tiles(so, _data(s, f), MIB, "descending")
        got = so.finish(_data(s, f)[ln // MIB * MIB:])
        assert got["length"] == ln and so.length == ln
        assert torch.equal(got["outboards"], want["outboards"]) and torch.equal(got["roots"], want["roots"]), (g, ln)
        assert list(got["ob_first"]) == list(want["ob_first"])
        so.close()
        # the outboard 8 bytes off a 16-byte boundary: the relocation's 8-byte moves
        size = want["outboards"].numel()
        so = m.bao.StreamOutboardOpen(ctx, ln + 7, g)
        _push_tiles(so, _data(s, f), 2 * MIB, "ascending")
        buf = torch.full((size + CANARY + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        root = torch.full((1, 8), -1, dtype=torch.int32, device="cuda")
        tail = _data(s, f)[ln // MIB * MIB:]
        rc = m.lib().b3w_bao_stream_open_finish(so._h, tail.data_ptr() if tail.numel() else None, tail.numel(), buf.data_ptr() + 8, size, root.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream, None)
        assert rc == m.B3W_OK
        assert torch.equal(buf[8:8 + size], want["outboards"]) and torch.equal(root, want["roots"]), (g, ln)
        assert bool((buf[:8] == 0xA5).all().item()) and bool((buf[8 + size:] == 0xA5).all().item())
        so.close()


@pytest.mark.parametrize("g", [0, 6])
def test_a_file_past_one_gib_takes_the_second_storey(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    ln = 1025 * MIB + 5
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1500 + g)
    d_file = torch.randint(0, 256, (ln,), dtype=torch.uint8, device="cuda", generator=gen)
    want = _batch_outboard(m, ctx, d_file, g)
    so = m.bao.StreamOutboardOpen(ctx, 1100 * MIB, g)
    _push_tiles(so, d_file, 64 * MIB, "two streams")
    _check(m, so, d_file, want, g, (g, ln))
    so.close()


def test_push_many_takes_every_length_at_once_with_mixed_group_sizes():
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    gs = [GS[f % len(GS)] for f in range(len(LENS))]
    sessions = [m.bao.StreamOutboardOpen(ctx, ln + 3 * MIB, gs[f]) for f, ln in enumerate(LENS)]
    for r in range(max(LENS) // MIB):                                          # round r: MiB r of every file that has one, in one call
        live = [f for f, ln in enumerate(LENS) if (r + 1) * MIB <= ln]
        m.bao.push_many([sessions[f] for f in live], [r * MIB] * len(live), [_data(s, f)[r * MIB:(r + 1) * MIB] for f in live])
    for f, ln in enumerate(LENS):
        got = sessions[f].finish(_data(s, f)[ln // MIB * MIB:])
        want = _ref(s, f, gs[f])
        assert got["length"] == ln
        assert torch.equal(got["outboards"], want["outboards"]) and torch.equal(got["roots"], want["roots"]), (gs[f], ln)
        sessions[f].close()


@pytest.mark.parametrize("g", [0, 4])
def test_push_many_with_a_session_twice_and_no_mixture_of_kinds(g):
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    f = LENS.index(5 * MIB + 5)
    d, ln, want = _data(s, f), LENS[f], _ref(s, f, g)
    so = m.bao.StreamOutboardOpen(ctx, 64 * MIB, g)
    known = m.bao.StreamOutboard(ctx, ln, g)
    known.outboards.fill_(0xA5)
    for pair in ([so, known], [known, so]):                                    # a mixed call: refused whole, nothing changes
        with pytest.raises(m.B3WError, match="entry 1"):
            m.bao.push_many(pair, [0, 0], [d[:MIB], d[:MIB]])
    with pytest.raises(m.B3WError, match="entry 1.*named twice"):              # the same tile twice in a call
        m.bao.push_many([so, so], [MIB, 0], [d[MIB:3 * MIB], d[:2 * MIB]])
    assert so._bytes == 0
    m.bao.push_many([so, so], [3 * MIB, 0], [d[3 * MIB:5 * MIB], d[:2 * MIB]])   # twice, disjoint tiles
    m.bao.push_many([so], [2 * MIB], [d[2 * MIB:3 * MIB]])
    _check(m, so, d, want, g, (g, "twice in a call"))
    for off, nb in m.bao.windows(ln, MIB):                                     # the known-length session lost nothing to the refusals
        known.push(off, d[off:off + nb])
    import torch
    assert torch.equal(known.finish()["outboards"], want["outboards"])
    so.close()
    known.close()


@pytest.mark.parametrize("g", [0, 6])
def test_refused_calls_launch_nothing_and_leave_the_session_usable(g):
    import torch
    s = _setup()
    m, ctx, L = s["m"], s["ctx"], s["m"].lib()
    f = LENS.index(2049 * K + 3)                                               # tiles 0 and 1 and a tail of 1 KiB + 3
    f3 = LENS.index(3 * MIB)
    d, ln, want = _data(s, f), LENS[f], _ref(s, f, g)
    big = _data(s, LENS.index(5 * MIB + 5))
    st = torch.cuda.current_stream().cuda_stream
    size = want["outboards"].numel()

    def refused(rc, text):
        assert rc == m.B3W_E_BAD_ARGUMENT and text in ctx.last_error(), (rc, ctx.last_error())

    def push(se, off, w):
        return L.b3w_bao_stream_push(se._h, off, w.data_ptr(), w.numel(), st)

    h = ctypes.c_void_p()
    refused(L.b3w_bao_stream_open_begin(ctx.handle, MIB, g, 16, 1 << 20, 16, 1 << 20, None), "null session pointer")
    refused(L.b3w_bao_stream_open_begin(ctx.handle, MIB, 7, 16, 1 << 20, 16, 1 << 20, ctypes.byref(h)), "group_log")
    refused(L.b3w_bao_stream_open_begin(ctx.handle, MIB, g, None, 1 << 20, 16, 1 << 20, ctypes.byref(h)), "null pointer")
    refused(L.b3w_bao_stream_open_begin(ctx.handle, MIB, g, 24, 1 << 20, 16, 1 << 20, ctypes.byref(h)), "16-byte aligned")
    refused(L.b3w_bao_stream_open_begin(ctx.handle, MIB, g, 16, 8, 16, 1 << 20, ctypes.byref(h)), "staging is smaller")
    refused(L.b3w_bao_stream_open_begin(ctx.handle, MIB, g, 16, 1 << 20, 16, 8, ctypes.byref(h)), "scratch is smaller")
    refused(L.b3w_bao_stream_open_begin(ctx.handle, (1 << 40) + 1, g, 16, 1 << 62, 16, 1 << 62, ctypes.byref(h)), "2^30 chunks")
    assert not h.value

    # a file longer than the capacity: refused at finish, and the session completes as the 2 MiB it has room for
    se = m.bao.StreamOutboardOpen(ctx, 2 * MIB + 5, g)
    assert push(se, 0, d[:2 * MIB]) == m.B3W_OK
    buf = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    root = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    refused(L.b3w_bao_stream_open_finish(se._h, d[2 * MIB:].data_ptr(), K + 3, buf.data_ptr(), size, root.data_ptr(), st, None), "capacity")
    assert bool((buf == 0xA5).all().item())
    _check(m, se, d[:2 * MIB], _batch_outboard(m, ctx, d[:2 * MIB], g), g, (g, "above the capacity"))
    se.close()

    cases = ["ragged window", "offset off a MiB", "past the capacity", "tile twice", "tile 1 missing", "tail of 1 MiB", "null tail", "small outboard",
             "finish of the other kind", "finish twice and push after"]
    for case in cases:
        se = m.bao.StreamOutboardOpen(ctx, 3 * MIB, g)
        file, ref = d, want
        if case == "ragged window":
            refused(push(se, 0, d[:MIB + K]), "whole tiles")
            refused(push(se, 2 * MIB, d[2 * MIB:]), "whole tiles")
            assert push(se, 0, d[:2 * MIB]) == m.B3W_OK
        elif case == "offset off a MiB":
            refused(push(se, K, d[K:K + MIB]), "multiple of 1 MiB")
            assert push(se, 0, d[:2 * MIB]) == m.B3W_OK
        elif case == "past the capacity":
            refused(push(se, 2 * MIB, big[2 * MIB:4 * MIB]), "capacity")
            refused(push(se, 3 * MIB, big[3 * MIB:4 * MIB]), "capacity")
            assert push(se, MIB, d[MIB:2 * MIB]) == m.B3W_OK and push(se, 0, d[:MIB]) == m.B3W_OK
        elif case == "tile twice":
            assert push(se, MIB, d[MIB:2 * MIB]) == m.B3W_OK
            refused(push(se, 0, d[:2 * MIB]), "tile 1 was pushed before")
            assert push(se, 0, d[:MIB]) == m.B3W_OK
        elif case == "tile 1 missing":
            file, ref = _data(s, f3), _ref(s, f3, g)
            assert push(se, 0, file[:MIB]) == m.B3W_OK and push(se, 2 * MIB, file[2 * MIB:]) == m.B3W_OK
            rc, buf, _, _ = _finish_into(m, se, file, ref["outboards"].numel())
            refused(rc, "tile 1 has not been pushed")
            assert bool((buf == 0xA5).all().item())
            assert push(se, MIB, file[MIB:2 * MIB]) == m.B3W_OK
        elif case == "tail of 1 MiB":
            assert push(se, 0, d[:MIB]) == m.B3W_OK
            n = ctypes.c_uint64(77)
            buf = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
            root = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
            refused(L.b3w_bao_stream_open_finish(se._h, d[MIB:].data_ptr(), MIB, buf.data_ptr(), size, root.data_ptr(), st, ctypes.byref(n)), "1 MiB or more")
            assert n.value == 77 and bool((buf == 0xA5).all().item())
            assert push(se, MIB, d[MIB:2 * MIB]) == m.B3W_OK
        elif case in ("null tail", "small outboard"):
            assert push(se, 0, d[:2 * MIB]) == m.B3W_OK
            buf = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
            root = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
            if case == "null tail":
                refused(L.b3w_bao_stream_open_finish(se._h, None, K + 3, buf.data_ptr(), size, root.data_ptr(), st, None), "null tail")
            else:
                refused(L.b3w_bao_stream_open_finish(se._h, d[2 * MIB:].data_ptr(), K + 3, buf.data_ptr(), size - 1, root.data_ptr(), st, None), "outboard is smaller")
                refused(L.b3w_bao_stream_open_finish(se._h, d[2 * MIB:].data_ptr(), K + 3, buf.data_ptr() + 4, size, root.data_ptr(), st, None), "aligned")
                refused(L.b3w_bao_stream_open_finish(se._h, d[2 * MIB:].data_ptr(), K + 3, None, size, root.data_ptr(), st, None), "null pointer")
            assert bool((buf == 0xA5).all().item())
        elif case == "finish of the other kind":
            assert push(se, 0, d[:2 * MIB]) == m.B3W_OK
            refused(L.b3w_bao_stream_finish(se._h, st), "open session")
            hs = np.array([se._h.value], dtype=np.uint64)
            refused(L.b3w_bao_stream_finish_many(ctx.handle, hs.ctypes.data, 1, st), "entry 0")
            known = m.bao.StreamOutboard(ctx, ln, g)
            for off, nb in m.bao.windows(ln, 3 * MIB):
                known.push(off, d[off:off + nb])
            hs = np.array([known._h.value, se._h.value], dtype=np.uint64)
            refused(L.b3w_bao_stream_finish_many(ctx.handle, hs.ctypes.data, 2, st), "entry 1")
            assert torch.equal(known.finish()["outboards"], ref["outboards"])   # (atomic: the refusal did not finish the known-length one)
            known.close()
        else:
            assert push(se, 0, d[:2 * MIB]) == m.B3W_OK
        _check(m, se, file, ref, g, (g, case))                                 # ... and the same session completes with the right bytes
        if case == "finish twice and push after":
            rc, buf, _, _ = _finish_into(m, se, file, size)
            refused(rc, "finished")
            assert bool((buf == 0xA5).all().item())
            refused(push(se, 2 * MIB, big[2 * MIB:3 * MIB]), "finished")
            with pytest.raises(m.B3WError, match="finished"):
                m.bao.push_many([se], [2 * MIB], [big[2 * MIB:3 * MIB]])
        se.close()


@pytest.mark.parametrize("g", [4, 6])
def test_forty_fresh_sessions_agree_with_the_batch_call(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    ln = 3 * MIB + 5
    gen = torch.Generator(device="cuda")
    gen.manual_seed(150 + g)
    for rep in range(40):
        d_file = torch.randint(0, 256, (ln,), dtype=torch.uint8, device="cuda", generator=gen)
        want = _batch_outboard(m, ctx, d_file, g)
        so = m.bao.StreamOutboardOpen(ctx, 4 * MIB, g)
        _push_tiles(so, d_file, MIB, "ascending")
        _check(m, so, d_file, want, g, (g, rep))
        so.close()


class _ShortReads(io.RawIOBase):
    """a reader that hands out at most `step` bytes a call"""

    def __init__(self, data, step):
        self.data, self.at, self.step = memoryview(data), 0, step

    def readinto(self, b):
        k = min(len(b), self.step, len(self.data) - self.at)
        b[:k] = self.data[self.at:self.at + k]
        self.at += k
        return k


@pytest.mark.parametrize("g", [0, 4])
def test_the_helper_streams_a_source_of_unknown_length(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]

    def same(got, f):
        want = _ref(s, f, g)
        assert got["length"] == LENS[f]
        assert torch.equal(got["outboards"], want["outboards"]) and torch.equal(got["roots"], want["roots"]), (g, LENS[f])
        assert list(got["ob_first"]) == list(want["ob_first"])
    for ln in (0, MIB, 3 * MIB + 5, 5 * MIB + 5):
        f = LENS.index(ln)
        data = _host(s, f).tobytes()
        for window in (MIB, 2 * MIB):
            for ring in (1, 2):
                same(m.bao.outboard_stream_open(ctx, io.BytesIO(data), 8 * MIB, window, g, ring), f)
                same(m.bao.outboard_stream_open(ctx, data, 8 * MIB, window, g, ring), f)
    f = LENS.index(5 * MIB + 5)
    same(m.bao.outboard_stream_open(ctx, _ShortReads(_host(s, f), 1000003), 6 * MIB, 2 * MIB, g), f)
    same(m.bao.outboard_stream_open(ctx, _ShortReads(_host(s, f), 1000003), LENS[f], MIB, g, 3), f)   # (a capacity of exactly the length)
    same(m.bao.outboard_stream_open(ctx, _host(s, f), LENS[f], MIB, g), f)                            # (a numpy buffer)
    with pytest.raises(m.B3WError, match="capacity"):
        m.bao.outboard_stream_open(ctx, io.BytesIO(_host(s, f).tobytes()), LENS[f] - 1, MIB, g)
    with pytest.raises(m.B3WError, match="capacity"):
        m.bao.outboard_stream_open(ctx, io.BytesIO(_host(s, f).tobytes()), 2 * MIB, 2 * MIB, g)
    same(m.bao.outboard_stream_open(ctx, io.BytesIO(_host(s, f).tobytes()), LENS[f], 2 * MIB, g), f)  # the context is none the worse


def test_the_helpers_device_memory_does_not_grow_with_the_file():
    """The helper makes a device window per ring slot that gets bytes, the staging, the scratch, and in finish the outboard and the
    32-byte root: nothing else, so the peak of the bytes REQUESTED of the allocator rises by exactly their sum (requested_bytes counts
    what was asked for, not the allocator's rounding).  A source that ends on a window's last byte makes no slot for the empty read
    that finds the end.  max_memory_allocated counts blocks instead: sizes are rounded up to 512 bytes, and the caching allocator
    hands out a cached block of more than 1 MiB whole where splitting it would leave less than 1 MiB, so each of the four large
    allocations (two windows, staging, outboard) may count up to 1 MiB above its size: SLACK.  A helper that kept the file on the
    device would rise by the file, 64 MiB more for the longer one."""
    import torch
    s = _setup()
    m, ctx, L = s["m"], s["ctx"], s["m"].lib()
    rng = np.random.default_rng(151)
    window, g, capacity = 2 * MIB, 0, 80 * MIB
    SLACK = 4 * MIB
    session = L.b3w_bao_stream_open_staging_bytes(capacity, g) + L.b3w_bao_stream_open_scratch_bytes(capacity)
    m.bao.outboard_stream_open(ctx, io.BytesIO(bytes(MIB)), capacity, window, g, 2)                     # (warm: streams, the context's slots)
    rise = {}
    for ln, ring in ((8 * MIB + 5, 2), (72 * MIB + 5, 2), (4 * MIB, 3), (2 * MIB, 2), (5, 2)):
        data = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        asked = torch.cuda.memory_stats()["requested_bytes.all.current"]
        torch.cuda.reset_peak_memory_stats()
        got = m.bao.outboard_stream_open(ctx, io.BytesIO(data), capacity, window, g, ring)
        torch.cuda.synchronize()
        rise[ln] = torch.cuda.max_memory_allocated() - before
        asked = torch.cuda.memory_stats()["requested_bytes.all.peak"] - asked
        fixed = min(ring, -(-ln // window)) * window + session
        exact = fixed + m.bao.group_outboard_size(ln, g) + 32
        bound = fixed + m.bao.group_outboard_size(ln, g) + SLACK
        print(f"outboard_stream_open of {ln} bytes, ring {ring}: {asked} bytes requested ({exact} expected), max_memory_allocated rose by "
              f"{rise[ln]}, bound {bound} (windows + staging + scratch {fixed})")
        assert got["length"] == ln
        assert asked == exact, (ln, ring, asked, exact)
        assert rise[ln] <= bound, (ln, rise[ln], bound)
        del got
    small, large = 8 * MIB + 5, 72 * MIB + 5
    assert session + 2 * window + m.bao.group_outboard_size(large, g) + SLACK < large      # (the bound tells a resident file from a streamed one)
    assert rise[large] - rise[small] <= m.bao.group_outboard_size(large, g) - m.bao.group_outboard_size(small, g) + SLACK
