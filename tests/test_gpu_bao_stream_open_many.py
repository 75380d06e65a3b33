"""Many open-length sessions finished at once (b3w_bao_stream_open_finish_many, bao.open_finish_many / outboard_stream_open_many):
whatever the lengths, the group sizes, the outboards' alignment and the tails' places, one call leaves for every session byte for
byte what the batch calls leave for the same bytes as a batch of one (outboard_batch for g = 0, outboard_groups_batch otherwise),
and nothing behind the outboard; files past 1 GiB take the second storey beside small ones; a refused call launches nothing, changes
no session and names the entry; more calls in flight than staging slots; repeated rounds agree; the Python call equals finish() on
twin sessions; the helper streams sources of unknown length through lanes and its device memory does not grow with the number of
files beyond the results.

Outboards are pre-filled with 0xA5 and have CANARY bytes behind them (and 16 in front); data comes from seeded generators.

One reason of refusal has no case here: more than 2^31 - 1 workgroups in one grid.  A session moves at most 2^22 workgroups (2^20
tiles of a file of 2^30 chunks, four pieces a block at g = 0), so the call would need 512 sessions of a tebibyte each, pushed."""
import ctypes
import io

import numpy as np
import pytest

import b3w_testlib as T
from test_gpu_bao_batch import _arena

pytestmark = pytest.mark.gpu

K = 1024
MIB = 1 << 20
LENS = [0, 1, MIB - 1, MIB, MIB + 1, 2 * MIB, 2049 * K + 3, 3 * MIB + 5, 5 * MIB + 5, 17 * MIB + 5]
MIXED = [0, 1, 3, 4, 5, 6]
CANARY = 64
FRONT = 16
UNSET = (1 << 64) - 7

_state = {}


def _setup():
    """one context, one arena of every length on the device and, per (file, group_log) asked for, the batch call's outboard and
    root of the file as a batch of one: made once, shared, never written to"""
    if not _state:
        import torch
        m = T.pkg()
        arena, offsets = _arena(LENS, seed=16)
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


class _Entry:
    """a fresh open session for the bytes of d_file with its whole MiB still to push, the tail `tail_shift` bytes into a tensor of
    its own (tail_shift None: where it lies in the file), and an outboard buffer `ob_shift` bytes off a 16-byte boundary"""

    def __init__(self, m, ctx, d_file, g, want, capacity=None, tail_shift=None, ob_shift=0):
        import torch
        self.d, self.g, self.want, self.ln = d_file, g, want, d_file.numel()
        self.se = m.bao.StreamOutboardOpen(ctx, self.ln + 3 * MIB if capacity is None else capacity, g)
        self.whole = self.ln // MIB * MIB
        tail = d_file[self.whole:]
        if tail_shift is not None and tail.numel():
            own = torch.empty(tail_shift + tail.numel(), dtype=torch.uint8, device="cuda")
            assert own.data_ptr() % 16 == 0
            own[tail_shift:] = tail
            tail = own[tail_shift:]
        self.tail = tail
        self.size = want["outboards"].numel()
        assert self.size == m.bao.group_outboard_size(self.ln, g)
        self.shift = ob_shift
        self.buf = torch.full((FRONT + self.size + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.root = torch.full((1, 8), -1, dtype=torch.int32, device="cuda")

    ob_ptr = property(lambda self: self.buf.data_ptr() + self.shift)
    tail_ptr = property(lambda self: self.tail.data_ptr() if self.tail.numel() else 0)

    def untouched(self):
        return bool((self.buf == 0xA5).all().item()) and bool((self.root == -1).all().item())

    def check(self, what, ln=None):
        import torch
        assert torch.equal(self.buf[self.shift:self.shift + self.size], self.want["outboards"]), (what, "the outboard")
        assert torch.equal(self.root, self.want["roots"]), (what, "the root")
        assert bool((self.buf[:self.shift] == 0xA5).all().item()) and bool((self.buf[self.shift + self.size:] == 0xA5).all().item()), (what, "the canary")


def _entry(s, f, g, **kw):
    return _Entry(s["m"], s["ctx"], _data(s, f), g, _ref(s, f, g), **kw)


def _push_all(m, entries, stream=0):
    """the whole MiB of every entry that has one, in ONE push_many"""
    live = [e for e in entries if e.whole]
    m.bao.push_many([e.se for e in live], [0] * len(live), [e.d[:e.whole] for e in live], stream=stream)


def _args(entries):
    """the call's six arrays as lists"""
    return dict(handles=[e.se._h.value for e in entries], tail_ptrs=[e.tail_ptr for e in entries], tail_bytes=[e.tail.numel() for e in entries],
                ob_ptrs=[e.ob_ptr for e in entries], ob_bytes=[e.size for e in entries], root_ptrs=[e.root.data_ptr() for e in entries])


ORDER = ("handles", "tail_ptrs", "tail_bytes", "ob_ptrs", "ob_bytes", "root_ptrs")


def _raw(m, ctx, args, stream=None, null=None, want_lens=True):
    """b3w_bao_stream_open_finish_many over the lists of `args` (`null`: the array passed as NULL) -> rc, out_lens"""
    import torch
    arrays = [np.array([x or 0 for x in args[k]], dtype=np.uint64) for k in ORDER]
    n = len(args["handles"])
    lens = np.full(n, UNSET, dtype=np.uint64)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = m.lib().b3w_bao_stream_open_finish_many(ctx.handle, *[None if k == null else a.ctypes.data for k, a in zip(ORDER, arrays)], n, st,
                                                 lens.ctypes.data if want_lens else None)
    return rc, lens


def _finish(s, entries, stream=None):
    m, ctx = s["m"], s["ctx"]
    rc, lens = _raw(m, ctx, _args(entries), stream)
    assert rc == m.B3W_OK, ctx.last_error()
    assert [int(x) for x in lens] == [e.ln for e in entries]


@pytest.mark.parametrize("g", ["mixed", 0, 1, 3, 6])
def test_every_length_in_one_call(g):
    """17 tiles at g = 6 cross a relocation workgroup of 16 blocks; 3 tiles at g = 3 leave a workgroup half filled; g = 0 has four
    pieces a block; a uniform g = 0 runs the plain instantiations of the reused kernels, every other call the group ones"""
    s = _setup()
    m = s["m"]
    gs = [MIXED[f % len(MIXED)] for f in range(len(LENS))] if g == "mixed" else [g] * len(LENS)
    entries = [_entry(s, f, gs[f]) for f in range(len(LENS))]
    for e in entries:
        e.se.staging.fill_(0x5A)
    _push_all(m, entries)
    _finish(s, entries)
    for e in entries:
        e.check((g, e.g, e.ln))
        e.se.close()


def test_outboards_on_and_off_the_16_byte_boundary_and_tails_at_odd_places():
    s = _setup()
    m = s["m"]
    entries = [_entry(s, f, (0, 4, 2)[f % 3], tail_shift=(0, 3, 8)[(f // 2) % 3], ob_shift=(0, 8)[f % 2]) for f in range(len(LENS))]
    assert {e.ob_ptr % 16 for e in entries} == {0, 8}
    assert {e.tail_ptr % 16 for e in entries if e.tail.numel()} == {0, 3, 8}
    _push_all(m, entries)
    _finish(s, entries)
    for e in entries:
        e.check((e.g, e.ln, e.shift))
        e.se.close()
    # ... and the other way round: the neighbours swap their phases
    entries = [_entry(s, f, (6, 0, 1)[f % 3], tail_shift=(8, 0, 3)[f % 3], ob_shift=(8, 0)[f % 2]) for f in range(len(LENS))]
    _push_all(m, entries)
    _finish(s, entries)
    for e in entries:
        e.check((e.g, e.ln, e.shift))
        e.se.close()


@pytest.mark.parametrize("g", [0, 6])
def test_a_file_past_one_gib_takes_the_second_storey_beside_small_ones(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    ln = 1025 * MIB + 5
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1600 + g)
    d_file = torch.randint(0, 256, (ln,), dtype=torch.uint8, device="cuda", generator=gen)
    big = _Entry(m, ctx, d_file, g, _batch_outboard(m, ctx, d_file, g), capacity=1100 * MIB)
    entries = [_entry(s, LENS.index(MIB), g), big, _entry(s, LENS.index(0), g)]
    _push_all(m, entries)
    _finish(s, entries)
    for e in entries:
        e.check((g, e.ln))
        e.se.close()


CASES = ["tile 1 missing", "tail of 1 MiB", "null tail", "above the capacity", "null outboard", "null root", "misaligned outboard", "misaligned root",
         "small outboard", "finished", "null session", "another context", "not open", "twice", "null array"]


@pytest.mark.parametrize("case", CASES)
def test_a_refused_call_launches_nothing_changes_no_session_and_names_the_entry(case):
    import torch
    s = _setup()
    m, ctx, L = s["m"], s["ctx"], s["m"].lib()
    f0, f1, f2 = LENS.index(2049 * K + 3), LENS.index(3 * MIB + 5), LENS.index(MIB + 1)
    d1 = _data(s, f1)
    if case == "above the capacity":                                           # room for the three MiB and not for the tail
        mid = _Entry(m, ctx, d1, 4, _ref(s, f1, 4), capacity=3 * MIB)
    else:
        mid = _entry(s, f1, 4)
    entries = [_entry(s, f0, 0), mid, _entry(s, f2, 6, ob_shift=8)]
    if case == "tile 1 missing":
        m.bao.push_many([entries[0].se, mid.se, mid.se, entries[2].se], [0, 0, 2 * MIB, 0],
                        [entries[0].d[:2 * MIB], d1[:MIB], d1[2 * MIB:3 * MIB], entries[2].d[:MIB]])
    else:
        _push_all(m, entries)
    args = _args(entries)
    text, keep, null = None, [], None
    if case == "tile 1 missing":
        text = "tile 1 has not been pushed"
    elif case == "tail of 1 MiB":
        args["tail_bytes"][1], text = MIB, "1 MiB or more"
    elif case == "null tail":
        args["tail_ptrs"][1], text = 0, "null tail"
    elif case == "above the capacity":
        text = "capacity"
    elif case == "null outboard":
        args["ob_ptrs"][1], text = 0, "null pointer"
    elif case == "null root":
        args["root_ptrs"][1], text = 0, "null pointer"
    elif case == "misaligned outboard":
        args["ob_ptrs"][1], text = mid.ob_ptr + 4, "aligned"
    elif case == "misaligned root":
        args["root_ptrs"][1], text = mid.root.data_ptr() + 2, "aligned"
    elif case == "small outboard":
        args["ob_bytes"][1], text = mid.size - 1, "outboard is smaller"
    elif case == "finished":                                                   # by the per-session call, into a buffer of its own
        own = _entry(s, f1, 4)
        n = ctypes.c_uint64()
        assert L.b3w_bao_stream_open_finish(mid.se._h, mid.tail_ptr, mid.tail.numel(), own.ob_ptr, own.size, own.root.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream, ctypes.byref(n)) == m.B3W_OK
        own.check("open_finish")
        own.se.close()
        text = "the session is finished"
    elif case == "null session":
        args["handles"][1], text = 0, "null session"
    elif case == "another context":
        other = m.Context("nova_vesta", 0)
        alien = m.bao.StreamOutboardOpen(other, 4 * MIB, 4)
        keep = [other, alien]
        args["handles"][1], text = alien._h.value, "another context"
    elif case == "not open":
        known = m.bao.StreamOutboard(ctx, LENS[f1], 4)
        keep = [known]
        args["handles"][1], text = known._h.value, "not an open session"
    elif case == "twice":
        for k in ORDER:                                                        # entry 0 once more, arguments and all
            args[k][1] = args[k][0]
        text = "appears twice"
    for null in ORDER if case == "null array" else [None]:
        rc, lens = _raw(m, ctx, args, null=null)
        assert rc == m.B3W_E_BAD_ARGUMENT, (case, null)
        err = ctx.last_error()
        assert ("null array" in err) if null else ("entry 1" in err and text in err), (case, err)
        assert all(int(x) == UNSET for x in lens)
    torch.cuda.synchronize()
    for e in entries:
        assert e.untouched(), (case, e.ln)
    # the same three sessions then complete through a good call
    if case == "tile 1 missing":
        mid.se.push(MIB, d1[MIB:2 * MIB])
    if case == "above the capacity":                                           # ... as the three MiB it has room for
        whole = d1[:3 * MIB]
        mid.want, mid.tail, mid.ln = _batch_outboard(m, ctx, whole, 4), whole[:0], 3 * MIB
        old, mid.size = mid.size, m.bao.group_outboard_size(3 * MIB, 4)
        assert mid.size <= old
    good = [entries[0], entries[2]] if case == "finished" else entries
    _finish(s, good)
    for e in good:
        e.check((case, e.ln))
    if case == "above the capacity":
        assert bool((mid.buf[mid.size:] == 0xA5).all().item())
    # ... and a session the many-call has finished is finished for both calls
    e = good[-1]
    rc, _ = _raw(m, ctx, _args([e]))
    assert rc == m.B3W_E_BAD_ARGUMENT and "entry 0" in ctx.last_error() and "finished" in ctx.last_error()
    assert L.b3w_bao_stream_open_finish(e.se._h, e.tail_ptr, e.tail.numel(), e.ob_ptr, e.size, e.root.data_ptr(), 0, None) == m.B3W_E_BAD_ARGUMENT
    assert "finished" in ctx.last_error()
    torch.cuda.synchronize()
    e.check((case, "after the refused second finishes"))
    for e in entries:
        e.se.close()
    for k in reversed(keep):
        k.close()


def test_no_entry_is_no_launch_and_needs_no_array():
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    assert m.lib().b3w_bao_stream_open_finish_many(ctx.handle, None, None, None, None, None, None, 0, None, None) == m.B3W_OK
    assert m.bao.open_finish_many([]) == []


def test_twelve_calls_in_flight_on_two_streams_outlast_the_staging_ring():
    import torch
    s = _setup()
    m = s["m"]
    files = [LENS.index(2049 * K + 3), LENS.index(3 * MIB + 5), LENS.index(MIB + 1), LENS.index(1)]
    cur = torch.cuda.current_stream()
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    calls = [[_entry(s, f, MIXED[(c + i) % len(MIXED)], ob_shift=8 * ((c + i) & 1)) for i, f in enumerate(files)] for c in range(12)]
    for st in sides:
        st.wait_stream(cur)                                                    # (the arena, the references and the fills come first)
    for c, entries in enumerate(calls):                                        # no synchronise in here: 12 tables, 8 staging slots
        st = sides[c & 1].cuda_stream
        _push_all(m, entries, stream=st)
        _finish(s, entries, stream=st)
    for st in sides:
        cur.wait_stream(st)
    torch.cuda.synchronize()
    for c, entries in enumerate(calls):
        for e in entries:
            e.check((c, e.g, e.ln))
            e.se.close()


@pytest.mark.parametrize("g", [4, 6])
def test_forty_rounds_of_fresh_sessions_agree_with_the_batch_call(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    lens = [3 * MIB + 5, MIB + 1, 2 * MIB, 5 * MIB + 5]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(160 + g)
    for rep in range(40):
        rows = (1, 2, 3, 40)[rep % 4]
        d_file = torch.randint(0, 256, (max(lens),), dtype=torch.uint8, device="cuda", generator=gen)
        want = {ln: _batch_outboard(m, ctx, d_file[:ln], g) for ln in lens[:rows]}
        entries = [_Entry(m, ctx, d_file[:lens[i % 4]], g, want[lens[i % 4]], ob_shift=8 * (i & 1)) for i in range(rows)]
        _push_all(m, entries)
        _finish(s, entries)
        for e in entries:
            e.check((g, rep, e.ln))
            e.se.close()


def test_the_python_call_equals_finish_on_twin_sessions():
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    gs = [MIXED[(f + 1) % len(MIXED)] for f in range(len(LENS))]
    twins = [[m.bao.StreamOutboardOpen(ctx, ln + MIB, gs[f]) for f, ln in enumerate(LENS)] for _ in range(2)]
    for group in twins:
        live = [f for f, ln in enumerate(LENS) if ln >= MIB]
        m.bao.push_many([group[f] for f in live], [0] * len(live), [_data(s, f)[:LENS[f] // MIB * MIB] for f in live])
    tails = [_data(s, f)[ln // MIB * MIB:] if ln % MIB else None for f, ln in enumerate(LENS)]
    got = m.bao.open_finish_many(twins[0], tails)
    assert len(got) == len(LENS)
    for f, ln in enumerate(LENS):
        one, want = twins[1][f].finish(tails[f]), _ref(s, f, gs[f])
        assert got[f]["length"] == one["length"] == ln and twins[0][f].length == ln
        assert set(got[f]) == set(one)
        assert torch.equal(got[f]["outboards"], one["outboards"]) and torch.equal(got[f]["roots"], one["roots"]), (gs[f], ln)
        assert list(got[f]["ob_first"]) == list(one["ob_first"])
        assert torch.equal(got[f]["outboards"], want["outboards"]) and torch.equal(got[f]["roots"], want["roots"]), (gs[f], ln, "the batch call")
        assert got[f]["outboards"].shape == one["outboards"].shape and got[f]["roots"].shape == one["roots"].shape
    with pytest.raises(m.B3WError, match="entry 0.*finished"):                 # atomically: the refusal names the entry
        m.bao.open_finish_many(twins[0][:2])
    with pytest.raises(m.B3WError, match="tails"):
        m.bao.open_finish_many(twins[0][:2], [None])
    for group in twins:
        for se in group:
            se.close()


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
def test_the_helper_streams_sources_of_unknown_length_through_three_lanes(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    window = 2 * MIB
    fs = [LENS.index(ln) for ln in (5 * MIB + 5, 3 * MIB + 5, 2049 * K + 3, 17 * MIB + 5, 0, 2 * MIB, MIB)]

    def sources():
        return [io.BytesIO(_host(s, fs[0]).tobytes()), _host(s, fs[1]).tobytes(), _host(s, fs[2]), _ShortReads(_host(s, fs[3]), 1000003),
                b"", io.BytesIO(_host(s, fs[5]).tobytes()), io.BytesIO(_host(s, fs[6]).tobytes())]
    assert LENS[fs[5]] % window == 0                                           # (it ends exactly on a window's last byte)
    caps = [8 * MIB, LENS[fs[1]], 4 * MIB, LENS[fs[3]], 0, LENS[fs[5]], 3 * MIB]
    for ring in (2, 1, 3):
        got = m.bao.outboard_stream_open_many(ctx, sources(), caps, window, g, lanes=3, ring=ring)
        assert len(got) == len(fs)
        for i, f in enumerate(fs):
            want = _ref(s, f, g)
            assert got[i]["length"] == LENS[f], (g, ring, i)
            assert torch.equal(got[i]["outboards"], want["outboards"]) and torch.equal(got[i]["roots"], want["roots"]), (g, ring, LENS[f])
            assert list(got[i]["ob_first"]) == list(want["ob_first"])
    # a source that yields more than its capacity raises, and the current stream is none the worse for it
    over = list(caps)
    over[3] = LENS[fs[3]] - 1
    with pytest.raises(m.B3WError, match="source 3 yields more than its capacity"):
        m.bao.outboard_stream_open_many(ctx, sources(), over, window, g, lanes=3)
    f = fs[0]
    again = _batch_outboard(m, ctx, _data(s, f), g)                            # an unrelated call on the current stream
    assert torch.equal(again["outboards"], _ref(s, f, g)["outboards"]) and torch.equal(again["roots"], _ref(s, f, g)["roots"])
    one = m.bao.outboard_stream_open_many(ctx, [_host(s, f)], [LENS[f]], MIB, g, lanes=3)   # (more lanes than files)
    assert one[0]["length"] == LENS[f] and torch.equal(one[0]["outboards"], _ref(s, f, g)["outboards"])


def test_the_helpers_device_memory_does_not_grow_with_the_number_of_files_beyond_the_results():
    """The helper makes the slabs (ring x lanes x window_bytes) once, a staging and a scratch per OPEN lane, dropped when the file
    is finished, and per file the outboard and the 32-byte root it returns.  So the peak of max_memory_allocated above the start for
    12 equal files exceeds the peak for 6 by exactly the six added outboards and roots, each rounded up to the allocator's 512
    bytes (every one of these is a small allocation, which the caching allocator splits exactly).  A helper that kept every
    session's staging and scratch until the end would exceed it by six of those as well (27 648 bytes more).
    Measured on an MI355X: 6 files 6 329 856 bytes, 12 files 6 354 432 bytes, the difference 24 576 = 6 x (3 584 + 512)."""
    import torch
    s = _setup()
    m, ctx, L = s["m"], s["ctx"], s["m"].lib()
    g, ln, capacity, window = 6, 3 * MIB + 5, 4 * MIB, MIB
    data = _host(s, LENS.index(ln)).tobytes()
    want = _ref(s, LENS.index(ln), g)

    def up(x):
        return -(-x // 512) * 512
    m.bao.outboard_stream_open_many(ctx, [data] * 3, [capacity] * 3, window, g, lanes=3)   # (warm: streams, the context's staging slots)
    rise = {}
    for n in (6, 12):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        got = m.bao.outboard_stream_open_many(ctx, [io.BytesIO(data) for _ in range(n)], [capacity] * n, window, g, lanes=3)
        torch.cuda.synchronize()
        rise[n] = torch.cuda.max_memory_allocated() - before
        assert all(torch.equal(r["outboards"], want["outboards"]) and torch.equal(r["roots"], want["roots"]) for r in got)
        del got
    result = up(m.bao.group_outboard_size(ln, g)) + up(32)
    session = up(L.b3w_bao_stream_open_staging_bytes(capacity, g)) + up(L.b3w_bao_stream_open_scratch_bytes(capacity))
    print(f"outboard_stream_open_many, lanes 3, files of {ln} bytes at g = {g}: max_memory_allocated rose by {rise[6]} for 6 files and {rise[12]} for 12; "
          f"a result is {result} bytes, a session's staging and scratch {session}")
    assert rise[12] - rise[6] == 6 * result, (rise, result)
    assert rise[6] >= 2 * 3 * window + 3 * session + 6 * result
