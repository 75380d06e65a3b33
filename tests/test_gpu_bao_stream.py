"""Outboards and verification of files streamed in windows (bao.StreamOutboard / StreamVerify / outboard_stream / verify_stream,
b3w_bao_stream_*): whatever the window size, the order of the windows and the streams they come on, a session leaves byte for byte
what the batch calls leave for the same file as a batch of one; a window's unit statuses are final with its push; repeated sessions
agree; a refused call launches nothing and leaves the session usable; the helpers stream from host memory through a ring whose
device memory does not grow with the file."""
import ctypes
import io

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
from test_gpu_bao_batch import _arena, _file

pytestmark = pytest.mark.gpu

GS = [0, 1, 4, 6]
K = 1024
MIB = 1 << 20
NONE = (1 << 64) - 1
LENS = [0, 1, K, K + 1, 64 * K, 65 * K, 1 << 20, (1 << 20) + 1, 2049 * K + 3, 3 << 20, (5 << 20) + 5]
TAMPERED = [2049 * K + 3, (5 << 20) + 5]

_state = {}


def _setup():
    """one context, one arena of every length on the device and, per group_log, the batch calls' outboard and root of every file as a
    batch of one: made once, shared, never written to"""
    if not _state:
        import torch
        m = T.pkg()
        arena, offsets = _arena(LENS, seed=12)
        _state.update(m=m, ctx=m.Context("nova_vesta", 0), arena=arena, offsets=offsets, d_arena=torch.from_numpy(arena).cuda(), ref={})
    return _state


def _data(s, f):
    """file f on the device (a view of the arena: 16-byte aligned starts)"""
    a = int(s["offsets"][f])
    return s["d_arena"][a:a + LENS[f]]


def _batch_outboard(m, ctx, d_file, g):
    n = d_file.numel()
    return m.bao.outboard_batch(ctx, d_file, [0], [n]) if g == 0 else m.bao.outboard_groups_batch(ctx, d_file, [0], [n], g)


def _ref(s, f, g):
    if (f, g) not in s["ref"]:
        s["ref"][f, g] = _batch_outboard(s["m"], s["ctx"], _data(s, f), g)
    return s["ref"][f, g]


def _push_all(session, d_file, window, order):
    """every window of the file (window = 0: the whole file as one) in `order`; leaves the current stream behind all of them"""
    import torch
    m = T.pkg()
    n = d_file.numel()
    wins = m.bao.windows(n, window) if window else ([(0, n)] if n else [])
    if order == "ascending":
        for off, nb in wins:
            session.push(off, d_file[off:off + nb])
    elif order == "descending":
        for off, nb in reversed(wins):
            session.push(off, d_file[off:off + nb])
    else:                                                                      # odd windows on one stream, even ones on another
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


ORDERS = ["ascending", "descending", "two streams"]


@pytest.mark.parametrize("g", GS)
def test_outboards_equal_the_batch_calls(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    for f, ln in enumerate(LENS):
        want = _ref(s, f, g)
        for window in (MIB, 2 * MIB, 0):
            for order in ORDERS:
                so = m.bao.StreamOutboard(ctx, ln, g)
                so.outboards.fill_(0xA5)
                so.roots.fill_(-1)
                _push_all(so, _data(s, f), window, order)
                got = so.finish()
                assert torch.equal(got["outboards"], want["outboards"]), (g, ln, window, order)
                assert torch.equal(got["roots"], want["roots"]), (g, ln, window, order)
                assert list(got["ob_first"]) == list(want["ob_first"])
                so.close()


@pytest.mark.parametrize("g", [0, 4])
def test_a_window_off_a_16_byte_boundary(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    f = LENS.index((5 << 20) + 5)
    ln = LENS[f]
    shifted = torch.empty(ln + 16, dtype=torch.uint8, device="cuda")
    shifted[3:3 + ln] = _data(s, f)
    d_file = shifted[3:3 + ln]
    assert d_file.data_ptr() % 16 == 3
    so = m.bao.StreamOutboard(ctx, ln, g)
    so.push(0, _data(s, f)[:2 * MIB])
    so.push(2 * MIB, d_file[2 * MIB:4 * MIB])                                  # this window alone is read off the boundary
    so.push(4 * MIB, _data(s, f)[4 * MIB:])
    got, want = so.finish(), _ref(s, f, g)
    assert torch.equal(got["outboards"], want["outboards"]) and torch.equal(got["roots"], want["roots"])
    sv = m.bao.StreamVerify(ctx, ln, want["outboards"], want["roots"], g)
    _push_all(sv, d_file, MIB, "descending")
    out = sv.finish()
    assert not out["unit_status"].any().item() and int(out["file_status"].item()) == 0 and int(out["first_bad"].item()) == -1


@pytest.mark.parametrize("g", [0, 4])
def test_two_storeys_1026_tiles(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    ln = (1 << 30) + (1 << 20) + 5
    gen = torch.Generator(device="cuda")
    gen.manual_seed(256)
    d_file = torch.randint(0, 256, (ln,), dtype=torch.uint8, device="cuda", generator=gen)
    want = _batch_outboard(m, ctx, d_file, g)
    so = m.bao.StreamOutboard(ctx, ln, g)
    _push_all(so, d_file, 256 * MIB, "descending")
    got = so.finish()
    assert torch.equal(got["outboards"], want["outboards"]) and torch.equal(got["roots"], want["roots"])
    so.close()
    sv = m.bao.StreamVerify(ctx, ln, want["outboards"], want["roots"], g)
    _push_all(sv, d_file, 256 * MIB, "two streams")
    out = sv.finish()
    ref = m.bao.verify_batch(ctx, d_file, [0], [ln], want["outboards"], want["roots"], g)
    for k in ("unit_status", "file_status", "first_bad"):
        assert torch.equal(out[k], ref[k]), (g, k)
    assert not out["unit_status"].any().item() and int(out["file_status"].item()) == 0 and int(out["first_bad"].item()) == -1
    sv.close()


@pytest.mark.parametrize("g", GS)
def test_clean_files_verify(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    for f, ln in enumerate(LENS):
        ob = _ref(s, f, g)
        ref = m.bao.verify_batch(ctx, _data(s, f), [0], [ln], ob["outboards"], ob["roots"], g)
        for window, order in ((MIB, "ascending"), (2 * MIB, "descending"), (0, "ascending"), (MIB, "two streams")):
            sv = m.bao.StreamVerify(ctx, ln, ob["outboards"], ob["roots"], g)
            sv.unit_status.fill_(0xEE)
            _push_all(sv, _data(s, f), window, order)
            out = sv.finish()
            assert out["unit_status"].numel() == (m.bao.num_chunks(ln) + (1 << g) - 1) >> g
            assert not out["unit_status"].any().item(), (g, ln, window, order)
            assert int(out["file_status"].item()) == 0 and int(out["first_bad"].cpu().numpy().view(np.uint64)[0]) == NONE, (g, ln, window, order)
            for k in ("unit_status", "file_status", "first_bad"):
                assert torch.equal(out[k], ref[k])
            assert list(out["unit_first"]) == list(ref["unit_first"])
            sv.close()


@pytest.mark.parametrize("g", [0, 4])
@pytest.mark.parametrize("ln", TAMPERED)
def test_tampered_files_against_the_batch_call_and_the_host_decoder(ln, g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    f = LENS.index(ln)
    ob = _ref(s, f, g)
    T1 = 1024 >> g                                                             # units to a tile
    nu = (m.bao.num_chunks(ln) + (1 << g) - 1) >> g
    spans = GR.node_spans(nu)
    inside, above = spans.index((T1, T1 // 2)), 1                              # a node of the second tile; the root's left child
    assert spans[above][1] > T1
    scenarios = {"chunk": ("data", MIB + 5000), "node inside a tile": ("ob", 8 + 64 * inside + 11), "node above the tiles": ("ob", 8 + 64 * above + 43),
                 "root": ("root", 5), "header": ("ob", 2)}
    for name, (what, at) in scenarios.items():
        d_file, d_ob, d_root = _data(s, f).clone(), ob["outboards"].clone(), ob["roots"].clone()
        if what == "data":
            d_file[at] ^= 1
        elif what == "ob":
            d_ob[at] ^= 1
        else:
            d_root[0, at] ^= 0x10000
        ref = m.bao.verify_batch(ctx, d_file, [0], [ln], d_ob, d_root, g)
        sv = m.bao.StreamVerify(ctx, ln, d_ob, d_root, g)
        sv.unit_status.fill_(0xEE)
        sv.push(0, d_file[:MIB])
        if name == "chunk":                                                    # the first window is clean: known before the bad one is pushed
            first = sv.unit_status[:T1].cpu().numpy()
            assert not first.any(), (g, ln)
            assert bool((sv.unit_status[T1:] == 0xEE).all().item())
        for off, nb in m.bao.windows(ln, MIB)[1:]:
            sv.push(off, d_file[off:off + nb])
        out = sv.finish()
        for k in ("unit_status", "file_status", "first_bad"):
            assert torch.equal(out[k], ref[k]), (g, ln, name, k)
        st = out["unit_status"].cpu().numpy()
        assert st.any(), (g, ln, name)
        hs, hfs, hfb = m.bao.verify_host(d_file.cpu().numpy().tobytes(), d_ob.cpu().numpy().tobytes(), d_root.cpu().numpy().view(np.uint32)[0], g)
        assert np.array_equal(hs, st), (g, ln, name)
        assert (hfs, hfb) == (int(out["file_status"].item()), int(out["first_bad"].cpu().numpy().view(np.uint64)[0])), (g, ln, name)
        if name == "chunk":
            bad = (MIB + 5000) // 1024 >> g
            assert list(np.nonzero(st)[0]) == [bad] and st[bad] == 1
        sv.close()


@pytest.mark.parametrize("g", [4, 6])
def test_forty_sessions_agree(g):
    """equality over repeated sessions: what showed the level loop's missing LDS wait in the group outboard kernels"""
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    f = LENS.index(3 << 20)
    want = _ref(s, f, g)
    for k in range(40):
        so = m.bao.StreamOutboard(ctx, LENS[f], g)
        _push_all(so, _data(s, f), MIB, ORDERS[k % 3])
        got = so.finish()
        assert torch.equal(got["outboards"], want["outboards"]) and torch.equal(got["roots"], want["roots"]), (g, k)
        so.close()
        sv = m.bao.StreamVerify(ctx, LENS[f], want["outboards"], want["roots"], g)
        _push_all(sv, _data(s, f), MIB, ORDERS[k % 3])
        out = sv.finish()
        assert not out["unit_status"].any().item() and int(out["file_status"].item()) == 0 and int(out["first_bad"].item()) == -1, (g, k)
        sv.close()


def _refused(m, ctx, rc, word):
    assert rc == m.B3W_E_BAD_ARGUMENT
    assert word in ctx.last_error(), ctx.last_error()


@pytest.mark.parametrize("kind", ["outboard", "verify"])
def test_refusals_launch_nothing_and_leave_the_session_usable(kind):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    L = m.lib()
    g = 4
    f = LENS.index((5 << 20) + 5)
    ln, d_file, want = LENS[f], _data(s, f), _ref(s, f, g)
    cur = torch.cuda.current_stream().cuda_stream
    if kind == "outboard":
        se = m.bao.StreamOutboard(ctx, ln, g)
        outputs = [se.outboards, se.roots, se.scratch]
    else:
        se = m.bao.StreamVerify(ctx, ln, want["outboards"], want["roots"], g)
        outputs = [se.unit_status]
    for t in outputs:
        t.fill_(0x5A)
    if kind == "verify":                                                       # (begin has written these: they stay as it left them)
        outputs += [se.scratch, se.file_status, se.first_bad]
    torch.cuda.synchronize()
    snapshot = [t.clone() for t in outputs]
    h, base = se._h, d_file.data_ptr()
    push, finish = L.b3w_bao_stream_push, L.b3w_bao_stream_finish
    _refused(m, ctx, push(h, 512 * K, base + 512 * K, MIB, cur), "multiple of 1 MiB")           # an offset inside a tile
    _refused(m, ctx, push(h, MIB, base + MIB, MIB + 512 * K, cur), "whole tiles")                # not whole tiles, not the file's end
    _refused(m, ctx, push(h, MIB, base + MIB, 0, cur), "empty")
    _refused(m, ctx, push(h, 5 * MIB, base + 5 * MIB, 6, cur), "past")                           # one byte past the end
    _refused(m, ctx, push(h, 6 * MIB, base, MIB, cur), "past")
    _refused(m, ctx, push(h, 0, None, MIB, cur), "null")
    _refused(m, ctx, finish(h, cur), "not been pushed")                                          # every tile is missing
    torch.cuda.synchronize()
    now = outputs
    assert all(torch.equal(a, b) for a, b in zip(now, snapshot)), "a refused call wrote something"
    # ... a tile pushed twice, alone or inside a larger window, and finish while one is missing: refused, with part of the file pushed
    se.push(MIB, d_file[MIB:3 * MIB])
    _refused(m, ctx, push(h, 2 * MIB, base + 2 * MIB, MIB, cur), "pushed before")
    _refused(m, ctx, push(h, 0, base, 2 * MIB, cur), "pushed before")
    se.push(0, d_file[:MIB])
    se.push(4 * MIB, d_file[4 * MIB:])
    _refused(m, ctx, finish(h, cur), "1 of 6 tiles")
    se.push(3 * MIB, d_file[3 * MIB:4 * MIB])
    out = se.finish()                                                                            # the session finishes correctly after all that
    if kind == "outboard":
        assert torch.equal(out["outboards"], want["outboards"]) and torch.equal(out["roots"], want["roots"])
    else:
        assert not out["unit_status"].any().item() and int(out["file_status"].item()) == 0 and int(out["first_bad"].item()) == -1
    done = [t.clone() for t in now]
    _refused(m, ctx, push(h, 0, base, MIB, cur), "finished")                                     # a push, and a finish, after finish
    _refused(m, ctx, finish(h, cur), "finished")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(now, done))
    se.close()
    # begin: a group_log above 6, a length past 2^30 chunks, a small scratch — no session comes back
    ob, root, scr = want["outboards"].data_ptr(), want["roots"].data_ptr(), torch.empty(1024, dtype=torch.uint8, device="cuda")
    st8, fs, fb = torch.empty(512, dtype=torch.uint8, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")

    def begin(length, gl, scratch_bytes):
        hh = ctypes.c_void_p()
        if kind == "outboard":
            rc = L.b3w_bao_stream_outboard_begin(ctx.handle, length, gl, ob, root, scr.data_ptr(), scratch_bytes, ctypes.byref(hh))
        else:
            rc = L.b3w_bao_stream_verify_begin(ctx.handle, length, gl, ob, root, st8.data_ptr(), fs.data_ptr(), fb.data_ptr(), scr.data_ptr(), scratch_bytes,
                                               cur, ctypes.byref(hh))
        assert not hh
        return rc
    _refused(m, ctx, begin(ln, 7, 1024), "group_log")
    _refused(m, ctx, begin((1 << 40) + 1025, 0, 1 << 62), "2^30 chunks")
    _refused(m, ctx, begin(ln, g, L.b3w_bao_stream_scratch_bytes(ln, 0 if kind == "outboard" else 1) - 1), "scratch")
    with pytest.raises(m.B3WError):
        m.bao.StreamOutboard(ctx, ln, 7)
    # an empty file takes no push, and finishes
    se = m.bao.StreamOutboard(ctx, 0, g) if kind == "outboard" else m.bao.StreamVerify(ctx, 0, _ref(s, 0, g)["outboards"], _ref(s, 0, g)["roots"], g)
    _refused(m, ctx, push(se._h, 0, base, MIB, cur), "past")
    _refused(m, ctx, push(se._h, 0, base, 0, cur), "empty")
    out = se.finish()
    if kind == "outboard":
        assert torch.equal(out["outboards"], _ref(s, 0, g)["outboards"]) and torch.equal(out["roots"], _ref(s, 0, g)["roots"])
    else:
        assert out["unit_status"].cpu().tolist() == [0] and int(out["file_status"].item()) == 0 and int(out["first_bad"].item()) == -1
    se.close()


class _Reader:
    """readinto in short, uneven reads, as a socket gives them"""

    def __init__(self, data):
        self.raw, self.k = io.BytesIO(data), 0

    def readinto(self, view):
        self.k += 1
        return self.raw.readinto(view[:(300 * K + 7) * (1 + self.k % 3)])


@pytest.mark.parametrize("g", [0, 4])
def test_helpers_stream_from_host_memory(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    f = LENS.index((5 << 20) + 5)
    ln, want = LENS[f], _ref(s, f, g)
    host = np.frombuffer(_file(s["arena"], s["offsets"], LENS, f), dtype=np.uint8)
    pinned = torch.from_numpy(host.copy()).pin_memory()
    for source in (lambda: host, lambda: _Reader(host.tobytes()), lambda: host.tobytes(), lambda: pinned):
        got = m.bao.outboard_stream(ctx, source(), ln, MIB, g, ring=2)
        assert torch.equal(got["outboards"], want["outboards"]) and torch.equal(got["roots"], want["roots"])
        out = m.bao.verify_stream(ctx, source(), ln, want["outboards"], want["roots"], MIB, g, ring=2)
        ref = m.bao.verify_batch(ctx, _data(s, f), [0], [ln], want["outboards"], want["roots"], g)
        for k in ("unit_status", "file_status", "first_bad"):
            assert torch.equal(out[k], ref[k]), (g, k)
    # a bad byte in the host's copy is found where it lies; a short source is refused
    dirty = host.copy()
    dirty[3 * MIB + 77] ^= 4
    out = m.bao.verify_stream(ctx, dirty, ln, want["outboards"], want["roots"], 2 * MIB, g, ring=3)
    st = out["unit_status"].cpu().numpy()
    assert list(np.nonzero(st)[0]) == [3 * 1024 >> g] and int(out["file_status"].item()) == 1 and int(out["first_bad"].item()) == 3 * 1024 >> g
    with pytest.raises(m.B3WError):
        m.bao.outboard_stream(ctx, host[:ln - 1], ln, MIB, g)
    torch.cuda.synchronize()
    # an empty file, and a one-byte one
    for f2 in (LENS.index(0), LENS.index(1)):
        got = m.bao.outboard_stream(ctx, _file(s["arena"], s["offsets"], LENS, f2), LENS[f2], MIB, g)
        assert torch.equal(got["outboards"], _ref(s, f2, g)["outboards"]) and torch.equal(got["roots"], _ref(s, f2, g)["roots"])


def test_the_helpers_device_memory_does_not_grow_with_the_file():
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    ln, window, ring = 8 * MIB, MIB, 2
    host = np.random.default_rng(8).integers(0, 256, ln, dtype=np.uint8)
    ob_bytes = m.bao.outboard_size(ln)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = m.bao.outboard_stream(ctx, host, ln, window, 0, ring=ring)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    bound = ring * window + ob_bytes + m.bao.stream_scratch_bytes(ln, m.bao.STREAM_OUTBOARD) + 64 * K
    print(f"outboard_stream of {ln} bytes: device memory rose by {rise}, bound {bound}")
    assert rise < bound < ln
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = m.bao.verify_stream(ctx, host, ln, got["outboards"], got["roots"], window, 0, ring=ring)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    bound = ring * window + m.bao.stream_scratch_bytes(ln, m.bao.STREAM_VERIFY) + 8 * K + 12 + 64 * K          # (the outboard is the caller's; a status a chunk)
    print(f"verify_stream of {ln} bytes: device memory rose by {rise}, bound {bound}")
    assert rise < bound < ln
    assert not out["unit_status"].any().item() and int(out["file_status"].item()) == 0
    d_host = torch.from_numpy(host).cuda()
    want = m.bao.outboard_batch(ctx, d_host, [0], [ln])
    assert torch.equal(got["outboards"], want["outboards"]) and torch.equal(got["roots"], want["roots"])
