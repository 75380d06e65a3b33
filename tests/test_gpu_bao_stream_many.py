"""Many stream sessions pushed and finished in one launch (bao.push_many / finish_many / outboard_stream_many / verify_stream_many,
b3w_bao_stream_push_many / _finish_many): whatever the sessions, their group sizes and the entries' shapes, the calls leave byte for
byte what the per-session calls and the batch calls leave; tampered sessions do not touch their clean neighbours; a refused call
launches nothing and changes no session; more calls in flight than staging slots; the helpers hand lanes on and their device memory
does not grow with the files."""
import io

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
from test_gpu_bao_batch import _file
from test_gpu_bao_stream import GS, K, LENS, MIB, NONE, TAMPERED, _batch_outboard, _data, _ref, _setup

pytestmark = pytest.mark.gpu

KEYS = ("unit_status", "file_status", "first_bad")


def _push_rounds(m, sessions, d_files, window=MIB, stream=0):
    """round r: window r of every session that has one, in ONE push_many"""
    wins = [m.bao.windows(d.numel(), window) for d in d_files]
    for r in range(max((len(w) for w in wins), default=0)):
        live = [i for i, w in enumerate(wins) if r < len(w)]
        m.bao.push_many([sessions[i] for i in live], [wins[i][r][0] for i in live],
                        [d_files[i][wins[i][r][0]:wins[i][r][0] + wins[i][r][1]] for i in live], stream=stream)


def _same_outboard(got, want):
    import torch
    return torch.equal(got["outboards"], want["outboards"]) and torch.equal(got["roots"], want["roots"]) and list(got["ob_first"]) == list(want["ob_first"])


def _clean_verify(s, f, g):
    """verify_batch of file f alone against its own outboard: made once"""
    key = ("clean", f, g)
    if key not in s["ref"]:
        ob = _ref(s, f, g)
        s["ref"][key] = s["m"].bao.verify_batch(s["ctx"], _data(s, f), [0], [LENS[f]], ob["outboards"], ob["roots"], g)
    return s["ref"][key]


@pytest.mark.parametrize("g", GS + ["mixed"])
def test_every_length_as_a_session_at_once(g):
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    gs = [GS[f % len(GS)] for f in range(len(LENS))] if g == "mixed" else [g] * len(LENS)
    sessions = [m.bao.StreamOutboard(ctx, ln, gs[f]) for f, ln in enumerate(LENS)]
    for se in sessions:
        se.outboards.fill_(0xA5)
        se.roots.fill_(-1)
    _push_rounds(m, sessions, [_data(s, f) for f in range(len(LENS))])
    got = m.bao.finish_many(sessions)
    for f, ln in enumerate(LENS):
        assert _same_outboard(got[f], _ref(s, f, gs[f])), (g, ln, "the batch call")
        one = m.bao.StreamOutboard(ctx, ln, gs[f])                            # the per-session route
        for off, nb in m.bao.windows(ln, MIB):
            one.push(off, _data(s, f)[off:off + nb])
        assert _same_outboard(got[f], one.finish()), (g, ln, "push / finish")
        one.close()
    for se in sessions:
        se.close()


@pytest.mark.parametrize("g", [0, 4])
def test_a_session_twice_in_a_call_descending_off_the_16_byte_boundary(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    f = LENS.index((5 << 20) + 5)
    ln, want = LENS[f], _ref(s, f, g)
    copies = {}
    for shift in (1, 8):
        buf = torch.empty(ln + 32, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[shift:shift + ln] = _data(s, f)
        copies[shift] = buf[shift:shift + ln]
    so = m.bao.StreamOutboard(ctx, ln, g)
    sv = m.bao.StreamVerify(ctx, ln, want["outboards"], want["roots"], g)
    sv.unit_status.fill_(0xEE)
    for se in (so, sv):
        # two calls, each with the one session twice: windows [4 MiB, end) and [2, 4) MiB, then [1, 2) and [0, 1)
        for (o1, e1), (o8, e8) in (((4 * MIB, ln), (2 * MIB, 4 * MIB)), ((MIB, 2 * MIB), (0, MIB))):
            w1, w8 = copies[1][o1:e1], copies[8][o8:e8]
            assert w1.data_ptr() % 16 == 1 and w8.data_ptr() % 16 == 8
            m.bao.push_many([se, se], [o1, o8], [w1, w8])
    got, out = m.bao.finish_many([so])[0], m.bao.finish_many([sv])[0]
    assert _same_outboard(got, want)
    ref = _clean_verify(s, f, g)
    for k in KEYS:
        assert torch.equal(out[k], ref[k]), (g, k)
    so.close()
    sv.close()


@pytest.mark.parametrize("g", GS)
def test_clean_files_verify(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    sessions = [m.bao.StreamVerify(ctx, ln, _ref(s, f, g)["outboards"], _ref(s, f, g)["roots"], g) for f, ln in enumerate(LENS)]
    for se in sessions:
        se.unit_status.fill_(0xEE)
    _push_rounds(m, sessions, [_data(s, f) for f in range(len(LENS))])
    outs = m.bao.finish_many(sessions)
    for f, ln in enumerate(LENS):
        out, ref = outs[f], _clean_verify(s, f, g)
        assert out["unit_status"].numel() == (m.bao.num_chunks(ln) + (1 << g) - 1) >> g
        assert not out["unit_status"].any().item(), (g, ln)
        assert int(out["file_status"].item()) == 0 and int(out["first_bad"].cpu().numpy().view(np.uint64)[0]) == NONE, (g, ln)
        for k in KEYS:
            assert torch.equal(out[k], ref[k]), (g, ln, k)
        assert list(out["unit_first"]) == list(ref["unit_first"])
    for se in sessions:
        se.close()


@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("what", ["chunk", "node", "root", "header"])
def test_tampered_sessions_beside_clean_ones(what, g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    T1 = 1024 >> g                                                             # units to a tile
    sessions, d_files, refs, hosts = [], [], [], []
    for ln in TAMPERED:                                                        # the tampered sessions first, then every length clean
        f = LENS.index(ln)
        ob = _ref(s, f, g)
        d_file, d_ob, d_root = _data(s, f).clone(), ob["outboards"].clone(), ob["roots"].clone()
        nu = (m.bao.num_chunks(ln) + (1 << g) - 1) >> g
        if what == "chunk":
            d_file[MIB + 5000] ^= 1
        elif what == "node":                                                   # a node of the second tile in one file, the root's left child in the other
            node = GR.node_spans(nu).index((T1, T1 // 2)) if ln == TAMPERED[0] else 1
            d_ob[8 + 64 * node + 11] ^= 1
        elif what == "root":
            d_root[0, 5] ^= 0x10000
        else:
            d_ob[2] ^= 1
        refs.append(m.bao.verify_batch(ctx, d_file, [0], [ln], d_ob, d_root, g))
        hosts.append(m.bao.verify_host(d_file.cpu().numpy().tobytes(), d_ob.cpu().numpy().tobytes(), d_root.cpu().numpy().view(np.uint32)[0], g))
        sessions.append(m.bao.StreamVerify(ctx, ln, d_ob, d_root, g))
        d_files.append(d_file)
    for f, ln in enumerate(LENS):
        ob = _ref(s, f, g)
        sessions.append(m.bao.StreamVerify(ctx, ln, ob["outboards"], ob["roots"], g))
        d_files.append(_data(s, f))
        refs.append(_clean_verify(s, f, g))
    for se in sessions:
        se.unit_status.fill_(0xEE)
    _push_rounds(m, sessions, d_files)
    outs = m.bao.finish_many(sessions)
    for i, (out, ref) in enumerate(zip(outs, refs)):
        for k in KEYS:
            assert torch.equal(out[k], ref[k]), (g, what, i, k)
    for i in range(len(TAMPERED)):
        st = outs[i]["unit_status"].cpu().numpy()
        hs, hfs, hfb = hosts[i]
        assert st.any() and np.array_equal(hs, st), (g, what, i)
        assert (hfs, hfb) == (int(outs[i]["file_status"].item()), int(outs[i]["first_bad"].cpu().numpy().view(np.uint64)[0])), (g, what, i)
        if what == "chunk":
            bad = (MIB + 5000) // 1024 >> g
            assert list(np.nonzero(st)[0]) == [bad] and st[bad] == 1
    for out in outs[len(TAMPERED):]:                                           # the clean sessions: untouched by their neighbours
        assert not out["unit_status"].any().item() and int(out["file_status"].item()) == 0 and int(out["first_bad"].item()) == -1
    for se in sessions:
        se.close()


@pytest.mark.parametrize("g", [0, 4])
def test_two_storeys_beside_a_small_file(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    ln = (1 << 30) + (1 << 20) + 5                                             # 1 026 tiles: a second merge storey
    gen = torch.Generator(device="cuda")
    gen.manual_seed(256)
    d_big = torch.randint(0, 256, (ln,), dtype=torch.uint8, device="cuda", generator=gen)
    f = LENS.index(3 << 20)
    d_files = [d_big, _data(s, f)]
    wants = [_batch_outboard(m, ctx, d_big, g), _ref(s, f, g)]
    so = [m.bao.StreamOutboard(ctx, d.numel(), g) for d in d_files]
    _push_rounds(m, so, d_files, window=256 * MIB)
    for got, want in zip(m.bao.finish_many(so), wants):
        assert _same_outboard(got, want), g
    sv = [m.bao.StreamVerify(ctx, d.numel(), w["outboards"], w["roots"], g) for d, w in zip(d_files, wants)]
    _push_rounds(m, sv, d_files, window=256 * MIB)
    outs = m.bao.finish_many(sv)
    ref = m.bao.verify_batch(ctx, d_big, [0], [ln], wants[0]["outboards"], wants[0]["roots"], g)
    for k in KEYS:
        assert torch.equal(outs[0][k], ref[k]) and torch.equal(outs[1][k], _clean_verify(s, f, g)[k]), (g, k)
    assert not outs[0]["unit_status"].any().item() and int(outs[0]["file_status"].item()) == 0 and int(outs[0]["first_bad"].item()) == -1
    for se in so + sv:
        se.close()


@pytest.mark.parametrize("g", [4, 6])
def test_forty_rounds_of_fresh_data(g):
    """the store-light instantiations, whose level loops need the LDS wait spelled out: every byte of forty rounds"""
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    lens = [3 << 20, 2049 * K + 3, 65 * K, (1 << 20) + 1]
    offsets = np.cumsum([0] + [(ln + 15) // 16 * 16 for ln in lens])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(40 + g)
    for k in range(40):
        arena = torch.randint(0, 256, (int(offsets[-1]),), dtype=torch.uint8, device="cuda", generator=gen)
        want = m.bao.outboard_groups_batch(ctx, arena, offsets[:-1], lens, g)
        d_files = [arena[int(offsets[i]):int(offsets[i]) + ln] for i, ln in enumerate(lens)]
        so = [m.bao.StreamOutboard(ctx, ln, g) for ln in lens]
        _push_rounds(m, so, d_files)
        for i, got in enumerate(m.bao.finish_many(so)):
            a, b = int(want["ob_first"][i]), int(want["ob_first"][i + 1])
            assert torch.equal(got["outboards"], want["outboards"][a:b]) and torch.equal(got["roots"][0], want["roots"][i]), (g, k, i)
        sv = [m.bao.StreamVerify(ctx, ln, got["outboards"], got["roots"], g) for ln, got in zip(lens, [dict(outboards=x.outboards, roots=x.roots) for x in so])]
        _push_rounds(m, sv, d_files)
        for i, out in enumerate(m.bao.finish_many(sv)):
            assert not out["unit_status"].any().item() and int(out["file_status"].item()) == 0 and int(out["first_bad"].item()) == -1, (g, k, i)
        for se in so + sv:
            se.close()


def _raw_push(m, ctx, sessions, offsets, ptrs, nbytes, stream):
    hs = np.array([se._h.value if se is not None else 0 for se in sessions], dtype=np.uint64)
    off, ptr, nb = (np.array(a, dtype=np.uint64) for a in (offsets, ptrs, nbytes))
    return m.lib().b3w_bao_stream_push_many(ctx.handle, hs.ctypes.data, off.ctypes.data, ptr.ctypes.data, nb.ctypes.data, hs.size, stream)


def _raw_finish(m, ctx, sessions, stream):
    hs = np.array([se._h.value if se is not None else 0 for se in sessions], dtype=np.uint64)
    return m.lib().b3w_bao_stream_finish_many(ctx.handle, hs.ctypes.data, hs.size, stream)


def _refused(m, ctx, rc, *words):
    assert rc == m.B3W_E_BAD_ARGUMENT
    for word in words:
        assert word in ctx.last_error(), ctx.last_error()


def test_nothing_and_nulls_with_a_context():
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    L, cur = m.lib(), torch.cuda.current_stream().cuda_stream
    one = np.zeros(1, dtype=np.uint64)
    assert L.b3w_bao_stream_push_many(ctx.handle, None, None, None, None, 0, cur) == m.B3W_OK
    assert L.b3w_bao_stream_finish_many(ctx.handle, None, 0, cur) == m.B3W_OK
    for hole in range(4):                                                      # one null array among the four
        args = [None if i == hole else one.ctypes.data for i in range(4)]
        _refused(m, ctx, L.b3w_bao_stream_push_many(ctx.handle, *args, 1, cur), "null array")
    _refused(m, ctx, L.b3w_bao_stream_finish_many(ctx.handle, None, 1, cur), "null array")
    _refused(m, ctx, _raw_push(m, ctx, [None], [0], [16], [MIB], cur), "entry 0", "null session")
    _refused(m, ctx, _raw_finish(m, ctx, [None], cur), "entry 0", "null session")
    other = m.Context("nova_vesta", 0)                                         # a session of another context
    se = m.bao.StreamOutboard(other, MIB, 0)
    _refused(m, ctx, _raw_push(m, ctx, [se], [0], [_data(s, LENS.index(1 << 20)).data_ptr()], [MIB], cur), "entry 0", "another context")
    _refused(m, ctx, _raw_finish(m, ctx, [se], cur), "entry 0", "another context")
    se.close()
    other.close()


@pytest.mark.parametrize("bad", ["offset", "pushed before", "named twice", "other kind", "finished", "null window"])
def test_a_refused_call_launches_nothing_and_changes_no_session(bad):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    g = 4
    f = LENS.index((5 << 20) + 5)
    ln, d_file, want = LENS[f], _data(s, f), _ref(s, f, g)
    base, cur = d_file.data_ptr(), torch.cuda.current_stream().cuda_stream
    S = [m.bao.StreamOutboard(ctx, ln, g) for _ in range(5)]
    f1 = LENS.index(1 << 20)
    fin = m.bao.StreamOutboard(ctx, MIB, g)                                    # a finished session of one tile
    fin.push(0, _data(s, f1))
    fin.finish()
    ver = m.bao.StreamVerify(ctx, ln, want["outboards"], want["roots"], g)
    ver.unit_status.fill_(0xA5)
    outputs = [ver.unit_status, fin.outboards, fin.roots]
    for se in S:
        for t in (se.outboards, se.roots, se.scratch):
            t.fill_(0xA5)
            outputs.append(t)
    if bad == "pushed before":
        S[2].push(MIB, d_file[MIB:2 * MIB])
    torch.cuda.synchronize()
    snapshot = [t.clone() for t in outputs]
    # five entries, tile 0 of a session each; the third is the bad one
    third = {"offset": (S[2], 512 * K, base + 512 * K, MIB, "multiple of 1 MiB"), "pushed before": (S[2], MIB, base + MIB, MIB, "pushed before"),
             "named twice": (S[0], 0, base, MIB, "named twice"), "other kind": (ver, 0, base, MIB, "kind"),
             "finished": (fin, 0, _data(s, f1).data_ptr(), MIB, "finished"), "null window": (S[2], 0, 0, MIB, "null")}[bad]
    ses = [S[0], S[1], third[0], S[3], S[4]]
    rc = _raw_push(m, ctx, ses, [0, 0, third[1], 0, 0], [base, base, third[2], base, base], [MIB, MIB, third[3], MIB, MIB], cur)
    _refused(m, ctx, rc, "entry 2", third[4])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outputs, snapshot)), "a refused call wrote something"
    # the same call without the bad entry; had the refused call marked a tile, this one would be refused ("pushed before")
    good = [S[0], S[1], S[3], S[4]]
    assert _raw_push(m, ctx, good, [0] * 4, [base] * 4, [MIB] * 4, cur) == m.B3W_OK, ctx.last_error()
    m.bao.push_many(good, [MIB] * 4, [d_file[MIB:]] * 4)
    todo = [(0, MIB), (2 * MIB, ln)] if bad == "pushed before" else [(0, ln)]
    m.bao.push_many([S[2]] * (len(todo) - 1), [a for a, _ in todo[1:]], [d_file[a:b] for a, b in todo[1:]])
    # finish_many with a session that lacks a tile (S[2]'s first window): refused whole, nobody is finished
    torch.cuda.synchronize()
    snapshot = [t.clone() for t in outputs]
    _refused(m, ctx, _raw_finish(m, ctx, S, cur), "entry 2", "not been pushed")
    _refused(m, ctx, _raw_finish(m, ctx, [S[0], S[1], S[0]], cur), "entry 2", "twice")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outputs, snapshot)), "a refused finish wrote something"
    m.bao.push_many([S[2]], [todo[0][0]], [d_file[todo[0][0]:todo[0][1]]])
    for got in m.bao.finish_many(S):
        assert _same_outboard(got, want), bad
    _refused(m, ctx, _raw_finish(m, ctx, S, cur), "entry 0", "finished")
    for se in S + [fin, ver]:
        se.close()


def test_more_calls_in_flight_than_staging_slots():
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    n_ses, tiles = 16, 8
    lens = [tiles * MIB - (977 * i if i % 3 == 0 else 0) for i in range(n_ses)]   # some end in a ragged tile
    offsets = np.arange(n_ses + 1, dtype=np.uint64) * (tiles * MIB)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    arena = torch.randint(0, 256, (int(offsets[-1]),), dtype=torch.uint8, device="cuda", generator=gen)
    want = {0: m.bao.outboard_batch(ctx, arena, offsets[:-1], lens), 4: m.bao.outboard_groups_batch(ctx, arena, offsets[:-1], lens, 4)}
    gs = [0 if i % 2 == 0 else 4 for i in range(n_ses)]
    so = [m.bao.StreamOutboard(ctx, lens[i], gs[i]) for i in range(n_ses)]
    cur = torch.cuda.current_stream()
    sides = [torch.cuda.Stream() for _ in range(4)]
    for st in sides:
        st.wait_stream(cur)
    for k in range(64):                                                        # call k: tile k // 8 of two sessions; no host synchronise between the calls
        pair, t = (2 * (k % 8), 2 * (k % 8) + 1), k // 8
        wins = [arena[int(offsets[i]) + t * MIB:int(offsets[i]) + min((t + 1) * MIB, lens[i])] for i in pair]
        m.bao.push_many([so[i] for i in pair], [t * MIB] * 2, wins, stream=sides[k % 4].cuda_stream)
    for st in sides:
        cur.wait_stream(st)
    for i, got in enumerate(m.bao.finish_many(so)):
        w = want[gs[i]]
        a, b = int(w["ob_first"][i]), int(w["ob_first"][i + 1])
        assert torch.equal(got["outboards"], w["outboards"][a:b]) and torch.equal(got["roots"][0], w["roots"][i]), i
    for se in so:
        se.close()


class _Reader:
    """readinto in short, uneven reads, as a socket gives them"""

    def __init__(self, data):
        self.raw, self.k = io.BytesIO(data), 0

    def readinto(self, view):
        self.k += 1
        return self.raw.readinto(view[:(300 * K + 7) * (1 + self.k % 3)])


@pytest.mark.parametrize("g", [0, 4])
def test_helpers_hand_lanes_on_over_a_mix_of_sources(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    hosts = [np.frombuffer(_file(s["arena"], s["offsets"], LENS, f), dtype=np.uint8) for f in range(len(LENS))]
    kinds = [lambda h: h, lambda h: _Reader(h.tobytes()), lambda h: h.tobytes(), lambda h: torch.from_numpy(h.copy()).pin_memory()]

    def sources():
        return [kinds[f % 4](h) for f, h in enumerate(hosts)]
    want = m.bao.outboard_batch(ctx, s["d_arena"], s["offsets"], LENS) if g == 0 else m.bao.outboard_groups_batch(ctx, s["d_arena"], s["offsets"], LENS, g)
    got = m.bao.outboard_stream_many(ctx, sources(), LENS, MIB, g, lanes=3, ring=2)
    assert _same_outboard(got, want), g
    ref = m.bao.verify_batch(ctx, s["d_arena"], s["offsets"], LENS, want["outboards"], want["roots"], g)
    out = m.bao.verify_stream_many(ctx, sources(), LENS, want["outboards"], want["roots"], MIB, g, lanes=3, ring=2)
    for k in KEYS:
        assert torch.equal(out[k], ref[k]), (g, k)
    assert list(out["unit_first"]) == list(ref["unit_first"])
    # a bad byte in one host copy is found where it lies, and nowhere else; windows of 2 MiB, a lane more than files left over
    f = LENS.index((5 << 20) + 5)
    dirty = [h for h in hosts]
    dirty[f] = hosts[f].copy()
    dirty[f][3 * MIB + 77] ^= 4
    out = m.bao.verify_stream_many(ctx, dirty, LENS, want["outboards"], want["roots"], 2 * MIB, g, lanes=4, ring=3)
    st, uf = out["unit_status"].cpu().numpy(), ref["unit_first"]
    assert list(np.nonzero(st)[0]) == [int(uf[f]) + (3 * 1024 >> g)]
    assert out["file_status"].cpu().tolist() == [1 if i == f else 0 for i in range(len(LENS))]
    assert int(out["first_bad"][f].item()) == 3 * 1024 >> g
    with pytest.raises(m.B3WError):
        m.bao.outboard_stream_many(ctx, [hosts[f][:-1]], [LENS[f]], MIB, g, lanes=1)
    torch.cuda.synchronize()
    assert m.bao.outboard_stream_many(ctx, [], [], MIB, g, lanes=2)["outboards"].numel() == 0


def test_the_helpers_device_memory_does_not_grow_with_the_files():
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    n, ln, window, lanes, ring = 12, 8 * MIB, MIB, 3, 2
    rng = np.random.default_rng(14)
    hosts = [rng.integers(0, 256, ln, dtype=np.uint8) for _ in range(n)]
    lens = [ln] * n
    ob_bytes = n * m.bao.outboard_size(ln) + n * 32
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = m.bao.outboard_stream_many(ctx, hosts, lens, window, 0, lanes=lanes, ring=ring)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    bound = ring * lanes * window + ob_bytes + n * m.bao.stream_scratch_bytes(ln, m.bao.STREAM_OUTBOARD) + 64 * K
    print(f"outboard_stream_many of {n} x {ln} bytes: device memory rose by {rise}, bound {bound}")
    assert rise < bound < n * ln
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = m.bao.verify_stream_many(ctx, hosts, lens, got["outboards"], got["roots"], window, 0, lanes=lanes, ring=ring)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    bound = ring * lanes * window + n * (8 * K + 12) + n * m.bao.stream_scratch_bytes(ln, m.bao.STREAM_VERIFY) + 64 * K   # (the outboards are the caller's; a status a chunk)
    print(f"verify_stream_many of {n} x {ln} bytes: device memory rose by {rise}, bound {bound}")
    assert rise < bound < n * ln
    assert not out["unit_status"].any().item() and not out["file_status"].any().item()
    d_all = torch.from_numpy(np.concatenate(hosts)).cuda()
    want = m.bao.outboard_batch(ctx, d_all, [i * ln for i in range(n)], lens)
    assert _same_outboard(got, want)
