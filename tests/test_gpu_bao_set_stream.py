"""Set slices taken in windows on the device (b3w_bao_set_slice_stream_begin / _push / _finish / _free; bao.SetSliceStream,
bao.ingest_set_slice_stream).  The oracle is the one-shot receiver on the same slice: bao.ingest_set_slices into an arena that starts
at an odd byte, bao.ingest_set_slices_packed with and without an outboard - every output compared byte for byte between 0xA5 walls -
and the host call b3w_bao_set_slice_ingest.  The slices come from the device provider (held against the restatement in
test_gpu_bao_set); every window is pushed from a buffer of its own between random bytes, so a read outside the window (but for the
carried area) cannot verify.  Files: 3 MiB + 5 bytes, 5 MiB + 300 bytes, 40 chunks and the empty file."""
import ctypes
import functools
import struct

import numpy as np
import pytest

import b3w_testlib as T
import bao_set_ref as RS
import bao_set_stream_ref as SR
from test_bao_set_cpu import set_shapes
from test_gpu_bao_ingest import BAD, FILL, K, _walled, _walls_intact

pytestmark = pytest.mark.gpu

GS = [0, 4, 6]
LENGTHS = [3 * (1 << 20) + 5, 5 * (1 << 20) + 300, 40 * K, 0]
SKEW = 1                                                                   # the file starts at an odd byte of the arena
MIN = SR.MIN_WINDOW
KINDS = ("arena", "packed", "decode")                                      # packed slots with an outboard; without one


@functools.lru_cache(maxsize=None)
def _world():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    rng = np.random.default_rng(33)
    files = []
    for ln in LENGTHS:
        data = rng.integers(0, 256, ln, dtype=np.uint8)
        d_src = torch.from_numpy(data).cuda()
        made = {g: m.bao.outboard_batch(ctx, d_src, [0], [ln]) if g == 0 else m.bao.outboard_groups_batch(ctx, d_src, [0], [ln], g) for g in GS}
        files.append(dict(len=ln, n=m.bao.num_chunks(ln), data=data, d_src=d_src, made=made, roots=made[0]["roots"]))
    torch.cuda.synchronize()
    return dict(m=m, ctx=ctx, files=files)


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """as test_gpu_bao_set does it: the module's device tensors come from a pool of its own and go with it"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        _slice.cache_clear()
        if _world.cache_info().currsize:
            _world()["ctx"].close()
        _world.cache_clear()
        gc.collect()
    del pool


def _sets(n):
    """the shapes of the issue that fit a file of n chunks -> {name: runs (a tuple)}"""
    sh = set_shapes(n)
    names = ("every second chunk", "{1023, 1025}", "the whole file", "a run ending on the last chunk")
    return {name: tuple(sh[name]) for name in names if name in sh}


def _fc(runs):
    return np.array([a for a, _ in runs], dtype=np.uint64), np.array([k for _, k in runs], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _slice(f, g, runs):
    """the provider's set slice of file f (computed once, left unchanged) -> (the packed tensor: the slice from byte 8 on, its size)"""
    w = _world()
    m, x = w["m"], w["files"][f]
    first, count = _fc(runs)
    out = m.bao.set_slices_arena(w["ctx"], x["d_src"], [0], [x["len"]], x["made"][g]["outboards"], np.zeros(len(runs), dtype=np.uint32), first, count, group_log=g)
    return out["slices"], m.bao.set_slice_size(x["len"], first, count)


def _receiver(w, f, g, kind, runs, seed=7):
    """fresh outputs between walls: the destination (arena: the file from byte SKEW; else the slots), outboard, bitmap"""
    import torch
    x = w["files"][f]
    total = sum(k for _, k in runs)
    size = x["len"] + SKEW + 3 if kind == "arena" else total * K
    whole_d, d_dest = _walled(size)
    ob_bytes = w["m"].bao.group_outboard_size(x["len"], g)
    whole_o, d_obs = _walled(ob_bytes)
    words = (x["n"] + 63) // 64
    pre = np.random.default_rng(seed).integers(0, 1 << 63, words, dtype=np.int64)
    full = np.zeros(words, dtype=np.uint64)
    c = np.arange(x["n"], dtype=np.uint64)
    np.bitwise_or.at(full, (c >> np.uint64(6)).astype(np.int64), np.uint64(1) << (c & np.uint64(63)))
    pre &= full.view(np.int64)                                             # (the pad bits are the library's to leave clear)
    return dict(kind=kind, whole_d=whole_d, d_dest=d_dest, size=size, whole_o=whole_o, d_obs=d_obs if kind != "decode" else None, ob_bytes=ob_bytes,
                d_have=torch.from_numpy(pre.copy()).cuda(), total=total)


def _one_shot(w, f, g, r, runs, d_slices, roots=None):
    m, x = w["m"], w["files"][f]
    first, count = _fc(runs)
    fi = np.zeros(len(runs), dtype=np.uint32)
    roots = x["roots"] if roots is None else roots
    if r["kind"] == "arena":
        return m.bao.ingest_set_slices(w["ctx"], r["d_dest"], [SKEW], [x["len"]], r["d_obs"], roots, fi, first, count, d_slices, group_log=g, d_have=r["d_have"])
    return m.bao.ingest_set_slices_packed(w["ctx"], [x["len"]], r["d_obs"], roots, fi, first, count, d_slices, group_log=g, d_have=r["d_have"], d_chunks=r["d_dest"])


def _session(w, f, g, r, runs, window_bytes, roots=None):
    m, x = w["m"], w["files"][f]
    first, count = _fc(runs)
    dest = r["d_dest"][SKEW:SKEW + x["len"]] if r["kind"] == "arena" else r["d_dest"]
    return m.bao.SetSliceStream(w["ctx"], x["len"], first, count, x["roots"] if roots is None else roots, d_dest=dest, d_outboard=r["d_obs"], group_log=g,
                                window_bytes=window_bytes, packed=r["kind"] != "arena", d_have=r["d_have"])


def _window(d_slices, a, b, seed=0):
    """slice bytes [a, b) in a buffer of their own between random bytes, at 8 modulo 16 for a == 0 and 16-byte aligned otherwise"""
    import torch
    lead = 256 + (0 if a else 8)
    buf = torch.from_numpy(np.random.default_rng(1000 + seed).integers(0, 256, lead + (b - a) + 256, dtype=np.uint8)).cuda()
    buf[lead:lead + b - a] = d_slices[8 + a:8 + b]
    return buf[lead:lead + b - a]


def _same(r, q, out, got):
    """the streamed receiver q and its dict `got` against the one-shot receiver r and its dict `out`: every byte between the walls"""
    import torch
    for key in ("set_status", "set_first_bad", "chunk_status"):
        assert torch.equal(out[key], got[key]), key
    for key in ("set_file", "set_range_first", "set_chunk_first", "slice_first"):
        assert (out[key] == got[key]).all(), key
    assert torch.equal(r["whole_d"], q["whole_d"]) and torch.equal(r["whole_o"], q["whole_o"]) and torch.equal(r["d_have"], q["d_have"])
    assert _walls_intact(q["whole_d"], q["size"]) and _walls_intact(q["whole_o"], q["ob_bytes"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("g", GS)
def test_windows_of_one_row_two_rows_and_the_whole_slice_equal_the_one_shot_call(g, kind):
    w = _world()
    rows_seen = set()
    for f, x in enumerate(w["files"]):
        for name, runs in _sets(x["n"]).items():
            d_slices, size = _slice(f, g, runs)
            cuts, B = SR.row_cuts(x["len"], list(runs))
            assert cuts[-1] == size
            rows_seen.add((B, len(cuts) - 1))
            r = _receiver(w, f, g, kind, runs)
            out = _one_shot(w, f, g, r, runs, d_slices)
            assert not out["chunk_status"].any().item() and out["set_status"].tolist() == [0] and out["set_first_bad"].tolist() == [-1]
            for bounds in (cuts, SR.every(cuts, 2), [0, size]):
                q = _receiver(w, f, g, kind, runs)
                s = _session(w, f, g, q, runs, max(MIN, size))
                for i, (a, b) in enumerate(zip(bounds, bounds[1:])):
                    s.push(a, _window(d_slices, a, b, i))
                got = s.finish()
                s.close()
                _same(r, q, out, got)
                if kind != "arena":
                    assert got["chunks"] is q["d_dest"] and (got["slot_first"] == out["slot_first"]).all()
    assert {(1024, 6), (1024, 4), (1024, 3), (64, 2), (64, 1)} <= rows_seen


def _host(w, f, g, runs, sl, root):
    """b3w_bao_set_slice_ingest over the same slice from buffers of 0xEE -> (data, outboard, set status, first bad, chunk statuses)"""
    m, x = w["m"], w["files"][f]
    data, ob = np.full(x["len"], FILL, dtype=np.uint8), np.full(m.bao.group_outboard_size(x["len"], g), FILL, dtype=np.uint8)
    first, count = _fc(runs)
    st, fb, cs = m.bao.ingest_set_slice_host(data, ob, x["len"], first, count, root, sl, g)
    return data, ob, st, -1 if fb is None else fb, cs.tolist()


def _tampers(x, runs, cuts):
    """-> [(what, the slice offset of the flipped byte, the chunks it must spoil (a predicate), the status they get)]"""
    places = SR.places(x["len"], list(runs))
    wanted = RS.chunks_of(runs)
    in_row_1 = next(c for c in wanted if c >= 1024)
    return [("the header", 3, lambda c: True, 3),
            ("the root node, carried into every later window", places[("node", 0, x["n"])] + 37, lambda c: True, 2),
            ("a node of depth 2 whose subtree ends before the last window", places[("node", 0, 2048)] + 5, lambda c: c < 2048, 2),
            ("a chunk in window 2 only", places[("chunk", in_row_1)] + 700, lambda c: c == in_row_1, 1),
            ("a node inside a tile", places[("node", 1024, 512)] + 63, lambda c: 1024 <= c < 1536, 2)]


@pytest.mark.parametrize("kind", ["arena", "decode"])
@pytest.mark.parametrize("g", [0, 4])
def test_one_flip_at_a_time_beside_good_chunks(g, kind):
    import torch
    w = _world()
    f = 1
    x = w["files"][f]
    runs = _sets(x["n"])["every second chunk"]
    wanted = RS.chunks_of(runs)
    clean, size = _slice(f, g, runs)
    cuts, _ = SR.row_cuts(x["len"], list(runs))
    assert len(cuts) == 7
    root = x["roots"].cpu().numpy().view(np.uint32).reshape(-1).tolist()
    for what, at, spoiled, status in _tampers(x, runs, cuts):
        d_slices = clean.clone()
        d_slices[8 + at] ^= 0x20
        r = _receiver(w, f, g, kind, runs)
        out = _one_shot(w, f, g, r, runs, d_slices)
        cs = out["chunk_status"].cpu().tolist()
        assert cs == [status if spoiled(c) else 0 for c in wanted], what
        if kind == "arena":                                                # the one-shot call where it is held against the host call today
            data, ob, st, fb, hcs = _host(w, f, g, runs, d_slices[8:8 + size].cpu().numpy().tobytes(), root)
            assert (out["set_status"].tolist(), out["set_first_bad"].tolist(), cs) == ([st], [fb], hcs), what
            assert (r["d_dest"][SKEW:SKEW + x["len"]].cpu().numpy() == data).all() and (r["d_obs"].cpu().numpy() == ob).all(), what
        q = _receiver(w, f, g, kind, runs)
        s = _session(w, f, g, q, runs, MIN)
        for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
            s.push(a, _window(d_slices, a, b, i))
            bad = [c for c, st in zip(wanted, cs) if st and c < 1024 * (i + 1)]         # what the rows so far hold
            worst = max([st for c, st in zip(wanted, cs) if c < 1024 * (i + 1)])
            assert (s.set_status.tolist(), s.set_first_bad.tolist()) == ([worst], [bad[0] if bad else -1]), (what, i)
        got = s.finish()
        s.close()
        _same(r, q, out, got)
        assert torch.equal(q["d_have"], r["d_have"])


class _OddReader:
    """readinto in pieces of odd sizes"""

    def __init__(self, data):
        self.data, self.at, self.k = memoryview(data), 0, 0

    def readinto(self, view):
        self.k += 1
        nb = min(len(view), len(self.data) - self.at, 1 + (7919 * self.k) % 100003)
        view[:nb] = self.data[self.at:self.at + nb]
        self.at += nb
        return nb


@pytest.mark.parametrize("kind", ["arena", "packed"])
def test_the_helper_from_host_bytes_and_from_a_reader(kind):
    w = _world()
    m = w["m"]
    for f, g, name, window in ((0, 4, "the whole file", MIN), (1, 0, "every second chunk", 2 * MIN), (2, 6, "the whole file", MIN), (3, 0, "the whole file", MIN)):
        x = w["files"][f]
        runs = _sets(x["n"])[name]
        d_slices, size = _slice(f, g, runs)
        first, count = _fc(runs)
        assert len(m.bao.set_slice_cuts(x["len"], first, count, window)) == (4 if f == 0 else 3 if f == 1 else 2)
        r = _receiver(w, f, g, kind, runs)
        out = _one_shot(w, f, g, r, runs, d_slices)
        sl = d_slices[8:8 + size].cpu().numpy().tobytes()
        for source in (sl, _OddReader(sl)):
            q = _receiver(w, f, g, kind, runs)
            dest = q["d_dest"][SKEW:SKEW + x["len"]] if kind == "arena" else q["d_dest"]
            got = m.bao.ingest_set_slice_stream(w["ctx"], source, x["len"], first, count, x["roots"], d_dest=dest, d_outboard=q["d_obs"], group_log=g,
                                                window_bytes=window, packed=kind != "arena", d_have=q["d_have"])
            assert set(got) == set(out)
            _same(r, q, out, got)


@pytest.mark.parametrize("g", [0, 4])
def test_the_loop_closes_with_thirty_percent_missing(g):
    """have_runs -> set_slices_arena -> the streamed receiver -> the bitmap is full and the file is the source's"""
    import torch
    w = _world()
    m, ctx = w["m"], w["ctx"]
    for f in (0, 1):
        x = w["files"][f]
        rng = np.random.default_rng(70 + f)
        held = rng.random(x["n"]) >= 0.3
        d_have = m.bao.have_new([x["len"]])
        words = np.zeros(d_have.numel(), dtype=np.uint64)
        c = np.flatnonzero(held).astype(np.uint64)
        np.bitwise_or.at(words, (c >> np.uint64(6)).astype(np.int64), np.uint64(1) << (c & np.uint64(63)))
        d_have.copy_(torch.from_numpy(words.view(np.int64)))
        whole_a, d_arena = _walled(x["len"] + SKEW)
        file = d_arena[SKEW:SKEW + x["len"]]
        mask = torch.from_numpy(np.repeat(held, K)[:x["len"]]).cuda()
        file[mask] = x["d_src"][mask]
        d_obs = x["made"][g]["outboards"].clone()
        runs = m.bao.have_runs(ctx, d_have, [x["len"]], kind="missing")
        files, first, count = runs["files"], runs["first_chunks"], runs["n_chunks"]
        assert int(np.sum(count)) == int((~held).sum()) and len(files) > 200
        out = m.bao.set_slices_arena(ctx, x["d_src"], [0], [x["len"]], x["made"][g]["outboards"], files, first, count, group_log=g)
        size = m.bao.set_slice_size(x["len"], first, count)
        got = m.bao.ingest_set_slice_stream(ctx, out["slices"][8:8 + size].cpu().numpy(), x["len"], first, count, x["roots"], d_dest=file, d_outboard=d_obs,
                                            group_log=g, window_bytes=MIN, d_have=d_have)
        assert got["set_status"].tolist() == [0] and not got["chunk_status"].any().item() and got["chunk_status"].numel() == int((~held).sum())
        again = m.bao.have_runs(ctx, d_have, [x["len"]], kind="missing")
        assert len(again["files"]) == 0 and again["file_have"].cpu().tolist() == [x["n"]]
        assert torch.equal(file, x["d_src"]) and torch.equal(d_obs, x["made"][g]["outboards"]) and _walls_intact(whole_a, x["len"] + SKEW)


def test_a_destination_past_4_gib():
    """test_gpu_bao_set's fictitious file of 5 GiB + 300 B in an arena that is never initialised, its slice pushed a row a window: the
    cuts are small, the chunks land past byte 2^32 of the destination; only the written places are read back"""
    import torch
    from test_gpu_bao_set import _fabricate, _preorder
    w = _world()
    m = w["m"]
    length = (5 << 30) + 300
    n = m.bao.num_chunks(length)
    rng = np.random.default_rng(65)
    runs = [(7, 1), ((1 << 22) - 1, 3), (n - 1, 1)]
    wanted = RS.chunks_of(runs)
    chosen = {c: rng.integers(0, 256, min(K, length - c * K), dtype=np.uint8).tobytes() for c in wanted}
    sl, root, nodes = _fabricate(length, wanted, chosen, rng)
    first, count = _fc(runs)
    cuts = [int(c) for c in m.bao.set_slice_cuts(length, first, count, MIN)]
    rows, _ = SR.row_cuts(length, runs)
    assert cuts == [0, len(sl)] and len(rows) == 5
    d_slices = torch.from_numpy(np.frombuffer(bytes(8) + sl, dtype=np.uint8).copy()).cuda()
    d_root = torch.from_numpy(np.array(root, dtype=np.uint32).view(np.int32)).cuda()
    d_arena = torch.empty(length + 16, dtype=torch.uint8, device="cuda")
    d_obs = torch.empty(m.bao.group_outboard_size(length, 0), dtype=torch.uint8, device="cuda")
    d_have = m.bao.have_new([length])
    s = m.bao.SetSliceStream(w["ctx"], length, first, count, d_root, d_dest=d_arena[SKEW:SKEW + length], d_outboard=d_obs, window_bytes=MIN, d_have=d_have)
    for i, (a, b) in enumerate(zip(rows, rows[1:])):
        s.push(a, _window(d_slices, a, b, i))
    out = s.finish()
    s.close()
    assert out["set_status"].tolist() == [0] and out["set_first_bad"].tolist() == [-1] and out["chunk_status"].tolist() == [0] * 5
    assert d_obs[:8].cpu().numpy().tobytes() == struct.pack("<Q", length)
    for (lo, size), node in nodes.items():
        i = _preorder(n, lo, size)
        assert d_obs[8 + 64 * i:8 + 64 * i + 64].cpu().numpy().tobytes() == node, (lo, size)
    for c in wanted:
        at = SKEW + c * K
        assert d_arena[at:at + len(chosen[c])].cpu().numpy().tobytes() == chosen[c], c
        assert (int(d_have[c >> 6].item()) >> (c & 63)) & 1
    assert int((d_have != 0).sum().item()) == 4
    del d_arena, d_obs


def _c_session(w, f, g, q, runs, scratch, st, fb, cs):
    """begin through the C ABI with the caller's outputs -> the session handle"""
    import torch
    L, x = w["m"].lib(), w["files"][f]
    first, count = _fc(runs)
    h = ctypes.c_void_p()
    dest = q["d_dest"][SKEW:SKEW + x["len"]]
    rc = L.b3w_bao_set_slice_stream_begin(w["ctx"].handle, x["len"], g, first.ctypes.data, count.ctypes.data, first.size, x["roots"].data_ptr(), 0, dest.data_ptr(),
                                          dest.numel(), q["d_obs"].data_ptr(), q["d_have"].data_ptr(), cs.data_ptr(), st.data_ptr(), fb.data_ptr(),
                                          scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream, ctypes.byref(h))
    assert rc == 0 and h.value, w["ctx"].last_error()
    return h


def test_a_whole_session_allocates_nothing():
    import torch
    w = _world()
    L, f, g = w["m"].lib(), 1, 0
    x = w["files"][f]
    runs = _sets(x["n"])["every second chunk"]
    d_slices, size = _slice(f, g, runs)
    cuts, _ = SR.row_cuts(x["len"], list(runs))
    first, count = _fc(runs)
    r = _receiver(w, f, g, "arena", runs)
    out = _one_shot(w, f, g, r, runs, d_slices)
    q = _receiver(w, f, g, "arena", runs)
    wins = [_window(d_slices, a, b, i) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    fb = torch.full((1,), -2, dtype=torch.int64, device="cuda")
    cs = torch.full((q["total"],), -1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(L.b3w_bao_set_slice_stream_scratch_bytes(x["len"], first.ctypes.data, count.ctypes.data, first.size, MIN), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated(), torch.cuda.memory_allocated()
    h = _c_session(w, f, g, q, runs, scratch, st, fb, cs)
    for (a, b), win in zip(zip(cuts, cuts[1:]), wins):
        assert L.b3w_bao_set_slice_stream_push(h, a, win.data_ptr(), b - a, stream) == 0, w["ctx"].last_error()
    assert L.b3w_bao_set_slice_stream_finish(h) == 0
    L.b3w_bao_set_slice_stream_free(h)
    torch.cuda.synchronize()
    assert (torch.cuda.max_memory_allocated(), torch.cuda.memory_allocated()) == before
    _same(r, q, out, dict(out, set_status=st, set_first_bad=fb, chunk_status=cs))


def test_refusals_leave_everything_untouched_and_the_session_usable():
    import torch
    w = _world()
    L, ctx, f, g = w["m"].lib(), w["ctx"], 1, 4
    x = w["files"][f]
    runs = _sets(x["n"])["every second chunk"]
    d_slices, size = _slice(f, g, runs)
    cuts, _ = SR.row_cuts(x["len"], list(runs))
    first, count = _fc(runs)
    r = _receiver(w, f, g, "arena", runs)
    out = _one_shot(w, f, g, r, runs, d_slices)
    q = _receiver(w, f, g, "arena", runs)
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    fb = torch.full((1,), -2, dtype=torch.int64, device="cuda")
    cs = torch.full((q["total"],), -1, dtype=torch.int32, device="cuda")
    need = L.b3w_bao_set_slice_stream_scratch_bytes(x["len"], first.ctypes.data, count.ctypes.data, first.size, 2 * MIN)
    assert need == 1552 + 16 * 4                                            # rows of about 590 KB: three in a window of 2.2 MB, and the short last row
    whole_s, scratch = _walled(need)
    stream = torch.cuda.current_stream().cuda_stream
    h = _c_session(w, f, g, q, runs, scratch, st, fb, cs)
    whole = _window(d_slices, 0, size, 99)
    wins = [_window(d_slices, a, b, i) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]
    two = _window(d_slices, cuts[1], cuts[3], 50)

    def state():
        torch.cuda.synchronize()
        return [t.clone() for t in (q["whole_d"], q["whole_o"], q["d_have"], st, fb, cs, whole_s)]

    def refused(rc, word, was):
        assert rc == BAD and word in ctx.last_error(), (rc, word, ctx.last_error())
        assert all(torch.equal(a, b) for a, b in zip(was, state())), word

    push = lambda off, win, nb: L.b3w_bao_set_slice_stream_push(h, off, win.data_ptr() if win is not None else None, nb, stream)
    was = state()
    assert st.tolist() == [0] and fb.tolist() == [-1]                     # begin: "0, none"
    refused(push(cuts[1], wins[1], cuts[2] - cuts[1]), "out of order", was)
    refused(push(0, wins[0], cuts[1] - 16), "does not end on a cut", was)
    refused(push(0, wins[0], size + 16), "past the slice's end", was)
    refused(push(0, whole[8:], cuts[1]), "8 modulo 16", was)
    refused(push(0, None, cuts[1]), "null window", was)
    refused(push(0, wins[0], 0), "null window", was)
    refused(push(0, whole, size), "the scratch holds", was)
    refused(L.b3w_bao_set_slice_stream_finish(h), "have not been pushed", was)
    assert push(0, wins[0], cuts[1]) == 0, ctx.last_error()
    was = state()
    refused(push(0, wins[0], cuts[1]), "out of order", was)
    refused(push(cuts[2], wins[2], cuts[3] - cuts[2]), "out of order", was)
    refused(push(cuts[1], two[8:], cuts[3] - cuts[1] - 8), "does not end on a cut", was)
    misaligned = _window(d_slices, cuts[1] - 8, cuts[2], 51)[8:]
    refused(push(cuts[1], misaligned, cuts[2] - cuts[1]), "not 16-byte aligned", was)
    refused(L.b3w_bao_set_slice_stream_finish(h), "have not been pushed", was)
    assert push(cuts[1], two, cuts[3] - cuts[1]) == 0, ctx.last_error()   # two rows a window
    for i in range(3, 6):
        assert push(cuts[i], wins[i], cuts[i + 1] - cuts[i]) == 0, ctx.last_error()
    was = state()
    refused(push(cuts[5], wins[5], cuts[6] - cuts[5]), "pushed to its end", was)
    assert L.b3w_bao_set_slice_stream_finish(h) == 0
    refused(push(0, wins[0], cuts[1]), "finished", was)
    refused(L.b3w_bao_set_slice_stream_finish(h), "finished", was)
    L.b3w_bao_set_slice_stream_free(h)
    _same(r, q, out, dict(out, set_status=st, set_first_bad=fb, chunk_status=cs))
    assert _walls_intact(whole_s, need)
    # begin: what the one-shot call refuses, and a scratch that cannot hold one row; nothing is written, no session comes back
    was = state()
    h2 = ctypes.c_void_p(77)
    dest = q["d_dest"][SKEW:SKEW + x["len"]]

    def begin(first=first, count=count, g=g, kind=0, dest_ptr=dest.data_ptr(), dest_bytes=dest.numel(), ob=q["d_obs"].data_ptr(), st_ptr=st.data_ptr(),
              scratch_ptr=scratch.data_ptr(), scratch_bytes=need, root=x["roots"].data_ptr()):
        return L.b3w_bao_set_slice_stream_begin(ctx.handle, x["len"], g, first.ctypes.data, count.ctypes.data, first.size, root, kind, dest_ptr, dest_bytes, ob,
                                                q["d_have"].data_ptr(), cs.data_ptr(), st_ptr, fb.data_ptr(), scratch_ptr, scratch_bytes,
                                                stream, ctypes.byref(h2))
    for kw, word in ((dict(g=7), "group_log"), (dict(kind=2), "destination kind"), (dict(ob=None), "null pointer"), (dict(root=None), "null pointer"),
                     (dict(st_ptr=None), "null pointer"), (dict(dest_bytes=x["len"] - 1), "reaches past"), (dict(first=first[::-1].copy()), "ascending"),
                     (dict(count=np.zeros_like(count)), "no chunk"), (dict(scratch_bytes=1552 + 15), "scratch"), (dict(scratch_ptr=scratch.data_ptr() + 8), "scratch"),
                     (dict(scratch_ptr=None), "scratch"), (dict(kind=1, dest_ptr=dest.data_ptr()), "16-byte aligned")):
        h2.value = 77
        rc = begin(**kw)
        assert rc == BAD and word in ctx.last_error() and not h2.value, (kw, rc, ctx.last_error())
        assert all(torch.equal(a, b) for a, b in zip(was, state())), kw
