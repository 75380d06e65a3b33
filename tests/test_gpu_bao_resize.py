"""Outboards of resident files after appends and truncations (bao.outboard_resize_batch, b3w_bao_outboard_resize_batch_device).  The
yardstick is always what a caller did before: outboard_batch (g = 0) / outboard_groups_batch over the same arena with the old and with
the new lengths, every outboard byte and every root.  One arena holds a slot per transition (tests/bao_resize_ref.py), each of capacity
max(old, new) and starting at an odd byte, and three files that are never listed.  The new outboards go into a buffer of 0xA5 between
0xA5 guards: what the call may not write is still 0xA5 afterwards.  That the kept tiles' bytes are not read is shown by poison."""
import functools

import numpy as np
import pytest

import b3w_testlib as T
import bao_resize_ref as RR
from test_gpu_bao_batch import _arena

pytestmark = pytest.mark.gpu

K, M, GS = RR.K, RR.M, RR.GS
GUARD = 4096
UNLISTED = [0, 5 * K, 2 * M + 1]
N_T = len(RR.TRANSITIONS)
OLD = [o for o, _ in RR.TRANSITIONS] + UNLISTED
NEW = [n for _, n in RR.TRANSITIONS] + UNLISTED
LISTED = list(range(N_T))
ROOT_FILL = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def _setup():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    caps = [max(o, n) for o, n in zip(OLD, NEW)]
    arena, offsets = _arena(caps, starts_odd=set(range(len(caps))), seed=18)
    assert all(int(o) % 2 == 1 for o in offsets)                              # every file starts at an odd byte
    return dict(m=m, ctx=ctx, offsets=offsets, caps=caps, d_arena=torch.from_numpy(arena).cuda())


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """every device tensor of this module (the arena, the yardsticks, the 1 GiB file) comes from a pool of the allocator that is the
    module's own and goes with it: the modules behind this one that measure device memory find the default pool's cached blocks as they
    would without this one"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        if _setup.cache_info().currsize:
            _setup()["ctx"].close()
        _yard.cache_clear()
        _setup.cache_clear()
        gc.collect()
    del pool


def _batch(s, d_arena, offsets, lens, g):
    m = s["m"]
    return m.bao.outboard_batch(s["ctx"], d_arena, offsets, lens) if g == 0 else m.bao.outboard_groups_batch(s["ctx"], d_arena, offsets, lens, g)


@functools.lru_cache(maxsize=None)
def _yard(g, new):
    """the yardstick over the arena with the old (new = False) or the new lengths, computed once and left unchanged"""
    s = _setup()
    return _batch(s, s["d_arena"], s["offsets"], NEW if new else OLD, g)


def _places(m, lens, g, phase=None, reverse=False, gap=0):
    """-> (ob_first, total): a place for every file's outboard; phase None: packed in file order; else every place at `phase` modulo 16, in
    file order or the reverse, `gap` bytes and more between them"""
    sizes = [m.bao.group_outboard_size(int(x), g) for x in lens]
    first = np.zeros(len(lens), dtype=np.uint64)
    at = 0
    for f in (reversed(range(len(lens))) if reverse else range(len(lens))):
        if phase is not None:
            at = (at + gap + 15) // 16 * 16 + phase
        first[f] = at
        at += sizes[f]
    return first, at + gap


def _placed(m, yard, lens, g, first, total, fill):
    """the yardstick's outboards copied to the places `first` of a buffer of `total` bytes of `fill`"""
    import torch
    buf = torch.full((total,), fill, dtype=torch.uint8, device="cuda")
    for f, ln in enumerate(lens):
        a, size = int(yard["ob_first"][f]), m.bao.group_outboard_size(int(ln), g)
        buf[int(first[f]):int(first[f]) + size] = yard["outboards"][a:a + size]
    return buf


def _resize_and_check(s, g, d_arena, d_old, old_first, new_first, total_new, files, what):
    """the call into a guarded buffer of 0xA5; afterwards the listed files' extents and roots are the yardstick's and every other byte of
    the buffer, every other root and the whole old buffer are what they were"""
    import torch
    m = s["m"]
    want = _yard(g, True)
    keep_old = d_old.clone()
    buf = torch.full((total_new + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    d_new = buf[GUARD:GUARD + total_new]
    assert d_new.data_ptr() % 16 == 0 and d_old.data_ptr() % 16 == 0
    d_roots = torch.full((len(NEW), 8), ROOT_FILL, dtype=torch.int32, device="cuda")
    m.bao.outboard_resize_batch(s["ctx"], d_arena, s["offsets"], OLD, NEW, d_old, old_first, d_new, new_first, d_roots, files, group_log=g)
    torch.cuda.synchronize()
    expect = torch.full_like(buf, 0xA5)
    expect_roots = torch.full_like(d_roots, ROOT_FILL)
    for f in files:
        a, size = int(want["ob_first"][f]), m.bao.group_outboard_size(NEW[f], g)
        expect[GUARD + int(new_first[f]):GUARD + int(new_first[f]) + size] = want["outboards"][a:a + size]
        expect_roots[f] = want["roots"][f]
    for f in files:                                                           # file by file first, for a message that names the transition
        a, size = GUARD + int(new_first[f]), m.bao.group_outboard_size(NEW[f], g)
        diff = (buf[a:a + size] != expect[a:a + size]).nonzero()
        assert diff.numel() == 0, (what, g, f, OLD[f], NEW[f], int(diff[0].item()))
        assert torch.equal(d_roots[f], expect_roots[f]), (what, g, f, OLD[f], NEW[f])
    assert torch.equal(buf, expect), (what, g, int((buf != expect).nonzero()[0].item()))
    assert torch.equal(d_roots, expect_roots), (what, g)
    assert torch.equal(d_old, keep_old), (what, g)


@pytest.mark.parametrize("g", GS)
def test_all_transitions_in_one_call(g):
    s = _setup()
    m = s["m"]
    old = _yard(g, False)
    new_first, total = _places(m, NEW, g)
    assert total == int(_yard(g, True)["ob_first"][-1])
    _resize_and_check(s, g, s["d_arena"], old["outboards"], old["ob_first"], new_first, total, LISTED, "packed")


@pytest.mark.parametrize("g", GS)
def test_kept_tiles_and_unlisted_files_are_not_read(g):
    """the first T MiB of every listed file, every byte of the unlisted files and the unlisted files' old outboards are 0xEE at the call
    (the yardstick was made beforehand)"""
    s = _setup()
    m = s["m"]
    old = _yard(g, False)
    _yard(g, True)
    d_arena = s["d_arena"].clone()
    d_old = old["outboards"].clone()
    for f in range(len(NEW)):
        a = int(s["offsets"][f])
        if f in LISTED:
            d_arena[a:a + RR.kept_tiles(OLD[f], NEW[f]) * M] = 0xEE
        else:
            d_arena[a:a + s["caps"][f]] = 0xEE
            d_old[int(old["ob_first"][f]):int(old["ob_first"][f + 1])] = 0xEE
    new_first, total = _places(m, NEW, g)
    _resize_and_check(s, g, d_arena, d_old, old["ob_first"], new_first, total, LISTED, "poisoned")


@pytest.mark.parametrize("g", [0, 4])
@pytest.mark.parametrize("phases", [(8, 0), (0, 8), (8, 8)])
def test_the_result_does_not_depend_on_the_places_phases(phases, g):
    """a place at p modulo 16 puts the nodes at p + 8: the 16-byte moves serve (0, 0) alone (the packed layouts mix all four pairs)"""
    s = _setup()
    m = s["m"]
    old_first, old_total = _places(m, OLD, g, phase=phases[0], gap=40)
    new_first, new_total = _places(m, NEW, g, phase=phases[1], gap=24)
    assert all(int(x) % 16 == phases[0] for x in old_first) and all(int(x) % 16 == phases[1] for x in new_first)
    d_old = _placed(m, _yard(g, False), OLD, g, old_first, old_total, 0x33)
    _resize_and_check(s, g, s["d_arena"], d_old, old_first, new_first, new_total, LISTED, phases)


@pytest.mark.parametrize("g", [0, 6])
def test_places_in_reverse_file_order_with_gaps(g):
    s = _setup()
    m = s["m"]
    old_first, old_total = _places(m, OLD, g, phase=0, reverse=True, gap=200)
    new_first, new_total = _places(m, NEW, g, phase=8, reverse=True, gap=1000)
    assert int(old_first[0]) > int(old_first[N_T - 1]) and int(new_first[0]) > int(new_first[N_T - 1])
    d_old = _placed(m, _yard(g, False), OLD, g, old_first, old_total, 0x33)
    files = [f for f in reversed(LISTED) if f != 3]                           # (and the list itself out of order, one transition left out)
    _resize_and_check(s, g, s["d_arena"], d_old, old_first, new_first, new_total, files, "reversed")


@pytest.mark.parametrize("g", [0, 4])
def test_a_file_past_1_gib_grows_and_shrinks(g):
    """1 025 M + 5 -> 1 026 M + 300 (1 025 kept tiles, two merge storeys) -> 1 023 M (1 023 kept tiles, no byte read, one storey)"""
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    lens = [1025 * M + 5, 1026 * M + 300, 1023 * M]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1026)
    d_arena = torch.randint(0, 256, (3 + max(lens),), dtype=torch.uint8, device="cuda", generator=gen)
    offsets = [3]
    d_prev = _batch(s, d_arena, offsets, [lens[0]], g)["outboards"]
    for old_len, new_len in zip(lens, lens[1:]):
        want = _batch(s, d_arena, offsets, [new_len], g)
        kept = RR.kept_tiles(old_len, new_len)
        d_read = d_arena.clone()
        d_read[3:3 + kept * M] = 0xEE
        size = m.bao.group_outboard_size(new_len, g)
        buf = torch.full((size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        d_roots = torch.full((1, 8), ROOT_FILL, dtype=torch.int32, device="cuda")
        keep = d_prev.clone()
        m.bao.outboard_resize_batch(ctx, d_read, offsets, [old_len], [new_len], d_prev, [0], buf[GUARD:GUARD + size], [0], d_roots, [0], group_log=g)
        torch.cuda.synchronize()
        del d_read
        assert torch.equal(buf[GUARD:GUARD + size], want["outboards"]), (g, old_len, new_len, int((buf[GUARD:GUARD + size] != want["outboards"]).nonzero()[0].item()))
        assert torch.equal(d_roots, want["roots"]) and torch.equal(d_prev, keep), (g, old_len, new_len)
        assert bool((buf[:GUARD] == 0xA5).all().item()) and bool((buf[-GUARD:] == 0xA5).all().item())
        d_prev = buf[GUARD:GUARD + size].clone()


@pytest.mark.parametrize("g", [4, 6])
def test_thirty_calls_that_build_on_one_another(g):
    """one file through 3M+5 -> 5M+1 -> 8M -> 9M+3K -> 4M -> 3M-1 -> 3M+5 -> ..., the result of each call the next one's old outboard, between two
    buffers; then the last result serves verification, planning and an update in place"""
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    slot = RR.TRANSITIONS.index((8 * M, 9 * M + 3 * K))
    offsets = [int(s["offsets"][slot])]
    d_arena = s["d_arena"]
    cap = m.bao.group_outboard_size(max(RR.CHAIN), g)
    bufs = [torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_roots = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    length = RR.CHAIN[0]
    first = _batch(s, d_arena, offsets, [length], g)
    bufs[0][:first["outboards"].numel()] = first["outboards"]
    for k in range(30):
        new_len = RR.CHAIN[(k + 1) % len(RR.CHAIN)]
        m.bao.outboard_resize_batch(ctx, d_arena, offsets, [length], [new_len], bufs[k % 2], [0], bufs[(k + 1) % 2], [0], d_roots, [0], group_log=g)
        length = new_len
    assert length == RR.CHAIN[0]
    want = _batch(s, d_arena, offsets, [length], g)
    size = want["outboards"].numel()
    d_obs = bufs[0][:size].clone()
    assert torch.equal(d_obs, want["outboards"]) and torch.equal(d_roots, want["roots"]), g
    out = m.bao.verify_batch(ctx, d_arena, offsets, [length], d_obs, d_roots, g)
    assert not out["unit_status"].any().item() and not out["file_status"].any().item()
    chunks = [0, 1023, 1024, 2047, m.bao.num_chunks(length) - 1]
    plan = m.bao.plan_samples_arena(ctx, d_arena, offsets, [length], d_obs, d_roots, [0] * len(chunks), chunks, g)
    assert (plan["sample_status"] == 0).all()
    d_now = d_arena.clone()
    d_now[offsets[0] + 1500 * K + 9] ^= 1
    m.bao.outboard_update_batch(ctx, d_now, offsets, [length], d_obs, d_roots, [0], [1500], [1], group_log=g)
    want = _batch(s, d_now, offsets, [length], g)
    assert torch.equal(d_obs, want["outboards"]) and torch.equal(d_roots, want["roots"]), g


def _call_args(s, g, files):
    """what the refusal and memory tests pass: packed old outboards, a new buffer of 0xA5, roots of a pattern"""
    import torch
    m = s["m"]
    old = _yard(g, False)
    new_first, total = _places(m, NEW, g)
    d_new = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    d_roots = torch.full((len(NEW), 8), ROOT_FILL, dtype=torch.int32, device="cuda")
    return old, new_first, d_new, d_roots


def test_the_call_makes_the_scratch_and_no_other_device_memory():
    import torch
    s = _setup()
    m = s["m"]
    g = 1
    files = [9, 10, 7, 4, 0]                                                  # 2M+5K: 3 tiles; 5M+1: 6; M+1: 2; 65K and 1 B: none
    old, new_first, d_new, d_roots = _call_args(s, g, files)
    ln, fi = np.array(NEW, dtype=np.uint64), np.array(files, dtype=np.uint32)
    need = m.lib().b3w_bao_resize_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fi.size)
    assert need == 32 * (3 + 6 + 2)

    def call():
        m.bao.outboard_resize_batch(s["ctx"], s["d_arena"], s["offsets"], OLD, NEW, old["outboards"], old["ob_first"], d_new, new_first, d_roots, files, group_log=g)
    call()                                                                    # (warm: the context's staging slot is its own)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    call()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - start
    print(f"outboard_resize_batch: device memory rose by {rise} bytes for a scratch of {need}")
    assert rise == (need + 511) // 512 * 512                                   # (the allocator hands out multiples of 512)
    want = _yard(g, True)
    for f in files:
        a, size = int(want["ob_first"][f]), m.bao.group_outboard_size(NEW[f], g)
        assert torch.equal(d_new[int(new_first[f]):int(new_first[f]) + size], want["outboards"][a:a + size]) and torch.equal(d_roots[f], want["roots"][f])


def test_refusals_are_atomic_and_name_the_entry():
    import torch
    s = _setup()
    m = s["m"]
    L = m.lib()
    ctx = m.Context("compression", 0)                                         # (any context resizes)
    g = 1
    files = [10, 4, 0, 12]                                                    # 5M+1: 6 tiles; 65K; 1 B; 9M+3K: 10 tiles
    old, new_first, d_new, d_roots = _call_args(s, g, files)
    d_old = old["outboards"].clone()
    d_arena = s["d_arena"]
    off, lo, ln = (np.ascontiguousarray(x, dtype=np.uint64) for x in (s["offsets"], OLD, NEW))
    of, nf = np.ascontiguousarray(old["ob_first"], dtype=np.uint64), np.ascontiguousarray(new_first, dtype=np.uint64)
    fi = np.array(files, dtype=np.uint32)
    need = L.b3w_bao_resize_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fi.size)
    assert need == 32 * 16
    d_scratch = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    bad = m.B3W_E_BAD_ARGUMENT
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena=d_arena.data_ptr(), arena_bytes=d_arena.numel(), offsets=off, old_lens=lo, new_lens=ln, n_files=ln.size, gl=g, old_first=of,
             olds=d_old.data_ptr(), new_first_=nf, news=d_new.data_ptr(), roots=d_roots.data_ptr(), listed=fi, n=None, scratch=d_scratch.data_ptr(),
             scratch_bytes=need):
        p = lambda a: None if a is None else a.ctypes.data
        return L.b3w_bao_outboard_resize_batch_device(ctx.handle, arena, arena_bytes, p(offsets), p(old_lens), p(new_lens), n_files, gl, p(old_first), olds,
                                                      p(new_first_), news, roots, p(listed), (0 if listed is None else listed.size) if n is None else n,
                                                      scratch, scratch_bytes, stream)

    def bent(a, f, v):
        b = a.copy()
        b[f] = v
        return b
    F = 10
    entry = "entry 0 (file %d)" % F
    cases = [(dict(offsets=None), "null"), (dict(old_lens=None), "null"), (dict(new_lens=None), "null"), (dict(old_first=None), "null"),
             (dict(olds=None), "null"), (dict(new_first_=None), "null"), (dict(news=None), "null"), (dict(roots=None), "null"),
             (dict(listed=None, n=4), "null"), (dict(arena=None), entry + ": a null arena"), (dict(gl=7), "group_log"),
             (dict(n_files=F), entry + ": the file index"),
             (dict(listed=np.array(files + [4], dtype=np.uint32), scratch_bytes=need + 16), "entry 4 (file 4): the file is listed twice (entry 1"),
             (dict(arena_bytes=int(off[F]) + NEW[F] - 1), entry + ": the file reaches past arena_bytes"),
             (dict(old_lens=bent(lo, F, (1 << 40) + 1)), entry + ": a file of more than 2^30 chunks"),
             (dict(new_lens=bent(ln, F, (1 << 40) + 1), arena_bytes=1 << 41), entry + ": a file of more than 2^30 chunks"),
             (dict(olds=d_old.data_ptr() + 4), "8-byte aligned"), (dict(news=d_new.data_ptr() + 4), "8-byte aligned"),
             (dict(roots=d_roots.data_ptr() + 2), "4-byte aligned"),
             (dict(old_first=bent(of, F, int(of[F]) + 4)), entry + ": an outboard offset"), (dict(new_first_=bent(nf, F, int(nf[F]) + 4)), entry + ": an outboard offset"),
             (dict(news=d_old.data_ptr(), new_first_=of), entry + ": the file's old and new outboards overlap"),
             (dict(news=d_old.data_ptr(), new_first_=bent(nf, F, int(of[F]) + m.bao.group_outboard_size(OLD[F], g) - 8)), entry + ": the file's old and new outboards overlap"),
             (dict(scratch_bytes=need - 1), "scratch"), (dict(scratch=None), "scratch"), (dict(scratch=d_scratch.data_ptr() + 8), "scratch")]
    for kw, word in cases:
        assert call(**kw) == bad, kw
        assert ctx.last_error().startswith("bao resize: ") and word in ctx.last_error(), (kw, ctx.last_error())
    # a bad entry behind good ones: nothing of the good ones is done
    for f, word in ((len(NEW), "the file index"), (10, "listed twice")):
        assert call(listed=np.array(files + [f], dtype=np.uint32), scratch_bytes=need + 16) == bad
        assert word in ctx.last_error() and "entry 4 (file %d)" % f in ctx.last_error(), ctx.last_error()
    assert all(int(off[f]) + NEW[f] < int(off[13]) for f in files)             # (file 13 lies behind the good ones)
    assert call(listed=np.array(files + [13], dtype=np.uint32), arena_bytes=int(off[13]) + NEW[13] - 1, scratch_bytes=need + 32 * 4) == bad
    assert "entry 4 (file 13): the file reaches past arena_bytes" in ctx.last_error(), ctx.last_error()
    # a grid of more than 2^31 - 1 workgroups: 32 768 files of 2^20 kept tiles each at g = 6 (16 blocks a relocation workgroup); host arrays only
    n_big = 32768
    big = np.full(n_big, 1 << 40, dtype=np.uint64)
    # (the new places far behind the old buffer, wherever the two tensors lie: nothing there is touched by a refused call)
    zeros, far = np.zeros(n_big, dtype=np.uint64), np.full(n_big, (max(0, d_old.data_ptr() - d_new.data_ptr()) + (1 << 32)) // 8 * 8, dtype=np.uint64)
    assert call(arena_bytes=1 << 41, offsets=zeros, old_lens=big, new_lens=big, n_files=n_big, gl=6, old_first=zeros, new_first_=far,
                listed=np.arange(n_big, dtype=np.uint32)) == bad
    assert "entry %d (file %d)" % (n_big - 1, n_big - 1) in ctx.last_error() and "2^31 - 1 workgroups" in ctx.last_error(), ctx.last_error()
    assert L.b3w_bao_outboard_resize_batch_device(None, None, 0, None, None, None, 0, 0, None, None, None, None, None, None, 0, None, 0, None) == bad
    # the Python call: its own checks, and the library's refusal as an error
    with pytest.raises(m.B3WError, match="listed twice"):
        m.bao.outboard_resize_batch(ctx, d_arena, off, lo, ln, d_old, of, d_new, nf, d_roots, [10, 10], group_log=g)
    with pytest.raises(m.B3WError, match="reaches past d_new_outboards"):
        m.bao.outboard_resize_batch(ctx, d_arena, off, lo, ln, d_old, of, d_new[:int(nf[10]) + 64], nf, d_roots, [10], group_log=g)
    with pytest.raises(m.B3WError, match="reaches past d_old_outboards"):
        m.bao.outboard_resize_batch(ctx, d_arena, off, lo, ln, d_old[:int(of[10]) + 64], of, d_new, nf, d_roots, [10], group_log=g)
    with pytest.raises(m.B3WError, match="overlap"):
        m.bao.outboard_resize_batch(ctx, d_arena, off, lo, ln, d_old, of, d_old, of, d_roots, [12], group_log=g)
    torch.cuda.synchronize()
    assert torch.equal(d_old, old["outboards"]) and bool((d_new == 0xA5).all().item()) and bool((d_roots == ROOT_FILL).all().item())
    assert bool((d_scratch == 0x5A).all().item())
    # nothing listed: B3W_OK and nothing launched; then the good list
    assert call(n=0) == 0 and call(listed=None, n=0, scratch=None, scratch_bytes=0) == 0
    torch.cuda.synchronize()
    assert bool((d_new == 0xA5).all().item()) and bool((d_roots == ROOT_FILL).all().item()) and bool((d_scratch == 0x5A).all().item())
    assert call() == 0
    torch.cuda.synchronize()
    want = _yard(g, True)
    for f in files:
        a, size = int(want["ob_first"][f]), m.bao.group_outboard_size(NEW[f], g)
        assert torch.equal(d_new[int(nf[f]):int(nf[f]) + size], want["outboards"][a:a + size]) and torch.equal(d_roots[f], want["roots"][f]), f
    assert torch.equal(d_old, old["outboards"]) and bool((d_scratch[need:] == 0x5A).all().item())
    ctx.close()
