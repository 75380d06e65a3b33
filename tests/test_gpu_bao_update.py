"""Outboards updated in place after writes to resident files (bao.outboard_update_batch, b3w_bao_outboard_update_batch_device).  The
yardstick is always what a caller did before: outboard_batch (g = 0) / outboard_groups_batch over the arena as it is after the writes,
every outboard byte and every root.  The outboards sit between 0xA5 guards that must survive.  Sparseness is shown by poison: every
stored node with no dirty unit below it, every header of a file of more than 64 chunks, every byte of the arena outside the dirty units
and everything of the files without a dirty range is 0xEE before the call; afterwards the poisoned outboard bytes are still 0xEE and the
rest is the yardstick's, so nothing poisoned was read into a result or written."""
import functools

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
from test_gpu_bao_batch import _arena

pytestmark = pytest.mark.gpu

GS = [0, 1, 4, 6]
K = 1024
GUARD = 4096
COUNTS = [1, 2, 3, 64, 65, 1023, 1024, 1025, 2051]
# 0 B, 1 B, then every chunk count with a ragged and with a whole last chunk
LENS = [0, 1] + [x for k in COUNTS for x in (k * K - 300, k * K)]


def _ragged(k):
    return 2 + 2 * COUNTS.index(k)


def _whole(k):
    return 3 + 2 * COUNTS.index(k)


def _n(f):
    return max(1, -(-LENS[f] // K))


@functools.lru_cache(maxsize=None)
def _setup():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    arena, offsets = _arena(LENS, starts_odd=set(range(len(LENS))), seed=17)
    assert all(int(o) % 2 == 1 for o in offsets)                              # every file starts at an odd byte
    return dict(m=m, ctx=ctx, arena=arena, offsets=offsets, lens=np.array(LENS, dtype=np.uint64), d_arena=torch.from_numpy(arena).cuda())


def _yardstick(s, d_arena, g, lens=None, offsets=None):
    m = s["m"]
    lens, offsets = (s["lens"] if lens is None else lens), (s["offsets"] if offsets is None else offsets)
    return m.bao.outboard_batch(s["ctx"], d_arena, offsets, lens) if g == 0 else m.bao.outboard_groups_batch(s["ctx"], d_arena, offsets, lens, g)


@functools.lru_cache(maxsize=None)
def _old(g):
    """the outboards and roots of the arena before any write"""
    s = _setup()
    return _yardstick(s, s["d_arena"], g)


def _covered(ranges):
    """file -> the sorted chunks its ranges cover"""
    out = {}
    for f, a, c in ranges:
        out.setdefault(f, set()).update(range(a, min(_n(f), a + c)))
    return {f: sorted(v) for f, v in out.items() if v}


def _write(s, d_arena, cov, salt=0):
    """a byte flipped in every covered chunk, on the device, in place"""
    import torch
    pos = []
    for f, chunks in cov.items():
        for c in chunks:
            size = min(K, LENS[f] - c * K)
            if size > 0:
                pos.append(int(s["offsets"][f]) + c * K + (c * 7 + salt) % size)
    if pos:
        idx = torch.tensor(sorted(set(pos)), dtype=torch.int64, device="cuda")
        d_arena[idx] = d_arena[idx] ^ 1


def _guarded(d_obs):
    import torch
    buf = torch.full((d_obs.numel() + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + d_obs.numel()] = d_obs
    return buf, buf[GUARD:GUARD + d_obs.numel()]


def _guards_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all().item()) and bool((buf[-GUARD:] == 0xA5).all().item())


def _update(s, d_arena, d_obs, d_roots, ranges, g, **kw):
    s["m"].bao.outboard_update_batch(s["ctx"], d_arena, s["offsets"], s["lens"], d_obs, d_roots, [r[0] for r in ranges], [r[1] for r in ranges],
                                      [r[2] for r in ranges], group_log=g, **kw)


@functools.lru_cache(maxsize=None)
def _spans(n_units):
    return np.array(GR.node_spans(n_units), dtype=np.int64).reshape(-1, 2)


def _splits(n, depth=3):
    """the chunk boundaries of the top `depth` levels of splits of a tree over n chunks"""
    out, todo = [], [(0, n)]
    for _ in range(depth):
        nxt = []
        for first, m in todo:
            if m > 1:
                k = 1
                while k * 2 < m:
                    k *= 2
                out.append(first + k)
                nxt += [(first, k), (first + k, m - k)]
        todo = nxt
    return sorted(set(out))


def _scenarios():
    F, F2 = _ragged(2051), _whole(2051)
    every = range(len(LENS))
    sc = {
        "chunk 0 of every file": [(f, 0, 1) for f in every],
        "the ragged last chunk": [(f, _n(f) - 1, 1) for f in [1] + [_ragged(k) for k in COUNTS]],
        "both sides of the top three splits": [(f, b - 1, 2) for f in every if _n(f) >= 2 for b in _splits(_n(f))],
        "across a tile boundary": [(F, 1020, 11), (F2, 1020, 11), (_ragged(1025), 1020, 5), (_whole(1025), 1020, 5)],
        "one chunk in each of two tiles": [(F, 5, 1), (F, 1500, 1), (_whole(1025), 1024, 1), (_whole(1025), 1, 1)],
        "whole files": [(F, 0, 2051), (_ragged(3), 0, 3), (_whole(65), 0, 65), (0, 0, 1)],
        "overlapping, duplicate and unsorted": [(F, 1500, 10), (F, 3, 2), (_whole(65), 10, 50), (F, 1505, 20), (F, 3, 2), (_whole(65), 0, 20), (F, 2050, 1),
                                                (_ragged(64), 63, 1), (F, 4, 0), (_ragged(64), 63, 1), (_ragged(1023), 1000, 23), (_ragged(1023), 900, 101)],
        "one small file": [(_ragged(2), 1, 1)],
        "no range": [],
    }
    return sc


def _masks(s, cov, g, ob_first):
    """(arena bytes the call may read, outboard bytes it may write) as numpy bool arrays, by the contract: of a dirty file of more than 64
    chunks the dirty units' bytes and the nodes with a dirty unit below them; of a dirty file of at most 64 chunks everything; else nothing"""
    read = np.zeros(s["arena"].size, dtype=bool)
    write = np.zeros(int(ob_first[-1]), dtype=bool)
    for f, chunks in cov.items():
        off, n = int(s["offsets"][f]), _n(f)
        a, b = int(ob_first[f]), int(ob_first[f + 1])
        if n <= 64:
            read[off:off + LENS[f]] = True
            write[a:b] = True
            continue
        nu = (n + (1 << g) - 1) >> g
        dirty = np.zeros(nu + 1, dtype=np.int64)
        for u in sorted({c >> g for c in chunks}):
            dirty[u + 1] = 1
            read[off + (u << g) * K:off + min(LENS[f], ((u + 1) << g) * K)] = True
        below = np.cumsum(dirty)
        sp = _spans(nu)
        hit = np.nonzero(below[sp[:, 0] + sp[:, 1]] - below[sp[:, 0]] > 0)[0]
        for i in hit:
            write[a + 8 + 64 * i:a + 8 + 64 * i + 64] = True
    return read, write


@pytest.mark.parametrize("g", GS)
def test_every_dirty_set_against_the_batch_call_and_nothing_else_is_touched(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    old = _old(g)
    ob_first = [int(x) for x in old["ob_first"]]
    total = ob_first[-1]
    ee = torch.full((), 0xEE, dtype=torch.uint8, device="cuda")
    for name, ranges in _scenarios().items():
        cov = _covered(ranges)
        d_now = s["d_arena"].clone()
        _write(s, d_now, cov)
        want = _yardstick(s, d_now, g)
        changed = [f for f in cov if LENS[f]]
        assert all(not torch.equal(want["roots"][f], old["roots"][f]) for f in changed), name
        # every byte
        buf, d_obs = _guarded(old["outboards"])
        d_roots = old["roots"].clone()
        _update(s, d_now, d_obs, d_roots, ranges, g, ob_first=old["ob_first"] if len(ranges) % 2 else None)
        torch.cuda.synchronize()
        assert torch.equal(d_obs, want["outboards"]), (g, name, int((d_obs != want["outboards"]).nonzero()[0].item()))
        assert torch.equal(d_roots, want["roots"]), (g, name)
        assert _guards_intact(buf), (g, name)
        # nothing else: poison what the call may neither read nor write
        read, write = _masks(s, cov, g, ob_first)
        d_read, d_write = torch.from_numpy(read).cuda(), torch.from_numpy(write).cuda()
        d_poisoned = torch.where(d_read, d_now, ee)
        buf, d_obs = _guarded(torch.where(d_write, old["outboards"], ee))
        d_roots = old["roots"].clone()
        _update(s, d_poisoned, d_obs, d_roots, ranges, g)
        torch.cuda.synchronize()
        expect = torch.where(d_write, want["outboards"], ee)
        assert torch.equal(d_obs, expect), (g, name, int((d_obs != expect).nonzero()[0].item()))
        assert torch.equal(d_roots, want["roots"]), (g, name)                # (a file without a dirty range: its old root)
        assert _guards_intact(buf), (g, name)
        for f in range(len(LENS)):
            if f not in cov:
                assert not write[ob_first[f]:ob_first[f + 1]].any() and not read[int(s["offsets"][f]):int(s["offsets"][f]) + LENS[f]].any()
        # end to end: the updated outboards verify, and the written chunks' paths plan from them
        buf, d_obs = _guarded(old["outboards"])
        d_roots = old["roots"].clone()
        _update(s, d_now, d_obs, d_roots, ranges, g)
        out = m.bao.verify_batch(ctx, d_now, s["offsets"], s["lens"], d_obs, d_roots, g)
        assert not out["unit_status"].any().item() and not out["file_status"].any().item(), (g, name)
        samples = [(f, c) for f, chunks in cov.items() for c in chunks]
        if 0 < len(samples) <= 300:
            plan = m.bao.plan_samples_arena(ctx, d_now, s["offsets"], s["lens"], d_obs, d_roots, [f for f, _ in samples], [c for _, c in samples], g)
            assert (plan["sample_status"] == 0).all(), (g, name)
    assert total == int(old["outboards"].numel())


@pytest.mark.parametrize("g", [0, 4])
def test_a_file_of_1026_tiles_reaches_the_second_merge_launch(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(256)
    lens = [3000, (1 << 30) + (1 << 20) + 5, 1, 70 * 1024]
    offsets = np.array([0, 3008, 3008 + lens[1] + 3, 3008 + lens[1] + 16], dtype=np.uint64)
    d_arena = torch.randint(0, 256, (int(offsets[3]) + lens[3],), dtype=torch.uint8, device="cuda", generator=gen)
    old = _yardstick(s, d_arena, g, lens, offsets)
    n = m.bao.num_chunks(lens[1])
    assert n == 1025 * 1024 + 1
    chunks = [5, 1023 * 1024 + 7, 1024 * 1024, n - 1]                          # tile 0, tile 1 023, tile 1 024 and the last (5 bytes)
    ranges = [(1, c, 1) for c in chunks] + [(3, 69, 1), (0, 2, 1)]
    for f, c, _ in ranges:
        d_arena[int(offsets[f]) + c * K + 3] ^= 1
    buf, d_obs = _guarded(old["outboards"])
    d_roots = old["roots"].clone()
    fi, fc, nc = np.array([r[0] for r in ranges], dtype=np.uint32), np.array([r[1] for r in ranges], dtype=np.uint64), np.ones(len(ranges), dtype=np.uint64)
    ln = np.array(lens, dtype=np.uint64)
    assert m.lib().b3w_bao_update_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size) == 32 * (4 + 2)
    m.bao.outboard_update_batch(ctx, d_arena, offsets, lens, d_obs, d_roots, fi, fc, nc, group_log=g)
    want = _yardstick(s, d_arena, g, lens, offsets)
    torch.cuda.synchronize()
    assert not torch.equal(want["roots"][1], old["roots"][1]) and torch.equal(want["roots"][2], old["roots"][2])
    assert torch.equal(d_obs, want["outboards"]) and torch.equal(d_roots, want["roots"]) and _guards_intact(buf)
    # and sparse: only the nodes above the four chunks differ from before (20 levels at g = 0 over 2^20 + 1 025 chunks, fewer where they share)
    a, b = int(old["ob_first"][1]) + 8, int(old["ob_first"][2])
    differ = (d_obs[a:b].view(-1, 64) != old["outboards"][a:b].view(-1, 64)).any(dim=1).sum().item()
    assert 0 < differ <= 4 * 21, differ


@pytest.mark.parametrize("g", [4, 6])
def test_forty_repeated_calls_on_freshly_drawn_dirty_sets(g):
    """every byte after each of 40 calls that build on one another: the check for a level loop's barrier without its wait for the LDS
    stores before it, which shows only now and then (the r09 finding)"""
    import torch
    s = _setup()
    rng = np.random.default_rng(40 + g)
    old = _old(g)
    buf, d_obs = _guarded(old["outboards"])
    d_roots = old["roots"].clone()
    d_now = s["d_arena"].clone()
    big = [f for f in range(len(LENS)) if _n(f) > 64]
    for k in range(40):
        ranges = []
        for _ in range(int(rng.integers(1, 9))):
            f = int(rng.choice(big)) if rng.random() < 0.8 else int(rng.integers(0, len(LENS)))
            a = int(rng.integers(0, _n(f)))
            ranges.append((f, a, int(rng.integers(1, min(_n(f) - a, 70) + 1))))
        _write(s, d_now, _covered(ranges), salt=k)
        _update(s, d_now, d_obs, d_roots, ranges, g)
        want = _yardstick(s, d_now, g)
        assert torch.equal(d_obs, want["outboards"]) and torch.equal(d_roots, want["roots"]), (g, k, ranges)
    assert _guards_intact(buf)


def test_the_call_makes_the_scratch_and_no_other_device_memory():
    import torch
    s = _setup()
    m = s["m"]
    g = 1
    old = _old(g)
    F = _ragged(2051)
    ranges = [(F, 5, 1), (F, 1500, 1), (F, 2050, 1), (_whole(1025), 1024, 1), (_whole(1024), 7, 2), (_ragged(3), 0, 1)]
    d_obs, d_roots = old["outboards"].clone(), old["roots"].clone()
    _update(s, s["d_arena"], d_obs, d_roots, ranges, g)                       # (warm: the context's staging slot is its own)
    fi, fc, nc = (np.array([r[i] for r in ranges], dtype=t) for i, t in ((0, np.uint32), (1, np.uint64), (2, np.uint64)))
    need = m.lib().b3w_bao_update_scratch_bytes(s["lens"].ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)
    assert need == 32 * 4                                                      # three tiles of F and one of the 1 025-chunk file; one-tile files: none
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    _update(s, s["d_arena"], d_obs, d_roots, ranges, g)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - start
    print(f"outboard_update_batch: device memory rose by {rise} bytes for a scratch of {need}")
    assert rise == (need + 511) // 512 * 512                                   # (the allocator hands out multiples of 512)
    assert torch.equal(d_obs, old["outboards"]) and torch.equal(d_roots, old["roots"])   # (nothing was written to the files: the same bytes again)


def test_refusals_are_atomic_and_name_the_range():
    import torch
    s = _setup()
    m = s["m"]
    L = m.lib()
    ctx = m.Context("compression", 0)                                         # (any context updates)
    g = 1
    old = _old(g)
    buf, d_obs = _guarded(old["outboards"])
    d_roots = old["roots"].clone()
    d_arena, offsets, lens = s["d_arena"], s["offsets"], s["lens"]
    obf = np.ascontiguousarray(old["ob_first"], dtype=np.uint64)
    F, E = _ragged(2051), 0
    good = [(F, 5, 1), (_whole(1025), 1020, 5), (_ragged(3), 1, 1), (E, 0, 1)]
    fi, fc, nc = (np.array([r[i] for r in good], dtype=t) for i, t in ((0, np.uint32), (1, np.uint64), (2, np.uint64)))
    need = L.b3w_bao_update_scratch_bytes(lens.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)
    assert need == 32 * 3
    d_scratch = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    bad = m.B3W_E_BAD_ARGUMENT
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena=d_arena.data_ptr(), arena_bytes=d_arena.numel(), off=offsets.ctypes.data, ln=lens.ctypes.data, n_files=lens.size, gl=g, ob_first=obf.ctypes.data,
             obs=d_obs.data_ptr(), roots=d_roots.data_ptr(), files=fi.ctypes.data, first=fc.ctypes.data, count=nc.ctypes.data, n=fi.size,
             scratch=d_scratch.data_ptr(), scratch_bytes=need):
        return L.b3w_bao_outboard_update_batch_device(ctx.handle, arena, arena_bytes, off, ln, n_files, gl, ob_first, obs, roots, files, first, count, n,
                                                      scratch, scratch_bytes, stream)
    for kw, word in ((dict(off=None), "null"), (dict(ln=None), "null"), (dict(ob_first=None), "null"), (dict(obs=None), "null"), (dict(roots=None), "null"),
                     (dict(files=None), "null"), (dict(first=None), "null"), (dict(count=None), "null"), (dict(arena=None), "null arena"),
                     (dict(gl=7), "group_log"), (dict(obs=d_obs.data_ptr() + 4), "8-byte aligned"), (dict(scratch_bytes=need - 1), "scratch"),
                     (dict(scratch=None), "scratch"), (dict(scratch=d_scratch.data_ptr() + 8), "scratch"),
                     (dict(n_files=F), "range 0 (file %d, chunks 5 + 1): the file index" % F),
                     (dict(arena_bytes=int(offsets[F]) + LENS[F] - 1), "range 0 (file %d, chunks 5 + 1): the file reaches past arena_bytes" % F)):
        assert call(**kw) == bad, kw
        assert word in ctx.last_error(), (kw, ctx.last_error())
    # a bad range behind good ones: nothing of the good ones is done
    for f, a, c, word in ((len(LENS), 0, 1, "file index"), (F, 2051, 1, "reaches past the file's 2051 chunks"), (F, 2000, 52, "reaches past"),
                          (E, 1, 1, "reaches past the file's 1 chunks"), (_ragged(1), 0, 2, "reaches past"), (F, 1 << 63, 1 << 63, "reaches past")):
        fi2, fc2, nc2 = np.append(fi, np.uint32(f)), np.append(fc, np.uint64(a)), np.append(nc, np.uint64(c))
        assert call(files=fi2.ctypes.data, first=fc2.ctypes.data, count=nc2.ctypes.data, n=fi2.size, scratch_bytes=need + 16) == bad, (f, a, c)
        assert word in ctx.last_error() and "range 4 (file %d, chunks %d + %d)" % (f, a, c) in ctx.last_error(), ctx.last_error()
    assert L.b3w_bao_outboard_update_batch_device(None, None, 0, None, None, 0, 0, None, None, None, None, None, None, 0, None, 0, None) == bad
    with pytest.raises(m.B3WError):
        m.bao.outboard_update_batch(ctx, d_arena, offsets, lens, d_obs, d_roots, [len(LENS)], [0], [1], group_log=g)
    with pytest.raises(m.B3WError):
        m.bao.outboard_update_batch(ctx, d_arena, offsets, lens, d_obs, d_roots, [F], [2051], [1], group_log=g)
    with pytest.raises(m.B3WError):
        m.bao.outboard_update_batch(ctx, d_arena, offsets, lens, d_obs[:-64], d_roots, [F], [0], [1], group_log=g)
    torch.cuda.synchronize()
    assert torch.equal(d_obs, old["outboards"]) and torch.equal(d_roots, old["roots"]) and _guards_intact(buf)
    assert bool((d_scratch == 0x5A).all().item())
    # no range, or ranges of no chunks: B3W_OK and nothing launched; then the good ranges on the untouched arena: the same bytes again
    assert call(n=0) == 0 and call(n=0, files=None, first=None, count=None, scratch=None, scratch_bytes=0) == 0
    zero = np.zeros(fi.size, dtype=np.uint64)
    assert call(count=zero.ctypes.data, scratch=None, scratch_bytes=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(d_obs, old["outboards"]) and bool((d_scratch == 0x5A).all().item())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(d_obs, old["outboards"]) and torch.equal(d_roots, old["roots"]) and _guards_intact(buf)
    assert not bool((d_scratch[:need] == 0x5A).all().item()) and bool((d_scratch[need:] == 0x5A).all().item())
    ctx.close()
