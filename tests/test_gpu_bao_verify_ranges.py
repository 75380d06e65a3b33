"""Listed chunk ranges of resident files verified against their outboards (bao.verify_ranges_batch,
b3w_bao_verify_ranges_batch_device).  The oracle is always the whole-file call, bao.verify_batch, on the same (tampered) arena,
outboards and roots, read at the listed units; the per-range outputs are held against a host reduction of the oracle's bytes.  The
unit statuses sit between 0xA5 guards over a 0xEE prefill: every byte that is not of a listed unit (or of a listed file of at most 64
chunks) is still 0xEE afterwards.  What the contract says is not read is shown by poison: every arena byte outside the listed units,
every stored node with no listed unit below it and everything of the files without a range is 0xEE, and the result is unchanged."""
import functools

import numpy as np
import pytest

import b3w_testlib as T
from test_gpu_bao_batch import _arena
from test_gpu_bao_update import GS, GUARD, K, LENS, _covered, _n, _ragged, _scenarios, _spans, _whole

pytestmark = pytest.mark.gpu

NONE = -1                                                                 # UINT64_MAX as the int64 the Python call returns
FILL = 0xEE


@functools.lru_cache(maxsize=None)
def _setup():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    arena, offsets = _arena(LENS, starts_odd=set(range(len(LENS))), seed=19)
    assert all(int(o) % 2 == 1 for o in offsets)                              # every file starts at an odd byte
    return dict(m=m, ctx=ctx, arena=arena, offsets=offsets, lens=np.array(LENS, dtype=np.uint64), d_arena=torch.from_numpy(arena).cuda())


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """every device tensor of this module (the arena, the oracles, the 1 GiB file) comes from a pool of the allocator that is the
    module's own and goes with it: the modules behind this one that measure device memory find the default pool as they would without it"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        if _setup.cache_info().currsize:
            _setup()["ctx"].close()
        _made.cache_clear()
        _setup.cache_clear()
        gc.collect()
    del pool


@functools.lru_cache(maxsize=None)
def _made(g):
    """the outboards and roots of the untouched arena, computed once and left unchanged; unit_first beside them"""
    s = _setup()
    m = s["m"]
    out = m.bao.outboard_batch(s["ctx"], s["d_arena"], s["offsets"], s["lens"]) if g == 0 else \
        m.bao.outboard_groups_batch(s["ctx"], s["d_arena"], s["offsets"], s["lens"], g)
    out["unit_first"] = m.bao.verify_layout(s["lens"], g)
    return out


def _oracle(s, d_arena, d_obs, d_roots, g):
    out = s["m"].bao.verify_batch(s["ctx"], d_arena, s["offsets"], s["lens"], d_obs, d_roots, g)
    return out["unit_status"].cpu().numpy()


def _listed(ranges, g, uf, lens=LENS):
    """bool per packed unit: the call writes it (a unit with a listed chunk; every unit of a listed file of at most 64 chunks)"""
    out = np.zeros(int(uf[-1]), dtype=bool)
    for f, a, c in ranges:
        n = max(1, -(-int(lens[f]) // K))
        if c == 0:
            continue
        if n <= 64:
            out[int(uf[f]):int(uf[f + 1])] = True
        else:
            out[int(uf[f]) + (a >> g):int(uf[f]) + ((a + c - 1) >> g) + 1] = True
    return out


def _reduced(want, ranges, g, uf):
    rs, rf = [], []
    for f, a, c in ranges:
        w = want[int(uf[f]) + (a >> g):int(uf[f]) + ((a + c - 1) >> g) + 1] if c else want[:0]
        bad = np.nonzero(w)[0]
        rs.append(int(w.max()) if w.size else 0)
        rf.append((a >> g) + int(bad[0]) if bad.size else NONE)
    return rs, rf


def _ranged(s, d_arena, d_obs, d_roots, ranges, g, uf, **kw):
    """the ranged call over a guarded 0xEE prefill -> (unit bytes numpy, range statuses, range first bad units)"""
    import torch
    total = int(uf[-1])
    buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + total] = FILL
    out = s["m"].bao.verify_ranges_batch(s["ctx"], d_arena, s["offsets"], s["lens"], d_obs, d_roots, [r[0] for r in ranges], [r[1] for r in ranges],
                                         [r[2] for r in ranges], group_log=g, unit_status=buf[GUARD:GUARD + total], **kw)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all().item()) and bool((buf[-GUARD:] == 0xA5).all().item())
    return buf[GUARD:GUARD + total].cpu().numpy(), out["range_status"].cpu().tolist(), out["range_first_bad"].cpu().tolist()


def _held(s, d_arena, d_obs, d_roots, ranges, g, uf, tag, want=None, **kw):
    """the ranged call against the oracle on the same inputs; -> (the listed mask, the ranged call's three outputs)"""
    want = _oracle(s, d_arena, d_obs, d_roots, g) if want is None else want
    got = _ranged(s, d_arena, d_obs, d_roots, ranges, g, uf, **kw)
    listed = _listed(ranges, g, uf)
    assert (got[0][listed] == want[listed]).all(), (tag, np.nonzero(listed & (got[0] != want))[0][:5])
    assert (got[0][~listed] == FILL).all(), (tag, np.nonzero(~listed & (got[0] != FILL))[0][:5])
    assert (got[1], got[2]) == _reduced(want, ranges, g, uf), tag
    return listed, got


def _masks(s, ranges, g, ob_first):
    """(arena bytes, outboard bytes, files) the call may read, by the contract: of a listed file of more than 64 chunks the listed units'
    bytes, the header and the nodes with a listed unit below them; of a listed file of at most 64 chunks everything; else nothing"""
    arena = np.zeros(s["arena"].size, dtype=bool)
    obs = np.zeros(int(ob_first[-1]), dtype=bool)
    cov = _covered(ranges)
    for f, chunks in cov.items():
        off, n = int(s["offsets"][f]), _n(f)
        a, b = int(ob_first[f]), int(ob_first[f + 1])
        if n <= 64:
            arena[off:off + LENS[f]] = True
            obs[a:b] = True
            continue
        obs[a:a + 8] = True
        nu = (n + (1 << g) - 1) >> g
        hit = np.zeros(nu + 1, dtype=np.int64)
        for u in sorted({c >> g for c in chunks}):
            hit[u + 1] = 1
            arena[off + (u << g) * K:off + min(LENS[f], ((u + 1) << g) * K)] = True
        below = np.cumsum(hit)
        sp = _spans(nu)
        for i in np.nonzero(below[sp[:, 0] + sp[:, 1]] - below[sp[:, 0]] > 0)[0]:
            obs[a + 8 + 64 * i:a + 8 + 64 * i + 64] = True
    return arena, obs, sorted(cov)


@pytest.mark.parametrize("g", GS)
def test_every_range_set_against_the_whole_file_call_and_nothing_else_is_read_or_written(g):
    import torch
    s = _setup()
    made = _made(g)
    uf, ob_first = made["unit_first"], [int(x) for x in made["ob_first"]]
    clean = _oracle(s, s["d_arena"], made["outboards"], made["roots"], g)
    assert not clean.any()
    ee = torch.full((), FILL, dtype=torch.uint8, device="cuda")
    for name, ranges in _scenarios().items():
        listed, got = _held(s, s["d_arena"], made["outboards"], made["roots"], ranges, g, uf, (g, name), want=clean,
                            ob_first=made["ob_first"] if len(ranges) % 2 else None, unit_first=uf if len(ranges) % 3 else None)
        assert not got[0][listed].any() and not any(got[1]) and all(x == NONE for x in got[2]), (g, name)
        # poison on the device, the ranges in reverse order: the same bytes
        a_ok, o_ok, files = _masks(s, ranges, g, ob_first)
        d_arena = torch.where(torch.from_numpy(a_ok).cuda(), s["d_arena"], ee)
        d_obs = torch.where(torch.from_numpy(o_ok).cuda(), made["outboards"], ee)
        r_ok = torch.zeros(len(LENS), dtype=torch.bool)
        if files:
            r_ok[files] = True
        d_roots = torch.where(r_ok.cuda()[:, None], made["roots"].view(len(LENS), 8), torch.full((), -286331154, dtype=made["roots"].dtype, device="cuda"))
        back = list(reversed(ranges))
        p = _ranged(s, d_arena, d_obs, d_roots.contiguous(), back, g, uf)
        assert (p[0] == got[0]).all(), (g, name, np.nonzero(p[0] != got[0])[0][:5])
        assert (p[1], p[2]) == (list(reversed(got[1])), list(reversed(got[2]))), (g, name)


def _node_over(nu, units, smallest=True):
    """the index of the smallest (or largest but one: the root's left child) stored node over all of `units`"""
    sp = _spans(nu)
    over = [i for i in range(len(sp)) if sp[i, 0] <= min(units) and max(units) < sp[i, 0] + sp[i, 1]]
    return over[-1] if smallest else 1


@pytest.mark.parametrize("g", GS)
def test_one_tamper_each_is_reported_as_the_whole_file_call_reports_it(g):
    import torch
    s = _setup()
    made = _made(g)
    uf, ob_first = made["unit_first"], [int(x) for x in made["ob_first"]]
    F, W, S = _ragged(2051), _whole(1025), _ragged(3)
    nu = (2051 + (1 << g) - 1) >> g
    two_tiles = [(F, 5, 1), (F, 1500, 1), (W, 1024, 1), (S, 1, 1), (F, 1500, 0)]   # F: tiles 0 and 1 of 3; W: its one-chunk last tile
    last_tile = [(F, 2050, 1), (W, 3, 2)]                                      # F: tile 2 alone
    at_f, ob_f = int(s["offsets"][F]), ob_first[F]
    pair_5 = _node_over(nu, [(5 >> g) & ~1, ((5 >> g) & ~1) + 1])              # the lowest stored node over chunk 5's unit
    pair_700 = _node_over(nu, [(700 >> g) & ~1, ((700 >> g) & ~1) + 1])        # the same over chunk 700's: no listed unit below it
    cases = [                                                                  # name, ranges, what is flipped, the listed statuses that must show
        ("a listed chunk's byte", two_tiles, ("arena", at_f + 5 * K + 9), {1}),
        ("an unlisted chunk's byte in a listed tile", two_tiles, ("arena", at_f + 700 * K + 9), set()),
        ("an unlisted tile's byte", two_tiles, ("arena", at_f + 2050 * K + 9), set()),
        ("a tile-level node on a listed path", two_tiles, ("obs", ob_f + 8 + 64 * pair_5 + 40), {2}),
        ("a tile-level node on no listed path", two_tiles, ("obs", ob_f + 8 + 64 * pair_700 + 3), set()),
        ("a node of the storey above on a listed path", two_tiles, ("obs", ob_f + 8 + 64 * 1 + 33), {2}),
        ("the root node of the storey above", last_tile, ("obs", ob_f + 8 + 5), {2}),
        ("a node of the storey above on no listed path", last_tile, ("obs", ob_f + 8 + 64 * 1 + 33), set()),
        ("a root", two_tiles, ("roots", F * 8 + 2), {2}),
        ("a small file's root", two_tiles, ("roots", S * 8), {2} if g < 2 else {1}),    # (three chunks: one unit from g = 2 on, and then a wrong root is 1)
        ("a header", two_tiles, ("obs", ob_f + 1), {3}),
        ("a small file's header", two_tiles, ("obs", ob_first[S] + 7), {3}),
        ("an unlisted file's header, root and bytes", two_tiles, ("all", _whole(1024)), set()),
    ]
    for name, ranges, (what, at), shows in cases:
        d_arena, d_obs, d_roots = s["d_arena"].clone(), made["outboards"].clone(), made["roots"].clone().view(-1)
        if what in ("arena", "all"):
            d_arena[at if what == "arena" else int(s["offsets"][at]) + 77] ^= 0x20
        if what in ("obs", "all"):
            d_obs[at if what == "obs" else ob_first[at]] ^= 0x20
        if what in ("roots", "all"):
            d_roots[at if what == "roots" else at * 8] ^= 0x20
        listed, got = _held(s, d_arena, d_obs, d_roots, ranges, g, uf, (g, name))
        assert set(got[0][listed].tolist()) - {0} == shows, (g, name, set(got[0][listed].tolist()))
        assert set(got[1]) - {0} == shows, (g, name, got[1])


@pytest.mark.parametrize("g", [0, 4])
def test_a_file_of_1026_tiles_runs_the_storey_above_twice(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(257)
    lens = [3000, (1 << 30) + (1 << 20) + 5, 1, 70 * 1024]
    offsets = np.array([0, 3008, 3008 + lens[1] + 3, 3008 + lens[1] + 16], dtype=np.uint64)
    d_arena = torch.randint(0, 256, (int(offsets[3]) + lens[3],), dtype=torch.uint8, device="cuda", generator=gen)
    made = m.bao.outboard_batch(ctx, d_arena, offsets, lens) if g == 0 else m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
    uf = m.bao.verify_layout(lens, g)
    n = m.bao.num_chunks(lens[1])
    assert n == 1025 * 1024 + 1
    # tile 0, tile 1 023, across the 1 GiB split, the last tile (one chunk of 5 bytes), and two other files
    ranges = [(1, n - 1, 1), (1, 5, 2), (1, 1023 * 1024 + 7, 1), (1, 1024 * 1024 - 3, 6), (3, 69, 1), (0, 2, 1)]
    fi, fc, nc = (np.array([r[i] for r in ranges], dtype=t) for i, t in ((0, np.uint32), (1, np.uint64), (2, np.uint64)))
    ln = np.array(lens, dtype=np.uint64)
    assert m.lib().b3w_bao_verify_ranges_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size) == (36 * (4 + 2) + 15) // 16 * 16
    listed = torch.from_numpy(_listed(ranges, g, uf, lens)).cuda()
    first_span = (1 << 20) >> g                                                # the units of the first 1 024 tiles
    for name, flip in (("clean", None), ("a bad node in the top storey", int(made["ob_first"][1]) + 8 + 64 * 1 + 17)):
        d_obs = made["outboards"].clone()
        if flip is not None:
            d_obs[flip] ^= 1                                                   # the root's left child: the node over the first span
        want = m.bao.verify_batch(ctx, d_arena, offsets, lens, d_obs, made["roots"], g)["unit_status"]
        st = torch.full_like(want, FILL)
        out = m.bao.verify_ranges_batch(ctx, d_arena, offsets, lens, d_obs, made["roots"], fi, fc, nc, group_log=g, unit_status=st)
        torch.cuda.synchronize()
        assert torch.equal(st[listed], want[listed]) and bool((st[~listed] == FILL).all().item()), (g, name)
        rs, rf = _reduced(want.cpu().numpy(), ranges, g, uf)
        assert (out["range_status"].cpu().tolist(), out["range_first_bad"].cpu().tolist()) == (rs, rf), (g, name)
        if flip is None:
            assert not any(rs)
        else:                                                                  # exactly the ranges below the first span's node
            assert rs == [0, 2, 2, 2, 0, 0] and rf == [NONE, 5 >> g, (1023 * 1024 + 7) >> g, (1024 * 1024 - 3) >> g, NONE, NONE]
            f1 = int(uf[1])
            assert int(st[f1 + first_span - 1].item()) == 2 and int(st[f1 + first_span].item()) == 0


def test_the_call_makes_the_scratch_and_the_range_outputs_and_no_other_device_memory():
    import torch
    s = _setup()
    m = s["m"]
    L = m.lib()
    g = 1
    made = _made(g)
    uf = made["unit_first"]
    F = _ragged(2051)
    ranges = [(F, 5, 1), (F, 1500, 1), (F, 2050, 1), (_whole(1025), 1024, 1), (_whole(1024), 7, 2), (_ragged(3), 0, 1)]
    st = torch.full((int(uf[-1]),), FILL, dtype=torch.uint8, device="cuda")

    def run():
        return m.bao.verify_ranges_batch(s["ctx"], s["d_arena"], s["offsets"], s["lens"], made["outboards"], made["roots"], [r[0] for r in ranges],
                                         [r[1] for r in ranges], [r[2] for r in ranges], group_log=g, ob_first=made["ob_first"], unit_first=uf, unit_status=st)
    first = run()                                                              # (warm: the context's staging slot is its own)
    fi, fc, nc = (np.array([r[i] for r in ranges], dtype=t) for i, t in ((0, np.uint32), (1, np.uint64), (2, np.uint64)))
    need = L.b3w_bao_verify_ranges_scratch_bytes(s["lens"].ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)
    assert need == (36 * 4 + 15) // 16 * 16                                    # three tiles of F and one of the 1 025-chunk file; one-tile files: none
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    out = run()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - start
    print(f"verify_ranges_batch: device memory rose by {rise} bytes for a scratch of {need} and {len(ranges)} ranges")
    assert rise == (need + 511) // 512 * 512 + 2 * 512                         # (the allocator hands out multiples of 512: scratch, statuses, first bad)
    assert torch.equal(out["range_status"], first["range_status"]) and not out["range_status"].any().item()
    # the C call with everything handed in: a second call allocates nothing at all
    d_scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    rs, rf = torch.empty(len(ranges), dtype=torch.int32, device="cuda"), torch.empty(len(ranges), dtype=torch.int64, device="cuda")
    obf = np.ascontiguousarray(made["ob_first"], dtype=np.uint64)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    free0 = torch.cuda.mem_get_info()[0]
    assert L.b3w_bao_verify_ranges_batch_device(s["ctx"].handle, s["d_arena"].data_ptr(), s["d_arena"].numel(), s["offsets"].ctypes.data, s["lens"].ctypes.data,
                                                s["lens"].size, g, obf.ctypes.data, made["outboards"].data_ptr(), made["roots"].data_ptr(), fi.ctypes.data,
                                                fc.ctypes.data, nc.ctypes.data, fi.size, uf.ctypes.data, st.data_ptr(), rs.data_ptr(), rf.data_ptr(),
                                                d_scratch.data_ptr(), need, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == start and torch.cuda.mem_get_info()[0] >= free0   # (neither the allocator's memory nor the device's)
    assert not rs.any().item() and bool((rf == NONE).all().item())


def test_refusals_are_atomic_and_name_the_range():
    import torch
    s = _setup()
    m = s["m"]
    L = m.lib()
    ctx = m.Context("compression", 0)                                         # (any context verifies)
    g = 1
    made = _made(g)
    d_arena, offsets, lens = s["d_arena"], s["offsets"], s["lens"]
    obf = np.ascontiguousarray(made["ob_first"], dtype=np.uint64)
    uf = np.ascontiguousarray(made["unit_first"], dtype=np.uint64)
    F, E = _ragged(2051), 0
    good = [(F, 5, 1), (_whole(1025), 1020, 5), (_ragged(3), 1, 1), (E, 0, 1)]
    fi, fc, nc = (np.array([r[i] for r in good], dtype=t) for i, t in ((0, np.uint32), (1, np.uint64), (2, np.uint64)))
    need = L.b3w_bao_verify_ranges_scratch_bytes(lens.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)
    assert need == (36 * 3 + 15) // 16 * 16
    d_scratch = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    d_st = torch.full((int(uf[-1]),), FILL, dtype=torch.uint8, device="cuda")
    d_rs = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    d_rf = torch.full((8,), 7, dtype=torch.int64, device="cuda")
    bad = m.B3W_E_BAD_ARGUMENT
    stream = torch.cuda.current_stream().cuda_stream

    def call(arena=d_arena.data_ptr(), arena_bytes=d_arena.numel(), off=offsets.ctypes.data, ln=lens.ctypes.data, n_files=lens.size, gl=g, ob_first=obf.ctypes.data,
             obs=made["outboards"].data_ptr(), roots=made["roots"].data_ptr(), files=fi.ctypes.data, first=fc.ctypes.data, count=nc.ctypes.data, n=fi.size,
             unit_first=uf.ctypes.data, st=d_st.data_ptr(), rs=d_rs.data_ptr(), rf=d_rf.data_ptr(), scratch=d_scratch.data_ptr(), scratch_bytes=need):
        return L.b3w_bao_verify_ranges_batch_device(ctx.handle, arena, arena_bytes, off, ln, n_files, gl, ob_first, obs, roots, files, first, count, n,
                                                    unit_first, st, rs, rf, scratch, scratch_bytes, stream)

    def untouched():
        torch.cuda.synchronize()
        return bool((d_st == FILL).all().item()) and bool((d_rs == -7).all().item()) and bool((d_rf == 7).all().item()) and bool((d_scratch == 0x5A).all().item())
    obf_off, lens_long = obf.copy(), lens.copy()
    obf_off[F] += 4
    lens_long[F] = (1 << 40) + 1025
    for kw, word in ((dict(ob_first=obf_off.ctypes.data), "range 0 (file %d, chunks 5 + 1): the file's outboard offset is not a multiple of 8" % F),
                     (dict(ln=lens_long.ctypes.data), "range 0 (file %d, chunks 5 + 1): a file of more than 2^30 chunks" % F),
                     (dict(off=None), "null"), (dict(ln=None), "null"), (dict(ob_first=None), "null"), (dict(obs=None), "null"), (dict(roots=None), "null"),
                     (dict(files=None), "null"), (dict(first=None), "null"), (dict(count=None), "null"), (dict(arena=None), "null arena"),
                     (dict(unit_first=None), "null"), (dict(st=None), "null output"), (dict(rs=None), "null output"), (dict(rf=None), "null output"),
                     (dict(rf=d_rf.data_ptr() + 4), "d_range_first_bad is not 8-byte aligned"), (dict(rs=d_rs.data_ptr() + 2), "d_range_status not 4-byte aligned"),
                     (dict(gl=7), "group_log"), (dict(obs=made["outboards"].data_ptr() + 4), "8-byte aligned"), (dict(scratch_bytes=need - 1), "scratch"),
                     (dict(scratch=None), "scratch"), (dict(scratch=d_scratch.data_ptr() + 8), "scratch"),
                     (dict(n_files=F), "range 0 (file %d, chunks 5 + 1): the file index" % F),
                     (dict(arena_bytes=int(offsets[F]) + LENS[F] - 1), "range 0 (file %d, chunks 5 + 1): the file reaches past arena_bytes" % F)):
        assert call(**kw) == bad, kw
        assert word in ctx.last_error() and "bao verify ranges" in ctx.last_error(), (kw, ctx.last_error())
    # a bad range behind good ones: nothing of the good ones is done
    for f, a, c, word in ((len(LENS), 0, 1, "file index"), (F, 2051, 1, "reaches past the file's 2051 chunks"), (F, 2000, 52, "reaches past"),
                          (E, 1, 1, "reaches past the file's 1 chunks"), (_ragged(1), 0, 2, "reaches past"), (F, 1 << 63, 1 << 63, "reaches past")):
        fi2, fc2, nc2 = np.append(fi, np.uint32(f)), np.append(fc, np.uint64(a)), np.append(nc, np.uint64(c))
        assert call(files=fi2.ctypes.data, first=fc2.ctypes.data, count=nc2.ctypes.data, n=fi2.size, scratch_bytes=need + 16) == bad, (f, a, c)
        assert word in ctx.last_error() and "range 4 (file %d, chunks %d + %d)" % (f, a, c) in ctx.last_error(), ctx.last_error()
    assert L.b3w_bao_verify_ranges_batch_device(*[0 if i in (2, 5, 6, 13, 19) else None for i in range(21)]) == bad
    with pytest.raises(m.B3WError):
        m.bao.verify_ranges_batch(ctx, d_arena, offsets, lens, made["outboards"], made["roots"], [len(LENS)], [0], [1], group_log=g)
    with pytest.raises(m.B3WError):
        m.bao.verify_ranges_batch(ctx, d_arena, offsets, lens, made["outboards"], made["roots"], [F], [2051], [1], group_log=g, unit_status=d_st)
    with pytest.raises(m.B3WError):
        m.bao.verify_ranges_batch(ctx, d_arena, offsets, lens, made["outboards"][:-64], made["roots"], [F], [0], [1], group_log=g, unit_status=d_st)
    assert untouched()
    # no range: B3W_OK and nothing launched; ranges of no chunks: their outputs alone; then the good ranges
    assert call(n=0) == 0 and call(n=0, files=None, first=None, count=None, st=None, rs=None, rf=None, scratch=None, scratch_bytes=0) == 0
    assert untouched()
    zero = np.zeros(fi.size, dtype=np.uint64)
    assert call(count=zero.ctypes.data, scratch=None, scratch_bytes=0) == 0
    torch.cuda.synchronize()
    assert bool((d_st == FILL).all().item()) and bool((d_scratch == 0x5A).all().item())
    assert d_rs.cpu().tolist() == [0] * 4 + [-7] * 4 and d_rf.cpu().tolist() == [NONE] * 4 + [7] * 4
    assert call() == 0
    torch.cuda.synchronize()
    listed = torch.from_numpy(_listed(good, g, uf)).cuda()
    assert not d_st[listed].any().item() and bool((d_st[~listed] == FILL).all().item())
    assert d_rs.cpu().tolist() == [0] * 4 + [-7] * 4 and d_rf.cpu().tolist() == [NONE] * 4 + [7] * 4
    assert not bool((d_scratch[:need] == 0x5A).all().item()) and bool((d_scratch[need:] == 0x5A).all().item())
    ctx.close()


@pytest.mark.parametrize("g", [0, 4])
def test_after_an_update_the_listed_units_verify_and_a_missed_chunk_shows_at_its_unit(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    made = _made(g)
    uf = made["unit_first"]
    F, W = _ragged(2051), _whole(1025)
    ranges = [(F, 1020, 11), (F, 2050, 1), (W, 1024, 1), (W, 100, 3), (_ragged(3), 2, 1)]
    d_now = s["d_arena"].clone()
    for f, chunks in _covered(ranges).items():
        for c in chunks:
            d_now[int(s["offsets"][f]) + c * K + 1] ^= 0x40
    fa, fc, nc = [r[0] for r in ranges], [r[1] for r in ranges], [r[2] for r in ranges]
    # before the update the rewritten chunks are what the ranged call finds, as the whole-file call does
    listed, got = _held(s, d_now, made["outboards"], made["roots"], ranges, g, uf, (g, "before"))
    assert set(got[1]) == {1}
    d_obs, d_roots = made["outboards"].clone(), made["roots"].clone()
    m.bao.outboard_update_batch(ctx, d_now, s["offsets"], s["lens"], d_obs, d_roots, fa, fc, nc, group_log=g)
    listed, got = _held(s, d_now, d_obs, d_roots, ranges, g, uf, (g, "after"))
    assert not got[0][listed].any() and not any(got[1])
    # an update that misses one rewritten chunk (in a unit and a tile of its own): 1 at exactly its unit
    missed = 300
    d_now[int(s["offsets"][F]) + missed * K + 1] ^= 0x40
    m.bao.outboard_update_batch(ctx, d_now, s["offsets"], s["lens"], d_obs, d_roots, [F], [1500], [1], group_log=g)
    look = ranges + [(F, missed - 100, 200)]
    listed, got = _held(s, d_now, d_obs, d_roots, look, g, uf, (g, "missed"))
    hit = np.nonzero(got[0] == 1)[0].tolist()
    assert hit == [int(uf[F]) + (missed >> g)] and got[1] == [0] * len(ranges) + [1] and got[2][-1] == missed >> g
