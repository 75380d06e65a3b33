"""The sparse bao calls from packed chunk bytes (bao.outboard_update_packed, verify_ranges_packed, range_slices_packed;
b3w_bao_*_packed_device): files that are NOT resident.  The oracle is always the arena call of the same build over a resident copy of
the same file bytes, with the same outboards, roots, ranges and group_log: every output byte must be the arena call's and every byte it
leaves alone must stay (outboards and unit statuses sit between 0xA5 guards, statuses over a 0xEE prefill).  The packed buffer is made
by bao.pack_ranges and holds the listed chunks alone.  The world is the update test's files and four more lengths (1 025 B, 64 KiB + 1,
1 MiB + 1: a lone last tile, 3 MiB + 5), every file at an odd byte of the arena; the range sets are the update test's scenarios and
the kinds of tests/test_bao_packed_cpu.py, among them two ranges of one tile with a gap, which a kernel that addresses the packed
buffer by chunk index gets wrong."""
import functools

import numpy as np
import pytest

import b3w_testlib as T
from test_gpu_bao_batch import _arena
from test_gpu_bao_update import GUARD, K, LENS, _ragged, _scenarios, _whole

pytestmark = pytest.mark.gpu

GS = [0, 4, 6]
FILL = 0xEE
WLENS = LENS + [1025, 64 * K + 1, (1 << 20) + 1, 3 * (1 << 20) + 5]
B2, S65, M1, M3 = range(len(LENS), len(LENS) + 4)                          # 2 chunks; 65 (the last of 1 byte); 1 025 (a lone last tile); 3 073


def _n(f):
    return max(1, -(-WLENS[f] // K))


def _sets():
    """name -> ranges (file, first chunk, chunks): the update test's scenarios on its own files, and the kinds of the CPU test"""
    F, F2 = _ragged(2051), _whole(2051)
    sc = dict(_scenarios())
    sc.update({
        "two ranges of one tile with a gap": [(F, 3, 2), (F, 300, 5), (F, 1024 + 7, 1), (F, 1024 + 900, 3), (M3, 2048 + 1, 1), (M3, 2048 + 1000, 20), (S65, 1, 1),
                                              (S65, 40, 2)],
        "one chunk": [(M3, 1500, 1)],
        "across a unit boundary, unaligned at both ends": [(M3, 63, 3), (F2, 127, 66), (S65, 63, 2)],
        "across a tile boundary": [(M3, 1022, 4), (M3, 2040, 70), (M1, 1020, 5)],
        "short last chunks": [(M3, 3072, 1), (M1, 1024, 1), (S65, 64, 1), (B2, 1, 1), (1, 0, 1), (F, 2050, 1)],
        "whole files and empty ranges": [(M3, 0, 3073), (M1, 1025, 0), (0, 0, 1), (B2, 0, 2), (F, 7, 0), (S65, 0, 65)],
        "repeated, overlapping and unsorted": [(M3, 3000, 73), (M1, 5, 1), (M3, 10, 100), (B2, 1, 1), (M3, 3050, 5), (M3, 60, 10), (M1, 5, 1), (B2, 0, 1), (M3, 2047, 2)],
        "a small file between two large ones": [(_whole(1024), 1000, 3), (_ragged(1025), 0, 1), (_ragged(1025), 1024, 1), (_ragged(3), 1, 1), (_whole(3), 2, 1),
                                                (_ragged(64), 0, 1), (_whole(64), 63, 1), (_ragged(65), 64, 1), (_whole(65), 0, 2)],
    })
    return sc


@functools.lru_cache(maxsize=None)
def _setup():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    arena, offsets = _arena(WLENS, starts_odd=set(range(len(WLENS))), seed=27)
    return dict(m=m, ctx=ctx, arena=arena, offsets=offsets, lens=np.array(WLENS, dtype=np.uint64), d_arena=torch.from_numpy(arena).cuda())


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """every device tensor of this module comes from a pool of the allocator that is the module's own and goes with it"""
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


def _cols(ranges):
    return [r[0] for r in ranges], [r[1] for r in ranges], [r[2] for r in ranges]


def _covered(ranges):
    out = {}
    for f, a, c in ranges:
        out.setdefault(f, set()).update(range(a, min(_n(f), a + c)))
    return {f: sorted(v) for f, v in out.items() if v}


def _write(s, d_arena, cov, salt=0):
    """a byte flipped in every covered chunk, on the device, in place"""
    import torch
    pos = [int(s["offsets"][f]) + c * K + (c * 7 + salt) % min(K, WLENS[f] - c * K) for f, chunks in cov.items() for c in chunks if WLENS[f] - c * K > 0]
    if pos:
        idx = torch.tensor(sorted(set(pos)), dtype=torch.int64, device="cuda")
        d_arena[idx] = d_arena[idx] ^ 1


def _guarded(d_src, fill=None):
    """a copy of d_src (or as many bytes of `fill`) between 0xA5 guards -> (the whole buffer, the view between the guards)"""
    import torch
    buf = torch.full((d_src.numel() + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + d_src.numel()] = d_src if fill is None else fill
    return buf, buf[GUARD:GUARD + d_src.numel()]


def _pack(s, d_arena, ranges, g):
    return s["m"].bao.pack_ranges(d_arena, s["offsets"], s["lens"], *_cols(ranges), g).view(-1)


def _update_both(s, d_now, old, ranges, g, d_packed=None):
    """the arena call and the packed call from the same outboards and roots -> ((buffer, roots) of the arena call, of the packed call)"""
    m, ctx = s["m"], s["ctx"]
    d_packed = _pack(s, d_now, ranges, g) if d_packed is None else d_packed
    a_buf, a_obs = _guarded(old["outboards"])
    p_buf, p_obs = _guarded(old["outboards"])
    a_roots, p_roots = old["roots"].clone(), old["roots"].clone()
    m.bao.outboard_update_batch(ctx, d_now, s["offsets"], s["lens"], a_obs, a_roots, *_cols(ranges), group_log=g)
    m.bao.outboard_update_packed(ctx, d_packed, s["lens"], p_obs, p_roots, *_cols(ranges), group_log=g, ob_first=old["ob_first"] if len(ranges) % 2 else None)
    return (a_buf, a_roots), (p_buf, p_roots)


def _verify_both(s, d_arena, d_obs, d_roots, ranges, g, uf, d_packed=None):
    """-> the (guarded unit bytes, range statuses, first bad units) of the arena call and of the packed call, over the same prefill"""
    import torch
    m, ctx = s["m"], s["ctx"]
    d_packed = _pack(s, d_arena, ranges, g) if d_packed is None else d_packed
    got = []
    for packed in (False, True):
        buf, st = _guarded(torch.empty(int(uf[-1]), dtype=torch.uint8, device="cuda"), fill=FILL)
        if packed:
            out = m.bao.verify_ranges_packed(ctx, d_packed, s["lens"], d_obs, d_roots, *_cols(ranges), group_log=g, unit_status=st)
        else:
            out = m.bao.verify_ranges_batch(ctx, d_arena, s["offsets"], s["lens"], d_obs, d_roots, *_cols(ranges), group_log=g, unit_status=st)
        got.append((buf, out["range_status"], out["range_first_bad"]))
    return got


def _same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("g", GS)
def test_update_from_packed_bytes_writes_what_the_arena_call_writes(g):
    import torch
    s = _setup()
    old = _made(g)
    for name, ranges in _sets().items():
        cov = _covered(ranges)
        d_now = s["d_arena"].clone()
        _write(s, d_now, cov)
        want, got = _update_both(s, d_now, old, ranges, g)
        torch.cuda.synchronize()
        assert _same(want, got), (g, name, int((want[0] != got[0]).nonzero()[:1].sum().item()) - GUARD)
        assert bool((want[0][:GUARD] == 0xA5).all().item()) and bool((want[0][-GUARD:] == 0xA5).all().item())
        changed = [f for f in cov if WLENS[f]]
        assert all(not torch.equal(got[1][f], old["roots"][f]) for f in changed), (g, name)   # (the call did something)
    # the packed buffer holds the listed chunks alone: a run of one tile with a gap is a handful of slots
    lay = s["m"].bao.packed_layout(s["lens"], *_cols(_sets()["two ranges of one tile with a gap"]), g)
    assert lay["total_slots"] <= 11 * (1 << g) + 35


def _tampered(s, made, what, at):
    d_arena, d_obs, d_roots = s["d_arena"].clone(), made["outboards"].clone(), made["roots"].clone().view(-1)
    {"arena": d_arena, "obs": d_obs, "roots": d_roots}[what][at] ^= 0x20
    return d_arena, d_obs, d_roots


@pytest.mark.parametrize("g", GS)
def test_ranged_verify_from_packed_bytes_reports_what_the_arena_call_reports(g):
    import torch
    s = _setup()
    made = _made(g)
    uf, ob_first = made["unit_first"], [int(x) for x in made["ob_first"]]
    for name, ranges in _sets().items():                                       # clean arenas: every range set
        want, got = _verify_both(s, s["d_arena"], made["outboards"], made["roots"], ranges, g, uf)
        torch.cuda.synchronize()
        assert _same(want, got), (g, name)
        assert not got[1].any().item() and bool((got[2] == -1).all().item()), (g, name)
        listed = got[0][GUARD:-GUARD] != FILL
        assert bool((got[0][GUARD:-GUARD][listed] == 0).all().item()) and bool(listed.any().item()) == any(r[2] for r in ranges), (g, name)
    F = _ragged(2051)
    gap = _sets()["two ranges of one tile with a gap"]
    short = _sets()["short last chunks"] + [(_ragged(3), 1, 1)]
    at_f, at_m3 = int(s["offsets"][F]), int(s["offsets"][M3])
    cases = [                                                                  # one tamper each: name, ranges, what is flipped, the statuses that must show
        ("a listed chunk's byte behind the gap", gap, ("arena", at_f + 302 * K + 9), {1}),
        ("a listed chunk's byte in another tile", gap, ("arena", at_m3 + (2048 + 1010) * K + 1), {1}),
        ("an unlisted chunk's byte inside the gap", gap, ("arena", at_f + 700 * K + 9), set()),
        ("a short last chunk's last byte", short, ("arena", at_m3 + 3072 * K + 4), {1}),
        ("a small file's byte", short, ("arena", int(s["offsets"][B2]) + 1024), {1}),
        ("a node on a listed path", gap, ("obs", ob_first[F] + 8 + 64 * 1 + 33), {2}),
        ("the root node", short, ("obs", ob_first[M3] + 8 + 5), {2}),
        ("a header", gap, ("obs", ob_first[F] + 1), {3}),
        ("a small file's header", short, ("obs", ob_first[B2] + 7), {3}),
        ("a root", gap, ("roots", M3 * 8 + 2), {2}),
        ("a small file's root", short, ("roots", _ragged(3) * 8), {2} if g < 2 else {1}),
    ]
    for name, ranges, (what, at), shows in cases:
        d_arena, d_obs, d_roots = _tampered(s, made, what, at)
        want, got = _verify_both(s, d_arena, d_obs, d_roots, ranges, g, uf)
        torch.cuda.synchronize()
        assert _same(want, got), (g, name)
        assert set(got[1].cpu().tolist()) - {0} == shows, (g, name, got[1].cpu().tolist())


def _sliceable(ranges):
    return [r for r in ranges if r[2]]                                         # (the range-slice calls refuse a range of no chunks)


@pytest.mark.parametrize("g", GS)
def test_range_slices_from_packed_bytes_are_the_arena_calls_and_ingest_back_to_the_source(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    made = _made(g)
    for name, ranges in _sets().items():
        ranges = _sliceable(ranges)
        if not ranges:
            continue
        want = m.bao.range_slices_arena(ctx, s["d_arena"], s["offsets"], s["lens"], made["outboards"], *_cols(ranges), group_log=g)
        got = m.bao.range_slices_packed(ctx, _pack(s, s["d_arena"], ranges, g), s["lens"], made["outboards"], *_cols(ranges), group_log=g)
        torch.cuda.synchronize()
        assert (want["slice_first"] == got["slice_first"]).all() and torch.equal(want["slices"], got["slices"]), \
            (g, name, int((want["slices"] != got["slices"]).nonzero()[:1].sum().item()))
        # the loop closed: a receiver with nothing takes the slices in and holds the source's chunks and nothing else
        r_arena, r_obs = torch.zeros_like(s["d_arena"]), torch.zeros_like(made["outboards"])
        out = m.bao.ingest_range_slices(ctx, r_arena, s["offsets"], s["lens"], r_obs, made["roots"], *_cols(ranges), got["slices"], group_log=g)
        torch.cuda.synchronize()
        assert not out["range_status"].any().item(), (g, name)
        mask = np.zeros(s["arena"].size, dtype=bool)
        for f, chunks in _covered(ranges).items():
            for c in chunks:
                mask[int(s["offsets"][f]) + c * K:int(s["offsets"][f]) + min(WLENS[f], (c + 1) * K)] = True
        d_mask = torch.from_numpy(mask).cuda()
        assert torch.equal(r_arena[d_mask], s["d_arena"][d_mask]) and not r_arena[~d_mask].any().item(), (g, name)


def _padding(s, ranges, g):
    """(total_slots, total_bytes, bool per byte of the slots: it lies behind a short last chunk)"""
    lay = s["m"].bao.packed_layout(s["lens"], *_cols(ranges), g)
    pad = np.zeros(lay["total_slots"] * K, dtype=bool)
    for (f, _, _), slot, lo, cnt in zip(ranges, lay["range_slot"], lay["range_first"], lay["range_chunks"]):
        if cnt and int(lo + cnt) == _n(f):                                     # (the file's last chunk: maybe short; of a file of no bytes, empty)
            last = int(slot + cnt - 1) * K
            pad[last + WLENS[f] - (_n(f) - 1) * K:last + K] = True
    return lay["total_slots"], lay["total_bytes"], pad


@pytest.mark.parametrize("g", GS)
def test_nothing_behind_a_short_last_chunk_or_behind_total_bytes_is_read(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    made = _made(g)
    uf = made["unit_first"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(27 + g)
    sets = _sets()
    for name in ("short last chunks", "whole files and empty ranges", "two ranges of one tile with a gap", "the ragged last chunk"):
        ranges = sets[name]
        slots, total, pad = _padding(s, ranges, g)
        assert pad.any() or name == "two ranges of one tile with a gap"
        d_pad = torch.from_numpy(pad).cuda()
        d_now = s["d_arena"].clone()
        _write(s, d_now, _covered(ranges))
        clean = _pack(s, d_now, ranges, g)
        runs = []
        for k in range(3):
            # 0, 1: other random bytes behind every short last chunk and behind total_bytes; 2: at an odd address, packed_bytes == total_bytes
            room = torch.randint(0, 256, (slots * K + 4096 + 1,), dtype=torch.uint8, device="cuda", generator=gen)
            buf = room[1:] if k == 2 else room[:-1]
            buf[:slots * K] = torch.where(d_pad, buf[:slots * K], clean)
            d_packed = buf[:total] if k == 2 else buf
            assert d_packed.data_ptr() % 2 == (1 if k == 2 else 0) and d_packed.is_contiguous()
            upd = _update_both(s, d_now, made, ranges, g, d_packed=d_packed)
            ver = _verify_both(s, d_now, made["outboards"], made["roots"], ranges, g, uf, d_packed=d_packed)
            sl = m.bao.range_slices_packed(ctx, d_packed, s["lens"], made["outboards"], *_cols(_sliceable(ranges)), group_log=g)["slices"]
            torch.cuda.synchronize()
            assert _same(upd[0], upd[1]) and _same(ver[0], ver[1]), (g, name, k)   # (the arena calls' bytes, so the same in every run)
            runs.append(sl)
        want = m.bao.range_slices_arena(ctx, d_now, s["offsets"], s["lens"], made["outboards"], *_cols(_sliceable(ranges)), group_log=g)["slices"]
        assert all(torch.equal(want, sl) for sl in runs), (g, name)


@pytest.mark.parametrize("g", [0, 4])
def test_a_file_of_1026_tiles_from_a_packed_buffer_of_its_listed_chunks_alone(g):
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
    # the first tile (two ranges with a gap), the 1 024th, across the 1 GiB split, the last tile (one chunk of 5 bytes), and two other files
    ranges = [(1, n - 1, 1), (1, 5, 2), (1, 900, 1), (1, 1023 * 1024 + 7, 1), (1, 1024 * 1024 - 3, 6), (3, 69, 1), (0, 2, 1)]
    cols = _cols(ranges)
    lay = m.bao.packed_layout(lens, *cols, g)
    assert lay["total_slots"] < 200 and lay["total_bytes"] < (1 << 20)         # a handful of chunks of a file of 1 GiB
    # verify and slices on the clean arena; then writes, and the update
    d_packed = m.bao.pack_ranges(d_arena, offsets, lens, *cols, g).view(-1)
    assert d_packed.numel() == lay["total_slots"] * K
    for flip in (None, int(made["ob_first"][1]) + 8 + 64 * 1 + 17):            # clean; the node over the first span of 1 024 tiles
        d_obs = made["outboards"].clone()
        if flip is not None:
            d_obs[flip] ^= 1
        outs = []
        for packed in (False, True):
            st = torch.full((int(uf[-1]),), FILL, dtype=torch.uint8, device="cuda")
            if packed:
                out = m.bao.verify_ranges_packed(ctx, d_packed, lens, d_obs, made["roots"], *cols, group_log=g, unit_status=st)
            else:
                out = m.bao.verify_ranges_batch(ctx, d_arena, offsets, lens, d_obs, made["roots"], *cols, group_log=g, unit_status=st)
            outs.append((st, out["range_status"], out["range_first_bad"]))
        torch.cuda.synchronize()
        assert _same(*outs), (g, flip)
        assert outs[1][1].cpu().tolist() == ([0] * 7 if flip is None else [0, 2, 2, 2, 2, 0, 0]), (g, flip)
    want = m.bao.range_slices_arena(ctx, d_arena, offsets, lens, made["outboards"], *cols, group_log=g)["slices"]
    got = m.bao.range_slices_packed(ctx, d_packed, lens, made["outboards"], *cols, group_log=g)["slices"]
    assert torch.equal(want, got), g
    for f, a, c in ranges:
        d_arena[int(offsets[f]) + a * K + 3] ^= 1
    d_packed = m.bao.pack_ranges(d_arena, offsets, lens, *cols, g).view(-1)
    a_obs, a_roots, p_obs, p_roots = made["outboards"].clone(), made["roots"].clone(), made["outboards"].clone(), made["roots"].clone()
    m.bao.outboard_update_batch(ctx, d_arena, offsets, lens, a_obs, a_roots, *cols, group_log=g)
    m.bao.outboard_update_packed(ctx, d_packed, lens, p_obs, p_roots, *cols, group_log=g)
    torch.cuda.synchronize()
    assert torch.equal(a_obs, p_obs) and torch.equal(a_roots, p_roots), g
    assert not torch.equal(p_roots[1], made["roots"][1]) and torch.equal(p_roots[2], made["roots"][2])


def _c_args(s, made, ranges, g):
    """what the three C calls take, made once: the range arrays, the layouts, the scratches and the outputs"""
    import torch
    L = s["m"].lib()
    fi, fc, nc = (np.array(col, dtype=t) for col, t in zip(_cols(ranges), (np.uint32, np.uint64, np.uint64)))
    lens = s["lens"]
    a = dict(fi=fi, fc=fc, nc=nc, obf=np.ascontiguousarray(made["ob_first"], dtype=np.uint64), uf=np.ascontiguousarray(made["unit_first"], dtype=np.uint64))
    a["upd_need"] = L.b3w_bao_update_scratch_bytes(lens.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)
    a["ver_need"] = L.b3w_bao_verify_ranges_scratch_bytes(lens.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)
    a["upd_scratch"] = torch.full((a["upd_need"] + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    a["ver_scratch"] = torch.full((a["ver_need"] + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    a["obs_buf"], a["obs"] = _guarded(made["outboards"])
    a["roots"] = made["roots"].clone()
    a["st_buf"], a["st"] = _guarded(torch.empty(int(made["unit_first"][-1]), dtype=torch.uint8, device="cuda"), fill=FILL)
    a["rs"] = torch.full((fi.size,), -7, dtype=torch.int32, device="cuda")
    a["rf"] = torch.full((fi.size,), -7, dtype=torch.int64, device="cuda")
    sf = s["m"].bao.range_slice_layout(lens, fi, fc, nc)
    a["slices"] = torch.full((int(sf[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
    return a


def _c_calls(s, ctx, a, g, d_packed_ptr, packed_bytes, which=(0, 1, 2), **kw):
    """those of the three C calls that `which` names, each argument replaceable by name -> their return codes"""
    import torch
    L = s["m"].lib()
    lens = s["lens"]
    v = dict(packed=d_packed_ptr, packed_bytes=packed_bytes, ln=lens.ctypes.data, n_files=lens.size, gl=g, ob_first=a["obf"].ctypes.data, obs=a["obs"].data_ptr(),
             roots=a["roots"].data_ptr(), files=a["fi"].ctypes.data, first=a["fc"].ctypes.data, count=a["nc"].ctypes.data, n=a["fi"].size,
             unit_first=a["uf"].ctypes.data, st=a["st"].data_ptr(), rs=a["rs"].data_ptr(), rf=a["rf"].data_ptr(), slices=a["slices"].data_ptr(),
             upd_scratch=a["upd_scratch"].data_ptr(), upd_bytes=a["upd_need"], ver_scratch=a["ver_scratch"].data_ptr(), ver_bytes=a["ver_need"])
    v.update(kw)
    stream = torch.cuda.current_stream().cuda_stream
    calls = (lambda: L.b3w_bao_outboard_update_packed_device(ctx.handle, v["packed"], v["packed_bytes"], v["ln"], v["n_files"], v["gl"], v["ob_first"], v["obs"], v["roots"],
                                                    v["files"], v["first"], v["count"], v["n"], v["upd_scratch"], v["upd_bytes"], stream),
             lambda: L.b3w_bao_verify_ranges_packed_device(ctx.handle, v["packed"], v["packed_bytes"], v["ln"], v["n_files"], v["gl"], v["ob_first"], v["obs"], v["roots"],
                                                  v["files"], v["first"], v["count"], v["n"], v["unit_first"], v["st"], v["rs"], v["rf"], v["ver_scratch"],
                                                  v["ver_bytes"], stream),
             lambda: L.b3w_bao_range_slice_packed_device(ctx.handle, v["packed"], v["packed_bytes"], v["ln"], v["n_files"], v["gl"], v["obs"], v["files"], v["first"],
                                                v["count"], v["n"], v["slices"], stream))
    return tuple(calls[k]() for k in which)


GOOD = [(_ragged(2051), 5, 1), (_ragged(2051), 1500, 2), (_whole(1025), 1020, 5), (_ragged(3), 1, 1), (M3, 3072, 1), (0, 0, 1)]


def test_the_three_c_calls_allocate_no_device_memory():
    import torch
    s = _setup()
    g = 4
    made = _made(g)
    a = _c_args(s, made, GOOD, g)
    d_packed = _pack(s, s["d_arena"], GOOD, g)
    assert a["upd_need"] == 32 * 5 and a["ver_need"] == (36 * 5 + 15) // 16 * 16   # two tiles each of two files, one of a third; one-tile files: none
    assert _c_calls(s, s["ctx"], a, g, d_packed.data_ptr(), d_packed.numel()) == (0, 0, 0)   # (warm: the context's staging is its own)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    free0 = torch.cuda.mem_get_info()[0]
    assert _c_calls(s, s["ctx"], a, g, d_packed.data_ptr(), d_packed.numel()) == (0, 0, 0)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == start and torch.cuda.mem_get_info()[0] >= free0   # (neither the allocator's memory nor the device's)
    assert torch.equal(a["obs"], made["outboards"]) and torch.equal(a["roots"], made["roots"])   # (the files are as they were: the same bytes again)
    assert not a["rs"].any().item() and bool((a["rf"] == -1).all().item())


def test_refusals_are_atomic_and_name_the_range():
    import torch
    s = _setup()
    m = s["m"]
    ctx = m.Context("compression", 0)                                         # (any context)
    g = 1
    made = _made(g)
    a = _c_args(s, made, GOOD, g)
    d_packed = _pack(s, s["d_arena"], GOOD, g)
    lay = m.bao.packed_layout(s["lens"], *_cols(GOOD), g)
    total = lay["total_bytes"]
    assert total == d_packed.numel() - K + 5 and lay["total_slots"] * K == d_packed.numel()    # (the last slot holds a chunk of 5 bytes)
    bad, F = m.B3W_E_BAD_ARGUMENT, _ragged(2051)
    calls = ("bao update packed", "bao verify ranges packed", "bao range slice packed")

    def refused(which, word, **kw):
        src = (kw.pop("packed", d_packed.data_ptr()), kw.pop("packed_bytes", d_packed.numel()))
        for k in which:
            assert _c_calls(s, ctx, a, g, *src, which=(k,), **kw) == (bad,), (calls[k], kw)
            assert calls[k] in ctx.last_error() and word in ctx.last_error(), (calls[k], kw, ctx.last_error())
    every, sparse = (0, 1, 2), (0, 1)
    for kw, which, word in ((dict(ln=None), every, "null"), (dict(obs=None), every, "null"), (dict(files=None), every, "null"), (dict(first=None), every, "null"),
                            (dict(count=None), every, "null"), (dict(ob_first=None), sparse, "null"), (dict(roots=None), sparse, "null"),
                            (dict(unit_first=None), (1,), "null"), (dict(st=None), (1,), "null"), (dict(rs=None), (1,), "null"), (dict(rf=None), (1,), "null"),
                            (dict(slices=None), (2,), "null"), (dict(gl=7), every, "group_log"), (dict(obs=a["obs"].data_ptr() + 4), every, "8-byte"),
                            (dict(slices=a["slices"].data_ptr() + 8), (2,), "16-byte"), (dict(rf=a["rf"].data_ptr() + 4), (1,), "8-byte aligned"),
                            (dict(upd_bytes=a["upd_need"] - 1, ver_bytes=a["ver_need"] - 1), sparse, "scratch"), (dict(upd_scratch=None, ver_scratch=None), sparse, "scratch"),
                            (dict(upd_scratch=a["upd_scratch"].data_ptr() + 8, ver_scratch=a["ver_scratch"].data_ptr() + 8), sparse, "scratch"),
                            (dict(n_files=F), sparse, "range 0 (file %d, chunks 5 + 1): the file index" % F), (dict(n_files=F), (2,), "range 0: its file index"),
                            # the packed calls' own two: one byte short (the text gives the number needed), and no buffer at all
                            (dict(packed_bytes=total - 1), every, "packed_bytes is %d, the listed chunks take %d" % (total - 1, total)),
                            (dict(packed_bytes=0), every, "the listed chunks take %d" % total),
                            (dict(packed=None), every, "a null d_packed with %d bytes" % total)):
        refused(which, word, **kw)
    # a bad range behind good ones: nothing of the good ones is done
    for f, first, count, word, slice_word in ((len(WLENS), 0, 1, "file index", "file index"), (F, 2051, 1, "reaches past the file's 2051 chunks", "reaches past"),
                                              (F, 2000, 52, "reaches past", "reaches past"), (0, 1, 1, "reaches past the file's 1 chunks", "reaches past"),
                                              (F, 1 << 63, 1 << 63, "reaches past", "reaches past")):
        fi2, fc2, nc2 = np.append(a["fi"], np.uint32(f)), np.append(a["fc"], np.uint64(first)), np.append(a["nc"], np.uint64(count))
        kw = dict(files=fi2.ctypes.data, first=fc2.ctypes.data, count=nc2.ctypes.data, n=fi2.size, upd_bytes=a["upd_need"] + 16, ver_bytes=a["ver_need"] + 16)
        refused(sparse, "range 6 (file %d, chunks %d + %d)" % (f, first, count), **kw)
        refused(sparse, word, **kw)
        refused((2,), "range 6: ", **kw)
        refused((2,), slice_word, **kw)
    L = m.lib()
    assert L.b3w_bao_outboard_update_packed_device(None, None, 0, None, 0, 0, None, None, None, None, None, None, 0, None, 0, None) == bad
    assert L.b3w_bao_verify_ranges_packed_device(None, None, 0, None, 0, 0, None, None, None, None, None, None, 0, None, None, None, None, None, 0, None) == bad
    assert L.b3w_bao_range_slice_packed_device(None, None, 0, None, 0, 0, None, None, None, None, 0, None, None) == bad
    # the Python calls refuse a short buffer before the library does
    for call in (lambda: m.bao.outboard_update_packed(ctx, d_packed[:total - 1], s["lens"], a["obs"], a["roots"], *_cols(GOOD), group_log=g),
                 lambda: m.bao.verify_ranges_packed(ctx, d_packed[:total - 1], s["lens"], a["obs"], a["roots"], *_cols(GOOD), group_log=g, unit_status=a["st"]),
                 lambda: m.bao.range_slices_packed(ctx, d_packed[:total - 1], s["lens"], a["obs"], *_cols(GOOD), group_log=g)):
        with pytest.raises(m.B3WError, match="the listed chunks take %d" % total):
            call()
    torch.cuda.synchronize()

    def untouched():
        return torch.equal(a["obs_buf"][GUARD:-GUARD], made["outboards"]) and bool((a["obs_buf"][:GUARD] == 0xA5).all().item()) and \
            bool((a["obs_buf"][-GUARD:] == 0xA5).all().item()) and torch.equal(a["roots"], made["roots"]) and bool((a["st"] == FILL).all().item()) and \
            bool((a["st_buf"][:GUARD] == 0xA5).all().item()) and bool((a["st_buf"][-GUARD:] == 0xA5).all().item()) and bool((a["rs"] == -7).all().item()) and \
            bool((a["rf"] == -7).all().item()) and bool((a["slices"] == 0x5A).all().item()) and bool((a["upd_scratch"] == 0x5A).all().item()) and \
            bool((a["ver_scratch"] == 0x5A).all().item())
    assert untouched()
    # no range: B3W_OK and nothing launched, whatever else is null; then the good ranges, with packed_bytes == total_bytes exactly
    assert _c_calls(s, ctx, a, g, None, 0, n=0, files=None, first=None, count=None, ln=None, upd_scratch=None, upd_bytes=0, ver_scratch=None, ver_bytes=0) == (0, 0, 0)
    torch.cuda.synchronize()
    assert untouched()
    assert _c_calls(s, ctx, a, g, d_packed.data_ptr(), total) == (0, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(a["obs"], made["outboards"]) and torch.equal(a["roots"], made["roots"])   # (the untouched files: the same bytes again)
    assert not a["rs"].any().item() and bool((a["rf"] == -1).all().item()) and not bool((a["slices"] == 0x5A).all().item())
    assert not bool((a["upd_scratch"][:a["upd_need"]] == 0x5A).all().item()) and bool((a["upd_scratch"][a["upd_need"]:] == 0x5A).all().item())
    ctx.close()
