"""Set slices served from packed chunk bytes (bao.set_slices_packed; b3w_bao_set_slice_packed_device): the multi-range request of a
half-arrived file answered by a provider whose file is not resident.  THE ORACLE is the arena provider of the same build over a resident
copy (b3w_bao_set_slice_arena_device), byte for byte over a 0x5C prefill between 0xA5 guards: padding and guards stay untouched.  The
world is test_gpu_bao_set_plan's files plus one of 5 MiB + 300 bytes, at group_log 0, 4 and 6; the packed buffer holds the listed chunks
alone (bao.pack_ranges), with other random bytes behind every short last chunk and behind total_bytes, or at an odd address with
packed_bytes == total_bytes."""
import functools

import numpy as np
import pytest

import b3w_testlib as T
from test_gpu_bao_ingest import BAD, GUARD, K, _walls_intact
from test_gpu_bao_set_plan import FILES as PLAN_FILES, MIB, _arrays, shapes

pytestmark = pytest.mark.gpu

GS = [0, 4, 6]
PAD = 0x5C
FILES = PLAN_FILES + [(5 * MIB + 300, 4)]
F1025, BIG, F5 = 8, 9, 10


@functools.lru_cache(maxsize=None)
def _world():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    offsets, at = [], 0
    for ln, phase in FILES:
        at = (at + 15) // 16 * 16 + phase
        offsets.append(at)
        at += ln
    lens = [ln for ln, _ in FILES]
    arena = np.random.default_rng(30).integers(0, 256, at + 64, dtype=np.uint8)
    in_file = np.zeros(arena.size, dtype=bool)
    for o, ln in zip(offsets, lens):
        in_file[o:o + ln] = True
    d_src = torch.from_numpy(arena).cuda()
    offsets = np.array(offsets, dtype=np.uint64)
    made = {g: m.bao.outboard_batch(ctx, d_src, offsets, lens) if g == 0 else m.bao.outboard_groups_batch(ctx, d_src, offsets, lens, g) for g in GS}
    torch.cuda.synchronize()
    return dict(m=m, ctx=ctx, arena=arena, in_file=in_file, d_src=d_src, offsets=offsets, lens=lens, ln=np.array(lens, dtype=np.uint64),
                n=[m.bao.num_chunks(x) for x in lens], made=made, roots=made[0]["roots"])


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """the module's device tensors come from a pool of its own and go with it"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        if _world.cache_info().currsize:
            _world()["ctx"].close()
        _world.cache_clear()
        gc.collect()
    del pool


def _calls(w):
    """-> [(name, [(file, runs)])]: every shape of the planner's test on every file it fits, a call a shape; then the cases of this call's own"""
    per = [shapes(n) for n in w["n"]]
    calls = [(name, [(f, sh[name]) for f, sh in enumerate(per) if name in sh]) for name in sorted({name for sh in per for name in sh})]
    n5 = w["n"][F5]
    calls.append(("two runs of one tile with unlisted chunks between them", [(F1025, ((3, 2), (700, 3)))]))
    calls.append(("groups touched only partly", [(5, ((5, 1), (37, 2))), (F1025, ((17, 1), (100, 3), (1023, 2))), (BIG, ((5, 1), (70, 3), (1030, 1), (3072, 1)))]))
    calls.append(("the first and the last tile only", [(2, ((0, 1),)), (F5, ((3, 2), (1000, 24), (n5 - 70, 3), (n5 - 1, 1)))]))
    return calls


def _c_arena(w, g, sets, d_slices):
    import torch
    files, first, count = _arrays(sets)
    return w["m"].lib().b3w_bao_set_slice_arena_device(w["ctx"].handle, w["d_src"].data_ptr(), w["d_src"].numel(), w["offsets"].ctypes.data, w["ln"].ctypes.data,
                                                       len(w["lens"]), g, w["made"][g]["outboards"].data_ptr(), files.ctypes.data, first.ctypes.data,
                                                       count.ctypes.data, files.size, d_slices.data_ptr(), torch.cuda.current_stream().cuda_stream)


def _c_packed(w, g0, sets, slices0, packed0, **change):
    import torch
    files, first, count = _arrays(sets)
    kw = dict(ctx=w["ctx"].handle, d_packed=packed0.data_ptr() if packed0.numel() else None, packed_bytes=packed0.numel(), lens=w["ln"].ctypes.data,
              n_files=len(w["lens"]), g=g0, d_obs=w["made"][g0]["outboards"].data_ptr(), files=files.ctypes.data, first=first.ctypes.data,
              count=count.ctypes.data, n_ranges=files.size, d_slices=slices0.data_ptr())
    for name, value in change.items():
        kw[name] = value.ctypes.data if isinstance(value, np.ndarray) else value
    return w["m"].lib().b3w_bao_set_slice_packed_device(*kw.values(), torch.cuda.current_stream().cuda_stream)


def _prefilled(total):
    import torch
    whole = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    whole[GUARD:GUARD + total] = PAD
    return whole, whole[GUARD:GUARD + total]


def _short_tails(w, files, first, count, g):
    """(the packed layout, bool per byte of the slots: it lies behind a short last chunk)"""
    lay = w["m"].bao.packed_layout(w["lens"], files, first, count, g)
    pad = np.zeros(lay["total_slots"] * K, dtype=bool)
    for f, slot, lo, cnt in zip(files, lay["range_slot"], lay["range_first"], lay["range_chunks"]):
        if cnt and int(lo + cnt) == w["n"][f]:                                 # the file's last chunk: maybe short; of a file of no bytes, empty
            last = int(slot + cnt - 1) * K
            pad[last + w["lens"][f] - (w["n"][f] - 1) * K:last + K] = True
    return lay, pad


@pytest.mark.parametrize("g", GS)
def test_every_byte_is_the_arena_calls(g):
    import torch
    w = _world()
    m = w["m"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(300 + g)
    calls = _calls(w)
    assert any(w["n"][f] <= 64 for _, sets in calls for f, _ in sets) and any(w["lens"][f] % K for _, sets in calls for f, _ in sets)
    for name, sets in calls:
        files, first, count = _arrays(sets)
        total = int(m.bao.set_slice_layout(w["ln"], files, first, count)["slice_first"][-1])
        whole_a, want = _prefilled(total)
        assert _c_arena(w, g, sets, want) == 0, w["ctx"].last_error()
        lay, pad = _short_tails(w, files, first, count, g)
        slots, nbytes = lay["total_slots"], lay["total_bytes"]
        if name.startswith("two runs"):                                        # the gap: the unlisted chunks have no slot (g 0), or only their groups' (above)
            assert slots == {0: 5, 4: 32, 6: 128}[g]
        clean = m.bao.pack_ranges(w["d_src"], w["offsets"], w["lens"], files, first, count, g).view(-1)
        d_pad = torch.from_numpy(pad).cuda()
        for k in range(2):
            # 0: other random bytes behind every short last chunk and behind total_bytes; 1: at an odd address, packed_bytes == total_bytes
            room = torch.randint(0, 256, (slots * K + 4096 + 1,), dtype=torch.uint8, device="cuda", generator=gen)
            buf = room[1:] if k == 1 else room[:-1]
            buf[:slots * K] = torch.where(d_pad, buf[:slots * K], clean)
            d_packed = buf[:nbytes] if k == 1 else buf
            assert d_packed.data_ptr() % 2 == k and d_packed.is_contiguous()
            whole_p, got = _prefilled(total)
            assert _c_packed(w, g, sets, got, d_packed) == 0, w["ctx"].last_error()
            torch.cuda.synchronize()
            assert torch.equal(got, want), (g, name, k, int((got != want).nonzero()[:1].sum().item()))
            assert _walls_intact(whole_p, total) and _walls_intact(whole_a, total)
        # the Python call: the same dict, byte for byte
        a = m.bao.set_slices_arena(w["ctx"], w["d_src"], w["offsets"], w["lens"], w["made"][g]["outboards"], files, first, count, group_log=g)
        p = m.bao.set_slices_packed(w["ctx"], clean, w["lens"], w["made"][g]["outboards"], files, first, count, group_log=g)
        assert torch.equal(a["slices"], p["slices"]) and all(np.array_equal(a[key], p[key]) for key in a if key != "slices"), (g, name)


@pytest.mark.parametrize("g", [0, 4])
def test_the_loop_closes_from_packed_bytes(g):
    """have_runs -> pack_ranges -> set_slices_packed -> ingest_set_slices into an empty arena, in two rounds (what a random bitmap lacks,
    then the rest): the source's chunks, the provider's outboard and nothing else"""
    import torch
    w = _world()
    m, ctx = w["m"], w["ctx"]
    wf = m.bao.have_layout(w["lens"])
    rng = np.random.default_rng(310 + g)
    pretend = rng.integers(0, 1 << 64, int(wf[-1]), dtype=np.uint64).view(np.int64)
    for f, n in enumerate(w["n"]):                                            # (the pad bits stay clear)
        words = pretend[int(wf[f]):int(wf[f + 1])].view(np.uint64)
        if n % 64:
            words[-1] &= np.uint64((1 << (n % 64)) - 1)
    r_arena, r_obs = torch.zeros_like(w["d_src"]), torch.zeros_like(w["made"][g]["outboards"])
    d_have = m.bao.have_new(w["lens"])
    rounds = 0
    for d_ask in (torch.from_numpy(pretend).cuda(), d_have, d_have):
        runs = m.bao.have_runs(ctx, d_ask, w["lens"], kind="missing")
        files, first, count = runs["files"], runs["first_chunks"], runs["n_chunks"]
        if not len(files):
            break
        d_packed = m.bao.pack_ranges(w["d_src"], w["offsets"], w["lens"], files, first, count, g)
        assert g or d_packed.shape[0] < sum(w["n"])                           # never the whole world: the files are not resident
        sl = m.bao.set_slices_packed(ctx, d_packed, w["lens"], w["made"][g]["outboards"], files, first, count, group_log=g)
        out = m.bao.ingest_set_slices(ctx, r_arena, w["offsets"], w["lens"], r_obs, w["roots"], files, first, count, sl["slices"], group_log=g, d_have=d_have)
        assert not out["set_status"].any().item() and not out["chunk_status"].any().item()
        rounds += 1
    assert rounds == 2 and int(runs["n_runs"].item()) == 0 and runs["file_have"].cpu().tolist() == w["n"]
    got = r_arena.cpu().numpy()
    assert (got[w["in_file"]] == w["arena"][w["in_file"]]).all() and not got[~w["in_file"]].any()
    assert torch.equal(r_obs, w["made"][g]["outboards"])


def _some_sets(w):
    return [(1, ((0, 1),)), (6, ((0, 1), (2, 1), (63, 2))), (F1025, ((1, 2), (3, 1), (1000, 25))), (BIG, ((5, 1), (1020, 10), (3070, 3)))]


def test_the_call_allocates_nothing():
    import torch
    w = _world()
    m = w["m"]
    sets = _some_sets(w)
    files, first, count = _arrays(sets)
    d_packed = m.bao.pack_ranges(w["d_src"], w["offsets"], w["lens"], files, first, count, 4)
    total = int(m.bao.set_slice_layout(w["ln"], files, first, count)["slice_first"][-1])
    d_slices = torch.empty(total, dtype=torch.uint8, device="cuda")
    want = torch.empty(total, dtype=torch.uint8, device="cuda")
    for _ in range(2):                                                    # (the context's staging grows in the first round, outside the allocator)
        d_slices.fill_(PAD)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        assert _c_packed(w, 4, sets, d_slices, d_packed) == 0, w["ctx"].last_error()
        torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before
    want.fill_(PAD)
    assert _c_arena(w, 4, sets, want) == 0
    torch.cuda.synchronize()
    assert torch.equal(d_slices, want)


def test_refusals_leave_the_slices_untouched():
    import torch
    w = _world()
    m = w["m"]
    g = 0
    sets = _some_sets(w)
    files, first, count = _arrays(sets)
    lay = m.bao.packed_layout(w["lens"], files, first, count, g)
    d_packed = m.bao.pack_ranges(w["d_src"], w["offsets"], w["lens"], files, first, count, g).view(-1)
    total = int(m.bao.set_slice_layout(w["ln"], files, first, count)["slice_first"][-1])
    d_slices = torch.full((total,), PAD, dtype=torch.uint8, device="cuda")

    def refused(**change):
        rc = _c_packed(w, g, sets, d_slices, d_packed, **change)
        torch.cuda.synchronize()
        return rc == BAD and bool((d_slices == PAD).all().item())
    assert _c_packed(w, g, sets, d_slices, d_packed, ctx=None) == BAD and refused(g=7)
    for name in ("lens", "files", "first", "count", "d_obs", "d_slices"):
        assert refused(**{name: None}), name
    assert refused(d_obs=w["made"][g]["outboards"].data_ptr() + 4) and refused(d_slices=d_slices.data_ptr() + 8)
    last = files.size - 1
    j = next(i for i in range(2, files.size) if files[i] == files[i - 2])  # the third run of a set
    for what, at, value, named in (("files", last, len(w["lens"]), "file index"), ("count", 0, 0, "no chunk"), ("first", last, 1 << 40, "past"),
                                   ("count", last, 1 << 40, "past"), ("first", j, int(first[j - 1]), "disjoint"), ("first", j, int(first[j - 2]), "ascending"),
                                   ("files", last, 0, "ascending")):
        bad = {"files": files, "first": first, "count": count}[what].copy()
        bad[at] = value
        assert refused(**{what: bad}), (what, at, value)
        assert "range" in w["ctx"].last_error() and named in w["ctx"].last_error(), w["ctx"].last_error()
    long_lens = w["ln"].copy()
    long_lens[F1025] = ((1 << 30) + 1) * 1024                               # a file of 2^30 + 1 chunks
    assert refused(lens=long_lens) and "2^30" in w["ctx"].last_error()
    assert refused(d_packed=None) and str(lay["total_bytes"]) in w["ctx"].last_error()
    assert refused(packed_bytes=lay["total_bytes"] - 1) and str(lay["total_bytes"]) in w["ctx"].last_error()
    with pytest.raises(m.B3WError):
        m.bao.set_slices_packed(w["ctx"], d_packed, w["lens"], w["made"][0]["outboards"], files, first, count, group_log=7)
    with pytest.raises(m.B3WError):
        m.bao.set_slices_packed(w["ctx"], d_packed[:lay["total_bytes"] - 1], w["lens"], w["made"][0]["outboards"], files, first, count)
    with pytest.raises(m.B3WError):
        m.bao.set_slices_packed(w["ctx"], d_packed, w["lens"], w["made"][0]["outboards"], [0, 0], [1, 0], [1, 1])
    # no ranges: a no-op, whatever else is handed in
    assert m.lib().b3w_bao_set_slice_packed_device(w["ctx"].handle, None, 0, None, 0, 0, None, None, None, None, 0, None, None) == 0
    # and the same arguments unchanged are taken: exactly total_bytes are enough
    assert _c_packed(w, g, sets, d_slices, d_packed[:lay["total_bytes"]]) == 0, w["ctx"].last_error()
    want = torch.full((total,), PAD, dtype=torch.uint8, device="cuda")
    assert _c_arena(w, g, sets, want) == 0
    torch.cuda.synchronize()
    assert torch.equal(d_slices, want)
