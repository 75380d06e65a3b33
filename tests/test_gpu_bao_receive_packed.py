"""Slices taken into packed chunk slots (bao.ingest_slices_packed, ingest_range_slices_packed, ingest_set_slices_packed;
b3w_bao_slice_ingest_packed_device, b3w_bao_range_slice_ingest_packed_device, b3w_bao_set_slice_ingest_packed_device): the receivers for
files that are not resident.  The world is test_gpu_bao_set._world()'s (test_gpu_bao_ingest._setup()'s files and the two of several
tiles behind them).  EXPECTED VALUES COME FROM THE EXISTING CALLS: the arena receiver of the same kind is run on the same slices into an
arena of 0xEE, and the packed call must report its statuses, write its outboards and bitmap byte for byte, and leave in slot k the
arena's bytes of the k-th listed chunk where that chunk's status is 0 and 0xEE everywhere else; the host receivers (b3w_bao_*_ingest)
give a second opinion for one list of each kind.  Slices come from the existing providers; tampered ones from tests' own restatements."""
import functools

import numpy as np
import pytest

import b3w_testlib as T
import bao_range_ref as RR
import bao_set_ref as RS
from test_gpu_bao_ingest import BAD, FILL, GUARD, K, _setup, _walled, _walls_intact
from test_gpu_bao_set import _arrays, _expected, _host_ingest, _receiver, _receiver_sets, _tile_sets, _world, set_shapes, tampers

pytestmark = pytest.mark.gpu

GS = [0, 4, 6]
KINDS = ["one", "range", "set"]


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """as test_gpu_bao_set does it: the module's device tensors come from a pool of its own and go with it"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        _lists.cache_clear()
        _world.cache_clear()
        _expected.cache_clear()
        if _setup.cache_info().currsize:
            _setup()["ctx"].close()
        _setup.cache_clear()
        gc.collect()
    del pool


# ---- the lists --------------------------------------------------------------------------------------------------------------------------
def _flat(sets):
    return _arrays(sets)


@functools.lru_cache(maxsize=None)
def _lists():
    """-> {kind: {name: (files, first, count)}}: the clean lists of every kind (count is all ones for the one-chunk kind)"""
    w = _world()
    n = w["n"]
    f5, each, ends = _tile_sets(w)
    shapes = [set_shapes(k) for k in n]
    rng = np.random.default_rng(77)
    every = [(f, ((0, k),)) for f, k in enumerate(n)]
    last = [(f, ((k - 1, 1),)) for f, k in enumerate(n)]
    sets = {"every chunk of every file": every, "a set a file, sparse and dense": _receiver_sets(w), "one chunk in each tile": [(f5, each)],
            "first and last tile only": [(0, ((0, n[0]),)), (f5, ends)], "the short last chunk alone": last}
    for name in ("{0, 2}", "{63, 65}", "{1023, 1025}", "first and last chunk"):   # same block, adjacent blocks (rows of 64); apart (tiles)
        sets[name] = [(f, tuple(sh[name])) for f, sh in enumerate(shapes) if name in sh]
    big = [f for f, k in enumerate(n) if k > 1024]
    mid = [f for f, k in enumerate(n) if 64 < k <= 1025]
    assert big and mid
    over = []                                                              # ranges that overlap, repeat and come out of order
    for f in big + mid:
        k = n[f]
        a1 = min(60, k - 12)                                               # (across the 64-chunk boundary where the file reaches it)
        over += [(f, k - 3, 3), (f, a1, 10), (f, a1 + 5, 7), (f, 0, k), (f, a1, 10), (f, k // 2, min(k - k // 2, 70))]
    ranges = {name: _flat(s) for name, s in sets.items()}
    ranges["overlapping, repeated, out of order"] = (np.array([x[0] for x in over], dtype=np.uint32), np.array([x[1] for x in over], dtype=np.uint64),
                                                     np.array([x[2] for x in over], dtype=np.uint64))
    m = w["m"]
    ef, ec = m.bao.runs_chunks(*_flat(every))
    perm = rng.permutation(ef.size)
    pick = rng.integers(0, ef.size, 300)
    rep = np.concatenate([pick, pick[:40], pick[:7]])
    lf, lc = m.bao.runs_chunks(*_flat(last))
    ones = {"every chunk of every file": (ef[perm], ec[perm]), "repeated samples": (ef[rep], ec[rep]), "the short last chunk alone": (lf, lc)}
    ones = {name: (f, c, np.ones(f.size, dtype=np.uint64)) for name, (f, c) in ones.items()}
    return {"one": ones, "range": ranges, "set": {name: _flat(s) for name, s in sets.items()}}


def _names():
    return [(kind, name) for kind in KINDS for name in
            {"one": ["every chunk of every file", "repeated samples", "the short last chunk alone"],
             "range": ["every chunk of every file", "a set a file, sparse and dense", "one chunk in each tile", "first and last tile only",
                       "the short last chunk alone", "{63, 65}", "overlapping, repeated, out of order"],
             "set": ["every chunk of every file", "a set a file, sparse and dense", "one chunk in each tile", "first and last tile only",
                     "the short last chunk alone", "{0, 2}", "{63, 65}", "{1023, 1025}", "first and last chunk"]}[kind]]


# ---- the calls --------------------------------------------------------------------------------------------------------------------------
def _provide(w, kind, g, lst):
    """the existing provider of this kind over the source arena -> (the packed slices on the device, where each slice starts)"""
    m, (files, first, count) = w["m"], lst
    obs = w["made"][g]["outboards"]
    if kind == "one":
        out = m.bao.slices_arena(w["ctx"], w["d_src"], w["offsets"], w["lens"], obs, files, first, group_log=g)
    elif kind == "range":
        out = m.bao.range_slices_arena(w["ctx"], w["d_src"], w["offsets"], w["lens"], obs, files, first, count, group_log=g)
    else:
        out = m.bao.set_slices_arena(w["ctx"], w["d_src"], w["offsets"], w["lens"], obs, files, first, count, group_log=g)
    return out["slices"], out["slice_first"]


def _twin(w, kind, g, r, lst, d_slices, roots=None, have=True):
    """the arena receiver of this kind into r's arena, outboards and bitmap -> its dict"""
    m, (files, first, count) = w["m"], lst
    a = (w["ctx"], r["d_arena"], w["offsets"], w["lens"], r["d_obs"], w["roots"] if roots is None else roots, files, first)
    kw = dict(group_log=g, d_have=r["d_have"] if have else None)
    if kind == "one":
        return m.bao.ingest_slices(*a, d_slices, **kw)
    if kind == "range":
        return m.bao.ingest_range_slices(*a, count, d_slices, **kw)
    return m.bao.ingest_set_slices(*a, count, d_slices, **kw)


def _packed(w, kind, g, p, lst, d_slices, roots=None, have=True, obs=True, stream=0):
    """the packed receiver of this kind into p's slots, outboards and bitmap -> its dict"""
    m, (files, first, count) = w["m"], lst
    a = (w["ctx"], w["lens"], p["d_obs"] if obs else None, w["roots"] if roots is None else roots, files, first)
    kw = dict(group_log=g, d_have=p["d_have"] if have else None, d_chunks=p["d_chunks"], stream=stream)
    if kind == "one":
        return m.bao.ingest_slices_packed(*a, d_slices, **kw)
    if kind == "range":
        return m.bao.ingest_range_slices_packed(*a, count, d_slices, **kw)
    return m.bao.ingest_set_slices_packed(*a, count, d_slices, **kw)


def _slot_receiver(w, g, n_slots, seed=5):
    """test_gpu_bao_set's receiver (arena, outboards, bitmap) with a slot buffer of 0xEE between guards beside it"""
    r = _receiver(w, g, seed)
    r["whole_c"], r["d_chunks"] = _walled(K * n_slots)
    r["slot_bytes"] = K * n_slots
    return r


STATUS_KEYS = {"one": ["sample_status"], "range": ["range_status", "range_first_bad"], "set": ["set_status", "set_first_bad", "chunk_status"]}


def _expected_slots(w, arena, slots, status):
    """slot k: the arena's bytes of the k-th listed chunk where its status is 0, the fill everywhere else (on the device)"""
    import torch
    f, c, off, nb = slots
    base = torch.from_numpy(w["offsets"][f].astype(np.int64) + off.astype(np.int64)).cuda()
    take = torch.from_numpy(np.where(np.asarray(status) == 0, nb, 0).astype(np.int64)).cuda()
    col = torch.arange(K, device="cuda")
    pos = (base[:, None] + col[None, :]).clamp_(max=arena.numel() - 1)
    return torch.where(col[None, :] < take[:, None], arena[pos], torch.full_like(arena[:1], FILL)).reshape(-1)


def _chunk_status(w, kind, lst, d_slices, twin, roots=None):
    """a status per listed chunk from the existing calls: the twin's own where it reports one; for ranges the range planner's"""
    if kind == "one":
        return twin["sample_status"].cpu().numpy()
    if kind == "set":
        return twin["chunk_status"].cpu().numpy()
    files, first, count = lst
    if not twin["range_status"].any().item():
        return np.zeros(int(count.sum()), dtype=np.int32)
    return w["m"].bao.plan_samples_range_slices(w["ctx"], w["lens"], w["roots"] if roots is None else roots, files, first, count, d_slices)["sample_status"]


def _same_as_twin(w, kind, g, lst, d_slices, roots=None, have=True):
    """twin and packed call from 0xEE -> (the twin's receiver, the packed one's, the packed dict, the status per listed chunk)"""
    import torch
    m, (files, first, count) = w["m"], lst
    slots = m.bao.chunk_slots(w["lens"], files, first, count)
    n_slots = slots[0].size
    r, p = _slot_receiver(w, g, 0), _slot_receiver(w, g, n_slots)
    twin = _twin(w, kind, g, r, lst, d_slices, roots, have)
    got = _packed(w, kind, g, p, lst, d_slices, roots, have)
    for key in STATUS_KEYS[kind]:
        assert torch.equal(twin[key], got[key]), (kind, g, key)
    status = _chunk_status(w, kind, lst, d_slices, twin, roots)
    assert status.size == n_slots == int(got["slot_first"][-1]) and got["chunks"].data_ptr() == p["d_chunks"].data_ptr()
    assert torch.equal(p["d_obs"], r["d_obs"]), (kind, g, "the outboards are not the arena receiver's")
    assert torch.equal(p["d_have"], r["d_have"]) and (have or (p["d_have"].cpu().numpy() == p["pre"]).all())
    want = _expected_slots(w, r["d_arena"], slots, status)
    assert torch.equal(p["d_chunks"], want), (kind, g, "a slot is not the arena's chunk, or a byte beside a verified chunk was written")
    assert bool((p["d_arena"] == FILL).all().item()), "the packed call has no arena"
    for x, size in ((p["whole_c"], p["slot_bytes"]), (p["whole_o"], p["total"]), (r["whole_a"], r["size"]), (r["whole_o"], r["total"])):
        assert _walls_intact(x, size)
    return r, p, got, status, slots


# ---- clean lists ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("kind,name", _names())
def test_clean_lists_fill_their_slots_as_the_arena_receiver_fills_the_arena(kind, name, g):
    import torch
    w = _world()
    lst = _lists()[kind][name]
    d_slices, _ = _provide(w, kind, g, lst)
    r, p, got, status, slots = _same_as_twin(w, kind, g, lst, d_slices)
    assert not status.any()
    # and against the source itself: every listed chunk's bytes, the rest of a short last chunk's slot the fill
    assert torch.equal(p["d_chunks"], _expected_slots(w, w["d_src"], slots, status))
    f, c, off, nb = slots
    if name == "every chunk of every file":                                # the outboards are the provider's, byte for byte
        assert torch.equal(p["d_obs"], w["made"][g]["outboards"][:p["total"]])
        assert (nb == 0).any() and ((nb > 0) & (nb < K)).any() and (nb == K).any()
    if name == "repeated samples":
        assert len(set(zip(f.tolist(), c.tolist()))) < f.size
    if name == "overlapping, repeated, out of order":
        assert np.unique(np.stack([f.astype(np.uint64), c]), axis=1).shape[1] < f.size


@pytest.mark.parametrize("kind", KINDS)
def test_the_host_receivers_agree(kind):
    """a second opinion, one list a kind at g = 4: b3w_bao_*_ingest over the same slices, slice by slice on the host"""
    w = _world()
    m, g = w["m"], 4
    name = {"one": "repeated samples", "range": "overlapping, repeated, out of order", "set": "a set a file, sparse and dense"}[kind]
    files, first, count = lst = _lists()[kind][name]
    d_slices, sf = _provide(w, kind, g, lst)
    r, p, got, status, slots = _same_as_twin(w, kind, g, lst, d_slices)
    host = d_slices.cpu().numpy()
    ob_first, wf = w["made"][g]["ob_first"], w["wf"]
    arena, obs = np.full(w["arena"].size, FILL, dtype=np.uint8), np.full(int(ob_first[-1]), FILL, dtype=np.uint8)
    have = np.zeros(int(wf[-1]), dtype=np.uint64)
    if kind == "set":
        lay = m.bao.set_slice_layout(w["lens"], files, first, count)
        sets = [(int(f), tuple((int(a), int(k)) for a, k in zip(first[i:j], count[i:j])))
                for f, i, j in zip(lay["set_file"], lay["set_range_first"][:-1], lay["set_range_first"][1:])]
        sizes = [m.bao.set_slice_size(w["lens"][f], [a for a, _ in runs], [k for _, k in runs]) for f, runs in sets]
        slices = [host[int(at):int(at) + size].tobytes() for at, size in zip(lay["slice_first"][:-1], sizes)]
        arena, obs, have, st, fb, cs = _host_ingest(w, g, sets, slices, w["roots_host"])
        assert not any(st) and not any(cs)
        have = have.view(np.uint64)
    else:
        for i, (f, a, k) in enumerate(zip(files.tolist(), first.tolist(), count.tolist())):
            o, ln = int(w["offsets"][f]), w["lens"][f]
            data, ob = arena[o:o + ln], obs[int(ob_first[f]):int(ob_first[f + 1])]
            if kind == "one":
                sl = host[int(sf[i]):int(sf[i]) + m.bao.slice_size(ln, a)].tobytes()
                assert m.bao.ingest_slice_host(data, ob, ln, a, w["roots_host"][f], sl, g) == 0
                have[int(wf[f]) + (a >> 6)] |= np.uint64(1) << np.uint64(a & 63)
            else:
                sl = host[int(sf[i]):int(sf[i]) + m.bao.range_slice_size(ln, a, k)].tobytes()
                assert m.bao.ingest_range_slice_host(data, ob, ln, a, k, w["roots_host"][f], sl, g, have[int(wf[f]):int(wf[f + 1])]) == (0, None)
    import torch
    assert (p["d_obs"].cpu().numpy() == obs).all() and (p["d_have"].cpu().numpy() == (p["pre"] | have.view(np.int64))).all()
    assert torch.equal(p["d_chunks"], _expected_slots(w, torch.from_numpy(arena).cuda(), slots, status))


# ---- tampers ----------------------------------------------------------------------------------------------------------------------------
def _victims(w, kind):
    """-> (the list, [(its index of the victim slice, file, the restatement's slice, places, wanted chunks)])"""
    lens, n = w["lens"], w["n"]
    f_tile, f_70, f_one = lens.index(K * 1025), lens.index(70 * K + 1), next(f for f, ln in enumerate(lens) if 0 < ln <= K)
    f5 = len(lens) - 1
    out = []
    if kind == "set":
        sets = _receiver_sets(w)
        lst = _flat(sets)
        for f in (f_tile, f_70, f_one, f5):
            sl, places = _expected(f, sets[f][1])
            out.append((f, f, sl, places, RS.chunks_of(sets[f][1])))            # (a set a file, in file order: set f is file f's)
        return lst, out
    if kind == "range":
        rows = [(f_tile, 990, 35), (f_70, 3, 5), (f_tile, 0, 1025), (f_70, 60, 10), (f_one, 0, 1), (f_tile, 1010, 10), (f5, 2000, 1100)]
    else:
        rows = [(f_tile, 1000, 1), (f_70, 3, 1), (f_tile, 1024, 1), (f_70, 70, 1), (f_one, 0, 1), (f_tile, 1000, 1), (f5, 5120, 1)]
    lst = (np.array([x[0] for x in rows], dtype=np.uint32), np.array([x[1] for x in rows], dtype=np.uint64), np.array([x[2] for x in rows], dtype=np.uint64))
    for i in (0, 2, 3, 4, 6):
        f, a, k = rows[i]
        a0 = int(w["offsets"][f])
        data = w["arena"][a0:a0 + lens[f]].tobytes()
        key = ("set world", f)
        RR.seed(data, key)
        sl, places = RR.encode(data, a, k, key=key)
        out.append((i, f, sl, places, list(range(a, a + k))))
    return lst, out


@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("kind", KINDS)
def test_tampered_slices_leave_their_slots_alone_and_the_clean_ones_arrive(kind, g):
    """the existing tampers - a chunk byte (1), a node inside a block and one above it (2), the header (3) - a round a tamper, every
    victim beside good slices: the spoiled chunks' slots stay 0xEE, the clean ones arrive, every status is the arena receiver's"""
    import torch
    w = _world()
    lst, victims = _victims(w, kind)
    d_clean, sf = _provide(w, kind, g, lst)
    clean = d_clean.cpu().numpy()
    kinds = {i: [t for t in tampers(sl, places, wanted, w["lens"][f], [int(x) for x in w["roots_host"][f]]) if t[0] != "wrong root"]
             for i, f, sl, places, wanted in victims}
    for i, f, sl, places, wanted in victims:                               # the provider's slice is the restatement's
        assert clean[int(sf[i]):int(sf[i]) + len(sl)].tobytes() == sl, (kind, g, i)
    seen, whats = set(), set()
    for t in range(max(len(k) for k in kinds.values())):
        host = clean.copy()
        for i, f, sl, places, wanted in victims:
            if t < len(kinds[i]):
                what, bad, _, node = kinds[i][t]
                host[int(sf[i]):int(sf[i]) + len(bad)] = np.frombuffer(bad, dtype=np.uint8)
                whats.add(what)
        r, p, got, status, slots = _same_as_twin(w, kind, g, lst, torch.from_numpy(host).cuda())
        assert status.any() and not status.all(), (kind, g, t)
        bad_slots = p["d_chunks"].view(-1, K)[torch.from_numpy(status != 0).cuda()]
        assert bool((bad_slots == FILL).all().item())
        seen |= set(status.tolist())
    assert seen == {0, 1, 2, 3} and {"header", "the root node", "the last node", "a byte of the first wanted chunk"} <= whats
    # a wrong root: nothing of that file arrives
    roots = w["roots"].clone()
    for f in {f for _, f, _, _, _ in victims}:
        roots.view(-1)[8 * f + 3] ^= 0x10000
    r, p, got, status, slots = _same_as_twin(w, kind, g, lst, d_clean, roots=roots)
    hit = np.isin(slots[0], [f for _, f, _, _, _ in victims])
    assert (status[hit] != 0).all() and not status[~hit].any() and hit.any()


# ---- null outboards, optional arguments ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [0, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_null_outboards_decode_only(kind, g):
    import torch
    w = _world()
    name = {"one": "repeated samples", "range": "overlapping, repeated, out of order", "set": "a set a file, sparse and dense"}[kind]
    lst = _lists()[kind][name]
    d_slices, sf = _provide(w, kind, g, lst)
    host = d_slices.cpu().numpy().copy()
    of = w["m"].bao.set_slice_layout(w["lens"], *lst)["set_file"] if kind == "set" else lst[0]
    i = next(i for i, f in enumerate(of.tolist()) if w["n"][f] > 64)
    host[int(sf[i]) + 9] ^= 1                                              # (the root node of a slice: its chunks stay out, the others arrive)
    d_slices = torch.from_numpy(host).cuda()
    r, p, got, status, slots = _same_as_twin(w, kind, g, lst, d_slices)
    assert status.any() and not status.all()
    q = _slot_receiver(w, g, slots[0].size)
    before = (d_slices.clone(), w["roots"].clone())
    out = _packed(w, kind, g, q, lst, d_slices, obs=False)
    for key in STATUS_KEYS[kind]:
        assert torch.equal(out[key], got[key]), (kind, g, key)
    assert torch.equal(q["d_chunks"], p["d_chunks"]) and torch.equal(q["d_have"], p["d_have"])
    assert bool((q["d_obs"] == FILL).all().item()) and bool((q["d_arena"] == FILL).all().item())
    assert torch.equal(d_slices, before[0]) and torch.equal(w["roots"], before[1])
    assert _walls_intact(q["whole_c"], q["slot_bytes"]) and _walls_intact(q["whole_o"], q["total"])
    # and without the bitmap: the same slots and statuses, the bitmap handed to nobody
    q2 = _slot_receiver(w, g, slots[0].size)
    out2 = _packed(w, kind, g, q2, lst, d_slices, obs=False, have=False)
    assert all(torch.equal(out2[key], got[key]) for key in STATUS_KEYS[kind]) and torch.equal(q2["d_chunks"], p["d_chunks"])
    assert (q2["d_have"].cpu().numpy() == q2["pre"]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_without_a_bitmap_the_twin_without_one(kind):
    w = _world()
    lst = _lists()[kind]["the short last chunk alone"]
    d_slices, _ = _provide(w, kind, 0, lst)
    _same_as_twin(w, kind, 0, lst, d_slices, have=False)


# ---- the C calls: guards, optional outputs, refusals, no allocation ---------------------------------------------------------------------
def _int_walled(n, width):
    """n integers of `width` bytes, every byte 0xEE, between guards -> (whole, the middle as bytes, as integers)"""
    import torch
    whole, mid = _walled(width * n)
    return whole, mid, mid.view(torch.int32 if width == 4 else torch.int64)


def _c_setup(w, kind, g, lst, d_slices):
    import torch
    m, L = w["m"], w["m"].lib()
    files, first, count = lst
    slots = m.bao.chunk_slots(w["lens"], files, first, count)
    p = _slot_receiver(w, g, slots[0].size)
    args = (w["ln"].ctypes.data, len(w["lens"]), files.ctypes.data, first.ctypes.data, count.ctypes.data, files.size)
    need = 0 if kind == "one" else (L.b3w_bao_range_slice_ingest_scratch_bytes if kind == "range" else L.b3w_bao_set_slice_ingest_scratch_bytes)(*args)
    n_out = files.size if kind != "set" else m.bao.set_slice_layout(w["lens"], files, first, count)["set_file"].size
    p["st"], p["fb"], p["cs"], p["scratch"] = _int_walled(n_out, 4), _int_walled(n_out, 8), _int_walled(slots[0].size, 4), _walled(max(need, 16))
    p["need"], p["slots"], p["lst"], p["d_slices"] = need, slots, lst, d_slices
    return p


def _c_call(w, kind, g0, p, **change):
    import torch
    files, first, count = p["lst"]
    kw = dict(ctx=w["ctx"].handle, d_chunks=p["d_chunks"].data_ptr(), chunks_bytes=p["slot_bytes"], lens=w["ln"].ctypes.data, n_files=len(w["lens"]), g=g0,
              d_obs=p["d_obs"].data_ptr(), d_roots=w["roots"].data_ptr(), files=files.ctypes.data, first=first.ctypes.data)
    if kind != "one":
        kw["count"] = count.ctypes.data
    kw.update(n=files.size, d_slices=p["d_slices"].data_ptr(), d_st=p["st"][2].data_ptr())
    if kind != "one":
        kw["d_fb"] = p["fb"][2].data_ptr()
    if kind == "set":
        kw["d_cs"] = p["cs"][2].data_ptr()
    kw["d_have"] = p["d_have"].data_ptr()
    if kind != "one":
        kw.update(d_scratch=p["scratch"][1].data_ptr(), scratch_bytes=p["scratch"][1].numel())
    for name, value in change.items():
        assert name in kw, name
        kw[name] = value.ctypes.data if isinstance(value, np.ndarray) else value
    L = w["m"].lib()
    fn = {"one": L.b3w_bao_slice_ingest_packed_device, "range": L.b3w_bao_range_slice_ingest_packed_device, "set": L.b3w_bao_set_slice_ingest_packed_device}[kind]
    return fn(*kw.values(), torch.cuda.current_stream().cuda_stream)


def _c_untouched(p, pre):
    import torch
    torch.cuda.synchronize()
    return (all(bool((x == FILL).all().item()) for x in (p["d_chunks"], p["d_obs"], p["st"][1], p["fb"][1], p["cs"][1], p["scratch"][1]))
            and torch.equal(p["d_have"], pre))


def _c_walls(p):
    return (_walls_intact(p["whole_c"], p["slot_bytes"]) and _walls_intact(p["whole_o"], p["total"]) and all(
        _walls_intact(p[k][0], p[k][1].numel()) for k in ("st", "fb", "cs")) and _walls_intact(p["scratch"][0], p["scratch"][1].numel()))


@pytest.mark.parametrize("kind", KINDS)
def test_guards_optional_outputs_and_no_allocation(kind):
    """the C call with every output between 0xA5 guards - slots, outboards, statuses, scratch; the set call without a chunk status; and
    a second call allocates nothing"""
    import torch
    w = _world()
    g = 4
    lst = _lists()[kind]["a set a file, sparse and dense" if kind != "one" else "repeated samples"]
    d_slices, _ = _provide(w, kind, g, lst)
    r, ref, got, status, slots = _same_as_twin(w, kind, g, lst, d_slices)
    p = _c_setup(w, kind, g, lst, d_slices)
    assert _c_call(w, kind, g, p) == 0, w["ctx"].last_error()
    torch.cuda.synchronize()
    assert _c_walls(p)
    assert torch.equal(p["d_chunks"], ref["d_chunks"]) and torch.equal(p["d_obs"], ref["d_obs"]) and torch.equal(p["d_have"], ref["d_have"])
    assert torch.equal(p["st"][2], got[STATUS_KEYS[kind][0]])
    if kind != "one":
        assert torch.equal(p["fb"][2], got[STATUS_KEYS[kind][1]])
        used = p["scratch"][1][p["need"]:]
        assert bool((used == FILL).all().item()), "a byte of the scratch behind what the size call says was written"
    if kind == "set":
        assert torch.equal(p["cs"][2], got["chunk_status"])
        q = _c_setup(w, kind, g, lst, d_slices)
        assert _c_call(w, kind, g, q, d_cs=None, d_have=None) == 0, w["ctx"].last_error()
        torch.cuda.synchronize()
        assert torch.equal(q["d_chunks"], ref["d_chunks"]) and torch.equal(q["st"][2], got["set_status"]) and bool((q["cs"][1] == FILL).all().item())
        assert (q["d_have"].cpu().numpy() == q["pre"]).all() and _c_walls(q)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    assert _c_call(w, kind, g, p) == 0, w["ctx"].last_error()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_every_output_untouched(kind):
    import torch
    w = _world()
    m, g = w["m"], 0
    lst = _lists()[kind]["a set a file, sparse and dense" if kind != "one" else "repeated samples"]
    files, first, count = lst
    d_slices, _ = _provide(w, kind, g, lst)
    p = _c_setup(w, kind, g, lst, d_slices)
    pre = p["d_have"].clone()
    need = p["slot_bytes"]

    def refused(**change):
        return _c_call(w, kind, g, p, **change) == BAD and _c_untouched(p, pre)
    assert refused(chunks_bytes=need - 1), "a slot buffer one byte short"
    assert str(need) in w["ctx"].last_error() and "chunks_bytes" in w["ctx"].last_error(), w["ctx"].last_error()
    assert refused(d_chunks=p["d_chunks"].data_ptr() + 8), "slots that are not 16-byte aligned"
    assert "16-byte" in w["ctx"].last_error()
    assert refused(d_chunks=None), "no slot buffer"
    assert "d_chunks" in w["ctx"].last_error() and str(need) in w["ctx"].last_error()
    assert refused(ctx=None) and refused(g=7)
    for name in ("lens", "d_roots", "files", "first", "d_slices", "d_st") + (() if kind == "one" else ("count", "d_fb", "d_scratch")):
        assert refused(**{name: None}), name
    assert refused(d_obs=p["d_obs"].data_ptr() + 4) and refused(d_slices=d_slices.data_ptr() + 8) and refused(d_have=p["d_have"].data_ptr() + 4)
    bad_file, bad_first = files.copy(), first.copy()
    bad_file[-1], bad_first[-1] = len(w["lens"]), 1 << 40
    assert refused(files=bad_file) and refused(first=bad_first)
    if kind != "one":
        zero = count.copy()
        zero[0] = 0
        assert refused(count=zero) and refused(scratch_bytes=p["need"] - 16) and refused(d_scratch=p["scratch"][1].data_ptr() + 8)
        assert refused(d_fb=p["fb"][2].data_ptr() + 4)
    if kind == "set":
        swapped = first.copy()
        j = next(i for i in range(1, files.size) if files[i] == files[i - 1])
        swapped[j] = first[j - 1]
        assert refused(first=swapped) and "disjoint" in w["ctx"].last_error()
        assert refused(d_cs=p["cs"][2].data_ptr() + 2)
    with pytest.raises(m.B3WError):
        _packed(w, kind, 7, p, lst, d_slices)
    with pytest.raises(m.B3WError):                                        # the wrapper hands a short buffer through: the call says what it needs
        short = dict(p, d_chunks=p["d_chunks"][:need - 1024])
        _packed(w, kind, g, short, lst, d_slices)
    assert _c_untouched(p, pre)
    # an empty list: a no-op, whatever else is handed in
    L = m.lib()
    h = w["ctx"].handle
    if kind == "one":
        assert L.b3w_bao_slice_ingest_packed_device(h, None, 0, None, 0, 0, None, None, None, None, 0, None, None, None, None) == 0
    elif kind == "range":
        assert L.b3w_bao_range_slice_ingest_packed_device(h, None, 0, None, 0, 0, None, None, None, None, None, 0, None, None, None, None, None, 0, None) == 0
    else:
        assert L.b3w_bao_set_slice_ingest_packed_device(h, None, 0, None, 0, 0, None, None, None, None, None, 0, None, None, None, None, None, None, 0, None) == 0
    assert _c_untouched(p, pre)
    # and the same arguments unchanged are taken
    assert _c_call(w, kind, g, p) == 0, w["ctx"].last_error()
    torch.cuda.synchronize()
    assert not p["st"][2].any().item() and _c_walls(p)
    assert torch.equal(p["d_chunks"], _expected_slots(w, w["d_src"], p["slots"], np.zeros(p["slots"][0].size)))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("half", [False, True])
def test_provider_from_packed_bytes_to_files_on_the_host(half, g):
    """neither side holds a file on the device: set_slices_packed from the listed chunks alone, ingest_set_slices_packed into slots, the
    slots to the host, scatter_chunks into zeroed files.  The whole list gives the source's files; half of the chunks (a seeded bitmap
    through have_runs_host) exactly the listed bytes, and the outboards the arena receiver leaves for them"""
    import torch
    w = _world()
    m = w["m"]
    lens, n = w["lens"], w["n"]
    rng = np.random.default_rng(4242 + g)
    files, first, count = [], [], []
    for f, k in enumerate(n):
        have = np.zeros((k + 63) // 64, dtype=np.uint64)
        if half:
            bits = rng.random(k) < 0.5
            np.bitwise_or.at(have, np.flatnonzero(bits) >> 6, np.uint64(1) << (np.flatnonzero(bits) & 63).astype(np.uint64))
        a, c, _, _ = m.bao.have_runs_host(have, lens[f], kind="missing")
        files += [f] * a.size
        first += a.tolist()
        count += c.tolist()
    lst = (np.array(files, dtype=np.uint32), np.array(first, dtype=np.uint64), np.array(count, dtype=np.uint64))
    d_packed = m.bao.pack_ranges(w["arena"], w["offsets"], lens, *lst, group_log=g)
    prov = m.bao.set_slices_packed(w["ctx"], d_packed.reshape(-1), lens, w["made"][g]["outboards"], *lst, group_log=g)
    slots = m.bao.chunk_slots(lens, *lst)
    r, p = _slot_receiver(w, g, 0), _slot_receiver(w, g, slots[0].size)
    got = _packed(w, "set", g, p, lst, prov["slices"])
    assert not got["chunk_status"].any().item() and not got["set_status"].any().item()
    dest = [np.zeros(ln, dtype=np.uint8) for ln in lens]
    wrote = m.bao.scatter_chunks(dest, p["d_chunks"].cpu(), got["chunk_status"], slots)
    assert wrote == int(slots[3].sum())
    listed = [np.zeros(ln, dtype=bool) for ln in lens]                      # (a file at a time: the world has one file under two indices)
    for f, c, nb in zip(slots[0].tolist(), slots[1].tolist(), slots[3].tolist()):
        listed[f][K * c:K * c + nb] = True
    for f, ln in enumerate(lens):
        o = int(w["offsets"][f])
        assert (dest[f] == np.where(listed[f], w["arena"][o:o + ln], 0)).all(), (f, "not exactly the listed bytes")
    if not half:
        assert all(dest[f].tobytes() == w["arena"][int(w["offsets"][f]):int(w["offsets"][f]) + ln].tobytes() for f, ln in enumerate(lens))
        assert torch.equal(p["d_obs"], w["made"][g]["outboards"][:p["total"]])
    else:
        assert 0.3 < sum(int(x.sum()) for x in listed) / sum(lens) < 0.7
    twin = _twin(w, "set", g, r, lst, prov["slices"])
    obs, provider = p["d_obs"], w["made"][g]["outboards"][:p["total"]]
    assert torch.equal(obs, r["d_obs"]) and torch.equal(p["d_have"], r["d_have"]) and torch.equal(twin["chunk_status"], got["chunk_status"])
    written = obs != FILL
    assert torch.equal(obs[written], provider[written]) and int(written.sum().item()) > 0


def test_a_call_on_a_side_stream_orders_behind_what_it_was_told_to():
    """the default stream is busy and then fills the slot buffer; an event joins the side stream behind that fill; the call on the side
    stream must land in the verified slots after it"""
    import torch
    w = _world()
    g = 0
    lst = _lists()["set"]["every chunk of every file"]
    d_slices, _ = _provide(w, "set", g, lst)
    slots = w["m"].bao.chunk_slots(w["lens"], *lst)
    p = _slot_receiver(w, g, slots[0].size)
    busy = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for v in range(8):
        busy.fill_(v)
    p["d_chunks"].fill_(0x11)
    done = torch.cuda.Event()
    done.record()
    side.wait_event(done)
    with torch.cuda.stream(side):                                           # (the wrapper's own status tensors are made on the stream it runs on)
        got = _packed(w, "set", g, p, lst, d_slices, stream=side.cuda_stream)
    side.synchronize()
    torch.cuda.synchronize()
    assert not got["chunk_status"].any().item()
    want = _expected_slots(w, w["d_src"], slots, np.zeros(slots[0].size))
    verified = want != FILL                                                 # (a source byte of 0xEE is compared all the same below)
    assert torch.equal(p["d_chunks"][verified], want[verified])
    f, c, off, nb = slots
    cols = torch.arange(K, device="cuda")[None, :] < torch.from_numpy(nb.astype(np.int64)).cuda()[:, None]
    assert torch.equal(p["d_chunks"].view(-1, K)[cols], _expected_slots(w, w["d_src"], slots, np.zeros(f.size)).view(-1, K)[cols])
    assert bool((p["d_chunks"].view(-1, K)[~cols] == 0x11).all().item()), "the rest of a short last chunk's slot keeps the fill"
