"""Whole files verified against their outboards on the device (bao.verify_batch, b3w_bao_verify_batch_device): clean batches of every
shape give all-zero statuses; on tampered arenas, outboards and roots the status of every unit is the sample_status the existing
planners give a sample in that unit (plan_samples_batch with EVERY chunk as a sample, plan_samples_groups_batch with one sample a
group) and the host decoder's (bao.verify_host); tampering stays with the file it hits and file_status / first_bad are what
unit_status implies; repeated calls agree; the call is a batch; refusals come before anything is written."""
import statistics
import time

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
from test_gpu_bao_batch import _arena, _file
from test_gpu_bao_groups import _shapes

pytestmark = pytest.mark.gpu

GS = [0, 1, 4, 6]
K = 1024
NONE = (1 << 64) - 1
# small files (at most 64 chunks, several to a wave), one-tile files, files of several tiles (a lone last chunk, a short last tile, whole tiles)
SMALL, ONE_TILE, MULTI = [0, 700, 3 * K + 5, 37 * K, 64 * K, 2 * K], [100 * K + 77, 1 << 20, 65 * K], [(1 << 20) + 1, 2049 * K + 3, 3 << 20]
LENS = [SMALL[0], MULTI[0], SMALL[1], ONE_TILE[0], SMALL[2], MULTI[1], SMALL[3], ONE_TILE[1], SMALL[4], MULTI[2], SMALL[5], ONE_TILE[2]]


def _units(m, length, g):
    return (m.bao.num_chunks(length) + (1 << g) - 1) >> g


def _outboards(m, ctx, d_arena, offsets, lens, g):
    return m.bao.outboard_batch(ctx, d_arena, offsets, lens) if g == 0 else m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)


def _got(out):
    """verify_batch's dict on the host: (unit statuses, unit_first, file statuses, first bad units as uint64)"""
    return (out["unit_status"].cpu().numpy(), [int(x) for x in out["unit_first"]], out["file_status"].cpu().numpy(),
            out["first_bad"].cpu().numpy().view(np.uint64))


def _assert_summaries(st, uf, fs, fb):
    """file_status and first_bad are what unit_status implies"""
    for f in range(len(uf) - 1):
        mine = st[uf[f]:uf[f + 1]]
        bad = np.nonzero(mine)[0]
        assert int(fs[f]) == int(mine.max()), f
        assert int(fb[f]) == (int(bad[0]) if bad.size else NONE), f


def _assert_clean(m, out, lens, g):
    st, uf, fs, fb = _got(out)
    assert uf == [0] + list(np.cumsum([_units(m, int(x), g) for x in lens]))
    assert st.size == uf[-1] and not st.any(), np.nonzero(st)[0][:10]
    assert not fs.any() and (fb == NONE).all()


@pytest.mark.parametrize("g", GS)
def test_clean_batches(g):
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    # every shape, two files off a 16-byte boundary, an empty file, one file listed twice
    arena, offsets, lens = _shapes()
    assert 0 in lens and int(offsets[2]) % 2 == 1
    d_arena = torch.from_numpy(arena).cuda()
    ob = _outboards(m, ctx, d_arena, offsets, lens, g)
    _assert_clean(m, m.bao.verify_batch(ctx, d_arena, offsets, lens, ob["outboards"], ob["roots"], g), lens, g)
    none = m.bao.verify_batch(ctx, d_arena, [], [], ob["outboards"], ob["roots"], g)
    assert none["unit_status"].numel() == 0 and none["file_status"].numel() == 0 and list(none["unit_first"]) == [0]
    # many 4 KiB files, back to back, made on the device; every third one chunk shorter and ragged
    n_files = 20000
    lens = np.full(n_files, 4 * K, dtype=np.uint64)
    lens[::3] -= 1500
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    d_arena = torch.randint(0, 256, (int(lens.sum()),), dtype=torch.uint8, device="cuda", generator=gen)
    ob = _outboards(m, ctx, d_arena, offsets, lens, g)
    _assert_clean(m, m.bao.verify_batch(ctx, d_arena, offsets, lens, ob["outboards"], ob["roots"], g), lens, g)
    ctx.close()


@pytest.mark.parametrize("g", GS)
def test_a_clean_file_of_1026_tiles(g):
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(256)
    lens = [3000, (1 << 30) + (1 << 20) + 5, 1, 70 * 1024]
    offsets = np.array([0, 3008, 3008 + lens[1] + 3, 3008 + lens[1] + 16], dtype=np.uint64)
    d_arena = torch.randint(0, 256, (int(offsets[3]) + lens[3],), dtype=torch.uint8, device="cuda", generator=gen)
    ob = _outboards(m, ctx, d_arena, offsets, lens, g)
    out = m.bao.verify_batch(ctx, d_arena, offsets, lens, ob["outboards"], ob["roots"], g)
    _assert_clean(m, out, lens, g)
    # past the second storey too: a byte of the last tile, a node over the first 1 024 tiles, and the clean files beside them
    G = 1 << g
    d_arena[3008 + lens[1] - 3] ^= 1
    bad = ob["outboards"].clone()
    at = int(ob["ob_first"][1]) + 8
    bad[at + 64 + 9] ^= 1                                                   # node 1: the left subtree of the root, chunks [0, 2^20)
    st, uf, fs, fb = _got(m.bao.verify_batch(ctx, d_arena, offsets, lens, bad, ob["roots"], g))
    mine = st[uf[1]:uf[2]]
    assert mine.size == ((1 << 20) + 1024 + 1 + G - 1) // G
    assert (mine[:(1 << 20) // G] == 2).all() and not mine[(1 << 20) // G:-1].any() and mine[-1] == 1
    assert not st[:uf[1]].any() and not st[uf[2]:].any()
    assert list(fs) == [0, 2, 0, 0] and list(fb) == [NONE, 0, NONE, NONE]
    ctx.close()


def _node_of(spans, first, count):
    return spans.index((first, count))


def _scenarios(m, lens, g):
    """name -> (chunk bytes to flip: (file, chunk), node bytes: (file, node index), root words: file, headers: file)"""
    f_small, f_one, f_multi = LENS.index(37 * K), LENS.index(100 * K + 77), LENS.index(2049 * K + 3)
    f_lone, f_whole, f_mib, f_64k, f_one_chunk, f_empty = (LENS.index((1 << 20) + 1), LENS.index(3 << 20), LENS.index(1 << 20), LENS.index(64 * K),
                                                           LENS.index(700), LENS.index(0))
    n = [m.bao.num_chunks(x) for x in lens]
    nu = [_units(m, x, g) for x in lens]
    spans = {f: GR.node_spans(nu[f]) for f in range(len(lens))}
    T1 = 1024 >> g                                                           # units to a tile
    chunks = [(f, c) for f in (f_small, f_one, f_multi, f_whole) for c in (0, n[f] // 2, n[f] - 1)] + [(f_lone, 1024), (f_whole, 2048), (f_64k, 63)]
    lowest = [(f, nu[f] - 2) for f in (f_small, f_64k, f_one, f_mib, f_multi, f_whole, f_lone) if nu[f] >= 2]
    tile_roots = [(f_one, 0), (f_mib, 0), (f_multi, _node_of(spans[f_multi], T1, T1)), (f_whole, _node_of(spans[f_whole], 2 * T1, T1)),
                  (f_whole, _node_of(spans[f_whole], 0, T1))]
    above = [(f_lone, 0), (f_whole, _node_of(spans[f_whole], 0, 2 * T1)), (f_multi, 0)]
    assert all(spans[f][i][1] > T1 for f, i in above)
    roots = [f_small, f_one, f_whole, f_one_chunk, f_empty]
    headers = [f_64k, f_mib, f_multi, f_empty]
    return {
        "chunk bytes": (chunks, [], [], []),
        "lowest nodes": ([], lowest, [], []),
        "tile roots": ([], tile_roots, [], []),
        "above the tiles": ([], above, [], []),
        "roots": ([], [], roots, []),
        "headers": ([], [], [], headers),
        "mixed": ([(f_small, 3), (f_whole, 1500), (f_multi, 2048)], [(f_whole, _node_of(spans[f_whole], 0, T1)), (f_one, nu[f_one] - 2), (f_multi, 0)],
                  [f_lone], [f_mib]),
    }


def _plan_every_unit(m, ctx, d_arena, offsets, lens, d_obs, d_roots, g):
    """the oracle on the device: the existing planner with one sample in every unit of every file -> its sample_status"""
    files = np.concatenate([np.full(_units(m, x, g), f, dtype=np.uint32) for f, x in enumerate(lens)])
    chunks = np.concatenate([np.arange(_units(m, x, g), dtype=np.uint64) << np.uint64(g) for x in lens])
    if g == 0:
        cb = m.bao.chunk_bytes_batch(d_arena, offsets, lens, files, chunks)
        return m.bao.plan_samples_batch(ctx, d_obs, lens, d_roots, files, chunks, cb)["sample_status"]
    gb = m.bao.group_bytes_batch(d_arena, offsets, lens, files, chunks, g)
    return m.bao.plan_samples_groups_batch(ctx, d_obs, lens, d_roots, files, chunks, gb, g)["sample_status"]


@pytest.mark.parametrize("g", GS)
def test_tampered_batches_against_the_planner_and_the_host_decoder(g):
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    lens = LENS
    arena, offsets = _arena(lens, starts_odd=(3, 6), seed=21)
    d_clean = torch.from_numpy(arena).cuda()
    ob = _outboards(m, ctx, d_clean, offsets, lens, g)
    ob_first = [int(x) for x in ob["ob_first"]]
    _assert_clean(m, m.bao.verify_batch(ctx, d_clean, offsets, lens, ob["outboards"], ob["roots"], g), lens, g)
    assert not _plan_every_unit(m, ctx, d_clean, offsets, lens, ob["outboards"], ob["roots"], g).any()
    for name, (chunks, nodes, roots, headers) in _scenarios(m, lens, g).items():
        d_arena, d_obs, d_roots = d_clean.clone(), ob["outboards"].clone(), ob["roots"].clone()
        touched = set()
        for f, c in chunks:
            a = c * 1024
            d_arena[int(offsets[f]) + a + (c * 7) % min(1024, lens[f] - a)] ^= 1
            touched.add(f)
        for k, (f, i) in enumerate(nodes):
            assert 0 <= i < _units(m, lens[f], g) - 1
            d_obs[ob_first[f] + 8 + 64 * i + (11 * k + 32 * (k & 1)) % 64] ^= 1
            touched.add(f)
        for f in roots:
            d_roots[f, (f + 3) % 8] ^= 0x10000
            touched.add(f)
        for f in headers:
            d_obs[ob_first[f] + f % 8] ^= 1
            touched.add(f)
        st, uf, fs, fb = _got(m.bao.verify_batch(ctx, d_arena, offsets, lens, d_obs, d_roots, g))
        want = _plan_every_unit(m, ctx, d_arena, offsets, lens, d_obs, d_roots, g)
        assert st.size == want.size
        diff = np.nonzero(st != want)[0]
        assert diff.size == 0, (g, name, [(int(u), int(st[u]), int(want[u])) for u in diff[:8]])
        _assert_summaries(st, uf, fs, fb)
        # tampering stays local: every file that was not touched is clean, every touched one is not
        for f in range(len(lens)):
            assert bool(st[uf[f]:uf[f + 1]].any()) == (f in touched), (g, name, f)
            assert (int(fs[f]) != 0) == (f in touched) and (int(fb[f]) != NONE) == (f in touched), (g, name, f)
        # the host decoder on the touched files
        host_arena, host_obs, host_roots = d_arena.cpu().numpy(), d_obs.cpu().numpy(), d_roots.cpu().numpy().view(np.uint32)
        for f in sorted(touched):
            hs, hfs, hfb = m.bao.verify_host(_file(host_arena, offsets, lens, f), host_obs[ob_first[f]:ob_first[f + 1]].tobytes(), host_roots[f], g)
            assert np.array_equal(hs, st[uf[f]:uf[f + 1]]), (g, name, f)
            assert (hfs, hfb) == (int(fs[f]), int(fb[f])), (g, name, f)
    ctx.close()


@pytest.mark.parametrize("g", [4, 6])
def test_forty_repeated_calls_agree(g):
    """equality over repeated calls on one clean batch: what showed the level loop's missing LDS wait in the group outboard kernels"""
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    arena, offsets, lens = _shapes()
    d_arena = torch.from_numpy(arena).cuda()
    ob = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
    for k in range(40):
        out = m.bao.verify_batch(ctx, d_arena, offsets, lens, ob["outboards"], ob["roots"], g)
        assert not out["unit_status"].any().item() and not out["file_status"].any().item() and bool((out["first_bad"] == -1).all().item()), (g, k)
    ctx.close()


def test_it_is_a_batch():
    """4 096 files of 16 KiB: one call against a loop of one-file calls — the call's launches do not grow with the file count"""
    import torch
    m = T.pkg()
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    n_files, ln = 4096, 16 * 1024
    lens = np.full(n_files, ln, dtype=np.uint64)
    offsets = (np.arange(n_files, dtype=np.uint64) * ln)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(16)
    d_arena = torch.randint(0, 256, (n_files * ln,), dtype=torch.uint8, device="cuda", generator=gen)
    ob = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    d_obs, d_roots = ob["outboards"], ob["roots"]
    d_obs[int(ob["ob_first"][77]) + 8 + 64 * 3 + 1] ^= 1                   # (something to find)
    uf = m.bao.verify_layout(lens)
    d_st, d_fs, d_fb = (torch.empty(int(uf[-1]), dtype=torch.uint8, device="cuda"), torch.empty(n_files, dtype=torch.int32, device="cuda"),
                        torch.empty(n_files, dtype=torch.int64, device="cuda"))
    d_st1, d_fs1, d_fb1 = torch.empty_like(d_st), torch.empty_like(d_fs), torch.empty_like(d_fb)
    assert L.b3w_bao_verify_scratch_bytes(lens.ctypes.data, n_files) == 0
    stream = torch.cuda.current_stream().cuda_stream
    one_off, one_len = np.zeros(1, dtype=np.uint64), np.array([ln], dtype=np.uint64)
    base, obs, roots = d_arena.data_ptr(), d_obs.data_ptr(), d_roots.data_ptr()
    firsts, ufs = [int(x) for x in ob["ob_first"]], [int(x) for x in uf]

    def batch():
        t = time.perf_counter()
        rc = L.b3w_bao_verify_batch_device(ctx.handle, base, offsets.ctypes.data, lens.ctypes.data, n_files, 0, obs, roots, d_st.data_ptr(),
                                           d_fs.data_ptr(), d_fb.data_ptr(), None, 0, stream)
        torch.cuda.synchronize()
        assert rc == 0
        return time.perf_counter() - t

    def loop():
        t = time.perf_counter()
        for f in range(n_files):
            rc = L.b3w_bao_verify_batch_device(ctx.handle, base + f * ln, one_off.ctypes.data, one_len.ctypes.data, 1, 0, obs + firsts[f], roots + 32 * f,
                                               d_st1.data_ptr() + ufs[f], d_fs1.data_ptr() + 4 * f, d_fb1.data_ptr() + 8 * f, None, 0, stream)
            assert rc == 0
        torch.cuda.synchronize()
        return time.perf_counter() - t
    for _ in range(3):
        batch()
        loop()
    assert torch.equal(d_st, d_st1) and torch.equal(d_fs, d_fs1) and torch.equal(d_fb, d_fb1)
    assert int(d_fs.sum().item()) == 2 and int(d_fs[77].item()) == 2 and int(d_st.count_nonzero().item()) == 2
    t_batch = statistics.median(batch() for _ in range(5))
    t_loop = statistics.median(loop() for _ in range(5))
    print(f"4096 x 16 KiB: verify batch {t_batch * 1e3:.3f} ms, loop of one-file calls {t_loop * 1e3:.3f} ms, ratio {t_loop / t_batch:.1f}")
    assert t_batch < t_loop
    ctx.close()


def test_refusals_come_before_anything_is_written():
    import torch
    m = T.pkg()
    L = m.lib()
    ctx = m.Context("compression", 0)                                      # (any context verifies)
    lens = [37 * K, (2 << 20) + 5, 0, 100 * K]
    arena, offsets = _arena(lens, seed=4)
    ln = np.array(lens, dtype=np.uint64)
    d_arena = torch.from_numpy(arena).cuda()
    ob = m.bao.outboard_batch(ctx, d_arena, offsets, ln)
    uf = m.bao.verify_layout(ln)
    need = L.b3w_bao_verify_scratch_bytes(ln.ctypes.data, ln.size)
    assert need == (36 * 3 + 15) // 16 * 16
    d_st = torch.full((int(uf[-1]),), 0xA5, dtype=torch.uint8, device="cuda")
    d_fs = torch.full((4,), -77, dtype=torch.int32, device="cuda")
    d_fb = torch.full((5,), 1234567, dtype=torch.int64, device="cuda")
    d_scratch = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    bad = m.B3W_E_BAD_ARGUMENT

    def call(arena_ptr=d_arena.data_ptr(), g=0, obs=ob["outboards"].data_ptr(), roots=ob["roots"].data_ptr(), st=d_st.data_ptr(), fs=d_fs.data_ptr(),
             fb=d_fb.data_ptr(), scratch=d_scratch.data_ptr(), scratch_bytes=need, off=offsets.ctypes.data, lengths=ln.ctypes.data):
        return L.b3w_bao_verify_batch_device(ctx.handle, arena_ptr, off, lengths, ln.size, g, obs, roots, st, fs, fb, scratch, scratch_bytes,
                                             torch.cuda.current_stream().cuda_stream)
    for kw, word in ((dict(scratch_bytes=need - 1), "scratch"), (dict(g=7), "group_log"), (dict(scratch=None), "scratch"),
                     (dict(scratch=d_scratch.data_ptr() + 4), "scratch"), (dict(st=None), "null"), (dict(fs=None), "null"), (dict(fb=None), "null"),
                     (dict(obs=None), "null"), (dict(roots=None), "null"), (dict(off=None), "null"), (dict(lengths=None), "null"),
                     (dict(fb=d_fb.data_ptr() + 4), "aligned"), (dict(obs=ob["outboards"].data_ptr() + 4), "aligned"), (dict(arena_ptr=None), "arena")):
        assert call(**kw) == bad, kw
        assert word in ctx.last_error(), (kw, ctx.last_error())
    too_long = np.array([(1 << 40) + 1025], dtype=np.uint64)
    assert L.b3w_bao_verify_batch_device(ctx.handle, d_arena.data_ptr(), offsets.ctypes.data, too_long.ctypes.data, 1, 0, ob["outboards"].data_ptr(),
                                         ob["roots"].data_ptr(), d_st.data_ptr(), d_fs.data_ptr(), d_fb.data_ptr(), d_scratch.data_ptr(), 1 << 62, 0) == bad
    assert L.b3w_bao_verify_batch_device(None, None, None, None, 0, 0, None, None, None, None, None, None, 0, None) == bad
    with pytest.raises(m.B3WError):
        m.bao.verify_batch(ctx, d_arena, offsets + np.uint64(arena.size), ln, ob["outboards"], ob["roots"])      # past the end of the arena
    with pytest.raises(m.B3WError):
        m.bao.verify_batch(ctx, d_arena, offsets, ln, ob["outboards"], ob["roots"], 7)
    torch.cuda.synchronize()
    assert bool((d_st == 0xA5).all().item()) and bool((d_fs == -77).all().item()) and bool((d_fb == 1234567).all().item())
    assert bool((d_scratch == 0x5A).all().item())
    # no files: a no-op; and the same buffers through a call that runs: only the four files' entries are written
    assert L.b3w_bao_verify_batch_device(ctx.handle, None, None, None, 0, 0, None, None, None, None, None, None, 0, 0) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert not d_st.any().item() and not d_fs.any().item() and d_fb.cpu().tolist() == [-1, -1, -1, -1, 1234567]
    ctx.close()
