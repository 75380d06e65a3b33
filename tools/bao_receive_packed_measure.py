#!/usr/bin/env python3
"""tools/bao_receive_packed_measure.py <out_dir> [--parent-lib libb3wit.so] [--cases a,b,...] — the packed receivers
(b3w_bao_slice_ingest_packed_device, b3w_bao_range_slice_ingest_packed_device, b3w_bao_set_slice_ingest_packed_device) against the
arena receivers of the same kind over the same slices into a resident arena.

  yardstick   of the library given with --parent-lib (a build of the parent commit, loaded beside this one, a context of its own) or,
              without it, of this library: b3w_bao_slice_ingest_have_device, b3w_bao_range_slice_ingest_device,
              b3w_bao_set_slice_ingest_device into a 1 GiB arena.
  method      tools/bao_set_measure.py's: the routes alternating in one process, device events around each whole C call (the host's
              table fill and upload included), medians over about a second a route.  The yardstick runs as two interleaved series A
              and B; |median A - median B| is the spread a difference has to exceed.  BEFORE TIMING both routes run into buffers of
              0xEE and are compared: statuses, outboards and bitmap byte for byte, slot k against the arena's k-th listed chunk, the
              bytes behind a short chunk and every unlisted byte still 0xEE.
  cases       one 1 GiB file: the runs of a bitmap with half its chunks missing (set slices), 65 536 runs of one chunk (one-chunk and
              set slices), 4 096 runs of 16 (range slices), 64 runs of 1 024 chunks at starts that are not tile-aligned (range slices,
              g = 0 and g = 4).  With --decode each case also times the packed call with null outboards.
  expectation (supposed from the code, not measured beforehand): the packed call lands within the yardstick's spread of the arena call;
              recorded per case as within / slower / faster.  No profiler is run.
Writes <out_dir>/bao_receive_packed_measure.json."""
import argparse, ctypes, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats
from bao_range_measure import runs_64x1024, runs_half_missing, runs_of
from bao_set_measure import sorted_runs

m = __import__("hot-proofs-blake3-circom_amd")

FILL = 0xEE
N = BM.GIB // 1024
ONE = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 4 + \
      [ctypes.c_uint32] + [ctypes.c_void_p] * 4
RANGE = ONE[:11] + [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 5 + [ctypes.c_uint64, ctypes.c_void_p]
SET = ONE[:11] + [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 6 + [ctypes.c_uint64, ctypes.c_void_p]


def parent_library(path):
    """the yardstick library and a nova_vesta context of its own -> (lib, ctx handle)"""
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    for name, args in (("b3w_bao_slice_ingest_have_device", ONE), ("b3w_bao_range_slice_ingest_device", RANGE), ("b3w_bao_set_slice_ingest_device", SET)):
        getattr(P, name).restype, getattr(P, name).argtypes = i32, args
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


# name -> (the runs, ascending; group_log; the slice kinds measured)
CASES = {"half_missing": (runs_half_missing, 0, ("set",)), "65536x1": (sorted_runs(lambda rng: runs_of(rng, 65536, 1)), 0, ("one", "set")),
         "4096x16": (sorted_runs(lambda rng: runs_of(rng, 4096, 16)), 0, ("range",)), "64x1024": (runs_64x1024, 0, ("range",)),
         "64x1024_g4": (runs_64x1024, 4, ("range",))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default="", help="libb3wit.so built from the parent commit: the yardstick")
    ap.add_argument("--cases", default="", help="comma-separated subset of the case names")
    ap.add_argument("--decode", action="store_true", help="also time the packed calls with null outboards")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    if a.parent_lib:
        Y, y_ctx = parent_library(a.parent_lib)
        yard = f"{os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff}), a build of the parent commit loaded beside this library"
    else:
        Y, y_ctx = L, ctx.handle
        yard = "this library's arena receivers"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_src = torch.empty(BM.GIB + 16, dtype=torch.uint8, device="cuda")
    d_src[:] = torch.randint(0, 256, (BM.GIB + 16,), dtype=torch.uint8, device="cuda", generator=gen)
    d_arena = torch.empty(BM.GIB + 16, dtype=torch.uint8, device="cuda")
    lens = np.array([BM.GIB], dtype=np.uint64)
    offs = np.zeros(1, dtype=np.uint64)
    res = dict(device=torch.cuda.get_device_name(0), file_bytes=BM.GIB, arena_bytes=int(d_arena.numel()), yardstick=yard, profiler="none was run", cases={})
    want = [x for x in a.cases.split(",") if x]
    provider = {}
    for name, (make, gl, kinds) in CASES.items():
        if want and name not in want:
            continue
        if gl not in provider:
            provider[gl] = m.bao.outboard_groups_batch(ctx, d_src, offs, lens, gl) if gl else m.bao.outboard_batch(ctx, d_src, offs, lens)
        prov = provider[gl]
        d_roots = prov["roots"]
        first, count = make(np.random.default_rng(20))
        k = int(first.size)
        files = np.zeros(k, dtype=np.uint32)
        c_files, chunks = m.bao.runs_chunks(files, first, count)
        n_chunks = int(chunks.size)
        ids = torch.from_numpy(chunks.astype(np.int64)).cuda()
        for kind in kinds:
            if kind == "one":
                made = m.bao.slices_arena(ctx, d_src, offs, lens, prov["outboards"], c_files, chunks, group_log=gl)
                lst, n_out = (c_files, chunks), n_chunks
            elif kind == "range":
                made = m.bao.range_slices_arena(ctx, d_src, offs, lens, prov["outboards"], files, first, count, group_log=gl)
                lst, n_out = (files, first, count), k
            else:
                made = m.bao.set_slices_arena(ctx, d_src, offs, lens, prov["outboards"], files, first, count, group_log=gl)
                lst, n_out = (files, first, count), 1
            d_slices = made["slices"]
            d_chunks = torch.empty(n_chunks * 1024, dtype=torch.uint8, device="cuda")
            obs = {r: torch.empty(m.bao.group_outboard_size(BM.GIB, gl), dtype=torch.uint8, device="cuda") for r in ("arena", "packed")}
            have = {r: m.bao.have_new(lens) for r in ("arena", "packed")}
            st = {r: torch.empty(n_out, dtype=torch.int32, device="cuda") for r in ("arena", "packed")}
            fb = {r: torch.empty(n_out, dtype=torch.int64, device="cuda") for r in ("arena", "packed")}
            cs = {r: torch.empty(n_chunks, dtype=torch.int32, device="cuda") for r in ("arena", "packed")}
            args = (lens.ctypes.data, 1, files.ctypes.data, first.ctypes.data, count.ctypes.data, k)
            need = 0 if kind == "one" else (L.b3w_bao_range_slice_ingest_scratch_bytes if kind == "range" else L.b3w_bao_set_slice_ingest_scratch_bytes)(*args)
            scratch = torch.empty(max(16, need), dtype=torch.uint8, device="cuda")
            ptrs = tuple(x.ctypes.data for x in lst) + (lst[0].size,)

            def tail(r):
                out = (d_slices.data_ptr(), st[r].data_ptr())
                if kind != "one":
                    out += (fb[r].data_ptr(),)
                if kind == "set":
                    out += (cs[r].data_ptr(),)
                out += (have[r].data_ptr(),)
                return out + ((scratch.data_ptr(), scratch.numel()) if kind != "one" else ()) + (s,)
            y_fn = getattr(Y, {"one": "b3w_bao_slice_ingest_have_device", "range": "b3w_bao_range_slice_ingest_device", "set": "b3w_bao_set_slice_ingest_device"}[kind])
            n_fn = getattr(L, {"one": "b3w_bao_slice_ingest_packed_device", "range": "b3w_bao_range_slice_ingest_packed_device",
                               "set": "b3w_bao_set_slice_ingest_packed_device"}[kind])

            def arena():
                assert y_fn(y_ctx, d_arena.data_ptr(), d_arena.numel(), offs.ctypes.data, lens.ctypes.data, 1, gl, obs["arena"].data_ptr(), d_roots.data_ptr(), *ptrs,
                            *tail("arena")) == 0

            def packed():
                assert n_fn(ctx.handle, d_chunks.data_ptr(), d_chunks.numel(), lens.ctypes.data, 1, gl, obs["packed"].data_ptr(), d_roots.data_ptr(), *ptrs,
                            *tail("packed")) == 0, ctx.last_error()

            def decode():
                assert n_fn(ctx.handle, d_chunks.data_ptr(), d_chunks.numel(), lens.ctypes.data, 1, gl, None, d_roots.data_ptr(), *ptrs, *tail("packed")) == 0, ctx.last_error()
            # the check: both routes from 0xEE; slot k is the arena's k-th listed chunk, which is the source's
            d_arena.fill_(FILL)
            d_chunks.fill_(FILL)
            for r in obs:
                obs[r].fill_(FILL)
                have[r].zero_()
            arena()
            packed()
            torch.cuda.synchronize()
            assert not st["arena"].any().item() and torch.equal(st["arena"], st["packed"]), (name, kind)
            if kind != "one":
                assert bool((fb["arena"] == -1).all().item()) and torch.equal(fb["arena"], fb["packed"]), (name, kind)
            if kind == "set":
                assert not cs["arena"].any().item() and torch.equal(cs["arena"], cs["packed"]), (name, kind)
            assert torch.equal(obs["arena"], obs["packed"]) and torch.equal(have["arena"], have["packed"]), (name, kind)
            assert torch.equal(d_chunks.view(n_chunks, 1024), d_arena[:BM.GIB].view(N, 1024)[ids]), f"{name} {kind}: a slot is not the arena's chunk"
            assert torch.equal(d_chunks.view(n_chunks, 1024), d_src[:BM.GIB].view(N, 1024)[ids]), f"{name} {kind}: a slot is not the source's chunk"
            assert int((d_arena[:BM.GIB].view(N, 1024) != FILL).any(dim=1).sum().item()) == n_chunks
            row = dict(kind=kind, runs=k, chunks=n_chunks, group_log=gl, slice_bytes=int(d_slices.numel()), slot_bytes=int(d_chunks.numel()),
                       arena_bytes=int(d_arena.numel()), device_memory_saved_bytes=int(d_arena.numel() - d_chunks.numel()), rows=need // 16, checked=True)
            for _ in range(3):
                arena()
                packed()
            routes = {"arena_a": arena, "new": packed, "arena_b": arena}
            if a.decode:
                routes["decode"] = decode
            t = alternating(routes)
            row["new"], row["arena"] = stats(t["new"]), stats(t["arena_a"] + t["arena_b"])
            row["arena_spread_ms"] = abs(stats(t["arena_a"])["ms"] - stats(t["arena_b"])["ms"])
            row["new_over_arena"] = row["new"]["ms"] / row["arena"]["ms"]
            diff = row["new"]["ms"] - row["arena"]["ms"]
            row["verdict"] = "within the yardstick's spread" if abs(diff) <= row["arena_spread_ms"] else "slower" if diff > 0 else "faster"
            if a.decode:
                row["decode"] = stats(t["decode"])
            res["cases"][f"{name}/{kind}"] = row
            print(name, kind, json.dumps(row), flush=True)
            del d_slices, made, d_chunks, obs, st, fb, cs, scratch
        del ids
    res["not_taken"] = "files past 1 GiB; many files a call; per-kernel times (no profiler was run); the host's table fill apart from the launches; the copy of the slots to the host"
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_receive_packed_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
