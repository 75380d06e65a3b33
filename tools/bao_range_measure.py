#!/usr/bin/env python3
"""tools/bao_range_measure.py <out_dir> [--parent-lib libb3wit.so] [--cases a,b,...] — range slices (b3w_bao_range_slice_arena_device,
b3w_bao_range_slice_ingest_device) against the only way the library before them could serve and take in a run of chunks: one slice a chunk.

  yardstick   of the library given with --parent-lib (a build of the parent commit, loaded beside this one, a context of its own) or,
              without it, of this library: the provider is bao.runs_chunks (the rows broken into chunks on the host, which that route
              needs and which is inside the timed call) and b3w_bao_slice_arena_device; the receiver is b3w_bao_slice_ingest_have_device
              over the same chunks (the chunk list made beforehand).
  method      tools/bao_ingest_measure.py's: the routes alternating in one process, device events around each whole call (the host's table
              fill and upload included), medians over about a second a route, both routes' results compared before timing.  The yardstick
              runs as two interleaved series A and B; |median A - median B| is the spread a difference has to exceed to mean anything.
  cases       one 1 GiB file.  gate: 64 runs of 1 024 chunks at starts that are not tile-aligned (65 536 chunks), the file at a 16-byte
              aligned offset, g = 0.  Recorded: 65 536 runs of 1 chunk (equal bytes: the "when not to"), 4 096 runs of 16, the 262 thousand
              runs of a bitmap with half its chunks missing, the gate's shape at g = 4 and with the file at 1 modulo 16, and one range
              that is the whole file against bao.verify_batch plus a device copy of the bytes.
  gate        both new calls' medians lie below their yardstick's medians by more than the yardstick's spread.
Writes <out_dir>/bao_range_measure.json."""
import argparse, ctypes, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats

m = __import__("hot-proofs-blake3-circom_amd")

FILL = 0xEE
N = BM.GIB // 1024


def parent_library(path):
    """the yardstick library and a nova_vesta context of its own -> (lib, ctx handle)"""
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    P.b3w_bao_slice_arena_device.restype, P.b3w_bao_slice_arena_device.argtypes = i32, [vp, vp, u64, vp, vp, u32, u32, vp, vp, vp, u32, vp, vp]
    P.b3w_bao_slice_ingest_have_device.restype = i32
    P.b3w_bao_slice_ingest_have_device.argtypes = [vp, vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


def runs_64x1024(rng):
    slots = np.sort(rng.permutation(N // 2048)[:64])
    first = slots * 2048 + rng.integers(1, 1024, 64)                       # not tile-aligned, disjoint
    return first.astype(np.uint64), np.full(64, 1024, dtype=np.uint64)


def runs_of(rng, count, length):
    slots = rng.permutation(N // length)[:count]
    return (slots * length).astype(np.uint64), np.full(count, length, dtype=np.uint64)


def runs_half_missing(rng):
    missing = rng.random(N) < 0.5
    edge = np.diff(np.concatenate([[0], missing.astype(np.int8), [0]]))
    first, end = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    return first.astype(np.uint64), (end - first).astype(np.uint64)


# name -> (the runs, the file's offset in both arenas, group_log)
CASES = {"64x1024": (runs_64x1024, 0, 0), "65536x1": (lambda rng: runs_of(rng, 65536, 1), 0, 0), "4096x16": (lambda rng: runs_of(rng, 4096, 16), 0, 0),
         "half_missing": (runs_half_missing, 0, 0), "64x1024_g4": (runs_64x1024, 0, 4), "64x1024_offset1": (runs_64x1024, 1, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default="", help="libb3wit.so built from the parent commit: the yardstick")
    ap.add_argument("--cases", default="", help="comma-separated subset of the case names (whole_file among them)")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    if a.parent_lib:
        Y, y_ctx = parent_library(a.parent_lib)
        yard = f"{os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff}), a build of the parent commit loaded beside this library"
    else:
        Y, y_ctx = L, ctx.handle
        yard = "this library's one-chunk calls"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_src = torch.empty(BM.GIB + 16, dtype=torch.uint8, device="cuda")
    d_src[:] = torch.randint(0, 256, (BM.GIB + 16,), dtype=torch.uint8, device="cuda", generator=gen)
    d_dst = torch.empty(BM.GIB + 16, dtype=torch.uint8, device="cuda")
    y_dst = torch.empty(BM.GIB + 16, dtype=torch.uint8, device="cuda")
    lens = np.array([BM.GIB], dtype=np.uint64)
    res = dict(device=torch.cuda.get_device_name(0), file_bytes=BM.GIB, yardstick=yard, cases={})
    want = [x for x in a.cases.split(",") if x]
    provider = {}
    for name, (make, offset, gl) in CASES.items():
        if want and name not in want:
            continue
        offs = np.array([offset], dtype=np.uint64)
        if (offset, gl) not in provider:
            provider[(offset, gl)] = m.bao.outboard_groups_batch(ctx, d_src, offs, lens, gl) if gl else m.bao.outboard_batch(ctx, d_src, offs, lens)
        prov = provider[(offset, gl)]
        d_roots = prov["roots"]
        first, count = make(np.random.default_rng(20))
        k = int(first.size)
        files = np.zeros(k, dtype=np.uint32)
        c_files, chunks = m.bao.runs_chunks(files, first, count)
        n_chunks = int(chunks.size)
        sf = m.bao.range_slice_layout(lens, files, first, count)
        y_sf = m.bao.slice_layout(lens, c_files, chunks)
        d_slices = torch.empty(int(sf[-1]), dtype=torch.uint8, device="cuda")
        y_slices = torch.empty(int(y_sf[-1]), dtype=torch.uint8, device="cuda")
        d_obs = torch.empty(m.bao.group_outboard_size(BM.GIB, gl), dtype=torch.uint8, device="cuda")
        y_obs = torch.empty_like(d_obs)
        d_have, y_have = m.bao.have_new(lens), m.bao.have_new(lens)
        d_st = torch.empty(k, dtype=torch.int32, device="cuda")
        d_fb = torch.empty(k, dtype=torch.int64, device="cuda")
        y_st = torch.empty(n_chunks, dtype=torch.int32, device="cuda")
        need = L.b3w_bao_range_slice_ingest_scratch_bytes(lens.ctypes.data, 1, files.ctypes.data, first.ctypes.data, count.ctypes.data, k)
        d_scratch = torch.empty(max(16, need), dtype=torch.uint8, device="cuda")

        def provide():
            rc = L.b3w_bao_range_slice_arena_device(ctx.handle, d_src.data_ptr(), d_src.numel(), offs.ctypes.data, lens.ctypes.data, 1, gl, prov["outboards"].data_ptr(),
                                                    files.ctypes.data, first.ctypes.data, count.ctypes.data, k, d_slices.data_ptr(), s)
            assert rc == 0, ctx.last_error()

        def provide_yard():
            fi, ch = m.bao.runs_chunks(files, first, count)
            rc = Y.b3w_bao_slice_arena_device(y_ctx, d_src.data_ptr(), d_src.numel(), offs.ctypes.data, lens.ctypes.data, 1, gl, prov["outboards"].data_ptr(),
                                              fi.ctypes.data, ch.ctypes.data, ch.size, y_slices.data_ptr(), s)
            assert rc == 0, rc

        def ingest():
            rc = L.b3w_bao_range_slice_ingest_device(ctx.handle, d_dst.data_ptr(), d_dst.numel(), offs.ctypes.data, lens.ctypes.data, 1, gl, d_obs.data_ptr(),
                                                     d_roots.data_ptr(), files.ctypes.data, first.ctypes.data, count.ctypes.data, k, d_slices.data_ptr(),
                                                     d_st.data_ptr(), d_fb.data_ptr(), d_have.data_ptr(), d_scratch.data_ptr(), d_scratch.numel(), s)
            assert rc == 0, ctx.last_error()

        def ingest_yard():
            rc = Y.b3w_bao_slice_ingest_have_device(y_ctx, y_dst.data_ptr(), y_dst.numel(), offs.ctypes.data, lens.ctypes.data, 1, gl, y_obs.data_ptr(),
                                                    d_roots.data_ptr(), c_files.ctypes.data, chunks.ctypes.data, n_chunks, y_slices.data_ptr(), y_st.data_ptr(),
                                                    y_have.data_ptr(), s)
            assert rc == 0, rc
        # the check: both routes into buffers of 0xEE give the same arena, outboard and bitmap; the chunks are the source's
        for t in (d_dst, y_dst, d_obs, y_obs):
            t.fill_(FILL)
        d_have.zero_()
        y_have.zero_()
        provide()
        provide_yard()
        ingest()
        ingest_yard()
        torch.cuda.synchronize()
        assert not d_st.any().item() and not y_st.any().item() and bool((d_fb == -1).all().item()), name
        assert torch.equal(d_dst, y_dst) and torch.equal(d_obs, y_obs) and torch.equal(d_have, y_have), f"{name}: the two routes differ"
        ids = torch.from_numpy(chunks.astype(np.int64)).cuda()
        assert torch.equal(d_dst[offset:offset + BM.GIB].view(N, 1024)[ids], d_src[offset:offset + BM.GIB].view(N, 1024)[ids]), name
        assert int((d_dst[offset:offset + BM.GIB].view(N, 1024) != FILL).any(dim=1).sum().item()) == n_chunks
        expand = []
        for _ in range(9):
            t0 = time.perf_counter()
            m.bao.runs_chunks(files, first, count)
            expand.append((time.perf_counter() - t0) * 1e3)
        row = dict(runs=k, chunks=n_chunks, file_offset=offset, group_log=gl, range_slice_bytes=int(sf[-1]), one_chunk_slice_bytes=int(y_sf[-1]),
                   payload_bytes=n_chunks * 1024, runs_chunks_host_ms=float(np.median(expand)), checked=True)
        for _ in range(3):
            provide_yard(); provide(); ingest_yard(); ingest()
        for what, new, old in (("provider", provide, provide_yard), ("receiver", ingest, ingest_yard)):
            t = alternating({"yard_a": old, "new": new, "yard_b": old})
            r = dict(yardstick=stats(t["yard_a"] + t["yard_b"]), yardstick_a=stats(t["yard_a"]), yardstick_b=stats(t["yard_b"]), new=stats(t["new"]))
            r["yardstick_spread_ms"] = abs(r["yardstick_a"]["ms"] - r["yardstick_b"]["ms"])
            r["new_over_yardstick"] = r["new"]["ms"] / r["yardstick"]["ms"]
            r["new_below_yardstick_by_more_than_spread"] = bool(r["yardstick"]["ms"] - r["new"]["ms"] > r["yardstick_spread_ms"])
            row[what] = r
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del d_slices, y_slices, d_obs, y_obs, ids, d_st, d_fb, y_st, d_scratch
    if not want or "whole_file" in want:                                   # one range = the whole file, against verifying it where it lies plus a copy
        offs = np.zeros(1, dtype=np.uint64)
        if (0, 0) not in provider:
            provider[(0, 0)] = m.bao.outboard_batch(ctx, d_src, offs, lens)
        prov = provider[(0, 0)]
        files, first, count = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64), np.array([N], dtype=np.uint64)
        out = m.bao.range_slices_arena(ctx, d_src, offs, lens, prov["outboards"], files, first, count)
        d_obs = torch.full((m.bao.outboard_size(BM.GIB),), FILL, dtype=torch.uint8, device="cuda")
        d_dst.fill_(FILL)

        def whole_range():
            return m.bao.ingest_range_slices(ctx, d_dst, offs, lens, d_obs, prov["roots"], files, first, count, out["slices"])

        def provide_whole():
            m.bao.range_slices_arena(ctx, d_src, offs, lens, prov["outboards"], files, first, count)

        def verify_and_copy():
            m.bao.verify_batch(ctx, d_src, offs, lens, prov["outboards"], prov["roots"])
            y_dst[:BM.GIB].copy_(d_src[:BM.GIB])
        st = whole_range()
        torch.cuda.synchronize()
        assert st["range_status"].cpu().tolist() == [0] and torch.equal(d_dst[:BM.GIB], d_src[:BM.GIB]) and torch.equal(d_obs, prov["outboards"][:d_obs.numel()])
        for fn in (whole_range, provide_whole, verify_and_copy):
            for _ in range(3):
                fn()
        t = alternating({"ingest_range_slices": whole_range, "range_slices_arena": provide_whole, "verify_batch_and_copy": verify_and_copy})
        row = dict(note="the Python calls, their output buffers allocated inside the timed call", range_slice_bytes=int(out["slice_first"][-1]),
                   **{k: stats(v) for k, v in t.items()})
        res["cases"]["whole_file"] = row
        print("whole_file", json.dumps(row), flush=True)
    g = res["cases"].get("64x1024")
    if g:
        res["gate"] = dict(case="64x1024", passed=bool(g["provider"]["new_below_yardstick_by_more_than_spread"] and g["receiver"]["new_below_yardstick_by_more_than_spread"]),
                           provider=dict(yardstick_ms=g["provider"]["yardstick"]["ms"], new_ms=g["provider"]["new"]["ms"], spread_ms=g["provider"]["yardstick_spread_ms"]),
                           receiver=dict(yardstick_ms=g["receiver"]["yardstick"]["ms"], new_ms=g["receiver"]["new"]["ms"], spread_ms=g["receiver"]["yardstick_spread_ms"]))
    res["not_taken"] = "files past 1 GiB; per-kernel times; the run length at which the two routes cross (between 1 and 16 chunks a run)"
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_range_measure.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
