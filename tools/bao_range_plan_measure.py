#!/usr/bin/env python3
"""tools/bao_range_plan_measure.py <out_dir> [--parent-lib libb3wit.so] [--cases a,b,...] — step records planned from range slices
(b3w_sample_plan_range_slices_device) against the only way the library before it could plan the records of a run of chunks without an
outboard: one slice a chunk.

  yardstick   of the library given with --parent-lib (a build of the parent commit, loaded beside this one, a context of its own) or,
              without it, of this library: bao.runs_chunks (the rows broken into chunks on the host, inside the timed call) and
              b3w_bao_slice_arena_device — the slice extraction, timed on its own — then b3w_sample_plan_slices_device over those
              slices (the chunk list made beforehand): the planning, which is what the new call is held against.
  method      tools/bao_range_measure.py's: the routes alternating in one process, device events around each whole call (the host's table
              fill and upload included), medians over about a second a route, both routes' records and statuses compared before timing.
              The yardstick runs as two interleaved series A and B; |median A - median B| is the spread a difference has to exceed.
  cases       one 1 GiB file: 64 runs of 1 024 chunks at starts that are not tile-aligned, the same with the file at byte offset 1
              modulo 16, 4 096 runs of 16, 65 536 runs of 1, the 262 thousand runs of a bitmap with half its chunks missing.
  reported    per case the two extractions, the two plannings, new over yardstick, and the new call's rate against the bytes of records
              it writes.  No gate is fixed; `expectation` says whether the 64 x 1 024 planning lies below the yardstick's by more than
              its spread.
Writes <out_dir>/bao_range_plan_measure.json."""
import argparse, ctypes, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats
from bao_range_measure import N, runs_64x1024, runs_half_missing, runs_of

m = __import__("hot-proofs-blake3-circom_amd")


def parent_library(path):
    """the yardstick library and a nova_vesta context of its own -> (lib, ctx handle)"""
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    P.b3w_bao_slice_arena_device.restype, P.b3w_bao_slice_arena_device.argtypes = i32, [vp, vp, u64, vp, vp, u32, u32, vp, vp, vp, u32, vp, vp]
    P.b3w_sample_plan_slices_device.restype, P.b3w_sample_plan_slices_device.argtypes = i32, [vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp]
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


# name -> (the runs, the file's offset in the arena)
CASES = {"64x1024": (runs_64x1024, 0), "64x1024_offset1": (runs_64x1024, 1), "4096x16": (lambda rng: runs_of(rng, 4096, 16), 0),
         "65536x1": (lambda rng: runs_of(rng, 65536, 1), 0), "half_missing": (runs_half_missing, 0)}


def series(old, new):
    t = alternating({"yard_a": old, "new": new, "yard_b": old})
    r = dict(yardstick=stats(t["yard_a"] + t["yard_b"]), yardstick_a=stats(t["yard_a"]), yardstick_b=stats(t["yard_b"]), new=stats(t["new"]))
    r["yardstick_spread_ms"] = abs(r["yardstick_a"]["ms"] - r["yardstick_b"]["ms"])
    r["new_over_yardstick"] = r["new"]["ms"] / r["yardstick"]["ms"]
    r["new_below_yardstick_by_more_than_spread"] = bool(r["yardstick"]["ms"] - r["new"]["ms"] > r["yardstick_spread_ms"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default="", help="libb3wit.so built from the parent commit: the yardstick")
    ap.add_argument("--cases", default="", help="comma-separated subset of the case names")
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
    d_src = torch.randint(0, 256, (BM.GIB + 16,), dtype=torch.uint8, device="cuda", generator=gen)
    lens = np.array([BM.GIB], dtype=np.uint64)
    res = dict(device=torch.cuda.get_device_name(0), file_bytes=BM.GIB, yardstick=yard, cases={})
    want = [x for x in a.cases.split(",") if x]
    provider = {}
    for name, (make, offset) in CASES.items():
        if want and name not in want:
            continue
        offs = np.array([offset], dtype=np.uint64)
        if offset not in provider:
            provider[offset] = m.bao.outboard_batch(ctx, d_src, offs, lens)
        prov = provider[offset]
        d_roots = prov["roots"]
        first, count = make(np.random.default_rng(20))
        k = int(first.size)
        files = np.zeros(k, dtype=np.uint32)
        c_files, chunks = m.bao.runs_chunks(files, first, count)
        n_chunks = int(chunks.size)
        sf = m.bao.range_slice_layout(lens, files, first, count)
        y_sf = m.bao.slice_layout(lens, c_files, chunks)
        rrf = np.zeros(k + 1, dtype=np.uint64)
        rows = L.b3w_sample_rows_ranges(lens.ctypes.data, 1, files.ctypes.data, first.ctypes.data, count.ctypes.data, k, rrf.ctypes.data, None, None)
        assert rows == int(m.bao.sample_rows_batch(lens, c_files, chunks)[-1])
        d_slices = torch.empty(int(sf[-1]), dtype=torch.uint8, device="cuda")
        y_slices = torch.empty(int(y_sf[-1]), dtype=torch.uint8, device="cuda")
        d_recs = torch.full((rows, 32), -1, dtype=torch.int32, device="cuda")
        y_recs = torch.full((rows, 32), -2, dtype=torch.int32, device="cuda")
        d_cst = torch.full((n_chunks,), -1, dtype=torch.int32, device="cuda")
        y_cst = torch.full((n_chunks,), -1, dtype=torch.int32, device="cuda")
        d_st = torch.empty(k, dtype=torch.int32, device="cuda")
        d_fb = torch.empty(k, dtype=torch.int64, device="cuda")
        need = L.b3w_bao_range_slice_ingest_scratch_bytes(lens.ctypes.data, 1, files.ctypes.data, first.ctypes.data, count.ctypes.data, k)
        d_scratch = torch.empty(max(16, need), dtype=torch.uint8, device="cuda")

        def extract():
            rc = L.b3w_bao_range_slice_arena_device(ctx.handle, d_src.data_ptr(), d_src.numel(), offs.ctypes.data, lens.ctypes.data, 1, 0, prov["outboards"].data_ptr(),
                                                    files.ctypes.data, first.ctypes.data, count.ctypes.data, k, d_slices.data_ptr(), s)
            assert rc == 0, ctx.last_error()

        def extract_yard():
            fi, ch = m.bao.runs_chunks(files, first, count)
            rc = Y.b3w_bao_slice_arena_device(y_ctx, d_src.data_ptr(), d_src.numel(), offs.ctypes.data, lens.ctypes.data, 1, 0, prov["outboards"].data_ptr(),
                                              fi.ctypes.data, ch.ctypes.data, ch.size, y_slices.data_ptr(), s)
            assert rc == 0, rc

        def plan():
            rc = L.b3w_sample_plan_range_slices_device(ctx.handle, lens.ctypes.data, 1, d_roots.data_ptr(), files.ctypes.data, first.ctypes.data, count.ctypes.data, k,
                                                       d_slices.data_ptr(), d_recs.data_ptr(), d_cst.data_ptr(), d_st.data_ptr(), d_fb.data_ptr(),
                                                       d_scratch.data_ptr(), d_scratch.numel(), s)
            assert rc == 0, ctx.last_error()

        def plan_yard():
            rc = Y.b3w_sample_plan_slices_device(y_ctx, lens.ctypes.data, 1, d_roots.data_ptr(), c_files.ctypes.data, chunks.ctypes.data, n_chunks,
                                                 y_slices.data_ptr(), y_recs.data_ptr(), y_cst.data_ptr(), s)
            assert rc == 0, rc
        # the check: both routes' records and statuses are the same words
        extract()
        extract_yard()
        plan()
        plan_yard()
        torch.cuda.synchronize()
        assert not d_cst.any().item() and not y_cst.any().item() and not d_st.any().item() and bool((d_fb == -1).all().item()), name
        assert torch.equal(d_recs, y_recs), f"{name}: the two routes' records differ"
        row = dict(runs=k, chunks=n_chunks, file_offset=offset, rows=int(rows), record_bytes=int(rows) * 128, range_slice_bytes=int(sf[-1]),
                   one_chunk_slice_bytes=int(y_sf[-1]), checked=True)
        for _ in range(3):
            extract_yard(); extract(); plan_yard(); plan()
        row["extraction"] = series(extract_yard, extract)
        row["planning"] = series(plan_yard, plan)
        row["new_planning_record_gb_per_s"] = row["record_bytes"] / row["planning"]["new"]["ms"] / 1e6
        row["yardstick_planning_record_gb_per_s"] = row["record_bytes"] / row["planning"]["yardstick"]["ms"] / 1e6
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del d_slices, y_slices, d_recs, y_recs, d_cst, y_cst, d_st, d_fb, d_scratch
    g = res["cases"].get("64x1024")
    if g:
        p = g["planning"]
        res["expectation"] = dict(case="64x1024", met=p["new_below_yardstick_by_more_than_spread"], yardstick_ms=p["yardstick"]["ms"], new_ms=p["new"]["ms"],
                                  spread_ms=p["yardstick_spread_ms"])
    res["not_taken"] = "files past 1 GiB; per-kernel times; the run length at which the two routes cross; cooperative 16-byte stores of the rows"
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_range_plan_measure.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
