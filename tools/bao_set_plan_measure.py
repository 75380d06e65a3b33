#!/usr/bin/env python3
"""tools/bao_set_plan_measure.py <out_dir> [--parent-lib libb3wit.so] [--cases a,b,...] — the set planner
(b3w_sample_plan_set_slices_device) against the two ways the library before it plans the step records of the same chunks, and the set
provider from packed bytes (b3w_bao_set_slice_packed_device) against the arena provider over the resident file.

  yardsticks  of the library given with --parent-lib (or the environment's B3WIT_PARENT_LIB: a build of the parent commit, loaded beside
              this one, a context of its own) or, without it, of this library.  For the planner: RANGE, b3w_sample_plan_range_slices_device
              over range slices of the same list, and ONE-CHUNK, bao.runs_chunks inside the timed call plus b3w_sample_plan_slices_device
              over one-chunk slices of the same chunks.  For the packed provider: b3w_bao_set_slice_arena_device.
  method      tools/bao_set_measure.py's: the routes alternating in one process, device events around each whole C call (the host's
              table fill and upload included), medians over about a second a route, the routes' outputs compared before timing (the
              three planners' records and statuses word for word, the two providers' slices byte for byte).  Each yardstick runs as two
              interleaved series A and B; |median A - median B| is the spread a difference has to exceed.
  cases       one 1 GiB file: the runs of a bitmap with half its chunks missing (262 507 runs), 65 536 runs of 1 chunk, 4 096 runs of
              16, 64 runs of 1 024 chunks at starts that are not tile-aligned, and the last again at g = 4 (the planner reads no
              outboard: g only moves the packed provider and its layout).
  expectation on the half-missing shape and on 65 536 runs of one chunk the set planner beats the FASTER of its two yardsticks by more
              than that yardstick's spread; recorded as met or not.  No speed-up is expected of the packed provider: how far behind the
              arena call it lies is recorded.  No profiler is run.
Writes <out_dir>/bao_set_plan_measure.json."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats
from bao_set_measure import CASES, parent_library

m = __import__("hot-proofs-blake3-circom_amd")


def yardstick_library(path):
    """bao_set_measure's parent library with the planners' and the set provider's signatures"""
    import ctypes
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
    P, h = parent_library(path)
    P.b3w_sample_plan_slices_device.restype, P.b3w_sample_plan_slices_device.argtypes = i32, [vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp]
    P.b3w_sample_plan_range_slices_device.restype = i32
    P.b3w_sample_plan_range_slices_device.argtypes = [vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, u64, vp]
    P.b3w_bao_set_slice_arena_device.restype, P.b3w_bao_set_slice_arena_device.argtypes = i32, [vp, vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, u32, vp, vp]
    return P, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default=os.environ.get("B3WIT_PARENT_LIB", ""), help="libb3wit.so built from the parent commit: the yardstick")
    ap.add_argument("--cases", default="", help="comma-separated subset of the case names")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    if a.parent_lib:
        Y, y_ctx = yardstick_library(a.parent_lib)
        yard = f"{os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff}), a build of the parent commit loaded beside this library"
    else:
        Y, y_ctx = L, ctx.handle
        yard = "this library's range, one-chunk and arena calls"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_src = torch.empty(BM.GIB + 16, dtype=torch.uint8, device="cuda")
    d_src[:] = torch.randint(0, 256, (BM.GIB + 16,), dtype=torch.uint8, device="cuda", generator=gen)
    lens = np.array([BM.GIB], dtype=np.uint64)
    offs = np.zeros(1, dtype=np.uint64)
    res = dict(device=torch.cuda.get_device_name(0), file_bytes=BM.GIB, yardstick=yard, profiler="none was run", cases={})
    want = [x for x in a.cases.split(",") if x]
    provider = {}
    for name, (make, gl) in CASES.items():
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
        lists = (files.ctypes.data, first.ctypes.data, count.ctypes.data, k)
        # the three kinds of slices of the same chunks, each from its own provider
        sl = dict(set=m.bao.set_slices_arena(ctx, d_src, offs, lens, prov["outboards"], files, first, count, group_log=gl)["slices"],
                  range=m.bao.range_slices_arena(ctx, d_src, offs, lens, prov["outboards"], files, first, count, group_log=gl)["slices"],
                  one=m.bao.slices_arena(ctx, d_src, offs, lens, prov["outboards"], c_files, chunks, group_log=gl)["slices"])
        rrf, _, _ = m.bao.sample_rows_ranges(lens, files, first, count)
        rows = int(rrf[-1])
        recs = {r: torch.empty((rows, 32), dtype=torch.int32, device="cuda") for r in sl}
        st = {r: torch.empty(n_chunks, dtype=torch.int32, device="cuda") for r in sl}
        agg = {"set": (torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")),
               "range": (torch.empty(k, dtype=torch.int32, device="cuda"), torch.empty(k, dtype=torch.int64, device="cuda"))}
        need = {"set": L.b3w_bao_set_slice_ingest_scratch_bytes(lens.ctypes.data, 1, *lists), "range": L.b3w_bao_range_slice_ingest_scratch_bytes(lens.ctypes.data, 1, *lists)}
        scratch = {r: torch.empty(max(16, b), dtype=torch.uint8, device="cuda") for r, b in need.items()}

        def plan_set():
            assert L.b3w_sample_plan_set_slices_device(ctx.handle, lens.ctypes.data, 1, d_roots.data_ptr(), *lists, sl["set"].data_ptr(), recs["set"].data_ptr(),
                                                       st["set"].data_ptr(), agg["set"][0].data_ptr(), agg["set"][1].data_ptr(), scratch["set"].data_ptr(),
                                                       scratch["set"].numel(), s) == 0, ctx.last_error()

        def plan_range():
            assert Y.b3w_sample_plan_range_slices_device(y_ctx, lens.ctypes.data, 1, d_roots.data_ptr(), *lists, sl["range"].data_ptr(), recs["range"].data_ptr(),
                                                         st["range"].data_ptr(), agg["range"][0].data_ptr(), agg["range"][1].data_ptr(), scratch["range"].data_ptr(),
                                                         scratch["range"].numel(), s) == 0

        def plan_one():
            fi, ch = m.bao.runs_chunks(files, first, count)
            assert Y.b3w_sample_plan_slices_device(y_ctx, lens.ctypes.data, 1, d_roots.data_ptr(), fi.ctypes.data, ch.ctypes.data, ch.size, sl["one"].data_ptr(),
                                                   recs["one"].data_ptr(), st["one"].data_ptr(), s) == 0
        # the packed provider and its yardstick: the parent's arena provider over the resident file
        lay = m.bao.packed_layout(lens, files, first, count, gl)
        d_packed = m.bao.pack_ranges(d_src, offs, lens, files, first, count, gl).view(-1)
        out = {r: torch.empty_like(sl["set"]) for r in ("packed", "arena")}

        def provide_packed():
            assert L.b3w_bao_set_slice_packed_device(ctx.handle, d_packed.data_ptr(), d_packed.numel(), lens.ctypes.data, 1, gl, prov["outboards"].data_ptr(), *lists,
                                                     out["packed"].data_ptr(), s) == 0, ctx.last_error()

        def provide_arena():
            assert Y.b3w_bao_set_slice_arena_device(y_ctx, d_src.data_ptr(), d_src.numel(), offs.ctypes.data, lens.ctypes.data, 1, gl, prov["outboards"].data_ptr(), *lists,
                                                    out["arena"].data_ptr(), s) == 0
        # the check: the three planners' records and statuses word for word; the two providers' slices byte for byte
        for r in recs:
            recs[r].fill_(-1)
            st[r].fill_(-1)
        for r in out:
            out[r].zero_()
        for fn in (plan_set, plan_range, plan_one, provide_packed, provide_arena):
            fn()
        torch.cuda.synchronize()
        assert not any(t.any().item() for t in st.values()) and not any(x[0].any().item() for x in agg.values()), name
        for r in ("range", "one"):
            assert torch.equal(recs["set"], recs[r]), f"{name}: the set planner's records and the {r} planner's differ"
        assert torch.equal(out["packed"], out["arena"]) and torch.equal(out["arena"], sl["set"]), f"{name}: the packed provider's slices differ"
        row = dict(runs=k, chunks=n_chunks, group_log=gl, record_rows=rows, record_bytes=rows * 128, set_slice_bytes=int(sl["set"].numel()),
                   range_slice_bytes=int(sl["range"].numel()), one_chunk_slice_bytes=int(sl["one"].numel()), set_rows=need["set"] // 16, range_rows=need["range"] // 16,
                   packed_slots=int(lay["total_slots"]), packed_bytes=int(lay["total_bytes"]), checked=True)
        for _ in range(3):
            for fn in (plan_range, plan_one, plan_set, provide_arena, provide_packed):
                fn()
        t = alternating({"range_a": plan_range, "one_a": plan_one, "new": plan_set, "range_b": plan_range, "one_b": plan_one})
        r = dict(new=stats(t["new"]))
        for y in ("range", "one"):
            r[y] = stats(t[y + "_a"] + t[y + "_b"])
            r[y + "_spread_ms"] = abs(stats(t[y + "_a"])["ms"] - stats(t[y + "_b"])["ms"])
            r["new_over_" + y] = r["new"]["ms"] / r[y]["ms"]
        best = min(("range", "one"), key=lambda y: r[y]["ms"])
        r["faster_yardstick"] = best
        r["new_below_faster_yardstick_by_more_than_its_spread"] = bool(r[best]["ms"] - r["new"]["ms"] > r[best + "_spread_ms"])
        row["planner"] = r
        t = alternating({"arena_a": provide_arena, "new": provide_packed, "arena_b": provide_arena})
        p = dict(new=stats(t["new"]), arena=stats(t["arena_a"] + t["arena_b"]))
        p["arena_spread_ms"] = abs(stats(t["arena_a"])["ms"] - stats(t["arena_b"])["ms"])
        p["new_over_arena"] = p["new"]["ms"] / p["arena"]["ms"]
        p["new_behind_arena_ms"] = p["new"]["ms"] - p["arena"]["ms"]
        row["packed_provider"] = p
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del sl, recs, st, agg, scratch, out, d_packed
    met = {}
    for name in ("half_missing", "65536x1"):
        c = res["cases"].get(name)
        if c:
            r = c["planner"]
            met[name] = dict(met=r["new_below_faster_yardstick_by_more_than_its_spread"], new_ms=r["new"]["ms"], range_ms=r["range"]["ms"], one_ms=r["one"]["ms"],
                             range_spread_ms=r["range_spread_ms"], one_spread_ms=r["one_spread_ms"], faster_yardstick=r["faster_yardstick"])
    if met:
        res["expectation"] = dict(what="the set planner beats the faster of its two yardsticks by more than that yardstick's spread", cases=met,
                                  met=all(v["met"] for v in met.values()))
    res["not_taken"] = ("files past 1 GiB; many files a call; per-kernel times (no profiler was run); the host's table fill apart from the launches; the gather into "
                        "the packed buffer (bao.pack_ranges), which a provider with the file on disk does while it reads")
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_set_plan_measure.json"), "w"), indent=1)
    print(json.dumps(res.get("expectation"), indent=1))


if __name__ == "__main__":
    main()
