#!/usr/bin/env python3
"""tools/bao_slices_measure.py <out_dir> [--parent-lib libb3wit.so] [--quick] — bao slices on the device: extraction, and planning
from slices against the planner that reads full outboards.

4 096 samples over the 16 384 x 64 KiB batch and over the 1 x 1 GiB file (tools/bao_batch_measure.py's shapes):
  planning    b3w_sample_plan_slices_device on extracted slices against the yardstick, b3w_sample_plan_batch_device on full
              outboards and chunk bytes, same samples: of the library given with --parent-lib (a build of the commit before slices,
              loaded beside this one; its own context) or, without it, of this library.  Alternating in the same process, device
              events around each whole call (the host's table fill and upload included), medians over about a second a route.  The
              yardstick is measured as two interleaved series A and B; |median A - median B| is the spread a difference has to
              exceed to mean anything.  Beside the default route (16 lanes a sample, the running-h chain only where it is needed)
              the measurement switches' routes: 16 and 4 lanes with the chain for every sample, and one lane a sample with the
              chain, which is the lane-per-sample fall-back (sample_plan_one's work on a slice).  Records of all routes compared
              with the yardstick's once before timing.
  extraction  b3w_bao_slice_batch_device at group_log 0, 4 and 6, ms a call (no yardstick exists: the host helper does one chunk).
Writes <out_dir>/bao_slices_measure.json.  --quick: ten calls a route and shape, no timing — for a run under `rocprofv3
--kernel-trace --stats`, whose per-kernel call counts divided by ten are the launches of one call."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, parent_library, stats

m = __import__("hot-proofs-blake3-circom_amd")

QUICK_CALLS = 10
SAMPLES = 4096
ROUTES = {"slices": {}, "slices_16_chain": {"B3W_SLICE_PLAN_CHAIN": "1"}, "slices_4_chain": {"B3W_SLICE_PLAN_LANES": "4", "B3W_SLICE_PLAN_CHAIN": "1"},
          "slices_4": {"B3W_SLICE_PLAN_LANES": "4"}, "slices_1_chain": {"B3W_SLICE_PLAN_LANES": "1", "B3W_SLICE_PLAN_CHAIN": "1"}}


def with_env(env, fn):
    def run():
        for k in ("B3W_SLICE_PLAN_LANES", "B3W_SLICE_PLAN_CHAIN"):
            os.environ.pop(k, None)
        os.environ.update(env)
        fn()
        for k in env:
            os.environ.pop(k, None)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default="", help="libb3wit.so built from the commit before slices: the yardstick")
    ap.add_argument("--quick", action="store_true", help="ten calls a route and shape (under a profiler)")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    if a.parent_lib:
        Y, y_ctx = parent_library(a.parent_lib)
        yard = f"b3w_sample_plan_batch_device of {os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff})"
    else:
        Y, y_ctx = L, ctx.handle
        yard = "b3w_sample_plan_batch_device of this library"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_arena = torch.randint(0, 256, (BM.GIB + (1 << 20),), dtype=torch.uint8, device="cuda", generator=gen)
    res = dict(device=torch.cuda.get_device_name(0), samples=SAMPLES, yardstick=yard, planning={}, extraction={})
    rng = np.random.default_rng(7)
    all_shapes = BM.shapes()
    for name in ("16384x64KiB", "1x1GiB"):
        lens = np.array(all_shapes[name], dtype=np.uint64)
        offsets = (np.arange(lens.size, dtype=np.uint64) * np.uint64(int(lens[0]))).astype(np.uint64)      # back to back, 16-byte aligned starts
        files = rng.integers(0, lens.size, SAMPLES).astype(np.uint32)
        chunks = np.array([rng.integers(0, m.bao.num_chunks(int(lens[f]))) for f in files], dtype=np.uint64)
        full = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
        cb = m.bao.chunk_bytes_batch(d_arena, offsets, lens, files, chunks)
        rf = m.bao.sample_rows_batch(lens, files, chunks)
        sf = m.bao.slice_layout(lens, files, chunks)
        d_slices = torch.zeros(int(sf[-1]), dtype=torch.uint8, device="cuda")
        d_recs_y = torch.empty((int(rf[-1]), 32), dtype=torch.int32, device="cuda")
        d_recs_s = torch.empty_like(d_recs_y)
        d_st = torch.full((SAMPLES,), -1, dtype=torch.int32, device="cuda")

        def extract(g, obs, d_bytes, out=d_slices):
            rc = L.b3w_bao_slice_batch_device(ctx.handle, lens.ctypes.data, lens.size, g, obs.data_ptr(), files.ctypes.data, chunks.ctypes.data, SAMPLES,
                                              d_bytes.data_ptr(), out.data_ptr(), s)
            assert rc == 0, ctx.last_error()

        def plan_full():
            rc = Y.b3w_sample_plan_batch_device(y_ctx, lens.ctypes.data, lens.size, full["outboards"].data_ptr(), full["roots"].data_ptr(), files.ctypes.data,
                                                chunks.ctypes.data, SAMPLES, cb.data_ptr(), d_recs_y.data_ptr(), d_st.data_ptr(), s)
            assert rc == 0, rc

        def plan_slices():
            rc = L.b3w_sample_plan_slices_device(ctx.handle, lens.ctypes.data, lens.size, full["roots"].data_ptr(), files.ctypes.data, chunks.ctypes.data,
                                                 SAMPLES, d_slices.data_ptr(), d_recs_s.data_ptr(), d_st.data_ptr(), s)
            assert rc == 0, ctx.last_error()
        # extraction: g = 0 fills d_slices for the planner; g = 4, 6 into a second buffer that must come out the same
        ex_row = dict(samples=SAMPLES, slice_bytes=int(sf[-1]))
        extract(0, full["outboards"], cb)
        routes_x = {"g0": lambda: extract(0, full["outboards"], cb)}
        keep = []
        for g in (4, 6):
            grp = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
            gb = m.bao.group_bytes_batch(d_arena, offsets, lens, files, chunks, g)
            other = torch.zeros_like(d_slices)
            extract(g, grp["outboards"], gb, other)
            torch.cuda.synchronize()
            assert torch.equal(other, d_slices), f"{name} g = {g}: the slices from the group outboards differ"
            keep.append((grp, gb, other))
            routes_x[f"g{g}"] = (lambda g=g, grp=grp, gb=gb, other=other: extract(g, grp["outboards"], gb, other))
            ex_row[f"g{g}_bytes_in"] = int(gb.numel()) + int(grp["outboards"].numel())
        if a.quick:
            for fn in routes_x.values():
                for _ in range(QUICK_CALLS):
                    fn()
                torch.cuda.synchronize()
            ex_row["calls_each"] = QUICK_CALLS
        else:
            t = alternating(routes_x)
            ex_row.update({k: stats(v) for k, v in t.items()})
        res["extraction"][name] = ex_row
        print("extraction", name, json.dumps(ex_row), flush=True)
        del keep, routes_x
        # planning
        routes = {k: with_env(env, plan_slices) for k, env in ROUTES.items()}
        plan_full()
        torch.cuda.synchronize()
        if a.quick:                                                          # (under a profiler: the default route alone)
            routes = {"slices": routes["slices"]}
        for k, fn in routes.items():
            d_recs_s.zero_()
            fn()
            torch.cuda.synchronize()
            assert bool((d_st == 0).all().item()) and torch.equal(d_recs_y, d_recs_s), f"{name} {k}: the records differ from the yardstick's"
        row = dict(samples=SAMPLES, rows=int(rf[-1]), slice_bytes=int(sf[-1]), chunk_bytes=int(cb.numel()), full_outboard_bytes=int(full["outboards"].numel()),
                   records_equal=True)
        if a.quick:
            for fn in [plan_full] + list(routes.values()):
                for _ in range(QUICK_CALLS):
                    fn()
                torch.cuda.synchronize()
            row["calls_each"] = QUICK_CALLS
        else:
            t = alternating({"full_a": plan_full, **routes, "full_b": plan_full}, window_s=1.0)
            row.update(full=stats(t["full_a"] + t["full_b"]), full_a=stats(t["full_a"]), full_b=stats(t["full_b"]))
            row["yardstick_spread_ms"] = abs(row["full_a"]["ms"] - row["full_b"]["ms"])
            for k in routes:
                row[k] = stats(t[k])
                row[k + "_over_full"] = row[k]["ms"] / row["full"]["ms"]
            row["slices_minus_full_ms"] = row["slices"]["ms"] - row["full"]["ms"]
        res["planning"][name] = row
        print("planning", name, json.dumps(row), flush=True)
        del full, cb, d_slices, d_recs_y, d_recs_s
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_slices_measure.json" if not a.quick else "bao_slices_measure_quick.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
