#!/usr/bin/env python3
"""tools/bao_packed_measure.py <out_dir> [--cases a,b,...] [--group-log 0] — the three sparse bao calls from packed chunk bytes
(b3w_bao_outboard_update_packed_device, b3w_bao_verify_ranges_packed_device, b3w_bao_range_slice_packed_device) against their arena
counterparts of this library over a resident copy of the same files.  Measured, not gated: the kernel work per listed chunk is the
arena call's, so no speed-up is expected; what the packed calls save is the memory and the upload.

  method      tools/bao_update_measure.py's: the routes alternating in one process, device events around each whole C call (the host's
              sorting, layout, table fill and upload included), medians over about a second a route.  The arena call runs as two
              interleaved series A and B; |median A - median B| is the spread a difference has to exceed to mean anything.  The packed
              buffer is gathered before the clock starts (bao.pack_ranges): a caller with the file on disk reads it straight into place.
  cases       tools/bao_update_measure.py's shapes: 1 x 1 GiB with 1, 64 and 4 096 scattered 4 KiB ranges; 64 runs of 1 024 chunks of
              it at starts that are not tile-aligned (the range slices' case); 262 144 x 4 KiB with 4 096 listed files.
  checked     before a route is timed its outputs are compared byte for byte with the arena call's.
  recorded    beside the times: the device bytes each route needs for the files (the arena against total_bytes) and the bytes a caller
              whose files are on disk moves to the device for the call (every listed file whole against total_bytes).
Writes <out_dir>/bao_packed_measure.json."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats

m = __import__("hot-proofs-blake3-circom_amd")

BLOCK = 4096                                                               # bytes of one range: four chunks


def cases():
    """name -> (lens, files, first chunks, chunk counts)"""
    rng = np.random.default_rng(27)
    sh = BM.shapes()
    per = BLOCK // 1024
    out = {}
    blocks = BM.GIB // BLOCK
    for k in (1, 64, 4096):
        at = np.sort(rng.choice(blocks, k, replace=False)).astype(np.uint64)
        out[f"1x1GiB_{k}"] = (sh["1x1GiB"], np.zeros(k, dtype=np.uint32), at * per, np.full(k, per, dtype=np.uint64))
    starts = (np.arange(64, dtype=np.uint64) * 16384 + 517)                # 64 runs of 1 024 chunks, each across a tile boundary
    out["1x1GiB_64_runs_of_1024"] = (sh["1x1GiB"], np.zeros(64, dtype=np.uint32), starts, np.full(64, 1024, dtype=np.uint64))
    lens = sh["262144x4KiB"]
    files = np.sort(rng.choice(len(lens), 4096, replace=False)).astype(np.uint32)
    out["262144x4KiB_4096"] = (lens, files, np.zeros(4096, dtype=np.uint64), np.full(4096, per, dtype=np.uint64))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--cases", default="", help="comma-separated subset of the case names")
    ap.add_argument("--group-log", type=int, default=0)
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    gl = a.group_log
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_arena = torch.randint(0, 256, (BM.GIB + (1 << 20),), dtype=torch.uint8, device="cuda", generator=gen)
    res = dict(device=torch.cuda.get_device_name(0), arena_bytes=BM.GIB, group_log=gl, range_bytes=BLOCK,
               yardstick="the arena call of this library over the resident files, as two interleaved series", cases={})
    want = [x for x in a.cases.split(",") if x]
    for name, (lens_l, files, first, count) in cases().items():
        if want and name not in want:
            continue
        lens = np.array(lens_l, dtype=np.uint64)
        n_files, n = lens.size, files.size
        offsets = np.zeros(n_files, dtype=np.uint64)                       # back to back, every file from a 16-byte boundary
        at = 0
        for f, ln in enumerate(lens_l):
            offsets[f] = at
            at = (at + ln + 15) // 16 * 16
        assert at <= d_arena.numel()
        made = m.bao.outboard_batch(ctx, d_arena, offsets, lens) if gl == 0 else m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, gl)
        ob_first = np.ascontiguousarray(made["ob_first"], dtype=np.uint64)
        unit_first = m.bao.verify_layout(lens, gl)
        lay = m.bao.packed_layout(lens, files, first, count, gl)
        d_packed = m.bao.pack_ranges(d_arena, offsets, lens, files, first, count, gl).view(-1)
        need_u = L.b3w_bao_update_scratch_bytes(lens.ctypes.data, files.ctypes.data, first.ctypes.data, count.ctypes.data, n)
        need_v = L.b3w_bao_verify_ranges_scratch_bytes(lens.ctypes.data, files.ctypes.data, first.ctypes.data, count.ctypes.data, n)
        d_scratch = torch.empty(max(need_u, need_v, 16), dtype=torch.uint8, device="cuda")
        slice_first = m.bao.range_slice_layout(lens, files, first, count)
        common = (lens.ctypes.data, n_files, gl)
        rng_args = (files.ctypes.data, first.ctypes.data, count.ctypes.data, n)
        arena_args = (ctx.handle, d_arena.data_ptr(), d_arena.numel(), offsets.ctypes.data)
        packed_args = (ctx.handle, d_packed.data_ptr(), d_packed.numel())

        def outputs():
            return dict(obs=made["outboards"].clone(), roots=made["roots"].clone(), st=torch.full((int(unit_first[-1]),), 0xEE, dtype=torch.uint8, device="cuda"),
                        rs=torch.empty(n, dtype=torch.int32, device="cuda"), rf=torch.empty(n, dtype=torch.int64, device="cuda"),
                        slices=torch.zeros(int(slice_first[-1]), dtype=torch.uint8, device="cuda"))
        o_a, o_p = outputs(), outputs()

        def update(fn, src, o):
            rc = fn(*src, *common, ob_first.ctypes.data, o["obs"].data_ptr(), o["roots"].data_ptr(), *rng_args, d_scratch.data_ptr(), need_u, s)
            assert rc == 0, ctx.last_error()

        def verify(fn, src, o):
            rc = fn(*src, *common, ob_first.ctypes.data, made["outboards"].data_ptr(), made["roots"].data_ptr(), *rng_args, unit_first.ctypes.data, o["st"].data_ptr(),
                    o["rs"].data_ptr(), o["rf"].data_ptr(), d_scratch.data_ptr(), need_v, s)
            assert rc == 0, ctx.last_error()

        def slices(fn, src, o):
            rc = fn(*src, *common, made["outboards"].data_ptr(), *rng_args, o["slices"].data_ptr(), s)
            assert rc == 0, ctx.last_error()
        routes = {"update": (update, L.b3w_bao_outboard_update_batch_device, L.b3w_bao_outboard_update_packed_device, ("obs", "roots")),
                  "verify_ranges": (verify, L.b3w_bao_verify_ranges_batch_device, L.b3w_bao_verify_ranges_packed_device, ("st", "rs", "rf")),
                  "range_slices": (slices, L.b3w_bao_range_slice_arena_device, L.b3w_bao_range_slice_packed_device, ("slices",))}
        listed_file_bytes = int(lens[np.unique(files)].sum())
        row = dict(n_files=int(n_files), ranges=int(n), listed_chunks=int(lay["total_slots"]), total_bytes=int(lay["total_bytes"]),
                   device_bytes_for_files=dict(arena=int(lens.sum()), packed=int(lay["total_bytes"])),
                   host_to_device_bytes_for_files_on_disk=dict(arena=listed_file_bytes, packed=int(lay["total_bytes"])),
                   slice_bytes=int(slice_first[-1]), calls={})
        for what, (run, arena_fn, packed_fn, outs) in routes.items():
            run(arena_fn, arena_args, o_a)
            run(packed_fn, packed_args, o_p)
            torch.cuda.synchronize()
            assert all(torch.equal(o_a[k], o_p[k]) for k in outs), f"{name} {what}: the packed call differs from the arena call"
            for _ in range(3):
                run(arena_fn, arena_args, o_a)
                run(packed_fn, packed_args, o_p)
            t = alternating({"arena_a": lambda: run(arena_fn, arena_args, o_a), "packed": lambda: run(packed_fn, packed_args, o_p),
                             "arena_b": lambda: run(arena_fn, arena_args, o_a)})
            r = dict(arena=stats(t["arena_a"] + t["arena_b"]), arena_a=stats(t["arena_a"]), arena_b=stats(t["arena_b"]), packed=stats(t["packed"]), bytes_equal=True)
            r["arena_spread_ms"] = abs(r["arena_a"]["ms"] - r["arena_b"]["ms"])
            r["packed_minus_arena_ms"] = r["packed"]["ms"] - r["arena"]["ms"]
            r["packed_over_arena"] = r["packed"]["ms"] / r["arena"]["ms"]
            r["within_the_spread"] = abs(r["packed_minus_arena_ms"]) <= r["arena_spread_ms"]
            row["calls"][what] = r
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del made, d_packed, o_a, o_p
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_packed_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
