#!/usr/bin/env python3
"""tools/bao_verify_ranges_measure.py <out_dir> [--parent-lib libb3wit.so] [--cases a,b,...] [--group-log 0] [--no-planning] — listed
chunk ranges verified against their outboards (b3w_bao_verify_ranges_batch_device) against what a caller did before it: the whole-file
b3w_bao_verify_batch_device over the same files.

  yardstick   the whole-file call of the library given with --parent-lib (a build of the commit before the ranged call, loaded beside
              this one; its own context) or, without it, of this library.
  method      tools/bao_update_measure.py's: the routes alternating in one process, device events around each whole call (the host's
              sorting, table fill and upload included), medians over about a second a route.  The yardstick runs as two interleaved
              series A and B; |median A - median B| is the spread a difference has to exceed to mean anything.
  cases       1 x 1 GiB with 1, 64, 1 024 and 4 096 scattered 4 KiB ranges; every chunk of it in one range; a sweep of the number of
              ranges for the break-even; 262 144 x 4 KiB with 4 096 listed files.
  checked     before a case is timed a byte of the first listed chunk is flipped, and the ranged call's bytes at the listed units are
              compared with the yardstick's (the flip is undone afterwards).
  planning    the same single range through b3w_sample_plan_arena_device on a nova context: for comparison only, no gate.
  gate        on 1 x 1 GiB with one 4 KiB range the ranged call's median lies below the yardstick's by more than the spread.
Writes <out_dir>/bao_verify_ranges_measure.json."""
import argparse, ctypes, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats

m = __import__("hot-proofs-blake3-circom_amd")

BLOCK = 4096                                                               # bytes of one range: four chunks
SWEEP = [256, 2048]                                                        # ranges into the 1 GiB file, between the cases' 1 / 64 / 1 024 / 4 096 and all


def parent_library(path):
    """the yardstick library and a nova_vesta context of its own -> (lib, ctx handle)"""
    vp, u32, i32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    P.b3w_bao_verify_batch_device.restype, P.b3w_bao_verify_batch_device.argtypes = i32, [vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, u64, vp]
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


def cases():
    """name -> (lens, files, first chunks, chunk counts): whole 4 KiB blocks, scattered by a fixed seed, no block twice"""
    rng = np.random.default_rng(19)
    sh = BM.shapes()
    per = BLOCK // 1024
    out = {}
    blocks = BM.GIB // BLOCK
    for k in [1, 64, 1024, 4096] + SWEEP:
        at = np.sort(rng.choice(blocks, k, replace=False)).astype(np.uint64)
        out[f"1x1GiB_{k}"] = (sh["1x1GiB"], np.zeros(k, dtype=np.uint32), at * per, np.full(k, per, dtype=np.uint64))
    out["1x1GiB_all"] = (sh["1x1GiB"], np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64), np.full(1, BM.GIB // 1024, dtype=np.uint64))
    lens = sh["262144x4KiB"]
    files = np.sort(rng.choice(len(lens), 4096, replace=False)).astype(np.uint32)
    out["262144x4KiB_4096"] = (lens, files, np.zeros(4096, dtype=np.uint64), np.full(4096, per, dtype=np.uint64))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default="", help="libb3wit.so built from the commit before the ranged call: the yardstick")
    ap.add_argument("--cases", default="", help="comma-separated subset of the case names")
    ap.add_argument("--group-log", type=int, default=0)
    ap.add_argument("--no-planning", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    gl = a.group_log
    if a.parent_lib:
        Y, y_ctx = parent_library(a.parent_lib)
        yard = f"b3w_bao_verify_batch_device of {os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff}), loaded beside this library"
    else:
        Y, y_ctx = L, ctx.handle
        yard = "b3w_bao_verify_batch_device of this library"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_arena = torch.randint(0, 256, (BM.GIB + (1 << 20),), dtype=torch.uint8, device="cuda", generator=gen)
    base = d_arena.data_ptr()
    res = dict(device=torch.cuda.get_device_name(0), arena_bytes=BM.GIB, group_log=gl, range_bytes=BLOCK, yardstick=yard, cases={})
    want = [x for x in a.cases.split(",") if x]
    for name, (lens_l, files, first, count) in cases().items():
        if want and name not in want:
            continue
        lens = np.array(lens_l, dtype=np.uint64)
        n_files = lens.size
        offsets = np.zeros(n_files, dtype=np.uint64)                       # back to back, every file from a 16-byte boundary
        at = 0
        for f, ln in enumerate(lens_l):
            offsets[f] = at
            at = (at + ln + 15) // 16 * 16
        assert at <= d_arena.numel()
        made = m.bao.outboard_batch(ctx, d_arena, offsets, lens) if gl == 0 else m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, gl)
        ob_first = np.ascontiguousarray(made["ob_first"], dtype=np.uint64)
        unit_first = m.bao.verify_layout(lens, gl)
        d_obs, d_roots = made["outboards"], made["roots"]
        total = int(unit_first[-1])
        need_y = L.b3w_bao_verify_scratch_bytes(lens.ctypes.data, n_files)
        d_scratch_y = torch.empty(max(need_y, 16), dtype=torch.uint8, device="cuda")
        y_st = torch.empty(total, dtype=torch.uint8, device="cuda")
        y_fs, y_fb = torch.empty(n_files, dtype=torch.int32, device="cuda"), torch.empty(n_files, dtype=torch.int64, device="cuda")
        need_r = L.b3w_bao_verify_ranges_scratch_bytes(lens.ctypes.data, files.ctypes.data, first.ctypes.data, count.ctypes.data, files.size)
        d_scratch_r = torch.empty(max(need_r, 16), dtype=torch.uint8, device="cuda")
        r_st = torch.full((total,), 0xEE, dtype=torch.uint8, device="cuda")
        r_rs, r_rf = torch.empty(files.size, dtype=torch.int32, device="cuda"), torch.empty(files.size, dtype=torch.int64, device="cuda")

        def yardstick():
            rc = Y.b3w_bao_verify_batch_device(y_ctx, base, offsets.ctypes.data, lens.ctypes.data, n_files, gl, d_obs.data_ptr(), d_roots.data_ptr(),
                                               y_st.data_ptr(), y_fs.data_ptr(), y_fb.data_ptr(), d_scratch_y.data_ptr(), need_y, s)
            assert rc == 0, rc

        def ranged():
            rc = L.b3w_bao_verify_ranges_batch_device(ctx.handle, base, d_arena.numel(), offsets.ctypes.data, lens.ctypes.data, n_files, gl, ob_first.ctypes.data,
                                                      d_obs.data_ptr(), d_roots.data_ptr(), files.ctypes.data, first.ctypes.data, count.ctypes.data, files.size,
                                                      unit_first.ctypes.data, r_st.data_ptr(), r_rs.data_ptr(), r_rf.data_ptr(), d_scratch_r.data_ptr(), need_r, s)
            assert rc == 0, ctx.last_error()
        # the check: a byte of the first listed chunk flipped, the listed units' bytes against the yardstick's
        listed = torch.zeros(total, dtype=torch.bool, device="cuda")
        for f, a0, c in zip(files.tolist(), first.tolist(), count.tolist()):
            n = m.bao.num_chunks(int(lens[f]))
            lo, hi = (0, n - 1) if n <= 64 else (a0, a0 + c - 1)
            listed[int(unit_first[f]) + (lo >> gl):int(unit_first[f]) + (hi >> gl) + 1] = True
        spot = int(offsets[files[0]]) + int(first[0]) * 1024 + 5
        d_arena[spot] ^= 1
        yardstick()
        ranged()
        torch.cuda.synchronize()
        bad_unit = int(unit_first[files[0]]) + (int(first[0]) >> gl)
        assert int(y_st[bad_unit].item()) == 1 and int(r_rs[0].item()) == 1 and int(r_rf[0].item()) == int(first[0]) >> gl, name
        assert torch.equal(r_st[listed], y_st[listed]) and bool((r_st[~listed] == 0xEE).all().item()), f"{name}: the ranged call differs from the whole-file call"
        d_arena[spot] ^= 1
        yardstick()
        ranged()
        torch.cuda.synchronize()
        assert not y_st.any().item() and not r_st[listed].any().item() and not r_rs.any().item(), name
        tiles = len({(f, t) for f, a0, c in zip(files.tolist(), first.tolist(), count.tolist()) for t in range(a0 // 1024, (a0 + c - 1) // 1024 + 1)})
        row = dict(n_files=int(n_files), bytes=int(lens.sum()), ranges=int(files.size), listed_chunks=int(count.sum()), listed_tiles_or_small_files=tiles,
                   listed_fraction=int(count.sum()) / float(sum(m.bao.num_chunks(int(x)) for x in lens_l)), ranged_scratch_bytes=int(need_r), statuses_equal=True)
        for _ in range(3):
            yardstick()
            ranged()
        t = alternating({"yard_a": yardstick, "ranged": ranged, "yard_b": yardstick})
        row.update(yardstick=stats(t["yard_a"] + t["yard_b"]), yardstick_a=stats(t["yard_a"]), yardstick_b=stats(t["yard_b"]), ranged=stats(t["ranged"]))
        row["yardstick_spread_ms"] = abs(row["yardstick_a"]["ms"] - row["yardstick_b"]["ms"])
        row["yardstick_minus_ranged_ms"] = row["yardstick"]["ms"] - row["ranged"]["ms"]
        row["ranged_over_yardstick"] = row["ranged"]["ms"] / row["yardstick"]["ms"]
        row["ranged_wins_by_more_than_the_spread"] = row["yardstick_minus_ranged_ms"] > row["yardstick_spread_ms"]
        if name == "1x1GiB_1" and not a.no_planning:                       # the only other route to one range's statuses today: planned samples
            per = int(count[0])
            sf, sc = np.zeros(per, dtype=np.uint32), (int(first[0]) + np.arange(per)).astype(np.uint64)

            def planned():
                m.bao.plan_samples_arena(ctx, d_arena, offsets, lens, d_obs, d_roots, sf, sc, gl)
            for _ in range(3):
                planned()
            row["plan_samples_arena"] = stats(alternating({"planned": planned})["planned"])
            row["plan_samples_arena"]["note"] = "the Python call, its record and status buffers allocated inside the timed call; comparison only"
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del made, d_obs, d_roots, y_st, r_st, listed
    one = res["cases"].get("1x1GiB_1")
    if one:
        res["gate"] = dict(case="1x1GiB_1", passed=bool(one["ranged_wins_by_more_than_the_spread"]), yardstick_ms=one["yardstick"]["ms"],
                           ranged_ms=one["ranged"]["ms"], spread_ms=one["yardstick_spread_ms"])
    sweep = sorted((r["listed_tiles_or_small_files"], r["ranged_wins_by_more_than_the_spread"], n) for n, r in res["cases"].items() if n.startswith("1x1GiB_"))
    if sweep:
        winning = [k for k, w, _ in sweep if w]
        losing = [k for k, w, _ in sweep if not w]
        res["break_even_1x1GiB"] = dict(most_listed_tiles_that_win=max(winning) if winning else None,
                                        fewest_listed_tiles_that_do_not=min(losing) if losing else None, tiles_in_the_file=1024)
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_verify_ranges_measure.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
