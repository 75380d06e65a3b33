#!/usr/bin/env python3
"""tools/bao_resize_measure.py <out_dir> [--parent-lib libb3wit.so] [--quick] [--cases a,b,...] — outboards of resident files after
appends and truncations (b3w_bao_outboard_resize_batch_device) against what a caller did before it: the full
b3w_bao_[group_]outboard_batch_device over the files at their new lengths.

  yardstick   the batch call of the library given with --parent-lib (a build of the commit before the resize call, loaded beside this
              one; its own context) or, without it, of this library.  It runs over the files at their NEW lengths.
  method      tools/bao_update_measure.py's: the routes alternating in one process, device events around each whole call (the host's
              table fill and upload included), medians over about a second a route.  The yardstick runs as two interleaved series A and
              B; |median A - median B| is the spread a difference has to exceed to mean anything.
  cases       1 x 1 GiB at g = 0: an append of 4 KiB, of 1 MiB, of 64 MiB; 512 MiB -> 1 GiB; a truncation by 4 KiB and to 512 MiB
              ("1 GiB" is the longer of the two lengths).  The first and the fifth at g = 4.  (1 GiB + 512 KiB) + 4 KiB: both merge
              storeys.  16 384 x 64 KiB, each growing by 4 KiB: no tile is kept, everything is hashed again — what the call costs
              where it cannot gain.
  checked     before a case is timed every outboard byte and root of the resize is compared with the batch call's.
  gate        on 1 x 1 GiB with a 4 KiB append the resize beats the yardstick by more than the yardstick's spread.
Writes <out_dir>/bao_resize_measure.json.  --quick: ten resize calls a case and no timing, no yardstick series — for a run under
`rocprofv3 --kernel-trace --stats`, whose per-kernel call counts divided by ten are the launches of one call."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats
from bao_update_measure import parent_library

m = __import__("hot-proofs-blake3-circom_amd")

QUICK_CALLS = 10
KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30


def cases():
    """name -> (group_log, old lengths, new lengths)"""
    out = {}
    for g in (0, 4):
        tag = "" if g == 0 else "_g4"
        out["1x1GiB_append_4KiB" + tag] = (g, [GIB - 4 * KIB], [GIB])
        if g == 0:
            out["1x1GiB_append_1MiB"] = (g, [GIB - MIB], [GIB])
            out["1x1GiB_append_64MiB"] = (g, [GIB - 64 * MIB], [GIB])
            out["1x1GiB_from_512MiB"] = (g, [GIB // 2], [GIB])
        out["1x1GiB_truncate_by_4KiB" + tag] = (g, [GIB], [GIB - 4 * KIB])
        if g == 0:
            out["1x1GiB_truncate_to_512MiB"] = (g, [GIB], [GIB // 2])
    out["past1GiB_append_4KiB"] = (0, [GIB + 512 * KIB], [GIB + 516 * KIB])
    out["16384x64KiB_append_4KiB"] = (0, [64 * KIB] * 16384, [68 * KIB] * 16384)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default="", help="libb3wit.so built from the commit before the resize call: the yardstick")
    ap.add_argument("--quick", action="store_true", help="ten resize calls a case (under a profiler)")
    ap.add_argument("--cases", default="", help="comma-separated subset of the case names")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bao_resize_measure: no GPU")
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    if a.parent_lib:
        Y, y_ctx = parent_library(a.parent_lib)
        yard = f"b3w_bao_[group_]outboard_batch_device of {os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff}), loaded beside this library"
    else:
        Y, y_ctx = L, ctx.handle
        yard = "b3w_bao_[group_]outboard_batch_device of this library"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_arena = torch.randint(0, 256, (GIB + 70 * MIB,), dtype=torch.uint8, device="cuda", generator=gen)
    base = d_arena.data_ptr()
    res = dict(device=torch.cuda.get_device_name(0), yardstick=yard, cases={})
    want_cases = [x for x in a.cases.split(",") if x]
    for name, (gl, old_l, new_l) in cases().items():
        if want_cases and name not in want_cases:
            continue
        old_lens, new_lens = np.array(old_l, dtype=np.uint64), np.array(new_l, dtype=np.uint64)
        n_files = new_lens.size
        offsets = np.zeros(n_files, dtype=np.uint64)                       # back to back, every slot (the longer length) from a 16-byte boundary
        at = 0
        for f in range(n_files):
            offsets[f] = at
            at = (at + max(old_l[f], new_l[f]) + 15) // 16 * 16
        assert at <= d_arena.numel()
        files = np.arange(n_files, dtype=np.uint32)
        old_first, new_first = m.bao.group_batch_layout(old_lens, gl), m.bao.group_batch_layout(new_lens, gl)
        d_old = torch.empty(int(old_first[-1]), dtype=torch.uint8, device="cuda")
        d_new, d_want = (torch.empty(int(new_first[-1]), dtype=torch.uint8, device="cuda") for _ in range(2))
        d_roots_old, d_roots_new, d_roots_want = (torch.empty((n_files, 8), dtype=torch.int32, device="cuda") for _ in range(3))
        need_y = max(L.b3w_bao_batch_scratch_bytes(old_lens.ctypes.data, n_files), L.b3w_bao_batch_scratch_bytes(new_lens.ctypes.data, n_files))
        d_scratch_y = torch.empty(max(need_y, 16), dtype=torch.uint8, device="cuda")
        need_r = L.b3w_bao_resize_scratch_bytes(new_lens.ctypes.data, files.ctypes.data, files.size)
        d_scratch_r = torch.empty(max(need_r, 16), dtype=torch.uint8, device="cuda")

        def batch(lens, obs, roots):
            if gl:
                rc = Y.b3w_bao_group_outboard_batch_device(y_ctx, base, offsets.ctypes.data, lens.ctypes.data, n_files, gl, obs.data_ptr(), roots.data_ptr(),
                                                           d_scratch_y.data_ptr(), need_y, s)
            else:
                rc = Y.b3w_bao_outboard_batch_device(y_ctx, base, offsets.ctypes.data, lens.ctypes.data, n_files, obs.data_ptr(), roots.data_ptr(),
                                                     d_scratch_y.data_ptr(), need_y, s)
            assert rc == 0, rc

        def yardstick():
            batch(new_lens, d_want, d_roots_want)

        def resize():
            rc = L.b3w_bao_outboard_resize_batch_device(ctx.handle, base, d_arena.numel(), offsets.ctypes.data, old_lens.ctypes.data, new_lens.ctypes.data,
                                                        n_files, gl, old_first.ctypes.data, d_old.data_ptr(), new_first.ctypes.data, d_new.data_ptr(),
                                                        d_roots_new.data_ptr(), files.ctypes.data, files.size, d_scratch_r.data_ptr(), need_r, s)
            assert rc == 0, ctx.last_error()
        batch(old_lens, d_old, d_roots_old)                                # the outboards of before
        d_new.fill_(0xA5)
        resize()
        yardstick()
        torch.cuda.synchronize()
        assert torch.equal(d_new, d_want) and torch.equal(d_roots_new, d_roots_want), f"{name}: the resize differs from the batch call"
        kept = sum(int(L.b3w_bao_resize_kept_tiles(int(o), int(n))) for o, n in zip(old_l, new_l))
        tiles = sum((m.bao.num_chunks(int(n)) + 1023) // 1024 for n in new_l)
        row = dict(group_log=gl, n_files=int(n_files), old_bytes=int(old_lens.sum()), new_bytes=int(new_lens.sum()), kept_tiles=kept, hashed_tiles=tiles - kept,
                   new_outboard_bytes=int(new_first[-1]), resize_scratch_bytes=int(need_r), bytes_equal=True)
        if a.quick:
            for _ in range(QUICK_CALLS):
                resize()
            torch.cuda.synchronize()
            row["resize_calls"] = QUICK_CALLS
            res["cases"][name] = row
            continue
        for _ in range(3):
            yardstick()
            resize()
        t = alternating({"yard_a": yardstick, "resize": resize, "yard_b": yardstick})
        row.update(yardstick=stats(t["yard_a"] + t["yard_b"]), yardstick_a=stats(t["yard_a"]), yardstick_b=stats(t["yard_b"]), resize=stats(t["resize"]))
        row["yardstick_spread_ms"] = abs(row["yardstick_a"]["ms"] - row["yardstick_b"]["ms"])
        row["yardstick_minus_resize_ms"] = row["yardstick"]["ms"] - row["resize"]["ms"]
        row["resize_over_yardstick"] = row["resize"]["ms"] / row["yardstick"]["ms"]
        row["resize_wins_by_more_than_the_spread"] = row["yardstick_minus_resize_ms"] > row["yardstick_spread_ms"]
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del d_old, d_new, d_want
    if not a.quick:
        one = res["cases"].get("1x1GiB_append_4KiB")
        if one:
            res["gate"] = dict(case="1x1GiB_append_4KiB", passed=bool(one["resize_wins_by_more_than_the_spread"]), yardstick_ms=one["yardstick"]["ms"],
                               resize_ms=one["resize"]["ms"], spread_ms=one["yardstick_spread_ms"])
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_resize_measure.json" if not a.quick else "bao_resize_measure_quick.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
