#!/usr/bin/env python3
"""tools/bao_diff_measure.py <out_dir> [--cases a,b,...] — the outboard diff (b3w_bao_outboard_diff_device) beside the cost of reading its
inputs and beside the route a caller had without it.

  method      tools/bao_have_measure.py's: the routes alternating in one process, device events around each whole call (the host's
              work included), medians over about a second a route.  The copy runs as two interleaved series A and B;
              |median A - median B| is the spread a difference has to exceed to mean anything.
  shapes      one_file_g0      one 1 GiB file, full outboards, 1 % of its chunks rewritten in version b
              one_file_g4      the same, group outboards of 16 chunks
              small_files_g0   262 144 files of 4 chunks, full outboards, one chunk rewritten in every tenth file
  routes      diff     b3w_bao_outboard_diff_device of a's and b's outboards into a bitmap made once
              copy     a device-to-device copy of the same two outboards' bytes: the floor that reading them costs
              verify   what a caller did before, and it needs b's BYTES resident: b3w_bao_verify_batch_device of b's bytes against a's
                       outboards and roots, then b3w_bao_have_from_status_device, into buffers made once
  checked     before a shape is timed: the diff's bitmap is the rewritten chunks' units cleared and everything else set, and the
              verify route gives the same words.
No gate: the figures are findings.  Writes <out_dir>/bao_diff_measure.json."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats

m = __import__("hot-proofs-blake3-circom_amd")

K = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--cases", default="", help="comma-separated subset: one_file_g0, one_file_g4, small_files_g0")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    s = torch.cuda.current_stream().cuda_stream
    want = [x for x in a.cases.split(",") if x]
    res = dict(device=torch.cuda.get_device_name(0), cases={})
    rng = np.random.default_rng(31)
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_old = torch.randint(0, 256, (BM.GIB,), dtype=torch.uint8, device="cuda", generator=gen)
    n_chunks = BM.GIB // K
    shapes = {"one_file_g0": (np.array([BM.GIB], dtype=np.uint64), 0), "one_file_g4": (np.array([BM.GIB], dtype=np.uint64), 4),
              "small_files_g0": (np.full(262144, 4 * K, dtype=np.uint64), 0)}
    for name, (lens, g) in shapes.items():
        if want and name not in want:
            continue
        offsets = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
        if lens.size == 1:
            rewritten = np.sort(rng.permutation(n_chunks)[:n_chunks // 100])
        else:
            files = np.arange(0, lens.size, 10)
            rewritten = files * 4 + rng.integers(0, 4, files.size)
        d_new = d_old.clone()
        d_new.view(-1, K)[torch.from_numpy(rewritten).cuda()] ^= 0x55
        make = (lambda d: m.bao.outboard_batch(ctx, d, offsets, lens)) if g == 0 else (lambda d: m.bao.outboard_groups_batch(ctx, d, offsets, lens, g))
        old, new = make(d_old), make(d_new)
        ob_first = old["ob_first"]
        ob_bytes = int(ob_first[-1])
        pairs = np.arange(lens.size, dtype=np.uint32)
        word_first = m.bao.have_layout(lens)
        words = int(word_first[-1])
        d_same = torch.empty(words, dtype=torch.int64, device="cuda")
        d_route = torch.empty(words, dtype=torch.int64, device="cuda")
        d_copy = torch.empty(2 * ob_bytes, dtype=torch.uint8, device="cuda")
        unit_first = m.bao.verify_layout(lens, g)
        d_units = torch.empty(int(unit_first[-1]), dtype=torch.uint8, device="cuda")
        d_fstat = torch.empty(lens.size, dtype=torch.int32, device="cuda")
        d_fbad = torch.empty(lens.size, dtype=torch.int64, device="cuda")
        need = L.b3w_bao_verify_scratch_bytes(lens.ctypes.data, lens.size)
        d_scratch = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")

        def diff():
            rc = L.b3w_bao_outboard_diff_device(ctx.handle, lens.ctypes.data, ob_first.ctypes.data, old["outboards"].data_ptr(), ob_bytes, old["roots"].data_ptr(),
                                                lens.size, g, lens.ctypes.data, ob_first.ctypes.data, new["outboards"].data_ptr(), ob_bytes, new["roots"].data_ptr(),
                                                lens.size, g, pairs.ctypes.data, pairs.ctypes.data, lens.size, word_first.ctypes.data, d_same.data_ptr(), s)
            assert rc == 0, ctx.last_error()

        def copy():
            d_copy[:ob_bytes].copy_(old["outboards"])
            d_copy[ob_bytes:].copy_(new["outboards"])

        def verify():
            rc = L.b3w_bao_verify_batch_device(ctx.handle, d_new.data_ptr(), offsets.ctypes.data, lens.ctypes.data, lens.size, g, old["outboards"].data_ptr(),
                                               old["roots"].data_ptr(), d_units.data_ptr(), d_fstat.data_ptr(), d_fbad.data_ptr(),
                                               d_scratch.data_ptr() if need else None, need, s)
            assert rc == 0, ctx.last_error()
            rc = L.b3w_bao_have_from_status_device(ctx.handle, d_units.data_ptr(), lens.ctypes.data, lens.size, g, d_route.data_ptr(), s)
            assert rc == 0, ctx.last_error()
        diff()
        verify()
        torch.cuda.synchronize()
        bits = np.ones(n_chunks, bool)
        for k in range(1 << g):
            bits[(rewritten >> g << g) + k] = False
        expect = np.packbits(bits, bitorder="little").view(np.uint64) if lens.size == 1 else bits.reshape(-1, 4).astype(np.uint64) @ np.array([1, 2, 4, 8], dtype=np.uint64)
        got = d_same.cpu().numpy().view(np.uint64)
        assert (got == expect).all(), f"{name}: the diff's bitmap is not the rewritten chunks' units cleared"
        assert (d_route.cpu().numpy().view(np.uint64) == got).all(), f"{name}: the verify route gives other words"
        for _ in range(3):
            copy()
            diff()
            verify()
        t = alternating({"copy_a": copy, "diff": diff, "verify": verify, "copy_b": copy})
        row = dict(files=int(lens.size), chunks=n_chunks, group_log=g, words=words, outboard_bytes_both=2 * ob_bytes, rewritten_chunks=int(rewritten.size),
                   chunks_same=int(bits.sum()), checked=True, diff=stats(t["diff"]), verify=stats(t["verify"]), copy=stats(t["copy_a"] + t["copy_b"]),
                   copy_a=stats(t["copy_a"]), copy_b=stats(t["copy_b"]))
        row["spread_ms"] = abs(row["copy_a"]["ms"] - row["copy_b"]["ms"])
        row["diff_over_copy"] = row["diff"]["ms"] / row["copy"]["ms"]
        row["diff_over_verify"] = row["diff"]["ms"] / row["verify"]["ms"]
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del d_new, old, new, d_copy
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_diff_measure.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
