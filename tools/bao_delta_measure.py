#!/usr/bin/env python3
"""tools/bao_delta_measure.py <out_dir> [--cases a,b,...] — outboard deltas (b3w_bao_outboard_delta_device / _apply_device) beside the cost
of reading their inputs and beside the routes a caller had without them.

  method      tools/bao_diff_measure.py's: the routes alternating in one process, device events around each whole call (the host's
              work included), medians over about a second a route.  The copy of b's outboard runs as two interleaved series A and B;
              |median A - median B| is the spread a difference has to exceed to mean anything.  No profiler run.
  shapes      one_file_g0       one 1 GiB file, full outboards, 1 % of its chunks rewritten in version b
              one_file_g4       the same, group outboards of 16 chunks
              small_files_g0    262 144 files of 4 chunks, full outboards, one chunk rewritten in every tenth file
              one_file_g0_half  one 1 GiB file, full outboards, 50 % of its chunks rewritten
  routes      delta    the provider: a's and b's outboards into blobs at their bounds, buffers made once
              copy2    a device-to-device copy of the same two outboards' bytes: the provider's read floor
              diff     b3w_bao_outboard_diff_device over the same two outboards
              apply    the replica: the blobs verified and b's outboards assembled into a fresh buffer
              copy_a / copy_b   the copy of b's whole outboard: what a trusting replica did before
              verify   b3w_bao_verify_batch_device of b's RESIDENT file against b's outboard and root: the only way to catch a lying
                       outboard before
              check    outboard_check's two calls (the delta against nothing, applied into a scratch outboard) over b's outboards
  checked     before a shape is timed: every pair passes, the applied outboards are b's byte for byte, the check passes.
No gate: the figures are findings.  Writes <out_dir>/bao_delta_measure.json."""
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
    ap.add_argument("--cases", default="", help="comma-separated subset: one_file_g0, one_file_g4, small_files_g0, one_file_g0_half")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    s = torch.cuda.current_stream().cuda_stream
    want = [x for x in a.cases.split(",") if x]
    res = dict(device=torch.cuda.get_device_name(0), cases={})
    rng = np.random.default_rng(32)
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_old = torch.randint(0, 256, (BM.GIB,), dtype=torch.uint8, device="cuda", generator=gen)
    n_chunks = BM.GIB // K
    one = np.array([BM.GIB], dtype=np.uint64)
    shapes = {"one_file_g0": (one, 0, 100), "one_file_g4": (one, 4, 100), "small_files_g0": (np.full(262144, 4 * K, dtype=np.uint64), 0, 0),
              "one_file_g0_half": (one, 0, 2)}
    for name, (lens, g, share) in shapes.items():
        if want and name not in want:
            continue
        offsets = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
        if lens.size == 1:
            rewritten = np.sort(rng.permutation(n_chunks)[:n_chunks // share])
        else:
            files = np.arange(0, lens.size, 10)
            rewritten = files * 4 + rng.integers(0, 4, files.size)
        d_new = d_old.clone()
        d_new.view(-1, K)[torch.from_numpy(rewritten).cuda()] ^= 0x55
        make = (lambda d: m.bao.outboard_batch(ctx, d, offsets, lens)) if g == 0 else (lambda d: m.bao.outboard_groups_batch(ctx, d, offsets, lens, g))
        old, new = make(d_old), make(d_new)
        ob_first = np.ascontiguousarray(old["ob_first"], dtype=np.uint64)
        ob_bytes = int(ob_first[-1])
        n = int(lens.size)
        pairs = np.arange(n, dtype=np.uint32)
        none = np.full(n, m.bao.DELTA_NO_A, dtype=np.uint32)
        dfirst = m.bao.delta_layout(lens, g)
        d_delta = torch.empty(int(dfirst[-1]), dtype=torch.uint8, device="cuda")
        d_full = torch.empty(int(dfirst[-1]), dtype=torch.uint8, device="cuda")
        d_nodes = torch.empty(n, dtype=torch.int64, device="cuda")
        d_out = torch.zeros(ob_bytes, dtype=torch.uint8, device="cuda")
        d_status = torch.empty(n, dtype=torch.int32, device="cuda")
        d_bad = torch.empty(n, dtype=torch.int64, device="cuda")
        sc_bytes = int(L.b3w_bao_outboard_delta_scratch_bytes(lens.ctypes.data, n, pairs.ctypes.data, n, g))
        d_sc = torch.empty(sc_bytes, dtype=torch.uint8, device="cuda")
        word_first = m.bao.have_layout(lens)
        d_same = torch.empty(int(word_first[-1]), dtype=torch.int64, device="cuda")
        d_copy = torch.empty(2 * ob_bytes, dtype=torch.uint8, device="cuda")
        unit_first = m.bao.verify_layout(lens, g)
        d_units = torch.empty(int(unit_first[-1]), dtype=torch.uint8, device="cuda")
        d_fstat = torch.empty(n, dtype=torch.int32, device="cuda")
        d_fbad = torch.empty(n, dtype=torch.int64, device="cuda")
        need = L.b3w_bao_verify_scratch_bytes(lens.ctypes.data, n)
        d_vsc = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")

        def provider(pa, side, into):
            rc = L.b3w_bao_outboard_delta_device(ctx.handle, lens.ctypes.data, ob_first.ctypes.data, side["outboards"].data_ptr(), ob_bytes, side["roots"].data_ptr(), n,
                                                 lens.ctypes.data, ob_first.ctypes.data, new["outboards"].data_ptr(), ob_bytes, new["roots"].data_ptr(), n, g, g,
                                                 pa.ctypes.data, pairs.ctypes.data, n, dfirst.ctypes.data, into.data_ptr(), into.numel(), d_nodes.data_ptr(),
                                                 d_sc.data_ptr(), sc_bytes, s)
            assert rc == 0, ctx.last_error()

        def replica(pa, blobs):
            rc = L.b3w_bao_outboard_delta_apply_device(ctx.handle, lens.ctypes.data, ob_first.ctypes.data, old["outboards"].data_ptr(), ob_bytes, old["roots"].data_ptr(), n,
                                                       lens.ctypes.data, new["roots"].data_ptr(), n, g, pa.ctypes.data, pairs.ctypes.data, n, dfirst.ctypes.data,
                                                       blobs.data_ptr(), blobs.numel(), ob_first.ctypes.data, d_out.data_ptr(), ob_bytes, d_status.data_ptr(),
                                                       d_bad.data_ptr(), d_sc.data_ptr(), sc_bytes, s)
            assert rc == 0, ctx.last_error()

        def delta():
            provider(pairs, old, d_delta)

        def apply():
            replica(pairs, d_delta)

        def check():
            provider(none, old, d_full)
            replica(none, d_full)

        def copy2():
            d_copy[:ob_bytes].copy_(old["outboards"])
            d_copy[ob_bytes:].copy_(new["outboards"])

        def copy_b():
            d_copy[:ob_bytes].copy_(new["outboards"])

        def diff():
            rc = L.b3w_bao_outboard_diff_device(ctx.handle, lens.ctypes.data, ob_first.ctypes.data, old["outboards"].data_ptr(), ob_bytes, old["roots"].data_ptr(), n, g,
                                                lens.ctypes.data, ob_first.ctypes.data, new["outboards"].data_ptr(), ob_bytes, new["roots"].data_ptr(), n, g,
                                                pairs.ctypes.data, pairs.ctypes.data, n, word_first.ctypes.data, d_same.data_ptr(), s)
            assert rc == 0, ctx.last_error()

        def verify():
            rc = L.b3w_bao_verify_batch_device(ctx.handle, d_new.data_ptr(), offsets.ctypes.data, lens.ctypes.data, n, g, new["outboards"].data_ptr(),
                                               new["roots"].data_ptr(), d_units.data_ptr(), d_fstat.data_ptr(), d_fbad.data_ptr(), d_vsc.data_ptr() if need else None, need, s)
            assert rc == 0, ctx.last_error()
        check()
        torch.cuda.synchronize()
        assert not d_status.any().item() and torch.equal(d_out, new["outboards"]), f"{name}: the check does not pass"
        full_nodes = int(d_nodes.sum().item())
        d_out.zero_()
        delta()
        apply()
        verify()
        torch.cuda.synchronize()
        assert not d_status.any().item() and (d_bad == -1).all().item(), f"{name}: a pair did not pass"
        assert torch.equal(d_out, new["outboards"]), f"{name}: the applied outboards are not b's"
        assert not d_fstat.any().item()
        sent = int(d_nodes.sum().item())
        units = (int(L.b3w_bao_group_outboard_size(int(lens[0]), g)) - 8) // 64 + 1            # (the files of a shape are of one length)
        heads = n * (16 + 8 * ((units - 1 + 63) // 64))
        delta_bytes = heads + 64 * sent
        routes = {"copy_a": copy_b, "delta": delta, "copy2": copy2, "diff": diff, "apply": apply, "verify": verify, "check": check, "copy_b": copy_b}
        for _ in range(3):
            for f in routes.values():
                f()
        t = alternating(routes)
        row = dict(files=n, chunks=n_chunks, group_log=g, rewritten_chunks=int(rewritten.size), outboard_bytes_b=ob_bytes, nodes_b=full_nodes, nodes_sent=sent,
                   delta_bytes=delta_bytes, delta_over_outboard=delta_bytes / ob_bytes, checked=True, staging_bytes=72 * n + 8,
                   **{k: stats(t[k]) for k in ("delta", "copy2", "diff", "apply", "verify", "check", "copy_a", "copy_b")})
        row["copy_b_both"] = stats(t["copy_a"] + t["copy_b"])
        row["spread_ms"] = abs(row["copy_a"]["ms"] - row["copy_b"]["ms"])
        for x, y in (("delta", "copy2"), ("delta", "diff"), ("apply", "copy_b_both"), ("apply", "verify"), ("check", "verify")):
            row[f"{x}_over_{y}"] = row[x]["ms"] / row[y]["ms"]
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del d_new, old, new, d_copy, d_delta, d_full, d_out
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_delta_measure.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
