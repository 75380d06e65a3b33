#!/usr/bin/env python3
"""tools/bao_have_measure.py <out_dir> [--cases a,b,...] — the arrival bitmap: what recording costs the ingest, and the device's run lists
(b3w_bao_have_runs_device) against what a receiver did without them.

  method      tools/bao_ingest_measure.py's: the routes alternating in one process, device events around each whole call (the host's
              work and every copy to the host included), medians over about a second a route.  The yardstick runs as two interleaved
              series A and B; |median A - median B| is the spread a difference has to exceed to mean anything.
  ingest      b3w_bao_slice_ingest_have_device against b3w_bao_slice_ingest_device (the yardstick) of this build: the same 4 096 and
              65 536 distinct slices of one 1 GiB file, g = 0, the default lanes.  The three instantiations behind the existing entry
              have the parent commit's ISA text (profiles/r22/bao_have_kernel_resource_usage.txt), so there is no A/B against a parent build.
  runs        the missing runs, on the host at the end, of: one file of 2^20 chunks with 1 % and with 50 % of its chunks missing at random
              and with one missing run; 262 144 files of 4 chunks at 50 %.
                device   b3w_bao_have_runs_device into buffers made once, n_runs copied to the host, then the rows written
                host     (the yardstick) what a caller did before: the last ingest's sample_status (65 536 samples) copied to the host,
                         scattered into the caller's own map of every chunk, and the rows made from the map with numpy.  No library
                         call is in it, so the parent commit's library would give the same figures.
  checked     before a case is timed: the bitmap after the ingest holds exactly the slices' bits; both run routes give the same rows.
No gate: the figures are findings.  Writes <out_dir>/bao_have_measure.json."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats

m = __import__("hot-proofs-blake3-circom_amd")

N = BM.GIB // 1024
LAST_INGEST = 65536


def host_rows(have_map, file_first, d_status, slots):
    """the caller's own route: the statuses to the host, into the map, the map into rows (file, first chunk, count) of missing chunks"""
    st = d_status.cpu().numpy()
    have_map[slots[st == 0]] = True
    sel = ~have_map
    prev = np.empty_like(sel)
    prev[0] = False
    prev[1:] = sel[:-1]
    prev[file_first[:-1]] = False
    nxt = np.empty_like(sel)
    nxt[-1] = False
    nxt[:-1] = sel[1:]
    nxt[file_first[1:] - 1] = False
    starts, ends = np.nonzero(sel & ~prev)[0], np.nonzero(sel & ~nxt)[0]
    files = np.searchsorted(file_first, starts, side="right") - 1
    return files.astype(np.uint32), (starts - file_first[files]).astype(np.uint64), (ends - starts + 1).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--cases", default="", help="comma-separated subset: ingest_4096, ingest_65536, runs_1pct, runs_50pct, runs_one_run, runs_small_files")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    s = torch.cuda.current_stream().cuda_stream
    want = [x for x in a.cases.split(",") if x]
    res = dict(device=torch.cuda.get_device_name(0), cases={},
               existing_entry="not measured: b3w_bao_slice_ingest_kernel<1>, <4> and <16> have the parent commit's ISA text line for line")
    rng = np.random.default_rng(22)
    ingest_cases = [k for k in (4096, 65536) if not want or f"ingest_{k}" in want]
    if ingest_cases:
        gen = torch.Generator(device="cuda").manual_seed(1)
        d_src = torch.randint(0, 256, (BM.GIB,), dtype=torch.uint8, device="cuda", generator=gen)
        d_dst = torch.empty(BM.GIB, dtype=torch.uint8, device="cuda")
        lens, zero = np.array([BM.GIB], dtype=np.uint64), np.zeros(1, dtype=np.uint64)
        provider = m.bao.outboard_batch(ctx, d_src, zero, lens)
        d_roots = provider["roots"]
        d_obs = torch.empty(m.bao.outboard_size(BM.GIB), dtype=torch.uint8, device="cuda")
        for k in ingest_cases:
            chunks = rng.permutation(N)[:k].astype(np.uint64)
            files = np.zeros(k, dtype=np.uint32)
            d_slices = m.bao.slices_arena(ctx, d_src, zero, lens, provider["outboards"], files, chunks)["slices"]
            d_st = torch.empty(k, dtype=torch.int32, device="cuda")
            d_have = m.bao.have_new(lens)

            def plain():
                rc = L.b3w_bao_slice_ingest_device(ctx.handle, d_dst.data_ptr(), d_dst.numel(), zero.ctypes.data, lens.ctypes.data, 1, 0, d_obs.data_ptr(),
                                                   d_roots.data_ptr(), files.ctypes.data, chunks.ctypes.data, k, d_slices.data_ptr(), d_st.data_ptr(), s)
                assert rc == 0, ctx.last_error()

            def recording():
                rc = L.b3w_bao_slice_ingest_have_device(ctx.handle, d_dst.data_ptr(), d_dst.numel(), zero.ctypes.data, lens.ctypes.data, 1, 0, d_obs.data_ptr(),
                                                        d_roots.data_ptr(), files.ctypes.data, chunks.ctypes.data, k, d_slices.data_ptr(), d_st.data_ptr(),
                                                        d_have.data_ptr(), s)
                assert rc == 0, ctx.last_error()
            recording()
            torch.cuda.synchronize()
            bits = np.zeros(N, bool)
            bits[chunks.astype(np.int64)] = True
            assert not d_st.any().item()
            assert (d_have.cpu().numpy().view(np.uint64) == np.packbits(bits, bitorder="little").view(np.uint64)).all(), "the bitmap is not the slices' bits"
            for _ in range(3):
                plain()
                recording()
            t = alternating({"plain_a": plain, "recording": recording, "plain_b": plain})
            row = dict(slices=k, checked=True, plain=stats(t["plain_a"] + t["plain_b"]), plain_a=stats(t["plain_a"]), plain_b=stats(t["plain_b"]),
                       recording=stats(t["recording"]))
            row["spread_ms"] = abs(row["plain_a"]["ms"] - row["plain_b"]["ms"])
            row["recording_over_plain"] = row["recording"]["ms"] / row["plain"]["ms"]
            res["cases"][f"ingest_{k}"] = row
            print(f"ingest_{k}", json.dumps(row), flush=True)
            del d_slices
        del d_src, d_dst, d_obs, provider
    # ---- runs
    one = np.array([BM.GIB], dtype=np.uint64)
    small = np.full(262144, 4096, dtype=np.uint64)

    def missing_one_run(n):
        out = np.zeros(n, bool)
        out[n // 3:n // 3 + 5000] = True
        return out
    shapes = {"runs_1pct": (one, lambda n: rng.random(n) < 0.01), "runs_50pct": (one, lambda n: rng.random(n) < 0.5),
              "runs_one_run": (one, missing_one_run), "runs_small_files": (small, lambda n: rng.random(n) < 0.5)}
    for name, (lens, missing_of) in shapes.items():
        if want and name not in want:
            continue
        n_of = np.maximum(1, (lens + np.uint64(1023)) // np.uint64(1024)).astype(np.int64)
        total = int(n_of.sum())
        file_first = np.concatenate(([0], np.cumsum(n_of)))
        missing = missing_of(total)
        word_first = m.bao.have_layout(lens).astype(np.int64)
        # the bitmap as the ingests left it (files of 4 chunks: a word each, the chunks in its low bits)
        if lens.size == 1:
            words = np.packbits(~missing, bitorder="little").view(np.uint64)
        else:
            words = (~missing).reshape(-1, 4).astype(np.uint64) @ np.array([1, 2, 4, 8], dtype=np.uint64)
        assert words.size == int(word_first[-1])
        d_have = torch.from_numpy(words.view(np.int64).copy()).cuda()
        cap = m.bao.have_runs_bound(lens)
        d_f = torch.empty(cap, dtype=torch.int32, device="cuda")
        d_a, d_c = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda")
        d_n, d_h = torch.empty(1, dtype=torch.int64, device="cuda"), torch.empty(lens.size, dtype=torch.int64, device="cuda")
        need = L.b3w_bao_have_runs_scratch_bytes(lens.ctypes.data, lens.size)
        d_s = torch.empty(need, dtype=torch.uint8, device="cuda")
        got = {}

        def device():
            rc = L.b3w_bao_have_runs_device(ctx.handle, d_have.data_ptr(), lens.ctypes.data, lens.size, 0, 0, cap, d_f.data_ptr(), d_a.data_ptr(), d_c.data_ptr(),
                                            d_n.data_ptr(), d_h.data_ptr(), d_s.data_ptr(), need, s)
            assert rc == 0, ctx.last_error()
            n = int(d_n.item())
            got["rows"] = (d_f[:n].cpu().numpy().view(np.uint32), d_a[:n].cpu().numpy().view(np.uint64), d_c[:n].cpu().numpy().view(np.uint64))
        # the host's side: the map before the last ingest, that ingest's samples and their statuses on the device
        present = np.nonzero(~missing)[0]
        last = rng.permutation(present)[:LAST_INGEST]
        before = ~missing
        before[last] = False
        d_status = torch.zeros(last.size, dtype=torch.int32, device="cuda")

        def host():
            have_map = before.copy()                    # (the copy stands in for the map's state before this ingest: 1 byte a chunk)
            got["host"] = host_rows(have_map, file_first, d_status, last)
        device()
        host()
        assert all((x == y).all() for x, y in zip(got["rows"], got["host"])) and got["rows"][0].size == got["host"][0].size, name
        for _ in range(3):
            device()
            host()
        t = alternating({"host_a": host, "device": device, "host_b": host})
        row = dict(files=int(lens.size), chunks=total, words=int(word_first[-1]), missing_chunks=int(missing.sum()), runs=int(got["rows"][0].size),
                   last_ingest_samples=int(last.size), checked=True, host=stats(t["host_a"] + t["host_b"]), host_a=stats(t["host_a"]), host_b=stats(t["host_b"]),
                   device=stats(t["device"]))
        row["spread_ms"] = abs(row["host_a"]["ms"] - row["host_b"]["ms"])
        row["device_over_host"] = row["device"]["ms"] / row["host"]["ms"]

        def count_only():
            rc = L.b3w_bao_have_runs_device(ctx.handle, d_have.data_ptr(), lens.ctypes.data, lens.size, 0, 0, 0, None, None, None, d_n.data_ptr(), d_h.data_ptr(),
                                            d_s.data_ptr(), need, s)
            assert rc == 0, ctx.last_error()
            return int(d_n.item())
        assert count_only() == row["runs"]
        row["device_count_only"] = stats(alternating({"count": count_only})["count"])
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_have_measure.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
