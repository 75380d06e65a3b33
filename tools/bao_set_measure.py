#!/usr/bin/env python3
"""tools/bao_set_measure.py <out_dir> [--parent-lib libb3wit.so] [--cases a,b,...] — set slices (b3w_bao_set_slice_arena_device,
b3w_bao_set_slice_ingest_device) against the two ways the library before them serves and takes in the missing runs of a file.

  yardsticks  of the library given with --parent-lib (a build of the parent commit, loaded beside this one, a context of its own) or,
              without it, of this library: RANGE, one slice a run (b3w_bao_range_slice_arena_device, b3w_bao_range_slice_ingest_device),
              and ONE-CHUNK, one slice a chunk (bao.runs_chunks inside the timed provider call, b3w_bao_slice_arena_device,
              b3w_bao_slice_ingest_have_device over the chunk list made beforehand).
  method      tools/bao_range_measure.py's: the routes alternating in one process, device events around each whole C call (the host's
              table fill and upload included), medians over about a second a route, the three routes' results compared before timing.
              Each yardstick runs as two interleaved series A and B; |median A - median B| is the spread a difference has to exceed.
  cases       one 1 GiB file: the runs of a bitmap with half its chunks missing (262 507 runs), 65 536 runs of 1 chunk, 4 096 runs of
              16, 64 runs of 1 024 chunks at starts that are not tile-aligned, and the last again at g = 4.
  expectation on the half-missing shape both new calls beat the FASTER of the two yardsticks by more than that yardstick's spread;
              recorded as met or not.  No profiler is run.
Writes <out_dir>/bao_set_measure.json."""
import argparse, ctypes, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats
from bao_range_measure import runs_64x1024, runs_half_missing, runs_of

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
    P.b3w_bao_range_slice_arena_device.restype, P.b3w_bao_range_slice_arena_device.argtypes = i32, [vp, vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, u32, vp, vp]
    P.b3w_bao_range_slice_ingest_device.restype = i32
    P.b3w_bao_range_slice_ingest_device.argtypes = [vp, vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, u64, vp]
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


def sorted_runs(make):
    def f(rng):
        first, count = make(rng)
        order = np.argsort(first)
        return first[order], count[order]
    return f


# name -> (the runs, ascending, group_log)
CASES = {"half_missing": (runs_half_missing, 0), "65536x1": (sorted_runs(lambda rng: runs_of(rng, 65536, 1)), 0),
         "4096x16": (sorted_runs(lambda rng: runs_of(rng, 4096, 16)), 0), "64x1024": (runs_64x1024, 0), "64x1024_g4": (runs_64x1024, 4)}


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
        yard = "this library's range and one-chunk calls"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_src = torch.empty(BM.GIB + 16, dtype=torch.uint8, device="cuda")
    d_src[:] = torch.randint(0, 256, (BM.GIB + 16,), dtype=torch.uint8, device="cuda", generator=gen)
    dst = {k: torch.empty(BM.GIB + 16, dtype=torch.uint8, device="cuda") for k in ("set", "range", "one")}
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
        lay = m.bao.set_slice_layout(lens, files, first, count)
        sf = {"set": int(lay["slice_first"][-1]), "range": int(m.bao.range_slice_layout(lens, files, first, count)[-1]),
              "one": int(m.bao.slice_layout(lens, c_files, chunks)[-1])}
        slices = {r: torch.empty(b, dtype=torch.uint8, device="cuda") for r, b in sf.items()}
        obs = {r: torch.empty(m.bao.group_outboard_size(BM.GIB, gl), dtype=torch.uint8, device="cuda") for r in dst}
        have = {r: m.bao.have_new(lens) for r in dst}
        st = {"set": torch.empty(1, dtype=torch.int32, device="cuda"), "range": torch.empty(k, dtype=torch.int32, device="cuda"),
              "one": torch.empty(n_chunks, dtype=torch.int32, device="cuda")}
        fb = {"set": torch.empty(1, dtype=torch.int64, device="cuda"), "range": torch.empty(k, dtype=torch.int64, device="cuda")}
        d_cs = torch.empty(n_chunks, dtype=torch.int32, device="cuda")
        args = (lens.ctypes.data, 1, files.ctypes.data, first.ctypes.data, count.ctypes.data, k)
        need = {"set": L.b3w_bao_set_slice_ingest_scratch_bytes(*args), "range": L.b3w_bao_range_slice_ingest_scratch_bytes(*args)}
        scratch = {r: torch.empty(max(16, b), dtype=torch.uint8, device="cuda") for r, b in need.items()}
        ob = prov["outboards"].data_ptr()
        head = lambda h, d: (h, d.data_ptr(), d.numel(), offs.ctypes.data, lens.ctypes.data, 1, gl)

        def provide_set():
            assert L.b3w_bao_set_slice_arena_device(*head(ctx.handle, d_src), ob, files.ctypes.data, first.ctypes.data, count.ctypes.data, k,
                                                    slices["set"].data_ptr(), s) == 0, ctx.last_error()

        def provide_range():
            assert Y.b3w_bao_range_slice_arena_device(*head(y_ctx, d_src), ob, files.ctypes.data, first.ctypes.data, count.ctypes.data, k,
                                                      slices["range"].data_ptr(), s) == 0

        def provide_one():
            fi, ch = m.bao.runs_chunks(files, first, count)
            assert Y.b3w_bao_slice_arena_device(*head(y_ctx, d_src), ob, fi.ctypes.data, ch.ctypes.data, ch.size, slices["one"].data_ptr(), s) == 0

        def ingest_set():
            assert L.b3w_bao_set_slice_ingest_device(*head(ctx.handle, dst["set"]), obs["set"].data_ptr(), d_roots.data_ptr(), files.ctypes.data, first.ctypes.data,
                                                     count.ctypes.data, k, slices["set"].data_ptr(), st["set"].data_ptr(), fb["set"].data_ptr(), d_cs.data_ptr(),
                                                     have["set"].data_ptr(), scratch["set"].data_ptr(), scratch["set"].numel(), s) == 0, ctx.last_error()

        def ingest_range():
            assert Y.b3w_bao_range_slice_ingest_device(*head(y_ctx, dst["range"]), obs["range"].data_ptr(), d_roots.data_ptr(), files.ctypes.data,
                                                       first.ctypes.data, count.ctypes.data, k, slices["range"].data_ptr(), st["range"].data_ptr(),
                                                       fb["range"].data_ptr(), have["range"].data_ptr(), scratch["range"].data_ptr(), scratch["range"].numel(), s) == 0

        def ingest_one():
            assert Y.b3w_bao_slice_ingest_have_device(*head(y_ctx, dst["one"]), obs["one"].data_ptr(), d_roots.data_ptr(), c_files.ctypes.data, chunks.ctypes.data,
                                                      n_chunks, slices["one"].data_ptr(), st["one"].data_ptr(), have["one"].data_ptr(), s) == 0
        # the check: the three routes into buffers of 0xEE give the same arena, outboard and bitmap; the chunks are the source's
        for r in dst:
            dst[r].fill_(FILL)
            obs[r].fill_(FILL)
            have[r].zero_()
        for fn in (provide_set, provide_range, provide_one, ingest_set, ingest_range, ingest_one):
            fn()
        torch.cuda.synchronize()
        assert not any(t.any().item() for t in st.values()) and not d_cs.any().item() and all(bool((t == -1).all().item()) for t in fb.values()), name
        for r in ("range", "one"):
            assert torch.equal(dst["set"], dst[r]) and torch.equal(obs["set"], obs[r]) and torch.equal(have["set"], have[r]), f"{name}: set and {r} differ"
        ids = torch.from_numpy(chunks.astype(np.int64)).cuda()
        assert torch.equal(dst["set"][:BM.GIB].view(N, 1024)[ids], d_src[:BM.GIB].view(N, 1024)[ids]), name
        assert int((dst["set"][:BM.GIB].view(N, 1024) != FILL).any(dim=1).sum().item()) == n_chunks
        row = dict(runs=k, chunks=n_chunks, group_log=gl, payload_bytes=n_chunks * 1024, set_slice_bytes=sf["set"], range_slice_bytes=sf["range"],
                   one_chunk_slice_bytes=sf["one"], set_rows=need["set"] // 16, range_rows=need["range"] // 16, checked=True)
        for _ in range(3):
            for fn in (provide_range, provide_one, provide_set, ingest_range, ingest_one, ingest_set):
                fn()
        for what, new, rng_fn, one_fn in (("provider", provide_set, provide_range, provide_one), ("receiver", ingest_set, ingest_range, ingest_one)):
            t = alternating({"range_a": rng_fn, "one_a": one_fn, "new": new, "range_b": rng_fn, "one_b": one_fn})
            r = dict(new=stats(t["new"]))
            for y in ("range", "one"):
                r[y] = stats(t[y + "_a"] + t[y + "_b"])
                r[y + "_spread_ms"] = abs(stats(t[y + "_a"])["ms"] - stats(t[y + "_b"])["ms"])
                r["new_over_" + y] = r["new"]["ms"] / r[y]["ms"]
            best = min(("range", "one"), key=lambda y: r[y]["ms"])
            r["faster_yardstick"] = best
            r["new_below_faster_yardstick_by_more_than_its_spread"] = bool(r[best]["ms"] - r["new"]["ms"] > r[best + "_spread_ms"])
            row[what] = r
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del slices, obs, ids, st, fb, d_cs, scratch
    h = res["cases"].get("half_missing")
    if h:
        res["expectation"] = dict(case="half_missing", what="both new calls beat the faster of the two existing routes by more than that route's spread",
                                  met=bool(h["provider"]["new_below_faster_yardstick_by_more_than_its_spread"] and
                                           h["receiver"]["new_below_faster_yardstick_by_more_than_its_spread"]),
                                  provider={k: h["provider"][k] if k.endswith("ms") or k == "faster_yardstick" else h["provider"][k]["ms"]
                                            for k in ("new", "range", "one", "range_spread_ms", "one_spread_ms", "faster_yardstick")},
                                  receiver={k: h["receiver"][k] if k.endswith("ms") or k == "faster_yardstick" else h["receiver"][k]["ms"]
                                            for k in ("new", "range", "one", "range_spread_ms", "one_spread_ms", "faster_yardstick")})
    res["not_taken"] = "files past 1 GiB; many files a call; per-kernel times (no profiler was run); the host's table fill apart from the launches"
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_set_measure.json"), "w"), indent=1)
    print(json.dumps(res.get("expectation"), indent=1))


if __name__ == "__main__":
    main()
