#!/usr/bin/env python3
"""tools/bao_ingest_measure.py <out_dir> [--parent-lib libb3wit.so] [--cases a,b,...] — verified slices taken into a resident file and its
outboard (b3w_bao_slice_ingest_device) against the only device route that decoded slices before it: b3w_sample_plan_slices_device, which
verifies the same slices, writes step records nobody here asked for, places no byte and keeps no node.

  yardstick   b3w_sample_plan_slices_device of the library given with --parent-lib (a build of the commit before the ingest call, loaded
              beside this one; a nova context of its own) or, without it, of this library; over the same packed slices.
  method      tools/bao_verify_ranges_measure.py's: the routes alternating in one process, device events around each whole call (the
              host's table fill and upload included), medians over about a second a route.  The yardstick runs as two interleaved series
              A and B; |median A - median B| is the spread a difference has to exceed to mean anything.
  cases       one 1 GiB file; 4 096, 65 536 and 1 048 576 (every chunk) distinct slices into a file at a 16-byte aligned offset at g = 0;
              65 536 into a file at 1 modulo 16 (the narrow stores); 65 536 at g = 4; 65 536 and 4 096 with 16, 4 (and 1) lanes a sample
              (B3W_SLICE_INGEST_LANES); 4 096 through the host route: a loop of b3w_bao_slice_decode and one copy to the device.
  whole file  what taking the file in WHOLE costs instead: bao.outboard_batch and bao.verify_batch over the resident 1 GiB.
  checked     before a case is timed the slices go into buffers of 0xEE: every status is 0, the listed chunks' bytes are the source's,
              and every outboard node that was written is the provider's (every chunk listed: the whole outboard is).
  gate        65 536 slices, aligned, g = 0: the ingest call's median is at most the yardstick's plus the yardstick's spread.
Writes <out_dir>/bao_ingest_measure.json."""
import argparse, ctypes, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats

m = __import__("hot-proofs-blake3-circom_amd")

FILL = 0xEE
N = BM.GIB // 1024
# name -> (slices, the file's offset in the receiver's arena, group_log, B3W_SLICE_INGEST_LANES or None)
CASES = {"4096": (4096, 0, 0, None), "65536": (65536, 0, 0, None), "1048576_all": (N, 0, 0, None), "65536_offset1": (65536, 1, 0, None),
         "65536_g4": (65536, 0, 4, None), "65536_lanes16": (65536, 0, 0, "16"), "65536_lanes4": (65536, 0, 0, "4"), "65536_lanes1": (65536, 0, 0, "1"),
         "4096_lanes16": (4096, 0, 0, "16"), "4096_lanes4": (4096, 0, 0, "4")}


def parent_library(path):
    """the yardstick library and a nova_vesta context of its own -> (lib, ctx handle)"""
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    P.b3w_sample_plan_slices_device.restype, P.b3w_sample_plan_slices_device.argtypes = i32, [vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp]
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default="", help="libb3wit.so built from the commit before the ingest call: the yardstick")
    ap.add_argument("--cases", default="", help="comma-separated subset of the case names (host_4096 and whole_file among them)")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    if a.parent_lib:
        Y, y_ctx = parent_library(a.parent_lib)
        yard = f"b3w_sample_plan_slices_device of {os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff}), loaded beside this library"
    else:
        Y, y_ctx = L, ctx.handle
        yard = "b3w_sample_plan_slices_device of this library"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_src = torch.randint(0, 256, (BM.GIB,), dtype=torch.uint8, device="cuda", generator=gen)
    d_dst = torch.empty(BM.GIB + 16, dtype=torch.uint8, device="cuda")
    lens, zero = np.array([BM.GIB], dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    provider = {0: m.bao.outboard_batch(ctx, d_src, zero, lens)}
    d_roots = provider[0]["roots"]
    root_host = d_roots.cpu().numpy().view(np.uint32).reshape(8).copy()
    res = dict(device=torch.cuda.get_device_name(0), file_bytes=BM.GIB, yardstick=yard, cases={})
    want = [x for x in a.cases.split(",") if x]
    rng = np.random.default_rng(20)
    for name, (k, offset, gl, lanes) in CASES.items():
        if want and name not in want:
            continue
        if gl not in provider:
            provider[gl] = m.bao.outboard_groups_batch(ctx, d_src, zero, lens, gl)
        chunks = rng.permutation(N)[:k].astype(np.uint64)                  # distinct, in no order
        files = np.zeros(k, dtype=np.uint32)
        d_slices = m.bao.slices_arena(ctx, d_src, zero, lens, provider[0]["outboards"], files, chunks)["slices"]
        offs = np.array([offset], dtype=np.uint64)
        d_obs = torch.empty(m.bao.group_outboard_size(BM.GIB, gl), dtype=torch.uint8, device="cuda")
        d_st = torch.empty(k, dtype=torch.int32, device="cuda")
        rows = int(m.bao.sample_rows_batch(lens, files, chunks)[-1])
        d_recs = torch.empty((rows, 32), dtype=torch.int32, device="cuda")
        y_st = torch.empty(k, dtype=torch.int32, device="cuda")
        if lanes is None:
            os.environ.pop("B3W_SLICE_INGEST_LANES", None)
        else:
            os.environ["B3W_SLICE_INGEST_LANES"] = lanes

        def yardstick():
            rc = Y.b3w_sample_plan_slices_device(y_ctx, lens.ctypes.data, 1, d_roots.data_ptr(), files.ctypes.data, chunks.ctypes.data, k, d_slices.data_ptr(),
                                                 d_recs.data_ptr(), y_st.data_ptr(), s)
            assert rc == 0, rc

        def ingest():
            rc = L.b3w_bao_slice_ingest_device(ctx.handle, d_dst.data_ptr(), d_dst.numel(), offs.ctypes.data, lens.ctypes.data, 1, gl, d_obs.data_ptr(),
                                               d_roots.data_ptr(), files.ctypes.data, chunks.ctypes.data, k, d_slices.data_ptr(), d_st.data_ptr(), s)
            assert rc == 0, ctx.last_error()
        # the check: into buffers of 0xEE; the statuses, the listed chunks' bytes and the nodes that were written against the provider's
        d_dst.fill_(FILL)
        d_obs.fill_(FILL)
        d_st.fill_(-1)
        yardstick()
        ingest()
        torch.cuda.synchronize()
        assert not d_st.any().item() and not y_st.any().item(), name
        ids = torch.from_numpy(chunks.astype(np.int64)).cuda()
        assert torch.equal(d_dst[offset:offset + BM.GIB].view(N, 1024)[ids], d_src.view(N, 1024)[ids]), f"{name}: the chunks taken in are not the source's"
        assert bool((d_dst[:offset] == FILL).all().item()) and bool((d_dst[offset + BM.GIB:] == FILL).all().item())
        got, prov = d_obs[8:].view(-1, 64), provider[gl]["outboards"][8:d_obs.numel()].view(-1, 64)
        written = (got != FILL).any(dim=1)
        n_written = int(written.sum().item())
        assert torch.equal(d_obs[:8], provider[gl]["outboards"][:8]) and torch.equal(got[written], prov[written]), f"{name}: a node taken in is not the provider's"
        assert n_written == got.shape[0] if k == N else n_written >= (k >> gl) // 2, (name, n_written)
        P = (m.bao.slice_size(BM.GIB, 0) - 8 - 1024) // 64
        row = dict(slices=k, file_offset=offset, group_log=gl, lanes_env=lanes, slice_bytes=int(d_slices.numel()), nodes_written=n_written,
                   yardstick_record_bytes=rows * 128, stored_bytes_about=k * 1024 + n_written * 64, path_len_chunk0=P, checked=True)
        for _ in range(3):
            yardstick()
            ingest()
        t = alternating({"yard_a": yardstick, "ingest": ingest, "yard_b": yardstick})
        row.update(yardstick=stats(t["yard_a"] + t["yard_b"]), yardstick_a=stats(t["yard_a"]), yardstick_b=stats(t["yard_b"]), ingest=stats(t["ingest"]))
        row["yardstick_spread_ms"] = abs(row["yardstick_a"]["ms"] - row["yardstick_b"]["ms"])
        row["ingest_minus_yardstick_ms"] = row["ingest"]["ms"] - row["yardstick"]["ms"]
        row["ingest_over_yardstick"] = row["ingest"]["ms"] / row["yardstick"]["ms"]
        row["ingest_within_yardstick_plus_spread"] = row["ingest"]["ms"] <= row["yardstick"]["ms"] + row["yardstick_spread_ms"]
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del d_slices, d_recs, d_obs, ids, got, prov, written
    os.environ.pop("B3W_SLICE_INGEST_LANES", None)
    if not want or "host_4096" in want:                                    # the route a receiver had: the host decoder a slice at a time, one copy
        k = 4096
        chunks = rng.permutation(N)[:k].astype(np.uint64)
        files = np.zeros(k, dtype=np.uint32)
        out = m.bao.slices_arena(ctx, d_src, zero, lens, provider[0]["outboards"], files, chunks)
        host, sf = out["slices"].cpu().numpy(), out["slice_first"]
        slices = [host[int(sf[i]):int(sf[i]) + m.bao.slice_size(BM.GIB, int(c))].tobytes() for i, c in enumerate(chunks)]
        staging = torch.empty(k * 1024, dtype=torch.uint8).pin_memory()
        d_in = torch.empty(k * 1024, dtype=torch.uint8, device="cuda")
        base = staging.data_ptr()
        cnt, st = ctypes.c_uint32(), ctypes.c_int32()

        def host_route():
            for i, (c, sl) in enumerate(zip(chunks.tolist(), slices)):
                rc = L.b3w_bao_slice_decode(sl, len(sl), BM.GIB, c, root_host.ctypes.data, base + i * 1024, ctypes.byref(cnt), ctypes.byref(st))
                assert rc == 0 and st.value == 0 and cnt.value == 1024
            d_in.copy_(staging, non_blocking=True)
        host_route()
        torch.cuda.synchronize()
        ids = torch.from_numpy(chunks.astype(np.int64)).cuda()
        assert torch.equal(d_in.view(k, 1024), d_src.view(N, 1024)[ids])
        row = dict(slices=k, route="a Python loop of b3w_bao_slice_decode into pinned memory and one copy to the device; the bytes are not yet at their places and no node is kept")
        row["host"] = stats(alternating({"host": host_route})["host"])
        res["cases"]["host_4096"] = row
        print("host_4096", json.dumps(row), flush=True)
    if not want or "whole_file" in want:                                   # the file received whole instead: hash it where it lies
        def whole_outboard():
            m.bao.outboard_batch(ctx, d_src, zero, lens)

        def whole_verify():
            m.bao.verify_batch(ctx, d_src, zero, lens, provider[0]["outboards"], d_roots)
        for fn in (whole_outboard, whole_verify):
            for _ in range(3):
                fn()
        t = alternating({"outboard_batch": whole_outboard, "verify_batch": whole_verify})
        row = dict(note="the Python calls, their output buffers allocated inside the timed call; the 1 GiB is resident, its transfer is not in these figures",
                   outboard_batch=stats(t["outboard_batch"]), verify_batch=stats(t["verify_batch"]))
        res["cases"]["whole_file"] = row
        print("whole_file", json.dumps(row), flush=True)
    g = res["cases"].get("65536")
    if g:
        res["gate"] = dict(case="65536", passed=bool(g["ingest_within_yardstick_plus_spread"]), yardstick_ms=g["yardstick"]["ms"], ingest_ms=g["ingest"]["ms"],
                           spread_ms=g["yardstick_spread_ms"])
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_ingest_measure.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
