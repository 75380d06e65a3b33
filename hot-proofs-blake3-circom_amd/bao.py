"""Bao outboards and challenged chunk paths (b3w_bao_* / b3w_sample_*).

A data-availability challenge names a few chunk indices; the provider answers from the file and its bao outboard (the tree's
parent nodes, kept beside the file).  outboard() makes the outboard of a preimage in device memory; plan_samples() plans the step
records of the challenged chunk paths from the outboard and those chunks' bytes alone, verifying each path against the root;
prove_samples() runs their witnesses, constraint checks and commitments through the batch calls, batch by batch.  outboard_batch(),
plan_samples_batch() and prove_samples_batch() do the same for a whole batch of files of one device arena at once;
outboard_groups_batch(), plan_samples_groups_batch() and prove_samples_groups_batch() keep the outboards over chunk groups of
2^group_log chunks, 2^group_log times smaller, and recompute the levels inside a group from the group's bytes.  slices_batch() extracts the standard bao slices of challenged chunks from either kind
of outboard and plan_samples_slices() / prove_samples_slices() plan and prove from slices alone, so the prover need not hold the
outboards (decode_slice(): the host decoder).  plan_samples_arena() / prove_samples_arena() / slices_arena() are the provider's calls
without the gather: the sampled bytes are read where the files lie in the arena outboard_batch() took, at any byte offset.  verify_batch() is bao's decoder over whole files: every chunk (or chunk group) of
every file of a batch held against its outboard and root on the device, a status per unit (verify_host(): one file on the host).  StreamOutboard / StreamVerify take ONE file window by window (whole MiB, any order, any
stream) with the batch calls' results, and outboard_stream() / verify_stream() feed them from host memory or a reader through a ring
of windows: the file need never be resident on the device.  StreamOutboardOpen / outboard_stream_open() do the same for a file whose
LENGTH IS NOT KNOWN until its last byte (an upper bound instead): full MiB are hashed as they come into a staging area, and finish(),
which learns the length, moves them to their places in the outboard.  open_finish_many() ends many such sessions in one call of at
most four launches, and outboard_stream_open_many() keeps `lanes` sources of unknown length in flight with it.
outboard_update_batch() updates outboards and roots IN PLACE after writes into resident files, from the dirty chunk ranges alone
(chunk_ranges() makes them from byte ranges; update_host(): one file on the host).
verify_ranges_batch() is verify_batch() for the units that hold listed chunk ranges alone: only those are hashed, only the nodes above
them read, only their status bytes written, plus a status and a first bad unit per range (verify_ranges_host(): one file on the host).
ingest_slices() is the receiver's side of slices: slices verified against the roots on the device, the verified ones' chunks put at
their places in the arena and their path nodes at their places in the outboards (ingest_slice_host(): one slice on the host).
have_new() / ingest_slices(d_have=) keep a bitmap of the chunks that have arrived on the device, have_runs() turns it into the
missing (or present) chunk runs of every file and have_from_status() rebuilds it from verify_batch's statuses after a restart
(have_runs_host(), have_from_status_host(): one file on the host; runs_chunks(): the runs as sample lists).
ingest_slices_packed() / ingest_range_slices_packed() / ingest_set_slices_packed() are the receivers for files that are NOT resident:
the verified chunks go to one 1 024-byte slot each, in the order of the statuses (chunk_slots(): where each slot belongs in its file;
scatter_chunks(): the verified slots written there after the copy to the host), with the arena receivers' statuses, outboards and
bitmap - or, with d_outboards=None, nothing but the verified bytes: bao's decode on the device.
outboard_diff() names the chunks two versions of a file share from their outboards alone, as a bitmap in the arrival bitmap's layout:
a replica with a stale copy fetches only what have_runs() then lists as missing (diff_host(): one pair on the host).
outboard_delta() / apply_outboard_delta() serve and take in the nodes of a new version's outboard that a replica does not hold: a blob
per pair of files, verified against the new root node by node before the replica's outboard is written (delta_host() /
apply_delta_host(): one pair on the host; delta_bound() / delta_layout(): the sizes); outboard_check() holds whole outboards against
their roots without the files.
The records are
word for word those the chain planner writes for the same chunks (ChainPlanner.plan), so every step is the reference's
prove_chunk_hash step (rust_fold/src/main.rs:41-203 over hash_with_path's slice, rust_fold/src/blake3_hash.rs:17-93)."""
import ctypes

import numpy as np
import torch

from . import B3W_OK, B3WError, BodyBuffer, lib

STATUS = {0: "verified", 1: "chunk bytes do not match", 2: "a path node or the root does not match", 3: "outboard header is not the length"}


def _chk(ctx, rc, what):
    if rc != B3W_OK:
        raise B3WError(rc, f"{what}: status {rc}: {ctx.last_error() if ctx is not None else ''}")


def _stream(stream):
    return stream or torch.cuda.current_stream().cuda_stream


def num_chunks(length):
    return max(1, (length + 1023) // 1024)


def outboard_size(length):
    return lib().b3w_bao_outboard_size(length)


def outboard(ctx, d_preimage, stream=0):
    """-> (uint8 CUDA tensor: the bao outboard, root words as uint32 numpy [8] = BLAKE3(preimage)).
    d_preimage: a uint8 CUDA tensor (the device-resident case this is built for), or host bytes — those are copied to the device
    first, and for a large file that copy takes far longer than the outboard itself (outboard_stream hashes behind the copy, a window
    at a time, without the file ever being resident)."""
    if not isinstance(d_preimage, torch.Tensor):
        d_preimage = torch.from_numpy(np.frombuffer(bytes(d_preimage), dtype=np.uint8).copy()).cuda()
    assert d_preimage.is_cuda and d_preimage.dtype == torch.uint8 and d_preimage.is_contiguous()
    length = d_preimage.numel()
    n = num_chunks(length)
    dev = d_preimage.device
    ob = torch.empty(outboard_size(length), dtype=torch.uint8, device=dev)
    levels = torch.empty((2 * n + 64) * 8, dtype=torch.int32, device=dev)
    root = torch.empty(8, dtype=torch.int32, device=dev)
    _chk(ctx, lib().b3w_bao_outboard_device(ctx.handle, d_preimage.data_ptr() if length else None, length, ob.data_ptr(), levels.data_ptr(),
                                             root.data_ptr(), _stream(stream)), "b3w_bao_outboard_device")
    return ob, root.cpu().numpy().view(np.uint32).copy()


def path_nodes(chunk, n_chunks):
    """pre-order indices of the chunk's path nodes, root first (node i: outboard bytes [8 + 64 i, 8 + 64 i + 64))"""
    out = (ctypes.c_uint64 * 64)()
    cnt = ctypes.c_uint32()
    _chk(None, lib().b3w_bao_path_nodes(chunk, n_chunks, out, ctypes.byref(cnt)), "b3w_bao_path_nodes")
    return list(out[:cnt.value])


def slice_chunk(outboard_bytes, length, chunk, chunk_bytes):
    """the bao slice of one chunk (header, path nodes root first, the chunk's bytes) from a host outboard"""
    ob = outboard_bytes.cpu().numpy().tobytes() if isinstance(outboard_bytes, torch.Tensor) else bytes(outboard_bytes)
    cb = bytes(chunk_bytes)
    ln = ctypes.c_uint64()
    _chk(None, lib().b3w_bao_slice(ob, length, chunk, cb, None, ctypes.byref(ln)), "b3w_bao_slice")
    out = ctypes.create_string_buffer(ln.value)
    _chk(None, lib().b3w_bao_slice(ob, length, chunk, cb, out, ctypes.byref(ln)), "b3w_bao_slice")
    return out.raw


def sample_rows(length, chunks):
    """-> row_first (numpy uint64 [n_samples + 1]): sample s owns rows [row_first[s], row_first[s + 1])"""
    ch = np.ascontiguousarray(chunks, dtype=np.uint64)
    rf = np.zeros(ch.size + 1, dtype=np.uint64)
    total = lib().b3w_sample_rows(length, ch.ctypes.data, ch.size, rf.ctypes.data)
    if total < 0:
        raise B3WError(-total, "b3w_sample_rows: a chunk index is not below the chunk count")
    return rf


def chunk_bytes(preimage, chunks, device="cuda"):
    """the sampled chunks' bytes as plan_samples takes them (uint8 [n_samples, 1024], zero past the end): what a provider reads
    from its file for a challenge.  preimage: host bytes / numpy, or a CUDA tensor."""
    ch = [int(c) for c in chunks]
    if isinstance(preimage, torch.Tensor):
        pad = torch.zeros(num_chunks(preimage.numel()) * 1024, dtype=torch.uint8, device=preimage.device)
        pad[:preimage.numel()] = preimage
        return pad.view(-1, 1024)[torch.tensor(ch, dtype=torch.long, device=preimage.device)].contiguous()
    data = np.frombuffer(bytes(preimage), dtype=np.uint8)
    out = np.zeros((len(ch), 1024), dtype=np.uint8)
    for s, c in enumerate(ch):
        part = data[c * 1024:c * 1024 + 1024]
        out[s, :part.size] = part
    return torch.from_numpy(out).to(device)


def plan_samples(ctx, d_outboard, length, root, chunks, d_chunk_bytes, stream=0):
    """The step records of the challenged chunk paths, from the outboard and the sampled chunks' bytes alone.  Returns a dict:
    records (int32 CUDA [rows, 32], sample-major: each sample's leaf blocks, then its parent steps bottom up), row_first (numpy
    [n_samples + 1]), sample_status (numpy int32: 0 verified, 1 chunk bytes, 2 a path node or the root, 3 the header — STATUS),
    provable (numpy bool: the reference's fold of that path ends in the root, b3w_chain_path_provable)."""
    L = lib()
    ch = np.ascontiguousarray(chunks, dtype=np.uint64)
    rf = sample_rows(length, ch)
    dev = d_outboard.device
    assert d_chunk_bytes.is_cuda and d_chunk_bytes.dtype == torch.uint8 and d_chunk_bytes.numel() >= ch.size * 1024
    recs = torch.empty((int(rf[-1]), 32), dtype=torch.int32, device=dev)
    st = torch.full((ch.size,), -1, dtype=torch.int32, device=dev)
    rw = np.ascontiguousarray(root, dtype=np.uint32)
    _chk(ctx, L.b3w_sample_plan_device(ctx.handle, length, d_outboard.data_ptr(), rw.ctypes.data, ch.ctypes.data, ch.size,
                                       d_chunk_bytes.data_ptr(), recs.data_ptr(), st.data_ptr(), _stream(stream)), "b3w_sample_plan_device")
    n = num_chunks(length)
    provable = np.array([bool(L.b3w_chain_path_provable(int(c), n)) for c in ch], dtype=bool)
    return dict(records=recs, row_first=rf, sample_status=st.cpu().numpy(), provable=provable)


def prove_samples(ctx, d_outboard, length, root, chunks, d_chunk_bytes, batch_steps=4096, consumer=None, commit_key=None, r1cs=None,
                  stream=0):
    """plan_samples, then every row's witness through ONE body buffer of batch_steps bodies: per batch the witness kernel
    (b3w_batch_run_device), the constraint check (r1cs), the commitments from the records (commit_key) and
    consumer(d_bodies [count, body_bytes] uint8 view, pitch, first_row, count).  With a commit_key and neither consumer nor r1cs
    no bodies are written at all: the commitments come from the records alone (as b3w_chain_commit_only).
    Returns plan_samples' dict plus public (int32 CUDA [rows, 15]), status (int32 CUDA [rows]), violations (int32 CUDA [rows] or
    None) and points (uint8 CUDA [rows, 64] or None)."""
    s = _stream(stream)
    out = plan_samples(ctx, d_outboard, length, root, chunks, d_chunk_bytes, stream=s)
    return _prove_planned(ctx, out, batch_steps, consumer, commit_key, r1cs, s)


def _prove_planned(ctx, out, batch_steps, consumer, commit_key, r1cs, s):
    """the batch loop of prove_samples / prove_samples_batch over a plan's records; adds public, status, violations, points to `out`"""
    recs = out["records"]
    rows = recs.shape[0]
    dev = recs.device
    pub = torch.zeros((rows, ctx.public_words), dtype=torch.int32, device=dev)
    status = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    viol = torch.full((rows,), -1, dtype=torch.int32, device=dev) if r1cs is not None else None
    points = torch.zeros((rows, 64), dtype=torch.uint8, device=dev) if commit_key is not None else None
    bodies_needed = consumer is not None or r1cs is not None or commit_key is None
    body = ctx.body_bytes
    buf = BodyBuffer(ctx, min(batch_steps, max(rows, 1)) * body) if bodies_needed and rows else None
    try:
        view = buf.tensor() if buf is not None else None
        for r0 in range(0, rows, batch_steps):
            k = min(batch_steps, rows - r0)
            d_rec = recs.data_ptr() + r0 * 128
            if commit_key is not None:
                commit_key.commit_records_device(d_rec, k, points.data_ptr() + r0 * 64, status.data_ptr() + r0 * 4,
                                                 0 if bodies_needed else pub.data_ptr() + r0 * ctx.public_words * 4, s)
            if not bodies_needed:
                continue
            ctx.run_device(d_rec, k, buf.ptr, 0, pub.data_ptr() + r0 * ctx.public_words * 4, status.data_ptr() + r0 * 4, s)
            if r1cs is not None:
                r1cs.check_device(buf.ptr, k, 0, viol.data_ptr() + r0 * 4, 0, s)
            if consumer is not None:
                consumer(view[:k * body].view(k, body), body, r0, k)
        torch.cuda.synchronize(dev)
    finally:
        if buf is not None:
            buf.free()
    out.update(public=pub, status=status, violations=viol, points=points)
    return out


# ---- a batch of files --------------------------------------------------------------------------------------------------
def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def batch_layout(lens):
    """-> ob_first (numpy uint64 [n_files + 1]): file f's outboard is bytes [ob_first[f], ob_first[f + 1]) of the packed outboards"""
    ln = _u64(lens)
    ob_first = np.zeros(ln.size + 1, dtype=np.uint64)
    lib().b3w_bao_batch_layout(ln.ctypes.data, ln.size, ob_first.ctypes.data)
    return ob_first


def outboard_batch(ctx, d_arena, offsets, lens, stream=0):
    """The outboards and roots of every file of a batch in a number of launches that does not depend on the file count: file f is
    bytes [offsets[f], offsets[f] + lens[f]) of d_arena (a uint8 CUDA tensor; any offsets).  Returns a dict: outboards (uint8 CUDA
    tensor, packed in file order), ob_first (numpy uint64 [n_files + 1]), roots (int32 CUDA tensor [n_files, 8], left on the device:
    plan_samples_batch takes them there)."""
    L = lib()
    off, ln = _u64(offsets), _u64(lens)
    assert off.size == ln.size
    assert d_arena.is_cuda and d_arena.dtype == torch.uint8 and d_arena.is_contiguous()
    if ln.size and int((off + ln).max()) > d_arena.numel():
        raise B3WError(100, "outboard_batch: a file reaches past the end of the arena")
    dev = d_arena.device
    ob_first = batch_layout(ln)
    obs = torch.empty(int(ob_first[-1]), dtype=torch.uint8, device=dev)
    roots = torch.empty((ln.size, 8), dtype=torch.int32, device=dev)
    need = L.b3w_bao_batch_scratch_bytes(ln.ctypes.data, ln.size)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    _chk(ctx, L.b3w_bao_outboard_batch_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, off.ctypes.data, ln.ctypes.data, ln.size,
                                              obs.data_ptr(), roots.data_ptr(), scratch.data_ptr() if need else None, need, _stream(stream)),
         "b3w_bao_outboard_batch_device")
    return dict(outboards=obs, ob_first=ob_first, roots=roots)


def chunk_bytes_batch(arena, offsets, lens, files, chunks, device="cuda"):
    """the sampled chunks' bytes as plan_samples_batch takes them (uint8 [n_samples, 1024], zero past a file's end); sample s is chunk
    chunks[s] of file files[s].  arena: host bytes / numpy, or a CUDA tensor."""
    off, ln = _u64(offsets).astype(np.int64), _u64(lens).astype(np.int64)
    fi, ch = np.asarray(files, dtype=np.int64), np.asarray(chunks, dtype=np.int64)
    start = off[fi] + ch * 1024
    count = np.clip(ln[fi] - ch * 1024, 0, 1024)
    if isinstance(arena, torch.Tensor):
        dev = arena.device
        col = torch.arange(1024, device=dev)
        idx = torch.from_numpy(start).to(dev)[:, None] + col[None, :]
        live = col[None, :] < torch.from_numpy(count).to(dev)[:, None]
        if arena.numel() == 0:
            return torch.zeros((fi.size, 1024), dtype=torch.uint8, device=dev)
        got = arena[idx.clamp_(max=arena.numel() - 1)]
        return torch.where(live, got, torch.zeros((), dtype=torch.uint8, device=dev)).contiguous()
    data = np.frombuffer(bytes(arena), dtype=np.uint8) if not isinstance(arena, np.ndarray) else arena
    out = np.zeros((fi.size, 1024), dtype=np.uint8)
    for s in range(fi.size):
        out[s, :count[s]] = data[start[s]:start[s] + count[s]]
    return torch.from_numpy(out).to(device)


def sample_rows_batch(lens, files, chunks):
    """-> row_first (numpy uint64 [n_samples + 1]) of samples (files[s], chunks[s]), sample-major as sample_rows"""
    ln, ch = _u64(lens), _u64(chunks)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    assert fi.size == ch.size
    rf = np.zeros(ch.size + 1, dtype=np.uint64)
    total = lib().b3w_sample_rows_batch(ln.ctypes.data, ln.size, fi.ctypes.data, ch.ctypes.data, ch.size, rf.ctypes.data)
    if total < 0:
        raise B3WError(-total, "b3w_sample_rows_batch: a file index is not below the file count, or a chunk index not below its file's chunk count")
    return rf


def plan_samples_batch(ctx, d_outboards, lens, d_roots, files, chunks, d_chunk_bytes, stream=0):
    """plan_samples over a batch: sample s is chunk chunks[s] of file files[s]; d_outboards and d_roots as outboard_batch returns them
    (the roots stay on the device).  Returns the dict plan_samples returns, `provable` from each sample's own file."""
    L = lib()
    ln, ch = _u64(lens), _u64(chunks)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    rf = sample_rows_batch(ln, fi, ch)
    dev = d_outboards.device
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.numel() >= ln.size * 8
    assert d_chunk_bytes.is_cuda and d_chunk_bytes.dtype == torch.uint8 and d_chunk_bytes.numel() >= ch.size * 1024
    recs = torch.empty((int(rf[-1]), 32), dtype=torch.int32, device=dev)
    st = torch.full((ch.size,), -1, dtype=torch.int32, device=dev)
    _chk(ctx, L.b3w_sample_plan_batch_device(ctx.handle, ln.ctypes.data, ln.size, d_outboards.data_ptr(), d_roots.data_ptr(), fi.ctypes.data,
                                             ch.ctypes.data, ch.size, d_chunk_bytes.data_ptr(), recs.data_ptr(), st.data_ptr(), _stream(stream)),
         "b3w_sample_plan_batch_device")
    provable = np.array([bool(L.b3w_chain_path_provable(int(c), num_chunks(int(ln[f])))) for f, c in zip(fi, ch)], dtype=bool)
    return dict(records=recs, row_first=rf, sample_status=st.cpu().numpy(), provable=provable)


def prove_samples_batch(ctx, d_outboards, lens, d_roots, files, chunks, d_chunk_bytes, batch_steps=4096, consumer=None, commit_key=None,
                        r1cs=None, stream=0):
    """prove_samples over a batch of files: plan_samples_batch, then the same witness / constraint / commitment batches over its rows"""
    s = _stream(stream)
    out = plan_samples_batch(ctx, d_outboards, lens, d_roots, files, chunks, d_chunk_bytes, stream=s)
    return _prove_planned(ctx, out, batch_steps, consumer, commit_key, r1cs, s)


# ---- outboards over chunk groups ---------------------------------------------------------------------------------------
MAX_GROUP_LOG = 6
GROUP_STATUS = {**STATUS, 1: "the group's bytes do not match", 2: "a stored node or the root does not match"}


def group_outboard_size(length, group_log):
    """8 + 64 (n_groups - 1): the outboard over groups of 2^group_log chunks"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    return lib().b3w_bao_group_outboard_size(length, group_log)


def group_batch_layout(lens, group_log):
    """batch_layout for group outboards -> ob_first (numpy uint64 [n_files + 1])"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    ln = _u64(lens)
    ob_first = np.zeros(ln.size + 1, dtype=np.uint64)
    lib().b3w_bao_group_batch_layout(ln.ctypes.data, ln.size, group_log, ob_first.ctypes.data)
    return ob_first


def group_path_nodes(chunk, n_chunks, group_log):
    """indices in the group outboard of the stored part of the chunk's path, root first"""
    out = (ctypes.c_uint64 * 64)()
    cnt = ctypes.c_uint32()
    _chk(None, lib().b3w_bao_group_path_nodes(chunk, n_chunks, group_log, out, ctypes.byref(cnt)), "b3w_bao_group_path_nodes")
    return list(out[:cnt.value])


def outboard_groups_batch(ctx, d_arena, offsets, lens, group_log, stream=0):
    """outboard_batch writing group outboards (groups of 2^group_log chunks): the same dict, the outboards packed as
    group_batch_layout says; the roots are the files' BLAKE3 hashes as before."""
    L = lib()
    off, ln = _u64(offsets), _u64(lens)
    assert off.size == ln.size
    assert d_arena.is_cuda and d_arena.dtype == torch.uint8 and d_arena.is_contiguous()
    if ln.size and int((off + ln).max()) > d_arena.numel():
        raise B3WError(100, "outboard_groups_batch: a file reaches past the end of the arena")
    dev = d_arena.device
    ob_first = group_batch_layout(ln, group_log)
    obs = torch.empty(int(ob_first[-1]), dtype=torch.uint8, device=dev)
    roots = torch.empty((ln.size, 8), dtype=torch.int32, device=dev)
    need = L.b3w_bao_batch_scratch_bytes(ln.ctypes.data, ln.size)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    _chk(ctx, L.b3w_bao_group_outboard_batch_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, off.ctypes.data, ln.ctypes.data,
                                                    ln.size, group_log, obs.data_ptr(), roots.data_ptr(), scratch.data_ptr() if need else None,
                                                    need, _stream(stream)), "b3w_bao_group_outboard_batch_device")
    return dict(outboards=obs, ob_first=ob_first, roots=roots)


def group_bytes_batch(arena, offsets, lens, files, chunks, group_log, device="cuda"):
    """the bytes of the sampled chunks' groups as plan_samples_groups_batch takes them (uint8 [n_samples, 1024 << group_log], zero
    past a file's end): what a provider reads from its file for a challenge.  arena: host bytes / numpy, or a CUDA tensor."""
    off, ln = _u64(offsets).astype(np.int64), _u64(lens).astype(np.int64)
    fi, ch = np.asarray(files, dtype=np.int64), np.asarray(chunks, dtype=np.int64)
    width = 1024 << group_log
    rel = (ch >> group_log << group_log) * 1024
    start = off[fi] + rel
    count = np.clip(ln[fi] - rel, 0, width)
    if isinstance(arena, torch.Tensor):
        dev = arena.device
        if arena.numel() == 0:
            return torch.zeros((fi.size, width), dtype=torch.uint8, device=dev)
        col = torch.arange(width, device=dev)
        out = torch.empty((fi.size, width), dtype=torch.uint8, device=dev)
        step = max(1, (1 << 24) // width)                          # (the gather's index tensor: 128 MiB at a time)
        for a in range(0, fi.size, step):
            idx = torch.from_numpy(start[a:a + step]).to(dev)[:, None] + col[None, :]
            live = col[None, :] < torch.from_numpy(count[a:a + step]).to(dev)[:, None]
            out[a:a + step] = torch.where(live, arena[idx.clamp_(max=arena.numel() - 1)], torch.zeros((), dtype=torch.uint8, device=dev))
        return out
    data = np.frombuffer(bytes(arena), dtype=np.uint8) if not isinstance(arena, np.ndarray) else arena
    out = np.zeros((fi.size, width), dtype=np.uint8)
    for s in range(fi.size):
        out[s, :count[s]] = data[start[s]:start[s] + count[s]]
    return torch.from_numpy(out).to(device)


def plan_samples_groups_batch(ctx, d_group_outboards, lens, d_roots, files, chunks, d_group_bytes, group_log, stream=0):
    """plan_samples_batch from group outboards (outboard_groups_batch) and the sampled chunks' groups' bytes (group_bytes_batch): the
    same dict, records and rows word for word plan_samples_batch's.  sample_status: GROUP_STATUS — 1 means a byte of the chunk's
    GROUP does not match, the sampled chunk's or another's."""
    L = lib()
    ln, ch = _u64(lens), _u64(chunks)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    rf = sample_rows_batch(ln, fi, ch)
    dev = d_group_outboards.device
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.numel() >= ln.size * 8
    assert d_group_bytes.is_cuda and d_group_bytes.dtype == torch.uint8 and d_group_bytes.is_contiguous()
    assert d_group_bytes.numel() >= ch.size * (1024 << group_log)
    recs = torch.empty((int(rf[-1]), 32), dtype=torch.int32, device=dev)
    st = torch.full((ch.size,), -1, dtype=torch.int32, device=dev)
    _chk(ctx, L.b3w_sample_plan_group_batch_device(ctx.handle, ln.ctypes.data, ln.size, group_log, d_group_outboards.data_ptr(), d_roots.data_ptr(),
                                                   fi.ctypes.data, ch.ctypes.data, ch.size, d_group_bytes.data_ptr(), recs.data_ptr(), st.data_ptr(),
                                                   _stream(stream)), "b3w_sample_plan_group_batch_device")
    provable = np.array([bool(L.b3w_chain_path_provable(int(c), num_chunks(int(ln[f])))) for f, c in zip(fi, ch)], dtype=bool)
    return dict(records=recs, row_first=rf, sample_status=st.cpu().numpy(), provable=provable)


def prove_samples_groups_batch(ctx, d_group_outboards, lens, d_roots, files, chunks, d_group_bytes, group_log, batch_steps=4096, consumer=None,
                               commit_key=None, r1cs=None, stream=0):
    """prove_samples_batch over plan_samples_groups_batch's plan"""
    s = _stream(stream)
    out = plan_samples_groups_batch(ctx, d_group_outboards, lens, d_roots, files, chunks, d_group_bytes, group_log, stream=s)
    return _prove_planned(ctx, out, batch_steps, consumer, commit_key, r1cs, s)


# ---- slices: the provider extracts, the prover plans from them alone ------------------------------------------------------
def slice_size(length, chunk):
    """8 + 64 path_len + the chunk's byte count: the bao slice of one chunk"""
    size = lib().b3w_bao_slice_size(length, chunk)
    if not size:
        raise B3WError(100, "b3w_bao_slice_size: the chunk index is not below the chunk count")
    return size


def slice_layout(lens, files, chunks):
    """-> slice_first (numpy uint64 [n_samples + 1]): sample s's slice is the slice_size(lens[files[s]], chunks[s]) bytes from
    slice_first[s] of the packed slices (every start 8 modulo 16; what lies between slices is padding); the last entry is the total"""
    ln, ch = _u64(lens), _u64(chunks)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    assert fi.size == ch.size
    sf = np.zeros(ch.size + 1, dtype=np.uint64)
    total = lib().b3w_bao_slice_batch_layout(ln.ctypes.data, ln.size, fi.ctypes.data, ch.ctypes.data, ch.size, sf.ctypes.data)
    if total < 0:
        raise B3WError(-total, "b3w_bao_slice_batch_layout: a file index is not below the file count, or a chunk index not below its file's chunk count")
    return sf


def slices_batch(ctx, d_outboards, lens, files, chunks, d_bytes, group_log=0, stream=0):
    """The provider's side: the standard bao slices of samples (files[s], chunks[s]) in one launch.  group_log = 0: d_outboards as
    outboard_batch returns them, d_bytes as chunk_bytes_batch; group_log 1 .. 6: outboard_groups_batch's outboards and
    group_bytes_batch's bytes — the same slices.  Returns a dict: slices (uint8 CUDA tensor, packed), slice_first (slice_layout)."""
    ln, ch = _u64(lens), _u64(chunks)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    sf = slice_layout(ln, fi, ch)
    assert d_bytes.is_cuda and d_bytes.dtype == torch.uint8 and d_bytes.is_contiguous() and d_bytes.numel() >= ch.size * (1024 << group_log)
    d_slices = torch.zeros(int(sf[-1]), dtype=torch.uint8, device=d_outboards.device)
    _chk(ctx, lib().b3w_bao_slice_batch_device(ctx.handle, ln.ctypes.data, ln.size, group_log, d_outboards.data_ptr(), fi.ctypes.data, ch.ctypes.data,
                                               ch.size, d_bytes.data_ptr(), d_slices.data_ptr(), _stream(stream)), "b3w_bao_slice_batch_device")
    return dict(slices=d_slices, slice_first=sf)


def plan_samples_slices(ctx, lens, d_roots, files, chunks, d_slices, stream=0):
    """The prover's side: plan_samples_batch from the slices alone (slices_batch's tensor, or slices received and packed as
    slice_layout says) and the files' roots on the device — no outboard.  Returns the dict plan_samples_batch returns."""
    L = lib()
    ln, ch = _u64(lens), _u64(chunks)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    rf = sample_rows_batch(ln, fi, ch)
    sf = slice_layout(ln, fi, ch)
    dev = d_slices.device
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.numel() >= ln.size * 8
    assert d_slices.is_cuda and d_slices.dtype == torch.uint8 and d_slices.is_contiguous() and d_slices.numel() >= int(sf[-1])
    recs = torch.empty((int(rf[-1]), 32), dtype=torch.int32, device=dev)
    st = torch.full((ch.size,), -1, dtype=torch.int32, device=dev)
    _chk(ctx, L.b3w_sample_plan_slices_device(ctx.handle, ln.ctypes.data, ln.size, d_roots.data_ptr(), fi.ctypes.data, ch.ctypes.data, ch.size,
                                              d_slices.data_ptr(), recs.data_ptr(), st.data_ptr(), _stream(stream)), "b3w_sample_plan_slices_device")
    provable = np.array([bool(L.b3w_chain_path_provable(int(c), num_chunks(int(ln[f])))) for f, c in zip(fi, ch)], dtype=bool)
    return dict(records=recs, row_first=rf, sample_status=st.cpu().numpy(), provable=provable)


def prove_samples_slices(ctx, lens, d_roots, files, chunks, d_slices, batch_steps=4096, consumer=None, commit_key=None, r1cs=None, stream=0):
    """prove_samples_batch over plan_samples_slices' plan"""
    s = _stream(stream)
    out = plan_samples_slices(ctx, lens, d_roots, files, chunks, d_slices, stream=s)
    return _prove_planned(ctx, out, batch_steps, consumer, commit_key, r1cs, s)


def decode_slice(slice_bytes, length, chunk, root):
    """bao's decoder for one slice on the host -> (status as STATUS, the chunk's bytes — empty unless status is 0)"""
    sl = bytes(slice_bytes)
    rw = np.ascontiguousarray(root, dtype=np.uint32)
    out = ctypes.create_string_buffer(1024)
    cnt, st = ctypes.c_uint32(), ctypes.c_int32()
    _chk(None, lib().b3w_bao_slice_decode(sl, len(sl), length, chunk, rw.ctypes.data, out, ctypes.byref(cnt), ctypes.byref(st)), "b3w_bao_slice_decode")
    return st.value, out.raw[:cnt.value]


# ---- challenged paths and slices read in place from the arena -------------------------------------------------------------
def _arena_args(what, d_arena, offsets, lens, d_outboards, files, chunks, group_log):
    """the checks plan_samples_arena and slices_arena share -> (off, ln, fi, ch)"""
    off, ln, ch = _u64(offsets), _u64(lens), _u64(chunks)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    assert off.size == ln.size and fi.size == ch.size
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    assert d_arena.is_cuda and d_arena.dtype == torch.uint8 and d_arena.is_contiguous()
    ob_first = group_batch_layout(ln, group_log)
    assert d_outboards.is_cuda and d_outboards.dtype == torch.uint8 and d_outboards.is_contiguous() and d_outboards.numel() >= int(ob_first[-1]), what
    return off, ln, fi, ch


def plan_samples_arena(ctx, d_arena, offsets, lens, d_outboards, d_roots, files, chunks, group_log=0, stream=0):
    """plan_samples_batch (group_log = 0: full outboards) / plan_samples_groups_batch (1 .. 6: group outboards) with the samples' bytes
    read where the files lie: file f is bytes [offsets[f], offsets[f] + lens[f]) of d_arena, the uint8 CUDA tensor outboard_batch and
    verify_batch take, files at any byte offset.  No chunk_bytes_batch / group_bytes_batch gather, one launch, nothing outside a
    sample's own file read.  Returns the dict plan_samples_batch returns, the records word for word the same."""
    L = lib()
    off, ln, fi, ch = _arena_args("plan_samples_arena", d_arena, offsets, lens, d_outboards, files, chunks, group_log)
    rf = sample_rows_batch(ln, fi, ch)
    dev = d_outboards.device
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.numel() >= ln.size * 8
    recs = torch.empty((int(rf[-1]), 32), dtype=torch.int32, device=dev)
    st = torch.full((ch.size,), -1, dtype=torch.int32, device=dev)
    _chk(ctx, L.b3w_sample_plan_arena_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, d_arena.numel(), off.ctypes.data,
                                             ln.ctypes.data, ln.size, group_log, d_outboards.data_ptr(), d_roots.data_ptr(), fi.ctypes.data,
                                             ch.ctypes.data, ch.size, recs.data_ptr(), st.data_ptr(), _stream(stream)), "b3w_sample_plan_arena_device")
    provable = np.array([bool(L.b3w_chain_path_provable(int(c), num_chunks(int(ln[f])))) for f, c in zip(fi, ch)], dtype=bool)
    return dict(records=recs, row_first=rf, sample_status=st.cpu().numpy(), provable=provable)


def prove_samples_arena(ctx, d_arena, offsets, lens, d_outboards, d_roots, files, chunks, group_log=0, batch_steps=4096, consumer=None,
                        commit_key=None, r1cs=None, stream=0):
    """prove_samples_batch over plan_samples_arena's plan"""
    s = _stream(stream)
    out = plan_samples_arena(ctx, d_arena, offsets, lens, d_outboards, d_roots, files, chunks, group_log, stream=s)
    return _prove_planned(ctx, out, batch_steps, consumer, commit_key, r1cs, s)


def slices_arena(ctx, d_arena, offsets, lens, d_outboards, files, chunks, group_log=0, stream=0):
    """slices_batch with the sampled chunks' (group_log 1 .. 6: their groups') bytes read where the files lie in d_arena (as
    plan_samples_arena takes it): the same standard slices from either kind of outboard, one launch, no gather.  Returns the dict
    slices_batch returns."""
    off, ln, fi, ch = _arena_args("slices_arena", d_arena, offsets, lens, d_outboards, files, chunks, group_log)
    sf = slice_layout(ln, fi, ch)
    d_slices = torch.zeros(int(sf[-1]), dtype=torch.uint8, device=d_outboards.device)
    _chk(ctx, lib().b3w_bao_slice_arena_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, d_arena.numel(), off.ctypes.data,
                                               ln.ctypes.data, ln.size, group_log, d_outboards.data_ptr(), fi.ctypes.data, ch.ctypes.data, ch.size,
                                               d_slices.data_ptr(), _stream(stream)), "b3w_bao_slice_arena_device")
    return dict(slices=d_slices, slice_first=sf)


# ---- slices taken in: the receiver's side --------------------------------------------------------------------------------
def ingest_slices(ctx, d_arena, offsets, lens, d_outboards, d_roots, files, chunks, d_slices, group_log=0, stream=0, d_have=None):
    """The receiver's side, slices_arena's mirror image: the slices of samples (files[s], chunks[s]) in d_slices (packed as slice_layout
    says, e.g. slices_arena's tensor) are verified against the files' roots on the device, and every slice that VERIFIES puts its chunk's
    bytes at their place in d_arena (file f is bytes [offsets[f], offsets[f] + lens[f]), any byte offset), the stored nodes of its path
    at their pre-order places in file f's outboard in d_outboards (packed as batch_layout / group_batch_layout say: all nodes at
    group_log 0, the part above the group at 1 .. 6) and the header in front.  A slice that does not verify writes nothing but its
    status.  Samples may repeat and come in any order; once every chunk of a file has come in, its outboard is byte for byte
    outboard_batch's / outboard_groups_batch's.  One launch, nothing allocated but the status tensor.  The three tensors must not
    overlap.  When to call verify_stream / outboard_batch instead (MI355X): the call costs about 23 ns a slice — 4 096
    slices of a 1 GiB file 0.18 ms, 65 536 1.52, every chunk 23.7 for 2.27 times the file's bytes in slices — where outboard_batch over
    the whole resident GiB takes 0.43 ms.  So: slices for the sparse fetch, the repair and the remote read, up to a few per cent of a
    file's chunks; a file that arrives whole goes through verify_stream / outboard_batch on its bytes alone.
    d_have (have_new()'s tensor, or None): the arrival bitmap — every sample that verifies also sets its chunk's bit there
    (b3w_bao_slice_ingest_have_device: the same launch, the same bytes written, about 0.6 % slower — 65 536 slices 1.534 ms against
    1.525; have_runs() then lists what is missing).
    Returns dict(sample_status=<int32 CUDA tensor: 0 verified and written, 1 / 2 / 3 as STATUS>)."""
    off, ln, fi, ch = _arena_args("ingest_slices", d_arena, offsets, lens, d_outboards, files, chunks, group_log)
    sf = slice_layout(ln, fi, ch)
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.numel() >= ln.size * 8
    assert d_slices.is_cuda and d_slices.dtype == torch.uint8 and d_slices.is_contiguous() and d_slices.numel() >= int(sf[-1])
    st = torch.full((ch.size,), -1, dtype=torch.int32, device=d_slices.device)
    if d_have is not None:
        _have_tensor("ingest_slices", d_have, ln)
        _chk(ctx, lib().b3w_bao_slice_ingest_have_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, d_arena.numel(), off.ctypes.data,
                                                         ln.ctypes.data, ln.size, group_log, d_outboards.data_ptr(), d_roots.data_ptr(), fi.ctypes.data,
                                                         ch.ctypes.data, ch.size, d_slices.data_ptr(), st.data_ptr(), d_have.data_ptr(), _stream(stream)),
             "b3w_bao_slice_ingest_have_device")
        return dict(sample_status=st)
    _chk(ctx, lib().b3w_bao_slice_ingest_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, d_arena.numel(), off.ctypes.data,
                                                ln.ctypes.data, ln.size, group_log, d_outboards.data_ptr(), d_roots.data_ptr(), fi.ctypes.data,
                                                ch.ctypes.data, ch.size, d_slices.data_ptr(), st.data_ptr(), _stream(stream)), "b3w_bao_slice_ingest_device")
    return dict(sample_status=st)


def _writable(buf, what):
    a = buf if isinstance(buf, np.ndarray) else np.frombuffer(buf, dtype=np.uint8)
    if a.dtype != np.uint8 or not a.flags.c_contiguous or not a.flags.writeable:
        raise B3WError(100, f"ingest_slice_host: {what} is not a writable contiguous buffer of bytes")
    return a


def ingest_slice_host(data, outboard, length, chunk, root, slice_bytes, group_log=0):
    """ingest_slices for one slice on the host (no GPU): data (the file's `length` bytes) and outboard (its outboard of this group_log)
    are bytearrays or numpy uint8 buffers, written in place where the slice verifies -> the status as STATUS"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    d, ob = _writable(data, "data"), _writable(outboard, "outboard")
    if d.size != length or ob.size != group_outboard_size(length, group_log):
        raise B3WError(100, "ingest_slice_host: data is not of this length or the outboard not that of a file of this length")
    sl = bytes(slice_bytes)
    rw = np.ascontiguousarray(root, dtype=np.uint32)
    if rw.size != 8:
        raise B3WError(100, "ingest_slice_host: the root is 8 words")
    st = ctypes.c_int32()
    _chk(None, lib().b3w_bao_slice_ingest(sl, len(sl), length, chunk, rw.ctypes.data, group_log, d.ctypes.data if d.size else None, ob.ctypes.data,
                                          ctypes.byref(st)), "b3w_bao_slice_ingest")
    return st.value


# ---- the arrival bitmap: which chunks have come in, and what is still missing ----------------------------------------------
HAVE_KINDS = {"missing": 0, "present": 1}


def have_layout(lens):
    """-> word_first (numpy uint64 [n_files + 1]): file f owns words [word_first[f], word_first[f + 1]) of the bitmap, 64 chunks a
    word; chunk c is bit c & 63 of word word_first[f] + (c >> 6); the last entry is the total"""
    ln = _u64(lens)
    word_first = np.zeros(ln.size + 1, dtype=np.uint64)
    lib().b3w_bao_have_layout(ln.ctypes.data, ln.size, word_first.ctypes.data)
    return word_first


def have_new(lens, device="cuda"):
    """a cleared bitmap for these files: an int64 tensor of have_layout's size (ingest_slices(..., d_have=) sets its bits)"""
    return torch.zeros(int(have_layout(lens)[-1]), dtype=torch.int64, device=device)


def _have_tensor(what, d_have, ln):
    if not (isinstance(d_have, torch.Tensor) and d_have.is_cuda and d_have.dtype == torch.int64 and d_have.is_contiguous()
            and d_have.numel() >= int(have_layout(ln)[-1])):
        raise B3WError(100, f"{what}: d_have is not a contiguous int64 CUDA tensor of have_layout's size")


def _have_kind(kind):
    if kind not in HAVE_KINDS:
        raise B3WError(100, f"kind {kind!r} is neither 'missing' nor 'present'")
    return HAVE_KINDS[kind]


def have_runs_bound(lens, group_log=0):
    """the number of rows that always suffices: a file of u units has at most ceil(u / 2) runs of one kind"""
    n = np.maximum(1, (_u64(lens) + np.uint64(1023)) // np.uint64(1024))
    units = (n + np.uint64((1 << group_log) - 1)) >> np.uint64(group_log)
    return int(((units + np.uint64(1)) // np.uint64(2)).sum())


def have_runs(ctx, d_have, lens, kind="missing", group_log=0, capacity=None, stream=0):
    """The bitmap as ascending run lists, made on the device in at most four launches: kind "missing" lists the units (chunks, or
    groups of 2^group_log chunks, the last one possibly ragged) with at least one chunk clear, "present" those with every chunk set;
    a run is a maximal stretch of such units of one file, its row (file, first chunk, number of chunks) clipped to the file's chunk
    count — what verify_ranges_batch and outboard_update_batch take, and through runs_chunks() what slices_arena and ingest_slices
    take.  capacity (None: have_runs_bound, which always suffices; 0: count only) bounds the rows written; n_runs is the number found
    even above it.  Returns dict(files uint32, first_chunks uint64, n_chunks uint64: host numpy, the rows written; n_runs: int64 CUDA
    [1]; file_have: int64 CUDA [n_files], the chunks each file holds — it is complete when that is its chunk count).  When not to
    (MI355X): the C call never takes less than about 0.05 ms.  The missing rows of a file of 2^20 chunks are on the
    host in 0.11 ms (1 % missing) to 0.22 ms (50 %), against 0.67 to 3.64 ms for an ingest's statuses copied to the host, scattered
    into a map and made into rows with numpy; 262 144 files of 4 chunks take 0.66 ms against 8.18.  Nothing smaller was measured: with
    a few files of a few thousand chunks a caller that has the statuses on the host anyway may do as well there.  This wrapper also
    makes its output tensors on every call; a loop that matters keeps them and calls b3w_bao_have_runs_device."""
    L = lib()
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    k = _have_kind(kind)
    ln = _u64(lens)
    _have_tensor("have_runs", d_have, ln)
    dev = d_have.device
    cap = have_runs_bound(ln, group_log) if capacity is None else int(capacity)
    run_file = torch.empty(cap, dtype=torch.int32, device=dev)
    run_first = torch.empty(cap, dtype=torch.int64, device=dev)
    run_count = torch.empty(cap, dtype=torch.int64, device=dev)
    n_runs = torch.empty(1, dtype=torch.int64, device=dev)
    file_have = torch.empty(ln.size, dtype=torch.int64, device=dev)
    need = L.b3w_bao_have_runs_scratch_bytes(ln.ctypes.data, ln.size)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _chk(ctx, L.b3w_bao_have_runs_device(ctx.handle, d_have.data_ptr(), ln.ctypes.data, ln.size, group_log, k, cap, run_file.data_ptr() if cap else None,
                                         run_first.data_ptr() if cap else None, run_count.data_ptr() if cap else None, n_runs.data_ptr(),
                                         file_have.data_ptr() if ln.size else None, scratch.data_ptr(), scratch.numel(), _stream(stream)),
         "b3w_bao_have_runs_device")
    rows = min(int(n_runs.item()), cap)
    return dict(files=run_file[:rows].cpu().numpy().view(np.uint32), first_chunks=run_first[:rows].cpu().numpy().view(np.uint64),
                n_chunks=run_count[:rows].cpu().numpy().view(np.uint64), n_runs=n_runs, file_have=file_have)


def have_from_status(ctx, unit_status, lens, group_log=0, d_have=None, stream=0):
    """After a restart: the bitmap from verify_batch's / verify_ranges_batch's unit_status (uint8 CUDA, packed as verify_layout says
    for this group_log) over the half-filled arena and outboards.  Chunk c of file f is set where the status of its unit is 0 (0xFF,
    a unit the ranged call was not asked about, reads as absent); every word is written whole, pad bits zero — the one call that clears
    bits.  One launch.  d_have: written in place when given, made here otherwise -> d_have."""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    ln = _u64(lens)
    assert unit_status.is_cuda and unit_status.dtype == torch.uint8 and unit_status.is_contiguous() and unit_status.numel() >= int(verify_layout(ln, group_log)[-1])
    if d_have is None:
        d_have = torch.empty(int(have_layout(ln)[-1]), dtype=torch.int64, device=unit_status.device)
    _have_tensor("have_from_status", d_have, ln)
    _chk(ctx, lib().b3w_bao_have_from_status_device(ctx.handle, unit_status.data_ptr(), ln.ctypes.data, ln.size, group_log, d_have.data_ptr(), _stream(stream)),
         "b3w_bao_have_from_status_device")
    return d_have


def have_runs_host(have, length, kind="missing", group_log=0, capacity=None):
    """have_runs for one file on the host (no GPU): have = the file's words (numpy uint64) -> (first_chunks, n_chunks: the rows
    written, numpy uint64; n_runs: the number found; n_have: the chunks held)"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    k = _have_kind(kind)
    hv = _u64(have)
    if hv.size != (num_chunks(length) + 63) // 64:
        raise B3WError(100, "have_runs_host: the bitmap is not that of a file of this length")
    cap = have_runs_bound([length], group_log) if capacity is None else int(capacity)
    first, count = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    n_runs, n_have = ctypes.c_uint64(), ctypes.c_uint64()
    _chk(None, lib().b3w_bao_have_runs(hv.ctypes.data, length, group_log, k, cap, first.ctypes.data if cap else None, count.ctypes.data if cap else None,
                                       ctypes.byref(n_runs), ctypes.byref(n_have)), "b3w_bao_have_runs")
    rows = min(n_runs.value, cap)
    return first[:rows], count[:rows], n_runs.value, n_have.value


def have_from_status_host(unit_status, length, group_log=0):
    """have_from_status for one file on the host (no GPU): unit_status as verify_host returns it -> the file's words (numpy uint64)"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    st = np.ascontiguousarray(unit_status, dtype=np.uint8)
    n = num_chunks(length)
    if st.size != (n + (1 << group_log) - 1) >> group_log:
        raise B3WError(100, "have_from_status_host: the statuses are not those of a file of this length")
    have = np.zeros((n + 63) // 64, dtype=np.uint64)
    _chk(None, lib().b3w_bao_have_from_status(st.ctypes.data, length, group_log, have.ctypes.data), "b3w_bao_have_from_status")
    return have


def runs_chunks(files, first_chunks, n_chunks):
    """have_runs' rows as sample lists -> (files uint32, chunks uint64), a sample per chunk in the rows' order: what slices_arena and
    ingest_slices take"""
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    fc, nc = _ranges(first_chunks, n_chunks)
    if fi.size != fc.size:
        raise B3WError(100, f"runs_chunks: {fi.size} files and {fc.size} ranges")
    cnt = nc.astype(np.int64)
    starts = np.cumsum(cnt) - cnt
    within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(starts, cnt)
    return np.repeat(fi, cnt), (np.repeat(fc, cnt).astype(np.int64) + within).astype(np.uint64)


# ---- outboard diff: the chunks two versions of a file share, from their outboards alone -----------------------------------
def _diff_side(what, side, lens, d_outboards, d_roots, group_log, ob_first):
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"{what}: group_log_{side} {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    ln = _u64(lens)
    obf = group_batch_layout(ln, group_log) if ob_first is None else _u64(ob_first)
    if obf.size < ln.size:
        raise B3WError(100, f"{what}: {obf.size} outboard places for {ln.size} files of side {side}")
    if not (isinstance(d_outboards, torch.Tensor) and d_outboards.is_cuda and d_outboards.dtype == torch.uint8 and d_outboards.is_contiguous()):
        raise B3WError(100, f"{what}: d_outboards_{side} is not a contiguous uint8 CUDA tensor")
    if not (isinstance(d_roots, torch.Tensor) and d_roots.is_cuda and d_roots.is_contiguous() and d_roots.element_size() == 4 and d_roots.numel() >= ln.size * 8):
        raise B3WError(100, f"{what}: d_roots_{side} is not a contiguous CUDA tensor of 8 words a file")
    return ln, obf


def outboard_diff(ctx, lens_a, d_outboards_a, d_roots_a, lens_b, d_outboards_b, d_roots_b, pairs_a=None, pairs_b=None, group_log_a=0, group_log_b=0,
                  ob_first_a=None, ob_first_b=None, d_same=None, stream=0):
    """Which chunks of version b of a file does a holder of version a already have?  Answered on the device from the two outboards
    alone: pair i is (file pairs_a[i] of side a, file pairs_b[i] of side b; no lists: file i of both), a side its lengths, its
    outboards as outboard_batch (group_log 0) / outboard_groups_batch made them (at ob_first, any 8-byte-aligned places; None: the
    batch layout of its lens) and its roots.  The sides may be the same tensors and a file may be in many pairs.  With
    G = max(group_log_a, group_log_b) a unit is 2^G chunks (the last one ragged); its CV is stored in its parent's node (the finer
    outboard read at the coarser level), or is the root where the unit is the whole file, and unit u of b is SAME iff it exists in a,
    covers the same chunks, is the whole file in both or in neither, and the stored CVs are equal.  Returns dict(same: int64 CUDA, the
    bitmap in have_layout(pair_lens)'s layout, every word written whole, pad bits zero; word_first: numpy uint64 [n_pairs + 1];
    pair_lens: numpy uint64, the b lengths of the pairs — what have_runs, have_runs_bound and runs_chunks take as lens, the rows' file
    column then being the pair index).  A set bit means equal bytes; a clear bit "differs or not known": a chunk with equal bytes is
    still clear where another chunk of its unit differs or where its unit is the whole file on one side only.  Nothing is hashed and
    no file byte read; one launch.
    Sync from a stale replica, EQUAL LENGTHS: diff = outboard_diff(old side, new side); runs = have_runs(ctx, diff["same"],
    diff["pair_lens"], "missing"); the provider answers set_slices_arena over those runs; the replica calls ingest_set_slices(its own
    arena, its own OLD outboards, d_roots = the NEW roots, d_have = diff["same"]).  Nodes over unchanged chunks are right already and
    every node above a changed chunk arrives verified in the slice, so the replica ends with the provider's bytes and outboard byte
    for byte.  CHANGED LENGTH: first outboard_resize_batch over the replica's arena as it is at the new length (the bytes behind the
    old end are whatever lies there): an outboard consistent with what the replica holds; then the recipe above against it.
    When not to (MI355X): the C call never takes less than about 0.02 ms.  One 1 GiB file with 1 % of its chunks rewritten
    takes 0.033 ms (full outboards; copying the two outboards device to device takes 0.046) or 0.021 (group_log 4), where
    verify_batch of b's resident bytes against a's outboard followed by have_from_status takes 0.457 and 0.440; 262 144 files of 4
    chunks take 1.17 ms against 1.99, most of it the host's table (about 4 ns and 40 uploaded bytes a pair).  A caller who already
    holds b's bytes and must verify them anyway gets the same bitmap from that route, verified: this call verifies nothing and
    believes both outboards (verify_batch over the finished file is what catches a lying outboard).  This wrapper also makes the
    layouts and, with d_same=None, the bitmap on every call; a loop that matters keeps them and calls b3w_bao_outboard_diff_device."""
    what = "outboard_diff"
    la, ofa = _diff_side(what, "a", lens_a, d_outboards_a, d_roots_a, group_log_a, ob_first_a)
    lb, ofb = _diff_side(what, "b", lens_b, d_outboards_b, d_roots_b, group_log_b, ob_first_b)
    if (pairs_a is None) != (pairs_b is None):
        raise B3WError(100, f"{what}: one pair list without the other")
    if pairs_a is None:
        if la.size != lb.size:
            raise B3WError(100, f"{what}: no pair lists and {la.size} files against {lb.size}")
        pa = pb = np.arange(la.size, dtype=np.uint32)
    else:
        pa = np.ascontiguousarray(np.atleast_1d(pairs_a), dtype=np.uint32)
        pb = np.ascontiguousarray(np.atleast_1d(pairs_b), dtype=np.uint32)
        if pa.size != pb.size:
            raise B3WError(100, f"{what}: {pa.size} files of side a paired with {pb.size} of side b")
        if pa.size and (int(pa.max()) >= la.size or int(pb.max()) >= lb.size):
            raise B3WError(100, f"{what}: a pair names a file that is not below its side's file count")
    pair_lens = lb[pb] if pb.size else np.zeros(0, dtype=np.uint64)
    word_first = have_layout(pair_lens)
    if d_same is None:
        d_same = torch.empty(int(word_first[-1]), dtype=torch.int64, device=d_outboards_b.device)
    _have_tensor(what, d_same, pair_lens)
    _chk(ctx, lib().b3w_bao_outboard_diff_device(ctx.handle, la.ctypes.data, ofa.ctypes.data, d_outboards_a.data_ptr(), d_outboards_a.numel(), d_roots_a.data_ptr(),
                                                 la.size, group_log_a, lb.ctypes.data, ofb.ctypes.data, d_outboards_b.data_ptr(), d_outboards_b.numel(),
                                                 d_roots_b.data_ptr(), lb.size, group_log_b, pa.ctypes.data, pb.ctypes.data, pa.size, word_first.ctypes.data,
                                                 d_same.data_ptr(), _stream(stream)), "b3w_bao_outboard_diff_device")
    return dict(same=d_same, word_first=word_first, pair_lens=pair_lens)


def diff_host(outboard_a, len_a, root_a, outboard_b, len_b, root_b, group_log_a=0, group_log_b=0):
    """outboard_diff for one pair on the host (no GPU): the outboards as bytes (or tensors) of group_outboard_size(len, group_log), the
    roots as 8 words -> the pair's words (numpy uint64 [ceil(num_chunks(len_b) / 64)])"""
    sides = []
    for side, ob, ln, root, g in (("a", outboard_a, len_a, root_a, group_log_a), ("b", outboard_b, len_b, root_b, group_log_b)):
        if not 0 <= g <= MAX_GROUP_LOG:
            raise B3WError(100, f"diff_host: group_log_{side} {g} is not in 0 .. {MAX_GROUP_LOG}")
        if ln < 0:
            raise B3WError(100, f"diff_host: len_{side} is negative")
        ob = ob.cpu().numpy().tobytes() if isinstance(ob, torch.Tensor) else bytes(ob)
        if len(ob) != group_outboard_size(ln, g):
            raise B3WError(100, f"diff_host: outboard_{side}'s size is not that of a file of len_{side} bytes")
        rw = np.ascontiguousarray(np.asarray(root.cpu() if isinstance(root, torch.Tensor) else root).reshape(-1).astype(np.uint32))
        if rw.size != 8:
            raise B3WError(100, f"diff_host: root_{side} is not 8 words")
        sides.append((ob, rw))
    same = np.zeros((num_chunks(len_b) + 63) // 64, dtype=np.uint64)
    _chk(None, lib().b3w_bao_outboard_diff(sides[0][0], len_a, sides[0][1].ctypes.data, group_log_a, sides[1][0], len_b, sides[1][1].ctypes.data, group_log_b,
                                           same.ctypes.data), "b3w_bao_outboard_diff")
    return same


# ---- outboard deltas: the nodes of a new version that a replica does not hold, served and verified on arrival ---------------
DELTA_NO_A = 0xFFFFFFFF
DELTA_MALFORMED, DELTA_BAD_HASH, DELTA_NOT_HELD = 1, 2, 3


def _delta_g(what, group_log):
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"{what}: group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")


def delta_bound(length, group_log=0):
    """16 + 8 W + 64 (U - 1): the bytes that always suffice for the delta blob of a version of `length` bytes"""
    _delta_g("delta_bound", group_log)
    return int(lib().b3w_bao_outboard_delta_bound(int(length), group_log))


def delta_layout(lens_b, group_log=0, pairs_b=None):
    """-> numpy uint64 [n_pairs + 1]: the blobs' extents at their bounds, one behind the other (pairs_b None: pair i is file i)"""
    _delta_g("delta_layout", group_log)
    lb = _u64(lens_b)
    pb = np.arange(lb.size, dtype=np.uint32) if pairs_b is None else np.ascontiguousarray(np.atleast_1d(pairs_b), dtype=np.uint32)
    if pb.size and int(pb.max()) >= lb.size:
        raise B3WError(100, "delta_layout: a pair names a file that is not below the file count")
    first = np.zeros(pb.size + 1, dtype=np.uint64)
    lib().b3w_bao_outboard_delta_layout(lb.ctypes.data, lb.size, pb.ctypes.data, pb.size, group_log, first.ctypes.data)
    return first


def _delta_pairs(what, pairs_a, pairs_b, n_a, n_b):
    if (pairs_a is None) != (pairs_b is None):
        raise B3WError(100, f"{what}: one pair list without the other")
    if pairs_a is None:
        if n_a != n_b:
            raise B3WError(100, f"{what}: no pair lists and {n_a} files against {n_b}")
        return np.arange(n_a, dtype=np.uint32), np.arange(n_a, dtype=np.uint32)
    pa = np.ascontiguousarray(np.atleast_1d(pairs_a), dtype=np.uint32)
    pb = np.ascontiguousarray(np.atleast_1d(pairs_b), dtype=np.uint32)
    if pa.size != pb.size:
        raise B3WError(100, f"{what}: {pa.size} files of side a paired with {pb.size} of side b")
    held = pa[pa != DELTA_NO_A]
    if (held.size and int(held.max()) >= n_a) or (pb.size and int(pb.max()) >= n_b):
        raise B3WError(100, f"{what}: a pair names a file that is not below its side's file count")
    return pa, pb


def _delta_side_a(what, lens_a, d_outboards_a, d_roots_a, group_log, ob_first_a):
    """side a, or "the replica holds nothing" (lens_a None) -> (lens, places, outboards' address, bytes, roots' address)"""
    if lens_a is None:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), 0, 0, 0
    la, ofa = _diff_side(what, "a", lens_a, d_outboards_a, d_roots_a, group_log, ob_first_a)
    return la, ofa, d_outboards_a.data_ptr(), d_outboards_a.numel(), d_roots_a.data_ptr()


def _delta_scratch(what, d_scratch, lb, pb, group_log, device):
    need = int(lib().b3w_bao_outboard_delta_scratch_bytes(lb.ctypes.data, lb.size, pb.ctypes.data, pb.size, group_log))
    if d_scratch is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if not (isinstance(d_scratch, torch.Tensor) and d_scratch.is_cuda and d_scratch.dtype == torch.uint8 and d_scratch.is_contiguous() and d_scratch.numel() >= need):
        raise B3WError(100, f"{what}: d_scratch is not a contiguous uint8 CUDA tensor of {need} bytes")
    return d_scratch


def outboard_delta(ctx, lens_a, d_outboards_a, d_roots_a, lens_b, d_outboards_b, d_roots_b, pairs_a=None, pairs_b=None, group_log=0, ob_first_a=None,
                   ob_first_b=None, delta_first=None, d_delta=None, d_n_nodes=None, d_scratch=None, stream=0):
    """THE PROVIDER of outboard deltas (b3wit.h "outboard delta"): for every pair (file pairs_a[i] of the replica's version a, file
    pairs_b[i] of the new version b; DELTA_NO_A in pairs_a or lens_a=None: the replica holds nothing) the parent nodes of b's outboard
    that a does not already hold, as one self-describing blob: len_b, k, a bitmap of the nodes present, the k nodes in pre-order.  Both
    sides have one group_log.  A node is SAME, and left out, iff a's tree has a node over the same units and chunks below its root with
    an equal stored CV (the root: equal chunk counts and equal roots).  delta_first: the blobs' extents (None: delta_layout, which always
    suffices); a smaller extent gets the nodes that fit while n_nodes[i] still says k as found.  Returns dict(delta: uint8 CUDA,
    delta_first, n_nodes: int64 CUDA [n_pairs], pair_lens).  Nothing is hashed, no file byte read; at most four launches.
    When not to (MI355X): one 1 GiB file with 1 % of its chunks rewritten gives 4.7 MB for an outboard of 67.1 MB in
    0.065 ms (copying the two outboards 0.046, outboard_diff 0.032) and apply_outboard_delta takes 0.108 (copying b's outboard 0.022,
    verify_batch of b's resident file 0.432); with half of the chunks rewritten the blob is 0.86 of the outboard - send the outboard
    and run outboard_check (0.150 ms) instead; 262 144 files of 4 chunks take 1.94 ms and 2.02 where verify_batch takes 1.52: the
    host's table of 72 bytes a pair is the cost, so not for very many tiny files that are resident anyway.  This wrapper also makes
    the layouts and buffers on every call; a loop that matters keeps them and calls b3w_bao_outboard_delta_device."""
    what = "outboard_delta"
    _delta_g(what, group_log)
    la, ofa, a_ptr, a_bytes, ra_ptr = _delta_side_a(what, lens_a, d_outboards_a, d_roots_a, group_log, ob_first_a)
    lb, ofb = _diff_side(what, "b", lens_b, d_outboards_b, d_roots_b, group_log, ob_first_b)
    if lens_a is None and pairs_a is None:
        pairs_a, pairs_b = np.full(lb.size, DELTA_NO_A, dtype=np.uint32), np.arange(lb.size, dtype=np.uint32)
    pa, pb = _delta_pairs(what, pairs_a, pairs_b, la.size, lb.size)
    dev = d_outboards_b.device
    first = delta_layout(lb, group_log, pb) if delta_first is None else _u64(delta_first)
    if first.size != pa.size + 1:
        raise B3WError(100, f"{what}: delta_first has {first.size} entries for {pa.size} pairs")
    if d_delta is None:
        d_delta = torch.empty(int(first[-1]), dtype=torch.uint8, device=dev)
    if not (isinstance(d_delta, torch.Tensor) and d_delta.is_cuda and d_delta.dtype == torch.uint8 and d_delta.is_contiguous()):
        raise B3WError(100, f"{what}: d_delta is not a contiguous uint8 CUDA tensor")
    if d_n_nodes is None:
        d_n_nodes = torch.empty(pa.size, dtype=torch.int64, device=dev)
    if not (isinstance(d_n_nodes, torch.Tensor) and d_n_nodes.is_cuda and d_n_nodes.dtype == torch.int64 and d_n_nodes.is_contiguous() and d_n_nodes.numel() >= pa.size):
        raise B3WError(100, f"{what}: d_n_nodes is not a contiguous int64 CUDA tensor of one word a pair")
    d_scratch = _delta_scratch(what, d_scratch, lb, pb, group_log, dev)
    _chk(ctx, lib().b3w_bao_outboard_delta_device(ctx.handle, la.ctypes.data, ofa.ctypes.data, a_ptr, a_bytes, ra_ptr, la.size, lb.ctypes.data, ofb.ctypes.data,
                                                  d_outboards_b.data_ptr(), d_outboards_b.numel(), d_roots_b.data_ptr(), lb.size, group_log, group_log, pa.ctypes.data,
                                                  pb.ctypes.data, pa.size, first.ctypes.data, d_delta.data_ptr(), d_delta.numel(), d_n_nodes.data_ptr(),
                                                  d_scratch.data_ptr(), d_scratch.numel(), _stream(stream)), "b3w_bao_outboard_delta_device")
    return dict(delta=d_delta, delta_first=first, n_nodes=d_n_nodes, pair_lens=lb[pb] if pb.size else np.zeros(0, dtype=np.uint64))


def apply_outboard_delta(ctx, lens_a, d_outboards_a, d_roots_a, lens_b, d_roots_b, d_delta, delta_first, pairs_a=None, pairs_b=None, group_log=0,
                         ob_first_a=None, ob_first_out=None, d_outboards_out=None, d_pair_status=None, d_first_bad=None, d_scratch=None, stream=0):
    """THE REPLICA: every blob of d_delta (UNTRUSTED) is verified against b's root by hashing its nodes alone - one parent compression
    per present node, no file byte read - and only a pair that passes gets its output outboard written whole: present nodes at their
    pre-order places, every absent node from a's outboard at the place of the same span in a's tree.  pair_status: 0, DELTA_MALFORMED,
    DELTA_BAD_HASH or DELTA_NOT_HELD, the first that applies at the lowest node; first_bad: that node (2^64 - 1 as -1: none).  A pair
    with a status keeps its output extent as it was.  d_outboards_out None: a fresh buffer in the batch layout of the pairs' b lengths;
    d_outboards_out = d_outboards_a (with ob_first_out = the pairs' a places): IN PLACE, every pair then has U_a = U_b and only present
    nodes are written.  The outputs lie in rising order of the pairs.  What a pass proves: the output is consistent with b's root
    given that the subtrees copied from a were consistent with what a stores for them; nothing about file bytes.  Returns
    dict(outboards, ob_first, pair_status: int32 CUDA, first_bad: int64 CUDA).  Four launches."""
    what = "apply_outboard_delta"
    _delta_g(what, group_log)
    la, ofa, a_ptr, a_bytes, ra_ptr = _delta_side_a(what, lens_a, d_outboards_a, d_roots_a, group_log, ob_first_a)
    lb = _u64(lens_b)
    if not (isinstance(d_roots_b, torch.Tensor) and d_roots_b.is_cuda and d_roots_b.is_contiguous() and d_roots_b.element_size() == 4 and d_roots_b.numel() >= lb.size * 8):
        raise B3WError(100, f"{what}: d_roots_b is not a contiguous CUDA tensor of 8 words a file")
    if lens_a is None and pairs_a is None:
        pairs_a, pairs_b = np.full(lb.size, DELTA_NO_A, dtype=np.uint32), np.arange(lb.size, dtype=np.uint32)
    pa, pb = _delta_pairs(what, pairs_a, pairs_b, la.size, lb.size)
    if not (isinstance(d_delta, torch.Tensor) and d_delta.is_cuda and d_delta.dtype == torch.uint8 and d_delta.is_contiguous()):
        raise B3WError(100, f"{what}: d_delta is not a contiguous uint8 CUDA tensor")
    first = _u64(delta_first)
    if first.size != pa.size + 1:
        raise B3WError(100, f"{what}: delta_first has {first.size} entries for {pa.size} pairs")
    dev = d_delta.device
    pair_lens = lb[pb] if pb.size else np.zeros(0, dtype=np.uint64)
    if ob_first_out is None:
        layout = group_batch_layout(pair_lens, group_log)
        out_first, out_bytes = np.ascontiguousarray(layout[:-1], dtype=np.uint64), int(layout[-1])
    else:
        out_first, out_bytes = _u64(ob_first_out), None
        if out_first.size < pa.size:
            raise B3WError(100, f"{what}: {out_first.size} output places for {pa.size} pairs")
    if d_outboards_out is None:
        if out_bytes is None:
            raise B3WError(100, f"{what}: ob_first_out without d_outboards_out")
        d_outboards_out = torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
    if not (isinstance(d_outboards_out, torch.Tensor) and d_outboards_out.is_cuda and d_outboards_out.dtype == torch.uint8 and d_outboards_out.is_contiguous()):
        raise B3WError(100, f"{what}: d_outboards_out is not a contiguous uint8 CUDA tensor")
    if d_pair_status is None:
        d_pair_status = torch.empty(pa.size, dtype=torch.int32, device=dev)
    if d_first_bad is None:
        d_first_bad = torch.empty(pa.size, dtype=torch.int64, device=dev)
    if not (d_pair_status.is_cuda and d_pair_status.dtype == torch.int32 and d_pair_status.is_contiguous() and d_pair_status.numel() >= pa.size and
            d_first_bad.is_cuda and d_first_bad.dtype == torch.int64 and d_first_bad.is_contiguous() and d_first_bad.numel() >= pa.size):
        raise B3WError(100, f"{what}: d_pair_status / d_first_bad are not contiguous int32 / int64 CUDA tensors of one entry a pair")
    d_scratch = _delta_scratch(what, d_scratch, lb, pb, group_log, dev)
    _chk(ctx, lib().b3w_bao_outboard_delta_apply_device(ctx.handle, la.ctypes.data, ofa.ctypes.data, a_ptr, a_bytes, ra_ptr, la.size, lb.ctypes.data,
                                                        d_roots_b.data_ptr(), lb.size, group_log, pa.ctypes.data, pb.ctypes.data, pa.size, first.ctypes.data,
                                                        d_delta.data_ptr(), d_delta.numel(), out_first.ctypes.data, d_outboards_out.data_ptr(),
                                                        d_outboards_out.numel(), d_pair_status.data_ptr(), d_first_bad.data_ptr(), d_scratch.data_ptr(),
                                                        d_scratch.numel(), _stream(stream)), "b3w_bao_outboard_delta_apply_device")
    return dict(outboards=d_outboards_out, ob_first=out_first, pair_status=d_pair_status, first_bad=d_first_bad)


def outboard_check(ctx, lens, d_outboards, d_roots, group_log=0, ob_first=None):
    """Are these outboards consistent with their roots?  Answered WITHOUT the files: the delta of every outboard against nothing (all
    of its nodes) is applied into a scratch outboard, which hashes every node once against its parent's half and the root.  Returns
    dict(file_status: int32 CUDA, 0 or DELTA_BAD_HASH; first_bad: int64 CUDA, the lowest pre-order node whose compression is not what
    is stored above it, -1: none).  It proves nothing about file bytes (verify_batch does, and needs them resident).  MI355X: the
    outboard of a 1 GiB file in 0.150 ms (verify_batch of the file 0.432), group outboards of 16 chunks 0.075; 262 144 files of 4
    chunks 3.92 ms against 1.52 - not for very many tiny files."""
    made = outboard_delta(ctx, None, None, None, lens, d_outboards, d_roots, group_log=group_log, ob_first_b=ob_first)
    res = apply_outboard_delta(ctx, None, None, None, lens, d_roots, made["delta"], made["delta_first"], group_log=group_log)
    return dict(file_status=res["pair_status"], first_bad=res["first_bad"])


def _delta_host_side(what, side, ob, ln, root, g):
    if ob is None:
        return None, None
    if ln < 0:
        raise B3WError(100, f"{what}: len_{side} is negative")
    ob = ob.cpu().numpy().tobytes() if isinstance(ob, torch.Tensor) else bytes(ob)
    if len(ob) != group_outboard_size(ln, g):
        raise B3WError(100, f"{what}: outboard_{side}'s size is not that of a file of len_{side} bytes")
    return ob, _delta_root(what, side, root)


def _delta_root(what, side, root):
    if isinstance(root, (bytes, bytearray)):
        rw = np.frombuffer(bytes(root) + bytes(-len(root) % 4), dtype=np.uint32).copy()
    else:
        rw = np.ascontiguousarray(np.asarray(root.cpu() if isinstance(root, torch.Tensor) else root).reshape(-1).astype(np.uint32))
    if rw.size != 8:
        raise B3WError(100, f"{what}: root_{side} is not 8 words")
    return rw


def delta_host(outboard_a, len_a, root_a, outboard_b, len_b, root_b, group_log=0, capacity=None):
    """outboard_delta for one pair on the host (no GPU; outboard_a None: the replica holds nothing) -> (the blob: bytes of `capacity`
    (None: delta_bound) of which the header, the bitmap and the nodes that fit are written and the rest is zero; k as found)"""
    _delta_g("delta_host", group_log)
    a, ra = _delta_host_side("delta_host", "a", outboard_a, len_a, root_a, group_log)
    b, rb = _delta_host_side("delta_host", "b", outboard_b, len_b, root_b, group_log)
    if b is None:
        raise B3WError(100, "delta_host: no outboard_b")
    cap = delta_bound(len_b, group_log) if capacity is None else int(capacity)
    blob = np.zeros(cap, dtype=np.uint8)
    k = ctypes.c_uint64(0)
    _chk(None, lib().b3w_bao_outboard_delta(a, len_a if a is not None else 0, ra.ctypes.data if a is not None else None, b, len_b, rb.ctypes.data, group_log,
                                            blob.ctypes.data, cap, ctypes.addressof(k)), "b3w_bao_outboard_delta")
    return blob.tobytes(), int(k.value)


def apply_delta_host(outboard_a, len_a, root_a, len_b, root_b, blob, group_log=0):
    """apply_outboard_delta for one pair on the host -> (status, first bad node or -1, the outboard of b as bytes or None with a status)"""
    _delta_g("apply_delta_host", group_log)
    a, ra = _delta_host_side("apply_delta_host", "a", outboard_a, len_a, root_a, group_log)
    rb = _delta_root("apply_delta_host", "b", root_b)
    blob = bytes(blob)
    out = np.zeros(group_outboard_size(len_b, group_log), dtype=np.uint8)
    status, bad = ctypes.c_int32(0), ctypes.c_uint64(0)
    _chk(None, lib().b3w_bao_outboard_delta_apply(a, len_a if a is not None else 0, ra.ctypes.data if a is not None else None, len_b, rb.ctypes.data, group_log,
                                                  blob, len(blob), out.ctypes.data, ctypes.addressof(status), ctypes.addressof(bad)), "b3w_bao_outboard_delta_apply")
    return int(status.value), -1 if bad.value == 2 ** 64 - 1 else int(bad.value), out.tobytes() if status.value == 0 else None


# ---- range slices: the slice of a run of chunks, extracted and taken in ---------------------------------------------------
def range_slice_size(length, first_chunk, n_chunks):
    """8 + 64 U + the range's bytes: the bao slice of chunks [first_chunk, first_chunk + n_chunks), every shared node once"""
    size = lib().b3w_bao_range_slice_size(length, first_chunk, n_chunks)
    if not size:
        raise B3WError(100, "b3w_bao_range_slice_size: the range is empty or reaches past the chunk count")
    return size


def range_slice_layout(lens, files, first_chunks, n_chunks):
    """-> slice_first (numpy uint64 [n_ranges + 1]): range r's slice is the range_slice_size bytes from slice_first[r] of the packed
    slices (every start 8 modulo 16; what lies between slices is padding); the last entry is the total"""
    ln = _u64(lens)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    fc, nc = _ranges(first_chunks, n_chunks)
    assert fi.size == fc.size
    sf = np.zeros(fc.size + 1, dtype=np.uint64)
    total = lib().b3w_bao_range_slice_batch_layout(ln.ctypes.data, ln.size, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size, sf.ctypes.data)
    if total < 0:
        raise B3WError(-total, "b3w_bao_range_slice_batch_layout: a file index is not below the file count, or a range is empty or reaches past its file's chunk count")
    return sf


def _range_args(what, d_arena, offsets, lens, d_outboards, files, first_chunks, n_chunks, group_log):
    off, ln, fi, fc = _arena_args(what, d_arena, offsets, lens, d_outboards, files, first_chunks, group_log)
    fc, nc = _ranges(fc, n_chunks)
    return off, ln, fi, fc, nc


def range_slices_arena(ctx, d_arena, offsets, lens, d_outboards, files, first_chunks, n_chunks, group_log=0, stream=0):
    """The provider's side for runs of chunks: slices_arena with ranges (files[r], first_chunks[r], n_chunks[r]) — have_runs' rows as
    they come — where that takes one chunk a sample.  A range slice carries every node its chunks share once: 1 024 chunks of a 1 GiB
    file are 1.06 times their payload where 1 024 one-chunk slices are 2.26 times.  At most two launches; nothing is verified.
    Measured (MI355X, DESIGN.md §8g, against runs_chunks + slices_arena's C call of the commit before): 64 runs of 1 024 chunks
    0.08 ms against 4.37, the runs of a half-missing bitmap 13.3 against 38.7, 65 536 runs of one chunk 5.35 against 5.16 (level).
    Returns dict(slices: uint8 CUDA tensor, packed; slice_first: range_slice_layout)."""
    off, ln, fi, fc, nc = _range_args("range_slices_arena", d_arena, offsets, lens, d_outboards, files, first_chunks, n_chunks, group_log)
    sf = range_slice_layout(ln, fi, fc, nc)
    d_slices = torch.zeros(int(sf[-1]), dtype=torch.uint8, device=d_outboards.device)
    _chk(ctx, lib().b3w_bao_range_slice_arena_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, d_arena.numel(), off.ctypes.data,
                                                     ln.ctypes.data, ln.size, group_log, d_outboards.data_ptr(), fi.ctypes.data, fc.ctypes.data,
                                                     nc.ctypes.data, fc.size, d_slices.data_ptr(), _stream(stream)), "b3w_bao_range_slice_arena_device")
    return dict(slices=d_slices, slice_first=sf)


def ingest_range_slices(ctx, d_arena, offsets, lens, d_outboards, d_roots, files, first_chunks, n_chunks, d_slices, group_log=0, stream=0, d_have=None):
    """The receiver's side for runs of chunks, range_slices_arena's mirror image and ingest_slices' twin: every chunk of every range
    gets the status its own one-chunk slice would get, and the chunks of status 0 write what ingest_slices writes for them — bytes,
    stored path nodes, header, and their bit in d_have where one is given.  A bad node keeps out the chunks below it and no other.
    Ranges may overlap, repeat and come in any order.  At most three launches.  When not to (MI355X, DESIGN.md §8g, against a build
    of the commit before doing the same with ingest_slices over runs_chunks): 64 runs of 1 024 chunks of a 1 GiB file 0.21 ms against
    1.53, 4 096 runs of 16 0.47 against 1.52 — but a range takes at least a wave, so 65 536 runs of ONE chunk take 7.3 ms against 1.5
    and the 262 507 runs of a half-missing bitmap 21.1 against 11.7 (for 26 % fewer bytes): runs of one or two chunks are faster to
    take in through runs_chunks and ingest_slices; where between 2 and 16 chunks a run the two cross was not measured.  This wrapper
    makes its outputs and its scratch on every call; a loop that matters keeps them and calls b3w_bao_range_slice_ingest_device.
    Returns dict(range_status: int32 CUDA, the largest chunk status of each range; range_first_bad: int64 CUDA, the first chunk of
    the file whose status is not 0, -1 for none)."""
    L = lib()
    off, ln, fi, fc, nc = _range_args("ingest_range_slices", d_arena, offsets, lens, d_outboards, files, first_chunks, n_chunks, group_log)
    sf = range_slice_layout(ln, fi, fc, nc)
    dev = d_slices.device
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.numel() >= ln.size * 8
    assert d_slices.is_cuda and d_slices.dtype == torch.uint8 and d_slices.is_contiguous() and d_slices.numel() >= int(sf[-1])
    if d_have is not None:
        _have_tensor("ingest_range_slices", d_have, ln)
    st = torch.full((fc.size,), -1, dtype=torch.int32, device=dev)
    fb = torch.full((fc.size,), -2, dtype=torch.int64, device=dev)
    need = L.b3w_bao_range_slice_ingest_scratch_bytes(ln.ctypes.data, ln.size, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _chk(ctx, L.b3w_bao_range_slice_ingest_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, d_arena.numel(), off.ctypes.data,
                                                  ln.ctypes.data, ln.size, group_log, d_outboards.data_ptr(), d_roots.data_ptr(), fi.ctypes.data,
                                                  fc.ctypes.data, nc.ctypes.data, fc.size, d_slices.data_ptr(), st.data_ptr(), fb.data_ptr(),
                                                  d_have.data_ptr() if d_have is not None else None, scratch.data_ptr(), scratch.numel(),
                                                  _stream(stream)), "b3w_bao_range_slice_ingest_device")
    return dict(range_status=st, range_first_bad=fb)


def sample_rows_ranges(lens, files, first_chunks, n_chunks):
    """-> (range_row_first uint64 [n_ranges + 1], chunk_row_first uint64 [total chunks + 1], provable bool [total chunks]): the record
    rows of ranges (files[r], first_chunks[r], n_chunks[r]) — exactly sample_rows_batch over runs_chunks of the same ranges, the
    per-range firsts from a closed form — and b3w_chain_path_provable of every chunk, in runs_chunks' order"""
    ln = _u64(lens)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    fc, nc = _ranges(first_chunks, n_chunks)
    if fi.size != fc.size:
        raise B3WError(100, f"sample_rows_ranges: {fi.size} files and {fc.size} ranges")
    rrf = np.zeros(fc.size + 1, dtype=np.uint64)
    args = (ln.ctypes.data, ln.size, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size, rrf.ctypes.data)
    if lib().b3w_sample_rows_ranges(*args, None, None) < 0:               # (the ranges are checked before the per-chunk arrays are sized by them)
        raise B3WError(100, "b3w_sample_rows_ranges: a file index is not below the file count, or a range is empty or reaches past its file's chunk count")
    total = int(nc.sum(dtype=np.uint64))
    crf = np.zeros(total + 1, dtype=np.uint64)
    prov = np.zeros(max(total, 1), dtype=np.uint8)
    lib().b3w_sample_rows_ranges(*args, crf.ctypes.data, prov.ctypes.data)
    return rrf, crf, prov[:total].astype(bool)


def plan_samples_range_slices(ctx, lens, d_roots, files, first_chunks, n_chunks, d_slices, stream=0):
    """The prover's side for challenged RUNS of chunks: plan_samples_slices from range slices (range_slices_arena's tensor, or slices
    received and packed as range_slice_layout says) and the files' roots on the device — no outboard, no arena.  Every chunk gets the
    status and, word for word, the records plan_samples_slices gives its own one-chunk slice (the projection of the range slice onto
    it); a bad node spoils the chunks below it and no other; ranges may overlap, repeat and come in any order.  At most three
    launches.  When not to (MI355X, DESIGN.md §8g, against a build of the commit before planning one-chunk slices of the same chunks
    with b3w_sample_plan_slices_device): 64 runs of 1 024 chunks of a 1 GiB file 0.43 ms against 1.71, 4 096 runs of 16 0.53 against
    1.72 — but a range takes at least a wave, so 65 536 runs of ONE chunk take 7.9 ms against 1.7 and the 262 507 runs of a
    half-missing bitmap 23.4 against 13.4: runs of one or two chunks are faster to plan through runs_chunks and plan_samples_slices;
    where between 2 and 16 chunks a run the two cross was not measured.  This wrapper makes its outputs and scratch on every call.
    Returns the dict plan_samples_slices returns, keyed per chunk in runs_chunks order (records, row_first, sample_status, provable),
    plus range_row_first (uint64 [n_ranges + 1]), range_status (int32 CUDA) and range_first_bad (int64 CUDA, -1 for none)."""
    L = lib()
    ln = _u64(lens)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    fc, nc = _ranges(first_chunks, n_chunks)
    rrf, crf, provable = sample_rows_ranges(ln, fi, fc, nc)
    sf = range_slice_layout(ln, fi, fc, nc)
    dev = d_slices.device
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.numel() >= ln.size * 8
    assert d_slices.is_cuda and d_slices.dtype == torch.uint8 and d_slices.is_contiguous() and d_slices.numel() >= int(sf[-1])
    recs = torch.empty((int(rrf[-1]), 32), dtype=torch.int32, device=dev)
    st = torch.full((provable.size,), -1, dtype=torch.int32, device=dev)
    rst = torch.full((fc.size,), -1, dtype=torch.int32, device=dev)
    rfb = torch.full((fc.size,), -2, dtype=torch.int64, device=dev)
    need = L.b3w_bao_range_slice_ingest_scratch_bytes(ln.ctypes.data, ln.size, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _chk(ctx, L.b3w_sample_plan_range_slices_device(ctx.handle, ln.ctypes.data, ln.size, d_roots.data_ptr(), fi.ctypes.data, fc.ctypes.data, nc.ctypes.data,
                                                    fc.size, d_slices.data_ptr(), recs.data_ptr(), st.data_ptr(), rst.data_ptr(), rfb.data_ptr(),
                                                    scratch.data_ptr(), scratch.numel(), _stream(stream)), "b3w_sample_plan_range_slices_device")
    return dict(records=recs, row_first=crf, sample_status=st.cpu().numpy(), provable=provable, range_row_first=rrf, range_status=rst, range_first_bad=rfb)


def prove_samples_range_slices(ctx, lens, d_roots, files, first_chunks, n_chunks, d_slices, batch_steps=4096, consumer=None, commit_key=None, r1cs=None,
                               stream=0):
    """prove_samples_slices over plan_samples_range_slices' plan"""
    s = _stream(stream)
    out = plan_samples_range_slices(ctx, lens, d_roots, files, first_chunks, n_chunks, d_slices, stream=s)
    return _prove_planned(ctx, out, batch_steps, consumer, commit_key, r1cs, s)


def range_slice_host(outboard, length, first_chunk, n_chunks, range_bytes, group_log=0):
    """The slice of one range on the host (no GPU) from the file's outboard of this group_log and range_bytes: the bytes of the
    range's chunks (group_log 0) or of the whole groups it touches (above 0) -> bytes"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    size = range_slice_size(length, first_chunk, n_chunks)
    ob, rb = bytes(outboard), bytes(range_bytes)
    n = num_chunks(length)
    g0 = (first_chunk >> group_log) << group_log
    g1 = min(n, (((first_chunk + n_chunks - 1) >> group_log) + 1) << group_log)
    if len(ob) != group_outboard_size(length, group_log) or len(rb) != min(length, g1 * 1024) - g0 * 1024:
        raise B3WError(100, "range_slice_host: the outboard is not that of a file of this length, or range_bytes not the bytes of the touched groups")
    out = ctypes.create_string_buffer(size)
    got = lib().b3w_bao_range_slice(ob, length, group_log, first_chunk, n_chunks, rb, out, size)
    if got != size:
        raise B3WError(100 if got >= 0 else -got, "b3w_bao_range_slice")
    return out.raw


def decode_range_slice(slice_bytes, length, first_chunk, n_chunks, root):
    """The sequential decoder for one range slice on the host -> (range status as STATUS, first bad chunk or None, the range's bytes
    with the chunks that did not verify left zero)"""
    sl = bytes(slice_bytes)
    rw = np.ascontiguousarray(root, dtype=np.uint32)
    out = np.zeros(max(1, n_chunks) * 1024, dtype=np.uint8)
    st, fb = ctypes.c_int32(), ctypes.c_uint64()
    _chk(None, lib().b3w_bao_range_slice_decode(sl, len(sl), length, first_chunk, n_chunks, rw.ctypes.data, out.ctypes.data, ctypes.byref(st), ctypes.byref(fb)),
         "b3w_bao_range_slice_decode")
    end = min(length, (first_chunk + n_chunks) * 1024) - first_chunk * 1024
    return st.value, (None if fb.value == 2 ** 64 - 1 else fb.value), out[:end].tobytes()


def ingest_range_slice_host(data, outboard, length, first_chunk, n_chunks, root, slice_bytes, group_log=0, have=None):
    """ingest_range_slices for one range on the host (no GPU): data, outboard (and have: the file's bitmap words, numpy uint64, or None)
    are written in place where chunks verify -> (range status as STATUS, first bad chunk or None)"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    d, ob = _writable(data, "data"), _writable(outboard, "outboard")
    if d.size != length or ob.size != group_outboard_size(length, group_log):
        raise B3WError(100, "ingest_range_slice_host: data is not of this length or the outboard not that of a file of this length")
    if have is not None and not (isinstance(have, np.ndarray) and have.dtype == np.uint64 and have.flags.c_contiguous and have.flags.writeable
                                 and have.size == (num_chunks(length) + 63) // 64):
        raise B3WError(100, "ingest_range_slice_host: have is not the writable uint64 bitmap of a file of this length")
    sl = bytes(slice_bytes)
    rw = np.ascontiguousarray(root, dtype=np.uint32)
    if rw.size != 8:
        raise B3WError(100, "ingest_range_slice_host: the root is 8 words")
    st, fb = ctypes.c_int32(), ctypes.c_uint64()
    _chk(None, lib().b3w_bao_range_slice_ingest(sl, len(sl), length, first_chunk, n_chunks, rw.ctypes.data, group_log, d.ctypes.data if d.size else None,
                                                ob.ctypes.data, have.ctypes.data if have is not None else None, ctypes.byref(st), ctypes.byref(fb)),
         "b3w_bao_range_slice_ingest")
    return st.value, (None if fb.value == 2 ** 64 - 1 else fb.value)


# ---- set slices: one slice for all the wanted runs of a file --------------------------------------------------------------
def set_slice_size(length, first_chunks, n_chunks):
    """8 + 64 U_S + the bytes of S: the bao slice of the union S of one file's runs (ascending and disjoint, touching allowed), every
    shared node once"""
    fc, nc = _ranges(first_chunks, n_chunks)
    size = lib().b3w_bao_set_slice_size(length, fc.ctypes.data, nc.ctypes.data, fc.size)
    if not size:
        raise B3WError(100, "b3w_bao_set_slice_size: the list is empty, a run is empty or reaches past the chunk count, or the runs are not ascending and disjoint")
    return size


def set_slice_layout(lens, files, first_chunks, n_chunks):
    """The sets of a range list (ascending by (file, first chunk), disjoint: have_runs' rows as they come) -> dict(set_file uint32
    [n_sets], set_range_first uint32 [n_sets + 1], set_chunk_first uint64 [n_sets + 1], slice_first uint64 [n_sets + 1]): set s is the
    ranges [set_range_first[s], set_range_first[s + 1]) of file set_file[s], its per-chunk statuses lie from set_chunk_first[s], its
    slice from slice_first[s] of the packed slices (every start 8 modulo 16); the last entries are the totals"""
    ln = _u64(lens)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    fc, nc = _ranges(first_chunks, n_chunks)
    if fi.size != fc.size:
        raise B3WError(100, f"set_slice_layout: {fi.size} files and {fc.size} ranges")
    sfile = np.zeros(fc.size + 1, dtype=np.uint32)
    srf = np.zeros(fc.size + 1, dtype=np.uint32)
    scf = np.zeros(fc.size + 1, dtype=np.uint64)
    sf = np.zeros(fc.size + 1, dtype=np.uint64)
    k = ctypes.c_uint32()
    total = lib().b3w_bao_set_slice_batch_layout(ln.ctypes.data, ln.size, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size, sfile.ctypes.data,
                                                 srf.ctypes.data, scf.ctypes.data, sf.ctypes.data, ctypes.byref(k))
    if total < 0:
        raise B3WError(-total, "b3w_bao_set_slice_batch_layout: a file index is not below the file count, a range is empty or reaches past its file's "
                               "chunk count, or the list is not ascending by (file, first chunk) and disjoint")
    k = k.value
    return dict(set_file=sfile[:k].copy(), set_range_first=srf[:k + 1].copy(), set_chunk_first=scf[:k + 1].copy(), slice_first=sf[:k + 1].copy())


def set_slices_arena(ctx, d_arena, offsets, lens, d_outboards, files, first_chunks, n_chunks, group_log=0, stream=0):
    """The provider's side for ALL the wanted runs of a file in one slice: range_slices_arena's arguments, the ranges ascending by
    (file, first chunk) and disjoint - have_runs' rows as they come.  A file's runs make one set slice that carries every node they
    share once; a tile's lanes are busy with every wanted chunk of the tile however the chunks are cut into runs.  At most two
    launches; nothing is verified.  Measured (MI355X, DESIGN.md §8g, against a build of the commit before): the 262 507 runs of a
    half-missing 1 GiB file 3.20 ms against range_slices_arena's 13.22, for 593 MB against 892; but 4 096 scattered runs of 16 take
    0.35 ms against 0.25 and 64 runs of 1 024 0.110 against 0.081 — few long or sparse medium runs stay with the range call.  Returns dict(slices: uint8 CUDA tensor, packed; **set_slice_layout)."""
    off, ln, fi, fc, nc = _range_args("set_slices_arena", d_arena, offsets, lens, d_outboards, files, first_chunks, n_chunks, group_log)
    lay = set_slice_layout(ln, fi, fc, nc)
    d_slices = torch.zeros(int(lay["slice_first"][-1]) if fc.size else 0, dtype=torch.uint8, device=d_outboards.device)
    _chk(ctx, lib().b3w_bao_set_slice_arena_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, d_arena.numel(), off.ctypes.data,
                                                   ln.ctypes.data, ln.size, group_log, d_outboards.data_ptr(), fi.ctypes.data, fc.ctypes.data,
                                                   nc.ctypes.data, fc.size, d_slices.data_ptr(), _stream(stream)), "b3w_bao_set_slice_arena_device")
    return dict(slices=d_slices, **lay)


def ingest_set_slices(ctx, d_arena, offsets, lens, d_outboards, d_roots, files, first_chunks, n_chunks, d_slices, group_log=0, stream=0, d_have=None):
    """The receiver's side for set slices, set_slices_arena's mirror image: every wanted chunk gets the status its own one-chunk slice
    would get, and the chunks of status 0 write what ingest_slices writes for them - bytes, stored path nodes, header, and their bit
    in d_have where one is given.  A bad node keeps out the chunks below it and no other.  At most three launches.  When not to
    (MI355X, DESIGN.md §8g, against a build of the commit before): the 262 507 runs of a half-missing 1 GiB file take 3.70 ms against
    20.86 for ingest_range_slices and 16.85 for ingest_slices over runs_chunks, 65 536 runs of one chunk 1.30 against 5.45 and 2.17 —
    but a set takes a workgroup per touched tile, so 4 096 scattered runs of 16 take 0.78 ms against ingest_range_slices' 0.39, and
    64 runs of 1 024 chunks 0.237 against 0.214: a few long runs or a sparse scatter of medium ones stay with the range call.  This
    wrapper makes its outputs and its scratch on every call; a loop that matters keeps them and calls b3w_bao_set_slice_ingest_device.
    Returns dict(set_status: int32 CUDA, the largest chunk status of each set; set_first_bad: int64 CUDA, the first chunk of the file
    whose status is not 0, -1 for none; chunk_status: int32 CUDA, a wanted chunk each, set s's from set_chunk_first[s];
    **set_slice_layout)."""
    L = lib()
    off, ln, fi, fc, nc = _range_args("ingest_set_slices", d_arena, offsets, lens, d_outboards, files, first_chunks, n_chunks, group_log)
    lay = set_slice_layout(ln, fi, fc, nc)
    dev = d_slices.device
    n_sets = lay["set_file"].size
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.numel() >= ln.size * 8
    assert d_slices.is_cuda and d_slices.dtype == torch.uint8 and d_slices.is_contiguous() and d_slices.numel() >= (int(lay["slice_first"][-1]) if fc.size else 0)
    if d_have is not None:
        _have_tensor("ingest_set_slices", d_have, ln)
    st = torch.full((n_sets,), -1, dtype=torch.int32, device=dev)
    fb = torch.full((n_sets,), -2, dtype=torch.int64, device=dev)
    cs = torch.full((int(lay["set_chunk_first"][-1]),), -1, dtype=torch.int32, device=dev)
    need = L.b3w_bao_set_slice_ingest_scratch_bytes(ln.ctypes.data, ln.size, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _chk(ctx, L.b3w_bao_set_slice_ingest_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, d_arena.numel(), off.ctypes.data,
                                                ln.ctypes.data, ln.size, group_log, d_outboards.data_ptr(), d_roots.data_ptr(), fi.ctypes.data,
                                                fc.ctypes.data, nc.ctypes.data, fc.size, d_slices.data_ptr(), st.data_ptr(), fb.data_ptr(),
                                                cs.data_ptr() if cs.numel() else None, d_have.data_ptr() if d_have is not None else None,
                                                scratch.data_ptr(), scratch.numel(), _stream(stream)), "b3w_bao_set_slice_ingest_device")
    return dict(set_status=st, set_first_bad=fb, chunk_status=cs, **lay)


def plan_samples_set_slices(ctx, lens, d_roots, files, first_chunks, n_chunks, d_slices, stream=0):
    """The prover's side for set slices: plan_samples_range_slices from SET slices (set_slices_arena's or set_slices_packed's tensor,
    or slices received and packed as set_slice_layout says) and the files' roots on the device - no outboard, no arena.  The list is
    the set calls' (ascending by (file, first chunk), disjoint, touching allowed).  Every wanted chunk gets the status and, word for
    word, the records plan_samples_slices gives the projection of its set slice onto it; a bad node spoils the wanted chunks below it,
    in every row under it, and no other.  For such a list a set's wanted chunks in ascending order are the list's chunks in
    runs_chunks order, so the layout is sample_rows_ranges' over the same list: untampered, records and sample_status are byte for
    byte what plan_samples_range_slices writes from range slices of the same list.  At most three launches.  When not to (MI355X, one 1 GiB file, DESIGN.md §8g, against a
    build of the commit before planning the same chunks from range slices and, through runs_chunks, from one-chunk slices): the
    262 507 runs of a half-missing bitmap 5.08 ms against 23.10 and 18.38, 65 536 runs of one chunk 1.53 against 5.95 and 2.01 - but a
    set takes a workgroup per touched tile, so 4 096 scattered runs of 16 take 0.73 ms against plan_samples_range_slices' 0.45, and 64
    runs of 1 024 chunks 0.454 against 0.431: a few long runs or a sparse scatter of medium ones stay with the range planner.  This
    wrapper makes its outputs and scratch on every call.
    Returns the dict plan_samples_range_slices returns with set_status (int32 CUDA, a set each) and set_first_bad (int64 CUDA, the
    first chunk of the file whose status is not 0, -1 for none) for the range pair, plus range_row_first: set s owns the rows
    [range_row_first[set_range_first[s]], range_row_first[set_range_first[s + 1]]) and the statuses from set_chunk_first[s]
    (**set_slice_layout is in the dict)."""
    L = lib()
    ln = _u64(lens)
    fi = np.ascontiguousarray(files, dtype=np.uint32)
    fc, nc = _ranges(first_chunks, n_chunks)
    lay = set_slice_layout(ln, fi, fc, nc)
    rrf, crf, provable = sample_rows_ranges(ln, fi, fc, nc)
    dev = d_slices.device
    n_sets = lay["set_file"].size
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.numel() >= ln.size * 8
    assert d_slices.is_cuda and d_slices.dtype == torch.uint8 and d_slices.is_contiguous() and d_slices.numel() >= (int(lay["slice_first"][-1]) if fc.size else 0)
    recs = torch.empty((int(rrf[-1]), 32), dtype=torch.int32, device=dev)
    st = torch.full((provable.size,), -1, dtype=torch.int32, device=dev)
    sst = torch.full((n_sets,), -1, dtype=torch.int32, device=dev)
    sfb = torch.full((n_sets,), -2, dtype=torch.int64, device=dev)
    need = L.b3w_bao_set_slice_ingest_scratch_bytes(ln.ctypes.data, ln.size, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _chk(ctx, L.b3w_sample_plan_set_slices_device(ctx.handle, ln.ctypes.data, ln.size, d_roots.data_ptr(), fi.ctypes.data, fc.ctypes.data, nc.ctypes.data,
                                                  fc.size, d_slices.data_ptr(), recs.data_ptr(), st.data_ptr(), sst.data_ptr(), sfb.data_ptr(),
                                                  scratch.data_ptr(), scratch.numel(), _stream(stream)), "b3w_sample_plan_set_slices_device")
    return dict(records=recs, row_first=crf, sample_status=st.cpu().numpy(), provable=provable, range_row_first=rrf, set_status=sst, set_first_bad=sfb, **lay)


def prove_samples_set_slices(ctx, lens, d_roots, files, first_chunks, n_chunks, d_slices, batch_steps=4096, consumer=None, commit_key=None, r1cs=None,
                             stream=0):
    """prove_samples_slices over plan_samples_set_slices' plan"""
    s = _stream(stream)
    out = plan_samples_set_slices(ctx, lens, d_roots, files, first_chunks, n_chunks, d_slices, stream=s)
    return _prove_planned(ctx, out, batch_steps, consumer, commit_key, r1cs, s)


def set_slice_host(outboard, length, first_chunks, n_chunks, data, group_log=0):
    """The set slice of one file on the host (no GPU) from its outboard of this group_log and the file's bytes -> bytes"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    fc, nc = _ranges(first_chunks, n_chunks)
    size = set_slice_size(length, fc, nc)
    ob, d = bytes(outboard), bytes(data)
    if len(ob) != group_outboard_size(length, group_log) or len(d) != length:
        raise B3WError(100, "set_slice_host: the outboard is not that of a file of this length, or data not the file's bytes")
    out = ctypes.create_string_buffer(size)
    got = lib().b3w_bao_set_slice(ob, length, group_log, fc.ctypes.data, nc.ctypes.data, fc.size, d, out, size)
    if got != size:
        raise B3WError(100 if got >= 0 else -got, "b3w_bao_set_slice")
    return out.raw


def decode_set_slice(slice_bytes, length, first_chunks, n_chunks, root):
    """The sequential decoder for one set slice on the host -> (set status as STATUS, first bad chunk or None, chunk status int32 a
    wanted chunk, the wanted chunks' bytes at 1024 rank with the chunks that did not verify left zero)"""
    sl = bytes(slice_bytes)
    fc, nc = _ranges(first_chunks, n_chunks)
    rw = np.ascontiguousarray(root, dtype=np.uint32)
    total = int(nc.sum(dtype=np.uint64))
    out = np.zeros(max(1, total) * 1024, dtype=np.uint8)
    cs = np.full(max(1, total), -1, dtype=np.int32)
    st, fb = ctypes.c_int32(), ctypes.c_uint64()
    _chk(None, lib().b3w_bao_set_slice_decode(sl, len(sl), length, fc.ctypes.data, nc.ctypes.data, fc.size, rw.ctypes.data, out.ctypes.data, cs.ctypes.data,
                                              ctypes.byref(st), ctypes.byref(fb)), "b3w_bao_set_slice_decode")
    last = int(fc[-1] + nc[-1])
    end = total * 1024 - (1024 - (length - (last - 1) * 1024) if last == num_chunks(length) else 0)
    return st.value, (None if fb.value == 2 ** 64 - 1 else fb.value), cs[:total].copy(), out[:end].tobytes()


def ingest_set_slice_host(data, outboard, length, first_chunks, n_chunks, root, slice_bytes, group_log=0, have=None):
    """ingest_set_slices for one file on the host (no GPU): data, outboard (and have: the file's bitmap words, numpy uint64, or None)
    are written in place where chunks verify -> (set status as STATUS, first bad chunk or None, chunk status int32 a wanted chunk)"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    d, ob = _writable(data, "data"), _writable(outboard, "outboard")
    if d.size != length or ob.size != group_outboard_size(length, group_log):
        raise B3WError(100, "ingest_set_slice_host: data is not of this length or the outboard not that of a file of this length")
    if have is not None and not (isinstance(have, np.ndarray) and have.dtype == np.uint64 and have.flags.c_contiguous and have.flags.writeable
                                 and have.size == (num_chunks(length) + 63) // 64):
        raise B3WError(100, "ingest_set_slice_host: have is not the writable uint64 bitmap of a file of this length")
    sl = bytes(slice_bytes)
    fc, nc = _ranges(first_chunks, n_chunks)
    rw = np.ascontiguousarray(root, dtype=np.uint32)
    if rw.size != 8:
        raise B3WError(100, "ingest_set_slice_host: the root is 8 words")
    total = int(nc.sum(dtype=np.uint64))
    cs = np.full(max(1, total), -1, dtype=np.int32)
    st, fb = ctypes.c_int32(), ctypes.c_uint64()
    _chk(None, lib().b3w_bao_set_slice_ingest(sl, len(sl), length, fc.ctypes.data, nc.ctypes.data, fc.size, rw.ctypes.data, group_log,
                                              d.ctypes.data if d.size else None, ob.ctypes.data, have.ctypes.data if have is not None else None,
                                              cs.ctypes.data, ctypes.byref(st), ctypes.byref(fb)), "b3w_bao_set_slice_ingest")
    return st.value, (None if fb.value == 2 ** 64 - 1 else fb.value), cs[:total].copy()


# ---- verification: whole files against their outboards ------------------------------------------------------------------
def verify_layout(lens, group_log=0):
    """-> unit_first (numpy uint64 [n_files + 1]): file f's unit statuses are entries [unit_first[f], unit_first[f + 1]) of the packed
    statuses; a unit is a chunk (group_log 0) or a group of 2^group_log chunks"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    ln = _u64(lens)
    unit_first = np.zeros(ln.size + 1, dtype=np.uint64)
    lib().b3w_bao_verify_layout(ln.ctypes.data, ln.size, group_log, unit_first.ctypes.data)
    return unit_first


def verify_batch(ctx, d_arena, offsets, lens, d_outboards, d_roots, group_log=0, stream=0):
    """Bao's decoder over every unit of every file of a batch at once, in a number of launches that does not depend on the file count:
    the files as outboard_batch takes them, d_outboards / d_roots as outboard_batch (group_log 0) or outboard_groups_batch made them —
    or as they arrived from elsewhere.  Returns a dict, everything left on the device: unit_status (uint8 CUDA, packed as unit_first
    says; STATUS / GROUP_STATUS: 0 verified, 1 the unit's bytes, 2 a stored node on its path or the root, 3 the header), unit_first
    (numpy uint64 [n_files + 1]), file_status (int32 CUDA [n_files]: the largest status among the file's units), first_bad (int64 CUDA
    [n_files]: the lowest unit with a non-zero status, -1 = UINT64_MAX where there is none)."""
    L = lib()
    off, ln = _u64(offsets), _u64(lens)
    assert off.size == ln.size
    assert d_arena.is_cuda and d_arena.dtype == torch.uint8 and d_arena.is_contiguous()
    if ln.size and int((off + ln).max()) > d_arena.numel():
        raise B3WError(100, "verify_batch: a file reaches past the end of the arena")
    dev = d_arena.device
    unit_first = verify_layout(ln, group_log)
    ob_first = group_batch_layout(ln, group_log)
    assert d_outboards.is_cuda and d_outboards.dtype == torch.uint8 and d_outboards.is_contiguous() and d_outboards.numel() >= int(ob_first[-1])
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.element_size() == 4 and d_roots.numel() >= ln.size * 8
    unit_status = torch.empty(int(unit_first[-1]), dtype=torch.uint8, device=dev)
    file_status = torch.empty(ln.size, dtype=torch.int32, device=dev)
    first_bad = torch.empty(ln.size, dtype=torch.int64, device=dev)
    need = L.b3w_bao_verify_scratch_bytes(ln.ctypes.data, ln.size)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    _chk(ctx, L.b3w_bao_verify_batch_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, off.ctypes.data, ln.ctypes.data, ln.size,
                                            group_log, d_outboards.data_ptr(), d_roots.data_ptr(), unit_status.data_ptr(), file_status.data_ptr(),
                                            first_bad.data_ptr(), scratch.data_ptr() if need else None, need, _stream(stream)),
         "b3w_bao_verify_batch_device")
    return dict(unit_status=unit_status, unit_first=unit_first, file_status=file_status, first_bad=first_bad)


def verify_host(data, outboard, root, group_log=0):
    """verify_batch for one file on the host (no GPU) -> (unit_status numpy uint8, file_status, first_bad: an int, 2^64 - 1 = none)"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    data = bytes(data)
    ob = outboard.cpu().numpy().tobytes() if isinstance(outboard, torch.Tensor) else bytes(outboard)
    if len(ob) != group_outboard_size(len(data), group_log):
        raise B3WError(100, "verify_host: the outboard's size is not that of a file of this length")
    rw = np.ascontiguousarray(root, dtype=np.uint32)
    units = (num_chunks(len(data)) + (1 << group_log) - 1) >> group_log
    st = np.zeros(units, dtype=np.uint8)
    fs, fb = ctypes.c_int32(), ctypes.c_uint64()
    _chk(None, lib().b3w_bao_verify(data, len(data), ob, group_log, rw.ctypes.data, st.ctypes.data, ctypes.byref(fs), ctypes.byref(fb)), "b3w_bao_verify")
    return st, fs.value, fb.value


# ---- updates in place after writes to resident files -------------------------------------------------------------------------
def chunk_ranges(byte_offsets, byte_counts):
    """byte ranges [byte_offsets[i], + byte_counts[i]) within one file -> (first_chunks, n_chunks), numpy uint64, the chunks each write
    touches, in the order given.  Writes of no bytes are dropped; overlaps stay (the update calls merge them)."""
    off = np.atleast_1d(np.asarray(byte_offsets)).astype(np.int64)
    cnt = np.atleast_1d(np.asarray(byte_counts)).astype(np.int64)
    if off.shape != cnt.shape or off.ndim != 1:
        raise B3WError(100, f"chunk_ranges: {off.size} offsets and {cnt.size} counts")
    if (off < 0).any() or (cnt < 0).any():
        raise B3WError(100, "chunk_ranges: a negative offset or count")
    keep = cnt > 0
    off, cnt = off[keep], cnt[keep]
    first = off // 1024
    last = (off + cnt - 1) // 1024
    return first.astype(np.uint64), (last - first + 1).astype(np.uint64)


def _ranges(first_chunks, n_chunks):
    fc, nc = _u64(np.atleast_1d(first_chunks)), _u64(np.atleast_1d(n_chunks))
    if fc.size != nc.size:
        raise B3WError(100, f"{fc.size} first chunks and {nc.size} chunk counts")
    return fc, nc


def outboard_update_batch(ctx, d_arena, offsets, lens, d_outboards, d_roots, files, first_chunks, n_chunks, group_log=0, ob_first=None, stream=0):
    """After writes into resident files: d_outboards and d_roots, as outboard_batch (group_log 0) or outboard_groups_batch made them
    BEFORE the writes, updated IN PLACE to what those calls give for d_arena as it is now.  The dirty ranges are chunks
    [first_chunks[i], + n_chunks[i]) of file files[i] (chunk_ranges() makes them from byte ranges); they must cover every changed byte,
    may be unsorted, overlapping or repeated, and lengths do not change.  Only dirty chunks (whole groups for group_log > 0) are hashed and
    only the nodes above them written, in at most four launches; a dirty file of at most 64 chunks is rehashed whole.  A changed chunk
    the list misses is NOT detected: verify_batch then reports status 1 at that unit.  ob_first: batch_layout / group_batch_layout of
    lens, computed here when None (pass it for very many files: the call itself does no work per file).  The scratch (32 bytes a dirty
    tile) is made here.  Break-even against the batch call (MI355X): the cost follows the dirty TILES of 1 024 chunks and
    the number of ranges.  One 4 KiB write into 1 GiB takes 0.09 ms against 0.42; with a write in every tile (4 096 scattered writes,
    1.6 % of the chunks) the two are level; beyond, and with every chunk dirty, outboard_batch is the faster call."""
    L = lib()
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    off, ln = _u64(offsets), _u64(lens)
    fi = np.ascontiguousarray(np.atleast_1d(files), dtype=np.uint32)
    fc, nc = _ranges(first_chunks, n_chunks)
    if off.size != ln.size or fi.size != fc.size:
        raise B3WError(100, f"outboard_update_batch: {off.size} offsets and {ln.size} lengths, {fi.size} files and {fc.size} ranges")
    assert d_arena.is_cuda and d_arena.dtype == torch.uint8 and d_arena.is_contiguous()
    assert d_outboards.is_cuda and d_outboards.dtype == torch.uint8 and d_outboards.is_contiguous()
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.element_size() == 4 and d_roots.numel() >= ln.size * 8
    obf = group_batch_layout(ln, group_log) if ob_first is None else _u64(ob_first)
    if obf.size != ln.size + 1 or d_outboards.numel() < int(obf[-1]):
        raise B3WError(100, "outboard_update_batch: ob_first or d_outboards is not of these lengths' layout")
    if fi.size == 0:
        return
    if int(fi.max()) >= ln.size:
        raise B3WError(100, f"outboard_update_batch: file index {int(fi.max())} is not below the file count {ln.size}")
    need = L.b3w_bao_update_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)
    scratch = torch.empty(need, dtype=torch.uint8, device=d_arena.device) if need else None
    _chk(ctx, L.b3w_bao_outboard_update_batch_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, d_arena.numel(), off.ctypes.data,
                                                     ln.ctypes.data, ln.size, group_log, obf.ctypes.data, d_outboards.data_ptr(), d_roots.data_ptr(),
                                                     fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size, scratch.data_ptr() if need else None,
                                                     need, _stream(stream)), "b3w_bao_outboard_update_batch_device")


def update_host(data, outboard, root, first_chunks, n_chunks, group_log=0):
    """outboard_update_batch for one file on the host (no GPU) -> (outboard bytes, root as uint32 numpy [8]): the outboard (full, or the
    group outboard of group_log) and root of `data` as it is now from those of before the writes and the dirty chunk ranges"""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    data = bytes(data)
    ob = bytearray(outboard.cpu().numpy().tobytes() if isinstance(outboard, torch.Tensor) else bytes(outboard))
    if len(ob) != group_outboard_size(len(data), group_log):
        raise B3WError(100, "update_host: the outboard's size is not that of a file of this length")
    fc, nc = _ranges(first_chunks, n_chunks)
    rw = np.array(root, dtype=np.uint32)
    if rw.size != 8:
        raise B3WError(100, "update_host: the root is 8 words")
    buf = (ctypes.c_uint8 * len(ob)).from_buffer(ob)
    _chk(None, lib().b3w_bao_outboard_update(data, len(data), ctypes.addressof(buf), group_log, fc.ctypes.data, nc.ctypes.data, fc.size, rw.ctypes.data),
         "b3w_bao_outboard_update")
    del buf
    return bytes(ob), rw


# ---- verification of listed chunk ranges of resident files -------------------------------------------------------------------
def verify_ranges_batch(ctx, d_arena, offsets, lens, d_outboards, d_roots, files, first_chunks, n_chunks, group_log=0, ob_first=None, unit_first=None,
                        unit_status=None, stream=0):
    """verify_batch for the units that hold the listed chunks alone: ranges are chunks [first_chunks[i], + n_chunks[i]) of file
    files[i] (chunk_ranges() makes them from byte extents), unsorted, overlapping or repeated as they come.  Only listed units are
    hashed and only the stored nodes above them read, in at most five launches.  Returns a dict, everything but unit_first left on the
    device: unit_status (uint8 CUDA, packed as unit_first says): the byte of every unit with a listed chunk is what verify_batch
    writes there, NO OTHER BYTE IS WRITTEN (a listed file of at most 64 chunks excepted: all its bytes are) — so pass the same
    `unit_status` buffer to successive calls to build up the statuses of what a scrub has covered; without one a new buffer filled
    with 0xFF is made.  range_status (int32 CUDA [n_ranges]: the largest status among the units range i touches) and range_first_bad
    (int64 CUDA [n_ranges]: the lowest unit index within the file with a non-zero status among them, -1 = UINT64_MAX where there is
    none), in the order the ranges were given; unit_first (numpy uint64 [n_files + 1]).  ob_first / unit_first: group_batch_layout /
    verify_layout of lens, computed here when None (pass them for very many files: the call itself does no work per file).  When
    to call verify_batch instead (MI355X): one 4 KiB range of a 1 GiB file takes 0.10 ms against verify_batch's 0.43,
    1 024 scattered ones 0.23, 4 096 (a range in nearly every tile) 0.41, which is level; with every chunk listed it takes 0.59, 1.36
    times verify_batch.  So: this call while the ranges leave tiles out or most chunks of the tiles they touch unlisted, verify_batch
    when most of the file is listed."""
    L = lib()
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    off, ln = _u64(offsets), _u64(lens)
    fi = np.ascontiguousarray(np.atleast_1d(files), dtype=np.uint32)
    fc, nc = _ranges(first_chunks, n_chunks)
    if off.size != ln.size or fi.size != fc.size:
        raise B3WError(100, f"verify_ranges_batch: {off.size} offsets and {ln.size} lengths, {fi.size} files and {fc.size} ranges")
    assert d_arena.is_cuda and d_arena.dtype == torch.uint8 and d_arena.is_contiguous()
    assert d_outboards.is_cuda and d_outboards.dtype == torch.uint8 and d_outboards.is_contiguous()
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.element_size() == 4 and d_roots.numel() >= ln.size * 8
    obf = group_batch_layout(ln, group_log) if ob_first is None else _u64(ob_first)
    if obf.size != ln.size + 1 or d_outboards.numel() < int(obf[-1]):
        raise B3WError(100, "verify_ranges_batch: ob_first or d_outboards is not of these lengths' layout")
    uf = verify_layout(ln, group_log) if unit_first is None else _u64(unit_first)
    if uf.size != ln.size + 1:
        raise B3WError(100, "verify_ranges_batch: unit_first is not of these lengths' layout")
    dev = d_arena.device
    if unit_status is None:
        unit_status = torch.full((int(uf[-1]),), 0xFF, dtype=torch.uint8, device=dev)
    assert unit_status.is_cuda and unit_status.dtype == torch.uint8 and unit_status.is_contiguous() and unit_status.numel() >= int(uf[-1])
    range_status = torch.empty(fi.size, dtype=torch.int32, device=dev)
    range_first_bad = torch.empty(fi.size, dtype=torch.int64, device=dev)
    out = dict(unit_status=unit_status, range_status=range_status, range_first_bad=range_first_bad, unit_first=uf)
    if fi.size == 0:
        return out
    if int(fi.max()) >= ln.size:
        raise B3WError(100, f"verify_ranges_batch: file index {int(fi.max())} is not below the file count {ln.size}")
    need = L.b3w_bao_verify_ranges_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    _chk(ctx, L.b3w_bao_verify_ranges_batch_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, d_arena.numel(), off.ctypes.data,
                                                   ln.ctypes.data, ln.size, group_log, obf.ctypes.data, d_outboards.data_ptr(), d_roots.data_ptr(),
                                                   fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size, uf.ctypes.data, unit_status.data_ptr(),
                                                   range_status.data_ptr(), range_first_bad.data_ptr(), scratch.data_ptr() if need else None, need,
                                                   _stream(stream)), "b3w_bao_verify_ranges_batch_device")
    return out


def verify_ranges_host(data, outboard, root, first_chunks, n_chunks, group_log=0):
    """verify_ranges_batch for one file on the host (no GPU) -> (unit_status numpy uint8, range_status numpy int32, range_first_bad numpy
    uint64: 2^64 - 1 = none).  unit_status holds verify_host's byte at every unit with a listed chunk and 0xFF everywhere else (the
    host walk writes listed units only, whatever the file's size); only the listed units' bytes and the nodes above them are read."""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    data = bytes(data)
    ob = outboard.cpu().numpy().tobytes() if isinstance(outboard, torch.Tensor) else bytes(outboard)
    if len(ob) != group_outboard_size(len(data), group_log):
        raise B3WError(100, "verify_ranges_host: the outboard's size is not that of a file of this length")
    fc, nc = _ranges(first_chunks, n_chunks)
    rw = np.ascontiguousarray(root, dtype=np.uint32)
    if rw.size != 8:
        raise B3WError(100, "verify_ranges_host: the root is 8 words")
    units = (num_chunks(len(data)) + (1 << group_log) - 1) >> group_log
    st = np.full(units, 0xFF, dtype=np.uint8)
    rs, rf = np.zeros(fc.size, dtype=np.int32), np.zeros(fc.size, dtype=np.uint64)
    _chk(None, lib().b3w_bao_verify_ranges(data, len(data), ob, group_log, rw.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size, st.ctypes.data,
                                           rs.ctypes.data, rf.ctypes.data), "b3w_bao_verify_ranges")
    return st, rs, rf


# ---- the sparse calls from packed chunk bytes: files that are not resident ---------------------------------------------------
def _packed_args(what, lens, files, first_chunks, n_chunks, group_log):
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    ln = _u64(lens)
    fi = np.ascontiguousarray(np.atleast_1d(files), dtype=np.uint32)
    fc, nc = _ranges(first_chunks, n_chunks)
    if fi.size != fc.size:
        raise B3WError(100, f"{what}: {fi.size} files and {fc.size} ranges")
    return ln, fi, fc, nc


def packed_layout(lens, files, first_chunks, n_chunks, group_log=0):
    """Where the chunks that a sparse call over ranges (files[i], first_chunks[i], n_chunks[i]) reads lie in a packed buffer
    (b3w_bao_packed_layout): a file of at most 64 chunks lists all its chunks, any other one the whole groups of 2^group_log chunks its
    ranges touch; every listed chunk takes a slot of 1 024 bytes, files ascending, a file's distinct chunks ascending.  Returns a dict:
    range_slot, range_first, range_chunks (numpy uint64 [n_ranges]: the file's chunks [range_first[i], + range_chunks[i]) go to slot
    range_slot[i] onwards; 0 chunks for an empty range), total_slots, total_bytes (the end of the last byte a call reads)."""
    ln, fi, fc, nc = _packed_args("packed_layout", lens, files, first_chunks, n_chunks, group_log)
    slot, first, count = (np.zeros(fi.size, dtype=np.uint64) for _ in range(3))
    slots, nbytes = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().b3w_bao_packed_layout(ln.ctypes.data, ln.size, group_log, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size, slot.ctypes.data,
                                     first.ctypes.data, count.ctypes.data, ctypes.addressof(slots), ctypes.addressof(nbytes))
    if rc:
        raise B3WError(rc, "b3w_bao_packed_layout: a file index is not below the file count, a range reaches past its file's chunk count, or a file has more than 2^30 chunks")
    return dict(range_slot=slot, range_first=first, range_chunks=count, total_slots=slots.value, total_bytes=nbytes.value)


def pack_ranges(source, offsets, lens, files, first_chunks, n_chunks, group_log=0, device="cuda"):
    """The packed buffer of these ranges (uint8 [total_slots, 1024] on `device`, zero behind a short last chunk) gathered from `source`,
    where file f is bytes [offsets[f], + lens[f]): host bytes, a numpy array or a CUDA tensor, as chunk_bytes_batch takes them.  This is
    the gather a caller with the file on disk does itself: read range i's range_chunks[i] chunks from chunk range_first[i] on to
    1024 * range_slot[i] (packed_layout)."""
    lay = packed_layout(lens, files, first_chunks, n_chunks, group_log)
    fi = np.ascontiguousarray(np.atleast_1d(files), dtype=np.int64)
    cnt = lay["range_chunks"].astype(np.int64)
    dev = source.device if isinstance(source, torch.Tensor) else device
    out = torch.zeros((lay["total_slots"], 1024), dtype=torch.uint8, device=dev)
    if not cnt.sum():
        return out
    within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)          # 0 .. range_chunks[i] - 1 for every range in turn
    slots, at = np.unique(np.repeat(lay["range_slot"].astype(np.int64), cnt) + within, return_index=True)
    rows = chunk_bytes_batch(source, offsets, lens, np.repeat(fi, cnt)[at], (np.repeat(lay["range_first"].astype(np.int64), cnt) + within)[at], device=dev)
    out[torch.from_numpy(slots).to(out.device)] = rows.to(out.device)
    return out


def _packed_tensor(what, d_packed, lay):
    assert d_packed.is_cuda and d_packed.dtype == torch.uint8 and d_packed.is_contiguous(), what
    if d_packed.numel() < lay["total_bytes"]:
        raise B3WError(100, f"{what}: d_packed has {d_packed.numel()} bytes, the listed chunks take {lay['total_bytes']} (packed_layout)")


def outboard_update_packed(ctx, d_packed, lens, d_outboards, d_roots, files, first_chunks, n_chunks, group_log=0, ob_first=None, stream=0):
    """outboard_update_batch for files that are NOT resident: d_packed (uint8 CUDA, any alignment) holds the listed chunks of these
    ranges alone, as they are NOW, placed as packed_layout says (pack_ranges makes it), in place of d_arena and offsets.  Every byte of
    d_outboards and d_roots ends up what outboard_update_batch leaves there for an arena with the same file bytes; the same four
    launches at most, the same scratch.  When not to (MI355X): a file that IS resident.  The three packed calls are never
    faster than their arena counterparts (1 to 2 µs behind with a few ranges; with 4 096 ranges 0.02 ms behind on one 1 GiB file, 0.17 ms
    in its range slices, 0.07 to 0.12 ms over 4 096 small files: the layout on the host); what they save is the memory and the upload."""
    L = lib()
    ln, fi, fc, nc = _packed_args("outboard_update_packed", lens, files, first_chunks, n_chunks, group_log)
    assert d_outboards.is_cuda and d_outboards.dtype == torch.uint8 and d_outboards.is_contiguous()
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.element_size() == 4 and d_roots.numel() >= ln.size * 8
    obf = group_batch_layout(ln, group_log) if ob_first is None else _u64(ob_first)
    if obf.size != ln.size + 1 or d_outboards.numel() < int(obf[-1]):
        raise B3WError(100, "outboard_update_packed: ob_first or d_outboards is not of these lengths' layout")
    if fi.size == 0:
        return
    _packed_tensor("outboard_update_packed", d_packed, packed_layout(ln, fi, fc, nc, group_log))
    need = L.b3w_bao_update_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)
    scratch = torch.empty(need, dtype=torch.uint8, device=d_outboards.device) if need else None
    _chk(ctx, L.b3w_bao_outboard_update_packed_device(ctx.handle, d_packed.data_ptr() if d_packed.numel() else None, d_packed.numel(), ln.ctypes.data, ln.size,
                                                      group_log, obf.ctypes.data, d_outboards.data_ptr(), d_roots.data_ptr(), fi.ctypes.data, fc.ctypes.data,
                                                      nc.ctypes.data, fi.size, scratch.data_ptr() if need else None, need, _stream(stream)),
         "b3w_bao_outboard_update_packed_device")


def verify_ranges_packed(ctx, d_packed, lens, d_outboards, d_roots, files, first_chunks, n_chunks, group_log=0, ob_first=None, unit_first=None,
                         unit_status=None, stream=0):
    """verify_ranges_batch for files that are NOT resident — the range a reader just fetched, against the outboard that is: d_packed
    (uint8 CUDA, any alignment; pack_ranges makes it) holds the listed chunks of these ranges alone, placed as packed_layout says, in
    place of d_arena and offsets.  The same dict with the same bytes as verify_ranges_batch gives for an arena with the same file bytes;
    the same five launches at most, the same scratch."""
    L = lib()
    ln, fi, fc, nc = _packed_args("verify_ranges_packed", lens, files, first_chunks, n_chunks, group_log)
    assert d_outboards.is_cuda and d_outboards.dtype == torch.uint8 and d_outboards.is_contiguous()
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.element_size() == 4 and d_roots.numel() >= ln.size * 8
    obf = group_batch_layout(ln, group_log) if ob_first is None else _u64(ob_first)
    if obf.size != ln.size + 1 or d_outboards.numel() < int(obf[-1]):
        raise B3WError(100, "verify_ranges_packed: ob_first or d_outboards is not of these lengths' layout")
    uf = verify_layout(ln, group_log) if unit_first is None else _u64(unit_first)
    if uf.size != ln.size + 1:
        raise B3WError(100, "verify_ranges_packed: unit_first is not of these lengths' layout")
    dev = d_outboards.device
    if unit_status is None:
        unit_status = torch.full((int(uf[-1]),), 0xFF, dtype=torch.uint8, device=dev)
    assert unit_status.is_cuda and unit_status.dtype == torch.uint8 and unit_status.is_contiguous() and unit_status.numel() >= int(uf[-1])
    range_status = torch.empty(fi.size, dtype=torch.int32, device=dev)
    range_first_bad = torch.empty(fi.size, dtype=torch.int64, device=dev)
    out = dict(unit_status=unit_status, range_status=range_status, range_first_bad=range_first_bad, unit_first=uf)
    if fi.size == 0:
        return out
    _packed_tensor("verify_ranges_packed", d_packed, packed_layout(ln, fi, fc, nc, group_log))
    need = L.b3w_bao_verify_ranges_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    _chk(ctx, L.b3w_bao_verify_ranges_packed_device(ctx.handle, d_packed.data_ptr() if d_packed.numel() else None, d_packed.numel(), ln.ctypes.data, ln.size,
                                                    group_log, obf.ctypes.data, d_outboards.data_ptr(), d_roots.data_ptr(), fi.ctypes.data, fc.ctypes.data,
                                                    nc.ctypes.data, fi.size, uf.ctypes.data, unit_status.data_ptr(), range_status.data_ptr(),
                                                    range_first_bad.data_ptr(), scratch.data_ptr() if need else None, need, _stream(stream)),
         "b3w_bao_verify_ranges_packed_device")
    return out


def range_slices_packed(ctx, d_packed, lens, d_outboards, files, first_chunks, n_chunks, group_log=0, stream=0):
    """range_slices_arena for files that are NOT resident — the range slices have_runs asks a provider for: d_packed (uint8 CUDA, any
    alignment; pack_ranges makes it) holds the listed chunks of these ranges alone, placed as packed_layout says (at group_log > 0 the
    whole groups the ranges touch, which are hashed), in place of d_arena and offsets.  The same dict, byte for byte."""
    ln, fi, fc, nc = _packed_args("range_slices_packed", lens, files, first_chunks, n_chunks, group_log)
    ob_first = group_batch_layout(ln, group_log)
    assert d_outboards.is_cuda and d_outboards.dtype == torch.uint8 and d_outboards.is_contiguous() and d_outboards.numel() >= int(ob_first[-1])
    sf = range_slice_layout(ln, fi, fc, nc)
    _packed_tensor("range_slices_packed", d_packed, packed_layout(ln, fi, fc, nc, group_log))
    d_slices = torch.zeros(int(sf[-1]), dtype=torch.uint8, device=d_outboards.device)
    _chk(ctx, lib().b3w_bao_range_slice_packed_device(ctx.handle, d_packed.data_ptr() if d_packed.numel() else None, d_packed.numel(), ln.ctypes.data, ln.size,
                                                      group_log, d_outboards.data_ptr(), fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size,
                                                      d_slices.data_ptr(), _stream(stream)), "b3w_bao_range_slice_packed_device")
    return dict(slices=d_slices, slice_first=sf)


def set_slices_packed(ctx, d_packed, lens, d_outboards, files, first_chunks, n_chunks, group_log=0, stream=0):
    """set_slices_arena for files that are NOT resident - the multi-range request have_runs produces, answered by a provider whose file
    is on disk: d_packed (uint8 CUDA, any alignment; pack_ranges makes it) holds the listed chunks of these ranges alone, placed as
    packed_layout says (at group_log > 0 the whole groups the set touches, which are hashed; all of a file of at most 64 chunks), in
    place of d_arena and offsets.  The same dict, byte for byte.  At most two launches.  When not to (MI355X, DESIGN.md §8g, against the
    commit before's set_slices_arena over the resident 1 GiB file): a file that IS resident - never faster, and far behind with many
    runs (the layout over the run list on the host): the half-missing shape 7.04 ms against 3.18, 65 536 runs of one chunk 1.80
    against 0.79, 64 runs of 1 024 chunks 0.134 against 0.113; what it saves is the memory and the upload."""
    ln, fi, fc, nc = _packed_args("set_slices_packed", lens, files, first_chunks, n_chunks, group_log)
    lay = set_slice_layout(ln, fi, fc, nc)
    ob_first = group_batch_layout(ln, group_log)
    assert d_outboards.is_cuda and d_outboards.dtype == torch.uint8 and d_outboards.is_contiguous() and d_outboards.numel() >= int(ob_first[-1])
    if fc.size:
        _packed_tensor("set_slices_packed", d_packed, packed_layout(ln, fi, fc, nc, group_log))
    d_slices = torch.zeros(int(lay["slice_first"][-1]) if fc.size else 0, dtype=torch.uint8, device=d_outboards.device)
    _chk(ctx, lib().b3w_bao_set_slice_packed_device(ctx.handle, d_packed.data_ptr() if d_packed.numel() else None, d_packed.numel(), ln.ctypes.data, ln.size,
                                                    group_log, d_outboards.data_ptr(), fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size,
                                                    d_slices.data_ptr(), _stream(stream)), "b3w_bao_set_slice_packed_device")
    return dict(slices=d_slices, **lay)


# ---- slices taken into packed chunk slots: the receiver's side for files that are not resident ------------------------------
def chunk_slots(lens, files, first_chunks, n_chunks):
    """The slots of a packed receiver, one per listed chunk in the order of the per-chunk statuses: the ranges (files[r],
    first_chunks[r], n_chunks[r]) as given, a range's chunks ascending (one-chunk samples: n_chunks all 1).  -> (file uint32, chunk
    uint64, byte_offset uint64, nbytes uint32), arrays over the slots: slot k holds chunk[k] of file[k], whose nbytes[k] =
    min(1024, len - 1024 chunk) bytes belong at byte_offset[k] = 1024 chunk[k] of the file.  Host only."""
    ln = _u64(lens)
    fi = np.ascontiguousarray(np.atleast_1d(files), dtype=np.uint32)
    fc, nc = _ranges(first_chunks, n_chunks)
    if fi.size != fc.size:
        raise B3WError(100, f"chunk_slots: {fi.size} files and {fc.size} ranges")
    if fi.size and int(fi.max()) >= ln.size:
        raise B3WError(100, "chunk_slots: a file index is not below the file count")
    n = np.maximum((ln[fi] + np.uint64(1023)) // np.uint64(1024), np.uint64(1))
    if fi.size and ((fc >= n) | (nc > n - np.minimum(fc, n))).any():
        raise B3WError(100, "chunk_slots: a range reaches past its file's chunk count")
    f, c = runs_chunks(fi, fc, nc)
    off = c * np.uint64(1024)
    left = ln[f] - np.minimum(off, ln[f])
    return f, c, off, np.minimum(left, np.uint64(1024)).astype(np.uint32)


def scatter_chunks(dest, chunks_host, chunk_status, slots):
    """What a receiver does after the copy to the host: the VERIFIED chunks of a slot buffer to their places in the files.
    chunks_host: the slot buffer on the host (numpy uint8 or a CPU tensor, 1 024 bytes a slot); chunk_status: a status per slot (None:
    every slot verified), only those of status 0 are written; slots: chunk_slots' tuple for the call's list; dest: one entry per file,
    a writable buffer of the file's length (bytearray, numpy uint8, memoryview) or an object with seek(offset) and write(bytes).
    Verified chunks that touch - neighbouring slots, neighbouring chunks of one file - go out in ONE write.  -> the bytes written."""
    f, c, off, nb = slots
    buf = chunks_host.numpy() if isinstance(chunks_host, torch.Tensor) else np.asarray(chunks_host)
    buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    if buf.size < 1024 * f.size:
        raise B3WError(100, f"scatter_chunks: the slot buffer has {buf.size} bytes, {f.size} slots take {1024 * f.size}")
    ok = nb > 0
    if chunk_status is not None:
        st = chunk_status.cpu().numpy() if isinstance(chunk_status, torch.Tensor) else np.asarray(chunk_status)
        if st.size != f.size:
            raise B3WError(100, f"scatter_chunks: {st.size} statuses for {f.size} slots")
        ok &= st.reshape(-1) == 0
    at = np.flatnonzero(ok)
    if not at.size:
        return 0
    # slot k + 1 goes on where slot k ended: the next slot, the next chunk of the same file, behind a whole chunk
    joins = (np.diff(at) == 1) & (f[at[1:]] == f[at[:-1]]) & (c[at[1:]] == c[at[:-1]] + np.uint64(1)) & (nb[at[:-1]] == 1024)
    heads = np.flatnonzero(np.concatenate([[True], ~joins]))
    tails = np.concatenate([heads[1:], [at.size]]) - 1
    total = 0
    for h, t in zip(heads, tails):                                       # a step a WRITE, not a chunk
        k0, k1 = int(at[h]), int(at[t])
        nbytes = 1024 * (k1 - k0) + int(nb[k1])
        src, d, o = buf[1024 * k0:1024 * k0 + nbytes], dest[int(f[k0])], int(off[k0])
        if hasattr(d, "write"):
            d.seek(o)
            d.write(src.tobytes())
        else:
            a = _writable(d, "a destination")
            if o + nbytes > a.size:
                raise B3WError(100, f"scatter_chunks: file {int(f[k0])}'s buffer has {a.size} bytes, the write ends at {o + nbytes}")
            a[o:o + nbytes] = src
        total += nbytes
    return total


def _receive_args(what, lens, d_outboards, d_roots, files, d_slices, slices_bytes, group_log, d_have, d_chunks, n_slots):
    """the checks the three packed receivers share -> (the slot buffer, its pointer or None)"""
    ln = _u64(lens)
    assert d_slices.is_cuda and d_slices.dtype == torch.uint8 and d_slices.is_contiguous() and d_slices.numel() >= slices_bytes, what
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.numel() >= ln.size * 8, what
    if d_outboards is not None:
        ob_first = group_batch_layout(ln, group_log)
        assert d_outboards.is_cuda and d_outboards.dtype == torch.uint8 and d_outboards.is_contiguous() and d_outboards.numel() >= int(ob_first[-1]), what
    if d_have is not None:
        _have_tensor(what, d_have, ln)
    if d_chunks is None:
        d_chunks = torch.zeros((n_slots, 1024), dtype=torch.uint8, device=d_slices.device)
    assert d_chunks.is_cuda and d_chunks.dtype == torch.uint8 and d_chunks.is_contiguous(), what
    return d_chunks, (d_chunks.data_ptr() if d_chunks.numel() else None)


def ingest_slices_packed(ctx, lens, d_outboards, d_roots, files, chunks, d_slices, group_log=0, stream=0, d_have=None, d_chunks=None):
    """ingest_slices for files that are NOT resident: the verified chunks go to a SLOT BUFFER, sample i to d_chunks[1024 i : ] (uint8
    CUDA, 16-byte aligned; None: made here, zeroed), in place of d_arena and offsets.  Every status, outboard byte and bitmap bit is
    what ingest_slices gives for the same slices; a slice that does not verify leaves its slot alone, a short last chunk the rest of
    its slot.  d_outboards=None: DECODE - nothing but slots, statuses and the bitmap is written.  One launch.  Returns
    ingest_slices' dict plus chunks (the slot buffer) and slot_first (numpy uint64 [n_samples + 1]: sample i's slot, the total)."""
    ln, fi, fc, nc = _packed_args("ingest_slices_packed", lens, files, chunks, np.ones(np.size(chunks), dtype=np.uint64), group_log)
    sf = slice_layout(ln, fi, fc)
    d_chunks, p_chunks = _receive_args("ingest_slices_packed", ln, d_outboards, d_roots, fi, d_slices, int(sf[-1]), group_log, d_have, d_chunks, fc.size)
    st = torch.full((fc.size,), -1, dtype=torch.int32, device=d_slices.device)
    _chk(ctx, lib().b3w_bao_slice_ingest_packed_device(ctx.handle, p_chunks, d_chunks.numel(), ln.ctypes.data, ln.size, group_log,
                                                       d_outboards.data_ptr() if d_outboards is not None else None, d_roots.data_ptr(), fi.ctypes.data,
                                                       fc.ctypes.data, fc.size, d_slices.data_ptr(), st.data_ptr(),
                                                       d_have.data_ptr() if d_have is not None else None, _stream(stream)), "b3w_bao_slice_ingest_packed_device")
    return dict(sample_status=st, chunks=d_chunks, slot_first=np.arange(fc.size + 1, dtype=np.uint64))


def ingest_range_slices_packed(ctx, lens, d_outboards, d_roots, files, first_chunks, n_chunks, d_slices, group_log=0, stream=0, d_have=None, d_chunks=None):
    """ingest_range_slices for files that are NOT resident: range r's chunk c goes to slot slot_first[r] + (c - first_chunks[r]) of
    d_chunks, slot_first the running sum of the counts (chunk_slots gives every slot's file position) - overlapping ranges each have
    their own slots.  Statuses, outboards and bitmap as ingest_range_slices; d_outboards=None: decode.  At most three launches.
    Returns ingest_range_slices' dict plus chunks and slot_first (numpy uint64 [n_ranges + 1])."""
    L = lib()
    ln, fi, fc, nc = _packed_args("ingest_range_slices_packed", lens, files, first_chunks, n_chunks, group_log)
    sf = range_slice_layout(ln, fi, fc, nc)
    slot_first = np.concatenate([[0], np.cumsum(nc)]).astype(np.uint64)
    d_chunks, p_chunks = _receive_args("ingest_range_slices_packed", ln, d_outboards, d_roots, fi, d_slices, int(sf[-1]), group_log, d_have, d_chunks,
                                       int(slot_first[-1]))
    dev = d_slices.device
    st = torch.full((fc.size,), -1, dtype=torch.int32, device=dev)
    fb = torch.full((fc.size,), -2, dtype=torch.int64, device=dev)
    need = L.b3w_bao_range_slice_ingest_scratch_bytes(ln.ctypes.data, ln.size, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _chk(ctx, L.b3w_bao_range_slice_ingest_packed_device(ctx.handle, p_chunks, d_chunks.numel(), ln.ctypes.data, ln.size, group_log,
                                                         d_outboards.data_ptr() if d_outboards is not None else None, d_roots.data_ptr(), fi.ctypes.data,
                                                         fc.ctypes.data, nc.ctypes.data, fc.size, d_slices.data_ptr(), st.data_ptr(), fb.data_ptr(),
                                                         d_have.data_ptr() if d_have is not None else None, scratch.data_ptr(), scratch.numel(),
                                                         _stream(stream)), "b3w_bao_range_slice_ingest_packed_device")
    return dict(range_status=st, range_first_bad=fb, chunks=d_chunks, slot_first=slot_first)


def ingest_set_slices_packed(ctx, lens, d_outboards, d_roots, files, first_chunks, n_chunks, d_slices, group_log=0, stream=0, d_have=None, d_chunks=None):
    """ingest_set_slices for files that are NOT resident - the download of the missing half of a file into 537 MB of slots where the
    arena call needs the resident GiB: set s's wanted chunk of rank k goes to slot set_chunk_first[s] + k of d_chunks, which is
    chunk_status' index (chunk_slots gives every slot's file position, scatter_chunks writes the verified ones out).  Statuses,
    outboards and bitmap as ingest_set_slices; d_outboards=None: decode.  At most three launches.  When not to (MI355X, DESIGN.md §8g,
    against the commit before's arena receivers over the same slices of a 1 GiB file): a file that IS resident.  The packed receivers
    are level with their twins or just below - that shape 3.34 ms against 3.41, 65 536 single chunks 1.24 against 1.26 as set slices
    and 1.46 against 1.52 as one-chunk slices, 4 096 runs of 16 as range slices 0.395 against 0.400, 64 runs of 1 024 0.2120 against
    0.2113 (the one shape behind, by 0.3 %) - so what they save is the memory, not time.  Returns ingest_set_slices' dict plus chunks
    and slot_first (= set_chunk_first)."""
    L = lib()
    ln, fi, fc, nc = _packed_args("ingest_set_slices_packed", lens, files, first_chunks, n_chunks, group_log)
    lay = set_slice_layout(ln, fi, fc, nc)
    n_sets, total = lay["set_file"].size, int(lay["set_chunk_first"][-1]) if fc.size else 0
    d_chunks, p_chunks = _receive_args("ingest_set_slices_packed", ln, d_outboards, d_roots, fi, d_slices, int(lay["slice_first"][-1]) if fc.size else 0,
                                       group_log, d_have, d_chunks, total)
    dev = d_slices.device
    st = torch.full((n_sets,), -1, dtype=torch.int32, device=dev)
    fb = torch.full((n_sets,), -2, dtype=torch.int64, device=dev)
    cs = torch.full((total,), -1, dtype=torch.int32, device=dev)
    need = L.b3w_bao_set_slice_ingest_scratch_bytes(ln.ctypes.data, ln.size, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fc.size)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _chk(ctx, L.b3w_bao_set_slice_ingest_packed_device(ctx.handle, p_chunks, d_chunks.numel(), ln.ctypes.data, ln.size, group_log,
                                                       d_outboards.data_ptr() if d_outboards is not None else None, d_roots.data_ptr(), fi.ctypes.data,
                                                       fc.ctypes.data, nc.ctypes.data, fc.size, d_slices.data_ptr(), st.data_ptr(), fb.data_ptr(),
                                                       cs.data_ptr() if cs.numel() else None, d_have.data_ptr() if d_have is not None else None,
                                                       scratch.data_ptr(), scratch.numel(), _stream(stream)), "b3w_bao_set_slice_ingest_packed_device")
    return dict(set_status=st, set_first_bad=fb, chunk_status=cs, chunks=d_chunks, slot_first=lay["set_chunk_first"], **lay)


# ---- resident files after appends and truncations ---------------------------------------------------------------------------
def resize_kept_tiles(old_len, new_len):
    """floor(min(old_len, new_len) / 1 MiB): the tiles of 1 024 chunks whose nodes a resize moves and does not recompute"""
    if old_len < 0 or new_len < 0:
        raise B3WError(100, "resize_kept_tiles: a negative length")
    return lib().b3w_bao_resize_kept_tiles(old_len, new_len)


def outboard_resize_batch(ctx, d_arena, offsets, old_lens, new_lens, d_old_outboards, old_ob_first, d_new_outboards, new_ob_first, d_roots, files,
                          group_log=0, stream=0):
    """After appends to and truncations of resident files: file f is now bytes [offsets[f], + new_lens[f]) of d_arena, its first
    min(old, new) bytes what they were, and d_old_outboards[old_ob_first[f]:] holds its outboard (group_log 0) or group outboard as
    outboard_batch / outboard_groups_batch made it for old_lens[f].  For every file in `files` (each at most once; an equal length is
    allowed) d_new_outboards[new_ob_first[f]:] and d_roots[f] are afterwards byte for byte what those calls give for the arena as it is
    now with new_lens.  With T = resize_kept_tiles(old, new) the blocks of the first T tiles of 1 024 chunks are moved from the old
    outboard and their CVs taken from their first nodes, the tiles from T on are hashed, the storeys above run again: at most five
    launches.  No arena byte of a listed file below T MiB is read; d_old_outboards is never written; of d_new_outboards only the listed
    files' group_outboard_size(new_len) bytes and of d_roots only their rows are written; nothing of an unlisted file is touched.  The
    ob_first arrays are taken as they are and read at listed files only: any 8-byte-aligned places (need not be batch_layout's), but
    a file's old and new extent must not overlap.  The scratch (32 bytes a tile of the listed files of more than one tile) is made
    here.  When to call outboard_batch instead (MI355X): only kept tiles are a gain.  4 KiB appended to or cut from
    1 GiB takes 0.17 ms against 0.42 (as do 1 MiB and 64 MiB appended: a call that hashes a tile costs one workgroup's latency),
    512 MiB -> 1 GiB 0.27, 1 GiB -> 512 MiB 0.05 against 0.25; files below 1 MiB at either length keep no tile and take 1.14 times
    the batch call's time (16 384 files of 64 -> 68 KiB), so they belong to outboard_batch."""
    L = lib()
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    off, lo, ln = _u64(offsets), _u64(old_lens), _u64(new_lens)
    of, nf = _u64(old_ob_first), _u64(new_ob_first)
    fi = np.ascontiguousarray(np.atleast_1d(files), dtype=np.uint32)
    if not (off.size == lo.size == ln.size):
        raise B3WError(100, f"outboard_resize_batch: {off.size} offsets, {lo.size} old and {ln.size} new lengths")
    if of.size < ln.size or nf.size < ln.size:
        raise B3WError(100, f"outboard_resize_batch: {of.size} old and {nf.size} new outboard places for {ln.size} files")
    if fi.size == 0:
        return
    if int(fi.max()) >= ln.size:
        raise B3WError(100, f"outboard_resize_batch: file index {int(fi.max())} is not below the file count {ln.size}")
    if np.unique(fi).size != fi.size:
        raise B3WError(100, "outboard_resize_batch: a file is listed twice")
    assert d_arena.is_cuda and d_arena.dtype == torch.uint8 and d_arena.is_contiguous()
    assert d_old_outboards.is_cuda and d_old_outboards.dtype == torch.uint8 and d_old_outboards.is_contiguous()
    assert d_new_outboards.is_cuda and d_new_outboards.dtype == torch.uint8 and d_new_outboards.is_contiguous()
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.element_size() == 4 and d_roots.numel() >= ln.size * 8
    for f in fi.tolist():
        if int(of[f]) + group_outboard_size(int(lo[f]), group_log) > d_old_outboards.numel():
            raise B3WError(100, f"outboard_resize_batch: file {f}'s old outboard reaches past d_old_outboards")
        if int(nf[f]) + group_outboard_size(int(ln[f]), group_log) > d_new_outboards.numel():
            raise B3WError(100, f"outboard_resize_batch: file {f}'s new outboard reaches past d_new_outboards")
    need = L.b3w_bao_resize_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fi.size)
    scratch = torch.empty(need, dtype=torch.uint8, device=d_arena.device) if need else None
    _chk(ctx, L.b3w_bao_outboard_resize_batch_device(ctx.handle, d_arena.data_ptr() if d_arena.numel() else None, d_arena.numel(), off.ctypes.data,
                                                     lo.ctypes.data, ln.ctypes.data, ln.size, group_log, of.ctypes.data, d_old_outboards.data_ptr(),
                                                     nf.ctypes.data, d_new_outboards.data_ptr(), d_roots.data_ptr(), fi.ctypes.data, fi.size,
                                                     scratch.data_ptr() if need else None, need, _stream(stream)), "b3w_bao_outboard_resize_batch_device")


def resize_host(data, old_outboard, old_len, group_log=0):
    """outboard_resize_batch for one file on the host (no GPU) -> (outboard bytes, root as uint32 numpy [8]): the outboard (full, or the
    group outboard of group_log) and root of `data` (the file at its new length) from its outboard at old_len; the first
    min(old_len, len(data)) bytes of data are what they were.  The blocks of the resize_kept_tiles(old_len, len(data)) kept tiles are
    copied, and no byte of data below that many MiB is read."""
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    if old_len < 0:
        raise B3WError(100, "resize_host: a negative old length")
    data = bytes(data)
    ob = old_outboard.cpu().numpy().tobytes() if isinstance(old_outboard, torch.Tensor) else bytes(old_outboard)
    if len(ob) != group_outboard_size(old_len, group_log):
        raise B3WError(100, "resize_host: the old outboard's size is not that of a file of old_len bytes")
    out = bytearray(group_outboard_size(len(data), group_log))
    rw = np.zeros(8, dtype=np.uint32)
    buf = (ctypes.c_uint8 * len(out)).from_buffer(out)
    _chk(None, lib().b3w_bao_outboard_resize(data, len(data), ob, old_len, group_log, ctypes.addressof(buf), rw.ctypes.data), "b3w_bao_outboard_resize")
    del buf
    return bytes(out), rw


# ---- files streamed in windows ---------------------------------------------------------------------------------------------
TILE_BYTES = 1 << 20                                   # a window is whole tiles of 1 024 chunks, except where it ends the file
STREAM_OUTBOARD, STREAM_VERIFY = 0, 1
DEFAULT_WINDOW_BYTES = 64 << 20                        # the fastest of 4, 16 and 64 MiB from host memory (a push's fixed 0.11 ms is 10 % of its copy)


def stream_scratch_bytes(length, kind):
    return lib().b3w_bao_stream_scratch_bytes(length, kind)


def windows(length, window_bytes):
    """-> [(offset, bytes)]: the windows outboard_stream / verify_stream push, in order: whole windows of window_bytes (a positive
    multiple of 1 MiB), then what is left; they cover [0, length) exactly once.  An empty file has none."""
    if window_bytes <= 0 or window_bytes % TILE_BYTES:
        raise B3WError(100, f"window_bytes {window_bytes} is not a positive multiple of 1 MiB")
    return [(off, min(window_bytes, length - off)) for off in range(0, length, window_bytes)]


class _Stream:
    """the session's handle and the calls both kinds share"""

    def __init__(self, ctx, length, group_log):
        self._h = ctypes.c_void_p()
        if not 0 <= group_log <= MAX_GROUP_LOG:
            raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
        self.ctx, self.length, self.group_log = ctx, int(length), group_log

    def push(self, offset, d_window, stream=0):
        """the file's bytes [offset, offset + d_window.numel()) lie in d_window (a uint8 CUDA tensor, any alignment): one launch on
        `stream`.  offset: a multiple of 1 MiB; the size: a multiple of 1 MiB unless the window ends the file.  Any order, any stream."""
        assert d_window.is_cuda and d_window.dtype == torch.uint8 and d_window.is_contiguous()
        _chk(self.ctx, lib().b3w_bao_stream_push(self._h, offset, d_window.data_ptr(), d_window.numel(), _stream(stream)), "b3w_bao_stream_push")
        self._pushed(d_window.numel())

    def _finish(self, stream):
        _chk(self.ctx, lib().b3w_bao_stream_finish(self._h, _stream(stream)), "b3w_bao_stream_finish")

    def _pushed(self, nbytes):
        """(a push of nbytes went through: only an open session keeps count)"""

    def close(self):
        if self._h:
            lib().b3w_bao_stream_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        self.close()


class StreamOutboard(_Stream):
    """The outboard (group_log = 0: full; 1 .. 6: over chunk groups) and root of ONE file of `length` bytes pushed window by window:
    push(offset, d_window, stream) per window, then finish(stream), which the caller orders behind every push.  The session makes the
    outboard, the root and the scratch on the device and nothing that grows with the file's bytes."""

    def __init__(self, ctx, length, group_log=0, device="cuda"):
        super().__init__(ctx, length, group_log)
        self.ob_first = group_batch_layout([self.length], group_log)
        self.outboards = torch.empty(int(self.ob_first[-1]), dtype=torch.uint8, device=device)
        self.roots = torch.empty((1, 8), dtype=torch.int32, device=device)
        need = stream_scratch_bytes(self.length, STREAM_OUTBOARD)
        self.scratch = torch.empty(need, dtype=torch.uint8, device=device)
        _chk(ctx, lib().b3w_bao_stream_outboard_begin(ctx.handle, self.length, group_log, self.outboards.data_ptr(), self.roots.data_ptr(),
                                                      self.scratch.data_ptr() if need else None, need, ctypes.byref(self._h)), "b3w_bao_stream_outboard_begin")

    def finish(self, stream=0):
        """-> the dict outboard_batch / outboard_groups_batch return for this file as a batch of one"""
        self._finish(stream)
        return dict(outboards=self.outboards, ob_first=self.ob_first, roots=self.roots)


class StreamVerify(_Stream):
    """verify_batch for ONE file pushed window by window against its resident outboard and root.  The statuses of a window's units
    (self.unit_status) are final once that push's work on its stream is done: a bad window shows before the next one arrives."""

    def __init__(self, ctx, length, d_outboard, d_root, group_log=0, stream=0):
        super().__init__(ctx, length, group_log)
        dev = d_outboard.device
        self.unit_first = verify_layout([self.length], group_log)
        assert d_outboard.is_cuda and d_outboard.dtype == torch.uint8 and d_outboard.is_contiguous()
        assert d_outboard.numel() >= group_outboard_size(self.length, group_log)
        assert d_root.is_cuda and d_root.is_contiguous() and d_root.element_size() == 4 and d_root.numel() >= 8
        self.d_outboard, self.d_root = d_outboard, d_root
        self.unit_status = torch.empty(int(self.unit_first[-1]), dtype=torch.uint8, device=dev)
        self.file_status = torch.empty(1, dtype=torch.int32, device=dev)
        self.first_bad = torch.empty(1, dtype=torch.int64, device=dev)
        need = stream_scratch_bytes(self.length, STREAM_VERIFY)
        self.scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        _chk(ctx, lib().b3w_bao_stream_verify_begin(ctx.handle, self.length, group_log, d_outboard.data_ptr(), d_root.data_ptr(),
                                                    self.unit_status.data_ptr(), self.file_status.data_ptr(), self.first_bad.data_ptr(),
                                                    self.scratch.data_ptr() if need else None, need, _stream(stream), ctypes.byref(self._h)),
             "b3w_bao_stream_verify_begin")

    def finish(self, stream=0):
        """-> the dict verify_batch returns for this file as a batch of one"""
        self._finish(stream)
        return dict(unit_status=self.unit_status, unit_first=self.unit_first, file_status=self.file_status, first_bad=self.first_bad)


def _reader(source, length):
    """-> fill(dst, offset): dst (a writable numpy uint8 view) takes the source's bytes from `offset` on"""
    if hasattr(source, "readinto"):
        def fill(dst, offset):                          # (read in order: the offset is where the reader stands)
            view, got = memoryview(dst), 0
            while got < len(view):
                k = source.readinto(view[got:])
                if not k:
                    raise B3WError(100, f"the source ended at byte {offset + got}, before the length given ({length})")
                got += k
        return fill
    data = np.frombuffer(source, dtype=np.uint8) if not isinstance(source, np.ndarray) else source.reshape(-1).view(np.uint8)
    if data.size < length:
        raise B3WError(100, f"the source holds {data.size} bytes, fewer than the length given ({length})")

    def fill(dst, offset):
        dst[:] = data[offset:offset + dst.size]
    return fill


def _pump(session, source, length, window_bytes, ring):
    """the windows of `source` through `ring` pinned host buffers and `ring` device windows, each on a stream of its own: window i's
    copy, push and buffer-reuse event stay on stream i mod ring; the current stream ends up behind all of them"""
    if ring < 1:
        raise B3WError(100, "ring must be at least 1")
    wins = windows(length, window_bytes)
    size = max((b for _, b in wins), default=0)
    cur = torch.cuda.current_stream()
    # a pinned uint8 tensor is copied from where it lies: no host buffers, the device windows alone
    direct = source.reshape(-1) if isinstance(source, torch.Tensor) and source.dtype == torch.uint8 and source.is_pinned() else None
    if direct is not None and direct.numel() < length:
        raise B3WError(100, f"the source holds {direct.numel()} bytes, fewer than the length given ({length})")
    fill = _reader(source.numpy() if isinstance(source, torch.Tensor) else source, length) if wins and direct is None else None
    slots = [(torch.empty(size if direct is None else 0, dtype=torch.uint8, pin_memory=True), torch.empty(size, dtype=torch.uint8, device="cuda"),
              torch.cuda.Stream(), torch.cuda.Event()) for _ in range(min(ring, len(wins)))]
    for _, _, s, _ in slots:
        s.wait_stream(cur)                              # (what the caller enqueued before, e.g. the outboard's arrival, comes first)
    for i, (off, nb) in enumerate(wins):
        h, d, s, ev = slots[i % len(slots)]
        if direct is None:
            if i >= len(slots):
                ev.synchronize()                        # the slot's last copy and push are through with both buffers
            fill(h.numpy()[:nb], off)
        with torch.cuda.stream(s):                      # (the device window's reuse is ordered by its stream)
            d[:nb].copy_(h[:nb] if direct is None else direct[off:off + nb], non_blocking=True)
            session.push(off, d[:nb], stream=s.cuda_stream)
            ev.record(s)
    for _, _, s, _ in slots:
        cur.wait_stream(s)


def outboard_stream(ctx, source, length, window_bytes=DEFAULT_WINDOW_BYTES, group_log=0, ring=2):
    """The outboard and root of a file that is NOT resident on the device: `source` (bytes-like, a numpy buffer, or an object with
    readinto, read in order) goes through `ring` pinned host buffers and `ring` device windows of window_bytes (a multiple of 1 MiB),
    each on a stream of its own, so window i + 1 is copied while window i is hashed.  A source that is a pinned uint8 torch tensor is
    copied from where it lies, without the host buffers (filling them is the slow part: one host thread's memcpy).  Device memory made here is ring x window_bytes +
    the outboard + the scratch (32 bytes per MiB of file), WHATEVER THE FILE'S LENGTH — outboard_batch needs the whole file resident.
    Returns the dict outboard_batch / outboard_groups_batch return for this file as a batch of one; the work is enqueued, the
    current stream ordered behind it."""
    session = StreamOutboard(ctx, length, group_log)
    try:
        _pump(session, source, length, window_bytes, ring)
        return session.finish()
    finally:
        session.close()


def verify_stream(ctx, source, length, d_outboard, d_root, window_bytes=DEFAULT_WINDOW_BYTES, group_log=0, ring=2):
    """verify_batch for a file that is not resident on the device, against its resident outboard (d_outboard, full or over groups of
    2^group_log chunks) and root (d_root): the windows go as in outboard_stream.  Device memory made here is ring x window_bytes + the
    statuses (a byte a unit) + the scratch (36 bytes per MiB of file), whatever the file's length.  Returns the dict verify_batch
    returns for this file as a batch of one."""
    session = StreamVerify(ctx, length, d_outboard, d_root, group_log)
    try:
        _pump(session, source, length, window_bytes, ring)
        return session.finish()
    finally:
        session.close()


# ---- set slices taken in window by window as they arrive -------------------------------------------------------------------------------
SET_SLICE_STREAM_MIN_WINDOW = 8 + 64 * (24 + 1023) + (1 << 20)   # B3W_BAO_SET_SLICE_STREAM_MIN_WINDOW: no row's segment is longer
SET_SLICE_STREAM_CARRY_BYTES = 1552                    # B3W_BAO_SET_SLICE_STREAM_CARRY_BYTES
SET_STREAM_ARENA, SET_STREAM_PACKED = 0, 1
DEFAULT_SET_SLICE_WINDOW_BYTES = 64 << 20              # the fastest of 1.1, 8 and 64 MiB (a push costs about 0.17 ms whatever it holds)


def set_slice_cuts(length, first_chunks, n_chunks, window_bytes):
    """-> numpy uint64 [windows + 1]: the ascending offsets at which the set slice of these runs (ascending, disjoint) of a file of
    `length` bytes is cut into windows of at most window_bytes (>= SET_SLICE_STREAM_MIN_WINDOW), each filled greedily with as many
    whole rows as fit; from 0 to set_slice_size.  Host only; no step a chunk."""
    fc, nc = _ranges(first_chunks, n_chunks)
    L = lib()
    k = L.b3w_bao_set_slice_stream_cuts(length, fc.ctypes.data, nc.ctypes.data, fc.size, window_bytes, None, 0)
    if k < 0:
        raise B3WError(-k, "b3w_bao_set_slice_stream_cuts: no run, a run that is empty or reaches past the file's chunk count, a list that is not "
                           f"ascending and disjoint, a file of more than 2^30 chunks, or window_bytes below {SET_SLICE_STREAM_MIN_WINDOW}")
    out = np.zeros(k + 1, dtype=np.uint64)
    assert L.b3w_bao_set_slice_stream_cuts(length, fc.ctypes.data, nc.ctypes.data, fc.size, window_bytes, out.ctypes.data, out.size) == k
    return out


class SetSliceStream:
    """ingest_set_slices / ingest_set_slices_packed for ONE set (one file) whose slice arrives in windows cut at row boundaries
    (set_slice_cuts, or any cuts of the rows), pushed in slice order; the outputs are byte for byte the one-shot call's.  packed=False:
    d_dest is the file's place in an arena (a uint8 CUDA view of at least `length` bytes, any alignment) and d_outboard its outboard;
    packed=True: d_dest is the slot buffer (made here when None) and d_outboard may be None (decode).  The session makes its own
    statuses and scratch; window_bytes sizes the scratch: no pushed window may hold more rows than a window of that many bytes can.
    set_status is final for a window once its push is done on its stream: a bad window shows before the next one arrives.  Each push
    must be ordered behind the one before (the same stream, or events): the carried nodes are a serial dependency."""

    def __init__(self, ctx, length, first_chunks, n_chunks, d_root, d_dest=None, d_outboard=None, group_log=0, window_bytes=DEFAULT_SET_SLICE_WINDOW_BYTES,
                 packed=False, d_have=None, stream=0):
        self._h = ctypes.c_void_p()
        if not 0 <= group_log <= MAX_GROUP_LOG:
            raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
        L = lib()
        self.ctx, self.length, self.group_log, self.packed = ctx, int(length), group_log, bool(packed)
        fc, nc = _ranges(first_chunks, n_chunks)
        self.layout = set_slice_layout([self.length], np.zeros(fc.size, dtype=np.uint32), fc, nc)
        total = int(self.layout["set_chunk_first"][-1])
        need = L.b3w_bao_set_slice_stream_scratch_bytes(self.length, fc.ctypes.data, nc.ctypes.data, fc.size, window_bytes)
        if not need:
            raise B3WError(100, f"SetSliceStream: no run, or window_bytes {window_bytes} is below {SET_SLICE_STREAM_MIN_WINDOW}")
        assert d_root.is_cuda and d_root.is_contiguous() and d_root.element_size() == 4 and d_root.numel() >= 8
        dev = d_root.device
        if self.packed and d_dest is None:
            d_dest = torch.zeros(total * 1024, dtype=torch.uint8, device=dev)
        if d_dest is None or (not self.packed and d_outboard is None):
            raise B3WError(100, "SetSliceStream: an arena destination needs d_dest and d_outboard")
        assert d_dest.is_cuda and d_dest.dtype == torch.uint8 and d_dest.is_contiguous()
        if d_outboard is not None:
            assert d_outboard.is_cuda and d_outboard.dtype == torch.uint8 and d_outboard.is_contiguous()
            assert d_outboard.numel() >= group_outboard_size(self.length, group_log)
        if d_have is not None:
            _have_tensor("SetSliceStream", d_have, _u64([self.length]))
        self.d_dest, self.d_outboard, self.d_root, self.d_have = d_dest, d_outboard, d_root, d_have
        self.set_status = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self.set_first_bad = torch.full((1,), -2, dtype=torch.int64, device=dev)
        self.chunk_status = torch.full((total,), -1, dtype=torch.int32, device=dev)
        self.scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        _chk(ctx, L.b3w_bao_set_slice_stream_begin(ctx.handle, self.length, group_log, fc.ctypes.data, nc.ctypes.data, fc.size, d_root.data_ptr(),
                                                   SET_STREAM_PACKED if self.packed else SET_STREAM_ARENA, d_dest.data_ptr() if d_dest.numel() else None,
                                                   d_dest.numel(), d_outboard.data_ptr() if d_outboard is not None else None,
                                                   d_have.data_ptr() if d_have is not None else None, self.chunk_status.data_ptr(),
                                                   self.set_status.data_ptr(), self.set_first_bad.data_ptr(), self.scratch.data_ptr(), need,
                                                   _stream(stream), ctypes.byref(self._h)), "b3w_bao_set_slice_stream_begin")

    def push(self, offset, d_window, stream=0):
        """slice bytes [offset, offset + d_window.numel()) lie in d_window (a uint8 CUDA view whose first byte is at 8 modulo 16 for
        offset 0 and 16-byte aligned otherwise): from a cut to a cut, starting where the last window ended.  At most three launches."""
        assert d_window.is_cuda and d_window.dtype == torch.uint8 and d_window.is_contiguous()
        _chk(self.ctx, lib().b3w_bao_set_slice_stream_push(self._h, offset, d_window.data_ptr(), d_window.numel(), _stream(stream)),
             "b3w_bao_set_slice_stream_push")

    def finish(self):
        """-> the dict ingest_set_slices (packed: ingest_set_slices_packed) returns for this set as a call of one; no launch"""
        _chk(self.ctx, lib().b3w_bao_set_slice_stream_finish(self._h), "b3w_bao_set_slice_stream_finish")
        out = dict(set_status=self.set_status, set_first_bad=self.set_first_bad, chunk_status=self.chunk_status, **self.layout)
        if self.packed:
            out.update(chunks=self.d_dest, slot_first=self.layout["set_chunk_first"])
        return out

    def close(self):
        if self._h:
            lib().b3w_bao_set_slice_stream_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        self.close()


def ingest_set_slice_stream(ctx, source, length, first_chunks, n_chunks, d_root, d_dest=None, d_outboard=None, group_log=0,
                            window_bytes=DEFAULT_SET_SLICE_WINDOW_BYTES, packed=False, d_have=None):
    """ingest_set_slices for one set whose slice is NOT on the device: `source` (bytes-like, a numpy buffer, or an object with readinto,
    read in order) holds the set slice and goes through a ring of two pinned host buffers and two device windows cut by
    set_slice_cuts(window_bytes); the copies run on a side stream and are chained to the pushes (on the current stream) with events, so
    window i + 1 is copied while window i is verified.  Device memory made here is 2 x window_bytes + the statuses + the scratch,
    whatever the slice's size, where ingest_set_slices needs the whole slice resident.  When not to (MI355X, DESIGN.md §8g, the 593 MB
    slice of a half-missing 1 GiB file, against a build of the commit before's one-shot receiver over the resident slice): a slice that
    IS resident - a session of 9 windows of 64 MiB takes 4.66 ms against 3.39, 74 of 8 MiB 15.8, 986 of the least window 171.6 (50
    times): a push costs about 0.17 ms whatever it holds, so window_bytes defaults to the largest measured.  Returns the dict ingest_set_slices returns for
    this set as a call of one (packed=True: ingest_set_slices_packed's); the work is enqueued on the current stream."""
    cuts = [int(x) for x in set_slice_cuts(length, first_chunks, n_chunks, window_bytes)]
    session = SetSliceStream(ctx, length, first_chunks, n_chunks, d_root, d_dest, d_outboard, group_log, window_bytes, packed, d_have,
                             stream=torch.cuda.current_stream().cuda_stream)
    try:
        size = max(b - a for a, b in zip(cuts, cuts[1:]))
        fill = _reader(source, cuts[-1])
        cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
        ring = min(2, len(cuts) - 1)
        host = [torch.empty(size + 16, dtype=torch.uint8, pin_memory=True) for _ in range(ring)]
        dev = [torch.empty(size + 16, dtype=torch.uint8, device=d_root.device) for _ in range(ring)]
        copied, pushed = [torch.cuda.Event() for _ in range(ring)], [torch.cuda.Event() for _ in range(ring)]
        side.wait_stream(cur)                                 # (the windows are the current stream's memory: what the caller enqueued before may still read a block they reuse)
        for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
            k, lead = i % ring, 0 if a else 8                 # (the header's window starts at 8 modulo 16, as a packed slice does)
            if i >= ring:
                copied[k].synchronize()                       # the pinned buffer's last copy is through
            fill(host[k].numpy()[lead:lead + b - a], a)
            with torch.cuda.stream(side):
                if i >= ring:
                    side.wait_event(pushed[k])                # the device window's last push is through
                dev[k][lead:lead + b - a].copy_(host[k][lead:lead + b - a], non_blocking=True)
                copied[k].record(side)
            cur.wait_event(copied[k])
            session.push(a, dev[k][lead:lead + b - a], stream=cur.cuda_stream)
            pushed[k].record(cur)
        return session.finish()
    finally:
        session.close()


# ---- files whose length is not known up front -----------------------------------------------------------------------------------------
STREAM_OPEN = 2
OPEN_STAGING_PAD = 16                                  # B3W_BAO_STREAM_OPEN_STAGING_PAD


def _open_args(capacity, window_bytes, group_log, ring):
    """what StreamOutboardOpen / outboard_stream_open refuse before they make anything"""
    if ring < 1:
        raise B3WError(100, "ring must be at least 1")
    if window_bytes <= 0 or window_bytes % TILE_BYTES:
        raise B3WError(100, f"window_bytes {window_bytes} is not a positive multiple of 1 MiB")
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")
    if capacity < 0:
        raise B3WError(100, f"capacity {capacity} is negative")


class StreamOutboardOpen(_Stream):
    """StreamOutboard for a file of at most `capacity` bytes whose length is known only at the end: push(offset, d_window, stream) takes
    whole MiB (any order, any stream, each once), finish(d_tail, stream) the last bytes that fill no MiB, and with them the length.
    The session makes a staging area (the outboard's size for `capacity`) and a scratch at once, the outboard and root in finish()."""

    def __init__(self, ctx, capacity, group_log=0, device="cuda"):
        super().__init__(ctx, 0, group_log)
        _open_args(capacity, TILE_BYTES, group_log, 1)
        self.capacity, self.length, self._bytes, self.device = int(capacity), None, 0, device
        L = lib()
        n_stage, n_scr = L.b3w_bao_stream_open_staging_bytes(self.capacity, group_log), L.b3w_bao_stream_open_scratch_bytes(self.capacity)
        self.staging = torch.empty(n_stage, dtype=torch.uint8, device=device)
        self.scratch = torch.empty(n_scr, dtype=torch.uint8, device=device)
        _chk(ctx, L.b3w_bao_stream_open_begin(ctx.handle, self.capacity, group_log, self.staging.data_ptr(), n_stage, self.scratch.data_ptr(), n_scr,
                                              ctypes.byref(self._h)), "b3w_bao_stream_open_begin")

    def _pushed(self, nbytes):
        self._bytes += nbytes

    def finish(self, d_tail=None, stream=0):
        """d_tail: the file's last bytes, fewer than 1 MiB (a uint8 CUDA tensor, any alignment; None or empty: the file ends with its
        last MiB pushed).  The caller orders `stream` behind every push.  -> the dict outboard_batch / outboard_groups_batch return
        for this file as a batch of one, and `length`."""
        tail = 0 if d_tail is None else d_tail.numel()
        if tail:
            assert d_tail.is_cuda and d_tail.dtype == torch.uint8 and d_tail.is_contiguous()
        ob_first = group_batch_layout([self._bytes + tail], self.group_log)
        outboards = torch.empty(int(ob_first[-1]), dtype=torch.uint8, device=self.device)
        roots = torch.empty((1, 8), dtype=torch.int32, device=self.device)
        n = ctypes.c_uint64()
        _chk(self.ctx, lib().b3w_bao_stream_open_finish(self._h, d_tail.data_ptr() if tail else None, tail, outboards.data_ptr(), outboards.numel(),
                                                        roots.data_ptr(), _stream(stream), ctypes.byref(n)), "b3w_bao_stream_open_finish")
        self.length, self.outboards, self.ob_first, self.roots = n.value, outboards, ob_first, roots
        return dict(outboards=outboards, ob_first=ob_first, roots=roots, length=self.length)


def outboard_stream_open(ctx, source, capacity, window_bytes=DEFAULT_WINDOW_BYTES, group_log=0, ring=2):
    """outboard_stream for a source whose length is not known: `source` is an object with readinto, read until it returns 0 (a short
    read is not the end), or a bytes-like / numpy buffer, taken whole; `capacity` bounds its length, and a source that yields more
    raises B3WError.  The same ring of pinned host buffers and device windows, each on a stream of its own.  Of every window the whole
    MiB are pushed; what the last read leaves below a MiB is the tail and stays in its device window until finish has read it.  Device
    memory made here is ring x window_bytes + the staging (the outboard's size for `capacity`) + the scratch + the outboard.
    Returns StreamOutboardOpen.finish()'s dict; the work is enqueued, the current stream ordered behind it."""
    _open_args(capacity, window_bytes, group_log, ring)
    if hasattr(source, "readinto"):
        def fill(dst):
            view, got = memoryview(dst), 0
            while got < len(view):
                k = source.readinto(view[got:])
                if not k:
                    break
                got += k
            return got
    else:
        data = np.frombuffer(source, dtype=np.uint8) if not isinstance(source, np.ndarray) else source.reshape(-1).view(np.uint8)
        if data.size > capacity:
            raise B3WError(100, f"the source holds {data.size} bytes, more than the capacity ({capacity})")
        at = [0]

        def fill(dst):
            got = min(dst.size, data.size - at[0])
            dst[:got] = data[at[0]:at[0] + got]
            at[0] += got
            return got
    session = StreamOutboardOpen(ctx, capacity, group_log)
    try:
        size = min(window_bytes, max(TILE_BYTES, -(-int(capacity) // TILE_BYTES) * TILE_BYTES))
        cur = torch.cuda.current_stream()
        slots, total, tail, i = [], 0, None, 0
        try:
            while True:
                if i < ring:                            # (a slot is made when its turn first comes and the source still has bytes)
                    h = torch.empty(size, dtype=torch.uint8, pin_memory=True)
                else:
                    h, d, s, ev = slots[i % ring]
                    ev.synchronize()                    # the slot's last copy and push are through with both buffers
                got = fill(h.numpy())
                if total + got > capacity:
                    raise B3WError(100, f"the source yields more than the capacity ({capacity} bytes)")
                if not got:                             # the source ended on a window's last byte: no tail, and no slot for nothing
                    break
                if i < ring:
                    d, s, ev = torch.empty(size, dtype=torch.uint8, device="cuda"), torch.cuda.Stream(), torch.cuda.Event()
                    slots.append((h, d, s, ev))
                    s.wait_stream(cur)
                whole = got // TILE_BYTES * TILE_BYTES
                with torch.cuda.stream(s):
                    d[:got].copy_(h[:got], non_blocking=True)
                    if whole:
                        session.push(total, d[:whole], stream=s.cuda_stream)
                    ev.record(s)
                total += got
                i += 1
                if got < size:                          # the source has ended
                    tail = d[whole:got] if got > whole else None
                    break
        finally:                                        # (also on a raise: the staging and the windows are not freed under a push in flight)
            for _, _, s, _ in slots:
                cur.wait_stream(s)
        return session.finish(tail)
    finally:
        session.close()


# ---- many stream sessions in one launch --------------------------------------------------------------------------------------------
# Not measured yet ("many stream sessions in one launch"): 16 lanes of 4 MiB are 64 MiB a round, the bytes of one push
# at DEFAULT_WINDOW_BYTES.  The host-source pass that is to replace them is listed there as outstanding.
DEFAULT_MANY_WINDOW_BYTES = 4 << 20
DEFAULT_MANY_LANES = 16


def _handles(sessions):
    hs = np.array([s._h.value or 0 for s in sessions], dtype=np.uint64)
    if len(sessions) and not hs.all():
        raise B3WError(100, "a closed session")
    return hs


def push_many(sessions, offsets, d_windows, stream=0):
    """session.push(offsets[i], d_windows[i]) for every i, as ONE launch on `stream`: sessions are StreamOutboard / StreamVerify /
    StreamOutboardOpen objects of one context and one kind (their group_log may differ), d_windows uint8 CUDA tensors.  A session may appear more than once
    with disjoint windows.  If any entry would be refused nothing is launched and no session changes (B3WError names the entry)."""
    if not (len(sessions) == len(offsets) == len(d_windows)):
        raise B3WError(100, "push_many: sessions, offsets and d_windows differ in length")
    if not len(sessions):
        return
    for w in d_windows:
        assert w.is_cuda and w.dtype == torch.uint8 and w.is_contiguous()
    hs, off = _handles(sessions), _u64(offsets)
    ptr = np.array([w.data_ptr() for w in d_windows], dtype=np.uint64)
    nb = np.array([w.numel() for w in d_windows], dtype=np.uint64)
    ctx = sessions[0].ctx
    _chk(ctx, lib().b3w_bao_stream_push_many(ctx.handle, hs.ctypes.data, off.ctypes.data, ptr.ctypes.data, nb.ctypes.data, hs.size, _stream(stream)),
         "b3w_bao_stream_push_many")
    for s, w in zip(sessions, d_windows):
        s._pushed(w.numel())


def finish_many(sessions, stream=0):
    """session.finish() for every session in at most three launches on `stream`, which the caller orders behind every push
    -> the list of the dicts finish() returns"""
    if not len(sessions):
        return []
    _finish_many(sessions, stream)
    return [dict(outboards=s.outboards, ob_first=s.ob_first, roots=s.roots) if isinstance(s, StreamOutboard) else
            dict(unit_status=s.unit_status, unit_first=s.unit_first, file_status=s.file_status, first_bad=s.first_bad) for s in sessions]


def _finish_many(sessions, stream):
    hs = _handles(sessions)
    ctx = sessions[0].ctx
    _chk(ctx, lib().b3w_bao_stream_finish_many(ctx.handle, hs.ctypes.data, hs.size, _stream(stream)), "b3w_bao_stream_finish_many")


class _Lane(_Stream):
    """a session of the *_stream_many helpers: its outputs are the file's places in the packed results of the whole batch"""

    def __init__(self, ctx, kind, length, group_log, out, f):
        super().__init__(ctx, length, group_log)
        need = stream_scratch_bytes(self.length, kind)
        self.scratch = torch.empty(need, dtype=torch.uint8, device=out["device"])
        scr = self.scratch.data_ptr() if need else None
        ob = out["outboards"][int(out["ob_first"][f]):int(out["ob_first"][f + 1])]
        if kind == STREAM_OUTBOARD:
            _chk(ctx, lib().b3w_bao_stream_outboard_begin(ctx.handle, self.length, group_log, ob.data_ptr(), out["roots"][f].data_ptr(), scr, need,
                                                          ctypes.byref(self._h)), "b3w_bao_stream_outboard_begin")
        else:
            _chk(ctx, lib().b3w_bao_stream_verify_begin(ctx.handle, self.length, group_log, ob.data_ptr(), out["roots"].reshape(-1, 8)[f].data_ptr(),
                                                        out["unit_status"][int(out["unit_first"][f]):].data_ptr(), out["file_status"][f:].data_ptr(),
                                                        out["first_bad"][f:].data_ptr(), scr, need, _stream(0), ctypes.byref(self._h)),
                 "b3w_bao_stream_verify_begin")


def _many_args(sources, lengths, window_bytes, group_log, lanes, ring):
    """what the *_stream_many helpers refuse before they make anything"""
    if lanes < 1:
        raise B3WError(100, "lanes must be at least 1")
    if ring < 1:
        raise B3WError(100, "ring must be at least 1")
    if window_bytes <= 0 or window_bytes % TILE_BYTES:
        raise B3WError(100, f"window_bytes {window_bytes} is not a positive multiple of 1 MiB")
    if len(sources) != len(lengths):
        raise B3WError(100, f"{len(sources)} sources and {len(lengths)} lengths")
    if not 0 <= group_log <= MAX_GROUP_LOG:
        raise B3WError(100, f"group_log {group_log} is not in 0 .. {MAX_GROUP_LOG}")


def _pump_many(ctx, kind, sources, lengths, window_bytes, group_log, lanes, ring, out):
    """Up to `lanes` files open at once; a round copies the next window of every open file into one of `ring` device slabs of
    lanes x window_bytes (each slab with a stream and an event of its own) and makes ONE push_many of them; the files that end in a
    round are finished by one finish_many and their lanes handed on.  The current stream ends up behind everything."""
    n = len(sources)
    if not n:
        return
    lengths = [int(x) for x in lengths]
    lanes = min(lanes, n)
    # a pinned uint8 tensor is copied from where it lies; every other source goes through the pinned host slabs
    direct = [src.reshape(-1) if isinstance(src, torch.Tensor) and src.dtype == torch.uint8 and src.is_pinned() else None for src in sources]
    for f in range(n):
        if direct[f] is not None and direct[f].numel() < lengths[f]:
            raise B3WError(100, f"source {f} holds {direct[f].numel()} bytes, fewer than the length given ({lengths[f]})")
    staged = any(direct[f] is None and lengths[f] for f in range(n))
    cur = torch.cuda.current_stream()
    slabs = [dict(h=torch.empty(lanes * window_bytes if staged else 0, dtype=torch.uint8, pin_memory=True),
                  d=torch.empty(lanes * window_bytes, dtype=torch.uint8, device=out["device"]), s=torch.cuda.Stream(), ev=torch.cuda.Event(), used=False)
             for _ in range(ring)]
    for sl in slabs:
        sl["s"].wait_stream(cur)                        # (what the caller enqueued before, e.g. the outboards' arrival, comes first)
    every, open_, nxt, rnd = [], [None] * lanes, 0, 0   # open_[lane] = [session, file, fill, next offset]
    try:
        while True:
            ended = []
            for lane in range(lanes):                   # free lanes take the next files; a file of no bytes only needs its finish
                while open_[lane] is None and nxt < n:
                    f, nxt = nxt, nxt + 1
                    se = _Lane(ctx, kind, lengths[f], group_log, out, f)
                    every.append(se)
                    if not lengths[f]:
                        ended.append(se)
                        continue
                    src = sources[f]
                    fill = None if direct[f] is not None else _reader(src.numpy() if isinstance(src, torch.Tensor) else src, lengths[f])
                    open_[lane] = [se, f, fill, 0]
            live = [lane for lane in range(lanes) if open_[lane] is not None]
            if not live and not ended:
                break
            sl = slabs[rnd % ring]
            if live:
                if sl["used"] and staged:
                    sl["ev"].synchronize()              # the slab's last copies are through with the host buffer
                ses, offs, wins = [], [], []
                with torch.cuda.stream(sl["s"]):        # (the device slab's reuse is ordered by its stream)
                    for lane in live:
                        se, f, fill, off = open_[lane]
                        nb = min(window_bytes, lengths[f] - off)
                        d = sl["d"][lane * window_bytes:lane * window_bytes + nb]
                        if fill is None:
                            d.copy_(direct[f][off:off + nb], non_blocking=True)
                        else:
                            h = sl["h"][lane * window_bytes:lane * window_bytes + nb]
                            fill(h.numpy(), off)
                            d.copy_(h, non_blocking=True)
                        ses.append(se); offs.append(off); wins.append(d)
                        open_[lane][3] = off + nb
                        if off + nb == lengths[f]:
                            ended.append(se)
                            open_[lane] = None
                    push_many(ses, offs, wins, stream=sl["s"].cuda_stream)
                    sl["ev"].record(sl["s"])
                sl["used"] = True
            if ended:                                   # behind every push of theirs: the other slabs' last rounds too
                for other in slabs:
                    if other is not sl and other["used"]:
                        sl["s"].wait_event(other["ev"])
                _finish_many(ended, sl["s"].cuda_stream)
            rnd += 1
        for sl in slabs:
            cur.wait_stream(sl["s"])
    finally:
        for se in every:
            se.close()


def outboard_stream_many(ctx, sources, lengths, window_bytes=DEFAULT_MANY_WINDOW_BYTES, group_log=0, lanes=DEFAULT_MANY_LANES, ring=2, device="cuda"):
    """The outboards and roots of MANY files that are not resident on the device, `lanes` of them in flight at once: sources[f] is a
    source as outboard_stream takes one (bytes-like, numpy, an object with readinto, or a pinned uint8 tensor, which is copied from
    where it lies) of lengths[f] bytes.  Every round is one launch whatever `lanes` is (push_many), and so are the finishes of the
    files that end in it.  Device memory made here is ring x lanes x window_bytes + the outboards + the scratches (32 bytes per MiB of
    a file), however many files there are and whatever their lengths.  Returns the dict outboard_batch (group_log 0) /
    outboard_groups_batch return for the files as one batch; the work is enqueued, the current stream ordered behind it."""
    _many_args(sources, lengths, window_bytes, group_log, lanes, ring)
    ln = _u64([int(x) for x in lengths])
    ob_first = group_batch_layout(ln, group_log)
    out = dict(device=device, ob_first=ob_first, outboards=torch.empty(int(ob_first[-1]), dtype=torch.uint8, device=device),
               roots=torch.empty((ln.size, 8), dtype=torch.int32, device=device))
    _pump_many(ctx, STREAM_OUTBOARD, sources, lengths, window_bytes, group_log, lanes, ring, out)
    return dict(outboards=out["outboards"], ob_first=ob_first, roots=out["roots"])


def verify_stream_many(ctx, sources, lengths, d_outboards, d_roots, window_bytes=DEFAULT_MANY_WINDOW_BYTES, group_log=0, lanes=DEFAULT_MANY_LANES, ring=2):
    """verify_batch for MANY files that are not resident on the device against their resident outboards (d_outboards, packed as
    outboard_batch / outboard_groups_batch leave them) and roots (d_roots, 8 words a file): the windows go as in outboard_stream_many.
    Device memory made here is ring x lanes x window_bytes + the statuses (a byte a unit, 12 bytes a file) + the scratches (36 bytes
    per MiB of a file).  Returns the dict verify_batch returns for the files as one batch."""
    _many_args(sources, lengths, window_bytes, group_log, lanes, ring)
    ln = _u64([int(x) for x in lengths])
    ob_first, unit_first = group_batch_layout(ln, group_log), verify_layout(ln, group_log)
    assert d_outboards.is_cuda and d_outboards.dtype == torch.uint8 and d_outboards.is_contiguous() and d_outboards.numel() >= int(ob_first[-1])
    assert d_roots.is_cuda and d_roots.is_contiguous() and d_roots.element_size() == 4 and d_roots.numel() >= ln.size * 8
    dev = d_outboards.device
    out = dict(device=dev, ob_first=ob_first, outboards=d_outboards, roots=d_roots, unit_first=unit_first,
               unit_status=torch.empty(int(unit_first[-1]), dtype=torch.uint8, device=dev),
               file_status=torch.empty(ln.size, dtype=torch.int32, device=dev), first_bad=torch.empty(ln.size, dtype=torch.int64, device=dev))
    _pump_many(ctx, STREAM_VERIFY, sources, lengths, window_bytes, group_log, lanes, ring, out)
    return dict(unit_status=out["unit_status"], unit_first=unit_first, file_status=out["file_status"], first_bad=out["first_bad"])


# ---- many open-length sessions finished at once ----------------------------------------------------------------------------------
def open_finish_many(sessions, d_tails=None, stream=0):
    """session.finish(d_tails[i]) for every StreamOutboardOpen session (of one context, group_log free per session) as ONE call of at
    most four launches on `stream`, which the caller orders behind every push.  d_tails: a list of uint8 CUDA tensors or Nones (None:
    no session has a tail).  Every outboard and root is made as finish() makes them, the length known from the bytes counted.  If any
    entry would be refused nothing is launched and no session changes (B3WError names the entry).  -> the list of finish()'s dicts."""
    n = len(sessions)
    d_tails = [None] * n if d_tails is None else list(d_tails)
    if len(d_tails) != n:
        raise B3WError(100, f"open_finish_many: {n} sessions and {len(d_tails)} tails")
    if not n:
        return []
    for se in sessions:
        if not isinstance(se, StreamOutboardOpen):
            raise B3WError(100, "open_finish_many: not a StreamOutboardOpen session")
    hs = _handles(sessions)
    tails = [0 if t is None else t.numel() for t in d_tails]
    for t, nb in zip(d_tails, tails):
        if nb:
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    ob_firsts = [group_batch_layout([se._bytes + nb], se.group_log) for se, nb in zip(sessions, tails)]
    obs = [torch.empty(int(f[-1]), dtype=torch.uint8, device=se.device) for se, f in zip(sessions, ob_firsts)]
    roots = [torch.empty((1, 8), dtype=torch.int32, device=se.device) for se in sessions]
    tp = np.array([t.data_ptr() if nb else 0 for t, nb in zip(d_tails, tails)], dtype=np.uint64)
    op, rp = np.array([o.data_ptr() for o in obs], dtype=np.uint64), np.array([r.data_ptr() for r in roots], dtype=np.uint64)
    tb, ob = _u64(tails), _u64([o.numel() for o in obs])
    lens = np.zeros(n, dtype=np.uint64)
    ctx = sessions[0].ctx
    _chk(ctx, lib().b3w_bao_stream_open_finish_many(ctx.handle, hs.ctypes.data, tp.ctypes.data, tb.ctypes.data, op.ctypes.data, ob.ctypes.data,
                                                    rp.ctypes.data, n, _stream(stream), lens.ctypes.data), "b3w_bao_stream_open_finish_many")
    out = []
    for i, se in enumerate(sessions):
        se.length, se.outboards, se.ob_first, se.roots = int(lens[i]), obs[i], ob_firsts[i], roots[i]
        out.append(dict(outboards=obs[i], ob_first=ob_firsts[i], roots=roots[i], length=se.length))
    return out


def _open_many_args(sources, capacities, window_bytes, group_log, lanes, ring):
    """what outboard_stream_open_many refuses before it makes anything"""
    if lanes < 1:
        raise B3WError(100, "lanes must be at least 1")
    _open_args(0, window_bytes, group_log, ring)
    if len(sources) != len(capacities):
        raise B3WError(100, f"{len(sources)} sources and {len(capacities)} capacities")
    for f, (src, cap) in enumerate(zip(sources, capacities)):
        if cap < 0:
            raise B3WError(100, f"capacity {cap} of source {f} is negative")
        if not hasattr(src, "readinto"):                # a buffer is taken whole: its size is known at once
            size = src.nbytes if isinstance(src, np.ndarray) else memoryview(src).nbytes
            if size > cap:
                raise B3WError(100, f"source {f} holds {size} bytes, more than its capacity ({cap})")


def _open_reader(source):
    """-> fill(dst) -> the bytes put into dst (a writable numpy uint8 view): fewer than dst holds only at the source's end"""
    if hasattr(source, "readinto"):
        def fill(dst):
            view, got = memoryview(dst), 0
            while got < len(view):
                k = source.readinto(view[got:])
                if not k:
                    break
                got += k
            return got
        return fill
    data = np.frombuffer(source, dtype=np.uint8) if not isinstance(source, np.ndarray) else source.reshape(-1).view(np.uint8)
    at = [0]

    def fill(dst):
        got = min(dst.size, data.size - at[0])
        dst[:got] = data[at[0]:at[0] + got]
        at[0] += got
        return got
    return fill


def outboard_stream_open_many(ctx, sources, capacities, window_bytes=DEFAULT_MANY_WINDOW_BYTES, group_log=0, lanes=DEFAULT_MANY_LANES, ring=2):
    """outboard_stream_many for sources of UNKNOWN length, `lanes` of them in flight at once: sources[f] is what outboard_stream_open
    takes (an object with readinto, read until it returns 0, a short read not being the end; or a bytes-like / numpy buffer, taken
    whole) and capacities[f] bounds it; a source that yields more raises B3WError.  A round copies the next window of every open file
    into its place in one of `ring` slabs of lanes x window_bytes (pinned host + device, a stream and an event each), pushes the whole
    MiB of all lanes with ONE push_many and finishes the files that ended in the round with ONE open_finish_many on the slab's stream,
    their tails still lying in the slab; a file that ends exactly on a window's last byte is found by the empty read of the next round
    and gets no push and no tail.  Device memory made here is ring x lanes x window_bytes + per open lane a staging and a scratch for
    its file's capacity + the outboards and roots: a finished file's staging and scratch are dropped with its session.
    -> the list of StreamOutboardOpen.finish()'s dicts, one per file (no packed tensor: no length is known before a file's end); the
    work is enqueued, the current stream ordered behind it.
    The defaults are outboard_stream_many's and as unmeasured as they are there."""
    _open_many_args(sources, capacities, window_bytes, group_log, lanes, ring)
    n = len(sources)
    if not n:
        return []
    capacities = [int(c) for c in capacities]
    lanes = min(lanes, n)
    cur = torch.cuda.current_stream()
    slabs = [dict(h=torch.empty(lanes * window_bytes, dtype=torch.uint8, pin_memory=True),
                  d=torch.empty(lanes * window_bytes, dtype=torch.uint8, device="cuda"), s=torch.cuda.Stream(), ev=torch.cuda.Event(), used=False)
             for _ in range(ring)]
    for sl in slabs:
        sl["s"].wait_stream(cur)
    results, open_, nxt, rnd = [None] * n, [None] * lanes, 0, 0                # open_[lane] = [session, file, fill, bytes so far]
    try:
        try:
            while True:
                for lane in range(lanes):               # free lanes take the next files
                    if open_[lane] is None and nxt < n:
                        f, nxt = nxt, nxt + 1
                        open_[lane] = [StreamOutboardOpen(ctx, capacities[f], group_log), f, _open_reader(sources[f]), 0]
                live = [lane for lane in range(lanes) if open_[lane] is not None]
                if not live:
                    break
                sl = slabs[rnd % ring]
                if sl["used"]:
                    sl["ev"].synchronize()              # the slab's last copies, pushes and finishes are through with both buffers
                ses, offs, wins, ended, tails = [], [], [], [], []
                with torch.cuda.stream(sl["s"]):        # (the device slab's reuse is ordered by its stream)
                    for lane in live:
                        se, f, fill, total = open_[lane]
                        at = lane * window_bytes
                        got = fill(sl["h"][at:at + window_bytes].numpy())
                        if total + got > capacities[f]:
                            raise B3WError(100, f"source {f} yields more than its capacity ({capacities[f]} bytes)")
                        whole = got // TILE_BYTES * TILE_BYTES
                        if got:
                            sl["d"][at:at + got].copy_(sl["h"][at:at + got], non_blocking=True)
                        if whole:
                            ses.append(se); offs.append(total); wins.append(sl["d"][at:at + whole])
                        open_[lane][3] = total + got
                        if got < window_bytes:          # the source has ended: in this window, or on the last byte of the one before
                            ended.append(lane)
                            tails.append(sl["d"][at + whole:at + got] if got > whole else None)
                    push_many(ses, offs, wins, stream=sl["s"].cuda_stream)
                if ended:                               # behind every push of theirs: the other slabs' last rounds too
                    for other in slabs:
                        if other is not sl and other["used"]:
                            sl["s"].wait_event(other["ev"])
                    done = [open_[lane][0] for lane in ended]
                    # (outside the slab's stream: the outboards and roots are the current stream's memory, as the sessions' is)
                    for lane, got in zip(ended, open_finish_many(done, tails, stream=sl["s"].cuda_stream)):
                        results[open_[lane][1]] = got
                sl["ev"].record(sl["s"])
                sl["used"] = True
                if ended:
                    # The finished sessions' stagings and scratches are dropped here, and the next sessions (or outboards) may be given
                    # the same memory at once: every slab's stream is put behind these finishes first.
                    for other in slabs:
                        if other is not sl:
                            other["s"].wait_event(sl["ev"])
                    for lane in ended:
                        open_[lane][0].close()
                        open_[lane] = None
                    se = done = None                    # (the loop's own references: a dropped session's memory goes with the last one)
                rnd += 1
        finally:                                        # (also on a raise: nothing is dropped under work in flight)
            for sl in slabs:
                cur.wait_stream(sl["s"])
    finally:
        for ent in open_:
            if ent is not None:
                ent[0].close()
    return results
