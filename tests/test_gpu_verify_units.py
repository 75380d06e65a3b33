"""The tamper check (b3w_batch_verify_device: expand_verify, body_input_word, publish_counts in csrc/b3w_kernels.hip) pinned to the CPU
restatement tests/verify_ref.py: the verdict on EVERY 16-byte unit and every word of it, the edges of the tiling for every body
alignment, the attribution of counts to bodies, every input slot and every copy of an input atom, and the host wrapper.

The bodies under test are the ORACLE's, uploaded — never the witness kernels' — and every expected count is an integer from the oracle
and numpy.  Every launch writes into n + 8 words preset to a sentinel: the n counts must all be written, the 8 behind them not.
The plans executed here are proved on the CPU by tests/test_verify_ref_cpu.py."""
import numpy as np
import pytest

import b3w_testlib as T
import verify_ref as V

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7C0DE           # no count (<= 2 * nwit) and not 0xFFFFFFFF
FILL = 0xC3
N = V.N_EDGE

_cache = {}


def _records(circuit, n, first):
    W = T.workloads()
    return W.config2_compression(n, first=first) if circuit == "compression" else W.config3_nova(n, first=first)


def _verify(ctx, ptr, n, pitch):
    import torch
    d_mm = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    ctx.verify_device(ptr, n, pitch, d_mm.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    mm = d_mm.cpu().numpy().view(np.uint32)
    assert (mm[n:] == SENTINEL).all(), ("words behind the n counts were written", mm[n:])
    assert (mm[:n] != SENTINEL).all(), ("counts left unwritten", np.flatnonzero(mm[:n] == SENTINEL)[:8])
    return mm[:n].astype(np.int64)


def _place(d_packed, pad, base, n=None):
    """n bodies `body + pad` bytes apart, the first `base` bytes into a 256-byte aligned buffer of FILL; d_packed is [n, body] or one
    body for all.  -> (buffer, pointer of body 0, pitch, the [n, pitch] byte view of the bodies and their padding)"""
    import torch
    body = d_packed.shape[-1]
    n = d_packed.shape[0] if n is None else n
    pitch = body + pad
    buf = torch.full((base + n * pitch + 256,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    rows = buf[base: base + n * pitch].view(n, pitch)
    rows[:, :body] = d_packed
    return buf, buf.data_ptr() + base, pitch, rows


def _xor_bits(rows, plants):
    """plants [(body, unit, word, bit)]: XOR on the device, in place; applying it twice restores the buffer"""
    import torch
    bi = torch.tensor([p[0] for p in plants], device="cuda")
    by = torch.tensor([16 * p[1] + 4 * p[2] + p[3] // 8 for p in plants], device="cuda")
    val = torch.tensor([1 << (p[3] % 8) for p in plants], dtype=torch.uint8, device="cuda")
    rows[bi, by] = rows[bi, by] ^ val


def _attribution(circuit):
    """37 oracle bodies, body i with attribution_plan's i plants (on the host, before the upload), and the reference's counts; one circuit
    at a time is kept (tests c and e share it)"""
    if circuit not in _cache:
        _cache.clear()
        recs = _records(circuit, N, first=150)
        bad, bodies = T.oracle_batch_u32(circuit, recs)
        assert bad == 0
        bodies = bodies.copy()
        for i, plants in enumerate(V.attribution_plan(circuit)):
            for u, wd, bit in plants:
                V.plant(bodies[i], u, wd, bit)
        want = np.array([V.verify_ref(circuit, bodies[i]) for i in range(N)], dtype=np.int64)
        assert np.array_equal(want, np.arange(N))
        _cache[circuit] = (recs, bodies, want)
    return _cache[circuit]


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_sweep_every_unit_and_every_word(circuit):
    """a. 17 residue classes x 4 words = 68 bodies from 68 records, natural pitch (strides 4, 4, 4, 2): body 4 r + wd has every unit
    u = r (mod 17) outside the input slots tampered in word wd — bit slots receive values >= 2, the zero upper halves and words 2 / 3 of
    narrow slots non-zero values, each word of the 256-bit slots is hit in both halves.  Count = planted = reference, for every body."""
    import torch
    n = 4 * V.MOD
    recs = _records(circuit, n, first=1000)
    bad, bodies = T.oracle_batch_u32(circuit, recs)
    assert bad == 0
    bodies = bodies.copy()
    planted = np.array([V.plant_sweep(circuit, bodies[4 * r + wd], r, wd) for r in range(V.MOD) for wd in range(4)], dtype=np.int64)
    assert planted.sum() == 4 * (V.n_units(circuit) - V.input_units(circuit).size)
    want = np.array([V.verify_ref(circuit, bodies[b]) for b in range(n)], dtype=np.int64)
    assert np.array_equal(planted, want)
    ctx = T.pkg().Context(circuit, 0)
    d = torch.from_numpy(bodies).cuda()
    mm = _verify(ctx, d.data_ptr(), n, 0)
    print(circuit, "sweep: planted", planted[:8], "... counted", mm[:8], "...")
    wrong = [(b, b // 4, b % 4, int(mm[b]), int(want[b])) for b in range(n) if mm[b] != want[b]]
    assert not wrong, ("(body, residue, word, counted, planted)", wrong[:8])
    ctx.close()


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_edges_of_the_tiling_one_unit_alone_in_a_body(circuit):
    """b. n = 37 bodies, pitch pads {0, 32, 64, 96} x base offsets {0, 16, 32, 64, 96}: one plant in one edge unit of the victim's own j
    (first slots, first tile border, first group of four, the slots around the tail iteration and the last tile, the last slots — both
    halves) per victim, three launches per configuration (victims i = l mod 3, so every wave mixes victims and clean bodies and every
    body is a victim once).  Each victim reports exactly 1 — not 0 (a missed tail), not 2..4 (a clamped tile counted again) — and every
    other body 0.  The plants are XORed on the device and taken out again; one 37-body buffer per configuration."""
    import torch
    recs = _records(circuit, N, first=77)
    bad, bodies = T.oracle_batch_u32(circuit, recs)
    assert bad == 0
    bodies = bodies.copy()
    d_packed = torch.from_numpy(bodies).cuda()
    ctx = T.pkg().Context(circuit, 0)
    first = True
    for pad, base, launches in V.edge_plan(circuit):
        buf, ptr, pitch, rows = _place(d_packed, pad, base)
        clean = buf.clone()
        assert not _verify(ctx, ptr, N, pitch).any(), (pad, base, "clean oracle bodies")
        for plants in launches:
            want = np.zeros(N, dtype=np.int64)
            for i, u, wd, bit in plants:
                if first:                                                    # the reference's verdict; it does not depend on where the body lies
                    body = bodies[i].copy()
                    V.plant(body, u, wd, bit)
                    assert V.verify_ref(circuit, body) == 1
                want[i] = 1
            _xor_bits(rows, plants)
            mm = _verify(ctx, ptr, N, pitch)
            _xor_bits(rows, plants)
            wrong = [(i, V.tile_j(ptr + i * pitch), int(mm[i]), int(want[i])) for i in range(N) if mm[i] != want[i]]
            assert not wrong, (pad, base, "(body, j, counted, wanted)", wrong[:8],
                               "plants (body, unit, word, bit)", [p for p in plants if p[0] in {w[0] for w in wrong}][:8])
            first = False
        assert torch.equal(buf, clean), (pad, base, "the plants were not taken out again")
        del buf, rows, clean
    ctx.close()


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_counts_are_attributed_to_the_right_body(circuit):
    """c. body i carries exactly i tampered units (body 0 none), so neighbouring bodies of a wave — 1, 2 or 4 apart, W = 4 or 2 — all
    differ: mm[i] == i for every pitch pad."""
    import torch
    _recs, bodies, want = _attribution(circuit)
    d_packed = torch.from_numpy(bodies).cuda()
    ctx = T.pkg().Context(circuit, 0)
    for pad in V.PADS:
        buf, ptr, pitch, _rows = _place(d_packed, pad, 0)
        mm = _verify(ctx, ptr, N, pitch)
        assert np.array_equal(mm, want), (pad, mm)
        del buf, _rows
    ctx.close()


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_every_input_slot_and_every_copy_of_an_input_atom(circuit):
    """d. for every record word j, on a leaf-step and a parent-step body (or a compression body): bit 0 and bit 31 of the low word of
    in_slots[j] flipped — the count of the witness recomputed from the NEW record, exactly, or 0xFFFFFFFF where that record is refused;
    word 1, word 3 or a byte of the upper half set — 0xFFFFFFFF; every other slot holding a copy of an input atom flipped — exactly 1.
    One case per victim, victims three bodies apart, so every victim has clean bodies of the same record in its wave: they stay 0.
    Twice: natural pitch, and a pitch of whole 128-byte lines (stride 1) from a 16-byte aligned start."""
    import torch
    cases = V.input_cases(circuit)
    n = 3 * len(cases)
    ctx = T.pkg().Context(circuit, 0)
    body_bytes = T.NWIT[circuit] * 32
    for name, rec in V.base_records(circuit).items():
        rc, b = T.oracle_each_u32(circuit, rec[None, :])
        assert rc[0] == 0
        want = np.zeros(n, dtype=np.int64)
        for c, case in enumerate(cases):
            body = b[0].copy()
            V.apply_case(body, case)
            want[3 * c] = V.verify_ref(circuit, body)
        kinds = np.array([c[0] for c in cases])
        assert (want[0::3][kinds == "upper"] == V.REJECTED).all() and (want[0::3][kinds == "copy"] == 1).all()
        d_base = torch.from_numpy(b[0]).cuda()
        vi = torch.arange(0, n, 3, device="cuda")
        col = torch.tensor([8 * c[2] + c[3] for c in cases], device="cuda")
        mask = torch.from_numpy(np.array([c[4] for c in cases], dtype=np.uint32).view(np.int32)).cuda()
        for pad, base in ((0, 0), (-body_bytes % 128, 16)):
            buf, ptr, pitch, rows = _place(d_base, pad, base, n)
            words = buf[base: base + n * pitch].view(torch.int32).view(n, pitch // 4)
            words[vi, col] = words[vi, col] ^ mask
            mm = _verify(ctx, ptr, n, pitch)
            print(circuit, name, "pad", pad, "base", base, "low-word counts", mm[0::3][kinds == "low"][:10], "...")
            wrong = [(cases[i // 3] if i % 3 == 0 else "clean neighbour", i, int(mm[i]), int(want[i])) for i in range(n) if mm[i] != want[i]]
            assert not wrong, (name, pad, base, "(case (kind, word, slot, word of slot, mask), body, counted, wanted)", wrong[:8])
            del buf, rows, words
    ctx.close()


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_host_wrapper_returns_the_device_calls_counts(circuit):
    """e. Batch.verify() (b3w_batch_verify) over test c's bodies, copied into the batch's own buffer behind a run of the same records:
    the same array as b3w_batch_verify_device on that buffer, and the reference's."""
    import torch
    m = T.pkg()
    recs, bodies, want = _attribution(circuit)
    ctx = m.Context(circuit, 0)
    batch = m.Batch(ctx, N)
    batch.run(recs)
    assert not batch.verify().any()
    ptr, pitch = batch.device_ptr()

    class _Dev:
        def __init__(self, p, nb):
            self.__cuda_array_interface__ = {"shape": (nb,), "typestr": "|u1", "data": (p, False), "version": 2, "strides": None}
    d = torch.as_tensor(_Dev(ptr, N * pitch), device="cuda").view(N, pitch)
    d[:, :ctx.body_bytes] = torch.from_numpy(bodies).cuda()
    torch.cuda.synchronize()
    host = batch.verify()
    dev = _verify(ctx, ptr, N, pitch)
    assert host.dtype == np.uint32 and np.array_equal(host.astype(np.int64), dev) and np.array_equal(dev, want), (host, dev)
    del d
    batch.close(); ctx.close()
