"""b3w_batch_commit_device on bodies this library did not write: the verdict (0 / 103) of every case of tests/commit_domain_cases.py
compared exactly, the point of every verdict-0 case byte for byte with the plain-integer reference (tests/commit_domain_ref.py: the
generators are A + i B, so a commitment is two scalar multiplications), and the launch's count of point additions.

Which instantiation of b3w_commit_kernel a launch takes follows from b3w_launch_commit (it cannot be observed): T = 64 lanes per
witness for the 18-bit table, for more than 55 200 virtual bits and from 8 192 bodies on, else 32 (two witnesses per wave); the
Pasta modulus with compile-time limbs (B3wCurve9Vesta) for T = 64 on the Pallas curve, else the modulus at run time.

    key                          window  instantiation
    compression-w12              12      T 32, generic
    compression-w16-from17       16      T 32, generic
    compression-pallas-from45    12      T 32, Pasta modulus at run time
    compression-w18-narrow       18      T 64, generic
    compression-w12-8195         12      T 64, generic (8 195 bodies); the table's launch itself is T 32
    nova_bn254-w12 / -w16        12, 16  T 64, generic, inverse tables
    nova_vesta-w12 / -w16        12, 16  T 64, Vesta constants, inverse tables
    nova_vesta-w18-narrow        18      T 64, Vesta constants, inverse tables
    nova_vesta-on-bn254-narrow   12      T 32 (a narrow key), no inverse tables: the order of BN254 G1 is not the circuit's prime
    nova_vesta-folded            12      T 32 (43 876 virtual bits), codes 4 and 8-39, inverse tables
    compression-folded           12      T 32, code 4
    nova_bn254_o1-w12            12      T 64, generic, 64-bit and 256-bit slots, no tables
"""
import time

import numpy as np
import pytest

import b3w_testlib as T
import commit_domain_cases as C
import commit_domain_ref as R
import ec_ref as E

pytestmark = pytest.mark.gpu

_points = {}


def _reference_points(name, tab, curve):
    """[n, 64] bytes: the point of every verdict-0 case (zeros where the verdict is 103: not compared)"""
    if name not in _points:
        out = np.zeros((len(tab["cases"]), 64), dtype=np.uint8)
        memo = {}
        for k, sc in enumerate(C.reference_scalars(tab)):
            if sc is None:
                continue
            if sc not in memo:
                memo[sc] = np.frombuffer(E.points_to_bytes([R.point(curve, *sc)]), dtype=np.uint8)
            out[k] = memo[sc]
        _points[name] = out
    return _points[name]


def _compare(what, tab, order, st, pts, want_pts, with_status=True):
    names = [tab["cases"][i][0] for i in order]
    verdict = np.array([tab["cases"][i][3] for i in order], dtype=np.int32)
    if with_status:
        wrong = [(names[j], int(st[j]), int(verdict[j])) for j in range(len(order)) if st[j] != verdict[j]]
        assert not wrong, (what, "status", wrong[:8])
    want = want_pts[order]
    bad = [names[j] for j in range(len(order)) if verdict[j] == 0 and not np.array_equal(pts[j], want[j])]
    assert not bad, (what, "point", len(bad), bad[:8])


@pytest.mark.parametrize("name", [k[0] for k in C.KEYS])
def test_verdict_and_point_of_foreign_bodies(name):
    import torch
    t_start = time.perf_counter()
    m = T.pkg()
    (_, circuit, curve, first_slot, window, fold, n_large), tab, t, tables = C.key_table(name)
    n = len(tab["cases"])
    ctx = m.Context(circuit, 0)
    assert [int(w) for w in ctx.slot_widths()] == tab["widths"]
    body = ctx.body_bytes
    gens = E.related_points(curve, ctx.witness_size - first_slot)
    key = m.CommitKey(ctx, curve, E.points_to_bytes(gens), first_slot, window, fold=True if fold else None)
    assert key.window == window
    if fold:
        assert key.folded_slots == sum(1 for v in tab["mask"] if v)
    want_pts = _reference_points(name, tab, curve)
    s = torch.cuda.current_stream().cuda_stream
    # the bodies: the base bodies uploaded, expanded and edited on the device
    base, idx, ci, si, raw = C.bodies_plan(tab)
    d_base = torch.from_numpy(base).cuda()
    d = d_base.index_select(0, torch.from_numpy(idx).cuda())
    d.view(n, -1, 32)[torch.from_numpy(ci).cuda(), torch.from_numpy(si).cuda()] = torch.from_numpy(raw).cuda()

    def launch(rows, pitch, offset, status=True):
        """the bodies `rows` of d in a buffer of its own with this pitch, `offset` bytes into it, garbage between and around them"""
        k = len(rows)
        sel = d if k == n and list(rows) == list(range(n)) else d.index_select(0, torch.tensor(rows, device="cuda"))
        if pitch == body and offset == 0:
            buf, ptr = sel, sel.data_ptr()
        else:
            buf = torch.full((k * pitch + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            buf[offset:offset + k * pitch].view(k, pitch)[:, :body] = sel
            ptr = buf.data_ptr() + offset
        d_pts = torch.full((k, 64), 7, dtype=torch.uint8, device="cuda")
        d_st = torch.full((k,), -1, dtype=torch.int32, device="cuda")
        key.commit_device(ptr, k, 0 if pitch == body else pitch, d_pts.data_ptr(), d_st.data_ptr() if status else 0, s)
        torch.cuda.synchronize()
        return d_st.cpu().numpy(), d_pts.cpu().numpy()

    every = list(range(n))
    # 1. the table, packed, with the count of additions: flagged bodies count too (phase 2 runs on the low bits their classes keep)
    key.count(True)
    st, pts = launch(every, body, 0)
    adds, wits = key.counts()
    key.count(False)
    _compare("packed", tab, every, st, pts, want_pts)
    total, per = C.reference_additions(tab, window)
    assert wits == n
    if adds != total:                                          # name the cases: one launch per body
        off = []
        for k in every:
            key.count(True)
            launch([k], body, 0)
            a, _ = key.counts()
            if a != per[k]:
                off.append((tab["cases"][k][0], a, per[k]))
        key.count(False)
        pytest.fail(f"{name}: {adds} additions counted, {total} expected; by case (counted, expected): {off[:8]} ({len(off)} cases)")
    # 2. / 3. pitches, a bodies pointer 16 bytes into its buffer, launches of 4k + 2 and 4k + 1 bodies
    st, pts = launch(every[:n - 1], body + 16, 0)
    _compare("pitch + 16", tab, every[:n - 1], st, pts, want_pts)
    st, pts = launch(every[:n - 2], body + 48, 16)
    _compare("pitch + 48, 16 bytes in", tab, every[:n - 2], st, pts, want_pts)
    assert {n % 4, (n - 1) % 4, (n - 2) % 4} == {1, 2, 3}
    # 4. no status array: the same points
    st, pts = launch(every, body, 0, status=False)
    assert (st == -1).all()
    _compare("d_status = NULL", tab, every, st, pts, want_pts, with_status=False)
    # 5. a large launch: the table's cases first and last, copies of a base body between
    if n_large:
        half = (n + 1) // 2
        mid = next(k for k, c in enumerate(tab["cases"]) if c[3] == 0 and not c[2])
        rows = every[:half] + [mid] * (n_large - n) + every[half:]
        st, pts = launch(rows, body, 0)
        _compare(f"{n_large} bodies", tab, rows, st, pts, want_pts)
    key.close(); ctx.close()
    print(f"commit domain {name}: {n} cases, T {t}, {time.perf_counter() - t_start:.1f} s")


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_independent_generators_and_the_plain_sum(circuit):
    """The shortcut itself: two verdict-0 cases per circuit under a key of INDEPENDENT generators (ec_ref.random_points) over the last
    slots of the witness — the oracle's body as it stands and one with a wide slot replaced — against the plain multi-scalar sum
    ec_ref.commit of the committed vector.  (A witness's worth of independent points is 10 s of square roots; the last 340 slots
    of the O2 nova builds hold all 67 inverses, the last 3 000 of the other two their 64-bit and 256-bit slots.)"""
    import torch
    m = T.pkg()
    o2 = circuit in ("nova_bn254", "nova_vesta")
    curve = "pallas" if circuit == "nova_vesta" else "bn254_g1"
    first_slot = 22950 if o2 else 21000
    ctx = m.Context(circuit, 0)
    nslots = ctx.witness_size - first_slot
    _, vbits = R.first_virtual(R.classes(R.slot_widths(circuit), first_slot))
    tab = C.table(circuit, first_slot, False, o2, C.lanes_per_witness(vbits, 12, 2))
    gens = E.random_points(curve, nslots)
    key = m.CommitKey(ctx, curve, E.points_to_bytes(gens), first_slot, 12)
    inside = [k for k, c in enumerate(tab["cases"]) if c[3] == 0]
    wide = [k for k in inside if any(v >> 33 for sl, v in tab["cases"][k][2].items() if sl >= first_slot)]
    picks = [inside[0], wide[0]]
    assert not tab["cases"][picks[0]][2] and tab["cases"][picks[0]][1] == 0
    base, idx, ci, si, raw = C.bodies_plan(tab)
    d = torch.from_numpy(base).cuda().index_select(0, torch.from_numpy(idx[picks]).cuda())
    for j, k in enumerate(picks):
        for sl, v in tab["cases"][k][2].items():
            d[j, 32 * sl:32 * sl + 32] = torch.from_numpy(np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8).copy()).cuda()
    d_pts = torch.zeros((2, 64), dtype=torch.uint8, device="cuda")
    d_st = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    key.commit_device(d.data_ptr(), 2, 0, d_pts.data_ptr(), d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got, st = d_pts.cpu().numpy(), d_st.cpu().numpy()
    for j, k in enumerate(picks):
        vals = C.case_values(tab, tab["cases"][k])
        assert st[j] == 0
        assert E.point_from_bytes(got[j].tobytes()) == E.commit(R.committed(vals, tab["cls"]), gens, curve), tab["cases"][k][0]
    key.close(); ctx.close()


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_slot_widths_are_the_fixtures(circuit):
    """tests/golden/slot_widths.json is b3w_slot_widths of the four builds: the CPU side of these tests classifies slots by it"""
    m = T.pkg()
    ctx = m.Context(circuit, 0)
    assert [int(w) for w in ctx.slot_widths()] == R.slot_widths(circuit)
    ctx.close()
