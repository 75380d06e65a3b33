"""The edges of the record domain (tests/record_domain_cases.py) on every launch route of the batch kernels: the body-stream and
launch-shape variants, the persistent grid, the fill-ordered kernel, the trace + sweep pair, the tamper check, the constraint check
and commitments from records.  The oracle's bodies are uploaded once per circuit; every comparison is byte equality on the device."""
import os

import numpy as np
import pytest

import b3w_testlib as T
import ec_ref as E
import record_domain_cases as C
from ref_models import _blake3_compress_np, _nova_public_np

pytestmark = pytest.mark.gpu

FILL = 0x6B
PUB_FILL = 0x5A5A5A5A
VARIANTS = {
    "compression": [0, 1, 2, 3, 4, 5, 6, 7, 8, 22, 28, 84, 100, 200, 201],
    "nova_bn254": [0, 1, 2, 3, 4, 22, 27, 36, 84, 100, 200, 201],          # 20 + s: sliced; 4: persistent grid; 100: trace + sweep;
    "nova_vesta": [0, 1, 2, 3, 4, 22, 27, 36, 84, 100, 200, 201],          # 200 / 201: fill-ordered
    "nova_bn254_o1": [0, 1, 23, 36, 100],
}
CURVE = {"compression": "bn254_g1", "nova_bn254": "bn254_g1", "nova_vesta": "vesta", "nova_bn254_o1": "bn254_g1"}
STATUS = {"ok": 0, "assert": 4, "domain": 103}

_cache = {}


def _table(circuit):
    """The circuit's table, the oracle's bodies of its accepted rows in HBM, and the models' public words.  One circuit at a time is
    kept (the cases below are ordered by circuit)."""
    import torch
    if circuit in _cache:
        return _cache[circuit]
    _cache.clear()
    torch.cuda.empty_cache()
    names, recs, exp = C.stack(C.compression_rows() if circuit == "compression" else C.nova_rows())
    rc, bodies = T.oracle_each_u32(circuit, recs)
    assert [int(x) for x in rc] == [4 if e == "assert" else 0 for e in exp]
    acc = np.flatnonzero(rc == 0)                                            # rows with an oracle body: "ok" and "domain"
    t = dict(names=names, recs=recs, exp=exp, acc=acc, n=len(names),
             want_st=np.array([STATUS[e] for e in exp], dtype=np.int32),
             ok=np.array([e == "ok" for e in exp]),
             host_bodies={int(i): bodies[i].copy() for i in acc if any(s in names[i] for s in ("=+2047", "=-2047", "=+2048", "=-2048", "=+2049", "=-2049"))},
             d_oracle=torch.from_numpy(bodies[acc]).cuda(),
             pos={int(i): j for j, i in enumerate(acc)})
    if circuit == "compression":
        t["pub"] = _blake3_compress_np(recs[:, 0:8], recs[:, 8:24], recs[:, 24], recs[:, 25], recs[:, 26], recs[:, 27])
    else:
        t["pub"] = _nova_public_np(recs)
    _cache[circuit] = t
    return t


def _ctx(circuit, variant=None):
    m = T.pkg()
    if variant is None:
        return m.Context(circuit, 0)
    os.environ["B3W_VARIANT"] = str(variant)
    try:
        return m.Context(circuit, 0)
    finally:
        del os.environ["B3W_VARIANT"]


def _expected_buffer(t, order, body_bytes, pitch):
    """[n + 1, pitch] bytes: the oracle's body where the row is "ok", the fill pattern everywhere else — rejected rows, the padding
    between bodies and one row behind the last body"""
    import torch
    want = torch.full((t["n"] + 1, pitch), FILL, dtype=torch.uint8, device="cuda")
    dst = [j for j, i in enumerate(order) if t["ok"][i]]
    src = [t["pos"][int(i)] for i in order if t["ok"][i]]
    want[torch.tensor(dst, device="cuda"), :body_bytes] = t["d_oracle"][torch.tensor(src, device="cuda")]
    return want


def _first_difference(t, order, got, want, body_bytes):
    import torch
    for j in range(got.shape[0]):
        if not torch.equal(got[j], want[j]):
            at = int(torch.nonzero(got[j] != want[j])[0].item())
            name = t["names"][int(order[j])] if j < len(order) else "(behind the last body)"
            return f"position {j}, row {name!r} ({t['exp'][int(order[j])] if j < len(order) else '-'}): first difference in " + \
                   (f"slot {at // 32}, byte {at % 32}" if at < body_bytes else f"the padding, byte {at - body_bytes}")
    return None


def _cases():
    return [(c, v) for c in T.CIRCUITS for v in VARIANTS[c]]


@pytest.mark.parametrize("circuit,variant", _cases())
def test_every_route_at_the_edges_of_the_record_domain(circuit, variant):
    """run_device under B3W_VARIANT: "ok" rows status 0, body byte-equal to the oracle's, public words equal to the model's; "assert"
    rows status 4 and "domain" rows status 103 with the body left at the fill pattern; nothing between or behind bodies written.  Table
    order into a packed buffer, then reversed (other lane / quad / wave positions, other neighbours) into one with pitch = body + 96."""
    import torch
    t = _table(circuit)
    n = t["n"]
    ctx = _ctx(circuit, variant)
    s = torch.cuda.current_stream().cuda_stream
    for order, pitch in ((np.arange(n), ctx.body_bytes), (np.arange(n)[::-1].copy(), ctx.body_bytes + 96)):
        d_recs = torch.from_numpy(t["recs"][order].view(np.int32)).cuda()
        d_bodies = torch.full((n + 1, pitch), FILL, dtype=torch.uint8, device="cuda")
        d_pub = torch.full((n, ctx.public_words), PUB_FILL, dtype=torch.int32, device="cuda")
        d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ctx.run_device(d_recs.data_ptr(), n, d_bodies.data_ptr(), pitch, d_pub.data_ptr(), d_st.data_ptr(), s)
        torch.cuda.synchronize()
        st = d_st.cpu().numpy()
        wrong = [(t["names"][int(i)], int(st[j]), int(t["want_st"][i])) for j, i in enumerate(order) if st[j] != t["want_st"][i]]
        assert not wrong, (circuit, variant, wrong[:8])
        want = _expected_buffer(t, order, ctx.body_bytes, pitch)
        if not torch.equal(d_bodies, want):
            pytest.fail(f"{circuit} variant {variant} pitch {pitch}: " + _first_difference(t, order, d_bodies, want, ctx.body_bytes))
        pub = d_pub.cpu().numpy().view(np.uint32)
        for j, i in enumerate(order):
            if t["ok"][i]:
                assert np.array_equal(pub[j], t["pub"][i]), (circuit, variant, t["names"][int(i)], pub[j], t["pub"][i])
        del d_bodies, want
    ctx.close()


@pytest.mark.parametrize("variant", [200, 201])
def test_fill_order_refuses_the_unsimplified_build(variant):
    """The fill-ordered kernel exists for the compression circuit and the nova O2 builds: the O1 build says so, and writes nothing."""
    import torch
    m = T.pkg()
    t = _table("nova_bn254_o1")
    ctx = _ctx("nova_bn254_o1", variant)
    n = 8
    d_recs = torch.from_numpy(t["recs"][:n].view(np.int32)).cuda()
    d_bodies = torch.full((n, ctx.body_bytes), FILL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(m.B3WError) as e:
        ctx.run_device(d_recs.data_ptr(), n, d_bodies.data_ptr(), 0, 0, d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert e.value.status == m.B3W_E_BAD_ARGUMENT
    assert bool((d_bodies == FILL).all().item()) and bool((d_st == -1).all().item())
    ctx.close()


def _inverse_slot(body, k, p):
    """the slot of an oracle body that holds 1 / k mod p — found by its value, not through a layout"""
    want = np.frombuffer(pow(k % p, -1, p).to_bytes(32, "little"), dtype=np.uint8)
    hits = np.flatnonzero((body.reshape(-1, 32) == want).all(axis=1))
    assert hits.size == 1, (k, hits)
    return int(hits[0])


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_tamper_check_on_the_oracles_bodies(circuit):
    """verify_device on the uploaded oracle bodies (not on kernel output): 0 for every "ok" row, 0xFFFFFFFF for every "domain" row
    (include/b3wit.h: inputs outside this path's domain); after one flipped byte in an IsZero inverse of three rows — |k| = 2 047
    (the last tabulated inverse), 2 048 (the first computed one) and a negative k — exactly those rows report a mismatch."""
    import torch
    t = _table(circuit)
    ctx = _ctx(circuit)
    acc = t["acc"]
    d = t["d_oracle"].clone()
    s = torch.cuda.current_stream().cuda_stream

    def verify():
        d_mm = torch.full((len(acc),), 12345, dtype=torch.int32, device="cuda")
        ctx.verify_device(d.data_ptr(), len(acc), 0, d_mm.data_ptr(), s)
        torch.cuda.synchronize()
        return d_mm.cpu().numpy().view(np.uint32)
    want = np.array([0 if t["ok"][i] else 0xFFFFFFFF for i in acc], dtype=np.uint32)
    mm = verify()
    wrong = [(t["names"][int(i)], int(mm[j])) for j, i in enumerate(acc) if mm[j] != want[j]]
    assert not wrong, wrong[:8]
    if circuit != "compression":
        victims = []
        for prefix, k in (("e1=+2047/", 2047), ("e1=+2048/", 2048), ("e1=-2049/", -2049)):
            i = next(i for i, nm in enumerate(t["names"]) if nm.startswith(prefix))
            assert t["ok"][i] and C.ks(t["recs"][i])["e1"] == k
            slot = _inverse_slot(t["host_bodies"][i], k, T.PRIME[circuit])
            d[t["pos"][i], slot * 32 + 13] ^= 0x04
            victims.append(t["pos"][i])
        mm = verify()
        for j in range(len(acc)):
            if j in victims:
                assert 1 <= mm[j] != 0xFFFFFFFF, (t["names"][int(acc[j])], int(mm[j]))
            else:
                assert mm[j] == want[j], (t["names"][int(acc[j])], int(mm[j]))
    ctx.close()


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_constraint_check_on_the_oracles_bodies(circuit):
    """R1cs.check_device over the oracle's body of EVERY accepted row, "domain" rows included: no constraint violated.  The constraint
    systems come from the circuit text alone, so this is a line of evidence on the oracle itself at these edges."""
    import torch
    m = T.pkg()
    t = _table(circuit)
    ctx = _ctx(circuit)
    r1cs = m.R1cs(ctx)
    na = len(t["acc"])
    d_viol = torch.full((na,), -1, dtype=torch.int32, device="cuda")
    d_first = torch.full((na,), 0, dtype=torch.int32, device="cuda")
    r1cs.check_device(t["d_oracle"].data_ptr(), na, 0, d_viol.data_ptr(), d_first.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    viol, first = d_viol.cpu().numpy(), d_first.cpu().numpy().view(np.uint32)
    bad = [(t["names"][int(i)], int(viol[j]), int(first[j])) for j, i in enumerate(t["acc"]) if viol[j] != 0]
    assert not bad, bad[:8]
    r1cs.close(); ctx.close()


@pytest.mark.parametrize("circuit,window", [(c, w) for c in T.CIRCUITS for w in (12, 16)])
def test_commitments_from_records_at_the_edges(circuit, window):
    """commit_records_device over the whole table against commit_device on the uploaded oracle bodies: the statuses are run_device's
    (0 / 4 / 103), the points of status-0 rows are equal, every other row gets the point at infinity; and the plain-integer group
    law (tests/ec_ref.py) for four rows at |k| = 2 047 and 2 048 with both signs — both sides of the tabulated-point branch."""
    import torch
    m = T.pkg()
    t = _table(circuit)
    n, acc = t["n"], t["acc"]
    ctx = _ctx(circuit)
    curve, first_slot = CURVE[circuit], 3
    gens = E.related_points(curve, ctx.witness_size - first_slot)
    key = m.CommitKey(ctx, curve, E.points_to_bytes(gens), first_slot, window)
    s = torch.cuda.current_stream().cuda_stream
    d_recs = torch.from_numpy(t["recs"].view(np.int32)).cuda()
    # run_device's statuses (default route)
    d_bodies = torch.full((n, ctx.body_bytes), FILL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.run_device(d_recs.data_ptr(), n, d_bodies.data_ptr(), 0, 0, d_st.data_ptr(), s)
    del d_bodies
    want = torch.full((len(acc), 64), 9, dtype=torch.uint8, device="cuda")
    cst = torch.full((len(acc),), -1, dtype=torch.int32, device="cuda")
    key.commit_device(t["d_oracle"].data_ptr(), len(acc), 0, want.data_ptr(), cst.data_ptr(), s)
    got = torch.full((n, 64), 7, dtype=torch.uint8, device="cuda")
    st2 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    pub2 = torch.full((n, ctx.public_words), PUB_FILL, dtype=torch.int32, device="cuda")
    key.commit_records_device(d_recs.data_ptr(), n, got.data_ptr(), st2.data_ptr(), pub2.data_ptr(), s)
    torch.cuda.synchronize()
    st = st2.cpu().numpy()
    wrong = [(t["names"][i], int(st[i])) for i in range(n) if st[i] != t["want_st"][i]]
    assert not wrong, wrong[:8]
    assert torch.equal(st2, d_st)
    ok_rows = np.flatnonzero(t["ok"])
    ok_pos = torch.tensor([t["pos"][int(i)] for i in ok_rows], device="cuda")
    d_ok = torch.from_numpy(ok_rows).cuda()
    assert int(cst[ok_pos].abs().sum().item()) == 0
    g, w = got[d_ok], want[ok_pos]
    if not torch.equal(g, w):
        j = int(torch.nonzero((g != w).any(dim=1))[0].item())
        pytest.fail(f"{circuit} window {window}: the commitment from the record of row {t['names'][int(ok_rows[j])]!r} differs from the commitment of its body")
    rest = torch.from_numpy(np.flatnonzero(~t["ok"])).cuda()
    assert rest.numel() == 0 or int(got[rest].abs().sum().item()) == 0
    pub = pub2.cpu().numpy().view(np.uint32)
    assert np.array_equal(pub[ok_rows], t["pub"][ok_rows])
    if circuit != "compression":
        pts = got.cpu().numpy()
        for prefix in ("e1=+2047/", "e1=-2048/", "eqs[0]=-2047/", "eqs[63]=+2048/"):
            i = next(i for i, nm in enumerate(t["names"]) if nm.startswith(prefix))
            assert t["ok"][i]
            b = t["host_bodies"][i].reshape(-1, 32)
            vals = [int.from_bytes(b[s_].tobytes(), "little") for s_ in range(first_slot, b.shape[0])]
            assert E.point_from_bytes(pts[i].tobytes()) == E.commit(vals, gens, curve), t["names"][i]
    key.close(); ctx.close()
