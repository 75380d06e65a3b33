"""The table of foreign bodies (tests/commit_domain_cases.py) against the rule in plain integers (tests/commit_domain_ref.py), without
a GPU: the hand-written verdicts are the rule's, every base body is in domain, the table reaches every class, word position and road
it is meant to, the two-multiplication reference of a commitment equals the plain multi-scalar sum, and a folded key's committed
vector of a witness gives the plain key's point."""
import importlib

import pytest

import b3w_testlib as T
import commit_domain_cases as C
import commit_domain_ref as R
import ec_ref as E

NAMES = [k[0] for k in C.KEYS]


@pytest.mark.parametrize("name", NAMES)
def test_hand_written_verdicts_are_the_rule(name):
    row, tab, t, tables = C.key_table(name)
    cls = tab["cls"]
    for i, v in enumerate(tab["values"]):
        assert R.in_domain(v, cls), tab["names"][i]
    wrong = []
    for k, case in enumerate(tab["cases"]):
        nm, bi, edits, verdict = case
        inside = all(R.slot_in_domain(v, cls[s]) for s, v in edits.items())          # (the base is in domain: only these slots decide)
        if k % 16 == 0:
            assert inside == R.in_domain(C.case_values(tab, case), cls), nm
        if (verdict == 103) != (not inside) or verdict not in (0, 103):
            wrong.append(nm)
    assert not wrong, wrong[:8]
    C._check_coverage(tab)
    n = len(tab["cases"])
    assert {n % 4, (n - 1) % 4, (n - 2) % 4} == {1, 2, 3}
    # the size the table is meant to have: about 250 cases under a whole compression key, 300 and more under a whole nova key; a
    # folded compression key has bit slots only, a key over the last slots few sweep slots
    whole = row[3] < 100
    floor = (180 if row[1] == "compression" else 350) if row[5] else (250 if row[1] == "compression" else 300) if whole else 120
    assert floor <= n <= 420, (n, floor)


def test_both_roads_and_both_lane_counts_occur():
    roads = set()
    for name in NAMES:
        row, tab, t, tables = C.key_table(name)
        for s in tab["sweep"].get("bit", []):
            roads.add((t, C.road(tab["cls"], tab["first_slot"], t, s)))
    assert roads == {(32, "fast"), (32, "slow"), (64, "fast"), (64, "slow")}
    kinds = set()
    for name in NAMES:
        kinds |= set(C.key_table(name)[1]["sweep"])
    assert kinds == {"bit", "w32", "w64", "w256", "inverse", "folded", "onebit"}


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_two_multiplications_equal_the_plain_sum(circuit):
    """(sum v) A + (sum i v) B against ec_ref.commit over the generators A + i B themselves: three cases per circuit, under a key over
    the last slots (seconds in Python), with inverse tables where the build has them"""
    curve = "pallas" if circuit == "nova_vesta" else "bn254_g1"
    fs = 22950 if circuit in ("nova_bn254", "nova_vesta") else 21000
    tab = C.table(circuit, fs, False, circuit in ("nova_bn254", "nova_vesta"), 64)
    gens = E.related_points(curve, len(tab["widths"]) - fs)
    sc = C.reference_scalars(tab)
    picks = [k for k, c in enumerate(tab["cases"]) if c[3] == 0 and any(s >= fs for s in c[2])]
    picks = [next(k for k, c in enumerate(tab["cases"]) if c[3] == 0), picks[0], picks[-1]]
    for k in picks:
        vals = C.case_values(tab, tab["cases"][k])
        assert sc[k] == R.scalars(vals, tab["cls"], tab["coeffs"])
        assert R.point(curve, *sc[k]) == E.commit(R.committed(vals, tab["cls"]), gens, curve), tab["cases"][k][0]


@pytest.mark.parametrize("circuit", ["compression", "nova_bn254_o1", "nova_vesta"])
def test_folded_committed_vector_gives_the_plain_keys_point(circuit):
    """For a witness the folded key's point is the plain key's: in the exponents for the whole key (first_slot 0), and with
    fold.fold_generators' own points for a key over the last slots."""
    fold = importlib.import_module("hot-proofs-blake3-circom_amd.fold")
    b = C.bases(circuit)
    widths, p = b["widths"], T.PRIME[circuit]
    coeffs, mask = R.folded_coefficients(circuit, widths, 0)
    cls = R.classes(widths, 0, mask)
    assert sum(1 for m in mask if m) >= 400
    for i in (0, 1):
        a, bb = R.scalars(b["values"][i], cls, coeffs)
        assert a % p == sum(b["values"][i]) % p and bb % p == sum(s * v for s, v in enumerate(b["values"][i])) % p
    fs = {"compression": 22000, "nova_bn254_o1": 22400, "nova_vesta": 22000}[circuit]
    curve = "pallas" if circuit == "nova_vesta" else "bn254_g1"
    q, _ = E.CURVES[curve]
    gens = E.related_points(curve, len(widths) - fs)
    buf, fmask, stats = fold.fold_generators(R.r1cs_image(circuit), widths, fs, E.points_to_bytes(gens), curve)
    coeffs, mask = R.folded_coefficients(circuit, widths, fs)
    assert bytes(fmask) == bytes(mask) and any(mask)
    cls = R.classes(widths, fs, mask)
    for k in [k for k, m in enumerate(mask) if m != 1][::97] + [k for k, m in enumerate(mask) if m & 0x80][:3]:
        assert E.point_from_bytes(buf[64 * k:64 * k + 64]) == R.point(curve, *coeffs[k]), k       # the restated folding, slot by slot
    fg = [E.point_from_bytes(buf[64 * k:64 * k + 64]) for k in range(len(mask))]
    for i in (0, 1):
        vals = b["values"][i]
        assert E.commit(R.committed(vals, cls), fg, curve) == E.commit(vals[fs:], gens, curve)


def test_count_of_additions_follows_the_tabulated_inverses():
    """expected_additions on the edge body (eqs[i] = 2 049 - i): every gadget with |k| <= 2 047 costs one addition and none of its
    windows; the same body under a key without tables costs its windows."""
    row, tab, t, tables = C.key_table("nova_vesta-w12")
    assert tables
    edge = tab["names"].index("edge2049")
    vals = tab["values"][edge]
    got = R.tabulated_gadgets(vals, tab["cls"], tab["input_slots"], tab["p"])
    ks = R.gadget_args([vals[s] for s in tab["input_slots"]])
    assert ks[3:6] == [2049, 2048, 2047] and sorted(got) == [j for j, k in enumerate(ks) if 0 < abs(k) <= 2047] and len(got) == 65
    plain = R.classes(tab["widths"], 0)
    with_t = R.expected_additions(vals, tab["cls"], 12, R.INV_NK, tab["input_slots"], tab["p"])
    without = R.expected_additions(vals, plain, 12)
    assert with_t < without and R.expected_additions(vals, tab["cls"], 12) == without
    total, per = C.reference_additions(tab, 12)
    k = next(k for k, c in enumerate(tab["cases"]) if c[1] == edge and not c[2])
    assert per[k] == with_t
