"""The plans of tests/r1cs_cases.py proved on the CPU before tests/test_gpu_r1cs_rows.py trusts them: that the single-wire cases reach
EVERY row of every committed system on the road they claim, and that the edge systems hold every class of threshold value once satisfied
and once violated.  The valid body is body 1 of the oracle's witnesses for workloads.config2_compression(4, first=50) /
config3_nova(4, first=50) — the same body the GPU test uploads.  No GPU."""
import collections
import os
import random
import shutil
import subprocess

import pytest

import b3w_testlib as T
import r1cs_cases as C
import r1cs_ref as R

CSRC = os.path.join(T.PKG_DIR, "csrc")

# rows that are not booleanity rows, reached as the FIRST violated row by an on or top-up case (body 1; measured with plain integers)
FIRSTS = {"compression": 8640, "nova_bn254": 3951, "nova_vesta": 3951, "nova_bn254_o1": 8889}
# the only rows no on case can reach:  1 * () = ()  (A = {wire 0: 1}, B and C empty) — row 19 of the O2 nova systems
EXCEPTIONS = {"compression": [], "nova_bn254": [19], "nova_vesta": [19], "nova_bn254_o1": []}
EDGE = {"bn254": (T.BN254_R, T.NWIT["compression"]), "vesta": (T.VESTA_Q, T.NWIT["nova_vesta"])}


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_the_row_plan_reaches_every_row_on_its_road(circuit):
    sys_, z = C.committed(circuit)
    p = sys_["prime"]
    assert R.violated(sys_, z) == []
    plan = C.row_plan(sys_, z)
    by_wire = R.rows_of_wire(sys_)
    brow = C.bool_rows(sys_)
    rows = {"on": set(), "off": set(), "top-up": set()}
    firsts, wild0 = set(), None
    zz = list(z)
    checked = []
    for w, new, road in plan:
        zz[w] = new
        v = C.changed_violated(sys_, zz, w, by_wire)
        checked.append((w, new, v))
        zz[w] = z[w]
        assert v, ("a case that violates nothing", w, new, road)
        rows[road].update(v)
        if road != "off":
            assert new < 1 << 63 and not any(k in brow for k in v), (w, new, road)
            if v[0] not in brow:
                firsts.add(v[0])
        if (w, new) == (0, p + 1):
            wild0 = set(v)
    nonbool = [k for k in range(len(sys_["constraints"])) if k not in brow]
    missing = [k for k in nonbool if k not in rows["on"]]
    assert missing == EXCEPTIONS[circuit]
    for k in missing:
        a, b, c = sys_["constraints"][k]
        assert a == {0: 1} and not b and not c and k in wild0
    assert all(k in rows["off"] for k in brow)
    assert {w for w, _, _ in plan} == set(range(sys_["n_wires"]))
    print(circuit, "cases", collections.Counter(r for _, _, r in plan), "non-booleanity rows", len(nonbool), "as first", len(firsts))
    assert len(firsts) == FIRSTS[circuit]
    # changed_violated against the whole-body evaluator: 300 cases over the rows of the wire, 10 over every row of the system
    rng = random.Random(3)
    for i, (w, new, v) in enumerate(rng.sample(checked, 300) + [c for c in checked if c[0] == 0]):
        zz[w] = new
        assert R.violated(sys_, zz, by_wire[w] if i >= 10 else None) == v, (w, new)
        zz[w] = z[w]


@pytest.mark.parametrize("prime", sorted(EDGE))
def test_the_edge_bodies_hold_every_class_both_ways(prime):
    p, nw = EDGE[prime]
    E = C.edge_system(p, nw)
    bodies = C.edge_bodies(E)
    want = C.edge_expect(E, bodies)
    assert 300 <= len(bodies) <= 500
    cls = collections.defaultdict(lambda: [0, 0])
    for b, (count, first) in zip(bodies, want):
        cls[b["cls"]][count > 0] += 1
        assert (count == 0) == (first == C.NONE)
    wild = {"element p", "element p+1", "element 2^256-1"}          # no canonical representative: violated whatever the row says
    for name, (ok, bad) in cls.items():
        assert bad > 0 and (ok > 0 or name in wild), (name, ok, bad)
    names = set(cls)
    assert {f"element {n}" for n, _ in C.edge_elements(p)} <= names and {f"coefficient {n}" for n, _ in C.edge_coefs(p)} <= names
    assert {"term product", "sum of 64 terms", "sum of 65 terms", "sum of 300 terms", "cancelling sum", "part at the edge of 64 bits", "wide record wa", "wide record wb_n",
            "wide record wc", "wide record wk2", "wide record wa_exp", "wide record two terms", "wide record large d", "230 wide rows", "split tile", "careful t0", "careful tm",
            "careful tl", "careful wire 0", "bit run"} <= names
    # the 230-row body with violations on both sides of the 224th record: count and first are pinned by value
    many = [w for b, w in zip(bodies, want) if b["cls"] == "230 wide rows"]
    r0 = E["rows"]["many0"]
    for b in bodies:                                                # every one of the 230 rows holds a wide element: more than WIDE_CAP records
        if b["cls"] == "230 wide rows":
            assert sum(1 for i in range(230) if b["set"][E["g"][f"many{i}"]["W"]] >= 1 << 64) == 230 > C.WIDE_CAP
    assert many == [(0, C.NONE), (6, r0 + 5), (1, r0 + 224), (1, r0 + 229), (230, r0)]
    # shape of the system: rows in five tiles, a row whose operands all come from an earlier tile, a tile of more than SPLIT_GEN general rows
    home = collections.Counter(max(w for lc in row for w in lc) // C.TILE for row in E["constraints"])
    assert len(home) >= 5
    a, b, c = E["constraints"][E["rows"]["mul_allexp"]]
    assert max(list(a) + list(b)) // C.TILE < min(c) // C.TILE
    general = [k for k, row in enumerate(E["constraints"]) if max(w for lc in row for w in lc) // C.TILE == E["tiles"]["ts"] and k not in C.bool_rows(E)]
    assert len(general) > C.SPLIT_GEN
    # every body is zero but for its own wires, and wire 0 = 1 alone satisfies the system
    assert C.edge_expect(E, [dict(cls="", set={})]) == [(0, C.NONE)]
    img = C.edge_image(E)
    back = R.parse(img)
    assert back["constraints"] == E["constraints"] and back["n_wires"] == nw and back["prime"] == p


def test_the_host_program_takes_the_edge_systems_on_the_walk_road(tmp_path):
    """b3w_r1cs_host.cpp over the edge images (tests/r1cs_host_harness.cpp checks every index of the programs it builds): tiled, a walk
    program, and one unit more than tiles — the tile of 356 general rows is split."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "harness"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(T.ROOT, "tests", "r1cs_host_harness.cpp"), os.path.join(CSRC, "b3w_r1cs_host.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for prime, (p, nw) in EDGE.items():
        img = tmp_path / (prime + ".r1cs")
        img.write_bytes(C.edge_image(C.edge_system(p, nw)))
        r = subprocess.run([str(exe), str(img), str(nw), "0", "7"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        ntiles = (nw + C.TILE - 1) // C.TILE
        assert "tiled 1" in r.stdout and f"walk 1: {ntiles + 1} units over {ntiles} tiles" in r.stdout, r.stdout


def test_the_thresholds_the_cases_quote_are_the_sources():
    """The edge values of tests/r1cs_cases.py are written next to the comparisons they test; if a comparison moves, this test says so."""
    src = {n: open(os.path.join(CSRC, n)).read() for n in ("b3w_r1cs_walk.hip", "b3w_r1cs_host.cpp", "b3w_r1cs_defs.h", "b3w_r1cs_device.h")}
    for name, text in (("b3w_r1cs_host.cpp", "if (!hi && lo64 < (1ull << 62))"), ("b3w_r1cs_host.cpp", "if (!hi && n64 < (1ull << 62))"),
                       ("b3w_r1cs_host.cpp", "return not_small || nw > 256 ? 2 : 0;"),
                       ("b3w_r1cs_walk.hip", "k != 0ull && k <= (1ull << 62)"), ("b3w_r1cs_walk.hip", "(lo.y & 0x80000000u)"),
                       ("b3w_r1cs_walk.hip", "small && !(z >> 63) && hi < (1ull << 39)"), ("b3w_r1cs_walk.hip", "hi == 0ull && lo < (1ull << 54)"),
                       ("b3w_r1cs_walk.hip", "a_hi != ((long long)a_lo >> 63) || b_hi != ((long long)b_lo >> 63)"),
                       ("b3w_r1cs_walk.hip", "a_lo * b_lo != c_lo || __mul64hi((long long)a_lo, (long long)b_lo) != c_hi"),
                       ("b3w_r1cs_walk.hip", "c_hi < -(1ll << 61) || c_hi >= (1ll << 61)"), ("b3w_r1cs_walk.hip", "if (slot < B3W_WALK_WIDE_CAP)"),
                       ("b3w_r1cs_walk.hip", "else if (kmag >> 32) bad = gather_row("), ("b3w_r1cs_device.h", "lo = s_lo + (s_hi << 52);"),
                       ("b3w_r1cs_defs.h", "#define B3W_WALK_WIDE_CAP 224u"), ("b3w_r1cs_defs.h", "#define B3W_WALK_SPLIT_GEN 320u"),
                       ("b3w_r1cs_defs.h", "#define B3W_R1CS_TILE 1024u")):
        assert text in src[name], (name, text)
    assert (C.TILE, C.SPLIT_GEN, C.WIDE_CAP) == (1024, 320, 224)
