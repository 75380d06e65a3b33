"""The on-device constraint check (csrc/b3w_r1cs_walk.hip, b3w_r1cs.hip, b3w_r1cs_device.h) row by row and at the thresholds of its 64-bit
fast road.  tests/test_gpu_r1cs.py samples; here EVERY row of every committed system is violated at least once — the non-booleanity rows
while the body stays on the walk kernel's fast road (truth-table runs, two-counter sums, export area, the units of a split tile), the
booleanity rows on the road to the deferred kernel — and count and first violated row of every case are compared with plain integers.
The edge systems put elements, coefficients, term products, part sums and wide records on both sides of every comparison the fast road
makes.  Plans and expected verdicts: tests/r1cs_cases.py, proved on the CPU by tests/test_r1cs_cases_cpu.py.  The valid bodies are the
ORACLE's (built on the machine), uploaded; nothing here runs the witness kernels."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import b3w_testlib as T
import r1cs_cases as C

pytestmark = pytest.mark.gpu

CASES_PY = os.path.join(T.ROOT, "tests", "r1cs_cases.py")
EDGE = {"bn254": ("compression", T.BN254_R), "vesta": ("nova_vesta", T.VESTA_Q)}

_plans = {}


def _plan(circuit):
    """(body as uint8, plan, expected) of a committed system, computed once"""
    if circuit not in _plans:
        sys_, z = C.committed(circuit)
        plan = C.row_plan(sys_, z)
        body = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in z), dtype=np.uint8)
        _plans[circuit] = (body, plan, C.plan_expect(sys_, z, plan))
    return _plans[circuit]


def _compare(plan, want, count, first, what):
    wc, wf = np.array([w[0] for w in want], dtype=np.uint32), np.array([w[1] for w in want], dtype=np.uint32)
    wrong = np.flatnonzero((count != wc) | (first != wf))
    for j in wrong[:5]:
        print(what, "(wire, new, road)", (plan[j][0], hex(plan[j][1]), plan[j][2]), "got", (int(count[j]), int(first[j])), "want", want[j])
    assert wrong.size == 0, (what, int(wrong.size), "of", len(plan), "cases differ; first (wire, new, got, want):",
                             [(plan[j][0], hex(plan[j][1]), (int(count[j]), int(first[j])), want[j]) for j in wrong[:5]])


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_every_row_on_the_fast_road(circuit):
    """Every case of row_plan — on, top-up and off: about 60 000 single-wire changes of one valid oracle body, which between them violate
    every row of the system — through check_device in slabs of at most 4 096 bodies on the default road, in this process.  count and first
    of EVERY case equal the plan's; every 64th body of every slab is left untouched and reports (0, 0xFFFFFFFF)."""
    body, plan, want = _plan(circuit)
    m = T.pkg()
    ctx = m.Context(circuit, 0)
    r1cs = m.R1cs(ctx)
    assert r1cs.tiled and r1cs.n_wires * 32 == body.size
    t0 = time.time()
    count, first, clean_wrong = C.run_plan(r1cs, body, [c[0] for c in plan], [c[1] for c in plan])
    print(circuit, len(plan), "cases on the device in %.2f s" % (time.time() - t0))
    assert clean_wrong == 0
    _compare(plan, want, count, first, circuit)
    r1cs.close(); ctx.close()


def _child(args, env):
    r = subprocess.run([sys.executable, CASES_PY] + args, capture_output=True, text=True, cwd=T.ROOT, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0, (env, r.stderr[-1500:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_row_plan_on_the_other_roads(tmp_path):
    """The on-road cases of compression and of the circomkit nova build through the stream kernel (B3W_R1CS_GATHER=4) and through the walk
    kernel's other instantiation (B3W_R1CS_SIGNED flipped against the circuit's default: compression 0, nova_bn254_o1 1) — one child
    process per road, one after the other: the same plain-integer count and first for every case."""
    for circuit, flipped in (("compression", "1"), ("nova_bn254_o1", "0")):
        body, plan, want = _plan(circuit)
        on = [j for j, c in enumerate(plan) if c[2] == "on"]
        sub, subwant = [plan[j] for j in on], [want[j] for j in on]
        path = str(tmp_path / (circuit + ".npz"))
        np.savez(path, body=body, wires=np.array([c[0] for c in sub], dtype=np.int64),
                 values=np.frombuffer(b"".join(c[1].to_bytes(32, "little") for c in sub), dtype=np.uint8))
        for env in ({"B3W_R1CS_GATHER": "4"}, {"B3W_R1CS_GATHER": "0", "B3W_R1CS_SIGNED": flipped}):
            got = _child(["plan", circuit, path], env)
            assert got["clean_wrong"] == 0, (circuit, env)
            _compare(sub, subwant, np.array(got["count"], dtype=np.uint32), np.array(got["first"], dtype=np.uint32), (circuit, env))


@pytest.mark.parametrize("prime", sorted(EDGE))
def test_edge_systems(prime, tmp_path):
    """The edge system over BN254 (in the compression context) and over Vesta (nova_vesta: the top limb 0x40000000 takes walk_pack's rare
    branch for other values) with its 420 bodies on every road: walk (both instantiations, one workgroup, seven workgroups, every term
    multiplying), stream and gather.  (count, first) of every body equal the plain-integer evaluation on every road."""
    circuit, p = EDGE[prime]
    E = C.edge_system(p, T.NWIT[circuit])
    bodies = C.edge_bodies(E)
    want = C.edge_expect(E, bodies)
    img = tmp_path / "edge.r1cs"
    img.write_bytes(C.edge_image(E))
    for env in ({"B3W_R1CS_GATHER": "0"}, {"B3W_R1CS_GATHER": "1"}, {"B3W_R1CS_GATHER": "4"}, {"B3W_R1CS_GATHER": "0", "B3W_R1CS_SIGNED": "0"},
                {"B3W_R1CS_GATHER": "0", "B3W_R1CS_SIGNED": "1"}, {"B3W_R1CS_GATHER": "0", "B3W_R1CS_GRID": "1"}, {"B3W_R1CS_GATHER": "0", "B3W_R1CS_GRID": "7"},
                {"B3W_R1CS_GATHER": "0", "B3W_WALK_SHIFT_TERMS": "0"}):
        got = _child(["edge", circuit, str(img), str(p)], env)
        assert got["tiled"], "the edge system must take the tile kernels"
        wrong = [(i, bodies[i]["cls"], (c, f), want[i]) for i, (c, f) in enumerate(zip(got["count"], got["first"])) if (c, f) != want[i]]
        for w in wrong[:8]:
            print(prime, env, "(body, class, got, want)", w)
        assert not wrong, (prime, env, len(wrong), "bodies differ; (body, class, got, want):", wrong[:5])
