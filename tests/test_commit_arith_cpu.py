"""The commit kernels' field and group arithmetic (csrc/b3w_commit_arith.h) compiled for the host, under AddressSanitizer + UBSan,
at the operands where carries and lazy bounds can go wrong: tests/commit_arith_cases.py makes the rows and judges the raw results
against Python integers; tests/commit_arith_harness.cpp, a program of its own, applies the header's routines.  No GPU, no HIP,
nothing loaded into this process."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import commit_arith_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hot-proofs-blake3-circom_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("commit_arith") / "harness"
    cmd = ["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           os.path.join(ROOT, "tests", "commit_arith_harness.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def run_harness(harness, tmp_path, field, rows):
    src, dst = tmp_path / "rows.bin", tmp_path / "results.bin"
    with open(src, "wb") as f:
        f.write(np.array([field, len(rows)], dtype=np.uint32).tobytes())
        f.write(rows.tobytes())
    r = subprocess.run([harness, str(src), str(dst)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return np.fromfile(dst, dtype=np.uint32).reshape(len(rows), A.OUT_WORDS)


@pytest.mark.parametrize("field", sorted(A.FIELDS), ids=[A.FIELD_NAMES[f] for f in sorted(A.FIELDS)])
def test_arithmetic_keeps_its_promises_on_the_host(harness, tmp_path, field):
    T = A.table(field)
    print(f"{A.FIELD_NAMES[field]}: {len(T.rows)} rows")
    bad = A.check(T, run_harness(harness, tmp_path, field, T.packed()))
    assert not bad, "\n".join(bad)


def test_the_table_is_what_it_claims():
    """deterministic, every routine present for every instantiation that reaches it, within its size"""
    for field in A.FIELDS:
        T = A.table(field)
        ops = {A.OP_NAME[r[0]] for r in T.rows}
        nine = {n for n, c in A.OP.items() if c >= 20}
        assert nine <= ops and (field == 2 or ops == set(A.OP)), sorted(set(A.OP) - ops)
        assert 10_000 < len(T.rows) < 60_000
        for name, most in (("INV29", 48), ("FP_INV", 48)):
            assert sum(1 for r in T.rows if A.OP_NAME[r[0]] == name) <= most
    first = A.table(2).packed()
    A.table.cache_clear()
    assert np.array_equal(A.table(2).packed(), first)
