"""bench.py --dump-outputs on a box without a GPU: the helpers that choose and write what the timed path computed — float64 files
that hold every u32 word exactly, a fixed seeded sample of the rows of a large output, the 64 MB bound on all files together."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_outputs_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sample_rows_is_fixed_sorted_and_complete_for_small_outputs():
    b = _bench()
    a, c = b.sample_rows(4096, 16), b.sample_rows(4096, 16)
    assert np.array_equal(a, c) and len(a) == 16 and (np.diff(a) > 0).all() and 0 <= a[0] and a[-1] < 4096
    assert np.array_equal(b.sample_rows(10, 16), np.arange(10))


def test_written_files_hold_every_u32_word(tmp_path):
    b = _bench()
    words = np.array([[0, 1, 0xFFFFFFFF, 0x80000001]], dtype=np.uint32)
    bodies = words.view(np.uint8)                                     # uint8 rows are read as little-endian u32 words
    b.write_outputs(str(tmp_path), {"w": b.u32_words(words.view(np.int32)), "b": b.u32_words(bodies), "none": None})
    assert sorted(os.listdir(tmp_path)) == ["b.npy", "w.npy"]
    for name in ("w", "b"):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64 and np.array_equal(got.astype(np.uint32), words), name


def test_large_outputs_are_sampled_and_the_total_is_bounded(tmp_path):
    b = _bench()
    a = np.arange(100000 * 8, dtype=np.float64).reshape(100000, 8)
    part = b.rows_within("h", a, 1 << 20)
    assert set(part) == {"h", "h_rows"} and part["h"].nbytes <= 1 << 20
    assert np.array_equal(part["h"], a[part["h_rows"]]) and np.array_equal(part["h_rows"], b.rows_within("h", a, 1 << 20)["h_rows"])
    assert set(b.rows_within("h", a[:100], 1 << 20)) == {"h"}
    with pytest.raises(SystemExit):
        b.write_outputs(str(tmp_path / "big"), {"x": np.zeros((b.DUMP_LIMIT // 8) + 1)})
    assert not os.path.exists(tmp_path / "big")
