"""The arrival bitmap restated in plain Python / numpy (include/b3wit.h "the arrival bitmap"): the bit layout, the collapse of chunks
into units with a ragged last unit, maximal runs, counts, and the bitmap made from unit statuses.  Nothing here calls the library.

Layout: file f owns ceil(n_chunks / 64) words of 64 bits from word word_first[f]; chunk c is bit c & 63 of word word_first[f] + (c >> 6);
the bits at and above the chunk count in the last word are pad bits and count for nothing."""
import numpy as np

MISSING, PRESENT = 0, 1
KINDS = {"missing": MISSING, "present": PRESENT}


def num_chunks(length):
    return max(1, (length + 1023) // 1024)


def words(n_chunks):
    return (n_chunks + 63) // 64


def layout(lens):
    """-> word_first, a list of n_files + 1 entries"""
    out = [0]
    for ln in lens:
        out.append(out[-1] + words(num_chunks(ln)))
    return out


def pack(bits, pad=False):
    """a bool array, one entry per chunk -> the file's words (numpy uint64); pad: the pad bits set (what a careless caller may leave)"""
    bits = np.asarray(bits, dtype=bool)
    full = np.full(words(bits.size) * 64, bool(pad))
    full[:bits.size] = bits
    return np.packbits(full, bitorder="little").view(np.uint64).copy()


def unpack(have, n_chunks):
    """the file's words -> a bool array of its n_chunks chunks (the pad bits dropped)"""
    have = np.ascontiguousarray(have, dtype=np.uint64)
    assert have.size == words(n_chunks)
    return np.unpackbits(have.view(np.uint8), bitorder="little")[:n_chunks].astype(bool)


def units_full(bits, g):
    """-> per unit of 2^g chunks: every chunk the unit HAS is set (the ragged last unit is judged by its existing chunks)"""
    bits = np.asarray(bits, dtype=bool)
    F = 1 << g
    n_units = (bits.size + F - 1) // F
    padded = np.ones(n_units * F, dtype=bool)
    padded[:bits.size] = bits
    return padded.reshape(n_units, F).all(axis=1)


def runs(bits, g=0, kind=MISSING):
    """-> (rows: a list of (first chunk, number of chunks), ascending; n_have: the set chunks).  A run is a maximal stretch of selected
    units — PRESENT: every chunk set, MISSING: at least one clear — covering whole units, clipped to the chunk count."""
    bits = np.asarray(bits, dtype=bool)
    full = units_full(bits, g)
    sel = full if kind == PRESENT else ~full
    edge = np.diff(np.concatenate(([False], sel, [False])).astype(np.int8))
    first, stop = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]
    rows = [(int(a) << g, min(int(b) << g, bits.size) - (int(a) << g)) for a, b in zip(first, stop)]
    return rows, int(bits.sum())


def runs_slow(bits, g=0, kind=MISSING):
    """runs() unit by unit, without numpy: the definition read aloud (small cases)"""
    bits = [bool(b) for b in bits]
    n, F = len(bits), 1 << g
    rows, open_at = [], None
    for u in range((n + F - 1) // F):
        mine = bits[u * F:min((u + 1) * F, n)]
        sel = all(mine) if kind == PRESENT else not all(mine)
        if sel and open_at is None:
            open_at = u * F
        if not sel and open_at is not None:
            rows.append((open_at, u * F - open_at))
            open_at = None
    if open_at is not None:
        rows.append((open_at, n - open_at))
    return rows, sum(bits)


def batch_runs(haves, n_chunks, g=0, kind=MISSING):
    """a batch: haves[f] the words of file f -> (files, first_chunks, counts: numpy; file_have: list), rows ascending by (file, first)"""
    files, first, count, file_have = [], [], [], []
    for f, (hv, n) in enumerate(zip(haves, n_chunks)):
        rows, got = runs(unpack(hv, n), g, kind)
        files += [f] * len(rows)
        first += [r[0] for r in rows]
        count += [r[1] for r in rows]
        file_have.append(got)
    return np.array(files, dtype=np.uint32), np.array(first, dtype=np.uint64), np.array(count, dtype=np.uint64), file_have


def from_status(status, n_chunks, g=0):
    """unit statuses (one byte per unit of 2^g chunks) -> the file's words: chunk c is set where status[c >> g] == 0, pad bits zero"""
    status = np.asarray(status, dtype=np.uint8)
    assert status.size == (n_chunks + (1 << g) - 1) >> g
    return pack(np.repeat(status == 0, 1 << g)[:n_chunks])


def collapse(bits, g):
    """the chunks whose whole unit is set: what a bitmap at chunk granularity looks like through units of 2^g chunks"""
    bits = np.asarray(bits, dtype=bool)
    return np.repeat(units_full(bits, g), 1 << g)[:bits.size]
