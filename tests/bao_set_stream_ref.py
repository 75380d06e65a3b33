"""The cuts of a set slice taken in windows, restated from bao_set_ref.encode's emission order and not from the C code.  Test
infrastructure.

  Every element of the slice (a parent node or a chunk) has c0, the least wanted chunk under it; the slice is pre-order, so c0 never
  falls along it.  A ROW is a block of B aligned chunks with a wanted chunk in it: B = 64 where the set's first and last wanted chunks
  lie in the same or in adjacent blocks of 64, else 1 024.  cut[r] is the offset of the first element whose c0 lies in row r's block;
  cut[0] = 0 (the header rides with row 0) and cut[n_rows] is the slice's size.  The greedy plan fills a window with as many whole
  rows as fit max_window_bytes."""
import bisect

import bao_set_ref as RS
from bao_ref import CHUNK, _split, num_chunks

MIN_WINDOW = 8 + 64 * (24 + 1023) + 1048576


def elements(length, runs, places=None):
    """-> [(offset, bytes, c0)] of every element behind the header, in the slice's order: encode's walk without the hashing
    (places, a dict: filled as encode fills its own)"""
    n = num_chunks(length)
    wanted = RS.chunks_of(runs)
    out = []
    at = [8]
    places = {} if places is None else places

    def first_wanted(lo, hi):
        return wanted[bisect.bisect_left(wanted, lo)]

    def walk(lo, m):
        if m == 1:
            size = min(length, (lo + 1) * CHUNK) - lo * CHUNK
            places[("chunk", lo)] = at[0]
            out.append((at[0], size, lo))
            at[0] += size
            return
        s = _split(m)
        places[("node", lo, m)] = at[0]
        out.append((at[0], 64, first_wanted(lo, lo + m)))
        at[0] += 64
        if RS._meets(wanted, lo, lo + s):
            walk(lo, s)
        if RS._meets(wanted, lo + s, lo + m):
            walk(lo + s, m - s)
    walk(0, n)
    return out, at[0]


def places(length, runs):
    """-> bao_set_ref.encode's places, without its hashing"""
    out = {}
    elements(length, runs, out)
    return out


def block_size(runs):
    wanted_first, wanted_last = runs[0][0], runs[-1][0] + runs[-1][1] - 1
    return 64 if wanted_last // 64 - wanted_first // 64 <= 1 else 1024


def row_cuts(length, runs):
    """-> (cut[0 .. n_rows], B): the rows' cuts and the rows' kind"""
    els, size = elements(length, runs)
    B = block_size(runs)
    assert all(a[2] <= b[2] for a, b in zip(els, els[1:]))              # c0 never falls along the slice
    assert all(a[0] + a[1] == b[0] for a, b in zip(els, els[1:])) and els[-1][0] + els[-1][1] == size and els[0][0] == 8
    cuts, last = [], None
    for off, _, c0 in els:
        if c0 // B != last:
            last = c0 // B
            cuts.append(off if cuts else 0)
    return cuts + [size], B


def greedy(cuts, max_window_bytes):
    """-> the window boundaries (a sub-list of cuts from 0 to the size): each window takes whole rows while they fit"""
    assert max_window_bytes >= MIN_WINDOW
    out, i = [cuts[0]], 0
    while i < len(cuts) - 1:
        j = i + 1
        while j < len(cuts) - 1 and cuts[j + 1] - cuts[i] <= max_window_bytes:
            j += 1
        out.append(cuts[j])
        i = j
    return out


def every(cuts, k):
    """-> the boundaries of windows of k rows each (the last one what is left)"""
    return cuts[:-1:k] + [cuts[-1]]
