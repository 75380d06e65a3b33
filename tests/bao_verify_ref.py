"""Bao's decoder applied to every unit of a file at once, restated in plain Python on blake3_ref / bao_ref / bao_groups_ref from
the bao specification.  Test infrastructure.

  unit            a chunk (g = 0, full outboards) or a group of 2^g chunks (group outboards); max(1, ceil(n_chunks / 2^g)) of them
  status of a unit, the first rule that applies:
    3  the outboard's 8-byte header is not the file's length (every unit of the file)
    2  a stored node on the unit's path fails: the root node hashed with PARENT | ROOT is not the root, or a lower node hashed
       with PARENT is not its half of the stored node above it
    1  the unit's CV, computed from the file's bytes (the levels inside a group recomputed), is not its half of the lowest stored
       node on its path (a file of one unit: its ROOT-flagged CV is not the root)
    0  otherwise

One top-down walk of the stored tree: a node is judged by its own stored bytes against the stored half above it, never by anything
recomputed from the file's bytes, so a bad chunk marks its own unit alone and a bad node exactly the units below it."""
import struct

import bao_groups_ref as GR
import bao_ref as R
import blake3_ref as B


def num_units(length, g):
    return GR.num_groups(R.num_chunks(length), g)


def layout(lens, g):
    """-> unit_first [n_files + 1]: file f's statuses are entries [unit_first[f], unit_first[f + 1]) of the packed array"""
    out = [0]
    for length in lens:
        out.append(out[-1] + num_units(int(length), g))
    return out


def scratch_items(lens):
    """what the device call keeps per file in the caller's scratch: an entry per tile of 1 024 chunks of the files of more than one
    tile, plus one per 1 024 tiles of the files of more than 1 024 tiles"""
    items = 0
    for length in lens:
        tiles = (R.num_chunks(int(length)) + 1023) // 1024
        groups = (tiles + 1023) // 1024
        items += (tiles if tiles > 1 else 0) + (groups if groups > 1 else 0)
    return items


def _unit_cv(data, length, unit, g, root):
    n, G = R.num_chunks(length), 1 << g
    first = unit * G
    gn = min(G, n - first)
    cvs = GR._group_cvs(data[first * R.CHUNK:(first + gn) * R.CHUNK], length, first, gn, root and gn == 1)
    return list(GR._chunks_tree(cvs, 0, gn, root))


def verify(data, ob, root_words, length, g=0):
    """-> the status of every unit of a file of `length` bytes (`data`) held against the outboard `ob` (group_log g) and the root"""
    data, ob = bytes(data), bytes(ob)
    nu = num_units(length, g)
    assert len(data) == length and len(ob) == 8 + 64 * (nu - 1)
    if struct.unpack("<Q", ob[:8])[0] != length:
        return [3] * nu
    out = [None] * nu

    def walk(first, m, pos, want, bad, root):
        if m == 1:
            out[first] = 2 if bad else (1 if _unit_cv(data, length, first, g, root) != want else 0)
            return
        words = list(struct.unpack("<16I", ob[8 + 64 * pos:8 + 64 * pos + 64]))
        if B.compress(B.IV, words, 0, 64, B.PARENT | (B.ROOT if root else 0))[:8] != want:
            bad = True
        k = R._split(m)
        walk(first, k, pos + 1, words[:8], bad, False)
        walk(first + k, m - k, pos + k, words[8:], bad, False)
    walk(0, nu, 0, list(root_words), False, True)
    return out


def summary(status):
    """-> (file status: the largest unit status, first bad: the lowest unit with a non-zero status or 2^64 - 1)"""
    bad = [i for i, s in enumerate(status) if s]
    return max(status), bad[0] if bad else (1 << 64) - 1
