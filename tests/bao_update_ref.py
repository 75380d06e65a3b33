"""Outboards updated in place after writes, restated in plain Python on bao_ref / bao_groups_ref.  Test infrastructure.

A stored node is left CV || right CV.  After some chunks of a file changed, a node needs rewriting only where a dirty UNIT (a chunk
at g = 0, a group of 2^g chunks otherwise) lies below it, and of such a node only the half over a dirty unit; the other half is the
CV of a clean subtree and is already there.  update() walks the tree over the units top down, skips every subtree without a dirty
unit (reads nothing of it, writes nothing of it), hashes the dirty units from the file's bytes and rebuilds the nodes above them
from the new halves and the stored clean ones.  The result must be what bao_groups_ref.group_outboard gives for the file as it is."""
import struct

import bao_groups_ref as GR
import bao_ref as R

CHUNK = R.CHUNK
TILE = 1024                                                            # chunks to a tile, tiles to a span


def merge_ranges(ranges, n):
    """chunk ranges (first, count) of a file of n chunks, in any order -> sorted disjoint [first, end) pairs; empty ones dropped"""
    out = []
    for first, end in sorted((int(a), min(n, int(a) + int(c))) for a, c in ranges if int(c) > 0 and int(a) < n):
        if out and first <= out[-1][1]:
            out[-1][1] = max(out[-1][1], end)
        else:
            out.append([first, end])
    return [tuple(x) for x in out]


def dirty_units(ranges, n, g):
    """the units of a file of n chunks that hold a chunk of one of the ranges"""
    return sorted({c >> g for first, end in merge_ranges(ranges, n) for c in range(first, end)})


def dirty_nodes(n_units, units):
    """indices of the stored nodes (pre-order, over n_units units) with one of `units` below them"""
    have = set(units)
    return [i for i, (first, m) in enumerate(GR.node_spans(n_units)) if any(u in have for u in range(first, first + m))]


def _unit_cv(data, n, g, unit, root):
    first = unit << g
    gn = min(1 << g, n - first)
    cvs = GR._group_cvs(data[first * CHUNK:(first + gn) * CHUNK], len(data), first, gn, root and gn == 1)
    return GR._chunks_tree(cvs, 0, gn, root)


def update(data, ob, root, ranges, g):
    """data: the file as it is NOW; ob, root: its group outboard of g (g = 0: the full outboard) and root words from BEFORE the
    writes; ranges: (first chunk, count) pairs that cover every changed chunk.  -> (outboard bytes, root words)"""
    data = bytes(data)
    n = R.num_chunks(len(data))
    nu = GR.num_groups(n, g)
    dirty = set(dirty_units(ranges, n, g))
    nodes = bytearray(ob[8:])
    assert len(nodes) == 64 * (nu - 1)

    def walk(first, m, pos, is_root):
        """the CV of the subtree over units [first, first + m) whose node (m > 1) is node `pos`, or None where it has no dirty unit"""
        if not any(u in dirty for u in range(first, first + m)):
            return None
        if m == 1:
            return list(_unit_cv(data, n, g, first, is_root))
        k = R._split(m)
        left = walk(first, k, pos + 1, False)
        right = walk(first + k, m - k, pos + k, False)
        at = 64 * pos
        if left is not None:
            nodes[at:at + 32] = R._cv_bytes(left)
        if right is not None:
            nodes[at + 32:at + 64] = R._cv_bytes(right)
        words = list(struct.unpack("<16I", bytes(nodes[at:at + 64])))
        return GR._parent(words[:8], words[8:], is_root)
    top = walk(0, nu, 0, True)
    return bytes(ob[:8]) + bytes(nodes), (list(root) if top is None else list(top))


def poison(ob, n_units, units, value=0xEE):
    """the outboard with every stored node that has none of `units` below it overwritten with `value` -> (bytes, the nodes left)"""
    keep = set(dirty_nodes(n_units, units))
    out = bytearray(ob)
    for i in range(n_units - 1):
        if i not in keep:
            out[8 + 64 * i:8 + 64 * i + 64] = bytes([value]) * 64
    return bytes(out), keep


def scratch_items(lens, files, firsts, counts):
    """32-byte scratch entries of an update over these ranges: a dirty tile of a file of more than one tile, and a dirty span of
    1 024 tiles of a file of more than 1 024 tiles, each once"""
    tiles, spans = set(), set()
    for f, a, c in zip(files, firsts, counts):
        n = R.num_chunks(int(lens[f]))
        n_tiles = -(-n // TILE)
        if n <= 64 or n_tiles <= 1:
            continue
        for first, end in merge_ranges([(a, c)], n):
            for t in range(first // TILE, (end - 1) // TILE + 1):
                tiles.add((f, t))
                if n_tiles > TILE:
                    spans.add((f, t // TILE))
    return len(tiles) + len(spans)
