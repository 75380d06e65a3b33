"""What the tests of the resize calls (tests/test_bao_resize_cpu.py, tests/test_gpu_bao_resize.py) share: the transitions, the bytes of
a file at any length, and the host yardstick.  Test infrastructure.

  a file at length L = the first L bytes of one fixed stream, so the first min(old, new) bytes of a file are what they were
  yardstick          = a host path the resize calls do not touch: the whole outboard from bao.update_host with every chunk dirty over a
                       zeroed outboard whose header is set (b3w_bao_outboard_update's walk over host_subtree_cv); below 41 chunks the
                       plain-Python bao_groups_ref.group_outboard itself"""
import struct

import numpy as np

import b3w_testlib as T
import bao_groups_ref as GR
import bao_ref as R

K, M = 1024, 1 << 20
GS = (0, 1, 4, 6)
TRANSITIONS = [(0, 1), (1, 0), (0, 0), (K, K + 1), (64 * K, 65 * K), (65 * K, 64 * K), (M - 300, M), (M, M + 1), (M + 1, M),
               (2 * M - 300, 2 * M + 5 * K), (3 * M + 5 * K - 7, 5 * M + 1), (5 * M, 8 * M), (8 * M, 9 * M + 3 * K), (9 * M + 3 * K, 4 * M),
               (4 * M, 3 * M - 1), (3 * M + 17, 3 * M + 17)]
CHAIN = [3 * M + 5, 5 * M + 1, 8 * M, 9 * M + 3 * K, 4 * M, 3 * M - 1]       # the lengths a file runs through, over and over
_STREAM = None
_YARD = {}


def stream():
    """the fixed bytes, as a numpy uint8 array as long as the longest file of the transitions"""
    global _STREAM
    if _STREAM is None:
        _STREAM = np.random.default_rng(18).integers(0, 256, 9 * M + 3 * K, dtype=np.uint8)
    return _STREAM


def data(length):
    return stream()[:length].tobytes()


def all_dirty(file_bytes, g):
    """the yardstick's host path -> (outboard bytes, root words)"""
    m = T.pkg()
    n = R.num_chunks(len(file_bytes))
    zeroed = struct.pack("<Q", len(file_bytes)) + bytes(GR.group_outboard_size(len(file_bytes), g) - 8)
    ob, root = m.bao.update_host(file_bytes, zeroed, [0] * 8, [0], [n], g)
    return ob, [int(x) for x in root]


def yardstick(length, g):
    """-> (outboard bytes, root words) of the file at `length`"""
    if (length, g) not in _YARD:
        d = data(length)
        _YARD[(length, g)] = GR.group_outboard(d, g) if R.num_chunks(length) < 41 else all_dirty(d, g)
    return _YARD[(length, g)]


def kept_tiles(old_len, new_len):
    return min(old_len, new_len) // M


def tiles(length):
    return (R.num_chunks(length) + 1023) // 1024


def scratch_slots(new_len):
    """32-byte scratch slots of a listed file: a slot a tile for a file of more than one, one per 1 024 tiles more past 1 GiB"""
    t = tiles(new_len)
    return 0 if t <= 1 else t + ((t + 1023) // 1024 if t > 1024 else 0)
