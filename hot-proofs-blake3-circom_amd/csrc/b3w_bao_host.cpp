// b3w_bao_host.cpp — the bao calls of include/b3wit.h that never touch a device: the sizes and layouts, and the host mirrors that
// extract, decode and take in slices (UNTRUSTED input), verify, update and resize one file node by node.  Plain C++, no kernel and no
// HIP runtime call: tools/bao_range_host_check.cpp, bao_set_host_check.cpp, bao_have_host_check.cpp, bao_packed_host_check.cpp, bao_diff_host_check.cpp and bao_delta_host_check.cpp compile this file
// alone with AddressSanitizer + UBSan.  The formats are described where the kernels are (b3w_bao.hip, b3w_bao_have.hip); the arithmetic both sides share is
// b3w_bao_tree.h.  The device entry points stay in the .hip files, and b3w_sample_rows* beside them (they need b3w_plan_path_len).
#include "b3w_bao_plan.h"

#include <algorithm>

#include "../../include/b3wit.h"

namespace {

uint64_t read_header(const uint8_t *p) {
  uint64_t hdr = 0;
  for (int k = 0; k < 8; ++k) hdr |= (uint64_t)p[k] << (8 * k);
  return hdr;
}

// a stored node's sixteen words, and the CV it hashes to
void load_node(const uint8_t *node, uint32_t mw[16]) {
  for (int k = 0; k < 16; ++k) mw[k] = (uint32_t)node[4 * k] | ((uint32_t)node[4 * k + 1] << 8) | ((uint32_t)node[4 * k + 2] << 16) | ((uint32_t)node[4 * k + 3] << 24);
}
void parent_cv(const uint32_t m[16], bool root, uint32_t h[8]) {
  uint32_t ivv[8];
  iv(ivv);
  blake3_cv(ivv, m, 0, 0, 64, 4u | (root ? 8u : 0u), h);
}

// the CV of unit `u` of a group outboard: BLAKE3's tree over its chunks
void unit_cv(const uint8_t *data, uint64_t len, uint64_t n, uint32_t gl, uint64_t u, bool root, uint32_t h[8]) {
  const uint64_t c0 = u << gl, gn = n - c0 < (1ull << gl) ? n - c0 : (1ull << gl);
  host_subtree_cv(data, 0, len, c0, gn, root, h);
}

// the chunk ranges of one file as sorted unit ranges with ascending ends (for the walks' bisection); adjoining ones may overlap
std::vector<UpdRange> unit_ranges(uint64_t len, uint32_t gl, const uint64_t *first_chunk, const uint64_t *n_chunks, uint32_t n_ranges) {
  std::vector<uint32_t> zero(n_ranges, 0);
  std::vector<UpdRange> units = b3w_int_update_ranges(&len, zero.data(), first_chunk, n_chunks, n_ranges);
  for (UpdRange &r : units) { r.first >>= gl; r.end = (r.end + ((1ull << gl) - 1)) >> gl; }
  for (size_t i = 1; i < units.size(); ++i)
    if (units[i].end < units[i - 1].end) units[i].end = units[i - 1].end;
  return units;
}
// whether a range touches the units [first, first + cnt): the first range that ends behind `first` starts before first + cnt
bool touched(const std::vector<UpdRange> &units, uint64_t first, uint64_t cnt) {
  auto it = std::upper_bound(units.begin(), units.end(), first, [](uint64_t x, const UpdRange &r) { return x < r.end; });
  return it != units.end() && it->first < first + cnt;
}

void mask_set(uint32_t *mask, uint32_t lo, uint32_t hi) {
  for (uint32_t w = lo >> 5; w <= (hi - 1) >> 5; ++w) {
    const uint32_t a = w == lo >> 5 ? lo & 31 : 0, b = w == (hi - 1) >> 5 ? ((hi - 1) & 31) + 1 : 32;
    mask[w] |= (b == 32 ? ~0u : (1u << b) - 1) & ~((1u << a) - 1);
  }
}

// bao's decoder top down over the units [first, first + cnt) whose stored node (cnt > 1) is node `pos`: `want` is what the stored data
// above expects here, `bad` whether a node above failed.  With `units` (b3w_bao_verify_ranges) a subtree that no range touches is
// neither read nor written
void host_verify_walk(const uint8_t *data, uint64_t len, uint64_t n, uint32_t gl, const uint8_t *nodes, const std::vector<UpdRange> *units, uint64_t first,
                      uint64_t cnt, uint64_t pos, const uint32_t want[8], bool bad, bool root, uint8_t *status) {
  if (units && !touched(*units, first, cnt)) return;
  if (cnt == 1) {
    uint32_t h[8];
    unit_cv(data, len, n, gl, first, root, h);
    status[first] = bad ? 2 : memcmp(h, want, 32) != 0 ? 1 : 0;
    return;
  }
  uint32_t mw[16], o[8];
  load_node(nodes + 64 * pos, mw);
  parent_cv(mw, root, o);
  if (memcmp(o, want, 32) != 0) bad = true;
  const uint64_t k2 = left_of(cnt);
  host_verify_walk(data, len, n, gl, nodes, units, first, k2, pos + 1, mw, bad, false, status);
  host_verify_walk(data, len, n, gl, nodes, units, first + k2, cnt - k2, pos + k2, mw + 8, bad, false, status);
}

// the sparse walk over the units [first, first + cnt) whose stored node (cnt > 1) is node `pos`: false where no range touches them
// (nothing read, nothing written), else h = their CV, the dirty halves of the node stored
bool host_update_walk(const uint8_t *data, uint64_t len, uint64_t n, uint32_t gl, uint8_t *nodes, const std::vector<UpdRange> &units, uint64_t first,
                      uint64_t cnt, uint64_t pos, bool root, uint32_t h[8]) {
  if (!touched(units, first, cnt)) return false;
  if (cnt == 1) {
    unit_cv(data, len, n, gl, first, root, h);
    return true;
  }
  const uint64_t k2 = left_of(cnt);
  uint32_t m[16];
  uint8_t *node = nodes + 64 * pos;
  if (host_update_walk(data, len, n, gl, nodes, units, first, k2, pos + 1, false, m)) memcpy(node, m, 32); else memcpy(m, node, 32);
  if (host_update_walk(data, len, n, gl, nodes, units, first + k2, cnt - k2, pos + k2, false, m + 8)) memcpy(node + 32, m + 8, 32); else memcpy(m + 8, node + 32, 32);
  parent_cv(m, root, h);
  return true;
}

// the walk over the units [first, first + cnt) of the file at its new length, whose stored node (cnt > 1) is node `pos`: a kept tile's
// block is copied from the old outboard and its CV taken from the block's first node; everything else is hashed
void host_resize_walk(const uint8_t *data, uint64_t len, uint64_t n, uint32_t gl, const uint8_t *old_nodes, uint64_t old_units, uint64_t kept,
                      uint8_t *nodes, uint64_t first, uint64_t cnt, uint64_t pos, bool root, uint32_t h[8]) {
  const uint32_t sh = 10 - gl;
  uint32_t m[16];
  if (cnt == (1ull << sh) && !(first & (cnt - 1)) && (first >> sh) < kept) {
    const uint8_t *src = old_nodes + 64 * preorder_pos(old_units, first, cnt);
    memcpy(nodes + 64 * pos, src, (size_t)(cnt - 1) * 64);
    memcpy(m, src, 64);
    parent_cv(m, root, h);
    return;
  }
  if (cnt == 1) {
    unit_cv(data, len, n, gl, first, root, h);
    return;
  }
  const uint64_t k2 = left_of(cnt);
  host_resize_walk(data, len, n, gl, old_nodes, old_units, kept, nodes, first, k2, pos + 1, false, m);
  host_resize_walk(data, len, n, gl, old_nodes, old_units, kept, nodes, first + k2, cnt - k2, pos + k2, false, m + 8);
  memcpy(nodes + 64 * pos, m, 64);
  parent_cv(m, root, h);
}

// ---- range slices: one range, node by node ------------------------------------------------------------------------------------------
void put_words(uint8_t *dst, const uint32_t *w, uint32_t n) {
  for (uint32_t k = 0; k < n; ++k)
    for (int q = 0; q < 4; ++q) dst[4 * k + q] = (uint8_t)(w[k] >> (8 * q));
}

// the extractor's walk: the subtree over [lo, lo + size) of a file of n chunks, which meets [a, e); appends to out at `at`
struct RangeEnc { const uint8_t *ob, *bytes; uint64_t len, n, a, e, base_chunk; uint32_t gl; uint8_t *out; uint64_t at; };
void range_encode(RangeEnc &w, uint64_t lo, uint64_t size) {
  if (size == 1) {
    const uint64_t bytes = chunk_bytes(w.len, lo);
    if (bytes) memcpy(w.out + w.at, w.bytes + (lo - w.base_chunk) * 1024, bytes);
    w.at += bytes;
    return;
  }
  const uint64_t k = left_of(size), G = 1ull << w.gl;
  if (size > G) memcpy(w.out + w.at, w.ob + 8 + 64 * preorder_pos((w.n + G - 1) >> w.gl, lo >> w.gl, (size + G - 1) >> w.gl), 64);
  else {                                                  // inside a group: from the group's bytes
    uint32_t m[16];
    host_subtree_cv(w.bytes, w.base_chunk, w.len, lo, k, false, m);
    host_subtree_cv(w.bytes, w.base_chunk, w.len, lo + k, size - k, false, m + 8);
    put_words(w.out + w.at, m, 16);
  }
  w.at += 64;
  if (w.a < lo + k) range_encode(w, lo, k);
  if (w.e > lo + k) range_encode(w, lo + k, size - k);
}

// the decoder's walk, top down in slice order; the ingest's writes ride on it.  -> whether a chunk below verified
struct RangeDec {
  const uint8_t *sl; uint64_t len, n, a, e, at; bool hdr; uint32_t gl;
  uint8_t *out_bytes, *data, *ob; uint64_t *have;          // decode: out_bytes; ingest: data, ob, have (may be null)
  int32_t worst; uint64_t first_bad;
};
bool range_decode(RangeDec &w, uint64_t lo, uint64_t size, const uint32_t want[8], bool bad_above, bool root) {
  if (size == 1) {
    const uint64_t off = lo * 1024, bytes = chunk_bytes(w.len, lo);
    const uint8_t *src = w.sl + w.at;
    w.at += bytes;
    uint32_t h[8];
    host_chunk_cv(src, (uint32_t)bytes, lo, root ? 8u : 0u, h);
    const int32_t st = w.hdr ? 3 : bad_above ? 2 : memcmp(h, want, 32) != 0 ? 1 : 0;
    if (st) {
      if (st > w.worst) w.worst = st;
      if (lo < w.first_bad) w.first_bad = lo;
      return false;
    }
    if (bytes && w.out_bytes) memcpy(w.out_bytes + (lo - w.a) * 1024, src, bytes);
    if (bytes && w.data) memcpy(w.data + off, src, bytes);
    if (w.have) w.have[lo >> 6] |= 1ull << (lo & 63);
    return true;
  }
  const uint8_t *node = w.sl + w.at;
  w.at += 64;
  uint32_t mw[16], o[8];
  load_node(node, mw);
  parent_cv(mw, root, o);
  const bool bad = bad_above || memcmp(o, want, 32) != 0;
  const uint64_t k = left_of(size), G = 1ull << w.gl;
  bool any = false;
  if (w.a < lo + k) any |= range_decode(w, lo, k, mw, bad, false);
  if (w.e > lo + k) any |= range_decode(w, lo + k, size - k, mw + 8, bad, false);
  if (any && w.ob && size > G) memcpy(w.ob + 8 + 64 * preorder_pos((w.n + G - 1) >> w.gl, lo >> w.gl, (size + G - 1) >> w.gl), node, 64);
  return any;
}

int32_t range_decode_run(const uint8_t *slice, uint64_t slice_len, uint64_t len, uint64_t first, uint64_t count, const uint32_t *root, RangeDec &w) {
  const uint64_t n = num_chunks(len);
  if (!slice || !root || count == 0 || first >= n || count > n - first || slice_len != range_slice_bytes(len, n, first, count)) return B3W_E_BAD_ARGUMENT;
  w.sl = slice; w.len = len; w.n = n; w.a = first; w.e = first + count; w.at = 8; w.hdr = read_header(slice) != len; w.worst = 0; w.first_bad = ~0ull;
  const bool any = range_decode(w, 0, n, root, false, true);
  if (any && w.ob) memcpy(w.ob, slice, 8);
  return B3W_OK;
}

// ---- set slices: one file's runs, node by node (the range walks with "meets S" for "meets the range") ------------------------------------
struct SetEnc { const uint8_t *ob, *data; uint64_t len, n; const uint64_t *first, *count; uint64_t k; uint32_t gl; uint8_t *out; uint64_t at; };
void set_encode(SetEnc &w, uint64_t lo, uint64_t size) {
  if (size == 1) {
    const uint64_t bytes = chunk_bytes(w.len, lo);
    if (bytes) memcpy(w.out + w.at, w.data + lo * 1024, bytes);
    w.at += bytes;
    return;
  }
  const uint64_t k = left_of(size), G = 1ull << w.gl;
  if (size > G) memcpy(w.out + w.at, w.ob + 8 + 64 * preorder_pos((w.n + G - 1) >> w.gl, lo >> w.gl, (size + G - 1) >> w.gl), 64);
  else {                                                  // inside a group: from the group's bytes
    uint32_t m[16];
    host_subtree_cv(w.data, 0, w.len, lo, k, false, m);
    host_subtree_cv(w.data, 0, w.len, lo + k, size - k, false, m + 8);
    put_words(w.out + w.at, m, 16);
  }
  w.at += 64;
  if (set_meets(w.first, w.count, w.k, lo, lo + k)) set_encode(w, lo, k);
  if (set_meets(w.first, w.count, w.k, lo + k, lo + size)) set_encode(w, lo + k, size - k);
}

// the decoder's walk; chunks come in ascending order, so a chunk's rank is a running count
struct SetDec {
  const uint8_t *sl; uint64_t len, n; const uint64_t *first, *count; uint64_t k, at, rank; bool hdr; uint32_t gl;
  uint8_t *out_bytes, *data, *ob; uint64_t *have; int32_t *chunk_status;
  int32_t worst; uint64_t first_bad;
};
bool set_decode(SetDec &w, uint64_t lo, uint64_t size, const uint32_t want[8], bool bad_above, bool root) {
  if (size == 1) {
    const uint64_t bytes = chunk_bytes(w.len, lo), rank = w.rank++;
    const uint8_t *src = w.sl + w.at;
    w.at += bytes;
    uint32_t h[8];
    host_chunk_cv(src, (uint32_t)bytes, lo, root ? 8u : 0u, h);
    const int32_t st = w.hdr ? 3 : bad_above ? 2 : memcmp(h, want, 32) != 0 ? 1 : 0;
    if (w.chunk_status) w.chunk_status[rank] = st;
    if (st) {
      if (st > w.worst) w.worst = st;
      if (lo < w.first_bad) w.first_bad = lo;
      return false;
    }
    if (bytes && w.out_bytes) memcpy(w.out_bytes + rank * 1024, src, bytes);
    if (bytes && w.data) memcpy(w.data + lo * 1024, src, bytes);
    if (w.have) w.have[lo >> 6] |= 1ull << (lo & 63);
    return true;
  }
  const uint8_t *node = w.sl + w.at;
  w.at += 64;
  uint32_t mw[16], o[8];
  load_node(node, mw);
  parent_cv(mw, root, o);
  const bool bad = bad_above || memcmp(o, want, 32) != 0;
  const uint64_t k = left_of(size), G = 1ull << w.gl;
  bool any = false;
  if (set_meets(w.first, w.count, w.k, lo, lo + k)) any |= set_decode(w, lo, k, mw, bad, false);
  if (set_meets(w.first, w.count, w.k, lo + k, lo + size)) any |= set_decode(w, lo + k, size - k, mw + 8, bad, false);
  if (any && w.ob && size > G) memcpy(w.ob + 8 + 64 * preorder_pos((w.n + G - 1) >> w.gl, lo >> w.gl, (size + G - 1) >> w.gl), node, 64);
  return any;
}

int32_t set_decode_run(const uint8_t *slice, uint64_t slice_len, uint64_t len, const uint64_t *first, const uint64_t *count, uint32_t n_ranges,
                       const uint32_t *root, SetDec &w) {
  const uint64_t n = num_chunks(len);
  uint64_t bad;
  if (!slice || !root || !n_ranges || !first || !count || set_runs_wrong(n, first, count, n_ranges, &bad) ||
      slice_len != set_slice_bytes(len, first, count, n_ranges))
    return B3W_E_BAD_ARGUMENT;
  w.sl = slice; w.len = len; w.n = n; w.first = first; w.count = count; w.k = n_ranges; w.at = 8; w.rank = 0; w.hdr = read_header(slice) != len;
  w.worst = 0; w.first_bad = ~0ull;
  const bool any = set_decode(w, 0, n, root, false, true);
  if (any && w.ob) memcpy(w.ob, slice, 8);
  return B3W_OK;
}

}  // namespace

std::vector<UpdRange> b3w_int_update_ranges(const uint64_t *lens, const uint32_t *files, const uint64_t *first, const uint64_t *count, uint32_t n_ranges) {
  std::vector<UpdRange> v;
  v.reserve(n_ranges);
  for (uint32_t i = 0; i < n_ranges; ++i) {
    const uint64_t n = num_chunks(lens[files[i]]);
    if (!count[i] || first[i] >= n) continue;
    v.push_back(UpdRange{files[i], first[i], count[i] < n - first[i] ? first[i] + count[i] : n});
  }
  std::sort(v.begin(), v.end(), [](const UpdRange &a, const UpdRange &b) { return a.file != b.file ? a.file < b.file : a.first < b.first; });
  size_t k = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    if (k && v[k - 1].file == v[i].file && v[i].first <= v[k - 1].end) { if (v[i].end > v[k - 1].end) v[k - 1].end = v[i].end; }
    else v[k++] = v[i];
  }
  v.resize(k);
  return v;
}

UpdPlan b3w_int_update_plan(const uint64_t *lens, const std::vector<UpdRange> &ranges, uint32_t gl) {
  UpdPlan p;
  const uint64_t G1 = (1ull << gl) - 1;
  for (const UpdRange &r : ranges) {
    const uint64_t n = num_chunks(lens[r.file]);
    if (n <= 64) {
      if (p.small.empty() || p.small.back() != r.file) p.small.push_back(r.file);
      continue;
    }
    const uint64_t tiles = (n + B3W_TILE - 1) / B3W_TILE;
    uint64_t lo = r.first & ~G1, hi = (r.end + G1) & ~G1;
    if (hi > n) hi = n;
    for (uint64_t t = lo / B3W_TILE; t * B3W_TILE < hi; ++t) {
      if (p.tiles.empty() || p.tiles.back().file != r.file || p.tiles.back().idx != t) {
        UpdWg w{};
        w.file = r.file; w.idx = (uint32_t)t;
        w.out = tiles > 1 ? p.tile_slots++ : 0;
        p.tiles.push_back(w);
        if (tiles > 1) {                                              // the storey above: the tile is a dirty item of its span
          const uint32_t s = (uint32_t)(t / B3W_TILE);
          if (p.spans.empty() || p.spans.back().file != r.file || p.spans.back().idx != s) {
            UpdWg u{};
            u.file = r.file; u.idx = s; u.in = w.out;
            u.out = tiles > B3W_TILE ? p.span_slots++ : 0;
            p.spans.push_back(u);
            if (tiles > B3W_TILE) {
              if (p.tops.empty() || p.tops.back().file != r.file) {
                UpdWg v{};
                v.file = r.file; v.in = u.out;
                p.tops.push_back(v);
              }
              mask_set(p.tops.back().mask, s, s + 1);
            }
          }
          mask_set(p.spans.back().mask, (uint32_t)(t % B3W_TILE), (uint32_t)(t % B3W_TILE) + 1);
        }
      }
      const uint64_t t0 = t * B3W_TILE, a = lo > t0 ? lo : t0, b = hi < t0 + B3W_TILE ? hi : t0 + B3W_TILE;
      mask_set(p.tiles.back().mask, (uint32_t)(a - t0), (uint32_t)(b - t0));
    }
  }
  return p;
}

bool b3w_int_set_list(const uint64_t *lens, uint32_t n_files, const uint32_t *files, const uint64_t *first, const uint64_t *count, uint32_t n_ranges,
                      SetList &out) {
  out = SetList{};
  out.ufirst.resize(n_ranges);
  out.rank.resize(n_ranges);
  uint64_t at = slice_start(0);
  for (uint32_t i = 0; i < n_ranges;) {
    const uint32_t f = files[i];
    const char *why = nullptr;
    uint64_t bad = 0;
    uint32_t e = i;
    if (f >= n_files) why = "its file index is not below the file count";
    else {
      if (i && f < files[i - 1]) why = "the list is not ascending by (file, first chunk)";
      while (e < n_ranges && files[e] == f) ++e;
      if (!why) why = set_runs_wrong(num_chunks(lens[f]), first + i, count + i, e - i, &bad);
    }
    if (why) { out.why = "range " + std::to_string(i + bad) + ": " + why; return false; }
    SetEnt s{};
    s.file = f; s.range_first = i; s.range_end = e; s.chunk_first = out.chunks; s.slice = at;
    const uint64_t c0 = first[i], c1 = first[e - 1] + count[e - 1] - 1;
    s.shrt = set_is_short(c0, c1);
    if (s.shrt) s.rows = c1 / 64 - c0 / 64 + 1;
    else {
      uint64_t last = ~0ull;                               // the touched tiles: the runs ascend
      for (uint32_t r = i; r < e; ++r) {
        const uint64_t t0 = first[r] / B3W_TILE, t1 = (first[r] + count[r] - 1) / B3W_TILE;
        s.rows += t1 - t0 + (t0 == last ? 0 : 1);
        last = t1;
      }
    }
    for (uint32_t r = i; r < e; ++r) out.chunks += count[r];
    (s.shrt ? out.small : out.big) += s.rows;
    at = slice_start(at + set_slice_bytes(lens[f], first + i, count + i, e - i, out.ufirst.data() + i, out.rank.data() + i));
    out.sets.push_back(s);
    i = e;
  }
  out.bytes = at;
  return true;
}

void b3w_int_packed_range(uint64_t len, uint32_t gl, uint64_t a, uint64_t c, uint64_t *first, uint64_t *count) {
  const uint64_t n = num_chunks(len), G1 = (1ull << gl) - 1;
  if (n <= 64) { *first = 0; *count = n; return; }
  const uint64_t lo = a & ~G1, hi = (a + c + G1) & ~G1;
  *first = lo; *count = (hi < n ? hi : n) - lo;
}

PkLayout b3w_int_packed_layout(const uint64_t *lens, const std::vector<UpdRange> &ranges, uint32_t gl) {
  PkLayout p;
  for (const UpdRange &r : ranges) {
    uint64_t lo, cnt;
    b3w_int_packed_range(lens[r.file], gl, r.first, r.end - r.first, &lo, &cnt);
    if (!p.runs.empty() && p.runs.back().file == r.file && lo <= p.runs.back().end) {   // (whole groups of two ranges may meet where the ranges do not)
      PkRun &b = p.runs.back();
      if (lo + cnt > b.end) { p.slots += lo + cnt - b.end; b.end = lo + cnt; }
      continue;
    }
    p.runs.push_back(PkRun{r.file, lo, lo + cnt, p.slots});
    p.slots += cnt;
  }
  if (p.slots) p.bytes = 1024 * (p.slots - 1) + chunk_bytes(lens[p.runs.back().file], p.runs.back().end - 1);
  return p;
}

uint64_t PkLayout::slot_of(uint32_t file, uint64_t chunk) const {
  auto it = std::upper_bound(runs.begin(), runs.end(), chunk, [file](uint64_t c, const PkRun &r) { return file != r.file ? file < r.file : c < r.first; });
  const PkRun &r = *(it - 1);                                          // (a listed chunk: the last run that starts at or before it holds it)
  return r.slot + (chunk - r.first);
}

// ---- the set planner's and the packed set provider's row values (8 bytes a row beside the set table) ---------------------------------------
std::vector<uint64_t> b3w_int_range_row_first(const uint64_t *lens, const uint32_t *files, const uint64_t *first, const uint64_t *count, uint32_t n_ranges) {
  std::vector<uint64_t> row((size_t)n_ranges + 1);
  uint64_t at = 0;
  for (uint32_t i = 0; i < n_ranges; ++i) {
    const uint64_t len = lens[files[i]], n = num_chunks(len);
    row[i] = at;
    at += rows_before(len, n, first[i] + count[i]) - rows_before(len, n, first[i]);
  }
  row[n_ranges] = at;
  return row;
}

uint64_t b3w_int_set_row_base(uint64_t len, const uint64_t *first, const uint64_t *count, uint64_t k, const uint64_t *run_row, uint64_t a0) {
  const uint64_t n = num_chunks(len), i = set_run_behind(first, count, k, a0), cf = first[i] > a0 ? first[i] : a0;
  return run_row[i] + (rows_before(len, n, cf) - rows_before(len, n, first[i]));
}

uint64_t b3w_int_set_row_slot(const PkLayout &pk, uint32_t file, uint64_t len, uint32_t gl, const uint64_t *first, const uint64_t *count, uint64_t k,
                              uint64_t a0) {
  if (num_chunks(len) <= 64) return pk.slot_of(file, 0);
  const uint64_t i = set_run_behind(first, count, k, a0), cf = first[i] > a0 ? first[i] : a0;
  return pk.slot_of(file, cf & ~((1ull << gl) - 1));
}

// ---- the slot buffer of the packed receivers --------------------------------------------------------------------------------------------
uint64_t b3w_int_listed_chunks(const uint64_t *count, uint32_t n_ranges) {
  uint64_t sum = 0;
  for (uint32_t i = 0; i < n_ranges; ++i) {
    if (count[i] > ~0ull - sum) return ~0ull;
    sum += count[i];
  }
  return sum;
}

std::string b3w_int_slots_wrong(const void *d_chunks, uint64_t chunks_bytes, uint64_t listed) {
  if (listed > (~0ull >> 10)) return "the listed chunks' slots do not fit 64 bits of bytes";
  const std::string need = std::to_string(1024 * listed) + " bytes (1024 a listed chunk, " + std::to_string(listed) + " chunks)";
  if (listed && !d_chunks) return "a null d_chunks with a list that needs " + need;
  if ((uintptr_t)d_chunks & 15) return "d_chunks is not 16-byte aligned";
  if (chunks_bytes < 1024 * listed) return "chunks_bytes is " + std::to_string(chunks_bytes) + ", the slots take " + need;
  return std::string();
}

// ---- set slices taken in window by window: the cuts (b3wit.h "set slices in windows") ---------------------------------------------------
// cut[r], r > 0, is the end of the last wanted chunk in front of row r's block: the elements between that chunk and the row's first wanted
// chunk cf are the nodes of cf's path that do not hold the chunk before - every one has c0 = cf.  The rows are walked with the runs (the
// run that first reaches into a new block is the one being walked), a place is SetRuns' closed form: O(rows + runs), O(depth) a run on
// the file's ragged right edge, no step a chunk.
void b3w_int_set_stream_cuts(uint64_t len, const uint64_t *first, const uint64_t *count, uint32_t n_ranges, const SetList &l, std::vector<uint64_t> &cut) {
  const SetEnt &e = l.sets[0];
  const uint64_t n = num_chunks(len), B = e.shrt ? 64 : B3W_TILE;
  auto at = [&](uint64_t i, uint64_t c) { return 8 + 64 * set_nodes(n, l.ufirst[i], first[i], c) + 1024 * (l.rank[i] + (c - first[i])); };
  cut.clear();
  cut.reserve((size_t)e.rows + 1);
  uint64_t last = ~0ull;
  for (uint64_t i = 0; i < n_ranges; ++i)
    for (uint64_t blk = first[i] / B; blk <= (first[i] + count[i] - 1) / B; ++blk) {
      if (blk == last) continue;
      last = blk;
      const uint64_t a0 = blk * B;
      if (cut.empty()) cut.push_back(0);                  // (the header rides with row 0)
      else cut.push_back(1024 + (a0 > first[i] ? at(i, a0 - 1) : at(i - 1, first[i - 1] + count[i - 1] - 1)));
    }
  const uint64_t c_last = first[n_ranges - 1] + count[n_ranges - 1] - 1;
  cut.push_back(at(n_ranges - 1, c_last) + chunk_bytes(len, c_last));   // (set_slice_bytes, from the list's state)
}

bool b3w_int_set_stream_cuts(uint64_t len, const uint64_t *first, const uint64_t *count, uint32_t n_ranges, std::vector<uint64_t> &cut, bool *shrt,
                             std::string &why) {
  cut.clear();
  if (!n_ranges || !first || !count) { why = "a set has at least one run"; return false; }
  if (num_chunks(len) > (1ull << 30)) { why = "its file has more than 2^30 chunks"; return false; }
  const std::vector<uint32_t> files(n_ranges, 0);
  SetList l;
  if (!b3w_int_set_list(&len, 1, files.data(), first, count, n_ranges, l)) { why = l.why; return false; }
  b3w_int_set_stream_cuts(len, first, count, n_ranges, l, cut);
  if (shrt) *shrt = l.sets[0].shrt;
  return true;
}

extern "C" {

// ---- sizes and layouts ----------------------------------------------------------------------------------------------------------------
uint64_t b3w_bao_outboard_size(uint64_t len) { return group_outboard_bytes(len, 0); }

uint64_t b3w_bao_group_outboard_size(uint64_t len, uint32_t group_log) {
  return group_log > B3W_BAO_MAX_GROUP_LOG ? 0 : group_outboard_bytes(len, group_log);
}

uint64_t b3w_bao_group_batch_layout(const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, uint64_t *ob_first) {
  if (!ob_first || (!host_lens && n_files) || group_log > B3W_BAO_MAX_GROUP_LOG) return 0;
  uint64_t at = 0;
  for (uint32_t f = 0; f < n_files; ++f) { ob_first[f] = at; at += group_outboard_bytes(host_lens[f], group_log); }
  ob_first[n_files] = at;
  return at;
}

uint64_t b3w_bao_batch_layout(const uint64_t *host_lens, uint32_t n_files, uint64_t *ob_first) {
  return b3w_bao_group_batch_layout(host_lens, n_files, 0, ob_first);
}

uint64_t b3w_bao_batch_scratch_bytes(const uint64_t *host_lens, uint32_t n_files) {
  if (!host_lens) return 0;
  const BatchCounts k = batch_counts(host_lens, n_files);
  return (k.big_wgs + k.groups) * 32;
}

uint64_t b3w_bao_verify_layout(const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, uint64_t *unit_first) {
  if (!unit_first || (!host_lens && n_files) || group_log > B3W_BAO_MAX_GROUP_LOG) return 0;
  uint64_t at = 0;
  for (uint32_t f = 0; f < n_files; ++f) { unit_first[f] = at; at += n_units(host_lens[f], group_log); }
  unit_first[n_files] = at;
  return at;
}

uint64_t b3w_bao_verify_scratch_bytes(const uint64_t *host_lens, uint32_t n_files) {
  if (!host_lens) return 0;
  return (verify_entries(host_lens, n_files, nullptr) * 36 + 15) & ~15ull;           // the expected CV (32) and the flag (4) of every entry
}

uint64_t b3w_bao_stream_scratch_bytes(uint64_t len, uint32_t kind) {
  return kind == B3W_BAO_STREAM_OUTBOARD ? b3w_bao_batch_scratch_bytes(&len, 1) : kind == B3W_BAO_STREAM_VERIFY ? b3w_bao_verify_scratch_bytes(&len, 1) : 0;
}

uint64_t b3w_bao_stream_open_scratch_bytes(uint64_t capacity_bytes) {
  const uint64_t tiles = tiles_of(capacity_bytes);                     // (the tail's tile included)
  return (tiles + (tiles + B3W_TILE - 1) / B3W_TILE) * 32;
}

uint64_t b3w_bao_stream_open_block_pos(uint64_t len, uint32_t group_log, uint64_t tile) {
  if (group_log > B3W_BAO_MAX_GROUP_LOG || tile >= len / RES_TB) return UINT64_MAX;
  return preorder_pos(n_units(len, group_log), (tile * B3W_TILE) >> group_log, B3W_TILE >> group_log);
}

uint64_t b3w_bao_update_scratch_bytes(const uint64_t *host_lens, const uint32_t *host_files, const uint64_t *host_first_chunk,
                                      const uint64_t *host_n_chunks, uint32_t n_ranges) {
  if (!n_ranges || !host_lens || !host_files || !host_first_chunk || !host_n_chunks) return 0;
  const UpdPlan p = b3w_int_update_plan(host_lens, b3w_int_update_ranges(host_lens, host_files, host_first_chunk, host_n_chunks, n_ranges), 0);
  return (p.tile_slots + p.span_slots) * 32;
}

uint64_t b3w_bao_verify_ranges_scratch_bytes(const uint64_t *host_lens, const uint32_t *host_files, const uint64_t *host_first_chunk,
                                             const uint64_t *host_n_chunks, uint32_t n_ranges) {
  if (!n_ranges || !host_lens || !host_files || !host_first_chunk || !host_n_chunks) return 0;
  const UpdPlan p = b3w_int_update_plan(host_lens, b3w_int_update_ranges(host_lens, host_files, host_first_chunk, host_n_chunks, n_ranges), 0);
  return ((p.tile_slots + p.span_slots) * 36 + 15) & ~15ull;          // the expected CV (32) and the word (4) of every entry
}

int32_t b3w_bao_packed_layout(const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint32_t *host_files,
                              const uint64_t *host_first_chunk, const uint64_t *host_n_chunks, uint32_t n_ranges, uint64_t *range_slot,
                              uint64_t *range_first, uint64_t *range_chunks, uint64_t *total_slots, uint64_t *total_bytes) {
  if (!total_slots || !total_bytes || group_log > B3W_BAO_MAX_GROUP_LOG) return B3W_E_BAD_ARGUMENT;
  if (n_ranges && (!host_lens || !host_files || !host_first_chunk || !host_n_chunks)) return B3W_E_BAD_ARGUMENT;
  for (uint32_t i = 0; i < n_ranges; ++i) {                           // (the sparse calls' own refusals)
    if (host_files[i] >= n_files) return B3W_E_BAD_ARGUMENT;
    const uint64_t n = num_chunks(host_lens[host_files[i]]);
    if (n > (1ull << 30) || host_first_chunk[i] > n || host_n_chunks[i] > n - host_first_chunk[i]) return B3W_E_BAD_ARGUMENT;
  }
  const PkLayout p = b3w_int_packed_layout(host_lens, b3w_int_update_ranges(host_lens, host_files, host_first_chunk, host_n_chunks, n_ranges), group_log);
  for (uint32_t i = 0; i < n_ranges; ++i) {
    uint64_t first = 0, count = 0;
    if (host_n_chunks[i]) b3w_int_packed_range(host_lens[host_files[i]], group_log, host_first_chunk[i], host_n_chunks[i], &first, &count);
    if (range_slot) range_slot[i] = count ? p.slot_of(host_files[i], first) : 0;
    if (range_first) range_first[i] = first;
    if (range_chunks) range_chunks[i] = count;
  }
  *total_slots = p.slots;
  *total_bytes = p.bytes;
  return B3W_OK;
}

uint64_t b3w_bao_resize_kept_tiles(uint64_t old_len, uint64_t new_len) { return (old_len < new_len ? old_len : new_len) / RES_TB; }

uint64_t b3w_bao_resize_scratch_bytes(const uint64_t *host_new_lens, const uint32_t *host_files, uint32_t n_resized) {
  if (!n_resized || !host_new_lens || !host_files) return 0;
  uint64_t slots = 0;
  for (uint32_t i = 0; i < n_resized; ++i) slots += resize_slots(host_new_lens[host_files[i]]);
  return slots * 32;
}

uint64_t b3w_bao_have_layout(const uint64_t *host_lens, uint32_t n_files, uint64_t *word_first) {
  if (!word_first || (!host_lens && n_files)) return 0;
  uint64_t at = 0;
  for (uint32_t f = 0; f < n_files; ++f) { word_first[f] = at; at += (num_chunks(host_lens[f]) + 63) / 64; }
  word_first[n_files] = at;
  return at;
}

// ---- paths and slices of one chunk ------------------------------------------------------------------------------------------------------
int32_t b3w_bao_path_nodes(uint64_t chunk, uint64_t n_chunks, uint64_t *out_index, uint32_t *out_count) {
  if (!out_index || !out_count || !n_chunks || chunk >= n_chunks) return B3W_E_BAD_ARGUMENT;
  uint64_t p = 0, c = chunk, m = n_chunks;
  uint32_t i = 0;
  while (m > 1) {
    const uint64_t k = left_of(m);
    out_index[i++] = p;
    if (c < k) { p += 1; m = k; } else { p += k; c -= k; m -= k; }
  }
  *out_count = i;
  return B3W_OK;
}

int32_t b3w_bao_group_path_nodes(uint64_t chunk, uint64_t n_chunks, uint32_t group_log, uint64_t *out_index, uint32_t *out_count) {
  if (group_log > B3W_BAO_MAX_GROUP_LOG || !n_chunks || chunk >= n_chunks) return B3W_E_BAD_ARGUMENT;
  return b3w_bao_path_nodes(chunk >> group_log, (n_chunks + (1ull << group_log) - 1) >> group_log, out_index, out_count);
}

uint64_t b3w_bao_slice_size(uint64_t len, uint64_t chunk) {
  const uint64_t n = num_chunks(len);
  return chunk >= n ? 0 : slice_bytes(len, chunk, depth_in(chunk, n));
}

int64_t b3w_bao_slice_batch_layout(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_chunks,
                                   uint32_t n_samples, uint64_t *slice_first) {
  if (!slice_first || (n_samples && (!host_lens || !host_files || !host_chunks))) return -B3W_E_BAD_ARGUMENT;
  for (uint32_t s = 0; s < n_samples; ++s)
    if (host_files[s] >= n_files || host_chunks[s] >= num_chunks(host_lens[host_files[s]])) return -B3W_E_BAD_ARGUMENT;
  uint64_t at = slice_start(0);
  for (uint32_t s = 0; s < n_samples; ++s) {
    slice_first[s] = at;
    at = slice_start(at + b3w_bao_slice_size(host_lens[host_files[s]], host_chunks[s]));
  }
  slice_first[n_samples] = at;
  return (int64_t)at;
}

int32_t b3w_bao_slice(const uint8_t *outboard, uint64_t len, uint64_t chunk, const uint8_t *chunk_bytes_in, uint8_t *out, uint64_t *out_len) {
  const uint64_t n = num_chunks(len);
  if (!outboard || !out_len || chunk >= n) return B3W_E_BAD_ARGUMENT;
  if (read_header(outboard) != len) return B3W_E_BAD_ARGUMENT;
  uint64_t idx[64];
  uint32_t P = 0;
  (void)b3w_bao_path_nodes(chunk, n, idx, &P);
  const uint64_t bytes = chunk_bytes(len, chunk);
  *out_len = 8 + 64ull * P + bytes;
  if (!out) return B3W_OK;
  if (bytes && !chunk_bytes_in) return B3W_E_BAD_ARGUMENT;
  memcpy(out, outboard, 8);
  for (uint32_t i = 0; i < P; ++i) memcpy(out + 8 + 64ull * i, outboard + 8 + 64 * idx[i], 64);
  if (bytes) memcpy(out + 8 + 64ull * P, chunk_bytes_in, bytes);
  return B3W_OK;
}

int32_t b3w_bao_slice_decode(const uint8_t *slice, uint64_t slice_len, uint64_t len, uint64_t chunk, const uint32_t *root, uint8_t *out_chunk,
                             uint32_t *out_bytes, int32_t *out_status) {
  const uint64_t n = num_chunks(len);
  if (!slice || !root || !out_status || chunk >= n || slice_len != b3w_bao_slice_size(len, chunk)) return B3W_E_BAD_ARGUMENT;
  int32_t st = read_header(slice) != len ? 3 : 0;
  uint32_t want[8];
  for (int k = 0; k < 8; ++k) want[k] = root[k];
  const uint32_t P = depth_in(chunk, n);
  uint64_t cc = chunk, m = n;
  for (uint32_t i = 0; i < P; ++i) {                     // top down, as the sampled-path planner
    uint32_t mw[16], o[8];
    load_node(slice + 8 + 64ull * i, mw);
    parent_cv(mw, i == 0, o);
    if (memcmp(o, want, 32) != 0 && st == 0) st = 2;
    const uint64_t k2 = left_of(m);
    const bool left = cc < k2;
    for (int k = 0; k < 8; ++k) want[k] = left ? mw[k] : mw[8 + k];
    if (left) m = k2; else { cc -= k2; m -= k2; }
  }
  const uint32_t bytes = (uint32_t)(slice_len - 8 - 64ull * P);
  uint32_t h[8];
  host_chunk_cv(slice + 8 + 64ull * P, bytes, chunk, n == 1 ? 8u : 0u, h);
  if (memcmp(h, want, 32) != 0 && st == 0) st = 1;
  *out_status = st;
  if (out_bytes) *out_bytes = st == 0 ? bytes : 0;       // (the bytes are handed out only where they verified, as bao's decoder does)
  if (out_chunk && st == 0 && bytes) memcpy(out_chunk, slice + 8 + 64ull * P, bytes);
  return B3W_OK;
}

int32_t b3w_bao_slice_ingest(const uint8_t *slice, uint64_t slice_len, uint64_t len, uint64_t chunk, const uint32_t *root, uint32_t group_log,
                             uint8_t *data, uint8_t *outboard, int32_t *out_status) {
  if (group_log > B3W_BAO_MAX_GROUP_LOG || !outboard || (!data && len)) return B3W_E_BAD_ARGUMENT;
  int32_t st = 0;
  const int32_t rc = b3w_bao_slice_decode(slice, slice_len, len, chunk, root, nullptr, nullptr, out_status ? &st : nullptr);   // (refuses the rest)
  if (rc) return rc;
  *out_status = st;
  if (st) return B3W_OK;                                  // nothing unverified is written
  const uint64_t n = num_chunks(len);
  uint64_t idx[64];
  uint32_t U = 0;
  (void)b3w_bao_group_path_nodes(chunk, n, group_log, idx, &U);
  memcpy(outboard, slice, 8);
  for (uint32_t i = 0; i < U; ++i) memcpy(outboard + 8 + 64 * idx[i], slice + 8 + 64ull * i, 64);   // (the path's first U nodes are the stored ones)
  const uint64_t bytes = chunk_bytes(len, chunk);
  if (bytes) memcpy(data + chunk * 1024, slice + slice_len - bytes, bytes);
  return B3W_OK;
}

// ---- one file against, into and out of its outboard ------------------------------------------------------------------------------------
int32_t b3w_bao_verify(const uint8_t *data, uint64_t len, const uint8_t *outboard, uint32_t group_log, const uint32_t *root, uint8_t *unit_status,
                       int32_t *file_status, uint64_t *first_bad) {
  if ((!data && len) || !outboard || !root || !unit_status || group_log > B3W_BAO_MAX_GROUP_LOG) return B3W_E_BAD_ARGUMENT;
  const uint64_t n = num_chunks(len), units = n_units(len, group_log);
  if (read_header(outboard) != len) memset(unit_status, 3, (size_t)units);
  else host_verify_walk(data, len, n, group_log, outboard + 8, nullptr, 0, units, 0, root, false, true, unit_status);
  int32_t worst = 0;
  uint64_t first = ~0ull;
  for (uint64_t u = 0; u < units; ++u) {
    if (unit_status[u] > worst) worst = unit_status[u];
    if (unit_status[u] && first == ~0ull) first = u;
  }
  if (file_status) *file_status = worst;
  if (first_bad) *first_bad = first;
  return B3W_OK;
}

int32_t b3w_bao_verify_ranges(const uint8_t *data, uint64_t len, const uint8_t *outboard, uint32_t group_log, const uint32_t *root,
                              const uint64_t *host_first_chunk, const uint64_t *host_n_chunks, uint32_t n_ranges, uint8_t *unit_status,
                              int32_t *range_status, uint64_t *range_first_bad) {
  if ((!data && len) || !outboard || !root || !unit_status || group_log > B3W_BAO_MAX_GROUP_LOG || (n_ranges && (!host_first_chunk || !host_n_chunks)))
    return B3W_E_BAD_ARGUMENT;
  const uint64_t n = num_chunks(len);
  for (uint32_t i = 0; i < n_ranges; ++i)
    if (host_first_chunk[i] > n || host_n_chunks[i] > n - host_first_chunk[i]) return B3W_E_BAD_ARGUMENT;
  const std::vector<UpdRange> units = unit_ranges(len, group_log, host_first_chunk, host_n_chunks, n_ranges);
  if (!units.empty() && read_header(outboard) != len) {               // (read once, and only where something is listed)
    for (const UpdRange &r : units) memset(unit_status + r.first, 3, (size_t)(r.end - r.first));
  } else {
    host_verify_walk(data, len, n, group_log, outboard + 8, &units, 0, n_units(len, group_log), 0, root, false, true, unit_status);
  }
  for (uint32_t i = 0; i < n_ranges; ++i) {
    int32_t worst = 0;
    uint64_t first = ~0ull;
    if (host_n_chunks[i])
      for (uint64_t u = host_first_chunk[i] >> group_log; u <= (host_first_chunk[i] + host_n_chunks[i] - 1) >> group_log; ++u) {
        if (unit_status[u] > worst) worst = unit_status[u];
        if (unit_status[u] && first == ~0ull) first = u;
      }
    if (range_status) range_status[i] = worst;
    if (range_first_bad) range_first_bad[i] = first;
  }
  return B3W_OK;
}

int32_t b3w_bao_outboard_update(const uint8_t *data, uint64_t len, uint8_t *outboard, uint32_t group_log, const uint64_t *host_first_chunk,
                                const uint64_t *host_n_chunks, uint32_t n_ranges, uint32_t *root) {
  if ((!data && len) || !outboard || !root || group_log > B3W_BAO_MAX_GROUP_LOG || (n_ranges && (!host_first_chunk || !host_n_chunks))) return B3W_E_BAD_ARGUMENT;
  const uint64_t n = num_chunks(len);
  for (uint32_t i = 0; i < n_ranges; ++i)
    if (host_first_chunk[i] > n || host_n_chunks[i] > n - host_first_chunk[i]) return B3W_E_BAD_ARGUMENT;
  const std::vector<UpdRange> units = unit_ranges(len, group_log, host_first_chunk, host_n_chunks, n_ranges);
  uint32_t h[8];
  if (host_update_walk(data, len, n, group_log, outboard + 8, units, 0, n_units(len, group_log), 0, true, h)) memcpy(root, h, 32);
  return B3W_OK;
}

int32_t b3w_bao_outboard_resize(const uint8_t *data, uint64_t new_len, const uint8_t *old_outboard, uint64_t old_len, uint32_t group_log,
                                uint8_t *new_outboard, uint32_t *root) {
  if (!old_outboard || !new_outboard || !root || group_log > B3W_BAO_MAX_GROUP_LOG) return B3W_E_BAD_ARGUMENT;
  const uint64_t kept = b3w_bao_resize_kept_tiles(old_len, new_len);
  if (!data && new_len > kept * RES_TB) return B3W_E_BAD_ARGUMENT;
  if (num_chunks(old_len) > (1ull << 30) || num_chunks(new_len) > (1ull << 30)) return B3W_E_BAD_ARGUMENT;
  const uintptr_t a0 = (uintptr_t)old_outboard, a1 = a0 + group_outboard_bytes(old_len, group_log);
  const uintptr_t b0 = (uintptr_t)new_outboard, b1 = b0 + group_outboard_bytes(new_len, group_log);
  if (a0 < b1 && b0 < a1) return B3W_E_BAD_ARGUMENT;
  uint32_t h[8];
  host_resize_walk(data, new_len, num_chunks(new_len), group_log, old_outboard + 8, n_units(old_len, group_log), kept, new_outboard + 8, 0,
                   n_units(new_len, group_log), 0, true, h);
  for (int k = 0; k < 8; ++k) new_outboard[k] = (uint8_t)(new_len >> (8 * k));
  memcpy(root, h, 32);
  return B3W_OK;
}

// ---- range slices ---------------------------------------------------------------------------------------------------------------------
uint64_t b3w_bao_range_slice_size(uint64_t len, uint64_t first_chunk, uint64_t n_chunks) {
  const uint64_t n = num_chunks(len);
  if (n_chunks == 0 || first_chunk >= n || n_chunks > n - first_chunk) return 0;
  return range_slice_bytes(len, n, first_chunk, n_chunks);
}

int64_t b3w_bao_range_slice_batch_layout(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_first,
                                         const uint64_t *host_count, uint32_t n_ranges, uint64_t *slice_first) {
  if (!slice_first || (n_ranges && (!host_lens || !host_files || !host_first || !host_count))) return -B3W_E_BAD_ARGUMENT;
  for (uint32_t i = 0; i < n_ranges; ++i)
    if (host_files[i] >= n_files || !b3w_bao_range_slice_size(host_lens[host_files[i]], host_first[i], host_count[i])) return -B3W_E_BAD_ARGUMENT;
  uint64_t at = slice_start(0);
  for (uint32_t i = 0; i < n_ranges; ++i) {
    slice_first[i] = at;
    at = slice_start(at + b3w_bao_range_slice_size(host_lens[host_files[i]], host_first[i], host_count[i]));
  }
  slice_first[n_ranges] = at;
  return (int64_t)at;
}

uint64_t b3w_bao_range_slice_ingest_scratch_bytes(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_first,
                                                  const uint64_t *host_count, uint32_t n_ranges) {
  if (!host_lens || !host_files || !host_first || !host_count) return 0;
  uint64_t rows = 0;
  for (uint32_t i = 0; i < n_ranges; ++i) {
    if (host_files[i] >= n_files || !b3w_bao_range_slice_size(host_lens[host_files[i]], host_first[i], host_count[i])) return 0;
    rows += range_rows(host_first[i], host_count[i]);
  }
  return rows * 16;                                       // a row's status and first bad chunk
}

int64_t b3w_sample_rows_ranges(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_first,
                               const uint64_t *host_count, uint32_t n_ranges, uint64_t *range_row_first, uint64_t *chunk_row_first,
                               uint8_t *chunk_provable) {
  if (!range_row_first || (n_ranges && (!host_lens || !host_files || !host_first || !host_count))) return -B3W_E_BAD_ARGUMENT;
  for (uint32_t i = 0; i < n_ranges; ++i)
    if (host_files[i] >= n_files || !b3w_bao_range_slice_size(host_lens[host_files[i]], host_first[i], host_count[i])) return -B3W_E_BAD_ARGUMENT;
  uint64_t row = 0, at = 0;
  for (uint32_t i = 0; i < n_ranges; ++i) {
    const uint64_t len = host_lens[host_files[i]], n = num_chunks(len), a = host_first[i], k = host_count[i];
    range_row_first[i] = row;
    if (chunk_row_first || chunk_provable) {               // (asked for: the one loop over chunks)
      uint64_t r = row;
      for (uint64_t c = a; c < a + k; ++c, ++at) {
        if (chunk_row_first) chunk_row_first[at] = r;
        if (chunk_provable) chunk_provable[at] = path_provable(c, n) ? 1 : 0;
        r += chunk_blocks(len, c) + depth_in(c, n);
      }
    }
    row += rows_before(len, n, a + k) - rows_before(len, n, a);
  }
  range_row_first[n_ranges] = row;
  if (chunk_row_first) chunk_row_first[at] = row;
  return (int64_t)row;
}

int64_t b3w_bao_range_slice(const uint8_t *outboard, uint64_t len, uint32_t group_log, uint64_t first_chunk, uint64_t n_chunks, const uint8_t *range_bytes,
                            uint8_t *out, uint64_t out_len) {
  const uint64_t size = b3w_bao_range_slice_size(len, first_chunk, n_chunks);
  if (!size || group_log > B3W_BAO_MAX_GROUP_LOG) return -B3W_E_BAD_ARGUMENT;
  if (!out) return (int64_t)size;
  if (!outboard || (!range_bytes && len) || out_len < size) return -B3W_E_BAD_ARGUMENT;
  memcpy(out, outboard, 8);
  RangeEnc w{outboard, range_bytes, len, num_chunks(len), first_chunk, first_chunk + n_chunks, (first_chunk >> group_log) << group_log, group_log, out, 8};
  range_encode(w, 0, w.n);
  return (int64_t)w.at;
}

int32_t b3w_bao_range_slice_decode(const uint8_t *slice, uint64_t slice_len, uint64_t len, uint64_t first_chunk, uint64_t n_chunks, const uint32_t *root,
                                   uint8_t *out_bytes, int32_t *out_status, uint64_t *out_first_bad) {
  if (!out_status) return B3W_E_BAD_ARGUMENT;
  RangeDec w{};
  w.out_bytes = out_bytes;
  const int32_t rc = range_decode_run(slice, slice_len, len, first_chunk, n_chunks, root, w);
  if (rc) return rc;
  *out_status = w.worst;
  if (out_first_bad) *out_first_bad = w.first_bad;
  return B3W_OK;
}

int32_t b3w_bao_range_slice_ingest(const uint8_t *slice, uint64_t slice_len, uint64_t len, uint64_t first_chunk, uint64_t n_chunks, const uint32_t *root,
                                   uint32_t group_log, uint8_t *data, uint8_t *outboard, uint64_t *have, int32_t *out_status, uint64_t *out_first_bad) {
  if (group_log > B3W_BAO_MAX_GROUP_LOG || !outboard || (!data && len) || !out_status) return B3W_E_BAD_ARGUMENT;
  RangeDec w{};
  w.gl = group_log; w.data = data; w.ob = outboard; w.have = have;
  const int32_t rc = range_decode_run(slice, slice_len, len, first_chunk, n_chunks, root, w);
  if (rc) return rc;
  *out_status = w.worst;
  if (out_first_bad) *out_first_bad = w.first_bad;
  return B3W_OK;
}

// ---- set slices -----------------------------------------------------------------------------------------------------------------------
uint64_t b3w_bao_set_slice_size(uint64_t len, const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges) {
  uint64_t bad;
  if (!n_ranges || !host_first || !host_count || set_runs_wrong(num_chunks(len), host_first, host_count, n_ranges, &bad)) return 0;
  return set_slice_bytes(len, host_first, host_count, n_ranges);
}

int64_t b3w_bao_set_slice_batch_layout(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_first,
                                       const uint64_t *host_count, uint32_t n_ranges, uint32_t *set_file, uint32_t *set_range_first,
                                       uint64_t *set_chunk_first, uint64_t *slice_first, uint32_t *n_sets) {
  if (n_ranges && (!host_lens || !host_files || !host_first || !host_count)) return -B3W_E_BAD_ARGUMENT;
  SetList l;
  if (!b3w_int_set_list(host_lens, n_files, host_files, host_first, host_count, n_ranges, l)) return -B3W_E_BAD_ARGUMENT;
  const size_t k = l.sets.size();
  for (size_t s = 0; s < k; ++s) {
    if (set_file) set_file[s] = l.sets[s].file;
    if (set_range_first) set_range_first[s] = l.sets[s].range_first;
    if (set_chunk_first) set_chunk_first[s] = l.sets[s].chunk_first;
    if (slice_first) slice_first[s] = l.sets[s].slice;
  }
  if (set_range_first) set_range_first[k] = n_ranges;
  if (set_chunk_first) set_chunk_first[k] = l.chunks;
  if (slice_first) slice_first[k] = l.bytes;
  if (n_sets) *n_sets = (uint32_t)k;
  return (int64_t)l.bytes;
}

uint64_t b3w_bao_set_slice_ingest_scratch_bytes(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_first,
                                                const uint64_t *host_count, uint32_t n_ranges) {
  if (!host_lens || !host_files || !host_first || !host_count) return 0;
  SetList l;
  if (!b3w_int_set_list(host_lens, n_files, host_files, host_first, host_count, n_ranges, l)) return 0;
  return (l.big + l.small) * 16;                          // a row's status and first bad chunk
}

int64_t b3w_bao_set_slice_stream_cuts(uint64_t len, const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, uint64_t max_window_bytes,
                                      uint64_t *cuts_out, uint64_t cap) {
  std::vector<uint64_t> cut;
  std::string why;
  if (max_window_bytes < B3W_BAO_SET_SLICE_STREAM_MIN_WINDOW || !b3w_int_set_stream_cuts(len, host_first, host_count, n_ranges, cut, nullptr, why))
    return -B3W_E_BAD_ARGUMENT;
  // greedy: a window takes whole rows while they fit (a row always fits: it is never longer than the least window)
  const size_t rows = cut.size() - 1;
  uint64_t windows = 0;
  for (int pass = 0; pass < 2; ++pass) {
    windows = 0;
    for (size_t i = 0; i < rows;) {
      size_t j = i + 1;
      while (j < rows && cut[j + 1] - cut[i] <= max_window_bytes) ++j;
      if (pass) cuts_out[windows] = cut[i];
      ++windows;
      i = j;
    }
    if (pass) cuts_out[windows] = cut[rows];
    if (!cuts_out || cap < windows + 1) break;             // (the count alone: nothing is written into a list that is too short)
  }
  return (int64_t)windows;
}

uint64_t b3w_bao_set_slice_stream_scratch_bytes(uint64_t len, const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges,
                                                uint64_t max_window_bytes) {
  std::vector<uint64_t> cut;
  std::string why;
  if (max_window_bytes < B3W_BAO_SET_SLICE_STREAM_MIN_WINDOW || !b3w_int_set_stream_cuts(len, host_first, host_count, n_ranges, cut, nullptr, why)) return 0;
  const size_t rows = cut.size() - 1;
  uint64_t most = 0;
  for (size_t i = 0, j = 0; i < rows; ++i) {               // the most rows any window of that many bytes can hold, wherever it starts
    if (j < i + 1) j = i + 1;
    while (j < rows && cut[j + 1] - cut[i] <= max_window_bytes) ++j;
    if (j - i > most) most = j - i;
  }
  return B3W_BAO_SET_SLICE_STREAM_CARRY_BYTES + 16 * most;
}

int64_t b3w_bao_set_slice(const uint8_t *outboard, uint64_t len, uint32_t group_log, const uint64_t *host_first, const uint64_t *host_count,
                          uint32_t n_ranges, const uint8_t *data, uint8_t *out, uint64_t out_len) {
  const uint64_t size = b3w_bao_set_slice_size(len, host_first, host_count, n_ranges);
  if (!size || group_log > B3W_BAO_MAX_GROUP_LOG) return -B3W_E_BAD_ARGUMENT;
  if (!out) return (int64_t)size;
  if (!outboard || (!data && len) || out_len < size) return -B3W_E_BAD_ARGUMENT;
  memcpy(out, outboard, 8);
  SetEnc w{outboard, data, len, num_chunks(len), host_first, host_count, n_ranges, group_log, out, 8};
  set_encode(w, 0, w.n);
  return (int64_t)w.at;
}

int32_t b3w_bao_set_slice_decode(const uint8_t *slice, uint64_t slice_len, uint64_t len, const uint64_t *host_first, const uint64_t *host_count,
                                 uint32_t n_ranges, const uint32_t *root, uint8_t *out_bytes, int32_t *chunk_status, int32_t *out_status,
                                 uint64_t *out_first_bad) {
  if (!out_status) return B3W_E_BAD_ARGUMENT;
  SetDec w{};
  w.out_bytes = out_bytes; w.chunk_status = chunk_status;
  const int32_t rc = set_decode_run(slice, slice_len, len, host_first, host_count, n_ranges, root, w);
  if (rc) return rc;
  *out_status = w.worst;
  if (out_first_bad) *out_first_bad = w.first_bad;
  return B3W_OK;
}

int32_t b3w_bao_set_slice_ingest(const uint8_t *slice, uint64_t slice_len, uint64_t len, const uint64_t *host_first, const uint64_t *host_count,
                                 uint32_t n_ranges, const uint32_t *root, uint32_t group_log, uint8_t *data, uint8_t *outboard, uint64_t *have,
                                 int32_t *chunk_status, int32_t *out_status, uint64_t *out_first_bad) {
  if (group_log > B3W_BAO_MAX_GROUP_LOG || !outboard || (!data && len) || !out_status) return B3W_E_BAD_ARGUMENT;
  SetDec w{};
  w.gl = group_log; w.data = data; w.ob = outboard; w.have = have; w.chunk_status = chunk_status;
  const int32_t rc = set_decode_run(slice, slice_len, len, host_first, host_count, n_ranges, root, w);
  if (rc) return rc;
  *out_status = w.worst;
  if (out_first_bad) *out_first_bad = w.first_bad;
  return B3W_OK;
}

// ---- the arrival bitmap of one file, unit by unit (the device side: b3w_bao_have.hip) --------------------------------------------------
int32_t b3w_bao_have_runs(const uint64_t *have, uint64_t len, uint32_t group_log, uint32_t kind, uint64_t capacity, uint64_t *run_first,
                          uint64_t *run_count, uint64_t *n_runs, uint64_t *n_have) {
  if (!have || !n_runs || group_log > B3W_BAO_MAX_GROUP_LOG || (kind != B3W_BAO_HAVE_MISSING && kind != B3W_BAO_HAVE_PRESENT) ||
      (capacity && (!run_first || !run_count)))
    return B3W_E_BAD_ARGUMENT;
  const uint64_t n = num_chunks(len), F = 1ull << group_log;
  uint64_t runs = 0, set = 0, open_at = 0;
  bool open = false;
  for (uint64_t c = 0; c < n; c += F) {
    const uint64_t end = c + F < n ? c + F : n;
    uint64_t got = 0;
    for (uint64_t k = c; k < end; ++k) got += (have[k >> 6] >> (k & 63)) & 1;
    set += got;
    const bool sel = (kind == B3W_BAO_HAVE_PRESENT) == (got == end - c);
    if (sel && !open) { open = true; open_at = c; }
    if (open && (!sel || end == n)) {
      const uint64_t stop = sel ? end : c;
      if (runs < capacity) { run_first[runs] = open_at; run_count[runs] = stop - open_at; }
      ++runs;
      open = false;
    }
  }
  *n_runs = runs;
  if (n_have) *n_have = set;
  return B3W_OK;
}

int32_t b3w_bao_have_from_status(const uint8_t *status, uint64_t len, uint32_t group_log, uint64_t *have) {
  if (!status || !have || group_log > B3W_BAO_MAX_GROUP_LOG) return B3W_E_BAD_ARGUMENT;
  const uint64_t n = num_chunks(len);
  for (uint64_t w = 0; w < (n + 63) / 64; ++w) have[w] = 0;
  for (uint64_t c = 0; c < n; ++c)
    if (status[c >> group_log] == 0) have[c >> 6] |= 1ull << (c & 63);
  return B3W_OK;
}

// ---- the chunks two versions of one file share, from their outboards alone (the device side: the diff kernel in b3w_bao_have.hip) ------
int32_t b3w_bao_outboard_diff(const uint8_t *outboard_a, uint64_t len_a, const uint32_t *root_a, uint32_t group_log_a, const uint8_t *outboard_b,
                              uint64_t len_b, const uint32_t *root_b, uint32_t group_log_b, uint64_t *same_words) {
  if (!outboard_a || !root_a || !outboard_b || !root_b || !same_words || group_log_a > B3W_BAO_MAX_GROUP_LOG || group_log_b > B3W_BAO_MAX_GROUP_LOG)
    return B3W_E_BAD_ARGUMENT;
  const uint64_t na = num_chunks(len_a), nb = num_chunks(len_b);
  if (na > DIFF_MAX_CHUNKS || nb > DIFF_MAX_CHUNKS) return B3W_E_BAD_ARGUMENT;
  const uint32_t G = group_log_a > group_log_b ? group_log_a : group_log_b;
  for (uint64_t w = 0; w < (nb + 63) / 64; ++w) same_words[w] = 0;
  for (uint64_t u = 0; u < n_units(len_b, G); ++u) {
    if (!diff_unit_comparable((uint32_t)na, (uint32_t)nb, (uint32_t)u, G)) continue;
    const bool whole = nb <= (1ull << G);
    const void *cv_a = whole ? (const void *)root_a : outboard_a + diff_cv_at((uint32_t)na, group_log_a, (uint32_t)u, G);
    const void *cv_b = whole ? (const void *)root_b : outboard_b + diff_cv_at((uint32_t)nb, group_log_b, (uint32_t)u, G);
    if (memcmp(cv_a, cv_b, 32)) continue;
    for (uint64_t c = u << G; c < nb && c < (u + 1) << G; ++c) same_words[c >> 6] |= 1ull << (c & 63);
  }
  return B3W_OK;
}

// ---- outboard deltas on the host (the device side: the delta kernels in b3w_bao_have.hip; the verdicts: b3w_bao_tree.h) ------------------
static_assert(DELTA_MALFORMED == B3W_BAO_DELTA_MALFORMED && DELTA_BAD_HASH == B3W_BAO_DELTA_BAD_HASH && DELTA_NOT_HELD == B3W_BAO_DELTA_NOT_HELD, "b3wit.h");

uint64_t b3w_bao_outboard_delta_bound(uint64_t len_b, uint32_t group_log) {
  if (group_log > B3W_BAO_MAX_GROUP_LOG) return 0;
  const uint64_t ub = n_units(len_b, group_log);
  return 16 + 8 * delta_words(ub) + 64 * (ub - 1);
}

uint64_t b3w_bao_outboard_delta_layout(const uint64_t *host_lens_b, uint32_t n_files_b, const uint32_t *host_pair_b, uint32_t n_pairs, uint32_t group_log,
                                       uint64_t *delta_first) {
  if (!host_lens_b || !delta_first || group_log > B3W_BAO_MAX_GROUP_LOG) return 0;
  uint64_t at = 0;
  for (uint32_t i = 0; i < n_pairs; ++i) {
    const uint32_t fb = host_pair_b ? host_pair_b[i] : i;
    if (fb >= n_files_b) return 0;
    delta_first[i] = at;
    at += b3w_bao_outboard_delta_bound(host_lens_b[fb], group_log);
  }
  delta_first[n_pairs] = at;
  return at;
}

static bool delta_sides_of(const uint8_t *outboard_a, uint64_t len_a, const uint32_t *root_a, uint64_t len_b, const uint32_t *root_b, uint32_t g, DeltaSides &s) {
  if (!root_b || (outboard_a && !root_a) || g > B3W_BAO_MAX_GROUP_LOG) return false;
  const uint64_t na = outboard_a ? num_chunks(len_a) : 0, nb = num_chunks(len_b);
  if (na > DIFF_MAX_CHUNKS || nb > DIFF_MAX_CHUNKS) return false;
  s.ob_a = outboard_a;
  s.root_a = reinterpret_cast<const uint8_t *>(root_a);
  s.root_b = reinterpret_cast<const uint8_t *>(root_b);
  s.na = (uint32_t)na; s.nb = (uint32_t)nb;
  s.ua = outboard_a ? (uint32_t)n_units(len_a, g) : 0; s.ub = (uint32_t)n_units(len_b, g);
  s.g = g;
  return true;
}

int32_t b3w_bao_outboard_delta(const uint8_t *outboard_a, uint64_t len_a, const uint32_t *root_a, const uint8_t *outboard_b, uint64_t len_b,
                               const uint32_t *root_b, uint32_t group_log, uint8_t *blob, uint64_t blob_bytes, uint64_t *n_nodes) {
  DeltaSides s;
  if (!outboard_b || !blob || !n_nodes || !delta_sides_of(outboard_a, len_a, root_a, len_b, root_b, group_log, s)) return B3W_E_BAD_ARGUMENT;
  const uint64_t W = delta_words(s.ub);
  if (blob_bytes < 16 + 8 * W) return B3W_E_BAD_ARGUMENT;
  const uint64_t cap = (blob_bytes - 16 - 8 * W) / 64;
  uint64_t k = 0;
  memset(blob + 16, 0, 8 * W);
  for (uint32_t p = 0; p + 1 < s.ub; ++p) {
    if (delta_node_same(s, outboard_b, p)) continue;
    blob[16 + p / 8] |= (uint8_t)(1u << (p & 7));          // (little-endian words: bit p of the bitmap is bit p & 7 of byte p / 8)
    if (k < cap) memcpy(blob + 16 + 8 * W + 64 * k, outboard_b + 8 + 64ull * p, 64);
    ++k;
  }
  memcpy(blob, &len_b, 8);
  memcpy(blob + 8, &k, 8);
  *n_nodes = k;
  return B3W_OK;
}

int32_t b3w_bao_outboard_delta_apply(const uint8_t *outboard_a, uint64_t len_a, const uint32_t *root_a, uint64_t len_b, const uint32_t *root_b,
                                     uint32_t group_log, const uint8_t *blob, uint64_t blob_bytes, uint8_t *outboard_out, int32_t *status,
                                     uint64_t *first_bad) {
  DeltaSides s;
  if (!blob || !outboard_out || !status || !first_bad || !delta_sides_of(outboard_a, len_a, root_a, len_b, root_b, group_log, s)) return B3W_E_BAD_ARGUMENT;
  const uint64_t W = delta_words(s.ub);
  if (blob_bytes < 16 + 8 * W) return B3W_E_BAD_ARGUMENT;
  const uint64_t cap = (blob_bytes - 16 - 8 * W) / 64;
  std::vector<uint64_t> before(W + 1);                     // the set bits in front of every word
  before[0] = 0;
  for (uint64_t j = 0; j < W; ++j) before[j + 1] = before[j] + (uint64_t)__builtin_popcountll(delta_load64(blob + 16 + 8 * j));
  const auto rank = [&](uint32_t q) {
    return before[q >> 6] + (uint64_t)__builtin_popcountll(delta_load64(blob + 16 + 8 * (uint64_t)(q >> 6)) & ((1ull << (q & 63)) - 1));
  };
  uint64_t key = delta_check_head(blob, len_b, cap, before[W]);
  for (uint64_t p = 0; p < 64 * W; ++p) {
    const uint64_t one = delta_check_node(s, blob, cap, (uint32_t)p, rank);
    if (one < key) key = one;
  }
  *status = key == DELTA_OK ? 0 : (int32_t)(key & 3);
  *first_bad = key == DELTA_OK ? ~0ull : key >> 2;
  if (key != DELTA_OK) return B3W_OK;
  memcpy(outboard_out, &len_b, 8);
  for (uint32_t p = 0; p + 1 < s.ub; ++p) {
    const uint8_t *src;
    if ((delta_load64(blob + 16 + 8 * (uint64_t)(p >> 6)) >> (p & 63)) & 1) src = blob + 16 + 8 * W + 64 * rank(p);
    else {
      const uint64_t at = delta_copy_from(s, p);
      if (!at) continue;
      src = outboard_a + at;
    }
    uint8_t *dst = outboard_out + 8 + 64ull * p;
    if (src != dst) memcpy(dst, src, 64);
  }
  return B3W_OK;
}

}  // extern "C"
