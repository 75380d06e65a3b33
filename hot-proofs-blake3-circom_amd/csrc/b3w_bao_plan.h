// b3w_bao_plan.h — the plan of the sparse bao calls (update, ranged verification): defined in b3w_bao_host.cpp, where the scratch sizes
// use it; the device entry points of b3w_bao.hip build their tables from it, and their packed twins find their chunks' slots with the
// packed layout below.  Not installed.
#pragma once
#include <string>
#include <vector>

#include "b3w_bao_tree.h"

struct UpdRange { uint32_t file; uint64_t first, end; };              // chunks [first, end) of the file
// a workgroup of the plan: the file, the tile / span within it, its own scratch slot and the slot of its first dirty input item
struct UpdWg { uint32_t file, idx; uint64_t out, in; uint32_t mask[B3W_TILE / 32]; };
struct UpdPlan {
  std::vector<uint32_t> small;                                        // the dirty files of at most 64 chunks, ascending, each once
  std::vector<UpdWg> tiles, spans, tops;                              // the three storeys, sorted by (file, idx)
  uint64_t tile_slots = 0, span_slots = 0;                            // scratch: the dirty tiles of files of more than one tile, then the dirty spans past 1 GiB
};
// the ranges that are not empty, sorted by (file, first chunk), overlapping and adjoining ones of a file merged; ends clamped to the file
std::vector<UpdRange> b3w_int_update_ranges(const uint64_t *lens, const uint32_t *files, const uint64_t *first, const uint64_t *count, uint32_t n_ranges);
// what a call over these (sorted, merged) ranges launches; the chunk masks are expanded to whole groups of 1 << gl chunks
UpdPlan b3w_int_update_plan(const uint64_t *lens, const std::vector<UpdRange> &ranges, uint32_t gl);

// The sets of a set-slice call (b3wit.h "set slices"): a set is the maximal stretch of consecutive ranges of one file; its rows are one
// or two blocks of 64 chunks (shrt) or its touched tiles.
struct SetEnt { uint32_t file, range_first, range_end; uint64_t chunk_first, slice, rows; bool shrt; };
struct SetList {
  std::vector<SetEnt> sets;
  std::vector<uint64_t> ufirst, rank;                                 // a range: U_S of its first chunk, the set's wanted chunks in front of it (SetRuns)
  uint64_t big = 0, small = 0, chunks = 0, bytes = 0;                  // rows of 1 024 and of 64 chunks; the wanted chunks; the packed slices' bytes
  std::string why;                                                    // a refusal: "range i: ..."
};
// false for a list the set calls refuse (why names the range): a file index >= n_files, an empty range or one past its file, a list
// that is not ascending by (file, first chunk) or not disjoint
bool b3w_int_set_list(const uint64_t *lens, uint32_t n_files, const uint32_t *files, const uint64_t *first, const uint64_t *count, uint32_t n_ranges,
                      SetList &out);

// The cuts of ONE set's slice (b3wit.h "set slices in windows"): cut[r] the offset of the first element whose least wanted chunk lies in
// row r's block, rows in the table's order, cut[0] = 0 and cut[rows] the slice's size; *shrt (may be null): rows of 64.  false with why
// for a list the set calls refuse, no run at all, or a file of more than 2^30 chunks.
bool b3w_int_set_stream_cuts(uint64_t len, const uint64_t *first, const uint64_t *count, uint32_t n_ranges, std::vector<uint64_t> &cut, bool *shrt,
                             std::string &why);
// the same from the list b3w_int_set_list has made of these runs as the one file of a call (l.sets[0]): no second walk over the runs
void b3w_int_set_stream_cuts(uint64_t len, const uint64_t *first, const uint64_t *count, uint32_t n_ranges, const SetList &l, std::vector<uint64_t> &cut);

// The set planner's rows (b3w_sample_plan_set_slices_device).  For an ascending disjoint list a set's wanted chunks in ascending order are
// the list's chunks in order, so the record rows are b3w_sample_rows_ranges': run_row = its range_row_first (n_ranges + 1 values, from
// rows_before: O(depth) a range), and a table row's base is the first record row of the first wanted chunk at or behind chunk a0 (the
// block's start) of the set whose runs are (first, count)[0 .. k), run_row[] their first rows: the run that straddles or follows a0 and
// the part of it in front of the block.  64 bits; no step a chunk.
std::vector<uint64_t> b3w_int_range_row_first(const uint64_t *lens, const uint32_t *files, const uint64_t *first, const uint64_t *count, uint32_t n_ranges);
uint64_t b3w_int_set_row_base(uint64_t len, const uint64_t *first, const uint64_t *count, uint64_t k, const uint64_t *run_row, uint64_t a0);

// The packed layout (b3wit.h "sparse calls from packed chunk bytes"): the chunks b3w_int_update_plan has hashed, as runs of consecutive
// chunks of one file in consecutive slots of 1 024 bytes, sorted by (file, first chunk); no two runs of a file touch.
struct PkRun { uint32_t file; uint64_t first, end, slot; };           // chunks [first, end) of the file lie from slot `slot` on
struct PkLayout {
  std::vector<PkRun> runs;
  uint64_t slots = 0, bytes = 0;                                      // bytes: the end of the last listed chunk's last byte
  uint64_t slot_of(uint32_t file, uint64_t chunk) const;              // of a LISTED chunk
};
// over the (sorted, merged) ranges of b3w_int_update_ranges: a file of at most 64 chunks lists all its chunks, any other one the
// whole groups of 1 << gl chunks its ranges touch, clamped to the file
PkLayout b3w_int_packed_layout(const uint64_t *lens, const std::vector<UpdRange> &ranges, uint32_t gl);
// the chunks [*first, *first + *count) that range (file, a, c) of a call lists, c > 0: its groups, or all of a file of at most 64 chunks
void b3w_int_packed_range(uint64_t len, uint32_t gl, uint64_t a, uint64_t c, uint64_t *first, uint64_t *count);
// the packed set provider's row (b3w_bao_set_slice_packed_device): the slot of the first LISTED chunk of the block from chunk a0 on of
// the set whose runs are (first, count)[0 .. k) - chunk 0 of a file of at most 64 chunks, else the start of the group that holds the
// block's first wanted chunk; the block's listed chunks follow it slot by slot
uint64_t b3w_int_set_row_slot(const PkLayout &pk, uint32_t file, uint64_t len, uint32_t gl, const uint64_t *first, const uint64_t *count, uint64_t k,
                              uint64_t a0);

// The slot buffer of the packed RECEIVERS (b3wit.h "slices taken into packed chunk slots"): 1 024 bytes a listed chunk, in the order of
// the per-chunk statuses - sample i at slot i; range r's chunk c at slot chunk_first[r] + (c - first[r]), chunk_first the running sum of
// the counts; set s's wanted chunk of rank k at slot set_chunk_first[s] + k (SetEnt::chunk_first).
// the chunks a range list lists: the sum of the counts, UINT64_MAX where that does not fit
uint64_t b3w_int_listed_chunks(const uint64_t *count, uint32_t n_ranges);
// empty, or why a call over `listed` chunks refuses (d_chunks, chunks_bytes): null with a list that is not empty, not 16-byte aligned,
// too few bytes (the message names the bytes needed)
std::string b3w_int_slots_wrong(const void *d_chunks, uint64_t chunks_bytes, uint64_t listed);
