// gc_merge.h -- the garbage collector's range tree as a sort and two scans
// (__add_to_brtree -> brt_add, lib/brtree.c:44-108, walked by
// brt_loop_on_ranges into gc_data_stat_cb, mdsl/gc.c:746-753), stated once.
// The kernels of gc_merge.hip and the CPU composition of
// tests/native/gc_merge_host.cc only combine the functions of this header,
// which is plain C++17 outside hipcc.
//
// What the tree computes, whatever the order of insertion:
//   sort the ranges by low; a range starts a new extent if and only if its low
//   is strictly greater than the largest high seen so far (touching ranges
//   merge: the tree's compare returns 0 for them); an extent is [first low,
//   largest high); the walk delivers the extents in ascending order.
// The rules for n ranges:
//   drop    a range with high <= low (a u64 wrap of offset + len + 1; the
//           tree's comparator is inconsistent on such a node) is counted in
//           nwrapped and takes no part in anything else.  It gets the sort key
//           2^64 - 1, which no kept range has (its high would have to be
//           larger), and so sorts behind every kept range.
//   sort    LSD radix sort of the keys, kGcRadixBits a pass, high as the
//           payload.  A pass: per tile of kGcSortTile keys a histogram of the
//           pass's digit; an exclusive sum-scan of the table [digit][tile]; a
//           scatter of each key to its digit's and tile's base plus the number
//           of keys with that digit before it in the tile (stable), counted
//           in rounds of kGcRound keys.
//   runmax  inclusive max-scan over the sorted array of high (0 for a dropped
//           range).
//   heads   element i is a head if it is kept and (i == 0 or low[i] >
//           runmax[i - 1]); with an exclusive sum-scan of the heads a kept
//           element's extent is k = the heads before it, plus 1 if it is a
//           head itself, minus 1.
//   emit    the head writes out[k].low; the extent's last element (kept, and
//           i == n - 1 or i + 1 dropped or a head) writes out[k].high =
//           runmax[i]; only k < out_cap is written.
//   stat    nout = the heads, valid = the sum of high - low over the extents
//           (mod 2^64), max = the last extent's high (runmax[n - 1]; 0 with
//           none), nin = n, nwrapped as counted.
// Every scan is one primitive over tiles of kGcScanTile elements: a reduce per
// tile, one workgroup of kGcAggThreads over the tile aggregates (a loop with a
// carry), a downsweep per tile.  A scan of one tile is its downsweep alone.
#ifndef POM_GC_MERGE_H
#define POM_GC_MERGE_H

#include <stddef.h>
#include <stdint.h>

#include "pom_gc.h"

#ifdef __HIPCC__
#define GC_MERGE_FN __device__ __host__ __forceinline__
#else
#define GC_MERGE_FN static inline
#endif

constexpr uint32_t kGcMergeMaxN = POM_GC_MERGE_MAX;
constexpr uint32_t kGcRadixBits = 8;
constexpr uint32_t kGcRadix = 1u << kGcRadixBits;
constexpr uint32_t kGcPasses = 64 / kGcRadixBits;
constexpr uint32_t kGcSortThreads = 256;                // 4 waves, each a quarter of the tile
constexpr uint32_t kGcSortTile = 4096;
constexpr uint32_t kGcRound = 64;                       // keys a wave ranks at once
constexpr uint32_t kGcScanThreads = 256;
constexpr uint32_t kGcScanItems = 8;                    // consecutive elements a thread
constexpr uint32_t kGcScanTile = kGcScanThreads * kGcScanItems;
constexpr uint32_t kGcAggThreads = 1024;                // the aggregates' pass: its carry loop runs past this many tiles
constexpr uint64_t kGcDroppedKey = ~0ull;

static_assert(kGcRadix == kGcSortThreads, "one thread per digit sums a tile's histogram");
static_assert(kGcPasses % 2 == 0, "the sorted array ends in the buffer it started in");

GC_MERGE_FN bool gc_merge_kept(uint64_t low, uint64_t high)
{
    return high > low;
}

GC_MERGE_FN uint64_t gc_merge_key(uint64_t low, uint64_t high)
{
    return gc_merge_kept(low, high) ? low : kGcDroppedKey;
}

GC_MERGE_FN bool gc_merge_key_kept(uint64_t key)
{
    return key != kGcDroppedKey;
}

GC_MERGE_FN uint32_t gc_merge_digit(uint64_t key, uint32_t pass)
{
    return (uint32_t)(key >> (kGcRadixBits * pass)) & (kGcRadix - 1u);
}

// Where the scatter puts a key.  A tile is walked in rounds of kGcRound
// consecutive keys (a wave's lanes); base is where the round's first key of
// this digit goes (the scanned table's entry plus the digit's keys in the
// tile's earlier rounds), equal_before the keys of the same digit before this
// one in the round, of equal_in_round in all.
GC_MERGE_FN uint32_t gc_merge_slot(uint32_t base, uint32_t equal_before, uint32_t equal_in_round)
{
    (void)equal_in_round;
    return base + equal_before;
}

// The max-scan's input and operator.
GC_MERGE_FN uint64_t gc_merge_high(uint64_t key, uint64_t high)
{
    return gc_merge_key_kept(key) ? high : 0ull;
}

GC_MERGE_FN uint64_t gc_merge_max(uint64_t a, uint64_t b)
{
    return a > b ? a : b;
}

// Element i of the sorted array, with runmax[i - 1] (anything for i == 0).
GC_MERGE_FN bool gc_merge_head(uint32_t i, uint64_t key, uint64_t runmax_before)
{
    return gc_merge_key_kept(key) && (i == 0 || key > runmax_before);
}

// Element i is its extent's last: next_key is key[i + 1] (anything for i == n - 1).
GC_MERGE_FN bool gc_merge_last(uint32_t i, uint32_t n, uint64_t key, uint64_t next_key, uint64_t runmax)
{
    return gc_merge_key_kept(key) &&
           (i + 1u == n || !gc_merge_key_kept(next_key) || gc_merge_head(i + 1u, next_key, runmax));
}

// The extent of a kept element: `before` heads lie before it (the exclusive
// scan), and it may be one itself.
GC_MERGE_FN uint32_t gc_merge_extent(uint32_t before, bool head)
{
    return before + (head ? 1u : 0u) - 1u;
}

GC_MERGE_FN uint32_t gc_merge_tiles(uint32_t n, uint32_t tile)
{
    return n / tile + (n % tile != 0);
}

// The scratch of one merge of n ranges, as byte offsets (all multiples of 8):
//   key[0], val[0], key[1], val[1]   u64, n each: the sort's two buffers; the
//                                     sorted array ends in [0], and then
//                                     key[1] holds runmax and val[1] the
//                                     extent indices (u32)
//   table                            u32, kGcRadix per sort tile
//   agg                              u64, one per scan tile of the longest scan, and one more
//   part                             per scan tile of the ranges: {u64 sum, u32 heads, u32 kept}
struct gc_merge_layout {
    size_t o_key[2], o_val[2], o_table, o_agg, o_part, total;
    uint32_t sort_tiles, table_len, range_tiles, agg_len;
};

GC_MERGE_FN gc_merge_layout gc_merge_scratch_layout(uint32_t n)
{
    gc_merge_layout L{};
    size_t o = 0;
    for (uint32_t k = 0; k < 2; k++) {
        L.o_key[k] = o;
        o += 8 * (size_t)n;
        L.o_val[k] = o;
        o += 8 * (size_t)n;
    }
    L.sort_tiles = gc_merge_tiles(n, kGcSortTile);
    L.table_len = L.sort_tiles * kGcRadix;
    L.range_tiles = gc_merge_tiles(n, kGcScanTile);
    const uint32_t table_tiles = gc_merge_tiles(L.table_len, kGcScanTile);
    L.agg_len = (table_tiles > L.range_tiles ? table_tiles : L.range_tiles) + 1u;
    L.o_table = o;
    o += ((size_t)L.table_len * 4 + 7) & ~(size_t)7;
    L.o_agg = o;
    o += 8 * (size_t)L.agg_len;
    L.o_part = o;
    o += 16 * (size_t)L.range_tiles;
    L.total = o;
    return L;
}

#endif
