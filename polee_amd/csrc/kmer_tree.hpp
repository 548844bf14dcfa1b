// polee fit-tree: what the host builder (kmer_tree.cpp) and the device path (kmer_tree_device.hip) share.
#pragma once
#include <time.h>

#include "common.hpp"

namespace polee {

constexpr int KMER_K = POLEE_KMER_K;
constexpr int KMER_H = POLEE_KMER_H;
constexpr uint32_t KMER_EMPTY = 0xFFFFFFFFu;

struct KmerEdge {
    uint32_t u, v, mat, empt;  // 1-based nodes, u < v
};

// What the merge loop needs of the sketches.  The distinct non-zero values are ranked in ascending order, so a sketch is kept
// as ranks: equal values are equal ranks, the smaller value is the smaller rank, and an empty bin (KMER_EMPTY) loses every
// minimum -- the union of two sketches is the per-bin minimum of their ranks.
struct KmerIndex {
    int64_t n = 0;
    std::vector<uint32_t> ranks;      // [n][200], grows by one row per Jaccard merge
    std::vector<uint32_t> run_start;  // [R + 1]: the nodes that hold the value of rank r are ent[run_start[r] .. run_start[r + 1])
    std::vector<uint32_t> ent;        // 0-based nodes, grouped by rank
    std::vector<KmerEdge> edges;      // every pair with mat > 0, sorted by (u, v)
};

// POLEE_ERR_BAD_ARG unless every non-zero value v of the sketches [n][200] lies in bin (v - 1) mod 200 (and is not 2^64 - 1)
polee_status kmer_validate_sketches(polee_ctx *ctx, int64_t n, const uint64_t *sketches);
// the host-only way to the index (sorts on the host threads); POLEE_ERR_BAD_ARG for a value outside its bin or too many pairs
polee_status kmer_index_host(int64_t n, const uint64_t *sketches, KmerIndex &ix);
// steps 2-4 of the definition: Jaccard merges, Huffman phase, DFS.  Consumes the index.
polee_status kmer_tree_merge(KmerIndex &ix, int32_t *node_parent_idxs, int32_t *node_js);
// steps 3-4 alone, for every merge method: the Huffman phase over the active ones of the nodes [0, next) (0-based: transcripts
// 0 .. n-1, merged nodes from n on), then the DFS.  left / right / height have room for 2n - 1 nodes, active for `next`.
polee_status kmer_tree_finish(int64_t n, size_t next, std::vector<uint32_t> &left, std::vector<uint32_t> &right, std::vector<uint32_t> &height,
                              const std::vector<uint8_t> &active, int32_t *node_parent_idxs, int32_t *node_js);

inline uint32_t kmer_empt_of(const uint64_t *ma, const uint64_t *mb)
{
    return (uint32_t)(__builtin_popcountll(ma[0] & mb[0]) + __builtin_popcountll(ma[1] & mb[1]) + __builtin_popcountll(ma[2] & mb[2]) +
                      __builtin_popcountll(ma[3] & mb[3]));
}
inline void kmer_mask_of(const uint32_t *ranks, uint64_t *m)  // bit b: bin b is empty
{
    m[0] = m[1] = m[2] = m[3] = 0;
    for (int b = 0; b < KMER_H; ++b)
        if (ranks[b] == KMER_EMPTY) m[b >> 6] |= 1ull << (b & 63);
}

// ---- the device path's steps (kmer_tree_device.hip), shared with the rounds on the device (kmer_rounds_device.hip)
struct KmerClock;
struct KmerIndexDev {         // what of the index stays on the device
    DevBuf<uint32_t> ranks;   // [rows][200], the first n rows filled
    DevBuf<uint64_t> masks;   // [rows][4], bit b: bin b is empty
    DevBuf<KmerEdge> edges;   // NE of them, sorted by (u, v)
    uint32_t NE = 0;          // (0: the buffers may be unallocated)
};
polee_status kmer_check_offsets(polee_ctx *ctx, int64_t n, const int64_t *offsets, const uint8_t *bases, const char *who);
polee_status kmer_sketch_device(polee_ctx *ctx, int64_t n, const int64_t *offsets, const uint8_t *bases, DevBuf<uint64_t> &d_sk, KmerClock &clk);
polee_status kmer_index_device(polee_ctx *ctx, int64_t n, const uint64_t *d_sk, KmerIndex *host, KmerIndexDev *keep, size_t rows);

// sort on the host threads: sorted chunks, then rounds of pairwise merges
template <class T>
inline void kmer_parallel_sort(std::vector<T> &a)
{
    const size_t N = a.size();
    const size_t T0 = std::max<size_t>(1, std::min<size_t>(host_threads(), N >> 16));
    size_t parts = 1;
    while (parts < T0) parts <<= 1;
    if (parts == 1) {
        std::sort(a.begin(), a.end());
        return;
    }
    auto cut = [&](size_t k) { return (size_t)((unsigned __int128)N * k / parts); };
    parallel_chunks(parts, 1, [&](size_t lo, size_t, unsigned) { std::sort(a.begin() + (ptrdiff_t)cut(lo), a.begin() + (ptrdiff_t)cut(lo + 1)); });
    for (size_t w = 1; w < parts; w <<= 1)
        parallel_chunks(parts / (2 * w), 1, [&](size_t lo, size_t, unsigned) {
            std::inplace_merge(a.begin() + (ptrdiff_t)cut(2 * w * lo), a.begin() + (ptrdiff_t)cut(2 * w * lo + w),
                               a.begin() + (ptrdiff_t)cut(2 * w * lo + 2 * w));
        });
}

struct KmerClock {  // POLEE_BUILD_TIMING=1: the builder's phases on stderr
    bool on = getenv("POLEE_BUILD_TIMING") != nullptr;
    double t0;
    static double now()
    {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
    }
    KmerClock() : t0(now()) {}
    void lap(const char *what, hipStream_t stream = nullptr, bool sync = false)
    {
        if (!on) return;
        if (sync) (void)hipStreamSynchronize(stream);
        fprintf(stderr, "[kmer tree]   . %-26s %.4f s\n", what, now() - t0);
        t0 = now();
    }
};

}  // namespace polee
