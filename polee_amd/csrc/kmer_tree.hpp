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
