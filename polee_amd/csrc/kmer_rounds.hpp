// polee fit-tree, merge in rounds: what the host twin (kmer_rounds.cpp) and the device path
// (kmer_rounds_device.hip) share -- the priority of an edge, the edge record, the statistics.
#pragma once
#include "kmer_tree.hpp"

namespace polee {

struct KmerREdge {
    uint32_t u, v;  // 0-based nodes, u < v
    uint64_t key;   // bits of J << 32 | h32(u + 1, v + 1); never 0 (mat > 0)
};

struct KmerRoundsStats {
    int64_t rounds = 0, merges = 0, left = 0, reevaluated = 0;
    void store(int64_t *out) const
    {
        if (!out) return;
        out[0] = rounds;
        out[1] = merges;
        out[2] = left;
        out[3] = reevaluated;
    }
};

// the hash of edge_pri (hclust.cpp) on the 1-based node numbers lo < hi
__host__ __device__ inline uint32_t kmer_h32(uint32_t lo, uint32_t hi)
{
    uint64_t h = (uint64_t)lo * 0x9E3779B97F4A7C15ull ^ ((uint64_t)hi * 0xC2B2AE3D27D4EB4Full + 0x165667B19E3779F9ull);
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return (uint32_t)h;
}
// equal keys fall to the smaller (lo, hi): an atomic minimum over this
__host__ __device__ inline uint64_t kmer_pack(uint32_t u, uint32_t v) { return ((uint64_t)u << 32) | v; }

// bits of J = Float32(mat) / Float32(200 - empt), formed on the host only: the device reads them from a table
// [201][201] indexed [mat][empt] (entries with mat + empt > 200 are never read), so both sides hold the same bits
inline uint32_t kmer_jbits(uint32_t mat, uint32_t empt)
{
    const float J = (float)mat / (float)(KMER_H - (int)empt);
    uint32_t b;
    memcpy(&b, &J, 4);
    return b;
}
constexpr int KMER_JT = KMER_H + 1;
inline std::vector<uint32_t> kmer_jbits_table()
{
    std::vector<uint32_t> t((size_t)KMER_JT * KMER_JT, 0);
    for (uint32_t m = 0; m <= (uint32_t)KMER_H; ++m)
        for (uint32_t e = 0; m + e <= (uint32_t)KMER_H && e < (uint32_t)KMER_H; ++e) t[(size_t)m * KMER_JT + e] = kmer_jbits(m, e);
    return t;
}
inline uint64_t kmer_key(uint32_t u, uint32_t v, uint32_t mat, uint32_t empt) { return ((uint64_t)kmer_jbits(mat, empt) << 32) | kmer_h32(u + 1, v + 1); }

// One best-and-select step on the host: of E edges (0-based nodes below num_nodes, u < v, distinct pairs) those that are the best
// edge of both endpoints, as indexes into the edge array by descending priority.  bestkey / besttie: num_nodes entries each,
// any content.
void kmer_round_select_host(const KmerREdge *edges, size_t E, std::atomic<uint64_t> *bestkey, std::atomic<uint64_t> *besttie, std::vector<uint32_t> &chosen);

// the rounds of merges, the Huffman phase and the DFS from a host index; consumes it
polee_status kmer_tree_rounds_host(KmerIndex &ix, int32_t *node_parent_idxs, int32_t *node_js, KmerRoundsStats &st, KmerClock &clk);

}  // namespace polee
