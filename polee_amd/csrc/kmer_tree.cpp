// polee fit-tree on the host (upstream src/kmersketch.jl, src/kmercluster.jl): the sketch of a transcript's
// canonical 32-mers, the candidate pairs of a set of sketches, and the tree -- greedy Jaccard merges from a heap on
// (J desc, u, v), the Huffman phase over what is left, nodes in DFS pre-order.  Nothing here touches the GPU; kmer_tree_device.hip
// replaces the first two steps and hands the same KmerIndex to the same merge loop.
#include <queue>

#include "kmer_tree.hpp"

namespace polee {
namespace {

inline uint64_t mix64(uint64_t c)
{
    uint64_t z = c + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

void sketch_one(const uint8_t *s, int64_t len, uint64_t *out)
{
    uint64_t best[KMER_H];
    for (int b = 0; b < KMER_H; ++b) best[b] = ~0ull;
    uint64_t fw = 0, bw = 0;
    int run = 0;  // valid bases in a row, ending here
    for (int64_t i = 0; i < len; ++i) {
        const unsigned c = s[i] & 0xDFu;
        const bool ok = c == 'A' || c == 'C' || c == 'G' || c == 'T';
        const uint64_t code = ok ? ((c >> 1) ^ (c >> 2)) & 3u : 0u;
        fw = (fw << 2) | code;
        bw = (bw >> 2) | ((3 - code) << 62);
        run = ok ? std::min(run + 1, KMER_K) : 0;
        if (run < KMER_K) continue;
        const uint64_t h = std::min<uint64_t>(mix64(std::min(fw, bw)), ~0ull - 2);
        const int b = (int)(h % KMER_H);
        best[b] = std::min(best[b], h + 1);
    }
    for (int b = 0; b < KMER_H; ++b) out[b] = best[b] == ~0ull ? 0 : best[b];
}

struct Entry {
    uint64_t value;
    uint32_t node;
    bool operator<(const Entry &o) const { return value != o.value ? value < o.value : node < o.node; }
};

inline uint32_t empt_of(const uint64_t *ma, const uint64_t *mb) { return kmer_empt_of(ma, mb); }
inline void mask_of(const uint32_t *ranks, uint64_t *m) { kmer_mask_of(ranks, m); }

struct HeapEdge {
    float J;
    uint32_t u, v;
};
struct WorseEdge {  // std::priority_queue keeps the greatest on top: "less" = worse = smaller J, then larger u, then larger v
    bool operator()(const HeapEdge &a, const HeapEdge &b) const
    {
        if (a.J != b.J) return a.J < b.J;
        if (a.u != b.u) return a.u > b.u;
        return a.v > b.v;
    }
};

}  // namespace

polee_status kmer_validate_sketches(polee_ctx *ctx, int64_t n, const uint64_t *sk)
{
    std::atomic<int64_t> bad{-1};
    parallel_chunks((size_t)n, 4096, [&](size_t lo, size_t hi, unsigned) {
        for (size_t t = lo; t < hi; ++t)
            for (int b = 0; b < KMER_H; ++b) {
                const uint64_t v = sk[t * KMER_H + b];
                if (v != 0 && (v == ~0ull || (v - 1) % KMER_H != (uint64_t)b)) bad = (int64_t)t;
            }
    });
    if (bad >= 0)
        return fail(ctx, POLEE_ERR_BAD_ARG, "k-mer tree: sketch %lld holds a value outside its bin (a value v belongs in bin (v - 1) mod %d)",
                    (long long)bad.load(), KMER_H);
    return POLEE_OK;
}

polee_status kmer_index_host(int64_t n, const uint64_t *sk, KmerIndex &ix)
{
    ix.n = n;
    const size_t cells = (size_t)n * KMER_H;
    POLEE_TRY(kmer_validate_sketches(nullptr, n, sk));
    std::vector<size_t> cnt((size_t)n + 1, 0);
    parallel_chunks((size_t)n, 4096, [&](size_t lo, size_t hi, unsigned) {
        for (size_t t = lo; t < hi; ++t) {
            size_t c = 0;
            for (int b = 0; b < KMER_H; ++b) c += sk[t * KMER_H + b] != 0;
            cnt[t + 1] = c;
        }
    });
    for (size_t t = 0; t < (size_t)n; ++t) cnt[t + 1] += cnt[t];
    const size_t E = cnt[(size_t)n];
    std::vector<Entry> ent(E);
    parallel_chunks((size_t)n, 4096, [&](size_t lo, size_t hi, unsigned) {
        for (size_t t = lo; t < hi; ++t) {
            size_t o = cnt[t];
            for (int b = 0; b < KMER_H; ++b)
                if (sk[t * KMER_H + b]) ent[o++] = Entry{sk[t * KMER_H + b], (uint32_t)t};
        }
    });
    kmer_parallel_sort(ent);
    ix.ranks.assign(cells, KMER_EMPTY);
    ix.ent.resize(E);
    ix.run_start.clear();
    for (size_t i = 0; i < E; ++i) {
        if (i == 0 || ent[i].value != ent[i - 1].value) ix.run_start.push_back((uint32_t)i);
        ix.ent[i] = ent[i].node;
        ix.ranks[(size_t)ent[i].node * KMER_H + (size_t)((ent[i].value - 1) % KMER_H)] = (uint32_t)(ix.run_start.size() - 1);
    }
    ix.run_start.push_back((uint32_t)E);
    std::vector<Entry>().swap(ent);
    const size_t R = ix.run_start.size() - 1;
    uint64_t P = 0;
    for (size_t r = 0; r < R; ++r) {
        const uint64_t len = ix.run_start[r + 1] - ix.run_start[r];
        P += len * (len - 1) / 2;
    }
    if (P > (uint64_t)POLEE_KMER_MAX_PAIRS)
        return fail(nullptr, POLEE_ERR_BAD_ARG,
                    "k-mer tree: %llu co-occurring pairs of transcripts, more than POLEE_KMER_MAX_PAIRS = %llu (a k-mer shared by r transcripts "
                    "gives r (r - 1) / 2 of them: mask repeats, or exclude the transcripts that carry them)",
                    (unsigned long long)P, (unsigned long long)POLEE_KMER_MAX_PAIRS);
    std::vector<uint64_t> keys;
    keys.reserve((size_t)P);
    for (size_t r = 0; r < R; ++r)
        for (uint32_t a = ix.run_start[r]; a < ix.run_start[r + 1]; ++a)
            for (uint32_t b = a + 1; b < ix.run_start[r + 1]; ++b) keys.push_back(((uint64_t)(ix.ent[a] + 1) << 32) | (ix.ent[b] + 1));
    kmer_parallel_sort(keys);
    std::vector<uint64_t> masks((size_t)n * 4);
    parallel_chunks((size_t)n, 4096, [&](size_t lo, size_t hi, unsigned) {
        for (size_t t = lo; t < hi; ++t) mask_of(&ix.ranks[t * KMER_H], &masks[t * 4]);
    });
    ix.edges.clear();
    for (size_t i = 0; i < keys.size();) {
        size_t j = i + 1;
        while (j < keys.size() && keys[j] == keys[i]) ++j;
        const uint32_t u = (uint32_t)(keys[i] >> 32), v = (uint32_t)keys[i];
        ix.edges.push_back(KmerEdge{u, v, (uint32_t)(j - i), empt_of(&masks[(size_t)(u - 1) * 4], &masks[(size_t)(v - 1) * 4])});
        i = j;
    }
    return POLEE_OK;
}

polee_status kmer_tree_merge(KmerIndex &ix, int32_t *parents, int32_t *js)
{
    const int64_t n = ix.n;
    const size_t N = (size_t)(2 * n - 1);
    // nodes are 0-based here (transcripts 0 .. n-1, new nodes from n on in creation order): the same order as the definition's
    std::vector<uint32_t> left(N, 0), right(N, 0), height(N, 0);
    std::vector<uint8_t> active(N, 0);
    std::fill(active.begin(), active.begin() + n, 1);
    std::vector<uint64_t> masks((size_t)n * 4);
    masks.reserve(N * 4);
    for (size_t t = 0; t < (size_t)n; ++t) mask_of(&ix.ranks[t * KMER_H], &masks[t * 4]);
    std::vector<uint32_t> run_len(ix.run_start.size() - 1);
    for (size_t r = 0; r < run_len.size(); ++r) run_len[r] = ix.run_start[r + 1] - ix.run_start[r];
    std::vector<HeapEdge> first(ix.edges.size());
    for (size_t i = 0; i < first.size(); ++i) {
        const KmerEdge &e = ix.edges[i];
        first[i] = HeapEdge{(float)e.mat / (float)(KMER_H - (int)e.empt), e.u - 1, e.v - 1};
    }
    std::vector<KmerEdge>().swap(ix.edges);
    std::priority_queue<HeapEdge, std::vector<HeapEdge>, WorseEdge> heap(WorseEdge(), std::move(first));
    std::vector<uint32_t> count(N, 0), touched;
    size_t next = (size_t)n;
    while (!heap.empty()) {
        const HeapEdge e = heap.top();
        heap.pop();
        if (!active[e.u] || !active[e.v]) continue;  // (an endpoint was merged since: sketches never change, so nothing else goes stale)
        const uint32_t w = (uint32_t)next++;
        left[w] = e.u;
        right[w] = e.v;
        height[w] = 1 + std::max(height[e.u], height[e.v]);
        active[e.u] = active[e.v] = 0;
        active[w] = 1;
        ix.ranks.resize((size_t)(w + 1) * KMER_H);
        masks.resize((size_t)(w + 1) * 4);
        uint32_t *rw = &ix.ranks[(size_t)w * KMER_H];
        const uint32_t *ru = &ix.ranks[(size_t)e.u * KMER_H], *rv = &ix.ranks[(size_t)e.v * KMER_H];
        for (int b = 0; b < KMER_H; ++b) rw[b] = std::min(ru[b], rv[b]);
        mask_of(rw, &masks[(size_t)w * 4]);
        touched.clear();
        for (int b = 0; b < KMER_H; ++b) {
            if (rw[b] == KMER_EMPTY) continue;
            // the holders of this value: count the active ones, drop the merged ones (u or v is among them, so there is room
            // for w: the lists never grow)
            uint32_t *list = &ix.ent[ix.run_start[rw[b]]];
            uint32_t len = run_len[rw[b]], keep = 0;
            for (uint32_t i = 0; i < len; ++i) {
                const uint32_t x = list[i];
                if (!active[x]) continue;
                list[keep++] = x;
                if (count[x]++ == 0) touched.push_back(x);
            }
            list[keep++] = w;
            run_len[rw[b]] = keep;
        }
        for (uint32_t x : touched) {
            const uint32_t empt = empt_of(&masks[(size_t)x * 4], &masks[(size_t)w * 4]);
            heap.push(HeapEdge{(float)count[x] / (float)(KMER_H - (int)empt), x, w});
            count[x] = 0;
        }
    }
    return kmer_tree_finish(n, next, left, right, height, active, parents, js);
}

polee_status kmer_tree_finish(int64_t n, size_t next, std::vector<uint32_t> &left, std::vector<uint32_t> &right, std::vector<uint32_t> &height,
                              const std::vector<uint8_t> &active, int32_t *parents, int32_t *js)
{
    const size_t N = (size_t)(2 * n - 1);
    // Huffman phase (kmercluster.jl:245-254): the two nodes of smallest height, ties by node number; first popped = left
    typedef std::pair<uint32_t, uint32_t> HN;  // (height, node)
    std::priority_queue<HN, std::vector<HN>, std::greater<HN>> rest;
    for (size_t x = 0; x < next; ++x)
        if (active[x]) rest.push(HN(height[x], (uint32_t)x));
    while (rest.size() > 1) {
        const HN a = rest.top();
        rest.pop();
        const HN b = rest.top();
        rest.pop();
        const uint32_t w = (uint32_t)next++;
        left[w] = a.second;
        right[w] = b.second;
        height[w] = 1 + std::max(a.first, b.first);
        rest.push(HN(height[w], w));
    }
    // order_nodes (kmercluster.jl:69-93): DFS pre-order, right child first
    std::vector<std::pair<uint32_t, int32_t>> stack;
    stack.emplace_back(rest.top().second, 0);
    size_t out = 0;
    while (!stack.empty()) {
        const std::pair<uint32_t, int32_t> it = stack.back();
        stack.pop_back();
        const int32_t idx = (int32_t)++out;
        parents[idx - 1] = it.second;
        if ((int64_t)it.first < n) {
            js[idx - 1] = (int32_t)it.first + 1;
        } else {
            js[idx - 1] = 0;
            stack.emplace_back(left[it.first], idx);
            stack.emplace_back(right[it.first], idx);
        }
    }
    return out == N ? POLEE_OK : fail(nullptr, POLEE_ERR_UNSUPPORTED, "k-mer tree: %zu nodes written, %zu expected", out, N);
}

}  // namespace polee

using namespace polee;

extern "C" polee_status polee_kmer_sketch_host(int64_t n, const int64_t *offsets, const uint8_t *bases, uint64_t *sketches)
{
    return host_entry("polee_kmer_sketch_host", [&]() -> polee_status {
        if (n < 0 || !offsets || !sketches) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_kmer_sketch_host: null argument or negative n");
        for (int64_t t = 0; t < n; ++t)
            if (offsets[t] < 0 || offsets[t + 1] < offsets[t]) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_kmer_sketch_host: offsets must not decrease");
        if (n && offsets[n] > 0 && !bases) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_kmer_sketch_host: null bases");
        parallel_chunks((size_t)n, 64, [&](size_t lo, size_t hi, unsigned) {
            for (size_t t = lo; t < hi; ++t) sketch_one(bases + offsets[t], offsets[t + 1] - offsets[t], sketches + t * KMER_H);
        });
        return POLEE_OK;
    });
}

extern "C" polee_status polee_kmer_tree_host(int64_t n, const uint64_t *sketches, int32_t *node_parent_idxs, int32_t *node_js)
{
    return host_entry("polee_kmer_tree_host", [&]() -> polee_status {
        if (n < 1 || n > POLEE_KMER_MAX_N || !sketches || !node_parent_idxs || !node_js)
            return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_kmer_tree_host: null argument, or n outside 1 .. %lld", (long long)POLEE_KMER_MAX_N);
        KmerClock clk;
        KmerIndex ix;
        POLEE_TRY(kmer_index_host(n, sketches, ix));
        clk.lap("candidate edges (host)");
        POLEE_TRY(kmer_tree_merge(ix, node_parent_idxs, node_js));
        clk.lap("merge loop + DFS");
        return POLEE_OK;
    });
}
