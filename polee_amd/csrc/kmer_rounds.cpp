// polee fit-tree, merge in rounds, on the host threads: the twin of kmer_rounds_device.hip, pass for pass.
// Every edge has a priority (bits of J, a hash of its endpoints, the endpoints): a total order.  A round finds the best edge of
// every node (atomic maxima), merges the edges that are the best of both their endpoints, numbers the new nodes in the order of
// the priorities, and relabels the edges: untouched ones keep their key, the others are made canonical, de-duplicated and
// re-evaluated from the two rank rows.  Nothing depends on the order of the edge buffer, so nothing depends on the thread count.
#include <mutex>

#include "kmer_rounds.hpp"

namespace polee {
namespace {

constexpr size_t GRAIN = 16384;  // edges per chunk: a round with fewer runs on the calling thread

inline void atomic_max(std::atomic<uint64_t> &a, uint64_t v)
{
    uint64_t c = a.load(std::memory_order_relaxed);
    while (c < v && !a.compare_exchange_weak(c, v, std::memory_order_relaxed)) {
    }
}
inline void atomic_min(std::atomic<uint64_t> &a, uint64_t v)
{
    uint64_t c = a.load(std::memory_order_relaxed);
    while (c > v && !a.compare_exchange_weak(c, v, std::memory_order_relaxed)) {
    }
}

// a chunk's output staged in a small block and copied to its place in one piece: room claimed from a shared cursor
template <class T, int CAP = 512>
struct Stage {
    T buf[CAP];
    int fill = 0;
    T *out;
    std::atomic<size_t> &cursor;
    Stage(T *o, std::atomic<size_t> &c) : out(o), cursor(c) {}
    void push(const T &x)
    {
        buf[fill++] = x;
        if (fill == CAP) flush();
    }
    void flush()
    {
        if (!fill) return;
        const size_t at = cursor.fetch_add((size_t)fill, std::memory_order_relaxed);
        std::copy(buf, buf + fill, out + at);
        fill = 0;
    }
    ~Stage() { flush(); }
};

}  // namespace

void kmer_round_select_host(const KmerREdge *edges, size_t E, std::atomic<uint64_t> *bestkey, std::atomic<uint64_t> *besttie, std::vector<uint32_t> &chosen)
{
    parallel_chunks(E, GRAIN, [&](size_t lo, size_t hi, unsigned) {
        for (size_t e = lo; e < hi; ++e) {
            bestkey[edges[e].u].store(0, std::memory_order_relaxed);
            bestkey[edges[e].v].store(0, std::memory_order_relaxed);
            besttie[edges[e].u].store(~0ull, std::memory_order_relaxed);
            besttie[edges[e].v].store(~0ull, std::memory_order_relaxed);
        }
    });
    parallel_chunks(E, GRAIN, [&](size_t lo, size_t hi, unsigned) {
        for (size_t e = lo; e < hi; ++e) {
            atomic_max(bestkey[edges[e].u], edges[e].key);
            atomic_max(bestkey[edges[e].v], edges[e].key);
        }
    });
    parallel_chunks(E, GRAIN, [&](size_t lo, size_t hi, unsigned) {  // equal keys at a node: the smaller (lo, hi)
        for (size_t e = lo; e < hi; ++e) {
            const uint64_t pk = kmer_pack(edges[e].u, edges[e].v);
            if (bestkey[edges[e].u].load(std::memory_order_relaxed) == edges[e].key) atomic_min(besttie[edges[e].u], pk);
            if (bestkey[edges[e].v].load(std::memory_order_relaxed) == edges[e].key) atomic_min(besttie[edges[e].v], pk);
        }
    });
    chosen.clear();
    std::mutex mu;
    parallel_chunks(E, GRAIN, [&](size_t lo, size_t hi, unsigned) {
        uint32_t buf[256];
        int fill = 0;
        auto flush = [&] {
            std::lock_guard<std::mutex> g(mu);
            chosen.insert(chosen.end(), buf, buf + fill);
            fill = 0;
        };
        for (size_t e = lo; e < hi; ++e) {
            const KmerREdge &x = edges[e];
            const uint64_t pk = kmer_pack(x.u, x.v);
            if (bestkey[x.u].load(std::memory_order_relaxed) != x.key || bestkey[x.v].load(std::memory_order_relaxed) != x.key) continue;
            if (besttie[x.u].load(std::memory_order_relaxed) != pk || besttie[x.v].load(std::memory_order_relaxed) != pk) continue;
            buf[fill++] = (uint32_t)e;
            if (fill == 256) flush();
        }
        if (fill) flush();
    });
    std::sort(chosen.begin(), chosen.end(), [&](uint32_t a, uint32_t b) {  // larger key first, then the smaller (u, v)
        if (edges[a].key != edges[b].key) return edges[a].key > edges[b].key;
        return kmer_pack(edges[a].u, edges[a].v) < kmer_pack(edges[b].u, edges[b].v);
    });
}

polee_status kmer_tree_rounds_host(KmerIndex &ix, int32_t *parents, int32_t *js, KmerRoundsStats &st, KmerClock &clk)
{
    const int64_t n = ix.n;
    const size_t N = (size_t)(2 * n - 1);
    std::vector<uint32_t> left(N, 0), right(N, 0), height(N, 0), into(N);
    std::vector<uint8_t> active(N, 0);
    std::fill(active.begin(), active.begin() + n, 1);
    for (size_t x = 0; x < N; ++x) into[x] = (uint32_t)x;
    const size_t E0 = ix.edges.size();
    if (E0 >= 0xFFFFFFFFull) return fail(nullptr, POLEE_ERR_UNSUPPORTED, "k-mer tree (rounds): %zu candidate edges, at most 2^32 - 2 are indexed", E0);
    std::vector<KmerREdge> A(E0), B(E0);
    parallel_chunks(E0, GRAIN, [&](size_t lo, size_t hi, unsigned) {
        for (size_t i = lo; i < hi; ++i) {
            const KmerEdge &e = ix.edges[i];
            A[i] = KmerREdge{e.u - 1, e.v - 1, kmer_key(e.u - 1, e.v - 1, e.mat, e.empt)};
        }
    });
    std::vector<KmerEdge>().swap(ix.edges);
    std::vector<uint32_t>().swap(ix.ent);
    std::vector<uint32_t>().swap(ix.run_start);
    std::vector<uint64_t> masks;
    if (E0) {  // (rows are added by the round; the reservation is address space until then)
        ix.ranks.reserve(N * KMER_H);
        masks.reserve(N * 4);
    }
    masks.resize((size_t)n * 4);
    parallel_chunks((size_t)n, 4096, [&](size_t lo, size_t hi, unsigned) {
        for (size_t t = lo; t < hi; ++t) kmer_mask_of(&ix.ranks[t * KMER_H], &masks[t * 4]);
    });
    std::vector<std::atomic<uint64_t>> bestkey(E0 ? N : 0), besttie(E0 ? N : 0);
    std::vector<uint64_t> tk;
    tk.reserve(E0);
    std::vector<uint32_t> chosen;
    size_t EA = E0, next = (size_t)n;
    while (EA > 0) {
        kmer_round_select_host(A.data(), EA, bestkey.data(), besttie.data(), chosen);
        const size_t M = chosen.size();
        if (M == 0 || next + M > N) return fail(nullptr, POLEE_ERR_UNSUPPORTED, "k-mer tree (rounds): internal error: %zu merges with %zu nodes", M, next);
        ++st.rounds;
        st.merges += (int64_t)M;
        const size_t base = next;
        next += M;
        ix.ranks.resize(next * KMER_H);
        masks.resize(next * 4);
        parallel_chunks(M, 64, [&](size_t lo, size_t hi, unsigned) {
            for (size_t q = lo; q < hi; ++q) {
                const KmerREdge &e = A[chosen[q]];
                const uint32_t w = (uint32_t)(base + q);
                left[w] = e.u;
                right[w] = e.v;
                height[w] = 1 + std::max(height[e.u], height[e.v]);
                into[e.u] = into[e.v] = w;
                active[e.u] = active[e.v] = 0;
                active[w] = 1;
                uint32_t *rw = &ix.ranks[(size_t)w * KMER_H];
                const uint32_t *ru = &ix.ranks[(size_t)e.u * KMER_H], *rv = &ix.ranks[(size_t)e.v * KMER_H];
                for (int b = 0; b < KMER_H; ++b) rw[b] = std::min(ru[b], rv[b]);
                kmer_mask_of(rw, &masks[(size_t)w * 4]);
            }
        });
        // relabel: an edge inside one new node vanishes, an untouched one is kept as it is, the others give a pair to re-evaluate
        std::atomic<size_t> nkept{0}, ntouched{0};
        tk.resize(EA);
        parallel_chunks(EA, GRAIN, [&](size_t lo, size_t hi, unsigned) {
            Stage<KmerREdge> keep(B.data(), nkept);
            Stage<uint64_t> touch(tk.data(), ntouched);
            for (size_t i = lo; i < hi; ++i) {
                const KmerREdge &e = A[i];
                const uint32_t a = into[e.u], b = into[e.v];
                if (a == b) continue;
                if (a == e.u && b == e.v)
                    keep.push(e);
                else
                    touch.push(kmer_pack(std::min(a, b), std::max(a, b)));
            }
        });
        tk.resize(ntouched.load());
        kmer_parallel_sort(tk);
        tk.erase(std::unique(tk.begin(), tk.end()), tk.end());
        const size_t D = tk.size();
        st.reevaluated += (int64_t)D;
        size_t EB = nkept.load();
        if (EB + D > E0) return fail(nullptr, POLEE_ERR_UNSUPPORTED, "k-mer tree (rounds): internal error: the edge set grew (%zu + %zu > %zu)", EB, D, E0);
        parallel_chunks(D, 1024, [&](size_t lo, size_t hi, unsigned) {
            for (size_t i = lo; i < hi; ++i) {
                const uint32_t u = (uint32_t)(tk[i] >> 32), v = (uint32_t)tk[i];
                const uint32_t *ru = &ix.ranks[(size_t)u * KMER_H], *rv = &ix.ranks[(size_t)v * KMER_H];
                uint32_t mat = 0;
                for (int b = 0; b < KMER_H; ++b) mat += ru[b] == rv[b] && ru[b] != KMER_EMPTY;
                B[EB + i] = KmerREdge{u, v, mat ? kmer_key(u, v, mat, kmer_empt_of(&masks[(size_t)u * 4], &masks[(size_t)v * 4])) : 0};
            }
        });
        size_t o = EB;
        for (size_t i = EB; i < EB + D; ++i)  // (a pair whose shared values all lost their bins to smaller ones: mat = 0, no edge)
            if (B[i].key) B[o++] = B[i];
        A.swap(B);
        EA = o;
    }
    for (size_t x = 0; x < next; ++x) st.left += active[x];
    if (clk.on) {
        char what[64];
        snprintf(what, sizeof what, "rounds (%lld, host)", (long long)st.rounds);
        clk.lap(what);
    }
    POLEE_TRY(kmer_tree_finish(n, next, left, right, height, active, parents, js));
    clk.lap("Huffman + DFS");
    return POLEE_OK;
}

}  // namespace polee

using namespace polee;

extern "C" polee_status polee_kmer_tree_rounds_host(int64_t n, const uint64_t *sketches, int32_t *node_parent_idxs, int32_t *node_js, int64_t *stats)
{
    return host_entry("polee_kmer_tree_rounds_host", [&]() -> polee_status {
        if (n < 1 || n > POLEE_KMER_MAX_N || !sketches || !node_parent_idxs || !node_js)
            return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_kmer_tree_rounds_host: null argument, or n outside 1 .. %lld", (long long)POLEE_KMER_MAX_N);
        KmerClock clk;
        KmerIndex ix;
        POLEE_TRY(kmer_index_host(n, sketches, ix));
        clk.lap("index (host)");
        KmerRoundsStats st;
        POLEE_TRY(kmer_tree_rounds_host(ix, node_parent_idxs, node_js, st, clk));
        st.store(stats);
        return POLEE_OK;
    });
}
