// polee fit-tree, merge in rounds, on the device.  The same tree as kmer_rounds.cpp, node for node: priorities
// are a total order, new nodes are numbered in that order, J's bits come from one host-built table.  It starts from what
// kmer_index_device leaves on the device (ranks, masks, candidate edges); nothing of it is copied to the host.
//
// Per round, over the live edges (u, v, key):
//   best      atomic max of the key into bestkey[u], bestkey[v]; then, among the edges that hold a node's maximum, atomic min of the
//             packed (u, v) into besttie (equal 64-bit keys are rare, but part of the definition)
//   select    the edges that are the best of both endpoints are appended to the round's list and mark their endpoints; a counting
//             pass over the edges then tells kept from touched ones.  One read-back: {merges, kept, touched}.
//   order     the list sorted by priority (rocPRIM: by (u, v) ascending, then stably by key descending); the i-th gets node base + i
//   union     one wave per merge: per-bin minimum of the two rank rows, the emptiness mask by ballot
//   relabel   kept edges go to the other buffer as they are; a touched edge gives the canonical pair of its relabelled endpoints
//   re-evaluate  the pairs sorted; one wave per entry, the first of equal ones compares the two rank rows (ballot + popcount) and
//             appends the edge, or nothing where mat = 0
// The order of an edge buffer varies from run to run (appends through an atomic cursor); every consumer is an order-independent
// reduction or a sort by a total order, so the tree does not.  Integer atomics only.  The edge set never grows: two buffers of the
// initial size.  The number of live edges stays on the device: the next round's grids are sized by the bound kept + touched.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "kmer_rounds.hpp"

namespace polee {
namespace {

#define KR_HIP(expr) POLEE_HIP_TRY(ctx, expr)

// the counters of a round (two blocks, by the round's parity: a round reads the other block's `next`)
struct Counts {
    uint32_t merges, kept, touched, next;  // next: edges appended to the other buffer = the next round's live edges
    uint32_t tfill, overflow, pad0, pad1;  // tfill: pairs appended; overflow: an append beyond a buffer's room (never, by the argument)
};

struct Nodes {
    uint32_t *ranks;   // [rows][200]
    uint64_t *masks;   // [rows][4]
    uint32_t *into;    // merged node -> its new node, otherwise itself
    uint32_t *mround;  // the round (from 1) in which the node was merged, 0 = not yet
    uint32_t *mate;    // the node it was merged with
    uint32_t *left, *right, *height;
    uint8_t *active;
    unsigned long long *bestkey, *besttie;
};

inline unsigned grid_for(uint64_t count, unsigned per_block = 256) { return (unsigned)((count + per_block - 1) / per_block); }

// Where this lane's item goes when the lanes with `pred` append to a list: one atomic per wave.  Every lane of the wave calls it.
__device__ inline uint32_t wave_append(bool pred, uint32_t *cursor)
{
    const unsigned long long m = __ballot(pred);
    const int lane = (int)(threadIdx.x & 63u);
    const int leader = m ? __ffsll((long long)m) - 1 : 0;
    uint32_t base = 0;
    if (m && lane == leader) base = atomicAdd(cursor, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

__global__ void kr_first_edges_kernel(const KmerEdge *in, uint32_t E, const uint32_t *jt, KmerREdge *out)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const KmerEdge x = in[e];
    out[e] = KmerREdge{x.u - 1, x.v - 1, ((uint64_t)jt[x.mat * KMER_JT + x.empt] << 32) | kmer_h32(x.u, x.v)};
}
__global__ void kr_init_nodes_kernel(uint32_t N, uint32_t n, Nodes S)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= N) return;
    S.into[x] = x;
    S.mround[x] = 0;
    S.mate[x] = 0;
    S.left[x] = S.right[x] = S.height[x] = 0;
    S.active[x] = x < n ? 1 : 0;
    S.bestkey[x] = 0;
    S.besttie[x] = ~0ull;
}
__global__ void kr_best1_kernel(const KmerREdge *edges, uint32_t bound, const uint32_t *live, Nodes S)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= bound || e >= *live) return;
    const KmerREdge x = edges[e];
    atomicMax(&S.bestkey[x.u], (unsigned long long)x.key);
    atomicMax(&S.bestkey[x.v], (unsigned long long)x.key);
}
__global__ void kr_best2_kernel(const KmerREdge *edges, uint32_t bound, const uint32_t *live, Nodes S)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= bound || e >= *live) return;
    const KmerREdge x = edges[e];
    const unsigned long long pk = kmer_pack(x.u, x.v);
    if (S.bestkey[x.u] == x.key) atomicMin(&S.besttie[x.u], pk);
    if (S.bestkey[x.v] == x.key) atomicMin(&S.besttie[x.v], pk);
}
// sel_*: room for sel_cap merges (a node has one best edge, so the merges of a round share no endpoint: at most half the nodes)
__global__ void kr_select_kernel(const KmerREdge *edges, uint32_t bound, const uint32_t *live, Nodes S, uint32_t round, Counts *c, uint64_t *sel_key,
                                 uint64_t *sel_pack, uint32_t sel_cap, uint32_t *sel_edge)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = e < bound && e < *live;
    KmerREdge x{0, 0, 0};
    bool sel = false;
    if (in) {
        x = edges[e];
        const unsigned long long pk = kmer_pack(x.u, x.v);
        sel = S.bestkey[x.u] == x.key && S.bestkey[x.v] == x.key && S.besttie[x.u] == pk && S.besttie[x.v] == pk;
    }
    const uint32_t pos = wave_append(sel, &c->merges);
    if (!sel) return;
    if (pos >= sel_cap) {
        c->overflow = 1;
        return;
    }
    sel_key[pos] = x.key;
    sel_pack[pos] = kmer_pack(x.u, x.v);
    if (sel_edge) sel_edge[pos] = e;
    S.mround[x.u] = S.mround[x.v] = round;
    S.mate[x.u] = x.v;
    S.mate[x.v] = x.u;
}
// 0: kept as it is, 1: touched (an endpoint was merged, not with the other one), 2: inside one new node
__device__ inline int edge_fate(const KmerREdge &x, const Nodes &S, uint32_t round)
{
    const bool mu = S.mround[x.u] == round, mv = S.mround[x.v] == round;
    if (!mu && !mv) return 0;
    return (mu && S.mate[x.u] == x.v) ? 2 : 1;
}
__global__ void kr_count_kernel(const KmerREdge *edges, uint32_t bound, const uint32_t *live, Nodes S, uint32_t round, Counts *c)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    int fate = 2;
    if (e < bound && e < *live) fate = edge_fate(edges[e], S, round);
    const uint32_t k = (uint32_t)__popcll(__ballot(fate == 0)), t = (uint32_t)__popcll(__ballot(fate == 1));
    if ((threadIdx.x & 63u) == 0) {
        if (k) atomicAdd(&c->kept, k);
        if (t) atomicAdd(&c->touched, t);
    }
}
__global__ void kr_ids_kernel(uint32_t M, const uint64_t *sel_pack, uint32_t base, uint32_t N, Nodes S)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= M || base + q >= N) return;
    const uint32_t u = (uint32_t)(sel_pack[q] >> 32), v = (uint32_t)sel_pack[q], w = base + q;
    S.left[w] = u;
    S.right[w] = v;
    S.height[w] = 1 + max(S.height[u], S.height[v]);
    S.into[u] = S.into[v] = w;
    S.active[u] = S.active[v] = 0;
    S.active[w] = 1;
}
// one wave per merge: 200 ranks as three full strides of 64 and a tail of 8; an empty bin (all ones) loses every minimum
__global__ __launch_bounds__(256) void kr_union_kernel(uint32_t M, uint32_t base, uint32_t N, Nodes S)
{
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (q >= M || base + q >= N) return;
    const uint32_t w = base + q;
    const uint32_t *ru = S.ranks + (size_t)S.left[w] * KMER_H, *rv = S.ranks + (size_t)S.right[w] * KMER_H;
    uint32_t *rw = S.ranks + (size_t)w * KMER_H;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t b = 64u * (uint32_t)k + lane;
        const bool in = b < (uint32_t)KMER_H;
        uint32_t r = KMER_EMPTY;
        if (in) {
            r = min(ru[b], rv[b]);
            rw[b] = r;
        }
        const unsigned long long empty = __ballot(in && r == KMER_EMPTY);
        if (lane == 0) S.masks[(size_t)w * 4 + k] = empty;
    }
}
// kept edges to the other buffer (their endpoints' best is reset for the next round on the way); touched ones give a pair
__global__ void kr_relabel_kernel(const KmerREdge *edges, uint32_t bound, const uint32_t *live, Nodes S, uint32_t round, Counts *c, KmerREdge *out,
                                  uint32_t out_cap, uint64_t *pairs, uint32_t pairs_cap)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    int fate = 2;
    KmerREdge x{0, 0, 0};
    if (e < bound && e < *live) {
        x = edges[e];
        fate = edge_fate(x, S, round);
    }
    const uint32_t kp = wave_append(fate == 0, &c->next);
    const uint32_t tp = wave_append(fate == 1, &c->tfill);
    if (fate == 0) {
        if (kp >= out_cap) {
            c->overflow = 1;
            return;
        }
        out[kp] = x;
        S.bestkey[x.u] = S.bestkey[x.v] = 0;
        S.besttie[x.u] = S.besttie[x.v] = ~0ull;
    } else if (fate == 1) {
        if (tp >= pairs_cap) {
            c->overflow = 1;
            return;
        }
        const uint32_t a = S.into[x.u], b = S.into[x.v];
        pairs[tp] = kmer_pack(min(a, b), max(a, b));
    }
}
// pairs: sorted.  One wave per entry; the first of equal entries compares the two rows.
__global__ __launch_bounds__(256) void kr_reeval_kernel(const uint64_t *pairs, uint32_t T, uint32_t N, Nodes S, const uint32_t *jt, Counts *c, KmerREdge *out,
                                                        uint32_t out_cap, unsigned long long *reevaluated)
{
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= T) return;
    const uint64_t pk = pairs[i];
    if (i > 0 && pairs[i - 1] == pk) return;
    const uint32_t u = (uint32_t)(pk >> 32), v = (uint32_t)pk;
    if (u >= N || v >= N) return;
    const uint32_t *ru = S.ranks + (size_t)u * KMER_H, *rv = S.ranks + (size_t)v * KMER_H;
    uint32_t mat = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t b = 64u * (uint32_t)k + lane;
        bool same = false;
        if (b < (uint32_t)KMER_H) {
            const uint32_t a = ru[b];
            same = a == rv[b] && a != KMER_EMPTY;
        }
        mat += (uint32_t)__popcll(__ballot(same));
    }
    if (lane != 0) return;
    atomicAdd(reevaluated, 1ull);
    if (mat == 0) return;
    const uint64_t *mu = S.masks + (size_t)u * 4, *mv = S.masks + (size_t)v * 4;
    const uint32_t empt = __popcll(mu[0] & mv[0]) + __popcll(mu[1] & mv[1]) + __popcll(mu[2] & mv[2]) + __popcll(mu[3] & mv[3]);
    const uint32_t at = atomicAdd(&c->next, 1u);
    if (at >= out_cap) {
        c->overflow = 1;
        return;
    }
    out[at] = KmerREdge{u, v, ((uint64_t)jt[mat * KMER_JT + empt] << 32) | kmer_h32(u + 1, v + 1)};
    S.bestkey[u] = S.bestkey[v] = 0;
    S.besttie[u] = S.besttie[v] = ~0ull;
}

struct NodeBufs {
    DevBuf<uint32_t> into, mround, mate, left, right, height;
    DevBuf<uint8_t> active;
    DevBuf<unsigned long long> bestkey, besttie;
    polee_status alloc(polee_ctx *ctx, size_t N)
    {
        POLEE_TRY(into.alloc(ctx, N));
        POLEE_TRY(mround.alloc(ctx, N));
        POLEE_TRY(mate.alloc(ctx, N));
        POLEE_TRY(left.alloc(ctx, N));
        POLEE_TRY(right.alloc(ctx, N));
        POLEE_TRY(height.alloc(ctx, N));
        POLEE_TRY(active.alloc(ctx, N));
        POLEE_TRY(bestkey.alloc(ctx, N));
        POLEE_TRY(besttie.alloc(ctx, N));
        return POLEE_OK;
    }
    Nodes view(uint32_t *ranks, uint64_t *masks) { return Nodes{ranks, masks, into.p, mround.p, mate.p, left.p, right.p, height.p, active.p, bestkey.p, besttie.p}; }
};

// the round's list: selected edges, then ordered by priority
struct SelBufs {
    DevBuf<uint64_t> key, pack, key2, pack2;
    uint32_t cap = 0;
    polee_status alloc(polee_ctx *ctx, size_t c)
    {
        POLEE_TRY(key.alloc(ctx, c));
        POLEE_TRY(pack.alloc(ctx, c));
        POLEE_TRY(key2.alloc(ctx, c));
        POLEE_TRY(pack2.alloc(ctx, c));
        cap = (uint32_t)c;
        return POLEE_OK;
    }
};
size_t sort_pairs_bytes(size_t count, hipStream_t stream)
{
    size_t a = 0, b = 0;
    uint64_t *nil = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, a, nil, nil, nil, nil, count, 0, 64, stream);
    (void)rocprim::radix_sort_pairs_desc(nullptr, b, nil, nil, nil, nil, count, 0, 64, stream);
    return std::max(a, b);
}
size_t sort_keys_bytes(size_t count, hipStream_t stream)
{
    size_t a = 0;
    uint64_t *nil = nullptr;
    (void)rocprim::radix_sort_keys(nullptr, a, nil, nil, count, 0, 64, stream);
    return a;
}
// the M selected edges by descending priority; *pack_out: where the ordered (u, v) are (the input itself when M = 1)
polee_status order_selected(polee_ctx *ctx, DevScratch &tmp, SelBufs &sel, uint32_t M, const uint64_t **pack_out, const uint64_t **key_out)
{
    hipStream_t stream = ctx->stream;
    *pack_out = sel.pack.p;
    *key_out = sel.key.p;
    if (M < 2) return POLEE_OK;
    size_t bytes = 0;
    KR_HIP(rocprim::radix_sort_pairs(nullptr, bytes, sel.pack.p, sel.pack2.p, sel.key.p, sel.key2.p, (size_t)M, 0, 64, stream));
    KR_HIP(tmp.need(bytes ? bytes : 16));
    KR_HIP(rocprim::radix_sort_pairs(tmp.p, bytes, sel.pack.p, sel.pack2.p, sel.key.p, sel.key2.p, (size_t)M, 0, 64, stream));
    KR_HIP(rocprim::radix_sort_pairs_desc(nullptr, bytes, sel.key2.p, sel.key.p, sel.pack2.p, sel.pack.p, (size_t)M, 0, 64, stream));
    KR_HIP(tmp.need(bytes ? bytes : 16));
    KR_HIP(rocprim::radix_sort_pairs_desc(tmp.p, bytes, sel.key2.p, sel.key.p, sel.pack2.p, sel.pack.p, (size_t)M, 0, 64, stream));
    return POLEE_OK;
}

// best and select over E edges whose live count is *live; the round's counters c start as zero
void launch_select(hipStream_t stream, const KmerREdge *edges, uint32_t bound, const uint32_t *live, Nodes S, uint32_t round, Counts *c, SelBufs &sel,
                   uint32_t *sel_edge)
{
    kr_best1_kernel<<<grid_for(bound), 256, 0, stream>>>(edges, bound, live, S);
    kr_best2_kernel<<<grid_for(bound), 256, 0, stream>>>(edges, bound, live, S);
    kr_select_kernel<<<grid_for(bound), 256, 0, stream>>>(edges, bound, live, S, round, c, sel.key.p, sel.pack.p, sel.cap, sel_edge);
}

polee_status rounds_device(polee_ctx *ctx, int64_t n, KmerIndexDev &D, int32_t *parents, int32_t *js, KmerRoundsStats &st, KmerClock &clk)
{
    hipStream_t stream = ctx->stream;
    const size_t N = (size_t)(2 * n - 1);
    std::vector<uint32_t> left(N, 0), right(N, 0), height(N, 0);
    std::vector<uint8_t> active(N, 0);
    std::fill(active.begin(), active.begin() + n, 1);
    size_t next = (size_t)n;
    double t_small = 0;
    int64_t small_rounds = 0;
    if (D.NE > 0) {
        const uint32_t E0 = D.NE;
        DevScratch tmp(ctx);
        NodeBufs nb;
        SelBufs sel;
        DevBuf<KmerREdge> bufA, bufB;
        DevBuf<uint64_t> pairs, pairs2;
        DevBuf<uint32_t> jt;
        DevBuf<Counts> counts;
        DevBuf<unsigned long long> reeval;
        const size_t bytes = N * (6 * 4 + 1 + 2 * 8) + (size_t)E0 * (2 * sizeof(KmerREdge) + 2 * 8) + (size_t)n * 4 * 8;
        auto room = [&](polee_status s) {
            return s == POLEE_OK ? s
                                 : fail(ctx, POLEE_ERR_OOM, "k-mer tree (rounds): the node and edge arrays of %lld transcripts and %u candidate edges (%zu bytes, "
                                                            "besides %zu of ranks and masks) do not fit into the device's memory",
                                        (long long)n, E0, bytes, N * (KMER_H * 4 + 32));
        };
        POLEE_TRY(room(nb.alloc(ctx, N)));
        POLEE_TRY(room(sel.alloc(ctx, (size_t)n)));
        POLEE_TRY(room(bufA.alloc(ctx, E0)));
        POLEE_TRY(room(bufB.alloc(ctx, E0)));
        POLEE_TRY(room(pairs.alloc(ctx, E0)));
        POLEE_TRY(room(pairs2.alloc(ctx, E0)));
        POLEE_TRY(counts.alloc(ctx, 2));
        POLEE_TRY(reeval.alloc(ctx, 1));
        POLEE_TRY(jt.upload(ctx, kmer_jbits_table()));
        KR_HIP(tmp.need(std::max<size_t>(16, std::max(sort_pairs_bytes((size_t)n, stream), sort_keys_bytes(E0, stream)))));  // (no allocation per round)
        Nodes S = nb.view(D.ranks.p, D.masks.p);
        kr_init_nodes_kernel<<<grid_for(N), 256, 0, stream>>>((uint32_t)N, (uint32_t)n, S);
        kr_first_edges_kernel<<<grid_for(E0), 256, 0, stream>>>(D.edges.p, E0, jt.p, bufA.p);
        POLEE_KERNEL_CHECK(ctx);
        Counts start[2] = {};
        start[0].next = E0;  // (round 1 reads the block of parity 0)
        KR_HIP(hipMemcpyAsync(counts.p, start, sizeof start, hipMemcpyHostToDevice, stream));
        KR_HIP(hipMemsetAsync(reeval.p, 0, sizeof(unsigned long long), stream));
        KR_HIP(hipStreamSynchronize(stream));
        D.edges.release();
        KmerREdge *cur = bufA.p, *other = bufB.p;
        uint32_t bound = E0;
        for (uint32_t round = 1; bound > 0; ++round) {
            const double t0 = KmerClock::now();
            Counts *c = counts.p + (round & 1u);
            const uint32_t *live = &counts.p[(round & 1u) ^ 1u].next;
            KR_HIP(hipMemsetAsync(c, 0, sizeof(Counts), stream));
            launch_select(stream, cur, bound, live, S, round, c, sel, nullptr);
            kr_count_kernel<<<grid_for(bound), 256, 0, stream>>>(cur, bound, live, S, round, c);
            POLEE_KERNEL_CHECK(ctx);
            Counts h;
            KR_HIP(hipMemcpyAsync(&h, c, sizeof(Counts), hipMemcpyDeviceToHost, stream));
            KR_HIP(hipStreamSynchronize(stream));
            const uint32_t M = h.merges;
            if (M == 0) break;  // (the bound was not tight: no edge was left)
            if (h.overflow || next + M > N || (uint64_t)h.kept + h.touched > E0)
                return fail(ctx, POLEE_ERR_UNSUPPORTED, "k-mer tree (rounds, device): internal error in round %u: %u merges with %zu nodes, %u kept + %u touched of %u edges",
                            round, M, next, h.kept, h.touched, E0);
            ++st.rounds;
            st.merges += M;
            const uint64_t *pack_sorted, *key_sorted;
            POLEE_TRY(order_selected(ctx, tmp, sel, M, &pack_sorted, &key_sorted));
            const uint32_t base = (uint32_t)next;
            next += M;
            kr_ids_kernel<<<grid_for(M), 256, 0, stream>>>(M, pack_sorted, base, (uint32_t)N, S);
            kr_union_kernel<<<grid_for(M, 4), 256, 0, stream>>>(M, base, (uint32_t)N, S);
            kr_relabel_kernel<<<grid_for(bound), 256, 0, stream>>>(cur, bound, live, S, round, c, other, E0, pairs.p, E0);
            POLEE_KERNEL_CHECK(ctx);
            const uint32_t T = h.touched;
            const uint64_t *sorted = pairs.p;
            if (T > 1) {
                size_t b = 0;
                KR_HIP(rocprim::radix_sort_keys(nullptr, b, pairs.p, pairs2.p, (size_t)T, 0, 64, stream));
                KR_HIP(tmp.need(b ? b : 16));
                KR_HIP(rocprim::radix_sort_keys(tmp.p, b, pairs.p, pairs2.p, (size_t)T, 0, 64, stream));
                sorted = pairs2.p;
            }
            if (T > 0) {
                kr_reeval_kernel<<<grid_for(T, 4), 256, 0, stream>>>(sorted, T, (uint32_t)N, S, jt.p, c, other, E0, reeval.p);
                POLEE_KERNEL_CHECK(ctx);
            }
            std::swap(cur, other);
            bound = h.kept + T;
            if (clk.on && M < 64) {
                KR_HIP(hipStreamSynchronize(stream));
                t_small += KmerClock::now() - t0;
                ++small_rounds;
            }
        }
        unsigned long long re = 0;
        Counts last[2];
        KR_HIP(hipMemcpyAsync(&re, reeval.p, sizeof re, hipMemcpyDeviceToHost, stream));
        KR_HIP(hipMemcpyAsync(last, counts.p, sizeof last, hipMemcpyDeviceToHost, stream));
        KR_HIP(hipMemcpyAsync(left.data(), nb.left.p, next * 4, hipMemcpyDeviceToHost, stream));
        KR_HIP(hipMemcpyAsync(right.data(), nb.right.p, next * 4, hipMemcpyDeviceToHost, stream));
        KR_HIP(hipMemcpyAsync(height.data(), nb.height.p, next * 4, hipMemcpyDeviceToHost, stream));
        KR_HIP(hipMemcpyAsync(active.data(), nb.active.p, next, hipMemcpyDeviceToHost, stream));
        KR_HIP(hipStreamSynchronize(stream));
        if (last[0].overflow || last[1].overflow) return fail(ctx, POLEE_ERR_UNSUPPORTED, "k-mer tree (rounds, device): internal error: an edge buffer overflowed");
        st.reevaluated = (int64_t)re;
    }
    for (size_t x = 0; x < next; ++x) st.left += active[x];
    if (clk.on) {
        char what[96];
        snprintf(what, sizeof what, "rounds (%lld; %.4f s in %lld of < 64 merges)", (long long)st.rounds, t_small, (long long)small_rounds);
        clk.lap(what);
    }
    POLEE_TRY(kmer_tree_finish(n, next, left, right, height, active, parents, js));
    clk.lap("Huffman + DFS");
    return POLEE_OK;
}

polee_status tree_rounds_from_device_sketches(polee_ctx *ctx, int64_t n, const uint64_t *d_sk, int32_t *parents, int32_t *js, int64_t *stats, KmerClock &clk)
{
    KmerIndexDev D;
    POLEE_TRY(kmer_index_device(ctx, n, d_sk, nullptr, &D, (size_t)(2 * n - 1)));
    clk.lap("index (device)", ctx->stream, true);
    KmerRoundsStats st;
    POLEE_TRY(rounds_device(ctx, n, D, parents, js, st, clk));
    st.store(stats);
    return POLEE_OK;
}

// the debug entry's device half: edges 0-based; chosen: indexes into the edge array by descending priority
polee_status select_device(polee_ctx *ctx, uint32_t num_nodes, const std::vector<KmerREdge> &edges, std::vector<uint32_t> &chosen)
{
    hipStream_t stream = ctx->stream;
    const uint32_t E = (uint32_t)edges.size();
    chosen.clear();
    if (E == 0) return POLEE_OK;
    DevScratch tmp(ctx);
    NodeBufs nb;
    SelBufs sel;
    DevBuf<KmerREdge> d_edges;
    DevBuf<uint32_t> sel_edge, live;
    DevBuf<Counts> counts;
    POLEE_TRY(nb.alloc(ctx, num_nodes));
    POLEE_TRY(sel.alloc(ctx, E));
    POLEE_TRY(sel_edge.alloc(ctx, E));
    POLEE_TRY(counts.alloc(ctx, 1));
    POLEE_TRY(d_edges.upload(ctx, edges));
    POLEE_TRY(live.upload(ctx, &E, 1));
    Nodes S = nb.view(nullptr, nullptr);
    kr_init_nodes_kernel<<<grid_for(num_nodes), 256, 0, stream>>>(num_nodes, num_nodes, S);
    KR_HIP(hipMemsetAsync(counts.p, 0, sizeof(Counts), stream));
    launch_select(stream, d_edges.p, E, live.p, S, 1, counts.p, sel, sel_edge.p);
    POLEE_KERNEL_CHECK(ctx);
    Counts h;
    KR_HIP(hipMemcpyAsync(&h, counts.p, sizeof(Counts), hipMemcpyDeviceToHost, stream));
    KR_HIP(hipStreamSynchronize(stream));
    if (h.overflow || h.merges > E) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_kmer_round_select: more merges than edges (a pair listed twice?)");
    const uint32_t M = h.merges;
    if (M == 0) return POLEE_OK;
    // the order: the same two sorts as the rounds', then each ordered (u, v) is looked up among the selected edges
    std::vector<uint64_t> pack_unsorted(M), pack_sorted(M);
    std::vector<uint32_t> sedge(M);
    KR_HIP(hipMemcpyAsync(pack_unsorted.data(), sel.pack.p, (size_t)M * 8, hipMemcpyDeviceToHost, stream));
    POLEE_TRY(sel_edge.download(ctx, sedge.data(), M));
    const uint64_t *ps, *ks;
    POLEE_TRY(order_selected(ctx, tmp, sel, M, &ps, &ks));
    KR_HIP(hipMemcpyAsync(pack_sorted.data(), ps, (size_t)M * 8, hipMemcpyDeviceToHost, stream));
    KR_HIP(hipStreamSynchronize(stream));
    std::vector<std::pair<uint64_t, uint32_t>> byp(M);
    for (uint32_t i = 0; i < M; ++i) byp[i] = std::make_pair(pack_unsorted[i], sedge[i]);
    std::sort(byp.begin(), byp.end());
    for (uint32_t q = 0; q < M; ++q) {
        auto it = std::lower_bound(byp.begin(), byp.end(), std::make_pair(pack_sorted[q], 0u));
        if (it == byp.end() || it->first != pack_sorted[q]) return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_debug_kmer_round_select: internal error");
        chosen.push_back(it->second);
    }
    return POLEE_OK;
}

}  // namespace
}  // namespace polee

using namespace polee;

extern "C" polee_status polee_kmer_tree_rounds(polee_ctx *ctx, int64_t n, const uint64_t *sketches, int32_t *node_parent_idxs, int32_t *node_js, int64_t *stats)
{
    return ctx_entry(ctx, "polee_kmer_tree_rounds", [&]() -> polee_status {
        if (n < 1 || n > POLEE_KMER_MAX_N || !sketches || !node_parent_idxs || !node_js)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_kmer_tree_rounds: null argument, or n outside 1 .. %lld", (long long)POLEE_KMER_MAX_N);
        POLEE_TRY(kmer_validate_sketches(ctx, n, sketches));
        KmerClock clk;
        DevBuf<uint64_t> d_sk;
        POLEE_TRY(d_sk.upload(ctx, sketches, (size_t)n * KMER_H));
        clk.lap("upload");
        return tree_rounds_from_device_sketches(ctx, n, d_sk.p, node_parent_idxs, node_js, stats, clk);
    });
}

extern "C" polee_status polee_fit_tree_rounds(polee_ctx *ctx, int64_t n, const int64_t *offsets, const uint8_t *bases, int32_t *node_parent_idxs,
                                              int32_t *node_js, int64_t *stats)
{
    return ctx_entry(ctx, "polee_fit_tree_rounds", [&]() -> polee_status {
        POLEE_TRY(kmer_check_offsets(ctx, n, offsets, bases, "polee_fit_tree_rounds"));
        if (!node_parent_idxs || !node_js) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_fit_tree_rounds: null output");
        KmerClock clk;
        DevBuf<uint64_t> d_sk;
        POLEE_TRY(kmer_sketch_device(ctx, n, offsets, bases, d_sk, clk));
        return tree_rounds_from_device_sketches(ctx, n, d_sk.p, node_parent_idxs, node_js, stats, clk);
    });
}

// (a context or null = the selection on the host threads: host_entry, not ctx_entry, and the device branch selects the device itself)
extern "C" polee_status polee_debug_kmer_round_select(polee_ctx *ctx, int64_t num_nodes, int64_t E, const uint32_t *u, const uint32_t *v, const uint64_t *key,
                                                      uint8_t *merged_flags, int32_t *order)
{
    return host_entry("polee_debug_kmer_round_select", [&]() -> polee_status {
        if (num_nodes < 1 || num_nodes > 2 * POLEE_KMER_MAX_N || E < 0 || E >= (1LL << 31) || (E && (!u || !v || !key || !merged_flags || !order)))
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_kmer_round_select: null argument, or a count out of range");
        std::vector<KmerREdge> edges((size_t)E);
        for (int64_t e = 0; e < E; ++e) {
            if (u[e] < 1 || u[e] >= v[e] || (int64_t)v[e] > num_nodes || key[e] == 0)
                return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_kmer_round_select: edge %lld: nodes must be 1 <= u < v <= num_nodes, the key non-zero", (long long)e);
            edges[(size_t)e] = KmerREdge{u[e] - 1, v[e] - 1, key[e]};
            merged_flags[e] = 0;
            order[e] = -1;
        }
        std::vector<uint32_t> chosen;
        if (ctx) {
            POLEE_TRY(use_device(ctx));
            POLEE_TRY(select_device(ctx, (uint32_t)num_nodes, edges, chosen));
        } else {
            std::vector<std::atomic<uint64_t>> bestkey((size_t)num_nodes), besttie((size_t)num_nodes);
            kmer_round_select_host(edges.data(), edges.size(), bestkey.data(), besttie.data(), chosen);
        }
        for (size_t q = 0; q < chosen.size(); ++q) {
            merged_flags[chosen[q]] = 1;
            order[chosen[q]] = (int32_t)q;
        }
        return POLEE_OK;
    });
}
