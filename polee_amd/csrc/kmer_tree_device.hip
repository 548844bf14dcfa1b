// polee fit-tree on the device: the sketch kernel -- one-permutation MinHash of every transcript's canonical
// 32-mers, reduced in LDS -- and the candidate edges of a set of sketches: one radix sort of the (value, node) entries (a value
// determines its bin, so a run of equal values is the set of nodes that agree in that bin), r (r - 1) / 2 pair keys per run,
// a second sort, and a run-length encoding whose counts are the pairs' mat.  The merge loop itself is the host's
// (kmer_tree.cpp): it takes the same KmerIndex from here as from its own host-only set-up.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "kmer_tree.hpp"

namespace polee {
namespace {

#define KT_HIP(expr) POLEE_HIP_TRY(ctx, expr)
// a rocPRIM call: once for the size of its temporary storage, once for the work
#define KT_PRIM(call_with_tmp_bytes)                          \
    do {                                                      \
        size_t bytes = 0;                                     \
        void *tmp_p = nullptr;                                \
        KT_HIP(call_with_tmp_bytes);                          \
        KT_HIP(tmp.need(bytes ? bytes : 16));                 \
        tmp_p = tmp.p;                                        \
        KT_HIP(call_with_tmp_bytes);                          \
    } while (0)

constexpr int SK_THREADS = 256;
constexpr int SK_CHUNK = POLEE_KMER_SKETCH_CHUNK;  // windows per workgroup
constexpr int SK_MIN_S = 8;                        // fewest windows a lane rolls over (it reads 31 bases before its first)
static_assert(SK_CHUNK % SK_THREADS == 0, "a lane's share of a full chunk is a whole number of windows");

struct SketchWG {
    uint32_t t0, t1;  // transcripts [t0, t1): whole ones packed together, or one piece of a long one (split)
    uint32_t split, pad;
    int64_t w0, w1;  // split: windows [w0, w1) of transcript t0
};

__device__ inline uint64_t mix64(uint64_t c)
{
    uint64_t z = c + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Every lane rolls fw / bw over its own stretch of S consecutive windows (S + 31 bases, read as aligned 16-byte words: a
// transcript starts anywhere); the minima meet in a 1.6 KB LDS sketch.  A workgroup that holds whole transcripts stores the
// sketch; the pieces of a transcript longer than SK_CHUNK windows meet in global memory by 64-bit atomic minima, at most 200
// per workgroup.  `out` starts as all ones, the neutral element; kmer_finalize_kernel turns what is left of them into 0.
__global__ __launch_bounds__(SK_THREADS) void kmer_sketch_kernel(const uint8_t *__restrict__ bases, const int64_t *__restrict__ offsets,
                                                                 const SketchWG *__restrict__ plan, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long lds[KMER_H];
    const SketchWG wg = plan[blockIdx.x];
    for (uint32_t t = wg.t0; t < wg.t1; ++t) {
        const int64_t beg = offsets[t], len = offsets[t + 1] - beg;
        const int64_t w0 = wg.split ? wg.w0 : 0, w1 = wg.split ? wg.w1 : len - (KMER_K - 1);
        if (w1 <= w0) continue;  // (the same for the whole workgroup)
        for (int b = threadIdx.x; b < KMER_H; b += SK_THREADS) lds[b] = ~0ull;
        __syncthreads();
        const int64_t nw = w1 - w0;
        const int S = max(SK_MIN_S, (int)((nw + SK_THREADS - 1) / SK_THREADS));
        const int64_t a = w0 + (int64_t)threadIdx.x * S, e = min(w1, a + S);
        if (a < e) {
            const int64_t g0 = beg + a, g1 = beg + e + (KMER_K - 1);  // this lane's bases; g1 <= beg + len
            uint64_t fw = 0, bw = 0;
            int run = 0;  // valid bases in a row, ending here
            for (int64_t word = g0 & ~(int64_t)15; word < g1; word += 16) {
                const uint4 q = *reinterpret_cast<const uint4 *>(bases + word);
                const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int64_t pos = word + i;
                    if (pos < g0 || pos >= g1) continue;
                    const uint32_t c = (qw[i >> 2] >> (8 * (i & 3))) & 0xDFu;
                    const bool ok = c == 'A' || c == 'C' || c == 'G' || c == 'T';
                    const uint64_t code = ok ? ((c >> 1) ^ (c >> 2)) & 3u : 0u;
                    fw = (fw << 2) | code;
                    bw = (bw >> 2) | ((3 - code) << 62);
                    run = ok ? min(run + 1, KMER_K) : 0;
                    if (run == KMER_K && pos - g0 >= KMER_K - 1) {
                        const uint64_t c64 = fw < bw ? fw : bw, hh = mix64(c64), h = hh < ~0ull - 2 ? hh : ~0ull - 2;
                        const int b = (int)(h % KMER_H);
                        if (h + 1 < __hip_atomic_load(&lds[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMin(&lds[b], h + 1);
                    }
                }
            }
        }
        __syncthreads();
        for (int b = threadIdx.x; b < KMER_H; b += SK_THREADS) {
            const unsigned long long v = lds[b];
            if (!wg.split)
                out[(size_t)t * KMER_H + b] = v;
            else if (v != ~0ull)
                atomicMin(&out[(size_t)t * KMER_H + b], v);
        }
        __syncthreads();
    }
}

__global__ void kmer_finalize_kernel(unsigned long long *out, size_t cells)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cells && out[i] == ~0ull) out[i] = 0;
}

__global__ void kmer_iota_node_kernel(uint32_t *node, size_t cells)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cells) node[i] = (uint32_t)(i / KMER_H);
}

// sorted keys: the empty entries come first; *zeros = how many (it starts as 0: no empty entry leaves it there)
__global__ void kmer_zero_end_kernel(const uint64_t *key, size_t cells, uint32_t *zeros)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cells && key[i] == 0 && (i + 1 == cells || key[i + 1] != 0)) *zeros = (uint32_t)(i + 1);
}

__global__ void kmer_head_kernel(const uint64_t *key, uint32_t E, uint32_t *head)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < E) head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}

// incl: inclusive scan of the head flags.  ranks [n][200] starts as KMER_EMPTY; run_start has E + 1 entries
__global__ void kmer_rank_kernel(const uint64_t *key, const uint32_t *node, const uint32_t *head, const uint32_t *incl, uint32_t E,
                                 uint32_t *ranks, uint32_t *run_start)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    const uint32_t r = incl[i] - 1;
    ranks[(size_t)node[i] * KMER_H + (uint32_t)((key[i] - 1) % KMER_H)] = r;
    if (head[i]) run_start[r] = i;
    if (i + 1 == E) run_start[r + 1] = E;
}

__global__ void kmer_pair_count_kernel(const uint32_t *run_start, uint32_t R, uint64_t *pc)  // pc [R + 1], the last one 0
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > R) return;
    const uint64_t len = r < R ? run_start[r + 1] - run_start[r] : 0;
    pc[r] = len * (len - (len ? 1 : 0)) / 2;
}

// pair p of all: the run it belongs to by binary search in the scanned counts, then (a < b) within the run from the
// triangular numbering q = b (b - 1) / 2 + a.  The nodes of a run ascend (a stable sort of entries made in node order).
__global__ void kmer_pair_emit_kernel(const uint32_t *run_start, const uint64_t *poff, uint32_t R, const uint32_t *ent, uint64_t P, uint64_t *keys)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    uint32_t lo = 0, hi = R;  // the last r in [0, R) with poff[r] <= p
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (poff[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    const uint64_t q = p - poff[lo];
    uint64_t b = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)q)) * 0.5);
    while (b * (b - 1) / 2 > q) --b;
    while ((b + 1) * b / 2 <= q) ++b;
    const uint64_t a = q - b * (b - 1) / 2;
    const uint32_t s = run_start[lo];
    keys[p] = ((uint64_t)(ent[s + a] + 1) << 32) | (uint64_t)(ent[s + b] + 1);
}

__global__ void kmer_mask_kernel(const uint32_t *ranks, size_t n, uint64_t *masks)  // masks [n][4], bit b: bin b is empty
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * 4) return;
    const size_t t = i >> 2;
    const int w = (int)(i & 3);
    uint64_t m = 0;
    for (int b = w * 64; b < min(KMER_H, w * 64 + 64); ++b)
        if (ranks[t * KMER_H + b] == KMER_EMPTY) m |= 1ull << (b & 63);
    masks[i] = m;
}

__global__ void kmer_edge_kernel(const uint64_t *uniq, const uint32_t *counts, uint32_t NE, const uint64_t *masks, KmerEdge *edges)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NE) return;
    const uint32_t u = (uint32_t)(uniq[i] >> 32), v = (uint32_t)uniq[i];
    const uint64_t *ma = masks + (size_t)(u - 1) * 4, *mb = masks + (size_t)(v - 1) * 4;
    const uint32_t empt = __popcll(ma[0] & mb[0]) + __popcll(ma[1] & mb[1]) + __popcll(ma[2] & mb[2]) + __popcll(ma[3] & mb[3]);
    edges[i] = KmerEdge{u, v, counts[i], empt};
}

inline unsigned blocks_for(uint64_t count) { return (unsigned)((count + 255) / 256); }

}  // namespace

polee_status kmer_check_offsets(polee_ctx *ctx, int64_t n, const int64_t *offsets, const uint8_t *bases, const char *who)
{
    if (n < 1 || n > POLEE_KMER_MAX_N || !offsets) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: null offsets, or n outside 1 .. %lld", who, (long long)POLEE_KMER_MAX_N);
    if (offsets[0] != 0) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: offsets[0] must be 0", who);
    for (int64_t t = 0; t < n; ++t)
        if (offsets[t + 1] < offsets[t]) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: offsets must not decrease (transcript %lld)", who, (long long)t);
    if (offsets[n] > 0 && !bases) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: null bases", who);
    return POLEE_OK;
}

// sketches of n transcripts into d_sk [n][200], queued on the context's stream
polee_status kmer_sketch_device(polee_ctx *ctx, int64_t n, const int64_t *offsets, const uint8_t *bases, DevBuf<uint64_t> &d_sk, KmerClock &clk)
{
    hipStream_t stream = ctx->stream;
    const size_t cells = (size_t)n * KMER_H, total = (size_t)offsets[n];
    // the plan: whole transcripts packed up to SK_CHUNK windows per workgroup, longer ones cut into pieces of SK_CHUNK
    std::vector<SketchWG> plan;
    SketchWG pack{0, 0, 0, 0, 0, 0};
    int64_t packed = 0;
    auto flush = [&](uint32_t next) {
        if (packed > 0) plan.push_back(pack);
        pack.t0 = pack.t1 = next;
        packed = 0;
    };
    for (int64_t t = 0; t < n; ++t) {
        const int64_t nw = std::max<int64_t>(0, offsets[t + 1] - offsets[t] - (KMER_K - 1));
        if (nw > SK_CHUNK) {
            flush((uint32_t)t + 1);
            for (int64_t w = 0; w < nw; w += SK_CHUNK) plan.push_back(SketchWG{(uint32_t)t, (uint32_t)t + 1, 1, 0, w, std::min(nw, w + SK_CHUNK)});
            continue;
        }
        if (packed + nw > SK_CHUNK) flush((uint32_t)t);
        pack.t1 = (uint32_t)t + 1;
        packed += nw;
    }
    flush((uint32_t)n);
    DevBuf<uint8_t> d_bases;
    DevBuf<int64_t> d_off;
    DevBuf<SketchWG> d_plan;
    POLEE_TRY(d_bases.alloc(ctx, total + 32));  // (lanes read whole aligned 16-byte words: the last one may reach past the last base)
    if (total) KT_HIP(hipMemcpyAsync(d_bases.p, bases, total, hipMemcpyHostToDevice, stream));
    KT_HIP(hipMemsetAsync(d_bases.p + total, 0, 32, stream));
    POLEE_TRY(d_off.upload(ctx, offsets, (size_t)n + 1));
    if (!plan.empty()) POLEE_TRY(d_plan.upload(ctx, plan));
    POLEE_TRY(d_sk.alloc(ctx, cells));
    clk.lap("upload", stream, true);
    KT_HIP(hipMemsetAsync(d_sk.p, 0xFF, cells * sizeof(uint64_t), stream));
    if (!plan.empty()) {
        kmer_sketch_kernel<<<(unsigned)plan.size(), SK_THREADS, 0, stream>>>(d_bases.p, d_off.p, d_plan.p, (unsigned long long *)d_sk.p);
        POLEE_KERNEL_CHECK(ctx);
    }
    kmer_finalize_kernel<<<blocks_for(cells), 256, 0, stream>>>((unsigned long long *)d_sk.p, cells);
    POLEE_KERNEL_CHECK(ctx);
    KT_HIP(hipStreamSynchronize(stream));  // (the bases, offsets and plan go out of scope here)
    clk.lap("sketch kernel");
    return POLEE_OK;
}

// the index of the sketches d_sk [n][200] (valid ones: a value in its bin), from the device.  host: the greedy merge loop's copy
// (ranks, holder lists, edges); keep: what the rounds go on with where it is (ranks and masks with room for `rows` nodes, edges) --
// then nothing is copied to the host.
polee_status kmer_index_device(polee_ctx *ctx, int64_t n, const uint64_t *d_sk, KmerIndex *host, KmerIndexDev *keep, size_t rows)
{
    hipStream_t stream = ctx->stream;
    const size_t cells = (size_t)n * KMER_H;
    DevScratch tmp(ctx);
    KmerIndex none;
    KmerIndex &ix = host ? *host : none;
    KmerIndexDev mine;
    KmerIndexDev &D = keep ? *keep : mine;
    DevBuf<uint32_t> &ranks = D.ranks;
    DevBuf<uint64_t> &masks = D.masks;
    DevBuf<KmerEdge> &edges = D.edges;
    D.NE = 0;
    rows = std::max(rows, (size_t)n);
    ix.n = n;
    ix.edges.clear();
    DevBuf<uint64_t> key_s;
    DevBuf<uint32_t> node_in, node_s, d_count;
    POLEE_TRY(key_s.alloc(ctx, cells));
    POLEE_TRY(node_in.alloc(ctx, cells));
    POLEE_TRY(node_s.alloc(ctx, cells));
    POLEE_TRY(d_count.alloc(ctx, 4));
    KT_HIP(hipMemsetAsync(d_count.p, 0, 4 * sizeof(uint32_t), stream));
    kmer_iota_node_kernel<<<blocks_for(cells), 256, 0, stream>>>(node_in.p, cells);
    POLEE_KERNEL_CHECK(ctx);
    KT_PRIM(rocprim::radix_sort_pairs(tmp_p, bytes, d_sk, key_s.p, node_in.p, node_s.p, cells, 0, 64, stream));
    node_in.release();
    kmer_zero_end_kernel<<<blocks_for(cells), 256, 0, stream>>>(key_s.p, cells, d_count.p);
    POLEE_KERNEL_CHECK(ctx);
    uint32_t Z = 0;
    POLEE_TRY(d_count.download(ctx, &Z, 1));
    const uint32_t E = (uint32_t)(cells - Z);
    if (host) {
        ix.ranks.assign(cells, KMER_EMPTY);
        ix.ent.resize(E);
    }
    ix.run_start.assign(1, 0);
    if (E == 0) return POLEE_OK;
    const uint64_t *key = key_s.p + Z;
    const uint32_t *ent = node_s.p + Z;
    DevBuf<uint32_t> head, incl, run_start;
    POLEE_TRY(head.alloc(ctx, E));
    POLEE_TRY(incl.alloc(ctx, E));
    if (ranks.alloc(ctx, rows * KMER_H) != POLEE_OK)
        return fail(ctx, POLEE_ERR_OOM, "k-mer tree: the ranks of %zu nodes (%zu bytes) do not fit into the device's memory", rows, rows * KMER_H * sizeof(uint32_t));
    POLEE_TRY(run_start.alloc(ctx, (size_t)E + 1));
    KT_HIP(hipMemsetAsync(ranks.p, 0xFF, cells * sizeof(uint32_t), stream));
    kmer_head_kernel<<<blocks_for(E), 256, 0, stream>>>(key, E, head.p);
    POLEE_KERNEL_CHECK(ctx);
    KT_PRIM(rocprim::inclusive_scan(tmp_p, bytes, head.p, incl.p, (size_t)E, rocprim::plus<uint32_t>(), stream));
    kmer_rank_kernel<<<blocks_for(E), 256, 0, stream>>>(key, ent, head.p, incl.p, E, ranks.p, run_start.p);
    POLEE_KERNEL_CHECK(ctx);
    uint32_t R = 0;
    KT_HIP(hipMemcpyAsync(&R, incl.p + (E - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    KT_HIP(hipStreamSynchronize(stream));
    head.release();
    incl.release();
    if (host) {
        ix.run_start.resize((size_t)R + 1);
        POLEE_TRY(ranks.download(ctx, ix.ranks.data(), cells));
        POLEE_TRY(run_start.download(ctx, ix.run_start.data(), (size_t)R + 1));
        KT_HIP(hipMemcpyAsync(ix.ent.data(), ent, (size_t)E * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        KT_HIP(hipStreamSynchronize(stream));
    }
    key_s.release();
    // count before allocating
    DevBuf<uint64_t> pc, poff;
    POLEE_TRY(pc.alloc(ctx, (size_t)R + 1));
    POLEE_TRY(poff.alloc(ctx, (size_t)R + 1));
    kmer_pair_count_kernel<<<blocks_for((uint64_t)R + 1), 256, 0, stream>>>(run_start.p, R, pc.p);
    POLEE_KERNEL_CHECK(ctx);
    KT_PRIM(rocprim::exclusive_scan(tmp_p, bytes, pc.p, poff.p, (uint64_t)0, (size_t)R + 1, rocprim::plus<uint64_t>(), stream));
    uint64_t P = 0;
    KT_HIP(hipMemcpyAsync(&P, poff.p + R, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    KT_HIP(hipStreamSynchronize(stream));
    pc.release();
    if (P > (uint64_t)POLEE_KMER_MAX_PAIRS)
        return fail(ctx, POLEE_ERR_BAD_ARG,
                    "k-mer tree: %llu co-occurring pairs of transcripts, more than POLEE_KMER_MAX_PAIRS = %llu (a k-mer shared by r transcripts "
                    "gives r (r - 1) / 2 of them: mask repeats, or exclude the transcripts that carry them)",
                    (unsigned long long)P, (unsigned long long)POLEE_KMER_MAX_PAIRS);
    if (P == 0) return POLEE_OK;
    DevBuf<uint64_t> pk, pk_s, uniq;
    DevBuf<uint32_t> counts;
    POLEE_TRY(pk.alloc(ctx, (size_t)P));
    POLEE_TRY(pk_s.alloc(ctx, (size_t)P));
    kmer_pair_emit_kernel<<<blocks_for(P), 256, 0, stream>>>(run_start.p, poff.p, R, ent, P, pk.p);
    POLEE_KERNEL_CHECK(ctx);
    KT_PRIM(rocprim::radix_sort_keys(tmp_p, bytes, pk.p, pk_s.p, (size_t)P, 0, 64, stream));
    pk.release();
    POLEE_TRY(uniq.alloc(ctx, (size_t)P));
    POLEE_TRY(counts.alloc(ctx, (size_t)P));
    KT_PRIM(rocprim::run_length_encode(tmp_p, bytes, pk_s.p, (unsigned int)P, uniq.p, counts.p, d_count.p + 1, stream));
    POLEE_TRY(masks.alloc(ctx, rows * 4));
    kmer_mask_kernel<<<blocks_for((uint64_t)n * 4), 256, 0, stream>>>(ranks.p, (size_t)n, masks.p);
    POLEE_KERNEL_CHECK(ctx);
    uint32_t NE = 0;
    KT_HIP(hipMemcpyAsync(&NE, d_count.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    KT_HIP(hipStreamSynchronize(stream));
    pk_s.release();
    POLEE_TRY(edges.alloc(ctx, NE));
    kmer_edge_kernel<<<blocks_for(NE), 256, 0, stream>>>(uniq.p, counts.p, NE, masks.p, edges.p);
    POLEE_KERNEL_CHECK(ctx);
    D.NE = NE;
    if (host) {
        ix.edges.resize(NE);
        POLEE_TRY(edges.download(ctx, ix.edges.data(), NE));
    } else {
        KT_HIP(hipStreamSynchronize(stream));  // (uniq and counts go out of scope here)
    }
    return POLEE_OK;
}

namespace {

polee_status tree_from_device_sketches(polee_ctx *ctx, int64_t n, const uint64_t *d_sk, int32_t *parents, int32_t *js, KmerClock &clk)
{
    KmerIndex ix;
    POLEE_TRY(kmer_index_device(ctx, n, d_sk, &ix, nullptr, (size_t)n));
    clk.lap("candidate edges (device)");
    POLEE_TRY(kmer_tree_merge(ix, parents, js));
    clk.lap("merge loop + DFS");
    return POLEE_OK;
}

// (a null context: the host's index)
polee_status index_any(polee_ctx *ctx, const char *what, int64_t n, const uint64_t *sketches, KmerIndex &ix)
{
    if (n < 1 || n > POLEE_KMER_MAX_N || !sketches) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: null sketches, or n outside 1 .. %lld", what, (long long)POLEE_KMER_MAX_N);
    if (!ctx) return kmer_index_host(n, sketches, ix);
    POLEE_TRY(use_device(ctx));
    POLEE_TRY(kmer_validate_sketches(ctx, n, sketches));
    DevBuf<uint64_t> d_sk;
    POLEE_TRY(d_sk.upload(ctx, sketches, (size_t)n * KMER_H));
    return kmer_index_device(ctx, n, d_sk.p, &ix, nullptr, (size_t)n);
}

}  // namespace
}  // namespace polee

using namespace polee;

extern "C" polee_status polee_kmer_sketch(polee_ctx *ctx, int64_t n, const int64_t *offsets, const uint8_t *bases, uint64_t *sketches)
{
    return ctx_entry(ctx, "polee_kmer_sketch", [&]() -> polee_status {
        POLEE_TRY(kmer_check_offsets(ctx, n, offsets, bases, "polee_kmer_sketch"));
        if (!sketches) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_kmer_sketch: null output");
        KmerClock clk;
        DevBuf<uint64_t> d_sk;
        POLEE_TRY(kmer_sketch_device(ctx, n, offsets, bases, d_sk, clk));
        return d_sk.download(ctx, sketches, (size_t)n * KMER_H);
    });
}

extern "C" polee_status polee_kmer_tree(polee_ctx *ctx, int64_t n, const uint64_t *sketches, int32_t *node_parent_idxs, int32_t *node_js)
{
    return ctx_entry(ctx, "polee_kmer_tree", [&]() -> polee_status {
        if (n < 1 || n > POLEE_KMER_MAX_N || !sketches || !node_parent_idxs || !node_js)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_kmer_tree: null argument, or n outside 1 .. %lld", (long long)POLEE_KMER_MAX_N);
        POLEE_TRY(kmer_validate_sketches(ctx, n, sketches));
        KmerClock clk;
        DevBuf<uint64_t> d_sk;
        POLEE_TRY(d_sk.upload(ctx, sketches, (size_t)n * KMER_H));
        clk.lap("upload");
        return tree_from_device_sketches(ctx, n, d_sk.p, node_parent_idxs, node_js, clk);
    });
}

extern "C" polee_status polee_fit_tree(polee_ctx *ctx, int64_t n, const int64_t *offsets, const uint8_t *bases, int32_t *node_parent_idxs, int32_t *node_js)
{
    return ctx_entry(ctx, "polee_fit_tree", [&]() -> polee_status {
        POLEE_TRY(kmer_check_offsets(ctx, n, offsets, bases, "polee_fit_tree"));
        if (!node_parent_idxs || !node_js) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_fit_tree: null output");
        KmerClock clk;
        DevBuf<uint64_t> d_sk;
        POLEE_TRY(kmer_sketch_device(ctx, n, offsets, bases, d_sk, clk));
        return tree_from_device_sketches(ctx, n, d_sk.p, node_parent_idxs, node_js, clk);
    });
}

// (the two debug hooks below take a context or null = the host's index, so they open through host_entry, not ctx_entry, and
// index_any selects the device; an exception is then recorded in the thread's error only, not in the context's)
extern "C" polee_status polee_debug_kmer_edges_count(polee_ctx *ctx, int64_t n, const uint64_t *sketches, int64_t *count)
{
    return host_entry("polee_debug_kmer_edges_count", [&]() -> polee_status {
        if (!count) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_kmer_edges_count: null count");
        KmerIndex ix;
        POLEE_TRY(index_any(ctx, "polee_debug_kmer_edges_count", n, sketches, ix));
        *count = (int64_t)ix.edges.size();
        return POLEE_OK;
    });
}

extern "C" polee_status polee_debug_kmer_edges_fill(polee_ctx *ctx, int64_t n, const uint64_t *sketches, int64_t capacity, uint32_t *u, uint32_t *v,
                                                    uint32_t *mat, uint32_t *empt)
{
    return host_entry("polee_debug_kmer_edges_fill", [&]() -> polee_status {
        KmerIndex ix;
        POLEE_TRY(index_any(ctx, "polee_debug_kmer_edges_fill", n, sketches, ix));
        if ((int64_t)ix.edges.size() > capacity || (ix.edges.size() && (!u || !v || !mat || !empt)))
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_kmer_edges_fill: %zu edges, room for %lld", ix.edges.size(), (long long)capacity);
        for (size_t i = 0; i < ix.edges.size(); ++i) {
            u[i] = ix.edges[i].u;
            v[i] = ix.edges[i].v;
            mat[i] = ix.edges[i].mat;
            empt[i] = ix.edges[i].empt;
        }
        return POLEE_OK;
    });
}
