// Splicing features on the device (polee_splice_run): integer work throughout, and every variable-length product is
// counted, scanned and then emitted, so that no output position depends on the order in which threads finish.
//   1  one thread per exon writes its intron and, for an internal exon, its flank record (the same record feeds the overlap join)
//   2  LSD passes of rocprim::radix_sort_pairs over a permutation sort the records (their keys are wider than 64 bits)
//   3  cassette exons: one thread per unique flank looks its outer interval up in the unique introns
//      mutex exons: one thread per run of flanks with the same outer interval merges the middle exons into unions
//      alternative sites, retained introns: every internal exon walks forward over the exons that start within it; a lane takes a
//      short walk alone, the wave takes a long one together
//      alternative ends: (gene, coordinate) sorted, one thread per gene
//   4  the member rows of all of them (splice_features.hpp) are sorted, repeats dropped, and runs of equal keys become the feature table
//      and the two CSR lists
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <memory>
#include <utility>

#include "splice_features.hpp"

namespace polee {
namespace {

#define SP_HIP(expr) POLEE_HIP_TRY(ctx, expr)
// a rocPRIM call: once for the size of its temporary storage, once for the work
#define SP_PRIM(call_with_tmp_bytes)                          \
    do {                                                      \
        size_t bytes = 0;                                     \
        void *tmp_p = nullptr;                                \
        SP_HIP(call_with_tmp_bytes);                          \
        SP_HIP(tmp.need(bytes ? bytes : 16));                 \
        tmp_p = tmp.p;                                        \
        SP_HIP(call_with_tmp_bytes);                          \
    } while (0)

constexpr uint64_t SP_SENTINEL = ~(uint64_t)0;  // the first word of a record slot that holds nothing: sorts behind every record
constexpr uint32_t SP_LONG_WALK = 32;           // a walk over more exons than this is the wave's
inline unsigned blocks_for(uint64_t count) { return (unsigned)((count + 255) / 256); }

// ---- 1: records.  Slot e of both tables belongs to exon e; slots without a record carry the sentinel.
__global__ void sp_record_kernel(int64_t n, int64_t E, const int32_t *seq, const int8_t *strand, const int64_t *exon_ptr, const int64_t *first,
                                 const int64_t *last, uint64_t *i_ss, uint64_t *i_fl, uint64_t *i_tid, uint64_t *x_ss, uint64_t *x_outer, uint64_t *x_mid,
                                 uint64_t *x_tid)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    int64_t lo = 0, hi = n;  // the last t with exon_ptr[t] <= e
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) / 2;
        if (exon_ptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    const int64_t t = lo, b = exon_ptr[t], end = exon_ptr[t + 1];
    const uint64_t ss = sp_group(seq[t], strand[t]);
    const bool intron = e > b, inner = e > b && e + 1 < end;
    i_ss[e] = intron ? ss : SP_SENTINEL;
    i_fl[e] = intron ? sp_pack((uint32_t)last[e - 1] + 1, (uint32_t)first[e] - 1) : 0;
    i_tid[e] = (uint64_t)t + 1;
    x_ss[e] = inner ? ss : SP_SENTINEL;
    x_outer[e] = inner ? sp_pack((uint32_t)last[e - 1] + 1, (uint32_t)first[e + 1] - 1) : 0;
    x_mid[e] = sp_pack((uint32_t)first[e], (uint32_t)last[e]);
    x_tid[e] = (uint64_t)t + 1;
}

// ---- 2: sorting
__global__ void sp_iota_kernel(uint32_t *p, uint64_t N)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) p[i] = (uint32_t)i;
}
__global__ void sp_gather_kernel(const uint64_t *src, const uint32_t *perm, uint64_t N, uint64_t *dst)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) dst[i] = src[perm[i]];
}

// rows of `nw` words (most significant first) into ascending order: the words of the sorted rows replace the input
polee_status sort_rows(polee_ctx *ctx, DevScratch &tmp, uint64_t **words, int nw, size_t N)
{
    if (N == 0) return POLEE_OK;
    hipStream_t stream = ctx->stream;
    DevBuf<uint32_t> pa, pb;
    DevBuf<uint64_t> key, key_s;
    POLEE_TRY(pa.alloc(ctx, N));
    POLEE_TRY(pb.alloc(ctx, N));
    POLEE_TRY(key.alloc(ctx, N));
    POLEE_TRY(key_s.alloc(ctx, N));
    sp_iota_kernel<<<blocks_for(N), 256, 0, stream>>>(pa.p, N);
    POLEE_KERNEL_CHECK(ctx);
    uint32_t *pin = pa.p, *pout = pb.p;
    for (int k = nw - 1; k >= 0; --k) {  // (radix_sort_pairs is stable: least significant word first)
        sp_gather_kernel<<<blocks_for(N), 256, 0, stream>>>(words[k], pin, N, key.p);
        POLEE_KERNEL_CHECK(ctx);
        SP_PRIM(rocprim::radix_sort_pairs(tmp_p, bytes, key.p, key_s.p, pin, pout, N, 0, 64, stream));
        std::swap(pin, pout);
    }
    for (int k = 0; k < nw; ++k) {
        sp_gather_kernel<<<blocks_for(N), 256, 0, stream>>>(words[k], pin, N, key.p);
        POLEE_KERNEL_CHECK(ctx);
        SP_HIP(hipMemcpyAsync(words[k], key.p, N * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
    }
    SP_HIP(hipStreamSynchronize(stream));  // (the buffers go out of scope here)
    return POLEE_OK;
}

// head[i] = row i differs from row i - 1 in one of up to three words (a null pointer: no such word)
__global__ void sp_head_kernel(const uint64_t *a, const uint64_t *b, const uint64_t *c, uint64_t N, uint32_t *head)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    head[i] = i == 0 || a[i] != a[i - 1] || (b && b[i] != b[i - 1]) || (c && c[i] != c[i - 1]);
}
// the same over rows picked by an index list: row r of the list is row at[r] of the table
__global__ void sp_head_at_kernel(const uint64_t *a, const uint64_t *b, const uint32_t *at, uint64_t N, uint32_t *head)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    head[i] = i == 0 || a[at[i]] != a[at[i - 1]] || b[at[i]] != b[at[i - 1]];
}
// start[r] = the first row of run r, start[number of runs] = N; incl: the inclusive scan of head
__global__ void sp_runs_kernel(const uint32_t *head, const uint32_t *incl, uint64_t N, uint32_t *start)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (head[i]) start[incl[i] - 1] = (uint32_t)i;
    if (i == N - 1) start[incl[i]] = (uint32_t)N;
}

// the starts of the runs of equal (a, b, c) among N sorted rows: start [R + 1]
polee_status find_runs(polee_ctx *ctx, DevScratch &tmp, const uint64_t *a, const uint64_t *b, const uint64_t *c, const uint32_t *at, size_t N,
                       DevBuf<uint32_t> &start, uint32_t *R)
{
    hipStream_t stream = ctx->stream;
    *R = 0;
    POLEE_TRY(start.alloc(ctx, N + 1));
    if (N == 0) {
        SP_HIP(hipMemsetAsync(start.p, 0, sizeof(uint32_t), stream));
        return POLEE_OK;
    }
    DevBuf<uint32_t> head, incl;
    POLEE_TRY(head.alloc(ctx, N));
    POLEE_TRY(incl.alloc(ctx, N));
    if (at) sp_head_at_kernel<<<blocks_for(N), 256, 0, stream>>>(a, b, at, N, head.p);
    else sp_head_kernel<<<blocks_for(N), 256, 0, stream>>>(a, b, c, N, head.p);
    POLEE_KERNEL_CHECK(ctx);
    SP_PRIM(rocprim::inclusive_scan(tmp_p, bytes, head.p, incl.p, N, rocprim::plus<uint32_t>(), stream));
    sp_runs_kernel<<<blocks_for(N), 256, 0, stream>>>(head.p, incl.p, N, start.p);
    POLEE_KERNEL_CHECK(ctx);
    SP_HIP(hipMemcpyAsync(R, incl.p + (N - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SP_HIP(hipStreamSynchronize(stream));
    return POLEE_OK;
}

// offsets [N + 1] = the exclusive scan of counts [N] (counts [N] is set to 0 here); *total = offsets[N]
polee_status scan_counts(polee_ctx *ctx, DevScratch &tmp, DevBuf<uint64_t> &counts, size_t N, DevBuf<uint64_t> &offsets, uint64_t *total)
{
    hipStream_t stream = ctx->stream;
    POLEE_TRY(offsets.alloc(ctx, N + 1));
    SP_HIP(hipMemsetAsync(counts.p + N, 0, sizeof(uint64_t), stream));
    SP_PRIM(rocprim::exclusive_scan(tmp_p, bytes, counts.p, offsets.p, (uint64_t)0, N + 1, rocprim::plus<uint64_t>(), stream));
    SP_HIP(hipMemcpyAsync(total, offsets.p + N, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    SP_HIP(hipStreamSynchronize(stream));
    return POLEE_OK;
}

// the member rows, one array per word
struct Rows {
    uint64_t *w[5];
};
__device__ inline void put_row(const Rows &m, uint64_t at, uint64_t block, uint64_t group, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t side, uint32_t tid)
{
    m.w[0][at] = (block << 56) | group;
    m.w[1][at] = w1;
    m.w[2][at] = w2;
    m.w[3][at] = w3;
    m.w[4][at] = sp_pack(side, tid);
}

// ---- 3a: cassette exons.  Thread f: unique flank f = rows fstart[f] .. fstart[f + 1] of the sorted internal exons; the unique introns
// are the runs ustart [NU + 1] of the sorted introns.  off == null: counts [NF]; otherwise rows at base + off[f].
__global__ void sp_cassette_kernel(uint32_t NF, const uint32_t *fstart, const uint64_t *x_ss, const uint64_t *x_outer, const uint64_t *x_mid, const uint64_t *x_tid,
                                   uint32_t NU, const uint32_t *ustart, const uint64_t *i_ss, const uint64_t *i_fl, const uint64_t *i_tid, uint64_t *counts,
                                   const uint64_t *off, uint64_t base, Rows m)
{
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= NF) return;
    const uint32_t r0 = fstart[f], r1 = fstart[f + 1];
    const uint64_t ss = x_ss[r0], outer = x_outer[r0];
    uint32_t lo = 0, hi = NU;  // the first unique intron that is not below (ss, outer)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2, r = ustart[mid];
        if (i_ss[r] < ss || (i_ss[r] == ss && i_fl[r] < outer)) lo = mid + 1;
        else hi = mid;
    }
    const bool found = lo < NU && i_ss[ustart[lo]] == ss && i_fl[ustart[lo]] == outer;
    if (!off) {
        counts[f] = found ? (uint64_t)(r1 - r0) + (ustart[lo + 1] - ustart[lo]) : 0;
        return;
    }
    if (!found) return;
    uint64_t at = base + off[f];
    for (uint32_t r = r0; r < r1; ++r) put_row(m, at++, SP_CASSETTE, ss, x_mid[r0], outer, 0, 0, (uint32_t)x_tid[r]);
    for (uint32_t r = ustart[lo]; r < ustart[lo + 1]; ++r) put_row(m, at++, SP_CASSETTE, ss, x_mid[r0], outer, 0, 1, (uint32_t)i_tid[r]);
}

// ---- 3b: mutex exons.  Thread g: the unique flanks gstart[g] .. gstart[g + 1] share an outer interval, their middle exons ascend.
__global__ void sp_mutex_kernel(uint32_t NG, const uint32_t *gstart, const uint32_t *fstart, const uint64_t *x_ss, const uint64_t *x_outer, const uint64_t *x_mid,
                                const uint64_t *x_tid, uint64_t *counts, const uint64_t *off, uint64_t base, Rows m)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= NG) return;
    const uint32_t f0 = gstart[g], f1 = gstart[g + 1];
    uint32_t nun = 0, uf[2] = {0, 0}, ul[2] = {0, 0}, cur_last = 0, second = f1;
    for (uint32_t f = f0; f < f1; ++f) {
        const uint64_t mid = x_mid[fstart[f]];
        const uint32_t first = sp_hi(mid), last = sp_lo(mid);
        if (nun == 0 || first > cur_last) {
            if (nun < 2) uf[nun] = first, ul[nun] = last;
            if (nun == 1) second = f;
            ++nun;
            cur_last = last;
        } else {
            cur_last = max(cur_last, last);
            if (nun <= 2) {
                uf[nun - 1] = min(uf[nun - 1], first);
                ul[nun - 1] = cur_last;
            }
        }
    }
    const uint32_t r0 = fstart[f0], r1 = fstart[f1];
    if (!off) {
        counts[g] = nun == 2 ? (uint64_t)(r1 - r0) : 0;
        return;
    }
    if (nun != 2) return;
    const uint32_t rs = fstart[second];
    uint64_t at = base + off[g];
    for (uint32_t r = r0; r < r1; ++r)
        put_row(m, at++, SP_MUTEX, x_ss[r0], sp_pack(uf[0], ul[0]), sp_pack(uf[1], ul[1]), x_outer[r0], r >= rs ? 1u : 0u, (uint32_t)x_tid[r]);
}

// ---- 3c: the overlap join over the internal exons sorted by (ss, first, last)
__device__ inline SpExon load_exon(const uint64_t *x_mid, const uint64_t *x_outer, const uint64_t *x_tid, uint32_t i)
{
    const uint64_t mid = x_mid[i], outer = x_outer[i];
    return SpExon{sp_hi(mid), sp_lo(mid), sp_hi(outer), sp_lo(outer), (uint32_t)x_tid[i]};
}
// both orders of one overlapping pair: the number of rows, and with EMIT the rows themselves at `at`
template <bool EMIT>
__device__ inline uint32_t join_pair(const SpExon &a, const SpExon &b, uint64_t ss, const Rows &m, uint64_t at)
{
    uint32_t c = 0;
#pragma unroll
    for (int order = 0; order < 2; ++order) {
        const SpEvent e = order == 0 ? sp_eval(a, b) : sp_eval(b, a);
        if (e.block < 0) continue;
        if (EMIT) {
            put_row(m, at + c, (uint64_t)e.block, ss, sp_pack(e.c0, e.c1), sp_pack(e.c2, e.c3), 0, 0, e.inc);
            put_row(m, at + c + 1, (uint64_t)e.block, ss, sp_pack(e.c0, e.c1), sp_pack(e.c2, e.c3), 0, 1, e.exc);
        }
        c += 2;
    }
    return c;
}
__device__ inline uint32_t wave_exclusive_scan(uint32_t v, int lane, uint32_t *total)
{
    uint32_t s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(s, d, 64);
        if (lane >= d) s += t;
    }
    *total = __shfl(s, 63, 64);
    return s - v;
}

// A wave owns 64 consecutive exons.  Exon i walks over j = i + 1 .. end(i) - 1, the exons of its (seq, strand) that start at or before
// its last base.  Lanes first take their own exon when its walk is short; then the wave takes the long walks one after the other, 64
// partners at a time, and places a chunk's rows by a prefix sum over the lanes -- the same routine counts (EMIT false: counts [N], the
// number of pairs added to *pairs) and emits (rows at base + off[i]), so that both passes see the same pairs.
template <bool EMIT>
__global__ void __launch_bounds__(256) sp_join_kernel(uint32_t N, const uint64_t *x_ss, const uint64_t *x_mid, const uint64_t *x_outer, const uint64_t *x_tid,
                                                       uint64_t *counts, unsigned long long *pairs, const uint64_t *off, uint64_t base, Rows m)
{
    const int lane = threadIdx.x & 63;
    const uint32_t wave_base = (blockIdx.x * blockDim.x + threadIdx.x) & ~63u;  // (N < 2^31: the grid's threads fit into 32 bits)
    const uint32_t i = wave_base + lane;
    const bool valid = i < N;
    uint32_t end = i + 1;
    uint64_t ss = 0;
    SpExon a{0, 0, 0, 0, 0};
    if (valid) {
        ss = x_ss[i];
        a = load_exon(x_mid, x_outer, x_tid, i);
        uint32_t lo = i + 1, hi = N;  // the first j > i beyond (ss, a.last) in (ss, first)
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (x_ss[mid] > ss || (x_ss[mid] == ss && sp_hi(x_mid[mid]) > a.last)) hi = mid;
            else lo = mid + 1;
        }
        end = lo;
    }
    const uint32_t walk = end - (i + 1);
    const bool is_long = valid && walk > SP_LONG_WALK;
    if (valid && !is_long) {
        uint64_t at = EMIT ? base + off[i] : 0;
        uint64_t c = 0;
        for (uint32_t j = i + 1; j < end; ++j) c += join_pair<EMIT>(a, load_exon(x_mid, x_outer, x_tid, j), ss, m, at + c);
        if (!EMIT) counts[i] = c;
    }
    unsigned long long npairs = valid ? walk : 0;
    uint64_t todo = __ballot(is_long);
    while (todo) {  // (wave-uniform)
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t i2 = wave_base + l, end2 = __shfl(end, l, 64);
        const SpExon a2 = load_exon(x_mid, x_outer, x_tid, i2);
        const uint64_t ss2 = x_ss[i2];
        uint64_t run = EMIT ? base + off[i2] : 0;
        for (uint32_t j0 = i2 + 1; j0 < end2; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool on = j < end2;
            SpExon b{0, 0, 0, 0, 0};
            if (on) b = load_exon(x_mid, x_outer, x_tid, j);
            uint32_t c = on ? join_pair<false>(a2, b, ss2, m, 0) : 0, total;
            const uint32_t before = wave_exclusive_scan(c, lane, &total);
            if (EMIT && on) join_pair<true>(a2, b, ss2, m, run + before);
            run += total;
        }
        if (!EMIT && lane == 0) counts[i2] = run;
    }
    if (!EMIT) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) npairs += __shfl_down(npairs, d, 64);
        if (lane == 0 && npairs) atomicAdd(pairs, npairs);  // (a sum of integers: the same in any order, and no position comes from it)
    }
}

// ---- 3d: alternative ends.  skey / ekey: gene << 32 | first-exon start (last-exon end) sorted, with the transcripts beside them; both
// have the same runs of genes, gstart [NG + 1].  Thread g: the clusters of both sides of gene run g.
__global__ void sp_ends_kernel(uint32_t NG, const uint32_t *gstart, const uint64_t *skey, const uint32_t *stid, const uint64_t *ekey, const uint32_t *etid,
                               const int32_t *seq, const int8_t *strand, uint64_t *counts, const uint64_t *off, uint64_t base, Rows m)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= NG) return;
    const uint32_t g0 = gstart[g], g1 = gstart[g + 1], size = g1 - g0;
    if (size <= 1) {
        if (!off) counts[g] = 0;
        return;
    }
    uint32_t ncl[2] = {1, 1};
    for (uint32_t i = g0 + 1; i < g1; ++i) {
        ncl[0] += sp_lo(skey[i]) - sp_lo(skey[i - 1]) > SP_MERGE_DISTANCE;
        ncl[1] += sp_lo(ekey[i]) - sp_lo(ekey[i - 1]) > SP_MERGE_DISTANCE;
    }
    if (!off) {
        counts[g] = (uint64_t)(sp_emitted_clusters(ncl[0]) + sp_emitted_clusters(ncl[1])) * size;
        return;
    }
    uint32_t first_tid = stid[g0];
    for (uint32_t i = g0 + 1; i < g1; ++i) first_tid = min(first_tid, stid[i]);
    const int8_t sd = strand[first_tid - 1];
    const uint64_t ss = sp_group(seq[first_tid - 1], sd), gene = sp_hi(skey[g0]);
    const uint64_t span = sp_pack(sp_lo(skey[g0]), sp_lo(ekey[g0]));  // (max_last is the minimum of the ends, transcripts.jl:884)
    uint64_t at = base + off[g];
    for (int kind = 0; kind < 2; ++kind) {
        const uint64_t *key = kind == 0 ? skey : ekey;
        const uint32_t *tid = kind == 0 ? stid : etid;
        uint32_t todo = sp_emitted_clusters(ncl[kind]);
        for (uint32_t c0 = g0; c0 < g1 && todo > 0; --todo) {
            uint32_t c1 = c0 + 1;
            while (c1 < g1 && sp_lo(key[c1]) - sp_lo(key[c1 - 1]) <= SP_MERGE_DISTANCE) ++c1;
            for (uint32_t i = g0; i < g1; ++i)
                put_row(m, at++, sp_end_block(kind, sd), (gene << 1) | (uint64_t)kind, sp_pack(sp_lo(key[c0]), sp_lo(key[c1 - 1])), span, ss,
                        i >= c0 && i < c1 ? 0u : 1u, tid[i]);
            c0 = c1;
        }
    }
}
__global__ void sp_end_keys_kernel(int64_t n, const int32_t *gene_of, const int64_t *exon_ptr, const int64_t *first, const int64_t *last, uint64_t *skey,
                                   uint64_t *ekey, uint32_t *tid)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    skey[t] = sp_pack((uint32_t)gene_of[t], (uint32_t)first[exon_ptr[t]]);
    ekey[t] = sp_pack((uint32_t)gene_of[t], (uint32_t)last[exon_ptr[t + 1] - 1]);
    tid[t] = (uint32_t)t + 1;
}
__global__ void sp_shift_kernel(const uint64_t *key, uint64_t N, uint64_t *gene)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) gene[i] = key[i] >> 32;
}

// ---- 4: the sorted member rows into features.  flags [3][M + 1]: row i opens a feature; is a new included member; a new excluded one
__global__ void sp_flag_kernel(Rows m, uint64_t M, uint64_t *feat, uint64_t *inc, uint64_t *exc)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const bool f = i == 0 || m.w[0][i] != m.w[0][i - 1] || m.w[1][i] != m.w[1][i - 1] || m.w[2][i] != m.w[2][i - 1] || m.w[3][i] != m.w[3][i - 1];
    const bool u = f || m.w[4][i] != m.w[4][i - 1];
    const bool side = sp_hi(m.w[4][i]) != 0;
    feat[i] = f;
    inc[i] = u && !side;
    exc[i] = u && side;
}
__global__ void sp_table_kernel(Rows m, uint64_t M, const uint64_t *feat, const uint64_t *inc, const uint64_t *exc, const uint64_t *feat_off, const uint64_t *inc_off,
                                const uint64_t *exc_off, uint64_t *keys, int64_t *inc_ptr, int64_t *exc_ptr, int32_t *inc_idx, int32_t *exc_idx)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    if (feat[i]) {
        const uint64_t f = feat_off[i];
        for (int k = 0; k < 4; ++k) keys[4 * f + k] = m.w[k][i];
        inc_ptr[f] = (int64_t)inc_off[i];
        exc_ptr[f] = (int64_t)exc_off[i];
    }
    if (inc[i]) inc_idx[inc_off[i]] = (int32_t)sp_lo(m.w[4][i]);
    if (exc[i]) exc_idx[exc_off[i]] = (int32_t)sp_lo(m.w[4][i]);
}

polee_status run_device(polee_ctx *ctx, const polee_xb_transcripts *T, const int32_t *gene_of, polee_splice &r)
{
    int64_t E = 0, NXl = 0;
    POLEE_TRY(sp_validate(ctx, "polee_splice_run", T, gene_of, &E, &NXl));
    hipStream_t stream = ctx->stream;
    SpClock clk;
    DevScratch tmp(ctx);
    const int64_t n = T->n;
    const size_t NI = (size_t)(E - n), NX = (size_t)NXl;
    r.num_exons = E;
    r.num_internal = NXl;

    DevBuf<int32_t> d_seq, d_gene;
    DevBuf<int8_t> d_strand;
    DevBuf<int64_t> d_ptr, d_first, d_last;
    POLEE_TRY(d_seq.upload(ctx, T->seq, (size_t)n));
    POLEE_TRY(d_strand.upload(ctx, T->strand, (size_t)n));
    POLEE_TRY(d_ptr.upload(ctx, T->exon_ptr, (size_t)n + 1));
    POLEE_TRY(d_first.upload(ctx, T->exon_first, (size_t)E));
    POLEE_TRY(d_last.upload(ctx, T->exon_last, (size_t)E));
    if (gene_of) POLEE_TRY(d_gene.upload(ctx, gene_of, (size_t)n));
    clk.lap("upload", stream, true);

    // 1, 2: the records, sorted; the sentinels of the empty slots end up behind the NI introns and the NX internal exons
    DevBuf<uint64_t> i_ss, i_fl, i_tid, x_ss, x_outer, x_mid, x_tid, j_ss, j_mid, j_outer, j_tid;
    for (DevBuf<uint64_t> *b : {&i_ss, &i_fl, &i_tid, &x_ss, &x_outer, &x_mid, &x_tid, &j_ss, &j_mid, &j_outer, &j_tid}) POLEE_TRY(b->alloc(ctx, (size_t)E));
    sp_record_kernel<<<blocks_for((uint64_t)E), 256, 0, stream>>>(n, E, d_seq.p, d_strand.p, d_ptr.p, d_first.p, d_last.p, i_ss.p, i_fl.p, i_tid.p, x_ss.p, x_outer.p,
                                                                   x_mid.p, x_tid.p);
    POLEE_KERNEL_CHECK(ctx);
    SP_HIP(hipMemcpyAsync(j_ss.p, x_ss.p, (size_t)E * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
    SP_HIP(hipMemcpyAsync(j_mid.p, x_mid.p, (size_t)E * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
    SP_HIP(hipMemcpyAsync(j_outer.p, x_outer.p, (size_t)E * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
    SP_HIP(hipMemcpyAsync(j_tid.p, x_tid.p, (size_t)E * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
    clk.lap("records", stream, true);
    {
        uint64_t *wi[3] = {i_ss.p, i_fl.p, i_tid.p};
        POLEE_TRY(sort_rows(ctx, tmp, wi, 3, (size_t)E));
        uint64_t *wx[4] = {x_ss.p, x_outer.p, x_mid.p, x_tid.p};
        POLEE_TRY(sort_rows(ctx, tmp, wx, 4, (size_t)E));
        uint64_t *wj[4] = {j_ss.p, j_mid.p, j_outer.p, j_tid.p};
        POLEE_TRY(sort_rows(ctx, tmp, wj, 4, (size_t)E));
    }
    clk.lap("sort records", stream, true);

    // the runs: unique introns, unique flanks, and the flanks' groups by outer interval
    DevBuf<uint32_t> ustart, fstart, gstart;
    uint32_t NU = 0, NF = 0, NG = 0;
    POLEE_TRY(find_runs(ctx, tmp, i_ss.p, i_fl.p, nullptr, nullptr, NI, ustart, &NU));
    POLEE_TRY(find_runs(ctx, tmp, x_ss.p, x_outer.p, x_mid.p, nullptr, NX, fstart, &NF));
    POLEE_TRY(find_runs(ctx, tmp, x_ss.p, x_outer.p, nullptr, fstart.p, NF, gstart, &NG));
    clk.lap("runs", stream, true);

    // the alternative ends' sorted keys and gene runs
    DevBuf<uint64_t> skey, ekey, skey_s, ekey_s, gene_s;
    DevBuf<uint32_t> tid0, stid, etid, estart;
    uint32_t NE = 0;
    if (gene_of) {
        for (DevBuf<uint64_t> *b : {&skey, &ekey, &skey_s, &ekey_s, &gene_s}) POLEE_TRY(b->alloc(ctx, (size_t)n));
        for (DevBuf<uint32_t> *b : {&tid0, &stid, &etid}) POLEE_TRY(b->alloc(ctx, (size_t)n));
        sp_end_keys_kernel<<<blocks_for((uint64_t)n), 256, 0, stream>>>(n, d_gene.p, d_ptr.p, d_first.p, d_last.p, skey.p, ekey.p, tid0.p);
        POLEE_KERNEL_CHECK(ctx);
        SP_PRIM(rocprim::radix_sort_pairs(tmp_p, bytes, skey.p, skey_s.p, tid0.p, stid.p, (size_t)n, 0, 64, stream));
        SP_PRIM(rocprim::radix_sort_pairs(tmp_p, bytes, ekey.p, ekey_s.p, tid0.p, etid.p, (size_t)n, 0, 64, stream));
        sp_shift_kernel<<<blocks_for((uint64_t)n), 256, 0, stream>>>(skey_s.p, (uint64_t)n, gene_s.p);
        POLEE_KERNEL_CHECK(ctx);
        POLEE_TRY(find_runs(ctx, tmp, gene_s.p, nullptr, nullptr, nullptr, (size_t)n, estart, &NE));
        clk.lap("sort ends", stream, true);
    }

    // 3, counting: cassette [NF], mutex [NG], join [NX], ends [NE]
    DevBuf<uint64_t> c_cas, c_mut, c_join, c_end, o_cas, o_mut, o_join, o_end;
    DevBuf<unsigned long long> d_pairs;
    uint64_t M_cas = 0, M_mut = 0, M_join = 0, M_end = 0;
    const Rows none{{nullptr, nullptr, nullptr, nullptr, nullptr}};
    POLEE_TRY(d_pairs.alloc(ctx, 1));
    SP_HIP(hipMemsetAsync(d_pairs.p, 0, sizeof(unsigned long long), stream));
    POLEE_TRY(c_cas.alloc(ctx, (size_t)NF + 1));
    POLEE_TRY(c_mut.alloc(ctx, (size_t)NG + 1));
    POLEE_TRY(c_join.alloc(ctx, NX + 1));
    POLEE_TRY(c_end.alloc(ctx, (size_t)NE + 1));
    if (NF) {
        sp_cassette_kernel<<<blocks_for(NF), 256, 0, stream>>>(NF, fstart.p, x_ss.p, x_outer.p, x_mid.p, x_tid.p, NU, ustart.p, i_ss.p, i_fl.p, i_tid.p, c_cas.p, nullptr,
                                                               0, none);
        POLEE_KERNEL_CHECK(ctx);
        sp_mutex_kernel<<<blocks_for(NG), 256, 0, stream>>>(NG, gstart.p, fstart.p, x_ss.p, x_outer.p, x_mid.p, x_tid.p, c_mut.p, nullptr, 0, none);
        POLEE_KERNEL_CHECK(ctx);
        sp_join_kernel<false><<<blocks_for(NX), 256, 0, stream>>>((uint32_t)NX, j_ss.p, j_mid.p, j_outer.p, j_tid.p, c_join.p, d_pairs.p, nullptr, 0, none);
        POLEE_KERNEL_CHECK(ctx);
    }
    if (NE) {
        sp_ends_kernel<<<blocks_for(NE), 256, 0, stream>>>(NE, estart.p, skey_s.p, stid.p, ekey_s.p, etid.p, d_seq.p, d_strand.p, c_end.p, nullptr, 0, none);
        POLEE_KERNEL_CHECK(ctx);
    }
    POLEE_TRY(scan_counts(ctx, tmp, c_cas, NF, o_cas, &M_cas));
    POLEE_TRY(scan_counts(ctx, tmp, c_mut, NG, o_mut, &M_mut));
    POLEE_TRY(scan_counts(ctx, tmp, c_join, NX, o_join, &M_join));
    POLEE_TRY(scan_counts(ctx, tmp, c_end, NE, o_end, &M_end));
    unsigned long long pairs = 0;
    POLEE_TRY(d_pairs.download(ctx, &pairs, 1));
    r.num_pairs = (int64_t)pairs;
    clk.lap("count", stream, true);
    const uint64_t M = M_cas + M_mut + M_join + M_end;
    if (M >= ((uint64_t)1 << 32))
        return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_splice_run: %llu member rows before repeats are dropped, more than 2^32 - 1 (the host path takes those)",
                    (unsigned long long)M);
    if (M == 0) {
        sp_resize(r, 0);
        r.inc_ptr.assign(1, 0);
        r.exc_ptr.assign(1, 0);
        return POLEE_OK;
    }

    // 3, emitting
    DevBuf<uint64_t> mw[5];
    Rows m;
    for (int k = 0; k < 5; ++k) {
        POLEE_TRY(mw[k].alloc(ctx, (size_t)M));
        m.w[k] = mw[k].p;
    }
    if (M_cas) {
        sp_cassette_kernel<<<blocks_for(NF), 256, 0, stream>>>(NF, fstart.p, x_ss.p, x_outer.p, x_mid.p, x_tid.p, NU, ustart.p, i_ss.p, i_fl.p, i_tid.p, nullptr, o_cas.p,
                                                               0, m);
        POLEE_KERNEL_CHECK(ctx);
    }
    if (M_mut) {
        sp_mutex_kernel<<<blocks_for(NG), 256, 0, stream>>>(NG, gstart.p, fstart.p, x_ss.p, x_outer.p, x_mid.p, x_tid.p, nullptr, o_mut.p, M_cas, m);
        POLEE_KERNEL_CHECK(ctx);
    }
    if (M_join) {
        sp_join_kernel<true><<<blocks_for(NX), 256, 0, stream>>>((uint32_t)NX, j_ss.p, j_mid.p, j_outer.p, j_tid.p, nullptr, nullptr, o_join.p, M_cas + M_mut, m);
        POLEE_KERNEL_CHECK(ctx);
    }
    if (M_end) {
        sp_ends_kernel<<<blocks_for(NE), 256, 0, stream>>>(NE, estart.p, skey_s.p, stid.p, ekey_s.p, etid.p, d_seq.p, d_strand.p, nullptr, o_end.p, M_cas + M_mut + M_join,
                                                           m);
        POLEE_KERNEL_CHECK(ctx);
    }
    clk.lap("emit", stream, true);

    // 4: sort, drop repeats, run-length encode
    POLEE_TRY(sort_rows(ctx, tmp, m.w, 5, (size_t)M));
    clk.lap("sort members", stream, true);
    DevBuf<uint64_t> flag[3], foff[3];
    uint64_t tot[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) POLEE_TRY(flag[k].alloc(ctx, (size_t)M + 1));
    sp_flag_kernel<<<blocks_for(M), 256, 0, stream>>>(m, M, flag[0].p, flag[1].p, flag[2].p);
    POLEE_KERNEL_CHECK(ctx);
    for (int k = 0; k < 3; ++k) POLEE_TRY(scan_counts(ctx, tmp, flag[k], (size_t)M, foff[k], &tot[k]));
    const size_t F = (size_t)tot[0];
    DevBuf<uint64_t> keys;
    DevBuf<int64_t> inc_ptr, exc_ptr;
    DevBuf<int32_t> inc_idx, exc_idx;
    POLEE_TRY(keys.alloc(ctx, F * 4));
    POLEE_TRY(inc_ptr.alloc(ctx, F));
    POLEE_TRY(exc_ptr.alloc(ctx, F));
    POLEE_TRY(inc_idx.alloc(ctx, (size_t)tot[1] + 1));
    POLEE_TRY(exc_idx.alloc(ctx, (size_t)tot[2] + 1));
    sp_table_kernel<<<blocks_for(M), 256, 0, stream>>>(m, M, flag[0].p, flag[1].p, flag[2].p, foff[0].p, foff[1].p, foff[2].p, keys.p, inc_ptr.p, exc_ptr.p, inc_idx.p,
                                                       exc_idx.p);
    POLEE_KERNEL_CHECK(ctx);
    std::vector<uint64_t> h_keys(F * 4);
    sp_resize(r, F);
    r.inc_ptr.assign(F + 1, (int64_t)tot[1]);
    r.exc_ptr.assign(F + 1, (int64_t)tot[2]);
    r.inc_idx.resize((size_t)tot[1]);
    r.exc_idx.resize((size_t)tot[2]);
    POLEE_TRY(keys.download(ctx, h_keys.data(), F * 4));
    POLEE_TRY(inc_ptr.download(ctx, r.inc_ptr.data(), F));
    POLEE_TRY(exc_ptr.download(ctx, r.exc_ptr.data(), F));
    POLEE_TRY(inc_idx.download(ctx, r.inc_idx.data(), (size_t)tot[1]));
    POLEE_TRY(exc_idx.download(ctx, r.exc_idx.data(), (size_t)tot[2]));
    for (size_t f = 0; f < F; ++f) sp_decode(r, f, &h_keys[4 * f]);
    clk.lap("feature table");
    return POLEE_OK;
}

}  // namespace
}  // namespace polee

using namespace polee;

extern "C" polee_status polee_splice_run(polee_ctx *ctx, const polee_xb_transcripts *transcripts, const int32_t *gene_of_or_null, polee_splice **out)
{
    return ctx_entry(ctx, "polee_splice_run", [&]() -> polee_status {
        if (!out) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_splice_run: null output");
        *out = nullptr;
        std::unique_ptr<polee_splice> r(new polee_splice);
        POLEE_TRY(run_device(ctx, transcripts, gene_of_or_null, *r));
        *out = r.release();
        return POLEE_OK;
    });
}
