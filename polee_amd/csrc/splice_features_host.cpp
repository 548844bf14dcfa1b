// Splicing features on the host threads (polee_splice_run_host): the twin of splice_features.hip, element for element, and the
// handle's getters.  Plain C++ on POLEE_HOST_THREADS: the same member rows (splice_features.hpp), made by loops over sorted
// records, then one sort and one pass that drops repeats.
#include <algorithm>
#include <cstring>
#include <memory>

#include "kmer_tree.hpp"
#include "splice_features.hpp"

namespace polee {

polee_status sp_validate(polee_ctx *ctx, const char *who, const polee_xb_transcripts *T, const int32_t *gene_of, int64_t *E_out, int64_t *NX_out)
{
    if (!T || !T->seq || !T->strand || !T->exon_ptr) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: null transcripts", who);
    const int64_t n = T->n;
    if (n < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: no transcripts (n = %lld)", who, (long long)n);
    if (T->exon_ptr[0] != 0) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: exon_ptr[0] must be 0", who);
    const int64_t E = T->exon_ptr[n];
    if (E < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: no exons (exon_ptr[n] = %lld)", who, (long long)E);
    if (E >= ((int64_t)1 << 31)) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: %lld exons, more than 2^31 - 1", who, (long long)E);
    if (!T->exon_first || !T->exon_last) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: null exon coordinates", who);
    int64_t NX = 0;
    for (int64_t t = 0; t < n; ++t) {
        const int64_t lo = T->exon_ptr[t], hi = T->exon_ptr[t + 1];
        if (hi <= lo || hi > E) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: transcript %lld has no exons, or exon_ptr decreases", who, (long long)t + 1);
        if (T->seq[t] < 0) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: transcript %lld: negative sequence id", who, (long long)t + 1);
        if (T->strand[t] < -1 || T->strand[t] > 1) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: transcript %lld: strand must be -1, 0 or +1", who, (long long)t + 1);
        if (gene_of && gene_of[t] < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: transcript %lld: gene numbers are 1-based", who, (long long)t + 1);
        for (int64_t e = lo; e < hi; ++e) {
            const int64_t f = T->exon_first[e], l = T->exon_last[e];
            if (f < 1 || l < f || l > SP_MAX_COORD)
                return fail(ctx, POLEE_ERR_BAD_ARG, "%s: transcript %lld: exon [%lld, %lld] outside 1 .. 2^31 - 2, or empty", who, (long long)t + 1, (long long)f,
                            (long long)l);
            if (e > lo && f <= T->exon_last[e - 1])
                return fail(ctx, POLEE_ERR_BAD_ARG, "%s: transcript %lld: exons must ascend and not overlap", who, (long long)t + 1);
        }
        NX += std::max<int64_t>(0, hi - lo - 2);
    }
    *E_out = E;
    *NX_out = NX;
    return POLEE_OK;
}

void sp_resize(polee_splice &r, size_t F)
{
    r.type.resize(F);
    r.seq.resize(F);
    r.strand.resize(F);
    r.coords.resize(F * 4);
    r.end_span.resize(F * 2);
}

void sp_decode(polee_splice &r, size_t f, const uint64_t *w)
{
    const uint64_t block = w[0] >> 56;
    const bool ends = block == SP_ALT5P || block == SP_ALT3P;
    const uint64_t g = ends ? w[3] : (w[0] & (((uint64_t)1 << 56) - 1));
    const int8_t strand = (int8_t)((int)(g & 3) - 1);
    r.seq[f] = (int32_t)(g >> 2);
    r.strand[f] = strand;
    int64_t *c = &r.coords[f * 4], *s = &r.end_span[f * 2];
    c[0] = sp_hi(w[1]);
    c[1] = sp_lo(w[1]);
    c[2] = c[3] = s[0] = s[1] = -1;
    if (ends) {
        s[0] = sp_hi(w[2]);
        s[1] = sp_lo(w[2]);
    } else if (block != SP_RETAINED) {
        c[2] = sp_hi(w[2]);
        c[3] = sp_lo(w[2]);
    }
    switch (block) {
    case SP_CASSETTE: r.type[f] = SP_T_CASSETTE; break;
    case SP_MUTEX: r.type[f] = SP_T_MUTEX; break;
    case SP_ALTSITE:  // splicing.jl:336-338
        r.type[f] = (c[0] == c[2]) == (strand == 1) ? SP_T_ACCEPTOR : SP_T_DONOR;
        break;
    case SP_RETAINED: r.type[f] = SP_T_RETAINED; break;
    case SP_ALT5P: r.type[f] = SP_T_ALT5P; break;
    default: r.type[f] = SP_T_ALT3P; break;
    }
}

namespace {

struct Intron {
    uint64_t ss, fl;
    uint32_t tid;
    bool operator<(const Intron &o) const { return ss != o.ss ? ss < o.ss : fl != o.fl ? fl < o.fl : tid < o.tid; }
};
struct Internal {  // an internal exon = the middle of a flank
    uint64_t ss, outer, mid;
    uint32_t tid;
    bool operator<(const Internal &o) const
    {
        return ss != o.ss ? ss < o.ss : outer != o.outer ? outer < o.outer : mid != o.mid ? mid < o.mid : tid < o.tid;
    }
};
struct JoinRec {
    uint64_t ss, mid, outer;
    uint32_t tid;
    bool operator<(const JoinRec &o) const
    {
        return ss != o.ss ? ss < o.ss : mid != o.mid ? mid < o.mid : outer != o.outer ? outer < o.outer : tid < o.tid;
    }
};
struct EndRec {
    uint64_t key;  // gene << 32 | coordinate
    uint32_t tid;
    bool operator<(const EndRec &o) const { return key != o.key ? key < o.key : tid < o.tid; }
};

inline SpMember member(uint64_t block, uint64_t group, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t side, uint32_t tid)
{
    return SpMember{{(block << 56) | group, w1, w2, w3, sp_pack(side, tid)}};
}

polee_status run_host(const polee_xb_transcripts *T, const int32_t *gene_of, polee_splice &r)
{
    int64_t E = 0, NX = 0;
    POLEE_TRY(sp_validate(nullptr, "polee_splice_run_host", T, gene_of, &E, &NX));
    SpClock clk;
    const int64_t n = T->n;
    r.num_exons = E;
    r.num_internal = NX;
    std::vector<Intron> introns;
    std::vector<Internal> inner;
    introns.reserve((size_t)(E - n));
    inner.reserve((size_t)NX);
    for (int64_t t = 0; t < n; ++t) {
        const int64_t lo = T->exon_ptr[t], hi = T->exon_ptr[t + 1];
        const uint64_t ss = sp_group(T->seq[t], T->strand[t]);
        for (int64_t e = lo + 1; e < hi; ++e) {
            introns.push_back(Intron{ss, sp_pack((uint32_t)T->exon_last[e - 1] + 1, (uint32_t)T->exon_first[e] - 1), (uint32_t)t + 1});
            if (e + 1 < hi)
                inner.push_back(Internal{ss, sp_pack((uint32_t)T->exon_last[e - 1] + 1, (uint32_t)T->exon_first[e + 1] - 1),
                                         sp_pack((uint32_t)T->exon_first[e], (uint32_t)T->exon_last[e]), (uint32_t)t + 1});
        }
    }
    clk.lap("records");
    kmer_parallel_sort(introns);
    std::vector<JoinRec> join(inner.size());
    for (size_t i = 0; i < inner.size(); ++i) join[i] = JoinRec{inner[i].ss, inner[i].mid, inner[i].outer, inner[i].tid};
    kmer_parallel_sort(inner);
    kmer_parallel_sort(join);
    clk.lap("sort records");

    std::vector<SpMember> rows;
    // the unique introns: starts of the runs of (ss, fl)
    std::vector<size_t> ustart;
    for (size_t i = 0; i < introns.size(); ++i)
        if (i == 0 || introns[i].ss != introns[i - 1].ss || introns[i].fl != introns[i - 1].fl) ustart.push_back(i);
    ustart.push_back(introns.size());
    // cassette and mutually exclusive exons: runs of flanks within runs of outer intervals
    for (size_t g0 = 0; g0 < inner.size();) {
        size_t g1 = g0;
        while (g1 < inner.size() && inner[g1].ss == inner[g0].ss && inner[g1].outer == inner[g0].outer) ++g1;
        const uint64_t ss = inner[g0].ss, outer = inner[g0].outer;
        // the intron that equals the outer interval
        size_t lo = 0, hi = ustart.size() - 1;
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            const Intron &u = introns[ustart[mid]];
            if (u.ss < ss || (u.ss == ss && u.fl < outer)) lo = mid + 1;
            else hi = mid;
        }
        const bool found = lo + 1 < ustart.size() && introns[ustart[lo]].ss == ss && introns[ustart[lo]].fl == outer;
        uint32_t nun = 0;
        uint32_t uf[2] = {0, 0}, ul[2] = {0, 0}, cur_last = 0;
        size_t second = g1;  // the first row of the second union
        for (size_t f0 = g0; f0 < g1;) {
            size_t f1 = f0;
            while (f1 < g1 && inner[f1].mid == inner[f0].mid) ++f1;
            if (found) {
                for (size_t i = f0; i < f1; ++i) rows.push_back(member(SP_CASSETTE, ss, inner[f0].mid, outer, 0, 0, inner[i].tid));
                for (size_t i = ustart[lo]; i < ustart[lo + 1]; ++i) rows.push_back(member(SP_CASSETTE, ss, inner[f0].mid, outer, 0, 1, introns[i].tid));
            }
            const uint32_t first = sp_hi(inner[f0].mid), last = sp_lo(inner[f0].mid);
            if (nun == 0 || first > cur_last) {
                if (nun < 2) uf[nun] = first, ul[nun] = last;
                if (nun == 1) second = f0;
                ++nun;
                cur_last = last;
            } else {
                cur_last = std::max(cur_last, last);
                if (nun <= 2) {
                    uf[nun - 1] = std::min(uf[nun - 1], first);
                    ul[nun - 1] = cur_last;
                }
            }
            f0 = f1;
        }
        if (nun == 2)
            for (size_t i = g0; i < g1; ++i)
                rows.push_back(member(SP_MUTEX, ss, sp_pack(uf[0], ul[0]), sp_pack(uf[1], ul[1]), outer, i >= second ? 1u : 0u, inner[i].tid));
        g0 = g1;
    }
    clk.lap("cassette, mutex");

    // the overlap join: every exon walks forward over the exons that start within it
    {
        const size_t N = join.size();
        std::vector<std::vector<SpMember>> out(host_threads());
        std::vector<int64_t> pairs(host_threads(), 0);
        parallel_chunks(N, 4096, [&](size_t lo, size_t hi, unsigned th) {
            std::vector<SpMember> &o = out[th];
            for (size_t i = lo; i < hi; ++i) {
                const JoinRec &ra = join[i];
                const SpExon a{sp_hi(ra.mid), sp_lo(ra.mid), sp_hi(ra.outer), sp_lo(ra.outer), ra.tid};
                for (size_t j = i + 1; j < N && join[j].ss == ra.ss && sp_hi(join[j].mid) <= a.last; ++j) {
                    const JoinRec &rb = join[j];
                    const SpExon b{sp_hi(rb.mid), sp_lo(rb.mid), sp_hi(rb.outer), sp_lo(rb.outer), rb.tid};
                    ++pairs[th];
                    for (int order = 0; order < 2; ++order) {
                        const SpEvent e = order == 0 ? sp_eval(a, b) : sp_eval(b, a);
                        if (e.block < 0) continue;
                        o.push_back(member((uint64_t)e.block, ra.ss, sp_pack(e.c0, e.c1), sp_pack(e.c2, e.c3), 0, 0, e.inc));
                        o.push_back(member((uint64_t)e.block, ra.ss, sp_pack(e.c0, e.c1), sp_pack(e.c2, e.c3), 0, 1, e.exc));
                    }
                }
            }
        });
        for (unsigned th = 0; th < out.size(); ++th) {
            rows.insert(rows.end(), out[th].begin(), out[th].end());
            r.num_pairs += pairs[th];
        }
    }
    clk.lap("overlap join");

    if (gene_of) {
        std::vector<EndRec> st((size_t)n), en((size_t)n);
        for (int64_t t = 0; t < n; ++t) {
            st[(size_t)t] = EndRec{sp_pack((uint32_t)gene_of[t], (uint32_t)T->exon_first[T->exon_ptr[t]]), (uint32_t)t + 1};
            en[(size_t)t] = EndRec{sp_pack((uint32_t)gene_of[t], (uint32_t)T->exon_last[T->exon_ptr[t + 1] - 1]), (uint32_t)t + 1};
        }
        kmer_parallel_sort(st);
        kmer_parallel_sort(en);
        for (size_t g0 = 0; g0 < (size_t)n;) {
            size_t g1 = g0;
            while (g1 < (size_t)n && sp_hi(st[g1].key) == sp_hi(st[g0].key)) ++g1;
            const size_t m = g1 - g0;
            if (m > 1) {
                const uint64_t gene = sp_hi(st[g0].key);
                uint32_t first_tid = st[g0].tid;
                for (size_t i = g0; i < g1; ++i) first_tid = std::min(first_tid, st[i].tid);
                const int8_t strand = T->strand[first_tid - 1];
                const uint64_t ss = sp_group(T->seq[first_tid - 1], strand);
                const uint64_t span = sp_pack(sp_lo(st[g0].key), sp_lo(en[g0].key));  // (max_last: the minimum of the ends, :884)
                for (int kind = 0; kind < 2; ++kind) {
                    const std::vector<EndRec> &x = kind == 0 ? st : en;
                    uint32_t ncl = 1;
                    for (size_t i = g0 + 1; i < g1; ++i) ncl += sp_lo(x[i].key) - sp_lo(x[i - 1].key) > SP_MERGE_DISTANCE;
                    uint32_t todo = sp_emitted_clusters(ncl);
                    for (size_t c0 = g0; c0 < g1 && todo > 0; --todo) {
                        size_t c1 = c0 + 1;
                        while (c1 < g1 && sp_lo(x[c1].key) - sp_lo(x[c1 - 1].key) <= SP_MERGE_DISTANCE) ++c1;
                        for (size_t i = g0; i < g1; ++i)
                            rows.push_back(member(sp_end_block(kind, strand), (gene << 1) | (uint64_t)kind, sp_pack(sp_lo(x[c0].key), sp_lo(x[c1 - 1].key)), span,
                                                  ss, i >= c0 && i < c1 ? 0u : 1u, x[i].tid));
                        c0 = c1;
                    }
                }
            }
            g0 = g1;
        }
        clk.lap("alternative ends");
    }

    kmer_parallel_sort(rows);
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    clk.lap("sort members, unique");
    size_t F = 0;
    for (size_t i = 0; i < rows.size(); ++i) F += i == 0 || memcmp(rows[i].w, rows[i - 1].w, 4 * sizeof(uint64_t)) != 0;
    sp_resize(r, F);
    r.inc_ptr.assign(F + 1, 0);
    r.exc_ptr.assign(F + 1, 0);
    size_t f = 0;
    for (size_t i = 0; i < rows.size(); ++i) {
        if (i == 0 || memcmp(rows[i].w, rows[i - 1].w, 4 * sizeof(uint64_t)) != 0) {
            sp_decode(r, f, rows[i].w);
            r.inc_ptr[f] = (int64_t)r.inc_idx.size();
            r.exc_ptr[f] = (int64_t)r.exc_idx.size();
            ++f;
        }
        (sp_hi(rows[i].w[4]) == 0 ? r.inc_idx : r.exc_idx).push_back((int32_t)sp_lo(rows[i].w[4]));
    }
    r.inc_ptr[F] = (int64_t)r.inc_idx.size();
    r.exc_ptr[F] = (int64_t)r.exc_idx.size();
    clk.lap("feature table");
    return POLEE_OK;
}

}  // namespace
}  // namespace polee

using namespace polee;

extern "C" polee_status polee_splice_run_host(const polee_xb_transcripts *transcripts, const int32_t *gene_of_or_null, polee_splice **out)
{
    return host_entry("polee_splice_run_host", [&]() -> polee_status {
        if (!out) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_splice_run_host: null output");
        *out = nullptr;
        std::unique_ptr<polee_splice> r(new polee_splice);
        POLEE_TRY(run_host(transcripts, gene_of_or_null, *r));
        *out = r.release();
        return POLEE_OK;
    });
}

extern "C" polee_status polee_splice_sizes(const polee_splice *sf, int64_t *num_features, int64_t *num_included, int64_t *num_excluded, int64_t *num_exons,
                                           int64_t *num_internal_exons, int64_t *num_overlapping_pairs)
{
    return entry(sf, "polee_splice_sizes", [&](polee_ctx *) -> polee_status {
        if (num_features) *num_features = (int64_t)sf->type.size();
        if (num_included) *num_included = (int64_t)sf->inc_idx.size();
        if (num_excluded) *num_excluded = (int64_t)sf->exc_idx.size();
        if (num_exons) *num_exons = sf->num_exons;
        if (num_internal_exons) *num_internal_exons = sf->num_internal;
        if (num_overlapping_pairs) *num_overlapping_pairs = sf->num_pairs;
        return POLEE_OK;
    });
}

extern "C" polee_status polee_splice_get(const polee_splice *sf, int32_t *type, int32_t *seq, int8_t *strand, int64_t *coords, int64_t *end_span,
                                         int64_t *included_ptr, int32_t *included_idx, int64_t *excluded_ptr, int32_t *excluded_idx)
{
    return entry(sf, "polee_splice_get", [&](polee_ctx *) -> polee_status {
        auto copy = [](auto *dst, const auto &v) {
            if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * sizeof(v[0]));
        };
        copy(type, sf->type);
        copy(seq, sf->seq);
        copy(strand, sf->strand);
        copy(coords, sf->coords);
        copy(end_span, sf->end_span);
        copy(included_ptr, sf->inc_ptr);
        copy(included_idx, sf->inc_idx);
        copy(excluded_ptr, sf->exc_ptr);
        copy(excluded_idx, sf->exc_idx);
        return POLEE_OK;
    });
}

extern "C" void polee_splice_destroy(polee_splice *sf) { delete sf; }
