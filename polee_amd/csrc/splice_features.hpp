// Splicing features from the transcripts' exon structure (polee_splice_*): what the device path
// (splice_features.hip) and its host twin (splice_features_host.cpp) share -- the packed keys, the records, the if / elseif chain
// of get_alt_donor_acceptor_sites (src/transcripts.jl:717-786) and the decoding of a feature's key into the table's columns.
//
// Every product of the derivation is a set of MEMBER rows (feature key, side, transcript): five 64-bit words, compared word by word.
// Sorting them and dropping repeats gives the features in the project's order and, within a feature, the included (side 0) and the
// excluded (side 1) transcripts ascending and unique -- whatever order the rows were made in.
//   w0  block << 56 | group    block: SP_CASSETTE .. SP_ALT3P (the table's block order);
//                              group: seq << 2 | (strand + 1), for the alternative ends gene << 1 | (0 start clusters, 1 end clusters)
//   w1  included_first << 32 | included_last
//   w2  excluded_first << 32 | excluded_last     (alternative ends: min_first << 32 | max_last, as upstream computes them)
//   w3  mutex exons: the outer interval of the group (two groups may hold the same pair of unions); alternative ends: seq << 2 | (strand + 1)
//   w4  side << 32 | transcript (1-based)
// Coordinates are 1 .. 2^31 - 2, so that first - 1 and last + 1 fit into 32 bits without a sign.
#pragma once
#include <cstdint>
#include <vector>

#include "common.hpp"

namespace polee {

constexpr int64_t SP_MAX_COORD = ((int64_t)1 << 31) - 2;
constexpr uint32_t SP_MERGE_DISTANCE = 250;  // get_alt_fp_tp_ends' merge_distance (transcripts.jl:851)
enum : uint64_t { SP_CASSETTE = 0, SP_MUTEX = 1, SP_ALTSITE = 2, SP_RETAINED = 3, SP_ALT5P = 4, SP_ALT3P = 5 };
// the `type` column
enum : int32_t { SP_T_CASSETTE = 0, SP_T_MUTEX = 1, SP_T_ACCEPTOR = 2, SP_T_DONOR = 3, SP_T_RETAINED = 4, SP_T_ALT5P = 5, SP_T_ALT3P = 6 };

__host__ __device__ inline uint64_t sp_pack(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }
__host__ __device__ inline uint32_t sp_hi(uint64_t w) { return (uint32_t)(w >> 32); }
__host__ __device__ inline uint32_t sp_lo(uint64_t w) { return (uint32_t)w; }
__host__ __device__ inline uint64_t sp_group(int32_t seq, int8_t strand) { return ((uint64_t)(uint32_t)seq << 2) | (uint64_t)(strand + 1); }

// an internal exon with its flanks: metadata[2] = the previous exon's last + 1, metadata[3] = the next exon's first - 1
struct SpExon {
    uint32_t first, last, m2, m3, tid;
};
// what one ordered pair (a, b) of overlapping internal exons gives: nothing (block < 0), an alternative site or a retained intron
struct SpEvent {
    int block;
    uint32_t c0, c1, c2, c3, inc, exc;
};

// transcripts.jl:717-786, the chain's order kept; the last branch compares with a.last, as written
__host__ __device__ inline SpEvent sp_eval(const SpExon &a, const SpExon &b)
{
    SpEvent e;
    e.block = -1;
    e.c0 = e.c1 = e.c2 = e.c3 = e.inc = e.exc = 0;
    if (a.m3 == b.m3 && a.last != b.last) {
        e.block = (int)SP_ALTSITE;
        e.c1 = e.c3 = a.m3;
        if (a.last < b.last) {
            e.c0 = a.last + 1, e.c2 = b.last + 1, e.inc = a.tid, e.exc = b.tid;
        } else {
            e.c2 = a.last + 1, e.c0 = b.last + 1, e.exc = a.tid, e.inc = b.tid;
        }
    } else if (a.m2 == b.m2 && a.first != b.first) {
        e.block = (int)SP_ALTSITE;
        e.c0 = e.c2 = a.m2;
        if (a.first > b.first) {
            e.c1 = b.first - 1, e.c3 = a.first - 1, e.inc = b.tid, e.exc = a.tid;
        } else {
            e.c3 = b.first - 1, e.c1 = a.first - 1, e.exc = b.tid, e.inc = a.tid;
        }
    } else if (a.m3 < b.last) {
        e.block = (int)SP_RETAINED;
        e.c0 = a.last + 1, e.c1 = a.m3, e.inc = b.tid, e.exc = a.tid;
    } else if (b.m3 < a.last) {
        e.block = (int)SP_RETAINED;
        e.c0 = b.last + 1, e.c1 = b.m3, e.inc = a.tid, e.exc = b.tid;
    } else if (a.m2 > b.first) {
        e.block = (int)SP_RETAINED;
        e.c0 = a.m2, e.c1 = a.first - 1, e.inc = b.tid, e.exc = a.tid;
    } else if (b.m2 > a.last) {
        e.block = (int)SP_RETAINED;
        e.c0 = b.m2, e.c1 = b.first - 1, e.inc = a.tid, e.exc = b.tid;
    }
    return e;
}

// number of clusters to emit for a side with `nclusters` of them (transcripts.jl:891-916: none for one, the first of exactly two)
__host__ __device__ inline uint32_t sp_emitted_clusters(uint32_t nclusters) { return nclusters <= 1 ? 0u : nclusters == 2 ? 1u : nclusters; }
// the block of a start (kind 0) or end (kind 1) cluster: starts are 5' ends on the plus strand only (:906-910, :935-939)
__host__ __device__ inline uint64_t sp_end_block(int kind, int8_t strand) { return ((kind == 0) == (strand == 1)) ? SP_ALT5P : SP_ALT3P; }

struct SpMember {
    uint64_t w[5];
    bool operator<(const SpMember &o) const
    {
        for (int k = 0; k < 5; ++k)
            if (w[k] != o.w[k]) return w[k] < o.w[k];
        return false;
    }
    bool operator==(const SpMember &o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3] && w[4] == o.w[4]; }
};

}  // namespace polee

// the result, on the host whichever path made it
struct polee_splice {
    polee_ctx *ctx = nullptr;  // (none: nothing of the result stays on a device)
    std::vector<int32_t> type, seq;
    std::vector<int8_t> strand;
    std::vector<int64_t> coords, end_span;  // [F][4], [F][2]
    std::vector<int64_t> inc_ptr, exc_ptr;  // [F+1]
    std::vector<int32_t> inc_idx, exc_idx;
    int64_t num_exons = 0, num_internal = 0, num_pairs = 0;
};

namespace polee {

// sizes, order and ranges of the input; E = the number of exons, NX = the number of internal ones
polee_status sp_validate(polee_ctx *ctx, const char *who, const polee_xb_transcripts *T, const int32_t *gene_of, int64_t *E, int64_t *NX);
// the table's columns of feature f from the first four words of its key
void sp_decode(polee_splice &r, size_t f, const uint64_t *w);
// sizes the result for F features (inc_ptr / exc_ptr and the index lists stay the caller's)
void sp_resize(polee_splice &r, size_t F);

struct SpClock {  // POLEE_BUILD_TIMING=1: the phases on stderr
    bool on = getenv("POLEE_BUILD_TIMING") != nullptr;
    double t0;
    static double now()
    {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
    }
    SpClock() : t0(now()) {}
    void lap(const char *what, hipStream_t stream = nullptr, bool sync = false)
    {
        if (!on) return;
        if (sync) (void)hipStreamSynchronize(stream);
        fprintf(stderr, "[splicing]   . %-28s %.4f s\n", what, now() - t0);
        t0 = now();
    }
};

}  // namespace polee
