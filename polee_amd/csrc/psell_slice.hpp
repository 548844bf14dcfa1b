// The byte format of a PSELL slice (the layout itself: loglik_internal.hpp): its geometry, its offset word, its header words and the
// one decoder every lane-by-lane reader uses.  Everything here is constexpr or __host__ __device__ inline and keeps no state: the two
// builders (psell_build.cpp emit_slice on the host, psell_device.hip s3_emit_kernel on the device) lay a slice out by
// psell_slice_geom and the word helpers, the two kernels that decode ANY slice (psell_tile_body in loglik.hip: stream B and the
// cross-check; em_g64_tiles_kernel in em.hip: the f64 gradient behind the EM fixed-point residual) read it through
// PsellSliceReader, and tests/san/host_builders_main.cpp runs that reader on the host against the input matrix.
//
//   * Rows are split into six streams, each a contiguous range of tiles (in this order):
//       A1, A1M, A2, A2M = UNIFORM slices: all rows of a slice are stored under ONE transcript set, kept once per slice.
//         A1  (dense, sets of <= 16): uint16 lcol[128] header + float val[w][64], 4 B per entry: whole 64-row slices of
//              every run of identical rows, run remainders of >= 32 rows (zero padded), and dense UNION slices -- leftover
//              rows of neighbouring sets packed under the union of their sets with zeros where a row lacks a transcript
//              (a zero adds nothing to a row sum or a gradient, exactly) -- when the union is (almost) full.
//         A1M (MASKED, unions of <= 16): leftover rows whose sets differ -- any 64 rows whose union has <= 16 transcripts.
//              Header: uint32 hw[64] -- low half of hw[r] = the mask of fragment r (bit t: it is compatible with
//              transcript t of the union), high half of hw[t], t < 16, = the tile-local id of transcript t (0x8000 past
//              the union); then float val[i][64], the i-th non-zero of fragment r at position r of row i, for i < the
//              longest row of the slice.  (Every 32-bit word of a slice is a FINITE float -- ids < 128 or 0x8000 in the
//              high halves: the dense streams' kernels read the rows behind a slice's last transcript from their LDS
//              rings and multiply them by zero, and a ring may still hold a masked tile's bytes.)  Zeros cost no bytes: 4 B per non-zero + 4 B per
//              fragment + padding to the slice's longest row -- never more than the dense union slice, and below CSR's
//              8 B per non-zero + 4 B per fragment whatever the sets look like.  The kernel expands a fragment's values
//              with its mask (rank = popcount of the lower bits) and runs the same matrix-core phases.
//         A2  (dense, sets of 17..32): runs, remainders and union slices that are (almost) full.
//         A2M (MASKED, unions of 17..32): the leftover rows that fit no union of 16 -- fragments of a gene with many
//              isoforms.  Header: two rows of uint32 hw[64] (mask bits 0..15 / 16..31 in the low halves, the ids of
//              transcripts 0..15 / 16..31 in the high halves of each row's first sixteen words); values as in A1M.
//       BN, B = MIXED slices (float val[w][64]; uint16 lcol[w][64], 6 B per entry, any 64 fragments of the tile): the
//              leftover rows that fit no uniform slice at CSR's cost or less -- unrelated fragments, fewer than a handful
//              of which share any 32 transcripts.  BN: rows of <= 15 transcripts (with multiplicities a row float ks[64]
//              follows, at the next multiple of 256 bytes), lane = fragment, gathers from / LDS adds into the tile's
//              windows.
//         One persistent launch (loglik_stream_kernel) streams these five: the usual sample needs no other.
//              B: rows of more than 16 transcripts that found no uniform slice (more than 32, as a rule); the per-tile
//              kernel loglik_psell_kernel takes them in a second launch.  That kernel also runs over all other slices
//              on request (polee_debug_loglik_force_mixed): the independent second algorithm of the cross-check tests.
//       C     = rows kept in CSR (u32 ids, f32 values, u32 row offsets: 8 B per non-zero + 4 B per row): fragments with no structure at all,
//              whose mixed tiles would close on the dictionary before a slice is full -- the last resort that keeps
//              the layout below CSR's size for ANY matrix; loglik_csr_kernel (lane = row, global gathers / atomics).
//       S     = fragments compatible with ONE transcript (54 % of the rows of the reference's real-data fixture): not stored at
//              all.  Such a fragment adds log(X_ij) + log(x_j) to the log-likelihood and 1 / x_j to transcript j's
//              gradient (X_ij cancels: X_ij / (X_ij x_j)), ks_i times with multiplicities -- so the build keeps c_j = the
//              number of such fragments per transcript (single_cnt) and the constant sum of log X_ij (single_logsum), and
//              a pass adds c_j / x_j[k] and c_j log x_j[k] + const (single_rows_kernel): 4 B per TRANSCRIPT instead of
//              8 B + a slice lane per fragment.
//   * Each slice carries two flag bits (in the top bits of its offset word): "uniform" (its rows
//     are stored under one transcript set) and "continues" (the same set as the previous slice).  Runs of such
//     slices -- the bulk of real and synthetic data, where many fragments fall into the same
//     equivalence class -- keep their gradient contributions in registers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace polee {

constexpr int PSELL_LANES = 64;
enum : int { PSELL_A1 = 0, PSELL_A1M = 1, PSELL_A2 = 2, PSELL_A2M = 3, PSELL_BN = 4, PSELL_B = 5, PSELL_C = 6, PSELL_S = 7, PSELL_NSTREAMS = 8 };  // streams, in tile order (C and S have no tiles)

// ---- tile -> stream ------------------------------------------------------------------------------------------------------------
struct PsellTileBounds {  // the streams' tile ranges: A1 = [0, a1), A1M = [a1, a1m), A2 = [a1m, a2), A2M = [a2, a), BN = [a, s), B = the rest
    int a1, a1m, a2, a, s;
};
__host__ __device__ constexpr int psell_stream_of_tile(const PsellTileBounds &b, int64_t tile)
{
    return tile < b.a1 ? PSELL_A1 : (tile < b.a1m ? PSELL_A1M : (tile < b.a2 ? PSELL_A2 : (tile < b.a ? PSELL_A2M : (tile < b.s ? PSELL_BN : PSELL_B))));
}

// ---- the three slice formats ---------------------------------------------------------------------------------------------------
enum : int { PSELL_COMPACT = 0, PSELL_MASKED = 1, PSELL_MIXED = 2 };
// `masked`: the slice's own mark (the builders: its rows' form is 2; the readers: bit 29 of its offset word).  Every slice of streams
// A1M / A2M is masked; stream A1 carries marked masked slices behind its dense ones; no other stream has any.
__host__ __device__ constexpr int psell_kind(int stream, bool masked)
{
    return stream >= PSELL_BN ? PSELL_MIXED : (stream == PSELL_A1M || stream == PSELL_A2M || (stream == PSELL_A1 && masked) ? PSELL_MASKED : PSELL_COMPACT);
}
__host__ __device__ constexpr int psell_hdr_rows(int stream) { return stream == PSELL_A2M ? 2 : 1; }  // 256-byte header rows of a uniform slice
// with multiplicities every slice the persistent launch streams ends in a row float ks[64]; stream B's do not
__host__ __device__ constexpr bool psell_has_ks_row(int stream, bool has_ks) { return has_ks && stream != PSELL_B; }

// Uniform slices store fragment r of transcript row t at this position of the row's 64 values, chosen per stream so that
// the kernel's LDS operand reads are bank-conflict free: A1 (batched 4 x 4 outer products, narrow_stream) r ^ (t & 3);
// A2 (16 x 16 x 4 tiles, wide_stream) a rotation by 4 t.
__host__ __device__ constexpr uint32_t psell_row_pos(int stream, uint32_t t, uint32_t r) { return stream == PSELL_A1 ? (r ^ (t & 3u)) : (stream == PSELL_A2 ? ((r + 4u * t) & 63u) : r); }

// Byte offsets of a slice's parts from its start, and its size (a multiple of 128).  `rows` = rows of 64 values the slice stores: the
// set's transcripts (compact), the longest fragment (masked, mixed).
//   compact  uint16 lcol[128] | float val[rows][64] | (float ks[64])
//   masked   uint32 hw[hdr rows][64] | float val[rows][64] | (float ks[64])
//   mixed    float val[rows][64] | uint16 lcol[rows][64] | padding to 256 bytes | (BN: float ks[64])
struct PsellSliceGeom {
    uint32_t hdr, val, lcol, ks, bytes;  // (hdr: uniform slices; lcol: mixed slices; ks: where the row is, or would be)
};
__host__ __device__ constexpr PsellSliceGeom psell_slice_geom(int stream, bool masked, uint32_t rows, bool has_ks)
{
    const uint32_t ks_bytes = psell_has_ks_row(stream, has_ks) ? 256u : 0u;
    if (psell_kind(stream, masked) == PSELL_MIXED) {
        const uint32_t body = (rows * 384u + 255u) & ~255u;
        return PsellSliceGeom{0u, 0u, rows * 256u, body, body + ks_bytes};
    }
    const uint32_t val = 256u * (uint32_t)psell_hdr_rows(stream), ks = val + rows * 256u;
    return PsellSliceGeom{0u, val, 0u, ks, ks + ks_bytes};
}
// the inverse: a slice's rows from its size in 128-byte units
__host__ __device__ constexpr int psell_rows_from_units(int kind, int hrows, uint32_t units, bool has_ks_row)
{
    return kind == PSELL_MIXED ? (int)((units - (has_ks_row ? 2u : 0u)) / 3u) : (int)(units / 2u) - hrows - (has_ks_row ? 1 : 0);
}

// ---- the offset word: slice_off[s] = the slice's start in 128-byte units, its flags on top ------------------------------------------
constexpr uint32_t PSELL_OFF_MASK = 0x1fffffffu;  // slice_off entries carry the slice flags in bits 29..31
constexpr uint32_t PSELL_FLAG_MASKED_BIT = 29;    // bit 29: a MASKED slice (set for every slice of streams A1M / A2M; the cross-check kernel reads it)
// flags as the builders keep them: bit 0 uniform -> bit 30, bit 1 continues the previous slice's set -> bit 31, bit 2 masked -> bit 29
__host__ __device__ constexpr uint32_t psell_pack_off(uint32_t units, uint32_t flags)
{
    return units | ((flags & 3u) << 30) | (((flags >> 2) & 1u) << PSELL_FLAG_MASKED_BIT);
}
__host__ __device__ constexpr uint32_t psell_off_units(uint32_t e) { return e & PSELL_OFF_MASK; }
__host__ __device__ constexpr uint32_t psell_off_flags(uint32_t e) { return e >> 30; }  // bit 0 uniform, bit 1 continues
__host__ __device__ constexpr bool psell_off_masked(uint32_t e) { return ((e >> PSELL_FLAG_MASKED_BIT) & 1u) != 0; }

// ---- the header words of a masked slice: uint32 hw[hdr rows][64] --------------------------------------------------------------------
constexpr uint16_t PSELL_NO_COL = 0x8000u;  // header entries of a masked slice past its union (0x8000xxxx is a finite float)
// transcript t's id (or PSELL_NO_COL) rides in the high half of word psell_masked_id_slot(t), a lane's mask in the low halves of words
// lane (bits 0..15) and 64 + lane (bits 16..31): word = psell_masked_id_word(..) | psell_masked_mask_word(..)
__host__ __device__ constexpr uint32_t psell_masked_id_slot(uint32_t t) { return 64u * (t >> 4) + (t & 15u); }
__host__ __device__ constexpr uint32_t psell_masked_id_word(uint32_t local_id) { return local_id << 16; }
__host__ __device__ constexpr uint32_t psell_masked_mask_word(uint32_t mk, uint32_t hrow) { return hrow == 0 ? (mk & 0xffffu) : (mk >> 16); }
// ... and read back through the header's 16-bit halves
__host__ __device__ inline uint16_t psell_masked_id(const uint16_t *hdr, int t) { return hdr[128 * (t >> 4) + 2 * (t & 15) + 1]; }
__host__ __device__ inline uint32_t psell_masked_mask(const uint16_t *hdr, int hrows, int lane)
{
    uint32_t mk = hdr[2 * lane];
    if (hrows == 2) mk |= (uint32_t)hdr[128 + 2 * lane] << 16;
    return mk;
}

// ---- one lane's view of one slice -----------------------------------------------------------------------------------------------
// e0, e1: the slice's and the next slice's offset words.  The lane's row is (col(t), value(t)), t < w, col = the tile-local id: a
// compact slice gives every lane the set's w transcripts (zeros where a union row lacks one), a masked slice likewise with the
// lane's values expanded by its mask (rank = popcount of the lower bits), a mixed slice the lane's own entries padded to the
// slice's longest row with zeros under the last id.
struct PsellSliceReader {
    const uint16_t *hdr;  // uniform slices: the header
    const float *vbase;
    const uint16_t *cols;  // compact: the set's ids; mixed: the lane's column of lcol
    uint32_t mk;  // masked: the lane's mask
    int stream, lane, w;
    bool masked, mixed;
    __host__ __device__ PsellSliceReader(const uint8_t *data, uint32_t e0, uint32_t e1, int stream_, bool has_ks, int lane_) : stream(stream_), lane(lane_)
    {
        const int kind = psell_kind(stream, psell_off_masked(e0)), hrows = psell_hdr_rows(stream);
        masked = kind == PSELL_MASKED;
        mixed = kind == PSELL_MIXED;
        const uint8_t *base = data + (size_t)psell_off_units(e0) * 128;
        const int rows = psell_rows_from_units(kind, hrows, psell_off_units(e1) - psell_off_units(e0), psell_has_ks_row(stream, has_ks));
        const PsellSliceGeom G = psell_slice_geom(stream, masked, (uint32_t)rows, has_ks);
        hdr = reinterpret_cast<const uint16_t *>(base + G.hdr);
        vbase = reinterpret_cast<const float *>(base + G.val);
        cols = mixed ? reinterpret_cast<const uint16_t *>(base + G.lcol) + lane : hdr;
        w = rows;
        mk = 0;
        if (masked) {  // (rows = the longest fragment; the lanes' rows run over the union)
            w = 0;
            while (w < 16 * hrows && psell_masked_id(hdr, w) != PSELL_NO_COL) ++w;
            mk = psell_masked_mask(hdr, hrows, lane);
        }
    }
    __host__ __device__ float value(int t) const
    {
        if (masked) return (mk >> t) & 1u ? vbase[__builtin_popcount(mk & ((1u << t) - 1u)) * 64 + lane] : 0.0f;
        return vbase[t * 64 + (mixed ? lane : (int)psell_row_pos(stream, (uint32_t)t, (uint32_t)lane))];
    }
    __host__ __device__ int col(int t) const { return masked ? (int)psell_masked_id(hdr, t) : (int)cols[mixed ? t * 64 : t]; }
};

}  // namespace polee
