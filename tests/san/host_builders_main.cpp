// Sanitizer driver for the HOST builders of libpolee_hip: the layout builder (psell_build.cpp, through
// polee_debug_psell_build: csc_to_csr's partitioned transposition, keys / radix sort / runs, the two packing passes, slice
// emission in parallel chunks), the tree heuristic in the reference's order (polee_hclust) and in rounds on all host threads
// (polee_hclust_parallel: unions, candidate lists and list updates under striped spin locks).  Built host-only
// (--offload-host-only) with -fsanitize=address,undefined or -fsanitize=thread by `make -C polee_amd/csrc sanitize SAN=...`
// and run by tests/test_sanitizers.py; it touches no GPU.  Exit code 0 = every call succeeded and its output is well-formed
// (the sanitizer itself aborts on a finding).
// Every layout is also DECODED on the host, lane by lane, through the reader the device decoders use (PsellSliceReader,
// polee_amd/csrc/psell_slice.hpp) and held against the input matrix: check_decode below.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/polee_hip.h"
#include "../../include/polee_hip_debug.h"
#include "../../polee_amd/csrc/psell_slice.hpp"

struct Csc {
    int64_t m, n;
    std::vector<uint64_t> colptr;  // 1-based
    std::vector<uint32_t> rowval;  // 1-based
    std::vector<float> nzval;
};

// kind 0: genes with compatibility patterns (runs); 1: every fragment its own subset; 2: unstructured; 3: wide genes + strays
// + empty fragments
static Csc make(int kind, int64_t n, int64_t m, uint64_t seed)
{
    std::mt19937_64 rng(seed);
    std::vector<std::vector<uint32_t>> rows((size_t)m);
    std::vector<int64_t> gene_start;
    for (int64_t j = 0; j < n;) {
        gene_start.push_back(j);
        j += 1 + (int64_t)(rng() % (kind == 3 ? 40 : 12));
    }
    gene_start.push_back(n);
    const size_t G = gene_start.size() - 1;
    for (int64_t i = 0; i < m; ++i) {
        auto &r = rows[(size_t)i];
        if (kind == 3 && rng() % 50 == 0) continue;  // an empty fragment
        if (kind == 2) {
            const int k = 1 + (int)(rng() % 6);
            for (int t = 0; t < k; ++t) r.push_back((uint32_t)(rng() % (uint64_t)n));
        } else {
            const size_t g = (size_t)(rng() % G);
            const int64_t a = gene_start[g], b = std::min<int64_t>(gene_start[g + 1], n);
            if (kind == 0) {
                const uint64_t pat = 1 + (g * 7919 + rng() % 5) * 2654435761ull;
                for (int64_t j = a; j < b; ++j)
                    if ((pat >> ((j - a) % 60)) & 1) r.push_back((uint32_t)j);
                if (r.empty()) r.push_back((uint32_t)a);
            } else {
                for (int64_t j = a; j < b; ++j)
                    if (rng() % 4) r.push_back((uint32_t)j);
                if (r.empty()) r.push_back((uint32_t)a);
                if (kind == 3 && rng() % 20 == 0) r.push_back((uint32_t)(rng() % (uint64_t)n));  // a stray
            }
        }
        std::sort(r.begin(), r.end());
        r.erase(std::unique(r.begin(), r.end()), r.end());
    }
    Csc X;
    X.m = m;
    X.n = n;
    X.colptr.assign((size_t)n + 1, 0);
    for (auto &r : rows)
        for (uint32_t j : r) ++X.colptr[(size_t)j + 1];
    X.colptr[0] = 1;
    for (int64_t j = 0; j < n; ++j) X.colptr[(size_t)j + 1] += X.colptr[(size_t)j];
    const size_t nnz = (size_t)(X.colptr[(size_t)n] - 1);
    X.rowval.resize(nnz);
    X.nzval.resize(nnz);
    std::vector<uint64_t> cur(X.colptr.begin(), X.colptr.end() - 1);
    std::uniform_real_distribution<float> u(1e-6f, 1e-2f);
    for (int64_t i = 0; i < m; ++i)
        for (uint32_t j : rows[(size_t)i]) {
            const size_t p = (size_t)(cur[j]++ - 1);
            X.rowval[p] = (uint32_t)(i + 1);
            X.nzval[p] = u(rng);
        }
    return X;
}

// Every slice of the layout read back through PsellSliceReader, lanes 0..63: a lane's non-zero (transcript, value) pairs are exactly
// its fragment's row of X (bit-equal floats; zeros -- union slices' gaps, mixed slices' padding -- count only where X holds one), an
// empty lane decodes to no non-zero, the slice's size is what psell_slice_geom says, and with multiplicities its ks row is slice_ks.
static int check_decode(const char *what, const Csc &X, const polee_psell_view &v, bool has_ks)
{
    using polee::PsellSliceGeom;
    typedef std::pair<uint32_t, uint32_t> Entry;  // (transcript, the value's bits)
    auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
    std::vector<uint64_t> rowptr((size_t)X.m + 1, 0);
    for (uint32_t r : X.rowval) ++rowptr[r];  // (1-based: row i counts into rowptr[i + 1])
    for (int64_t i = 0; i < X.m; ++i) rowptr[(size_t)i + 1] += rowptr[(size_t)i];
    std::vector<Entry> ent(X.rowval.size());
    {
        std::vector<uint64_t> cur(rowptr.begin(), rowptr.end() - 1);
        for (int64_t j = 0; j < X.n; ++j)
            for (uint64_t p = X.colptr[(size_t)j] - 1; p < X.colptr[(size_t)j + 1] - 1; ++p) ent[cur[X.rowval[p] - 1]++] = Entry((uint32_t)j, bits(X.nzval[p]));
    }
    const polee::PsellTileBounds tb{(int)v.num_tiles_a1, (int)v.num_tiles_a1m, (int)v.num_tiles_a2, (int)v.num_tiles_a, (int)v.num_tiles_s};
    int bad = 0;
    std::vector<Entry> got;
    for (int64_t tile = 0; tile < v.num_tiles && bad < 5; ++tile) {
        const int stream = polee::psell_stream_of_tile(tb, tile);
        const uint32_t d0 = v.tile_dict[tile], L = v.tile_dict[tile + 1] - d0;
        for (uint32_t s = v.tile_slice[tile]; s < v.tile_slice[tile + 1] && bad < 5; ++s) {
            const uint32_t e0 = v.slice_off[s], e1 = v.slice_off[s + 1], units = polee::psell_off_units(e1) - polee::psell_off_units(e0);
            const bool masked = polee::psell_off_masked(e0);
            const int kind = polee::psell_kind(stream, masked);
            const int rows = polee::psell_rows_from_units(kind, polee::psell_hdr_rows(stream), units, polee::psell_has_ks_row(stream, has_ks));
            const PsellSliceGeom G = polee::psell_slice_geom(stream, masked, (uint32_t)rows, has_ks);
            if (rows < 0 || G.bytes != units * 128u || (size_t)polee::psell_off_units(e1) * 128 > (size_t)v.data_bytes) {
                fprintf(stderr, "%s: slice %u of stream %d: %u units, %d rows, %u bytes by its geometry\n", what, s, stream, units, rows, G.bytes);
                ++bad;
                continue;
            }
            if (polee::psell_has_ks_row(stream, has_ks) &&
                memcmp(v.data + (size_t)polee::psell_off_units(e0) * 128 + G.ks, v.slice_ks + (size_t)s * 64, 256) != 0) {
                fprintf(stderr, "%s: slice %u of stream %d: its ks row is not slice_ks\n", what, s, stream);
                ++bad;
            }
            for (int lane = 0; lane < 64; ++lane) {
                const polee::PsellSliceReader R(v.data, e0, e1, stream, has_ks, lane);
                const uint32_t r = v.row_order[(size_t)s * 64 + lane];
                const Entry *rb = r != ~0u ? ent.data() + rowptr[r] : nullptr, *re = r != ~0u ? ent.data() + rowptr[r + 1] : nullptr;
                got.clear();
                bool in_dict = true;
                for (int t = 0; t < R.w; ++t) {
                    const uint32_t c = (uint32_t)R.col(t);
                    const float val = R.value(t);
                    if (c >= L) {
                        in_dict = in_dict && val == 0.0f && kind == polee::PSELL_MASKED;  // (only PSELL_NO_COL may point past the dictionary)
                        continue;
                    }
                    const Entry e(v.dict[d0 + c], bits(val));
                    if (val != 0.0f || (rb && std::binary_search(rb, re, e))) got.push_back(e);
                }
                std::sort(got.begin(), got.end());
                if (!in_dict || got.size() != (size_t)(re - rb) || !std::equal(got.begin(), got.end(), rb)) {
                    fprintf(stderr, "%s: slice %u of stream %d (kind %d), lane %d, fragment %lld: decoded %zu entries, X has %zu\n", what, s, stream, kind,
                            lane, r != ~0u ? (long long)r : -1ll, got.size(), (size_t)(re - rb));
                    if (++bad >= 5) break;
                }
            }
        }
    }
    return bad;
}

static int check_tree(const char *what, int64_t n, const std::vector<int32_t> &par, const std::vector<int32_t> &js)
{
    // serialised tree (src/ptt.jl:89-116): 2n-1 nodes, node 1 the root (parent 0), parents precede children, n leaves
    int64_t leaves = 0;
    for (size_t i = 0; i < par.size(); ++i) {
        if (i == 0 ? par[i] != 0 : (par[i] < 1 || par[i] > (int32_t)i)) {
            fprintf(stderr, "%s: node %zu has parent %d\n", what, i + 1, par[i]);
            return 1;
        }
        if (js[i] != 0) ++leaves;
    }
    if (leaves != n) {
        fprintf(stderr, "%s: %lld leaves, expected %lld\n", what, (long long)leaves, (long long)n);
        return 1;
    }
    return 0;
}

int main(int argc, char **argv)
{
    const int64_t scale = argc > 1 ? atoll(argv[1]) : 1;
    setenv("POLEE_HOST_THREADS", "8", 0);
    int bad = 0;
    int64_t stream_nnz[6] = {};  // per sliced stream, over every layout built: the decode check has to see all six slice forms
    for (int kind = 0; kind < 4; ++kind) {
        const int64_t n = 3000 * scale, m = 200000 * scale;
        Csc X = make(kind, n, m, 1234 + (uint64_t)kind);
        std::vector<int64_t> ks((size_t)m);
        for (int64_t i = 0; i < m; ++i) ks[(size_t)i] = 1 + (i * 2654435761ll) % 5;
        for (int with_ks = 0; with_ks < 2; ++with_ks) {
            polee_psell_debug *h = nullptr;
            polee_status st = polee_debug_psell_build(X.m, X.n, X.colptr.data(), 8, X.rowval.data(), X.nzval.data(),
                                                      with_ks ? ks.data() : nullptr, &h);
            if (st != POLEE_OK) {
                fprintf(stderr, "layout, kind %d: status %d: %s\n", kind, (int)st, polee_last_error(nullptr));
                ++bad;
                continue;
            }
            polee_psell_view v;
            if (polee_debug_psell_view(h, &v) != POLEE_OK || v.m != X.m || v.n != X.n) {
                fprintf(stderr, "layout, kind %d: bad view\n", kind);
                ++bad;
            }
            // every stored fragment appears once: slices' lanes + CSR rows + collapsed single-transcript rows + empties
            std::vector<uint8_t> seen((size_t)m, 0);
            int64_t dup = 0, cnt = 0;
            for (int64_t s = 0; s < v.num_slices * 64; ++s)
                if (v.row_order[s] != ~0u) dup += seen[v.row_order[s]]++, ++cnt;
            for (int64_t r = 0; r < v.csr_num_rows; ++r) dup += seen[v.csr_rows[r]]++, ++cnt;
            for (int64_t r = 0; r < v.single_num_rows; ++r) dup += seen[v.single_rows[r]]++, ++cnt;
            if (dup != 0 || cnt + v.num_empty_rows != m) {
                fprintf(stderr, "layout, kind %d: %lld fragments accounted for of %lld (%lld twice, %lld empty)\n", kind, (long long)cnt,
                        (long long)m, (long long)dup, (long long)v.num_empty_rows);
                ++bad;
            }
            bad += check_decode(with_ks ? "decode (with ks)" : "decode", X, v, with_ks != 0);
            for (int q = 0; q < 6; ++q) stream_nnz[q] += v.stream_nnz[q];
            polee_debug_psell_free(h);
        }
        std::vector<int32_t> par((size_t)(2 * n - 1)), js((size_t)(2 * n - 1)), par2(par), js2(js);
        if (polee_hclust_parallel(X.m, X.n, X.colptr.data(), 8, X.rowval.data(), par.data(), js.data()) != POLEE_OK) {
            fprintf(stderr, "hclust_parallel, kind %d: %s\n", kind, polee_last_error(nullptr));
            ++bad;
        } else {
            bad += check_tree("hclust_parallel", n, par, js);
        }
        if (kind < 2) {  // (the exact mode is sequential: once per structure is enough)
            if (polee_hclust(X.m, X.n, X.colptr.data(), 8, X.rowval.data(), par2.data(), js2.data()) != POLEE_OK) {
                fprintf(stderr, "hclust, kind %d: %s\n", kind, polee_last_error(nullptr));
                ++bad;
            } else {
                bad += check_tree("hclust", n, par2, js2);
            }
        }
        polee_host_cache_trim();
    }
    for (int q = 0; q < 6; ++q)
        if (stream_nnz[q] == 0) {
            fprintf(stderr, "no layout has a slice of stream %d (A1, A1M, A2, A2M, BN, B = 0..5): the decode check did not see that form\n", q);
            ++bad;
        }
    printf("host builders under the sanitizer: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
