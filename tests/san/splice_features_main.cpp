// Sanitizer driver for the host twin of the splicing features (polee_amd/csrc/splice_features_host.cpp): the features of a generated
// annotation of 40 000 transcripts -- genes of 1 to 12 isoforms over a shared pool of exons with skipped exons, shifted splice sites,
// retained introns and shifted ends, with and without the alternative ends -- large enough for the sorts and the overlap join to run on
// all host threads.  Built host-only (--offload-host-only) with -fsanitize=address,undefined and with -fsanitize=thread by
// `make -C polee_amd/csrc sanitize-splice-features` and run there on the CPU; it touches no GPU and is not loaded into Python.  Exit code
// 0 = every call did what it should, the tables are well-formed and a second call gives the same ones (the sanitizer itself aborts on a
// finding).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/polee_hip.h"

static int fails = 0;
#define REQUIRE(cond)                                                   \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__);  \
            ++fails;                                                    \
        }                                                               \
    } while (0)

struct Result {
    int64_t F = 0, ni = 0, ne = 0, exons = 0, inner = 0, pairs = 0;
    std::vector<int32_t> type, seq, inc_idx, exc_idx;
    std::vector<int8_t> strand;
    std::vector<int64_t> coords, span, inc_ptr, exc_ptr;
    bool operator==(const Result &o) const
    {
        return F == o.F && pairs == o.pairs && type == o.type && seq == o.seq && strand == o.strand && coords == o.coords && span == o.span &&
               inc_ptr == o.inc_ptr && exc_ptr == o.exc_ptr && inc_idx == o.inc_idx && exc_idx == o.exc_idx;
    }
};

static Result run(const polee_xb_transcripts &T, const int32_t *gene_of)
{
    Result r;
    polee_splice *sf = nullptr;
    REQUIRE(polee_splice_run_host(&T, gene_of, &sf) == POLEE_OK);
    if (!sf) return r;
    REQUIRE(polee_splice_sizes(sf, &r.F, &r.ni, &r.ne, &r.exons, &r.inner, &r.pairs) == POLEE_OK);
    r.type.resize((size_t)r.F);
    r.seq.resize((size_t)r.F);
    r.strand.resize((size_t)r.F);
    r.coords.resize((size_t)r.F * 4);
    r.span.resize((size_t)r.F * 2);
    r.inc_ptr.resize((size_t)r.F + 1);
    r.exc_ptr.resize((size_t)r.F + 1);
    r.inc_idx.resize((size_t)r.ni);
    r.exc_idx.resize((size_t)r.ne);
    REQUIRE(polee_splice_get(sf, r.type.data(), r.seq.data(), r.strand.data(), r.coords.data(), r.span.data(), r.inc_ptr.data(), r.inc_idx.data(),
                             r.exc_ptr.data(), r.exc_idx.data()) == POLEE_OK);
    REQUIRE(polee_splice_get(sf, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == POLEE_OK);
    polee_splice_destroy(sf);
    return r;
}

static bool well_formed(const Result &r, int32_t n, bool ends)
{
    static const int block_of[7] = {0, 1, 2, 2, 3, 4, 5};
    for (int side = 0; side < 2; ++side) {
        const std::vector<int64_t> &ptr = side ? r.exc_ptr : r.inc_ptr;
        const std::vector<int32_t> &idx = side ? r.exc_idx : r.inc_idx;
        if (ptr[0] != 0 || ptr[(size_t)r.F] != (int64_t)idx.size()) return false;
        for (int64_t f = 0; f < r.F; ++f) {
            if (ptr[(size_t)f + 1] <= ptr[(size_t)f]) return false;  // (no feature without members on either side)
            for (int64_t k = ptr[(size_t)f]; k < ptr[(size_t)f + 1]; ++k) {
                if (idx[(size_t)k] < 1 || idx[(size_t)k] > n) return false;
                if (k > ptr[(size_t)f] && idx[(size_t)k] <= idx[(size_t)k - 1]) return false;
            }
        }
    }
    for (int64_t f = 0; f < r.F; ++f) {
        if (r.type[(size_t)f] < 0 || r.type[(size_t)f] > (ends ? 6 : 4)) return false;
        if (f > 0 && block_of[r.type[(size_t)f]] < block_of[r.type[(size_t)f - 1]]) return false;
        if ((r.span[(size_t)f * 2] >= 0) != (r.type[(size_t)f] >= 5)) return false;
    }
    return true;
}

int main()
{
    std::mt19937_64 rng(5);
    const int32_t n = 40000;
    std::vector<int32_t> seq, gene;
    std::vector<int8_t> strand;
    std::vector<int64_t> ptr(1, 0), first, last;
    int64_t cursor[3] = {2000, 2000, 2000};
    for (int32_t g = 1; (int32_t)seq.size() < n; ++g) {
        const int s = (int)(rng() % 3), k = 3 + (int)(rng() % 10);
        const int8_t sd = rng() % 2 ? 1 : -1;
        std::vector<int64_t> pf, pl;
        int64_t pos = cursor[s];
        for (int e = 0; e < k; ++e) {
            const int64_t len = 80 + (int64_t)(rng() % 300);
            pf.push_back(pos);
            pl.push_back(pos + len - 1);
            pos += len + 300 + (int64_t)(rng() % 2000);
        }
        cursor[s] = pos + 3000;
        const int isoforms = 1 + (int)(rng() % 12);
        for (int i = 0; i < isoforms && (int32_t)seq.size() < n; ++i) {
            std::vector<int64_t> f, l;
            for (int e = 0; e < k; ++e) {
                if (e > 0 && e + 1 < k && rng() % 4 == 0) continue;
                if (!f.empty() && rng() % 10 == 0) {  // a retained intron
                    l.back() = pl[(size_t)e];
                    continue;
                }
                f.push_back(pf[(size_t)e] + (e > 0 && rng() % 6 == 0 ? 12 : 0));
                l.push_back(pl[(size_t)e] + (e + 1 < k && rng() % 6 == 0 ? 27 : 0));
            }
            f.front() -= (int64_t)(rng() % 3) * 300;
            l.back() += (int64_t)(rng() % 3) * 300;
            first.insert(first.end(), f.begin(), f.end());
            last.insert(last.end(), l.begin(), l.end());
            ptr.push_back((int64_t)first.size());
            seq.push_back(s);
            strand.push_back(sd);
            gene.push_back(g);
        }
    }
    polee_xb_transcripts T{n, seq.data(), strand.data(), ptr.data(), first.data(), last.data()};
    const Result with = run(T, gene.data()), again = run(T, gene.data()), without = run(T, nullptr);
    REQUIRE(with.F > 1000 && with.pairs > 1000 && with.exons == (int64_t)first.size());
    REQUIRE(well_formed(with, n, true));
    REQUIRE(well_formed(without, n, false));
    REQUIRE(with == again);
    REQUIRE(without.F < with.F && without.pairs == with.pairs);
    bool seen[7] = {false, false, false, false, false, false, false};
    for (int32_t t : with.type) seen[t] = true;
    for (int t = 0; t < 7; ++t) REQUIRE(seen[t]);
    // refusals: no transcripts, overlapping exons, a coordinate beyond the range, a gene number of 0
    polee_splice *sf = nullptr;
    polee_xb_transcripts none{0, seq.data(), strand.data(), ptr.data(), first.data(), last.data()};
    REQUIRE(polee_splice_run_host(&none, nullptr, &sf) == POLEE_ERR_BAD_ARG && sf == nullptr);
    REQUIRE(polee_splice_run_host(nullptr, nullptr, &sf) == POLEE_ERR_BAD_ARG);
    REQUIRE(polee_splice_run_host(&T, nullptr, nullptr) == POLEE_ERR_BAD_ARG);
    std::vector<int64_t> bad = first;
    bad[1] = last[0];
    polee_xb_transcripts overlap{n, seq.data(), strand.data(), ptr.data(), bad.data(), last.data()};
    REQUIRE(ptr[1] < 2 || polee_splice_run_host(&overlap, nullptr, &sf) == POLEE_ERR_BAD_ARG);
    std::vector<int64_t> far = last;
    far.back() = ((int64_t)1 << 31) - 1;
    polee_xb_transcripts beyond{n, seq.data(), strand.data(), ptr.data(), first.data(), far.data()};
    REQUIRE(polee_splice_run_host(&beyond, nullptr, &sf) == POLEE_ERR_BAD_ARG);
    gene[7] = 0;
    REQUIRE(polee_splice_run_host(&T, gene.data(), &sf) == POLEE_ERR_BAD_ARG);
    if (fails) return 1;
    printf("splicing features on the host threads: ok (%d transcripts, %lld exons, %lld overlapping pairs, %lld features)\n", n, (long long)with.exons,
           (long long)with.pairs, (long long)with.F);
    return 0;
}
