// Sanitizer driver for the rounds merge of `polee fit-tree` on the host threads (polee_amd/csrc/kmer_rounds.cpp): the tree of
// sketches of a few hundred related sequences and of tie-heavy synthetic sketches with duplicates, empty ones and one value
// shared by many (polee_kmer_tree_rounds_host: the atomic maxima and minima of the best pass from all threads, the staged
// appends to the second edge buffer, the sort and de-duplication of the touched pairs, the unions, the Huffman phase, the
// DFS); 400 tie-heavy sketches give some 80 000 edges, several chunks per pass.  Built host-only (--offload-host-only) with
// -fsanitize=address,undefined and with -fsanitize=thread by `make -C polee_amd/csrc sanitize-kmer-rounds` and run there on the
// CPU; it touches no GPU and is not loaded into Python.  Exit code 0 = every call did what it should, every tree is well-formed
// and a second call gives the same one (the sanitizer itself aborts on a finding).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
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

static bool well_formed(const std::vector<int32_t> &parents, const std::vector<int32_t> &js, int64_t n)
{
    if ((int64_t)parents.size() != 2 * n - 1 || parents[0] != 0) return false;
    std::vector<int> seen((size_t)n + 1, 0), kids((size_t)(2 * n), 0);
    for (size_t i = 0; i < js.size(); ++i) {
        if (js[i] < 0 || js[i] > n) return false;
        if (js[i] > 0 && seen[(size_t)js[i]]++) return false;
        if (i > 0 && (parents[i] < 1 || parents[i] > (int32_t)i)) return false;
        if (i > 0) ++kids[(size_t)parents[i]];
    }
    for (size_t i = 0; i < js.size(); ++i)
        if (kids[i + 1] != (js[i] == 0 ? 2 : 0)) return false;
    return true;
}

static int64_t tree_of(const std::vector<uint64_t> &sk, int64_t n)
{
    std::vector<int32_t> p((size_t)(2 * n - 1)), j((size_t)(2 * n - 1)), p2(p.size()), j2(p.size());
    int64_t st[4] = {-1, -1, -1, -1}, st2[4];
    REQUIRE(polee_kmer_tree_rounds_host(n, sk.data(), p.data(), j.data(), st) == POLEE_OK);
    REQUIRE(well_formed(p, j, n));
    REQUIRE(st[0] >= 0 && st[0] <= st[1] && st[1] + st[2] == n && st[3] >= 0);  // (a merge takes one active node away)
    REQUIRE(polee_kmer_tree_rounds_host(n, sk.data(), p2.data(), j2.data(), st2) == POLEE_OK);
    REQUIRE(p == p2 && j == j2 && st[0] == st2[0] && st[3] == st2[3]);
    REQUIRE(polee_kmer_tree_rounds_host(n, sk.data(), p2.data(), j2.data(), nullptr) == POLEE_OK);  // (stats may be null)
    REQUIRE(p == p2 && j == j2);
    return st[0];
}

int main()
{
    std::mt19937_64 rng(11);
    // sequences: families of mutated copies, short ones, N-bearing ones, an empty one
    std::vector<std::string> seqs;
    while (seqs.size() < 300) {
        std::string f((size_t)(40 + rng() % 3000), 'A');
        for (char &c : f) c = "ACGT"[rng() % 4];
        const size_t copies = 1 + rng() % 5;
        for (size_t k = 0; k < copies; ++k) {
            std::string s = f;
            for (char &c : s)
                if (rng() % 100 == 0) c = "ACGTNacgt"[rng() % 9];
            if (rng() % 20 == 0) s.resize(rng() % 40);
            seqs.push_back(s);
        }
    }
    seqs.push_back("");
    const int64_t n = (int64_t)seqs.size();
    std::vector<int64_t> offsets((size_t)n + 1, 0);
    std::string bases;
    for (int64_t t = 0; t < n; ++t) {
        bases += seqs[(size_t)t];
        offsets[(size_t)t + 1] = (int64_t)bases.size();
    }
    std::vector<uint64_t> sk((size_t)n * POLEE_KMER_H);
    REQUIRE(polee_kmer_sketch_host(n, offsets.data(), (const uint8_t *)bases.data(), sk.data()) == POLEE_OK);
    REQUIRE(tree_of(sk, n) >= 1);
    // tie-heavy sketches: bins draw from small pools; duplicates; empty sketches; one value held by 150 of them
    for (int64_t m : {1, 2, 3, 17, 400}) {
        std::vector<uint64_t> s((size_t)m * POLEE_KMER_H, 0);
        for (int64_t t = 0; t < m; ++t)
            for (int b = 0; b < POLEE_KMER_H; ++b)
                if (rng() % 10 < 6) s[(size_t)t * POLEE_KMER_H + (size_t)b] = (uint64_t)(rng() % 5) * POLEE_KMER_H * 1000003ull + (uint64_t)b + 1;
        for (int64_t t = 0; t < std::min<int64_t>(m, 150); ++t) s[(size_t)t * POLEE_KMER_H + 9] = 7ull * POLEE_KMER_H + 9 + 1;
        if (m > 3) {
            std::copy(s.begin(), s.begin() + POLEE_KMER_H, s.begin() + 2 * POLEE_KMER_H);
            std::fill(s.begin() + POLEE_KMER_H, s.begin() + 2 * POLEE_KMER_H, 0ull);
        }
        const int64_t rounds = tree_of(s, m);
        REQUIRE(m < 2 || rounds >= 1);
    }
    std::vector<uint64_t> none((size_t)5 * POLEE_KMER_H, 0);  // nothing shared: no round, the Huffman phase joins all
    REQUIRE(tree_of(none, 5) == 0);
    std::vector<uint64_t> bad((size_t)3 * POLEE_KMER_H, 0);
    bad[5] = 8;  // h' = 7 belongs in bin 7
    std::vector<int32_t> p(5), j(5);
    REQUIRE(polee_kmer_tree_rounds_host(3, bad.data(), p.data(), j.data(), nullptr) == POLEE_ERR_BAD_ARG);
    REQUIRE(polee_kmer_tree_rounds_host(0, bad.data(), p.data(), j.data(), nullptr) == POLEE_ERR_BAD_ARG);
    if (fails) return 1;
    printf("kmer_tree rounds on the host threads: ok (%lld sequences)\n", (long long)n);
    return 0;
}
