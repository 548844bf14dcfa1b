// Sanitizer driver for the host builder of `polee fit-tree` (polee_amd/csrc/kmer_tree.cpp): sketches of a few hundred random
// and related sequences (polee_kmer_sketch_host), the tree of those and of tie-heavy synthetic sketches with duplicates, empty
// ones and one value shared by many (polee_kmer_tree_host: the sorts on the host threads, the pair keys, the merge loop's
// in-place holder lists, the Huffman phase, the DFS), and the rejection of a malformed sketch.  Built host-only
// (--offload-host-only) with -fsanitize=address,undefined by `make -C polee_amd/csrc sanitize-kmer-tree` and run there on the
// CPU; it touches no GPU and is not loaded into Python.  Exit code 0 = every call did what it should and every tree is
// well-formed (the sanitizer itself aborts on a finding).
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

static void tree_of(const std::vector<uint64_t> &sk, int64_t n)
{
    std::vector<int32_t> p((size_t)(2 * n - 1)), j((size_t)(2 * n - 1)), p2(p.size()), j2(p.size());
    REQUIRE(polee_kmer_tree_host(n, sk.data(), p.data(), j.data()) == POLEE_OK);
    REQUIRE(well_formed(p, j, n));
    REQUIRE(polee_kmer_tree_host(n, sk.data(), p2.data(), j2.data()) == POLEE_OK);
    REQUIRE(p == p2 && j == j2);
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
    for (int64_t t = 0; t < n; ++t)
        for (int b = 0; b < POLEE_KMER_H; ++b) {
            const uint64_t v = sk[(size_t)t * POLEE_KMER_H + (size_t)b];
            REQUIRE(v == 0 || (v - 1) % POLEE_KMER_H == (uint64_t)b);
        }
    tree_of(sk, n);
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
        tree_of(s, m);
    }
    std::vector<uint64_t> bad((size_t)3 * POLEE_KMER_H, 0);
    bad[5] = 8;  // h' = 7 belongs in bin 7
    std::vector<int32_t> p(5), j(5);
    REQUIRE(polee_kmer_tree_host(3, bad.data(), p.data(), j.data()) == POLEE_ERR_BAD_ARG);
    REQUIRE(polee_kmer_tree_host(0, bad.data(), p.data(), j.data()) == POLEE_ERR_BAD_ARG);
    if (fails) return 1;
    printf("kmer_tree host builder: ok (%lld sequences)\n", (long long)n);
    return 0;
}
