// Sanitizer driver for the host trainer of the bias model (polee_amd/csrc/bias_train_host.cpp): a full training on planted examples
// (skewed bases and a base that depends on its successor, so that the search commits rounds), a training from
// fragments that touch both transcript ends (pads on either side), hold N bases, are 20 bases long and cover a whole 20-base
// transcript, with a drawn and with a given background, one scored round from forced states up to order 6 at the last position that
// allows it, and the rejection of malformed input.  Built host-only (--offload-host-only) with -fsanitize=address,undefined and with
// -fsanitize=thread by `make -C polee_amd/csrc sanitize-bias-train` and run there on the CPU; it touches no GPU and is not loaded into
// Python.  Exit code 0 = every call did what it should (the sanitizer itself aborts on a finding).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../polee_amd/csrc/bias_train_common.hpp"

using namespace polee;
using namespace polee::biastrain;

static int fails = 0;
#define REQUIRE(cond)                                                   \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__);  \
            ++fails;                                                    \
        }                                                               \
    } while (0)

static void check_model(const Model &m)
{
    REQUIRE(m.trained);
    REQUIRE(m.accuracy >= 0.0 && m.accuracy <= 1.0);
    for (int side = 0; side < 2; ++side) {
        REQUIRE(m.ps[side].size() == (size_t)BT_K * 4 * BT_CTX);
        for (int j = 0; j < BT_K; ++j) {
            const int o = m.orders[side][j];
            REQUIRE(o >= -1 && o <= BT_MAXORDER && (o < 0 || j + o < BT_K));
            for (uint32_t nt = 0; nt < 4; ++nt)
                for (uint32_t ctx = 0; ctx < (uint32_t)BT_CTX; ++ctx) {
                    const float v = m.ps[side][((size_t)j * 4 + nt) * BT_CTX + ctx];
                    REQUIRE(std::isfinite(v) && v > 0.0f);
                    if (o < 0 || ctx >= (1u << (2 * o))) REQUIRE(v == 1.0f);
                }
        }
        const SearchState &s = m.trace[side];
        REQUIRE(s.rounds >= 0 && s.rounds <= BT_MAX_ROUNDS);
        for (int r = 0; r < s.rounds; ++r) REQUIRE(s.trace[r + 1] < s.trace[r]);
    }
    for (int i = 0; i < BT_GC_EXPANDED; ++i) REQUIRE(std::isfinite(m.gc_bins[i]) && m.gc_bins[i] > 0.0f);
}

int main()
{
    std::mt19937_64 rng(7);
    // planted examples: 1501 + 1501
    {
        const int64_t n = 1501, N = 2 * n;
        std::vector<uint8_t> l((size_t)N * BT_K), r((size_t)N * BT_K);
        std::vector<double> gc((size_t)N);
        for (int64_t e = 0; e < N; ++e) {
            for (int k = 0; k < BT_K; ++k) {
                l[(size_t)e * BT_K + k] = (uint8_t)(rng() & 3);
                r[(size_t)e * BT_K + k] = (uint8_t)(rng() & 3);
            }
            if (e < n) {
                if (rng() % 10 < 6) l[(size_t)e * BT_K + 2] = 0;
                if (rng() % 10 < 5) l[(size_t)e * BT_K + 19] = 1;
                if (rng() % 10 < 8) l[(size_t)e * BT_K + 18] = (uint8_t)((l[(size_t)e * BT_K + 19] + 1) & 3);
                r[(size_t)e * BT_K + 4] = 4;  // an N
            }
            gc[(size_t)e] = (double)(rng() % 201) / 200.0 * (e < n ? 1.0 : 0.8);
        }
        HostTrainer ht;
        ht.from_examples(n, n, l.data(), r.data(), gc.data());
        ht.run();
        check_model(ht.model);
        REQUIRE(ht.model.orders[0][2] >= 0 && ht.model.orders[0][19] >= 0 && ht.model.trace[0].rounds >= 2);
        int32_t orders[BT_K];
        double losses[BT_K], loss0 = 0.0;
        for (int j = 0; j < BT_K; ++j) orders[j] = -1;
        orders[2] = 5;
        orders[13] = 5;
        orders[19] = 0;
        orders[7] = 2;
        ht.candidates(0, orders, losses, &loss0);
        REQUIRE(std::isfinite(loss0) && std::isfinite(losses[2]) && std::isfinite(losses[13]) && std::isinf(losses[19]));
        orders[2] = 6;
        orders[13] = 6;
        ht.candidates(1, orders, losses, &loss0);
        REQUIRE(std::isinf(losses[2]) && std::isinf(losses[13]) && std::isfinite(losses[0]));
        check_model(ht.model);  // (a scored round leaves the trained model alone)
    }
    // fragments
    {
        const int32_t nt = 12;
        std::vector<int64_t> ptr(nt + 1, 0);
        for (int32_t t = 0; t < nt; ++t) ptr[(size_t)t + 1] = ptr[(size_t)t] + (t == 0 ? 20 : 20 + (int64_t)(rng() % 300));
        std::vector<uint8_t> tseq((size_t)ptr[nt]);
        for (auto &c : tseq) c = (uint8_t)(rng() % 100 == 0 ? 4 : rng() & 3);
        std::vector<int32_t> ft, ffl;
        std::vector<int64_t> fpos;
        for (int i = 0; i < 400; ++i) {
            const int32_t t = (int32_t)(i % nt);
            const int64_t tlen = ptr[(size_t)t + 1] - ptr[(size_t)t];
            const int32_t fl = i % 7 == 0 ? 20 : (int32_t)(20 + rng() % (uint64_t)(tlen - 19));
            const int64_t pos = i % 5 == 0 ? 1 : (i % 5 == 1 ? tlen - fl + 1 : 1 + (int64_t)(rng() % (uint64_t)(tlen - fl + 1)));
            ft.push_back(t), ffl.push_back(fl), fpos.push_back(pos);
        }
        Inputs in{nt, ptr.data(), tseq.data(), 400, ft.data(), fpos.data(), ffl.data(), 400, nullptr, nullptr, nullptr};
        REQUIRE(check_inputs(nullptr, "main", in) == POLEE_OK);
        HostTrainer ht;
        ht.from_fragments(in, 99);
        for (size_t i = 0; i < 400; ++i) {
            const int64_t tlen = ptr[(size_t)ft[i] + 1] - ptr[(size_t)ft[i]];
            REQUIRE(ht.bg_pos[i] >= 1 && ht.bg_pos[i] + ffl[i] - 1 <= tlen);
            REQUIRE(ht.gc[i] >= 0.0 && ht.gc[i] <= 1.0 && (ht.seq[0][i] >> 40) == 0 && (ht.seq[1][i] >> 40) == 0);
        }
        ht.run();
        check_model(ht.model);
        // the same with the drawn background given back as a list: the same examples (a pad's counter is the example's index, not its source)
        std::vector<int64_t> bpos = ht.bg_pos;
        Inputs in2 = in;
        in2.bg_t = ft.data(), in2.bg_tpos = bpos.data(), in2.bg_fl = ffl.data();
        REQUIRE(check_inputs(nullptr, "main", in2) == POLEE_OK);
        HostTrainer h2;
        h2.from_fragments(in2, 99);
        REQUIRE(h2.seq[0] == ht.seq[0] && h2.seq[1] == ht.seq[1] && h2.gc == ht.gc);
        // rejected input
        Inputs bad = in;
        bad.n_fg = bad.n_bg = 10;
        REQUIRE(check_inputs(nullptr, "main", bad) == POLEE_ERR_BAD_ARG);
        ffl[3] = 19;
        REQUIRE(check_inputs(nullptr, "main", in) == POLEE_ERR_BAD_ARG);
        ffl[3] = 20;
        fpos[3] = 0;
        REQUIRE(check_inputs(nullptr, "main", in) == POLEE_ERR_BAD_ARG);
        fpos[3] = ptr[(size_t)ft[3] + 1] - ptr[(size_t)ft[3]] - 18;
        REQUIRE(check_inputs(nullptr, "main", in) == POLEE_ERR_BAD_ARG);
        REQUIRE(check_counts(nullptr, "main", (int64_t)1 << 23, (int64_t)1 << 23) == POLEE_ERR_UNSUPPORTED);
    }
    if (fails) {
        fprintf(stderr, "bias_train_check: %d failed\n", fails);
        return 1;
    }
    printf("bias_train_check ok\n");
    return 0;
}
