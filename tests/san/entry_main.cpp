// Sanitizer driver for the three openers of the C entry points (polee_amd/csrc/common.hpp: entry, ctx_entry, host_entry): each is
// called with bodies that throw std::bad_alloc, std::runtime_error and an int, with a body that returns, and with a null handle or
// context; nothing may unwind, the status is POLEE_ERR_OOM / POLEE_ERR_UNSUPPORTED / POLEE_ERR_BAD_ARG, and polee_last_error names
// the entry point.  Built host-only (--offload-host-only) with -fsanitize=address,undefined by `make -C polee_amd/csrc sanitize-entry`,
// linked with ctx.hip only, and run there on the CPU.  The two runtime calls an opener makes (select the device, clear the
// last error) are answered here, so the program touches no GPU; it is not loaded into Python.
// Exit code 0 = every call did what it should (the sanitizer itself aborts on a finding).
#include <cstdio>
#include <cstring>
#include <new>
#include <stdexcept>

#include "../../polee_amd/csrc/common.hpp"

static int devices_selected = 0;
extern "C" hipError_t hipSetDevice(int)
{
    ++devices_selected;
    return hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }

static int fails = 0;
#define REQUIRE(cond)                                                   \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__);  \
            ++fails;                                                    \
        }                                                               \
    } while (0)

struct Handle {
    polee_ctx *ctx;
};

static bool error_is(const polee_ctx *ctx, const char *text) { return strcmp(polee_last_error(ctx), text) == 0; }

// what an opener makes of each kind of body; open(body) runs `body` under the opener with the name "polee_x"
template <class Open>
static void check_bodies(polee_ctx *ctx, Open &&open)
{
    REQUIRE(open([]() -> polee_status { return POLEE_OK; }) == POLEE_OK);
    REQUIRE(open([]() -> polee_status { throw std::bad_alloc(); }) == POLEE_ERR_OOM);
    REQUIRE(error_is(ctx, "polee_x: out of host memory"));
    REQUIRE(open([]() -> polee_status { throw std::runtime_error("broken"); }) == POLEE_ERR_UNSUPPORTED);
    REQUIRE(error_is(ctx, "polee_x: broken"));
    REQUIRE(open([]() -> polee_status { throw 7; }) == POLEE_ERR_UNSUPPORTED);
    REQUIRE(error_is(ctx, "polee_x: unknown exception"));
    REQUIRE(open([&]() -> polee_status { return polee::fail(ctx, POLEE_ERR_NONFINITE, "polee_x: the body's own"); }) == POLEE_ERR_NONFINITE);
    REQUIRE(error_is(ctx, "polee_x: the body's own"));
}

int main()
{
    polee_ctx c;
    c.device = 3;
    Handle h{&c};

    check_bodies(&c, [&](auto body) {
        return polee::entry(&h, "polee_x", [&](polee_ctx *ctx) -> polee_status {
            REQUIRE(ctx == &c);
            return body();
        });
    });
    REQUIRE(devices_selected == 5);  // (once per call, before the body)
    REQUIRE(polee::entry((Handle *)nullptr, "polee_x", [](polee_ctx *) -> polee_status { return POLEE_OK; }) == POLEE_ERR_BAD_ARG);
    REQUIRE(error_is(nullptr, "polee_x: null handle"));
    REQUIRE(polee::entry((const Handle *)nullptr, "polee_x", [](polee_ctx *) -> polee_status { throw 1; }) == POLEE_ERR_BAD_ARG);

    // a handle without a context (a bias trainer on the host): the body runs, no device is selected
    Handle hostonly{nullptr};
    check_bodies(nullptr, [&](auto body) {
        return polee::entry(&hostonly, "polee_x", [&](polee_ctx *ctx) -> polee_status {
            REQUIRE(ctx == nullptr);
            return body();
        });
    });
    REQUIRE(devices_selected == 5);

    check_bodies(&c, [&](auto body) { return polee::ctx_entry(&c, "polee_x", body); });
    REQUIRE(devices_selected == 10);
    REQUIRE(polee::ctx_entry(nullptr, "polee_x", []() -> polee_status { return POLEE_OK; }) == POLEE_ERR_BAD_ARG);
    REQUIRE(error_is(nullptr, "polee_x: null context"));

    check_bodies(nullptr, [&](auto body) { return polee::host_entry("polee_x", body); });
    REQUIRE(devices_selected == 10);  // (host_entry selects none)

    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
