// Stand-alone check of ar-vae_amd/csrc/dispatch.h (host only; built and run by tests/test_dispatch_host.py).
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "dispatch.h"

using arvae::with_bool;
using arvae::with_int;

static int g_failed = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failed;                                              \
        }                                                            \
    } while (0)

int main() {
    // a listed value: f exactly once, with that value as a constant, and true
    for (int v : {4, 8, 16}) {
        int calls = 0, seen = -1;
        const bool known = with_int<4, 8, 16>(v, [&](auto c) {
            static_assert(std::is_same<decltype(c), std::integral_constant<int, decltype(c)::value>>::value, "an integral_constant<int, V>");
            constexpr int V = decltype(c)::value;      // usable as a template argument
            static_assert(V == 4 || V == 8 || V == 16, "only the listed values are instantiated");
            ++calls;
            seen = V;
        });
        CHECK(known);
        CHECK(calls == 1);
        CHECK(seen == v);
    }
    // a value that is not listed: no call, and false
    for (int v : {0, 5, 17}) {
        int calls = 0;
        const bool known = with_int<4, 8, 16>(v, [&](auto) { ++calls; });
        CHECK(!known);
        CHECK(calls == 0);
    }
    // each branch of with_bool gets its type
    for (bool b : {false, true}) {
        int calls = 0;
        bool seen = !b;
        with_bool(b, [&](auto c) {
            static_assert(std::is_same<decltype(c), std::true_type>::value || std::is_same<decltype(c), std::false_type>::value,
                          "true_type or false_type");
            ++calls;
            seen = decltype(c)::value;
        });
        CHECK(calls == 1);
        CHECK(seen == b);
    }
    // two dispatchers nested: every combination, each exactly once
    int hits[2][2] = {{0, 0}, {0, 0}};
    for (bool b : {false, true})
        for (int v : {1, 2}) {
            const bool known = with_int<1, 2>(v, [&](auto c) {
                with_bool(b, [&](auto d) {
                    constexpr int V = decltype(c)::value;
                    constexpr bool B = decltype(d)::value;
                    ++hits[B ? 1 : 0][V - 1];
                });
            });
            CHECK(known);
        }
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) CHECK(hits[i][j] == 1);
    if (g_failed == 0) std::printf("dispatch.h: ok\n");
    return g_failed == 0 ? 0 : 1;
}
