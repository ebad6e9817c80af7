// The temperature route of range_amd/csrc/host_plan.h (plan_temperatures: shift mode of the softmax
// statistics and the route of a forward) on the CPU, built with g++ under AddressSanitizer /
// UndefinedBehaviorSanitizer by tests/test_temperatures_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <utility>

#include "../../range_amd/csrc/host_plan.h"

using namespace range_host;

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // both temperatures up to the cap of the constant shift: everything as before
    for (const auto& t : {std::pair<float, float>{12.f, 40.f}, {43.f, 43.f}, {15.f, 0.f}, {0.5f, 0.5f}, {43.f, -1.f}}) {
        for (int64_t B : {1, 16, 32, 33, 10000}) {
            const TempRoute r = plan_temperatures(t.first, t.second, B, true);
            CHECK(r.valid && r.shift == SHIFT_CONSTANT && r.topk_scan_ok);
            CHECK(r.one_pass == (B <= 32));
            CHECK(!plan_temperatures(t.first, t.second, B, false).one_pass);     // RANGE_SMALL_FORWARD=0
        }
    }
    // either above it: the running maximum, for both heads; small batches take the two passes; no in-scan lists
    for (const auto& t : {std::pair<float, float>{43.5f, 40.f}, {12.f, 200.f}, {100.f, 0.f}, {1000.f, 1000.f},
                          {std::nextafter(43.f, 44.f), 40.f}}) {
        for (int64_t B : {1, 20, 32, 33, 70}) {
            const TempRoute r = plan_temperatures(t.first, t.second, B, true);
            CHECK(r.valid && r.shift == SHIFT_RUNNING_MAX);
            CHECK(!r.one_pass && !r.topk_scan_ok);
        }
    }
    // a disabled geographic head does not count, whatever its number
    CHECK(plan_temperatures(12.f, -500.f, 8, true).shift == SHIFT_CONSTANT);
    // out of range: refused
    for (float bad : {0.f, -1.f, nan, inf, -inf, 1000.5f, std::nextafter(1000.f, 2000.f)}) {
        CHECK(!plan_temperatures(bad, 40.f, 8, true).valid);
        CHECK(!temperature_ok(bad, MAX_TAU_SHARP));
    }
    for (float bad : {nan, inf, 1000.5f}) CHECK(!plan_temperatures(12.f, bad, 8, true).valid);
    CHECK(plan_temperatures(1000.f, 1000.f, 8, true).valid && temperature_ok(1000.f, MAX_TAU_SHARP));
    CHECK(temperature_ok(43.f, MAX_TAU_CONSTANT) && !temperature_ok(43.5f, MAX_TAU_CONSTANT));
    std::printf("temp_route ok\n");
    return 0;
}
