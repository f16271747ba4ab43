// body_motion_sanitize_driver.cpp -- test infrastructure (tests/test_temporal_bodies_host.py): host/body_motion.cpp driven through the C ABI from a plain program, so
// that it can be built with -fsanitize=address,undefined and run on its own.  Every array is a heap block of exactly the size the header asks for (an overrun is an
// ASan report), prim_id holds INT_MIN and INT_MAX and the ranges reach INT_MAX (an overflow in the range test is a UBSan report).  Prints "ok" and returns 0.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/dsrt.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, dsrt_last_error()); return 1; } } while (0)

static void identity(float* p) { std::memset(p, 0, 12 * sizeof(float)); p[0] = p[5] = p[10] = 1.0f; }

int main() {
    for (int bodies : {1, 2, DSRT_MAX_BODIES}) {
        std::vector<int> first(bodies), num(bodies);
        std::vector<float> prev(12 * (size_t)bodies), cur(12 * (size_t)bodies);
        for (int b = 0; b < bodies; ++b) {
            first[b] = b * 100; num[b] = 100;
            identity(&prev[12 * (size_t)b]); identity(&cur[12 * (size_t)b]);
            cur[12 * (size_t)b + 3] = (float)b;                     // body b shifts by b along x
            cur[12 * (size_t)b + 1] = -1.0f; cur[12 * (size_t)b + 4] = 1.0f; cur[12 * (size_t)b] = cur[12 * (size_t)b + 5] = 0.0f;      // ... and turns by 90 degrees about z
        }
        first[bodies - 1] = INT_MAX - 50; num[bodies - 1] = INT_MAX;                // first + num does not fit an int: the range test must not overflow
        const int n = 4096;
        std::vector<int32_t> prim(n);
        std::vector<float> N(3 * (size_t)n), X(3 * (size_t)n), N2(3 * (size_t)n), X2(3 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            prim[i] = i % 7 == 0 ? INT_MIN : i % 7 == 1 ? INT_MAX : i % 7 == 2 ? -1 - i : (i * 37) % (bodies * 100 + 50);
            for (int k = 0; k < 3; ++k) { N[3 * (size_t)i + k] = k == 2 ? 1.0f : 0.0f; X[3 * (size_t)i + k] = (float)(i + k) * 0.25f; }
        }
        const DsrtBodyMotion m{bodies, first.data(), num.data(), prev.data(), cur.data(), prim.data()};
        CHECK(dsrt_body_motion_host(&m, n, N.data(), X.data(), N2.data(), X2.data()) == DSRT_OK);
        CHECK(dsrt_body_motion_host(&m, n, N.data(), X.data(), nullptr, X2.data()) == DSRT_OK);
        CHECK(dsrt_body_motion_host(&m, 0, N.data(), X.data(), N2.data(), X2.data()) == DSRT_OK);
        int moved = 0;
        for (int i = 0; i < n; ++i) {
            const bool same = std::memcmp(&X2[3 * (size_t)i], &X[3 * (size_t)i], 12) == 0;
            const bool on_moved = bodies > 1 && ((prim[i] >= 100 && prim[i] < 100 * (bodies - 1)) || prim[i] >= INT_MAX - 50);
            CHECK(same == !on_moved);
            moved += on_moved;
        }
        CHECK(bodies == 1 || moved > 0);
        // refusals: nothing is read beyond what was checked
        DsrtBodyMotion bad = m;
        bad.bodies = DSRT_MAX_BODIES + 1;
        CHECK(dsrt_body_motion_host(&bad, n, N.data(), X.data(), N2.data(), X2.data()) == DSRT_ERR_INVALID);
        bad = m; bad.poses_cur = nullptr;
        CHECK(dsrt_body_motion_host(&bad, n, N.data(), X.data(), N2.data(), X2.data()) == DSRT_ERR_INVALID);
        CHECK(dsrt_body_motion_host(&m, n, N.data(), X.data(), X.data(), X2.data()) == DSRT_ERR_INVALID);
        if (bodies > 1) {
            cur[12 * (size_t)(bodies - 1) + 7] = NAN;
            CHECK(dsrt_body_motion_host(&m, n, N.data(), X.data(), N2.data(), X2.data()) == DSRT_ERR_INVALID);
        }
    }
    CHECK(dsrt_body_motion_host(nullptr, 0, nullptr, nullptr, nullptr, nullptr) == DSRT_ERR_INVALID);
    std::puts("ok");
    return 0;
}
