// tools/sync_math_check.cpp — sync_atan2_turn (rust-modem_amd/csrc/modem_sync_math.h) against
// double atan2 on the host: 2^24 seeded random pairs with magnitudes from 2^-120 to 2^120, the
// axes, the octant boundaries and their f32 neighbours at every magnitude, zeros and non-finite
// input. Prints the worst error in turns; the exit status is 0 when it is within 2^-22.
//   g++ -O2 -std=c++17 -ffp-contract=off -I rust-modem_amd/csrc tools/sync_math_check.cpp -o sync_math_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "modem_sync_math.h"

static uint64_t rng_state = 0x5EED5A1C;
static uint64_t next_word() { return mk::chan_mix(rng_state += mk::kGolden); }

static double worst = 0.0;
static float worst_y = 0.f, worst_x = 0.f;
static uint64_t checked = 0;

static void check(float y, float x) {
    if (y == 0.f && x == 0.f) return;                           // 0 by definition: with the special values below
    const double got = (double)mk::sync_atan2_turn(y, x) * 0x1p-32;
    double d = got - std::atan2((double)y, (double)x) / 6.283185307179586476925286766559;
    d -= std::floor(d + 0.5);                                   // the distance mod 1
    d = std::fabs(d);
    if (d > worst) { worst = d; worst_y = y; worst_x = x; }
    ++checked;
}

static float nudge(float v, int ulps) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    u += (uint32_t)ulps;
    std::memcpy(&v, &u, 4);
    return v;
}

int main() {
    // random direction, random common magnitude 2^-120 .. 2^120 (the components within 2^-6 of it
    // or, every fourth pair, one of them up to 2^-24 smaller: the small-quotient end)
    for (uint32_t i = 0; i < (1u << 24); ++i) {
        const uint64_t w = next_word();
        const double a = (double)(w >> 11) * 0x1p-53 * 6.283185307179586;
        const int e = (int)((w & 0x7ff) % 241) - 120;
        double c = std::cos(a), s = std::sin(a);
        if ((i & 3) == 3) ((w >> 11) & 1 ? c : s) *= std::ldexp(1.0, -(int)((w >> 12) % 25));
        check((float)std::ldexp(s, e), (float)std::ldexp(c, e));
    }
    // axes, diagonals (the octant boundaries) and their neighbours, every sign, every magnitude
    for (int e = -120; e <= 120; ++e) {
        const float v = std::ldexp(1.0f, e);
        for (int sy = -1; sy <= 1; ++sy)
            for (int sx = -1; sx <= 1; ++sx)
                for (int ny = -2; ny <= 2; ++ny)
                    for (int nx = -2; nx <= 2; ++nx) {
                        if (!sy && !sx) continue;
                        check(sy * nudge(v, ny), sx * nudge(v, nx));
                        check(sy * nudge(v, ny), sx * nudge(v, nx) * 0x1p-30f);      // next to an axis
                        check(sy * nudge(v, ny) * 0x1p-30f, sx * nudge(v, nx));
                    }
    }
    int bad = 0;
    const float inf = INFINITY, nan = NAN;
    const float special[][2] = {{0.f, 0.f}, {-0.f, 0.f}, {0.f, -0.f}, {-0.f, -0.f}, {inf, 1.f}, {1.f, inf}, {-inf, inf},
                                {nan, 1.f}, {1.f, nan}, {nan, nan}, {inf, nan}, {nan, 0.f}, {0.f, nan}};
    for (const auto& p : special)
        if (mk::sync_atan2_turn(p[0], p[1]) != 0) { std::printf("sync_atan2_turn(%g, %g) != 0\n", p[0], p[1]); ++bad; }
    if (mk::sync_atan2_turn(0.f, 1.f) != 0 || mk::sync_atan2_turn(1.f, 0.f) != 0x40000000u ||
        mk::sync_atan2_turn(0.f, -1.f) != 0x80000000u || mk::sync_atan2_turn(-1.f, 0.f) != 0xC0000000u) {
        std::printf("the axes are not exact\n");
        ++bad;
    }
    std::printf("sync_atan2_turn: %llu pairs, worst error %.4g turns = 2^%.2f at (y %a, x %a); bound 2^-22\n",
                (unsigned long long)checked, worst, std::log2(worst), worst_y, worst_x);
    return bad || !(worst <= 0x1p-22) ? 1 : 0;
}
