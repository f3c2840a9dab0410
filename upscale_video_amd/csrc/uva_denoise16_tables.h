// uva_denoise16_tables.h -- the host-built tables of `-m n=K` at --bit-depth 16 (uva_denoise16.hip.h).
// Plain C++, no HIP: tests/host/denoise16_tables_check.cpp builds them in a program of its own and tests/test_denoise16.py
// compares every integer with the numpy definition's (tests/nlm16_ref.py lab16_tables, weight_table16).
#pragma once
#include <stdint.h>

#include <climits>
#include <cmath>
#include <vector>

namespace uva {

constexpr int NLM16_SQ_SHIFT = 8;        // per squared sample difference, before summing
constexpr int NLM16_IDX_SHIFT = 9;       // patch distance -> table index: 2^9 * 2^8 / 257^2 = 1.98 eight-bit units^2 per bin
constexpr int NLM16_TABLE_LIMIT = 1 << 22;
constexpr int LAB16_AB_OFF = 128 * 257;

struct Lab16Tables {
    uint32_t ftab[65536];                // rint(2^16 f(t / 65535)), f = cbrt above 0.008856, 7.787 t + 16/116 below
    uint32_t fwd[9];                     // (X/Xn, Y, Z/Zn) from (R, G, B), << 15
    int64_t inv[9];                      // (R, G, B) from (x, y, z) with the white point folded in, << 14
    int64_t l_mul, l_sub, a_mul, b_mul;  // << 20: F -> L16, (F_x - F_y) -> a16, (F_y - F_z) -> b16
    int64_t il_mul, il_add, ia_mul, ib_mul;   // << 40: L16 -> f_y, (a16 - 32896) -> f_x - f_y, (b16 - 32896) -> f_y - f_z
    int64_t f_thr, f_bias;               // << 24: f at the CIE threshold, 16/116
    int64_t lin_mul;                     // << 20: 1 / 7.787
};

// float64, one operation per statement: tests/nlm16_ref.py lab16_tables builds the same integers
inline void lab16_tables_host(Lab16Tables& t)
{
    const double bias = 16.0 / 116.0;
    for (int i = 0; i < 65536; ++i) {
        const double x = (double)i / 65535.0;
        double lin = 7.787 * x;
        lin = lin + bias;
        const double f = x > 0.008856 ? std::cbrt(x) : lin;
        t.ftab[i] = (uint32_t)std::lrint(65536.0 * f);
    }
    static const double rgb2xyz[9] = {0.412453, 0.357580, 0.180423, 0.212671, 0.715160, 0.072169, 0.019334, 0.119193, 0.950227};
    static const double xyz2rgb[9] = {3.240479, -1.53715, -0.498535, -0.969256, 1.875991, 0.041556, 0.055648, -0.204043, 1.057311};
    static const double d65[3] = {0.950456, 1.0, 1.088754};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double v = 32768.0 * rgb2xyz[i * 3 + j];
            t.fwd[i * 3 + j] = (uint32_t)std::lrint(v / d65[i]);
            v = 16384.0 * xyz2rgb[i * 3 + j];
            t.inv[i * 3 + j] = (int64_t)std::llrint(v * d65[j]);
        }
    const double q20 = 1048576.0, q24 = 16777216.0, q40 = 1099511627776.0;
    const double lscale = 116.0 * 655.35;
    const double l1 = lscale / 65536.0, l2 = 16.0 * 655.35, a1 = 128500.0 / 65536.0, b1 = 51400.0 / 65536.0;
    t.l_mul = (int64_t)std::llrint(q20 * l1);
    t.l_sub = (int64_t)std::llrint(q20 * l2);
    t.a_mul = (int64_t)std::llrint(q20 * a1);
    t.b_mul = (int64_t)std::llrint(q20 * b1);
    t.il_mul = (int64_t)std::llrint(q40 / lscale);
    t.il_add = (int64_t)std::llrint(q40 * bias);
    t.ia_mul = (int64_t)std::llrint(q40 / 128500.0);
    t.ib_mul = (int64_t)std::llrint(q40 / 51400.0);
    double thr = 7.787 * 0.008856;
    thr = thr + bias;
    t.f_thr = (int64_t)std::llrint(q24 * thr);
    t.f_bias = (int64_t)std::llrint(q24 * bias);
    t.lin_mul = (int64_t)std::llrint(q20 / 7.787);
}

// round(F exp(-i m16 / (h^2 cn))), weights below F / 1000 dropped, cut at (and including) the first zero
inline bool nlm16_weight_table(float h, int cn, std::vector<int>& table)
{
    const int fixed_point_mult = INT_MAX / (81 * 255);           // OpenCV's, for the 9 x 9 search window: 103969
    const double mult = (512.0 * 256.0) / (257.0 * 257.0 * 25.0);
    const double den = (double)h * h * cn;
    table.clear();
    for (int i = 0; i < NLM16_TABLE_LIMIT; ++i) {
        const double dist = i * mult;
        double w = std::exp(-dist / den);
        if (std::isnan(w)) w = 1.0;
        int weight = (int)std::lrint(fixed_point_mult * w);
        if (weight < 0.001 * fixed_point_mult) weight = 0;
        table.push_back(weight);
        if (weight == 0) return true;
    }
    return false;
}

}  // namespace uva
